// f16x3 implicit GEMM for stride-1 (kT,3,3) convs, kT in {1,3}, "same" padding: halo-staged input tiles.
//
// conv_gemm_dma_kernel gathers its A tile from global memory once per TAP: the 27-tap readout conv reads every activation 27
// times from L2 and splits it to f16 hi/lo 27 times.  Here a workgroup owns an output BRICK of 4 x 8 x 8 (t, h, w) positions of
// one sample (256 GEMM rows, 8 waves of 32 rows x BN columns) and the loop is channel chunk OUTER, tap INNER:
//   * per 32-channel chunk the brick plus its 1-cell halo is loaded ONCE (through registers), split to f16 hi/lo ONCE and
//     written to an LDS image of 64-B cells (hi plane, lo plane); cells outside the frame hold zeros;
//   * the taps then walk that image: an A fragment is an LDS read at a per-tap cell offset -- no global traffic, no VALU;
//   * only the weight block of (tap, chunk) is LDS-DMA'd per step (the blocked hi/lo planes of the other LDS-DMA kernels; with
//     C % 32 == 0 every 32-k block is one (tap, chunk) pair), double buffered;
//   * the next chunk's cells are requested into registers under the last tap of the current chunk.
// The summation order (chunk-major) differs from the tap-major kernels; accumulation is fp32 as everywhere.
#include "conv_common.h"

namespace mspi {

__device__ __attribute__((aligned(16))) float g_halo_zero16[4] = {0.f, 0.f, 0.f, 0.f};

typedef __attribute__((address_space(3))) void halo_lds_void;

constexpr int HB_T = 4, HB_H = 8, HB_W = 8;      // the brick: 256 rows
constexpr int HH = HB_H + 2, HW = HB_W + 2;      // halo plane: 10 x 10 cells

struct HaloArgs {
  const float* x;
  const _Float16* wb;
  const float* bias;
  const float* res;
  float* y;
  int N, T, H, W, C, Cout;
  long sN, sT, sH, sW;
  long ldy, ldw, ldr, wplane;
  int nbt, nbh, nbw, tiles_n;
  int act;
  float out_scale;
  int* status;
};

template <int KT, int TN>
__global__ __launch_bounds__(512) void conv_halo_kernel(const HaloArgs p) {
  constexpr int BN = 32 * TN;
  constexpr int HT = HB_T + KT - 1;               // halo planes
  constexpr int NCELL = HT * HH * HW;
  constexpr int IMG_PLANE = NCELL * 64;           // bytes of one f16 plane of the image: 32 channels per cell
  constexpr int P_BYTES = BN * 64;                // one f16 weight plane of a stage: BN rows x 32 k
  constexpr int WSTAGE = 2 * P_BYTES;
  constexpr int NGRP = BN / 16;                   // 16-row weight groups per plane
  constexpr int HBI = (NGRP + 7) / 8;             // weight DMA instructions per wave per plane
  constexpr int NLD = (NCELL * 8 + 511) / 512;    // float4 loads per thread per chunk
  constexpr int NTAP = KT * 9;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * IMG_PLANE + 2 * WSTAGE];
  unsigned char* wsm = smem + 2 * IMG_PLANE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  int b = blockIdx.x;
  const int tile_n = b % p.tiles_n; b /= p.tiles_n;
  const int bw_i = b % p.nbw; b /= p.nbw;
  const int bh_i = b % p.nbh; b /= p.nbh;
  const int bt_i = b % p.nbt;
  const int n = b / p.nbt;
  const int t0 = bt_i * HB_T, h0 = bh_i * HB_H, w0 = bw_i * HB_W, n0 = tile_n * BN;
  const float* xn = p.x + (long)n * p.sN;

  // ---- image staging assignment: float4 e = tid + 512 i of the chunk's NCELL x 8 float4; cell = e / 8, q = e % 8
  int g_off[NLD];      // offset of the cell's channel 4q inside the sample, -1: outside the frame (or past the image)
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int e = tid + 512 * i;
    const int cell = e >> 3, q = e & 7;
    const int tt = cell / (HH * HW), rem = cell - tt * (HH * HW);
    const int hh = rem / HW, ww = rem - hh * HW;
    const int t = t0 - KT / 2 + tt, h = h0 - 1 + hh, w = w0 - 1 + ww;
    const bool ok = cell < NCELL && (unsigned)t < (unsigned)p.T && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
    g_off[i] = ok ? (int)((long)t * p.sT + (long)h * p.sH + (long)w * p.sW) + q * 4 : -1;
  }
  float4 pre[NLD];
  auto image_load = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const float* src = g_off[i] >= 0 ? xn + g_off[i] + chunk * 32 : g_halo_zero16;
      pre[i] = *reinterpret_cast<const float4*>(src);
    }
  };
  auto image_store = [&]() {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = tid + 512 * i;
      const int cell = e >> 3, q = e & 7;
      if (cell < NCELL) {
        const float a4[4] = {pre[i].x, pre[i].y, pre[i].z, pre[i].w};
        v4h h4, l4;
#pragma unroll
        for (int c = 0; c < 4; ++c) { _Float16 hh_, ll_; split_f16(a4[c], hh_, ll_); h4[c] = hh_; l4[c] = ll_; }
        // cell row of 64 B = four 16-B segments of 8 channels; segment s sits in slot s ^ ((cell >> 2) & 3)
        const int o = cell * 64 + ((((q >> 1) ^ (cell >> 2)) & 3) << 4) + (q & 1) * 8;
        *reinterpret_cast<v4h*>(smem + o) = h4;
        *reinterpret_cast<v4h*>(smem + IMG_PLANE + o) = l4;
      }
    }
  };

  // ---- weight DMA: plane groups of 16 rows x 64 B; lane -> row lane/4, slot lane%4 holds segment slot ^ ((row >> 2) & 3)
  const int b_seg = (lane & 3) ^ ((lane >> 4) & 3);
  const int kt32 = (int)(p.ldw >> 5);
  auto weights_issue = [&](int st, int kb) {
    unsigned char* base = wsm + st * WSTAGE;
#pragma unroll
    for (int i = 0; i < HBI; ++i) {
      const int g = i * 8 + wave;
      if (g < NGRP) {      // wave-uniform
        const bool ok = n0 + g * 16 < p.Cout;      // blocked planes: rows are padded to 16 with zeros
        const _Float16* q = p.wb + ((long)((n0 >> 4) + (ok ? g : 0)) * kt32 + kb) * 512 + (lane >> 2) * 32 + b_seg * 8;
        const void* s_hi = ok ? (const void*)q : (const void*)g_halo_zero16;
        const void* s_lo = ok ? (const void*)(q + p.wplane) : (const void*)g_halo_zero16;
        __builtin_amdgcn_global_load_lds(s_hi, (halo_lds_void*)(base + g * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(s_lo, (halo_lds_void*)(base + P_BYTES + g * 1024), 16, 0, 0);
      }
    }
  };

  v16f acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  // this lane's fragment row: brick position (bt, bh, bw) = (wave / 2, (wave % 2) * 4 + li / 8, li % 8); tap (0,0,0) reads
  // halo cell (bt, bh, bw), tap (dt, dh, dw) the cell dt * 100 + dh * 10 + dw further on
  const int cell0 = (wave >> 1) * (HH * HW) + ((wave & 1) * 4 + (li >> 3)) * HW + (li & 7);

  const int nchunk = p.C >> 5;
  const int nsteps = nchunk * NTAP;
  image_load(0);
  weights_issue(0, 0);
  image_store();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int it = 0;
  for (int chunk = 0; chunk < nchunk; ++chunk) {
    int dt = 0, dh = 0, dw = 0;
    for (int tap = 0; tap < NTAP; ++tap, ++it) {
      const int cur = it & 1;
      if (it + 1 < nsteps) {      // the next step's weight block: next tap of this chunk, or tap 0 of the next chunk
        const bool last = tap + 1 == NTAP;
        weights_issue(cur ^ 1, last ? chunk + 1 : (tap + 1) * nchunk + chunk);
        if (last) image_load(chunk + 1);      // lands under this step's MFMAs
      }
      const int cell = cell0 + dt * (HH * HW) + dh * HW + dw;
      const unsigned char* wbase = wsm + cur * WSTAGE;
      const _Float16* Bh = reinterpret_cast<const _Float16*>(wbase);
      const _Float16* Bl = reinterpret_cast<const _Float16*>(wbase + P_BYTES);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int oa = cell * 64 + ((((2 * lh + sub) ^ (cell >> 2)) & 3) << 4);
        const v8h ah = *reinterpret_cast<const v8h*>(smem + oa);
        const v8h al = *reinterpret_cast<const v8h*>(smem + IMG_PLANE + oa);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int r = j * 32 + li;
          const int o = r * 32 + (((2 * lh + sub) ^ ((r >> 2) & 3)) << 3);
          const v8h bh = *reinterpret_cast<const v8h*>(&Bh[o]);
          const v8h bl = *reinterpret_cast<const v8h*>(&Bl[o]);
          if (!kSingleProduct) {
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[j], 0, 0, 0);
          }
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[j], 0, 0, 0);
        }
      }
      if (++dw == 3) { dw = 0; if (++dh == 3) { dh = 0; ++dt; } }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my weight DMAs (and image loads) have landed ...
      __syncthreads();                                      // ... everybody's have; weight stage `cur` and, after the last tap, the image are free
    }
    if (chunk + 1 < nchunk) {
      image_store();
      __syncthreads();
    }
  }

  // ---- epilogue: C/D layout col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) of the wave's 32 rows
  const int t = t0 + (wave >> 1);
  bool bad = false;
  auto epilogue = [&](auto act_c) {
    constexpr int ACT = decltype(act_c)::value;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + j * 32 + li;
      if (col >= p.Cout || t >= p.T) continue;
      const float bv = p.bias ? p.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int h = h0 + (wave & 1) * 4 + (r >> 2), w = w0 + 4 * lh + (r & 3);
        if (h < p.H && w < p.W) {
          const long row = (((long)n * p.T + t) * p.H + h) * p.W + w;
          const float pre_v = acc[j][r] * p.out_scale + bv + (p.res ? p.res[row * p.ldr + col] : 0.f);
          bad |= nonfinite(pre_v);
          p.y[row * p.ldy + col] = act_apply(pre_v, ACT);
        }
      }
    }
  };
  MSPI_DISPATCH_ACT(p.act, epilogue)
  report_nonfinite(p.status, bad);
}

template <int KT, int TN>
static void launch_halo(const HaloArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((conv_halo_kernel<KT, TN>), dim3(grid), dim3(512), 0, s, a);
}

}  // namespace mspi

using namespace mspi;

// kT * 1000 + BN, -1 with mspi_last_error() set for what the launch refuses
static int halo_select(const MspiConvDesc* d, const void* x) {
  MSPI_REQUIRE(d && x, "mspi_conv_halo_fwd: null argument");
  MSPI_REQUIRE(d->N > 0 && d->T > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->Cout > 0, "mspi_conv_halo_fwd: empty extent");
  MSPI_REQUIRE((d->kT == 1 || d->kT == 3) && d->kH == 3 && d->kW == 3, "mspi_conv_halo_fwd: kernel (%d,%d,%d) is not (1|3,3,3)", d->kT,
               d->kH, d->kW);
  MSPI_REQUIRE(d->strT == 1 && d->strH == 1 && d->strW == 1, "mspi_conv_halo_fwd: stride (%d,%d,%d) is not 1", d->strT, d->strH, d->strW);
  MSPI_REQUIRE(d->padT == d->kT / 2 && d->padH == 1 && d->padW == 1, "mspi_conv_halo_fwd: pad (%d,%d,%d) is not (kT/2,1,1)", d->padT,
               d->padH, d->padW);
  MSPI_REQUIRE(d->To == d->T && d->Ho == d->H && d->Wo == d->W, "mspi_conv_halo_fwd: output extent (%d,%d,%d) does not match the input's",
               d->To, d->Ho, d->Wo);
  MSPI_REQUIRE(d->prec == PREC_F16X3 && d->w_scale > 0.f, "mspi_conv_halo_fwd: f16x3 only (prec %d)", d->prec);
  MSPI_REQUIRE(d->C % 32 == 0, "mspi_conv_halo_fwd: C = %d is not a multiple of 32", d->C);
  MSPI_REQUIRE(d->sC == 1, "mspi_conv_halo_fwd: channels-last input only (sC = %ld)", (long)d->sC);
  MSPI_REQUIRE(aligned16(x) && (d->sN & 3) == 0 && (d->sT & 3) == 0 && (d->sH & 3) == 0 && (d->sW & 3) == 0,
               "mspi_conv_halo_fwd: input pointer and strides must be 16-B aligned");
  MSPI_REQUIRE(d->sW >= d->C && d->sH > 0 && d->sT > 0 && d->sN > 0, "mspi_conv_halo_fwd: bad strides");
  // offsets inside one sample are kept in 32 bits
  MSPI_REQUIRE((long)(d->T - 1) * d->sT + (long)(d->H - 1) * d->sH + (long)(d->W - 1) * d->sW + d->C < (1L << 31),
               "mspi_conv_halo_fwd: sample too large for 32-bit offsets");
  MSPI_REQUIRE(d->ldw == (long)d->kT * 9 * d->C, "mspi_conv_halo_fwd: ldw %ld != K", (long)d->ldw);
  MSPI_REQUIRE(d->w_blocked && aligned16(d->w_blocked), "mspi_conv_halo_fwd: needs the blocked weight planes (w_blocked)");
  MSPI_REQUIRE(d->ldy >= d->Cout, "mspi_conv_halo_fwd: ldy < Cout");
  const int bn = d->Cout <= 64 ? 64 : d->Cout <= 128 ? 128 : 192;
  const long grid = (long)d->N * ((d->T + HB_T - 1) / HB_T) * ((d->H + HB_H - 1) / HB_H) * ((d->W + HB_W - 1) / HB_W) * ((d->Cout + bn - 1) / bn);
  MSPI_REQUIRE(grid < (1L << 31) && (long)d->N * d->T * d->H * d->W < (1L << 31), "mspi_conv_halo_fwd: problem too large");
  return d->kT * 1000 + bn;
}

extern "C" int mspi_conv_halo_supported(const MspiConvDesc* d) {
  static const float probe[4] __attribute__((aligned(16))) = {0.f, 0.f, 0.f, 0.f};
  return d && halo_select(d, probe) > 0 ? 1 : 0;
}

extern "C" int mspi_conv_halo_variant(const MspiConvDesc* d, const void* x) { return halo_select(d, x); }

extern "C" int mspi_conv_halo_fwd(const MspiConvDesc* d, const float* x, const float* bias, const float* res, const float* gate,
                                  float* y, mspi_stream_t stream) {
  MSPI_REQUIRE(d && x && y, "mspi_conv_halo_fwd: null argument");
  MSPI_REQUIRE(!gate, "mspi_conv_halo_fwd: no gate");
  const int variant = halo_select(d, x);
  if (variant < 0) return variant;
  MSPI_REQUIRE(!res || d->ldr >= d->Cout, "mspi_conv_halo_fwd: ldr < Cout");
  const int bn = variant % 1000;
  HaloArgs a;
  a.x = x; a.wb = (const _Float16*)d->w_blocked; a.bias = bias; a.res = res; a.y = y;
  a.N = d->N; a.T = d->T; a.H = d->H; a.W = d->W; a.C = d->C; a.Cout = d->Cout;
  a.sN = d->sN; a.sT = d->sT; a.sH = d->sH; a.sW = d->sW;
  a.ldy = d->ldy; a.ldw = d->ldw; a.ldr = d->ldr;
  a.wplane = (long)((d->Cout + 15) / 16 * 16) * d->ldw;
  a.nbt = (d->T + HB_T - 1) / HB_T; a.nbh = (d->H + HB_H - 1) / HB_H; a.nbw = (d->W + HB_W - 1) / HB_W;
  a.tiles_n = (d->Cout + bn - 1) / bn;
  a.act = d->act;
  a.out_scale = 1.0f / d->w_scale;
  a.status = g_status_word;
  const unsigned grid = (unsigned)((long)d->N * a.nbt * a.nbh * a.nbw * a.tiles_n);
  hipStream_t s = (hipStream_t)stream;
  switch (variant) {
    case 1064: launch_halo<1, 2>(a, grid, s); break;
    case 1128: launch_halo<1, 4>(a, grid, s); break;
    case 1192: launch_halo<1, 6>(a, grid, s); break;
    case 3064: launch_halo<3, 2>(a, grid, s); break;
    case 3128: launch_halo<3, 4>(a, grid, s); break;
    case 3192: launch_halo<3, 6>(a, grid, s); break;
    default: MSPI_REQUIRE(false, "mspi_conv_halo_fwd: variant %d is not instantiated", variant);
  }
  return check_launch("mspi_conv_halo_fwd");
}
