// The head end of the X3D path: (1) below, the stride-2 a + b pair; (2) further down, the stem (x3d_stem_kernel).
//
// (1) X3D block, first half, for the FIRST block of a stage (spatial stride 2 in `b`), in ONE launch:
//   u = [swish]( b_bn( dw3x3x3 stride (1,2,2) pad 1 ( relu( a_bn( a(x) ) ) ) ) )  (+ squeeze-excite partial sums)
//
// Unfused, the 2.25x-wide `a` output is written at the INPUT resolution and read back by the strided depthwise kernel: four
// times the bytes of the result (360 MB each way for X3D-L stage 2 at batch 8).  Here it never leaves the CU.  Same scheme as
// x3d_ab_kernel (x3d_block.hip), with these differences:
//
//   workgroup = (sample, 7 x 7 OUTPUT tile = 15 x 15 input cells, 32-channel chunk of dim_inner, segment of TSEG frames),
//               512 threads: the ring is ~92 KB, one workgroup per CU, so the second wave per SIMD comes from the workgroup itself
//   ring slot = two planes, the even and the odd input columns of the tile, 15 rows x 8 cells x 32 floats each (the eighth
//               cell of the odd plane is padding): tap kw of output column wo reads cell wo (kw = 0, even plane), wo (kw = 1,
//               odd plane) or wo + 1 (kw = 2, even plane), so the threads of consecutive outputs read consecutive cells.
//               No pad floats: the channel quad q of cell c sits at quad q ^ (c & 3).  With that the 16-lane groups of the
//               depthwise phase's ds_read_b128 cover the 64 banks once, and the GEMM phase's 16-B stores are 2-way (free: the
//               store is bound by its register transfer).
//   pipeline  = the x rows of frame i + 1 are requested before the depthwise step of frame i and consumed after it: the L2 /
//               HBM latency of the only global read hides behind the depthwise phase.
// The halo costs 15 * 15 / (4 * 49) = 1.15x of `a` recomputation (stride 1: 1.47x), and `a` has K = 24.
// Bitwise reproducible: no atomics; SE partial sums are one row per workgroup, reduced in a fixed order by mspi_se_gate.
#include "conv_common.h"
#include <stdlib.h>
#include <string.h>

namespace mspi {

typedef float v4f_s2 __attribute__((ext_vector_type(4)));
typedef _Float16 v8h_s2 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_s2;

struct X3dAbS2Args {
  const float* x; const unsigned char* wa; const float* ba; const float* wb; const float* bb; float* u; float* pool;
  int N, T, H, W, Ho, Wo, Cin, Cmid;
  long ldx, ldu;
  int nch, tiles_w, tiles, nseg, tseg;
  int act;
  float inv_s;
  int* status;
  int dbg;      // MSPI_X3D_DBG (tools/x3d_ab_bench.py): 1 skip the GEMM phase, 2 skip the depthwise phase, 4 no x loads; 0 in production
};

constexpr int S2_TO = 7;                        // output tile edge
constexpr int S2_CH = 2 * S2_TO + 1;            // input rows (and columns) under it: 15
constexpr int S2_PW = 8;                        // cells per plane row: even columns 0, 2, .., 14; odd columns 1, .., 13 + one pad
constexpr int S2_PLANE = S2_CH * S2_PW;         // 120 cells
constexpr int S2_NCELL = 2 * S2_PLANE;          // 240 = 15 B tiles of 16 cells
constexpr int S2_SLOT = S2_NCELL * 32;          // floats per ring slot
constexpr int S2_THREADS = 512;

template <int KS>
__global__ __launch_bounds__(S2_THREADS, 1) void x3d_ab_s2_kernel(const X3dAbS2Args p) {
  constexpr int NBT = S2_NCELL / 16;                        // 15
  constexpr int NW = S2_THREADS / 64;                       // 8 waves
  constexpr int MAXT = (NBT + NW - 1) / NW;                 // B tiles per wave: 2
  constexpr int WA_BYTES = KS * 4096;                       // [ks][A tile 0/1][hi, lo][lane][8 halves]
  constexpr int NOUT = S2_TO * S2_TO;
  __shared__ __attribute__((aligned(16))) unsigned char s2_smem[WA_BYTES + 3 * S2_SLOT * 4 + 128];   // static: exceeds 64 KB
  float* ring = reinterpret_cast<float*>(s2_smem + WA_BYTES);
  float* bias_a = ring + 3 * S2_SLOT;                       // 32 floats

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // consecutive logical ids share an XCD: the nch workgroups that read one x tile, one per channel chunk, hit the same L2
  const int lb = xcd_logical_block((int)blockIdx.x, (int)gridDim.x);
  const int chunk = lb % p.nch;
  const int rest = lb / p.nch;
  const int tile = rest % p.tiles;
  const int seg = rest / p.tiles;
  const int n = blockIdx.y;
  const int h0 = (tile / p.tiles_w) * S2_TO, w0 = (tile % p.tiles_w) * S2_TO;     // output coordinates
  const int t0 = seg * p.tseg;
  const int tend = min(p.T, t0 + p.tseg);

  // ---- once per workgroup: this chunk's `a` weights (fragment order) into LDS, biases, this thread's depthwise weights
  for (int i = wave; i < WA_BYTES / 1024; i += NW)
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const float*>(p.wa + (long)chunk * WA_BYTES + (long)i * 1024 + lane * 16),
                                     (lds_void_s2*)(s2_smem + i * 1024), 16, 0, 0);
  if (tid < 32) bias_a[tid] = (chunk * 32 + tid < p.Cmid) ? p.ba[chunk * 32 + tid] : 0.f;
  const int q = tid & 7;                                    // channel quad of the depthwise phase
  const int cq = chunk * 32 + q * 4;
  const bool cok = cq < p.Cmid;
  float4 wreg[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) wreg[k] = cok ? *reinterpret_cast<const float4*>(p.wb + (long)k * p.Cmid + cq) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 bq = cok ? *reinterpret_cast<const float4*>(p.bb + cq) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 psum = make_float4(0.f, 0.f, 0.f, 0.f);
  bool bad = false;

  // ---- the cells of this lane's B tiles: ring position c = (plane * 15 + row) * 8 + j  <->  input (2 h0 - 1 + row, 2 w0 - 1 + 2 j + plane)
  const int li = lane & 15, kg = lane >> 4;
  int xoff[MAXT];                                           // floats from the frame's origin to this lane's 8 x values; -1 = zero padding
#pragma unroll
  for (int j = 0; j < MAXT; ++j) {
    const int c = (wave + NW * j) * 16 + li;
    const int plane = c / S2_PLANE, r = c - plane * S2_PLANE;
    const int cw = 2 * (r & 7) + plane;
    const int h = 2 * h0 - 1 + (r >> 3), w = 2 * w0 - 1 + cw;
    const bool in = c < S2_NCELL && cw < S2_CH && h >= 0 && h < p.H && w >= 0 && w < p.W;
    xoff[j] = in ? (int)(((long)h * p.W + w) * p.ldx) + 8 * kg : -1;
  }
  float4 raw[MAXT][KS][2];
  auto request = [&](int ta) {                              // all x loads of frame ta go out together; consumed a phase later
    const float* xf = p.x + (((long)n * p.T + ta) * p.H) * (long)p.W * p.ldx;
#pragma unroll
    for (int j = 0; j < MAXT; ++j)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bool kok = xoff[j] >= 0 && (32 * s + 8 * kg) < p.Cin && !(p.dbg & 4);
        const float* xr = kok ? xf + xoff[j] + 32 * s : xf;
        raw[j][s][0] = *reinterpret_cast<const float4*>(xr);
        raw[j][s][1] = *reinterpret_cast<const float4*>(xr + 4);
      }
  };
  const int nstep = (tend - t0) + 2;
  if (t0 - 1 >= 0 && !(p.dbg & 1)) request(t0 - 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // depthwise phase: thread = (output of the tile, channel quad)
  const int item = tid >> 3;
  const int oh = item / S2_TO, ow = item - oh * S2_TO;
#pragma unroll 1
  for (int i = 0; i < nstep; ++i) {
    const int ta = t0 - 1 + i;
    float* slot = ring + (i % 3) * S2_SLOT;
    if (p.dbg & 1) {
    } else if (ta < 0 || ta >= p.T) {                       // temporal zero padding of the depthwise conv
      for (int e = tid * 4; e < S2_SLOT; e += S2_THREADS * 4) *reinterpret_cast<float4*>(slot + e) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
      for (int j = 0; j < MAXT; ++j) {
        const int bt = wave + NW * j;
        if (bt >= NBT) break;
        const int c = bt * 16 + li;
        const bool inside = xoff[j] >= 0;
        v8h_s2 xh[KS], xl[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const bool kok = inside && (32 * s + 8 * kg) < p.Cin;
          const float4 a = raw[j][s][0], b = raw[j][s][1];
          const float v8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            _Float16 hh, ll;
            split_f16(kok ? v8[e] : 0.f, hh, ll);
            xh[s][e] = hh; xl[s][e] = ll;
          }
        }
#pragma unroll
        for (int at = 0; at < 2; ++at) {
          v4f_s2 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const unsigned char* wp = s2_smem + ((s * 2 + at) * 2) * 1024 + lane * 16;
            const v8h_s2 wh = *reinterpret_cast<const v8h_s2*>(wp);
            const v8h_s2 wl = *reinterpret_cast<const v8h_s2*>(wp + 1024);
            if (!kSingleProduct) {
              acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh[s], acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl[s], acc, 0, 0, 0);
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh[s], acc, 0, 0, 0);
          }
          // lane (li, kg): cell li of this B tile, channels at*16 + 4*kg + 0..3;  a_bn bias, ReLU, zero outside the frame
          const float4 bv = *reinterpret_cast<const float4*>(bias_a + at * 16 + 4 * kg);
          bad |= inside && (nonfinite(acc[0]) | nonfinite(acc[1]) | nonfinite(acc[2]) | nonfinite(acc[3]));
          float4 o;
          o.x = inside ? fmaxf(fmaf(acc[0], p.inv_s, bv.x), 0.f) : 0.f;
          o.y = inside ? fmaxf(fmaf(acc[1], p.inv_s, bv.y), 0.f) : 0.f;
          o.z = inside ? fmaxf(fmaf(acc[2], p.inv_s, bv.z), 0.f) : 0.f;
          o.w = inside ? fmaxf(fmaf(acc[3], p.inv_s, bv.w), 0.f) : 0.f;
          *reinterpret_cast<float4*>(slot + c * 32 + (((at * 4 + kg) ^ (c & 3)) << 2)) = o;
        }
      }
    }
    __syncthreads();
    // the next frame's x rows: in flight during the depthwise step (raw is dead until the next GEMM phase)
    if (i + 1 < nstep && ta + 1 >= 0 && ta + 1 < p.T && !(p.dbg & 1)) request(ta + 1);
    if (i >= 2 && !(p.dbg & 2) && item < NOUT) {
      const int to = t0 + i - 2;                            // output frame; its inputs: frames to-1, to, to+1 = steps i-2, i-1, i
      float4 acc = bq;
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        asm volatile("" ::: "memory");                      // keep the LDS reads of one tap plane (9 x 16 B) in flight, not all 27
        const float* sl = ring + ((i - 2 + dt) % 3) * S2_SLOT;
        float4 win[9];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const int c = ((kw & 1) * S2_CH + 2 * oh + kh) * S2_PW + ow + (kw >> 1);
            win[kh * 3 + kw] = *reinterpret_cast<const float4*>(sl + c * 32 + ((q ^ (c & 3)) << 2));
          }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const float4 wv = wreg[dt * 9 + k];
          acc.x = fmaf(win[k].x, wv.x, acc.x);
          acc.y = fmaf(win[k].y, wv.y, acc.y);
          acc.z = fmaf(win[k].z, wv.z, acc.z);
          acc.w = fmaf(win[k].w, wv.w, acc.w);
        }
      }
      psum.x += acc.x; psum.y += acc.y; psum.z += acc.z; psum.w += acc.w;
      if (p.act == MSPI_ACT_SWISH) {
        acc.x = fast_swish(acc.x); acc.y = fast_swish(acc.y); acc.z = fast_swish(acc.z); acc.w = fast_swish(acc.w);
      }
      if (cok)
        *reinterpret_cast<float4*>(p.u + ((((long)n * p.T + to) * p.Ho + (h0 + oh)) * (long)p.Wo + (w0 + ow)) * p.ldu + cq) = acc;
    }
    __syncthreads();
  }
  report_nonfinite(p.status, bad);
  if (p.pool) {     // squeeze-excite partial sums of the pre-activation output: one row per workgroup, fixed order
    float* red = ring;                                      // all ring reads are behind the loop's last barrier
    *reinterpret_cast<float4*>(red + tid * 4) = psum;
    __syncthreads();
    if (tid < 32) {
      const int qq = tid >> 2, comp = tid & 3;
      float s = 0.f;
      for (int r = 0; r < NOUT; ++r) s += red[(r * 8 + qq) * 4 + comp];
      const int c = chunk * 32 + tid;
      if (c < p.Cmid) p.pool[((long)n * (p.tiles * p.nseg) + (seg * p.tiles + tile)) * p.Cmid + c] = s;
    }
  }
}

template <int KS>
static void launch_ab_s2(const X3dAbS2Args& a, hipStream_t s) {
  const dim3 grid((unsigned)(a.nch * a.tiles * a.nseg), (unsigned)a.N);
  hipLaunchKernelGGL((x3d_ab_s2_kernel<KS>), grid, dim3(S2_THREADS), 0, s, a);
}

// frames per T segment: as long as possible (less `a` recomputation) while the grid still covers the chip about twice
static int x3d_s2_tseg(int N, int T, int tiles, int nch) {
  int best = T;
  for (int ts = T; ts >= 2; ts = (ts + 1) / 2) {
    best = ts;
    if ((long)N * tiles * nch * ((T + ts - 1) / ts) >= 448) break;
    if (ts == 2) break;
  }
  return best;
}

static void x3d_s2_geometry(const MspiX3dAbS2Desc* d, X3dAbS2Args& a) {
  a.Ho = d->H / 2; a.Wo = d->W / 2;
  a.nch = (d->Cmid + 31) / 32;
  a.tiles_w = a.Wo / S2_TO;
  a.tiles = (a.Ho / S2_TO) * a.tiles_w;
  a.tseg = x3d_s2_tseg(d->N, d->T, a.tiles, a.nch);
  a.nseg = (d->T + a.tseg - 1) / a.tseg;
}


// ---------------------------------------------------------------------------------------------------------------------------
// X3D stem in ONE launch:  y = relu( bn( temporal depthwise (5,1,1) pad 2 ( conv_xy (1,3,3) stride (1,2,2) pad (0,1,1), 3 -> 24 ) ) )
// Unfused, the 24-channel conv_xy output is written and read back (2 x 154 MB at batch 8).  Here a thread owns one output
// pixel and marches along T: conv_xy of the incoming frame (27 inputs x 24 channels, plain fp32 FMAs; the 792 weights travel
// as kernel arguments, so every FMA takes its weight from an SGPR) goes into a REGISTER ring of five frames, the 5-tap temporal conv + folded BN
// + ReLU of the frame two behind is computed from the ring and stored once.  No spatial halo; the only recomputation is two
// frames of conv_xy at each end of a T segment.  The input is the raw [N,3,T,H,W] clip with arbitrary (non-negative) strides;
// the next frame's 27 inputs are requested before the current frame's FMAs.
constexpr int STEM_C = 24;

struct X3dStemArgs {
  const float* x; float* y;
  // BY VALUE: kernel arguments are read through the scalar cache into SGPRs (3.4 KB of the 4 KB a launch may carry).
  // Channel-major, the order the FMAs consume them: wxy[c] = 27 taps (ci,kh,kw) + 1 pad; wt[c] = 5 taps, the bias, 2 pad
  float wxy[STEM_C][28], wt[STEM_C][8];
  int N, T, H, W, Ho, Wo;
  long sN, sC, sT, sH, sW, ldy;
  int tseg, nseg;
};

__global__ __launch_bounds__(256) void x3d_stem_kernel(const X3dStemArgs p) {
  const int npix = p.Ho * p.Wo;
  const int pix0 = blockIdx.x * 256 + threadIdx.x;
  const bool live = pix0 < npix;
  const int pix = live ? pix0 : 0;
  const int ho = pix / p.Wo, wo = pix - ho * p.Wo;
  const int n = blockIdx.z;
  const int t0 = blockIdx.y * p.tseg;
  const int tend = min(p.T, t0 + p.tseg);
  // the nine taps of this pixel: offset inside a (sample, channel, frame) plane, 0 and masked where the tap is padding
  int off[9];
  unsigned ok = 0;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int h = 2 * ho - 1 + kh, w = 2 * wo - 1 + kw;
      const bool in = h >= 0 && h < p.H && w >= 0 && w < p.W;
      off[kh * 3 + kw] = in ? (int)(h * p.sH + w * p.sW) : 0;
      ok |= (in ? 1u : 0u) << (kh * 3 + kw);
    }
  const float* xn = p.x + (long)n * p.sN;
  float nxt[27];
  auto request = [&](int f) {
    const float* xf = xn + (long)f * p.sT;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
      for (int k = 0; k < 9; ++k) nxt[ci * 9 + k] = xf[ci * p.sC + off[k]];
  };
  float ring[5][STEM_C];
#pragma unroll
  for (int j = 0; j < 5; ++j)
#pragma unroll
    for (int c = 0; c < STEM_C; ++c) ring[j][c] = 0.f;
  const int nstep = (tend - t0) + 4;
  if (t0 - 2 >= 0) request(t0 - 2);
#pragma unroll 1
  for (int i = 0; i < nstep; ++i) {
    const int f = t0 - 2 + i;                               // conv_xy frame of this step; output frame f - 2
    // an opaque zero in the weight index: the weight loads stay in the loop (hoisted, the 792 of them would spill the SGPR file)
    int z = 0;
    asm volatile("" : "+s"(z));
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < STEM_C; ++c) ring[j][c] = ring[j + 1][c];
    if (f >= 0 && f < p.T) {
      float cur[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) cur[k] = ((ok >> (k % 9)) & 1u) ? nxt[k] : 0.f;
      if (i + 1 < nstep && f + 1 < p.T) request(f + 1);
#pragma unroll
      for (int c = 0; c < STEM_C; ++c) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 27; ++k) a = fmaf(cur[k], p.wxy[c][z + k], a);
        ring[4][c] = a;
      }
    } else {
      if (i + 1 < nstep && f + 1 >= 0 && f + 1 < p.T) request(f + 1);
#pragma unroll
      for (int c = 0; c < STEM_C; ++c) ring[4][c] = 0.f;     // temporal zero padding
    }
    if (i >= 4) {
      const int to = f - 2;
      float* yp = p.y + ((((long)n * p.T + to) * p.Ho + ho) * (long)p.Wo + wo) * p.ldy;
#pragma unroll
      for (int c4 = 0; c4 < STEM_C; c4 += 4) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = c4 + e;
          float a = p.wt[c][z + 5];
#pragma unroll
          for (int k = 0; k < 5; ++k) a = fmaf(ring[k][c], p.wt[c][z + k], a);
          o[e] = relu_nan(a);      // nothing runs before this kernel: a NaN pixel has to leave it as a NaN (common.h)
        }
        if (live) *reinterpret_cast<float4*>(yp + c4) = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
  }
}

// frames per T segment: the whole clip when the pixels alone fill the chip (one wave per SIMD), else halved while >= 4
static int x3d_stem_tseg(const MspiX3dStemDesc* d) {
  const int ho = (d->H - 1) / 2 + 1, wo = (d->W - 1) / 2 + 1;
  const long waves = (long)d->N * ((ho * wo + 255) / 256) * 4;
  int ts = d->T;
  while (ts > 4 && waves * ((d->T + ts - 1) / ts) < 1024) ts = (ts + 1) / 2;
  return ts;
}

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_x3d_ab_s2_supported(const MspiX3dAbS2Desc* d) {
  if (!d) return 0;
  if (d->H < 2 || d->W < 2 || d->H % 2 || d->W % 2 || d->T < 1) return 0;
  const int ks = (d->Cin + 31) / 32;
  const bool tile_ok = (d->H / 2) % S2_TO == 0 && (d->W / 2) % S2_TO == 0;
  return ks >= 1 && ks <= 3 && tile_ok && d->Cin % 8 == 0 && d->Cmid % 4 == 0 && d->Cin >= 8 && d->Cmid >= 4;
}

extern "C" int mspi_x3d_ab_s2_pool_rows(const MspiX3dAbS2Desc* d) {
  if (!mspi_x3d_ab_s2_supported(d)) return 0;
  X3dAbS2Args a;
  x3d_s2_geometry(d, a);
  return a.tiles * a.nseg;
}

// The instantiation mspi_x3d_ab_s2_fwd runs: x3d_ab_s2_kernel<KS> as KS * 10000 + 7071 (7 x 7 output tiles, one output per
// thread); -1 = a descriptor the launch refuses.  mspi_x3d_ab_s2_fwd switches on this code.
static int x3d_ab_s2_select(const MspiX3dAbS2Desc* d) {
  MSPI_REQUIRE(mspi_x3d_ab_s2_supported(d), "mspi_x3d_ab_s2_fwd: shape N=%d T=%d H=%d W=%d Cin=%d Cmid=%d is outside the fused kernel's range",
               d->N, d->T, d->H, d->W, d->Cin, d->Cmid);
  MSPI_REQUIRE(d->N >= 1 && d->N < 65536 && d->ldx >= d->Cin && d->ldu >= d->Cmid && d->ldx % 4 == 0 && d->ldu % 4 == 0,
               "mspi_x3d_ab_s2_fwd: row strides must cover the row and be multiples of 4 floats");
  MSPI_REQUIRE((long)d->H * d->W * d->ldx < (1L << 31), "mspi_x3d_ab_s2_fwd: one frame of x must stay below 2^31 floats");
  MSPI_REQUIRE(d->act == MSPI_ACT_NONE || d->act == MSPI_ACT_SWISH, "mspi_x3d_ab_s2_fwd: act must be NONE or SWISH");
  MSPI_REQUIRE(d->wa_scale > 0.f, "mspi_x3d_ab_s2_fwd: wa_scale must be positive");
  return ((d->Cin + 31) / 32) * 10000 + 7071;
}

extern "C" int mspi_x3d_ab_s2_variant(const MspiX3dAbS2Desc* d) {
  MSPI_REQUIRE(d, "mspi_x3d_ab_s2_variant: null descriptor");
  return x3d_ab_s2_select(d);
}

extern "C" int mspi_x3d_ab_s2_fwd(const MspiX3dAbS2Desc* d, const void* x, const void* wa_packed, const void* bias_a, const void* wb,
                                  const void* bias_b, void* u, void* pool, void* stream) {
  MSPI_REQUIRE(d && x && wa_packed && bias_a && wb && bias_b && u, "mspi_x3d_ab_s2_fwd: null argument");
  const int variant = x3d_ab_s2_select(d);
  if (variant < 0) return variant;
  MSPI_REQUIRE(aligned16(x) && aligned16(u) && aligned16(wb) && aligned16(bias_b) && aligned16(wa_packed), "mspi_x3d_ab_s2_fwd: 16-byte alignment");
  X3dAbS2Args a;
  a.x = (const float*)x; a.wa = (const unsigned char*)wa_packed; a.ba = (const float*)bias_a; a.wb = (const float*)wb;
  a.bb = (const float*)bias_b; a.u = (float*)u; a.pool = (float*)pool;
  a.N = d->N; a.T = d->T; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cmid = d->Cmid; a.ldx = d->ldx; a.ldu = d->ldu;
  a.act = d->act; a.inv_s = 1.0f / d->wa_scale;
  static const int dbg = getenv("MSPI_X3D_DBG") ? atoi(getenv("MSPI_X3D_DBG")) : 0;
  static const int tseg_env = getenv("MSPI_X3D_TSEG") ? atoi(getenv("MSPI_X3D_TSEG")) : 0;
  a.dbg = dbg;
  a.status = g_status_word;
  x3d_s2_geometry(d, a);
  if (tseg_env > 0 && !pool) { a.tseg = tseg_env; a.nseg = (d->T + a.tseg - 1) / a.tseg; }
  hipStream_t s = (hipStream_t)stream;
  switch (variant / 10000) {
    case 1: launch_ab_s2<1>(a, s); break;
    case 2: launch_ab_s2<2>(a, s); break;
    default: launch_ab_s2<3>(a, s); break;
  }
  return check_launch("mspi_x3d_ab_s2_fwd");
}


extern "C" int mspi_x3d_stem_supported(const MspiX3dStemDesc* d) {
  if (!d) return 0;
  if (d->N < 1 || d->N >= 65536 || d->T < 1 || d->T >= 65536 || d->H < 1 || d->W < 1) return 0;
  if (d->sN < 0 || d->sC < 0 || d->sT < 0 || d->sH < 0 || d->sW < 0) return 0;
  // a tap's offset inside one (sample, channel, frame) plane is a 32-bit int in the kernel
  return (long)(d->H - 1) * d->sH + (long)(d->W - 1) * d->sW < (1L << 31) && (long)d->H * d->W < (1L << 31);
}

// x3d_stem_kernel has one instantiation; the code is the number of frames per T segment it runs with (-1: refused)
extern "C" int mspi_x3d_stem_variant(const MspiX3dStemDesc* d) {
  MSPI_REQUIRE(d, "mspi_x3d_stem_variant: null descriptor");
  MSPI_REQUIRE(mspi_x3d_stem_supported(d), "mspi_x3d_stem_fwd: shape N=%d T=%d H=%d W=%d or its strides are outside the fused stem's range",
               d->N, d->T, d->H, d->W);
  return x3d_stem_tseg(d);
}

extern "C" int mspi_x3d_stem_fwd(const MspiX3dStemDesc* d, const void* x, const void* wxy, const void* wt, const void* bias, void* y,
                                 void* stream) {
  MSPI_REQUIRE(d && x && wxy && wt && bias && y, "mspi_x3d_stem_fwd: null argument");
  const int tseg = mspi_x3d_stem_variant(d);
  if (tseg < 0) return tseg;
  MSPI_REQUIRE(d->ldy >= STEM_C && d->ldy % 4 == 0, "mspi_x3d_stem_fwd: the output row stride must cover 24 channels and be a multiple of 4 floats");
  MSPI_REQUIRE(aligned16(y) && (reinterpret_cast<uintptr_t>(x) & 3u) == 0, "mspi_x3d_stem_fwd: y must be 16-byte aligned, x 4-byte aligned");
  X3dStemArgs a;
  a.x = (const float*)x; a.y = (float*)y;
  const float *hxy = (const float*)wxy, *ht = (const float*)wt, *hb = (const float*)bias;
  memset(a.wxy, 0, sizeof(a.wxy)); memset(a.wt, 0, sizeof(a.wt));
  for (int c = 0; c < STEM_C; ++c) {
    for (int k = 0; k < 27; ++k) a.wxy[c][k] = hxy[k * STEM_C + c];
    for (int k = 0; k < 5; ++k) a.wt[c][k] = ht[k * STEM_C + c];
    a.wt[c][5] = hb[c];
  }
  a.N = d->N; a.T = d->T; a.H = d->H; a.W = d->W; a.Ho = (d->H - 1) / 2 + 1; a.Wo = (d->W - 1) / 2 + 1;
  a.sN = d->sN; a.sC = d->sC; a.sT = d->sT; a.sH = d->sH; a.sW = d->sW; a.ldy = d->ldy;
  a.tseg = tseg; a.nseg = (d->T + tseg - 1) / tseg;
  const dim3 grid((unsigned)((a.Ho * a.Wo + 255) / 256), (unsigned)a.nseg, (unsigned)a.N);
  hipLaunchKernelGGL(x3d_stem_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("mspi_x3d_stem_fwd");
}
