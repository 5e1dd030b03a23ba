// Backward of the decoder's readout tail (model/model_utils.py:403-409 as _SaliencyBase._readout_tail computes it):
//   a8 = conv r8 (4,1,1)/4   u = relu(up4(a8))   y10 = relu(conv r10 (1,3,3))   z = conv r12 (1,3,3) -> 1   out = z - lse(z)
// Four entry points, run in reverse:
//   mspi_logsumexp_sub_bwd  dz = g - exp(out) sum(g)                                   one workgroup per sample
//   mspi_conv_c1_bwd        d10 = (y10 > 0) conv_T(dz), dW12, db12                     one pass over y10
//   mspi_conv_wgrad_fwd     dW = dy^T im2col(x), db = sum dy                           fp32 MFMA, rows split over workgroups
//   mspi_upsample_bwd       adjoint of mspi_upsample_fwd, ReLU mask from the saved u   gather, one thread per source vector
// The data gradients of r10 and r8 are forward convolutions with transposed weights (mspi_conv_fwd and friends).
// Every sum that crosses a workgroup goes through the caller's workspace as per-workgroup partials, and a second launch
// adds them in a fixed order: no float atomics, bitwise repeatable.  Nothing here allocates or synchronises.
#include "common.h"
#include "conv_common.h"
#include "upsample_adjoint.h"

namespace mspi {

// ------------------------------------------------------------------------------------------------ shared pieces
// Sum (or max) over a workgroup of NW waves, result in every thread.  Fixed order: xor tree, then the waves left to right.
template <int NW>
__device__ __forceinline__ float rb_block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) r += sh[i];
  return r;
}

// Sum of S partial records for one output element, by 4 thread groups: group g adds records g, g + 4, ... in order, then
// (p0 + p1) + (p2 + p3).  part[4][64] in LDS; blockDim 256 = 64 elements x 4 groups.  Valid in group 0.
__device__ __forceinline__ float rb_sum_records(const float* __restrict__ p, long stride, int S, bool live, float (*part)[64]) {
  const int g = threadIdx.x >> 6, e = threadIdx.x & 63;
  float s = 0.f;
  if (live)
    for (int i = g; i < S; i += 4) s += p[(long)i * stride];
  part[g][e] = s;
  __syncthreads();
  return (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
}

// ------------------------------------------------------------------------------------------------ log-softmax backward
__global__ __launch_bounds__(1024) void logsumexp_sub_bwd_kernel(const float* __restrict__ logp, const float* __restrict__ g,
                                                                 float* __restrict__ dz, int L) {
  __shared__ float red[16];
  const long base = (long)blockIdx.x * L;
  float s = 0.f;
  for (int i = threadIdx.x; i < L; i += 1024) s += g[base + i];
  const float G = rb_block_sum<16>(s, red);
  for (int i = threadIdx.x; i < L; i += 1024) dz[base + i] = g[base + i] - expf(logp[base + i]) * G;
}

// ------------------------------------------------------------------------------------------------ last conv (C -> 1) backward
constexpr int C1_T = 256;              // threads per workgroup
constexpr int C1_ROWS = 1024;          // rows (output positions) per workgroup
constexpr int C1_REC = 9 * 64 + 4;     // floats per workgroup record: dW12 [9][C] then db12 (C <= 64)

__host__ __device__ inline int c1_groups(long M) { return (int)((M + C1_ROWS - 1) / C1_ROWS); }

// The nine taps of dz that reach position (h, w): s[kh * 3 + kw] = dz[h - (kh - 1)][w - (kw - 1)], 0 outside the image.
__device__ __forceinline__ void c1_taps(const float* __restrict__ dzn, int h, int w, int H, int W, float (&s)[9]) {
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int hh = h - (kh - 1), ww = w - (kw - 1);
      s[kh * 3 + kw] = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? dzn[(long)hh * W + ww] : 0.f;
    }
}

__global__ __launch_bounds__(C1_T) void conv_c1_bwd_kernel(const float* __restrict__ y, long ldy, const float* __restrict__ dz,
                                                           const float* __restrict__ w, float* __restrict__ d, long ldd,
                                                           float* __restrict__ ws, long M, int H, int W, int C) {
  __shared__ float4 shw[C1_T][9];      // 36 KB: every thread's dW12 partial
  __shared__ float shb[C1_T];
  const int CV = C >> 2, RP = C1_T / CV;           // channel vectors per row, rows per pass
  const int cv = threadIdx.x % CV, rr = threadIdx.x / CV;
  const bool live = rr < RP;
  float4 wt[9], acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    wt[t] = live ? *reinterpret_cast<const float4*>(w + t * C + cv * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float accb = 0.f;
  const long p0 = (long)blockIdx.x * C1_ROWS;
  const long p1 = p0 + C1_ROWS < M ? p0 + C1_ROWS : M;
  const long HW = (long)H * W;
  if (live) {
    for (long p = p0 + rr; p < p1; p += RP) {
      const long n = (long)((unsigned)p / (unsigned)HW);          // M < 2^31 (host-checked): 32-bit divisions
      const int q = (int)(p - n * HW), h = q / W, x = q - h * W;
      float s[9];
      c1_taps(dz + n * HW, h, x, H, W, s);
      const float4 v = *reinterpret_cast<const float4*>(y + p * ldy + cv * 4);
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        o.x = fmaf(s[t], wt[t].x, o.x); o.y = fmaf(s[t], wt[t].y, o.y); o.z = fmaf(s[t], wt[t].z, o.z); o.w = fmaf(s[t], wt[t].w, o.w);
        acc[t].x = fmaf(s[t], v.x, acc[t].x); acc[t].y = fmaf(s[t], v.y, acc[t].y);
        acc[t].z = fmaf(s[t], v.z, acc[t].z); acc[t].w = fmaf(s[t], v.w, acc[t].w);
      }
      o.x = v.x > 0.f ? o.x : 0.f; o.y = v.y > 0.f ? o.y : 0.f; o.z = v.z > 0.f ? o.z : 0.f; o.w = v.w > 0.f ? o.w : 0.f;
      *reinterpret_cast<float4*>(d + p * ldd + cv * 4) = o;
      if (cv == 0) accb += s[4];                   // the centre tap is dz[p] itself
    }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) shw[threadIdx.x][t] = acc[t];
  shb[threadIdx.x] = (live && cv == 0) ? accb : 0.f;
  __syncthreads();
  // the workgroup's record: element (t, c) is the sum over the RP row groups in order
  float* rec = ws + (long)blockIdx.x * C1_REC;
  for (int e = threadIdx.x; e < 9 * C; e += C1_T) {
    const int t = e / C, c = e - t * C;
    float sum = 0.f;
    for (int r = 0; r < RP; ++r) sum += reinterpret_cast<const float*>(&shw[r * CV + (c >> 2)][t])[c & 3];
    rec[e] = sum;
  }
  if (threadIdx.x == 0) {
    float sum = 0.f;
    for (int r = 0; r < RP; ++r) sum += shb[r * CV];
    rec[9 * C] = sum;
  }
}

// dW12 [9][C] and db12 from the workgroup records; grid ceil((9 C + 1) / 64), 256 threads.
__global__ __launch_bounds__(256) void conv_c1_bwd_reduce_kernel(const float* __restrict__ ws, int S, int C, float* __restrict__ dW,
                                                                 float* __restrict__ db) {
  __shared__ float part[4][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), n = 9 * C + 1;
  const float r = rb_sum_records(ws + e, C1_REC, S, e < n, part);
  if (threadIdx.x < 64 && e < n) {
    if (e < 9 * C) dW[e] = r;
    else *db = r;
  }
}

// ------------------------------------------------------------------------------------------------ conv weight gradient
// dW[co][(tap, ci)] = sum_m dy[m][co] * x[pos(m, tap)][ci] on v_mfma_f32_32x32x2_f32 with the ROW index as the contraction:
// D[i = co][j = ci of one 32-channel tile] += A[i][k] B[k][j] with k = two consecutive rows m.  Lane l feeds
// A = dy[m + (l >> 5)][l & 31] and B = x[pos(m + (l >> 5), tap)][32 cb + (l & 31)], both straight from memory as 128-byte row
// segments: no LDS on the way in.  A wave keeps WG_TPW (tap, channel-block) tiles in accumulators; blockIdx.y picks the tile
// group, blockIdx.x the slice of rows, whose four quarters go to the four waves.  The waves' accumulators are added through
// LDS in wave order and the slice's partial goes to the workspace: [slice][32][KT * 32] then [32] sums of dy.
constexpr int WG_T = 256;
constexpr int WG_TPW = 3;               // tiles per wave
constexpr int WG_U = 4;                 // row pairs in flight per wave
constexpr int WG_SLICE_SMALL = 256;     // rows per slice below WG_BIG_M rows
constexpr int WG_SLICE_BIG = 2048;      // rows per slice from WG_BIG_M rows on
constexpr long WG_BIG_M = 65536;
constexpr int WG_MAX_TAPS = 27;

struct WgradGeom {
  int N, T, H, W, C;
  long sN, sT, sH, sW;
  int kT, kH, kW, strT, strH, strW, padT, padH, padW;
  int To, Ho, Wo, Cout;
  long ldy, M;
  int CB, KT, slice;                    // channel blocks of 32, tiles = taps * CB, rows per slice
};

__host__ __device__ inline int wg_slice_rows(long M) { return M >= WG_BIG_M ? WG_SLICE_BIG : WG_SLICE_SMALL; }
__host__ __device__ inline long wg_record_floats(int KT) { return 32L * KT * 32 + 32; }

__global__ __launch_bounds__(WG_T) void conv_wgrad_kernel(WgradGeom g, const float* __restrict__ x, const float* __restrict__ dy,
                                                          float* __restrict__ ws) {
  __shared__ float sh[4][WG_TPW * 1024];           // 48 KB
  __shared__ float shb[4][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
  const int t0 = blockIdx.y * WG_TPW;
  // this wave's rows: a quarter of the slice
  const long s0 = (long)blockIdx.x * g.slice;
  const int quarter = g.slice >> 2;
  const long r0 = s0 + (long)wave * quarter;
  long r1 = r0 + quarter;
  if (r1 > g.M) r1 = g.M;

  // per tile: tap offsets and this lane's channel
  int tt[WG_TPW], th[WG_TPW], tw[WG_TPW], tc[WG_TPW];
  bool tok[WG_TPW];
#pragma unroll
  for (int j = 0; j < WG_TPW; ++j) {
    const int t = t0 + j;
    const int tap = t / g.CB, cb = t - tap * g.CB;
    tc[j] = cb * 32 + li;
    tok[j] = t < g.KT && tc[j] < g.C;
    tw[j] = tap % g.kW;
    th[j] = (tap / g.kW) % g.kH;
    tt[j] = tap / (g.kW * g.kH);
  }
  v16f acc[WG_TPW];
#pragma unroll
  for (int j = 0; j < WG_TPW; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  float bsum = 0.f;
  const bool cok = li < g.Cout;

  for (long m0 = r0; m0 < r1; m0 += 2 * WG_U) {
    float a[WG_U], b[WG_U][WG_TPW];
#pragma unroll
    for (int u = 0; u < WG_U; ++u) {
      const long m = m0 + 2 * u + lh;
      const bool rok = m < r1;
      a[u] = (rok && cok) ? dy[m * g.ldy + li] : 0.f;
      // m -> (n, to, ho, wo)
      unsigned q = rok ? (unsigned)m : 0u;             // M < 2^31 (checked on the host): 32-bit divisions
      const int wo = (int)(q % (unsigned)g.Wo); q /= (unsigned)g.Wo;
      const int ho = (int)(q % (unsigned)g.Ho); q /= (unsigned)g.Ho;
      const int to = (int)(q % (unsigned)g.To);
      const long n = (long)(q / (unsigned)g.To);
#pragma unroll
      for (int j = 0; j < WG_TPW; ++j) {
        const int ti = to * g.strT + tt[j] - g.padT, hi = ho * g.strH + th[j] - g.padH, wi = wo * g.strW + tw[j] - g.padW;
        const bool ok = rok && tok[j] && ti >= 0 && ti < g.T && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
        b[u][j] = ok ? x[n * g.sN + ti * g.sT + hi * g.sH + wi * g.sW + tc[j]] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < WG_U; ++u) {
      bsum += a[u];
#pragma unroll
      for (int j = 0; j < WG_TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u][j], acc[j], 0, 0, 0);
    }
  }
  // accumulator (reg r, lane) -> D[co = (r & 3) + 8 (r >> 2) + 4 lh][j = li]
#pragma unroll
  for (int j = 0; j < WG_TPW; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) sh[wave][j * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + li] = acc[j][r];
  bsum += __shfl_xor(bsum, 32, 64);                // the two rows of every pair
  if (lane < 32) shb[wave][lane] = bsum;
  __syncthreads();
  float* rec = ws + (long)blockIdx.x * wg_record_floats(g.KT);
  const int ldk = g.KT * 32;
  for (int e = threadIdx.x; e < WG_TPW * 1024; e += WG_T) {
    const int j = e >> 10, co = (e >> 5) & 31, c = e & 31;
    if (t0 + j < g.KT) rec[(long)co * ldk + (t0 + j) * 32 + c] = (sh[0][e] + sh[1][e]) + (sh[2][e] + sh[3][e]);
  }
  if (blockIdx.y == 0 && threadIdx.x < 32)
    rec[32L * ldk + threadIdx.x] = (shb[0][threadIdx.x] + shb[1][threadIdx.x]) + (shb[2][threadIdx.x] + shb[3][threadIdx.x]);
}

// dW [Cout][taps * C] and db [Cout] from the slice records; one thread group of four per output element.
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ ws, int S, int KT, int CB, int C, int Cout,
                                                                int taps, float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float part[4][64];
  const int K = taps * C, nW = Cout * K, n = nW + Cout;
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < n;
  long off = 0;
  if (live) {
    if (e < nW) {
      const int co = e / K, k = e - co * K, tap = k / C, ci = k - tap * C;
      off = (long)co * KT * 32 + (tap * CB + (ci >> 5)) * 32 + (ci & 31);
    } else {
      off = 32L * KT * 32 + (e - nW);
    }
  }
  const float r = rb_sum_records(ws + off, wg_record_floats(KT), S, live, part);
  if (threadIdx.x < 64 && live) {
    if (e < nW) dW[e] = r;
    else db[e - nW] = r;
  }
}

// ------------------------------------------------------------------------------------------------ up-sample adjoint
// Gather form of upsample_kernel's adjoint (up_gather, upsample_adjoint.h): one thread per source vector.
template <int K, bool RELU>
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const float* __restrict__ dy, long ldy, const float* __restrict__ u,
                                                           long ldu, float* __restrict__ dx, long ldx, int NT, int H, int W, int CV) {
  const long total = (long)NT * H * W * CV;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;      // one source vector per thread (fewer than 2^31, host-checked)
  if (idx < total) {
    const unsigned ui = (unsigned)idx;
    const int cv = (int)(ui % (unsigned)CV);
    unsigned pos = ui / (unsigned)CV;
    const int w = (int)(pos % (unsigned)W);
    pos /= (unsigned)W;
    const int h = (int)(pos % (unsigned)H);
    const long nt = (long)(pos / (unsigned)H);
    const float4 acc = up_gather<K, RELU>(dy, ldy, u, ldu, nt, h, w, H, W, cv);
    *reinterpret_cast<float4*>(dx + ((nt * H + h) * W + w) * ldx + cv * 4) = acc;
  }
}

// Why the launch refuses `d` (NULL: it does not); the pointers may be NULL when only the descriptor is asked about.
static const char* wgrad_refusal(const MspiConvDesc* d) {
  if (!d) return "null descriptor";
  if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0 || d->To <= 0 || d->Ho <= 0 || d->Wo <= 0) return "empty extent";
  if (d->kT <= 0 || d->kH <= 0 || d->kW <= 0 || d->strT <= 0 || d->strH <= 0 || d->strW <= 0 || d->padT < 0 || d->padH < 0 ||
      d->padW < 0)
    return "bad kernel, stride or padding";
  if ((long)d->kT * d->kH * d->kW > WG_MAX_TAPS) return "more than 27 taps";
  if (d->To != (d->T + 2 * d->padT - d->kT) / d->strT + 1 || d->Ho != (d->H + 2 * d->padH - d->kH) / d->strH + 1 ||
      d->Wo != (d->W + 2 * d->padW - d->kW) / d->strW + 1)
    return "output extent does not follow from the input extent";
  if (d->Cout < 4 || d->Cout > 32 || d->Cout % 4) return "stored Cout must be a multiple of 4, at most 32";
  if (d->C < 4 || d->C > 64 || d->C % 4) return "stored Cin must be a multiple of 4, at most 64";
  if (d->sC != 1) return "the input must be channels-last (sC == 1)";
  if (d->ldy < d->Cout) return "ldy < Cout";
  if ((long)d->N * d->To * d->Ho * d->Wo >= (1L << 31)) return "2^31 or more output rows";
  return nullptr;
}

static WgradGeom wgrad_geom(const MspiConvDesc* d) {
  WgradGeom g;
  g.N = d->N; g.T = d->T; g.H = d->H; g.W = d->W; g.C = d->C;
  g.sN = d->sN; g.sT = d->sT; g.sH = d->sH; g.sW = d->sW;
  g.kT = d->kT; g.kH = d->kH; g.kW = d->kW; g.strT = d->strT; g.strH = d->strH; g.strW = d->strW;
  g.padT = d->padT; g.padH = d->padH; g.padW = d->padW;
  g.To = d->To; g.Ho = d->Ho; g.Wo = d->Wo; g.Cout = d->Cout;
  g.ldy = d->ldy;
  g.M = (long)d->N * d->To * d->Ho * d->Wo;
  g.CB = (d->C + 31) / 32;
  g.KT = d->kT * d->kH * d->kW * g.CB;
  g.slice = wg_slice_rows(g.M);
  return g;
}

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_logsumexp_sub_bwd(const float* logp, const float* g, float* dz, int32_t N, int32_t L, mspi_stream_t stream) {
  MSPI_REQUIRE(logp && g && dz && N > 0 && L > 0, "mspi_logsumexp_sub_bwd: bad argument");
  hipLaunchKernelGGL(logsumexp_sub_bwd_kernel, dim3(N), dim3(1024), 0, (hipStream_t)stream, logp, g, dz, L);
  return check_launch("mspi_logsumexp_sub_bwd");
}

extern "C" size_t mspi_conv_c1_bwd_ws_bytes(int32_t N, int32_t H, int32_t W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)c1_groups((long)N * H * W) * C1_REC * sizeof(float);
}

extern "C" int mspi_conv_c1_bwd(const float* y, int64_t ldy, const float* dz, const float* w, float* d, int64_t ldd, float* dW,
                                float* db, void* ws, int32_t N, int32_t H, int32_t W, int32_t C, mspi_stream_t stream) {
  MSPI_REQUIRE(y && dz && w && d && dW && db && ws, "mspi_conv_c1_bwd: null argument");
  MSPI_REQUIRE(N > 0 && H > 0 && W > 0 && (long)N * H * W < (1L << 31), "mspi_conv_c1_bwd: bad extent");
  MSPI_REQUIRE(C >= 4 && C <= 64 && C % 4 == 0, "mspi_conv_c1_bwd: C must be a multiple of 4, at most 64");
  MSPI_REQUIRE(ldy >= C && ldd >= C && ldy % 4 == 0 && ldd % 4 == 0 && aligned16(y) && aligned16(d) && aligned16(w) && aligned16(ws),
               "mspi_conv_c1_bwd: row strides must be multiples of 4 (>= C), y / d / w / ws 16-byte aligned");
  const long M = (long)N * H * W;
  const int S = c1_groups(M);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conv_c1_bwd_kernel, dim3(S), dim3(C1_T), 0, st, y, (long)ldy, dz, w, d, (long)ldd, (float*)ws, M, H, W, C);
  hipLaunchKernelGGL(conv_c1_bwd_reduce_kernel, dim3((9 * C + 1 + 63) / 64), dim3(256), 0, st, (const float*)ws, S, C, dW, db);
  return check_launch("mspi_conv_c1_bwd");
}

extern "C" int mspi_conv_wgrad_supported(const MspiConvDesc* d) {
  const char* why = wgrad_refusal(d);
  if (why) set_error("mspi_conv_wgrad: %s", why);
  return why ? 0 : 1;
}

extern "C" size_t mspi_conv_wgrad_ws_bytes(const MspiConvDesc* d) {
  if (wgrad_refusal(d)) return 0;
  const WgradGeom g = wgrad_geom(d);
  return (size_t)((g.M + g.slice - 1) / g.slice) * wg_record_floats(g.KT) * sizeof(float);
}

extern "C" int mspi_conv_wgrad_variant(const MspiConvDesc* d, const void* x, const void* dy) {
  const char* why = wgrad_refusal(d);
  if (!why && !(aligned16(x) && aligned16(dy))) why = "x and dy must be 16-byte aligned";
  if (why) {
    set_error("mspi_conv_wgrad: %s", why);
    return -1;
  }
  return wg_slice_rows((long)d->N * d->To * d->Ho * d->Wo);
}

extern "C" int mspi_conv_wgrad_fwd(const MspiConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                                   mspi_stream_t stream) {
  MSPI_REQUIRE(x && dy && dW && db && ws, "mspi_conv_wgrad_fwd: null argument");
  if (mspi_conv_wgrad_variant(d, x, dy) < 0) return MSPI_EINVAL;
  MSPI_REQUIRE(aligned16(ws) && aligned16(dW), "mspi_conv_wgrad: dW and ws must be 16-byte aligned");
  const WgradGeom g = wgrad_geom(d);
  const int S = (int)((g.M + g.slice - 1) / g.slice);
  const int taps = d->kT * d->kH * d->kW;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conv_wgrad_kernel, dim3(S, (g.KT + WG_TPW - 1) / WG_TPW), dim3(WG_T), 0, st, g, x, dy, (float*)ws);
  const int n = d->Cout * taps * d->C + d->Cout;
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((n + 63) / 64), dim3(256), 0, st, (const float*)ws, S, g.KT, g.CB, d->C, d->Cout,
                     taps, dW, db);
  return check_launch("mspi_conv_wgrad_fwd");
}

extern "C" int mspi_upsample_bwd(const float* dy, int64_t ldy, const float* u, int64_t ldu, float* dx, int64_t ldx, int32_t NT,
                                 int32_t H, int32_t W, int32_t C, int32_t factor, int32_t act, mspi_stream_t stream) {
  MSPI_REQUIRE(dy && dx, "mspi_upsample_bwd: null argument");
  MSPI_REQUIRE(NT > 0 && H > 0 && W > 0 && C > 0, "mspi_upsample_bwd: bad extent");
  MSPI_REQUIRE(factor == 2 || factor == 4 || factor == 8, "mspi_upsample_bwd: factor must be 2, 4 or 8");
  MSPI_REQUIRE(act == MSPI_ACT_NONE || act == MSPI_ACT_RELU, "mspi_upsample_bwd: act must be MSPI_ACT_NONE or MSPI_ACT_RELU");
  MSPI_REQUIRE(act == MSPI_ACT_NONE || u, "mspi_upsample_bwd: MSPI_ACT_RELU needs the forward's output u");
  const bool relu = act == MSPI_ACT_RELU;
  MSPI_REQUIRE(C % 4 == 0 && ldy % 4 == 0 && ldx % 4 == 0 && ldy >= C && ldx >= C && aligned16(dy) && aligned16(dx) &&
                   (!relu || (ldu % 4 == 0 && ldu >= C && aligned16(u))),
               "mspi_upsample_bwd: C/ld must be multiples of 4, pointers 16-B aligned");
  const long total = (long)NT * H * W * (C / 4);
  MSPI_REQUIRE((long)NT * H * factor * W * factor * (C / 4) < (1L << 31), "mspi_upsample_bwd: more than 2^31 destination vectors");
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define MSPI_UP_BWD(KK)                                                                                                        \
  if (relu) hipLaunchKernelGGL((upsample_bwd_kernel<KK, true>), grid, block, 0, st, dy, (long)ldy, u, (long)ldu, dx, (long)ldx, \
                               NT, H, W, C / 4);                                                                                \
  else hipLaunchKernelGGL((upsample_bwd_kernel<KK, false>), grid, block, 0, st, dy, (long)ldy, u, (long)ldu, dx, (long)ldx, NT, \
                          H, W, C / 4);
  if (factor == 2) { MSPI_UP_BWD(2) } else if (factor == 4) { MSPI_UP_BWD(4) } else { MSPI_UP_BWD(8) }
#undef MSPI_UP_BWD
  return check_launch("mspi_upsample_bwd");
}
