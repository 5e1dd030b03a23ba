// Training kernels for the three convs in front of the readout tail (readout[0], [1]+BN, [4]+BN of model/model_utils.py:490-504):
//   mspi_conv_wgrad_wide_fwd   dW = dy^T im2col(x), db = sum dy for up to 192 x 192 channels and 27 taps, stride 1
//   mspi_bn_stats              per-channel mean, biased variance and 1/sqrt(var + eps) over the M rows of a batch
//   mspi_bn_apply              y = gamma (x - mean) rstd + beta, optional ReLU
//   mspi_bn_bwd                dgamma, dbeta and dx of that, x^ recomputed, the ReLU mask taken from the forward's output
// Every sum that crosses a workgroup goes through the caller's workspace as per-workgroup records that a second launch
// adds (or merges) in a fixed order: no float atomics, bitwise repeatable.  Nothing here allocates or synchronises.
#include "common.h"
#include "conv_common.h"

namespace mspi {

// ------------------------------------------------------------------------------------------------ wide weight gradient
// A workgroup owns one (32 output channels, 32 input channels) pair, ALL taps of it, and a slice of the output rows.  The
// rows come as boxes of TR x HR x WR output positions (<= 128 rows) of one sample.  Per box the workgroup stages, once,
//   dL [R][32]   its 32 columns of dy for the box's rows                                  (zero where the box leaves the map)
//   xL [P][32]   its 32 channels of x over the box grown by the kernel's halo, P = (TR + kT - 1)(HR + kH - 1)(WR + kW - 1)
//                positions                                                                (zero where that is padding)
// and every tap reads its B operand from xL at a constant offset from the row's own position: nothing is fetched per tap.
// v_mfma_f32_32x32x2_f32 with the ROW index as the contraction: D[co][ci] += A[co][k] B[k][ci], k = two consecutive rows of
// the box, lane l feeding A = dL[2 s + (l >> 5)][l & 31] and B = xL[pos(2 s + (l >> 5)) + tap][l & 31].  Wave w keeps taps
// w, w + 4, ... (up to TPW = 7 tiles = 112 accumulator registers) over the whole slice.  A 1 x 1 x 1 kernel has one tile:
// there the four waves take a quarter of every box's rows each and their accumulators are added through LDS in wave order.
// The slice's partial goes to the workspace as one record [Cout][taps * C] + [Cout], the layout of dW and db themselves.
constexpr int WW_T = 256;
constexpr int WW_ROWS = 128;            // output rows per staged box
constexpr int WW_MAX_POS = 368;         // staged input positions per box: 368 x 128 B = 46 KB
constexpr int WW_BPS_SMALL = 4;         // boxes per slice below WW_BIG_BOXES boxes
constexpr int WW_BPS_BIG = 32;          // boxes per slice from WW_BIG_BOXES boxes on
constexpr int WW_BIG_BOXES = 512;
constexpr int WW_MAX_TAPS = 27;
constexpr int WW_MAX_CH = 192;

struct WideGeom {
  int N, T, H, W, C;
  long sN, sT, sH, sW;
  int kT, kH, kW, padT, padH, padW;
  int To, Ho, Wo, Cout;
  long ldy;
  int TR, HR, WR;                       // box of output positions
  int BT, BH, BW;                       // staged box of input positions
  int nbT, nbH, nbW;                    // boxes per axis
  int R, P;                             // rows per box (padded to a multiple of 8), staged positions
  long NB;                              // boxes in all
  int bps, S;                           // boxes per slice, slices
  int taps, CBi, CBo, K;                // K = taps * C
};

__host__ __device__ inline int ww_x_floats(int P) { return P * 32 > 4096 ? P * 32 : 4096; }   // 4096: the four waves' tiles (1 tap)
__host__ __device__ inline long ww_record_floats(int Cout, int K) { return (long)Cout * K + Cout; }

template <int TPW, bool SPLIT>
__global__ __launch_bounds__(WW_T) void conv_wgrad_wide_kernel(WideGeom g, const float* __restrict__ x, const float* __restrict__ dy,
                                                               float* __restrict__ ws) {
  extern __shared__ float4 ww_lds[];
  float* xL = reinterpret_cast<float*>(ww_lds);
  float* dL = xL + ww_x_floats(g.P);
  int* tbl = reinterpret_cast<int*>(dL + g.R * 32);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int cob = blockIdx.y / g.CBi, cib = blockIdx.y - cob * g.CBi;
  const int rows = g.TR * g.HR * g.WR;

  // row of the box -> its position in the staged input box (x 32 floats); the padding rows read position 0 against dy = 0
  for (int r = tid; r < g.R; r += WW_T) {
    int v = 0;
    if (r < rows) {
      const int wr = r % g.WR, q = r / g.WR, hr = q % g.HR, tr = q / g.HR;
      v = (tr * g.BH + hr) * g.BW + wr;
    }
    tbl[r] = v * 32;
  }
  int toff[TPW];
  bool tok[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int tap = SPLIT ? 0 : wave + 4 * j;
    tok[j] = tap < g.taps;
    const int t = tok[j] ? tap : 0;
    const int kw = t % g.kW, kh = (t / g.kW) % g.kH, kt = t / (g.kW * g.kH);
    toff[j] = ((kt * g.BH + kh) * g.BW + kw) * 32 + li;
  }
  v16f acc[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  float bsum = 0.f;

  const long b0 = (long)blockIdx.x * g.bps;
  const long b1 = b0 + g.bps < g.NB ? b0 + g.bps : g.NB;
  const int c4 = (tid & 7) * 4;
  for (long b = b0; b < b1; ++b) {
    unsigned q = (unsigned)b;                            // fewer than 2^31 rows (host-checked), so fewer boxes
    const int wo0 = (int)(q % (unsigned)g.nbW) * g.WR; q /= (unsigned)g.nbW;
    const int ho0 = (int)(q % (unsigned)g.nbH) * g.HR; q /= (unsigned)g.nbH;
    const int to0 = (int)(q % (unsigned)g.nbT) * g.TR;
    const long n = (long)(q / (unsigned)g.nbT);
    __syncthreads();                                     // the previous box has been read (first pass: tbl is written)
    for (int p = tid >> 3; p < g.P; p += WW_T / 8) {
      const int pw = p % g.BW, q2 = p / g.BW, ph = q2 % g.BH, pt = q2 / g.BH;
      const int ti = to0 + pt - g.padT, hi = ho0 + ph - g.padH, wi = wo0 + pw - g.padW;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ti >= 0 && ti < g.T && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W)
        v = *reinterpret_cast<const float4*>(x + n * g.sN + ti * g.sT + hi * g.sH + wi * g.sW + cib * 32 + c4);
      *reinterpret_cast<float4*>(xL + p * 32 + c4) = v;
    }
    for (int r = tid >> 3; r < g.R; r += WW_T / 8) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) {
        const int wr = r % g.WR, q2 = r / g.WR, hr = q2 % g.HR, tr = q2 / g.HR;
        const int to = to0 + tr, ho = ho0 + hr, wo = wo0 + wr;
        if (to < g.To && ho < g.Ho && wo < g.Wo) {
          const long m = ((n * g.To + to) * g.Ho + ho) * g.Wo + wo;
          v = *reinterpret_cast<const float4*>(dy + m * g.ldy + cob * 32 + c4);
        }
      }
      *reinterpret_cast<float4*>(dL + r * 32 + c4) = v;
    }
    __syncthreads();
    const int steps = SPLIT ? g.R >> 3 : g.R >> 1;
    const int s0 = SPLIT ? wave * steps : 0;
#pragma unroll 2
    for (int s = s0; s < s0 + steps; ++s) {
      const int r = 2 * s + lh;
      const float a = dL[r * 32 + li];
      const int base = tbl[r];
      bsum += a;
#pragma unroll
      for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xL[base + toff[j]], acc[j], 0, 0, 0);
    }
  }

  // accumulator (reg r, lane) -> D[co = (r & 3) + 8 (r >> 2) + 4 lh][ci = li]
  float* rec = ws + (long)blockIdx.x * ww_record_floats(g.Cout, g.K);
  bsum += __shfl_xor(bsum, 32, 64);                      // the two rows of every pair
  if (!SPLIT) {
#pragma unroll
    for (int j = 0; j < TPW; ++j)
      if (tok[j]) {
        const int tap = wave + 4 * j;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          rec[(long)(cob * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * g.K + tap * g.C + cib * 32 + li] = acc[j][r];
      }
    if (cib == 0 && wave == 0 && lane < 32) rec[(long)g.Cout * g.K + cob * 32 + lane] = bsum;
  } else {
    __syncthreads();                                     // the last box has been read
#pragma unroll
    for (int r = 0; r < 16; ++r) xL[wave * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + li] = acc[0][r];
    if (lane < 32) dL[wave * 32 + lane] = bsum;
    __syncthreads();
    for (int e = tid; e < 1024; e += WW_T)
      rec[(long)(cob * 32 + (e >> 5)) * g.K + cib * 32 + (e & 31)] = (xL[e] + xL[1024 + e]) + (xL[2048 + e] + xL[3072 + e]);
    if (cib == 0 && tid < 32) rec[(long)g.Cout * g.K + cob * 32 + tid] = (dL[tid] + dL[32 + tid]) + (dL[64 + tid] + dL[96 + tid]);
  }
}

// dW [Cout][taps * C] then db [Cout], both in the records' own layout; one thread group of four per element.
__global__ __launch_bounds__(256) void conv_wgrad_wide_reduce_kernel(const float* __restrict__ ws, int S, int nW, int n,
                                                                     float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float part[4][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < n;
  const float r = rt_sum_records(ws + (live ? e : 0), n, S, live, part);
  if (threadIdx.x < 64 && live) {
    if (e < nW) dW[e] = r;
    else db[e - nW] = r;
  }
}

static const char* wide_refusal(const MspiConvDesc* d) {
  if (!d) return "null descriptor";
  if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0 || d->To <= 0 || d->Ho <= 0 || d->Wo <= 0) return "empty extent";
  if (d->kT <= 0 || d->kH <= 0 || d->kW <= 0 || d->strT <= 0 || d->strH <= 0 || d->strW <= 0 || d->padT < 0 || d->padH < 0 ||
      d->padW < 0)
    return "bad kernel, stride or padding";
  if ((long)d->kT * d->kH * d->kW > WW_MAX_TAPS) return "more than 27 taps";
  if (d->strT != 1 || d->strH != 1 || d->strW != 1) return "stride must be 1";
  if (d->To != d->T + 2 * d->padT - d->kT + 1 || d->Ho != d->H + 2 * d->padH - d->kH + 1 || d->Wo != d->W + 2 * d->padW - d->kW + 1)
    return "output extent does not follow from the input extent";
  if (d->Cout < 32 || d->Cout > WW_MAX_CH || d->Cout % 32) return "stored Cout must be a multiple of 32, at most 192";
  if (d->C < 32 || d->C > WW_MAX_CH || d->C % 32) return "stored Cin must be a multiple of 32, at most 192";
  if (d->sC != 1) return "the input must be channels-last (sC == 1)";
  if (d->sN % 4 || d->sT % 4 || d->sH % 4 || d->sW % 4 || d->sW < d->C) return "input strides must be multiples of 4, sW >= Cin";
  if (d->ldy < d->Cout || d->ldy % 4) return "ldy must be a multiple of 4, >= Cout";
  if ((long)d->N * d->To * d->Ho * d->Wo >= (1L << 31)) return "2^31 or more output rows";
  return nullptr;
}

static int ww_ceil_div(int a, int b) { return (a + b - 1) / b; }

static WideGeom wide_geom(const MspiConvDesc* d) {
  WideGeom g;
  g.N = d->N; g.T = d->T; g.H = d->H; g.W = d->W; g.C = d->C;
  g.sN = d->sN; g.sT = d->sT; g.sH = d->sH; g.sW = d->sW;
  g.kT = d->kT; g.kH = d->kH; g.kW = d->kW; g.padT = d->padT; g.padH = d->padH; g.padW = d->padW;
  g.To = d->To; g.Ho = d->Ho; g.Wo = d->Wo; g.Cout = d->Cout;
  g.ldy = d->ldy;
  g.taps = d->kT * d->kH * d->kW;
  const long M = (long)d->N * d->To * d->Ho * d->Wo;
  // a 1 x 1 x 1 kernel over dense rows has no geometry: one line of M positions, so that a box is 128 rows of any map
  if (g.taps == 1 && !d->padT && !d->padH && !d->padW && d->sH == d->W * d->sW && d->sT == d->H * d->sH && d->sN == d->T * d->sT) {
    g.N = g.T = g.H = g.To = g.Ho = 1;
    g.W = g.Wo = (int)M;
    g.sH = g.sT = g.sN = M * g.sW;
  }
  g.WR = g.Wo < 8 ? g.Wo : 8;
  g.HR = g.Ho < 4 ? g.Ho : 4;
  g.TR = g.To < WW_ROWS / (g.WR * g.HR) ? g.To : WW_ROWS / (g.WR * g.HR);
  g.HR = g.Ho < WW_ROWS / (g.WR * g.TR) ? g.Ho : WW_ROWS / (g.WR * g.TR);
  g.WR = g.Wo < WW_ROWS / (g.TR * g.HR) ? g.Wo : WW_ROWS / (g.TR * g.HR);
  while ((g.TR + g.kT - 1) * (g.HR + g.kH - 1) * (g.WR + g.kW - 1) > WW_MAX_POS) {      // ends: 1 x 1 x 1 stages <= 27 positions
    if (g.WR >= g.HR && g.WR >= g.TR) g.WR = (g.WR + 1) / 2;
    else if (g.HR >= g.TR) g.HR = (g.HR + 1) / 2;
    else g.TR = (g.TR + 1) / 2;
  }
  g.BT = g.TR + g.kT - 1; g.BH = g.HR + g.kH - 1; g.BW = g.WR + g.kW - 1;
  g.P = g.BT * g.BH * g.BW;
  g.R = (g.TR * g.HR * g.WR + 7) / 8 * 8;
  g.nbT = ww_ceil_div(g.To, g.TR); g.nbH = ww_ceil_div(g.Ho, g.HR); g.nbW = ww_ceil_div(g.Wo, g.WR);
  g.NB = (long)g.N * g.nbT * g.nbH * g.nbW;
  g.bps = g.NB >= WW_BIG_BOXES ? WW_BPS_BIG : WW_BPS_SMALL;
  g.S = (int)((g.NB + g.bps - 1) / g.bps);
  g.CBi = g.C / 32; g.CBo = g.Cout / 32;
  g.K = g.taps * g.C;
  return g;
}

// ------------------------------------------------------------------------------------------------ BatchNorm on batch statistics
// Rows [M][C] channels-last, C = 4 CV.  A workgroup takes BN_ROWS rows: thread (rr, cv) walks rows rr, rr + RP, ... of channel
// vector cv, RP = 256 / CV; the RP partials of a channel are added through LDS in order.
constexpr int BN_T = 256;
constexpr int BN_ROWS = 512;

__host__ __device__ inline int bn_groups(long M) { return (int)((M + BN_ROWS - 1) / BN_ROWS); }

// element c of the sum over the RP row lanes of sh[rr * CV + cv]
__device__ __forceinline__ float bn_lane_sum(const float4* sh, int c, int CV, int RP) {
  float s = 0.f;
  for (int r = 0; r < RP; ++r) s += reinterpret_cast<const float*>(&sh[r * CV + (c >> 2)])[c & 3];
  return s;
}

// Group record: mean [C] then M2 [C] = sum (x - mean)^2 of the group's rows, from sums of d = x - shift with the group's
// first row as the shift: |shift - mean| is of the order of the deviation, so sum d^2 - (sum d)^2 / n does not cancel.
__global__ __launch_bounds__(BN_T) void bn_stats_kernel(const float* __restrict__ x, long ld, long M, int C, float* __restrict__ ws) {
  __shared__ float4 sh1[BN_T], sh2[BN_T];
  const int CV = C >> 2, RP = BN_T / CV;
  const int cv = threadIdx.x % CV, rr = threadIdx.x / CV;
  const long p0 = (long)blockIdx.x * BN_ROWS;
  const long p1 = p0 + BN_ROWS < M ? p0 + BN_ROWS : M;
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
  if (rr < RP) {
    const float4 sft = *reinterpret_cast<const float4*>(x + p0 * ld + cv * 4);
    for (long p = p0 + rr; p < p1; p += RP) {
      const float4 v = *reinterpret_cast<const float4*>(x + p * ld + cv * 4);
      const float dx = v.x - sft.x, dy = v.y - sft.y, dz = v.z - sft.z, dw = v.w - sft.w;
      s1.x += dx; s1.y += dy; s1.z += dz; s1.w += dw;
      s2.x = fmaf(dx, dx, s2.x); s2.y = fmaf(dy, dy, s2.y); s2.z = fmaf(dz, dz, s2.z); s2.w = fmaf(dw, dw, s2.w);
    }
  }
  sh1[threadIdx.x] = s1;
  sh2[threadIdx.x] = s2;
  __syncthreads();
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    const float n = (float)(p1 - p0);
    const float a = bn_lane_sum(sh1, c, CV, RP), b = bn_lane_sum(sh2, c, CV, RP);
    const float m2 = b - a * a / n;
    float* rec = ws + (long)blockIdx.x * 2 * C;
    rec[c] = x[p0 * ld + c] + a / n;
    rec[C + c] = relu_nan(m2);      // clamps rounding below 0; the NaN of a channel holding a NaN / Inf must stay one (common.h)
  }
}

// Chan's merge of the group records, left to right; one thread per channel.
__global__ __launch_bounds__(BN_T) void bn_stats_merge_kernel(const float* __restrict__ ws, int G, long M, int C, float eps,
                                                              float* __restrict__ mean, float* __restrict__ var,
                                                              float* __restrict__ rstd) {
  const int c = threadIdx.x;
  if (c >= C) return;
  float mu = ws[c], m2 = ws[C + c];
  long n = M < BN_ROWS ? M : BN_ROWS;
  for (int g = 1; g < G; ++g) {
    const long nb = g < G - 1 ? BN_ROWS : M - (long)(G - 1) * BN_ROWS;
    const float mb = ws[(long)g * 2 * C + c], m2b = ws[(long)g * 2 * C + C + c];
    const float delta = mb - mu, nt = (float)(n + nb);
    mu += delta * ((float)nb / nt);
    m2 += m2b + delta * delta * ((float)n * ((float)nb / nt));
    n += nb;
  }
  const float v = m2 / (float)M;
  mean[c] = mu;
  var[c] = v;
  rstd[c] = 1.f / sqrtf(v + eps);
}

template <bool RELU>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ y, long ldy, long total,
                                                       int CV) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;           // fewer than 2^31 vectors (host-checked)
  if (idx >= total) return;
  const unsigned ui = (unsigned)idx;
  const int cv = (int)(ui % (unsigned)CV);
  const long row = (long)(ui / (unsigned)CV);
  const float4 v = *reinterpret_cast<const float4*>(x + row * ldx + cv * 4);
  const float4 mu = *reinterpret_cast<const float4*>(mean + cv * 4), rs = *reinterpret_cast<const float4*>(rstd + cv * 4);
  const float4 ga = *reinterpret_cast<const float4*>(gamma + cv * 4), be = *reinterpret_cast<const float4*>(beta + cv * 4);
  float4 o;
  o.x = fmaf((v.x - mu.x) * rs.x, ga.x, be.x); o.y = fmaf((v.y - mu.y) * rs.y, ga.y, be.y);
  o.z = fmaf((v.z - mu.z) * rs.z, ga.z, be.z); o.w = fmaf((v.w - mu.w) * rs.w, ga.w, be.w);
  if (RELU) {
    o.x = relu_nan(o.x); o.y = relu_nan(o.y); o.z = relu_nan(o.z); o.w = relu_nan(o.w);      // NaN statistics stay visible (common.h)
  }
  *reinterpret_cast<float4*>(y + row * ldy + cv * 4) = o;
}

// Group record: sum dy [C] then sum dy x^ [C], dy masked by the forward's output (y > 0) when there was a ReLU.
template <bool RELU>
__global__ __launch_bounds__(BN_T) void bn_bwd_sums_kernel(const float* __restrict__ dy, long lddy, const float* __restrict__ x,
                                                           long ldx, const float* __restrict__ y, long ldy,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd, long M,
                                                           int C, float* __restrict__ ws) {
  __shared__ float4 sh1[BN_T], sh2[BN_T];
  const int CV = C >> 2, RP = BN_T / CV;
  const int cv = threadIdx.x % CV, rr = threadIdx.x / CV;
  const long p0 = (long)blockIdx.x * BN_ROWS;
  const long p1 = p0 + BN_ROWS < M ? p0 + BN_ROWS : M;
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
  if (rr < RP) {
    const float4 mu = *reinterpret_cast<const float4*>(mean + cv * 4), rs = *reinterpret_cast<const float4*>(rstd + cv * 4);
    for (long p = p0 + rr; p < p1; p += RP) {
      float4 g = *reinterpret_cast<const float4*>(dy + p * lddy + cv * 4);
      const float4 v = *reinterpret_cast<const float4*>(x + p * ldx + cv * 4);
      if (RELU) {
        const float4 o = *reinterpret_cast<const float4*>(y + p * ldy + cv * 4);
        g.x = o.x > 0.f ? g.x : 0.f; g.y = o.y > 0.f ? g.y : 0.f; g.z = o.z > 0.f ? g.z : 0.f; g.w = o.w > 0.f ? g.w : 0.f;
      }
      s1.x += g.x; s1.y += g.y; s1.z += g.z; s1.w += g.w;
      s2.x = fmaf(g.x, (v.x - mu.x) * rs.x, s2.x); s2.y = fmaf(g.y, (v.y - mu.y) * rs.y, s2.y);
      s2.z = fmaf(g.z, (v.z - mu.z) * rs.z, s2.z); s2.w = fmaf(g.w, (v.w - mu.w) * rs.w, s2.w);
    }
  }
  sh1[threadIdx.x] = s1;
  sh2[threadIdx.x] = s2;
  __syncthreads();
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    float* rec = ws + (long)blockIdx.x * 2 * C;
    rec[c] = bn_lane_sum(sh1, c, CV, RP);
    rec[C + c] = bn_lane_sum(sh2, c, CV, RP);
  }
}

// dbeta [C] and dgamma [C] from the group records; grid ceil(2 C / 64).
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ ws, int G, int C, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta) {
  __shared__ float part[4][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < 2 * C;
  const float r = rt_sum_records(ws + (live ? e : 0), 2L * C, G, live, part);
  if (threadIdx.x < 64 && live) {
    if (e < C) dbeta[e] = r;
    else dgamma[e - C] = r;
  }
}

template <bool RELU>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, long lddy, const float* __restrict__ x,
                                                           long ldx, const float* __restrict__ y, long ldy,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                           const float* __restrict__ dbeta, float* __restrict__ dx, long lddx,
                                                           long total, int CV, float invM) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;           // fewer than 2^31 vectors (host-checked)
  if (idx >= total) return;
  const unsigned ui = (unsigned)idx;
  const int cv = (int)(ui % (unsigned)CV);
  const long row = (long)(ui / (unsigned)CV);
  float4 g = *reinterpret_cast<const float4*>(dy + row * lddy + cv * 4);
  const float4 v = *reinterpret_cast<const float4*>(x + row * ldx + cv * 4);
  if (RELU) {
    const float4 o = *reinterpret_cast<const float4*>(y + row * ldy + cv * 4);
    g.x = o.x > 0.f ? g.x : 0.f; g.y = o.y > 0.f ? g.y : 0.f; g.z = o.z > 0.f ? g.z : 0.f; g.w = o.w > 0.f ? g.w : 0.f;
  }
  const float4 mu = *reinterpret_cast<const float4*>(mean + cv * 4), rs = *reinterpret_cast<const float4*>(rstd + cv * 4);
  const float4 ga = *reinterpret_cast<const float4*>(gamma + cv * 4);
  const float4 dg = *reinterpret_cast<const float4*>(dgamma + cv * 4), db = *reinterpret_cast<const float4*>(dbeta + cv * 4);
  float4 o;
  o.x = ga.x * rs.x * (g.x - db.x * invM - (v.x - mu.x) * rs.x * (dg.x * invM));
  o.y = ga.y * rs.y * (g.y - db.y * invM - (v.y - mu.y) * rs.y * (dg.y * invM));
  o.z = ga.z * rs.z * (g.z - db.z * invM - (v.z - mu.z) * rs.z * (dg.z * invM));
  o.w = ga.w * rs.w * (g.w - db.w * invM - (v.w - mu.w) * rs.w * (dg.w * invM));
  *reinterpret_cast<float4*>(dx + row * lddx + cv * 4) = o;
}

static const char* bn_refusal(int64_t M, int32_t C) {
  if (M == 1) return "M = 1: batch statistics need more than one value per channel";
  if (M <= 0) return "no rows";
  if (C < 4 || C > WW_MAX_CH || C % 4) return "C must be a multiple of 4, at most 192";
  if (M * (C / 4) >= (1L << 31)) return "2^31 or more channel vectors";
  return nullptr;
}

static bool bn_rows_ok(const void* p, int64_t ld, int32_t C) { return p && aligned16(p) && ld >= C && ld % 4 == 0; }

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_conv_wgrad_wide_supported(const MspiConvDesc* d) {
  const char* why = wide_refusal(d);
  if (why) set_error("mspi_conv_wgrad_wide: %s", why);
  return why ? 0 : 1;
}

extern "C" size_t mspi_conv_wgrad_wide_ws_bytes(const MspiConvDesc* d) {
  if (wide_refusal(d)) return 0;
  const WideGeom g = wide_geom(d);
  return (size_t)g.S * ww_record_floats(g.Cout, g.K) * sizeof(float);
}

extern "C" int mspi_conv_wgrad_wide_variant(const MspiConvDesc* d, const void* x, const void* dy) {
  const char* why = wide_refusal(d);
  if (!why && !(aligned16(x) && aligned16(dy))) why = "x and dy must be 16-byte aligned";
  if (why) {
    set_error("mspi_conv_wgrad_wide: %s", why);
    return -1;
  }
  return wide_geom(d).bps;
}

extern "C" int mspi_conv_wgrad_wide_fwd(const MspiConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                                        mspi_stream_t stream) {
  MSPI_REQUIRE(x && dy && dW && db && ws, "mspi_conv_wgrad_wide_fwd: null argument");
  if (mspi_conv_wgrad_wide_variant(d, x, dy) < 0) return MSPI_EINVAL;
  MSPI_REQUIRE(aligned16(ws) && aligned16(dW), "mspi_conv_wgrad_wide: dW and ws must be 16-byte aligned");
  const WideGeom g = wide_geom(d);
  const size_t lds = (size_t)(ww_x_floats(g.P) + g.R * 33) * sizeof(float);
  const dim3 grid(g.S, g.CBo * g.CBi), block(WW_T);
  hipStream_t st = (hipStream_t)stream;
  float* w = (float*)ws;
  if (g.taps == 1) hipLaunchKernelGGL((conv_wgrad_wide_kernel<1, true>), grid, block, lds, st, g, x, dy, w);
  else if (g.taps <= 4) hipLaunchKernelGGL((conv_wgrad_wide_kernel<1, false>), grid, block, lds, st, g, x, dy, w);
  else if (g.taps <= 12) hipLaunchKernelGGL((conv_wgrad_wide_kernel<3, false>), grid, block, lds, st, g, x, dy, w);
  else hipLaunchKernelGGL((conv_wgrad_wide_kernel<7, false>), grid, block, lds, st, g, x, dy, w);
  const int nW = g.Cout * g.K, n = nW + g.Cout;
  hipLaunchKernelGGL(conv_wgrad_wide_reduce_kernel, dim3((n + 63) / 64), dim3(256), 0, st, (const float*)ws, g.S, nW, n, dW, db);
  return check_launch("mspi_conv_wgrad_wide_fwd");
}

extern "C" size_t mspi_bn_ws_bytes(int64_t M, int32_t C) {
  if (bn_refusal(M, C)) return 0;
  return (size_t)bn_groups(M) * 2 * C * sizeof(float);
}

extern "C" int mspi_bn_stats(const float* x, int64_t ldx, int64_t M, int32_t C, float eps, float* mean, float* var, float* rstd,
                             void* ws, mspi_stream_t stream) {
  const char* why = bn_refusal(M, C);
  MSPI_REQUIRE(!why, "mspi_bn_stats: %s", why);
  MSPI_REQUIRE(mean && var && rstd && ws && eps >= 0.f, "mspi_bn_stats: null argument or negative eps");
  MSPI_REQUIRE(bn_rows_ok(x, ldx, C), "mspi_bn_stats: x must be 16-byte aligned, ldx a multiple of 4, >= C");
  const int G = bn_groups(M);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_stats_kernel, dim3(G), dim3(BN_T), 0, st, x, (long)ldx, (long)M, C, (float*)ws);
  hipLaunchKernelGGL(bn_stats_merge_kernel, dim3(1), dim3(BN_T), 0, st, (const float*)ws, G, (long)M, C, eps, mean, var, rstd);
  return check_launch("mspi_bn_stats");
}

extern "C" int mspi_bn_apply(const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                             const float* beta, float* y, int64_t ldy, int64_t M, int32_t C, int32_t act, mspi_stream_t stream) {
  const char* why = bn_refusal(M, C);
  MSPI_REQUIRE(!why, "mspi_bn_apply: %s", why);
  MSPI_REQUIRE(act == MSPI_ACT_NONE || act == MSPI_ACT_RELU, "mspi_bn_apply: act must be MSPI_ACT_NONE or MSPI_ACT_RELU");
  MSPI_REQUIRE(mean && rstd && gamma && beta && aligned16(mean) && aligned16(rstd) && aligned16(gamma) && aligned16(beta),
               "mspi_bn_apply: mean, rstd, gamma and beta must be 16-byte aligned");
  MSPI_REQUIRE(bn_rows_ok(x, ldx, C) && bn_rows_ok(y, ldy, C),
               "mspi_bn_apply: x and y must be 16-byte aligned, their row strides multiples of 4, >= C");
  const long total = (long)M * (C / 4);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (act == MSPI_ACT_RELU)
    hipLaunchKernelGGL((bn_apply_kernel<true>), grid, block, 0, st, x, (long)ldx, mean, rstd, gamma, beta, y, (long)ldy, total, C / 4);
  else
    hipLaunchKernelGGL((bn_apply_kernel<false>), grid, block, 0, st, x, (long)ldx, mean, rstd, gamma, beta, y, (long)ldy, total, C / 4);
  return check_launch("mspi_bn_apply");
}

extern "C" int mspi_bn_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* y, int64_t ldy,
                           const float* mean, const float* rstd, const float* gamma, float* dx, int64_t lddx, float* dgamma,
                           float* dbeta, void* ws, int64_t M, int32_t C, mspi_stream_t stream) {
  const char* why = bn_refusal(M, C);
  MSPI_REQUIRE(!why, "mspi_bn_bwd: %s", why);
  MSPI_REQUIRE(mean && rstd && gamma && dgamma && dbeta && ws && aligned16(mean) && aligned16(rstd) && aligned16(gamma) &&
                   aligned16(dgamma) && aligned16(dbeta),
               "mspi_bn_bwd: mean, rstd, gamma, dgamma and dbeta must be 16-byte aligned, ws not null");
  MSPI_REQUIRE(bn_rows_ok(dy, lddy, C) && bn_rows_ok(x, ldx, C) && bn_rows_ok(dx, lddx, C) && (!y || bn_rows_ok(y, ldy, C)),
               "mspi_bn_bwd: dy, x, y and dx must be 16-byte aligned, their row strides multiples of 4, >= C");
  const int G = bn_groups(M);
  const long total = (long)M * (C / 4);
  const dim3 grid((unsigned)((total + 255) / 256));
  const float invM = 1.f / (float)M;
  hipStream_t st = (hipStream_t)stream;
  float* w = (float*)ws;
  if (y) {
    hipLaunchKernelGGL((bn_bwd_sums_kernel<true>), dim3(G), dim3(BN_T), 0, st, dy, (long)lddy, x, (long)ldx, y, (long)ldy, mean, rstd,
                       (long)M, C, w);
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((2 * C + 63) / 64), dim3(256), 0, st, (const float*)w, G, C, dgamma, dbeta);
    hipLaunchKernelGGL((bn_bwd_apply_kernel<true>), grid, dim3(256), 0, st, dy, (long)lddy, x, (long)ldx, y, (long)ldy, mean, rstd,
                       gamma, (const float*)dgamma, (const float*)dbeta, dx, (long)lddx, total, C / 4, invM);
  } else {
    hipLaunchKernelGGL((bn_bwd_sums_kernel<false>), dim3(G), dim3(BN_T), 0, st, dy, (long)lddy, x, (long)ldx, y, (long)ldy, mean, rstd,
                       (long)M, C, w);
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((2 * C + 63) / 64), dim3(256), 0, st, (const float*)w, G, C, dgamma, dbeta);
    hipLaunchKernelGGL((bn_bwd_apply_kernel<false>), grid, dim3(256), 0, st, dy, (long)lddy, x, (long)ldx, y, (long)ldy, mean, rstd,
                       gamma, (const float*)dgamma, (const float*)dbeta, dx, (long)lddx, total, C / 4, invM);
  }
  return check_launch("mspi_bn_bwd");
}
