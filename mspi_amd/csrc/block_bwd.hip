// Backward of the laterals' ConvNextBlock (model/model_utils.py:306-354): the three pieces no other file has.  Entry points
// (include/mspi_block_train_hip.h), all fp32:
//   mspi_gelu_bwd        g = GELU(z) again and dz = dg (Phi(z) + z phi(z))                  one element-wise pass
//   mspi_layernorm_bwd   dx per row, dgamma / dbeta over the rows, mean and rstd recomputed    one pass + the ordered add
//   mspi_dwconv_wgrad    dW [taps][C] and db [C] of the (7,1,1) and (1,7,7) depthwise convs   one pass + the ordered add
// Every sum that crosses a workgroup goes through the caller's workspace as one record per workgroup, which a second launch
// adds in a fixed order (rt_sum_records, common.h): bitwise repeatable.  Nothing here allocates or synchronises.
#include "common.h"
#include "../../include/mspi_block_train_hip.h"

namespace mspi {

// Sum of the S records [n] in ws, element e to a[e] (e < nA) or b[e - nA]; grid ceil(n / 64).
__global__ __launch_bounds__(256) void block_reduce_kernel(const float* __restrict__ ws, int S, int n, int nA, float* __restrict__ a,
                                                           float* __restrict__ b) {
  __shared__ float part[4][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < n;
  const float r = rt_sum_records(ws + (live ? e : 0), n, S, live, part);
  if (threadIdx.x < 64 && live) {
    if (e < nA) a[e] = r;
    else b[e - nA] = r;
  }
}

// ------------------------------------------------------------------------------------------------ GELU
// gelu_erf's pieces (common.h) once more for the derivative: q = 0.5 erfc(|u| / sqrt 2), Phi = 1 - q or q, phi = e / sqrt(2 pi).
__device__ __forceinline__ float gelu_erf_grad(float u) {
  const float au = fabsf(u);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f * 0.70710678118654752440f, au, 1.f));
  const float e = __builtin_amdgcn_exp2f(u * u * (-0.5f * 1.4426950408889634f));
  float y = fmaf(0.5f * 1.061405429f, t, 0.5f * -1.453152027f);
  y = fmaf(y, t, 0.5f * 1.421413741f);
  y = fmaf(y, t, 0.5f * -0.284496736f);
  y = fmaf(y, t, 0.5f * 0.254829592f);
  const float q = y * t * e;
  const float cdf = u >= 0.f ? 1.f - q : q;
  return fmaf(u, e * 0.39894228040143267794f, cdf);
}

// A workgroup takes RB consecutive rows, its threads their RB * CV vectors in order.  g may be z and dz may be dg: a thread
// stores only what it has loaded.
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float* z, long ldz, const float* dg, long lddg, float* g, long ldg,
                                                       float* dz, long lddz, long M, int CV, int RB) {
  const long r0 = (long)blockIdx.x * RB;
  const int n = RB * CV;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int rr = i / CV, cv = i - rr * CV;
    const long row = r0 + rr;
    if (row >= M) break;
    const float4 u = *reinterpret_cast<const float4*>(z + row * ldz + cv * 4);
    const float4 d = *reinterpret_cast<const float4*>(dg + row * lddg + cv * 4);
    if (g) *reinterpret_cast<float4*>(g + row * ldg + cv * 4) = make_float4(gelu_erf(u.x), gelu_erf(u.y), gelu_erf(u.z), gelu_erf(u.w));
    *reinterpret_cast<float4*>(dz + row * lddz + cv * 4) =
        make_float4(d.x * gelu_erf_grad(u.x), d.y * gelu_erf_grad(u.y), d.z * gelu_erf_grad(u.z), d.w * gelu_erf_grad(u.w));
  }
}

// ------------------------------------------------------------------------------------------------ LayerNorm
// The lanes of layernorm_kernel<16, VPT> (rowops.hip): 16 lanes own a row, lane `sub` its vectors sub, sub + 16, ...; mean and
// rstd by the same two passes and the same xor tree, so x^ has the forward's bits.  A workgroup walks LNB_ROWS rows, 16 at a
// time, and keeps its lanes' shares of dgamma and dbeta in registers; they meet across the four row slots of a wave by two
// shuffles, across the four waves through LDS in wave order, and leave as one record [dbeta | dgamma].
constexpr int LNB_ROWS = 256;
constexpr int LNB_MAXC = 256;

__host__ __device__ inline int lnb_groups(long M) { return (int)((M + LNB_ROWS - 1) / LNB_ROWS); }

__device__ __forceinline__ float row16_sum(float s) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

template <int VPT>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, long ldx, const float* dy, long lddy,
                                                            const float* __restrict__ gamma, float eps, float* dx, long lddx,
                                                            float* __restrict__ ws, long M, int C) {
  __shared__ float4 sh[4][2][16 * VPT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 15;
  const int nv = C >> 2;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 gam[VPT], sg[VPT], sb[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = sub + 16 * j;
    gam[j] = *reinterpret_cast<const float4*>(gamma + (i < nv ? i : 0) * 4);
    sg[j] = zero;
    sb[j] = zero;
  }
  const long base = (long)blockIdx.x * LNB_ROWS;
  for (int pass = 0; pass < LNB_ROWS / 16; ++pass) {
    if (base + pass * 16 >= M) break;                 // uniform over the workgroup
    const long row = base + pass * 16 + wave * 4 + (lane >> 4);
    const bool rok = row < M;                         // dead rows stay in the shuffles on row 0's data and add nothing
    const long rr = rok ? row : 0;
    float4 v[VPT], d[VPT];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int i = sub + 16 * j;
      const float4 t = *reinterpret_cast<const float4*>(x + rr * ldx + (i < nv ? i : 0) * 4);
      const float4 u = *reinterpret_cast<const float4*>(dy + rr * lddy + (i < nv ? i : 0) * 4);
      v[j] = i < nv ? t : zero;
      d[j] = i < nv ? u : zero;
      s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
    const float mean = row16_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      if (sub + 16 * j < nv) {
        const float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, e = v[j].w - mean;
        q += (a * a + b * b) + (c * c + e * e);
      }
    }
    const float rstd = rsqrtf(row16_sum(q) / (float)C + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      if (sub + 16 * j < nv) {
        v[j] = make_float4((v[j].x - mean) * rstd, (v[j].y - mean) * rstd, (v[j].z - mean) * rstd, (v[j].w - mean) * rstd);   // x^
        const float4 a = make_float4(d[j].x * gam[j].x, d[j].y * gam[j].y, d[j].z * gam[j].z, d[j].w * gam[j].w);
        s1 += (a.x + a.y) + (a.z + a.w);
        s2 += (a.x * v[j].x + a.y * v[j].y) + (a.z * v[j].z + a.w * v[j].w);
      }
    }
    const float m1 = row16_sum(s1) / (float)C, m2 = row16_sum(s2) / (float)C;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int i = sub + 16 * j;
      if (rok && i < nv) {
        float4 o;
        o.x = rstd * (d[j].x * gam[j].x - m1 - v[j].x * m2);
        o.y = rstd * (d[j].y * gam[j].y - m1 - v[j].y * m2);
        o.z = rstd * (d[j].z * gam[j].z - m1 - v[j].z * m2);
        o.w = rstd * (d[j].w * gam[j].w - m1 - v[j].w * m2);
        *reinterpret_cast<float4*>(dx + row * lddx + i * 4) = o;
        sg[j].x = fmaf(d[j].x, v[j].x, sg[j].x); sg[j].y = fmaf(d[j].y, v[j].y, sg[j].y);
        sg[j].z = fmaf(d[j].z, v[j].z, sg[j].z); sg[j].w = fmaf(d[j].w, v[j].w, sg[j].w);
        sb[j].x += d[j].x; sb[j].y += d[j].y; sb[j].z += d[j].z; sb[j].w += d[j].w;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      sg[j].x += __shfl_xor(sg[j].x, o, 64); sg[j].y += __shfl_xor(sg[j].y, o, 64);
      sg[j].z += __shfl_xor(sg[j].z, o, 64); sg[j].w += __shfl_xor(sg[j].w, o, 64);
      sb[j].x += __shfl_xor(sb[j].x, o, 64); sb[j].y += __shfl_xor(sb[j].y, o, 64);
      sb[j].z += __shfl_xor(sb[j].z, o, 64); sb[j].w += __shfl_xor(sb[j].w, o, 64);
    }
    if (lane < 16) {
      sh[wave][0][sub + 16 * j] = sb[j];
      sh[wave][1][sub + 16 * j] = sg[j];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * nv) {
    const int which = (int)threadIdx.x / nv, i = (int)threadIdx.x - which * nv;
    const float4 a = sh[0][which][i], b = sh[1][which][i], c = sh[2][which][i], e = sh[3][which][i];
    float* rec = ws + (long)blockIdx.x * 2 * C + which * C + i * 4;
    *reinterpret_cast<float4*>(rec) = make_float4((a.x + b.x) + (c.x + e.x), (a.y + b.y) + (c.y + e.y), (a.z + b.z) + (c.z + e.z),
                                                  (a.w + b.w) + (c.w + e.w));
  }
}

static const char* lnb_refusal(int64_t M, int32_t C) {
  if (M <= 0) return "no rows";
  if (M >= (1L << 31)) return "2^31 or more rows";
  if (C < 4 || C > LNB_MAXC || C % 4) return "C must be a multiple of 4, at most 256";
  return nullptr;
}

static bool rows_ok(const void* p, int64_t ld, int32_t C) { return p && aligned16(p) && ld >= C && ld % 4 == 0; }

// ------------------------------------------------------------------------------------------------ depthwise weight gradient
// One kernel for both shapes.  A LINE is what the 7 taps slide along: a row of W positions under (1,7,7), the T frames of one
// spatial position under (7,1,1).  Thread (q, r) owns channel quad q and
//   KH = 7: kernel row r -- for output line h it reads input line h + r - 3 (zeros outside the frame) and keeps dW[r][0..6];
//   KH = 1: line slot r  -- it takes lines r, r + 7, ... of the band and keeps dW[0..6]; the 7 slots meet through LDS in order.
// Along a line it keeps x[w - 3 .. w + 3] in a register window that rotates by one slot per step (the loop is unrolled by 7, so
// every slot index is a constant), loads one x and one dy vector per step and does 7 FMAs on four channels.  A workgroup owns
// a band of lines of one frame (KH = 7) or sample (KH = 1) and QG channel quads, and writes its part of the band's record
// [taps + 1][C]: dW, then db.
constexpr int DWG_BAND7 = 4;         // output rows per workgroup, (1,7,7)
constexpr int DWG_BAND1 = 56;        // positions per workgroup, (7,1,1): 8 per line slot
constexpr int DWG_MAXQ = 36;         // channel quads per workgroup: 7 x 36 = 252 threads

struct DwWgArgs {
  const float* x;
  const float* dy;
  float* ws;
  long xo, xl, xs;      // x: floats between frames | samples, between lines, between steps along a line
  long yo, yl, ys;      // dy likewise
  int nLines, L, C, band, nBands;
};

template <int KH>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const DwWgArgs a) {
  const int q = threadIdx.x, r = threadIdx.y, QG = blockDim.x;
  const int cq = blockIdx.y * QG + q;
  const bool live = cq * 4 < a.C;
  const int outer = blockIdx.x / a.nBands, bandi = blockIdx.x - outer * a.nBands;
  const int l0 = bandi * a.band, l1 = l0 + a.band < a.nLines ? l0 + a.band : a.nLines;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc[7], db = zero;
#pragma unroll
  for (int k = 0; k < 7; ++k) acc[k] = zero;
  if (live) {
    const float* xb = a.x + (long)outer * a.xo + cq * 4;
    const float* yb = a.dy + (long)outer * a.yo + cq * 4;
    const int L = a.L;
    for (int l = KH == 7 ? l0 : l0 + r; l < l1; l += KH == 7 ? 1 : 7) {
      const int xi = KH == 7 ? l + r - 3 : l;
      const bool xin = xi >= 0 && xi < a.nLines;
      const float* xp = xb + (long)(xin ? xi : 0) * a.xl;
      const float* dp = yb + (long)l * a.yl;
      float4 win[7];
#pragma unroll
      for (int k = 0; k < 6; ++k) win[k] = (xin && k >= 3 && k - 3 < L) ? *reinterpret_cast<const float4*>(xp + (long)(k - 3) * a.xs) : zero;
      for (int w0 = 0; w0 < L; w0 += 7) {
#pragma unroll
        for (int s = 0; s < 7; ++s) {
          const int w = w0 + s;
          if (w < L) {
            win[(s + 6) % 7] = (xin && w + 3 < L) ? *reinterpret_cast<const float4*>(xp + (long)(w + 3) * a.xs) : zero;
            const float4 d = *reinterpret_cast<const float4*>(dp + (long)w * a.ys);
#pragma unroll
            for (int k = 0; k < 7; ++k) fma4(acc[k], d, win[(s + k) % 7]);      // slot (s + k) % 7 holds x[w + k - 3]
            if (KH == 1 || r == 3) { db.x += d.x; db.y += d.y; db.z += d.z; db.w += d.w; }
          }
        }
      }
    }
  }
  float* rec = a.ws + (long)blockIdx.x * (KH * 7 + 1) * a.C + cq * 4;
  if constexpr (KH == 7) {
    if (live) {
#pragma unroll
      for (int k = 0; k < 7; ++k) *reinterpret_cast<float4*>(rec + (long)(r * 7 + k) * a.C) = acc[k];
      if (r == 3) *reinterpret_cast<float4*>(rec + (long)49 * a.C) = db;
    }
  } else {
    __shared__ float4 sh[7][8][DWG_MAXQ];
#pragma unroll
    for (int k = 0; k < 7; ++k) sh[r][k][q] = acc[k];
    sh[r][7][q] = db;
    __syncthreads();
    if (live) {
      for (int k = r; k < 8; k += 7) {         // thread (q, r) adds tap r over the slots in order; r = 0 also db
        float4 s = sh[0][k][q];
        for (int t = 1; t < 7; ++t) {
          const float4 v = sh[t][k][q];
          s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<float4*>(rec + (long)k * a.C) = s;
      }
    }
  }
}

struct DwWgGeom {
  int KH, QG, groups, outer, nLines, L, band, nBands, taps;
  long xo, xl, xs, yo, yl, ys;
};

static const char* dwg_refusal(const MspiDwConvDesc* d, DwWgGeom& g) {
  if (!d) return "null descriptor";
  if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return "bad extent";
  if (d->C > 4096) return "more than 4096 channels";
  if (d->C % 4 || d->ldx % 4 || d->ldy % 4 || d->ldx < d->C || d->ldy < d->C) return "C and the row strides must be multiples of 4, ld >= C";
  if (d->strT != 1 || d->strH != 1 || d->strW != 1) return "stride must be 1";
  const bool kt = d->kT == 7 && d->kH == 1 && d->kW == 1 && d->padT == 3 && d->padH == 0 && d->padW == 0;
  const bool ks = d->kT == 1 && d->kH == 7 && d->kW == 7 && d->padT == 0 && d->padH == 3 && d->padW == 3;
  if (!kt && !ks) return "kernel must be (7,1,1) with padding (3,0,0) or (1,7,7) with padding (0,3,3)";
  if (d->To != d->T || d->Ho != d->H || d->Wo != d->W) return "the output extent must be the input's (\"same\" padding)";
  const long hw = (long)d->H * d->W, rows = (long)d->N * d->T * hw;
  if (rows >= (1L << 31)) return "2^31 or more rows";
  const int CV = d->C / 4;
  g.groups = (CV + DWG_MAXQ - 1) / DWG_MAXQ;
  g.QG = (CV + g.groups - 1) / g.groups;
  if (ks) {
    g.KH = 7; g.taps = 49; g.outer = d->N * d->T; g.nLines = d->H; g.L = d->W; g.band = DWG_BAND7;
    g.xo = hw * d->ldx; g.xl = (long)d->W * d->ldx; g.xs = d->ldx;
    g.yo = hw * d->ldy; g.yl = (long)d->W * d->ldy; g.ys = d->ldy;
  } else {
    if (hw >= (1L << 31)) return "2^31 or more rows";
    g.KH = 1; g.taps = 7; g.outer = d->N; g.nLines = (int)hw; g.L = d->T; g.band = DWG_BAND1;
    g.xo = (long)d->T * hw * d->ldx; g.xl = d->ldx; g.xs = hw * d->ldx;
    g.yo = (long)d->T * hw * d->ldy; g.yl = d->ldy; g.ys = hw * d->ldy;
  }
  g.nBands = (g.nLines + g.band - 1) / g.band;
  if ((long)g.outer * g.nBands >= (1L << 31)) return "2^31 or more workgroups";
  return nullptr;
}

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_gelu_bwd(const float* z, int64_t ldz, const float* dg, int64_t lddg, float* g, int64_t ldg, float* dz,
                             int64_t lddz, int64_t M, int32_t C, mspi_stream_t stream) {
  MSPI_REQUIRE(z && dg && dz, "mspi_gelu_bwd: null argument (only g may be NULL)");
  MSPI_REQUIRE(M > 0 && C > 0, "mspi_gelu_bwd: bad extent");
  MSPI_REQUIRE(M < (1L << 31), "mspi_gelu_bwd: 2^31 or more rows");
  MSPI_REQUIRE((C & 3) == 0 && rows_ok(z, ldz, C) && rows_ok(dg, lddg, C) && rows_ok(dz, lddz, C) && (!g || rows_ok(g, ldg, C)),
               "mspi_gelu_bwd: C/ld must be multiples of 4 with ld >= C, pointers 16-B aligned");
  const int CV = C / 4;
  int RB = 2048 / CV;                   // about 8 vectors a thread
  RB = RB < 1 ? 1 : (RB > 256 ? 256 : RB);
  const long blocks = (M + RB - 1) / RB;
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, (long)ldz, dg, (long)lddg, g,
                     (long)ldg, dz, (long)lddz, (long)M, CV, RB);
  return check_launch("mspi_gelu_bwd");
}

extern "C" size_t mspi_layernorm_bwd_ws_bytes(int64_t M, int32_t C) {
  if (lnb_refusal(M, C)) return 0;
  return (size_t)lnb_groups(M) * 2 * C * sizeof(float);
}

extern "C" int mspi_layernorm_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* gamma, float eps,
                                  float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws, int64_t M, int32_t C,
                                  mspi_stream_t stream) {
  MSPI_REQUIRE(x && dy && gamma && dx && dgamma && dbeta && ws, "mspi_layernorm_bwd: null argument");
  const char* why = lnb_refusal(M, C);
  MSPI_REQUIRE(!why, "mspi_layernorm_bwd: %s", why);
  MSPI_REQUIRE(eps >= 0.f, "mspi_layernorm_bwd: negative eps");
  MSPI_REQUIRE(rows_ok(x, ldx, C) && rows_ok(dy, lddy, C) && rows_ok(dx, lddx, C),
               "mspi_layernorm_bwd: x, dy and dx must be 16-byte aligned, their row strides multiples of 4, >= C");
  MSPI_REQUIRE(aligned16(gamma) && aligned16(ws), "mspi_layernorm_bwd: gamma and ws must be 16-byte aligned");
  const int G = lnb_groups(M), nv = C / 4;
  hipStream_t st = (hipStream_t)stream;
  float* w = (float*)ws;
#define MSPI_LNB(VPT)                                                                                                             \
  hipLaunchKernelGGL((layernorm_bwd_kernel<VPT>), dim3(G), dim3(256), 0, st, x, (long)ldx, dy, (long)lddy, gamma, eps, dx, (long)lddx, \
                     w, (long)M, C)
  if (nv <= 16) MSPI_LNB(1);            // the row widths of layernorm_kernel<16, VPT> (ln_select, rowops.hip)
  else if (nv <= 32) MSPI_LNB(2);
  else MSPI_LNB(4);
#undef MSPI_LNB
  hipLaunchKernelGGL(block_reduce_kernel, dim3((2 * C + 63) / 64), dim3(256), 0, st, (const float*)w, G, 2 * C, C, dbeta, dgamma);
  return check_launch("mspi_layernorm_bwd");
}

extern "C" int mspi_dwconv_wgrad_supported(const MspiDwConvDesc* d) {
  DwWgGeom g;
  const char* why = dwg_refusal(d, g);
  if (why) set_error("mspi_dwconv_wgrad: %s", why);
  return why ? 0 : 1;
}

extern "C" size_t mspi_dwconv_wgrad_ws_bytes(const MspiDwConvDesc* d) {
  DwWgGeom g;
  if (dwg_refusal(d, g)) return 0;
  return (size_t)g.outer * g.nBands * (g.taps + 1) * d->C * sizeof(float);
}

extern "C" int mspi_dwconv_wgrad(const MspiDwConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                                 mspi_stream_t stream) {
  DwWgGeom g;
  const char* why = dwg_refusal(d, g);
  MSPI_REQUIRE(!why, "mspi_dwconv_wgrad: %s", why);
  MSPI_REQUIRE(x && dy && dW && db && ws, "mspi_dwconv_wgrad: null argument");
  MSPI_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(ws), "mspi_dwconv_wgrad: x, dy and ws must be 16-byte aligned");
  DwWgArgs a;
  a.x = x; a.dy = dy; a.ws = (float*)ws;
  a.xo = g.xo; a.xl = g.xl; a.xs = g.xs; a.yo = g.yo; a.yl = g.yl; a.ys = g.ys;
  a.nLines = g.nLines; a.L = g.L; a.C = d->C; a.band = g.band; a.nBands = g.nBands;
  const int S = g.outer * g.nBands, n = (g.taps + 1) * d->C;
  const dim3 grid((unsigned)S, (unsigned)g.groups), block(g.QG, 7);
  hipStream_t st = (hipStream_t)stream;
  if (g.KH == 7) hipLaunchKernelGGL((dwconv_wgrad_kernel<7>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((dwconv_wgrad_kernel<1>), grid, block, 0, st, a);
  hipLaunchKernelGGL(block_reduce_kernel, dim3((n + 63) / 64), dim3(256), 0, st, (const float*)ws, S, n, g.taps * d->C, dW, db);
  return check_launch("mspi_dwconv_wgrad");
}
