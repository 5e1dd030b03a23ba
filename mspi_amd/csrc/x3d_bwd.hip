// Backward of one stride-1 X3D residual block on batch statistics (SlowFast/resnet_helper.py:213-360, 490-616): the pieces no
// other file has.  Entry points (include/mspi_x3d_train_hip.h), all fp32:
//   mspi_dwconv3_wgrad     dW [C][27] (and db) of the depthwise (3,3,3) conv                  one pass + the ordered add
//   mspi_bn_gate_act_fwd   y = act(res + gate bn(x)), ReLU | Swish | none                     one element-wise pass
//   mspi_gate_swish_bwd    dv and dgate of s = swish(gate bn(v0)), everything recomputed      one pass + the ordered add
//   mspi_se_train_fwd      p, h, gate of the squeeze-excite MLP on [N][C] rows                one launch, a workgroup a sample
//   mspi_se_train_bwd      dW1, db1, dW2, db2, dp of it, the samples in index order           two launches
//   mspi_relu_mask_add     dx += (y > 0 ? g : 0)                                              one element-wise pass
// Every sum that crosses a workgroup goes through the caller's workspace as records, which a second launch adds in a fixed
// order (rt_sum_records, common.h): bitwise repeatable, no float read-modify-write anywhere.  Nothing here allocates or
// synchronises.
#include "common.h"
#include "../../include/mspi_x3d_train_hip.h"

namespace mspi {

constexpr int X3B_MAXC = 4096;

static bool x3b_rows_ok(const void* p, int64_t ld, int32_t C) { return p && aligned16(p) && ld >= C && ld % 4 == 0; }

// ------------------------------------------------------------------------------------------------ depthwise (3,3,3) weight gradient
// The plan of dwconv_wgrad_kernel<7> (block_bwd.hip) on short lines: thread (q, r) owns channel quad q and the (kt, kh) pair
// r = 3 kt + kh.  For output line (n, t, h) it reads input line (n, t + kt - 1, h + kh - 1), zeros outside the frame, keeps
// x[w - 1 .. w + 1] in a window of three named registers whose roles rotate by one per step (the loop is written out three steps
// at a time), loads one x and one dy vector per step and does 3 FMAs on four channels.  A workgroup owns a band of consecutive
// lines and QG channel quads and writes its part of the band's record [28][C]: the taps kt, kh, kw in that order, then db.
constexpr int DW3_MAXQ = 28;         // channel quads per workgroup: 9 x 28 = 252 threads
constexpr int DW3_RECORDS = 256;     // the band rule aims at this many records (mspi_x3d_train_hip.h)

struct Dw3Args {
  const float* x;
  const float* dy;
  float* ws;
  long ldx, ldy;
  int T, H, W, C, nLines, band;
};

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__global__ __launch_bounds__(256) void dwconv3_wgrad_kernel(const Dw3Args a) {
  const int q = threadIdx.x, r = threadIdx.y, QG = blockDim.x;
  const int cq = blockIdx.y * QG + q;
  const bool live = cq * 4 < a.C;
  const int kt = r / 3, kh = r - kt * 3;
  const int l0 = blockIdx.x * a.band, l1 = l0 + a.band < a.nLines ? l0 + a.band : a.nLines;
  float4 acc0 = f4zero(), acc1 = f4zero(), acc2 = f4zero(), db = f4zero();
  if (live) {
    const int W = a.W;
    for (int l = l0; l < l1; ++l) {
      const int h = l % a.H, nt = l / a.H, t = nt % a.T;
      const int ti = t + kt - 1, hi = h + kh - 1;
      const bool xin = ti >= 0 && ti < a.T && hi >= 0 && hi < a.H;
      const long xl = xin ? (long)l + (long)(kt - 1) * a.H + (kh - 1) : 0;            // the input line's number
      const float* xp = a.x + xl * W * a.ldx + cq * 4;
      const float* dp = a.dy + (long)l * W * a.ldy + cq * 4;
      float4 w0 = f4zero(), w1 = xin ? *reinterpret_cast<const float4*>(xp) : f4zero(), w2 = f4zero();
      // one step at position POS = w: LO holds x[w - 1], MID x[w], and HI takes x[w + 1]
#define MSPI_DW3_STEP(POS, LO, MID, HI)                                                                          \
  if ((POS) < W) {                                                                                               \
    HI = (xin && (POS) + 1 < W) ? *reinterpret_cast<const float4*>(xp + (long)((POS) + 1) * a.ldx) : f4zero();         \
    const float4 d = *reinterpret_cast<const float4*>(dp + (long)(POS) * a.ldy);                                 \
    fma4(acc0, d, LO);                                                                                         \
    fma4(acc1, d, MID);                                                                                        \
    fma4(acc2, d, HI);                                                                                         \
    if (r == 4) { db.x += d.x; db.y += d.y; db.z += d.z; db.w += d.w; }                                        \
  }
      for (int w = 0; w < W; w += 3) {
        MSPI_DW3_STEP(w, w0, w1, w2)
        MSPI_DW3_STEP(w + 1, w1, w2, w0)
        MSPI_DW3_STEP(w + 2, w2, w0, w1)
      }
#undef MSPI_DW3_STEP
    }
    float* rec = a.ws + (long)blockIdx.x * 28 * a.C + cq * 4;
    *reinterpret_cast<float4*>(rec + (long)(r * 3) * a.C) = acc0;
    *reinterpret_cast<float4*>(rec + (long)(r * 3 + 1) * a.C) = acc1;
    *reinterpret_cast<float4*>(rec + (long)(r * 3 + 2) * a.C) = acc2;
    if (r == 4) *reinterpret_cast<float4*>(rec + (long)27 * a.C) = db;
  }
}

// Sum of the S records [28][C] in record order: element e = tap C + c to dW[c][tap] (tap < 27) or db[c]; grid ceil(n / 64),
// n = 27 C without db, 28 C with it.
__global__ __launch_bounds__(256) void dwconv3_reduce_kernel(const float* __restrict__ ws, int S, int n, int C, float* __restrict__ dW,
                                                             float* __restrict__ db) {
  __shared__ float part[4][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < n;
  const float r = rt_sum_records(ws + (live ? e : 0), (long)28 * C, S, live, part);
  if (threadIdx.x < 64 && live) {
    const int tap = e / C, c = e - tap * C;
    if (tap < 27) dW[(long)c * 27 + tap] = r;
    else db[c] = r;
  }
}

struct Dw3Geom {
  int groups, QG, nLines, band, nBands;
};

static const char* dw3_refusal(const MspiDwConvDesc* d, Dw3Geom& g) {
  if (!d) return "null descriptor";
  if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return "bad extent";
  if (d->C > X3B_MAXC) return "more than 4096 channels";
  if (d->C % 4 || d->ldx % 4 || d->ldy % 4 || d->ldx < d->C || d->ldy < d->C) return "C and the row strides must be multiples of 4, ld >= C";
  if (d->strT != 1 || d->strH != 1 || d->strW != 1) return "stride must be 1";
  if (d->kT != 3 || d->kH != 3 || d->kW != 3 || d->padT != 1 || d->padH != 1 || d->padW != 1) return "kernel must be (3,3,3) with padding (1,1,1)";
  if (d->To != d->T || d->Ho != d->H || d->Wo != d->W) return "the output extent must be the input's (\"same\" padding)";
  const long lines = (long)d->N * d->T * d->H;
  if (lines * d->W >= (1L << 31)) return "2^31 or more rows";
  const int CV = d->C / 4;
  g.groups = (CV + DW3_MAXQ - 1) / DW3_MAXQ;
  g.QG = (CV + g.groups - 1) / g.groups;
  g.nLines = (int)lines;
  g.band = (int)((lines + DW3_RECORDS - 1) / DW3_RECORDS);
  g.nBands = (g.nLines + g.band - 1) / g.band;
  return nullptr;
}

// ------------------------------------------------------------------------------------------------ BatchNorm apply, gate, residual, act
template <int ACT>
__device__ __forceinline__ float x3b_act(float v) {
  if (ACT == MSPI_ACT_RELU) return relu_nan(v);
  if (ACT == MSPI_ACT_SWISH) return fast_swish(v);
  return v;
}

// Thread i of the grid takes the vectors i, i + stride, ... of the M x CV rows.
template <int ACT>
__global__ __launch_bounds__(256) void bn_gate_act_kernel(const float* x, long ldx, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ gate,
                                                          const float* res, long ldr, float* y, long ldy, long total, int CV, int R) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / CV;
    const int cv = (int)(i - row * CV);
    const float4 v = *reinterpret_cast<const float4*>(x + row * ldx + cv * 4);
    const float4 mu = *reinterpret_cast<const float4*>(mean + cv * 4), rs = *reinterpret_cast<const float4*>(rstd + cv * 4);
    const float4 ga = *reinterpret_cast<const float4*>(gamma + cv * 4), be = *reinterpret_cast<const float4*>(beta + cv * 4);
    float4 o = make_float4(fmaf((v.x - mu.x) * rs.x, ga.x, be.x), fmaf((v.y - mu.y) * rs.y, ga.y, be.y),
                           fmaf((v.z - mu.z) * rs.z, ga.z, be.z), fmaf((v.w - mu.w) * rs.w, ga.w, be.w));
    if (gate) {
      const float4 g = *reinterpret_cast<const float4*>(gate + (row / R) * (long)(CV * 4) + cv * 4);
      o = make_float4(o.x * g.x, o.y * g.y, o.z * g.z, o.w * g.w);
    }
    if (res) {
      const float4 s = *reinterpret_cast<const float4*>(res + row * ldr + cv * 4);
      o = make_float4(s.x + o.x, s.y + o.y, s.z + o.z, s.w + o.w);
    }
    *reinterpret_cast<float4*>(y + row * ldy + cv * 4) = make_float4(x3b_act<ACT>(o.x), x3b_act<ACT>(o.y), x3b_act<ACT>(o.z), x3b_act<ACT>(o.w));
  }
}

// ------------------------------------------------------------------------------------------------ gate and Swish backward
constexpr int GSB_ROWS = 32;         // rows of a sample per workgroup: one record of dgate
constexpr int GSB_Q = 64;            // channel quads per workgroup; 4 row slots beside them

__host__ __device__ inline int gsb_bands(int R) { return (R + GSB_ROWS - 1) / GSB_ROWS; }

// dw / ds of s = w sigmoid(w), on the forward's sigmoid
__device__ __forceinline__ float swish_grad(float w) {
  const float sg = fast_sigmoid(w);
  return sg * fmaf(w, 1.f - sg, 1.f);
}

// Thread (q, rs): channel quad blockIdx.z * 64 + q, rows rs, rs + 4, ... of band blockIdx.x of sample blockIdx.y.  The four row
// slots meet through LDS in slot order.
template <bool GATE>
__global__ __launch_bounds__(256) void gate_swish_bwd_kernel(const float* ds, long ldds, const float* __restrict__ v0, long ldv,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ gate, float* dv, long lddv,
                                                             float* __restrict__ ws, int R, int C) {
  __shared__ float4 sh[4][GSB_Q];
  const int q = threadIdx.x & (GSB_Q - 1), rs = threadIdx.x >> 6;
  const int cv = blockIdx.z * GSB_Q + q;
  const bool live = cv * 4 < C;
  const int n = blockIdx.y;
  const int r0 = blockIdx.x * GSB_ROWS, r1 = r0 + GSB_ROWS < R ? r0 + GSB_ROWS : R;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float4 mu = *reinterpret_cast<const float4*>(mean + cv * 4), rsd = *reinterpret_cast<const float4*>(rstd + cv * 4);
    const float4 ga = *reinterpret_cast<const float4*>(gamma + cv * 4), be = *reinterpret_cast<const float4*>(beta + cv * 4);
    float4 g = make_float4(1.f, 1.f, 1.f, 1.f);
    if (GATE) g = *reinterpret_cast<const float4*>(gate + (long)n * C + cv * 4);
    for (int r = r0 + rs; r < r1; r += 4) {
      const long row = (long)n * R + r;
      const float4 u = *reinterpret_cast<const float4*>(v0 + row * ldv + cv * 4);
      const float4 d = *reinterpret_cast<const float4*>(ds + row * ldds + cv * 4);
      const float4 v = make_float4(fmaf((u.x - mu.x) * rsd.x, ga.x, be.x), fmaf((u.y - mu.y) * rsd.y, ga.y, be.y),
                                   fmaf((u.z - mu.z) * rsd.z, ga.z, be.z), fmaf((u.w - mu.w) * rsd.w, ga.w, be.w));
      const float4 dw = make_float4(d.x * swish_grad(v.x * g.x), d.y * swish_grad(v.y * g.y), d.z * swish_grad(v.z * g.z),
                                    d.w * swish_grad(v.w * g.w));
      *reinterpret_cast<float4*>(dv + row * lddv + cv * 4) = make_float4(dw.x * g.x, dw.y * g.y, dw.z * g.z, dw.w * g.w);
      if (GATE) {
        acc.x = fmaf(dw.x, v.x, acc.x); acc.y = fmaf(dw.y, v.y, acc.y); acc.z = fmaf(dw.z, v.z, acc.z); acc.w = fmaf(dw.w, v.w, acc.w);
      }
    }
  }
  if (GATE) {
    sh[rs][q] = acc;
    __syncthreads();
    if (rs == 0 && live) {
      const float4 a = sh[0][q], b = sh[1][q], c = sh[2][q], e = sh[3][q];
      float* rec = ws + ((long)n * gridDim.x + blockIdx.x) * C + cv * 4;
      *reinterpret_cast<float4*>(rec) = make_float4((a.x + b.x) + (c.x + e.x), (a.y + b.y) + (c.y + e.y), (a.z + b.z) + (c.z + e.z),
                                                    (a.w + b.w) + (c.w + e.w));
    }
  }
}

// dgate[n][e]: the sum of sample n's S band records in band order; grid (ceil(C / 64), N).
__global__ __launch_bounds__(256) void gate_reduce_kernel(const float* __restrict__ ws, int S, int C, float* __restrict__ dgate) {
  __shared__ float part[4][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < C;
  const long n = blockIdx.y;
  const float r = rt_sum_records(ws + n * S * C + (live ? e : 0), C, S, live, part);
  if (threadIdx.x < 64 && live) dgate[n * C + e] = r;
}

static const char* gsb_refusal(int32_t N, int32_t R, int32_t C) {
  if (N <= 0 || N >= 65536) return "0 < N < 65536 samples";
  if (R <= 0) return "no rows (R <= 0)";
  if ((long)N * R >= (1L << 31)) return "2^31 or more rows";
  if (C <= 0 || C > X3B_MAXC || C % 4) return "C must be a multiple of 4 with 0 < C <= 4096";
  return nullptr;
}

// ------------------------------------------------------------------------------------------------ squeeze-excite MLP
constexpr int SE_MAXF = 64;

// The dot of a row of wrow (stride ws) with the LDS vector v over n entries, by the lanes of one wave: lane l takes entries
// l, l + 64, ... as one fmaf chain, then the wave's xor tree.
__device__ __forceinline__ float se_wave_dot(const float* __restrict__ wrow, long stride, const float* v, int n) {
  float s = 0.f;
  for (int i = threadIdx.x & 63; i < n; i += 64) s = fmaf(wrow[i * stride], v[i], s);
  return wave_sum(s);
}

__global__ __launch_bounds__(256) void se_train_fwd_kernel(const float* __restrict__ pool0, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, float* __restrict__ p, float* __restrict__ h,
                                                           float* __restrict__ gate, int C, int F) {
  __shared__ float sp[X3B_MAXC];
  __shared__ float shh[SE_MAXF];
  const long n = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float v = fmaf((pool0[n * C + c] - mean[c]) * rstd[c], gamma[c], beta[c]);
    sp[c] = v;
    p[n * C + c] = v;
  }
  __syncthreads();
  for (int f = threadIdx.x >> 6; f < F; f += 4) {
    const float v = relu_nan(se_wave_dot(w1 + (long)f * C, 1, sp, C) + b1[f]);
    if ((threadIdx.x & 63) == 0) {
      shh[f] = v;
      h[n * F + f] = v;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = b2[c];
    for (int f = 0; f < F; ++f) s = fmaf(w2[(long)c * F + f], shh[f], s);
    gate[n * C + c] = fast_sigmoid(s);
  }
}

// One workgroup a sample: dz2 and dz1 to the sample's record [C + F], dp to its row.
__global__ __launch_bounds__(256) void se_train_bwd_kernel(const float* __restrict__ dgate, const float* __restrict__ gate,
                                                           const float* __restrict__ h, const float* __restrict__ w1,
                                                           const float* __restrict__ w2, float* __restrict__ dp, float* __restrict__ ws,
                                                           int C, int F) {
  __shared__ float s2[X3B_MAXC];
  __shared__ float s1[SE_MAXF];
  const long n = blockIdx.x;
  float* rec = ws + n * (C + F);
  for (int c = threadIdx.x; c < C; c += 256) {
    const float g = gate[n * C + c];
    const float v = dgate[n * C + c] * (g * (1.f - g));
    s2[c] = v;
    rec[c] = v;
  }
  __syncthreads();
  for (int f = threadIdx.x >> 6; f < F; f += 4) {
    const float dh = se_wave_dot(w2 + f, F, s2, C);
    if ((threadIdx.x & 63) == 0) {
      const float v = h[n * F + f] > 0.f ? dh : 0.f;
      s1[f] = v;
      rec[C + f] = v;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int f = 0; f < F; ++f) s = fmaf(w1[(long)f * C + c], s1[f], s);
    dp[n * C + c] = s;
  }
}

// Element e of dW2 [C][F] | db2 [C] | dW1 [F][C] | db1 [F]: the N samples in index order, one thread each.
__global__ __launch_bounds__(256) void se_train_wgrad_kernel(const float* __restrict__ ws, const float* __restrict__ h,
                                                             const float* __restrict__ p, float* __restrict__ dw1,
                                                             float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2,
                                                             int N, int C, int F) {
  const int CF = C * F;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * CF + C + F) return;
  const int S = C + F;
  float s = 0.f;
  if (e < CF) {
    const int c = e / F, f = e - c * F;
    for (int n = 0; n < N; ++n) s = fmaf(ws[(long)n * S + c], h[(long)n * F + f], s);
    dw2[e] = s;
  } else if (e < CF + C) {
    const int c = e - CF;
    for (int n = 0; n < N; ++n) s += ws[(long)n * S + c];
    db2[c] = s;
  } else if (e < 2 * CF + C) {
    const int i = e - CF - C, f = i / C, c = i - f * C;
    for (int n = 0; n < N; ++n) s = fmaf(ws[(long)n * S + C + f], p[(long)n * C + c], s);
    dw1[i] = s;
  } else {
    const int f = e - 2 * CF - C;
    for (int n = 0; n < N; ++n) s += ws[(long)n * S + C + f];
    db1[f] = s;
  }
}

static const char* se_refusal(int32_t N, int32_t C, int32_t F) {
  if (N <= 0 || N >= 65536) return "0 < N < 65536 samples";
  if (C <= 0 || C > X3B_MAXC || C % 4) return "C must be a multiple of 4 with 0 < C <= 4096";
  if (F <= 0 || F > SE_MAXF) return "0 < F <= 64 (fc1.out_channels)";
  return nullptr;
}

// ------------------------------------------------------------------------------------------------ the residual's skip path
__global__ __launch_bounds__(256) void relu_mask_add_kernel(float* dx, long lddx, const float* __restrict__ g, long ldg,
                                                            const float* __restrict__ y, long ldy, long total, int CV) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / CV;
    const int cv = (int)(i - row * CV);
    const float4 o = *reinterpret_cast<const float4*>(y + row * ldy + cv * 4);
    const float4 d = *reinterpret_cast<const float4*>(g + row * ldg + cv * 4);
    float4 a = *reinterpret_cast<const float4*>(dx + row * lddx + cv * 4);
    a.x += o.x > 0.f ? d.x : 0.f; a.y += o.y > 0.f ? d.y : 0.f; a.z += o.z > 0.f ? d.z : 0.f; a.w += o.w > 0.f ? d.w : 0.f;
    *reinterpret_cast<float4*>(dx + row * lddx + cv * 4) = a;
  }
}

static unsigned x3b_grid(long total) {
  const long b = (total + 255) / 256;
  return (unsigned)(b > 8192 ? 8192 : b);
}

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_dwconv3_wgrad_supported(const MspiDwConvDesc* d) {
  Dw3Geom g;
  const char* why = dw3_refusal(d, g);
  if (why) set_error("mspi_dwconv3_wgrad: %s", why);
  return why ? 0 : 1;
}

extern "C" size_t mspi_dwconv3_wgrad_ws_bytes(const MspiDwConvDesc* d) {
  Dw3Geom g;
  if (dw3_refusal(d, g)) return 0;
  return (size_t)g.nBands * 28 * d->C * sizeof(float);
}

extern "C" int mspi_dwconv3_wgrad(const MspiDwConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                                  mspi_stream_t stream) {
  Dw3Geom g;
  const char* why = dw3_refusal(d, g);
  MSPI_REQUIRE(!why, "mspi_dwconv3_wgrad: %s", why);
  MSPI_REQUIRE(x && dy && dW && ws, "mspi_dwconv3_wgrad: null argument (only db may be NULL)");
  MSPI_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dW) && aligned16(db) && aligned16(ws),
               "mspi_dwconv3_wgrad: x, dy, dW, db and ws must be 16-byte aligned");
  Dw3Args a;
  a.x = x; a.dy = dy; a.ws = (float*)ws;
  a.ldx = d->ldx; a.ldy = d->ldy;
  a.T = d->T; a.H = d->H; a.W = d->W; a.C = d->C; a.nLines = g.nLines; a.band = g.band;
  const int n = (db ? 28 : 27) * d->C;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dwconv3_wgrad_kernel, dim3((unsigned)g.nBands, (unsigned)g.groups), dim3(g.QG, 9), 0, st, a);
  hipLaunchKernelGGL(dwconv3_reduce_kernel, dim3((n + 63) / 64), dim3(256), 0, st, (const float*)ws, g.nBands, n, d->C, dW, db);
  return check_launch("mspi_dwconv3_wgrad");
}

extern "C" int mspi_bn_gate_act_fwd(const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                                    const float* beta, const float* gate, const float* res, int64_t ldr, float* y, int64_t ldy,
                                    int64_t M, int32_t R, int32_t C, int32_t act, mspi_stream_t stream) {
  MSPI_REQUIRE(x && mean && rstd && gamma && beta && y, "mspi_bn_gate_act_fwd: null argument (only gate and res may be NULL)");
  MSPI_REQUIRE(M > 0 && M < (1L << 31), "mspi_bn_gate_act_fwd: M=%ld: 0 < M < 2^31 rows", (long)M);
  MSPI_REQUIRE(C > 0 && C <= X3B_MAXC && C % 4 == 0, "mspi_bn_gate_act_fwd: C=%d: C must be a multiple of 4 with 0 < C <= 4096", C);
  MSPI_REQUIRE(R > 0 && M % R == 0, "mspi_bn_gate_act_fwd: R=%d: the rows of a sample must divide M=%ld", R, (long)M);
  MSPI_REQUIRE(act == MSPI_ACT_NONE || act == MSPI_ACT_RELU || act == MSPI_ACT_SWISH,
               "mspi_bn_gate_act_fwd: act must be MSPI_ACT_NONE, MSPI_ACT_RELU or MSPI_ACT_SWISH");
  MSPI_REQUIRE(x3b_rows_ok(x, ldx, C) && x3b_rows_ok(y, ldy, C) && (!res || x3b_rows_ok(res, ldr, C)),
               "mspi_bn_gate_act_fwd: x, res and y must be 16-byte aligned, their row strides multiples of 4, >= C");
  MSPI_REQUIRE(aligned16(mean) && aligned16(rstd) && aligned16(gamma) && aligned16(beta) && aligned16(gate),
               "mspi_bn_gate_act_fwd: mean, rstd, gamma, beta and gate must be 16-byte aligned");
  const int CV = C / 4;
  const long total = (long)M * CV;
  hipStream_t st = (hipStream_t)stream;
#define MSPI_BGA(A)                                                                                                                  \
  hipLaunchKernelGGL((bn_gate_act_kernel<A>), dim3(x3b_grid(total)), dim3(256), 0, st, x, (long)ldx, mean, rstd, gamma, beta, gate, res, \
                     (long)ldr, y, (long)ldy, total, CV, R)
  if (act == MSPI_ACT_RELU) MSPI_BGA(MSPI_ACT_RELU);
  else if (act == MSPI_ACT_SWISH) MSPI_BGA(MSPI_ACT_SWISH);
  else MSPI_BGA(MSPI_ACT_NONE);
#undef MSPI_BGA
  return check_launch("mspi_bn_gate_act_fwd");
}

extern "C" size_t mspi_gate_swish_bwd_ws_bytes(int32_t N, int32_t R, int32_t C) {
  if (gsb_refusal(N, R, C)) return 0;
  return (size_t)N * gsb_bands(R) * C * sizeof(float);
}

extern "C" int mspi_gate_swish_bwd(const float* ds, int64_t ldds, const float* v0, int64_t ldv, const float* mean, const float* rstd,
                                   const float* gamma, const float* beta, const float* gate, float* dv, int64_t lddv, float* dgate,
                                   void* ws, int32_t N, int32_t R, int32_t C, mspi_stream_t stream) {
  MSPI_REQUIRE(ds && v0 && mean && rstd && gamma && beta && dv, "mspi_gate_swish_bwd: null argument");
  MSPI_REQUIRE(!gate || (dgate && ws), "mspi_gate_swish_bwd: with a gate, dgate and ws must be given");
  const char* why = gsb_refusal(N, R, C);
  MSPI_REQUIRE(!why, "mspi_gate_swish_bwd: N=%d R=%d C=%d: %s", N, R, C, why);
  MSPI_REQUIRE(x3b_rows_ok(ds, ldds, C) && x3b_rows_ok(v0, ldv, C) && x3b_rows_ok(dv, lddv, C),
               "mspi_gate_swish_bwd: ds, v0 and dv must be 16-byte aligned, their row strides multiples of 4, >= C");
  MSPI_REQUIRE(aligned16(mean) && aligned16(rstd) && aligned16(gamma) && aligned16(beta) && aligned16(gate) && aligned16(dgate) && aligned16(ws),
               "mspi_gate_swish_bwd: mean, rstd, gamma, beta, gate, dgate and ws must be 16-byte aligned");
  const int nb = gsb_bands(R), CV = C / 4;
  const dim3 grid((unsigned)nb, (unsigned)N, (unsigned)((CV + GSB_Q - 1) / GSB_Q));
  hipStream_t st = (hipStream_t)stream;
  if (gate) {
    hipLaunchKernelGGL((gate_swish_bwd_kernel<true>), grid, dim3(256), 0, st, ds, (long)ldds, v0, (long)ldv, mean, rstd, gamma, beta, gate,
                       dv, (long)lddv, (float*)ws, R, C);
    hipLaunchKernelGGL(gate_reduce_kernel, dim3((C + 63) / 64, (unsigned)N), dim3(256), 0, st, (const float*)ws, nb, C, dgate);
  } else {
    hipLaunchKernelGGL((gate_swish_bwd_kernel<false>), grid, dim3(256), 0, st, ds, (long)ldds, v0, (long)ldv, mean, rstd, gamma, beta, gate,
                       dv, (long)lddv, (float*)ws, R, C);
  }
  return check_launch("mspi_gate_swish_bwd");
}

extern "C" int mspi_se_train_fwd(const float* pool0, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                 const float* w1, const float* b1, const float* w2, const float* b2, float* p, float* h, float* gate,
                                 int32_t N, int32_t C, int32_t F, mspi_stream_t stream) {
  MSPI_REQUIRE(pool0 && mean && rstd && gamma && beta && w1 && b1 && w2 && b2 && p && h && gate, "mspi_se_train_fwd: null argument");
  const char* why = se_refusal(N, C, F);
  MSPI_REQUIRE(!why, "mspi_se_train_fwd: N=%d C=%d F=%d: %s", N, C, F, why);
  MSPI_REQUIRE(aligned16(pool0) && aligned16(mean) && aligned16(rstd) && aligned16(gamma) && aligned16(beta) && aligned16(w1) &&
                   aligned16(b1) && aligned16(w2) && aligned16(b2) && aligned16(p) && aligned16(h) && aligned16(gate),
               "mspi_se_train_fwd: every pointer must be 16-byte aligned");
  hipLaunchKernelGGL(se_train_fwd_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, pool0, mean, rstd, gamma, beta, w1, b1,
                     w2, b2, p, h, gate, C, F);
  return check_launch("mspi_se_train_fwd");
}

extern "C" size_t mspi_se_train_bwd_ws_bytes(int32_t N, int32_t C, int32_t F) {
  if (se_refusal(N, C, F)) return 0;
  return (size_t)N * (C + F) * sizeof(float);
}

extern "C" int mspi_se_train_bwd(const float* dgate, const float* gate, const float* h, const float* p, const float* w1,
                                 const float* w2, float* dw1, float* db1, float* dw2, float* db2, float* dp, void* ws, int32_t N,
                                 int32_t C, int32_t F, mspi_stream_t stream) {
  MSPI_REQUIRE(dgate && gate && h && p && w1 && w2 && dw1 && db1 && dw2 && db2 && dp && ws, "mspi_se_train_bwd: null argument");
  const char* why = se_refusal(N, C, F);
  MSPI_REQUIRE(!why, "mspi_se_train_bwd: N=%d C=%d F=%d: %s", N, C, F, why);
  MSPI_REQUIRE(aligned16(dgate) && aligned16(gate) && aligned16(h) && aligned16(p) && aligned16(w1) && aligned16(w2) && aligned16(dw1) &&
                   aligned16(db1) && aligned16(dw2) && aligned16(db2) && aligned16(dp) && aligned16(ws),
               "mspi_se_train_bwd: every pointer must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(se_train_bwd_kernel, dim3((unsigned)N), dim3(256), 0, st, dgate, gate, h, w1, w2, dp, (float*)ws, C, F);
  const int n = 2 * C * F + C + F;
  hipLaunchKernelGGL(se_train_wgrad_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)ws, h, p, dw1, db1, dw2, db2, N, C, F);
  return check_launch("mspi_se_train_bwd");
}

extern "C" int mspi_relu_mask_add(float* dx, int64_t lddx, const float* g, int64_t ldg, const float* y, int64_t ldy, int64_t M,
                                  int32_t C, mspi_stream_t stream) {
  MSPI_REQUIRE(dx && g && y, "mspi_relu_mask_add: null argument");
  MSPI_REQUIRE(M > 0 && M < (1L << 31), "mspi_relu_mask_add: M=%ld: 0 < M < 2^31 rows", (long)M);
  MSPI_REQUIRE(C > 0 && C % 4 == 0, "mspi_relu_mask_add: C=%d: C must be a positive multiple of 4", C);
  MSPI_REQUIRE(x3b_rows_ok(dx, lddx, C) && x3b_rows_ok(g, ldg, C) && x3b_rows_ok(y, ldy, C),
               "mspi_relu_mask_add: dx, g and y must be 16-byte aligned, their row strides multiples of 4, >= C");
  const int CV = C / 4;
  const long total = (long)M * CV;
  hipLaunchKernelGGL(relu_mask_add_kernel, dim3(x3b_grid(total)), dim3(256), 0, (hipStream_t)stream, dx, (long)lddx, g, (long)ldg, y,
                     (long)ldy, total, CV);
  return check_launch("mspi_relu_mask_add");
}
