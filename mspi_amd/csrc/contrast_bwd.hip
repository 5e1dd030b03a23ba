// Backward of the contrastive head (model/model_utils.py:545-552): the three pieces no other file has.  Entry points
// (include/mspi_contrast_train_hip.h), all fp32:
//   mspi_neg_cosine_bwd       dp of out = -scale mean_n cos(p_n, z_n), z constant             one launch, a workgroup a row
//   mspi_layernorm_act_bwd    LayerNorm backward for rows of C <= 2048 under an optional ReLU  one pass + the ordered add
//   mspi_mean_rows_bwd        dx[n][r][:] (+)= g[n][:] / R into a row range of a wider slab    one launch
// The head works on M = B rows (one per clip), so none of the three is after throughput: each keeps a row with one owner (a
// workgroup for the cosine, a wave for the LayerNorm) so that nothing is added across owners except dgamma / dbeta, which leave
// as one record per workgroup and are added by a second launch in record order.  Two runs give equal bits.
#include "common.h"
#include "../../include/mspi_contrast_train_hip.h"

namespace mspi {

constexpr float COS_EPS = 1e-8f;         // F.cosine_similarity's eps, on each norm (neg_cosine_kernel, rowops.hip)

// The forward's sums in the forward's order: thread t takes columns t, t + 256, ... as one fmaf chain, then the wave's xor tree
// and the four waves in wave order (block_reduce of rowops.hip).
__device__ __forceinline__ float ncb_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void neg_cosine_bwd_kernel(const float* __restrict__ p, const float* __restrict__ z,
                                                             const float* __restrict__ g, float* __restrict__ dp, int N, int C,
                                                             float scale, int* status) {
  __shared__ float red[4];
  const long n = blockIdx.x;
  const float* pr = p + n * C;
  const float* zr = z + n * C;
  float dot = 0.f, pp = 0.f, zz = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float a = pr[c], b = zr[c];
    dot = fmaf(a, b, dot);
    pp = fmaf(a, a, pp);
    zz = fmaf(b, b, zz);
  }
  dot = ncb_block_sum(dot, red);
  pp = ncb_block_sum(pp, red);
  zz = ncb_block_sum(zz, red);
  const float np_raw = sqrtf(pp);
  const float np = max_nan(np_raw, COS_EPS), nz = max_nan(sqrtf(zz), COS_EPS);      // a NaN norm stays a NaN
  const float coef = -g[0] * scale / (float)N;
  const float inv = 1.f / (np * nz);
  // below the clamp np is a constant and only the first term is left; a NaN norm takes the second term and stays a NaN
  const float k2 = np_raw < COS_EPS ? 0.f : dot * inv / (np * np);
  bool bad = false;
  for (int c4 = threadIdx.x; c4 < (C >> 2); c4 += 256) {
    const float4 a = *reinterpret_cast<const float4*>(pr + c4 * 4), b = *reinterpret_cast<const float4*>(zr + c4 * 4);
    const float4 o = make_float4(coef * (b.x * inv - k2 * a.x), coef * (b.y * inv - k2 * a.y), coef * (b.z * inv - k2 * a.z),
                                 coef * (b.w * inv - k2 * a.w));
    bad |= nonfinite(o.x) || nonfinite(o.y) || nonfinite(o.z) || nonfinite(o.w);
    *reinterpret_cast<float4*>(dp + n * C + c4 * 4) = o;
  }
  report_nonfinite(status, bad);
}

// ------------------------------------------------------------------------------------------------ LayerNorm, C <= 2048, ReLU mask
constexpr int LNA_ROWS = 8;              // rows a workgroup (one wave) walks: one record of dbeta | dgamma
constexpr int LNA_MAXC = 2048;

__host__ __device__ inline long lna_groups(long M) { return (M + LNA_ROWS - 1) / LNA_ROWS; }

// Lane l owns the vectors l, l + 64, ... of the row (VPT of them: 8 at C = 2048).
template <int VPT>
__global__ __launch_bounds__(64) void layernorm_act_bwd_kernel(const float* x, long ldx, const float* dy, long lddy, const float* y,
                                                               long ldy, const float* __restrict__ gamma, float eps, float* dx,
                                                               long lddx, float* __restrict__ ws, long M, int C, int* status) {
  const int lane = threadIdx.x;
  const int nv = C >> 2;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 sg[VPT], sb[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    sg[j] = zero;
    sb[j] = zero;
  }
  const long base = (long)blockIdx.x * LNA_ROWS;
  bool bad = false;
  for (int r = 0; r < LNA_ROWS; ++r) {
    const long row = base + r;
    if (row >= M) break;                                  // uniform over the wave
    float4 v[VPT], d[VPT];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int i = lane + 64 * j;
      v[j] = zero;
      d[j] = zero;
      if (i < nv) {
        v[j] = *reinterpret_cast<const float4*>(x + row * ldx + i * 4);
        d[j] = *reinterpret_cast<const float4*>(dy + row * lddy + i * 4);
        if (y) {                                          // the ReLU's mask; a NaN in y is neither > 0 nor <= 0 and stays
          const float4 t = *reinterpret_cast<const float4*>(y + row * ldy + i * 4);
          d[j].x = t.x > 0.f ? d[j].x : (t.x <= 0.f ? 0.f : t.x);
          d[j].y = t.y > 0.f ? d[j].y : (t.y <= 0.f ? 0.f : t.y);
          d[j].z = t.z > 0.f ? d[j].z : (t.z <= 0.f ? 0.f : t.z);
          d[j].w = t.w > 0.f ? d[j].w : (t.w <= 0.f ? 0.f : t.w);
        }
      }
      s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      if (lane + 64 * j < nv) {
        const float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, e = v[j].w - mean;
        q += (a * a + b * b) + (c * c + e * e);
      }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int i = lane + 64 * j;
      if (i < nv) {
        const float4 gm = *reinterpret_cast<const float4*>(gamma + i * 4);
        v[j] = make_float4((v[j].x - mean) * rstd, (v[j].y - mean) * rstd, (v[j].z - mean) * rstd, (v[j].w - mean) * rstd);   // x^
        sg[j].x = fmaf(d[j].x, v[j].x, sg[j].x); sg[j].y = fmaf(d[j].y, v[j].y, sg[j].y);
        sg[j].z = fmaf(d[j].z, v[j].z, sg[j].z); sg[j].w = fmaf(d[j].w, v[j].w, sg[j].w);
        sb[j].x += d[j].x; sb[j].y += d[j].y; sb[j].z += d[j].z; sb[j].w += d[j].w;
        d[j] = make_float4(d[j].x * gm.x, d[j].y * gm.y, d[j].z * gm.z, d[j].w * gm.w);                                       // d gamma
        s1 += (d[j].x + d[j].y) + (d[j].z + d[j].w);
        s2 += (d[j].x * v[j].x + d[j].y * v[j].y) + (d[j].z * v[j].z + d[j].w * v[j].w);
      }
    }
    const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C;
    // every load of the row is behind the two sums above, so dx may be dy
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int i = lane + 64 * j;
      if (i < nv) {
        const float4 o = make_float4(rstd * (d[j].x - m1 - v[j].x * m2), rstd * (d[j].y - m1 - v[j].y * m2),
                                     rstd * (d[j].z - m1 - v[j].z * m2), rstd * (d[j].w - m1 - v[j].w * m2));
        bad |= nonfinite(o.x) || nonfinite(o.y) || nonfinite(o.z) || nonfinite(o.w);
        *reinterpret_cast<float4*>(dx + row * lddx + i * 4) = o;
      }
    }
  }
  report_nonfinite(status, bad);
  float* rec = ws + (long)blockIdx.x * 2 * C;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int i = lane + 64 * j;
    if (i < nv) {
      *reinterpret_cast<float4*>(rec + i * 4) = sb[j];
      *reinterpret_cast<float4*>(rec + C + i * 4) = sg[j];
    }
  }
}

// Sum of the S records [n] in ws in record order, element e to a[e] (e < nA) or b[e - nA]; grid ceil(n / 64).
__global__ __launch_bounds__(256) void contrast_reduce_kernel(const float* __restrict__ ws, long S, int n, int nA,
                                                              float* __restrict__ a, float* __restrict__ b, int* status) {
  __shared__ float part[4][64];
  const int g = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int e = blockIdx.x * 64 + l;
  float s = 0.f;
  if (e < n)
    for (long i = g; i < S; i += 4) s += ws[i * n + e];
  part[g][l] = s;
  __syncthreads();
  if (g == 0 && e < n) {
    const float r = (part[0][l] + part[1][l]) + (part[2][l] + part[3][l]);
    report_nonfinite(status, nonfinite(r));
    if (e < nA) a[e] = r;
    else b[e - nA] = r;
  }
}

// ------------------------------------------------------------------------------------------------ the adjoint of mean_rows
__global__ __launch_bounds__(256) void mean_rows_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, long ldx,
                                                            long sample_stride, int R, int C, int accumulate, int* status) {
  const int nv = C >> 2;
  const long n = blockIdx.y, total = (long)R * nv;
  const float fr = (float)R;
  bool bad = false;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / nv;
    const int c4 = (int)(idx - r * nv);
    const float4 t = *reinterpret_cast<const float4*>(g + n * C + c4 * 4);
    float4 o = make_float4(t.x / fr, t.y / fr, t.z / fr, t.w / fr);
    float* dst = dx + n * sample_stride + r * ldx + c4 * 4;
    if (accumulate) {
      const float4 u = *reinterpret_cast<const float4*>(dst);
      o = make_float4(u.x + o.x, u.y + o.y, u.z + o.z, u.w + o.w);
    }
    bad |= nonfinite(o.x) || nonfinite(o.y) || nonfinite(o.z) || nonfinite(o.w);
    *reinterpret_cast<float4*>(dst) = o;
  }
  report_nonfinite(status, bad);
}

static const char* lna_refusal(int64_t M, int32_t C) {
  if (M <= 0) return "no rows (M <= 0)";
  if (M >= (1L << 31)) return "2^31 or more rows";
  if (C <= 0 || C > LNA_MAXC || C % 4) return "C must be a multiple of 4 with 0 < C <= 2048";
  return nullptr;
}

static bool lna_rows_ok(const void* p, int64_t ld, int32_t C) { return aligned16(p) && ld >= C && ld % 4 == 0; }

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_neg_cosine_bwd(const float* p, const float* z, const float* g, float* dp, int32_t N, int32_t C, float scale,
                                   mspi_stream_t stream) {
  MSPI_REQUIRE(p && z && g && dp, "mspi_neg_cosine_bwd: null argument");
  MSPI_REQUIRE(N > 0, "mspi_neg_cosine_bwd: N=%d: no rows (N <= 0)", N);
  MSPI_REQUIRE(C > 0 && C % 4 == 0, "mspi_neg_cosine_bwd: C=%d: C must be a positive multiple of 4", C);
  MSPI_REQUIRE(aligned16(p) && aligned16(z) && aligned16(dp) && (reinterpret_cast<uintptr_t>(g) & 3u) == 0,
               "mspi_neg_cosine_bwd: p, z and dp must be 16-byte aligned, g 4-byte aligned");
  hipLaunchKernelGGL(neg_cosine_bwd_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, p, z, g, dp, N, C, scale,
                     g_status_word);
  return check_launch("mspi_neg_cosine_bwd");
}

extern "C" size_t mspi_layernorm_act_bwd_ws_bytes(int64_t M, int32_t C) {
  if (lna_refusal(M, C)) return 0;
  return (size_t)lna_groups(M) * 2 * C * sizeof(float);
}

extern "C" int mspi_layernorm_act_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* y, int64_t ldy,
                                      const float* gamma, float eps, float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws,
                                      int64_t M, int32_t C, mspi_stream_t stream) {
  MSPI_REQUIRE(x && dy && gamma && dx && dgamma && dbeta && ws, "mspi_layernorm_act_bwd: null argument");
  const char* why = lna_refusal(M, C);
  MSPI_REQUIRE(!why, "mspi_layernorm_act_bwd: M=%ld C=%d: %s", (long)M, C, why);
  MSPI_REQUIRE(eps >= 0.f, "mspi_layernorm_act_bwd: negative eps");
  MSPI_REQUIRE(lna_rows_ok(x, ldx, C) && lna_rows_ok(dy, lddy, C) && lna_rows_ok(dx, lddx, C) && (!y || lna_rows_ok(y, ldy, C)),
               "mspi_layernorm_act_bwd: x, dy, y and dx must be 16-byte aligned, their row strides multiples of 4, >= C");
  MSPI_REQUIRE(aligned16(gamma) && aligned16(dgamma) && aligned16(dbeta) && aligned16(ws),
               "mspi_layernorm_act_bwd: gamma, dgamma, dbeta and ws must be 16-byte aligned");
  const long G = lna_groups(M);
  hipStream_t st = (hipStream_t)stream;
  float* w = (float*)ws;
  const int vpt = (C / 4 + 63) / 64;
#define MSPI_LNA_LAUNCH(V)                                                                                                      \
  hipLaunchKernelGGL(layernorm_act_bwd_kernel<V>, dim3((unsigned)G), dim3(64), 0, st, x, (long)ldx, dy, (long)lddy, y, (long)ldy, \
                     gamma, eps, dx, (long)lddx, w, (long)M, C, g_status_word)
  if (vpt <= 2) MSPI_LNA_LAUNCH(2);
  else if (vpt <= 4) MSPI_LNA_LAUNCH(4);
  else MSPI_LNA_LAUNCH(8);
#undef MSPI_LNA_LAUNCH
  hipLaunchKernelGGL(contrast_reduce_kernel, dim3((2 * C + 63) / 64), dim3(256), 0, st, (const float*)w, G, 2 * C, C, dbeta, dgamma,
                     g_status_word);
  return check_launch("mspi_layernorm_act_bwd");
}

extern "C" int mspi_mean_rows_bwd(const float* g, float* dx, int64_t ldx, int64_t sample_stride, int32_t N, int32_t R, int32_t C,
                                  int32_t accumulate, mspi_stream_t stream) {
  MSPI_REQUIRE(g && dx, "mspi_mean_rows_bwd: null argument");
  MSPI_REQUIRE(N > 0 && N < 65536, "mspi_mean_rows_bwd: N=%d: 0 < N < 65536 samples", N);
  MSPI_REQUIRE(R > 0, "mspi_mean_rows_bwd: R=%d: no rows (R <= 0)", R);
  MSPI_REQUIRE(C > 0 && C % 4 == 0, "mspi_mean_rows_bwd: C=%d: C must be a positive multiple of 4", C);
  MSPI_REQUIRE(aligned16(g) && aligned16(dx), "mspi_mean_rows_bwd: g and dx must be 16-byte aligned");
  MSPI_REQUIRE(ldx >= C && ldx % 4 == 0, "mspi_mean_rows_bwd: ldx=%ld: the row stride must be a multiple of 4, >= C=%d", (long)ldx, C);
  MSPI_REQUIRE(sample_stride % 4 == 0 && (N == 1 || sample_stride >= (int64_t)R * ldx),
               "mspi_mean_rows_bwd: sample_stride=%ld: the sample stride must be a multiple of 4, >= R * ldx", (long)sample_stride);
  const long blocks = ((long)R * (C / 4) + 255) / 256;
  hipLaunchKernelGGL(mean_rows_bwd_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks), (unsigned)N), dim3(256), 0,
                     (hipStream_t)stream, g, dx, (long)ldx, (long)sample_stride, R, C, accumulate, g_status_word);
  return check_launch("mspi_mean_rows_bwd");
}
