// The training criterion (utils/loss.py:26-49 over utils/compute_saliency_metrics.py:9-108) with its gradient: the four
// per-sample terms KL, CC, SIM, NSS of a LOG map against the density / fixation map, and d(w_kl KL - w_cc CC - w_nss NSS)
// / d(log map).  Unlike metrics.hip (one workgroup per sample, three walks) every sample is split over chunks of SL_C
// values on a (chunks, N) grid; a chunk lives in its workgroup's registers, so its own mean is known before its centred
// moments are taken, and chunk moments are merged about the sample mean (Chan et al.): Q = sum_c M2_c + n_c (m_c - m)^2.
// Chunk partials go to the caller's workspace and are combined in a fixed order (lanes over chunks, then the xor tree
// of wave_sum): no float atomics, bitwise repeatable.
//   pass 1   sums, ranges, chunk-centred moments                          -> ws partials
//   pass 2   every wave combines pass 1's partials, then KL, SIM, T sums   -> ws partials, sample statistics
//   finish   one wave per sample: the four terms, T into the statistics
//   backward one element-wise pass from the statistics
#include "common.h"

namespace mspi {

constexpr int SL_T = 256;              // threads per workgroup
constexpr int SL_E = 8;                // values per thread
constexpr int SL_C = SL_T * SL_E;      // values per chunk
constexpr int SL_ST = 16;              // floats of statistics per sample
constexpr int SL_P1 = 12;              // floats per chunk, pass 1
constexpr int SL_P2 = 4;               // floats per chunk, pass 2
constexpr float SL_EPS = 2.2204e-16f;

// Workspace of one sample: SlStats, then [chunks][SL_P1], then [chunks][SL_P2].
struct SlStats { float P, G, F, ms, mg, Qs, Qg, A, D, mns, mxs, mng, mxg, T, r0, r1; };
static_assert(sizeof(SlStats) == SL_ST * 4, "SlStats");

__host__ __device__ inline int sl_chunks(int L) { return (L + SL_C - 1) / SL_C; }
__host__ __device__ inline size_t sl_sample_floats(int L) { return SL_ST + (size_t)sl_chunks(L) * (SL_P1 + SL_P2); }

// K sums (or maxima) over the workgroup; every thread gets them.  Fixed order: xor tree, then the four waves.
template <int K, bool MAX>
__device__ __forceinline__ void sl_block_reduce(float (&v)[K], float* sh) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = MAX ? wave_max(v[k]) : wave_sum(v[k]);
  __syncthreads();                       // sh may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k * 4 + (threadIdx.x >> 6)] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float a = sh[k * 4], b = sh[k * 4 + 1], c = sh[k * 4 + 2], d = sh[k * 4 + 3];
    v[k] = MAX ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : (a + b) + (c + d);
  }
}

// Position inside the chunk of a thread's k-th value: two float4 per thread, or eight strided scalars.
template <bool VEC>
__device__ __forceinline__ int sl_pos(int k) {
  return VEC ? (((int)threadIdx.x + SL_T * (k >> 2)) << 2) + (k & 3) : (int)threadIdx.x + SL_T * k;
}

template <bool VEC>
__device__ __forceinline__ void sl_load(const float* __restrict__ p, int cnt, float (&v)[SL_E], float fill) {
  if (VEC) {
#pragma unroll
    for (int q = 0; q < SL_E / 4; ++q) {
      const int i = ((int)threadIdx.x + SL_T * q) << 2;
      float4 t;
      if (i + 4 <= cnt) {
        t = *reinterpret_cast<const float4*>(p + i);
      } else {
        t.x = i < cnt ? p[i] : fill; t.y = i + 1 < cnt ? p[i + 1] : fill;
        t.z = i + 2 < cnt ? p[i + 2] : fill; t.w = i + 3 < cnt ? p[i + 3] : fill;
      }
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < SL_E; ++k) { const int i = sl_pos<false>(k); v[k] = i < cnt ? p[i] : fill; }
  }
}

// A chunk of the three maps in registers: s = exp(log map), 0 beyond the row's end (g and f too).
template <bool VEC>
__device__ __forceinline__ void sl_load_chunk(const float* __restrict__ x_, const float* __restrict__ g_,
                                              const float* __restrict__ f_, int cnt, float (&s)[SL_E], float (&g)[SL_E],
                                              float (&f)[SL_E]) {
  sl_load<VEC>(x_, cnt, s, 0.f);
  sl_load<VEC>(g_, cnt, g, 0.f);
  sl_load<VEC>(f_ ? f_ : g_, f_ ? cnt : 0, f, 0.f);          // no fixation map: all 0, nothing is read
#pragma unroll
  for (int k = 0; k < SL_E; ++k) s[k] = sl_pos<VEC>(k) < cnt ? __expf(s[k]) : 0.f;
}

template <bool VEC>
__device__ __forceinline__ void sl_pass1(const float* __restrict__ x_, const float* __restrict__ g_, const float* __restrict__ f_,
                                         int cnt, float* __restrict__ out, float* sh) {
  float s[SL_E], g[SL_E], f[SL_E];
  sl_load_chunk<VEC>(x_, g_, f_, cnt, s, g, f);
  float a[3] = {0.f, 0.f, 0.f};
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};     // max s, -min s, max g, -min g
#pragma unroll
  for (int k = 0; k < SL_E; ++k) {
    a[0] += s[k]; a[1] += g[k]; a[2] += f[k];
    if (sl_pos<VEC>(k) < cnt) {
      m[0] = fmaxf(m[0], s[k]); m[1] = fmaxf(m[1], -s[k]); m[2] = fmaxf(m[2], g[k]); m[3] = fmaxf(m[3], -g[k]);
    }
  }
  sl_block_reduce<3, false>(a, sh);
  sl_block_reduce<4, true>(m, sh);
  const float ms = a[0] / (float)cnt, mg = a[1] / (float)cnt;    // the chunk's own means
  float q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < SL_E; ++k) {
    if (sl_pos<VEC>(k) < cnt) {
      const float ds = s[k] - ms, dg = g[k] - mg;
      q[0] = fmaf(ds, ds, q[0]); q[1] = fmaf(dg, dg, q[1]); q[2] = fmaf(ds, dg, q[2]); q[3] = fmaf(ds, f[k], q[3]);
    }
  }
  sl_block_reduce<4, false>(q, sh);
  if (threadIdx.x == 0) {
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2];
    out[3] = q[0]; out[4] = q[1]; out[5] = q[2]; out[6] = q[3];
    out[7] = -m[1]; out[8] = m[0]; out[9] = -m[3]; out[10] = m[2]; out[11] = 0.f;
  }
}

__global__ __launch_bounds__(SL_T) void salloss_pass1_kernel(const float* __restrict__ logmap, const float* __restrict__ gt,
                                                             const float* __restrict__ fix, float* __restrict__ ws, int L,
                                                             int aligned) {
  __shared__ float sh[16];
  const int c = blockIdx.x, n = blockIdx.y;
  const long base = (long)n * L + (long)c * SL_C;
  const int cnt = min(SL_C, L - c * SL_C);
  float* out = ws + (size_t)n * sl_sample_floats(L) + SL_ST + (size_t)c * SL_P1;
  const float* f_ = fix ? fix + base : nullptr;
  if (aligned && (base & 3) == 0) sl_pass1<true>(logmap + base, gt + base, f_, cnt, out, sh);
  else sl_pass1<false>(logmap + base, gt + base, f_, cnt, out, sh);
}

// The sample's statistics from pass 1's partials, computed by one wave: lane l takes chunks l, l + 64, ... in order.
__device__ __forceinline__ SlStats sl_combine(const float* __restrict__ p1, int chunks, int L) {
  const int lane = threadIdx.x & 63;
  float P = 0.f, G = 0.f, F = 0.f, mxs = -INFINITY, nmns = -INFINITY, mxg = -INFINITY, nmng = -INFINITY;
  for (int c = lane; c < chunks; c += 64) {
    const float* q = p1 + (size_t)c * SL_P1;
    P += q[0]; G += q[1]; F += q[2];
    nmns = fmaxf(nmns, -q[7]); mxs = fmaxf(mxs, q[8]); nmng = fmaxf(nmng, -q[9]); mxg = fmaxf(mxg, q[10]);
  }
  SlStats st;
  st.P = wave_sum(P); st.G = wave_sum(G); st.F = wave_sum(F);
  st.mns = -wave_max(nmns); st.mxs = wave_max(mxs); st.mng = -wave_max(nmng); st.mxg = wave_max(mxg);
  st.ms = st.P / (float)L; st.mg = st.G / (float)L;
  float Qs = 0.f, Qg = 0.f, A = 0.f, D = 0.f;
  for (int c = lane; c < chunks; c += 64) {
    const float* q = p1 + (size_t)c * SL_P1;
    const float cnt = (float)min(SL_C, L - c * SL_C);
    const float ds = q[0] / cnt - st.ms, dg = q[1] / cnt - st.mg;     // chunk mean - sample mean
    Qs += fmaf(cnt * ds, ds, q[3]); Qg += fmaf(cnt * dg, dg, q[4]); A += fmaf(cnt * ds, dg, q[5]); D += fmaf(ds, q[2], q[6]);
  }
  st.Qs = wave_sum(Qs); st.Qg = wave_sum(Qg); st.A = wave_sum(A); st.D = wave_sum(D);
  st.T = 0.f; st.r0 = 0.f; st.r1 = 0.f;
  return st;
}

template <bool VEC>
__device__ __forceinline__ void sl_pass2(const float* __restrict__ x_, const float* __restrict__ g_, int cnt, const SlStats& st,
                                         int L, float* __restrict__ out, float* sh) {
  float s[SL_E], g[SL_E];
  sl_load<VEC>(x_, cnt, s, 0.f);
  sl_load<VEC>(g_, cnt, g, 0.f);
  const float invP = 1.f / st.P, invG = 1.f / st.G;
  // similarity :46-70: the normalised maps' sums are (sum - L min) / (max - min), pass 1 has all three
  const float rs = 1.f / (st.mxs - st.mns), rg = 1.f / (st.mxg - st.mng);
  const float ks = rs / ((st.P - (float)L * st.mns) * rs), kg = rg / ((st.G - (float)L * st.mng) * rg);
  float a[3] = {0.f, 0.f, 0.f};          // KL, SIM, T = sum a_i sp_i
#pragma unroll
  for (int k = 0; k < SL_E; ++k) {
    if (sl_pos<VEC>(k) < cnt) {
      const float sv = __expf(s[k]);
      const float sp = sv * invP, gp = g[k] * invG;
      const float r = gp / (sp + SL_EPS);
      a[0] += gp * logf(SL_EPS + r);
      a[1] += min_nan((sv - st.mns) * ks, (g[k] - st.mng) * kg);
      a[2] -= r * (r / (SL_EPS + r)) * sp;     // a_i = -gp^2 / ((sp + eps)(eps (sp + eps) + gp)) = -r^2 / (eps + r)
    }
  }
  sl_block_reduce<3, false>(a, sh);
  if (threadIdx.x == 0) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = 0.f; }
}

__global__ __launch_bounds__(SL_T) void salloss_pass2_kernel(const float* __restrict__ logmap, const float* __restrict__ gt,
                                                             float* __restrict__ ws, int L, int aligned) {
  __shared__ float sh[16];
  const int c = blockIdx.x, n = blockIdx.y, chunks = gridDim.x;
  float* w = ws + (size_t)n * sl_sample_floats(L);
  // Every wave of every chunk merges all chunk partials again: the same bits everywhere, and under one loop trip per lane
  // at the training shape (42 chunks).  The reads grow as chunks^2 per sample (150 chunks at 480x640, read by 600 waves);
  // if maps of that size matter, merge once in a launch of its own between the passes.
  const SlStats st = sl_combine(w + SL_ST, chunks, L);
  if (c == 0 && threadIdx.x == 0) *reinterpret_cast<SlStats*>(w) = st;
  const long base = (long)n * L + (long)c * SL_C;
  const int cnt = min(SL_C, L - c * SL_C);
  float* out = w + SL_ST + (size_t)chunks * SL_P1 + (size_t)c * SL_P2;
  if (aligned && (base & 3) == 0) sl_pass2<true>(logmap + base, gt + base, cnt, st, L, out, sh);
  else sl_pass2<false>(logmap + base, gt + base, cnt, st, L, out, sh);
}

__global__ __launch_bounds__(64) void salloss_finish_kernel(float* __restrict__ ws, float* __restrict__ terms, int L, int has_fix) {
  const int n = blockIdx.x, lane = threadIdx.x, chunks = sl_chunks(L);
  float* w = ws + (size_t)n * sl_sample_floats(L);
  const float* p2 = w + SL_ST + (size_t)chunks * SL_P1;
  float kl = 0.f, sim = 0.f, T = 0.f;
  for (int c = lane; c < chunks; c += 64) { kl += p2[c * SL_P2]; sim += p2[c * SL_P2 + 1]; T += p2[c * SL_P2 + 2]; }
  kl = wave_sum(kl); sim = wave_sum(sim); T = wave_sum(T);
  if (lane == 0) {
    SlStats* st = reinterpret_cast<SlStats*>(w);
    st->T = T;
    const float sd = sqrtf(st->Qs / (float)(L - 1));           // torch.std: unbiased
    terms[n * 4 + 0] = kl;
    terms[n * 4 + 1] = st->A / sqrtf(st->Qs * st->Qg);
    terms[n * 4 + 2] = sim;
    terms[n * 4 + 3] = has_fix ? st->D / ((sd + SL_EPS) * st->F) : 0.f;
  }
}

// Per-sample coefficients of the gradient with the weights folded in:
//   dlog = s * (kl (a - T) - c1 (dg - c2 ds) - (n1 (f - n0) - n2 ds))
struct SlCoef { float invP, invG, ms, mg, T, kl, c1, c2, n0, n1, n2; };

__device__ __forceinline__ float sl_grad(float x, float g, float f, const SlCoef& k) {
  const float s = __expf(x);
  const float sp = s * k.invP, gp = g * k.invG;
  const float r = gp / (sp + SL_EPS);
  const float a = -r * (r / (SL_EPS + r));
  const float ds = s - k.ms, dg = g - k.mg;
  return s * (k.kl * (a - k.T) - k.c1 * (dg - k.c2 * ds) - (k.n1 * (f - k.n0) - k.n2 * ds));
}

template <bool HAS_F>
__global__ __launch_bounds__(SL_T) void salloss_bwd_kernel(const float* __restrict__ logmap, const float* __restrict__ gt,
                                                           const float* __restrict__ fix, const float* __restrict__ ws,
                                                           const float* __restrict__ grad_out, float w_kl, float w_cc,
                                                           float w_nss, float* __restrict__ dlog, int L, int aligned) {
  const int n = blockIdx.y;
  const SlStats st = *reinterpret_cast<const SlStats*>(ws + (size_t)n * sl_sample_floats(L));
  const float go = *grad_out;
  SlCoef k;
  k.invP = 1.f / st.P; k.invG = 1.f / st.G; k.ms = st.ms; k.mg = st.mg; k.T = st.T;
  k.kl = go * w_kl * k.invP;
  k.c1 = go * w_cc / sqrtf(st.Qs * st.Qg);
  k.c2 = st.A / st.Qs;
  k.n0 = k.n1 = k.n2 = 0.f;
  if (HAS_F) {
    const float sd = sqrtf(st.Qs / (float)(L - 1)), se = sd + SL_EPS;
    k.n0 = st.F / (float)L;
    k.n1 = go * w_nss / (se * st.F);
    k.n2 = go * w_nss * st.D / (se * se * (float)(L - 1) * sd * st.F);
  }
  const long base = (long)n * L;
  const float* x_ = logmap + base;
  const float* g_ = gt + base;
  const float* f_ = HAS_F ? fix + base : nullptr;
  float* d_ = dlog + base;
  const int stride = gridDim.x * SL_T, first = blockIdx.x * SL_T + threadIdx.x;
  if (aligned && (base & 3) == 0) {
    const int L4 = L >> 2;
    for (int i = first; i < L4; i += stride) {
      const float4 x = reinterpret_cast<const float4*>(x_)[i], g = reinterpret_cast<const float4*>(g_)[i];
      float4 f = {0.f, 0.f, 0.f, 0.f};
      if (HAS_F) f = reinterpret_cast<const float4*>(f_)[i];
      float4 d;
      d.x = sl_grad(x.x, g.x, f.x, k); d.y = sl_grad(x.y, g.y, f.y, k);
      d.z = sl_grad(x.z, g.z, f.z, k); d.w = sl_grad(x.w, g.w, f.w, k);
      reinterpret_cast<float4*>(d_)[i] = d;
    }
    const int i = (L4 << 2) + first;                       // the row's last L % 4 values
    if (i < L) d_[i] = sl_grad(x_[i], g_[i], HAS_F ? f_[i] : 0.f, k);
  } else {
    for (int i = first; i < L; i += stride) d_[i] = sl_grad(x_[i], g_[i], HAS_F ? f_[i] : 0.f, k);
  }
}

}  // namespace mspi

extern "C" size_t mspi_saliency_loss_ws_bytes(int32_t N, int32_t L) {
  if (N <= 0 || L <= 1) return 0;
  return (size_t)N * mspi::sl_sample_floats(L) * sizeof(float);
}

extern "C" int mspi_saliency_loss_fwd(const float* logmap, const float* gt, const float* fix, float* terms, void* ws, int32_t N,
                                      int32_t L, mspi_stream_t stream) {
  MSPI_REQUIRE(logmap && gt && terms && ws && N > 0 && N <= 65535 && L > 1, "mspi_saliency_loss_fwd: bad argument");
  MSPI_REQUIRE(mspi::aligned16(ws), "mspi_saliency_loss_fwd: ws must be 16-byte aligned");
  const int chunks = mspi::sl_chunks(L);
  const int aligned = mspi::aligned16(logmap) && mspi::aligned16(gt) && (!fix || mspi::aligned16(fix));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mspi::salloss_pass1_kernel, dim3(chunks, N), dim3(mspi::SL_T), 0, st, logmap, gt, fix, (float*)ws, L, aligned);
  hipLaunchKernelGGL(mspi::salloss_pass2_kernel, dim3(chunks, N), dim3(mspi::SL_T), 0, st, logmap, gt, (float*)ws, L, aligned);
  hipLaunchKernelGGL(mspi::salloss_finish_kernel, dim3(N), dim3(64), 0, st, (float*)ws, terms, L, fix ? 1 : 0);
  return mspi::check_launch("mspi_saliency_loss_fwd");
}

extern "C" int mspi_saliency_loss_bwd(const float* logmap, const float* gt, const float* fix, const void* ws, const float* grad_out,
                                      float w_kl, float w_cc, float w_nss, float* dlog, int32_t N, int32_t L, mspi_stream_t stream) {
  MSPI_REQUIRE(logmap && gt && ws && grad_out && dlog && N > 0 && N <= 65535 && L > 1, "mspi_saliency_loss_bwd: bad argument");
  MSPI_REQUIRE(mspi::aligned16(ws), "mspi_saliency_loss_bwd: ws must be 16-byte aligned");
  const bool has_f = fix && w_nss != 0.f;                  // without fixations the NSS term and its 4 bytes per value drop out
  const int aligned = mspi::aligned16(logmap) && mspi::aligned16(gt) && (!has_f || mspi::aligned16(fix)) && mspi::aligned16(dlog);
  const dim3 grid(mspi::sl_chunks(L), N), block(mspi::SL_T);
  hipStream_t st = (hipStream_t)stream;
  if (has_f)
    hipLaunchKernelGGL(mspi::salloss_bwd_kernel<true>, grid, block, 0, st, logmap, gt, fix, (const float*)ws, grad_out, w_kl, w_cc,
                       w_nss, dlog, L, aligned);
  else
    hipLaunchKernelGGL(mspi::salloss_bwd_kernel<false>, grid, block, 0, st, logmap, gt, fix, (const float*)ws, grad_out, w_kl, w_cc,
                       0.f, dlog, L, aligned);
  return mspi::check_launch("mspi_saliency_loss_bwd");
}
