// Saliency metrics as device reductions: KL divergence, linear correlation (CC), similarity (SIM) and normalised
// scanpath saliency (NSS) of a predicted map against the ground-truth density / fixation map, one workgroup per
// sample, three passes over the H*W values (they stay in L2), fixed-order tree reductions (bitwise reproducible).
// Formulas follow utils/compute_saliency_metrics.py:9-108 of the reference term by term (eps = 2.2204e-16, unbiased
// std, min-max normalisation before SIM); the per-sample values are written, the batch mean is the host's.
// Below them the same file's auc_judd (:111-203), the counting part of auc_shuff (:206-276) and ig (:278-308): integer
// counts and fixed-order reductions only, so these launches are bitwise reproducible too.
#include "common.h"

namespace mspi {

constexpr int MT = 1024;   // threads per workgroup

__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();                       // sh may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < MT / 64; ++i) t += sh[i];
  return t;
}
__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = sh[0];
#pragma unroll
  for (int i = 1; i < MT / 64; ++i) t = fmaxf(t, sh[i]);
  return t;
}

__global__ __launch_bounds__(MT) void saliency_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                              const float* __restrict__ fix, float* __restrict__ out,
                                                              int L, int pred_is_log) {
  __shared__ float sh[MT / 64];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* s_ = pred + (long)n * L;
  const float* g_ = gt + (long)n * L;
  const float* f_ = fix ? fix + (long)n * L : nullptr;
  const float eps = 2.2204e-16f;
  auto S = [&](int i) { return pred_is_log ? __expf(s_[i]) : s_[i]; };

  // pass A: sums and ranges
  float ss = 0.f, sg = 0.f, sf = 0.f, mns = INFINITY, mxs = -INFINITY, mng = INFINITY, mxg = -INFINITY;
  for (int i = tid; i < L; i += MT) {
    const float s = S(i), g = g_[i];
    ss += s; sg += g;
    mns = fminf(mns, s); mxs = fmaxf(mxs, s); mng = fminf(mng, g); mxg = fmaxf(mxg, g);
    if (f_) sf += f_[i];
  }
  ss = block_sum(ss, sh); sg = block_sum(sg, sh); sf = block_sum(sf, sh);
  mxs = block_max(mxs, sh); mxg = block_max(mxg, sh);
  mns = -block_max(-mns, sh); mng = -block_max(-mng, sh);
  const float mean_s = ss / (float)L, mean_g = sg / (float)L;
  const float rs = 1.f / (mxs - mns), rg = 1.f / (mxg - mng);

  // pass B: centred second moments, sums of the min-max normalised maps
  float qs = 0.f, qg = 0.f, ns = 0.f, ng = 0.f;
  for (int i = tid; i < L; i += MT) {
    const float s = S(i), g = g_[i];
    const float ds = s - mean_s, dg = g - mean_g;
    qs = fmaf(ds, ds, qs); qg = fmaf(dg, dg, qg);
    ns += (s - mns) * rs; ng += (g - mng) * rg;
  }
  qs = block_sum(qs, sh); qg = block_sum(qg, sh); ns = block_sum(ns, sh); ng = block_sum(ng, sh);
  const float std_s = sqrtf(qs / (float)(L - 1)), std_g = sqrtf(qg / (float)(L - 1));   // torch.std: unbiased

  // pass C: the four metrics' sums
  float kl = 0.f, ab = 0.f, aa = 0.f, bb = 0.f, sim = 0.f, ns_f = 0.f;
  for (int i = tid; i < L; i += MT) {
    const float s = S(i), g = g_[i];
    const float sp = s / ss, gp = g / sg;
    kl += gp * logf(eps + gp / (sp + eps));
    const float sz = (s - mean_s) / std_s, gz = (g - mean_g) / std_g;
    ab = fmaf(sz, gz, ab); aa = fmaf(sz, sz, aa); bb = fmaf(gz, gz, bb);
    sim += min_nan((s - mns) * rs / ns, (g - mng) * rg / ng);
    if (f_) ns_f += (s - mean_s) / (std_s + eps) * f_[i];
  }
  kl = block_sum(kl, sh); ab = block_sum(ab, sh); aa = block_sum(aa, sh); bb = block_sum(bb, sh);
  sim = block_sum(sim, sh); ns_f = block_sum(ns_f, sh);
  if (tid == 0) {
    out[n * 4 + 0] = kl;
    out[n * 4 + 1] = ab / sqrtf(aa * bb);
    out[n * 4 + 2] = sim;
    out[n * 4 + 3] = f_ ? ns_f / sf : 0.f;
  }
}

// ---- information gain (compute_saliency_metrics.py:278-308): the KL term's structure with a third map ----
__global__ __launch_bounds__(MT) void saliency_ig_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         const float* __restrict__ base, float* __restrict__ out, int L) {
  __shared__ float sh[MT / 64];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* s_ = pred + (long)n * L;
  const float* g_ = gt + (long)n * L;
  const float* b_ = base + (long)n * L;
  const float eps = 2.2204e-16f;
  float ss = 0.f, sg = 0.f, sb = 0.f;
  for (int i = tid; i < L; i += MT) { ss += s_[i]; sg += g_[i]; sb += b_[i]; }
  ss = block_sum(ss, sh); sg = block_sum(sg, sh); sb = block_sum(sb, sh);
  float ig = 0.f;
  for (int i = tid; i < L; i += MT) ig += g_[i] / sg * (logf(eps + s_[i] / ss) - logf(eps + b_[i] / sb));
  ig = block_sum(ig, sh);
  if (tid == 0) out[n] = ig;
}

// Integer sums are order-independent: exact and reproducible whatever the arrival order.
__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// min and max of a map in its own type; every thread gets both.  sh: 2 * MT / 64 values.
template <typename T>
__device__ __forceinline__ void block_minmax(const T* __restrict__ s, int L, T* sh, T& mn, T& mx) {
  T lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < L; i += MT) { const T v = s[i]; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo; hi = b > hi ? b : hi;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = lo; sh[MT / 64 + (threadIdx.x >> 6)] = hi; }
  __syncthreads();
  mn = sh[0]; mx = sh[MT / 64];
#pragma unroll
  for (int i = 1; i < MT / 64; ++i) { mn = sh[i] < mn ? sh[i] : mn; mx = sh[MT / 64 + i] > mx ? sh[MT / 64 + i] : mx; }
}

// ---- shuffled AUC, device part (compute_saliency_metrics.py:206-276): 9 + 9 counts and the two fixation counts ----
__global__ __launch_bounds__(MT) void saliency_sauc_kernel(const float* __restrict__ sal, const float* __restrict__ gt,
                                                           const float* __restrict__ other, int* __restrict__ counts,
                                                           int H, int W) {
  __shared__ float shf[2 * MT / 64];
  __shared__ int acc[20];
  const int m = blockIdx.x, tid = threadIdx.x, L = H * W;
  const float* s_ = sal + (long)m * L;
  const float* g_ = gt + (long)m * L;
  const float* o_ = other + (long)m * L;
  if (tid < 20) acc[tid] = 0;
  float mn, mx;
  block_minmax<float>(s_, L, shf, mn, mx);       // its barriers also publish acc = 0
  const float range = mx - mn;
  // the float32 values that the Python floats 0.1 .. 0.9 become inside numpy's float32 comparison
  const float th[9] = {0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f, 0.9f};
  int c[20];
#pragma unroll
  for (int k = 0; k < 20; ++k) c[k] = 0;
  for (int p = tid; p < L; p += MT) {
    const float s = (s_[p] - mn) / range, g = g_[p];
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] += ((s >= th[k] ? 1.f : 0.f) + g == 2.f) ? 1 : 0;
    c[18] += g == 1.f ? 1 : 0;
    if (o_[p] == 1.f) {
      const int row = p / W, col = p - row * W;
      const int code = row * H + col;             // :226 -- H, not W
      int r2 = code % H - 1;                      // :246 -- row -1 is the last row
      if (r2 < 0) r2 = H - 1;
      const int c2 = code / H;                    // < W whenever H <= W (the host refuses H > W)
      const float r = (s_[r2 * W + c2] - mn) / range;
#pragma unroll
      for (int k = 0; k < 9; ++k) c[9 + k] += r > th[k] ? 1 : 0;
      c[19] += 1;
    }
  }
#pragma unroll
  for (int k = 0; k < 20; ++k) {
    const int v = wave_isum(c[k]);
    if ((tid & 63) == 0 && v) atomicAdd(&acc[k], v);
  }
  __syncthreads();
  if (tid < 20) counts[m * 20 + tid] = acc[tid];
}

// ---- AUC-Judd (compute_saliency_metrics.py:111-203) ----
// Per-map scratch: AucHead, then room for L thresholds (sized for double), then L + 1 counters.
struct AucHead { double mn, mx; int n; int pad[11]; };   // 64 bytes
constexpr int AUC_LDS_N = 4096;     // thresholds kept in LDS (32 KiB as double) beside their counters (16 KiB)
constexpr int AUC_PIX = 8;          // pixels per thread of the counting pass

__host__ __device__ inline size_t auc_list_off() { return sizeof(AucHead); }
__host__ __device__ inline size_t auc_hist_off(int L) { return sizeof(AucHead) + (size_t)L * 8; }
__host__ __device__ inline size_t auc_map_bytes(int L) { return (auc_hist_off(L) + (size_t)(L + 1) * 4 + 63) / 64 * 64; }

// Bitonic network in its one-direction form (the first step of every round pairs i with i ^ (k - 1), the later steps
// with i ^ j; every comparator leaves the larger value at the lower index).  With all comparators pointing the same
// way, positions >= n behave as -inf padding that never moves, so any n sorts without storage for the padding.
template <typename T>
__device__ __forceinline__ void sort_desc(T* a, int n) {
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int mask = (j == (k >> 1)) ? k - 1 : j;
      __syncthreads();
      for (int t = threadIdx.x; t < (n2 >> 1); t += MT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));     // bit j of i is 0
        const int p = i ^ mask;                                    // p > i
        if (p < n) {
          const T x = a[i], y = a[p];
          if (x < y) { a[i] = y; a[p] = x; }
        }
      }
    }
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(MT) void auc_prepare_kernel(const T* __restrict__ sal, const float* __restrict__ fix,
                                                         char* __restrict__ ws, int* __restrict__ nfix, int L) {
  __shared__ T shm[2 * MT / 64];
  __shared__ T lst[AUC_LDS_N];
  __shared__ int cnt;
  const int m = blockIdx.x, tid = threadIdx.x;
  const T* s_ = sal + (long)m * L;
  const float* f_ = fix + (long)m * L;
  char* w = ws + (size_t)m * auc_map_bytes(L);
  AucHead* head = reinterpret_cast<AucHead*>(w);
  T* list = reinterpret_cast<T*>(w + auc_list_off());
  int* hist = reinterpret_cast<int*>(w + auc_hist_off(L));
  if (tid == 0) cnt = 0;
  T mn, mx;
  block_minmax<T>(s_, L, shm, mn, mx);           // its barriers also publish cnt = 0
  const T range = mx - mn;
  // the normalised values at the fixations, in arrival order (the sort below makes that order irrelevant)
  for (int i = tid; i < L; i += MT)
    if (f_[i] > 0.f) list[atomicAdd(&cnt, 1)] = (s_[i] - mn) / range;
  __syncthreads();
  const int n = cnt;
  if (n <= AUC_LDS_N) {
    for (int i = tid; i < n; i += MT) lst[i] = list[i];
    sort_desc<T>(lst, n);
    for (int i = tid; i < n; i += MT) list[i] = lst[i];
  } else {
    sort_desc<T>(list, n);
  }
  for (int i = tid; i <= n; i += MT) hist[i] = 0;
  if (tid == 0) { head->mn = (double)mn; head->mx = (double)mx; head->n = n; nfix[m] = n; }
}

// Counting pass: a pixel of value v adds one to bucket j = first index with thresh[j] <= v (n: below every threshold);
// above[i] = #{S >= thresh[i]} is then the inclusive prefix sum of the buckets.
template <typename T>
__global__ __launch_bounds__(MT) void auc_count_kernel(const T* __restrict__ sal, char* __restrict__ ws, int L) {
  __shared__ T lst[AUC_LDS_N];
  __shared__ int hl[AUC_LDS_N + 1];
  const int m = blockIdx.y, tid = threadIdx.x;
  const T* s_ = sal + (long)m * L;
  char* w = ws + (size_t)m * auc_map_bytes(L);
  const AucHead* head = reinterpret_cast<const AucHead*>(w);
  const T* list = reinterpret_cast<const T*>(w + auc_list_off());
  int* hist = reinterpret_cast<int*>(w + auc_hist_off(L));
  const int n = head->n;
  if (n == 0) return;
  const T mn = (T)head->mn, range = (T)head->mx - (T)head->mn;   // both were of type T: the round trip is exact
  const bool lds = n <= AUC_LDS_N;
  if (lds) {
    for (int i = tid; i < n; i += MT) lst[i] = list[i];
    for (int i = tid; i <= n; i += MT) hl[i] = 0;
    __syncthreads();
  }
  const int base = blockIdx.x * (MT * AUC_PIX);
  auto pass = [&](const T* th, int* h) {           // called once per address space, so the searches are ds / global reads
#pragma unroll
    for (int u = 0; u < AUC_PIX; ++u) {
      const int i = base + u * MT + tid;
      if (i < L) {
        const T v = (s_[i] - mn) / range;
        int lo = 0, hi = n;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (th[mid] <= v) hi = mid; else lo = mid + 1;
        }
        atomicAdd(&h[lo], 1);
      }
    }
  };
  if (lds) pass(lst, hl); else pass(list, hist);
  if (lds) {
    __syncthreads();
    for (int i = tid; i <= n; i += MT)
      if (hl[i]) atomicAdd(&hist[i], hl[i]);
  }
}

// Scan of the buckets and the float64 trapezoid of tp over fp (:169-182): points p = 0 .. n + 1 with (fp, tp) = (0, 0),
// ((above[p-1] - (p-1)) / (L - n), p / n) for p = 1 .. n, (1, 1); term k joins the points k and k + 1.
__global__ __launch_bounds__(MT) void auc_finish_kernel(const char* __restrict__ ws, double* __restrict__ score, int L) {
  __shared__ int part[MT];
  __shared__ double red[MT / 64];
  const int m = blockIdx.x, tid = threadIdx.x;
  const char* w = ws + (size_t)m * auc_map_bytes(L);
  const AucHead* head = reinterpret_cast<const AucHead*>(w);
  const int* hist = reinterpret_cast<const int*>(w + auc_hist_off(L));
  const int n = head->n;
  if (n == 0 || !(head->mx > head->mn)) {          // no fixation (:133), or 0/0 everywhere (:156)
    if (tid == 0) score[m] = __builtin_nan("");
    return;
  }
  const int per = (n + MT - 1) / MT;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += hist[i];
  part[tid] = s;
  __syncthreads();
  if (tid < 64) {                                   // exclusive scan of the MT partial sums by one wave
    int run = 0;
    for (int c = 0; c < MT / 64; ++c) {
      const int v = part[c * 64 + tid];
      int inc = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (tid >= o) inc += t; }
      part[c * 64 + tid] = run + inc - v;
      run += __shfl(inc, 63, 64);
    }
  }
  __syncthreads();
  const double dn = (double)n, dneg = (double)(L - n);
  int above = part[tid];                           // above[lo - 1]
  double sum = 0.0;
  for (int i = lo; i < hi; ++i) {
    const double fp0 = i == 0 ? 0.0 : (double)(above - (i - 1)) / dneg, tp0 = (double)i / dn;
    above += hist[i];
    const double fp1 = (double)(above - i) / dneg, tp1 = (double)(i + 1) / dn;
    sum += (fp1 - fp0) * (tp1 + tp0) / 2.0;
  }
  if (tid == 0) {                                   // term n: point n to (1, 1); above[n-1] = L - #{below every threshold}
    const double fp0 = (double)((L - hist[n]) - (n - 1)) / dneg;
    sum += (1.0 - fp0) * (1.0 + 1.0) / 2.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < MT / 64; ++i) t += red[i];
    score[m] = t;
  }
}

template <typename T>
static void auc_launch(const void* sal, const float* fix, double* score, int* nfix, void* ws, int N, int L, hipStream_t st) {
  const int chunks = (L + MT * AUC_PIX - 1) / (MT * AUC_PIX);
  hipLaunchKernelGGL(auc_prepare_kernel<T>, dim3(N), dim3(MT), 0, st, (const T*)sal, fix, (char*)ws, nfix, L);
  hipLaunchKernelGGL(auc_count_kernel<T>, dim3(chunks, N), dim3(MT), 0, st, (const T*)sal, (char*)ws, L);
  hipLaunchKernelGGL(auc_finish_kernel, dim3(N), dim3(MT), 0, st, (const char*)ws, score, L);
}

}  // namespace mspi

extern "C" size_t mspi_saliency_auc_ws_bytes(int32_t N, int32_t L) {
  if (N <= 0 || L <= 1) return 0;
  return (size_t)N * mspi::auc_map_bytes(L);
}

extern "C" int mspi_saliency_auc_judd(const void* sal, int32_t is_f64, const float* fix, double* score, int32_t* nfix,
                                      void* ws, int32_t N, int32_t L, mspi_stream_t stream) {
  MSPI_REQUIRE(sal && fix && score && nfix && ws && N > 0 && N <= 65535 && L > 1, "mspi_saliency_auc_judd: bad argument");
  MSPI_REQUIRE(mspi::aligned16(ws), "mspi_saliency_auc_judd: ws must be 16-byte aligned");
  if (is_f64) mspi::auc_launch<double>(sal, fix, score, nfix, ws, N, L, (hipStream_t)stream);
  else mspi::auc_launch<float>(sal, fix, score, nfix, ws, N, L, (hipStream_t)stream);
  return mspi::check_launch("mspi_saliency_auc_judd");
}

extern "C" int mspi_saliency_sauc_counts(const float* sal, const float* gt, const float* other, int32_t* counts, int32_t N,
                                         int32_t H, int32_t W, mspi_stream_t stream) {
  MSPI_REQUIRE(sal && gt && other && counts && N > 0 && H > 0 && W > 0 && (int64_t)H * W > 1 && (int64_t)H * W < (1 << 30),
               "mspi_saliency_sauc_counts: bad argument");
  MSPI_REQUIRE(H <= W, "mspi_saliency_sauc_counts: H = %d > W = %d: the reference's other-fixation index (row * H + col, read "
               "back as [k %% H - 1][k / H]) leaves the map", H, W);
  hipLaunchKernelGGL(mspi::saliency_sauc_kernel, dim3(N), dim3(mspi::MT), 0, (hipStream_t)stream, sal, gt, other, counts, H, W);
  return mspi::check_launch("mspi_saliency_sauc_counts");
}

extern "C" int mspi_saliency_ig(const float* pred, const float* gt, const float* base, float* out, int32_t N, int32_t L,
                                mspi_stream_t stream) {
  MSPI_REQUIRE(pred && gt && base && out && N > 0 && L > 1, "mspi_saliency_ig: bad argument");
  hipLaunchKernelGGL(mspi::saliency_ig_kernel, dim3(N), dim3(mspi::MT), 0, (hipStream_t)stream, pred, gt, base, out, L);
  return mspi::check_launch("mspi_saliency_ig");
}

extern "C" int mspi_saliency_metrics(const float* pred, const float* gt, const float* fix, float* out, int32_t N, int32_t L,
                                     int32_t pred_is_log, mspi_stream_t stream) {
  MSPI_REQUIRE(pred && gt && out && N > 0 && L > 1, "mspi_saliency_metrics: bad argument");
  hipLaunchKernelGGL(mspi::saliency_metrics_kernel, dim3(N), dim3(mspi::MT), 0, (hipStream_t)stream, pred, gt, fix, out, L,
                     pred_is_log);
  return mspi::check_launch("mspi_saliency_metrics");
}
