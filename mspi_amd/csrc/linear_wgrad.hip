// Weight and bias gradient of an nn.Linear layer over rows: the transformer Block's qkv, proj, fc1 and fc2 and the SyncBlock's
// vis_proj.  Entry point (include/mspi_linear_train_hip.h), fp32:
//   mspi_linear_wgrad   dW [N][K] = dy^T x and db [N] = the column sums of dy            one pass + the ordered add
// v_mfma_f32_32x32x2_f32 with the rows as the contraction: D[n][k] += A[n][r] B[r][k], r = two consecutive rows, lane l feeding
// A = dy[r + (l >> 5)][n0 + (l & 31)] and B = x[r + (l >> 5)][k0 + (l & 31)] -- both operands along their rows as they lie in
// memory, no transpose anywhere.
// A workgroup owns a LW_BN x LW_BK = 128 x 128 block of dW and one slice of L rows; wave w the 64 x 64 quarter (w >> 1, w & 1) as
// 2 x 2 accumulator tiles of 32 x 32, four independent MFMA chains.  Rows are staged LW_RC = 32 at a time as two panels
// [32][128], dy and x, each global float read once per workgroup; a bank is a column, so the one-float-per-lane operand reads
// are conflict free.  Two LDS buffers: the global loads of panel p + 1 are issued into registers BEFORE the 64 MFMAs a wave
// spends on panel p and land in the other buffer after them, so one barrier a panel and no load latency in the open.
// Blocks past N or K: a wave whose quarter starts past N or past K does nothing; inside a live quarter a tile past the edge
// multiplies staged zeros and is not stored.  Sums that cross a workgroup go through the caller's workspace as one record
// [N][K] + [N] per slice, which the second launch adds in slice order (rt_sum_records, common.h): bitwise repeatable.  Nothing
// here allocates or synchronises.
#include "common.h"
#include "../../include/mspi_linear_train_hip.h"

namespace mspi {

typedef float lw_v16f __attribute__((ext_vector_type(16)));

constexpr int LW_T = 256;
constexpr int LW_RC = 32;                // rows per staged panel
constexpr int LW_BN = 128;               // dW rows (columns of dy) per workgroup
constexpr int LW_BK = 128;               // dW columns (columns of x) per workgroup
constexpr int LW_MAX_W = 4096;           // widest N and K
constexpr int LW_WANT_WGS = 512;         // about two workgroups a CU on 256 CUs
constexpr int LW_MIN_SLICE = 128;        // rows: four panels at least, so the pipeline has something to hide under
constexpr long LW_MAX_SLICE = (1L << 31) - 32;      // the most rows an int names, in whole panels
constexpr int LW_PANEL = LW_RC * 128;    // floats per panel

struct LinWgradArgs {
  const float* x;
  const float* dy;
  float* ws;
  long ldx, lddy, M;
  int N, K, L;
  int bias;
};

__host__ __device__ inline long lw_record_floats(int N, int K) { return (long)N * K + N; }

// rows per slice: the header's formula
static int lw_slice_rows(long M, int N, int K) {
  const int blocks = ((N + LW_BN - 1) / LW_BN) * ((K + LW_BK - 1) / LW_BK);
  const int want = LW_WANT_WGS / blocks > 1 ? LW_WANT_WGS / blocks : 1;
  const long per = (M + want - 1) / want;
  const long L = (per + LW_RC - 1) / LW_RC * LW_RC;
  return (int)(L < LW_MIN_SLICE ? LW_MIN_SLICE : (L > LW_MAX_SLICE ? LW_MAX_SLICE : L));
}

__global__ __launch_bounds__(LW_T) void linear_wgrad_kernel(const LinWgradArgs p) {
  __shared__ float4 smem4[2 * 2 * LW_PANEL / 4];                  // [buffer][dy | x][32][128]: 64 KB
  float* smem = reinterpret_cast<float*>(smem4);
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the branch around the MFMAs below is uniform
  const int nh = wave >> 1, kh = wave & 1;
  const int n0 = blockIdx.x * LW_BN, k0 = blockIdx.y * LW_BK;
  const bool busy = n0 + nh * 64 < p.N && k0 + kh * 64 < p.K;     // my quarter has at least its first tile

  // staging roles: thread (sr, sq) loads column quad sq of rows sr, sr + 8, sr + 16, sr + 24 of both panels
  const int sq = tid & 31, sr = tid >> 5;
  const bool dlive = n0 + sq * 4 < p.N, xlive = k0 + sq * 4 < p.K;    // a quad never straddles an edge: N % 4 == K % 4 == 0
  const float* dsrc = p.dy + n0 + sq * 4;
  const float* xsrc = p.x + k0 + sq * 4;
  const long m0s = (long)blockIdx.z * p.L;
  const long m1s = m0s + p.L < p.M ? m0s + p.L : p.M;
  const int panels = (int)((m1s - m0s + LW_RC - 1) / LW_RC);

  float4 pd[4], px[4];
  auto fetch = [&](long m0) {                                     // rows past the slice are selected to zero, never read
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long row = m0 + sr + 8 * j;
      pd[j] = px[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < m1s) {
        if (dlive) pd[j] = *reinterpret_cast<const float4*>(dsrc + row * p.lddy);
        if (xlive) px[j] = *reinterpret_cast<const float4*>(xsrc + row * p.ldx);
      }
    }
  };
  auto stash = [&](float* buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<float4*>(buf + (sr + 8 * j) * 128 + sq * 4) = pd[j];
      *reinterpret_cast<float4*>(buf + LW_PANEL + (sr + 8 * j) * 128 + sq * 4) = px[j];
    }
  };

  lw_v16f acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float bs0 = 0.f, bs1 = 0.f;                                     // db of my two channel tiles: the A operands, row parity lh

  fetch(m0s);
  stash(smem);
  __syncthreads();
  for (int pn = 0; pn < panels; ++pn) {
    const float* cur = smem + (pn & 1) * 2 * LW_PANEL;
    const bool more = pn + 1 < panels;                            // uniform over the workgroup
    if (more) fetch(m0s + (long)(pn + 1) * LW_RC);
    if (busy) {
      const float* dr = cur + lh * 128 + nh * 64 + li;
      const float* xr = cur + LW_PANEL + lh * 128 + kh * 64 + li;
#pragma unroll
      for (int i = 0; i < LW_RC / 2; ++i) {
        const float a0 = dr[i * 256], a1 = dr[i * 256 + 32], b0 = xr[i * 256], b1 = xr[i * 256 + 32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        bs0 += a0;
        bs1 += a1;
      }
    }
    if (more) stash(smem + ((pn + 1) & 1) * 2 * LW_PANEL);        // its last readers passed the barrier of panel pn - 1
    __syncthreads();
  }

  if (!busy) return;
  // accumulator (reg r, lane) -> D[n = (r & 3) + 8 (r >> 2) + 4 lh][k = li] of its tile
  float* rec = p.ws + (long)blockIdx.z * lw_record_floats(p.N, p.K);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int nt = n0 + nh * 64 + i * 32;
    if (nt >= p.N) continue;                                      // N % 32 == 0: a tile is whole or absent
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + kh * 64 + j * 32 + li;
      if (k < p.K) {
#pragma unroll
        for (int r = 0; r < 16; ++r) rec[(long)(nt + (r & 3) + 8 * (r >> 2) + 4 * lh) * p.K + k] = acc[i][j][r];
      }
    }
  }
  if (p.bias && blockIdx.y == 0 && kh == 0) {
    float* rb = rec + (long)p.N * p.K + n0 + nh * 64;
    bs0 += __shfl_xor(bs0, 32, 64);                               // the two rows of every pair
    bs1 += __shfl_xor(bs1, 32, 64);
    if (lane < 32) {
      rb[lane] = bs0;
      if (n0 + nh * 64 + 32 < p.N) rb[32 + lane] = bs1;
    }
  }
}

// dW [N][K] then db [N] (n = nW without a bias), both in the records' own layout, slice by slice in order; grid ceil(n / 64).
__global__ __launch_bounds__(256) void linear_wgrad_reduce_kernel(const float* __restrict__ ws, int S, long stride, long nW, long n,
                                                                  float* __restrict__ dW, float* __restrict__ db, int* status) {
  __shared__ float part[4][64];
  const long e = (long)blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = e < n;
  const float r = rt_sum_records(ws + (live ? e : 0), stride, S, live, part);
  if (threadIdx.x < 64 && live) {
    if (e < nW) dW[e] = r;
    else db[e - nW] = r;
    report_nonfinite(status, nonfinite(r));
  }
}

static const char* lw_refusal(int64_t M, int32_t N, int32_t K) {
  if (M <= 0) return "no rows (M must be positive)";
  if (M >= (1L << 31)) return "2^31 or more rows";
  if (N > LW_MAX_W || K > LW_MAX_W) return "N and K must be at most 4096";
  if (N < 32 || N % 32) return "N must be a multiple of 32 (N % 32 == 0)";
  if (K < 4 || K % 4) return "K must be a multiple of 4 (K % 4 == 0)";
  return nullptr;
}

static const char* lw_operand_refusal(const void* x, int64_t ldx, const void* dy, int64_t lddy, int32_t N, int32_t K) {
  if (!x || !dy) return "null argument";
  if (!aligned16(x) || !aligned16(dy)) return "x and dy must be 16-byte aligned";
  if (ldx % 4 || lddy % 4) return "row strides must be multiples of 4 floats";
  if (ldx < K || lddy < N) return "row strides must be >= the width (ldx >= K, lddy >= N)";
  return nullptr;
}

}  // namespace mspi

using namespace mspi;

extern "C" size_t mspi_linear_wgrad_ws_bytes(int64_t M, int32_t N, int32_t K) {
  if (lw_refusal(M, N, K)) return 0;
  const int L = lw_slice_rows(M, N, K);
  return (size_t)((M + L - 1) / L) * lw_record_floats(N, K) * sizeof(float);
}

extern "C" int mspi_linear_wgrad_variant(const void* x, int64_t ldx, const void* dy, int64_t lddy, int64_t M, int32_t N, int32_t K) {
  const char* why = lw_refusal(M, N, K);
  if (!why) why = lw_operand_refusal(x, ldx, dy, lddy, N, K);
  if (why) {
    set_error("mspi_linear_wgrad: %s", why);
    return -1;
  }
  return lw_slice_rows(M, N, K);
}

extern "C" int mspi_linear_wgrad(const float* x, int64_t ldx, const float* dy, int64_t lddy, float* dW, float* db, void* ws,
                                 int64_t M, int32_t N, int32_t K, mspi_stream_t stream) {
  MSPI_REQUIRE(dW && ws, "mspi_linear_wgrad: null argument");
  if (mspi_linear_wgrad_variant(x, ldx, dy, lddy, M, N, K) < 0) return MSPI_EINVAL;
  MSPI_REQUIRE(aligned16(dW) && aligned16(ws) && aligned16(db), "mspi_linear_wgrad: dW, db and ws must be 16-byte aligned");
  LinWgradArgs a;
  a.x = x; a.dy = dy; a.ws = (float*)ws;
  a.ldx = ldx; a.lddy = lddy; a.M = M;
  a.N = N; a.K = K; a.L = lw_slice_rows(M, N, K);
  a.bias = db ? 1 : 0;
  const int S = (int)((M + a.L - 1) / a.L);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(linear_wgrad_kernel, dim3((N + LW_BN - 1) / LW_BN, (K + LW_BK - 1) / LW_BK, S), dim3(LW_T), 0, st, a);
  const long nW = (long)N * K, n = nW + (db ? N : 0);
  hipLaunchKernelGGL(linear_wgrad_reduce_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, (const float*)ws, S,
                     lw_record_floats(N, K), nW, n, dW, db, g_status_word);
  return check_launch("mspi_linear_wgrad");
}
