// Backward of the decoder stage between the lateral outputs and readout[0] (model/model_utils.py:155-170, 566-572): the SA row
// gate and the top-down sums of up-samples.  Two entry points (include/mspi_train_hip.h), both fp32 and memory-bound:
//   mspi_rowgate_bwd        dx = dy (1 + gate), dz = gate (1 - gate) sum_c dy x      one pass over dy and x
//   mspi_upsample_sum_bwd   dx (= | +=) sum_j up_{k_j}^T(dy_j)                      gather, one thread per dx vector
// The other launches of that backward are in readout_bwd.hip and readout_train.hip.  No float atomics: a row's sum stays inside
// the lanes that own the row and the gather visits its cells in a fixed order, so both are bitwise repeatable.  Nothing here
// allocates or synchronises.
#include "common.h"
#include "upsample_adjoint.h"
#include "../../include/mspi_train_hip.h"

namespace mspi {

// ------------------------------------------------------------------------------------------------ row gate
// L lanes own a row (L a power of two, 64 / L rows per wave): lane l takes the 16-byte vectors l, l + L, ... of the row in
// ascending order, then the L partial sums meet in an xor tree, after which every lane of the group holds the same bits.
// dx may be dy: a lane stores only the vector it has just loaded.
template <int L>
__global__ __launch_bounds__(256) void rowgate_bwd_kernel(const float* dy, long lddy, const float* __restrict__ x, long ldx,
                                                          const float* __restrict__ gate, float* dx, long lddx,
                                                          float* __restrict__ dz, long M, int CV) {
  const long row = (long)blockIdx.x * (256 / L) + threadIdx.x / L;
  const int l = threadIdx.x & (L - 1);
  const bool live = row < M;             // dead rows stay in the shuffles with a zero sum
  float s = 0.f, g = 0.f;
  if (live) {
    g = gate[row];
    const float g1 = 1.f + g;
    const float* pdy = dy + row * lddy;
    const float* px = x + row * ldx;
    for (int cv = l; cv < CV; cv += L) {
      const float4 d = *reinterpret_cast<const float4*>(pdy + cv * 4);
      const float4 v = *reinterpret_cast<const float4*>(px + cv * 4);
      s = fmaf(d.x, v.x, s); s = fmaf(d.y, v.y, s); s = fmaf(d.z, v.z, s); s = fmaf(d.w, v.w, s);
      if (dx) *reinterpret_cast<float4*>(dx + row * lddx + cv * 4) = make_float4(d.x * g1, d.y * g1, d.z * g1, d.w * g1);
    }
  }
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (live && l == 0) dz[row] = g * (1.f - g) * s;
}

// ------------------------------------------------------------------------------------------------ sum of up-sample adjoints
struct UpSumBwdArgs {
  const float* p[3];
  long ld[3];
  int k[3];
};

template <int J>
__global__ __launch_bounds__(256) void upsample_sum_bwd_kernel(UpSumBwdArgs a, float* __restrict__ dx, long lddx, int NT, int H,
                                                               int W, int CV, int accumulate) {
  const long total = (long)NT * H * W * CV;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;      // one dx vector per thread (fewer than 2^31, host-checked)
  if (idx < total) {
    const unsigned ui = (unsigned)idx;
    const int cv = (int)(ui % (unsigned)CV);
    unsigned pos = ui / (unsigned)CV;
    const int w = (int)(pos % (unsigned)W);
    pos /= (unsigned)W;
    const int h = (int)(pos % (unsigned)H);
    const long nt = (long)(pos / (unsigned)H);
    float* d = dx + ((nt * H + h) * W + w) * lddx + cv * 4;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (accumulate) o = *reinterpret_cast<const float4*>(d);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      float4 t;
      if (a.k[j] == 2) t = up_gather<2, false>(a.p[j], a.ld[j], nullptr, 0, nt, h, w, H, W, cv);
      else if (a.k[j] == 4) t = up_gather<4, false>(a.p[j], a.ld[j], nullptr, 0, nt, h, w, H, W, cv);
      else t = up_gather<8, false>(a.p[j], a.ld[j], nullptr, 0, nt, h, w, H, W, cv);
      o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
    }
    *reinterpret_cast<float4*>(d) = o;
  }
}

}  // namespace mspi

using namespace mspi;

extern "C" int mspi_rowgate_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gate, float* dx,
                                int64_t lddx, float* dz, int64_t M, int32_t C, mspi_stream_t stream) {
  MSPI_REQUIRE(dy && x && gate && dz, "mspi_rowgate_bwd: null argument (only dx may be NULL)");
  MSPI_REQUIRE(M > 0 && C > 0, "mspi_rowgate_bwd: bad extent");
  MSPI_REQUIRE((C & 3) == 0 && (lddy & 3) == 0 && lddy >= C && (ldx & 3) == 0 && ldx >= C && aligned16(dy) && aligned16(x),
               "mspi_rowgate_bwd: C/ld must be multiples of 4 with ld >= C, pointers 16-B aligned");
  MSPI_REQUIRE(!dx || ((lddx & 3) == 0 && lddx >= C && aligned16(dx)),
               "mspi_rowgate_bwd: C/ld must be multiples of 4 with ld >= C, pointers 16-B aligned");
  const int CV = C / 4;
  const hipStream_t st = (hipStream_t)stream;
#define MSPI_RGB(LL)                                                                                                          \
  do {                                                                                                                        \
    const long blocks = (M + (256 / LL) - 1) / (256 / LL);                                                                    \
    MSPI_REQUIRE(blocks < (1L << 31), "mspi_rowgate_bwd: more than 2^31 workgroups");                                         \
    hipLaunchKernelGGL((rowgate_bwd_kernel<LL>), dim3((unsigned)blocks), dim3(256), 0, st, dy, (long)lddy, x, (long)ldx, gate, \
                       dx, (long)lddx, dz, (long)M, CV);                                                                      \
  } while (0)
  // the largest power of two that leaves no lane of a row idle, at most 16 (192 channels: 16 lanes x 3 vectors, 4 rows a wave)
  if (CV >= 16) MSPI_RGB(16);
  else if (CV >= 8) MSPI_RGB(8);
  else if (CV >= 4) MSPI_RGB(4);
  else if (CV >= 2) MSPI_RGB(2);
  else MSPI_RGB(1);
#undef MSPI_RGB
  return check_launch("mspi_rowgate_bwd");
}

extern "C" int mspi_upsample_sum_bwd(const float* const* dys, const int64_t* lddy, const int32_t* factors, int32_t J, float* dx,
                                     int64_t lddx, int32_t NT, int32_t H, int32_t W, int32_t C, int32_t accumulate,
                                     mspi_stream_t stream) {
  MSPI_REQUIRE(dys && lddy && factors && dx, "mspi_upsample_sum_bwd: null argument");
  MSPI_REQUIRE(J >= 1 && J <= 3, "mspi_upsample_sum_bwd: 1 to 3 sources");
  MSPI_REQUIRE(NT > 0 && H > 0 && W > 0 && C > 0, "mspi_upsample_sum_bwd: bad extent");
  MSPI_REQUIRE((C & 3) == 0 && (lddx & 3) == 0 && lddx >= C && aligned16(dx),
               "mspi_upsample_sum_bwd: C/ld must be multiples of 4 with ld >= C, pointers 16-B aligned");
  UpSumBwdArgs a = {};
  for (int j = 0; j < J; ++j) {
    const int k = factors[j];
    MSPI_REQUIRE(k == 2 || k == 4 || k == 8, "mspi_upsample_sum_bwd: every factor must be 2, 4 or 8");
    MSPI_REQUIRE(dys[j] && (lddy[j] & 3) == 0 && lddy[j] >= C && aligned16(dys[j]),
                 "mspi_upsample_sum_bwd: C/ld must be multiples of 4 with ld >= C, pointers 16-B aligned");
    MSPI_REQUIRE((long)NT * H * k * W * k * (C / 4) < (1L << 31), "mspi_upsample_sum_bwd: more than 2^31 source vectors");
    a.p[j] = dys[j];
    a.ld[j] = (long)lddy[j];
    a.k[j] = k;
  }
  const long total = (long)NT * H * W * (C / 4);
  MSPI_REQUIRE(total < (1L << 31), "mspi_upsample_sum_bwd: more than 2^31 destination vectors");
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (J == 1) hipLaunchKernelGGL((upsample_sum_bwd_kernel<1>), grid, block, 0, st, a, dx, (long)lddx, NT, H, W, C / 4, accumulate);
  else if (J == 2) hipLaunchKernelGGL((upsample_sum_bwd_kernel<2>), grid, block, 0, st, a, dx, (long)lddx, NT, H, W, C / 4, accumulate);
  else hipLaunchKernelGGL((upsample_sum_bwd_kernel<3>), grid, block, 0, st, a, dx, (long)lddx, NT, H, W, C / 4, accumulate);
  return check_launch("mspi_upsample_sum_bwd");
}
