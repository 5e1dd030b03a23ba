// Bringing saved saliency maps and dataset annotations to one size on the device (mspi_amd/evaluate.py):
//   mspi_resize_bilinear_fwd   cv2.resize(..., INTER_LINEAR) of utils/compute_saliency_metrics.py:119-122 (prediction -> fixation
//                              map's size) and of avsp_dataloader.py:176 (density -> model size), uint8 or fp32 in, fp32 out
//   mspi_resize_fixation_fwd   avsp_dataloader.py:16-31 resize_fixation: every fixation moves to its rounded scaled coordinate
// Both are memory-bound maps of a few MB; neither allocates, synchronises or copies, and neither uses a float atomic.
// postproc.hip has a resize of its own, fused with a min/max reduction and with fp32 coordinates; its output is pinned by
// tests and it is left alone.
#include "common.h"

namespace mspi {

// Source position of output index d on an axis scaled in -> out, pixel centres aligned:
//   x = (d + 0.5) * in / out - 0.5 = ((2d + 1) * in - out) / (2 * out)
// as an exact integer quotient: i0 = floor(x), and the weight of i0 + 1 is rem / (2 * out) with both integers below 2^24
// (extents <= 2^23, checked on the host), so ONE IEEE fp32 division rounds the exact weight once.  Edges clamp as OpenCV does:
// left of the first centre or at / right of the last one the weight is 0 on the clamped index.
__device__ __forceinline__ void src_coord(int d, int in, int out, int& i0, int& i1, float& w) {
  const long num = (2L * d + 1) * in - out;
  const int den = 2 * out;
  if (num < 0) { i0 = i1 = 0; w = 0.f; return; }
  const long q = num / den;
  if (q >= in - 1) { i0 = i1 = in - 1; w = 0.f; return; }
  i0 = (int)q;
  i1 = i0 + 1;
  w = (float)(int)(num - q * den) / (float)den;
}

// w == 0 returns a itself: the identity resize is then a copy bit for bit (also of -0, inf and NaN samples)
__device__ __forceinline__ float lerp1(float a, float b, float w) { return w == 0.f ? a : (1.f - w) * a + w * b; }

// One lane = 4 consecutive output pixels of one row, stored as one 16-byte vector; the 64 lanes of a wave cover 256
// consecutive outputs, whose sources are two contiguous row segments of the input (row-coalesced reads, L2 serves the reuse
// between the two rows and between neighbouring output rows).  idx runs over N * Ho * ceil(Wo / 4).
template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const T* __restrict__ src, float* __restrict__ dst, long total,
                                                              int H, int W, int Ho, int Wo, int chunks) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long row = idx / chunks;                 // n * Ho + ho
  const int wo = (int)(idx - row * chunks) * 4;
  const long n = row / Ho;
  const int ho = (int)(row - n * Ho);
  int h0, h1;
  float lh;
  src_coord(ho, H, Ho, h0, h1, lh);
  const T* r0 = src + (n * H + h0) * (long)W;
  const T* r1 = src + (n * H + h1) * (long)W;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int x = wo + e < Wo ? wo + e : Wo - 1;   // the lanes of a ragged last chunk recompute the last pixel; not stored
    int w0, w1;
    float lw;
    src_coord(x, W, Wo, w0, w1, lw);
    const float top = lerp1((float)r0[w0], (float)r0[w1], lw);
    const float bot = lerp1((float)r1[w0], (float)r1[w1], lw);
    v[e] = lerp1(top, bot, lh);
  }
  float* o = dst + row * Wo + wo;
  // the real pointer is tested: Wo % 4 != 0 leaves every other row off the 16-byte grid
  if (wo + 4 <= Wo && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int e = 0; e < 4 && wo + e < Wo; ++e) o[e] = v[e];
  }
}

// n floats of zero, 16 bytes per lane where the pointer allows
__global__ __launch_bounds__(256) void zero_fill_kernel(float* __restrict__ y, long n) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  float* p = y + i;
  if (i + 4 <= n && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    *reinterpret_cast<float4*>(p) = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int e = 0; e < 4 && i + e < n; ++e) p[e] = 0.f;
  }
}

// avsp_dataloader.py:23-29 on one coordinate: int(np.round(i * ratio)) with the float64 ratio the reference forms first
// (:18-19), half to even, and the `== extent` step back (the largest product is below extent + 0.5).
__device__ __forceinline__ int fix_coord(int i, double ratio, int extent) {
  const int c = (int)rint((double)i * ratio);
  return c < extent - 1 ? c : extent - 1;
}

// One lane = 4 consecutive input pixels of one row (one 16-byte load where aligned).  A non-zero pixel (np.argwhere: NaN
// counts) stores the constant 1.0f at its target.  Several sources may share a target: the racing stores write the same
// value, so the result does not depend on their order.  Runs after zero_fill_kernel on the same stream.
__global__ __launch_bounds__(256) void fixation_scatter_kernel(const float* __restrict__ fix, float* __restrict__ dst, long total,
                                                               int H, int W, int row, int col, int chunks, double ratio_row,
                                                               double ratio_col) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long r_all = idx / chunks;               // n * H + r
  const int c0 = (int)(idx - r_all * chunks) * 4;
  const long n = r_all / H;
  const int r = (int)(r_all - n * H);
  const float* p = fix + r_all * W + c0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (c0 + 4 <= W && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    for (int e = 0; e < 4 && c0 + e < W; ++e) v[e] = p[e];
  }
  if (!(v[0] != 0.f || v[1] != 0.f || v[2] != 0.f || v[3] != 0.f)) return;     // almost every lane: fixations are sparse
  float* out = dst + (n * row + fix_coord(r, ratio_row, row)) * (long)col;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (v[e] != 0.f) out[fix_coord(c0 + e, ratio_col, col)] = 1.0f;            // c0 + e < W wherever v[e] was loaded
}

}  // namespace mspi

using namespace mspi;

static const int32_t kMaxExtent = 1 << 23;    // src_coord: 2 * extent and the remainder stay exact fp32 integers

extern "C" int mspi_resize_bilinear_fwd(const void* src, int32_t src_is_u8, float* dst, int32_t N, int32_t H, int32_t W,
                                        int32_t Ho, int32_t Wo, mspi_stream_t stream) {
  MSPI_REQUIRE(src && dst, "mspi_resize_bilinear_fwd: null pointer");
  MSPI_REQUIRE(N > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "mspi_resize_bilinear_fwd: zero extent (N %d, %d x %d -> %d x %d)", N, H,
               W, Ho, Wo);
  MSPI_REQUIRE(H <= kMaxExtent && W <= kMaxExtent && Ho <= kMaxExtent && Wo <= kMaxExtent,
               "mspi_resize_bilinear_fwd: extent above 2^23 (%d x %d -> %d x %d)", H, W, Ho, Wo);
  const int chunks = (Wo + 3) / 4;
  const long total = (long)N * Ho * chunks;
  const long blocks = (total + 255) / 256;
  MSPI_REQUIRE(blocks <= 0x7fffffffL, "mspi_resize_bilinear_fwd: %d maps of %d x %d are too many for one launch", N, Ho, Wo);
  hipStream_t s = (hipStream_t)stream;
  if (src_is_u8)
    hipLaunchKernelGGL(resize_bilinear_kernel<unsigned char>, dim3((unsigned)blocks), dim3(256), 0, s,
                       reinterpret_cast<const unsigned char*>(src), dst, total, H, W, Ho, Wo, chunks);
  else
    hipLaunchKernelGGL(resize_bilinear_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const float*>(src),
                       dst, total, H, W, Ho, Wo, chunks);
  return check_launch("mspi_resize_bilinear_fwd");
}

extern "C" int mspi_resize_fixation_fwd(const float* fix, float* dst, int32_t N, int32_t H, int32_t W, int32_t row, int32_t col,
                                        mspi_stream_t stream) {
  MSPI_REQUIRE(fix && dst, "mspi_resize_fixation_fwd: null pointer");
  MSPI_REQUIRE(N > 0 && H > 0 && W > 0 && row > 0 && col > 0, "mspi_resize_fixation_fwd: zero extent (N %d, %d x %d -> %d x %d)", N,
               H, W, row, col);
  const long n_out = (long)N * row * col;
  const long zb = ((n_out + 3) / 4 + 255) / 256;
  const int chunks = (W + 3) / 4;
  const long total = (long)N * H * chunks;
  const long sb = (total + 255) / 256;
  MSPI_REQUIRE(zb <= 0x7fffffffL && sb <= 0x7fffffffL, "mspi_resize_fixation_fwd: %d maps of %d x %d -> %d x %d are too many for one "
               "launch", N, H, W, row, col);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)zb), dim3(256), 0, s, dst, n_out);
  hipLaunchKernelGGL(fixation_scatter_kernel, dim3((unsigned)sb), dim3(256), 0, s, fix, dst, total, H, W, row, col, chunks,
                     (double)row / (double)H, (double)col / (double)W);
  return check_launch("mspi_resize_fixation_fwd");
}
