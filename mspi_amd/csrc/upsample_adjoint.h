// Gather form of the bilinear up-sample's adjoint, shared by mspi_upsample_bwd (readout_bwd.hip) and mspi_upsample_sum_bwd
// (fusion_bwd.hip): the same taps, weights and fmaf order in both, so one source's gradient has the same bits from either.
#pragma once
#include "common.h"

namespace mspi {

// Source cell (h, w) collects the destination cells whose two taps per axis (h0, h1 = min(h0 + 1, H - 1), weights 1 - lh, lh;
// align_corners=False, clamped at 0) include it: for an even factor k those are ho in [k h - k / 2, k h + 3 k / 2), clipped to
// the image.  Factors 2, 4, 8 make every weight a dyadic fraction.
template <int K>
__device__ __forceinline__ void up_axis_weights(int h, int H, float (&wt)[2 * K]) {
  const float inv = 1.f / (float)K;
#pragma unroll
  for (int j = 0; j < 2 * K; ++j) {
    const int ho = K * h - K / 2 + j;
    float f = ((float)ho + 0.5f) * inv - 0.5f;
    f = f < 0.f ? 0.f : f;
    const int h0 = (int)f;
    const int h1 = h0 + (h0 < H - 1 ? 1 : 0);
    const float l = f - (float)h0;
    float v = 0.f;
    if (ho >= 0 && ho < K * H) v = (h0 == h ? 1.f - l : 0.f) + (h1 == h ? l : 0.f);
    wt[j] = v;
  }
}

// sum over the destination cells of dy [NT][H K][W K] (row stride ldy) that tap source cell (nt, h, w), channel vector cv, in a
// fixed order (rows, then columns, ascending).  RELU: cells whose forward output u is <= 0 are skipped.
template <int K, bool RELU>
__device__ __forceinline__ float4 up_gather(const float* __restrict__ dy, long ldy, const float* __restrict__ u, long ldu, long nt,
                                            int h, int w, int H, int W, int cv) {
  const int Ho = H * K, Wo = W * K;
  float wh[2 * K], ww[2 * K];
  up_axis_weights<K>(h, H, wh);
  up_axis_weights<K>(w, W, ww);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int jh = 0; jh < 2 * K; ++jh) {
    const int ho = K * h - K / 2 + jh;
    if (ho < 0 || ho >= Ho) continue;
#pragma unroll
    for (int jw = 0; jw < 2 * K; ++jw) {
      const int wo = K * w - K / 2 + jw;
      if (wo < 0 || wo >= Wo) continue;
      const long row = (nt * Ho + ho) * Wo + wo;
      float4 gv = *reinterpret_cast<const float4*>(dy + row * ldy + cv * 4);
      if (RELU) {
        const float4 uv = *reinterpret_cast<const float4*>(u + row * ldu + cv * 4);
        gv.x = uv.x > 0.f ? gv.x : 0.f; gv.y = uv.y > 0.f ? gv.y : 0.f;
        gv.z = uv.z > 0.f ? gv.z : 0.f; gv.w = uv.w > 0.f ? gv.w : 0.f;
      }
      const float c = wh[jh] * ww[jw];
      acc.x = fmaf(c, gv.x, acc.x); acc.y = fmaf(c, gv.y, acc.y); acc.z = fmaf(c, gv.z, acc.z); acc.w = fmaf(c, gv.w, acc.w);
    }
  }
  return acc;
}

}  // namespace mspi
