/*
 * mspi_contrast_train_hip.h -- backward entry points of the contrastive head (model/model_utils.py:545-552 upstream): the mean
 * over each modality's tokens, projector (Linear-LN-ReLU x2, Linear-LN) and predictor (Linear-LN-ReLU, Linear) on M = B rows,
 * and loss_av = 0.5 mean -cos(p_vis, z_aud) + 0.5 mean -cos(p_aud, z_vis) with z detached.
 *
 * Why an eighth header: for the reason mspi_block_train_hip.h gives -- the symbol sets of the seven older headers are pinned by
 * tables inside existing test files.  The entry points below live in the SAME library (csrc/contrast_bwd.hip) and are held to
 * the same three contracts (declared = exported = bound; capture-safe launches; non-finite data propagates) by
 * tests/test_sync_train.py.  The Python binding mirrors the split (_lib._CONTRAST_SIGNATURES / CONTRAST_EXPORTS).
 * MSPI_ABI_VERSION is unchanged.
 *
 * Conventions: those of mspi_block_train_hip.h -- fp32 device memory owned by the caller, 0 or a negative MSPI_E* code with the
 * reason in mspi_last_error(), launches on the caller's stream only, no allocation, memcpy, memset, synchronisation, device
 * query or mutable static (graph-capture safe, the first call included).  No float read-modify-write on shared memory cells:
 * every output element is written by exactly one workgroup, and a sum that crosses a workgroup goes through the caller's
 * workspace `ws` as one record per workgroup, which a second launch adds in record order, so every result is bitwise
 * repeatable.  `ws` need not be initialised.  Non-finite data: PROPAGATE; a non-finite stored output also sets the status word
 * (mspi_set_status_word).
 *
 * What the head's backward takes from elsewhere: the weight gradients of its ten linear layers from mspi_linear_wgrad
 * (mspi_linear_train_hip.h), their data gradients from mspi_conv_fwd on transposed packs at MSPI_PREC_F32.
 */
#ifndef MSPI_CONTRAST_TRAIN_HIP_H
#define MSPI_CONTRAST_TRAIN_HIP_H

#include "mspi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gradient of mspi_neg_cosine(p, z, out, N, C, scale, .) with respect to p for the gradient g[0] of out (a DEVICE scalar:
 * nothing synchronises); z is a constant (the caller detaches it).  With np = max(|p_n|, 1e-8), nz = max(|z_n|, 1e-8), the
 * forward's clamps,
 *   dp[n,:] = -g[0] scale / N ( z_n / (np nz) - (p_n . z_n) p_n / (np^3 nz) ),   the second term only where |p_n| >= 1e-8
 * (below that the clamp holds np constant).  p, z, dp dense [N][C]; dp may not overlap p or z.  One workgroup a row; the row's
 * three sums are taken in the forward kernel's order.  0 < N < 2^31, C a multiple of 4, C > 0; pointers 16-byte aligned
 * (g: 4-byte).  A NaN or Inf in row n of p or z stays inside row n of dp; one in g reaches every row. */
int mspi_neg_cosine_bwd(const float* p, const float* z, const float* g, float* dp, int32_t N, int32_t C, float scale,
                        mspi_stream_t stream);

/* Backward of y = act(layernorm(x) gamma + beta) over the C channels of each of M rows, act = ReLU where y is given and the
 * identity where y is NULL: with d = dy where y > 0 (y NULL: everywhere), 0 where y <= 0 (a NaN in y stays a NaN),
 *   dx = rstd (d gamma - mean_c(d gamma) - x^ mean_c(d gamma x^)),   dgamma = sum_rows d x^,   dbeta = sum_rows d.
 * mspi_layernorm_bwd stops at 256 channels and mspi_layernorm_bwd_wide at 512, neither has the mask; this one takes
 * 0 < C <= 2048, C % 4 == 0, 0 < M < 2^31.  One wave a row: the row sits in registers (8 float4 a lane at 2048) and the two row
 * sums stay inside the wave; mean and rstd are computed again from x (two passes, eps >= 0).  A workgroup is one wave and
 * walks 8 rows; its dbeta | dgamma go to ws as one record [2 C], and a second launch adds the ceil(M / 8) records in record
 * order.  mspi_layernorm_act_bwd_ws_bytes(M, C): ceil(M / 8) * 2 C * 4, host arithmetic, 0 for an (M, C) the launch refuses.
 * dx may be dy (same pointer and stride).  Row strides multiples of 4 floats and >= C; x, dy, y, gamma, dx, dgamma, dbeta and ws
 * 16-byte aligned.  A NaN or Inf in row r of x, dy or y stays inside row r of dx and reaches the columns of dgamma / dbeta it
 * feeds; one in gamma[c] reaches every row of dx. */
size_t mspi_layernorm_act_bwd_ws_bytes(int64_t M, int32_t C);
int mspi_layernorm_act_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* y, int64_t ldy,
                           const float* gamma, float eps, float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws,
                           int64_t M, int32_t C, mspi_stream_t stream);

/* The adjoint of mspi_mean_rows: dx[n][r][:] (+)= g[n][:] / R for the R rows of each of N samples, 16-byte stores.  g dense
 * [N][C]; row r of sample n of dx lies at dx + n sample_stride + r ldx, so dx may be a row range of a wider slab (the visual or
 * the audio tokens of [B][Rv+Ra][512]); rows outside the range are not touched.  accumulate != 0 adds to what dx holds.
 * 0 < N < 65536, 0 < R < 2^31, C a multiple of 4, C > 0; ldx and sample_stride multiples of 4 floats, ldx >= C,
 * sample_stride >= R ldx where N > 1; g and dx 16-byte aligned. */
int mspi_mean_rows_bwd(const float* g, float* dx, int64_t ldx, int64_t sample_stride, int32_t N, int32_t R, int32_t C,
                       int32_t accumulate, mspi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MSPI_CONTRAST_TRAIN_HIP_H */
