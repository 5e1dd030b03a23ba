/*
 * mspi_x3d_train_hip.h -- backward entry points of one stride-1 X3D residual block (SlowFast/resnet_helper.py:213-360 and
 * 490-616 upstream) with its three BatchNorm layers on BATCH statistics:
 *   z_a = a(x); t = relu(bn_a(z_a)); v0 = b(t) depthwise (3,3,3); v = bn_b(v0); g = sigmoid(fc2(relu(fc1(mean_THW(v)))))
 *   s = swish(v g); z_c = c(s); y = relu(x + bn_c(z_c)).
 * The pieces no other header has: the weight gradient of the 3x3x3 depthwise conv, the BatchNorm apply with the SE gate, the
 * residual and Swish in one pass, the backward of that gate-and-Swish, the squeeze-excite MLP forward and backward on [N][C]
 * rows, and the residual's skip path under the ReLU mask.
 *
 * Why a ninth header: for the reason mspi_block_train_hip.h gives -- the symbol sets of the eight older headers are pinned by
 * tables inside existing test files.  The entry points below live in the SAME library (csrc/x3d_bwd.hip) and are held to the
 * same three contracts (declared = exported = bound; capture-safe launches; non-finite data propagates) by
 * tests/test_x3d_block_train.py.  The Python binding mirrors the split (_lib._X3D_SIGNATURES / X3D_EXPORTS).
 * MSPI_ABI_VERSION is unchanged.
 *
 * Conventions: those of mspi_block_train_hip.h -- fp32 device memory owned by the caller, 0 or a negative MSPI_E* code with the
 * reason in mspi_last_error(), launches on the caller's stream only, no allocation, memcpy, memset, synchronisation, device
 * query or mutable static (graph-capture safe, the first call included).  No float read-modify-write on shared memory cells:
 * every output element is written by exactly one thread, and a sum that crosses a workgroup goes through the caller's
 * workspace `ws` as records, which a second launch adds in record order, so every result is bitwise repeatable.  `ws` need not
 * be initialised.  Non-finite data: PROPAGATE (mspi_hip.h at mspi_set_status_word).
 *
 * What the block's backward takes from elsewhere: mspi_bn_stats / _apply / _bwd (mspi_hip.h) over channel slices of at most 192,
 * mspi_linear_wgrad (mspi_linear_train_hip.h) for the two pointwise convs, mspi_conv_fwd on transposed packs at MSPI_PREC_F32
 * for their data gradients, mspi_dwconv_fwd on the flipped taps for the depthwise conv's, mspi_mean_rows and
 * mspi_mean_rows_bwd (mspi_contrast_train_hip.h) around the squeeze-excite MLP.
 */
#ifndef MSPI_X3D_TRAIN_HIP_H
#define MSPI_X3D_TRAIN_HIP_H

#include "mspi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weight (and, where db is not NULL, bias) gradient of a depthwise (3,3,3) conv with padding (1,1,1), stride 1, "same" extent:
 *   dW[c][kt][kh][kw] = sum_{n,t,h,w} dy[n,t,h,w,c] x[n,t+kt-1,h+kh-1,w+kw-1,c],   db[c] = sum dy[n,t,h,w,c],
 * positions outside the frame counting as zeros (a NaN in dy beside the frame's edge therefore reaches the taps that look
 * outside: NaN * 0).  x and dy are rows [N T H W] read by their row strides d->ldx and d->ldy (>= C, multiples of 4), so a
 * channel slice of a wider buffer works; dW is in the parameter's layout [C][1][3][3][3], db [C].  C % 4 == 0, C <= 4096,
 * fewer than 2^31 rows; x, dy, dW, db and ws 16-byte aligned.  mspi_dwconv_wgrad (mspi_block_train_hip.h) refuses this kernel
 * shape and existing tests hold it to that: hence a new entry point.
 *
 * Plan.  A LINE is the W positions of one (n, t, h); there are L = N T H of them, numbered in that order.  A workgroup owns a
 * BAND of consecutive output lines and a group of at most 28 channel quads; thread (q, r) owns channel quad q and the
 * (kt, kh) = (r / 3, r % 3) pair, 9 pairs in threadIdx.y.  For output line (n, t, h) it reads input line (n, t+kt-1, h+kh-1)
 * (zeros outside the frame), slides a 3-wide register window of x along W, loads one x and one dy vector per step and does 3
 * FMAs on four channels into three float4 accumulators.  It writes its three rows of the band's record [28][C]: the 27 taps,
 * then db (by the centre pair).  A second launch adds the records in band order and writes dW transposed into [C][27].
 * The band rule, a pure function of the descriptor:
 *   band = max(1, ceil(L / 256)) lines,   records = ceil(L / band)  (<= 256),
 * so the X3D-L maps give 224 records at stage 5 (8 clips: 896 lines of 12, band 4; 2 clips: 224 lines, band 1) and 256 / 224
 * at stage 4 (1792 lines of 24, band 7; 448 lines, band 2), times ceil(C / 4 / 28) channel groups of workgroups.
 * mspi_dwconv3_wgrad_ws_bytes: records * 28 * C * 4, host arithmetic, 0 for a descriptor the launch refuses;
 * mspi_dwconv3_wgrad_supported: 1 or 0 for the descriptor alone, the reason in mspi_last_error(). */
int mspi_dwconv3_wgrad_supported(const MspiDwConvDesc* d);
size_t mspi_dwconv3_wgrad_ws_bytes(const MspiDwConvDesc* d);
int mspi_dwconv3_wgrad(const MspiDwConvDesc* d, const float* x, const float* dy, float* dW, float* db /* may be NULL */, void* ws,
                       mspi_stream_t stream);

/* y[r][c] = act(res[r][c] + gate[n(r)][c] (gamma_c (x[r][c] - mean_c) rstd_c + beta_c)) over M rows of C channels, n(r) = r / R
 * with R the rows of one sample (M % R == 0).  gate [M / R][C] dense or NULL (1), res (row stride ldr) or NULL (0), act
 * MSPI_ACT_RELU, MSPI_ACT_SWISH (w sigmoid(w), the division-free sigmoid of the inference kernels) or MSPI_ACT_NONE.  One pass:
 * it serves s = swish(g bn_b(v0)) and y = relu(x + bn_c(z_c)) of the block, and the backward's recompute of s.  y may be x or
 * res (same pointer and stride).  0 < M < 2^31, C % 4 == 0, 0 < C <= 4096 (the 192-channel cap of mspi_bn_apply does not
 * apply); row strides multiples of 4, >= C; every pointer 16-byte aligned.  The ReLU keeps a NaN. */
int mspi_bn_gate_act_fwd(const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         const float* gate, const float* res, int64_t ldr, float* y, int64_t ldy, int64_t M, int32_t R, int32_t C,
                         int32_t act, mspi_stream_t stream);

/* Backward of s = swish(w), w = v g, v = gamma (v0 - mean) rstd + beta, g = gate[n][c] (NULL: 1), for the gradient ds: v, w
 * and sigma = sigmoid(w) are computed again from the pre-norm v0,
 *   dw = ds sigma (1 + w (1 - sigma)),   dv[r][c] = dw g,   dgate[n][c] = sum_{rows of sample n} dw v   (with a gate only).
 * N samples of R rows.  A workgroup owns 32 consecutive rows of one sample and 64 channel quads; its share of dgate leaves as
 * one record [C] per 32-row band, and a second launch adds a sample's ceil(R / 32) records in band order.
 * mspi_gate_swish_bwd_ws_bytes(N, R, C): N ceil(R / 32) C 4, host arithmetic, 0 for what the launch refuses; without a gate
 * dgate and ws may be NULL.  dv may be ds (same pointer and stride).  0 < N < 65536, 0 < R, N R < 2^31, C % 4 == 0,
 * 0 < C <= 4096; row strides multiples of 4, >= C; every pointer 16-byte aligned. */
size_t mspi_gate_swish_bwd_ws_bytes(int32_t N, int32_t R, int32_t C);
int mspi_gate_swish_bwd(const float* ds, int64_t ldds, const float* v0, int64_t ldv, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, const float* gate, float* dv, int64_t lddv, float* dgate, void* ws,
                        int32_t N, int32_t R, int32_t C, mspi_stream_t stream);

/* The squeeze-excite MLP (SlowFast/resnet_helper.py:27-73) behind a BatchNorm on batch statistics, on N rows of C channels:
 * from pool0[n][c] = mean_THW(v0) (mspi_mean_rows) and the norm's vectors,
 *   p = gamma (pool0 - mean) rstd + beta   (the mean of a per-channel affine map is the affine map of the mean),
 *   h = relu(W1 p + b1),   gate = sigmoid(W2 h + b2),
 * W1 [F][C], b1 [F], W2 [C][F], b2 [C] in the nn.Conv3d layouts (1x1x1 kernels, dense).  Stores p [N][C], h [N][F] and
 * gate [N][C].  One workgroup a sample; every sum has one owner (a wave's lanes in a fixed tree, or one thread in index order).
 * 0 < N < 65536, C % 4 == 0, 0 < C <= 4096, 0 < F <= 64; every pointer 16-byte aligned. */
int mspi_se_train_fwd(const float* pool0, const float* mean, const float* rstd, const float* gamma, const float* beta,
                      const float* w1, const float* b1, const float* w2, const float* b2, float* p, float* h, float* gate,
                      int32_t N, int32_t C, int32_t F, mspi_stream_t stream);

/* Its backward from dgate [N][C], with the forward's p, h and gate:
 *   dz2 = dgate gate (1 - gate),  dh = W2^T dz2,  dz1 = dh where h > 0 (0 elsewhere),  dp = W1^T dz1        [N][C]
 *   dW2[c][f] = sum_n dz2[n][c] h[n][f],  db2 = sum_n dz2,  dW1[f][c] = sum_n dz1[n][f] p[n][c],  db1 = sum_n dz1,
 * the samples added in index order.  The first launch (a workgroup a sample) writes dp and the sample's record dz2 | dz1
 * [C + F] to ws; the second gives every element of the four gradients one thread.  mspi_se_train_bwd_ws_bytes(N, C, F):
 * N (C + F) 4, 0 for what the launch refuses.  mspi_mean_rows_bwd(dp, dv, accumulate) then adds dp / R to every row of the
 * sample, which completes dv.  Limits as mspi_se_train_fwd. */
size_t mspi_se_train_bwd_ws_bytes(int32_t N, int32_t C, int32_t F);
int mspi_se_train_bwd(const float* dgate, const float* gate, const float* h, const float* p, const float* w1, const float* w2,
                      float* dw1, float* db1, float* dw2, float* db2, float* dp, void* ws, int32_t N, int32_t C, int32_t F,
                      mspi_stream_t stream);

/* dx[r][c] += (y[r][c] > 0 ? g[r][c] : 0): the skip path of y = relu(x + f(x)), the y > 0 select of mspi_bn_bwd.  M rows of C
 * channels; 0 < M < 2^31, C % 4 == 0, C > 0; row strides multiples of 4, >= C; every pointer 16-byte aligned. */
int mspi_relu_mask_add(float* dx, int64_t lddx, const float* g, int64_t ldg, const float* y, int64_t ldy, int64_t M, int32_t C,
                       mspi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MSPI_X3D_TRAIN_HIP_H */
