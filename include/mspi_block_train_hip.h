/*
 * mspi_block_train_hip.h -- backward entry points of the ConvNextBlock at the end of each lateral (model/model_utils.py:306-354
 * upstream): dw(7,1,1) -> dw(1,7,7) -> channel LayerNorm -> 1x1x1 (x4) -> GELU -> 1x1x1 -> + input.
 *
 * Why a third header: the symbol sets of mspi_hip.h and of mspi_train_hip.h are pinned, name by name, by tables inside existing
 * test files (mspi_train_hip.h says which), and a change that adds kernels does not edit existing tests.  The entry points
 * below live in the SAME library (csrc/block_bwd.hip), follow the same conventions and are held to the same three contracts
 * (declared = exported = bound; capture-safe launches; non-finite data propagates) by tests/test_lateral_train.py.  The Python
 * binding mirrors the split (_lib._BLOCK_SIGNATURES / BLOCK_EXPORTS).  MSPI_ABI_VERSION is unchanged.
 *
 * Conventions: those of mspi_hip.h -- fp32 device memory owned by the caller, channels-last rows with a row stride in floats,
 * 0 or a negative MSPI_E* code with the reason in mspi_last_error(), launches on the caller's stream only, no allocation,
 * memcpy, memset, synchronisation or mutable static (graph-capture safe, the first call included).  No float atomics: a sum
 * that crosses a workgroup goes through the caller's workspace `ws` as one record per workgroup, and a second launch adds the
 * records in a fixed order, so every result is bitwise repeatable.  `ws` need not be initialised.  Non-finite data: PROPAGATE.
 *
 * What the block's backward takes from elsewhere: the data gradients of the two depthwise convs are mspi_dwconv_fwd on the
 * flipped taps (padding 3 under kernel 7 is symmetric), the weight gradients of the two 1x1x1 convs mspi_conv_wgrad_wide_fwd
 * on 192-channel slices, their data gradients mspi_conv_fwd on transposed packs at MSPI_PREC_F32.
 */
#ifndef MSPI_BLOCK_TRAIN_HIP_H
#define MSPI_BLOCK_TRAIN_HIP_H

#include "mspi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of g = GELU(z) (erf form, the arithmetic of MSPI_ACT_GELU), element-wise on rows [M][C]:
 *   g  = z Phi(z)                          the forward's activation again: the operand of the second conv's weight gradient
 *   dz = dg (Phi(z) + z phi(z))
 * g may be NULL (not stored; ldg is then not read) or z itself; dz may be dg: a thread stores only the vector it has loaded.
 * C % 4 == 0, every row stride a multiple of 4 and >= C, every pointer 16-byte aligned, M < 2^31.
 * A NaN in z or dg makes dz non-finite at that position, one in z also g; z = +-Inf gives a NaN (Inf * 0), as torch does. */
int mspi_gelu_bwd(const float* z, int64_t ldz, const float* dg, int64_t lddg, float* g /*or NULL*/, int64_t ldg, float* dz,
                  int64_t lddz, int64_t M, int32_t C, mspi_stream_t stream);

/* Backward of y = gamma x^ + beta, x^ = (x - mean) rstd over the C channels of each row (nn.LayerNorm, biased variance):
 *   dx     = rstd (dy gamma - mean_c(dy gamma) - x^ mean_c(dy gamma x^))
 *   dgamma = sum_rows dy x^,   dbeta = sum_rows dy
 * The forward saves nothing: mean and rstd are computed again from x, in the order of mspi_layernorm_fwd (same lanes, same
 * tree), so x^ has the forward's bits.  A row's sums stay inside the 16 lanes that own it; the column sums go through ws
 * (mspi_layernorm_bwd_ws_bytes(M, C) bytes, 0 = refused) as one record [dbeta | dgamma] per 256 rows.  dx may be dy.
 * C % 4 == 0 and C <= 256, row strides multiples of 4 and >= C, pointers 16-byte aligned, 0 < M < 2^31, eps >= 0. */
size_t mspi_layernorm_bwd_ws_bytes(int64_t M, int32_t C);
int mspi_layernorm_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* gamma, float eps, float* dx,
                       int64_t lddx, float* dgamma, float* dbeta, void* ws, int64_t M, int32_t C, mspi_stream_t stream);

/* Weight and bias gradient of mspi_dwconv_fwd for the forward's descriptor d (d->ldx: row stride of x, d->ldy: of dy):
 *   dW[tap][c] = sum_p dy[p][c] x[p + tap - pad][c]   (x is 0 outside the frame),   db[c] = sum_p dy[p][c]
 * dW is [kT*kH*kW][C] tap-major, the layout of the forward's w; db [C].  Supported: stride 1 and "same" padding with kernel
 * (7,1,1) (pad (3,0,0)) or (1,7,7) (pad (0,3,3)), C % 4 == 0; anything else is refused with the reason in mspi_last_error()
 * (mspi_dwconv_wgrad_supported: 1 / 0, host only).  A thread owns four channels and one kernel row and slides a 7-wide register
 * window along the kernel's axis; a workgroup owns a band of lines of one frame and writes one record [taps + 1][C] to ws
 * (mspi_dwconv_wgrad_ws_bytes(d) bytes, 0 = refused).  act is not read: dy is the gradient in front of any activation. */
int mspi_dwconv_wgrad_supported(const MspiDwConvDesc* d);
size_t mspi_dwconv_wgrad_ws_bytes(const MspiDwConvDesc* d);
int mspi_dwconv_wgrad(const MspiDwConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                      mspi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MSPI_BLOCK_TRAIN_HIP_H */
