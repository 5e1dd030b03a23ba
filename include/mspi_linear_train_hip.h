/*
 * mspi_linear_train_hip.h -- weight and bias gradient of an nn.Linear layer y = x W^T + b over rows: the four linear layers of
 * the SyncBlock's transformer Blocks (qkv 512 -> 1536, proj 512 -> 512, fc1 512 -> 2048, fc2 2048 -> 512) and the vis_proj in
 * front of them (C4 -> 512, C4 in {192, 768, 784, 1024, 2048} by backbone).
 *
 * Why a seventh header: for the reason mspi_block_train_hip.h gives -- the symbol sets of the six older headers are pinned by
 * tables inside existing test files.  The entry points below live in the SAME library (csrc/linear_wgrad.hip) and are held to
 * the same three contracts (declared = exported = bound; capture-safe launches; non-finite data propagates) by
 * tests/test_sync_tokens_train.py.  The Python binding mirrors the split (_lib._LINEAR_SIGNATURES / LINEAR_EXPORTS).
 * MSPI_ABI_VERSION is unchanged.
 *
 * Conventions: those of mspi_block_train_hip.h -- fp32 device memory owned by the caller, 0 or a negative MSPI_E* code with the
 * reason in mspi_last_error(), launches on the caller's stream only, no allocation, memcpy, memset, synchronisation, device
 * query or mutable static (graph-capture safe, the first call included).  No float read-modify-write on shared memory cells: a
 * workgroup writes one record of its block to the caller's workspace `ws`, and a second launch adds the records in slice
 * order, so every result is bitwise repeatable.  `ws` need not be initialised.  Non-finite data: PROPAGATE.
 */
#ifndef MSPI_LINEAR_TRAIN_HIP_H
#define MSPI_LINEAR_TRAIN_HIP_H

#include "mspi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dW[n][k] = sum_r dy[r][n] x[r][k],   db[n] = sum_r dy[r][n]   (db may be NULL: no bias)
 * x [M][K] with row stride ldx, dy [M][N] with row stride lddy, both read where they lie (a column range of a wider buffer, the
 * [rows][3][4][128] slab mspi_attn_bwd writes); dW dense [N][K], the layout of nn.Linear.weight; db [N].
 * Supported: 0 < M < 2^31; N a multiple of 32, K a multiple of 4, both at most 4096 (the last 32-column tile of K may be
 * ragged); row strides multiples of 4 floats, >= the width; x, dy, dW, db and ws 16-byte aligned.  Anything else is refused
 * with the reason in mspi_last_error().
 * v_mfma_f32_32x32x2_f32 with the rows as the contraction, so both operands are read along their rows as they lie: a k-ordered
 * fmaf chain per slice.  A workgroup owns a 128 x 128 block of dW (its four waves 2 x 2 tiles of 32 x 32 each) and one slice of
 * the rows; it stages panels of 32 rows of dy and x through two LDS buffers, the next panel's global loads in flight under the
 * current panel's MFMAs, and writes one record to ws; the second launch adds the records in slice order.
 * The slices are a pure function of (M, N, K), no device query, so the bits do not depend on the machine:
 *     blocks = ceil(N / 128) * ceil(K / 128)
 *     want   = max(1, 512 / blocks)                      integer division: about two workgroups a CU on 256 CUs
 *     L      = max(128, 32 * ceil(ceil(M / want) / 32))  rows per slice, whole panels (and at most 2^31 - 32)
 *     S      = ceil(M / L)                               slices; the last may be short
 * mspi_linear_wgrad_ws_bytes: S * (N * K + N) * 4, host arithmetic, 0 for an (M, N, K) the launch refuses.
 * mspi_linear_wgrad_variant (host only): L, or -1 for exactly what the launch refuses of x, dy and the extents, the reason in
 * mspi_last_error().
 * Rows past M (the odd row of the 2-row MFMA step, the tail of a panel, the tail of the last slice) and columns past K are
 * selected to zero: never read, and never multiplied by zero.
 * A NaN or Inf in x[r][k] reaches dW[:, k] and never db; one in dy[r][n] reaches dW[n, :] and db[n].  A non-finite stored
 * output sets the status word (mspi_set_status_word). */
size_t mspi_linear_wgrad_ws_bytes(int64_t M, int32_t N, int32_t K);
int mspi_linear_wgrad_variant(const void* x, int64_t ldx, const void* dy, int64_t lddy, int64_t M, int32_t N, int32_t K);
int mspi_linear_wgrad(const float* x, int64_t ldx, const float* dy, int64_t lddy, float* dW, float* db, void* ws, int64_t M,
                      int32_t N, int32_t K, mspi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MSPI_LINEAR_TRAIN_HIP_H */
