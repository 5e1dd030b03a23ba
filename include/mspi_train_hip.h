/*
 * mspi_train_hip.h -- training entry points of libmspi_hip.so that are declared apart from mspi_hip.h.
 *
 * Why a second header: the symbol set of mspi_hip.h is pinned, name by name, by tables inside three test files
 * (tests/test_capi_host.py, tests/test_launch_ledger.py, tests/test_nonfinite_ledger.py), and a change that adds kernels does
 * not edit existing tests.  The entry points below live in the SAME library, follow the same conventions and are held to the
 * same three contracts (declared = exported = bound; capture-safe launches; non-finite data propagates) by a ledger of their
 * own, tests/test_fusion_train.py.  The Python binding mirrors the split (_lib._TRAIN_SIGNATURES / TRAIN_EXPORTS).
 * MSPI_ABI_VERSION is unchanged: nothing declared in mspi_hip.h has moved.  Folding the two headers and the ledgers' tables
 * together is a later change.
 *
 * Conventions: those of mspi_hip.h -- fp32 device memory owned by the caller, channels-last rows with a row stride in floats,
 * 0 or a negative MSPI_E* code with the reason in mspi_last_error(), launches on the caller's stream only, no allocation,
 * memcpy, synchronisation or mutable static (graph-capture safe, the first call included); host arrays are read during the
 * call.  Both entry points are free of float atomics and bitwise repeatable.  Non-finite data: PROPAGATE.
 */
#ifndef MSPI_TRAIN_HIP_H
#define MSPI_TRAIN_HIP_H

#include "mspi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of the SA gate y = x * m + x with m = sigmoid(z) per row (model/model_utils.py:164, 167-170; forward:
 * mspi_rowgate, which takes m from the sigmoid epilogue of the conv in front of it):
 *   dx[r][c] = dy[r][c] * (1 + gate[r])
 *   dz[r]    = gate[r] * (1 - gate[r]) * sum_c dy[r][c] * x[r][c]      the gradient of the PRE-sigmoid logit
 * x is the UNGATED input of the forward, gate [M] the sigmoid it multiplied by.  One pass: every dy and x element is read
 * once.  The row's sum runs over the lanes that own the row in a fixed order.  dx == NULL skips the store (lddx is then not
 * read); dx may be dy.  C % 4 == 0, every row stride a multiple of 4 and >= C, dy, x and dx 16-byte aligned.
 * A NaN or Inf in dy, x or gate makes dz of that row non-finite, one in dy or gate also dx at that position. */
int mspi_rowgate_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gate, float* dx /*or NULL*/,
                     int64_t lddx, float* dz, int64_t M, int32_t C, mspi_stream_t stream);

/* Adjoint of mspi_upsample_sum_fwd, the top-down sums of model/model_utils.py:566-570:
 *   dx[NT][H][W][C] (= | +=) sum_{j < J} up_{factors[j]}^T(dys[j])
 * dys[j] is [NT][H * factors[j]][W * factors[j]][C] with row stride lddy[j]; J <= 3, every factor 2, 4 or 8; source
 * coordinates and edge clamping are those of mspi_upsample_fwd.  Gather form: one thread per dx vector visits the cells that
 * tap it in a fixed order, j ascending, each term with the arithmetic of mspi_upsample_bwd (act = MSPI_ACT_NONE), so J = 1
 * without accumulate gives that entry point's bits.  dys / lddy / factors are host arrays of J entries, read during the call.
 * C % 4 == 0, row strides multiples of 4 and >= C, every pointer 16-byte aligned. */
int mspi_upsample_sum_bwd(const float* const* dys, const int64_t* lddy, const int32_t* factors, int32_t J, float* dx,
                          int64_t lddx, int32_t NT, int32_t H, int32_t W, int32_t C, int32_t accumulate, mspi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MSPI_TRAIN_HIP_H */
