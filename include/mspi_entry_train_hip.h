/*
 * mspi_entry_train_hip.h -- weight gradient of the laterals' entry convs (model/model_utils.py:440-470 upstream): latlayer_k[0],
 * a 1x1x1 conv C_k -> 192, and where present latlayer_k[1], an (s,1,1) / stride (s,1,1) conv 192 -> 192, which the forward runs
 * composed as ONE conv with kernel == stride along T (autograd.compose_lateral).
 *
 * Why a fourth header: for the reason mspi_block_train_hip.h gives -- the symbol sets of the three older headers are pinned by
 * tables inside existing test files.  The entry points below live in the SAME library (csrc/entry_bwd.hip) and are held to the
 * same three contracts (declared = exported = bound; capture-safe launches; non-finite data propagates) by
 * tests/test_entry_train.py.  The Python binding mirrors the split (_lib._ENTRY_SIGNATURES / ENTRY_EXPORTS).  MSPI_ABI_VERSION
 * is unchanged.
 *
 * Conventions: those of mspi_block_train_hip.h -- fp32 device memory owned by the caller, channels-last rows, 0 or a negative
 * MSPI_E* code with the reason in mspi_last_error(), launches on the caller's stream only, no allocation, memcpy, memset,
 * synchronisation or mutable static (graph-capture safe, the first call included).  No float atomics: a sum that crosses a
 * workgroup goes through the caller's workspace `ws` as one record per workgroup, and a second launch adds the records in a
 * fixed order, so every result is bitwise repeatable.  `ws` need not be initialised.  Non-finite data: PROPAGATE.
 */
#ifndef MSPI_ENTRY_TRAIN_HIP_H
#define MSPI_ENTRY_TRAIN_HIP_H

#include "mspi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weight and bias gradient of mspi_conv_fwd for the forward's descriptor d (d->ldy: row stride of dy) where the kernel equals
 * its stride along T and is 1x1 in space: k = (s,1,1), stride (s,1,1), no padding, s in {1, 2, 4}:
 *   dW[co][tap][ci] = sum_r dy[r][co] x[n, to s + tap, h, w][ci]      r = (n, to, h, w),  To = floor(T / s)
 *   db[co]          = sum_r dy[r][co]
 * dW is dense [Cout][s C], the layout mspi_conv_wgrad_fwd writes (the row order of the forward's weights); db [Cout].  Frames
 * beyond To s are never read.
 * Supported: stored Cout a multiple of 32 up to 192; stored C any multiple of 4 up to 2560 (the last 32-column tile may be
 * ragged, and a tile may straddle two taps); input strides sN, sT, sH, sW arbitrary multiples of 4 with sC == 1 (channel slices
 * of wider buffers, token views into a slab with a batch stride); ldy a multiple of 4, >= Cout; x, dy, dW and ws 16-byte
 * aligned; fewer than 2^31 output rows.  Anything else is refused with the reason in mspi_last_error().
 * v_mfma_f32_32x32x2_f32 with the rows as the contraction: the columns (tap, ci) of a row are one line of s C values, cut
 * into tiles of 32.  A workgroup owns a slice of the rows, up to four column tiles and all of Cout; its four waves share the
 * (Cout / 32) x (column tiles) accumulator tiles round-robin, so three column tiles keep four waves as busy as four do.  It
 * stages 32 rows at a time through LDS, dy and x once each, and writes one record [Cout][s C] (+ [Cout], from the workgroups of
 * the first column group) to ws; the second launch adds the records in slice order.
 * One table of variants, by output rows R: a slice is 64 rows below 1024 rows, 256 below 32768, 512 from there on.
 * mspi_conv_wgrad_entry_supported: 1 or 0 for the descriptor alone; mspi_conv_wgrad_entry_variant: rows per slice, or -1 for
 * exactly what the launch refuses (descriptor or pointers), the reason in mspi_last_error(); mspi_conv_wgrad_entry_ws_bytes:
 * host arithmetic, 0 for a refused descriptor.  All three are host only.
 * A NaN or Inf in a used x[r][ci] reaches dW[:, tap, ci] and never db; one in dy[r][co] reaches dW[co] and db[co]. */
int mspi_conv_wgrad_entry_supported(const MspiConvDesc* d);
size_t mspi_conv_wgrad_entry_ws_bytes(const MspiConvDesc* d);
int mspi_conv_wgrad_entry_variant(const MspiConvDesc* d, const void* x, const void* dy);
int mspi_conv_wgrad_entry(const MspiConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                          mspi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MSPI_ENTRY_TRAIN_HIP_H */
