/*
 * mspi_adapter_train_hip.h -- weight gradient of the adapter's Inception (Adapter.conv, backbones/s3d.py upstream): eight
 * conv -> BatchNorm3d -> ReLU layers, 1x1x1, (1,3,3) and (3,1,1), whose widths 16, 48, 64, 96, 192, 208 and 416 are multiples
 * of 16 but not all of 32, so that five of them fit no older weight-gradient kernel.
 *
 * Why a fifth header: for the reason mspi_block_train_hip.h gives -- the symbol sets of the four older headers are pinned by
 * tables inside existing test files.  The entry points below live in the SAME library (csrc/adapter_bwd.hip) and are held to the
 * same three contracts (declared = exported = bound; capture-safe launches; non-finite data propagates) by
 * tests/test_adapter_train.py.  The Python binding mirrors the split (_lib._ADAPTER_SIGNATURES / ADAPTER_EXPORTS).
 * MSPI_ABI_VERSION is unchanged.
 *
 * Conventions: those of mspi_entry_train_hip.h -- fp32 device memory owned by the caller, channels-last rows, 0 or a negative
 * MSPI_E* code with the reason in mspi_last_error(), launches on the caller's stream only, no allocation, memcpy, memset,
 * synchronisation or mutable static (graph-capture safe, the first call included).  No float atomics: a sum that crosses a
 * workgroup goes through the caller's workspace `ws` as one record per row slice, and a second launch adds the records in
 * slice order, so every result is bitwise repeatable.  `ws` need not be initialised.  Non-finite data: PROPAGATE.
 */
#ifndef MSPI_ADAPTER_TRAIN_HIP_H
#define MSPI_ADAPTER_TRAIN_HIP_H

#include "mspi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weight and bias gradient of mspi_conv_fwd for the forward's descriptor d (d->ldy: row stride of dy) of a stride-1 "same" conv
 * with kernel (1,1,1), (1,3,3) pad (0,1,1) or (3,1,1) pad (1,0,0):
 *   dW[co][tap][ci] = sum_m dy[m][co] x[pos(m, tap)][ci]      m = (n, t, h, w)
 *   db[co]          = sum_m dy[m][co]                          written when db != NULL
 * dW is dense [Cout][taps C], the layout mspi_conv_wgrad_fwd writes (the row order of the forward's weights).  Padding is zero
 * per image and per clip: a tap never reads across an n boundary, a (1,3,3) tap never across a frame.
 * Supported: stored C a multiple of 16 up to 416, stored Cout a multiple of 16 up to 208; sC == 1, the other input strides
 * and ldy multiples of 4 with ldy >= Cout (x a channel slice of a wider buffer, dy a channel slice of wider rows); x, dy, dW
 * and ws 16-byte aligned; fewer than 2^31 rows.  Anything else is refused with the reason in mspi_last_error().
 * v_mfma_f32_16x16x4_f32 with the rows as the contraction.  The rows are cut into boxes of at most 32 positions of one image
 * (32 rows; lines x columns of a frame; frames x positions of a clip).  A workgroup owns a slice of the boxes, a group of
 * 16-wide input-channel tiles, every tap and all of Cout; it stages a box's dy columns and its x channels with the halo in LDS
 * once (positions outside the image as zeros) and every tap reads them from there.  Its accumulator tiles go round-robin to
 * the four waves, at most 30 each, so a wave has independent accumulators in flight.  It writes one record [Cout][taps C]
 * (+ [Cout], from the workgroups of the first channel group) to ws; the second launch adds the records in slice order.
 * One table of variants, by rows R: a slice is 64 rows (two boxes) below 1024 rows, 128 below 8192, 256 from there on.
 * mspi_conv_wgrad_t16_supported: 1 or 0 for the descriptor alone; mspi_conv_wgrad_t16_variant: rows per slice, or -1 for
 * exactly what the launch refuses (descriptor or pointers), the reason in mspi_last_error(); mspi_conv_wgrad_t16_ws_bytes:
 * host arithmetic, 0 for a refused descriptor.  All three are host only.
 * A NaN or Inf in a used x[r][ci] reaches dW[:, tap, ci] and never db; one in dy[r][co] reaches dW[co] and db[co]. */
int mspi_conv_wgrad_t16_supported(const MspiConvDesc* d);
size_t mspi_conv_wgrad_t16_ws_bytes(const MspiConvDesc* d);
int mspi_conv_wgrad_t16_variant(const MspiConvDesc* d, const void* x, const void* dy);
int mspi_conv_wgrad_t16(const MspiConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                        mspi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MSPI_ADAPTER_TRAIN_HIP_H */
