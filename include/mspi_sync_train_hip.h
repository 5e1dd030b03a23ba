/*
 * mspi_sync_train_hip.h -- backward entry points of the SyncBlock's transformer Block (model/model_utils.py:84-152 upstream):
 * x + proj(attention(LayerNorm(x))), then + fc2(GELU(fc1(LayerNorm(.)))), at dim 512 with 4 heads of 128.
 *
 * Why a sixth header: for the reason mspi_block_train_hip.h gives -- the symbol sets of the five older headers are pinned by
 * tables inside existing test files.  The entry points below live in the SAME library (csrc/sync_bwd.hip) and are held to the
 * same three contracts (declared = exported = bound; capture-safe launches; non-finite data propagates) by
 * tests/test_sync_block_train.py.  The Python binding mirrors the split (_lib._SYNC_SIGNATURES / SYNC_EXPORTS).
 * MSPI_ABI_VERSION is unchanged.
 *
 * Conventions: those of mspi_block_train_hip.h -- fp32 device memory owned by the caller, 0 or a negative MSPI_E* code with the
 * reason in mspi_last_error(), launches on the caller's stream only, no allocation, memcpy, memset, synchronisation or mutable
 * static (graph-capture safe, the first call included).  No float read-modify-write on shared memory cells: every output
 * element is written by exactly one workgroup, and a sum that crosses a workgroup goes through the caller's workspace `ws` as
 * one record per workgroup, which a second launch adds in a fixed order, so every result is bitwise repeatable.  `ws` need not
 * be initialised.  Non-finite data: PROPAGATE.
 *
 * What the Block's backward takes from elsewhere: mspi_gelu_bwd, the weight gradients of the four linear layers from
 * mspi_linear_wgrad (mspi_linear_train_hip.h; one launch pair a layer, dqkv read in its slab), their data gradients from
 * mspi_conv_fwd on transposed packs at MSPI_PREC_F32.
 */
#ifndef MSPI_SYNC_TRAIN_HIP_H
#define MSPI_SYNC_TRAIN_HIP_H

#include "mspi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of o = softmax(scale q k^T) v, addressed by the forward's descriptor, for the output gradient dO:
 *   P = softmax(scale q k^T),  Delta_i = sum_d dO_id o_id
 *   dv = P^T dO,  dP = dO v^T,  dS = P (dP - Delta),  dq = scale dS k,  dk = scale dS^T q
 * q, k, v carry the descriptor's strides; dq, dk, dv take the strides of q, k, v (a [rows][3][heads][128] slab is written in
 * place of a dense triple, and the GEMMs that follow read it as it stands); o and dO take the o strides.  No output may
 * overlap an input.  Nq and Nk are independent, any value >= 1.
 * fp32 on v_mfma_f32_32x32x2_f32; d->prec must be MSPI_PREC_F32 (the operands are gradients at the scale of the loss, where the
 * f16x3 split is not exact).  (D, Dv) in {(128,128)}; any other pair is refused with this list.  No bias, no mask, no token
 * index: nmask and nwin must be 0.  Strides multiples of 4 floats, pointers 16-byte aligned, B * Hh < 65536.
 * The forward stores no statistics: the first launch computes the max-shifted log-sum-exp and Delta of every query row into
 * ws (mspi_attn_bwd_ws_bytes(d) bytes, 0 = refused) and dq; the second dk and dv.  Keys past Nk have probability exactly 0,
 * queries past Nq add exactly 0.  A non-finite stored output sets the status word (mspi_set_status_word).
 * mspi_attn_bwd_variant (host only): 10^7 + D * 10^4 + Dv * 10, or -1 for a descriptor the launch refuses, the reason in
 * mspi_last_error().
 * A NaN or Inf in q, k, v, o or dO of one (sequence, head) stays inside that (sequence, head). */
size_t mspi_attn_bwd_ws_bytes(const MspiAttnDesc* d);
int mspi_attn_bwd_variant(const MspiAttnDesc* d);
int mspi_attn_bwd(const MspiAttnDesc* d, const float* q, const float* k, const float* v, const float* o, const float* dO,
                  float* dq, float* dk, float* dv, void* ws, mspi_stream_t stream);

/* mspi_layernorm_bwd (mspi_block_train_hip.h) for rows of 256 < C <= 512 channels, C % 4 == 0; other widths are refused by
 * name.  Same contract: dx, dgamma, dbeta from x, dy and gamma; mean and rstd are computed again from x in the order of the
 * forward's kernel for these widths (32 lanes a row, four vectors a lane), so x^ has the forward's bits; the column sums go
 * through ws (mspi_layernorm_bwd_wide_ws_bytes(M, C) bytes, 0 = refused) as one record [dbeta | dgamma] per 256 rows.
 * dx may be dy.  Row strides multiples of 4 and >= C, pointers 16-byte aligned, 0 < M < 2^31, eps >= 0. */
size_t mspi_layernorm_bwd_wide_ws_bytes(int64_t M, int32_t C);
int mspi_layernorm_bwd_wide(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* gamma, float eps, float* dx,
                            int64_t lddx, float* dgamma, float* dbeta, void* ws, int64_t M, int32_t C, mspi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MSPI_SYNC_TRAIN_HIP_H */
