/*
 * mspi_hip.h -- C ABI of libmspi_hip.so: the MI355X (gfx950) kernels behind MSPI's
 * saliency-inference hot path.
 *
 * The reference (oraclefina/MSPI) has no FFI boundary on this path: every op below is an
 * ATen call issued from a torch.nn.Module.forward.  Each entry point
 * therefore cites the reference call site(s) whose arithmetic it replaces; the Python
 * host (mspi_amd/) reaches them through ctypes with raw device pointers
 * (tensor.data_ptr()) and the caller's hipStream_t.  See INTEGRATION.md for the binding.
 *
 * Conventions
 *   - all tensors are fp32, device memory, owned by the caller; nothing is allocated here
 *   - activations are channels-last: a tensor [N,T,H,W,C] is a row-major matrix of
 *     M = N*T*H*W rows with a row stride `ld` (floats, multiple of 4) and C columns.
 *     ld > C lets a producer write straight into a channel slice of a concat buffer.
 *   - every function returns 0 or a negative MSPI_E* code and never throws; the message
 *     is available from mspi_last_error() (thread-local)
 *   - kernels are stateless and re-entrant; launches go to `stream` and return
 *     immediately (graph-capture safe: no sync, no allocation, no memcpy inside).
 *     That includes the FIRST call of a process, on any device and any thread: no entry
 *     point initialises anything lazily, and none keeps a mutable static.  Host arrays
 *     and descriptors are read during the call; a captured graph holds its own copy.
 *     tests/test_launch_ledger.py holds every entry point to this (a source scan, one
 *     capture + replay case per launching entry point, a cold-capture child process, a
 *     second device); tests/test_replay_ledger.py replays every model through hipGraphs.
 */
#ifndef MSPI_HIP_H
#define MSPI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSPI_ABI_VERSION 2   /* 2: blocked plane layout (mspi_gemm_sp_fwd and friends), MspiConvDesc.w_blocked */

typedef void* mspi_stream_t; /* hipStream_t */

enum {
  MSPI_OK = 0,
  MSPI_EINVAL = -1,   /* bad descriptor (shape/stride/alignment) */
  MSPI_ELAUNCH = -2,  /* hip launch error */
  MSPI_ENODEV = -3    /* no gfx950 device / code object not loadable */
};

enum { MSPI_ACT_NONE = 0, MSPI_ACT_RELU = 1, MSPI_ACT_GELU = 2, MSPI_ACT_SIGMOID = 3, MSPI_ACT_SWISH = 4 };

/* GEMM arithmetic.  F32: v_mfma_f32_32x32x2_f32 (exact fp32).  F16X3: every fp32 operand is split into
 * hi + lo f16 halves (22 significand bits) and the product is formed as hi*hi + hi*lo + lo*hi by three
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation -- fp32-level accuracy (<= 2^-21 relative per product) on
 * the 16x faster f16 matrix pipe.  Operands must satisfy |x| < 65504 and |w * w_scale| < 65504. */
enum { MSPI_PREC_F32 = 0, MSPI_PREC_F16X3 = 1 };

int mspi_version(void);
const char* mspi_last_error(void);
/* Range guard.  f16x3 operands must satisfy |x| < 65504 (beyond it the f16 hi half is inf).  The GEMM kernels (mspi_conv_fwd,
 * mspi_conv_splitk_fwd, mspi_gemm_sp_fwd, mspi_rowgemm_fwd, mspi_mlp_fwd, mspi_x3d_ab_fwd, mspi_x3d_ab_s2_fwd) check their pre-activation
 * results and store 1 into *word when one is inf or NaN -- whatever the cause (operand out of range, non-finite input).
 * `word` must be device-visible: a 4-byte word of pinned host memory (hipHostMalloc / torch pin_memory) lets the caller read
 * it without a device call, after the event that covers the launches; the caller clears it.  NULL (default): no report.
 * Process-global; set it before launching from several threads.
 *
 * Non-finite data (tests/test_nonfinite_ledger.py holds every entry point to it): a NaN or Inf in a floating-point operand
 * never leaves an entry point as plausible finite data without a trace.  Every output that depends on it is non-finite
 * (PROPAGATE), or *word is 1 (FLAG); outputs that do not depend on it are unaffected.
 *   FLAG       the GEMM family on its pre-activation results (the seven above, mspi_conv_halo_fwd, mspi_x3d_ca_fwd: their
 *              ReLU is fmaxf, which turns a NaN into 0 after the check), attention on its stored outputs, and
 *              mspi_postprocess_u8, whose u8 output cannot carry a NaN, on the resized map.
 *   PROPAGATE  every other entry point with floating-point output, as torch does: ReLU and max keep a NaN
 *              (mspi_x3d_stem_fwd, mspi_dwconv_fwd, mspi_maxpool_fwd, mspi_se_gate, mspi_layernorm_fwd / _sp_fwd,
 *              mspi_upsample_fwd / _sum_fwd, mspi_bn_stats / _apply, the other row operations and training kernels). */
int mspi_set_status_word(int32_t* device_visible_word);

/* number of visible HIP devices whose arch is gfx950 (0 if none). */
int mspi_device_count(void);

/* ------------------------------------------------------------------------------------
 * Dense convolution / linear as an MFMA (v_mfma_f32_32x32x2_f32) implicit GEMM.
 *   y[m, co] = act( sum_k A[m,k] * w[co,k] + bias[co] (+ res[m,co]) )
 * m runs over (n, to, ho, wo); k over (kt, kh, kw, ci) with ci fastest.
 * Replaces: nn.Conv3d / nn.Conv2d / nn.Linear with eval-mode BatchNorm folded in --
 *   SlowFast/resnet_helper.py:296-303,335-342 (X3D a / c), :427-464 (bottleneck a/b/c),
 *   :579-591 (branch1); SlowFast/stem_helper.py:262-269 (x3d conv_xy), :171-181 (basic stem);
 *   backbones/resnet.py:79-90,30-52; backbones/s3d.py:41-52,95-116;
 *   model/model_utils.py:43-46,92-94 (Linear), :324-327 (pwconv), :367-377 (smooth),
 *   :439-440 (lateral), :490-503 (readout); backbones/MViT.py:1059-1061;
 *   backbones/video_swin_transformer.py:151-153,449.
 * The input is addressed through element strides so NCDHW user tensors (clips, audio)
 * are consumed without a layout pass.  `gate` (optional, 1x1x1 stride-1 unpadded only) applies the
 * X3D squeeze-excite scale and Swish to A on the fly:
 *   A'[m,k] = swish(A[m,k] * gate[n(m), k])      (SlowFast/resnet_helper.py:66-73,76-103)
 * ------------------------------------------------------------------------------------ */
typedef struct MspiConvDesc {
  int32_t N, T, H, W, C;           /* input extent; C = channels as stored */
  int64_t sN, sT, sH, sW, sC;      /* input element strides */
  int32_t kT, kH, kW;
  int32_t strT, strH, strW;
  int32_t padT, padH, padW;
  int32_t To, Ho, Wo;              /* output extent (checked against the formula) */
  int32_t Cout;                    /* output columns written (stored width) */
  int64_t ldy;                     /* output row stride */
  int64_t ldw;                     /* weight row stride, >= kT*kH*kW*C, multiple of 4, zero padded */
  int64_t ldr;                     /* residual row stride (res != NULL) */
  int32_t act;                     /* MSPI_ACT_* applied last */
  int32_t prec;                    /* MSPI_PREC_F32: w is float [Cout][ldw];
                                      MSPI_PREC_F16X3: w is _Float16 [2][Cout][ldw] = hi/lo split of w*w_scale,
                                      ldw % 32 == 0 (see below) */
  float w_scale;                   /* F16X3: power-of-two pre-scale of the weights (undone in the epilogue) */
  int32_t tile;                    /* -1: library heuristic; else a kernel instantiation picked by the caller's
                                      autotuner, by this table (kTiles in csrc/conv_common.h is its source):
                                        code   kind                           rows x columns      mspi_gemm_sp_fwd
                                        0      1 register-staged, 4 waves     128 x 128           -
                                        1      1                              128 x 64            -
                                        2      1                              128 x 32            -
                                        3      1 (split-K: kind 3)            64 x 64             -
                                        4      2 register-staged, 8 waves     128 x 128           -
                                        5      2                              256 x 128           -
                                        6      4 LDS-DMA, 4 waves             128 x 128           128 x 128
                                        7      4                              128 x 64            128 x 64
                                        8      4                              128 x all (<= 256)  -
                                        9      4                              128 x 96            128 x 96
                                        10     4                              128 x 192           128 x 192
                                        11     4                              128 x 32            128 x 256
                                        12     5 LDS-DMA, 8 waves             256 x 256           256 x 256
                                        13     5                              256 x 192           256 x 192
                                        14     5                              256 x 128           256 x 128
                                      Kinds 4 and 5 need f16x3 and the 16-B gather.  "all": one column tile of
                                      roundup32(Cout) columns.  Last column: the tile mspi_gemm_sp_fwd runs under the
                                      code (its kinds are 6 and 7), "-" = the heuristic, as for -1. */
  const void* w_blocked;           /* optional (NULL: none), F16X3 only: the same hi/lo weight planes BLOCKED as described at
                                      mspi_gemm_sp_fwd (16 output channels x 32 k = 1 KB contiguous per block, k-fastest,
                                      rows zero-padded to a multiple of 16).  The LDS-DMA kernels (tile 6..14, and the
                                      heuristic when it picks them) stage their weights from it: every piece is then 8 full
                                      cache lines instead of 16 half lines.  The other kernels read `w`. */
} MspiConvDesc;

int mspi_conv_fwd(const MspiConvDesc* d, const float* x, const float* w, const float* bias /*[Cout] or NULL*/,
                  const float* res /*NULL or [M][ldr]*/, const float* gate /*NULL or [N][C]*/,
                  float* y, mspi_stream_t stream);

/* Split-K form of mspi_conv_fwd for problems with few output tiles and a long contraction (M*Cout small, K large:
 * the SA / smoothing convs on 14x14 maps, the audio ResNet's last stages, SlowFast s5): ksplit workgroups share each
 * 64x64 output tile, each owns a contiguous range of K steps and writes its partial sums to the workspace
 * (mspi_conv_splitk_ws_bytes(d, ksplit) bytes); a second launch adds the slices in order and applies bias, residual and
 * activation -- bitwise reproducible, no atomics.  No gate; Cout % 4 == 0. */
size_t mspi_conv_splitk_ws_bytes(const MspiConvDesc* d, int32_t ksplit);
int mspi_conv_splitk_fwd(const MspiConvDesc* d, const float* x, const float* w, const float* bias, const float* res,
                         float* y, void* workspace, int32_t ksplit, mspi_stream_t stream);
/* Which kernel instantiation mspi_conv_fwd (ksplit <= 1) or mspi_conv_splitk_fwd (ksplit >= 2) launches for this descriptor,
 * input pointer and gate pointer in this process (host only, no GPU call, no pointer dereferenced: x and gate are looked at
 * for NULL and 16-B alignment, a NULL x is refused; the MSPI_CONV_* switches are read once per process):
 *   kind * 10000000 + BM * 10000 + BN * 10 + form
 * kind, BM = rows and BN = columns as in the table at MspiConvDesc.tile, kind 3 = split-K (64 x 64 tiles); form =
 * 2 * (scalar gather) + prec for kinds 1..3, 0 = generic gather / 1 = dense (1x1x1, stride 1, no padding) / 2 = dense with
 * the gate for kinds 4 and 5.
 * -1 = a descriptor the launch refuses (mspi_last_error() says why).  The launches select their kernel by this same
 * function; the weight, output and residual pointers are checked at launch only. */
int mspi_conv_variant(const MspiConvDesc* d, const float* x, const float* gate, int32_t ksplit);

/* ------------------------------------------------------------------------------------
 * Halo-staged f16x3 implicit GEMM for stride-1 convs with kernel (kT,3,3), kT in {1,3}, pad (kT/2,1,1), on fp32
 * channels-last input (dense or a channel slab: sC == 1, 16-B aligned pointer and strides, C % 32 == 0).  A workgroup owns
 * an output brick of 4 x 8 x 8 (t,h,w) positions of one sample; per 32-channel chunk it stages the brick and its 1-cell
 * halo once, split to f16 hi/lo once, into LDS and walks the taps there: only the weight block of (tap, chunk) is fetched
 * per step.  Same descriptor and epilogue contract as mspi_conv_fwd (bias, optional residual, activation, range guard);
 * weights are d->w_blocked (required), `tile` is ignored, no gate.  The summation order is chunk-major (fp32 accumulate).
 * No allocation: capture safe.  A second implementation beside mspi_conv_fwd: that entry point never selects it.
 * ------------------------------------------------------------------------------------ */
int mspi_conv_halo_fwd(const MspiConvDesc* d, const float* x, const float* bias, const float* res, const float* gate /* must be NULL */,
                       float* y, mspi_stream_t stream);
/* 1 when mspi_conv_halo_fwd takes this descriptor (with a 16-B aligned input), else 0 (host only). */
int mspi_conv_halo_supported(const MspiConvDesc* d);
/* Which instantiation mspi_conv_halo_fwd launches: conv_halo_kernel<kT, BN / 32> as kT * 1000 + BN (BN = 64 / 128 / 192 output
 * columns per workgroup: the smallest that holds Cout, 192 beyond); -1 = a descriptor or input pointer the launch refuses
 * (mspi_last_error() says why).  Host only; the launch selects by this function. */
int mspi_conv_halo_variant(const MspiConvDesc* d, const void* x);

/* ------------------------------------------------------------------------------------
 * Depthwise convolution, channels-last, bias (= folded BN) + activation fused; optional
 * per-(n,c) PARTIAL sums of the pre-activation output for squeeze-excite: pool is
 * [N][mspi_dwconv_pool_rows(d)][C], one row per workgroup, written (not accumulated) in a
 * fixed order -- no atomics, bitwise reproducible; mspi_se_gate reduces the rows.
 * Replaces: X3D `b` 3x3x3 (SlowFast/resnet_helper.py:310-319) + b_bn (+ Swish :76-103),
 *   X3D stem (5,1,1) (SlowFast/stem_helper.py:270-283), ConvNextBlock.dwconv_t/dwconv_s
 *   (model/model_utils.py:321-322), MViT pool_q/k/v (backbones/MViT.py:1093-1133),
 *   timm ConvNeXt conv_dw 7x7.
 * w is [kT*kH*kW][C] (tap-major), x rows have stride ldx, y rows ldy.
 * ------------------------------------------------------------------------------------ */
typedef struct MspiDwConvDesc {
  int32_t N, T, H, W, C;
  int64_t ldx, ldy;
  int32_t kT, kH, kW;
  int32_t strT, strH, strW;
  int32_t padT, padH, padW;
  int32_t To, Ho, Wo;
  int32_t act;
} MspiDwConvDesc;

int mspi_dwconv_fwd(const MspiDwConvDesc* d, const float* x, const float* w, const float* bias,
                    float* y, float* pool /*NULL or [N][rows][C]*/, mspi_stream_t stream);
/* partial-sum rows per sample that mspi_dwconv_fwd writes for this descriptor (-1: pooling unsupported) */
int mspi_dwconv_pool_rows(const MspiDwConvDesc* d);
/* Which kernel instantiation mspi_dwconv_fwd launches for this descriptor in this process (host only, no GPU call; the
 * MSPI_DW_* switches are read once per process; the pool argument does not change the choice):
 *   kind * 1000 + K * 100 + stride * 10 + SW
 * kind 1 = LDS-staged (dw_lds_kernel<K, SW>, stride 1), 2 = register tile (dw_tile_kernel<K, stride, SW, 2>),
 * 3 = strip (dw_strip_kernel<K, W stride, 4>), 4 = generic (dw_kernel: 4000); -1 = invalid descriptor.
 * mspi_dwconv_fwd selects its kernel by this same function. */
int mspi_dwconv_variant(const MspiDwConvDesc* d);

/* Squeeze-excite gate: gate[n,c] = sigmoid(fc2(relu(fc1(inv_count * sum_r pool[n,r,:]))))
 * (SlowFast/resnet_helper.py:27-73).  w1 [F][C], b1 [F], w2 [C][F], b2 [C]. */
int mspi_se_gate(const float* pool, int32_t rows, float inv_count, const float* w1, const float* b1,
                 const float* w2, const float* b2, float* gate, int32_t N, int32_t C, int32_t F,
                 mspi_stream_t stream);
/* Which instantiation mspi_se_gate launches for C channels and F hidden units (host only, no GPU call):
 * 1 = se_gate_kernel<true> (C <= 512 and F <= 32: both weight matrices preloaded into registers), 2 = se_gate_kernel<false>
 * (generic loops); -1 = an extent the launch refuses (C or F <= 0, or [G*C | C | F] floats beyond the 64 KB of LDS).
 * mspi_se_gate selects its kernel by this same function. */
int mspi_se_gate_variant(int32_t C, int32_t F);

/* ------------------------------------------------------------------------------------
 * LayerNorm over the C columns of each row, one wavefront per row:
 *   y[n,r,:] = act( (x[n,r,:]-mean)/sqrt(var+eps) * gamma + beta ) + table[r, :]
 * Rows are addressed as base + n*sN + r*ld for n < N, r < R on both sides, so a producer can
 * write token slabs of a [N, R_total, C] sequence buffer (the torch.cat at
 * model/model_utils.py:277 disappears).  table (optional) has R rows.
 * Replaces nn.LayerNorm at model/model_utils.py:231-233 (+ sinusoid table add :273-274),
 *   :139,145 (Block), :296 (LayerNorm3d), :404-435 (projector LN+ReLU);
 *   backbones/MViT.py:1714; backbones/video_swin_transformer.py:306; timm LayerNorm2d.
 * ------------------------------------------------------------------------------------ */
int mspi_layernorm_fwd(const float* x, int64_t ldx, int64_t sNx, float* y, int64_t ldy, int64_t sNy,
                       const float* gamma, const float* beta, float eps, int32_t N, int32_t R, int32_t C,
                       int32_t act, const float* table /*NULL or [R][C]*/, mspi_stream_t stream);
/* Which instantiation mspi_layernorm_fwd (planes_out = 0) / mspi_layernorm_sp_fwd (planes_out = 1) launches for rows of C
 * floats (host only, no GPU call): LPR * 100 + VPT of layernorm_kernel<LPR, VPT> -- LPR lanes per row, VPT float4 per lane --
 * 1601 (C <= 64), 1602 (<= 128), 1604 (<= 256), 3204 (<= 512), 6404 (<= 1024), 6408 (<= 2048), 6412 (<= 3072); -1 = a width
 * the launch refuses (C % 4 != 0, C > 3072, planes_out with C % 32 != 0).  The launch selects its kernel by this same function. */
int mspi_layernorm_variant(int32_t C, int32_t planes_out);

/* ------------------------------------------------------------------------------------
 * Fused multi-head attention (flash style, MFMA, online softmax, fp32 in / fp32 accumulate):
 *   o[b,h,i,:] = softmax_j( scale * q[b,h,i,:] . k[b,h,j,:] + biasT[h,j,i] + maskT[b % nmask,j,i] ) v[b,h,j,:] (+ res)
 * q/k/v/o (and res, with o's strides) are addressed as base + b*sB + h*sH + token*sT + d (d contiguous).
 * D = head dim of q/k, Dv = head dim of v/o; the instantiated pairs are listed at MspiAttnDesc.
 * biasT / maskT (optional) are stored key-major ([.][Nk][Nq]).
 * A non-finite stored output sets the status word (mspi_set_status_word), as the GEMM epilogues do; padded query rows and
 * key tiles never do.
 * tok_idx (optional, [nwin][N] int32): windowed sequences -- sequence b is window b % nwin of sample b / nwin
 * (strides sB then address the SAMPLE) and its token t lives at row tok_idx[b % nwin][t] of that sample, for
 * q, k, v, res and o alike: Swin's cyclic shift, window partition, window reverse and un-shift
 * (backbones/video_swin_transformer.py:61-87,245-268) become index arithmetic inside the kernel.
 * Replaces model/model_utils.py:102-106 (SyncBlock), backbones/MViT.py:1261-1301 (pooled attention, residual
 * pooling as `res`), backbones/video_swin_transformer.py:169-187 (window attention, bias table + shift mask).
 * ------------------------------------------------------------------------------------ */
typedef struct MspiAttnDesc {
  /* (D, Dv) in {(32,32),(64,64),(96,96),(128,128),(128,96),(144,96),(160,96)} (kAttnPairs in csrc/attn.hip); any other pair is
   * refused with this list by mspi_attn_fwd / mspi_attn_fwd_ws and answered with -1 by mspi_attn_variant */
  int32_t B, Hh, Nq, Nk, D, Dv, nmask, nwin;
  int64_t q_sB, q_sH, q_sT;
  int64_t k_sB, k_sH, k_sT;
  int64_t v_sB, v_sH, v_sT;
  int64_t o_sB, o_sH, o_sT;
  float scale;
  int32_t prec;   /* MSPI_PREC_F32: fp32 MFMA; MSPI_PREC_F16X3: split products on the f16 pipe (fp32-accurate) */
} MspiAttnDesc;

int mspi_attn_fwd(const MspiAttnDesc* d, const float* q, const float* k, const float* v, const float* res,
                  const float* biasT, const float* maskT, const int32_t* tok_idx, float* o, mspi_stream_t stream);

/* The same attention (f16x3 only) with K and V split ONCE per (sequence, head) into f16 hi/lo planes in a caller-owned
 * workspace of mspi_attn_ws_bytes(d) bytes, instead of by every query tile of that head on its own copy: two launches (plane
 * kernel, attention kernel), results bit-identical to mspi_attn_fwd.  mspi_attn_ws_bytes returns 0 for other precisions.
 * Without bias, mask and token index the attention kernel is the software-pipelined form (csrc/attn.hip, attn_pipe_kernel:
 * the planes are then per-tile LDS images staged by LDS-DMA); same products in the same order, same results.
 * Few-query shapes (fewer than 256 query tiles over all heads, at least 24 key tiles; no bias, mask or token index) are
 * additionally split along the keys: up to 8 workgroups per query tile each walk a slice of the key tiles and a third
 * launch merges their (O, running max, running sum) in fixed order -- deterministic, equal to the one-pass result up to
 * fp32 rounding of the merge; the workspace size accounts for the partial results.  MSPI_ATTN_KSPLIT=0 switches it off.
 * mspi_attn_ws_bytes does not look at the pair (D, Dv); the launch refuses the pairs that are not at MspiAttnDesc. */
size_t mspi_attn_ws_bytes(const MspiAttnDesc* d);
int mspi_attn_fwd_ws(const MspiAttnDesc* d, const float* q, const float* k, const float* v, const float* res,
                     const float* biasT, const float* maskT, const int32_t* tok_idx, float* o, void* workspace,
                     mspi_stream_t stream);
/* Which kernels the attention launch for this descriptor runs in this process (host only, no GPU call; the MSPI_ATTN_*
 * switches are read once per process): has_bias / has_mask / has_tok = the optional arguments are given, has_ws = the
 * call is mspi_attn_fwd_ws (else mspi_attn_fwd).
 *   kind * 10000000 + D * 10000 + Dv * 10 + (1 if the key split's merge pass runs)
 * kind 1 = fp32 (attn_kernel<D, Dv>), 2 = f16x3 without planes (attn_f16x3_kernel<D, Dv>), 3 = f16x3 on prefetched
 * planes (attn_f16x3_kernel<D, Dv, true, true>), 4 = the same without prefetch (<D, Dv, true, false>, MSPI_ATTN_PF=0),
 * 5 = software pipeline (attn_pipe_kernel<D, Dv>); -1 = prec, or a (D, Dv) that is not at MspiAttnDesc, not instantiated.
 * mspi_attn_fwd / mspi_attn_fwd_ws select their kernels by this same function. */
int mspi_attn_variant(const MspiAttnDesc* d, int32_t has_bias, int32_t has_mask, int32_t has_tok, int32_t has_ws);

/* MViTv2 decomposed relative positions folded into the attention contraction (backbones/MViT.py:905-997):
 *   qa[b,h,i,:] = [ scale*q_i | q_i.Rh[hq(i),0..kH) | q_i.Rw[wq(i),0..kW) | q_i.Rt[tq(i),0..kT) | 0 ]   (DA columns)
 *   ka[b,h,j,:] = [ k_j | onehot_kH(hk(j)) | onehot_kW(wk(j)) | onehot_kT(tk(j)) | 0 ]
 * so that qa.ka^T = scale*q.k + rel_h + rel_w + rel_t exactly; feed qa/ka to mspi_attn_fwd with D = DA, scale 1.
 * q rows are [B*Nq][ldq] with head h at column h*Dh (likewise k); Rh/Rw/Rt are the gathered tables
 * [qH][kH][Dh], [qW][kW][Dh], [qT][kT][Dh]. */
typedef struct MspiMvitAugDesc {
  int32_t B, heads, Dh, DA;
  int32_t qT, qH, qW, kT, kH, kW;
  int64_t ldq, ldk;
  float scale;
} MspiMvitAugDesc;

int mspi_mvit_qk_augment(const MspiMvitAugDesc* d, const float* q, const float* k, const float* Rh, const float* Rw,
                         const float* Rt, float* qa, float* ka, mspi_stream_t stream);

/* Same result with the dot products done by a GEMM: P[(b*Nq + tok)*heads + head][ldp] = q_row . T^T, T = the rows of the
 * three (length-matched) relative-position tables stacked; idx_h [qH][kH], idx_w [qW][kW], idx_t [qT][kT] give the column
 * of P that holds q . R*[position, j] (the relative distance of backbones/MViT.py:905-990 plus the table's offset).  The
 * caller computes P with mspi_conv_fwd / mspi_rowgemm_fwd on the q rows; this call only copies and gathers. */
int mspi_mvit_qk_augment_p(const MspiMvitAugDesc* d, const float* q, const float* k, const float* P, int64_t ldp,
                           const int32_t* idx_h, const int32_t* idx_w, const int32_t* idx_t, float* qa, float* ka,
                           mspi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * X3D block, first half, fused (csrc/x3d_block.hip):
 *   u = act( b_bn( dw3x3x3( relu( a_bn( a(x) ) ) ) ) ),  act = SWISH (blocks without squeeze-excite) or NONE (+ pool)
 * Replaces X3DTransform's a, a_bn, a_relu, b, b_bn (SlowFast/resnet_helper.py:296-319) for the stride-1 blocks; the
 * 2.25x-wide `a` output stays in LDS.  x: [N,T,H,W] rows of ldx floats (Cin stored channels, Cin % 8 == 0); u: rows of
 * ldu floats (Cmid stored channels).  wa_packed: mspi_x3d_ab_packed_bytes(Cin, Cmid) bytes, f16 hi/lo of a's weights
 * (BN folded) times wa_scale in MFMA fragment order [chunk of 32 outputs][k32 step][16-row half][hi,lo][lane][8]: element
 * e of lane l = W[chunk*32 + half*16 + (l & 15)][32*step + 8*(l >> 4) + e], zero padded.  wb: fp32 [27][Cmid] taps
 * (kt,kh,kw major) with b_bn folded, bias_a / bias_b fp32.  pool (optional): [N][mspi_x3d_ab_pool_rows(d)][Cmid] partial
 * sums of the PRE-activation output for mspi_se_gate (one row per workgroup, no atomics).
 * H % 7 == 0 and (W % 14 == 0 or W == 7); Cin <= 96 or Cin in (160, 192]. */
typedef struct MspiX3dAbDesc {
  int32_t N, T, H, W;
  int32_t Cin, Cmid;               /* stored channel counts */
  int64_t ldx, ldu;
  int32_t act;                     /* MSPI_ACT_NONE or MSPI_ACT_SWISH, applied to u (not to the pooled sums) */
  float wa_scale;                  /* power-of-two pre-scale of a's weights */
} MspiX3dAbDesc;

int mspi_x3d_ab_supported(const MspiX3dAbDesc* d);
int mspi_x3d_ab_pool_rows(const MspiX3dAbDesc* d);
size_t mspi_x3d_ab_packed_bytes(int32_t Cin, int32_t Cmid);
int mspi_x3d_ab_fwd(const MspiX3dAbDesc* d, const void* x, const void* wa_packed, const void* bias_a, const void* wb,
                    const void* bias_b, void* u, void* pool /*or NULL*/, mspi_stream_t stream);
/* Which instantiation mspi_x3d_ab_fwd launches (host only; pool does not change it): x3d_ab_kernel<KS, TH, TW, SL> as
 * KS * 10000 + TH * 1000 + TW * 10 + SL (KS = ceil(Cin / 32), 7 x 14 tiles when W % 14 == 0, else 7 x 7); -1 = a
 * descriptor the launch refuses.  mspi_x3d_ab_fwd selects by this function. */
int mspi_x3d_ab_variant(const MspiX3dAbDesc* d);

/* ------------------------------------------------------------------------------------
 * The same first half for the FIRST block of a stage, whose `b` has spatial stride 2 (csrc/x3d_head.hip):
 *   u = act( b_bn( dw3x3x3, stride (1,2,2), pad (1,1,1) ( relu( a_bn( a(x) ) ) ) ) )
 * The `a` output, four times the size of u, stays in LDS instead of being written and read back at the input resolution.
 * x: [N,T,H,W] rows of ldx floats; u: [N,T,H/2,W/2] rows of ldu floats.  wa_packed, wb, bias_a, bias_b, act, wa_scale and
 * pool ([N][mspi_x3d_ab_s2_pool_rows(d)][Cmid], one row per workgroup, pad channels zero, consumed by mspi_se_gate) are
 * those of mspi_x3d_ab_fwd; mspi_x3d_ab_packed_bytes(Cin, Cmid) gives the size of wa_packed.
 * H and W even, (H/2) % 7 == 0 and (W/2) % 7 == 0 (7 x 7 output tiles, so W/2 % 14 == 0 is covered); Cin <= 96, Cin % 8 == 0,
 * Cmid % 4 == 0; one frame of x below 2^31 floats. */
typedef struct MspiX3dAbS2Desc {
  int32_t N, T, H, W;              /* the INPUT extent */
  int32_t Cin, Cmid;               /* stored channel counts */
  int64_t ldx, ldu;
  int32_t act;                     /* MSPI_ACT_NONE or MSPI_ACT_SWISH, applied to u (not to the pooled sums) */
  float wa_scale;                  /* power-of-two pre-scale of a's weights */
} MspiX3dAbS2Desc;

int mspi_x3d_ab_s2_supported(const MspiX3dAbS2Desc* d);
int mspi_x3d_ab_s2_pool_rows(const MspiX3dAbS2Desc* d);   /* tiles * T segments, tiles = (H/14) * (W/14) */
int mspi_x3d_ab_s2_fwd(const MspiX3dAbS2Desc* d, const void* x, const void* wa_packed, const void* bias_a, const void* wb,
                       const void* bias_b, void* u, void* pool /*or NULL*/, mspi_stream_t stream);
/* Which instantiation mspi_x3d_ab_s2_fwd launches (host only): x3d_ab_s2_kernel<KS> as KS * 10000 + 7071 (KS = ceil(Cin /
 * 32), 7 x 7 output tiles, one output per thread); -1 = a descriptor the launch refuses. */
int mspi_x3d_ab_s2_variant(const MspiX3dAbS2Desc* d);

/* ------------------------------------------------------------------------------------
 * X3D stem in one launch (csrc/x3d_head.hip; SlowFast/stem_helper.py:207-290):
 *   y = relu( bn( conv (5,1,1) pad 2, depthwise ( conv_xy (1,3,3), stride (1,2,2), pad (0,1,1), 3 -> 24, no bias ) ) )
 * x: the raw clip [N,3,T,H,W], fp32, element strides sN, sC, sT, sH, sW (non-negative; (H-1)*sH + (W-1)*sW < 2^31).
 * y: [N,T,Ho,Wo] rows of ldy floats, 24 channels, Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1.  wxy: fp32 [27][24], tap (ci,kh,kw)
 * major; wt: fp32 [5][24] temporal taps with the BN scale folded; bias: the folded BN shift [24] -- all three are HOST
 * pointers: the 792 weights travel as kernel arguments (read into SGPRs), and are copied at the call, so a captured graph
 * holds its own copy.  All products are fp32 FMAs (no f16 split: no operand range to watch).  The conv_xy result stays in
 * registers. */
typedef struct MspiX3dStemDesc {
  int32_t N, T, H, W;
  int64_t sN, sC, sT, sH, sW;
  int64_t ldy;
} MspiX3dStemDesc;

int mspi_x3d_stem_supported(const MspiX3dStemDesc* d);
/* x3d_stem_kernel has one instantiation; the code is the number of frames per T segment of the launch; -1 = refused. */
int mspi_x3d_stem_variant(const MspiX3dStemDesc* d);
int mspi_x3d_stem_fwd(const MspiX3dStemDesc* d, const void* x, const void* wxy, const void* wt, const void* bias, void* y,
                      mspi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Max pooling, channels-last, -inf padding.
 * Replaces nn.MaxPool3d / MaxPool2d at model/model_utils.py:189,206;
 *   backbones/resnet.py:82; SlowFast/stem_helper.py:195-197; backbones/MViT.py:1403-1409.
 * ------------------------------------------------------------------------------------ */
int mspi_maxpool_fwd(const MspiDwConvDesc* d, const float* x, float* y, mspi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Bilinear spatial up-sampling by an integer factor (align_corners=False; T untouched,
 * which is what trilinear with scale (1,k,k) computes), optionally accumulating:
 *   dst[n,t,ho,wo,:] = act( (dst[n,t,ho,wo,:] +) bilinear(src[n,t,:,:,:]) )
 * Replaces nn.Upsample at model/model_utils.py:158,208,486-488,498 and the adds at :566-570.
 * ------------------------------------------------------------------------------------ */
int mspi_upsample_fwd(const float* src, int64_t lds, float* dst, int64_t ldd, int32_t NT, int32_t H,
                      int32_t W, int32_t C, int32_t factor, int32_t accumulate, int32_t act,
                      mspi_stream_t stream);

/* The sum of J <= 3 such up-samples in one pass over dst (the decoder's top-down fusion):
 *   dst[n,t,ho,wo,:] = act( (dst[n,t,ho,wo,:] +) sum_j bilinear_{factors[j]}(srcs[j][n,t,:,:,:]) )
 * srcs / lds / factors are host arrays of J entries; source j is [NT, Ho / factors[j], Wo / factors[j], C] with row
 * stride lds[j] (every factor divides Ho and Wo).  Each term uses the arithmetic of mspi_upsample_fwd and the terms are added
 * left to right, so the result is bit-identical to J launches of mspi_upsample_fwd(accumulate = 1) (the first with the
 * caller's accumulate, the last with act). */
int mspi_upsample_sum_fwd(const float* const* srcs, const int64_t* lds, const int32_t* factors, int32_t J, float* dst,
                          int64_t ldd, int32_t NT, int32_t Ho, int32_t Wo, int32_t C, int32_t accumulate, int32_t act,
                          mspi_stream_t stream);

/* 2x2 spatial space-to-depth of Swin's PatchMerging (backbones/video_swin_transformer.py:311-326):
 * y[n,t,h,w, q*C + c] = x[n,t,2h+dh(q),2w+dw(q),c] with (dh,dw)(q) = (0,0),(1,0),(0,1),(1,1).  H, W even. */
int mspi_space_to_depth(const float* x, int64_t ldx, float* y, int64_t ldy, int32_t NT, int32_t H, int32_t W,
                        int32_t C, mspi_stream_t stream);

/* SA gating x*m + x (model/model_utils.py:167-170): x[m,:] *= (1 + mask[m]), in place. */
int mspi_rowgate(float* x, int64_t ldx, const float* mask, int64_t M, int32_t C, mspi_stream_t stream);

/* out[n,:] -= logsumexp(out[n,:]) over L elements per sample (model/model_utils.py:572). */
int mspi_logsumexp_sub(float* x, int32_t N, int32_t L, mspi_stream_t stream);

/* out[n,c] = mean over R rows of x[n,r,c] (nn.AdaptiveAvgPool, model/model_utils.py:402-403,543-544). */
int mspi_mean_rows(const float* x, int64_t ldx, int64_t rows_per_sample_stride, float* out, int32_t N,
                   int32_t R, int32_t C, mspi_stream_t stream);

/* The same mean for long samples (MorphFC re-weighting, backbones/MorphMLP.py:62,104: 25088 rows per sample): two
 * deterministic stages through a caller-owned workspace of N * mspi_mean_rows_slices(R) * C floats.
 * mspi_mean_rows_slices returns 0 when the one-stage mspi_mean_rows is the right call (R < 1024). */
int mspi_mean_rows_slices(int32_t R);
int mspi_mean_rows_ws(const float* x, int64_t ldx, int64_t rows_per_sample_stride, float* out, float* ws, int32_t N,
                      int32_t R, int32_t C, mspi_stream_t stream);

/* out[0] (+)= scale * mean_n( -cos(p[n,:], z[n,:]) )   (D(), model/model_utils.py:285-290). */
int mspi_neg_cosine(const float* p, const float* z, float* out, int32_t N, int32_t C, float scale,
                    int32_t accumulate, mspi_stream_t stream);

/* Saliency-map post-processing (inference.py:66-69,85-89; OpenCV upstream -- parity unpinned):
 * out[n] = uint8( round( 255 * minmax( resize_bilinear( exp( GaussianBlur11x11(logmap[n]) ), Ho x Wo ) ) ) ).
 * workspace: mspi_postprocess_workspace(...) bytes of device memory.  H, W >= 6: the blur reflects once, and for a map smaller
 * than its radius no reference defines the result (refused).
 * Holds no state: the 11 Gaussian taps are computed on the host in every call and travel to the blur kernel by value in its
 * arguments (a captured graph holds its own copy), so the first call of a process may be a captured one, and any device and
 * any thread may call (tests/test_launch_ledger.py: the cold-capture child and the second-device test). */
size_t mspi_postprocess_workspace(int32_t N, int32_t H, int32_t W, int32_t Ho, int32_t Wo);
int mspi_postprocess_u8(const float* logmap, unsigned char* out, void* workspace, int32_t N, int32_t H, int32_t W,
                        int32_t Ho, int32_t Wo, mspi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Grey JPEG encoding on the device (csrc/jpegenc.hip).  Replaces: cv2.imwrite of the uint8 map (inference.py:89-91).
 * Baseline sequential JPEG, one 8-bit component, 8x8 blocks in raster order, no restart markers, the Annex K luminance
 * Huffman tables: libjpeg's file byte for byte (integer "islow" FDCT, its quantiser rounding, jpeg_quality_scaling), which
 * is what PIL.Image.save(format="JPEG", quality=q) and cv2.imwrite write for a grey image. */
typedef struct MspiJpegDesc {
  int32_t B, H, W;              /* B maps [H, W] uint8; H, W in 1...65535 */
  int32_t quality;              /* 1...100 */
  int64_t pitch, map_stride;    /* bytes between rows / between maps; rows need no alignment */
  int64_t file_stride, cap;     /* files row b starts at b * file_stride; nothing is written at or beyond cap of a row */
  uint16_t div[64];             /* quantiser divisors 8 * q[k] in zigzag order: 8 * the DQT payload of the header */
  const void* header;           /* DEVICE copy of what mspi_jpeg_gray_header wrote for (H, W, quality) */
  int32_t header_len;
} MspiJpegDesc;

/* Host only (inference.py:89-91): SOI, APP0 (JFIF 1.01, units 0, density 1x1), DQT, SOF0, the DC and AC DHT segments and SOS
 * into dst[0, cap): 328 bytes, the bytes libjpeg's writer puts in front of the scan.  Returns the length or MSPI_EINVAL. */
int mspi_jpeg_gray_header(int32_t H, int32_t W, int32_t quality, unsigned char* dst, int64_t cap);
/* Host only (inference.py:89-91): the worst-case file size of an H x W map -- 20 + 63 * 26 bits per block, every scan byte
 * stuffed, header and EOI; 0 for H or W outside 1...65535. */
size_t mspi_jpeg_gray_bound(int32_t H, int32_t W);
/* Host only (inference.py:89-91): bytes of device workspace mspi_jpeg_gray_fwd needs (8-byte aligned); 0 for bad arguments. */
size_t mspi_jpeg_gray_ws_bytes(int32_t B, int32_t H, int32_t W);
/* Encode (inference.py:89-91): files[b * file_stride ...] = the JPEG file of maps[b], lengths[b] = its size in bytes.  Four
 * launches on `stream`, integer arithmetic only, bitwise reproducible.  Refuses (MSPI_EINVAL) null pointers, H or W outside
 * 1...65535, quality outside 1...100, divisors that are not the quality's, cap below mspi_jpeg_gray_bound(H, W) and maps
 * whose bound does not fit the int32 length. */
int mspi_jpeg_gray_fwd(const MspiJpegDesc* d, const unsigned char* maps, unsigned char* files, int32_t* lengths, void* ws,
                       mspi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * JPEG frame decoding on the device (csrc/jpegdec.hip).  Replaces: Image.open(path).convert('RGB') of the input frames
 * (inference.py:154-165).  Baseline sequential DCT (SOF0), 8 bit, one interleaved scan, no restart interval; one component
 * (grey, replicated to RGB) or YCbCr with 4:4:4, 4:2:2 (h2v1) or 4:2:0 (h2v2) sampling; any 8-bit DQT, any DHT; chroma width
 * >= 2.  The result is libjpeg-turbo's default decode pixel for pixel: integer "islow" IDCT, fancy up-sampling, its fixed-point
 * colour conversion.  Everything else is refused by the host parser and decoded by the caller on the host. */
typedef struct MspiJpegDecTables {   /* the tables of one image; B of them on the DEVICE for mspi_jpeg_dec_fwd */
  int32_t scan_len;                  /* bytes of entropy-coded data, stuffed zero bytes included */
  int32_t reserved;
  uint16_t quant[3][64];             /* the quantiser of each component, natural (row-major) order */
  uint8_t comp_dc[4], comp_ac[4];    /* Huffman table (0 / 1) of each component */
  uint8_t counts[4][16];             /* DC 0, DC 1, AC 0, AC 1: the number of codes of length 1...16 */
  uint8_t vals[4][256];              /* their symbols in code order */
} MspiJpegDecTables;
typedef struct MspiJpegDecInfo {
  int32_t H, W, ncomp;               /* ncomp 1 or 3 */
  int32_t hs, vs;                    /* sampling factors of the first component: 1x1, 2x1 or 2x2 (1x1 for ncomp 1) */
  int32_t scan_off, scan_len;        /* the entropy-coded bytes are file[scan_off, scan_off + scan_len) */
  int32_t reserved;
  MspiJpegDecTables tables;
} MspiJpegDecInfo;
typedef struct MspiJpegDecDesc {
  int32_t B, H, W, ncomp, hs, vs;    /* B images of one geometry */
  int32_t S;                         /* bits per subsequence: a multiple of 32, >= 128, ceil(8 * scan_cap / S) <= 1024 */
  int32_t reserved;
  int64_t scan_stride, scan_cap;     /* image b's scan starts at scans + b * scan_stride; every scan_len <= scan_cap */
  int64_t pitch, img_stride;         /* bytes between rows (>= 3 * W) and between images of rgb */
} MspiJpegDecDesc;

/* Host only (inference.py:154-165): walk the markers of file[0, n) and fill *info.  The scan ends at the first FF that is
 * followed by neither 00 nor an RST marker.  Returns MSPI_EINVAL, with the reason in mspi_last_error(), for what the device
 * does not decode: progressive, arithmetic coding, 12 bit, a restart interval, several scans, 4 components, an Adobe
 * transform other than 1, other sampling factors, 16-bit DQT, missing tables, empty or truncated headers. */
int mspi_jpeg_dec_parse(const unsigned char* file, int64_t n, MspiJpegDecInfo* info);
/* Host only (inference.py:154-165): bytes of device workspace mspi_jpeg_dec_fwd needs (16-byte aligned); 0 for a descriptor
 * it refuses. */
size_t mspi_jpeg_dec_ws_bytes(const MspiJpegDecDesc* d);
/* Decode (inference.py:154-165): rgb[b * img_stride + y * pitch + 3 * x + c] = the pixels of image b.  scans: the stuffed scan
 * bytes on the device; tables: B MspiJpegDecTables on the device, 8-byte aligned; status[b] = 0 when the scan held exactly the
 * expected blocks and ended inside its final byte (1 / 2: fewer / more blocks, 3: ended elsewhere; the pixels are then
 * undefined but stay inside the image); passes[b] = passes of the entropy decoder behind the first (the guess), the confirming one
 * included.  Launches on `stream` only (unstuff, entropy decode, DC prediction, IDCT, up-sample + convert, one memset), no
 * allocation, no host synchronisation, integer arithmetic only: bitwise reproducible.  Refuses (MSPI_EINVAL) null pointers,
 * bad sizes or sampling, pitch < 3 * W, a bad S and more than 1024 subsequences before any launch. */
int mspi_jpeg_dec_fwd(const MspiJpegDecDesc* d, const unsigned char* scans, const MspiJpegDecTables* tables, unsigned char* rgb,
                      int32_t* status, int32_t* passes, void* ws, mspi_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Fused channel MLP on rows:  y = res + W2 . act( W1 . LN(x) + b1 ) + b2,  the 4C-wide hidden
 * activation stays on the CU (csrc/mlp_fused.hip).  f16x3 split products, fp32 accumulate.
 * Replaces: timm ConvNeXt block norm -> mlp.fc1 -> GELU -> mlp.fc2 -> gamma -> + shortcut
 *   (via model/model_utils.py:361,380), and the LN -> Mlp -> residual tail of
 *   SwinTransformerBlock3D.forward_part2 (backbones/video_swin_transformer.py:262-263) and
 *   MultiScaleBlock (backbones/MViT.py:1420-1432) when dim_out == dim.
 * C in {96, 192}; hidden a multiple of 32, <= 1024; x, res, y row-major with strides ldx/ldr/ldy.
 * w_packed: mspi_mlp_packed_bytes(C, hidden) bytes of f16, per hidden chunk j of 32 units
 *   W1 part [ks < C/16][hi,lo][lane < 64][e < 8] = W1s[j*32 + lane%32][16 ks + 8 (lane/32) + e]
 *   W2 part [s < 2][ct < C/32][hi,lo][lane][e]   = W2s[ct*32 + lane%32][j*32 + (2s + e/4)*8 + 4 (lane/32) + e%4]
 * with W1s = w1_scale * fc1.weight [hidden, C], W2s = w2_scale * (out_scale (.) fc2.weight) [C, hidden],
 * hi = f16(Ws), lo = f16(Ws - hi)  (engine.pack_mlp builds it). */
typedef struct {
  int64_t M;                 /* rows */
  int32_t C, hidden;
  int64_t ldx, ldr, ldy;     /* row strides in floats */
  int32_t ln;                /* 1: LayerNorm over C (gamma, beta, eps) applied to x first */
  int32_t act;               /* MSPI_ACT_* between the two layers */
  float eps;
  float w1_scale, w2_scale;  /* powers of two the packed weights were multiplied by */
} MspiMlpDesc;
size_t mspi_mlp_packed_bytes(int32_t C, int32_t hidden);
int mspi_mlp_fwd(const MspiMlpDesc* d, const void* x, const void* gamma, const void* beta, const void* w_packed,
                 const void* b1, const void* b2, const void* res, void* y, mspi_stream_t stream);
/* Which instantiation mspi_mlp_fwd launches (host only; MSPI_MLP_TM is read once per process): mlp_fused_kernel<C, TM, NS, NWV>
 * as C * 1000 + TM * 100 + NS * 10 + NWV; -1 = a descriptor the launch refuses.  mspi_mlp_fwd selects by this function. */
int mspi_mlp_variant(const MspiMlpDesc* d);

/* ------------------------------------------------------------------------------------
 * Row-stationary thin GEMM (1x1x1 conv / Linear with K <= 224 and few output columns):
 *   y[M, N] = act( x'[M, K] . W^T + bias (+ res) ),   x' = x, or swish(x * gate[row / rows_per_sample]) when gate != NULL.
 * Same contract as mspi_conv_fwd on a dense 1x1x1 stride-1 problem; a different kernel (csrc/mlp_fused.hip) and a
 * different weight packing.  Replaces: X3DTransform.a / .c (SlowFast/resnet_helper.py:296-351, with the SE scale :333
 * and Swish :339 as the gate prologue), ResBlock.branch1 (:540-556), X3D conv5 pieces (backbones/X3D.py).
 * K, N: storage columns of x / y (multiples of 4, pad columns zero).  mspi_rowgemm_supported(K, N) says whether the
 * shape is covered (K <= 224, N <= 1024).
 * w_packed: mspi_rowgemm_packed_bytes(K, N) bytes of f16; with KSB = 2, 4, 8 or 14 k-steps of 16 (the smallest
 * covering K) and Ws = w_scale * W [N, K] zero-padded:  [chunk j < ceil(N/32)][ks < KSB][hi,lo][lane < 64][e < 8]
 *   = Ws[j*32 + lane%32][16 ks + 8 (lane/32) + e]   (engine.pack_rowgemm builds it). */
typedef struct {
  int64_t M;
  int32_t K, N;
  int64_t ldx, ldr, ldy, ldg;   /* row strides in floats (ldg: gate rows) */
  int32_t act;
  int32_t rows_per_sample;      /* gate row index = row / rows_per_sample */
  float w_scale;
} MspiRowGemmDesc;
size_t mspi_rowgemm_packed_bytes(int32_t K, int32_t N);
int mspi_rowgemm_supported(int32_t K, int32_t N);
int mspi_rowgemm_fwd(const MspiRowGemmDesc* d, const void* x, const void* w_packed, const void* bias, const void* res,
                     const void* gate, void* y, mspi_stream_t stream);
/* Which instantiation mspi_rowgemm_fwd launches (host only): rowgemm_kernel<KSB, GATE> as KSB * 10 + GATE, has_gate = a gate
 * is given; -1 = a descriptor the launch refuses.  mspi_rowgemm_fwd selects by this function. */
int mspi_rowgemm_variant(const MspiRowGemmDesc* d, int32_t has_gate);

/* ------------------------------------------------------------------------------------
 * X3D block seam, one launch for the end of block i and the start of block i+1 of a stage (csrc/mlp_fused.hip):
 *   y[M, Cx] = relu( u'[M, D] . Wc^T + bc + res ),   u' = u, or swish(u * gate[row / rows_per_sample]) when gate != NULL
 *   t[M, D]  = relu( y . Wa^T + ba )
 * Replaces: X3DTransform.c + c_bn, the residual add and ReLU of ResBlock.forward (SlowFast/resnet_helper.py:339-351,
 * :607-616), followed by the next block's X3DTransform.a + a_bn + a_relu (:296-307); the SE scale (:333) and Swish
 * (:339) of block i are the gate prologue, as in mspi_rowgemm_fwd.  Results are those of the two mspi_rowgemm_fwd
 * calls it stands for, up to fp32 summation order.
 * D: stored columns of u and t (the stage's inner width, <= 224), Cx: stored columns of res and y (<= 256); multiples of 4.
 * w_packed: mspi_x3d_ca_packed_bytes(D, Cx) bytes = mspi_mlp_fwd's packing with C = D padded to 128 or 224,
 * hidden = Cx padded to 32, W1s = wc_scale * Wc [Cx, D], W2s = wa_scale * Wa [D, Cx], zero padding (engine.pack_x3d_ca). */
typedef struct {
  int64_t M;
  int32_t D, Cx;
  int64_t ldu, ldr, ldy, ldt, ldg;   /* row strides in floats */
  int32_t rows_per_sample;
  float wc_scale, wa_scale;
} MspiX3dCaDesc;
size_t mspi_x3d_ca_packed_bytes(int32_t D, int32_t Cx);
int mspi_x3d_ca_supported(int32_t D, int32_t Cx);
int mspi_x3d_ca_fwd(const MspiX3dCaDesc* d, const void* u, const void* gate, const void* w_packed, const void* bc,
                    const void* ba, const void* res, void* y, void* t, mspi_stream_t stream);
/* Which instantiation mspi_x3d_ca_fwd launches (host only): x3d_ca_kernel<C, GATE> as C * 10 + GATE (C = D padded to 128 or
 * 224), has_gate = a gate is given; -1 = a descriptor the launch refuses.  mspi_x3d_ca_fwd selects by this function. */
int mspi_x3d_ca_variant(const MspiX3dCaDesc* d, int32_t has_gate);

/* Saliency metrics (utils/compute_saliency_metrics.py:9-108; the terms of utils/loss.py:26-49): per sample n,
 * out[n] = { KL(gt || pred), CC(pred, gt), SIM(pred, gt), NSS(pred, fix) } over the L = H*W values of each map.
 * pred is the predicted map (pred_is_log: the model's log-probability map, exponentiated on the fly), gt the
 * ground-truth density, fix the binary fixation map (NULL: NSS is written as 0).  Batch means are the caller's. */
int mspi_saliency_metrics(const float* pred, const float* gt, const float* fix, float* out /*[N][4]*/, int32_t N, int32_t L,
                          int32_t pred_is_log, mspi_stream_t stream);

/* AUC-Judd (utils/compute_saliency_metrics.py:111-203, a port of the MIT benchmark's AUC_Judd), one score per map.
 * sal holds N maps of L values, float (is_f64 = 0: the reference's jitter=False arithmetic) or double (is_f64 = 1: the
 * caller has added the jitter noise, :150, which promotes the map to float64 upstream); fix is the fixation map
 * (a pixel is a fixation where fix > 0).  Per map: min-max normalisation with an IEEE division in the map's own type
 * (:153-154), the normalised values at the n fixations sorted descending as thresholds (:164-168),
 * above[i] = #{S >= thresh[i]} over all L pixels as integer counts (:176), tp / fp in float64 (:177-179) and the
 * trapezoid of tp over fp (:182).  score[m] is NaN for a map without fixations (:133-136) or a constant map (0/0
 * everywhere, :156-159); nfix[m] = n.  Any n is accepted; n = L divides by zero as upstream does.  Three launches
 * (range + compaction + sort; the pixel pass over several workgroups per map; scan + trapezoid), integer atomics
 * only: bitwise reproducible.  ws: mspi_saliency_auc_ws_bytes(N, L) bytes of device scratch, 16-byte aligned. */
size_t mspi_saliency_auc_ws_bytes(int32_t N, int32_t L);
int mspi_saliency_auc_judd(const void* sal, int32_t is_f64, const float* fix, double* score /*[N]*/, int32_t* nfix /*[N]*/,
                           void* ws, int32_t N, int32_t L, mspi_stream_t stream);

/* The device part of shuffled AUC (utils/compute_saliency_metrics.py:206-276): per map of H x W floats, after the float32
 * min-max normalisation of normalize_map (:33-43, IEEE division), with th_k = (float)(k / 10), k = 1..9 (numpy compares a
 * float32 array with a Python float in float32):
 *   counts[m][k-1]     = #{ (s >= th_k ? 1 : 0) + gt == 2 }                        (:258-260)
 *   counts[m][9 + k-1] = #{ other-fixations whose looked-up value r > th_k }       (:265)
 *   counts[m][18]      = #{ gt == 1 }   (sum(gt) of a binary map, :221)
 *   counts[m][19]      = #{ other == 1 }                                           (:223-227)
 * An other-fixation at (row, col) is encoded as k = row * H + col (:226, H not W) and read back as
 * s[k % H - 1][k / H] with row -1 wrapping to H - 1 (:246); that stays inside the map only for H <= W, so H > W is
 * refused (upstream raises IndexError).  Every split of the reference permutes ALL other-fixations and only counts, so
 * the splits are equal and one evaluation suffices; round(x, 4), the sort of the 11 points and the trapezoid
 * (:267-274) are a few float64 operations on these counts and are the host's. */
int mspi_saliency_sauc_counts(const float* sal, const float* gt, const float* other, int32_t* counts /*[N][20]*/, int32_t N,
                              int32_t H, int32_t W, mspi_stream_t stream);

/* Information gain over a baseline map (utils/compute_saliency_metrics.py:278-308): per map, with every map divided by
 * its own sum, out[m] = sum(gt * (log(eps + pred) - log(eps + base))), eps = 2.2204e-16.  Batch means are the caller's. */
int mspi_saliency_ig(const float* pred, const float* gt, const float* base, float* out /*[N]*/, int32_t N, int32_t L,
                     mspi_stream_t stream);

/* The training criterion with its gradient (utils/loss.py:26-49: kl - cc [- 0.1 nss] of the model's LOG map).
 * mspi_saliency_loss_fwd writes the four per-sample values of mspi_saliency_metrics(..., pred_is_log = 1) to terms
 * (fix NULL: NSS is written as 0) and leaves the per-sample statistics of the backward in ws.  Each sample is split over
 * chunks of 2048 values on a (chunks, N) grid: pass one writes per-chunk sums, ranges and chunk-centred moments, pass two
 * merges them about the sample mean and writes the KL / SIM sums, a one-wave launch per sample finishes.  Partials are
 * combined in a fixed order, no float atomics: bitwise repeatable.
 * mspi_saliency_loss_bwd is one element-wise pass:
 *   dlog = *grad_out * d(w_kl KL - w_cc CC - w_nss NSS) / d logmap,
 * every sample with the same weights (the caller folds the 1/N of a batch mean into them); fix NULL or w_nss == 0 drops the
 * NSS term and its load.  grad_out is a DEVICE scalar read by the kernel.  logmap / gt / fix must be the arrays the forward
 * saw.  16-byte loads and stores on every row whose base is 16-byte aligned in all arrays, 4-byte ones on the others.
 * Neither call synchronises or allocates (graph capture safe).  ws: mspi_saliency_loss_ws_bytes(N, L) bytes of device
 * scratch, 16-byte aligned; the query is host arithmetic, 0 for N <= 0 or L <= 1.  N <= 65535. */
size_t mspi_saliency_loss_ws_bytes(int32_t N, int32_t L);
int mspi_saliency_loss_fwd(const float* logmap, const float* gt, const float* fix /*may be NULL*/, float* terms /*[N][4]*/,
                           void* ws, int32_t N, int32_t L, mspi_stream_t stream);
int mspi_saliency_loss_bwd(const float* logmap, const float* gt, const float* fix /*may be NULL*/, const void* ws,
                           const float* grad_out /*device scalar*/, float w_kl, float w_cc, float w_nss, float* dlog /*[N][L]*/,
                           int32_t N, int32_t L, mspi_stream_t stream);

/* Backward of the decoder's readout tail (csrc/readout_bwd.hip): conv (4,1,1)/4 64 -> 32, x4 bilinear up-sample + ReLU,
 * conv (1,3,3) 32 -> 32 + ReLU, conv (1,3,3) 32 -> 1, x - logsumexp(x).  Sums that cross a workgroup go through the caller's
 * workspace as per-workgroup records and a second launch adds the records in a fixed order: no float atomics, bitwise
 * repeatable.  No call allocates or synchronises.  Workspaces are device scratch, 16-byte aligned.
 *
 * mspi_logsumexp_sub_bwd: dz[n][i] = g[n][i] - exp(logp[n][i]) * sum_i g[n][i]; logp is the forward's output.  One
 * workgroup per sample.
 *
 * mspi_conv_c1_bwd: the last conv (1,3,3) pad (0,1,1) C -> 1 and the ReLU in front of it, one pass over y [M = N*H*W][C]
 * (the saved post-ReLU activations, row stride ldy), dz [N][H][W], w [9][C] (tap (kh,kw), channel fastest):
 *   d[p][c]    = (y[p][c] > 0) * sum_tap dz[p - tap] * w[tap][c]     (row stride ldd; zero padding per image)
 *   dW[tap][c] = sum_p dz[p - tap] * y[p][c],   db[0] = sum dz
 * Workgroups of 1024 rows; ws: mspi_conv_c1_bwd_ws_bytes(N, H, W) bytes (host arithmetic, 0 for an empty extent).
 * C % 4 == 0, C <= 64; y, d, w 16-byte aligned, ldy and ldd multiples of 4.
 *
 * mspi_conv_wgrad_fwd: weight gradient of the convolution `d` describes (the forward's descriptor; ldy = row stride of dy,
 * the weight, activation and precision members are not read): dW[co][(kt,kh,kw,ci)] = sum_m dy[m][co] * x[pos(m, tap)][ci]
 * dense [Cout][kT*kH*kW*C] fp32 (the row order of the forward's weights, unscaled) and db[co] = sum_m dy[m][co].  The rows
 * are the contraction of v_mfma_f32_32x32x2_f32 (an exact fp32 fmaf chain); they are split into slices of 256 rows, 2048
 * from 65536 rows on, one slice and three (tap, 32-channel) tiles per workgroup.  Supported: stored Cout <= 32 and C <= 64,
 * both multiples of 4, at most 27 taps, sC == 1, fewer than 2^31 rows, x and dy 16-byte aligned.
 * mspi_conv_wgrad_supported: 1 or 0 for the descriptor alone; mspi_conv_wgrad_variant: the slice length in rows, or -1 for
 * exactly what the launch refuses (descriptor or pointers), the reason in mspi_last_error(); mspi_conv_wgrad_ws_bytes: host
 * arithmetic, 0 for a refused descriptor.
 *
 * mspi_upsample_bwd: adjoint of mspi_upsample_fwd (same factor, source coordinates and edge clamping): dx [NT][H][W][C] from
 * dy [NT][H*factor][W*factor][C], one thread per source vector gathering the <= 2 factor x 2 factor destination cells that
 * tap it.  act == MSPI_ACT_RELU: u is the forward's output (row stride ldu) and cells with u <= 0 are skipped -- the mask
 * of the ReLU in the forward's epilogue; MSPI_ACT_NONE: u is not read.  C % 4 == 0, factor 2, 4 or 8. */
int mspi_logsumexp_sub_bwd(const float* logp, const float* g, float* dz, int32_t N, int32_t L, mspi_stream_t stream);
size_t mspi_conv_c1_bwd_ws_bytes(int32_t N, int32_t H, int32_t W);
int mspi_conv_c1_bwd(const float* y, int64_t ldy, const float* dz, const float* w, float* d, int64_t ldd, float* dW /*[9][C]*/,
                     float* db /*[1]*/, void* ws, int32_t N, int32_t H, int32_t W, int32_t C, mspi_stream_t stream);
int mspi_conv_wgrad_supported(const MspiConvDesc* d);
size_t mspi_conv_wgrad_ws_bytes(const MspiConvDesc* d);
int mspi_conv_wgrad_variant(const MspiConvDesc* d, const void* x, const void* dy);
int mspi_conv_wgrad_fwd(const MspiConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                        mspi_stream_t stream);
int mspi_upsample_bwd(const float* dy, int64_t ldy, const float* u /*NULL without ReLU*/, int64_t ldu, float* dx, int64_t ldx,
                      int32_t NT, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t act, mspi_stream_t stream);

/* Training kernels for the convs in front of the readout tail (csrc/readout_train.hip).  fp32; every entry point is bitwise
 * repeatable: sums that cross a workgroup go through `ws` as per-workgroup records added (merged) in a fixed order.
 *
 * mspi_conv_wgrad_wide_fwd: mspi_conv_wgrad_fwd's result (dW dense [Cout][kT*kH*kW*C], db [Cout]) for wide layers: stored
 * C and Cout multiples of 32, each at most 192, at most 27 taps, stride 1, sC == 1, input strides and ldy multiples of 4,
 * fewer than 2^31 rows, x and dy 16-byte aligned.  A workgroup owns a (32 x 32)-channel pair with all its taps and a slice
 * of the rows; it stages boxes of at most 128 output positions -- its columns of dy and its channels of x over the box grown
 * by the kernel's halo -- through LDS once each, and every tap reads from there (v_mfma_f32_32x32x2_f32, rows as the
 * contraction).  A slice is 4 boxes, 32 from 512 boxes on; a 1x1x1 kernel over dense rows takes boxes of 128 consecutive rows.
 * mspi_conv_wgrad_wide_supported: 1 or 0 for the descriptor alone; mspi_conv_wgrad_wide_variant: boxes per slice, or -1 for
 * exactly what the launch refuses, the reason in mspi_last_error(); mspi_conv_wgrad_wide_ws_bytes: host arithmetic, 0 for a
 * refused descriptor.
 *
 * BatchNorm on batch statistics over rows [M][C], C a multiple of 4 up to 192, M >= 2 (M == 1 is refused by name, as torch
 * refuses it); row strides multiples of 4, every pointer 16-byte aligned; ws: mspi_bn_ws_bytes(M, C) bytes.
 * mspi_bn_stats: mean, biased variance and rstd = 1 / sqrt(var + eps) per channel.  Groups of 512 rows give (mean, M2)
 * records from sums shifted by the group's first row; a second launch merges them left to right by Chan's formula.
 * mspi_bn_apply: y = gamma (x - mean) rstd + beta, then ReLU when act == MSPI_ACT_RELU (MSPI_ACT_NONE otherwise).
 * mspi_bn_bwd: dbeta = sum dy, dgamma = sum dy x^, dx = gamma rstd (dy - dbeta / M - x^ dgamma / M) with x^ = (x - mean) rstd
 * recomputed from the pre-norm x.  y != NULL: the forward's post-ReLU output, dy counts only where y > 0.  Three launches:
 * group sums, their ordered add, the apply. */
int mspi_conv_wgrad_wide_supported(const MspiConvDesc* d);
size_t mspi_conv_wgrad_wide_ws_bytes(const MspiConvDesc* d);
int mspi_conv_wgrad_wide_variant(const MspiConvDesc* d, const void* x, const void* dy);
int mspi_conv_wgrad_wide_fwd(const MspiConvDesc* d, const float* x, const float* dy, float* dW, float* db, void* ws,
                             mspi_stream_t stream);
size_t mspi_bn_ws_bytes(int64_t M, int32_t C);
int mspi_bn_stats(const float* x, int64_t ldx, int64_t M, int32_t C, float eps, float* mean, float* var, float* rstd, void* ws,
                  mspi_stream_t stream);
int mspi_bn_apply(const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma, const float* beta,
                  float* y, int64_t ldy, int64_t M, int32_t C, int32_t act, mspi_stream_t stream);
int mspi_bn_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* y /*NULL without ReLU*/, int64_t ldy,
                const float* mean, const float* rstd, const float* gamma, float* dx, int64_t lddx, float* dgamma, float* dbeta,
                void* ws, int64_t M, int32_t C, mspi_stream_t stream);

/* Bilinear resize of N maps [H][W] -> [Ho][Wo], what upstream does with cv2.resize(..., INTER_LINEAR default) when it brings
 * the prediction to the fixation map's size (utils/compute_saliency_metrics.py:119-122) and the density to the model's size
 * (avsp_dataloader.py:176).  src is uint8 (src_is_u8 != 0: a decoded image, values used as 0..255, unscaled) or float; dst is
 * float.  Pixel centres aligned, src = (dst + 0.5) * in / out - 0.5, edges clamped, no antialiasing when shrinking.  The
 * source index and its fractional weight are exact integer arithmetic, the weight rounded once to fp32; the arithmetic on
 * the samples is fp32 (at most 13 roundings per output, each <= 2^-24 max|src|).  Ho == H && Wo == W copies (converts) bit
 * for bit.  One launch, 16-byte stores; extents up to 2^23.  Parity with OpenCV's own fixed-point path is not pinned. */
int mspi_resize_bilinear_fwd(const void* src, int32_t src_is_u8, float* dst, int32_t N, int32_t H, int32_t W, int32_t Ho,
                             int32_t Wo, mspi_stream_t stream);

/* resize_fixation (avsp_dataloader.py:16-31) for N fixation maps [H][W] -> [row][col]: every non-zero input pixel (r, c) sets
 * dst[min(rint(r * (row / H)), row - 1)][min(rint(c * (col / W)), col - 1)] = 1, everything else is 0.  The ratio is the
 * float64 quotient the reference forms first (:18-19), the product float64, the rounding half to even (np.round, :23-24):
 * equal to the reference bit for bit, shrinking, enlarging or identity.  Two launches on `stream`: a zero fill of dst, then
 * stores of the constant 1.0f from the non-zero inputs (sources that share a target write the same value). */
int mspi_resize_fixation_fwd(const float* fix, float* dst, int32_t N, int32_t H, int32_t W, int32_t row, int32_t col,
                             mspi_stream_t stream);

/* MorphMLP token regrouping (backbones/MorphMLP.py:49-58,87-100,134-137: the reshape/permute/reshape chains around
 * mlp_h / mlp_w / mlp_t) as ONE strided gather: y is dense with extents dims[0..5] (dims[5] innermost),
 * y[i0..i5] = x[sum_k i_k * strides[k]]; strides[5] must be 1, src_elems bounds the reads. */
typedef struct MspiPermuteDesc {
  int32_t dims[6];
  int64_t strides[6];
  int64_t src_elems;
} MspiPermuteDesc;
int mspi_permute_fwd(const MspiPermuteDesc* d, const float* x, float* y, mspi_stream_t stream);
/* Which instantiation mspi_permute_fwd launches (host only, no GPU call; x and y are only inspected for alignment):
 * 4 = 16-byte vectors (dims[5] % 4 == 0, strides[0..4] % 4 == 0, both pointers 16-byte aligned), 1 = scalar; -1 = a
 * descriptor the launch refuses.  mspi_permute_fwd selects its kernel by this same function. */
int mspi_permute_variant(const MspiPermuteDesc* d, const float* x, const float* y);

/* MorphFC re-weighting (backbones/MorphMLP.py:64-67,104-107): y[n,r,c] = sum_j softmax_j(logit[n, c*J + j]) * src_j[n,r,c]
 * over dense [N, rows_per_sample, C] operands; J = 3 (a, b, c) or 2 (a, b; c may be NULL). */
int mspi_gated_sum_fwd(const float* a, const float* b, const float* c, const float* logit, float* y, int32_t N,
                       int64_t rows_per_sample, int32_t C, int32_t J, mspi_stream_t stream);

/* Log-spectrogram windows of the clip loop (inference.py:24-63: torchaudio Spectrogram(n_fft=512, hop_length=160) on
 * audio[start:end] (optionally time-reversed), log(p + 1e-6), per-column standardisation over the 257 bins with the
 * unbiased std, crop / pad with 0.02 to Wa columns).  wave: 16 kHz mono samples on the device; seg [B][3] =
 * (start, length, reversed) on the device, seg_host the same table on the host (bounds are validated before the launch);
 * window: 512 Hann coefficients on the device; out [B][257][Wa]. */
int mspi_logspec_fwd(const float* wave, int64_t n_wave, const int32_t* seg, const int32_t* seg_host, int32_t B,
                     const float* window, float* out, int32_t Wa, mspi_stream_t stream);

/* Frame pre-processing (inference.py:154-165: torchvision Resize on a PIL image = PIL's antialiased bilinear resampling,
 * ToTensor, Normalize).  rgb: uint8 [Hin][Win][3] on the device; tmp: Hin*Wout*3 bytes of device scratch; out: fp32
 * [3][Hout][Wout] planes `out_plane_stride` floats apart.  hb/vb: [n][2] = (first input index, taps) per output
 * column / row, hk/vk: [n][hks|vks] 22-bit fixed-point taps -- PIL's precompute_coeffs + normalize_coeffs_8bpc tables,
 * built by the caller (mspi_amd/preproc.py) and resident on the device; mean3/std3: host floats. */
int mspi_resize_norm_fwd(const unsigned char* rgb, int32_t Hin, int32_t Win, unsigned char* tmp, float* out,
                         int64_t out_plane_stride, int32_t Hout, int32_t Wout, const int32_t* hb, const int32_t* hk,
                         int32_t hks, const int32_t* vb, const int32_t* vk, int32_t vks, const float* mean3_host,
                         const float* std3_host, mspi_stream_t stream);

/* Clip assembly: N decoded frames of ONE source size -> their slots of a fp32 [B][3][T][Hout][Wout] clip tensor, the
 * arithmetic of mspi_resize_norm_fwd (bit for bit) in one launch, without a scratch buffer: a workgroup stages the
 * horizontally resampled rows its output tile taps in LDS and runs the vertical pass from there.  frames: uint8
 * [N][Hin][Win][3], packed, 4-byte aligned, on the device; slots [N]: frame i goes to out[b][:][t] with b * T + t = slots[i]
 * (device table; slots_host is the same table on the host: every slot is checked to be < B * T and written once before the
 * launch); element (b, c, t, y, x) of out is at b * sB + c * sC + t * sT + y * sH + x floats.  hb / hk / vb / vk: as for
 * mspi_resize_norm_fwd; hb_host / vb_host: host copies of the two bounds tables (checked against Win / Hin, and the tile
 * height is planned from vb_host).  Returns MSPI_EINVAL without launching where no tile fits the LDS budget
 * (mspi_clip_resize_plan tells in advance); the caller then runs mspi_resize_norm_fwd per frame.
 * mspi_clip_resize_plan (host only): plan4 = { output rows per tile, staged rows per tile (tile k stages the input rows
 * [vb[k * TH][0], + staged)), input rows per load batch, LDS bytes per workgroup }. */
int mspi_clip_resize_plan(const int32_t* vb_host, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout, int32_t vks,
                          int32_t* plan4);
int mspi_clip_resize_norm_fwd(const unsigned char* frames, int32_t N, int32_t Hin, int32_t Win, const int32_t* slots,
                              const int32_t* slots_host, float* out, int32_t B, int32_t T, int64_t sB, int64_t sC, int64_t sT,
                              int64_t sH, int32_t Hout, int32_t Wout, const int32_t* hb, const int32_t* hb_host,
                              const int32_t* hk, int32_t hks, const int32_t* vb, const int32_t* vb_host, const int32_t* vk,
                              int32_t vks, const float* mean3_host, const float* std3_host, mspi_stream_t stream);

/* Pre-split activations.  The f16x3 GEMM computes x*w from f16 hi/lo halves of both operands; the weights are split at pack
 * time, and a producer may hand the activations over ALREADY split: two f16 planes (hi plane, lo plane `plane` elements
 * later; hi = f16(x), lo = f16(x - hi) -- the same split the kernels otherwise do in registers, so results are
 * bit-identical).  Each plane is BLOCKED: K % 32 == 0, the row count is padded to a multiple of 16, and element (m, k) sits at
 *     ((m / 16) * (K / 32) + k / 32) * 512 + (m % 16) * 32 + k % 32        (halves)
 * i.e. a 16-row x 32-column block is 1 KB contiguous and the blocks of a row group follow each other along k: the k32 stage
 * of a 16-row group is one contiguous 1-KB LDS-DMA piece of 8 full cache lines (row-major planes hand the loader 16 half
 * lines per piece: 30 instead of 43 B/clk/CU of fill, tools/dma_issue_probe.hip).  `ld` arguments of planes must equal K;
 * `plane` >= roundup16(M) * K; the pad rows are read (never stored): keep them finite.
 * mspi_gemm_sp_fwd is the dense (1x1x1 / nn.Linear) GEMM on such planes: both operands go HBM -> LDS -> MFMA with no
 * conversion work in the loop.  d: as for mspi_conv_fwd with C % 32 == 0, ldw == C, prec f16x3; `w`: the f16 hi/lo weight
 * planes of mspi_conv_fwd BLOCKED the same way (rows = output channels, zero-padded to a multiple of 16; lo plane
 * roundup16(Cout) * K halves after the hi plane; engine.sp_weights builds it);
 * d->tile: the last column of the table at MspiConvDesc.tile.  The result goes to y
 * (fp32 rows, ldy) or, when y_planes != NULL, to blocked output planes (ldys == Cout, Cout % 32 == 0) for the next GEMM.
 * mspi_split_planes_fwd converts fp32 rows. */
int mspi_layernorm_sp_fwd(const float* x, int64_t ldx, int64_t sample_stride_x, void* planes, int64_t ldo, int64_t plane,
                          const float* gamma, const float* beta, float eps, int32_t N, int32_t R, int32_t C, int32_t act,
                          mspi_stream_t stream);   /* mspi_layernorm_fwd writing pre-split planes (rows dense, n*R + r) */
int mspi_split_planes_fwd(const float* x, int64_t ldx, int64_t M, int32_t K, void* planes, int64_t ldo, int64_t plane,
                          mspi_stream_t stream);
/* planes -> fp32 rows (hi + lo): for a consumer that was moved off the f16x3 path after its producer had emitted planes */
int mspi_join_planes_fwd(const void* planes, int64_t ldi, int64_t plane, int64_t M, int32_t K, float* y, int64_t ldy,
                         mspi_stream_t stream);
int mspi_gemm_sp_fwd(const MspiConvDesc* d, const void* x_planes, int64_t ldx, int64_t xplane, const float* w,
                     const float* bias, const float* res, float* y, void* y_planes, int64_t ldys, int64_t yplane,
                     mspi_stream_t stream);
/* Which instantiation mspi_gemm_sp_fwd launches for this descriptor (host only; y_planes is looked at for NULL only):
 *   kind * 10000000 + BM * 10000 + BN * 10 + form,  kind 6 = 128 rows / 4 waves, 7 = 256 rows / 8 waves,
 * form 0 = fp32 rows out, 1 = blocked planes out; -1 = a descriptor the launch refuses (mspi_last_error() says why).
 * mspi_gemm_sp_fwd selects by this function; the plane strides are checked at launch only. */
int mspi_gemm_sp_variant(const MspiConvDesc* d, const void* y_planes);

/* y = a + b over n floats (plain residual add where no producer can fuse it). */
int mspi_add(const float* a, const float* b, float* y, int64_t n, mspi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MSPI_HIP_H */
