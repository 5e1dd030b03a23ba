"""Host-side plumbing between the reference-shaped nn.Modules and the C ABI.

* `CL`   -- a channels-last activation: M = N*T*H*W rows x C columns, row stride `ld`
            (floats, multiple of 4) inside a flat fp32 torch buffer.  Slicing channels is free,
            which is how concats are eliminated (producers write into their slice).
* pack_* -- weight packing, done once per parameter version: packs.py, whose names are re-exported here.
* op wrappers -- conv / dwconv / layernorm / ... : fill the POD descriptor, pass raw device
            pointers and torch's current hipStream_t.  No CPU fallback anywhere.
"""
import ctypes as C
import os as _os
from functools import partial

import numpy as np
import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SWISH, PREC_F16X3, PREC_F32, AttnDesc, ConvDesc,
                   DwConvDesc, MspiError, MvitAugDesc, check)
from .packs import (DEFAULT_PREC, SP_ENABLED, PackedConv, PackedDw, PackedMlp, PackedX3dAb, PackedX3dCa, PackedX3dStem,
                    _pack_rowgemm, _pad_vec, fold_bn, mlp_supported, pack_conv, pack_dwconv, pack_mlp, pack_mlp_tail,
                    pack_x3d_ab, pack_x3d_ab_s2, pack_x3d_ca, pack_x3d_stem, rowgemm_ksb, rowgemm_supported, rup4,
                    sp_supported, sp_weights, x3d_ca_supported)

__all__ = ["CL", "SP", "alloc", "alloc_sp", "pack_conv", "pack_dwconv", "PackedConv", "PackedDw", "conv", "dwconv", "maxpool",
           "layernorm", "attention", "upsample", "upsample_sum", "rowgate", "logsumexp_sub", "mean_rows", "neg_cosine", "se_gate",
           "add", "fold_bn", "conv_wgrad", "conv_c1_bwd", "upsample_bwd", "logsumexp_sub_bwd", "conv_wgrad_wide",
           "conv_wgrad_wide_variant", "bn_stats", "bn_apply", "bn_bwd", "rowgate_bwd", "upsample_sum_bwd", "gelu_bwd",
           "layernorm_bwd", "dwconv_wgrad", "conv_wgrad_entry", "conv_wgrad_entry_variant", "conv_wgrad_t16",
           "conv_wgrad_t16_variant", "attention_bwd", "layernorm_bwd_wide", "linear_wgrad",
           "linear_wgrad_variant", "neg_cosine_bwd", "layernorm_act_bwd", "mean_rows_bwd", "dwconv3_wgrad", "bn_gate_act",
           "gate_swish_bwd", "se_train_fwd", "se_train_bwd", "relu_mask_add", "ACT_NONE", "ACT_RELU", "ACT_GELU", "ACT_SIGMOID", "ACT_SWISH"]


# ----------------------------------------------------------------------------- conv autotuning
# Like cudnn.benchmark (which the reference switches on, inference.py:189): the first time a conv shape is seen
# with autotuning enabled, every kernel instantiation that applies is timed on the real tensors and the fastest is
# remembered.  Off by default (tile -1 = the library's heuristic); bench.py / inference enable it before the
# hipGraph is captured.  The cache is keyed by the GEMM shape, so it is shared by all layers with that shape.
AUTOTUNE = {"on": _os.environ.get("MSPI_AUTOTUNE", "0") == "1", "cache": {}, "reps": 3}


def autotune(on=True):
    AUTOTUNE["on"] = bool(on)


def save_autotune(path):
    """Write the tile choices made so far (MIOpen's find-db role): {repr(shape key): tile code}."""
    import json
    with open(path, "w") as f:
        json.dump({repr(k): v for k, v in AUTOTUNE["cache"].items()}, f, indent=0, sort_keys=True)


def load_autotune(path):
    """Adopt tile choices saved by save_autotune; shapes not in the file fall back to the library heuristic
    (or are tuned, when autotune is on).  Returns the number of entries."""
    import ast
    import json
    with open(path) as f:
        AUTOTUNE["cache"].update({ast.literal_eval(k): int(v) for k, v in json.load(f).items()})
    return len(AUTOTUNE["cache"])


THIN = 100            # kernel choice "row-stationary thin GEMM" next to MspiConvDesc.tile codes 0..14
SPLITK = 200          # kernel choice SPLITK + S: split-K with S slices (mspi_conv_splitk_fwd)
SPLITK_ENABLED = _os.environ.get("MSPI_SPLITK", "1") != "0"   # A/B switch
HALO = 300            # kernel choice "halo-staged implicit GEMM" (mspi_conv_halo_fwd): stride-1 (1|3,3,3) convs, C % 32 == 0
HALO_ENABLED = _os.environ.get("MSPI_CONV_HALO", "1") != "0"   # A/B switch
THIN_DEFAULT = True   # without autotuning: take the thin kernel wherever it applies
THIN_ENABLED = _os.environ.get("MSPI_THIN", "1") != "0"   # A/B switch


_TUNE_LOG = _os.environ.get("MSPI_TUNE_LOG") == "1"


def _tune_conv(launch, key, candidates):
    best, best_t, times = -1, float("inf"), []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for tile in candidates:
        if launch(tile) != 0:
            continue
        e0.record()
        for _ in range(AUTOTUNE["reps"]):
            launch(tile)
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1)
        times.append((tile, t / AUTOTUNE["reps"]))
        if t < best_t:
            best, best_t = tile, t
    AUTOTUNE["cache"][key] = best
    if _TUNE_LOG:       # MSPI_TUNE_LOG=1: every candidate's time (ms per launch, alone on the chip) to stderr
        import sys
        print("[tune] %s -> %d  %s" % (key, best, " ".join("%d:%.4f" % tt for tt in times)), file=sys.stderr)
    return best


def _choose(key, tile, default, candidates, launch, *call):
    """The kernel choice of one call: the forced `tile`; else, while autotuning, what the cache holds for `key` or, on first
    sight, the fastest of candidates(*call) (timed now and cached); else what the cache holds; else `default`."""
    if tile is not None:
        return tile
    choice = AUTOTUNE["cache"].get(key)
    if choice is None and AUTOTUNE["on"] and not torch.cuda.is_current_stream_capturing():
        return _tune_conv(launch, key, candidates(*call))
    return default if choice is None else choice


# ----------------------------------------------------------------------------- per-launch timing
class Profiler:
    """Per-launch HIP-event timing of the C-ABI calls, on the stream the kernels are launched on
    (torch's current stream).  Used by bench.py for the roofline line; off by default."""
    active = None

    def __init__(self):
        self.records = []   # (kernel_name, flops, bytes, start_event, end_event, detail)

    def __enter__(self):
        Profiler.active = self
        return self

    def __exit__(self, *a):
        Profiler.active = None

    def summary(self):
        """{kernel: dict(calls, ms, flops, bytes)} -- call after torch.cuda.synchronize()."""
        out = {}
        for name, fl, by, e0, e1, _ in self.records:
            d = out.setdefault(name, {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["calls"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += by
        return out


class _Timed:
    __slots__ = ("name", "flops", "bytes", "e0", "detail")

    def __init__(self, name, flops=0.0, nbytes=0.0, detail=""):
        self.name, self.flops, self.bytes, self.detail = name, flops, nbytes, detail

    def __enter__(self):
        if Profiler.active is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        p = Profiler.active
        if p is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            p.records.append((self.name, self.flops, self.bytes, self.e0, e1, self.detail))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(t):
    if not t.is_cuda:
        raise MspiError("mspi_amd runs on the GPU only (tensor on %s); there is no CPU fallback" % t.device)
    cur = torch.cuda.current_device()
    if t.device.index != cur:      # _stream() hands every launch the current stream of the CURRENT device
        raise MspiError("tensor on %s, but the current device is cuda:%d: the launch would go to the wrong device's stream; "
                        "call under torch.cuda.device(%d)" % (t.device, cur, t.device.index))
    if _STATUS["word"] is None:
        _register_status_word()


# ----------------------------------------------------------------------------- f16x3 operand range
# f16x3 splits an fp32 operand into f16 hi + lo halves.  Weights are pre-scaled by a power of two at pack time; activations
# are split as they are, which is exact to 2^-22 relative while 2^-5 <~ |x| < 65504 for the LARGEST entries of the tensor:
# beyond 65504 the hi half is inf; far below, the lo half sinks into f16 subnormals (absolute error 2^-25 per element,
# whatever its size).  Two safeguards:
#  * RANGE GUARD (always on): the GEMM and attention kernels store 1 into a pinned host word when a result is inf / NaN
#    (mspi_set_status_word); range_flag() / check_range() read it -- no device call, the caller synchronises first.
#  * RANGE CHECK on first sight of a pack (the first, autotuning forward -- the same "first input is representative"
#    contract as cudnn.benchmark upstream, inference.py:19): max|x| of the layer's input outside [2^-5, 2^15] moves THAT layer
#    to the fp32 MFMA path (exact fp32 fmaf chain, 5.3x the MFMA time) for good.  MSPI_RANGE_CHECK=0 disables it.
# NON-FINITE DATA (include/mspi_hip.h at mspi_set_status_word; tests/test_nonfinite_ledger.py): a NaN or
# Inf in an operand never leaves a kernel as plausible finite data without a trace.  The GEMM family (pre-activation
# results), attention (stored outputs) and postprocess_u8 (whose u8 output cannot carry a NaN) FLAG it in the status word;
# every other kernel with floating-point output PROPAGATES it as torch does (its ReLU and max keep a NaN), so the next GEMM
# flags it or the map itself is NaN.  Outputs that do not depend on the poison are unaffected either way.
_STATUS = {"word": None}
RANGE_CHECK = {"on": _os.environ.get("MSPI_RANGE_CHECK", "1") != "0", "lo": 2.0 ** -5, "hi": 2.0 ** 15, "moved": []}


def _register_status_word():
    w = torch.zeros(1, dtype=torch.int32).pin_memory()
    check(_lib.load().mspi_set_status_word(w.data_ptr()), "mspi_set_status_word")
    _STATUS["word"] = w


def range_flag(reset=True):
    """True when a flagging kernel (GEMM family, attention, postprocess_u8) has produced a non-finite result since the last
    reset; the other kernels hand a NaN / Inf on in their output instead.  Host read of a pinned word: valid for launches the
    caller has synchronised with (an event / stream / device sync)."""
    w = _STATUS["word"]
    if w is None:
        return False
    bad = bool(int(w[0]))
    if bad and reset:
        w[0] = 0
    return bad


def check_range(sync=True):
    """Raise MspiError when an f16x3 GEMM or attention has overflowed, or a GEMM, attention or postprocess_u8 was fed
    non-finite data, since the last check.  Kernels in front of them propagate a NaN / Inf rather than flag it, so a poisoned
    forward raises here at its next GEMM, or returns a map that is itself non-finite."""
    if sync and torch.cuda.is_available():
        torch.cuda.synchronize()
    if range_flag():
        raise MspiError("a GEMM or attention produced inf/NaN: an activation left the f16x3 range (|x| >= 65504; attention: "
                        "|q| >= 1023, |k|, |v| >= 4094) or the input was not finite; "
                        "let the first forward see representative data (engine.autotune(True): out-of-range layers move to the "
                        "fp32 path) or run with MSPI_GEMM_PREC=f32")


def _range_check(pk, amax_fn, what):
    """First sight of a pack while tuning: move it to the fp32 path if its input's magnitude is outside the f16x3 window."""
    if pk.checked:
        return
    pk.checked = True
    amax = float(amax_fn())
    if not (amax == amax) or amax >= RANGE_CHECK["hi"] or 0.0 < amax < RANGE_CHECK["lo"]:
        pk.w, pk.ldw, pk.prec, pk.thin, pk.w_scale = pk.w32, pk.ldw32, PREC_F32, None, 1.0
        RANGE_CHECK["moved"].append((what, amax))


class CL:
    """Channels-last activation view: rows (n,t,h,w) x C stored channels, row stride ld."""
    __slots__ = ("buf", "off", "N", "T", "H", "W", "C", "ld", "sN")

    def __init__(self, buf, off, N, T, H, W, Cc, ld, sN=None):
        self.buf, self.off, self.N, self.T, self.H, self.W, self.C, self.ld = buf, off, N, T, H, W, Cc, ld
        self.sN = T * H * W * ld if sN is None else sN  # sample stride (floats); dense unless a token slab

    @property
    def dense(self):
        return self.sN == self.T * self.H * self.W * self.ld

    @property
    def Cs(self):
        """stored channels"""
        return rup4(self.C) if self.C > 1 else 1

    @property
    def M(self):
        return self.N * self.T * self.H * self.W

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def slice(self, c0, c):
        assert c0 % 4 == 0 and c0 + c <= self.ld
        return CL(self.buf, self.off + c0, self.N, self.T, self.H, self.W, c, self.ld, self.sN)

    def reshape(self, N, T, H, W):
        assert N * T * H * W == self.M and self.dense
        return CL(self.buf, self.off, N, T, H, W, self.C, self.ld)

    def tokens(self, r0, T, H, W):
        """Rows [r0, r0+T*H*W) of every sample as a [N,T,H,W,C] view (sample stride kept)."""
        assert r0 + T * H * W <= self.T * self.H * self.W
        return CL(self.buf, self.off + r0 * self.ld, self.N, T, H, W, self.C, self.ld, self.sN)

    def as_ncdhw(self, channels=None):
        """Logical [N,C,T,H,W] view (no copy) -- what the reference's modules return."""
        c = self.C if channels is None else channels
        ld, T, H, W = self.ld, self.T, self.H, self.W
        return self.buf.as_strided((self.N, c, T, H, W), (self.sN, 1, H * W * ld, W * ld, ld),
                                   self.buf.storage_offset() + self.off)

    def as_nthwc(self):
        """Logical [N,T,H,W,C] view (no copy) -- what the autograd Functions take and return."""
        ld, H, W = self.ld, self.H, self.W
        return self.buf.as_strided((self.N, self.T, H, W, self.C), (self.sN, H * W * ld, W * ld, ld, 1),
                                   self.buf.storage_offset() + self.off)

    def as_rows(self, channels=None):
        c = self.C if channels is None else channels
        assert self.dense
        return self.buf.as_strided((self.M, c), (self.ld, 1), self.buf.storage_offset() + self.off)


def alloc(N, T, H, W, Cc, device, ld=None):
    if ld is None:
        ld = rup4(Cc) if Cc > 1 else 1
    buf = torch.empty(N * T * H * W * ld, dtype=torch.float32, device=device)
    return CL(buf, 0, N, T, H, W, Cc, ld)


class SP:
    """Pre-split activation rows: two f16 planes (hi, lo) in one buffer -- what a producer's epilogue hands to the f16x3 GEMM so
    that neither operand needs conversion work in the loop (include/mspi_hip.h, mspi_gemm_sp_fwd).  Each plane is BLOCKED:
    16 rows x 32 columns = 1 KB contiguous per block, blocks column-fastest, rows allocated to a multiple of 16 (ld == C).
    Same logical shape as a dense CL; only GEMM-shaped consumers (conv on 1x1x1 / Linear packs) accept it."""
    __slots__ = ("buf", "N", "T", "H", "W", "C", "ld")

    def __init__(self, buf, N, T, H, W, Cc, ld):
        self.buf, self.N, self.T, self.H, self.W, self.C, self.ld = buf, N, T, H, W, Cc, ld

    @property
    def M(self):
        return self.N * self.T * self.H * self.W

    @property
    def plane(self):
        return (self.M + 15) // 16 * 16 * self.ld      # blocked planes: rows allocated to a multiple of 16

    @property
    def ptr(self):
        return self.buf.data_ptr()


def alloc_sp(N, T, H, W, Cc, device):
    assert Cc % 32 == 0
    m = N * T * H * W
    mp = (m + 15) // 16 * 16
    buf = torch.empty(2 * mp * Cc, dtype=torch.float16, device=device)
    if mp != m:      # the rows that pad the last 16-row group are read by the GEMM (their outputs are never stored) and by the range check
        buf.view(2, mp * Cc)[:, (mp - 16) * Cc:].zero_()
    return SP(buf, N, T, H, W, Cc, Cc)


def join_planes(sp):
    """SP -> dense CL of fp32 rows (hi + lo)."""
    out = alloc(sp.N, sp.T, sp.H, sp.W, sp.C, sp.buf.device)
    check(_lib.load().mspi_join_planes_fwd(sp.ptr, sp.ld, sp.plane, sp.M, sp.C, out.ptr, out.ld, _stream()), "mspi_join_planes_fwd")
    return out


def from_rows(t2d):
    """Wrap a contiguous [M, C] tensor (C % 4 == 0) as a CL with N=M, T=H=W=1."""
    assert t2d.dim() == 2 and t2d.stride(1) == 1 and t2d.stride(0) % 4 == 0
    return CL(t2d, 0, t2d.shape[0], 1, 1, 1, t2d.shape[1], t2d.stride(0))


def _tuning():
    return AUTOTUNE["on"] and RANGE_CHECK["on"] and DEFAULT_PREC == PREC_F16X3 and not torch.cuda.is_current_stream_capturing()


def range_check_input(pk, x):
    """First-sight range check of PackedConv `pk` on its input `x` (CL), for callers that bypass conv() with a fused kernel
    built from the pack's f16x3 planes (X3D a + b).  Returns True while the pack is on the f16x3 path."""
    if _tuning() and pk.prec == PREC_F16X3:
        _range_check(pk, lambda: (x.as_rows()[:, : x.C] if x.dense else x.buf).abs().max(), "conv %s %d -> %d" % (pk.k, pk.cin, pk.cout))
    return pk.prec == PREC_F16X3


def _x3d_ab_desc(x, pk, out_ld, act, cls=_lib.X3dAbDesc):
    d = cls()
    d.N, d.T, d.H, d.W = x.N, x.T, x.H, x.W
    d.Cin, d.Cmid, d.ldx, d.ldu, d.act, d.wa_scale = pk.cin_s, pk.cmid_s, x.ld, out_ld, act, pk.wa_scale
    return d


_x3d_ab_s2_desc = partial(_x3d_ab_desc, cls=_lib.X3dAbS2Desc)


def x3d_ab_supported(x, pk):
    return pk is not None and x.dense and x.Cs == pk.cin_s and bool(_lib.load().mspi_x3d_ab_supported(C.byref(_x3d_ab_desc(x, pk, pk.cmid_s, ACT_NONE))))


def x3d_ab_s2_supported(x, pk):
    return pk is not None and x.dense and x.Cs == pk.cin_s and bool(_lib.load().mspi_x3d_ab_s2_supported(C.byref(_x3d_ab_s2_desc(x, pk, pk.cmid_s, ACT_NONE))))


# what differs between the two strides of `b`: (stride, descriptor class, Profiler names, entry point's name)
_AB = (1, _lib.X3dAbDesc, "x3d_ab", "x3d_ab_pool", "mspi_x3d_ab_fwd")
_AB_S2 = (2, _lib.X3dAbS2Desc, "x3d_ab_s2", "x3d_ab_s2_pool", "mspi_x3d_ab_s2_fwd")


def _x3d_ab(rec, fwd, pool_rows, x, pk, pool, out):
    """The fused a + b pair of record `rec`, launched by the library's `fwd` / `pool_rows` of that stride."""
    s, desc, name, pooled, entry = rec
    _need_gpu(x.buf)
    if out is None:
        out = alloc(x.N, x.T, x.H // s, x.W // s, pk.cmid, x.buf.device)
    elif (out.N, out.T, out.H, out.W, out.Cs) != (x.N, x.T, x.H // s, x.W // s, pk.cmid_s) or not out.dense:
        raise MspiError("%s: the output tensor does not match the layer" % name)
    d = _x3d_ab_desc(x, pk, out.ld, ACT_NONE if pool else ACT_SWISH, desc)
    part = torch.empty(x.N, pool_rows(C.byref(d)), pk.cmid_s, dtype=torch.float32, device=x.buf.device) if pool else None
    # integer-valued doubles, exact: with out.M == x.M (stride 1) these are 2 M (Cin + 27) Cmid and 4 M (C + Cmid) to the bit
    with _Timed(pooled if pool else name, 2.0 * x.M * pk.cin_s * pk.cmid + 2.0 * out.M * 27 * pk.cmid,
                4.0 * (x.M * x.C + out.M * pk.cmid), "in=%s Cin=%d Cmid=%d" % ((x.N, x.T, x.H, x.W), x.C, pk.cmid)):
        check(fwd(C.byref(d), x.ptr, pk.wa.data_ptr(), pk.ba.data_ptr(), pk.wb.data_ptr(), pk.bb.data_ptr(), out.ptr,
                  part.data_ptr() if pool else None, _stream()), entry)
    return (out, part) if pool else out


def x3d_ab(x, pk, pool=False):
    """u = act(b_bn(dw3x3x3(relu(a_bn(a(x)))))) in one launch (csrc/x3d_block.hip); pool=True: no activation, also returns
    the [N, rows, C] partial sums of u for the squeeze-excite gate (X3DTransform with SE); otherwise act = Swish."""
    lib = _lib.load()
    return _x3d_ab(_AB, lib.mspi_x3d_ab_fwd, lib.mspi_x3d_ab_pool_rows, x, pk, pool, None)


def x3d_ab_s2(x, pk, pool=False, out=None):
    """u = act(b_bn(dw3x3x3 stride (1,2,2)(relu(a_bn(a(x)))))) in one launch (csrc/x3d_head.hip); pool=True: no activation,
    also returns the [N, rows, C] partial sums of u for the squeeze-excite gate; otherwise act = Swish."""
    lib = _lib.load()
    if not x3d_ab_s2_supported(x, pk):
        raise MspiError("x3d_ab_s2: input %s with %d channels is outside the fused kernel's range" % ((x.N, x.T, x.H, x.W), x.C))
    return _x3d_ab(_AB_S2, lib.mspi_x3d_ab_s2_fwd, lib.mspi_x3d_ab_s2_pool_rows, x, pk, pool, out)


def _x3d_stem_desc(x, ldy):
    d = _lib.X3dStemDesc()
    d.N, _, d.T, d.H, d.W = x.shape
    d.sN, d.sC, d.sT, d.sH, d.sW = x.stride()
    d.ldy = ldy
    return d


def x3d_stem_supported(x, pk):
    return pk is not None and isinstance(x, torch.Tensor) and x.dim() == 5 and x.shape[1] == 3 and x.dtype == torch.float32 \
        and x.data_ptr() % 4 == 0 and bool(_lib.load().mspi_x3d_stem_supported(C.byref(_x3d_stem_desc(x, 24))))


def x3d_stem(x, pk, out=None):
    """relu(bn(temporal dw (5,1,1)(conv_xy (1,3,3)/(1,2,2)(x)))) of the raw clip x [N,3,T,H,W] (any strides) in one launch
    (csrc/x3d_head.hip): the 24-channel conv_xy result stays in registers."""
    lib = _lib.load()
    _need_gpu(x)
    if not x3d_stem_supported(x, pk):
        raise MspiError("x3d_stem: input %s is outside the fused stem's range" % (tuple(x.shape),))
    N, _, T, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = alloc(N, T, Ho, Wo, 24, x.device)
    elif (out.N, out.T, out.H, out.W, out.Cs) != (N, T, Ho, Wo, 24) or not out.dense:
        raise MspiError("x3d_stem: the output tensor does not match the layer")
    d = _x3d_stem_desc(x, out.ld)
    with _Timed("x3d_stem", 2.0 * out.M * 24 * (27 + 5), 4.0 * (N * 3 * T * H * W + out.M * 24), "in=%s" % (tuple(x.shape),)):
        check(lib.mspi_x3d_stem_fwd(C.byref(d), x.data_ptr(), pk.wxy.data_ptr(), pk.wt.data_ptr(), pk.bias.data_ptr(), out.ptr,
                                    _stream()), "mspi_x3d_stem_fwd")
    return out


def x3d_ca(u, pk, res, gate=None):
    """(y, t) = (relu(c(u') + res), relu(a_next(y))) in one launch (csrc/mlp_fused.hip); u' = swish(u * gate) with a gate."""
    lib = _lib.load()
    _need_gpu(u.buf)
    if not (u.dense and res.dense) or u.Cs != pk.d_s or res.Cs != pk.cx_s or res.M != u.M:
        raise MspiError("x3d_ca: u %s / res %s do not match the pack (%d, %d)" % ((u.M, u.Cs), (res.M, res.Cs), pk.d_s, pk.cx_s))
    if pk.w.device != u.buf.device:
        raise MspiError("x3d_ca: packed weights live on %s, the input on %s" % (pk.w.device, u.buf.device))
    y = alloc(u.N, u.T, u.H, u.W, pk.cx, u.buf.device)
    t = alloc(u.N, u.T, u.H, u.W, pk.d, u.buf.device)
    d = _lib.X3dCaDesc()
    d.M, d.D, d.Cx = u.M, pk.d_s, pk.cx_s
    d.ldu, d.ldr, d.ldy, d.ldt, d.ldg = u.ld, res.ld, y.ld, t.ld, pk.d_s
    d.rows_per_sample, d.wc_scale, d.wa_scale = u.T * u.H * u.W, pk.wc_scale, pk.wa_scale
    with _Timed("x3d_ca", 4.0 * u.M * pk.d * pk.cx, 4.0 * u.M * (2 * pk.d + 2 * pk.cx),
                "M=%d D=%d Cx=%d%s" % (u.M, pk.d, pk.cx, " +gate" if gate is not None else "")):
        check(lib.mspi_x3d_ca_fwd(C.byref(d), u.ptr, gate.data_ptr() if gate is not None else None, pk.w.data_ptr(),
                                  pk.bc.data_ptr(), pk.ba.data_ptr(), res.ptr, y.ptr, t.ptr, _stream()), "mspi_x3d_ca_fwd")
    return y, t


# ----------------------------------------------------------------------------- op wrappers
def _out_extent(T, H, W, k, s, p):
    return ((T + 2 * p[0] - k[0]) // s[0] + 1, (H + 2 * p[1] - k[1]) // s[1] + 1, (W + 2 * p[2] - k[2]) // s[2] + 1)


# The tile codes of MspiConvDesc.tile, as kTiles in csrc/conv_common.h declares them: code -> (kind, BM, BN), kind the leading
# digit of the variant code.  BN 0 = every output channel in one column tile.
REG4, REG8, DMA128, DMA256 = 1, 2, 4, 5
TILES = {0: (REG4, 128, 128), 1: (REG4, 128, 64), 2: (REG4, 128, 32), 3: (REG4, 64, 64), 4: (REG8, 128, 128), 5: (REG8, 256, 128),
         6: (DMA128, 128, 128), 7: (DMA128, 128, 64), 8: (DMA128, 128, 0), 9: (DMA128, 128, 96), 10: (DMA128, 128, 192),
         11: (DMA128, 128, 32), 12: (DMA256, 256, 256), 13: (DMA256, 256, 192), 14: (DMA256, 256, 128)}
UNTUNED = (0, 5, 11)      # conv() does not time these (0: code 4's 8 waves run the same tile better)
# mspi_gemm_sp_fwd takes the LDS-DMA codes with a fixed BN (11 as 128 x 256): 128 x {128,64,96,192,256}, 256 x {256,192,128}
SP_TILES = tuple(t for t, (kind, _, bn) in TILES.items() if kind >= DMA128 and bn)


def _tiles(*kinds, all_cols=False):
    return [t for t, (kind, _, bn) in TILES.items() if kind in kinds and t not in UNTUNED and (bn == 0) == all_cols]


def gemm_kernel_name(code):
    """Profiler name of the instantiation a variant code (mspi_conv_variant, mspi_gemm_sp_variant) stands for."""
    kind, bm, bn, form = code // 10 ** 7, code // 10 ** 4 % 1000, code // 10 % 1000, code % 10
    if kind in (REG4, REG8):
        how = ("s" if form & 2 else "v4") + ("w8" if kind == REG8 else "")
        return "conv_gemm<%d,%d,%s,%s>" % (bm, bn, how, "f16x3" if form & 1 else "f32")
    return "conv_gemm<%d,%d,%s,f16x3>" % (bm, bn, "dma" if kind in (DMA128, DMA256) else "dma-presplit")


W_BLOCKED = _os.environ.get("MSPI_W_BLOCKED", "1") != "0"      # A/B switch: blocked weights for the LDS-DMA kernels on fp32 activations


def _sp_tiles(M):
    return [t for t in SP_TILES if TILES[t][0] != DMA256 or M >= 4096]


def _conv_sp(x, pk, out, res, act, tile, sp_out):
    """Dense GEMM on pre-split activation planes; result as fp32 rows (CL) or, sp_out, as planes for the next GEMM."""
    lib = _lib.load()
    _need_gpu(x.buf)
    if pk.k != (1, 1, 1) or pk.stride != (1, 1, 1) or pk.pad != (0, 0, 0) or pk.prec != PREC_F16X3:
        raise MspiError("conv: split-plane activations feed 1x1x1 / Linear f16x3 layers only")
    if x.C != pk.cin_s or pk.ldw != x.C:
        raise MspiError("conv: split-plane input has %d channels, weights were packed for %d (ldw %d)" % (x.C, pk.cin_s, pk.ldw))
    dev = x.buf.device
    if pk.w.device != dev:
        raise MspiError("conv: packed weights live on %s, the input on %s" % (pk.w.device, dev))
    M = x.M
    if sp_out:
        if res is not None or pk.cout_s % 32:
            raise MspiError("conv: split-plane output takes no residual and needs Cout %% 32 == 0")
        out = alloc_sp(x.N, x.T, x.H, x.W, pk.cout_s, dev)
    else:
        if out is None:
            out = alloc(x.N, x.T, x.H, x.W, pk.cout, dev)
        if out.M != M or out.Cs != pk.cout_s or not out.dense:
            raise MspiError("conv: output CL does not match %d rows x %d channels" % (M, pk.cout))
    if res is not None and (res.M != M or not res.dense):
        raise MspiError("conv: residual rows %d != output rows %d (or residual not dense)" % (res.M, M))
    d = ConvDesc()
    d.N, d.T, d.H, d.W, d.C = x.N, x.T, x.H, x.W, x.C
    d.kT = d.kH = d.kW = d.strT = d.strH = d.strW = 1
    d.To, d.Ho, d.Wo, d.Cout = x.T, x.H, x.W, pk.cout_s
    d.ldy = 0 if sp_out else out.ld
    d.ldw, d.ldr = pk.ldw, (res.ld if res is not None else 0)
    d.act = pk.act if act is None else act
    d.prec, d.w_scale = pk.prec, pk.w_scale
    args = (x.ptr, x.ld, x.plane, sp_weights(pk).data_ptr(), pk.bias.data_ptr() if pk.bias is not None else None,
            res.ptr if res is not None else None, None if sp_out else out.ptr, out.ptr if sp_out else None,
            out.ld if sp_out else 0, out.plane if sp_out else 0, _stream())

    def launch(t):
        d.tile = t
        return lib.mspi_gemm_sp_fwd(C.byref(d), *args)

    choice = _choose(("sp", M, x.C, pk.cout_s, res is not None, bool(sp_out)), tile, -1, _sp_tiles, launch, M)
    with _Timed("conv_gemm", 2.0 * M * pk.cin * pk.cout, 4.0 * (M * pk.cin + M * pk.cout * (2 if res is not None else 1) + pk.cout * pk.cin),
                "M=%d K=%d(1x%d) N=%d pre-split%s%s" % (M, pk.cin, pk.cin, pk.cout, " +res" if res is not None else "", " ->planes" if sp_out else "")) as tm:
        check(launch(choice), "mspi_gemm_sp_fwd")
        if Profiler.active is not None:
            tm.name = gemm_kernel_name(lib.mspi_gemm_sp_variant(C.byref(d), args[7]))
    return out


def _conv_kernels(pk, d, M, rg, halo, gate):
    cands = _tiles(REG4, REG8)
    if pk.prec == PREC_F16X3 and d.sC == 1 and d.C % 4 == 0:
        cands += _tiles(DMA128) + (_tiles(DMA128, all_cols=True) if pk.cout_s <= 256 else [])
        if M >= 16384:
            cands += _tiles(DMA256)        # 256-row / 8-wave form of the LDS-DMA kernel
    if rg is not None:
        cands.append(THIN)
    if halo:
        cands.append(HALO)
    nk = pk.ldw // 32
    if SPLITK_ENABLED and gate is None and -(-M // 64) * -(-pk.cout_s // 64) <= 384 and nk >= 32:
        # few output tiles, long contraction: K slices across workgroups (mspi_conv_splitk_fwd)
        cands += [SPLITK + S for S in (2, 4, 8) if nk >= 8 * S]
    return cands


def conv(x, pk, out=None, res=None, gate=None, act=None, tile=None, sp_out=False):
    """x: CL, or a raw 5-D [N,C,T,H,W] / 4-D [N,C,H,W] torch tensor with arbitrary strides.
    tile: force a kernel instantiation (MspiConvDesc.tile); None = autotune cache / library heuristic."""
    lib = _lib.load()
    tuning = AUTOTUNE["on"] and RANGE_CHECK["on"] and pk.prec == PREC_F16X3 and not torch.cuda.is_current_stream_capturing()
    if isinstance(x, SP):
        if tuning:   # planes: the hi plane carries the magnitude (an out-of-range layer is fixed from the NEXT forward on: its
            #          producer stops emitting planes once this pack is fp32)
            _range_check(pk, lambda: x.buf[: x.plane].abs().max(), "planes -> %dx%d" % (pk.cin, pk.cout))      # the hi plane (pad rows are zero)
        if pk.prec == PREC_F16X3:
            return _conv_sp(x, pk, out, res, act, tile, sp_out)
        # The range check has moved this layer to the fp32 path while its producer had already emitted planes (from the next
        # forward on the producer hands over fp32 rows: mlp_tail / layernorm_for_gemm look at the pack's precision): rebuild
        # the rows (hi + lo = 22 bits of the value) and take the fp32 path for this one call.
        x, sp_out = join_planes(x), False
    if tuning:
        _range_check(pk, (lambda: (x.as_rows()[:, : x.C] if x.dense else x.buf).abs().max()) if isinstance(x, CL) else (lambda: x.abs().max()),
                     "conv %s %d -> %d" % (pk.k, pk.cin, pk.cout))
    if sp_out:
        raise MspiError("conv: split-plane output needs a split-plane input (mspi_gemm_sp_fwd)")
    d = ConvDesc()
    if isinstance(x, CL):
        _need_gpu(x.buf)
        N, T, H, W, Cin = x.N, x.T, x.H, x.W, x.Cs
        d.sN, d.sT, d.sH, d.sW, d.sC = x.sN, H * W * x.ld, W * x.ld, x.ld, 1
        xptr, dev = x.ptr, x.buf.device
    else:
        _need_gpu(x)
        if x.dim() == 4:
            x = x[:, :, None]
        if x.dtype != torch.float32:
            raise MspiError("conv: input must be fp32")
        N, Cin, T, H, W = x.shape
        sN, sC, sT, sH, sW = x.stride()
        d.sN, d.sT, d.sH, d.sW, d.sC = sN, sT, sH, sW, sC
        xptr, dev = x.data_ptr(), x.device
    if Cin != pk.cin_s:
        raise MspiError("conv: input has %d stored channels, weights were packed for %d" % (Cin, pk.cin_s))
    if pk.w.device != dev:   # a host pointer handed to a kernel is a GPU memory fault, not an exception
        raise MspiError("conv: packed weights live on %s, the input on %s" % (pk.w.device, dev))
    To, Ho, Wo = _out_extent(T, H, W, pk.k, pk.stride, pk.pad)
    if out is None:
        out = alloc(N, To, Ho, Wo, pk.cout, dev)
    if (out.N, out.T, out.H, out.W) != (N, To, Ho, Wo) or out.Cs != pk.cout_s or not out.dense:
        raise MspiError("conv: output CL %s does not match %s" % ((out.N, out.T, out.H, out.W, out.C), (N, To, Ho, Wo, pk.cout)))
    d.N, d.T, d.H, d.W, d.C = N, T, H, W, Cin
    d.kT, d.kH, d.kW = pk.k
    d.strT, d.strH, d.strW = pk.stride
    d.padT, d.padH, d.padW = pk.pad
    d.To, d.Ho, d.Wo = To, Ho, Wo
    d.Cout = pk.cout_s
    d.ldy, d.ldw = out.ld, pk.ldw
    d.ldr = res.ld if res is not None else 0
    d.act = pk.act if act is None else act
    d.prec, d.w_scale = pk.prec, pk.w_scale
    d.w_blocked = sp_weights(pk).data_ptr() if (pk.prec == PREC_F16X3 and W_BLOCKED) else None      # the LDS-DMA kernels' weight source
    if res is not None and (res.M != out.M or not res.dense):
        raise MspiError("conv: residual rows %d != output rows %d (or residual not dense)" % (res.M, out.M))
    M = N * To * Ho * Wo
    taps = pk.k[0] * pk.k[1] * pk.k[2]
    tm = _Timed("conv_gemm", 2.0 * M * taps * pk.cin * pk.cout,
                4.0 * (N * T * H * W * pk.cin + M * pk.cout * (2 if res is not None else 1) + pk.cout * taps * pk.cin),
                "M=%d K=%d(%dx%d) N=%d s=%s%s%s" % (M, taps * pk.cin, taps, pk.cin, pk.cout, pk.stride,
                                                  " +res" if res is not None else "", " +gate" if gate is not None else ""))
    args = (xptr, pk.w.data_ptr(), pk.bias.data_ptr() if pk.bias is not None else None,
            res.ptr if res is not None else None, gate.data_ptr() if gate is not None else None, out.ptr, _stream())
    # the row-stationary thin GEMM (mspi_rowgemm_fwd) is a second implementation of dense 1x1x1 layers with K <= 224:
    # kernel choice THIN competes with the tile codes of mspi_conv_fwd in the autotuner
    rg = None
    if THIN_ENABLED and pk.thin is not None and isinstance(x, CL) and x.dense:
        rg = _lib.RowGemmDesc()
        rg.M, rg.K, rg.N = M, pk.cin_s, pk.cout_s
        rg.ldx, rg.ldy, rg.ldr, rg.ldg = x.ld, out.ld, d.ldr, pk.cin_s
        rg.act, rg.rows_per_sample, rg.w_scale = d.act, To * Ho * Wo, pk.w_scale
        rg_args = (xptr, pk.thin.data_ptr(), args[2], args[3], args[4], out.ptr, args[6])

    # the halo-staged kernel (mspi_conv_halo_fwd) is a second implementation of stride-1 (1|3,3,3) convs: kernel choice HALO
    halo = bool(HALO_ENABLED and gate is None and d.w_blocked and pk.k[1:] == (3, 3) and xptr % 16 == 0 and
                lib.mspi_conv_halo_supported(C.byref(d)))

    def launch(t):
        if t == THIN:
            return lib.mspi_rowgemm_fwd(C.byref(rg), *rg_args)
        if t == HALO:
            return lib.mspi_conv_halo_fwd(C.byref(d), args[0], args[2], args[3], None, out.ptr, args[6])
        if t >= SPLITK:      # split-K: t - SPLITK slices of the contraction, partial sums through a scratch buffer
            S = t - SPLITK
            ws = torch.empty(S * M * pk.cout_s, dtype=torch.float32, device=dev)   # stream-ordered: safe to drop after the launch
            d.tile = 3
            return lib.mspi_conv_splitk_fwd(C.byref(d), args[0], args[1], args[2], args[3], args[5], ws.data_ptr(), S, args[6])
        d.tile = t
        return lib.mspi_conv_fwd(C.byref(d), *args)

    key = (M, taps * pk.cin_s, pk.cout_s, pk.k, pk.stride, pk.prec, d.sC == 1, res is not None, gate is not None, rg is not None, halo)
    choice = _choose(key, tile, None, _conv_kernels, launch, pk, d, M, rg, halo, gate)
    if choice is None:      # nothing forced, tuned or cached
        choice = THIN if rg is not None and THIN_DEFAULT else -1
    if choice == THIN and rg is None:
        raise MspiError("conv: the thin-GEMM kernel does not cover this call")
    if choice == HALO and not halo:
        raise MspiError("conv: the halo-staged kernel does not cover this call")
    with tm:
        check(launch(choice), "mspi_rowgemm_fwd" if choice == THIN else "mspi_conv_halo_fwd" if choice == HALO else
              "mspi_conv_splitk_fwd" if choice >= SPLITK else "mspi_conv_fwd")
        if Profiler.active is not None:
            if choice == THIN:
                tm.name = "rowgemm<%d,f16x3>" % rowgemm_ksb(pk.cin_s)
            elif choice == HALO:
                v = lib.mspi_conv_halo_variant(C.byref(d), xptr)
                tm.name = "conv_halo<%d,%d,f16x3>" % (v // 1000, v % 1000)
            elif choice >= SPLITK:
                tm.name = "conv_gemm<64,64,splitk%d>" % (choice - SPLITK)
            else:
                tm.name = gemm_kernel_name(lib.mspi_conv_variant(C.byref(d), xptr, args[4], 1))
    return out


def _dw_desc(x, k, s, p, out_ld):
    d = DwConvDesc()
    assert x.dense
    d.N, d.T, d.H, d.W, d.C = x.N, x.T, x.H, x.W, x.Cs
    d.ldx, d.ldy = x.ld, out_ld
    d.kT, d.kH, d.kW = k
    d.strT, d.strH, d.strW = s
    d.padT, d.padH, d.padW = p
    d.To, d.Ho, d.Wo = _out_extent(x.T, x.H, x.W, k, s, p)
    return d


def dwconv_variant(x, pk):
    """The kernel instantiation dwconv(x, pk) launches in this process (mspi_dwconv_variant: host only, no GPU call)."""
    return _lib.load().mspi_dwconv_variant(C.byref(_dw_desc(x, pk.k, pk.stride, pk.pad, x.ld)))


def dwconv(x, pk, out=None, pool=False, act=None):
    """pool=True (X3D squeeze-excite): also returns the [N, rows, C] partial sums of the pre-activation output."""
    lib = _lib.load()
    _need_gpu(x.buf)
    if x.Cs != pk.c_s:
        raise MspiError("dwconv: input has %d channels, weights packed for %d" % (x.C, pk.c_s))
    if pk.w.device != x.buf.device:
        raise MspiError("dwconv: packed weights live on %s, the input on %s" % (pk.w.device, x.buf.device))
    To, Ho, Wo = _out_extent(x.T, x.H, x.W, pk.k, pk.stride, pk.pad)
    if out is None:
        out = alloc(x.N, To, Ho, Wo, x.C, x.buf.device)
    d = _dw_desc(x, pk.k, pk.stride, pk.pad, out.ld)
    d.act = pk.act if act is None else act
    part = None
    if pool:
        rows = lib.mspi_dwconv_pool_rows(C.byref(d))
        if rows <= 0:
            raise MspiError("dwconv: squeeze-excite pooling is not supported for kernel %s stride %s" % (pk.k, pk.stride))
        part = torch.empty(x.N, rows, pk.c_s, dtype=torch.float32, device=x.buf.device)
    taps = pk.k[0] * pk.k[1] * pk.k[2]
    with _Timed("dwconv_pool" if pool else "dwconv", 2.0 * out.M * taps * pk.c, 4.0 * (x.M + out.M) * pk.c,
                "in=%s C=%d k=%s s=%s" % ((x.N, x.T, x.H, x.W), pk.c, pk.k, pk.stride)):
        check(lib.mspi_dwconv_fwd(C.byref(d), x.ptr, pk.w.data_ptr(), pk.bias.data_ptr(), out.ptr,
                                  part.data_ptr() if pool else None, _stream()), "mspi_dwconv_fwd")
    return (out, part) if pool else out


def maxpool(x, k, s, p, out=None):
    lib = _lib.load()
    _need_gpu(x.buf)
    To, Ho, Wo = _out_extent(x.T, x.H, x.W, k, s, p)
    if out is None:
        out = alloc(x.N, To, Ho, Wo, x.C, x.buf.device)
    d = _dw_desc(x, k, s, p, out.ld)
    d.act = ACT_NONE
    with _Timed("maxpool", 0.0, 4.0 * (x.M + x.N * To * Ho * Wo) * x.C):
        check(lib.mspi_maxpool_fwd(C.byref(d), x.ptr, out.ptr, _stream()), "mspi_maxpool_fwd")
    return out


def se_gate(pool, inv_count, w1, b1, w2, b2, gate=None):
    """pool: [N, rows, C] partial sums from dwconv(pool=True) -> gate [N, C]."""
    lib = _lib.load()
    N, rows, Cc = pool.shape
    if gate is None:
        gate = torch.empty(N, Cc, dtype=torch.float32, device=pool.device)
    check(lib.mspi_se_gate(pool.data_ptr(), rows, float(inv_count), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                           b2.data_ptr(), gate.data_ptr(), N, Cc, w1.shape[0], _stream()), "mspi_se_gate")
    return gate


def layernorm(x, gamma, beta, eps, out=None, act=ACT_NONE, table=None, sp=False):
    """Rows of x -> rows of out; x and out may be token slabs (sample stride != dense).
    sp=True: the result as pre-split f16 planes (SP) for a following GEMM."""
    lib = _lib.load()
    _need_gpu(x.buf)
    if sp:
        assert out is None and table is None and x.C % 32 == 0
        o = alloc_sp(x.N, x.T, x.H, x.W, x.C, x.buf.device)
        with _Timed("layernorm", 8.0 * x.M * x.C, 8.0 * x.M * x.C, "M=%d C=%d ->planes" % (x.M, x.C)):
            check(lib.mspi_layernorm_sp_fwd(x.ptr, x.ld, x.sN, o.ptr, o.ld, o.plane, gamma.data_ptr(), beta.data_ptr(), float(eps),
                                            x.N, x.T * x.H * x.W, x.C, act, _stream()), "mspi_layernorm_sp_fwd")
        return o
    if out is None:
        out = alloc(x.N, x.T, x.H, x.W, x.C, x.buf.device)
    R = x.T * x.H * x.W
    assert out.N == x.N and out.T * out.H * out.W == R and out.C == x.C
    P = 0 if table is None else table.shape[0]
    assert table is None or P == R
    with _Timed("layernorm", 8.0 * x.M * x.C, 8.0 * x.M * x.C, "M=%d C=%d" % (x.M, x.C)):
        check(lib.mspi_layernorm_fwd(x.ptr, x.ld, x.sN, out.ptr, out.ld, out.sN, gamma.data_ptr(), beta.data_ptr(),
                                     float(eps), x.N, R, x.C, act, table.data_ptr() if table is not None else None,
                                     _stream()), "mspi_layernorm_fwd")
    return out


def attention(qkv, B, Ntok, heads, hd, scale, out=None, biasT=None, maskT=None, tok_idx=None, rows_per_sample=None, slot=None):
    """qkv: CL with rows (b, token) and 3*heads*hd columns laid out [3][heads][hd]
    (what `qkv.reshape(B,N,3,h,hd)` means, model/model_utils.py:100).  B sequences of Ntok tokens.
    biasT [heads][Ntok][Ntok] / maskT [nmask][Ntok][Ntok]: key-major additive terms (Swin).
    tok_idx int32 [nwin][Ntok]: the B = samples*nwin sequences are windows whose token t sits at row
    tok_idx[win][t] of its sample (shifted-window attention without gather/scatter passes).
    rows_per_sample: rows of qkv (and of the output) per sample when that is not nwin*Ntok -- Swin on a grid that is
    not a multiple of the window keeps ONE extra row per sample for all padding tokens (tok_idx points there).
    slot: the calling layer's dict of precision decisions (see _attn_prec); None = the shape-keyed process-wide table."""
    lib = _lib.load()
    _need_gpu(qkv.buf)
    Cc = heads * hd
    assert qkv.C == 3 * Cc and qkv.dense and (rows_per_sample is not None or qkv.M == B * Ntok)
    if out is None:
        out = alloc(qkv.N, qkv.T, qkv.H, qkv.W, Cc, qkv.buf.device)
    d = AttnDesc()
    d.B, d.Hh, d.Nq, d.Nk, d.D, d.Dv = B, heads, Ntok, Ntok, hd, hd
    d.nmask = 0 if maskT is None else maskT.shape[0]
    d.nwin = 0 if tok_idx is None else tok_idx.shape[0]
    if rows_per_sample is None:
        rows_per_sample = Ntok * max(d.nwin, 1)
    d.q_sB = d.k_sB = d.v_sB = rows_per_sample * qkv.ld
    d.q_sH = d.k_sH = d.v_sH = hd
    d.q_sT = d.k_sT = d.v_sT = qkv.ld
    d.o_sB, d.o_sH, d.o_sT = rows_per_sample * out.ld, hd, out.ld
    d.scale = float(scale)
    d.prec = _attn_prec(("qkv", heads, hd, Ntok, d.nwin), lambda: qkv.as_rows()[:, :Cc].abs().max() * abs(float(scale)),
                        lambda: qkv.as_rows()[:, Cc:].abs().max(), slot)
    base = qkv.ptr
    with _Timed("attention", 4.0 * B * heads * Ntok * Ntok * hd, 16.0 * B * Ntok * Cc, "B=%d h=%d N=%d d=%d" % (B, heads, Ntok, hd)):
        _attn_launch(lib, d, base, base + 4 * Cc, base + 8 * Cc, None,
                     biasT.data_ptr() if biasT is not None else None, maskT.data_ptr() if maskT is not None else None,
                     tok_idx.data_ptr() if tok_idx is not None else None, out.ptr, qkv.buf.device)
    return out


ATTN_PLANES = _os.environ.get("MSPI_ATTN_PLANES", "1") != "0"      # A/B switch: K / V split once per head (mspi_attn_fwd_ws)
# f16x3 attention scales q by 64 and k, v by 16 before the split (csrc/attn.hip): |q * scale| >= 1023 or |k|, |v| >= 4094 is inf
# in the hi half.  First sight of an attention LAYER (per shape) while tuning: operands beyond a quarter of that move that
# layer's shape to the fp32 MFMA kernel for good (same contract as the GEMM packs' range check).  The decision lives in the
# `slot` dict the module passes from its packed plan (pk["attn_prec"]), so every layer is checked on its own data and a
# weight reload, .to() or in-place write (the plan is rebuilt: module.HipModule.pk) checks again.  ATTN_PREC: the shape-keyed table of callers without a slot.
ATTN_PREC = {}
LAST_ATTN = [None]      # (descriptor, has_bias, has_mask, has_tok, has_ws) of the last attention launch: attn_variant()


def attn_slot(pk):
    """The per-layer precision slot kept in a module's packed plan `pk` (rebuilt with it)."""
    return pk.setdefault("attn_prec", {})


def _attn_prec(key, amax_q, amax_kv, slot=None):
    if DEFAULT_PREC != PREC_F16X3:
        return DEFAULT_PREC
    table = ATTN_PREC if slot is None else slot
    prec = table.get(key)
    if prec is None:
        if not _tuning():
            return PREC_F16X3
        aq, akv = float(amax_q()), float(amax_kv())
        bad = not (aq == aq and akv == akv) or aq >= 256.0 or akv >= 1024.0
        prec = table[key] = PREC_F32 if bad else PREC_F16X3
        if bad:
            RANGE_CHECK["moved"].append(("attention %s" % (key,), max(aq, akv)))
    return prec


def attn_variant():
    """The kernels of the last attention launch (mspi_attn_variant: host only, no GPU call); None before the first."""
    if LAST_ATTN[0] is None:
        return None
    return _lib.load().mspi_attn_variant(C.byref(LAST_ATTN[0][0]), *LAST_ATTN[0][1:])


def _attn_launch(lib, d, q, k, v, res, biasT, maskT, tok_idx, o, dev):
    nbytes = lib.mspi_attn_ws_bytes(C.byref(d)) if ATTN_PLANES else 0
    LAST_ATTN[0] = (d, biasT is not None, maskT is not None, tok_idx is not None, nbytes > 0)
    if nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)      # stream-ordered: safe to drop after the launch
        check(lib.mspi_attn_fwd_ws(C.byref(d), q, k, v, res, biasT, maskT, tok_idx, o, ws.data_ptr(), _stream()), "mspi_attn_fwd_ws")
    else:
        check(lib.mspi_attn_fwd(C.byref(d), q, k, v, res, biasT, maskT, tok_idx, o, _stream()), "mspi_attn_fwd")


def mlp(x, pk, res=None, ln=None, eps=1e-6, out=None, split=None):
    """out = res + fc2(act(fc1(LN(x)))) in one launch (mspi_mlp_fwd); ln = (gamma, beta) or None.
    split: the same pair as two PackedConv (fc1 with the activation, fc2), if the caller has them -- used by the first-sight
    range check (else built from the fused pack's sources)."""
    lib = _lib.load()
    _need_gpu(x.buf)
    if pk.fallback is None and not pk.checked and _tuning():
        # First sight of this fused pair while tuning: run it ONCE as LayerNorm + two GEMMs, whose packs go through conv()'s
        # range check on their real inputs (fc1: the normalised rows, fc2: the activations).  If either leaves the f16x3
        # window the pair stays unfused on the fp32 path for good; otherwise the fused kernel takes over from the next call.
        pk.checked = True
        if split is None:
            w1, b1, w2, b2, osc = pk.src
            split = (pack_conv(w1, b1, act=pk.act, device=pk.w.device), pack_conv(w2, b2, out_scale=osc, device=pk.w.device))
        y = conv(conv(layernorm(x, ln[0], ln[1], eps) if ln is not None else x, split[0]), split[1], res=res, out=out)
        if split[0].prec != PREC_F16X3 or split[1].prec != PREC_F16X3:
            pk.fallback = split
        return y
    if pk.fallback is not None:
        return conv(conv(layernorm(x, ln[0], ln[1], eps) if ln is not None else x, pk.fallback[0]), pk.fallback[1], res=res, out=out)
    if x.C != pk.c or not x.dense:
        raise MspiError("mlp: input has %d channels (dense=%s), packed for %d" % (x.C, x.dense, pk.c))
    if pk.w.device != x.buf.device:
        raise MspiError("mlp: packed weights live on %s, the input on %s" % (pk.w.device, x.buf.device))
    if out is None:
        out = alloc(x.N, x.T, x.H, x.W, pk.c, x.buf.device)
    if res is not None and (res.M != x.M or not res.dense):
        raise MspiError("mlp: residual rows %d != rows %d (or residual not dense)" % (res.M, x.M))
    d = _lib.MlpDesc()
    d.M, d.C, d.hidden = x.M, pk.c, pk.hidden
    d.ldx, d.ldy, d.ldr = x.ld, out.ld, (res.ld if res is not None else 0)
    d.ln, d.act, d.eps = (1 if ln is not None else 0), pk.act, eps
    d.w1_scale, d.w2_scale = pk.s1, pk.s2
    with _Timed("mlp_fused", 4.0 * x.M * pk.c * pk.hidden, 4.0 * x.M * pk.c * (3 if res is not None else 2),
                "M=%d C=%d hidden=%d" % (x.M, pk.c, pk.hidden)):
        check(lib.mspi_mlp_fwd(C.byref(d), x.ptr, ln[0].data_ptr() if ln is not None else None,
                               ln[1].data_ptr() if ln is not None else None, pk.w.data_ptr(), pk.b1.data_ptr(),
                               pk.b2.data_ptr(), res.ptr if res is not None else None, out.ptr, _stream()), "mspi_mlp_fwd")
    return out


def layernorm_for_gemm(x, gamma, beta, eps, *packs):
    """LayerNorm whose result is consumed ONLY by the dense GEMMs `packs`: handed over as pre-split planes when every
    consumer can take them (K a multiple of 32, K >= 256: below that the thin-GEMM kernels on fp32 rows are faster)."""
    if sp_supported(x.C) and x.C >= 256 and all(p.k == (1, 1, 1) and p.stride == (1, 1, 1) and p.ldw == x.C and p.prec == PREC_F16X3
                                                 for p in packs):
        return layernorm(x, gamma, beta, eps, sp=True)
    return layernorm(x, gamma, beta, eps)


def mlp_tail(x, packed, ln, eps, res):
    """res + fc2(GELU(fc1(LayerNorm(x)))) with packed = pack_mlp_tail(...), ln = (gamma, beta)."""
    if packed[0] == "fused":
        return mlp(x, packed[1], res=res, ln=ln, eps=eps)
    if sp_supported(x.C) and sp_supported(packed[1].cout_s) and packed[1].ldw == x.C and packed[2].ldw == packed[1].cout_s \
            and packed[1].prec == PREC_F16X3 and packed[2].prec == PREC_F16X3:
        # LN -> planes, fc1 + GELU -> planes, fc2 (+res) -> fp32 rows: no operand is converted inside a GEMM loop
        return conv(conv(layernorm(x, ln[0], ln[1], eps, sp=True), packed[1], sp_out=True), packed[2], res=res)
    return conv(conv(layernorm(x, ln[0], ln[1], eps), packed[1]), packed[2], res=res)


def space_to_depth(x, out=None):
    """Swin PatchMerging gather: [N,T,H,W,C] -> [N,T,H/2,W/2,4C], quadrant order (0,0),(1,0),(0,1),(1,1)."""
    lib = _lib.load()
    assert x.dense and x.C % 4 == 0
    if out is None:
        out = alloc(x.N, x.T, x.H // 2, x.W // 2, 4 * x.C, x.buf.device)
    with _Timed("space_to_depth", 0.0, 8.0 * x.M * x.C):
        check(lib.mspi_space_to_depth(x.ptr, x.ld, out.ptr, out.ld, x.N * x.T, x.H, x.W, x.C, _stream()), "mspi_space_to_depth")
    return out


def mvit_attention(q, k, v, B, heads, hd, scale, q_thw, k_thw, Rh, Rw, Rt, out=None, rel_gemm=None, slot=None):
    """MViTv2 pooled attention with decomposed relative positions and residual pooling (backbones/MViT.py:1261-1301).
    q: CL rows (b, tq,hq,wq) x heads*hd (pooled + normed); k, v likewise over the pooled key grid.
    Rh / Rw / Rt: gathered tables [q_size][k_size][hd].  rel_gemm = (packed_tables, idx_h, idx_w, idx_t): the q . R dot
    products as ONE thin GEMM of the q rows against all distinct table rows (pack_conv of their stack) followed by a gather
    (mspi_mvit_qk_augment_p) instead of the per-(row, j) dot-product kernel.
    slot: the calling layer's dict of precision decisions (see _attn_prec).
    Returns CL rows (b, q token) x heads*hd = softmax(...) v + q."""
    lib = _lib.load()
    _need_gpu(q.buf)
    Nq, Nk = q_thw[0] * q_thw[1] * q_thw[2], k_thw[0] * k_thw[1] * k_thw[2]
    J = k_thw[0] + k_thw[1] + k_thw[2]
    DA = 128 if hd + J <= 128 else (144 if hd + J <= 144 else 160)      # k16 steps of S: 8 / 9 / 10
    if hd != 96 or hd + J > DA:
        raise MspiError("mvit_attention: head_dim %d with %d relative-position columns is not instantiated" % (hd, J))
    dev = q.buf.device
    qa = torch.empty(B * heads * Nq * DA, dtype=torch.float32, device=dev)
    ka = torch.empty(B * heads * Nk * DA, dtype=torch.float32, device=dev)
    a = MvitAugDesc()
    a.B, a.heads, a.Dh, a.DA = B, heads, hd, DA
    a.qT, a.qH, a.qW = q_thw
    a.kT, a.kH, a.kW = k_thw
    a.ldq, a.ldk, a.scale = q.ld, k.ld, float(scale)
    if rel_gemm is not None and q.dense and q.ld == heads * hd:
        pkT, idx_h, idx_w, idx_t = rel_gemm
        rows = CL(q.buf, q.off, q.M * heads, 1, 1, 1, hd, hd)           # (b, token, head) rows of hd channels
        P = conv(rows, pkT)
        with _Timed("mvit_qk_augment", 0.0, 4.0 * B * heads * (Nq + Nk) * (hd + DA)):
            check(lib.mspi_mvit_qk_augment_p(C.byref(a), q.ptr, k.ptr, P.ptr, P.ld, idx_h.data_ptr(), idx_w.data_ptr(),
                                             idx_t.data_ptr(), qa.data_ptr(), ka.data_ptr(), _stream()), "mspi_mvit_qk_augment_p")
    else:
        with _Timed("mvit_qk_augment", 2.0 * B * heads * Nq * J * hd, 4.0 * B * heads * (Nq + Nk) * (hd + DA)):
            check(lib.mspi_mvit_qk_augment(C.byref(a), q.ptr, k.ptr, Rh.data_ptr(), Rw.data_ptr(), Rt.data_ptr(),
                                           qa.data_ptr(), ka.data_ptr(), _stream()), "mspi_mvit_qk_augment")
    if out is None:
        out = alloc(q.N, q.T, q.H, q.W, heads * hd, dev)
    d = AttnDesc()
    d.B, d.Hh, d.Nq, d.Nk, d.D, d.Dv, d.nmask = B, heads, Nq, Nk, DA, hd, 0
    d.q_sB, d.q_sH, d.q_sT = heads * Nq * DA, Nq * DA, DA
    d.k_sB, d.k_sH, d.k_sT = heads * Nk * DA, Nk * DA, DA
    d.v_sB, d.v_sH, d.v_sT = Nk * v.ld, hd, v.ld
    d.o_sB, d.o_sH, d.o_sT = Nq * out.ld, hd, out.ld
    d.scale = 1.0
    d.prec = _attn_prec(("mvit", heads, hd, Nq, Nk), lambda: qa.abs().max(), lambda: torch.maximum(ka.abs().max(), v.buf.abs().max()),
                        slot)
    assert q.ld == out.ld and q.dense and out.dense   # residual pooling reads q with o's strides
    with _Timed("attention", 2.0 * B * heads * Nq * Nk * (DA + hd), 4.0 * B * heads * (Nq * (DA + 2 * hd) + Nk * (DA + hd)),
                "B=%d h=%d Nq=%d Nk=%d d=%d+%d" % (B, heads, Nq, Nk, DA, hd)):
        _attn_launch(lib, d, qa.data_ptr(), ka.data_ptr(), v.ptr, q.ptr, None, None, None, out.ptr, dev)
    return out


def upsample(src, factor, dst=None, accumulate=False, act=ACT_NONE):
    lib = _lib.load()
    assert src.dense
    if dst is None:
        assert not accumulate
        dst = alloc(src.N, src.T, src.H * factor, src.W * factor, src.C, src.buf.device)
    assert (dst.N, dst.T, dst.H, dst.W) == (src.N, src.T, src.H * factor, src.W * factor) and dst.C == src.C
    assert dst.dense
    with _Timed("upsample", 0.0, 4.0 * (src.M + dst.M * (2 if accumulate else 1)) * src.C):
        check(lib.mspi_upsample_fwd(src.ptr, src.ld, dst.ptr, dst.ld, src.N * src.T, src.H, src.W, src.Cs, factor,
                                    1 if accumulate else 0, act, _stream()), "mspi_upsample_fwd")
    return dst


def upsample_sum(dst, srcs, accumulate=True, act=ACT_NONE):
    """dst (= or +=) sum of up-samples: srcs = [(CL, integer factor), ...], at most three, in one pass over dst.
    Bit-identical to the chain of upsample(src, k, dst=dst, accumulate=True) calls it replaces."""
    lib = _lib.load()
    J = len(srcs)
    for s, k in srcs:
        assert s.dense and s.C == dst.C and (dst.N, dst.T) == (s.N, s.T)
        assert k >= 1 and (dst.H, dst.W) == (s.H * k, s.W * k)
    assert dst.dense
    ptrs = (C.c_void_p * max(J, 1))(*[s.ptr for s, _ in srcs])
    lds = (C.c_int64 * max(J, 1))(*[s.ld for s, _ in srcs])
    ks = (C.c_int32 * max(J, 1))(*[k for _, k in srcs])
    with _Timed("upsample_sum", 0.0, 4.0 * (sum(s.M for s, _ in srcs) + dst.M * (2 if accumulate else 1)) * dst.C):
        check(lib.mspi_upsample_sum_fwd(ptrs, lds, ks, J, dst.ptr, dst.ld, dst.N * dst.T, dst.H, dst.W, dst.Cs,
                                        1 if accumulate else 0, act, _stream()), "mspi_upsample_sum_fwd")
    return dst


def rowgate(x, mask):
    lib = _lib.load()
    assert mask.M == x.M and mask.ld == 1
    assert x.dense and mask.dense
    with _Timed("rowgate", 0.0, 8.0 * x.M * x.C):
        check(lib.mspi_rowgate(x.ptr, x.ld, mask.ptr, x.M, x.Cs, _stream()), "mspi_rowgate")
    return x


def logsumexp_sub(t, N, L):
    lib = _lib.load()
    check(lib.mspi_logsumexp_sub(t.data_ptr(), N, L, _stream()), "mspi_logsumexp_sub")
    return t


# ----------------------------------------------------------------------------- readout tail backward (csrc/readout_bwd.hip)
WGRAD_SLICES = (256, 2048)      # rows per slice of mspi_conv_wgrad_fwd: the codes mspi_conv_wgrad_variant answers
WGRAD_BIG_M = 65536             # rows from which the long slice is taken
C1_BWD_ROWS = 1024              # rows per workgroup of mspi_conv_c1_bwd


def logsumexp_sub_bwd(logp, g, dz=None):
    """dz = g - exp(logp) * sum(g) per sample: backward of logsumexp_sub.  logp (the forward's output) and g are [N, ...]
    fp32 tensors of one shape."""
    lib = _lib.load()
    _need_gpu(logp)
    if logp.shape != g.shape or logp.dim() < 2 or logp.dtype != torch.float32 or g.dtype != torch.float32 or g.device != logp.device:
        raise MspiError("logsumexp_sub_bwd: logp %s / g %s must be fp32 tensors of one shape on one device" % (tuple(logp.shape), tuple(g.shape)))
    logp, g = logp.contiguous(), g.contiguous()
    N = logp.shape[0]
    if dz is None:
        dz = torch.empty_like(logp)
    with _Timed("logsumexp_sub_bwd", 0.0, 12.0 * logp.numel()):
        check(lib.mspi_logsumexp_sub_bwd(logp.data_ptr(), g.data_ptr(), dz.data_ptr(), N, logp.numel() // N, _stream()),
              "mspi_logsumexp_sub_bwd")
    return dz


def conv_c1_bwd(y, dz, weight):
    """Backward of the last conv (1,3,3) pad (0,1,1) C -> 1 and of the ReLU that produced its input.  y: CL [N,1,H,W,C], the
    saved post-ReLU activations; dz [N,H,W]; weight: the parameter [1,C,1,3,3].  Returns (d, dW, db): d a CL like y, the
    gradient in front of the ReLU; dW [1,C,1,3,3] and db [1] in the parameter's layout."""
    lib = _lib.load()
    _need_gpu(y.buf)
    Cc = y.Cs
    if y.T != 1 or not y.dense or tuple(dz.shape) != (y.N, y.H, y.W) or dz.dtype != torch.float32 or dz.device != y.buf.device:
        raise MspiError("conv_c1_bwd: y %s and dz %s do not match" % ((y.N, y.T, y.H, y.W, y.C), tuple(dz.shape)))
    if tuple(weight.shape) != (1, y.C, 1, 3, 3) or Cc != y.C or Cc > 64:
        raise MspiError("conv_c1_bwd: weight %s is not a (1,3,3) conv from %d channels (a multiple of 4, at most 64) to 1"
                        % (tuple(weight.shape), y.C))
    dev = y.buf.device
    dz = dz.contiguous()
    w = weight.detach().float().reshape(Cc, 9).t().contiguous().to(dev)          # [tap][c]
    d = alloc(y.N, 1, y.H, y.W, y.C, dev)
    dW = torch.empty(9, Cc, dtype=torch.float32, device=dev)
    db = torch.empty(1, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_conv_c1_bwd_ws_bytes(y.N, y.H, y.W) // 4, dtype=torch.float32, device=dev)   # stream-ordered
    with _Timed("conv_c1_bwd", 4.0 * y.M * 9 * Cc, 8.0 * y.M * Cc, "M=%d C=%d" % (y.M, Cc)):
        check(lib.mspi_conv_c1_bwd(y.ptr, y.ld, dz.data_ptr(), w.data_ptr(), d.ptr, d.ld, dW.data_ptr(), db.data_ptr(),
                                   ws.data_ptr(), y.N, y.H, y.W, Cc, _stream()), "mspi_conv_c1_bwd")
    return d, dW.t().reshape(1, Cc, 1, 3, 3), db


def _wgrad_desc(x, dy, pk):
    To, Ho, Wo = _out_extent(x.T, x.H, x.W, pk.k, pk.stride, pk.pad)
    d = ConvDesc()
    d.N, d.T, d.H, d.W, d.C = x.N, x.T, x.H, x.W, x.Cs
    d.sN, d.sT, d.sH, d.sW, d.sC = x.sN, x.H * x.W * x.ld, x.W * x.ld, x.ld, 1
    d.kT, d.kH, d.kW = pk.k
    d.strT, d.strH, d.strW = pk.stride
    d.padT, d.padH, d.padW = pk.pad
    d.To, d.Ho, d.Wo = To, Ho, Wo
    d.Cout, d.ldy = pk.cout_s, dy.ld
    return d


def conv_wgrad_variant(x, dy, pk):
    """The instantiation conv_wgrad(x, dy, pk) launches (rows per slice), -1 where it refuses; host only."""
    return _lib.load().mspi_conv_wgrad_variant(C.byref(_wgrad_desc(x, dy, pk)), x.ptr, dy.ptr)


def conv_wgrad(x, dy, pk):
    """Weight and bias gradient of conv(x, pk) for the output gradient dy (CL, one row per output position, in front of any
    activation).  Returns (dW, db) in the parameter's own layout, [Co,Ci,kt,kh,kw] and [Co]."""
    lib = _lib.load()
    _need_gpu(x.buf)
    if x.Cs != pk.cin_s or dy.Cs != pk.cout_s:
        raise MspiError("conv_wgrad: x has %d / dy %d stored channels, the layer %d -> %d" % (x.Cs, dy.Cs, pk.cin_s, pk.cout_s))
    d = _wgrad_desc(x, dy, pk)
    if not dy.dense or dy.M != x.N * d.To * d.Ho * d.Wo or dy.buf.device != x.buf.device:
        raise MspiError("conv_wgrad: dy has %d rows, the layer's output %d (or dy is not dense)" % (dy.M, x.N * d.To * d.Ho * d.Wo))
    if lib.mspi_conv_wgrad_variant(C.byref(d), x.ptr, dy.ptr) < 0:
        raise MspiError("conv_wgrad: %s" % lib.mspi_last_error().decode("utf-8", "replace"))
    dev = x.buf.device
    kt, kh, kw = pk.k
    dW = torch.empty(pk.cout_s, kt, kh, kw, pk.cin_s, dtype=torch.float32, device=dev)
    db = torch.empty(pk.cout_s, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_conv_wgrad_ws_bytes(C.byref(d)) // 4, dtype=torch.float32, device=dev)   # stream-ordered
    taps = kt * kh * kw
    with _Timed("conv_wgrad", 2.0 * dy.M * taps * pk.cin * pk.cout, 4.0 * (x.M * pk.cin + dy.M * pk.cout),
                "M=%d K=%d(%dx%d) N=%d" % (dy.M, taps * pk.cin, taps, pk.cin, pk.cout)):
        check(lib.mspi_conv_wgrad_fwd(C.byref(d), x.ptr, dy.ptr, dW.data_ptr(), db.data_ptr(), ws.data_ptr(), _stream()),
              "mspi_conv_wgrad_fwd")
    return dW[:pk.cout, :, :, :, :pk.cin].permute(0, 4, 1, 2, 3), db[:pk.cout]


def upsample_bwd(dy, factor, u=None, act=ACT_NONE, dx=None):
    """Adjoint of upsample(src, factor, act=act): dy is the gradient of the up-sampled CL; with act == ACT_RELU, u is the
    forward's output and supplies the ReLU mask.  Returns the gradient of src: a new CL, or dx (e.g. a channel slice)."""
    lib = _lib.load()
    _need_gpu(dy.buf)
    if factor not in (2, 4, 8) or dy.H % factor or dy.W % factor or not dy.dense:
        raise MspiError("upsample_bwd: factor %s must be 2, 4 or 8 and divide the dense gradient's %d x %d" % (factor, dy.H, dy.W))
    if act not in (ACT_NONE, ACT_RELU) or (act == ACT_RELU) != (u is not None):
        raise MspiError("upsample_bwd: act is ACT_NONE without u, or ACT_RELU with the forward's output u")
    if u is not None and ((u.N, u.T, u.H, u.W, u.Cs) != (dy.N, dy.T, dy.H, dy.W, dy.Cs) or not u.dense or u.buf.device != dy.buf.device):
        raise MspiError("upsample_bwd: u does not match the gradient")
    if dx is None:
        dx = alloc(dy.N, dy.T, dy.H // factor, dy.W // factor, dy.C, dy.buf.device)
    elif (dx.N, dx.T, dx.H, dx.W, dx.C) != (dy.N, dy.T, dy.H // factor, dy.W // factor, dy.C) or not dx.dense or dx.buf.device != dy.buf.device:
        raise MspiError("upsample_bwd: dx does not match the gradient divided by the factor")
    with _Timed("upsample_bwd", 0.0, 4.0 * (dx.M + dy.M * (2 if u is not None else 1)) * dy.C):
        check(lib.mspi_upsample_bwd(dy.ptr, dy.ld, u.ptr if u is not None else None, u.ld if u is not None else 0, dx.ptr, dx.ld,
                                    dy.N * dy.T, dx.H, dx.W, dy.Cs, factor, act, _stream()), "mspi_upsample_bwd")
    return dx


# ----------------------------------------------------------------------------- readout head training (csrc/readout_train.hip)
WGRAD_WIDE_BOX_ROWS = 128       # output rows per staged box of mspi_conv_wgrad_wide_fwd
WGRAD_WIDE_SLICES = (4, 32)     # boxes per slice: the codes mspi_conv_wgrad_wide_variant answers
WGRAD_WIDE_BIG_BOXES = 512      # boxes from which the long slice is taken
BN_ROWS = 512                   # rows per workgroup record of mspi_bn_stats / mspi_bn_bwd


def conv_wgrad_wide_variant(x, dy, pk):
    """The instantiation conv_wgrad_wide(x, dy, pk) launches (boxes per slice), -1 where it refuses; host only."""
    return _lib.load().mspi_conv_wgrad_wide_variant(C.byref(_wgrad_desc(x, dy, pk)), x.ptr, dy.ptr)


def conv_wgrad_wide(x, dy, pk):
    """conv_wgrad for the wide layers of the readout (stored channels multiples of 32 up to 192, stride 1, <= 27 taps): every
    operand staged through LDS once per workgroup.  Returns (dW, db) in the parameter's layout."""
    lib = _lib.load()
    _need_gpu(x.buf)
    if x.Cs != pk.cin_s or dy.Cs != pk.cout_s:
        raise MspiError("conv_wgrad_wide: x has %d / dy %d stored channels, the layer %d -> %d" % (x.Cs, dy.Cs, pk.cin_s, pk.cout_s))
    d = _wgrad_desc(x, dy, pk)
    if not dy.dense or dy.M != x.N * d.To * d.Ho * d.Wo or dy.buf.device != x.buf.device:
        raise MspiError("conv_wgrad_wide: dy has %d rows, the layer's output %d (or dy is not dense)"
                        % (dy.M, x.N * d.To * d.Ho * d.Wo))
    if lib.mspi_conv_wgrad_wide_variant(C.byref(d), x.ptr, dy.ptr) < 0:
        raise MspiError("conv_wgrad_wide: %s" % lib.mspi_last_error().decode("utf-8", "replace"))
    dev = x.buf.device
    kt, kh, kw = pk.k
    dW = torch.empty(pk.cout_s, kt, kh, kw, pk.cin_s, dtype=torch.float32, device=dev)
    db = torch.empty(pk.cout_s, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_conv_wgrad_wide_ws_bytes(C.byref(d)) // 4, dtype=torch.float32, device=dev)   # stream-ordered
    taps = kt * kh * kw
    with _Timed("conv_wgrad_wide", 2.0 * dy.M * taps * pk.cin * pk.cout, 4.0 * (x.M * pk.cin + dy.M * pk.cout),
                "M=%d K=%d(%dx%d) N=%d" % (dy.M, taps * pk.cin, taps, pk.cin, pk.cout)):
        check(lib.mspi_conv_wgrad_wide_fwd(C.byref(d), x.ptr, dy.ptr, dW.data_ptr(), db.data_ptr(), ws.data_ptr(), _stream()),
              "mspi_conv_wgrad_wide_fwd")
    return dW[:pk.cout, :, :, :, :pk.cin].permute(0, 4, 1, 2, 3), db[:pk.cout]


def _bn_rows(name, x):
    if not x.dense or x.Cs != x.C:
        raise MspiError("%s: rows must be dense with a channel count that is a multiple of 4" % name)
    return x.M, x.C


def _bn_vec(name, what, t, Cc, dev):
    if t.dtype != torch.float32 or t.numel() != Cc or t.device != dev or not t.is_contiguous():
        raise MspiError("%s: %s must be a contiguous fp32 [%d] tensor on %s" % (name, what, Cc, dev))
    return t.data_ptr()


def bn_stats(x, eps=1e-5):
    """Per-channel batch statistics of the CL x over its M rows: (mean, biased var, rstd = 1 / sqrt(var + eps)), fp32 [C]."""
    lib = _lib.load()
    _need_gpu(x.buf)
    M, Cc = _bn_rows("bn_stats", x)
    dev = x.buf.device
    out = torch.empty(3, Cc, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_bn_ws_bytes(M, Cc) // 4, dtype=torch.float32, device=dev)                     # stream-ordered
    with _Timed("bn_stats", 4.0 * M * Cc, 4.0 * M * Cc, "M=%d C=%d" % (M, Cc)):
        check(lib.mspi_bn_stats(x.ptr, x.ld, M, Cc, eps, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(),
                                _stream()), "mspi_bn_stats")
    return out[0], out[1], out[2]


def bn_apply(x, mean, rstd, gamma, beta, act=ACT_NONE, out=None):
    """y = gamma (x - mean) rstd + beta, then ReLU with act == ACT_RELU; a CL like x."""
    lib = _lib.load()
    _need_gpu(x.buf)
    M, Cc = _bn_rows("bn_apply", x)
    dev = x.buf.device
    if out is None:
        out = alloc(x.N, x.T, x.H, x.W, x.C, dev)
    ptrs = [_bn_vec("bn_apply", n, t, Cc, dev) for n, t in (("mean", mean), ("rstd", rstd), ("gamma", gamma), ("beta", beta))]
    with _Timed("bn_apply", 3.0 * M * Cc, 8.0 * M * Cc, "M=%d C=%d" % (M, Cc)):
        check(lib.mspi_bn_apply(x.ptr, x.ld, ptrs[0], ptrs[1], ptrs[2], ptrs[3], out.ptr, out.ld, M, Cc, act, _stream()),
              "mspi_bn_apply")
    return out


def bn_bwd(dy, x, mean, rstd, gamma, y=None, dx=None):
    """Backward of bn_apply(x, ...) on batch statistics for the output gradient dy; y: the forward's post-ReLU output when
    it ran with ACT_RELU (the mask), None otherwise.  Returns (dx, dgamma, dbeta): a CL like x (a new one, or dx: e.g. a channel
    slice of a wider buffer) and two fp32 [C]."""
    lib = _lib.load()
    _need_gpu(x.buf)
    M, Cc = _bn_rows("bn_bwd", x)
    dev = x.buf.device
    for t in (dy, y):
        if t is not None and ((t.M, t.C) != (M, Cc) or not t.dense or t.buf.device != dev):
            raise MspiError("bn_bwd: dy and y must match x (%d rows x %d channels, dense)" % (M, Cc))
    ptrs = [_bn_vec("bn_bwd", n, t, Cc, dev) for n, t in (("mean", mean), ("rstd", rstd), ("gamma", gamma))]
    if dx is None:
        dx = alloc(x.N, x.T, x.H, x.W, x.C, dev)
    elif (dx.M, dx.C) != (M, Cc) or not dx.dense or dx.buf.device != dev:
        raise MspiError("bn_bwd: dx must match x (%d rows x %d channels, dense)" % (M, Cc))
    dgb = torch.empty(2, Cc, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_bn_ws_bytes(M, Cc) // 4, dtype=torch.float32, device=dev)                     # stream-ordered
    with _Timed("bn_bwd", 8.0 * M * Cc, 4.0 * M * Cc * (6 if y is not None else 4), "M=%d C=%d" % (M, Cc)):
        check(lib.mspi_bn_bwd(dy.ptr, dy.ld, x.ptr, x.ld, y.ptr if y is not None else None, y.ld if y is not None else 0,
                              ptrs[0], ptrs[1], ptrs[2], dx.ptr, dx.ld, dgb[0].data_ptr(), dgb[1].data_ptr(), ws.data_ptr(),
                              M, Cc, _stream()), "mspi_bn_bwd")
    return dx, dgb[0], dgb[1]


# ----------------------------------------------------------------------------- SA gating / fusion backward (csrc/fusion_bwd.hip)
def rowgate_bwd(dy, x, gate, need_dx=True):
    """Backward of rowgate(x, gate): dy the gradient of the gated rows, x the UNGATED input, gate the CL [.., 1] of sigmoids.
    Returns (dx, dz): dx = dy (1 + gate), a new CL like dy (None with need_dx=False); dz [M] fp32, the gradient of the logit in
    front of the sigmoid."""
    lib = _lib.load()
    _need_gpu(dy.buf)
    dev = dy.buf.device
    if not dy.dense or not x.dense or (x.M, x.Cs) != (dy.M, dy.Cs) or dy.Cs != dy.C or x.buf.device != dev:
        raise MspiError("rowgate_bwd: dy (%d rows x %d) and x (%d rows x %d) must be dense, alike and a multiple of 4 wide"
                        % (dy.M, dy.C, x.M, x.C))
    if gate.M != dy.M or gate.ld != 1 or not gate.dense or gate.buf.device != dev:
        raise MspiError("rowgate_bwd: gate must hold one value per row (%d rows, ld 1), got %d rows, ld %d" % (dy.M, gate.M, gate.ld))
    dx = alloc(dy.N, dy.T, dy.H, dy.W, dy.C, dev) if need_dx else None
    dz = torch.empty(dy.M, dtype=torch.float32, device=dev)
    with _Timed("rowgate_bwd", 2.0 * dy.M * dy.C, 4.0 * dy.M * (dy.C * (3 if need_dx else 2) + 2), "M=%d C=%d" % (dy.M, dy.C)):
        check(lib.mspi_rowgate_bwd(dy.ptr, dy.ld, x.ptr, x.ld, gate.ptr, dx.ptr if need_dx else None, dx.ld if need_dx else 0,
                                   dz.data_ptr(), dy.M, dy.Cs, _stream()), "mspi_rowgate_bwd")
    return dx, dz


def upsample_sum_bwd(dx, srcs, accumulate=False):
    """Adjoint of upsample_sum: dx (= or +=) sum of the up-sample adjoints of srcs = [(CL gradient, factor 2 | 4 | 8), ...], at
    most three, in one pass over dx.  dx None: a new CL (accumulate must be off).  Returns dx."""
    lib = _lib.load()
    J = len(srcs)
    if not 1 <= J <= 3:
        raise MspiError("upsample_sum_bwd: 1 to 3 sources, got %d" % J)
    g0, k0 = srcs[0]
    _need_gpu(g0.buf)
    dev = g0.buf.device
    if k0 not in (2, 4, 8) or g0.H % k0 or g0.W % k0:
        raise MspiError("upsample_sum_bwd: factor %s must be 2, 4 or 8 and divide the gradient's %d x %d" % (k0, g0.H, g0.W))
    if dx is None:
        if accumulate:
            raise MspiError("upsample_sum_bwd: accumulate needs the dx to add to")
        dx = alloc(g0.N, g0.T, g0.H // k0, g0.W // k0, g0.C, dev)
    if not dx.dense or dx.Cs != dx.C or dx.buf.device != dev:
        raise MspiError("upsample_sum_bwd: dx must be dense, a multiple of 4 wide and on %s" % dev)
    for g, k in srcs:
        if k not in (2, 4, 8) or not g.dense or g.buf.device != dev or (g.N, g.T, g.H, g.W, g.C) != (dx.N, dx.T, dx.H * k, dx.W * k, dx.C):
            raise MspiError("upsample_sum_bwd: a dense gradient [%d,%d,%d,%d,%d] with factor %s is not factor (2, 4 or 8) times dx "
                            "[%d,%d,%d,%d,%d]" % (g.N, g.T, g.H, g.W, g.C, k, dx.N, dx.T, dx.H, dx.W, dx.C))
    ptrs = (C.c_void_p * J)(*[g.ptr for g, _ in srcs])
    lds = (C.c_int64 * J)(*[g.ld for g, _ in srcs])
    ks = (C.c_int32 * J)(*[k for _, k in srcs])
    with _Timed("upsample_sum_bwd", 0.0, 4.0 * (sum(g.M for g, _ in srcs) + dx.M * (2 if accumulate else 1)) * dx.C,
                "M=%d C=%d k=%s" % (dx.M, dx.C, ",".join(str(k) for _, k in srcs))):
        check(lib.mspi_upsample_sum_bwd(ptrs, lds, ks, J, dx.ptr, dx.ld, dx.N * dx.T, dx.H, dx.W, dx.Cs, 1 if accumulate else 0,
                                        _stream()), "mspi_upsample_sum_bwd")
    return dx

# ----------------------------------------------------------------------------- ConvNextBlock backward (csrc/block_bwd.hip)
LN_BWD_ROWS = 256               # rows per workgroup record of mspi_layernorm_bwd
LN_BWD_MAX_CH = 256             # widest row mspi_layernorm_bwd takes


def _rows_like(name, what, t, ref):
    if (t.M, t.C) != (ref.M, ref.C) or not t.dense or t.buf.device != ref.buf.device:
        raise MspiError("%s: %s must match (%d rows x %d channels, dense, on %s)" % (name, what, ref.M, ref.C, ref.buf.device))


def gelu_bwd(z, dg, need_g=True, inplace=False):
    """Backward of g = GELU(z) (erf form) for the gradient dg: returns (g, dz), CLs like z -- g the forward's activation again
    (None with need_g=False), dz = dg (Phi(z) + z phi(z)).  inplace=True: g overwrites z and dz overwrites dg."""
    lib = _lib.load()
    _need_gpu(z.buf)
    if not z.dense or z.Cs != z.C:
        raise MspiError("gelu_bwd: rows must be dense with a channel count that is a multiple of 4 (%d rows x %d)" % (z.M, z.C))
    _rows_like("gelu_bwd", "dg", dg, z)
    dev = z.buf.device
    g = (z if inplace else alloc(z.N, z.T, z.H, z.W, z.C, dev)) if need_g else None
    dz = dg if inplace else alloc(z.N, z.T, z.H, z.W, z.C, dev)
    with _Timed("gelu_bwd", 40.0 * z.M * z.C, 4.0 * z.M * z.C * (4 if need_g else 3), "M=%d C=%d" % (z.M, z.C)):
        check(lib.mspi_gelu_bwd(z.ptr, z.ld, dg.ptr, dg.ld, g.ptr if need_g else None, g.ld if need_g else 0, dz.ptr, dz.ld,
                                z.M, z.C, _stream()), "mspi_gelu_bwd")
    return g, dz


def layernorm_bwd(dy, x, gamma, eps=1e-5):
    """Backward of layernorm(x, gamma, beta, eps) over the channels of each row for the output gradient dy; mean and rstd are
    computed again from x.  Returns (dx, dgamma, dbeta): a CL like x and two fp32 [C]."""
    lib = _lib.load()
    _need_gpu(x.buf)
    M, Cc = _bn_rows("layernorm_bwd", x)
    if Cc > LN_BWD_MAX_CH:
        raise MspiError("layernorm_bwd: rows of %d channels, at most %d" % (Cc, LN_BWD_MAX_CH))
    _rows_like("layernorm_bwd", "dy", dy, x)
    dev = x.buf.device
    gp = _bn_vec("layernorm_bwd", "gamma", gamma, Cc, dev)
    dx = alloc(x.N, x.T, x.H, x.W, x.C, dev)
    dgb = torch.empty(2, Cc, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_layernorm_bwd_ws_bytes(M, Cc) // 4, dtype=torch.float32, device=dev)          # stream-ordered
    with _Timed("layernorm_bwd", 20.0 * M * Cc, 12.0 * M * Cc, "M=%d C=%d" % (M, Cc)):
        check(lib.mspi_layernorm_bwd(x.ptr, x.ld, dy.ptr, dy.ld, gp, float(eps), dx.ptr, dx.ld, dgb[0].data_ptr(), dgb[1].data_ptr(),
                                     ws.data_ptr(), M, Cc, _stream()), "mspi_layernorm_bwd")
    return dx, dgb[0], dgb[1]


def dwconv_wgrad(x, dy, pk):
    """Weight and bias gradient of dwconv(x, pk) for the output gradient dy (in front of any activation); pk gives the layer's
    geometry only.  Returns (dW, db) in the parameter's own layout, [C,1,kt,kh,kw] and [C]."""
    lib = _lib.load()
    _need_gpu(x.buf)
    if x.Cs != pk.c_s or dy.Cs != pk.c_s:
        raise MspiError("dwconv_wgrad: x has %d / dy %d stored channels, the layer %d" % (x.Cs, dy.Cs, pk.c_s))
    if not x.dense or not dy.dense or (dy.N, dy.T, dy.H, dy.W) != (x.N, x.T, x.H, x.W) or dy.buf.device != x.buf.device:
        raise MspiError("dwconv_wgrad: dy [%d,%d,%d,%d] must be dense and have the extent of x [%d,%d,%d,%d]"
                        % (dy.N, dy.T, dy.H, dy.W, x.N, x.T, x.H, x.W))
    d = _dw_desc(x, pk.k, pk.stride, pk.pad, dy.ld)
    if not lib.mspi_dwconv_wgrad_supported(C.byref(d)):
        raise MspiError("dwconv_wgrad: %s" % lib.mspi_last_error().decode("utf-8", "replace"))
    dev = x.buf.device
    taps = pk.k[0] * pk.k[1] * pk.k[2]
    dW = torch.empty(taps, pk.c_s, dtype=torch.float32, device=dev)
    db = torch.empty(pk.c_s, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_dwconv_wgrad_ws_bytes(C.byref(d)) // 4, dtype=torch.float32, device=dev)      # stream-ordered
    with _Timed("dwconv_wgrad", 2.0 * x.M * taps * pk.c, 8.0 * x.M * pk.c, "in=%s C=%d k=%s" % ((x.N, x.T, x.H, x.W), pk.c, pk.k)):
        check(lib.mspi_dwconv_wgrad(C.byref(d), x.ptr, dy.ptr, dW.data_ptr(), db.data_ptr(), ws.data_ptr(), _stream()),
              "mspi_dwconv_wgrad")
    return dW[:, :pk.c].t().reshape(pk.c, 1, *pk.k), db[:pk.c]


# ----------------------------------------------------------------------------- lateral entry convs (csrc/entry_bwd.hip)
WGRAD_ENTRY_SLICES = (64, 256, 512)     # rows per slice: the codes mspi_conv_wgrad_entry_variant answers
WGRAD_ENTRY_ROWS = (1024, 32768)        # output rows from which the second and the third are taken
WGRAD_ENTRY_MAX_CIN = 2560              # widest stored input mspi_conv_wgrad_entry takes


def conv_wgrad_entry_variant(x, dy, pk):
    """The instantiation conv_wgrad_entry(x, dy, pk) launches (rows per slice), -1 where it refuses; host only."""
    return _lib.load().mspi_conv_wgrad_entry_variant(C.byref(_wgrad_desc(x, dy, pk)), x.ptr, dy.ptr)


def conv_wgrad_entry(x, dy, pk):
    """conv_wgrad for the laterals' entry convs: kernel (s,1,1) == stride, s in {1, 2, 4}, no padding, stored Cout a multiple of
    32 up to 192, stored Cin any multiple of 4 up to 2560; x may be a channel slice of a wider buffer or a token view into a
    slab (its own sample stride).  pk gives the layer's geometry only.  Returns (dW [Co,Ci,s,1,1], db [Co])."""
    lib = _lib.load()
    _need_gpu(x.buf)
    if x.Cs != pk.cin_s or dy.Cs != pk.cout_s:
        raise MspiError("conv_wgrad_entry: x has %d / dy %d stored channels, the layer %d -> %d" % (x.Cs, dy.Cs, pk.cin_s, pk.cout_s))
    d = _wgrad_desc(x, dy, pk)
    if not dy.dense or dy.M != x.N * d.To * d.Ho * d.Wo or dy.buf.device != x.buf.device:
        raise MspiError("conv_wgrad_entry: dy has %d rows, the layer's output %d (or dy is not dense)"
                        % (dy.M, x.N * d.To * d.Ho * d.Wo))
    if lib.mspi_conv_wgrad_entry_variant(C.byref(d), x.ptr, dy.ptr) < 0:
        raise MspiError("conv_wgrad_entry: %s" % lib.mspi_last_error().decode("utf-8", "replace"))
    dev = x.buf.device
    s = pk.k[0]
    dW = torch.empty(pk.cout_s, s, 1, 1, pk.cin_s, dtype=torch.float32, device=dev)
    db = torch.empty(pk.cout_s, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_conv_wgrad_entry_ws_bytes(C.byref(d)) // 4, dtype=torch.float32, device=dev)   # stream-ordered
    with _Timed("conv_wgrad_entry", 2.0 * dy.M * s * pk.cin * pk.cout, 4.0 * dy.M * (s * pk.cin + pk.cout),
                "M=%d K=%d(%dx%d) N=%d" % (dy.M, s * pk.cin, s, pk.cin, pk.cout)):
        check(lib.mspi_conv_wgrad_entry(C.byref(d), x.ptr, dy.ptr, dW.data_ptr(), db.data_ptr(), ws.data_ptr(), _stream()),
              "mspi_conv_wgrad_entry")
    return dW[:pk.cout, :, :, :, :pk.cin].permute(0, 4, 1, 2, 3), db[:pk.cout]


# ----------------------------------------------------------------------------- adapter (csrc/adapter_bwd.hip)
WGRAD_T16_SLICES = (64, 128, 256)       # rows per slice: the codes mspi_conv_wgrad_t16_variant answers
WGRAD_T16_ROWS = (1024, 8192)           # rows from which the second and the third are taken
WGRAD_T16_MAX_CIN, WGRAD_T16_MAX_COUT = 416, 208


def conv_wgrad_t16_variant(x, dy, pk):
    """The instantiation conv_wgrad_t16(x, dy, pk) launches (rows per slice), -1 where it refuses; host only."""
    return _lib.load().mspi_conv_wgrad_t16_variant(C.byref(_wgrad_desc(x, dy, pk)), x.ptr, dy.ptr)


def conv_wgrad_t16(x, dy, pk, bias=False):
    """conv_wgrad on 16 x 16 tiles for the adapter's layers: a stride-1 "same" conv (1,1,1), (1,3,3) or (3,1,1), stored Cin a
    multiple of 16 up to 416, stored Cout a multiple of 16 up to 208; x and dy may be channel slices of wider buffers.  pk gives
    the layer's geometry only.  Returns (dW [Co,Ci,kt,kh,kw], db [Co] or None without bias)."""
    lib = _lib.load()
    _need_gpu(x.buf)
    if x.Cs != pk.cin_s or dy.Cs != pk.cout_s:
        raise MspiError("conv_wgrad_t16: x has %d / dy %d stored channels, the layer %d -> %d" % (x.Cs, dy.Cs, pk.cin_s, pk.cout_s))
    d = _wgrad_desc(x, dy, pk)
    if not dy.dense or dy.M != x.M or dy.buf.device != x.buf.device:
        raise MspiError("conv_wgrad_t16: dy has %d rows, the layer's output %d (or dy has a sample stride of its own)" % (dy.M, x.M))
    if lib.mspi_conv_wgrad_t16_variant(C.byref(d), x.ptr, dy.ptr) < 0:
        raise MspiError("conv_wgrad_t16: %s" % lib.mspi_last_error().decode("utf-8", "replace"))
    dev = x.buf.device
    kt, kh, kw = pk.k
    dW = torch.empty(pk.cout_s, kt, kh, kw, pk.cin_s, dtype=torch.float32, device=dev)
    db = torch.empty(pk.cout_s, dtype=torch.float32, device=dev) if bias else None
    ws = torch.empty(lib.mspi_conv_wgrad_t16_ws_bytes(C.byref(d)) // 4, dtype=torch.float32, device=dev)     # stream-ordered
    taps = kt * kh * kw
    with _Timed("conv_wgrad_t16", 2.0 * dy.M * taps * pk.cin * pk.cout, 4.0 * dy.M * (pk.cin + pk.cout),
                "M=%d K=%d(%dx%d) N=%d" % (dy.M, taps * pk.cin, taps, pk.cin, pk.cout)):
        check(lib.mspi_conv_wgrad_t16(C.byref(d), x.ptr, dy.ptr, dW.data_ptr(), db.data_ptr() if bias else None, ws.data_ptr(),
                                      _stream()), "mspi_conv_wgrad_t16")
    return dW.permute(0, 4, 1, 2, 3), db


# ----------------------------------------------------------------------------- transformer Block backward (csrc/sync_bwd.hip)
ATTN_BWD_PAIRS = ((128, 128),)           # the (D, Dv) pairs mspi_attn_bwd is instantiated for
LN_BWD_WIDE_CH = (260, 512)              # the row widths mspi_layernorm_bwd_wide takes; below them mspi_layernorm_bwd


def attention_bwd(qkv, o, dO, B, Ntok, heads, hd, scale, out=None):
    """Backward of o = attention(qkv, B, Ntok, heads, hd, scale) for the output gradient dO: returns dqkv, a CL like qkv with
    columns [3][heads][hd] = [dq | dk | dv].  o and dO are CLs of heads * hd columns with the rows of qkv.  out: the CL to write
    (a slab like qkv; not qkv itself).  fp32 MFMA whatever the forward ran on: dO is a gradient (autograd._pack_dgrad)."""
    lib = _lib.load()
    for t in (qkv, o, dO) + ((out,) if out is not None else ()):
        _need_gpu(t.buf)
    Cc = heads * hd
    if (hd, hd) not in ATTN_BWD_PAIRS:
        raise MspiError("attention_bwd: head dim (D=%d, Dv=%d) not in %s" % (hd, hd, list(ATTN_BWD_PAIRS)))
    if qkv.C != 3 * Cc or qkv.M != B * Ntok:
        raise MspiError("attention_bwd: qkv is %d rows x %d columns, expected %d x %d ([3][%d][%d])" % (qkv.M, qkv.C, B * Ntok, 3 * Cc, heads, hd))
    for name, t in (("o", o), ("dO", dO)):
        if t.M != qkv.M or t.C != Cc or t.buf.device != qkv.buf.device:
            raise MspiError("attention_bwd: %s is %d rows x %d columns on %s, expected %d x %d on %s"
                            % (name, t.M, t.C, t.buf.device, qkv.M, Cc, qkv.buf.device))
    if out is None:
        out = alloc(qkv.N, qkv.T, qkv.H, qkv.W, 3 * Cc, qkv.buf.device)
    elif out.M != qkv.M or out.C != 3 * Cc or out.buf.device != qkv.buf.device:
        raise MspiError("attention_bwd: out is %d rows x %d columns on %s, expected %d x %d on %s"
                        % (out.M, out.C, out.buf.device, qkv.M, 3 * Cc, qkv.buf.device))
    d = AttnDesc()
    d.B, d.Hh, d.Nq, d.Nk, d.D, d.Dv, d.nmask, d.nwin = B, heads, Ntok, Ntok, hd, hd, 0, 0
    d.q_sB = d.k_sB = d.v_sB = Ntok * qkv.ld
    d.q_sH = d.k_sH = d.v_sH = hd
    d.q_sT = d.k_sT = d.v_sT = qkv.ld
    d.o_sB, d.o_sH, d.o_sT = Ntok * o.ld, hd, o.ld
    d.scale, d.prec = float(scale), PREC_F32
    if out.ld != qkv.ld or dO.ld != o.ld:
        raise MspiError("attention_bwd: out must have the row stride of qkv (%d, got %d) and dO that of o (%d, got %d)"
                        % (qkv.ld, out.ld, o.ld, dO.ld))
    ws = torch.empty(lib.mspi_attn_bwd_ws_bytes(C.byref(d)) // 4, dtype=torch.float32, device=qkv.buf.device)      # stream-ordered
    with _Timed("attention_bwd", 14.0 * B * heads * Ntok * Ntok * hd, 4.0 * B * Ntok * Cc * 8, "B=%d h=%d N=%d d=%d" % (B, heads, Ntok, hd)):
        check(lib.mspi_attn_bwd(C.byref(d), qkv.ptr, qkv.ptr + 4 * Cc, qkv.ptr + 8 * Cc, o.ptr, dO.ptr, out.ptr, out.ptr + 4 * Cc,
                                out.ptr + 8 * Cc, ws.data_ptr(), _stream()), "mspi_attn_bwd")
    return out


def layernorm_bwd_wide(dy, x, gamma, eps=1e-5):
    """layernorm_bwd for rows of 256 < C <= 512 channels (mspi_layernorm_bwd_wide): returns (dx, dgamma, dbeta), a CL like x and
    two fp32 [C]."""
    lib = _lib.load()
    _need_gpu(x.buf)
    M, Cc = _bn_rows("layernorm_bwd_wide", x)
    if not LN_BWD_WIDE_CH[0] <= Cc <= LN_BWD_WIDE_CH[1]:
        raise MspiError("layernorm_bwd_wide: rows of %d channels, takes %d to %d (layernorm_bwd below)" % ((Cc,) + LN_BWD_WIDE_CH))
    _rows_like("layernorm_bwd_wide", "dy", dy, x)
    dev = x.buf.device
    gp = _bn_vec("layernorm_bwd_wide", "gamma", gamma, Cc, dev)
    dx = alloc(x.N, x.T, x.H, x.W, x.C, dev)
    dgb = torch.empty(2, Cc, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_layernorm_bwd_wide_ws_bytes(M, Cc) // 4, dtype=torch.float32, device=dev)     # stream-ordered
    with _Timed("layernorm_bwd_wide", 20.0 * M * Cc, 12.0 * M * Cc, "M=%d C=%d" % (M, Cc)):
        check(lib.mspi_layernorm_bwd_wide(x.ptr, x.ld, dy.ptr, dy.ld, gp, float(eps), dx.ptr, dx.ld, dgb[0].data_ptr(),
                                          dgb[1].data_ptr(), ws.data_ptr(), M, Cc, _stream()), "mspi_layernorm_bwd_wide")
    return dx, dgb[0], dgb[1]


# ----------------------------------------------------------------------------- linear layers (csrc/linear_wgrad.hip)
LINEAR_WGRAD_MAX_W = 4096                # widest N and K mspi_linear_wgrad takes
LINEAR_WGRAD_WGS = 512                   # workgroups its slice arithmetic aims at (include/mspi_linear_train_hip.h)


def linear_wgrad_variant(x, dy):
    """Rows per slice of the launch linear_wgrad(x, dy) makes, -1 where it refuses; host only."""
    return _lib.load().mspi_linear_wgrad_variant(x.ptr, x.ld, dy.ptr, dy.ld, x.M, dy.C, x.C)


def linear_wgrad(x, dy, bias=True):
    """Weight and bias gradient of y = x W^T + b over rows (mspi_linear_wgrad): x a CL of M rows x K columns, dy one of M rows x N
    columns, each read where it lies (a channel slice of a wider buffer, the slab attention_bwd writes).  N a multiple of 32, K a
    multiple of 4, both at most 4096.  Returns (dW [N, K], db [N] or None without bias)."""
    lib = _lib.load()
    _need_gpu(x.buf)
    _need_gpu(dy.buf)
    if dy.buf.device != x.buf.device:
        raise MspiError("linear_wgrad: x on %s, dy on %s" % (x.buf.device, dy.buf.device))
    if dy.M != x.M:
        raise MspiError("linear_wgrad: x has %d rows, dy %d: the row counts must match" % (x.M, dy.M))
    if not x.dense or not dy.dense:
        raise MspiError("linear_wgrad: x and dy must be rows one row stride apart (no sample stride of their own)")
    M, N, K = x.M, dy.C, x.C
    if lib.mspi_linear_wgrad_variant(x.ptr, x.ld, dy.ptr, dy.ld, M, N, K) < 0:
        raise MspiError("linear_wgrad: %d rows, x %d wide (row stride %d), dy %d wide (row stride %d): %s"
                        % (M, K, x.ld, N, dy.ld, lib.mspi_last_error().decode("utf-8", "replace")))
    dev = x.buf.device
    dW = torch.empty(N, K, dtype=torch.float32, device=dev)
    db = torch.empty(N, dtype=torch.float32, device=dev) if bias else None
    ws = torch.empty(lib.mspi_linear_wgrad_ws_bytes(M, N, K) // 4, dtype=torch.float32, device=dev)          # stream-ordered
    with _Timed("linear_wgrad", 2.0 * M * N * K, 4.0 * M * (N + K), "M=%d K=%d N=%d" % (M, K, N)):
        check(lib.mspi_linear_wgrad(x.ptr, x.ld, dy.ptr, dy.ld, dW.data_ptr(), db.data_ptr() if bias else None, ws.data_ptr(),
                                    M, N, K, _stream()), "mspi_linear_wgrad")
    return dW, db


# ----------------------------------------------------------------------------- contrastive head (csrc/contrast_bwd.hip)
LN_ACT_BWD_MAX_CH = 2048                 # widest row mspi_layernorm_act_bwd takes
LN_ACT_BWD_ROWS = 8                      # rows per workgroup record of mspi_layernorm_act_bwd


def neg_cosine_bwd(p, z, g, scale):
    """The gradient of neg_cosine(p, z, out, scale, .) with respect to p for the gradient g of out, a one-element fp32 tensor on
    the device (read by the kernel: nothing synchronises); z is a constant.  p, z: dense CLs of N rows x C columns.  Returns dp,
    a CL like p."""
    lib = _lib.load()
    _need_gpu(p.buf)
    if (z.M, z.C) != (p.M, p.C) or p.ld != p.C or z.ld != z.C or not p.dense or not z.dense or z.buf.device != p.buf.device:
        raise MspiError("neg_cosine_bwd: p and z must be dense rows of one shape on one device (p %d x %d, z %d x %d)"
                        % (p.M, p.C, z.M, z.C))
    if g.dtype != torch.float32 or g.numel() != 1 or g.device != p.buf.device:
        raise MspiError("neg_cosine_bwd: g must be one fp32 element on %s, got %s %s on %s"
                        % (p.buf.device, g.dtype, tuple(g.shape), g.device))
    dp = alloc(p.N, p.T, p.H, p.W, p.C, p.buf.device, ld=p.C)
    with _Timed("neg_cosine_bwd", 8.0 * p.M * p.C, 12.0 * p.M * p.C, "N=%d C=%d" % (p.M, p.C)):
        check(lib.mspi_neg_cosine_bwd(p.ptr, z.ptr, g.data_ptr(), dp.ptr, p.M, p.C, float(scale), _stream()), "mspi_neg_cosine_bwd")
    return dp


def layernorm_act_bwd(dy, x, gamma, eps=1e-5, y=None, inplace=False):
    """Backward of act(layernorm(x, gamma, beta, eps)) for rows of up to 2048 channels (mspi_layernorm_act_bwd): act is the ReLU
    where the forward's output y is given (dy counts only where y > 0), the identity with y None.  inplace=True writes dx over
    dy.  Returns (dx, dgamma, dbeta): a CL like x and two fp32 [C]."""
    lib = _lib.load()
    _need_gpu(x.buf)
    M, Cc = _bn_rows("layernorm_act_bwd", x)
    if Cc > LN_ACT_BWD_MAX_CH:
        raise MspiError("layernorm_act_bwd: rows of %d channels, at most %d" % (Cc, LN_ACT_BWD_MAX_CH))
    _rows_like("layernorm_act_bwd", "dy", dy, x)
    if y is not None:
        _rows_like("layernorm_act_bwd", "y", y, x)
    dev = x.buf.device
    gp = _bn_vec("layernorm_act_bwd", "gamma", gamma, Cc, dev)
    dx = dy if inplace else alloc(x.N, x.T, x.H, x.W, x.C, dev)
    dgb = torch.empty(2, Cc, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_layernorm_act_bwd_ws_bytes(M, Cc) // 4, dtype=torch.float32, device=dev)       # stream-ordered
    with _Timed("layernorm_act_bwd", 20.0 * M * Cc, 4.0 * M * Cc * (3 if y is None else 4), "M=%d C=%d" % (M, Cc)):
        check(lib.mspi_layernorm_act_bwd(x.ptr, x.ld, dy.ptr, dy.ld, None if y is None else y.ptr, 0 if y is None else y.ld, gp,
                                         float(eps), dx.ptr, dx.ld, dgb[0].data_ptr(), dgb[1].data_ptr(), ws.data_ptr(), M, Cc,
                                         _stream()), "mspi_layernorm_act_bwd")
    return dx, dgb[0], dgb[1]


def mean_rows_bwd(g, dx, accumulate=False):
    """The adjoint of mean_rows(x, N, R, out): dx[n, r, :] (+)= g[n, :] / R over the R = T*H*W rows of each sample of the CL dx
    (a token view into a slab: rows outside it are not touched).  g: contiguous fp32 [N, C]."""
    lib = _lib.load()
    _need_gpu(dx.buf)
    if g.dtype != torch.float32 or tuple(g.shape) != (dx.N, dx.C) or not g.is_contiguous() or g.device != dx.buf.device:
        raise MspiError("mean_rows_bwd: g must be contiguous fp32 [%d, %d] on %s, got %s %s on %s"
                        % (dx.N, dx.C, dx.buf.device, g.dtype, tuple(g.shape), g.device))
    R = dx.T * dx.H * dx.W
    with _Timed("mean_rows_bwd", 1.0 * dx.M * dx.C, 4.0 * dx.M * dx.C * (2 if accumulate else 1), "N=%d R=%d C=%d" % (dx.N, R, dx.C)):
        check(lib.mspi_mean_rows_bwd(g.data_ptr(), dx.ptr, dx.ld, dx.sN, dx.N, R, dx.C, 1 if accumulate else 0, _stream()),
              "mspi_mean_rows_bwd")
    return dx


# ----------------------------------------------------------------------------- X3D block backward (csrc/x3d_bwd.hip)
X3D_TRAIN_MAX_CH = 4096                  # widest row the mspi_x3d_train_hip.h entry points take
SE_TRAIN_MAX_F = 64                      # widest fc1.out_channels mspi_se_train_fwd / _bwd take
DWCONV3_WGRAD_RECORDS = 256              # records the band rule of mspi_dwconv3_wgrad aims at
GATE_SWISH_BWD_ROWS = 32                 # rows of a sample per record of mspi_gate_swish_bwd


def _x3d_rows(name, what, t, ref=None):
    """A CL of dense samples, a multiple of 4 wide and at most X3D_TRAIN_MAX_CH, on the GPU; shaped like ref where given."""
    _need_gpu(t.buf)
    if not t.dense or t.Cs != t.C or t.C > X3D_TRAIN_MAX_CH:
        raise MspiError("%s: %s must be dense rows with a channel count that is a multiple of 4, at most %d (%d rows x %d)"
                        % (name, what, X3D_TRAIN_MAX_CH, t.M, t.C))
    if ref is not None and ((t.N, t.T, t.H, t.W, t.C) != (ref.N, ref.T, ref.H, ref.W, ref.C) or t.buf.device != ref.buf.device):
        raise MspiError("%s: %s [%d,%d,%d,%d,%d] must match [%d,%d,%d,%d,%d] on %s"
                        % (name, what, t.N, t.T, t.H, t.W, t.C, ref.N, ref.T, ref.H, ref.W, ref.C, ref.buf.device))


def _x3d_mat(name, what, t, shape, dev):
    if t.dtype != torch.float32 or t.numel() != shape[0] * shape[1] or t.device != dev or not t.is_contiguous():
        raise MspiError("%s: %s must be a contiguous fp32 tensor of %d x %d elements on %s, got %s %s on %s"
                        % (name, what, shape[0], shape[1], dev, t.dtype, tuple(t.shape), t.device))
    return t.data_ptr()


def dwconv3_wgrad(x, dy, bias=False):
    """Weight (and with bias=True bias) gradient of a depthwise (3,3,3) conv, padding (1,1,1), stride 1, for the output gradient
    dy (mspi_dwconv3_wgrad); x and dy are read where they lie (channel slices of wider buffers).  Returns (dW [C,1,3,3,3], db [C]
    or None)."""
    lib = _lib.load()
    _x3d_rows("dwconv3_wgrad", "x", x)
    _x3d_rows("dwconv3_wgrad", "dy", dy, x)
    d = _dw_desc(x, (3, 3, 3), (1, 1, 1), (1, 1, 1), dy.ld)
    if not lib.mspi_dwconv3_wgrad_supported(C.byref(d)):
        raise MspiError("dwconv3_wgrad: %s" % lib.mspi_last_error().decode("utf-8", "replace"))
    dev = x.buf.device
    dW = torch.empty(x.C, 1, 3, 3, 3, dtype=torch.float32, device=dev)
    db = torch.empty(x.C, dtype=torch.float32, device=dev) if bias else None
    ws = torch.empty(lib.mspi_dwconv3_wgrad_ws_bytes(C.byref(d)) // 4, dtype=torch.float32, device=dev)     # stream-ordered
    with _Timed("dwconv3_wgrad", 54.0 * x.M * x.C, 8.0 * x.M * x.C, "in=%s C=%d" % ((x.N, x.T, x.H, x.W), x.C)):
        check(lib.mspi_dwconv3_wgrad(C.byref(d), x.ptr, dy.ptr, dW.data_ptr(), db.data_ptr() if bias else None, ws.data_ptr(),
                                     _stream()), "mspi_dwconv3_wgrad")
    return dW, db


def bn_gate_act(x, mean, rstd, gamma, beta, gate=None, res=None, act=ACT_NONE, out=None):
    """y = act(res + gate (gamma (x - mean) rstd + beta)) in one pass (mspi_bn_gate_act_fwd): gate fp32 [N, C] per sample or
    None, res a CL like x or None, act ACT_RELU, ACT_SWISH or ACT_NONE.  Returns a CL like x (a new one, or out)."""
    lib = _lib.load()
    _x3d_rows("bn_gate_act", "x", x)
    dev = x.buf.device
    if act not in (ACT_NONE, ACT_RELU, ACT_SWISH):
        raise MspiError("bn_gate_act: act must be ACT_NONE, ACT_RELU or ACT_SWISH, got %s" % (act,))
    ptrs = [_bn_vec("bn_gate_act", n, t, x.C, dev) for n, t in (("mean", mean), ("rstd", rstd), ("gamma", gamma), ("beta", beta))]
    gp = None if gate is None else _x3d_mat("bn_gate_act", "gate", gate, (x.N, x.C), dev)
    if res is not None:
        _x3d_rows("bn_gate_act", "res", res, x)
    if out is None:
        out = alloc(x.N, x.T, x.H, x.W, x.C, dev)
    else:
        _x3d_rows("bn_gate_act", "out", out, x)
    with _Timed("bn_gate_act", 6.0 * x.M * x.C, 4.0 * x.M * x.C * (2 if res is None else 3), "M=%d C=%d" % (x.M, x.C)):
        check(lib.mspi_bn_gate_act_fwd(x.ptr, x.ld, ptrs[0], ptrs[1], ptrs[2], ptrs[3], gp, None if res is None else res.ptr,
                                       0 if res is None else res.ld, out.ptr, out.ld, x.M, x.T * x.H * x.W, x.C, act, _stream()),
              "mspi_bn_gate_act_fwd")
    return out


def gate_swish_bwd(ds, v0, mean, rstd, gamma, beta, gate=None, inplace=False):
    """Backward of s = swish(gate bn(v0)) for the gradient ds (mspi_gate_swish_bwd), the norm, the product and the sigmoid
    computed again from the pre-norm v0.  Returns (dv, dgate): a CL like v0 (over ds with inplace=True) and fp32 [N, C], None
    without a gate."""
    lib = _lib.load()
    _x3d_rows("gate_swish_bwd", "v0", v0)
    _x3d_rows("gate_swish_bwd", "ds", ds, v0)
    dev = v0.buf.device
    N, R, Cc = v0.N, v0.T * v0.H * v0.W, v0.C
    ptrs = [_bn_vec("gate_swish_bwd", n, t, Cc, dev) for n, t in (("mean", mean), ("rstd", rstd), ("gamma", gamma), ("beta", beta))]
    gp = None if gate is None else _x3d_mat("gate_swish_bwd", "gate", gate, (N, Cc), dev)
    if N >= 65536:
        raise MspiError("gate_swish_bwd: %d samples, fewer than 65536" % N)
    dv = ds if inplace else alloc(v0.N, v0.T, v0.H, v0.W, Cc, dev)
    dgate = ws = None
    if gate is not None:
        dgate = torch.empty(N, Cc, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.mspi_gate_swish_bwd_ws_bytes(N, R, Cc) // 4, dtype=torch.float32, device=dev)  # stream-ordered
    with _Timed("gate_swish_bwd", 20.0 * v0.M * Cc, 12.0 * v0.M * Cc, "N=%d R=%d C=%d" % (N, R, Cc)):
        check(lib.mspi_gate_swish_bwd(ds.ptr, ds.ld, v0.ptr, v0.ld, ptrs[0], ptrs[1], ptrs[2], ptrs[3], gp, dv.ptr, dv.ld,
                                      None if gate is None else dgate.data_ptr(), None if gate is None else ws.data_ptr(), N, R, Cc,
                                      _stream()), "mspi_gate_swish_bwd")
    return dv, dgate


def _se_dims(name, pool, b1):
    _need_gpu(pool)
    if pool.dim() != 2 or pool.dtype != torch.float32 or not pool.is_contiguous():
        raise MspiError("%s: the rows must be contiguous fp32 [N, C], got %s %s" % (name, pool.dtype, tuple(pool.shape)))
    N, Cc, F = pool.shape[0], pool.shape[1], b1
    if not 0 < N < 65536 or Cc % 4 or not 0 < Cc <= X3D_TRAIN_MAX_CH or not 0 < F <= SE_TRAIN_MAX_F:
        raise MspiError("%s: N=%d C=%d F=%d: fewer than 65536 samples, C a multiple of 4 up to %d, fc1.out_channels F up to %d"
                        % (name, N, Cc, F, X3D_TRAIN_MAX_CH, SE_TRAIN_MAX_F))
    return N, Cc, F


def se_train_fwd(pool0, mean, rstd, gamma, beta, w1, b1, w2, b2):
    """The squeeze-excite MLP behind a BatchNorm on batch statistics (mspi_se_train_fwd): pool0 fp32 [N, C] = mean_rows of the
    pre-norm map, w1 [F,C,1,1,1], b1 [F], w2 [C,F,1,1,1], b2 [C] contiguous fp32.  Returns (p [N, C], h [N, F], gate [N, C])."""
    lib = _lib.load()
    N, Cc, F = _se_dims("se_train_fwd", pool0, b1.numel())
    dev = pool0.device
    vec = [_bn_vec("se_train_fwd", n, t, Cc, dev) for n, t in (("mean", mean), ("rstd", rstd), ("gamma", gamma), ("beta", beta))]
    pw1, pw2 = _x3d_mat("se_train_fwd", "fc1.weight", w1, (F, Cc), dev), _x3d_mat("se_train_fwd", "fc2.weight", w2, (Cc, F), dev)
    pb1, pb2 = _bn_vec("se_train_fwd", "fc1.bias", b1, F, dev), _bn_vec("se_train_fwd", "fc2.bias", b2, Cc, dev)
    p, gate = (torch.empty(N, Cc, dtype=torch.float32, device=dev) for _ in range(2))
    h = torch.empty(N, F, dtype=torch.float32, device=dev)
    with _Timed("se_train_fwd", 4.0 * N * Cc * F, 8.0 * Cc * F, "N=%d C=%d F=%d" % (N, Cc, F)):
        check(lib.mspi_se_train_fwd(pool0.data_ptr(), vec[0], vec[1], vec[2], vec[3], pw1, pb1, pw2, pb2, p.data_ptr(), h.data_ptr(),
                                    gate.data_ptr(), N, Cc, F, _stream()), "mspi_se_train_fwd")
    return p, h, gate


def se_train_bwd(dgate, gate, h, p, w1, w2):
    """Backward of se_train_fwd from dgate [N, C] with the forward's p, h and gate (mspi_se_train_bwd), the samples added in index
    order.  Returns (dw1 [F,C,1,1,1], db1 [F], dw2 [C,F,1,1,1], db2 [C], dp [N, C]); mean_rows_bwd(dp, dv, accumulate=True) is
    the caller's."""
    lib = _lib.load()
    N, Cc, F = _se_dims("se_train_bwd", dgate, h.shape[-1] if h.dim() == 2 else 0)
    dev = dgate.device
    pg, pp = _x3d_mat("se_train_bwd", "gate", gate, (N, Cc), dev), _x3d_mat("se_train_bwd", "p", p, (N, Cc), dev)
    ph = _x3d_mat("se_train_bwd", "h", h, (N, F), dev)
    pw1, pw2 = _x3d_mat("se_train_bwd", "fc1.weight", w1, (F, Cc), dev), _x3d_mat("se_train_bwd", "fc2.weight", w2, (Cc, F), dev)
    dw1 = torch.empty(F, Cc, 1, 1, 1, dtype=torch.float32, device=dev)
    dw2 = torch.empty(Cc, F, 1, 1, 1, dtype=torch.float32, device=dev)
    db1, db2 = torch.empty(F, dtype=torch.float32, device=dev), torch.empty(Cc, dtype=torch.float32, device=dev)
    dp = torch.empty(N, Cc, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.mspi_se_train_bwd_ws_bytes(N, Cc, F) // 4, dtype=torch.float32, device=dev)        # stream-ordered
    with _Timed("se_train_bwd", 8.0 * N * Cc * F, 16.0 * Cc * F, "N=%d C=%d F=%d" % (N, Cc, F)):
        check(lib.mspi_se_train_bwd(dgate.data_ptr(), pg, ph, pp, pw1, pw2, dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(),
                                    db2.data_ptr(), dp.data_ptr(), ws.data_ptr(), N, Cc, F, _stream()), "mspi_se_train_bwd")
    return dw1, db1, dw2, db2, dp


def relu_mask_add(dx, g, y):
    """dx += g where y > 0 (mspi_relu_mask_add): the skip path of y = relu(x + f(x)).  Returns dx."""
    lib = _lib.load()
    _need_gpu(dx.buf)
    for what, t in (("dx", dx), ("g", g), ("y", y)):
        if not t.dense or t.Cs != t.C or (t.M, t.C) != (dx.M, dx.C) or t.buf.device != dx.buf.device:
            raise MspiError("relu_mask_add: %s must be dense rows, a multiple of 4 wide, like dx (%d rows x %d on %s)"
                            % (what, dx.M, dx.C, dx.buf.device))
    with _Timed("relu_mask_add", 1.0 * dx.M * dx.C, 16.0 * dx.M * dx.C, "M=%d C=%d" % (dx.M, dx.C)):
        check(lib.mspi_relu_mask_add(dx.ptr, dx.ld, g.ptr, g.ld, y.ptr, y.ld, dx.M, dx.C, _stream()), "mspi_relu_mask_add")
    return dx


def mean_rows(x, N, R, out):
    """x: CL with R = T*H*W rows per sample (token slabs allowed); out [N, C] tensor."""
    lib = _lib.load()
    assert x.N == N and x.T * x.H * x.W == R
    S = lib.mspi_mean_rows_slices(R)
    if S:      # long samples: two deterministic stages through a workspace (stream-ordered: safe to drop after the launch)
        ws = torch.empty(N * S * x.C, dtype=torch.float32, device=x.buf.device)
        check(lib.mspi_mean_rows_ws(x.ptr, x.ld, x.sN, out.data_ptr(), ws.data_ptr(), N, R, x.C, _stream()), "mspi_mean_rows_ws")
    else:
        check(lib.mspi_mean_rows(x.ptr, x.ld, x.sN, out.data_ptr(), N, R, x.C, _stream()), "mspi_mean_rows")
    return out


def neg_cosine(p, z, out, scale, accumulate):
    lib = _lib.load()
    assert p.ld == p.C and z.ld == z.C and p.dense and z.dense
    check(lib.mspi_neg_cosine(p.ptr, z.ptr, out.data_ptr(), p.M, p.C, float(scale), 1 if accumulate else 0, _stream()),
          "mspi_neg_cosine")
    return out


def add(a, b, y):
    lib = _lib.load()
    check(lib.mspi_add(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), _stream()), "mspi_add")
    return y


def permute(src, dims, strides, out=None):
    """Strided gather (mspi_permute_fwd): dense fp32 tensor of shape `dims` (<= 6, innermost contiguous on both sides)
    with out[i0..] = src.flat[sum_k i_k * strides[k]].  src: a CL (its buffer from .ptr on) or a flat torch tensor."""
    lib = _lib.load()
    if isinstance(src, CL):
        _need_gpu(src.buf)
        ptr, n_src, dev = src.ptr, src.buf.numel() - src.off, src.buf.device
    else:
        _need_gpu(src)
        ptr, n_src, dev = src.data_ptr(), src.numel(), src.device
    dims, strides = list(dims), list(strides)
    assert len(dims) == len(strides) <= 6
    pad = 6 - len(dims)
    d = _lib.PermuteDesc()
    d.dims[:] = [1] * pad + dims
    d.strides[:] = [0] * pad + strides
    d.src_elems = n_src
    n = 1
    for v in dims:
        n *= v
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=dev)
    assert out.numel() == n
    with _Timed("permute", 0.0, 8.0 * n):
        check(lib.mspi_permute_fwd(C.byref(d), ptr, out.data_ptr(), _stream()), "mspi_permute_fwd")
    return out


def gated_sum(srcs, logit, out=None):
    """sum_j softmax_j(logit[n, c*J+j]) * srcs[j][n,r,c] over dense CLs of one shape (J = len(srcs) in {2, 3})."""
    lib = _lib.load()
    a = srcs[0]
    for s_ in srcs:
        _need_gpu(s_.buf)
        assert s_.dense and s_.ld == a.C and (s_.N, s_.M, s_.C) == (a.N, a.M, a.C)
    if out is None:
        out = alloc(a.N, a.T, a.H, a.W, a.C, a.buf.device)
    J = len(srcs)
    assert logit.shape == (a.N, a.C * J) and logit.is_contiguous() and out.ld == a.C
    with _Timed("gated_sum", 0.0, 4.0 * (J + 1) * a.M * a.C):
        check(lib.mspi_gated_sum_fwd(srcs[0].ptr, srcs[1].ptr, srcs[2].ptr if J == 3 else None, logit.data_ptr(), out.ptr,
                                     a.N, a.M // a.N, a.C, J, _stream()), "mspi_gated_sum_fwd")
    return out


def postprocess_u8(logmap, out_hw, out=None):
    """[N,H,W] log-probability maps (GPU) -> uint8 [N,Ho,Wo] grey maps: blur, exp, resize, min-max, round.
    out: where the last kernel writes -- a device tensor (default: a new one) or a PINNED host tensor, which the kernel
    addresses directly (no D2H copy is queued; the caller synchronises on an event behind the launch before reading)."""
    lib = _lib.load()
    _need_gpu(logmap)
    N, H, W = logmap.shape
    Ho, Wo = out_hw
    logmap = logmap.contiguous()
    ws = torch.empty(lib.mspi_postprocess_workspace(N, H, W, Ho, Wo), dtype=torch.uint8, device=logmap.device)
    if out is None:
        out = torch.empty(N, Ho, Wo, dtype=torch.uint8, device=logmap.device)
    elif not (out.dtype == torch.uint8 and tuple(out.shape) == (N, Ho, Wo) and out.is_contiguous()
              and (out.is_cuda or out.is_pinned())):
        raise MspiError("postprocess_u8: out must be a contiguous uint8 [N,Ho,Wo] device tensor or pinned host tensor")
    check(lib.mspi_postprocess_u8(logmap.data_ptr(), out.data_ptr(), ws.data_ptr(), N, H, W, Ho, Wo, _stream()),
          "mspi_postprocess_u8")
    return out


_JPEG_PLANS = {}


def jpeg_encode_gray(maps_u8, quality=95):
    """[B,H,W] uint8 grey maps (GPU) -> (files uint8 [B,cap], lengths int32 [B]), both on the GPU: files[b, :lengths[b]] is the
    baseline JPEG file libjpeg writes for maps[b] at `quality` -- PIL.Image.save(format="JPEG", quality=quality), byte for
    byte (inference.py:89-91 writes with cv2.imwrite).  Rows of `maps_u8` may be a view into a wider buffer (unit stride along
    W).  The header template and the workspace are cached per (H, W, quality, B), so calls of one shape must be ordered on one
    stream; no host synchronisation."""
    lib = _lib.load()
    _need_gpu(maps_u8)
    if maps_u8.dtype != torch.uint8 or maps_u8.dim() != 3:
        raise MspiError("jpeg_encode_gray: maps must be a uint8 [B,H,W] tensor, got %s %s" % (maps_u8.dtype, tuple(maps_u8.shape)))
    B, H, W = maps_u8.shape
    if maps_u8.stride(2) != 1 or maps_u8.stride(1) < W or (B > 1 and maps_u8.stride(0) < maps_u8.stride(1) * (H - 1) + W):
        maps_u8 = maps_u8.contiguous()
    key = (H, W, int(quality), B, maps_u8.device)
    plan = _JPEG_PLANS.get(key)
    if plan is None:
        cap = lib.mspi_jpeg_gray_bound(H, W)
        host = (C.c_ubyte * 512)()
        n = lib.mspi_jpeg_gray_header(H, W, int(quality), host, 512)
        check(min(n, 0), "mspi_jpeg_gray_header")
        d = _lib.JpegDesc()
        d.B, d.H, d.W, d.quality, d.file_stride, d.cap, d.header_len = B, H, W, int(quality), cap, cap, n
        for k in range(64):
            d.div[k] = 8 * host[25 + k]                  # the DQT payload: SOI 2 + APP0 18 + DQT marker, length, index 5
        header = torch.tensor(list(host[:n]), dtype=torch.uint8).to(maps_u8.device)
        ws = torch.empty(lib.mspi_jpeg_gray_ws_bytes(B, H, W), dtype=torch.uint8, device=maps_u8.device)
        d.header = header.data_ptr()
        plan = _JPEG_PLANS[key] = (d, header, ws, cap)
    d, header, ws, cap = plan
    d.pitch, d.map_stride = maps_u8.stride(1), maps_u8.stride(0)
    files = torch.empty(B, cap, dtype=torch.uint8, device=maps_u8.device)
    lengths = torch.empty(B, dtype=torch.int32, device=maps_u8.device)
    check(lib.mspi_jpeg_gray_fwd(C.byref(d), maps_u8.data_ptr(), files.data_ptr(), lengths.data_ptr(), ws.data_ptr(), _stream()),
          "mspi_jpeg_gray_fwd")
    return files, lengths


# ----------------------------------------------------------------------------- JPEG frame decoding (csrc/jpegdec.hip)
_JPEG_DEC = {}      # per device: pinned staging buffer + the event of its last upload, device input buffer, workspace


def jpeg_probe(data):
    """The parsed header (a _lib.JpegDecInfo: H, W, ncomp, hs, vs, scan_off, scan_len, tables) of a JPEG file given as bytes,
    or None where the device decoder does not take it (progressive, restart markers, CMYK, ...: `_lib.load().mspi_last_error()`
    says which) -- the caller then decodes that file on the host.  Host only."""
    lib = _lib.load()
    info = _lib.JpegDecInfo()
    if lib.mspi_jpeg_dec_parse(C.cast(C.c_char_p(bytes(data)), C.c_void_p), len(data), C.byref(info)) != 0:
        return None
    return info


def jpeg_subseq_bits(scan_bytes):
    """Bits per subsequence for scans of up to `scan_bytes` bytes: at most 1024 subsequences, none shorter than 1024 bits."""
    return max(1024, (-(-8 * scan_bytes // 1024) + 31) // 32 * 32)


def _grown(slot, key, nbytes, make):
    buf = slot.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = slot[key] = make(max(nbytes, 0 if buf is None else 2 * buf.numel()))
    return buf


def jpeg_decode_rgb(files, subseq_bits=None, device=None, infos=None):
    """files: a list of N `bytes`, baseline JPEG files of ONE geometry (size, components, sampling) -> (rgb uint8 [N,H,W,3],
    status int32 [N], passes int32 [N]), all on the GPU: rgb[i] is np.asarray(PIL.Image.open(files[i]).convert("RGB")) pixel
    for pixel wherever status[i] == 0 (inference.py:154-165 decodes with PIL); a non-zero status marks a truncated or corrupt
    scan, whose pixels the caller replaces.  Only the scans and tables are uploaded: they are packed into one pinned staging
    buffer that is reused from call to call (the call waits for the previous upload from it) and go up in one copy on the
    current stream; the staging, input and workspace buffers are cached per device, so calls must be ordered on one stream.
    Raises MspiError for mixed geometry and for a file the parser refuses (`jpeg_probe` tells in advance)."""
    lib = _lib.load()
    if not files:
        raise MspiError("jpeg_decode_rgb: no files")
    if infos is None:
        infos = [jpeg_probe(f) for f in files]
    for k, info in enumerate(infos):
        if info is None:
            jpeg_probe(files[k])
            raise MspiError("jpeg_decode_rgb: file %d: %s" % (k, lib.mspi_last_error().decode("utf-8", "replace")))
    geo = lambda i: (i.H, i.W, i.ncomp, i.hs, i.vs)      # noqa: E731
    if any(geo(i) != geo(infos[0]) for i in infos):
        raise MspiError("jpeg_decode_rgb: mixed geometry in one batch: %s" % sorted({geo(i) for i in infos}))
    if device is None and not torch.cuda.is_available():
        raise MspiError("jpeg_decode_rgb: needs an MI355X; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise MspiError("jpeg_decode_rgb: runs on the GPU only (device %s)" % dev)
    N, first = len(files), infos[0]
    cap = (max(i.scan_len for i in infos) + 15) // 16 * 16
    tsz = C.sizeof(_lib.JpegDecTables)
    total = N * (tsz + cap)
    d = _lib.JpegDecDesc()
    d.B, d.H, d.W, d.ncomp, d.hs, d.vs = N, first.H, first.W, first.ncomp, first.hs, first.vs
    d.S = int(subseq_bits) if subseq_bits is not None else jpeg_subseq_bits(cap)
    d.scan_stride, d.scan_cap, d.pitch, d.img_stride = cap, cap, 3 * first.W, 3 * first.W * first.H
    need = lib.mspi_jpeg_dec_ws_bytes(C.byref(d))
    if need == 0:
        raise MspiError("jpeg_decode_rgb: %s" % lib.mspi_last_error().decode("utf-8", "replace"))
    slot = _JPEG_DEC.setdefault(dev, {})
    stage = _grown(slot, "stage", total, lambda n: torch.empty(n, dtype=torch.uint8).pin_memory())
    if slot.get("uploaded") is not None:
        slot["uploaded"].synchronize()               # the previous call's copy out of the staging buffer
    host = stage.numpy()
    for k, (f, info) in enumerate(zip(files, infos)):
        host[k * tsz:(k + 1) * tsz] = np.frombuffer(C.string_at(C.addressof(info.tables), tsz), dtype=np.uint8)
        host[N * tsz + k * cap:N * tsz + k * cap + info.scan_len] = np.frombuffer(f, dtype=np.uint8, count=info.scan_len,
                                                                                  offset=info.scan_off)
    inp = _grown(slot, "input", total, lambda n: torch.empty(n, dtype=torch.uint8, device=dev))
    ws = _grown(slot, "ws", need, lambda n: torch.empty(n, dtype=torch.uint8, device=dev))
    with torch.cuda.device(dev):
        inp[:total].copy_(stage[:total], non_blocking=True)
        slot["uploaded"] = torch.cuda.Event()
        slot["uploaded"].record()
        rgb = torch.empty(N, first.H, first.W, 3, dtype=torch.uint8, device=dev)
        status = torch.empty(N, dtype=torch.int32, device=dev)
        passes = torch.empty(N, dtype=torch.int32, device=dev)
        check(lib.mspi_jpeg_dec_fwd(C.byref(d), inp.data_ptr() + N * tsz, inp.data_ptr(), rgb.data_ptr(), status.data_ptr(),
                                    passes.data_ptr(), ws.data_ptr(), _stream()), "mspi_jpeg_dec_fwd")
    return rgb, status, passes
