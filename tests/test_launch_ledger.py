"""Ledger of how every entry point of libmspi_hip.so launches.

The contract (include/mspi_hip.h, first comment block; DESIGN.md section 3 "Capture rules"): kernels are stateless and
re-entrant; launches go to the caller's stream and return immediately; no synchronisation, allocation or memcpy inside, on the
first call of a process as on any other, on any device; host arrays and descriptors are read during the call, and a captured
graph holds its own copy.  bench.py and inference.py --graph never launch eagerly, so this is what the production path rests on.

CPU: every name of _lib.EXPORTS is a key of LAUNCH_LEDGER (it launches) or of LAUNCH_EXCLUDED (a host-only query); a ledger
value is a row of this file or the name of an existing capture test that replays the entry point with NEW input values (its
existence and gpu mark are asserted); a scan of csrc/ finds no runtime call other than a launch outside a pinned allow-list
and no mutable function-local static, and is shown to report both on the lines of the old mspi_postprocess_u8.

GPU, one row per distinct launch, on the smallest row of the kernel's own ledger (the rows of test_nonfinite_ledger.py where
their run() is capturable once operands and packs are on the device; rows of this file where it packs weights, copies from
the host, synchronises or writes in place).  Static device operands, two input sets A and B:
  1. eager on A and on B -> want_A, want_B (they differ: asserted);
  2. A in the static operands; the launch, INCLUDING the engine wrapper's workspace allocation, is captured with
     torch.cuda.graph on a non-default stream in the default (global) capture-error mode;
  3. every output is filled with a sentinel;
  4. B is written into the static operands, replay: outputs == want_B;
  5. A is written, two replays: outputs == want_A after each.
All comparisons are bitwise (the entry points are documented bitwise repeatable, and a replay runs the same kernels on the
same data).  A launch that went to another stream is not in the graph: the sentinel survives.  A value baked in at capture
gives want_A where want_B is due.  Scratch that does not survive gives garbage on the second replay.  The status word stays 0.
Host-argument rows add one step: after the capture and before the first replay, the host buffers the call read (weights of
the fused stem, the arrays of mspi_upsample_sum_fwd, seg_host, mean / std, ctypes descriptors) are overwritten and dropped.

Preparation is split from launch by a DRY pass: the row's launch runs once with the library's launching entry points replaced
by stubs and the engine's pack_* functions recorded; the later passes get the recorded packs back.  So weights are packed and
the Python wrappers' own caches (resize coefficient tables, the JPEG header plan) are filled without one call of the entry
point -- which the cold-capture child needs: one fresh process in which, for each row, the capture is the first call of that
entry point, with no eager warm-up.  mspi_postprocess_u8 is the row it exists for; any future lazy initialisation fails it.

Second device (skipped with fewer than two GPUs): postprocess_u8, an f16x3 conv (the status word is pinned host memory) and
jpeg_encode_gray under torch.cuda.device(1) are bit-equal to device 0, and engine._need_gpu refuses a tensor that is not on
the current device before anything is launched."""
import contextlib
import copy
import ctypes as C
import io
import json
import math
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and ROOT not in sys.path:      # the cold-capture child is this file run as a script
    sys.path.insert(0, ROOT)

import test_gemm_ledger as GL          # noqa: E402
import test_kernel_ledger as KL        # noqa: E402
import test_nonfinite_ledger as NF     # noqa: E402
import test_rowop_ledger as RL         # noqa: E402
from test_kernel_ledger import _guard  # noqa: E402

SENTINEL = NF.SENTINEL
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# ------------------------------------------------------------------------------------------------------------ the two lists
_CITED = {      # existing capture tests that replay the entry point on input values it was not captured with
    "mspi_clip_resize_norm_fwd": "test_clip_loader.py::test_assemble_clips_in_a_captured_graph",
    "mspi_saliency_loss_fwd": "test_sal_loss_grad.py::test_hip_forward_and_backward_inside_graph_capture",
    "mspi_saliency_loss_bwd": "test_sal_loss_grad.py::test_hip_forward_and_backward_inside_graph_capture",
}
# test_evaluate.py::test_hip_resizes_inside_graph_capture and test_saliency_auc.py::test_hip_launches_inside_graph_capture replay
# the capture-time inputs only: the two resizes and the four metric kernels have rows here.

# entry point -> the rows of this file (what they cover), or "<file>::<test>" of a cited capture test
LAUNCH_LEDGER = {
    "mspi_conv_fwd": "register fp32 / f16x3 (descriptor overwritten), LDS-DMA 128 / 256 rows, gated",
    "mspi_conv_splitk_fwd": "two launches: slices into the workspace, then the reduction",
    "mspi_conv_halo_fwd": "halo-staged 3x3x3",
    "mspi_rowgemm_fwd": "thin GEMM, gated",
    "mspi_gemm_sp_fwd": "planes in, rows out and planes out",
    "mspi_mlp_fwd": "with and without the fused LayerNorm",
    "mspi_x3d_ab_fwd": "Swish and pooled",
    "mspi_x3d_ab_s2_fwd": "Swish and pooled",
    "mspi_x3d_ca_fwd": "with and without the gate",
    "mspi_x3d_stem_fwd": "host row: wxy, wt, bias overwritten after the capture",
    "mspi_dwconv_fwd": "LDS (descriptor overwritten), tile, strip, generic; ReLU, Swish, pooled",
    "mspi_maxpool_fwd": "two kernels",
    "mspi_se_gate": "both kernels",
    "mspi_layernorm_fwd": "C 64 / 96, act none / ReLU",
    "mspi_layernorm_sp_fwd": "planes out",
    "mspi_split_planes_fwd": "round trip, and in front of mspi_gemm_sp_fwd",
    "mspi_join_planes_fwd": "round trip",
    "mspi_attn_fwd": "fp32 and f16x3; descriptor overwritten",
    "mspi_attn_fwd_ws": "planes, pipeline, key split + merge (two and three launches through the workspace); descriptor overwritten",
    "mspi_mvit_qk_augment": "q, k, tables",
    "mspi_mvit_qk_augment_p": "q, k, P",
    "mspi_upsample_fwd": "factors 2 / 4 / 8, accumulate, ReLU",
    "mspi_upsample_sum_fwd": "J = 2; host row J = 3: srcs / lds / factors overwritten after the capture",
    "mspi_rowgate": "x, mask",
    "mspi_space_to_depth": "x",
    "mspi_permute_fwd": "vector and scalar kernels",
    "mspi_gated_sum_fwd": "two sources",
    "mspi_add": "a, b",
    "mspi_mean_rows": "one launch",
    "mspi_mean_rows_ws": "two launches through the workspace",
    "mspi_neg_cosine": "store, then accumulate",
    "mspi_logsumexp_sub": "in place on a copy made inside the capture",
    "mspi_postprocess_u8": "four launches through the workspace; the cold-capture row",
    "mspi_logsumexp_sub_bwd": "g, logp",
    "mspi_conv_c1_bwd": "launches through the workspace",
    "mspi_upsample_bwd": "factors 2 / 4 / 8",
    "mspi_conv_wgrad_fwd": "slices into the workspace, then the reduction",
    "mspi_conv_wgrad_wide_fwd": "slices into the workspace, then the reduction",
    "mspi_bn_stats": "records into the workspace, then the merge",
    "mspi_bn_apply": "ReLU",
    "mspi_bn_bwd": "records into the workspace, then the merge, then dx",
    "mspi_logspec_fwd": "host row: seg_host overwritten after the capture",
    "mspi_resize_norm_fwd": "host row: mean3 / std3 overwritten after the capture; two launches through tmp",
    "mspi_resize_bilinear_fwd": "float32 and uint8 maps",
    "mspi_resize_fixation_fwd": "binary maps",
    "mspi_saliency_metrics": "log map, density, fixations",
    "mspi_saliency_auc_judd": "float32 and float64 (jittered) maps: three launches through the workspace",
    "mspi_saliency_sauc_counts": "map, fixations, other fixations",
    "mspi_saliency_ig": "map, density, baseline",
    "mspi_jpeg_gray_fwd": "launches through the workspace; compared up to each file's length",
    "mspi_jpeg_dec_fwd": "memset + five launches through the workspace",
}
LAUNCH_LEDGER.update(_CITED)

# the host-only queries: what the non-finite ledger tags _HOST, and the registration of the status word
LAUNCH_EXCLUDED = {n for n, why in NF.NONFINITE_EXCLUDED.items() if why == NF._HOST} | {"mspi_set_status_word"}


# -------------------------------------------------------------------------------------------------------------- the harness
class Row:
    """One launch (or a short chain) of an entry point.  make(which) -> CPU operands of input set "A" / "B" (tensors become
    the static device operands; anything else is passed through); launch(E, dev, t, host) -> {name: output}, capturable once
    the dry pass has run; it appends to `host` every host buffer it handed to the library (a host-argument row).
    scribble: the ctypes arrays and descriptors the engine wrapper passed are overwritten after the capture as well.
    post(outs) -> the part of the outputs that is defined (the JPEG files up to their lengths)."""

    def __init__(self, name, entries, make, launch, shape=None, scribble=False, post=None):
        self.name, self.entries = name, (entries,) if isinstance(entries, str) else tuple(entries)
        self.make, self.launch, self.scribble, self.post = make, launch, scribble, post
        self._shape = shape

    def shape(self):
        if self._shape:
            return self._shape
        t = self.make("A")
        return " ".join("%s[%s]" % (k, ",".join(str(n) for n in v.shape)) for k, v in t.items() if torch.is_tensor(v))[:120]


ROWS = []


def _row(*a, **k):
    ROWS.append(Row(*a, **k))


@contextlib.contextmanager
def _tap(lib, stub):
    """Every launching entry point of `lib` behind a recorder; stub: the call is not made (the dry pass)."""
    saved = {n: getattr(lib, n) for n in LAUNCH_LEDGER}
    calls = []

    def wrap(name, fn):
        def call(*a):
            calls.append((name, a))
            return 0 if stub else fn(*a)
        return call
    for n, fn in saved.items():
        setattr(lib, n, wrap(n, fn))
    try:
        yield calls
    finally:
        for n, fn in saved.items():
            setattr(lib, n, fn)


@contextlib.contextmanager
def _packs(E, memo, record):
    """engine.pack_*: recorded in call order in the dry pass (device tensors go back to the host first, as a module's
    parameters would), handed back in the same order afterwards -- no packing, no upload inside a capture."""
    names = [n for n in dir(E) if n.startswith("pack_") and callable(getattr(E, n))]
    saved = {n: getattr(E, n) for n in names}
    at = [0]

    def wrap(fn):
        def call(*a, **k):
            i = at[0]
            at[0] += 1
            if record:
                a = [x.cpu() if torch.is_tensor(x) and x.is_cuda else x for x in a]
                memo.append(fn(*a, **k))
            return memo[i]
        return call
    for n, fn in saved.items():
        setattr(E, n, wrap(fn))
    try:
        yield
    finally:
        for n, fn in saved.items():
            setattr(E, n, fn)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))


def _fill(t):
    t.fill_(SENTINEL if t.is_floating_point() else (0xA5 if t.dtype == torch.uint8 else -777))


def _scribble(objs):
    """Overwrite host buffers the library was handed: CPU tensors, numpy arrays, ctypes arrays and structures."""
    for o in objs:
        if torch.is_tensor(o):
            assert not o.is_cuda
            o.fill_(float("nan") if o.is_floating_point() else 0x5A)
        elif isinstance(o, np.ndarray):
            o.fill(0x5A5A5A5A if o.dtype.itemsize >= 4 else 0x5A)
        else:
            C.memset(C.addressof(o), 0xA5, C.sizeof(o))


def _ctypes_args(calls):
    out = []
    for _, args in calls:
        for a in args:
            if isinstance(a, (C.Array, C.Structure)):
                out.append(a)
            elif hasattr(a, "_obj") and isinstance(a._obj, (C.Array, C.Structure)):      # C.byref(descriptor)
                out.append(a._obj)
    return out


class _Run:
    """A row on a device: the static operands, the recorded packs, and the passes over the row's launch."""

    def __init__(self, row, E, dev):
        self.row, self.E, self.dev, self.lib = row, E, dev, E._lib.load()
        self.sets = {w: row.make(w) for w in ("A", "B")}
        self.t = {k: (v.to(dev).clone() if torch.is_tensor(v) else v) for k, v in self.sets["A"].items()}
        self.memo = []
        with _tap(self.lib, stub=True) as calls, _packs(E, self.memo, record=True):
            row.launch(E, dev, self.t, [])
        assert {n for n, _ in calls} >= set(row.entries) - set(_CITED), \
            "%s: the launch never calls %s" % (row.name, sorted(set(row.entries) - {n for n, _ in calls}))
        torch.cuda.synchronize()

    def load(self, which):
        for k, v in self.sets[which].items():
            if torch.is_tensor(v):
                self.t[k].copy_(v)

    def launch(self, host=None):
        with _packs(self.E, self.memo, record=False):
            return self.row.launch(self.E, self.dev, self.t, [] if host is None else host)

    def capture(self, host):
        side = torch.cuda.Stream(self.dev)
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with _tap(self.lib, stub=False) as calls:
            with torch.cuda.graph(graph, stream=side):      # capture_error_mode: the default, "global"
                outs = self.launch(host)
        if self.row.scribble:
            host.extend(_ctypes_args(calls))
        return graph, outs

    def read(self, outs):
        torch.cuda.synchronize()
        assert not self.E.range_flag(), "%s: the status word went up on finite data" % self.row.name
        outs = {k: v.detach().clone() for k, v in outs.items()}
        return self.row.post(outs) if self.row.post else outs


def _equal(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, "%s %s: %s %s, eager %s %s" % (
            what, k, got[k].dtype, tuple(got[k].shape), want[k].dtype, tuple(want[k].shape))
        if not _bits_equal(got[k], want[k]):
            g, w = got[k].double(), want[k].double()
            left = int((g == (SENTINEL if got[k].is_floating_point() else (0xA5 if got[k].dtype == torch.uint8 else -777))).sum())
            raise AssertionError("%s: output %s differs from the eager launch in %d of %d elements (max |d| %.3e; %d still hold the "
                                 "sentinel)" % (what, k, int((g != w).sum()), g.numel(), (g - w).abs().nan_to_num(float("inf")).max().item(), left))


# ---------------------------------------------------------------------------------------- rows: the non-finite ledger's cases
# Their run() is capturable when `t` already holds device tensors (`.to(dev)` is then the tensor itself) and pack_* is
# recorded: what is left are launches, torch fills and device-to-device copies.  Not taken: the fused stem (host weights), the
# attention rows (KL._attn_direct synchronises), mvit_qk_augment_p (a float64 GEMM for P inside run()), logsumexp_sub (writes
# its operand in place) and the criterion (cited); they have rows of their own below.
_OWN = ("x3d_stem", "attn-", "mvit_aug_p", "logsumexp_sub-", "saliency_loss")
_SCRIBBLED = {"conv-reg-f16x3-x", "dwconv-1717-relu-x"}      # the conv and the dwconv descriptor rows


def _permuted(t, seed):
    """Input set B of a non-finite case: every float tensor's elements in a seeded random order (the value distribution --
    positive gates, post-ReLU activations, log-probabilities -- stays what the case made it)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in t.items():
        if torch.is_tensor(v) and v.is_floating_point() and v.numel() > 1:
            out[k] = v.reshape(-1)[torch.randperm(v.numel(), generator=g)].view(v.shape).contiguous()
        else:
            out[k] = v
    return out


def _nonfinite_rows():
    seen = set()
    for c in NF.CASES:
        if id(c.run) in seen or c.name.startswith(_OWN) or (c.name.startswith("logsumexp_sub_bwd") and "logsumexp_sub_bwd" in seen):
            continue
        seen.add(id(c.run))
        if c.name.startswith("logsumexp_sub_bwd"):
            seen.add("logsumexp_sub_bwd")

        def make(which, c=c):
            t = c.make()
            return t if which == "A" else _permuted(t, len(c.name) + 1000)

        _row(c.name, c.entries, make, lambda E, dev, t, host, c=c: c.run(E, dev, t), scribble=c.name in _SCRIBBLED)


_nonfinite_rows()


# --------------------------------------------------------------------------------------------------- rows: host arguments
def _stem_rows():
    N, T, H, W = 2, 6, 28, 28      # the non-finite ledger's stem shape
    g = torch.Generator().manual_seed(T + H + W)
    wxy = torch.randn(24, 3, 1, 3, 3, generator=g) / math.sqrt(27)
    wt = torch.randn(24, 1, 5, 1, 1, generator=g) / math.sqrt(5)
    b = torch.rand(24, generator=g) * 0.4 - 0.2

    def make(which):
        return dict(x=torch.randn(N, 3, T, H, W, generator=torch.Generator().manual_seed(10 + (which == "B"))))

    def launch(E, dev, t, host):
        pk = copy.copy(E.pack_x3d_stem(wxy, wt, None))      # fresh host arrays for this call: they travel as kernel arguments
        pk.wxy, pk.wt, pk.bias = pk.wxy.clone(), pk.wt.clone(), b.clone()
        host.extend([pk.wxy, pk.wt, pk.bias])
        out = NF._sentinel(E, N, T, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 24, dev)
        return {"y": E.x3d_stem(t["x"], pk, out=out).as_ncdhw(24)}

    _row("x3d_stem-host-weights", "mspi_x3d_stem_fwd", make, launch, scribble=True)


def _upsample_sum_rows():
    NT, Ho, Wo, Cc = 2, 8, 16, 24

    def make(which):
        g = torch.Generator().manual_seed(816 + (which == "B"))
        return dict(s0=torch.randn(NT, Cc, 1, Ho // 2, Wo // 2, generator=g), s1=torch.randn(NT, Cc, 1, Ho // 4, Wo // 4, generator=g),
                    s2=torch.randn(NT, Cc, 1, Ho // 8, Wo // 8, generator=g), base=torch.randn(NT, Cc, 1, Ho, Wo, generator=g))

    def launch(E, dev, t, host):
        dst = NF._cl(E, t["base"], dev)
        E.upsample_sum(dst, [(NF._cl(E, t["s0"], dev), 2), (NF._cl(E, t["s1"], dev), 4), (NF._cl(E, t["s2"], dev), 8)], accumulate=True,
                       act=NF.RELU)
        return {"y": dst.as_ncdhw()}

    _row("upsample_sum-J3-host-arrays", "mspi_upsample_sum_fwd", make, launch, scribble=True)


def _logspec_rows():
    import logspec_restate as LS
    Wa = LS.WAS[1]
    segs = [w for i, w in enumerate(LS.WINDOWS) if i not in LS.SILENT_WINDOWS][:5]

    def make(which):
        wave = LS.make_wave().clone()
        return dict(wave=wave if which == "A" else wave.flip(0).contiguous(), seg=torch.tensor(segs, dtype=torch.int32),
                    window=torch.hann_window(512, dtype=torch.float32))

    def launch(E, dev, t, host):
        seg_host = np.ascontiguousarray(np.asarray(segs, dtype=np.int32).reshape(-1, 3))
        host.append(seg_host)
        out = torch.full((len(segs), 1, 257, Wa), SENTINEL, device=dev)
        E.check(E._lib.load().mspi_logspec_fwd(t["wave"].data_ptr(), t["wave"].numel(), t["seg"].data_ptr(), seg_host.ctypes.data, len(segs),
                                               t["window"].data_ptr(), out.data_ptr(), Wa, E._stream()), "mspi_logspec_fwd")
        return {"y": out}

    _row("logspec-host-seg", "mspi_logspec_fwd", make, launch, shape="wave%d windows%d Wa%d" % (LS.N_WAVE, len(segs), Wa))


def _attn_rows():
    pair = 128 * 10000 + 96 * 10      # the non-finite ledger's rows: the (128, 96) pair in every form
    kinds = {"f32": 10000000 + pair, "f16x3": 20000000 + pair, "planes": 30000000 + pair, "pipe": 50000000 + pair, "merge": 50000000 + pair + 1}
    for kind, code in kinds.items():
        row = KL.ATTN_LEDGER[code]
        B, Hh, Nq, Nk, D, Dv, prec, bias, mask, tok, ws, res = row

        def make(which, row=row, code=code):
            t, _ = KL._attn_inputs(row, code % 100003 + (which == "B"))
            return t

        def launch(E, dev, t, host, row=row, code=code):
            """KL._attn_direct without its synchronise; the descriptor is a fresh host structure per call."""
            B, Hh, Nq, Nk, D, Dv, prec, bias, mask, tok, ws, res = row
            lib = E._lib.load()
            S, _, Rq, _ = t["q"].shape
            Rk = t["k"].shape[2]
            o = torch.full((S, Hh, Rq, Dv), SENTINEL, device=dev)
            d = KL._attn_desc(B, Hh, Nq, Nk, D, Dv, prec)
            d.nmask = t["nmask"] if mask else 0
            d.nwin = t["nwin"] if tok else 0
            d.q_sB, d.q_sH, d.q_sT = Hh * Rq * D, Rq * D, D
            d.k_sB, d.k_sH, d.k_sT = Hh * Rk * D, Rk * D, D
            d.v_sB, d.v_sH, d.v_sT = Hh * Rk * Dv, Rk * Dv, Dv
            d.o_sB, d.o_sH, d.o_sT = Hh * Rq * Dv, Rq * Dv, Dv
            d.scale = t["scale"]
            host.append(d)
            ptrs = [t[n].data_ptr() if t[n] is not None else None for n in ("res", "biasT", "maskT", "tok")]
            assert lib.mspi_attn_variant(C.byref(d), bias, mask, tok, ws) == code
            if ws:
                wsb = torch.empty(lib.mspi_attn_ws_bytes(C.byref(d)), dtype=torch.uint8, device=dev)
                E.check(lib.mspi_attn_fwd_ws(C.byref(d), t["q"].data_ptr(), t["k"].data_ptr(), t["v"].data_ptr(), *ptrs, o.data_ptr(),
                                             wsb.data_ptr(), E._stream()), "mspi_attn_fwd_ws")
            else:
                E.check(lib.mspi_attn_fwd(C.byref(d), t["q"].data_ptr(), t["k"].data_ptr(), t["v"].data_ptr(), *ptrs, o.data_ptr(),
                                          E._stream()), "mspi_attn_fwd")
            return {"o": o}

        _row("attn-%s" % kind, "mspi_attn_fwd_ws" if ws else "mspi_attn_fwd", make, launch)

    case = RL.AUG_CASES[0]
    da, k_thw = case
    Dh, heads, B = RL.AUG_DH, RL.AUG_HEADS, RL.AUG_B
    nq, nk = math.prod(RL.AUG_Q), math.prod(k_thw)
    ncol = sum(q * k for q, k in zip((RL.AUG_Q[1], RL.AUG_Q[2], RL.AUG_Q[0]), (k_thw[1], k_thw[2], k_thw[0])))
    ldp = (ncol + 3) // 4 * 4

    def make_p(which):
        q, k = RL._aug_inputs(case)[:2]
        g = torch.Generator().manual_seed(da + (which == "B"))
        if which == "B":
            q, k = q.flip(0).contiguous(), k.flip(1).contiguous()
        nh, nw = RL.AUG_Q[1] * k_thw[1], RL.AUG_Q[2] * k_thw[2]
        where = torch.arange(ncol, dtype=torch.int32)
        # P stands for q x every table row: the kernel only reads it, so it is an operand like any other here
        return dict(q=q.reshape(B * nq, heads * Dh), k=k.reshape(B * nk, heads * Dh), P=torch.randn(B * nq * heads, ldp, generator=g),
                    ih=where[:nh].view(RL.AUG_Q[1], k_thw[1]).contiguous(), iw=where[nh:nh + nw].view(RL.AUG_Q[2], k_thw[2]).contiguous(),
                    it=where[nh + nw:].view(RL.AUG_Q[0], k_thw[0]).contiguous())

    def launch_p(E, dev, t, host):
        qa = torch.full((B, heads, nq, da), SENTINEL, device=dev)
        ka = torch.full((B, heads, nk, da), SENTINEL, device=dev)
        a = RL._aug_desc(da, k_thw, heads * Dh, heads * Dh)
        host.append(a)
        E.check(E._lib.load().mspi_mvit_qk_augment_p(C.byref(a), t["q"].data_ptr(), t["k"].data_ptr(), t["P"].data_ptr(), ldp,
                                                     t["ih"].data_ptr(), t["iw"].data_ptr(), t["it"].data_ptr(), qa.data_ptr(), ka.data_ptr(),
                                                     E._stream()), "mspi_mvit_qk_augment_p")
        return {"qa": qa, "ka": ka}

    _row("mvit_aug_p", "mspi_mvit_qk_augment_p", make_p, launch_p)


def _small_rows():
    lse = RL.LSE_CASES[2]

    def make_lse(which):
        x = RL._lse_inputs(lse)
        return dict(x=x if which == "A" else x.flip(1).contiguous())

    def launch_lse(E, dev, t, host):
        buf = t["x"].clone().reshape(-1)      # the kernel writes in place: the copy is part of the captured work
        E.logsumexp_sub(buf, *lse)
        return {"y": buf.view(*lse)}

    _row("logsumexp_sub", "mspi_logsumexp_sub", make_lse, launch_lse)


# ----------------------------------------------------------------------------------- rows: integer paths and the metrics
def _integer_rows():
    Hin, Win, Hout, Wout = 48, 64, 32, 48

    def make_rgb(which):
        rng = np.random.default_rng(5 + (which == "B"))
        return dict(rgb=torch.from_numpy(rng.integers(0, 256, (Hin, Win, 3), dtype=np.uint8)))

    def launch_rn(E, dev, t, host):
        from mspi_amd import preproc as P
        out = torch.full((3, Hout, Wout), SENTINEL, device=dev)
        return {"y": P.resize_normalize(t["rgb"], (Hout, Wout), MEAN, STD, out=out)}

    _row("resize_norm-host-mean-std", "mspi_resize_norm_fwd", make_rgb, launch_rn, scribble=True)

    def make_maps(which):
        rng = np.random.default_rng(2 + (which == "B"))
        return dict(x=torch.from_numpy(rng.standard_normal((2, 24, 40)).astype(np.float32)),
                    u=torch.from_numpy(rng.integers(0, 256, (2, 31, 53), dtype=np.uint8)),
                    f=torch.from_numpy((rng.random((2, 31, 53)) < 0.02).astype(np.float32)))

    def launch_rs(E, dev, t, host):
        from mspi_amd import evaluate as EV
        return {"up": EV.resize_maps(t["x"], (31, 53)), "down": EV.resize_maps(t["u"], (24, 40)), "fix": EV.resize_fixations(t["f"], (24, 40))}

    _row("eval-resizes", ("mspi_resize_bilinear_fwd", "mspi_resize_fixation_fwd"), make_maps, launch_rs)

    def make_u8(which):
        rng = np.random.default_rng(95 + (which == "B"))
        yy, xx = np.mgrid[0:33, 0:47]
        smooth = 127 + 100 * np.sin(yy / 5.0 + (which == "B")) * np.cos(xx / 7.0)
        return dict(maps=torch.from_numpy(np.clip(smooth[None] + rng.normal(0, 6, (2, 33, 47)), 0, 255).astype(np.uint8)))

    def launch_je(E, dev, t, host):
        files, lengths = E.jpeg_encode_gray(t["maps"], quality=95)
        return {"files": files, "lengths": lengths}

    def post_je(outs):      # the bytes behind a file's end are never written
        cap = outs["files"].shape[1]
        keep = torch.arange(cap, device=outs["files"].device)[None] < outs["lengths"][:, None]
        return {"files": torch.where(keep, outs["files"], torch.zeros_like(outs["files"])), "lengths": outs["lengths"]}

    _row("jpeg_gray", "mspi_jpeg_gray_fwd", make_u8, launch_je, post=post_je)

    def _jpeg_files():
        from PIL import Image
        rng = np.random.default_rng(48)
        yy, xx = np.mgrid[0:48, 0:64]
        files = []
        for i in range(2):
            img = np.stack([127 + 90 * np.sin(yy / (4.0 + i) + c) * np.cos(xx / (6.0 + c)) for c in range(3)], -1) + rng.normal(0, 8, (48, 64, 3))
            buf = io.BytesIO()
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=75, subsampling=2)
            files.append(buf.getvalue())
        return files

    state = {}

    def _dec_setup(E):
        """engine.jpeg_decode_rgb's descriptor and input packing (its staging copy from pinned memory is the caller's side of
        the entry point); sets A and B are the same two files in either order, so one descriptor serves both."""
        if not state:
            from mspi_amd import _lib as L
            files = _jpeg_files()
            infos = [E.jpeg_probe(f) for f in files]
            assert all(i is not None for i in infos)
            first, n = infos[0], len(files)
            cap = (max(i.scan_len for i in infos) + 15) // 16 * 16
            tsz = C.sizeof(L.JpegDecTables)

            def pack(order):
                host = np.zeros(n * (tsz + cap), dtype=np.uint8)
                for k, j in enumerate(order):
                    f, info = files[j], infos[j]
                    host[k * tsz:(k + 1) * tsz] = np.frombuffer(C.string_at(C.addressof(info.tables), tsz), dtype=np.uint8)
                    host[n * tsz + k * cap:n * tsz + k * cap + info.scan_len] = np.frombuffer(f, dtype=np.uint8, count=info.scan_len,
                                                                                            offset=info.scan_off)
                return torch.from_numpy(host)
            geo = dict(B=n, H=first.H, W=first.W, ncomp=first.ncomp, hs=first.hs, vs=first.vs, S=E.jpeg_subseq_bits(cap), scan_stride=cap,
                       scan_cap=cap, pitch=3 * first.W, img_stride=3 * first.W * first.H)
            state.update(A=pack((0, 1)), B=pack((1, 0)), geo=geo, tsz=tsz, n=n)
        return state

    def make_dec(which):
        from mspi_amd import engine as E
        return dict(inp=_dec_setup(E)[which])

    def launch_dec(E, dev, t, host):
        from mspi_amd import _lib as L
        lib, st = E._lib.load(), _dec_setup(E)
        d = L.JpegDecDesc()
        for k, v in st["geo"].items():
            setattr(d, k, v)
        host.append(d)
        n, g = st["n"], st["geo"]
        ws = torch.empty(lib.mspi_jpeg_dec_ws_bytes(C.byref(d)), dtype=torch.uint8, device=dev)
        rgb = torch.full((n, g["H"], g["W"], 3), 0xA5, dtype=torch.uint8, device=dev)
        status = torch.full((n,), -777, dtype=torch.int32, device=dev)
        passes = torch.full((n,), -777, dtype=torch.int32, device=dev)
        E.check(lib.mspi_jpeg_dec_fwd(C.byref(d), t["inp"].data_ptr() + n * st["tsz"], t["inp"].data_ptr(), rgb.data_ptr(), status.data_ptr(),
                                      passes.data_ptr(), ws.data_ptr(), E._stream()), "mspi_jpeg_dec_fwd")
        return {"rgb": rgb, "status": status, "passes": passes}

    _row("jpeg_dec", "mspi_jpeg_dec_fwd", make_dec, launch_dec, shape="2 files 48x64 4:2:0")

    def make_eval(which):
        import test_saliency_auc as TA
        sal, fix, other, dens, base, noise = TA._seeded_batch(2, 40, 64, [30, 7], seed=5 + (which == "B"))
        t = {k: torch.from_numpy(v) for k, v in dict(sal=sal, fix=fix, other=other, dens=dens, base=base, noise=noise).items()}
        t["logmap"] = torch.log_softmax(t["sal"].flatten(1) * 3, 1).view_as(t["sal"])
        return t

    def launch_eval(E, dev, t, host):
        from mspi_amd import metrics as M
        return {"four": M.per_sample(t["logmap"], t["dens"], t["fix"], pred_is_log=True), "judd32": M.auc_judd_per_sample(t["sal"], t["fix"], jitter=False),
                "judd64": M.auc_judd_per_sample(t["sal"], t["fix"], jitter=t["noise"]), "sauc": M.sauc_counts(t["sal"], t["fix"], t["other"]),
                "ig": M.ig_per_sample(t["sal"], t["dens"], t["base"])}

    _row("eval-metrics", ("mspi_saliency_metrics", "mspi_saliency_auc_judd", "mspi_saliency_sauc_counts", "mspi_saliency_ig"), make_eval,
         launch_eval)


for _family in (_stem_rows, _upsample_sum_rows, _logspec_rows, _attn_rows, _small_rows, _integer_rows):
    _family()
BY_NAME = {r.name: r for r in ROWS}
HOST_ROWS = ("x3d_stem-host-weights", "upsample_sum-J3-host-arrays", "logspec-host-seg", "resize_norm-host-mean-std", "conv-reg-f16x3-x",
             "attn-f16x3", "dwconv-1717-relu-x")


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_every_entry_point_is_classified():
    from mspi_amd import _lib
    names = set(_lib.EXPORTS)
    both = set(LAUNCH_LEDGER) & LAUNCH_EXCLUDED
    assert not both, "classified twice: %s" % sorted(both)
    missing = names - set(LAUNCH_LEDGER) - LAUNCH_EXCLUDED
    assert not missing, "entry points without a launch classification (add a row, or it is a host-only query): %s" % sorted(missing)
    stale = (set(LAUNCH_LEDGER) | LAUNCH_EXCLUDED) - names
    assert not stale, "classified, but no entry point: %s" % sorted(stale)
    # every export that is no host-only query launches: the integer paths and the metric kernels are ledger keys
    assert {"mspi_jpeg_gray_fwd", "mspi_jpeg_dec_fwd", "mspi_resize_norm_fwd", "mspi_clip_resize_norm_fwd", "mspi_resize_fixation_fwd",
            "mspi_resize_bilinear_fwd", "mspi_saliency_metrics", "mspi_saliency_auc_judd", "mspi_saliency_sauc_counts",
            "mspi_saliency_ig"} <= set(LAUNCH_LEDGER)
    covered = {e for r in ROWS for e in r.entries}
    assert covered == set(LAUNCH_LEDGER) - set(_CITED), "ledger entries without a row / rows outside the ledger: %s" % sorted(
        covered ^ (set(LAUNCH_LEDGER) - set(_CITED)))
    assert len(BY_NAME) == len(ROWS), "two rows share a name"
    assert all(n in BY_NAME for n in HOST_ROWS)


def test_multi_launch_entry_points_have_rows_of_their_own():
    """The entry points whose workspace carries partial results between their launches: a row here, never a citation."""
    need = {"mspi_conv_splitk_fwd": ["conv-splitk-x"], "mspi_attn_fwd_ws": ["attn-planes", "attn-pipe", "attn-merge"],
            "mspi_mean_rows_ws": ["mean_rows-2-x"], "mspi_bn_stats": ["bn_stats-x"], "mspi_bn_apply": ["bn_apply-relu-x"],
            "mspi_bn_bwd": ["bn_bwd-dy"], "mspi_conv_wgrad_fwd": ["conv_wgrad-x"], "mspi_conv_wgrad_wide_fwd": ["conv_wgrad_wide-x"],
            "mspi_saliency_auc_judd": ["eval-metrics"], "mspi_jpeg_gray_fwd": ["jpeg_gray"], "mspi_jpeg_dec_fwd": ["jpeg_dec"]}
    for entry, rows in need.items():
        assert entry not in _CITED
        for name in rows:
            assert name in BY_NAME and entry in BY_NAME[name].entries, (entry, name)


@pytest.mark.parametrize("entry", sorted(_CITED))
def test_cited_capture_test_exists_and_runs_on_the_gpu(entry):
    """A rename of a cited test cannot silently drop the entry point's coverage."""
    import importlib
    module, name = _CITED[entry].split("::")
    assert module.endswith(".py")
    fn = getattr(importlib.import_module(module[:-3]), name, None)
    assert callable(fn), "%s cites %s, which does not exist" % (entry, _CITED[entry])
    marks = [m.name for m in getattr(fn, "pytestmark", [])] + [m.name for m in getattr(sys.modules[fn.__module__], "pytestmark", [])
                                                               if hasattr(m, "name")]
    assert "gpu" in marks, "%s is not marked gpu" % _CITED[entry]


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_row_input_sets_differ(name):
    """B is not A: 'a value baked in at capture gives want_A where want_B is due' needs two different wants."""
    row = BY_NAME[name]
    a, b = row.make("A"), row.make("B")
    assert set(a) == set(b)
    differ = 0
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
            differ += not torch.equal(a[k], b[k])
    assert differ > 0


# ---- the source scan
CSRC = os.path.join(ROOT, "mspi_amd", "csrc")
# runtime calls that queue work on the caller's stream or read an error code: what an entry point may do
_LAUNCH_CALLS = {"hipLaunchKernelGGL", "hipGetLastError", "hipPeekAtLastError", "hipGetErrorString"}
# every other runtime call, as (file, call): the device-count query (no launch, no stream) and the decoder's coefficient clear,
# which is the Async form on the caller's stream
SCAN_ALLOWED = {("capi.hip", "hipGetDeviceCount"), ("capi.hip", "hipGetDeviceProperties"), ("jpegdec.hip", "hipMemsetAsync")}
_NAMED = re.compile(r"^hip(Malloc\w*|Free\w*|HostMalloc|Memcpy\w*|\w*Synchronize|StreamCreate\w*|EventCreate\w*|Memset\w*)$")


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _scan(fname, text):
    """[(file, line, what)] of a source text: runtime calls that are neither a launch nor allow-listed for that file, and
    function-local statics that are not const / constexpr."""
    found = []
    for no, line in enumerate(_strip_comments(text).split("\n"), 1):
        for m in re.finditer(r"\b(hip[A-Z]\w*)\s*\(", line):
            call = m.group(1)
            if call in _LAUNCH_CALLS or (fname, call) in SCAN_ALLOWED:
                continue
            if call == "hipMemsetAsync" or not _NAMED.match(call):
                found.append((fname, no, "runtime call %s outside the allow-list" % call))
            else:
                found.append((fname, no, "forbidden runtime call %s" % call))
        m = re.match(r"^\s+static\s+(?!const\b|constexpr\b|inline\b|__device__|__host__|__global__|__forceinline__)", line)
        if m and "(" not in line.split("=")[0].split(";")[0]:      # indented: inside a function or a class; not a member function
            found.append((fname, no, "mutable function-local static: %s" % line.strip()))
    return found


def test_source_scan_of_csrc_is_clean():
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    assert len(files) >= 20 and "postproc.hip" in files and "common.h" in files
    found, seen = [], set()
    for f in files:
        with open(os.path.join(CSRC, f)) as fh:
            text = fh.read()
        found += _scan(f, text)
        seen |= {(f, c) for c in re.findall(r"\b(hip[A-Z]\w*)\s*\(", _strip_comments(text))}
    assert not found, "csrc/ breaks the capture rules:\n" + "\n".join("%s:%d: %s" % f for f in found)
    assert SCAN_ALLOWED <= seen, "allow-listed, but no longer in the source: %s" % sorted(SCAN_ALLOWED - seen)
    with open(os.path.join(CSRC, "postproc.hip")) as fh:
        assert "c_gauss11" not in fh.read()


_OLD_POSTPROC = """
extern "C" int mspi_postprocess_u8(const float* logmap, unsigned char* out, void* workspace, int32_t N, mspi_stream_t stream) {
  static bool init = false;
  if (!init) {   // cv2.getGaussianKernel(11, sigma = 2.0)
    float k[11];
    if (hipMemcpyToSymbol(HIP_SYMBOL(c_gauss11), k, sizeof(k)) != hipSuccess) {
      (void)hipGetLastError();
      return MSPI_ELAUNCH;
    }
    init = true;
  }
  static const int dbg = getenv("MSPI_DBG") ? 1 : 0;   /* a const environment read: allowed; hipMalloc( in a comment: ignored */
  hipLaunchKernelGGL(blur_exp_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logmap);
  return check_launch("mspi_postprocess_u8");
}
"""


def test_source_scan_bites_on_the_old_postprocess():
    """The two lines the scan exists for (the entry point as it was before it lost its state), and the other forbidden forms."""
    found = _scan("postproc.hip", _OLD_POSTPROC)
    what = [w for _, _, w in found]
    assert len(found) == 2, found
    assert any("hipMemcpyToSymbol" in w and "forbidden" in w for w in what) and any("static bool init" in w for w in what)
    assert [no for _, no, _ in found] == [3, 6]
    for call in ("hipMalloc(&p, 4)", "hipMallocAsync(&p, 4, s)", "hipFree(p)", "hipHostMalloc(&p, 4)", "hipMemcpy(a, b, 4, k)",
                 "hipMemcpyAsync(a, b, 4, k, s)", "hipDeviceSynchronize()", "hipStreamSynchronize(s)", "hipEventSynchronize(e)",
                 "hipStreamCreate(&s)", "hipStreamCreateWithFlags(&s, 0)", "hipEventCreate(&e)", "hipEventCreateWithFlags(&e, 0)",
                 "hipMemset(p, 0, 4)", "hipMemsetAsync(p, 0, 4, s)", "hipSetDevice(0)"):
        assert len(_scan("rowops.hip", "void f() {\n  %s;\n}\n" % call)) == 1, call
    assert _scan("jpegdec.hip", "  if (hipMemsetAsync(w, 0, n, s) != hipSuccess) return -1;\n") == []
    assert len(_scan("jpegdec.hip", "  hipMemset(w, 0, n);\n")) == 1
    assert _scan("attn.hip", "  static const AttnEnv env = [] { return AttnEnv(); }();\n  static constexpr int KP = 4;\n") == []
    assert len(_scan("attn.hip", "  static int calls = 0;\n")) == 1 and len(_scan("attn.hip", "  static thread_local int n;\n")) == 1


# ------------------------------------------------------------------------------------------------------------ GPU tests
def _environment(E):
    KL._no_switches(KL.SWITCHES + GL.SWITCHES + RL.SWITCHES)
    E.autotune(False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_capture_and_replay_equal_eager(dev, name):
    from mspi_amd import engine as E
    _environment(E)
    _guard(E, dev)
    row = BY_NAME[name]
    run = _Run(row, E, dev)
    want = {}
    for which in ("A", "B"):
        run.load(which)
        want[which] = run.read(run.launch())
    assert any(not _bits_equal(want["A"][k], want["B"][k]) for k in want["A"]), "%s: input sets A and B give one result" % name
    run.load("A")
    host = []
    graph, outs = run.capture(host)
    if name in HOST_ROWS:
        assert host, "%s: a host-argument row that handed the library no host buffer" % name
    _scribble(host)      # the host data the call read is gone before the first replay: the graph holds its own copy
    del host
    for o in outs.values():
        _fill(o)
    torch.cuda.synchronize()
    run.load("B")
    graph.replay()
    _equal(run.read(outs), want["B"], "%s replay on B" % name)
    run.load("A")
    for i in (1, 2):
        graph.replay()
        _equal(run.read(outs), want["A"], "%s replay %d on A" % (name, i))
    print("%s: %s  %s  replay B / A / A: equal" % (name, "+".join(row.entries), row.shape()))


# ---- cold capture: one fresh process, no eager warm-up
# The child's wall time on an MI355X, interpreter start and imports included: 3.0 s for the 84 rows (0.8 s in its own loop;
# profiles/r17_launch_replay.txt).  The limit is about five times that, rounded up; test_bench_contract.py gives its children,
# which do far more work, 300 s.
COLD_TIMEOUT = 20


def _cold_main():
    """The child: for each row the capture is the first call of its entry point in this process (the dry pass in front of it
    stubs the entry points out).  One JSON line when a row starts, one with its verdict; exit 1 at the first capture error or
    mismatch."""
    from mspi_amd import engine as E
    dev = torch.device("cuda:0")
    E.autotune(False)
    _guard(E, dev)
    t0 = time.perf_counter()
    for row in ROWS:
        print(json.dumps({"case": row.name, "stage": "start"}), flush=True)
        try:
            run = _Run(row, E, dev)
            graph, outs = run.capture([])
            for o in outs.values():
                _fill(o)
            graph.replay()
            got = run.read(outs)
            want = run.read(run.launch())
            _equal(got, want, "%s cold capture" % row.name)
        except Exception as e:      # noqa: BLE001 -- reported to the parent, which fails the test
            print(json.dumps({"case": row.name, "stage": "done", "equal": False, "error": "%s: %s" % (type(e).__name__, str(e)[:400])}), flush=True)
            sys.exit(1)
        print(json.dumps({"case": row.name, "stage": "done", "equal": True}), flush=True)
    print(json.dumps({"case": None, "stage": "end", "seconds": round(time.perf_counter() - t0, 2)}), flush=True)


@pytest.mark.gpu
def test_cold_capture_in_a_fresh_process(dev):
    """One fresh Python process walks every row; a status that means a fault, an abort or a hang of the child ends the whole
    session (nothing more is started on a GPU that may be in a bad state).  Wall time and limit: see COLD_TIMEOUT."""
    from mspi_amd import engine as E
    _environment(E)
    last, lines, status = None, [], None
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cold"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           universal_newlines=True, timeout=COLD_TIMEOUT)
        status, out, err = p.returncode, p.stdout, p.stderr
    except subprocess.TimeoutExpired as e:
        status, out, err = 124, e.stdout or "", e.stderr or ""
        out = out.decode() if isinstance(out, bytes) else out
        err = err.decode() if isinstance(err, bytes) else err
    wall = time.perf_counter() - t0
    for line in out.splitlines():
        if line.startswith("{"):
            rec = json.loads(line)
            lines.append(rec)
            if rec.get("case"):
                last = rec["case"]
    if status in (134, 139, 124, 137) or status < 0:
        # a fault, an abort or a hang of the child: nothing more starts on the GPU in this session
        pytest.exit("cold-capture child ended with status %s at row %s; stderr: %s" % (status, last, err[-800:]), returncode=3)
    done = {r["case"]: r for r in lines if r.get("stage") == "done"}
    bad = [r for r in done.values() if not r["equal"]]
    assert status == 0 and not bad, "cold capture: status %d, %s\nstderr: %s" % (status, bad or "no row reported a mismatch", err[-1500:])
    assert set(done) == set(BY_NAME), "rows the child did not report: %s" % sorted(set(BY_NAME) - set(done))
    print("cold-capture child: %d rows equal, wall time %.1f s (child's own loop %.1f s), limit %d s"
          % (len(done), wall, lines[-1].get("seconds", float("nan")), COLD_TIMEOUT))


# ---- a second device
@pytest.mark.gpu
def test_second_device_equals_the_first(dev):
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs visible to the process (%d here)" % torch.cuda.device_count())
    _environment(E)
    pp = RL.PP_CASES[2]
    conv = NF.BY_NAME["conv-reg-f16x3-x"]
    maps, u8 = RL._pp_maps(pp), BY_NAME["jpeg_gray"].make("A")["maps"]

    def three(d):
        _guard(E, d)
        got = {"pp": E.postprocess_u8(maps.to(d), pp[3:]), "conv": conv.run(E, d, conv.make())["y"]}
        files, lengths = E.jpeg_encode_gray(u8.to(d), quality=95)
        got = BY_NAME["jpeg_gray"].post({"files": files, "lengths": lengths}) | got
        torch.cuda.synchronize(d)
        assert not E.range_flag(), "the status word went up on %s" % d
        return {k: v.cpu() for k, v in got.items()}

    first = three(dev)
    dev1 = torch.device("cuda:1")
    with torch.cuda.device(1):
        second = three(dev1)
        on1 = maps.to(dev1)
    assert not (first["pp"] == first["pp"].reshape(-1)[0]).all(), "device 0 already gives a constant map"
    for k in first:
        assert _bits_equal(first[k], second[k]), "%s on cuda:1 differs from cuda:0 (%d elements)" % (k, int((first[k] != second[k]).sum()))
    # a tensor that is not on the current device: refused before anything is launched
    assert torch.cuda.current_device() == 0
    with _tap(E._lib.load(), stub=False) as calls:
        with pytest.raises(MspiError, match=r"cuda:1.*cuda:0"):
            E.postprocess_u8(on1, pp[3:])
        with pytest.raises(MspiError, match=r"cuda:1.*cuda:0"):
            E.jpeg_encode_gray(u8.to(dev1))
    assert calls == []
    with torch.cuda.device(1), pytest.raises(MspiError, match=r"cuda:0.*cuda:1"):
        E.postprocess_u8(maps.to(dev), pp[3:])
    print("second device: postprocess_u8, f16x3 conv, jpeg_encode_gray on cuda:1 == cuda:0; wrong-device tensors refused")


if __name__ == "__main__" and sys.argv[1:] == ["--cold"]:
    _cold_main()
