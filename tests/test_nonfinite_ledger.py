"""Ledger of what every entry point of libmspi_hip.so does with a NaN or an Inf in its floating-point operands.

The contract (engine.py above _STATUS, include/mspi_hip.h at mspi_set_status_word, DESIGN.md "Non-finite data"): feed an
entry point a tensor in which one to three elements are NaN (and, separately, +Inf and -Inf), evaluate the same operation
in float64 torch on the CPU on the same poisoned operands, then
  (a) every output position where the float64 reference is NaN or Inf is non-finite in the kernel's output, OR the range
      flag (engine.range_flag()) is up after a synchronise; an entry point whose output type cannot carry a NaN (u8) must
      raise the flag;
  (b) every output position where the reference is finite is finite in the kernel's output and inside that kernel's own
      ledger bar (1e-5 of max |finite ref| for the fp32 kernels, 2e-5 where the kernel's own test uses 2e-5), whether or not
      the flag went up: a poison never leaks into rows, channels or samples that do not depend on it.
(a) is one-directional: with Inf the reference itself is sometimes finite (relu(-inf) == 0, max(-inf, x) == x) and (b) then
pins the kernel to the same finite value; which of inf / NaN comes out is not pinned, only "not finite".

A kernel that legitimately spreads a poison further than torch does is named in B_EXCEPTIONS with its reason; for such a
case (b) holds on every position the poison cannot reach (the positions where the reference of the NaN poison is finite).

CPU: every name of _lib.EXPORTS is a key of NONFINITE_LEDGER or of NONFINITE_EXCLUDED; every ledger entry has a case; the
float64 reference of every NaN case has a non-finite output and, for a local case, a finite one; the exception list is
pinned; the oracle's log-softmax makes any poison of the 64-pixel X3D-L case an all-NaN map.
GPU: every case x {NaN, +Inf, -Inf} on the smallest row of the kernel's own ledger, outputs prefilled with a finite sentinel
(so "unwritten" and "propagated" stay apart); whole models on a poisoned clip / spectrogram, untuned and first-sight tuned."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gemm_ledger as GL
import test_kernel_ledger as KL
import test_rowop_ledger as RL
from test_kernel_ledger import _guard, _rel_close      # the tolerance rule and the flag reset of the ledgers

SENTINEL = -777.25
TOL = 1e-5
POISONS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
F32, F16X3 = 0, 1
RELU, SWISH = 1, 4

# --------------------------------------------------------------------------------------------------------- the two lists
# entry point -> what the cases of that entry cover.  Every key has at least one case below (asserted on the CPU).
NONFINITE_LEDGER = {
    "mspi_conv_fwd": "register fp32 / register f16x3 / LDS-DMA 128 and 256 rows, ReLU; x, res, gate",
    "mspi_conv_splitk_fwd": "split-K, ReLU; x, res",
    "mspi_conv_halo_fwd": "halo-staged 3x3x3, ReLU; x, res",
    "mspi_rowgemm_fwd": "thin GEMM, ReLU; x, res, gate",
    "mspi_gemm_sp_fwd": "pre-split planes in, rows out and planes out, ReLU; x, res",
    "mspi_mlp_fwd": "fused MLP with and without the fused LayerNorm; x, res",
    "mspi_x3d_ab_fwd": "fused a + b, Swish and pooled; x",
    "mspi_x3d_ab_s2_fwd": "stride-2 fused a + b, Swish and pooled; x",
    "mspi_x3d_ca_fwd": "fused c + next a; u, res, gate",
    "mspi_x3d_stem_fwd": "fused stem; x",
    "mspi_dwconv_fwd": "LDS, tile, strip and generic kernels, ReLU and Swish, pooled partial sums; x",
    "mspi_maxpool_fwd": "x",
    "mspi_se_gate": "both kernels; pool",
    "mspi_layernorm_fwd": "act none and ReLU; x",
    "mspi_layernorm_sp_fwd": "planes out, act none and ReLU; x",
    "mspi_split_planes_fwd": "round trip with mspi_join_planes_fwd; x",
    "mspi_join_planes_fwd": "round trip with mspi_split_planes_fwd; x",
    "mspi_attn_fwd": "fp32 and f16x3; q, k, v, res",
    "mspi_attn_fwd_ws": "planes, pipeline, key split + merge; q, k, v, res",
    "mspi_mvit_qk_augment": "q, k",
    "mspi_mvit_qk_augment_p": "q (and the P it was multiplied into), k",
    "mspi_upsample_fwd": "factors 2 / 4 / 8, act none and ReLU, accumulate; src, dst",
    "mspi_upsample_sum_fwd": "two sources, accumulate, ReLU; src, dst",
    "mspi_rowgate": "x, mask",
    "mspi_space_to_depth": "x",
    "mspi_permute_fwd": "vector and scalar kernels; src",
    "mspi_gated_sum_fwd": "src, logit",
    "mspi_add": "a",
    "mspi_mean_rows": "x",
    "mspi_mean_rows_ws": "x",
    "mspi_neg_cosine": "p (a whole-tensor reduction)",
    "mspi_logsumexp_sub": "x",
    "mspi_postprocess_u8": "the u8 sink: the flag is required",
    "mspi_logsumexp_sub_bwd": "g, logp",
    "mspi_conv_c1_bwd": "dz, y",
    "mspi_upsample_bwd": "dy",
    "mspi_conv_wgrad_fwd": "x, dy",
    "mspi_conv_wgrad_wide_fwd": "x, dy",
    "mspi_bn_stats": "x",
    "mspi_bn_apply": "ReLU; x, mean",
    "mspi_bn_bwd": "dy",
    "mspi_saliency_loss_fwd": "log map of one sample",
    "mspi_saliency_loss_bwd": "log map of one sample",
    "mspi_logspec_fwd": "one wave sample",
}

_HOST = "host-only query: no GPU launch, no activation operand"
_INT = "integer data path: reads u8 / bitstream bytes, no floating-point activation operand"
_EVAL = ("saliency metric / AUC / IG kernel: its NaN pattern is pinned by tests/test_eval_kernels.py, and its binning code was "
         "not re-read for data-derived indices")
NONFINITE_EXCLUDED = {
    "mspi_version": _HOST, "mspi_last_error": _HOST, "mspi_device_count": _HOST,
    "mspi_set_status_word": "registers the word the flag lives in; exercised by every GPU case",
    "mspi_conv_splitk_ws_bytes": _HOST, "mspi_conv_variant": _HOST, "mspi_conv_halo_supported": _HOST,
    "mspi_conv_halo_variant": _HOST, "mspi_dwconv_pool_rows": _HOST, "mspi_dwconv_variant": _HOST,
    "mspi_se_gate_variant": _HOST, "mspi_layernorm_variant": _HOST, "mspi_attn_ws_bytes": _HOST, "mspi_attn_variant": _HOST,
    "mspi_mean_rows_slices": _HOST, "mspi_permute_variant": _HOST, "mspi_gemm_sp_variant": _HOST,
    "mspi_saliency_auc_ws_bytes": _HOST, "mspi_saliency_loss_ws_bytes": _HOST, "mspi_conv_c1_bwd_ws_bytes": _HOST,
    "mspi_conv_wgrad_supported": _HOST, "mspi_conv_wgrad_ws_bytes": _HOST, "mspi_conv_wgrad_variant": _HOST,
    "mspi_conv_wgrad_wide_supported": _HOST, "mspi_conv_wgrad_wide_ws_bytes": _HOST, "mspi_conv_wgrad_wide_variant": _HOST,
    "mspi_bn_ws_bytes": _HOST, "mspi_rowgemm_packed_bytes": _HOST, "mspi_rowgemm_supported": _HOST,
    "mspi_rowgemm_variant": _HOST, "mspi_x3d_ca_packed_bytes": _HOST, "mspi_x3d_ca_supported": _HOST,
    "mspi_x3d_ca_variant": _HOST, "mspi_x3d_ab_supported": _HOST, "mspi_x3d_ab_pool_rows": _HOST,
    "mspi_x3d_ab_packed_bytes": _HOST, "mspi_x3d_ab_variant": _HOST, "mspi_x3d_ab_s2_supported": _HOST,
    "mspi_x3d_ab_s2_pool_rows": _HOST, "mspi_x3d_ab_s2_variant": _HOST, "mspi_x3d_stem_supported": _HOST,
    "mspi_x3d_stem_variant": _HOST, "mspi_mlp_packed_bytes": _HOST, "mspi_mlp_variant": _HOST,
    "mspi_postprocess_workspace": _HOST, "mspi_clip_resize_plan": _HOST,
    "mspi_jpeg_gray_header": _HOST, "mspi_jpeg_gray_bound": _HOST, "mspi_jpeg_gray_ws_bytes": _HOST,
    "mspi_jpeg_dec_parse": _HOST, "mspi_jpeg_dec_ws_bytes": _HOST,
    "mspi_jpeg_gray_fwd": _INT, "mspi_jpeg_dec_fwd": _INT, "mspi_resize_norm_fwd": _INT, "mspi_clip_resize_norm_fwd": _INT,
    "mspi_resize_fixation_fwd": _INT,
    "mspi_resize_bilinear_fwd": "evaluation-side resize of saved u8 / float maps in front of the metric kernels: out of scope "
                                "with them (tests/test_evaluate.py)",
    "mspi_saliency_metrics": _EVAL, "mspi_saliency_auc_judd": _EVAL, "mspi_saliency_sauc_counts": _EVAL, "mspi_saliency_ig": _EVAL,
}

# (case, poison) -> why the kernel may be non-finite where torch is finite.  (b) then holds outside the poison's reach.
_SPLIT = ("the f16 hi/lo split of an Inf is (inf, inf - inf = NaN): a key whose logit torch drives to -inf (weight 0) is a NaN "
          "logit here, so the whole row is NaN where torch's row is finite; the flag is up")
B_EXCEPTIONS = {("attn-%s-k" % kind, sign): _SPLIT for kind in ("f16x3", "planes", "pipe", "merge") for sign in ("+inf", "-inf")}
B_EXCEPTION_KEYS = {("attn-f16x3-k", "+inf"), ("attn-f16x3-k", "-inf"), ("attn-planes-k", "+inf"), ("attn-planes-k", "-inf"),
                    ("attn-pipe-k", "+inf"), ("attn-pipe-k", "-inf"), ("attn-merge-k", "+inf"), ("attn-merge-k", "-inf")}


# ------------------------------------------------------------------------------------------------------------- the cases
class Case:
    """One launch (or two) of an entry point.  make() -> CPU fp32 operands; where: [(operand, index)] to poison;
    ref(t) -> {name: float64 reference}; run(E, dev, t) -> {name: kernel output}.  local: the reference keeps finite outputs
    under a NaN poison (everything but whole-tensor reductions).  elementwise: the bar is tol * |ref| per element."""

    def __init__(self, name, entries, make, where, ref, run, tol=TOL, local=True, elementwise=False, sink=None):
        self.name, self.entries = name, (entries,) if isinstance(entries, str) else tuple(entries)
        self.make, self.where, self.ref, self.run = make, where, ref, run
        self.tol, self.local, self.elementwise, self.sink = tol, local, elementwise, sink

    def operands(self, value):
        t = self.make()
        for key, idx in self.where:
            t[key][idx] = value
        return t


CASES = []


def _case(*a, **k):
    CASES.append(Case(*a, **k))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _cl(E, t5, dev):
    """NCDHW cpu tensor -> dense CL on the device."""
    N, Cc, T, H, W = t5.shape
    x = E.alloc(N, T, H, W, Cc, dev)
    x.buf.zero_()
    x.as_ncdhw().copy_(t5.to(dev))
    return x


def _sentinel(E, N, T, H, W, Cc, dev):
    o = E.alloc(N, T, H, W, Cc, dev)
    o.buf.fill_(SENTINEL)
    return o


def _rows(t5):
    return t5.permute(0, 2, 3, 4, 1).reshape(-1, t5.shape[1])


def _three(shape, c0=1, c1=None):
    """Three poison positions of an [N, C, T, H, W] operand, all in sample 0: the corner of frame 0 (only padding-adjacent
    taps of a conv see it), an interior one, and the last position of the sample (a row / tile edge)."""
    N, Cc, T, H, W = shape
    c1 = Cc - 1 if c1 is None else c1
    return [(0, c0, 0, 0, 0), (0, c1, T // 2, H // 2, W // 2), (0, 0, T - 1, H - 1, W - 1)]


# ---- conv / GEMM family
def _conv_cases():
    from mspi_amd import engine as E
    kinds = {     # name -> (entry, geometry, C, Cout, precision, tile, operands to poison)
        "conv-reg-f32": ("mspi_conv_fwd", GL.TAPS, 20, 44, F32, 3, ("x", "res")),
        "conv-reg-f16x3": ("mspi_conv_fwd", GL.DENSE, 20, 44, F16X3, 3, ("x", "res")),
        "conv-splitk": ("mspi_conv_splitk_fwd", GL.CUBE, 20, 76, F16X3, E.SPLITK + 2, ("x", "res")),
        "conv-dma128": ("mspi_conv_fwd", GL.TAPS, 20, 76, F16X3, 7, ("x", "res")),
        "conv-dma128-gate": ("mspi_conv_fwd", GL.DENSE3, 20, 76, F16X3, 7, ("gate",)),
        "conv-dma256": ("mspi_conv_fwd", GL.DENSE, 20, 140, F16X3, 14, ("x", "res")),
        "conv-halo": ("mspi_conv_halo_fwd", GL.CUBE, 32, 44, F16X3, E.HALO, ("x", "res")),
        "rowgemm": ("mspi_rowgemm_fwd", GL.DENSE3, 28, 44, F16X3, E.THIN, ("x", "res", "gate")),
    }
    for name, (entry, geom, Cc, Co, prec, tile, operands) in kinds.items():
        k, s, p, (N, T, H, W) = geom
        gated = "gate" in operands
        M0 = math.prod((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip((T, H, W), k, s, p))      # output rows per sample

        def make(Cc=Cc, Co=Co, k=k, N=N, T=T, H=H, W=W, M0=M0, seed=len(name) * 131 + Co):
            g = _gen(seed)
            return dict(x=torch.randn(N, Cc, T, H, W, generator=g), w=torch.randn(Co, Cc, *k, generator=g) / math.sqrt(Cc * math.prod(k)),
                        b=torch.randn(Co, generator=g), res=torch.randn(N * M0, Co, generator=g), gate=torch.rand(N, Cc, generator=g) * 2)

        def ref(t, s=s, p=p, gated=gated):
            x = GL._swish_gate(t["x"].double(), t["gate"].double()) if gated else t["x"].double()
            y = _rows(F.conv3d(x, t["w"].double(), t["b"].double(), s, p))
            return {"y": F.relu(y + t["res"].double())}

        def run(E, dev, t, s=s, p=p, prec=prec, tile=tile, gated=gated, Co=Co):
            pk = E.pack_conv(t["w"], t["b"], None, s, p, E.ACT_RELU, device=dev, prec=prec)
            x = _cl(E, t["x"], dev)
            To, Ho, Wo = E._out_extent(x.T, x.H, x.W, pk.k, s, p)
            out = _sentinel(E, x.N, To, Ho, Wo, Co, dev)
            gd = GL._nan_tail(t["gate"], dev) if gated else None
            E.conv(x, pk, out=out, res=E.from_rows(t["res"].to(dev)), gate=gd, tile=tile)
            return {"y": out.as_rows()[:, :Co]}

        for op in operands:
            where = {"x": [("x", i) for i in _three((N, Cc, T, H, W))], "res": [("res", (5, 3)), ("res", (M0 - 1, Co - 1))],
                     "gate": [("gate", (0, 2))]}[op]
            _case("%s-%s" % (name, op), entry, make, where, ref, run)


def _gemm_sp_cases():
    N, T, H, W, K = 2, 3, 7, 9, 64
    M = N * T * H * W
    for planes_out, Co, operands in ((False, 140, ("x", "res")), (True, 160, ("x",))):
        def make(Co=Co):
            g = _gen(6000 + Co)
            return dict(x=torch.randn(M, K, generator=g), w=torch.randn(Co, K, generator=g) / math.sqrt(K), b=torch.randn(Co, generator=g),
                        res=torch.randn(M, Co, generator=g))

        def ref(t, planes_out=planes_out):
            y = t["x"].double() @ t["w"].double().t() + t["b"].double()
            return {"y": F.relu(y if planes_out else y + t["res"].double())}

        def run(E, dev, t, planes_out=planes_out, Co=Co):
            lib = E._lib.load()
            pk = E.pack_conv(t["w"], t["b"], act=E.ACT_RELU, device=dev, prec=F16X3)
            xs = E.alloc_sp(N, T, H, W, K, dev)
            xd = t["x"].to(dev).contiguous()
            E.check(lib.mspi_split_planes_fwd(xd.data_ptr(), K, M, K, xs.ptr, xs.ld, xs.plane, E._stream()), "mspi_split_planes_fwd")
            if planes_out:
                return {"y": E.join_planes(E.conv(xs, pk, tile=6, sp_out=True)).as_rows()[:, :Co]}
            out = _sentinel(E, N, T, H, W, Co, dev)
            E.conv(xs, pk, out=out, res=E.from_rows(t["res"].to(dev)), tile=6)
            return {"y": out.as_rows()[:, :Co]}

        for op in operands:
            where = {"x": [("x", (0, 5)), ("x", (127, K - 1)), ("x", (128, 0))], "res": [("res", (5, 3)), ("res", (188, Co - 1))]}[op]
            _case("gemm_sp-%s-%s" % ("planes" if planes_out else "rows", op), "mspi_gemm_sp_fwd", make, where, ref, run)


def _mlp_cases():
    M, Cc, hidden = 300, 96, 64

    def make():
        g = _gen(96134)
        return dict(x=torch.randn(M, Cc, generator=g) * 1.5 + 0.25, w1=torch.randn(hidden, Cc, generator=g) / math.sqrt(Cc),
                    b1=torch.randn(hidden, generator=g) * 0.5, w2=torch.randn(Cc, hidden, generator=g) / math.sqrt(hidden),
                    b2=torch.randn(Cc, generator=g), gam=torch.randn(Cc, generator=g) * 0.5 + 1, bet=torch.randn(Cc, generator=g) * 0.5,
                    res=torch.randn(M, Cc, generator=g))

    for ln in (1, 0):
        def ref(t, ln=ln):
            d = {k: v.double() for k, v in t.items()}
            h = F.layer_norm(d["x"], (Cc,), d["gam"], d["bet"], 1e-6) if ln else d["x"]
            return {"y": F.gelu(h @ d["w1"].t() + d["b1"]) @ d["w2"].t() + d["b2"] + d["res"]}

        def run(E, dev, t, ln=ln):
            pk = E.pack_mlp(t["w1"], t["b1"], t["w2"], t["b2"], device=dev)
            out = _sentinel(E, M, 1, 1, 1, Cc, dev)
            E.mlp(E.from_rows(t["x"].to(dev)), pk, res=E.from_rows(t["res"].to(dev)), ln=(t["gam"].to(dev), t["bet"].to(dev)) if ln else None,
                  eps=1e-6, out=out)
            return {"y": out.as_rows()[:, :Cc]}

        for op, where in (("x", [("x", (0, 5)), ("x", (127, Cc - 1)), ("x", (299, 0))]), ("res", [("res", (5, 3)), ("res", (299, Cc - 1))])):
            _case("mlp-ln%d-%s" % (ln, op), "mspi_mlp_fwd", make, where, ref, run)


def _x3d_cases():
    # fused a + b, stride 1 (row 27142 of test_gemm_ledger.py) and stride 2 (the first case shape family of test_x3d_head.py)
    for s2, (N, T, H, W, Cin, Cmid) in ((False, GL.X3D_AB_LEDGER[27142]), (True, (2, 3, 14, 28, 24, 52))):
        def make(N=N, T=T, H=H, W=W, Cin=Cin, Cmid=Cmid):
            g = _gen(Cin * 100 + Cmid)
            return dict(x=torch.randn(N, Cin, T, H, W, generator=g), wa=torch.randn(Cmid, Cin, 1, 1, 1, generator=g) / math.sqrt(Cin),
                        ba=torch.randn(Cmid, generator=g) * 0.5, wb=torch.randn(Cmid, 1, 3, 3, 3, generator=g) / math.sqrt(27),
                        bb=torch.randn(Cmid, generator=g))

        for pool in (False, True):
            def ref(t, s2=s2, pool=pool, Cmid=Cmid):
                a = F.relu(F.conv3d(t["x"].double(), t["wa"].double(), t["ba"].double()))
                u = F.conv3d(a, t["wb"].double(), t["bb"].double(), (1, 2, 2) if s2 else 1, 1, 1, Cmid)
                return {"u": u, "pool": u.sum((2, 3, 4))} if pool else {"u": u * torch.sigmoid(u)}

            def run(E, dev, t, s2=s2, pool=pool, Cmid=Cmid):
                pa = E.pack_conv(t["wa"], t["ba"], None, act=E.ACT_RELU, device=dev, prec=F16X3)
                pb = E.pack_dwconv(t["wb"], t["bb"], None, (1, 2, 2) if s2 else (1, 1, 1), (1, 1, 1), device=dev)
                pk = (E.pack_x3d_ab_s2 if s2 else E.pack_x3d_ab)(pa, pb)
                x = _cl(E, t["x"], dev)
                got = (E.x3d_ab_s2 if s2 else E.x3d_ab)(x, pk, pool=pool)
                if pool:
                    return {"u": got[0].as_ncdhw(Cmid), "pool": got[1].sum(1)[:, :Cmid]}
                return {"u": got.as_ncdhw(Cmid)}

            _case("x3d_ab%s-%s-x" % ("_s2" if s2 else "", "pool" if pool else "swish"), "mspi_x3d_ab_s2_fwd" if s2 else "mspi_x3d_ab_fwd",
                  make, [("x", i) for i in _three((N, Cin, T, H, W))], ref, run)

    # fused c + next a (rows 1280 / 1281 of test_gemm_ledger.py)
    for code in (1280, 1281):
        N, rps, D, Cx = GL.X3D_CA_LEDGER[code]
        gated, M = code % 10 == 1, N * rps

        def make(N=N, D=D, Cx=Cx, M=M, code=code):
            g = _gen(code)
            return dict(u=torch.randn(M, D, generator=g), wc=torch.randn(Cx, D, generator=g) / math.sqrt(D), bc=torch.randn(Cx, generator=g) * 0.5,
                        wa=torch.randn(D, Cx, generator=g) / math.sqrt(Cx), ba=torch.randn(D, generator=g) * 0.5,
                        res=torch.randn(M, Cx, generator=g), gate=torch.rand(N, D, generator=g) * 2)

        def ref(t, gated=gated, rps=rps, M=M):
            d = {k: v.double() for k, v in t.items()}
            u = GL._swish_gate(d["u"], d["gate"][torch.arange(M) // rps]) if gated else d["u"]
            y = F.relu(u @ d["wc"].t() + d["bc"] + d["res"])
            return {"y": y, "t": F.relu(y @ d["wa"].t() + d["ba"])}

        def run(E, dev, t, gated=gated, N=N, rps=rps, D=D, Cx=Cx):
            pk = E.pack_x3d_ca(E.pack_conv(t["wc"], t["bc"], act=E.ACT_RELU, device=dev, prec=F16X3),
                               E.pack_conv(t["wa"], t["ba"], act=E.ACT_RELU, device=dev, prec=F16X3))
            uc, rc = E.alloc(N, 1, 1, rps, D, dev), E.alloc(N, 1, 1, rps, Cx, dev)
            uc.as_rows()[:, :D] = t["u"].to(dev)
            rc.as_rows()[:, :Cx] = t["res"].to(dev)
            y, tt = E.x3d_ca(uc, pk, rc, gate=GL._nan_tail(t["gate"], dev) if gated else None)
            return {"y": y.as_rows()[:, :Cx], "t": tt.as_rows()[:, :D]}

        ops = {"u": [("u", (0, 5)), ("u", (rps - 1, D - 1))], "res": [("res", (5, 3)), ("res", (rps - 1, Cx - 1))]}
        if gated:
            ops["gate"] = [("gate", (0, 2))]
        for op, where in ops.items():
            _case("x3d_ca-%d-%s" % (code, op), "mspi_x3d_ca_fwd", make, where, ref, run)

    # fused stem: relu(bn(temporal dw (5,1,1)(conv_xy (1,3,3) / (1,2,2)))) with the BatchNorm folded
    N, T, H, W = 2, 6, 28, 28

    def make_stem():
        g = _gen(T + H + W)
        return dict(x=torch.randn(N, 3, T, H, W, generator=g), wxy=torch.randn(24, 3, 1, 3, 3, generator=g) / math.sqrt(27),
                    wt=torch.randn(24, 1, 5, 1, 1, generator=g) / math.sqrt(5), b=torch.rand(24, generator=g) * 0.4 - 0.2)

    def ref_stem(t):
        y = F.conv3d(t["x"].double(), t["wxy"].double(), None, (1, 2, 2), (0, 1, 1))
        return {"y": F.relu(F.conv3d(y, t["wt"].double(), t["b"].double(), 1, (2, 0, 0), 1, 24))}

    def run_stem(E, dev, t):
        pk = E.pack_x3d_stem(t["wxy"], t["wt"], None)
        pk.bias = t["b"].clone()
        out = _sentinel(E, N, T, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 24, dev)
        return {"y": E.x3d_stem(t["x"].to(dev), pk, out=out).as_ncdhw(24)}

    _case("x3d_stem-x", "mspi_x3d_stem_fwd", make_stem, [("x", i) for i in _three((N, 3, T, H, W), c0=0, c1=1)], ref_stem, run_stem, tol=2e-5)


# ---- depthwise, pooling, squeeze-excite
def _dw_cases():
    for code in (1717, 2317, 3714, 4000):      # one row per kind: LDS-staged, register tile, strip, generic
        N, Cc, T, H, W, k, s, p = KL.DW_LEDGER[code]

        def make(N=N, Cc=Cc, T=T, H=H, W=W, k=k, code=code):
            g = _gen(code)
            return dict(x=torch.randn(N, Cc, T, H, W, generator=g), w=torch.randn(Cc, 1, *k, generator=g) / math.sqrt(math.prod(k)),
                        b=torch.randn(Cc, generator=g))

        for how in ("relu", "swish", "pool"):
            if how == "pool" and not KL._pool_supported(k, s):
                continue

            def ref(t, how=how, s=s, p=p, Cc=Cc):
                u = F.conv3d(t["x"].double(), t["w"].double(), t["b"].double(), s, p, 1, Cc)
                return {"y": u, "pool": u.sum((2, 3, 4))} if how == "pool" else {"y": F.relu(u) if how == "relu" else u * torch.sigmoid(u)}

            def run(E, dev, t, how=how, s=s, p=p, Cc=Cc, code=code):
                pk = E.pack_dwconv(t["w"], t["b"], None, s, p, E.ACT_NONE, device=dev)
                x = _cl(E, t["x"], dev)
                assert E.dwconv_variant(x, pk) == code
                To, Ho, Wo = E._out_extent(x.T, x.H, x.W, pk.k, s, p)
                out = _sentinel(E, x.N, To, Ho, Wo, Cc, dev)
                if how == "pool":
                    _, part = E.dwconv(x, pk, out=out, pool=True, act=E.ACT_NONE)
                    return {"y": out.as_ncdhw(), "pool": part.sum(1)[:, :Cc]}
                E.dwconv(x, pk, out=out, act=RELU if how == "relu" else SWISH)
                return {"y": out.as_ncdhw()}

            _case("dwconv-%d-%s-x" % (code, how), "mspi_dwconv_fwd", make, [("x", i) for i in _three((N, Cc, T, H, W), c1=5)], ref, run)

    for case in (RL.MAXPOOL_CASES[0], RL.MAXPOOL_CASES[4]):
        N, Cc, T, H, W, k, s, p = case

        def make(N=N, Cc=Cc, T=T, H=H, W=W):
            return dict(x=torch.randn(N, Cc, T, H, W, generator=_gen(Cc + T + H)))

        def ref(t, k=k, s=s, p=p):
            return {"y": F.max_pool3d(t["x"].double(), k, s, p)}

        def run(E, dev, t, k=k, s=s, p=p, Cc=Cc):
            x = _cl(E, t["x"], dev)
            To, Ho, Wo = E._out_extent(x.T, x.H, x.W, k, s, p)
            out = _sentinel(E, x.N, To, Ho, Wo, Cc, dev)
            return {"y": E.maxpool(x, k, s, p, out=out).as_ncdhw()}

        _case("maxpool-k%d%d%d-x" % k, "mspi_maxpool_fwd", make, [("x", i) for i in _three((N, Cc, T, H, W), c1=5)], ref, run, tol=0.0)

    for code, case in ((1, RL.SE_LEDGER[1][0]), (2, RL.SE_LEDGER[2][0])):
        def make(case=case):
            return dict(zip(("pool", "w1", "b1", "w2", "b2"), RL._se_inputs(case)))

        def ref(t):
            return {"gate": RL._se_eval([t[k] for k in ("pool", "w1", "b1", "w2", "b2")], torch.float64)}

        def run(E, dev, t, case=case):
            gate = torch.full((case[3], case[0]), SENTINEL, device=dev)
            td = [t[k].to(dev) for k in ("pool", "w1", "b1", "w2", "b2")]
            E.se_gate(td[0], RL.SE_INV, *td[1:], gate=gate)
            return {"gate": gate}

        _case("se_gate-%d-pool" % code, "mspi_se_gate", make, [("pool", (0, 3, 7))], ref, run)


# ---- normalisation and the f16 planes
def _norm_cases():
    for c in (64, 96):
        for act in (0, RELU):
            for planes in (False, True):
                def make(c=c):
                    return dict(zip(("x", "g", "b", "tab"), RL._ln_inputs(c)))

                def ref(t, act=act):
                    return {"y": RL._ln_eval((t["x"], t["g"], t["b"], t["tab"]), act, False, torch.float64)}

                def run(E, dev, t, act=act, planes=planes, c=c):
                    N, R = RL.LN_N, RL.LN_R
                    x = E.CL(t["x"].to(dev).reshape(-1), 0, N, R, 1, 1, c, c)
                    g, b = t["g"].to(dev), t["b"].to(dev)
                    if planes:
                        return {"y": E.join_planes(E.layernorm(x, g, b, 1e-5, act=act, sp=True)).as_rows()[:, :c].view(N, R, c)}
                    out = _sentinel(E, N, R, 1, 1, c, dev)
                    E.layernorm(x, g, b, 1e-5, out=out, act=act)
                    return {"y": out.buf.view(N, R, c)}

                _case("layernorm%s-C%d-act%d-x" % ("_sp" if planes else "", c, act), "mspi_layernorm_sp_fwd" if planes else "mspi_layernorm_fwd",
                      make, [("x", (0, 2, 5)), ("x", (1, RL.LN_R - 1, c - 1))], ref, run)

    M, K = 47, 96

    def make_sj():
        g = _gen(M + K)
        x = torch.exp2(torch.rand(M, K, generator=g) * 19 - 4) * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1)
        return dict(x=x.clamp(-32767.0, 32767.0))

    def run_sj(E, dev, t):
        lib = E._lib.load()
        xd = t["x"].to(dev).contiguous()
        sp = E.alloc_sp(1, 1, 1, M, K, dev)
        E.check(lib.mspi_split_planes_fwd(xd.data_ptr(), K, M, K, sp.ptr, sp.ld, sp.plane, E._stream()), "mspi_split_planes_fwd")
        y = torch.full((M, K), SENTINEL, device=dev)
        E.check(lib.mspi_join_planes_fwd(sp.ptr, sp.ld, sp.plane, M, K, y.data_ptr(), K, E._stream()), "mspi_join_planes_fwd")
        return {"y": y}

    _case("split_join-x", ("mspi_split_planes_fwd", "mspi_join_planes_fwd"), make_sj, [("x", (3, 5)), ("x", (M - 1, K - 1))],
          lambda t: {"y": t["x"].double()}, run_sj, tol=2.0 ** -21, elementwise=True)


# ---- attention
def _attn_cases():
    pair = 128 * 10000 + 96 * 10      # the (128, 96) pair: every form of it carries the residual
    kinds = {"f32": 10000000 + pair, "f16x3": 20000000 + pair, "planes": 30000000 + pair, "pipe": 50000000 + pair, "merge": 50000000 + pair + 1}
    for kind, code in kinds.items():
        row = KL.ATTN_LEDGER[code]

        def make(row=row, code=code):
            t, _ = KL._attn_inputs(row, code % 100003)
            return t

        def ref(t, row=row):
            return {"o": KL._attn_ref(row, t)}

        def run(E, dev, t, row=row, code=code):
            out, variant = KL._attn_direct(E, row, t, dev, fill=SENTINEL)
            assert variant == code
            return {"o": out}

        Rq, Rk = (2 if row[9] else 1) * row[2], (2 if row[9] else 1) * row[3]
        h1 = row[1] - 1
        for op, idx in (("q", (0, h1, Rq // 2, 5)), ("k", (0, 0, Rk - 1, 17)), ("v", (0, h1, 3, row[5] - 1)), ("res", (0, 0, Rq - 1, 0))):
            # a poisoned key reaches every query row of its sequence and head: with one sequence and one head, every output
            _case("attn-%s-%s" % (kind, op), "mspi_attn_fwd_ws" if row[10] else "mspi_attn_fwd", make, [(op, idx)], ref, run,
                  local=not (op == "k" and row[0] * row[1] == 1))

    # MViT's q / k augment: qa = [scale q | q . R | 0], ka = [k | one-hot | 0]
    case = RL.AUG_CASES[0]
    da, k_thw = case
    Dh, heads, B = RL.AUG_DH, RL.AUG_HEADS, RL.AUG_B
    nq, nk, J = math.prod(RL.AUG_Q), math.prod(k_thw), sum(k_thw)

    def make_aug():
        return dict(zip(("q", "k", "Rh", "Rw", "Rt"), RL._aug_inputs(case)))

    def ref_aug(t):
        tt = tuple(t[n] for n in ("q", "k", "Rh", "Rw", "Rt"))
        qh = t["q"].double().view(B, nq, heads, Dh).transpose(1, 2) * float(torch.tensor(Dh ** -0.5, dtype=torch.float32))
        qa = torch.cat([qh, RL._aug_rel_eval(tt, case, torch.float64), torch.zeros(B, heads, nq, da - Dh - J, dtype=torch.float64)], -1)
        tok = torch.arange(nk)
        onehot = torch.zeros(nk, J, dtype=torch.float64)
        onehot[tok, (tok // k_thw[2]) % k_thw[1]] = 1
        onehot[tok, k_thw[1] + tok % k_thw[2]] = 1
        onehot[tok, k_thw[1] + k_thw[2] + tok // (k_thw[2] * k_thw[1])] = 1
        ka = torch.cat([t["k"].double().view(B, nk, heads, Dh).transpose(1, 2), onehot.expand(B, heads, nk, J),
                        torch.zeros(B, heads, nk, da - Dh - J, dtype=torch.float64)], -1)
        return {"qa": qa, "ka": ka}

    def run_aug(E, dev, t, entry="rel"):
        lib = E._lib.load()
        ld = heads * Dh
        qd, kd = t["q"].reshape(B * nq, ld).to(dev).contiguous(), t["k"].reshape(B * nk, ld).to(dev).contiguous()
        qa = torch.full((B, heads, nq, da), SENTINEL, device=dev)
        ka = torch.full((B, heads, nk, da), SENTINEL, device=dev)
        a = RL._aug_desc(da, k_thw, ld, ld)
        if entry == "rel":
            tabs = [t[n].to(dev).contiguous() for n in ("Rh", "Rw", "Rt")]
            E.check(lib.mspi_mvit_qk_augment(C.byref(a), qd.data_ptr(), kd.data_ptr(), *[v.data_ptr() for v in tabs], qa.data_ptr(),
                                             ka.data_ptr(), E._stream()), "mspi_mvit_qk_augment")
        else:      # P = q rows x every table row, evaluated in float64 on the poisoned q and rounded once
            allrows = torch.cat([t[n].reshape(-1, Dh) for n in ("Rh", "Rw", "Rt")])
            ncol = allrows.shape[0]
            P = (t["q"].reshape(B * nq * heads, Dh).double() @ allrows.double().t()).float()
            ldp = (ncol + 3) // 4 * 4
            Pd = torch.zeros(B * nq * heads, ldp, device=dev)
            Pd[:, :ncol] = P.to(dev)
            nh, nw = RL.AUG_Q[1] * k_thw[1], RL.AUG_Q[2] * k_thw[2]
            where = torch.arange(ncol)
            idx = [where[:nh].view(RL.AUG_Q[1], k_thw[1]), where[nh:nh + nw].view(RL.AUG_Q[2], k_thw[2]), where[nh + nw:].view(RL.AUG_Q[0], k_thw[0])]
            idx = [v.to(torch.int32).to(dev).contiguous() for v in idx]
            E.check(lib.mspi_mvit_qk_augment_p(C.byref(a), qd.data_ptr(), kd.data_ptr(), Pd.data_ptr(), ldp, *[v.data_ptr() for v in idx],
                                               qa.data_ptr(), ka.data_ptr(), E._stream()), "mspi_mvit_qk_augment_p")
        return {"qa": qa, "ka": ka}

    for op, idx in (("q", (0, 5, 7)), ("k", (1, nk - 1, heads * Dh - 1))):
        _case("mvit_aug-%s" % op, "mspi_mvit_qk_augment", make_aug, [(op, idx)], ref_aug, run_aug)
        _case("mvit_aug_p-%s" % op, "mspi_mvit_qk_augment_p", make_aug, [(op, idx)], ref_aug, lambda E, dev, t: run_aug(E, dev, t, "p"))


# ---- row ops
def _up64(x, k):
    """Bilinear up-sample of [NT, C, 1, H, W] in float64, as a 2-D operation: F.interpolate in "trilinear" mode (what
    test_rowop_ledger._up_eval calls, equal on finite data) multiplies every tap by a zero depth weight as well, and 0 * inf
    turns an Inf the operation hands on with weight 1 into a NaN that is no property of the operation."""
    return F.interpolate(x.double()[:, :, 0], scale_factor=k, mode="bilinear", align_corners=False)[:, :, None] if k > 1 else x.double()


def _rowop_cases():
    ups = {"k2": RL.UPSAMPLE_CASES[0], "k4": RL.UPSAMPLE_CASES[1], "k8": RL.UPSAMPLE_CASES[2], "k2-relu": RL.UPSAMPLE_CASES[8],
           "k4-acc-relu": RL.UPSAMPLE_CASES[4]}
    for name, case in ups.items():
        nt, h, w, c, k, acc, act = case

        def make(case=case):
            return dict(zip(("x", "base"), RL._up_inputs(case)))

        def ref(t, case=case):
            k, acc, act = case[4:]
            y = _up64(t["x"], k)
            return {"y": RL._act(y + t["base"].double() if acc else y, act)}

        def run(E, dev, t, case=case):
            nt, h, w, c, k, acc, act = case
            src = _cl(E, t["x"], dev)
            dst = _cl(E, t["base"], dev) if acc else _sentinel(E, nt, 1, h * k, w * k, c, dev)
            E.upsample(src, k, dst=dst, accumulate=acc, act=act)
            return {"y": dst.as_ncdhw()}

        ops = {"x": [("x", (0, 3, 0, 0, 0)), ("x", (0, 5, 0, h // 2, w // 2))]}
        if acc:
            ops["base"] = [("base", (0, 3, 0, 1, 2))]
        for op, where in ops.items():
            _case("upsample-%s-%s" % (name, op), "mspi_upsample_fwd", make, where, ref, run)

    NT, Ho, Wo, Cc = 2, 8, 16, 24

    def make_us():
        g = _gen(816)
        return dict(s0=torch.randn(NT, Cc, 1, Ho // 2, Wo // 2, generator=g), s1=torch.randn(NT, Cc, 1, Ho // 4, Wo // 4, generator=g),
                    base=torch.randn(NT, Cc, 1, Ho, Wo, generator=g))

    def ref_us(t):
        return {"y": F.relu(_up64(t["s0"], 2) + t["base"].double() + _up64(t["s1"], 4))}

    def run_us(E, dev, t):
        dst = _cl(E, t["base"], dev)
        E.upsample_sum(dst, [(_cl(E, t["s0"], dev), 2), (_cl(E, t["s1"], dev), 4)], accumulate=True, act=RELU)
        return {"y": dst.as_ncdhw()}

    for op, idx in (("s0", (0, 3, 0, 1, 2)), ("s1", (0, 5, 0, 0, 0)), ("base", (0, 7, 0, 3, 3))):
        _case("upsample_sum-%s" % op, "mspi_upsample_sum_fwd", make_us, [(op, idx)], ref_us, run_us)

    rg = RL.ROWGATE_CASES[0]

    def run_rg(E, dev, t):
        n, tt, h, w, c = rg
        x = _cl(E, t["x"], dev)
        E.rowgate(x, E.CL(t["m"].to(dev).reshape(-1).contiguous(), 0, n, tt, h, w, 1, 1))
        return {"y": x.as_ncdhw()}

    for op, idx in (("x", (0, 3, 1, 2, 3)), ("m", (0, 0, 2, 4, 6))):
        _case("rowgate-%s" % op, "mspi_rowgate", lambda: dict(zip(("x", "m"), RL._rowgate_inputs(rg))), [(op, idx)],
              lambda t: {"y": RL._rowgate_eval((t["x"], t["m"]), torch.float64)}, run_rg)

    n, tt, h, w, c = RL.S2D_CASES[0]

    def ref_s2d(t):
        rows = t["x"].double().permute(0, 2, 3, 4, 1).reshape(n, tt, h // 2, 2, w // 2, 2, c)
        return {"y": rows.permute(0, 1, 2, 4, 5, 3, 6).reshape(n, tt, h // 2, w // 2, 4 * c).permute(0, 4, 1, 2, 3)}

    def run_s2d(E, dev, t):
        out = _sentinel(E, n, tt, h // 2, w // 2, 4 * c, dev)
        return {"y": E.space_to_depth(_cl(E, t["x"], dev), out=out).as_ncdhw()}

    _case("space_to_depth-x", "mspi_space_to_depth", lambda: dict(x=torch.randn(n, c, tt, h, w, generator=_gen(c))),
          [("x", (0, 3, 0, 0, 0)), ("x", (0, 5, 1, 3, 5))], ref_s2d, run_s2d, tol=0.0)

    for code, pname in ((4, "broadcast"), (1, "innermost_6")):
        dims, strides, xoff, yoff = RL.PERMUTE_LEDGER[code][pname]
        n_src = RL._span(dims, strides) + 1

        def run_perm(E, dev, t, dims=dims, strides=strides, code=code):
            src = t["x"].to(dev)
            out = torch.full((math.prod(dims),), SENTINEL, device=dev)
            d = RL._perm_desc(dims, strides, src.numel())
            assert E._lib.load().mspi_permute_variant(C.byref(d), src.data_ptr(), out.data_ptr()) == code
            return {"y": E.permute(src, dims, strides, out=out)}

        _case("permute-%d-x" % code, "mspi_permute_fwd", lambda n_src=n_src: dict(x=torch.randn(n_src, generator=_gen(n_src))),
              [("x", (3,)), ("x", (n_src - 1,))], lambda t, dims=dims, strides=strides: {"y": t["x"].double().as_strided(tuple(dims), tuple(strides)).reshape(-1)},
              run_perm, tol=0.0)

    gs = RL.GATED_CASES[0]

    def make_gs():
        t = RL._gated_inputs(gs)
        return dict(a=t[0], b=t[1], logit=t[2])

    def run_gs(E, dev, t):
        n, r, c, j = gs
        cls = [E.CL(t[k].to(dev).reshape(-1), 0, n, 1, r, 1, c, c) for k in ("a", "b")]
        out = _sentinel(E, n, 1, r, 1, c, dev)
        E.gated_sum(cls, t["logit"].to(dev), out=out)
        return {"y": out.buf.view(n, r, c)}

    for op, idx in (("a", (0, 7, 3)), ("logit", (1, 10))):
        _case("gated_sum-%s" % op, "mspi_gated_sum_fwd", make_gs, [(op, idx)],
              lambda t: {"y": RL._gated_eval([t["a"], t["b"], t["logit"]], gs, torch.float64)}, run_gs)

    def run_add(E, dev, t):
        y = torch.full((1003,), SENTINEL, device=dev)
        return {"y": E.add(t["a"].to(dev), t["b"].to(dev), y)}

    _case("add-a", "mspi_add", lambda: dict(a=torch.randn(1003, generator=_gen(1)), b=torch.randn(1003, generator=_gen(2))),
          [("a", (17,)), ("a", (1002,))], lambda t: {"y": t["a"].double() + t["b"].double()}, run_add)

    for form, case in ((1, RL.MEAN_LEDGER[1][1]), (2, RL.MEAN_LEDGER[2][1])):
        r, c, n = case

        def run_mean(E, dev, t, r=r, c=c, n=n, form=form):
            assert RL._mean_form(r) == form
            out = torch.full((n, c), SENTINEL, device=dev)
            E.mean_rows(E.CL(t["x"].to(dev).reshape(-1), 0, n, r, 1, 1, c, c), n, r, out)
            return {"y": out}

        _case("mean_rows-%d-x" % form, "mspi_mean_rows_ws" if form == 2 else "mspi_mean_rows", lambda case=case: dict(x=RL._mean_inputs(case)),
              [("x", (0, 5, 7)), ("x", (1, r - 1, c - 1))], lambda t: {"y": t["x"].double().mean(1)}, run_mean)

    cos = RL.COS_CASES[0]

    def run_cos(E, dev, t):
        p, z = (E.from_rows(t[k].to(dev)) for k in ("p", "z"))
        loss = torch.full((1,), SENTINEL, device=dev)
        E.neg_cosine(p, z, loss, 0.5, False)
        E.neg_cosine(z, p, loss, 0.5, True)
        return {"y": loss}

    _case("neg_cosine-p", "mspi_neg_cosine", lambda: dict(zip(("p", "z"), RL._cos_inputs(cos))), [("p", (1, 7))],
          lambda t: {"y": RL._cos_eval((t["p"], t["z"]), torch.float64)}, run_cos, local=False)

    lse = RL.LSE_CASES[2]

    def run_lse(E, dev, t):
        buf = t["x"].to(dev).reshape(-1).contiguous()
        E.logsumexp_sub(buf, *lse)
        return {"y": buf.view(*lse)}

    _case("logsumexp_sub-x", "mspi_logsumexp_sub", lambda: dict(x=RL._lse_inputs(lse)), [("x", (0, 5))],
          lambda t: {"y": RL._lse_eval(t["x"], torch.float64)}, run_lse)


# ---- the u8 sink
PP_CASE = RL.PP_CASES[2]      # (3, 64, 96, 33, 33)


def _pp_float(logmap, out_hw):
    """test_rowop_ledger._pp_f64 up to, not including, the min-max normalisation and the rounding: what must be finite."""
    k = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / 8.0)
    k = k / k.sum()
    x = F.pad(logmap[None, None].double(), (5, 5, 5, 5), mode="reflect")
    x = torch.exp(F.conv2d(F.conv2d(x, k.view(1, 1, 1, 11)), k.view(1, 1, 11, 1)))
    return F.interpolate(x, size=out_hw, mode="bilinear", align_corners=False)[0, 0]


def _sink_cases():
    def run(E, dev, t):
        return {"u8": E.postprocess_u8(t["maps"].to(dev), PP_CASE[3:])}

    _case("postprocess_u8-maps", "mspi_postprocess_u8", lambda: dict(maps=RL._pp_maps(PP_CASE)), [("maps", (0, 20, 30))],
          lambda t: {"u8": torch.stack([_pp_float(m, PP_CASE[3:]) for m in t["maps"]])}, run, sink="u8")


# ---- training kernels
def _train_cases():
    import readout_restate as RR

    N, L = 2, 1023

    def make_lb():
        g = _gen(77)
        return dict(logp=torch.log_softmax(torch.randn(N, L, generator=g) * 3, 1), g=torch.randn(N, L, generator=g))

    def ref_lb(t):
        return {"dz": t["g"].double() - t["logp"].double().exp() * t["g"].double().sum(1, keepdim=True)}

    for op in ("g", "logp"):
        _case("logsumexp_sub_bwd-%s" % op, "mspi_logsumexp_sub_bwd", make_lb, [(op, (0, 5))], ref_lb,
              lambda E, dev, t: {"dz": E.logsumexp_sub_bwd(t["logp"].to(dev), t["g"].to(dev), dz=torch.full((N, L), SENTINEL, device=dev))})

    # last conv (1,3,3) C -> 1 and the ReLU in front of it
    Nc, Hc, Wc, Cc = 2, 9, 11, 32

    def make_c1():
        g = _gen(911)
        return dict(y=F.relu(torch.randn(Nc, Cc, 1, Hc, Wc, generator=g)), dz=torch.randn(Nc, Hc, Wc, generator=g),
                    w=torch.randn(1, Cc, 1, 3, 3, generator=g) / math.sqrt(9 * Cc))

    def ref_c1(t):
        y, dz, w = t["y"].double(), t["dz"].double()[:, None, None], t["w"].double()
        d = torch.nn.grad.conv3d_input(y.shape, w, dz, padding=(0, 1, 1))
        return {"d": torch.where(y > 0, d, torch.zeros_like(d)), "dW": torch.nn.grad.conv3d_weight(y, w.shape, dz, padding=(0, 1, 1)),
                "db": dz.sum().view(1)}

    def run_c1(E, dev, t):
        d, dW, db = E.conv_c1_bwd(_cl(E, t["y"], dev), t["dz"].to(dev), t["w"])
        return {"d": d.as_ncdhw(), "dW": dW, "db": db}

    _case("conv_c1_bwd-dz", "mspi_conv_c1_bwd", make_c1, [("dz", (0, 4, 5))], ref_c1, run_c1, tol=2e-5)
    _case("conv_c1_bwd-y", "mspi_conv_c1_bwd", make_c1, [("y", (0, 3, 0, 4, 5))], ref_c1, run_c1, tol=2e-5)

    for k in (2, 4, 8):
        def make_ub(k=k):
            return dict(dy=torch.randn(2, 8, 1, 3 * k, 4 * k, generator=_gen(k)))

        def ref_ub(t, k=k):
            x = torch.zeros(2, 8, 1, 3, 4, dtype=torch.float64, requires_grad=True)
            y = F.interpolate(x, scale_factor=(1, k, k), mode="trilinear", align_corners=False)
            return {"dx": torch.autograd.grad(y, x, t["dy"].double())[0]}

        _case("upsample_bwd-k%d-dy" % k, "mspi_upsample_bwd", make_ub, [("dy", (0, 3, 0, k + 1, 2 * k))], ref_ub,
              lambda E, dev, t, k=k: {"dx": E.upsample_bwd(_cl(E, t["dy"], dev), k).as_ncdhw()}, tol=2e-5)

    # weight gradients: the narrow kernel on (1,3,3) 32 -> 12, the wide one on (1,3,3) 64 -> 32
    for wide, (Ci, Co, shape) in ((False, (32, 12, (2, 1, 9, 11))), (True, (64, 32, (2, 3, 5, 9)))):
        kk, pad = (1, 3, 3), (0, 1, 1)

        def make_wg(Ci=Ci, Co=Co, shape=shape):
            g = _gen(Ci + Co)
            n, tt, h, w = shape
            return dict(x=torch.randn(n, Ci, tt, h, w, generator=g), dy=torch.randn(n, Co, tt, h, w, generator=g))

        def ref_wg(t, Ci=Ci, Co=Co):
            return {"dW": torch.nn.grad.conv3d_weight(t["x"].double(), (Co, Ci) + kk, t["dy"].double(), padding=pad),
                    "db": t["dy"].double().sum((0, 2, 3, 4))}

        def run_wg(E, dev, t, wide=wide, Ci=Ci, Co=Co):
            pk = E.pack_conv(torch.zeros(Co, Ci, *kk), torch.zeros(Co), None, (1, 1, 1), pad, E.ACT_NONE, device=dev)
            dW, db = (E.conv_wgrad_wide if wide else E.conv_wgrad)(_cl(E, t["x"], dev), _cl(E, t["dy"], dev), pk)
            return {"dW": dW, "db": db}

        for op, idx in (("x", (0, 5, 0, 2, 3)), ("dy", (0, 7, 0, 2, 3))):
            _case("conv_wgrad%s-%s" % ("_wide" if wide else "", op), "mspi_conv_wgrad_wide_fwd" if wide else "mspi_conv_wgrad_fwd",
                  make_wg, [(op, idx)], ref_wg, run_wg, tol=2e-5)

    # BatchNorm on batch statistics: M = 600 rows (two workgroup records) x 64 channels
    shape = (2, 64, 3, 10, 10)

    def make_bn():
        g = _gen(600)
        x = torch.randn(*shape, generator=g) * 2 + 0.5
        return dict(x=x, dy=torch.randn(*shape, generator=g), gamma=torch.rand(64, generator=g) + 0.5, beta=torch.randn(64, generator=g) * 0.3,
                    mean=x.mean((0, 2, 3, 4)), rstd=1.0 / torch.sqrt(x.var((0, 2, 3, 4), unbiased=False) + 1e-5))

    def ref_stats(t):
        _, mean, var, rstd = RR.bn_forward(t["x"].double(), t["gamma"].double(), t["beta"].double())
        return {"mean": mean, "var": var, "rstd": rstd}

    def run_stats(E, dev, t):
        return dict(zip(("mean", "var", "rstd"), E.bn_stats(_cl(E, t["x"], dev), eps=1e-5)))

    _case("bn_stats-x", "mspi_bn_stats", make_bn, [("x", (0, 3, 1, 2, 3))], ref_stats, run_stats, tol=2e-5)
    _case("bn_stats-x-second-record", "mspi_bn_stats", make_bn, [("x", (1, 5, 2, 9, 9))], ref_stats, run_stats, tol=2e-5)

    def ref_apply(t):
        v = lambda a: a.double().view(1, -1, 1, 1, 1)
        return {"y": F.relu(v(t["gamma"]) * (t["x"].double() - v(t["mean"])) * v(t["rstd"]) + v(t["beta"]))}

    def run_apply(E, dev, t):
        out = _sentinel(E, shape[0], *shape[2:], 64, dev)
        E.bn_apply(_cl(E, t["x"], dev), *[t[k].to(dev) for k in ("mean", "rstd", "gamma", "beta")], act=RELU, out=out)
        return {"y": out.as_ncdhw()}

    _case("bn_apply-relu-x", "mspi_bn_apply", make_bn, [("x", (0, 3, 1, 2, 3))], ref_apply, run_apply, tol=2e-5)
    _case("bn_apply-relu-mean", "mspi_bn_apply", make_bn, [("mean", (3,))], ref_apply, run_apply, tol=2e-5)

    def ref_bwd(t):
        d = {k: v.double() for k, v in t.items()}
        dx, dgamma, dbeta = RR.bn_backward(d["dy"], d["x"], d["mean"], d["rstd"], d["gamma"], torch.ones_like(d["dy"]))
        return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta}

    def run_bwd(E, dev, t):
        dx, dgamma, dbeta = E.bn_bwd(_cl(E, t["dy"], dev), _cl(E, t["x"], dev), *[t[k].to(dev) for k in ("mean", "rstd", "gamma")])
        return {"dx": dx.as_ncdhw(), "dgamma": dgamma, "dbeta": dbeta}

    _case("bn_bwd-dy", "mspi_bn_bwd", make_bn, [("dy", (0, 3, 1, 2, 3))], ref_bwd, run_bwd, tol=2e-5)

    # the training criterion: per-sample terms and the gradient of the loss
    import sal_loss_restate as S
    B, Hs, Ws = 3, 33, 31

    def make_sl():
        x, g, f = (torch.from_numpy(a) for a in S.make_case(B, Hs, Ws, 5))
        return dict(x=x, g=g, f=f)

    def run_sl_fwd(E, dev, t):
        from mspi_amd import metrics as M
        return {"terms": M.sal_loss_terms(t["x"].to(dev), t["g"].to(dev), t["f"].to(dev))}

    def run_sl_bwd(E, dev, t):
        from mspi_amd import metrics as M
        xg = t["x"].to(dev).requires_grad_(True)
        M.SalLoss()(xg, t["g"].to(dev), t["f"].to(dev)).backward()
        return {"grad": xg.grad}

    _case("saliency_loss_fwd-x", "mspi_saliency_loss_fwd", make_sl, [("x", (1, 7, 9))], lambda t: {"terms": S.terms(t["x"], t["g"], t["f"])},
          run_sl_fwd, tol=2e-5)
    _case("saliency_loss_bwd-x", "mspi_saliency_loss_bwd", make_sl, [("x", (1, 7, 9))], lambda t: {"grad": S.loss_grad(t["x"], t["g"], t["f"])},
          run_sl_bwd, tol=2e-5)


for _family in (_conv_cases, _gemm_sp_cases, _mlp_cases, _x3d_cases, _dw_cases, _norm_cases, _attn_cases, _rowop_cases, _sink_cases,
                _train_cases):
    _family()
BY_NAME = {c.name: c for c in CASES}
CASE_IDS = ["%s:%s" % (c.name, p) for c in CASES for p in POISONS]
CASE_PARAMS = [(c.name, p) for c in CASES for p in POISONS]

_REFS = {}


def _reference(name, poison):
    """(operands, {output: float64 reference}) of one case and poison, evaluated once and left unchanged."""
    if (name, poison) not in _REFS:
        case = BY_NAME[name]
        t = case.operands(POISONS[poison])
        _REFS[(name, poison)] = (t, {k: v.detach() for k, v in case.ref(t).items()})
    return _REFS[(name, poison)]


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_every_entry_point_is_classified():
    from mspi_amd import _lib
    names = set(_lib.EXPORTS)
    both = set(NONFINITE_LEDGER) & set(NONFINITE_EXCLUDED)
    assert not both, "classified twice: %s" % sorted(both)
    missing = names - set(NONFINITE_LEDGER) - set(NONFINITE_EXCLUDED)
    assert not missing, "entry points without a non-finite classification (add cases, or exclude with a reason): %s" % sorted(missing)
    stale = (set(NONFINITE_LEDGER) | set(NONFINITE_EXCLUDED)) - names
    assert not stale, "classified, but no entry point: %s" % sorted(stale)
    assert all(isinstance(r, str) and len(r) > 10 for r in NONFINITE_EXCLUDED.values())
    # mspi_logspec_fwd has its own test below (its bar and its silent columns are those of test_logspec_kernel.py)
    covered = {e for c in CASES for e in c.entries} | {"mspi_logspec_fwd"}
    assert covered == set(NONFINITE_LEDGER), "ledger entries without a case / cases outside the ledger: %s" % sorted(covered ^ set(NONFINITE_LEDGER))
    assert len(BY_NAME) == len(CASES), "two cases share a name"


def test_exception_list_is_pinned():
    assert set(B_EXCEPTIONS) == B_EXCEPTION_KEYS
    assert all(name in BY_NAME and poison in POISONS for name, poison in B_EXCEPTIONS)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_reference_of_the_poisoned_input_is_not_vacuous(name):
    """(a) asserts something: the NaN poison reaches at least one output of the float64 reference; (b) asserts something: a
    local case keeps at least one finite output.  An Inf may be absorbed by the operation itself (max, ReLU, a softmax weight of
    exactly 0): the reference is then finite there and (b) pins the kernel to the same value."""
    case = BY_NAME[name]
    _, ref = _reference(name, "nan")
    bad = sum(int((~torch.isfinite(v)).sum()) for v in ref.values())
    fin = sum(int(torch.isfinite(v).sum()) for v in ref.values())
    assert bad > 0, "the poison reaches no output"
    assert (fin > 0) == case.local, "local = %s, but %d finite outputs" % (case.local, fin)
    clean = case.ref(case.make())
    assert all(torch.isfinite(v).all() for v in clean.values()), "the clean operands already give a non-finite reference"


def test_oracle_map_of_a_poisoned_input_is_all_nan(golden_dir):
    """The log-softmax over a sample's map makes any surviving poison global in that sample: oracle.restate on the 64-pixel
    X3D-L case returns an all-NaN map for the poisoned sample under each poison of the model-level test and finite maps for the
    other samples, so "raises, or every element of the poisoned sample's map is non-finite" is what torch does."""
    import test_oracle_golden as OG
    from oracle import restate as R
    g = np.load(os.path.join(golden_dir, "av_x3dl_64.npz"))
    cfg, sd, clips, audio = OG._model(g, "x3dl", "AudioVisualSaliencyModel")
    for what in MODEL_POISONS:
        c, a, n = _poison_inputs(clips.clone(), audio.clone(), what)
        with torch.no_grad():
            out, _ = R.audio_visual_forward(sd, c, a, "x3dl", cfg.MODEL.LATERAL_BOOL, cfg.MODEL.LATERAL_STRIDE)
        assert out.shape[0] > 1 and torch.isnan(out[n]).all(), what
        assert all(torch.isfinite(out[i]).all() for i in range(out.shape[0]) if i != n), what


# ------------------------------------------------------------------------------------------------------------ GPU tests
def _holds(case, poison, got, ref, flag, reach):
    """(a) and (b) of the module docstring for one run; `reach`: where the NaN poison's reference is non-finite."""
    name = "%s %s" % (case.name, poison)
    exempt = (case.name, poison) in B_EXCEPTIONS
    for key, r in ref.items():
        g = got[key].detach().cpu()
        assert tuple(g.shape) == tuple(r.shape), "%s %s: shape %s, reference %s" % (name, key, tuple(g.shape), tuple(r.shape))
        if case.sink == "u8":
            continue
        g = g.double()
        bad = ~torch.isfinite(r)
        lost = bad & torch.isfinite(g)
        print("%s %s: %d of %d reference outputs non-finite, %d of them finite in the kernel, flag %s"
              % (name, key, int(bad.sum()), bad.numel(), int(lost.sum()), flag))
        assert flag or not lost.any(), "(a) %s %s: %d outputs finite (first %s = %g) where the reference is not, and no flag" \
            % (name, key, int(lost.sum()), tuple(lost.nonzero()[0].tolist()), g[lost][0].item())
        fin = ~bad & ~reach[key] if exempt else ~bad
        if exempt:      # an exception that is no longer needed leaves the list
            assert (~bad & ~torch.isfinite(g)).any(), "%s: listed in B_EXCEPTIONS, but finite wherever the reference is" % name
        if not fin.any():
            continue
        leaked = fin & ~torch.isfinite(g)
        assert not leaked.any(), "(b) %s %s: %d non-finite outputs (first %s) where the reference is finite" \
            % (name, key, int(leaked.sum()), tuple(leaked.nonzero()[0].tolist()))
        assert not (g[fin] == SENTINEL).any() or (r[fin] == SENTINEL).any(), "(b) %s %s: outputs left unwritten" % (name, key)
        err = (g - r).abs()[fin]
        if case.elementwise:
            assert (err <= case.tol * r.abs()[fin]).all(), "(b) %s %s: worst %.3e |ref|" % (name, key, (err / r.abs()[fin]).max().item())
        else:
            scale = r[fin].abs().max().item()
            print("%s %s: finite outputs within %.2e of max|finite ref| (bar %.0e)" % (name, key, err.max().item() / max(scale, 1e-300), case.tol))
            assert err.max().item() <= case.tol * scale, "(b) %s %s: max abs err %.3e, %.1e of max|finite ref| %.3e" \
                % (name, key, err.max().item(), err.max().item() / max(scale, 1e-300), scale)


@pytest.mark.gpu
@pytest.mark.parametrize("name,poison", CASE_PARAMS, ids=CASE_IDS)
def test_kernel_propagates_or_flags(dev, name, poison):
    from mspi_amd import engine as E
    KL._no_switches(KL.SWITCHES + GL.SWITCHES + RL.SWITCHES)
    case = BY_NAME[name]
    t, ref = _reference(name, poison)
    reach = {k: ~torch.isfinite(v) for k, v in _reference(name, "nan")[1].items()}
    _guard(E, dev)
    got = case.run(E, dev, t)
    torch.cuda.synchronize()
    flag = E.range_flag()
    if case.sink == "u8":
        _holds_u8(E, dev, case, poison, got["u8"].cpu(), ref["u8"], t, flag)
    _holds(case, poison, got, ref, flag, reach)


def _holds_u8(E, dev, case, poison, got, ref, t, flag):
    """The u8 sink: a map whose float64 resize holds a non-finite value must raise the flag; every other map of the batch is
    byte-identical to the same map run alone, and within the cap of test_rowop_ledger.py of the float64 pipeline."""
    bad = [i for i in range(ref.shape[0]) if not torch.isfinite(ref[i]).all()]
    print("postprocess_u8 %s: maps %s non-finite in float64, flag %s" % (poison, bad, flag))
    assert flag or not bad, "(a) postprocess_u8 %s: map %s is not finite, the u8 output cannot say so, and no flag" % (poison, bad)
    for i in range(ref.shape[0]):
        if i in bad:
            continue
        want = RL._pp_f64(t["maps"][i], PP_CASE[3:])
        d = (got[i].int() - want.int()).abs()
        assert d.max() <= 1 and (d > 0).float().mean() < 0.02, "(b) postprocess_u8 %s: map %d off by %d levels" % (poison, i, int(d.max()))
        alone = E.postprocess_u8(t["maps"][i:i + 1].to(dev), PP_CASE[3:]).cpu()
        assert torch.equal(alone[0], got[i]), "(b) map %d of the poisoned batch differs from the same map run alone" % i
    torch.cuda.synchronize()
    E.range_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", list(POISONS))
def test_logspec_propagates_or_flags(dev, poison):
    """One poisoned wave sample: the frames whose 512-sample window holds it are non-finite (the flag is not involved: the
    kernel is no GEMM); every other frame, every other window and the pad columns stay inside test_logspec_kernel.py's bar."""
    import logspec_restate as LS
    import test_logspec_kernel as TL
    from mspi_amd import engine as E
    from mspi_amd import preproc as P
    Wa = LS.WAS[0]
    wave = TL._wave().clone()
    at = 8000      # inside six of the windows, outside the attenuated and the silent stretch
    assert not LS.SILENCE[0] <= at < LS.SILENCE[1] and not LS.ATTENUATED[0] <= at < LS.ATTENUATED[1]
    wave[at] = POISONS[poison]
    _guard(E, dev)
    out = P.log_spectrogram(wave.to(dev), list(LS.WINDOWS), Wa).cpu()
    torch.cuda.synchronize()
    flag = E.range_flag()
    hit = 0
    for i, (st, ln, rev) in enumerate(LS.WINDOWS):
        ref, std = LS.log_spectrogram_window(wave, st, ln, bool(rev), Wa)
        bad = ~torch.isfinite(ref)
        hit += int(bad.sum())
        lost = bad & torch.isfinite(out[i].double())
        assert flag or not lost.any(), "(a) logspec %s window %d: %d finite outputs where the reference is not" % (poison, i, int(lost.sum()))
        cols = ~(std < TL.LOW_STD) & ~torch.isnan(std) & ~bad.any(0).any(0)
        n = TL._nframes(ln, Wa)
        assert torch.isfinite(out[i][:, :, cols]).all() and (out[i][:, :, n:] == LS.PAD).all()
        if cols.any():
            err = (out[i].double() - ref)[:, :, cols].abs().max().item()
            assert err <= TL.BAR, "(b) logspec %s window %d: max abs err %.3e" % (poison, i, err)
    assert hit > 0, "the poison reaches no frame of the reference"


# ---------------------------------------------------------------------------------------------------------- whole models
MODEL_POISONS = ("nan-corner-pixel", "+inf-mid-pixel", "nan-spectrogram-bin")


def _poison_inputs(clips, audio, what):
    """(clips, audio, index of the poisoned sample)"""
    if what == "nan-corner-pixel":
        clips[0, 0, 0, 0, 0] = float("nan")      # corner of frame 0: only padding-adjacent taps see it
        return clips, audio, 0
    if what == "+inf-mid-pixel":
        clips[-1, 1, clips.shape[2] // 2, clips.shape[3] // 2, clips.shape[4] // 2] = float("inf")
        return clips, audio, clips.shape[0] - 1
    audio[(0,) * (audio.dim() - 2) + (audio.shape[-2] // 2, audio.shape[-1] // 2)] = float("nan")
    return clips, audio, 0


def _av(case, name, cls="AudioVisualSaliencyModel"):
    def build(dev, golden_dir):
        import test_parity_gpu as PG
        g = PG._g(golden_dir, case)
        cfg, m, clips, audio = PG._build(g, name, cls, dev)
        visual = cls == "VisualSaliencyModel"
        fwd = (lambda c, a: m(c)[0]) if visual else (lambda c, a: m(c, a)[0])
        # the golden check of test_parity_gpu.py: max abs error of the log map below MAP_TOL
        return fwd, clips, None if visual else audio, lambda out: (out.cpu() - torch.as_tensor(g["out"])).abs().max().item() / PG.MAP_TOL
    return build


def _x3d_alone(dev, golden_dir):
    import test_parity_gpu as PG
    from mspi_amd import testing as T
    from mspi_amd.backbones.X3D import X3D
    from mspi_amd.config import cfg
    g = PG._g(golden_dir, "x3dl_backbone_64")
    m = T.seeded(lambda: X3D(cfg.MODEL.X3D.PATH_CFG), int(g["seed"])).to(dev)
    clips, _ = T.synth_inputs(int(g["batch"]), 16, int(g["size"]), int(g["size"]), seed=int(g["seed"]), device=dev)
    return (lambda c, a: m([c])[3]), clips, None, lambda out: T.feature_error(out, g, "v4") / 1e-4


def _resnet_alone(dev, golden_dir):
    import test_parity_gpu as PG
    from mspi_amd import testing as T
    from mspi_amd.backbones.resnet import ResNet
    g = PG._g(golden_dir, "resnet18_audio_111")
    m = T.seeded(ResNet, int(g["seed"])).to(dev)
    _, audio = T.synth_inputs(int(g["batch"]), Wa=111, H=8, W=8, seed=int(g["seed"]), device=dev)
    return (lambda c, a: m(a)), None, audio, lambda out: PG._relerr(out, g["out"]) / 1e-4


MODELS = {"av_x3dl_64": _av("av_x3dl_64", "x3dl"), "av_slowfast_64": _av("av_slowfast_64", "slowfast4x16"), "av_s3d_64": _av("av_s3d_64", "s3d"),
          "av_uniformer_64": _av("av_uniformer_64", "uniformerb"), "x3d_backbone_64": _x3d_alone,
          "vis_x3dl_64": _av("vis_x3dl_64", "x3dl", "VisualSaliencyModel"), "resnet18_audio": _resnet_alone,
          "av_mvit_224": _av("av_mvit_224", "mvitv2s"), "av_swin_s_224": _av("av_swin_s_224", "videoswins"),
          "av_morphmlp_224": _av("av_morphmlp_224", "morphmlps")}


@pytest.mark.gpu
@pytest.mark.parametrize("tuned", [False, True], ids=["untuned", "first-sight"])
@pytest.mark.parametrize("model", list(MODELS))
def test_model_never_returns_a_finite_map_without_the_flag(dev, golden_dir, model, tuned):
    """A poisoned clip pixel or spectrogram bin: engine.check_range() raises, or every element of the poisoned sample's output
    is non-finite (what the oracle's log-softmax gives, pinned on the CPU above).  The two backbones alone end in no softmax;
    the same rule holds for them because X3D's squeeze-excite pooling spreads a poison over its whole sample and the
    receptive field of every ResNet-18 output covers the whole spectrogram.  First-sight
    tuned: _range_check sees amax != amax and moves the layer to the fp32 path, which holds the contract just the same;
    pk.checked / pk.prec of a moved layer may stay moved.  Afterwards the flag is clear and a clean forward of the same model
    still matches its golden: no poison is left in a pack, a workspace or a cached decision."""
    from mspi_amd import engine as E
    fwd, clips, audio, golden_err = MODELS[model](dev, golden_dir)      # golden_err: the error as a fraction of test_parity_gpu.py's bar
    _guard(E, dev)
    moved, cache, attn = len(E.RANGE_CHECK["moved"]), dict(E.AUTOTUNE["cache"]), dict(E.ATTN_PREC)
    try:
        E.autotune(tuned)
        for what in MODEL_POISONS:
            if (audio if what == "nan-spectrogram-bin" else clips) is None:
                continue
            c, a, n = _poison_inputs(None if clips is None else clips.clone(), None if audio is None else audio.clone(), what)
            with torch.no_grad():
                out = fwd(c, a)
            raised = False
            try:
                E.check_range()
            except E.MspiError:
                raised = True
            finite = int(torch.isfinite(out[n]).sum())
            print("%s %s %s: check_range raised %s, %d of %d outputs of sample %d finite, %d layers moved to fp32 so far"
                  % (model, "tuned" if tuned else "untuned", what, raised, finite, out[n].numel(), n, len(E.RANGE_CHECK["moved"]) - moved))
            assert raised or finite == 0, "%s: sample %d has %d finite values and no flag" % (what, n, finite)
            assert not E.range_flag(), "check_range left the flag up"
        E.autotune(False)
        with torch.no_grad():      # with whatever the poisoned forwards left in the packs and in the tuning cache
            out = fwd(clips, audio)
        E.check_range()
    finally:
        E.autotune(False)
        del E.RANGE_CHECK["moved"][moved:]
        E.AUTOTUNE["cache"].clear()
        E.AUTOTUNE["cache"].update(cache)
        E.ATTN_PREC.clear()
        E.ATTN_PREC.update(attn)
    err = golden_err(out)
    assert err < 1.0, "clean forward after the poisoned ones: %.2f of the golden bar" % err
