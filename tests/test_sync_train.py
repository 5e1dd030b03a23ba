"""trainable(..., sync=True): the SyncBlock and the contrastive head train beside the stage ladder -- csrc/contrast_bwd.hip
(mspi_neg_cosine_bwd, mspi_layernorm_act_bwd, mspi_mean_rows_bwd, declared in include/mspi_contrast_train_hip.h), their engine
wrappers, autograd.ContrastHead, the data gradients of autograd.LateralEntry, the keyword of model.trainable and --sync of
mspi_amd.train.

Yardsticks: tests/golden/contrast_head.npz holds "tiny" (B = 1, one visual and one audio token) with the float64 loss_av, the
slab's gradient and the 36 tensors' gradients that torch autograd gives through torch.nn layers with upstream's arguments
(tools/gen_contrast_golden.py; each dW, rank one at one row, as db and its other factor), and the seed of "odd" (B = 2, 6 visual
and 5 audio tokens); tests/contrast_restate.py is the float64 restatement in this project's order with its analytic backward,
pinned to that fixture and, here, to torch autograd on "odd".  The SyncBlock's 39 gradients in the whole model are judged
against tests/sync_tokens_restate.py, fed the run's own v4, audio map and slab gradient.

Bounds.  Every tensor: max |got - ref| / max |ref| <= GRAD_TOL = 2e-5, the project's bar for gradients
(tests/test_readout_train.py); every test prints its figure before it asserts.  The kernels are chains of fp32 fmaf and
shuffle trees over at most 2048 terms, about 1e-7 of sum |a b|; the condition on the inputs -- torch FLOAT32 autograd on the CPU
at least ten times under the bar against float64 on every case used here -- is asserted by
test_cases_are_well_conditioned_in_fp32, so the bar cannot hide a badly conditioned case (p and z are drawn with row norms of
order 1, LayerNorm inputs with a per-row spread of order 1)."""
import contextlib
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import contrast_restate as CR
import sync_block_restate as SR
import sync_tokens_restate as TR
from test_adapter_train import BN_NAMES
from test_adapter_train import _trained_names as _adapter_trained_names
from test_entry_train import MODELS as ENTRY_MODELS
from test_entry_train import _trained_names as _entry_trained_names
from test_fusion_train import _declared, _judge, _poisoned, _replayed, _stream
from test_readout_train import GRAD_TOL
from test_sync_block_train import _judge_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_neg_cosine_bwd", "mspi_layernorm_act_bwd_ws_bytes", "mspi_layernorm_act_bwd", "mspi_mean_rows_bwd")
OLDER_HEADERS = ("mspi_hip.h", "mspi_train_hip.h", "mspi_block_train_hip.h", "mspi_entry_train_hip.h", "mspi_adapter_train_hip.h",
                 "mspi_sync_train_hip.h", "mspi_linear_train_hip.h")
LN_ROWS = 8                                       # rows per record of mspi_layernorm_act_bwd
COS_CASES = [(1, 4), (2, 2048), (5, 516)]         # (N, C)
LN_CASES = [(1, 512), (2, 2048), (3, 1028), (LN_ROWS + 1, 516)]      # (M, C); the last: just above one record's rows
MEAN_CASES = [(1, 1, 512), (2, 7, 512)]           # (N, R, C)
ENTRY_SHAPES = [(1, 4, 1, 3), (2, 5, 2, 3)]       # (B, T, h, w)
ENTRY_STRIDES = (1, 2, 4)
ENTRY_C, ENTRY_C2, ENTRY_EXTRA = 24, 512, 5       # x 24 wide; x2 the first Rv rows of a [B, Rv + 5, 512] slab
HEAD_CASES = {"tiny": (1, 1, 1), "odd": (2, 6, 5)}      # (B, Rv, Ra)
AV_MODELS = [m for m in ENTRY_MODELS if m[2] == "AudioVisualSaliencyModel"]
SYNC_COUNTS = {"aud_vis_sync_block.": 39, "vis_projector.": 12, "mlp_vis.": 6, "aud_projector.": 12, "mlp_aud.": 6}
COS_SCALE, COS_G = 0.5, 0.7


def _rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).double().cpu()
    return (got - ref).abs().max().item() / ref.abs().max().item()


# ------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def _cos_case(shape):
    """fp32 p, z [N, C] with row norms of order 1 and the float64 dp for g = 0.7, scale 0.5; computed once."""
    N, C = shape
    gen = torch.Generator().manual_seed(9100 + N + C)
    p, z = torch.randn(N, C, generator=gen) / C ** 0.5, torch.randn(N, C, generator=gen) / C ** 0.5
    return p, z, CR.neg_cosine_bwd(p.double(), z.double(), COS_G, COS_SCALE)


@functools.lru_cache(maxsize=None)
def _ln_case(shape):
    """fp32 x (per-row spread 1 around a per-row offset), dy, gamma, the forward's ReLU output y in fp32 from float64, and the
    float64 (dx, dgamma, dbeta) with and without the mask; computed once."""
    M, C = shape
    gen = torch.Generator().manual_seed(9200 + M + C)
    x = torch.randn(M, C, generator=gen) + torch.randn(M, 1, generator=gen)
    dy = torch.randn(M, C, generator=gen)
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    y = torch.relu(CR.layernorm(x.double(), gamma.double(), beta.double())).float()
    return x, dy, gamma, beta, y, {True: CR.layernorm_act_bwd(dy.double(), x.double(), gamma.double(), y.double()),
                                   False: CR.layernorm_act_bwd(dy.double(), x.double(), gamma.double())}


@functools.lru_cache(maxsize=None)
def _mean_case(shape):
    N, R, C = shape
    gen = torch.Generator().manual_seed(9300 + N + R + C)
    return torch.randn(N, C, generator=gen), torch.randn(N, R, C, generator=gen)      # g, what dx holds under accumulate


def _entry_grads(c, dtype):
    """(dx, dx2) of G . conv(s,1,1)/s(conv1x1x1([x | x2])) from torch's conv3d autograd."""
    import torch.nn.functional as F
    B, T, h, w = c["shape"]
    Rv = T * h * w
    xin = torch.cat([c["x"], c["slab"][:, :Rv].reshape(B, T, h, w, ENTRY_C2)], -1).to(dtype).permute(0, 4, 1, 2, 3).requires_grad_(True)
    y = F.conv3d(F.conv3d(xin, c["w0"].to(dtype), c["b0"].to(dtype)), c["w1"].to(dtype), stride=(c["s"], 1, 1))
    y.backward(c["G"].to(dtype).permute(0, 4, 1, 2, 3))
    d = xin.grad.permute(0, 2, 3, 4, 1)
    return d[..., :ENTRY_C], d[..., ENTRY_C:]


@functools.lru_cache(maxsize=None)
def _entry_case(s, shape):
    B, T, h, w = shape
    gen = torch.Generator().manual_seed(9400 + 10 * s + T)
    cin = ENTRY_C + ENTRY_C2
    c = {"s": s, "shape": shape, "x": torch.randn(B, T, h, w, ENTRY_C, generator=gen),
         "slab": torch.randn(B, T * h * w + ENTRY_EXTRA, ENTRY_C2, generator=gen),
         "w0": torch.randn(192, cin, 1, 1, 1, generator=gen) / cin ** 0.5, "b0": 0.1 * torch.randn(192, generator=gen),
         "w1": torch.randn(192, 192, s, 1, 1, generator=gen) / (192 * s) ** 0.5, "G": torch.randn(B, T // s, h, w, 192, generator=gen)}
    c["ref"] = _entry_grads(c, torch.float64)
    return c


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "contrast_head.npz"))
    return {k: z[k] for k in z.files}


def _gold_grad(k):
    g = _gold()
    if k.split(".")[-1].startswith("w"):
        return np.outer(g["tiny.%s" % k.replace(".w", ".b")], g["tiny.%s.v" % k])
    return g["tiny.%s" % k]


@functools.lru_cache(maxsize=None)
def _head(key):
    """(case, float64 loss, float64 gradients by "slab" and CR.NAMES) of the restatement; computed once."""
    B, Rv, Ra = HEAD_CASES[key]
    case = CR.make_case(B, Rv, Ra, int(_gold()[key + ".shape"][-1]))
    loss, grads = CR.backward(case)
    return case, loss, grads


# ------------------------------------------------------------------------------------------------------------- CPU
def test_contrast_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    from mspi_amd import engine as E
    declared, _ = _declared("mspi_contrast_train_hip.h")
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert declared == set(NEW_SYMBOLS) == set(_lib.CONTRAST_EXPORTS) == set(_lib._CONTRAST_SIGNATURES)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _lib._CONTRAST_SIGNATURES[name][1], name
    older = set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.BLOCK_EXPORTS) | set(_lib.ENTRY_EXPORTS) | \
        set(_lib.ADAPTER_EXPORTS) | set(_lib.SYNC_EXPORTS) | set(_lib.LINEAR_EXPORTS)
    for header in OLDER_HEADERS:
        older |= _declared(header)[0]
    assert not older & set(NEW_SYMBOLS)
    base, base_text = _declared("mspi_hip.h")
    assert base == set(_lib.EXPORTS)
    assert re.search(r"#define MSPI_ABI_VERSION 2\b", base_text) and lib.mspi_version() == 2
    for name in ("neg_cosine_bwd", "layernorm_act_bwd", "mean_rows_bwd"):
        assert callable(getattr(E, name)) and name in E.__all__
    assert E.LN_ACT_BWD_ROWS == LN_ROWS and E.LN_ACT_BWD_MAX_CH == 2048
    src = open(os.path.join(ROOT, "mspi_amd", "csrc", "contrast_bwd.hip")).read()
    assert "atomic" not in src.lower()
    mk = open(os.path.join(ROOT, "mspi_amd", "csrc", "Makefile")).read()
    assert "contrast_bwd.hip" in mk and mk.count("mspi_contrast_train_hip.h") == 2 and "-fno-slp-vectorize" in mk


def test_host_refusals():
    from mspi_amd import _lib
    lib = _lib.load()

    def err():
        return lib.mspi_last_error().decode()

    # ---- mspi_neg_cosine_bwd
    base = dict(p=4096, z=8192, g=12288, dp=16384, N=3, C=8)

    def cos(**kw):
        a = dict(base, **kw)
        return lib.mspi_neg_cosine_bwd(a["p"], a["z"], a["g"], a["dp"], a["N"], a["C"], 0.5, None), err()
    for name in ("p", "z", "g", "dp"):
        rc, why = cos(**{name: None})
        assert rc == -1 and "mspi_neg_cosine_bwd: null argument" in why, (name, rc, why)
    for name, off in (("p", 4), ("z", 4), ("dp", 8), ("g", 2)):
        rc, why = cos(**{name: base[name] + off})
        assert rc == -1 and "mspi_neg_cosine_bwd" in why and "aligned" in why, (name, rc, why)
    for text, kw in {"multiple of 4": dict(C=6), "multiple of 4 ": dict(C=0), "multiple of 4  ": dict(C=-4), "no rows": dict(N=0),
                     "no rows ": dict(N=-2)}.items():
        rc, why = cos(**kw)
        assert rc == -1 and "mspi_neg_cosine_bwd: " in why and text.strip() in why, (text, rc, why)

    # ---- mspi_layernorm_act_bwd: the launch and the workspace size refuse the same extents
    base = dict(x=4096, ldx=16, dy=8192, lddy=16, y=12288, ldy=16, gamma=16384, dx=20480, lddx=16, dgamma=24576, dbeta=28672,
                ws=32768, M=5, C=16)

    def ln(**kw):
        a = dict(base, **kw)
        rc = lib.mspi_layernorm_act_bwd(a["x"], a["ldx"], a["dy"], a["lddy"], a["y"], a["ldy"], a["gamma"], 1e-5, a["dx"], a["lddx"],
                                        a["dgamma"], a["dbeta"], a["ws"], a["M"], a["C"], None)
        return rc, err()
    for name in ("x", "dy", "gamma", "dx", "dgamma", "dbeta", "ws"):      # y may be NULL: no mask
        rc, why = ln(**{name: None})
        assert rc == -1 and "mspi_layernorm_act_bwd: null argument" in why, (name, rc, why)
    for name in ("x", "dy", "y", "gamma", "dx", "dgamma", "dbeta", "ws"):
        rc, why = ln(**{name: base[name] + 4})
        assert rc == -1 and "mspi_layernorm_act_bwd" in why and "16-byte aligned" in why, (name, rc, why)
    wide = dict(ldx=2052, lddy=2052, ldy=2052, lddx=2052)
    shapes = {"multiple of 4": dict(C=18, ldx=20, lddy=20, ldy=20, lddx=20), "C <= 2048": dict(C=2052, **wide), "0 < C": dict(C=0),
              "no rows": dict(M=0), "no rows ": dict(M=-3), "2^31": dict(M=1 << 31), "2^31 ": dict(M=(1 << 31) + 9)}
    for text, kw in shapes.items():
        rc, why = ln(**kw)
        assert rc == -1 and "mspi_layernorm_act_bwd: " in why and text.strip() in why, (text, rc, why)
        a = dict(base, **kw)
        assert lib.mspi_layernorm_act_bwd_ws_bytes(a["M"], a["C"]) == 0, text
    for name in ("ldx", "lddy", "ldy", "lddx"):
        for bad, text in ((12, ">= C"), (18, "multiples of 4")):
            rc, why = ln(**{name: bad})
            assert rc == -1 and "mspi_layernorm_act_bwd: " in why and text in why, (name, bad, rc, why)
    for M, C in [(1, 4), (LN_ROWS, 2048), (LN_ROWS + 1, 516), (11472, 512), ((1 << 31) - 1, 2048)]:
        assert lib.mspi_layernorm_act_bwd_ws_bytes(M, C) == -(-M // LN_ROWS) * 2 * C * 4, (M, C)

    # ---- mspi_mean_rows_bwd
    base = dict(g=4096, dx=8192, ldx=16, ss=16 * 7, N=2, R=7, C=16)

    def mean(**kw):
        a = dict(base, **kw)
        return lib.mspi_mean_rows_bwd(a["g"], a["dx"], a["ldx"], a["ss"], a["N"], a["R"], a["C"], 0, None), err()
    for name in ("g", "dx"):
        rc, why = mean(**{name: None})
        assert rc == -1 and "mspi_mean_rows_bwd: null argument" in why, (name, rc, why)
        rc, why = mean(**{name: base[name] + 4})
        assert rc == -1 and "mspi_mean_rows_bwd" in why and "16-byte aligned" in why, (name, rc, why)
    for text, kw in {"multiple of 4": dict(C=18, ldx=20, ss=140), "multiple of 4 ": dict(C=0), "0 < N < 65536": dict(N=0),
                     "0 < N < 65536 ": dict(N=65536), "no rows": dict(R=0), "no rows ": dict(R=-1), ">= C": dict(ldx=12),
                     "row stride must be a multiple of 4": dict(ldx=18), ">= R * ldx": dict(ss=16 * 6),
                     "sample stride must be a multiple of 4": dict(ss=114)}.items():
        rc, why = mean(**kw)
        assert rc == -1 and "mspi_mean_rows_bwd: " in why and text.strip() in why, (text, rc, why)


def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["names"]) == tuple(sorted(HEAD_CASES)) and tuple(g["grads"]) == ("slab",) + CR.NAMES and len(CR.NAMES) == 36
    for c, (B, Rv, Ra) in HEAD_CASES.items():
        assert tuple(g[c + ".shape"][:-1]) == (B, Rv, Ra)
    assert g["tiny.slab"].shape == (1, 2, 512) and g["tiny.slab"].dtype == np.float64 and g["tiny.loss"].shape == ()
    case = _head("tiny")[0]
    for k in CR.NAMES:
        assert _gold_grad(k).shape == case[k].shape and _gold_grad(k).dtype == np.float64, k
    assert not any(k.startswith("odd.") and k != "odd.shape" for k in g)          # "odd" is its seed
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "contrast_head.npz")) < 1 << 20


def test_restatement_matches_the_fixture():
    case, loss, grads = _head("tiny")
    g = _gold()
    assert abs(loss.item() - float(g["tiny.loss"])) <= 1e-12 * abs(float(g["tiny.loss"]))
    assert CR.rel_err(grads["slab"], g["tiny.slab"]) <= 1e-12
    for k in CR.NAMES:
        assert CR.rel_err(grads[k], _gold_grad(k)) <= 1e-12, k


def test_restatement_matches_torch_autograd_on_odd():
    """ "odd" is stored as its seed: torch.nn layers with upstream's arguments, float64, built here."""
    case, loss, grads = _head("odd")
    ref_loss, ref = CR.upstream_grads(case)
    assert abs(loss.item() - ref_loss.item()) <= 1e-12 * abs(ref_loss.item())
    assert sorted(ref) == sorted(grads) and len(ref) == 37
    for k in ref:
        assert CR.rel_err(grads[k], ref[k]) <= 1e-12, k
    # the embeddings enter the loss as constants: a head whose predictions are detached instead has no gradient at all
    assert all(grads[k].abs().max() > 0 for k in grads)


def test_cases_are_well_conditioned_in_fp32():
    """torch FLOAT32 autograd on the CPU against float64, on every case the GPU tests use: at least ten times under the bar."""
    import torch.nn.functional as F
    worst = {}

    def note(what, got, ref):
        worst[what] = max(worst.get(what, 0.0), _rel(got, ref))
    for shape in COS_CASES:
        p, z, ref = _cos_case(shape)
        leaf = p.clone().requires_grad_(True)
        (-COS_SCALE * F.cosine_similarity(leaf, z, dim=-1).mean() * COS_G).backward()
        note("neg_cosine_bwd %s" % (shape,), leaf.grad, ref)
    for shape in LN_CASES:
        x, dy, gamma, beta, y, refs = _ln_case(shape)
        for masked in (True, False):
            leaf, gm, bt = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
            out = F.layer_norm(leaf, (shape[1],), gm, bt, CR.EPS)
            (torch.relu(out) if masked else out).backward(dy)
            for name, got, ref in zip(("dx", "dgamma", "dbeta"), (leaf.grad, gm.grad, bt.grad), refs[masked]):
                note("layernorm_act_bwd %s mask=%s %s" % (shape, masked, name), got, ref)
    for shape in MEAN_CASES:
        g, _ = _mean_case(shape)
        leaf = torch.zeros(shape, requires_grad=True)
        leaf.mean(1).backward(g)
        note("mean_rows_bwd %s" % (shape,), leaf.grad, CR.mean_rows_bwd(g.double(), shape[1]))
    for s in ENTRY_STRIDES:
        for shape in ENTRY_SHAPES:
            c = _entry_case(s, shape)
            for name, got, ref in zip(("dx", "dx2"), _entry_grads(c, torch.float32), c["ref"]):
                note("LateralEntry s=%d %s %s" % (s, shape, name), got, ref)
    for key in HEAD_CASES:
        case, loss, grads = _head(key)
        l32, g32 = CR.upstream_grads(case, dtype=torch.float32)
        note("ContrastHead %s loss" % key, l32, loss)
        for k in grads:
            note("ContrastHead %s d %s" % (key, k), g32[k], grads[k])
    for what, e in sorted(worst.items(), key=lambda kv: -kv[1])[:8]:
        print("torch fp32 vs float64, %s: %.2e" % (what, e))
    bad = {k: e for k, e in worst.items() if not e <= GRAD_TOL / 10}
    assert not bad, bad


def _sync_names(m):
    from mspi_amd import autograd as A
    return sorted(n for n, _ in m.named_parameters() if n.startswith(A.SYNC_PREFIXES))


@pytest.mark.parametrize("name,total", [("x3dl", 182), ("s3d", 180), ("slowfast4x16", 178)])
def test_trainable_sync_flags_modes_refusals_and_restore(name, total):
    from mspi_amd import autograd as A
    from mspi_amd import testing as T
    from mspi_amd._lib import MspiError
    from mspi_amd.model import model_utils as pm
    assert A.SYNC_PREFIXES == tuple(SYNC_COUNTS) and A.STAGE_NAMES[-1] == "adapter" and len(A.STAGE_NAMES) == 6
    m = T.seeded(lambda: pm.AudioVisualSaliencyModel(T.make_cfg(name)), 0)
    first = next(m.visnet.parameters())
    first.requires_grad_(False)
    before = {n: p.requires_grad for n, p in m.named_parameters()}

    def on():
        return sorted(n for n, p in m.named_parameters() if p.requires_grad)
    sync = _sync_names(m)
    assert len(sync) == 75 and {p: sum(n.startswith(p) for n in sync) for p in SYNC_COUNTS} == SYNC_COUNTS
    assert [n for n, _ in m.named_parameters() if n.startswith(("vis_projector.", "mlp_vis.", "aud_projector.", "mlp_aud."))] == \
        ["%s_projector.%s" % (s, t[10:]) if t.startswith("projector") else "mlp_%s.%s" % (s, t[4:]) for s in ("vis", "aud")
         for t in A.CONTRAST_TENSORS]
    state = dict(m.named_parameters())
    head = [n for n in state if n.startswith(A.SYNC_PREFIXES[1:])]
    assert len(head) == 36 and all(t is state[n] for t, n in zip(m._contrast_tensors(), head))
    assert m.trainable("adapter", sync=True) is m
    full = on()
    assert full == sorted(_adapter_trained_names(m) + sync) and len(full) == total
    assert not any(p.requires_grad for mod in (m.visnet, m.image_encoder, m.audnet) for p in mod.parameters())
    # no module gains a mode: frozen_encoder() leaves exactly the adapter stage's BatchNorm layers in train()
    m.train()
    m.frozen_encoder()
    assert sorted(n for n, s in m.named_modules() if s.training) == BN_NAMES and sorted(m._batch_stat_modules()) == BN_NAMES
    m._check_eval()
    assert m._training_tail() == "cat"
    with torch.no_grad():
        assert m._training_tail() is False
    m.trainable("adapter")                                      # a plain stage and back
    assert on() == _adapter_trained_names(m) and m._training_tail() == "cat"
    m.trainable("lateral_entries", sync=True)
    assert on() == sorted(_entry_trained_names(m) + sync) and len(on()) == total - 24 and m._training_tail() == "inputs"
    if name == "x3dl":
        assert len(on()) == 158
    m.trainable("adapter", sync=True)
    assert on() == full
    for low in ("readout_tail", "readout", "fusion", "lateral_blocks"):
        with pytest.raises(MspiError, match="trainable\\('%s', sync=True\\): the SyncBlock reaches the map only through latlayer_3's "
                                            "entry conv.*'lateral_entries' or 'adapter'" % low):
            m.trainable(low, sync=True)
        assert on() == full
    with pytest.raises(MspiError, match="trainable\\(None, sync=True\\): the SyncBlock reaches"):
        m.trainable(None, sync=True)
    with pytest.raises(MspiError, match="'lateral_entries' and 'adapter' are"):
        m.trainable("sync", sync=True)
    assert on() == full
    m.trainable(None)
    assert {n: p.requires_grad for n, p in m.named_parameters()} == before and not first.requires_grad
    assert m._training_tail() is False
    if name == "x3dl":
        v = T.seeded(lambda: pm.VisualSaliencyModel(T.make_cfg(name)), 0)
        flags = {n: p.requires_grad for n, p in v.named_parameters()}
        with pytest.raises(MspiError, match="trainable\\('adapter', sync=True\\): VisualSaliencyModel has neither a SyncBlock"):
            v.trainable("adapter", sync=True)
        assert {n: p.requires_grad for n, p in v.named_parameters()} == flags and v._training_tail() is False


def test_train_accepts_sync_up_to_the_gpu_check(monkeypatch):
    from mspi_amd import train
    from mspi_amd._lib import MspiError
    assert train.TRAINABLE_ADAPTER == ("adapter",)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for stage in ("adapter", "lateral_entries"):
        with pytest.raises(SystemExit, match="MI355X"):
            train.main(["--trainable", stage, "--sync"])
    for stage in ("readout", "readout_tail", "fusion", "lateral_blocks"):
        with pytest.raises(MspiError, match="--sync with --trainable %s: .*lateral_entries or adapter" % stage):
            train.main(["--trainable", stage, "--sync"])
    with pytest.raises(MspiError, match="--sync with --no_sound"):
        train.main(["--trainable", "adapter", "--sync", "--no_sound"])
    assert train.build_parser().parse_args([]).sync is False
    doc = train.__doc__
    assert "Still frozen in all six: the SyncBlock, the contrastive projectors and every encoder" in doc and "--sync" in doc


# ------------------------------------------------------------------------------------------------------------- GPU, kernels
def _cos_launch(dev, p, z, g=COS_G, static=None):
    """mspi_neg_cosine_bwd on dense p, z [N, C]; dp into a NaN-filled buffer with 64 cells to spare."""
    from mspi_amd import _lib
    lib = _lib.load()
    N, C = p.shape
    t = static if static is not None else {"p": p.contiguous().to(dev), "z": z.contiguous().to(dev),
                                            "g": torch.full((1,), g, device=dev)}
    buf = torch.full((N * C + 64,), float("nan"), device=dev)
    _lib.check(lib.mspi_neg_cosine_bwd(t["p"].data_ptr(), t["z"].data_ptr(), t["g"].data_ptr(), buf.data_ptr(), N, C, COS_SCALE,
                                       _stream()), "mspi_neg_cosine_bwd")
    return buf[:N * C].view(N, C), buf


@pytest.mark.gpu
@pytest.mark.parametrize("shape", COS_CASES, ids=lambda s: "x".join(map(str, s)))
def test_hip_neg_cosine_bwd_vs_fp64(dev, shape):
    from mspi_amd import engine as E
    p, z, ref = _cos_case(shape)
    dp, buf = _cos_launch(dev, p, z)
    torch.cuda.synchronize()
    _judge_grad("neg_cosine_bwd %s" % (shape,), dp, ref)
    assert torch.isnan(buf[p.numel():]).all()
    assert torch.equal(_cos_launch(dev, p, z)[0], dp), "two runs differ"
    # the engine wrapper makes the same launch
    pc, zc = E.from_rows(p.to(dev)), E.from_rows(z.to(dev))
    got = E.neg_cosine_bwd(pc, zc, torch.full((1,), COS_G, device=dev), COS_SCALE)
    assert torch.equal(got.as_rows(), dp)
    # rows below the clamp keep only the first term: |p| = 0 gives -g scale / N z / (1e-8 |z|)
    p0 = p.clone()
    p0[0] = 0.0
    dp0, _ = _cos_launch(dev, p0, z)
    _judge_grad("neg_cosine_bwd %s, a zero row" % (shape,), dp0, CR.neg_cosine_bwd(p0.double(), z.double(), COS_G, COS_SCALE))


def _ln_launch(dev, x, dy, y, gamma, pad=0, alias=False, static=None):
    """mspi_layernorm_act_bwd on x, dy, y [M, C] (y None: no mask): dense with pad = 0; otherwise each a column range, 4 columns
    in, of a NaN-filled [M + 2][C + pad] buffer.  alias: dx is dy.  dgamma and dbeta are written into NaN-filled rows with 8 cells
    to spare.  Returns (dx, dgamma, dbeta, (the whole dx buffer, the whole dgamma | dbeta buffer))."""
    from mspi_amd import _lib
    lib = _lib.load()
    M, C = x.shape

    def place(t, name):
        if static is not None:
            return static[name], C
        if not pad:
            return t.contiguous().to(dev), C
        buf = torch.full((M + 2, C + pad), float("nan"), device=dev)
        buf[:M, 4:4 + C] = t.to(dev)
        return buf[:, 4:], C + pad
    xs, ldx = place(x, "x")
    ds, lddy = place(dy, "dy")
    ys, ldy = place(y, "y") if y is not None else (None, 0)
    gm = static["gamma"] if static is not None else gamma.contiguous().to(dev)
    if alias:
        dxs, lddx, whole = ds, lddy, None
    else:
        whole = torch.full((M + 2, C + pad), float("nan"), device=dev)
        dxs, lddx = whole[:, 4 if pad else 0:], C + pad
    dgb = torch.full((2, C + 8), float("nan"), device=dev)
    ws = torch.empty(lib.mspi_layernorm_act_bwd_ws_bytes(M, C) // 4, device=dev)
    assert ws.numel() == -(-M // LN_ROWS) * 2 * C
    _lib.check(lib.mspi_layernorm_act_bwd(xs.data_ptr(), ldx, ds.data_ptr(), lddy, None if ys is None else ys.data_ptr(), ldy,
                                          gm.data_ptr(), CR.EPS, dxs.data_ptr(), lddx, dgb[0].data_ptr(), dgb[1].data_ptr(),
                                          ws.data_ptr(), M, C, _stream()), "mspi_layernorm_act_bwd")
    return dxs[:M, :C], dgb[0, :C], dgb[1, :C], (whole, dgb)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("shape", LN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_hip_layernorm_act_bwd_vs_fp64(dev, shape, masked):
    from mspi_amd import engine as E
    M, C = shape
    x, dy, gamma, beta, y, refs = _ln_case(shape)
    rdx, rdg, rdb = refs[masked]
    ym = y if masked else None
    print("layernorm_act_bwd (%d, %d): %d record(s), %d of %d cells under the mask" % (M, C, -(-M // LN_ROWS), int((y <= 0).sum()) if masked else 0, M * C))
    first = None
    for pad, alias in ((0, False), (12, False), (12, True), (0, True)):
        what = "layernorm_act_bwd (%d, %d) %s%s%s" % (M, C, "relu" if masked else "plain", ", in wider buffers" if pad else "", ", dx over dy" if alias else "")
        dx, dg, db, (whole, dgb) = _ln_launch(dev, x, dy, ym, gamma, pad, alias)
        torch.cuda.synchronize()
        _judge_grad(what + " dx", dx, rdx)
        _judge_grad(what + " dgamma", dg, rdg)
        _judge_grad(what + " dbeta", db, rdb)
        assert torch.isnan(dgb[:, C:]).all()
        if whole is not None:                      # every cell of dx written and nothing else
            keep = torch.ones_like(whole, dtype=torch.bool)
            keep[:M, (4 if pad else 0):(4 if pad else 0) + C] = False
            assert torch.isnan(whole[keep]).all() and torch.isfinite(whole[~keep]).all()
        if first is None:
            first = (dx.clone(), dg.clone(), db.clone())
        else:                                      # where the operands lie, and dx over dy, change nothing
            assert torch.equal(dx, first[0]) and torch.equal(dg, first[1]) and torch.equal(db, first[2]), what
    xc, dc, yc = (E.from_rows(t.to(dev)) for t in (x, dy, y))
    dx, dg, db = E.layernorm_act_bwd(dc, xc, gamma.to(dev), CR.EPS, y=yc if masked else None)
    assert torch.equal(dx.as_rows(), first[0]) and torch.equal(dg, first[1]) and torch.equal(db, first[2])
    dx2, _, _ = E.layernorm_act_bwd(dc, xc, gamma.to(dev), CR.EPS, y=yc if masked else None, inplace=True)
    assert dx2 is dc and torch.equal(dc.as_rows(), first[0])


def _mean_launch(dev, g, prev, accumulate, static=None):
    """mspi_mean_rows_bwd into rows [3, 3 + R) of a NaN-filled [N][12][C + 8] slab (under accumulate those rows hold prev)."""
    from mspi_amd import _lib
    lib = _lib.load()
    N, R, C = prev.shape
    slab = torch.full((N, 12, C + 8), float("nan"), device=dev)
    if accumulate:
        slab[:, 3:3 + R, :C] = static["prev"] if static is not None else prev.to(dev)
    gd = static["g"] if static is not None else g.contiguous().to(dev)
    view = slab[:, 3:, :]
    _lib.check(lib.mspi_mean_rows_bwd(gd.data_ptr(), view.data_ptr(), C + 8, 12 * (C + 8), N, R, C, 1 if accumulate else 0, _stream()),
               "mspi_mean_rows_bwd")
    return slab[:, 3:3 + R, :C], slab


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("shape", MEAN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_hip_mean_rows_bwd_vs_fp64(dev, shape, accumulate):
    from mspi_amd import engine as E
    N, R, C = shape
    g, prev = _mean_case(shape)
    ref = CR.mean_rows_bwd(g.double(), R) + (prev.double() if accumulate else 0.0)
    dx, slab = _mean_launch(dev, g, prev, accumulate)
    torch.cuda.synchronize()
    _judge_grad("mean_rows_bwd %s accumulate=%s" % (shape, accumulate), dx, ref)
    outside = torch.ones_like(slab, dtype=torch.bool)
    outside[:, 3:3 + R, :C] = False
    assert torch.isnan(slab[outside]).all()                    # rows (and columns) outside the range are not touched
    assert torch.equal(_mean_launch(dev, g, prev, accumulate)[0], dx)
    # the engine wrapper on a token view of a [N, 12, C] slab
    buf = torch.full((N, 12, C), float("nan"), device=dev)
    if accumulate:
        buf[:, 3:3 + R] = prev.to(dev)
    E.mean_rows_bwd(g.to(dev), E.CL(buf.view(-1), 0, N, 12, 1, 1, C, C).tokens(3, R, 1, 1), accumulate=accumulate)
    assert torch.equal(buf[:, 3:3 + R], dx) and torch.isnan(buf[:, :3]).all() and torch.isnan(buf[:, 3 + R:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_hip_contrast_kernels_nonfinite_operands_propagate(dev, value):
    from mspi_amd import engine as E
    E._need_gpu(torch.empty(1, device=dev))

    def flagged(launch):
        E.range_flag()
        out = launch()
        torch.cuda.synchronize()
        return out, E.range_flag()
    # ---- neg_cosine_bwd: a poisoned row of p or z stays in its row of dp; g reaches every row
    p, z, _ = _cos_case((5, 516))
    for name, idx in (("p", (1, 3)), ("z", (4, 515)), ("g", None)):
        ops = {"p": p, "z": z}
        g = COS_G
        if name == "g":
            g = value
        else:
            ops[name] = _poisoned(ops[name], idx, value)
        ref = CR.neg_cosine_bwd(ops["p"].double(), ops["z"].double(), g, COS_SCALE)
        (dp, _), flag = flagged(lambda: _cos_launch(dev, ops["p"], ops["z"], g))
        assert flag, "neg_cosine_bwd %s: a poisoned output did not set the status word" % name
        _judge("neg_cosine_bwd %s -> dp" % name, dp, ref)
        bad = ~torch.isfinite(dp.cpu())
        assert bad.all() if name == "g" else (bad[idx[0]].all() and int(bad.sum()) == p.shape[1]), name
    # ---- layernorm_act_bwd
    x, dy, gamma, beta, y, _ = _ln_case((3, 1028))
    lit = int(torch.argmax(y[1]))                              # a cell the ReLU lets through: its dy counts
    for name, idx in (("x", (2, 5)), ("dy", (1, lit)), ("y", (1, lit)), ("gamma", (lit,))):
        ops = {"x": x, "dy": dy, "y": y, "gamma": gamma}
        ops[name] = _poisoned(ops[name], idx, value)
        rdx, rdg, rdb = CR.layernorm_act_bwd(ops["dy"].double(), ops["x"].double(), ops["gamma"].double(), ops["y"].double())
        (dx, dg, db, _), flag = flagged(lambda: _ln_launch(dev, ops["x"], ops["dy"], ops["y"], ops["gamma"], 12))
        what = "layernorm_act_bwd %s" % name
        if name == "y" and value == float("inf"):              # +Inf in y is a cell the ReLU lets through: finite everywhere
            assert not flag
            for k, got, ref in (("dx", dx, rdx), ("dgamma", dg, rdg), ("dbeta", db, rdb)):
                _judge_grad("%s (+Inf) -> %s" % (what, k), got, ref)
            continue
        assert flag, "%s: a poisoned output did not set the status word" % what
        _judge(what + " -> dx", dx, rdx)
        bad = ~torch.isfinite(dx.cpu())
        if name == "gamma":                                    # every row of dx, and neither dgamma nor dbeta
            assert bad.all()
            _judge_grad(what + " -> dgamma (independent)", dg, rdg)
            _judge_grad(what + " -> dbeta (independent)", db, rdb)
        else:                                                  # its own row of dx
            assert bad[idx[0]].all() and int(bad.sum()) == x.shape[1]
            _judge(what + " -> dgamma", dg, rdg)
            if name == "x":                                    # every column of dgamma and never dbeta
                assert (~torch.isfinite(dg.cpu())).all()
                _judge_grad(what + " -> dbeta (independent)", db, rdb)
            else:                                              # its own column of both
                _judge(what + " -> dbeta", db, rdb)
                assert int((~torch.isfinite(dg.cpu())).sum()) == 1 and int((~torch.isfinite(db.cpu())).sum()) == 1
    # ---- mean_rows_bwd: g[n, c] reaches column c of sample n's rows; what dx holds under accumulate its own cell
    g, prev = _mean_case((2, 7, 512))
    bad_g = _poisoned(g, (1, 9), value)
    (dx, _), flag = flagged(lambda: _mean_launch(dev, bad_g, prev, True))
    assert flag
    _judge("mean_rows_bwd g -> dx", dx, CR.mean_rows_bwd(bad_g.double(), 7) + prev.double())
    assert int((~torch.isfinite(dx.cpu())).sum()) == 7
    bad_prev = _poisoned(prev, (0, 6, 511), value)
    (dx, _), flag = flagged(lambda: _mean_launch(dev, g, bad_prev, True))
    assert flag
    _judge("mean_rows_bwd dx (accumulate) -> dx", dx, CR.mean_rows_bwd(g.double(), 7) + bad_prev.double())
    assert int((~torch.isfinite(dx.cpu())).sum()) == 1
    # clean operands leave the status word alone
    (dp, _), f1 = flagged(lambda: _cos_launch(dev, p, z))
    (dx, dg, db, _), f2 = flagged(lambda: _ln_launch(dev, x, dy, y, gamma, 12))
    (dm, _), f3 = flagged(lambda: _mean_launch(dev, g, prev, True))
    assert not (f1 or f2 or f3) and all(torch.isfinite(t).all() for t in (dp, dx, dg, db, dm))


@pytest.mark.gpu
def test_hip_contrast_kernels_capture_and_replay(dev):
    gen = torch.Generator().manual_seed(78)
    p, z, _ = _cos_case((5, 516))
    other = {"p": torch.randn(5, 516, generator=gen) / 23.0, "z": torch.randn(5, 516, generator=gen) / 23.0, "g": torch.tensor([-1.3])}

    def cos(t, host):
        return {"dp": _cos_launch(dev, p, z, static=t)[0]}
    _replayed(dev, {"A": {"p": p, "z": z, "g": torch.tensor([COS_G])}, "B": other}, cos)

    x, dy, gamma, beta, y, _ = _ln_case((LN_ROWS + 1, 516))
    other = {"x": torch.randn(x.shape, generator=gen), "dy": torch.randn(x.shape, generator=gen),
             "y": torch.relu(torch.randn(x.shape, generator=gen)), "gamma": torch.randn(516, generator=gen)}

    def ln(t, host):
        dx, dg, db, _ = _ln_launch(dev, x, dy, y, gamma, static=t)
        return {"dx": dx, "dgamma": dg, "dbeta": db}
    _replayed(dev, {"A": {"x": x, "dy": dy, "y": y, "gamma": gamma}, "B": other}, ln)

    g, prev = _mean_case((2, 7, 512))
    other = {"g": torch.randn(g.shape, generator=gen), "prev": torch.randn(prev.shape, generator=gen)}

    def mean(t, host):
        return {"dx": _mean_launch(dev, g, prev, True, static=t)[0]}
    _replayed(dev, {"A": {"g": g, "prev": prev}, "B": other}, mean)


# ------------------------------------------------------------------------------------------------------------- GPU, Functions
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ENTRY_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("s", ENTRY_STRIDES)
def test_hip_lateral_entry_data_gradients(dev, s, shape):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    E.autotune(False)
    c = _entry_case(s, shape)
    B, T, h, w = shape
    Rv = T * h * w

    def run(inputs):
        x = c["x"].to(dev).requires_grad_(inputs)
        slab = c["slab"].to(dev).requires_grad_(inputs)
        ps = [c[k].to(dev).requires_grad_(True) for k in ("w0", "b0", "w1")]
        x2 = slab[:, :Rv].view(B, T, h, w, ENTRY_C2)           # a token view into the slab, read where it lies
        y = A.LateralEntry.apply(x, x2, *ps)
        with E.Profiler() as prof:
            y.backward(c["G"].to(dev))
        return y.detach(), x.grad, slab.grad, [p.grad for p in ps], [r[0] for r in prof.records]
    y, dx, dslab, dws, names = run(True)
    y0, none, none2, dws0, names0 = run(False)
    assert none is None and none2 is None and torch.equal(y0, y)
    # with detached inputs nothing more is launched than the weight gradients need, and they keep their bits
    assert all(torch.equal(a, b) for a, b in zip(dws, dws0)) and names[-len(names0):] == names0 and len(names) > len(names0)
    print("LateralEntry s=%d %s: backward launches %s" % (s, shape, names))
    _judge_grad("LateralEntry s=%d %s dx" % (s, shape), dx, c["ref"][0])
    _judge_grad("LateralEntry s=%d %s dx2" % (s, shape), dslab[:, :Rv].reshape(B, T, h, w, ENTRY_C2), c["ref"][1])
    assert not dslab[:, Rv:].any()                             # the view's backward: the rows behind the visual tokens get zeros
    live = T // s * s
    if live < T:                                               # frames no output reads: exactly zero
        assert not dx[:, live:].any() and not dslab[:, :Rv].reshape(B, T, h, w, ENTRY_C2)[:, live:].any()
        assert not c["ref"][0][:, live:].any()
    if (T, s) == (5, 2):
        assert live == 4
    again = run(True)
    assert torch.equal(again[1], dx) and torch.equal(again[2], dslab)
    # each input's gradient only when it is asked for
    x = c["x"].to(dev)
    slab = c["slab"].to(dev).requires_grad_(True)
    ps = [c[k].to(dev) for k in ("w0", "b0", "w1")]
    A.LateralEntry.apply(x, slab[:, :Rv].view(B, T, h, w, ENTRY_C2), *ps).backward(c["G"].to(dev))
    assert torch.equal(slab.grad, dslab)


def _head_modules(case, dev):
    """vis_projector, mlp_vis, aud_projector, mlp_aud as AudioVisualSaliencyModel builds them, holding the case's tensors."""
    import torch.nn as nn
    h = CR.HIDDEN

    def projector():
        return nn.Sequential(nn.Linear(CR.DIM, h), nn.LayerNorm(h), nn.ReLU(inplace=True), nn.Linear(h, h), nn.LayerNorm(h),
                             nn.ReLU(inplace=True), nn.Linear(h, h), nn.LayerNorm(h))

    def predictor():
        return nn.Sequential(nn.Linear(h, 512), nn.LayerNorm(512), nn.ReLU(), nn.Linear(512, h))
    mods = [projector(), predictor(), projector(), predictor()]
    params = [p for m in mods for p in m.parameters()]
    assert len(params) == len(CR.NAMES)
    with torch.no_grad():
        for p, k in zip(params, CR.NAMES):
            p.copy_(torch.from_numpy(case[k]))
    return [m.to(dev) for m in mods]


def _inference_loss(mods, slab, Rv, dev):
    """loss_av as AudioVisualSaliencyModel._sync_and_lateral3 launches it on a slab: the method itself on a stand-in that hands
    it the slab in the SyncBlock's place, with the plan built layer by layer as AudioVisualSaliencyModel._pack builds it."""
    from mspi_amd import engine as E
    from mspi_amd.model import model_utils as pm
    B, R, D = slab.shape
    x = E.CL(slab.detach().contiguous().view(-1), 0, B, R, 1, 1, D, D)

    def f(t):
        return t.detach().float().contiguous()

    def lin_ln(lin, ln):
        return E.pack_conv(lin.weight, lin.bias), f(ln.weight), f(ln.bias)
    pk = {}
    for name, pr, ml in (("vis", mods[0], mods[1]), ("aud", mods[2], mods[3])):
        pk[name] = [lin_ln(pr[0], pr[1]), lin_ln(pr[3], pr[4]), lin_ln(pr[6], pr[7]), lin_ln(ml[0], ml[1]),
                    E.pack_conv(ml[3].weight, ml[3].bias)]

    class Fork:
        def keep(self, t):
            pass

        @contextlib.contextmanager
        def branch(self, i, refork=False):
            yield
    stand_in = types.SimpleNamespace(aud_vis_sync_block=types.SimpleNamespace(run=lambda v, a: x), _lateral=lambda *a, **k: None,
                                     _embed=pm.AudioVisualSaliencyModel._embed)
    v4, aud = E.CL(x.buf, 0, B, Rv, 1, 1, 8, 8), E.CL(x.buf, 0, B, R - Rv, 1, 1, D, D)    # only their extents and device are read
    with torch.no_grad():
        _, loss = pm.AudioVisualSaliencyModel._sync_and_lateral3(stand_in, pk, v4, aud, Fork())
    return loss


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(HEAD_CASES))
def test_hip_contrast_head_end_to_end(dev, key, monkeypatch):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    E.autotune(False)
    monkeypatch.setitem(E.AUTOTUNE, "cache", {})
    case, ref_loss, ref = _head(key)
    B, Rv, Ra = HEAD_CASES[key]
    mods = _head_modules(case, dev)
    params = [p for m in mods for p in m.parameters()]

    def run(wrt=None, slab_grad=True):
        for p, k in zip(params, CR.NAMES):
            p.grad = None
            p.requires_grad_(wrt is None or k in wrt)
        slab = torch.from_numpy(case["slab"]).float().to(dev).requires_grad_(slab_grad)
        loss = A.ContrastHead.apply(slab, Rv, *params)
        assert loss.dim() == 0 and loss.requires_grad
        with E.Profiler() as prof:
            loss.backward()
        return loss.detach(), slab.grad, {k: p.grad for p, k in zip(params, CR.NAMES)}, [r[0] for r in prof.records]
    loss, dslab, grads, names = run()
    print("ContrastHead %s: backward launches %s" % (key, names))
    # the bits of the inference path's second return on the same modules and slab
    want = _inference_loss(mods, torch.from_numpy(case["slab"]).float().to(dev), Rv, dev)
    assert want.dim() == 0 and torch.equal(loss, want)
    e = abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())
    print("ContrastHead %s loss_av %.6f: %.2e" % (key, loss.item(), e))
    assert e <= GRAD_TOL
    if key == "tiny":
        e = abs(loss.item() - float(_gold()["tiny.loss"])) / abs(float(_gold()["tiny.loss"]))
        assert e <= GRAD_TOL
    _judge_grad("ContrastHead %s d slab" % key, dslab, _gold()["tiny.slab"] if key == "tiny" else ref["slab"])
    assert all(g is not None for g in grads.values()) and len(grads) == 36
    for k in CR.NAMES:
        _judge_grad("ContrastHead %s d %s" % (key, k), grads[k], _gold_grad(k) if key == "tiny" else ref[k])
    assert names.count("neg_cosine_bwd") == 2 and names.count("linear_wgrad") == 10 and names.count("layernorm_act_bwd") == 8 and \
        names.count("mean_rows_bwd") == 2
    # a second call gives the same bits
    loss2, dslab2, grads2, _ = run()
    assert torch.equal(loss2, loss) and torch.equal(dslab2, dslab) and all(torch.equal(grads2[k], grads[k]) for k in grads)
    # each gradient only when it is asked for: the chain stops behind the lowest layer that is
    for only, lins, lns in (("aud.w2", 1, 2), ("vis.e3", 0, 1), ("vis.b0", 1, 4)):
        l3, d3, g3, n3 = run(wrt=(only,), slab_grad=False)
        assert torch.equal(l3, loss) and d3 is None and torch.equal(g3[only], grads[only])
        assert all(g is None for k, g in g3.items() if k != only)
        assert (n3.count("neg_cosine_bwd"), n3.count("linear_wgrad"), n3.count("layernorm_act_bwd"), n3.count("mean_rows_bwd")) == \
            (1, lins, lns, 0), (only, n3)


@pytest.mark.gpu
def test_hip_contrast_head_refuses_by_name(dev):
    from mspi_amd import autograd as A
    from mspi_amd._lib import MspiError
    case = _head("tiny")[0]
    params = [p for m in _head_modules(case, dev) for p in m.parameters()]
    slab = torch.from_numpy(case["slab"]).float().to(dev)
    with pytest.raises(MspiError, match="GPU only"):
        A.ContrastHead.apply(slab.cpu(), 1, *[p.cpu() for p in params])
    with pytest.raises(MspiError, match=r"ContrastHead: slab must be fp32 \[B, Rv\+Ra, 512\]"):
        A.ContrastHead.apply(slab[0], 1, *params)
    with pytest.raises(MspiError, match="0 < Rv = 2 < Rv\\+Ra"):
        A.ContrastHead.apply(slab, 2, *params)
    with pytest.raises(MspiError, match="expected 36 tensors"):
        A.ContrastHead.apply(slab, 1, *params[:-1])
    with pytest.raises(MspiError, match=r"ContrastHead: aud mlp.0.weight is \(2048, 512\)"):
        A.ContrastHead.apply(slab, 1, *params[:30], params[34], *params[31:])
    leaf = slab.clone().requires_grad_(True)
    gx, = torch.autograd.grad(A.ContrastHead.apply(leaf, 1, *params), leaf, create_graph=True)
    with pytest.raises(RuntimeError):       # no double backward: the gradient carries no graph, or one that refuses
        torch.autograd.grad(gx.sum(), leaf)


# ------------------------------------------------------------------------------------------------------------- GPU, whole model
@pytest.mark.gpu
@pytest.mark.parametrize("case,name,cls,entries_total", AV_MODELS, ids=[m[0] for m in AV_MODELS])
def test_hip_whole_model_trains_its_sync_block_and_contrastive_head(dev, golden_dir, monkeypatch, case, name, cls, entries_total):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    from mspi_amd import metrics as M
    from mspi_amd.model import model_utils as pm
    from test_readout_tail import _batches, _build
    total = entries_total + 24 + 75
    E.autotune(False)          # bits are compared, and an empty cache pins the library's own kernel choices
    monkeypatch.setitem(E.AUTOTUNE, "cache", {})
    g, cfg, make, clips, audio = _build(golden_dir, case, name, cls, dev)
    m = make().to(dev)
    off, off_loss = m(clips, audio)
    label = _batches(clips, audio, 1, True)[0][2].to(dev)
    sync = _sync_names(m)
    stage = _adapter_trained_names(m)
    # 1. the switch on under no_grad: the launches of inference, both outputs with the switch-off bits
    m.trainable("adapter", sync=True)
    m.train()
    m.frozen_encoder()
    with torch.no_grad():
        quiet, quiet_loss = m(clips, audio)
    assert torch.equal(quiet, off) and torch.equal(quiet_loss, off_loss) and not quiet.requires_grad and not quiet_loss.requires_grad

    def grads_of():
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    # the same stage without sync: the map and the older gradients to compare with
    m.trainable("adapter")
    for p in m.parameters():
        p.grad = None
    plain, plain_loss = m(clips, audio)
    assert plain.requires_grad and not plain_loss.requires_grad and torch.equal(plain_loss, off_loss)
    M.SalLoss()(plain, label).backward()
    plain_grads = grads_of()
    assert sorted(plain_grads) == stage
    m.trainable("adapter", sync=True)
    calls = []

    def recorded(module, vis, aud):
        slab = A.sync_block(module, vis, aud)
        rec = {"vis": vis.detach().clone(), "aud": aud.detach().clone()}
        slab.register_hook(lambda gr, rec=rec: rec.__setitem__("G", gr.detach().clone()))
        calls.append(rec)
        return slab
    monkeypatch.setattr(pm, "sync_block", recorded)

    def step_grads():
        for p in m.parameters():
            p.grad = None
        out, loss_av = m(clips, audio)
        assert out.requires_grad and loss_av.requires_grad and loss_av.dim() == 0
        (M.SalLoss()(out, label) + loss_av).backward()
        return out.detach().clone(), loss_av.detach().clone(), grads_of()
    start = {k: v.clone() for k, v in m.state_dict().items()}
    params = [p for p in m.parameters() if p.requires_grad]
    assert len(params) == total
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0)
    out1, loss1, grads = step_grads()
    out2, loss2, grads2 = step_grads()
    monkeypatch.setattr(pm, "sync_block", A.sync_block)
    # 2. the map of the stage without sync, loss_av of the no-grad forward
    assert torch.equal(out1, plain.detach()) and torch.equal(loss1, off_loss)
    # 3. the stage's names plus the 75, finite, twice the same bits, the older gradients untouched by loss_av
    assert sorted(grads) == sorted(stage + sync) and len(grads) == total and len(calls) == 2
    assert all(torch.isfinite(gr).all() for gr in grads.values())
    assert torch.equal(out1, out2) and torch.equal(loss1, loss2) and all(torch.equal(grads2[n], grads[n]) for n in grads)
    assert all(torch.equal(grads[n], plain_grads[n]) for n in stage)
    # 4. the SyncBlock's 39 gradients against the float64 restatement, fed this very run's v4, audio map and slab gradient
    rec = calls[0]
    sb = m.aud_vis_sync_block
    B, t, h, w, C4 = rec["vis"].shape
    tc = {"B": B, "thw": (t, h, w), "C4": C4, "Rv": t * h * w, "Ra": rec["aud"].shape[1] * rec["aud"].shape[2] * rec["aud"].shape[3],
          "vis": rec["vis"].double().cpu().numpy(), "aud": rec["aud"].double().cpu().numpy(), "G": rec["G"].double().cpu().numpy(),
          "vpos": sb.vis_pos_embed[0].double().numpy(), "apos": sb.aud_pos_embed[0].double().numpy()}
    tc.update({k: start["aud_vis_sync_block." + n].double().cpu().numpy() for k, n in zip(TR.EMBED, A.SYNC_EMBED_TENSORS)})
    tc["blocks"] = [{k: start["aud_vis_sync_block.blocks.%d.%s" % (i, n)].double().cpu().numpy() for k, n in zip(SR.NAMES, A.BLOCK_TENSORS)}
                    for i in range(len(sb.blocks))]
    _, ref_e, ref_b = TR.backward(tc)
    print("%s: %d visual and %d audio tokens, C4 = %d" % (case, tc["Rv"], tc["Ra"], C4))
    for k, n in zip(TR.EMBED, A.SYNC_EMBED_TENSORS):
        _judge_grad("%s d aud_vis_sync_block.%s" % (case, n), grads["aud_vis_sync_block." + n], ref_e[k])
    for i in range(len(sb.blocks)):
        for k, n in zip(SR.NAMES, A.BLOCK_TENSORS):
            _judge_grad("%s d aud_vis_sync_block.blocks.%d.%s" % (case, i, n), grads["aud_vis_sync_block.blocks.%d.%s" % (i, n)], ref_b[i][k])
    # 5. an AdamW step moves every trained tensor whose gradient is not exactly zero; the no-grad forward uses the stepped values
    opt.step()
    moved = set(stage + sync) | {"%s.%s" % (mod, n) for mod in BN_NAMES for n in ("running_mean", "running_var", "num_batches_tracked")}
    still = {n for n in stage + sync if not grads[n].any()}
    print("%s: gradient exactly zero: %s" % (case, sorted(still)))
    assert still <= {"readout.12.bias"}                        # tests/test_entry_train.py says why that one IS zero
    for k, v in m.state_dict().items():
        assert torch.equal(v, start[k]) == (k not in moved - still), k
    with torch.no_grad():
        trained, trained_loss = m(clips, audio)
    assert not torch.equal(trained, off) and not torch.equal(trained_loss, off_loss)
    assert torch.isfinite(trained).all() and torch.isfinite(trained_loss)
    fresh = make()
    fresh.load_state_dict(m.state_dict())
    again, again_loss = fresh.to(dev)(clips, audio)
    assert torch.equal(again, trained) and torch.equal(again_loss, trained_loss)      # every pack followed its parameters
    m.trainable(None)
    m.eval()
    plain_map, plain_av = m(clips, audio)
    assert torch.equal(plain_map, trained) and torch.equal(plain_av, trained_loss) and not plain_map.requires_grad
