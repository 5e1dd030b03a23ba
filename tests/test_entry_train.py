"""The trainable entry convs of the laterals: csrc/entry_bwd.hip (mspi_conv_wgrad_entry and its three host companions, declared
in include/mspi_entry_train_hip.h), engine.conv_wgrad_entry / conv_wgrad_entry_variant, autograd.LateralEntry,
_SaliencyBase.trainable("lateral_entries"), mspi_amd.train --trainable lateral_entries.

Yardsticks: tests/golden/lateral_entry.npz holds "tiny" ((B, T, h, w) = (1, 2, 1, 2), C = 24, s = 2) with, in float64, the
output and the three gradients of <y, G> that torch autograd gives through nn.Conv3d(C, mid, 1) and
nn.Conv3d(mid, mid, (s,1,1), (s,1,1), bias=False) (tools/gen_lateral_entry_golden.py), and the seed and geometry of every
other case.  The STORED "tiny" is mid = 32 wide (at 192 the float64 gradient of the second conv alone is 590 KB, eight times
lateral_block.npz, which the fixture must not outgrow); from its seed "tiny" runs at 192 like every other case.
tests/lateral_entry_restate.py is the float64 restatement in this project's order -- compose, one conv, the chain rule through
the composition -- pinned to that fixture and, here, to torch autograd on "odd", "plain" (no second conv) and "split" (two inputs).

Bounds.  Every gradient tensor: max |got - ref| / max |ref| <= GRAD_TOL = 2e-5, the project's bar for gradients
(tests/test_readout_train.py); every test prints its figure before it asserts.  Torch FLOAT32 on the CPU agrees with float64,
worst of y and the gradients (tools/gen_lateral_entry_golden.py prints them): tiny 6.1e-7, odd 4.5e-7, tail 4.3e-7, s4 7.2e-7,
ragged112 7.2e-7, ragged44 6.2e-7, split 4.0e-7, plain 6.9e-7, widest 5.1e-7, slice 5.8e-7 -- the bar leaves a factor of 27
on the worst case, above ten on every one.  The layers have no nonlinearity: no kink caveats.  The "variants" cases are not in
the fixture (their float64 reference is computed here from a seed): 1024 and 32768 output rows, the smallest row counts of the
second and the third slice length; fp32 sums of that many products of standard normals stay below 1e-6 of the largest entry.

The ledger part holds the entry point to what tests/test_fusion_train.py holds its two: declared = exported = bound, capture +
replay with the operands and the host descriptor overwritten in between, and a NaN / +Inf in each floating operand reaching
every output that depends on it and no other."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import fusion_restate as FR
import lateral_entry_restate as ER
import lateral_restate as LR
import readout_restate as R
from test_fusion_train import BATCH_STAT, _declared, _judge, _poisoned, _replayed, _stream
from test_readout_train import GRAD_TOL, _cl, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_conv_wgrad_entry_supported", "mspi_conv_wgrad_entry_ws_bytes", "mspi_conv_wgrad_entry_variant",
               "mspi_conv_wgrad_entry")
BLOCK_SYMBOLS = {"mspi_gelu_bwd", "mspi_layernorm_bwd_ws_bytes", "mspi_layernorm_bwd", "mspi_dwconv_wgrad_supported",
                 "mspi_dwconv_wgrad_ws_bytes", "mspi_dwconv_wgrad"}
# name: ((B, T, h, w), C, s, second conv); C is the two inputs' widths summed where SPLIT names the first one's
CASES = {"tiny": ((1, 2, 1, 2), 24, 2, True), "odd": ((2, 6, 5, 3), 24, 2, True), "tail": ((1, 5, 3, 3), 48, 2, True),
         "s4": ((1, 8, 7, 12), 48, 4, True), "ragged112": ((1, 4, 3, 5), 112, 2, True), "ragged44": ((1, 4, 3, 5), 44, 2, True),
         "split": ((2, 4, 2, 3), 192 + 512, 4, True), "plain": ((1, 2, 3, 5), 320, 1, False),
         "widest": ((1, 1, 2, 2), 2048 + 512, 1, False), "slice": ((1, 2, 4, 4), 32, 2, True)}
SPLIT = {"split": 192, "widest": 2048}
SLICE_LD = 96                                   # "slice": x is the last 32 channels of rows 96 wide
SLAB_EXTRA = 5                                  # the second input of a split case: a view into a [B, Rv + 5, 512] slab
# one case for every further variant code: the smallest row count that takes it
VARIANTS = {"rows1024": ((1, 2, 32, 32), 24, 2, 256, 9701), "rows32768": ((1, 2, 128, 256), 24, 2, 512, 9702)}
END_TO_END = ("odd", "s4", "split", "plain", "widest")


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "lateral_entry.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _restated(key):
    """(case, {name: gradient}, (dWc, dbc)) in float64 at mid = 192, computed once and left unchanged."""
    if key in VARIANTS:
        shape, C, s, _, seed = VARIANTS[key]
        second = True
    else:
        (shape, C, s, second), seed = CASES[key], int(_gold()["%s_seed" % key])
    case = ER.make_case(*shape, C, s, seed, second)
    x = torch.from_numpy(case["x"]).double()
    if key == "tail":                            # the fifth frame is never read: NaN there must reach nothing
        case["x"][:, :, 4] = np.nan
        x = x.clone()
        x[:, :, 4] = 0.0
    composed = ER.composed_grads(x, torch.from_numpy(case["G"]).double(), s)
    return case, (None if key in VARIANTS else ER.backward(case, x=x)), composed


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["cases"]) == tuple(CASES)
    for c, (shape, C, s, second) in CASES.items():
        assert tuple(g["%s_geom" % c]) == shape + (C, s, int(second)), c
    mid = int(g["tiny_mid"])
    assert mid == 32
    shapes = {"w0": (mid, 24, 1, 1, 1), "b0": (mid,), "w1": (mid, mid, 2, 1, 1)}
    for k in ER.NAMES:
        assert g["tiny_d_%s" % k].shape == shapes[k] and g["tiny_d_%s" % k].dtype == np.float64
    assert g["tiny_y"].shape == (1, mid, 1, 1, 2) and g["tiny_y"].dtype == np.float64
    golden = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(golden, "lateral_entry.npz")) <= os.path.getsize(os.path.join(golden, "lateral_block.npz"))


def test_restatement_matches_the_fixture():
    g = _gold()
    shape, C, s, second = CASES["tiny"]
    case = ER.make_case(*shape, C, s, int(g["tiny_seed"]), second, mid=int(g["tiny_mid"]))
    assert (ER.forward(case) - torch.from_numpy(g["tiny_y"])).abs().max().item() <= 1e-12
    grads = ER.backward(case)
    for k in ER.NAMES:
        assert _err(grads[k], g["tiny_d_%s" % k]) <= 1e-12, k


@pytest.mark.parametrize("key", ["odd", "plain", "split"])
def test_restatement_matches_torch_autograd(key):
    """Stored as seeds: the two nn.Conv3d layers as upstream builds them, float64, built here.  "plain" has no second conv,
    "split" is the concat of the two inputs."""
    case, grads, _ = _restated(key)
    y, ref = ER.upstream_grads(case)
    assert _err(ER.forward(case), y) <= 1e-12
    assert sorted(grads) == sorted(ref) and ("w1" in ref) == CASES[key][3]
    for k in ref:
        assert _err(grads[k], ref[k]) <= 1e-12, k


def test_entry_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    from mspi_amd import engine as E
    entry, text = _declared("mspi_entry_train_hip.h")
    block, _ = _declared("mspi_block_train_hip.h")
    train, _ = _declared("mspi_train_hip.h")
    base, base_text = _declared("mspi_hip.h")
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert entry == set(NEW_SYMBOLS) == set(_lib.ENTRY_EXPORTS) == set(_lib._ENTRY_SIGNATURES)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _lib._ENTRY_SIGNATURES[name][1], name
    # the three pinned symbol sets are as they were, the ABI version unchanged
    assert block == set(_lib.BLOCK_EXPORTS) == BLOCK_SYMBOLS
    assert train == set(_lib.TRAIN_EXPORTS) == {"mspi_rowgate_bwd", "mspi_upsample_sum_bwd"}
    assert base == set(_lib.EXPORTS) and not (base | train | block) & set(NEW_SYMBOLS)
    assert re.search(r"#define MSPI_ABI_VERSION 2\b", base_text) and lib.mspi_version() == 2
    whole = open(os.path.join(ROOT, "include", "mspi_entry_train_hip.h")).read()
    assert "mspi_block_train_hip.h" in whole and "bitwise repeatable" in whole      # the conventions it says it follows
    for name in ("conv_wgrad_entry", "conv_wgrad_entry_variant"):
        assert callable(getattr(E, name)) and name in E.__all__
    src = open(os.path.join(ROOT, "mspi_amd", "csrc", "entry_bwd.hip")).read()
    assert "atomic" not in src.lower()
    mk = open(os.path.join(ROOT, "mspi_amd", "csrc", "Makefile")).read()
    assert "entry_bwd.hip" in mk and "mspi_entry_train_hip.h" in mk and mk.count("mspi_block_train_hip.h") == 2
    assert "-fno-slp-vectorize" in mk


def _desc(N=1, T=4, H=3, W=5, C=24, Cout=192, k=(2, 1, 1), stride=None, pad=(0, 0, 0), ld=None, sN=None, sC=1, ldy=None, To=None):
    from mspi_amd import _lib
    stride = k if stride is None else stride
    ld = C if ld is None else ld
    d = _lib.ConvDesc()
    d.N, d.T, d.H, d.W, d.C = N, T, H, W, C
    d.sW, d.sH, d.sT, d.sC = ld, W * ld, H * W * ld, sC
    d.sN = T * H * W * ld if sN is None else sN
    d.kT, d.kH, d.kW = k
    d.strT, d.strH, d.strW = stride
    d.padT, d.padH, d.padW = pad
    d.To, d.Ho, d.Wo = [(n + 2 * p - kk) // st + 1 for n, p, kk, st in zip((T, H, W), pad, k, stride)]
    if To is not None:
        d.To = To
    d.Cout, d.ldy = Cout, (Cout if ldy is None else ldy)
    return d


def test_host_refusals():
    from mspi_amd import _lib
    lib = _lib.load()

    def err():
        return lib.mspi_last_error().decode()

    def run(d, x=4096, dy=8192, dW=12288, db=16384, ws=20480):
        return lib.mspi_conv_wgrad_entry(ctypes.byref(d) if d is not None else None, x, dy, dW, db, ws, None), err()

    good = _desc()
    assert lib.mspi_conv_wgrad_entry_supported(ctypes.byref(good)) == 1
    assert lib.mspi_conv_wgrad_entry_variant(ctypes.byref(good), 4096, 8192) == 64          # 30 rows: the short slice
    assert lib.mspi_conv_wgrad_entry_ws_bytes(ctypes.byref(good)) == 1 * (192 * 48 + 192) * 4  # one slice, [Cout][s C] + [Cout]
    for rows, code in ((1023, 64), (1024, 256), (32767, 256), (32768, 512)):
        assert lib.mspi_conv_wgrad_entry_variant(ctypes.byref(_desc(T=1, H=1, W=rows, k=(1, 1, 1))), 4096, 8192) == code, rows
    assert lib.mspi_conv_wgrad_entry_ws_bytes(ctypes.byref(_desc(T=1, H=1, W=1025, k=(1, 1, 1)))) == 5 * (192 * 24 + 192) * 4
    for ok in (_desc(k=(1, 1, 1)), _desc(T=9, k=(4, 1, 1)), _desc(T=5), _desc(C=2560, k=(1, 1, 1)), _desc(C=44), _desc(Cout=32),
               _desc(ld=96, C=32), _desc(sN=4 * 3 * 5 * 24 + 5 * 24), _desc(ldy=200)):
        assert lib.mspi_conv_wgrad_entry_supported(ctypes.byref(ok)) == 1, err()
    refused = {"C % 4": _desc(C=26), "at most 2560": _desc(C=2564), "at most 192": _desc(Cout=224), "at most 192 ": _desc(Cout=48),
               "spatial taps": _desc(k=(2, 3, 3), stride=(2, 1, 1)), "spatial taps ": _desc(k=(1, 1, 3), stride=(1, 1, 1)),
               "stride must equal the kernel": _desc(k=(2, 1, 1), stride=(1, 1, 1)),
               "stride must equal the kernel ": _desc(k=(1, 1, 1), stride=(1, 2, 2)),
               "stride must equal the kernel  ": _desc(k=(2, 1, 1), stride=(4, 1, 1)), "1, 2 or 4": _desc(T=6, k=(3, 1, 1)),
               "padding must be 0": _desc(T=6, pad=(1, 0, 0)), "sC == 1": _desc(sC=2), "multiples of 4": _desc(ld=26),
               "multiples of 4 ": _desc(sN=4 * 3 * 5 * 24 + 2), "ldy must be": _desc(ldy=190), "ldy must be ": _desc(ldy=128),
               "empty extent": _desc(W=0), "empty extent ": _desc(T=1), "output extent": _desc(To=1),
               "2^31": _desc(N=1 << 11, T=2, H=1 << 10, W=1 << 10)}
    for text, d in refused.items():
        assert lib.mspi_conv_wgrad_entry_supported(ctypes.byref(d)) == 0 and text.strip() in err(), (text, err())
        assert lib.mspi_conv_wgrad_entry_ws_bytes(ctypes.byref(d)) == 0
        assert lib.mspi_conv_wgrad_entry_variant(ctypes.byref(d), 4096, 8192) == -1
        rc, why = run(d)
        assert rc == -1 and "mspi_conv_wgrad_entry" in why and text.strip() in why, (text, rc, why)
    assert lib.mspi_conv_wgrad_entry_supported(None) == 0 and lib.mspi_conv_wgrad_entry_variant(None, 4096, 8192) == -1
    for rc, why in (run(good, x=None), run(good, dy=None), run(good, dW=None), run(good, db=None), run(good, ws=None)):
        assert rc == -1 and "null argument" in why, (rc, why)
    for rc, why in (run(good, x=4100), run(good, dy=8200), run(good, ws=20484), run(good, dW=12292)):      # misaligned pointers
        assert rc == -1 and "16-byte aligned" in why, (rc, why)
    assert lib.mspi_conv_wgrad_entry_variant(ctypes.byref(good), 4100, 8192) == -1 and "16-byte aligned" in err()


def _entry_names(m):
    names = []
    for k in range(4):
        seq = getattr(m, "latlayer_%d" % k)
        names += ["latlayer_%d.0.weight" % k, "latlayer_%d.0.bias" % k] + (["latlayer_%d.1.weight" % k] if len(seq) == 3 else [])
    return names


def _block_names(m):
    return ["latlayer_%d.%d.%s" % (k, len(getattr(m, "latlayer_%d" % k)) - 1, n) for k in range(4) for n in LR.STATE_KEYS.values()]


def _trained_names(m, entries=True):
    return sorted(list(R.STATE_KEYS.values()) + list(FR.STATE_KEYS.values()) + _block_names(m) + (_entry_names(m) if entries else []))


@pytest.mark.parametrize("name,entries,total", [("x3dl", 12, 83), ("s3d", 10, 81), ("slowfast4x16", 8, 79)])
def test_trainable_lateral_entries_flags_modes_and_restore(monkeypatch, name, entries, total):
    from mspi_amd import testing as T
    from mspi_amd._lib import MspiError
    from mspi_amd.model import model_utils as pm
    m = T.seeded(lambda: pm.AudioVisualSaliencyModel(T.make_cfg(name)), 0)
    first = next(m.visnet.parameters())
    first.requires_grad_(False)
    before = {n: p.requires_grad for n, p in m.named_parameters()}
    assert m.trainable("lateral_entries") is m
    on = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert on == _trained_names(m) and len(on) == total and len(_entry_names(m)) == entries
    assert not any(p.requires_grad for mod in (m.adapter, m.aud_vis_sync_block, m.visnet, m.image_encoder, m.audnet)
                   for p in mod.parameters())
    m.train()
    m.frozen_encoder()
    assert sorted(n for n, s in m.named_modules() if s.training) == BATCH_STAT and not m.training
    m._check_eval()
    assert m._training_tail() == "inputs"
    with torch.no_grad():
        assert m._training_tail() is False
    for other in (m.latlayer_0[0], m.adapter, m.latlayer_3[-1]):
        other.train()
        with pytest.raises(MspiError, match="under trainable\\('lateral_entries'\\) only readout.2, readout.5 and the three"):
            m._check_eval()
        m.frozen_encoder()
    m._check_eval()
    m.trainable("lateral_blocks")                               # switching over and back
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == _trained_names(m, entries=False)
    assert m._training_tail() == "entries"
    m.adapter.train()
    with pytest.raises(MspiError, match="under trainable\\('lateral_blocks'\\) only readout.2, readout.5 and the three"):
        m._check_eval()
    m.frozen_encoder()
    m.trainable("lateral_entries")
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == on
    for bad in ("laterals", "decoder", "all", ""):
        with pytest.raises(MspiError, match="readout_tail"):
            m.trainable(bad)
    m.trainable(None)
    assert {n: p.requires_grad for n, p in m.named_parameters()} == before and not first.requires_grad
    monkeypatch.setattr(pm, "DECODER_FUSED", False)
    with pytest.raises(MspiError, match="MSPI_DECODER_FUSED"):
        m.trainable("lateral_entries")


def test_compose_lateral_has_moved_and_kept_its_alias():
    from mspi_amd import autograd as A
    from mspi_amd.model import model_utils as pm
    torch.manual_seed(3)
    c0 = torch.nn.Conv3d(24, 192, 1)
    c1 = torch.nn.Conv3d(192, 192, (2, 1, 1), (2, 1, 1), bias=False)
    w, b = pm._compose_lateral(c0, c1)
    w2, b2 = A.compose_lateral(c0.weight, c0.bias, c1.weight)
    assert torch.equal(w, w2) and torch.equal(b, b2) and w.dtype == torch.float32 and tuple(w.shape) == (192, 24, 2, 1, 1)
    case = {"w0": c0.weight.detach().numpy(), "b0": c0.bias.detach().numpy(), "w1": c1.weight.detach().numpy(), "s": 2}
    wc, bc = ER.compose(case)
    assert _err(w[:, :, :, 0, 0], wc) <= 1e-6 and _err(b, bc) <= 1e-6


def test_train_accepts_lateral_entries_up_to_the_gpu_check(monkeypatch):
    from mspi_amd import train
    from mspi_amd._lib import MspiError
    assert train.TRAINABLE_ENTRIES == ("lateral_entries",) and train.TRAINABLE_BLOCKS == ("lateral_blocks",)
    assert train.TRAINABLE == ("readout_tail", "readout") and train.TRAINABLE_STAGES == train.TRAINABLE + ("fusion",)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="MI355X"):
        train.main(["--trainable", "lateral_entries"])
    with pytest.raises(MspiError, match="--trainable laterals: only readout_tail, readout can be trained on a frozen pyramid, and "
                                        "fusion.*lateral_blocks.*lateral_entries"):
        train.main(["--trainable", "laterals"])
    doc = train.__doc__
    assert "--trainable lateral_entries" in doc and "--trainable lateral_blocks" in doc and "Still frozen" in doc


# ------------------------------------------------------------------------------------------------------------- GPU
def _inputs(key, dev, x5=None):
    """The case's input(s) on the device as the product hands them over: [(CL, first channel, width)].  "slice": the last 32
    channels of rows 96 wide, NaN elsewhere; the second input of a split case: a token view into a [B, Rv + 5, 512] slab of NaN."""
    from mspi_amd import engine as E
    case = _restated(key)[0]
    x5 = torch.from_numpy(case["x"]) if x5 is None else x5
    if key not in SPLIT:
        return [(_cl(x5, dev, SLICE_LD if key == "slice" else None), 0, x5.shape[1])]
    c1 = SPLIT[key]
    B, C, T, h, w = x5.shape
    Rv, c2 = T * h * w, C - c1
    slab = torch.full((B, Rv + SLAB_EXTRA, c2), float("nan"), device=dev)
    slab[:, :Rv] = x5[:, c1:].permute(0, 2, 3, 4, 1).reshape(B, Rv, c2).to(dev)
    view = E.CL(slab.view(-1), 0, B, Rv + SLAB_EXTRA, 1, 1, c2, c2).tokens(0, T, h, w)
    assert not view.dense and view.sN == (Rv + SLAB_EXTRA) * c2
    return [(_cl(x5[:, :c1].contiguous(), dev), 0, c1), (view, c1, c2)]


def _geom(cin, s):
    from mspi_amd import autograd as A
    return A._geometry((s, 1, 1), (0, 0, 0), cin, ER.MID, (s, 1, 1))


def _kernel(key, dev, x5=None, G5=None, scale=1.0):
    """(dWc [co,ci,s], dbc) of the kernel over the case's input(s), the column blocks side by side."""
    from mspi_amd import engine as E
    case = _restated(key)[0]
    G = _cl((torch.from_numpy(case["G"]) if G5 is None else G5) * scale, dev)
    dWs, dbs = [], []
    for x, _, c in _inputs(key, dev, x5):
        dW, db = E.conv_wgrad_entry(x, G, _geom(c, case["s"]))
        dWs.append(dW[:, :, :, 0, 0])
        dbs.append(db)
    for db in dbs[1:]:
        assert torch.equal(db.view(torch.int32), dbs[0].view(torch.int32))       # db reads dy alone: the same bits, a NaN included
    return torch.cat(dWs, 1), dbs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(CASES) + list(VARIANTS))
def test_hip_entry_wgrad_kernel_vs_fp64(dev, key):
    """dW and db of the kernel against float64 on every case; twice, for equal bits."""
    from mspi_amd import engine as E
    case, _, (rW, rb) = _restated(key)
    want = VARIANTS[key][3] if key in VARIANTS else 64
    for x, _, c in _inputs(key, dev):
        assert E.conv_wgrad_entry_variant(x, _cl(case["G"], dev), _geom(c, case["s"])) == want
    dW, db = _kernel(key, dev)
    assert torch.isfinite(dW).all() and torch.isfinite(db).all()
    eW, eb = _err(dW, rW), _err(db, rb)
    print("%s: dW %.2e db %.2e" % (key, eW, eb))
    assert eW <= GRAD_TOL and eb <= GRAD_TOL
    dW2, db2 = _kernel(key, dev)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)        # bitwise repeatable


@pytest.mark.gpu
def test_hip_entry_wgrad_narrow_output(dev):
    """The fixture's own "tiny" at mid = 32, the narrowest output the kernel takes, against the STORED float64 gradients
    (without a second conv dW0 = dWc, so the kernel's result is compared through the chain rule's last step on the host)."""
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    g = _gold()
    shape, C, s, second = CASES["tiny"]
    case = ER.make_case(*shape, C, s, int(g["tiny_seed"]), second, mid=32)
    dW, db = E.conv_wgrad_entry(_cl(case["x"], dev), _cl(case["G"], dev), A._geometry((s, 1, 1), (0, 0, 0), C, 32, (s, 1, 1)))
    w0, b0, w1 = (torch.from_numpy(case[k]).double() for k in ("w0", "b0", "w1"))
    dwc, dbc = dW[:, :, :, 0, 0].double().cpu(), db.double().cpu()
    got = {"w1": torch.einsum("oit,mi->omt", dwc, w0.flatten(1)) + dbc[:, None, None] * b0[None, :, None],
           "w0": torch.einsum("omt,oit->mi", w1[:, :, :, 0, 0], dwc), "b0": torch.einsum("omt,o->m", w1[:, :, :, 0, 0], dbc)}
    for k in ER.NAMES:
        e = _err(got[k].reshape(g["tiny_d_%s" % k].shape), g["tiny_d_%s" % k])
        print("tiny at mid 32, d %s: %.2e" % (k, e))
        assert e <= GRAD_TOL, k


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["odd", "split"])
def test_hip_entry_wgrad_loss_scale(dev, key):
    """G scaled by 2^-20 and 2^12: powers of two, so the gradients are the unscaled ones' bits, scaled."""
    dW, db = _kernel(key, dev)
    _, _, (rW, rb) = _restated(key)
    for e in (-20, 12):
        sW, sb = _kernel(key, dev, scale=2.0 ** e)
        eW, eb = _err(sW * 2.0 ** -e, rW), _err(sb * 2.0 ** -e, rb)
        print("%s x 2^%d: dW %.2e db %.2e" % (key, e, eW, eb))
        assert eW <= GRAD_TOL and eb <= GRAD_TOL
        assert torch.equal(sW * 2.0 ** -e, dW) and torch.equal(sb * 2.0 ** -e, db)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("key", ["odd", "s4", "split"])
def test_hip_entry_wgrad_nonfinite_operands_propagate(dev, key, value):
    """A poison in a used x[r][ci] reaches exactly dW[:, ci, tap] and not db; one in dy[r][co] exactly dW[co] and db[co]."""
    case, _, (rW, rb) = _restated(key)
    s = case["s"]
    B, C, T, h, w = case["x"].shape
    x5, G5 = torch.from_numpy(case["x"]), torch.from_numpy(case["G"])
    for ci, t in ((1, 0), (C - 1, (T // s) * s - 1)):           # the first input's second channel; the last channel, last used frame
        dW, db = _kernel(key, dev, x5=_poisoned(x5, (B - 1, ci, t, h - 1, w // 2), value))
        ref = rW.clone()
        ref[:, ci, t % s] = float("nan")
        _judge("%s x[ci %d, frame %d] -> dW" % (key, ci, t), dW, ref)
        assert torch.isfinite(db).all() and _err(db, rb) <= GRAD_TOL
    for co in (0, 37, ER.MID - 1):
        dW, db = _kernel(key, dev, G5=_poisoned(G5, (0, co, 0, h // 2, w - 1), value))
        refW, refb = rW.clone(), rb.clone()
        refW[co] = float("nan")
        refb[co] = float("nan")
        _judge("%s dy[co %d] -> dW" % (key, co), dW, refW)
        _judge("%s dy[co %d] -> db" % (key, co), db, refb)


@pytest.mark.gpu
def test_hip_entry_wgrad_capture_and_replay(dev):
    """The raw entry point, the first call included: operands and the host descriptor overwritten between capture and replay."""
    from mspi_amd import _lib
    lib = _lib.load()
    for key in ("odd", "s4"):
        shape, C, s, _ = CASES[key]
        B, T, h, w = shape

        def operands(seed):
            c = ER.make_case(*shape, C, s, seed)
            return {"x": torch.from_numpy(c["x"]).permute(0, 2, 3, 4, 1).contiguous(),
                    "dy": torch.from_numpy(c["G"]).permute(0, 2, 3, 4, 1).contiguous()}

        def launch(t, host):
            d = _desc(N=B, T=T, H=h, W=w, C=C, k=(s, 1, 1))
            host.append(d)                                          # the descriptor: read during the call, overwritten before the replay
            dW, db = torch.empty(ER.MID, s * C, device=dev), torch.empty(ER.MID, device=dev)
            ws = torch.empty(lib.mspi_conv_wgrad_entry_ws_bytes(ctypes.byref(d)) // 4, device=dev)
            _lib.check(lib.mspi_conv_wgrad_entry(ctypes.byref(d), t["x"].data_ptr(), t["dy"].data_ptr(), dW.data_ptr(), db.data_ptr(),
                                                 ws.data_ptr(), _stream()), "mspi_conv_wgrad_entry")
            return {"dW": dW, "db": db}
        _replayed(dev, {"A": operands(41), "B": operands(42)}, launch)


def _as_tensor(cl):
    return cl.buf.as_strided((cl.N, cl.T, cl.H, cl.W, cl.C), (cl.sN, cl.H * cl.W * cl.ld, cl.W * cl.ld, cl.ld, 1),
                             cl.buf.storage_offset() + cl.off)


@pytest.mark.gpu
@pytest.mark.parametrize("key", END_TO_END)
def test_hip_lateral_entry_end_to_end(dev, key):
    """y has the bits of the launches of _SaliencyBase._lateral (packs built here the way _pack_lateral built them before the
    helper was shared), every gradient is within the bar of the restatement, and two runs give equal bits."""
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    case, ref, _ = _restated(key)
    s, second = case["s"], "w1" in case
    ins = _inputs(key, dev)
    # the inference launches
    c0 = torch.nn.Conv3d(case["w0"].shape[1], ER.MID, 1)
    with torch.no_grad():
        c0.weight.copy_(torch.from_numpy(case["w0"]))
        c0.bias.copy_(torch.from_numpy(case["b0"]))
    if second:
        c1 = torch.nn.Conv3d(ER.MID, ER.MID, (s, 1, 1), (s, 1, 1), bias=False)
        with torch.no_grad():
            c1.weight.copy_(torch.from_numpy(case["w1"]))
        w0 = c0.weight.detach().double().flatten(1)
        w1 = c1.weight.detach().double()[:, :, :, 0, 0]
        w = torch.einsum("omt,mi->oit", w1, w0)[:, :, :, None, None].float()
        b = torch.einsum("omt,m->o", w1, c0.bias.detach().double()).float()
    else:
        w, b = c0.weight.detach().float(), c0.bias.detach().float()
    w, b = w.to(dev), b.to(dev)
    if len(ins) == 1:
        want = E.conv(ins[0][0], E.pack_conv(w, b, None, (s, 1, 1), (0, 0, 0)))
    else:
        split = ins[0][2]
        want = E.conv(ins[0][0], E.pack_conv(w[:, :split].contiguous(), b, None, (s, 1, 1), (0, 0, 0)))
        want = E.conv(ins[1][0], E.pack_conv(w[:, split:].contiguous(), None, None, (s, 1, 1), (0, 0, 0)), res=want)
    want = want.buf.view(want.N, want.T, want.H, want.W, want.ld).clone()

    def run():
        ps = {k: torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in ("w0", "b0") + (("w1",) if second else ())}
        ts = [_as_tensor(cl) for cl, _, _ in ins]
        y = A.LateralEntry.apply(ts[0], ts[1] if len(ts) == 2 else None, ps["w0"], ps["b0"], ps.get("w1"))
        y.backward(torch.from_numpy(case["G"]).permute(0, 2, 3, 4, 1).contiguous().to(dev))
        return y.detach(), {k: p.grad for k, p in ps.items()}
    y, grads = run()
    assert torch.equal(y, want)
    ey = _err(y.permute(0, 4, 1, 2, 3), ER.forward(case, x=torch.nan_to_num(torch.from_numpy(case["x"]))))
    print("%s: y %.2e" % (key, ey))
    assert ey <= GRAD_TOL          # f16x3 products carry 22 significand bits (2.4e-7 each) and do not add up coherently
    assert sorted(grads) == sorted(ref)
    for k in ref:
        assert grads[k].shape == ref[k].shape and torch.isfinite(grads[k]).all()
        e = _err(grads[k], ref[k])
        print("%s: d %s %.2e" % (key, k, e))
        assert e <= GRAD_TOL, k
    y2, grads2 = run()
    assert torch.equal(y2, y) and all(torch.equal(grads2[k], grads[k]) for k in grads)


@pytest.mark.gpu
def test_hip_lateral_entry_refuses_by_name(dev):
    from mspi_amd import autograd as A
    from mspi_amd._lib import MspiError
    x = torch.randn(1, 2, 3, 5, 24, device=dev)
    w0, b0 = torch.randn(192, 24, 1, 1, 1, device=dev), torch.randn(192, device=dev)
    w1 = torch.randn(192, 192, 2, 1, 1, device=dev)
    with pytest.raises(MspiError, match="GPU only"):
        A.LateralEntry.apply(x.cpu(), None, w0.cpu(), b0.cpu(), w1.cpu())
    with pytest.raises(MspiError, match="x must be fp32 \\[B,T,h,w,C\\]"):
        A.LateralEntry.apply(x[0], None, w0, b0, w1)
    with pytest.raises(MspiError, match="the input has 24 channels"):
        A.LateralEntry.apply(x, None, w0[:, :20].contiguous(), b0, w1)
    with pytest.raises(MspiError, match="latlayer\\[1\\] is"):
        A.LateralEntry.apply(x, None, w0, b0, torch.randn(192, 192, 3, 1, 1, device=dev))
    with pytest.raises(MspiError, match="x2 .* does not have the extent"):
        A.LateralEntry.apply(x, torch.randn(1, 2, 3, 4, 8, device=dev), torch.randn(192, 32, 1, 1, 1, device=dev), b0, w1)
    y = A.LateralEntry.apply(x, None, w0.requires_grad_(True), b0, w1)
    assert tuple(y.shape) == (1, 1, 3, 5, 192) and y.requires_grad


# ---- the whole model
MODELS = [("av_x3dl_64", "x3dl", "AudioVisualSaliencyModel", 83), ("vis_x3dl_64", "x3dl", "VisualSaliencyModel", 83),
          ("av_s3d_64", "s3d", "AudioVisualSaliencyModel", 81), ("av_slowfast_64", "slowfast4x16", "AudioVisualSaliencyModel", 79)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,name,cls,total", MODELS, ids=[m[0] for m in MODELS])
def test_hip_whole_model_trains_its_lateral_entries(dev, golden_dir, monkeypatch, case, name, cls, total):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    from mspi_amd import metrics as M
    from mspi_amd._lib import MspiError
    from mspi_amd.model import model_utils as pm
    from test_readout_tail import _batches, _build
    E.autotune(False)          # bits are compared, and an empty cache pins the library's own kernel choices
    monkeypatch.setitem(E.AUTOTUNE, "cache", {})      # (tests/test_lateral_train.py::test_hip_whole_model_trains_its_lateral_blocks says why)
    sound = cls == "AudioVisualSaliencyModel"
    g, cfg, make, clips, audio = _build(golden_dir, case, name, cls, dev)
    args = (clips, audio) if sound else (clips,)
    m = make().to(dev)
    off = m(*args)[0]
    label = _batches(clips, audio, 1, True)[0][2].to(dev)

    def step_grads():
        for p in m.parameters():
            p.grad = None
        out = m(*args)[0]
        assert out.requires_grad
        M.SalLoss()(out, label).backward()
        return out.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    m.trainable("lateral_blocks")
    m.train()
    m.frozen_encoder()
    b_out, b_grads = step_grads()
    assert len(b_grads) == 71

    m.trainable("lateral_entries")
    m.eval()
    with pytest.raises(MspiError, match="frozen_encoder"):      # eval() BatchNorm and a graph: batch statistics would be a surprise
        m(*args)
    m.train()
    m.frozen_encoder()
    with torch.no_grad():      # the launches of inference; the step above has moved the five layers' running statistics
        quiet = m(*args)[0]
    assert not quiet.requires_grad

    calls = []

    class Recorded:
        @staticmethod
        def apply(x, x2, w0, b0, w1):
            y = A.LateralEntry.apply(x, x2, w0, b0, w1)
            rec = {"x": (x if x2 is None else torch.cat([x, x2], 4)).detach().clone(), "s": 1 if w1 is None else w1.shape[2]}
            y.register_hook(lambda gr, rec=rec: rec.__setitem__("G", gr.detach().clone()))
            calls.append(rec)
            return y
    monkeypatch.setattr(pm, "LateralEntry", Recorded)
    start = {k: v.clone() for k, v in m.state_dict().items()}
    params = [p for p in m.parameters() if p.requires_grad]
    assert len(params) == total
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0)
    e_out, e_grads = step_grads()
    monkeypatch.setattr(pm, "LateralEntry", A.LateralEntry)
    # on identical weights and input: the map and the 71 gradients trainable("lateral_blocks") produces have its bits
    assert torch.equal(e_out, b_out)
    assert sorted(e_grads) == _trained_names(m) and len(calls) == 4
    for n, gr in b_grads.items():
        assert torch.equal(e_grads[n], gr), n
    # the entry gradients against the float64 restatement, fed the recorded inputs and the G of this very run
    for k, rec in enumerate(calls):
        seq = getattr(m, "latlayer_%d" % k)
        c = {"w0": seq[0].weight.detach().cpu().numpy(), "b0": seq[0].bias.detach().cpu().numpy(), "s": rec["s"]}
        if len(seq) == 3:
            c["w1"] = seq[1].weight.detach().cpu().numpy()
        c["x"], c["G"] = (rec[n].permute(0, 4, 1, 2, 3).cpu().numpy() for n in ("x", "G"))
        ref = ER.backward(c)
        for n in ref:
            got = e_grads["latlayer_%d.%s" % (k, ER.STATE_KEYS[n])]
            assert torch.isfinite(got).all()
            e = _err(got, ref[n])
            print("%s latlayer_%d d %s: %.2e" % (case, k, n, e))
            assert e <= GRAD_TOL, (k, n)
    opt.step()
    moved = set(_trained_names(m)) | {"%s.%s" % (mod, n) for mod in BATCH_STAT for n in ("running_mean", "running_var", "num_batches_tracked")}
    # AdamW without weight decay leaves a tensor whose gradient is exactly zero where it is.  The true gradient of
    # readout.12.bias IS zero (the log-softmax behind it is shift invariant): what fp32 leaves of it is rounding, and on the s3d
    # fixture that is 0.0 -- with the bits trainable("lateral_blocks") gives, as asserted above.  Only that tensor may stand still.
    still = {n for n in _trained_names(m) if not e_grads[n].any()}
    print("%s: gradient exactly zero: %s" % (case, sorted(still)))
    assert still <= {"readout.12.bias"}
    for k, v in m.state_dict().items():
        assert torch.equal(v, start[k]) == (k not in moved - still), k
    with torch.no_grad():
        trained = m(*args)[0]
    assert not torch.equal(trained, quiet) and not torch.equal(trained, off) and torch.isfinite(trained).all()
    fresh = make()
    fresh.load_state_dict(m.state_dict())
    again = fresh.to(dev)(*args)[0]
    assert torch.equal(again, trained)
    m.trainable(None)
    m.eval()
    plain = m(*args)[0]
    assert torch.equal(plain, trained) and not plain.requires_grad


@pytest.mark.gpu
@pytest.mark.parametrize("case,name,cls,total", MODELS, ids=[m[0] for m in MODELS])
def test_hip_entries_switch_on_under_no_grad_is_the_switch_off_map(dev, golden_dir, case, name, cls, total):
    from mspi_amd import engine as E
    from test_readout_tail import _build
    E.autotune(False)
    g, cfg, make, clips, audio = _build(golden_dir, case, name, cls, dev)
    args = (clips, audio) if cls == "AudioVisualSaliencyModel" else (clips,)
    m = make().to(dev)
    off = m(*args)[0]
    m.trainable("lateral_entries")
    m.train()
    m.frozen_encoder()
    with torch.no_grad():
        quiet = m(*args)[0]
    assert torch.equal(quiet, off) and not quiet.requires_grad
