"""The trainable adapter: csrc/adapter_bwd.hip (mspi_conv_wgrad_t16 and its three host companions, declared in
include/mspi_adapter_train_hip.h), engine.conv_wgrad_t16 / conv_wgrad_t16_variant, the gradient of `masks` in autograd.Fusion,
autograd.Adapter, _SaliencyBase.trainable("adapter"), mspi_amd.train --trainable adapter.

Yardsticks: tests/golden/adapter.npz holds "tiny" ((B, T, h, w) = (1, 2, 2, 3), 12 rows, at the scaled-down widths
adapter_restate.SMALL) with, in float64, the Inception's output and the 24 gradients of <masks, G> that torch autograd gives
through torch.nn layers built with upstream's arguments (tools/gen_adapter_golden.py), and the seeds of "odd" ((2, 2, 3, 5),
SMALL), "full" ((1, 4, 3, 4), the model's widths 416 -> 192 | 96 -> 208 -> 208 | 16 -> 48 -> 48 | 64) and of the two
fusion_restate cases on which the gradient of `masks` is checked.  tests/adapter_restate.py is the float64 restatement in this
project's launch order, pinned to that fixture and, here, to torch autograd on "odd" and at the real widths on "full".

Bounds.  Every gradient tensor: max |got - ref| / max |ref| <= GRAD_TOL = 2e-5, the project's bar for gradients
(tests/test_readout_train.py); every test prints its figure before it asserts.  Torch FLOAT32 on the CPU agrees with float64,
worst of masks and the gradients (tools/gen_adapter_golden.py prints them): tiny 1.4e-6, odd 1.6e-6, full 1.3e-6, fusion_tiny
3.4e-7, fusion_odd 1.4e-6 -- the bar leaves a factor of 12 on the worst case.  The seeds were searched for that agreement, which
keeps every ReLU unit off its kink.  The kernel cases are not in the fixture: their float64 reference is computed here from a
seed; fp32 fmaf chains over at most 8192 products of standard normals stay below 1e-6 of the largest entry.

The ledger part holds the entry point to what tests/test_entry_train.py holds its one: declared = exported = bound, capture +
replay with the operands and the host descriptor overwritten in between, and a NaN / +Inf in each floating operand reaching
every output that depends on it and no other.  The header declares FOUR symbols (the launch and its three host companions)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import adapter_restate as AR
import fusion_restate as FR
from test_entry_train import MODELS as ENTRY_MODELS
from test_entry_train import _desc as _entry_desc
from test_entry_train import _trained_names as _entry_trained_names
from test_fusion_train import BATCH_STAT, _declared, _fusion_args, _judge, _poisoned, _replayed, _stream
from test_readout_train import GRAD_TOL, _cl, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_conv_wgrad_t16_supported", "mspi_conv_wgrad_t16_ws_bytes", "mspi_conv_wgrad_t16_variant", "mspi_conv_wgrad_t16")
ENTRY_SYMBOLS = {"mspi_conv_wgrad_entry_supported", "mspi_conv_wgrad_entry_ws_bytes", "mspi_conv_wgrad_entry_variant",
                 "mspi_conv_wgrad_entry"}
K111, K133, K311 = ((1, 1, 1), (0, 0, 0)), ((1, 3, 3), (0, 1, 1)), ((3, 1, 1), (1, 0, 0))
# (C, Cout): the kernel shape its layer uses
WIDTHS = {(16, 16): K111, (16, 48): K133, (48, 48): K311, (96, 208): K133, (208, 208): K311, (416, 16): K111, (416, 192): K111}
SHAPES = ((1, 1, 1, 3), (2, 2, 2, 3), (2, 4, 3, 5))
# one case for every further variant code: the smallest row count that takes it
VARIANTS = {"rows1024": ((1, 1, 32, 32), (16, 48), 128), "rows8192": ((1, 2, 64, 64), (48, 48), 256)}
DY_OFFSETS = (192, 400, 448)                     # where the model's branches lie in the 512-wide gradient of masks
CASES = {"tiny": ((1, 2, 2, 3), AR.SMALL), "odd": ((2, 2, 3, 5), AR.SMALL), "full": ((1, 4, 3, 4), AR.WIDTHS)}
BN_NAMES = sorted(BATCH_STAT + list(AR.BN_KEYS.values()))
MODELS = list(ENTRY_MODELS)                      # the fixtures and encoders of the entry convs' test: vis_x3dl_64 is among them
assert any(m[0] == "vis_x3dl_64" for m in MODELS)


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "adapter.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _restated(key):
    """(case, saved, grads) of the Inception in float64, computed once and left unchanged."""
    shape, widths = CASES[key]
    case = AR.make_case(*shape, int(_gold()["%s_seed" % key]), widths)
    sv = AR.forward(case)
    return case, sv, AR.backward(case, sv)


@functools.lru_cache(maxsize=None)
def _fusion_case(key):
    g = _gold()
    fp = FR.make_case(*[int(v) for v in g["%s_shape" % key]], int(g["%s_seed" % key]))
    return fp, AR.fusion_dmasks(fp)


@functools.lru_cache(maxsize=None)
def _wcase(shape, C, Co, seed=0):
    """(x, dy) fp32 [N,C,T,H,W] and the float64 (dW, db) for the kernel shape of the widths' layer."""
    B, T, h, w = shape
    gen = torch.Generator().manual_seed(1000 * C + Co + seed)
    x, dy = torch.randn(B, C, T, h, w, generator=gen), torch.randn(B, Co, T, h, w, generator=gen)
    return x, dy, AR.wgrad(x, dy, *WIDTHS[(C, Co)])


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["cases"]) == tuple(CASES) and tuple(g["fusion_cases"]) == ("fusion_tiny", "fusion_odd")
    for c, (shape, widths) in CASES.items():
        assert tuple(g["%s_shape" % c]) == shape and tuple(g["%s_widths" % c]) == tuple(widths), c
        assert shape[0] * shape[1] * shape[2] * shape[3] >= 12 and not any(v % 16 for v in widths)
    geo = AR.geometry(AR.SMALL)
    for l in AR.LAYERS:
        cin, cout, k, _ = geo[l]
        assert g["tiny_d_w_%s" % l].shape == (cout, cin) + k and g["tiny_d_w_%s" % l].dtype == np.float64
        assert g["tiny_d_gam_%s" % l].shape == g["tiny_d_bet_%s" % l].shape == (cout,)
    assert g["tiny_masks"].shape == (1, 80, 2, 2, 3) and g["tiny_masks"].dtype == np.float64
    golden = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(golden, "adapter.npz")) < os.path.getsize(os.path.join(golden, "readout.npz"))
    assert sum(AR.WIDTHS[i] for i in (1, 3, 5, 6)) == 512 and AR.slices() == {"b0": (0, 192), "b1t": (192, 208), "b2t": (400, 48), "b3": (448, 64)}


def test_restatement_matches_the_fixture():
    g = _gold()
    _, sv, grads = _restated("tiny")
    assert (sv["masks"] - torch.from_numpy(g["tiny_masks"])).abs().max().item() <= 1e-12
    for k in AR.PARAMS:
        assert _err(grads[k], g["tiny_d_%s" % k]) <= 1e-12, k


@pytest.mark.parametrize("key", ["odd", "full"])
def test_restatement_matches_torch_autograd(key):
    """Stored as seeds: Inception as upstream builds it, float64, BatchNorm in .train(), built here -- "full" at the real
    widths 416 -> 192 / 96 -> 208 -> 208 / 16 -> 48 -> 48 / 64."""
    case, sv, grads = _restated(key)
    masks, ref, layers = AR.upstream_grads(case)
    assert _err(sv["masks"], masks) <= 1e-12
    for k in AR.PARAMS:
        assert _err(grads[k], ref[k]) <= 1e-12, k
    for l, (_, bn) in layers.items():
        rm, rv = AR.running_stats(sv[l])
        assert _err(rm, bn.running_mean) <= 1e-12 and _err(rv, bn.running_var) <= 1e-12 and int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("key", ["fusion_tiny", "fusion_odd"])
def test_restated_dmasks_matches_torch_autograd(key):
    fp, dm = _fusion_case(key)
    assert _err(dm, AR.fusion_dmasks_upstream(fp)) <= 1e-12


def test_adapter_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    from mspi_amd import engine as E
    adapter, _ = _declared("mspi_adapter_train_hip.h")
    entry, _ = _declared("mspi_entry_train_hip.h")
    base, base_text = _declared("mspi_hip.h")
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert adapter == set(NEW_SYMBOLS) == set(_lib.ADAPTER_EXPORTS) == set(_lib._ADAPTER_SIGNATURES)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _lib._ADAPTER_SIGNATURES[name][1], name
    # the pinned symbol sets are as they were, the ABI version unchanged
    assert entry == set(_lib.ENTRY_EXPORTS) == ENTRY_SYMBOLS
    old = base | entry | set(_lib.TRAIN_EXPORTS) | set(_lib.BLOCK_EXPORTS)
    assert base == set(_lib.EXPORTS) and not old & set(NEW_SYMBOLS)
    assert re.search(r"#define MSPI_ABI_VERSION 2\b", base_text) and lib.mspi_version() == 2
    whole = open(os.path.join(ROOT, "include", "mspi_adapter_train_hip.h")).read()
    assert "mspi_entry_train_hip.h" in whole and "bitwise repeatable" in whole      # the conventions it says it follows
    for name in ("conv_wgrad_t16", "conv_wgrad_t16_variant"):
        assert callable(getattr(E, name)) and name in E.__all__
    src = open(os.path.join(ROOT, "mspi_amd", "csrc", "adapter_bwd.hip")).read()
    assert "atomic" not in src.lower() and "mfma_f32_16x16x4f32" in src
    mk = open(os.path.join(ROOT, "mspi_amd", "csrc", "Makefile")).read()
    assert "adapter_bwd.hip" in mk and mk.count("mspi_adapter_train_hip.h") == 2 and "-fno-slp-vectorize" in mk


def _desc(N=2, T=4, H=3, W=5, C=96, Cout=208, k=(1, 3, 3), pad=(0, 1, 1), stride=(1, 1, 1), **kw):
    return _entry_desc(N=N, T=T, H=H, W=W, C=C, Cout=Cout, k=k, stride=stride, pad=pad, **kw)


def test_host_refusals():
    from mspi_amd import _lib
    lib = _lib.load()

    def err():
        return lib.mspi_last_error().decode()

    def run(d, x=4096, dy=8192, dW=12288, db=16384, ws=20480):
        return lib.mspi_conv_wgrad_t16(ctypes.byref(d) if d is not None else None, x, dy, dW, db, ws, None), err()

    good = _desc()
    assert lib.mspi_conv_wgrad_t16_supported(ctypes.byref(good)) == 1
    assert lib.mspi_conv_wgrad_t16_variant(ctypes.byref(good), 4096, 8192) == 64            # 120 rows: the short slice
    # (1,3,3) on 3 x 5 frames: one box of 15 rows per frame, two boxes per slice: 8 frames -> 4 records [Cout][9 C] + [Cout]
    assert lib.mspi_conv_wgrad_t16_ws_bytes(ctypes.byref(good)) == 4 * (208 * 9 * 96 + 208) * 4
    for rows, code in ((1023, 64), (1024, 128), (8191, 128), (8192, 256), (2688, 128), (10752, 256)):
        d = _desc(N=1, T=1, H=1, W=rows, k=(1, 1, 1), pad=(0, 0, 0))
        assert lib.mspi_conv_wgrad_t16_variant(ctypes.byref(d), 4096, 8192) == code, rows
    d = _desc(N=1, T=1, H=1, W=1025, C=16, Cout=16, k=(1, 1, 1), pad=(0, 0, 0))             # 33 boxes of 32 rows, 4 per slice
    assert lib.mspi_conv_wgrad_t16_ws_bytes(ctypes.byref(d)) == 9 * (16 * 16 + 16) * 4
    for ok in (_desc(k=(1, 1, 1), pad=(0, 0, 0)), _desc(C=208, k=(3, 1, 1), pad=(1, 0, 0)), _desc(T=1, H=1, W=3), _desc(C=416, Cout=16),
               _desc(C=16, Cout=16), _desc(ld=128), _desc(sN=4 * 3 * 5 * 96 + 5 * 96), _desc(ldy=512), _desc(C=416, Cout=208)):
        assert lib.mspi_conv_wgrad_t16_supported(ctypes.byref(ok)) == 1, err()
    refused = {"C % 16": _desc(C=24), "C % 16 ": _desc(C=104), "C <= 416": _desc(C=432), "Cout % 16": _desc(Cout=200),
               "Cout % 16 ": _desc(Cout=8), "Cout <= 208": _desc(Cout=224), "stride must be 1": _desc(stride=(1, 2, 2)),
               "stride must be 1 ": _desc(k=(3, 1, 1), pad=(1, 0, 0), stride=(2, 1, 1)),
               "kernel must be": _desc(k=(3, 3, 3), pad=(1, 1, 1)), "kernel must be ": _desc(k=(1, 3, 3), pad=(0, 0, 0)),
               "kernel must be  ": _desc(k=(1, 1, 3), pad=(0, 0, 1)), "kernel must be   ": _desc(k=(3, 1, 1), pad=(0, 0, 0)),
               "sC == 1": _desc(sC=2), "multiples of 4": _desc(ld=98), "multiples of 4 ": _desc(sN=4 * 3 * 5 * 96 + 2),
               "ldy must be": _desc(ldy=192), "ldy must be ": _desc(ldy=210), "empty extent": _desc(W=0),
               "output extent": _desc(To=3), "2^31": _desc(N=1 << 11, T=1, H=1 << 10, W=1 << 10)}
    for text, d in refused.items():
        assert lib.mspi_conv_wgrad_t16_supported(ctypes.byref(d)) == 0 and text.strip() in err(), (text, err())
        assert lib.mspi_conv_wgrad_t16_ws_bytes(ctypes.byref(d)) == 0
        assert lib.mspi_conv_wgrad_t16_variant(ctypes.byref(d), 4096, 8192) == -1
        rc, why = run(d)
        assert rc == -1 and "mspi_conv_wgrad_t16" in why and text.strip() in why, (text, rc, why)
    assert lib.mspi_conv_wgrad_t16_supported(None) == 0 and lib.mspi_conv_wgrad_t16_variant(None, 4096, 8192) == -1
    for rc, why in (run(good, x=None), run(good, dy=None), run(good, dW=None), run(good, ws=None)):      # db may be NULL
        assert rc == -1 and "null argument" in why, (rc, why)
    for rc, why in (run(good, x=4100), run(good, dy=8200), run(good, ws=20484), run(good, dW=12292)):      # misaligned pointers
        assert rc == -1 and "16-byte aligned" in why, (rc, why)
    assert lib.mspi_conv_wgrad_t16_variant(ctypes.byref(good), 4100, 8192) == -1 and "16-byte aligned" in err()


def _trained_names(m):
    return sorted(_entry_trained_names(m) + list(AR.STATE_KEYS.values()))


@pytest.mark.parametrize("name,total", [("x3dl", 107), ("s3d", 105), ("slowfast4x16", 103)])
def test_trainable_adapter_flags_modes_and_restore(monkeypatch, name, total):
    from mspi_amd import testing as T
    from mspi_amd._lib import MspiError
    from mspi_amd.model import model_utils as pm
    m = T.seeded(lambda: pm.AudioVisualSaliencyModel(T.make_cfg(name)), 0)
    first = next(m.visnet.parameters())
    first.requires_grad_(False)
    before = {n: p.requires_grad for n, p in m.named_parameters()}
    assert m.trainable("adapter") is m
    on = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert on == _trained_names(m) and len(on) == total and len(AR.STATE_KEYS) == 24
    assert not any(p.requires_grad for mod in (m.aud_vis_sync_block, m.visnet, m.image_encoder, m.audnet, m.vis_projector, m.mlp_aud)
                   for p in mod.parameters())
    ts, bns = m.adapter.tensors()
    state = dict(m.named_parameters())
    assert len(ts) == 24 and len(bns) == 8 and all(t is state[AR.STATE_KEYS[k]] for t, k in zip(ts, AR.PARAMS))
    m.train()
    m.frozen_encoder()
    assert sorted(n for n, s in m.named_modules() if s.training) == BN_NAMES and len(BN_NAMES) == 13 and not m.training
    assert sorted(m._batch_stat_modules()) == BN_NAMES
    m._check_eval()
    assert m._training_tail() == "cat"
    with torch.no_grad():
        assert m._training_tail() is False
    for other in (m.latlayer_0[0], m.adapter, m.adapter.conv.branch1[1], m.image_encoder):
        other.train()
        with pytest.raises(MspiError, match="under trainable\\('adapter'\\) only readout.2, readout.5, the three sa_k.conv_mask.0.bn "
                                            "and the eight BatchNorm layers of adapter.conv"):
            m._check_eval()
        m.frozen_encoder()
    m._check_eval()
    for older, tail, count in (("lateral_entries", "inputs", total - 24), ("fusion", "laterals", 31), ("readout_tail", True, 6)):
        m.trainable(older)                                      # switching over and back
        assert sum(p.requires_grad for p in m.parameters()) == count and m._training_tail() == tail
        assert not any(p.requires_grad for p in m.adapter.parameters())
        m.frozen_encoder()
        assert not any(s.training for s in m.adapter.modules())
        m.trainable("adapter")
        assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == on
    m.adapter.conv.branch0[0].bn.train()
    m.trainable("lateral_entries")
    with pytest.raises(MspiError, match="under trainable\\('lateral_entries'\\) only readout.2, readout.5 and the three"):
        m._check_eval()
    m.frozen_encoder()
    for bad in ("inception", "masks", "all", ""):
        with pytest.raises(MspiError, match="'lateral_entries' and 'adapter' are"):
            m.trainable(bad)
    m.trainable(None)
    assert {n: p.requires_grad for n, p in m.named_parameters()} == before and not first.requires_grad
    monkeypatch.setattr(pm, "DECODER_FUSED", False)
    with pytest.raises(MspiError, match="trainable\\('adapter'\\) needs the fused decoder path.*MSPI_DECODER_FUSED=0"):
        m.trainable("adapter")


def test_train_accepts_adapter_up_to_the_gpu_check(monkeypatch):
    from mspi_amd import train
    from mspi_amd._lib import MspiError
    assert train.TRAINABLE_ADAPTER == ("adapter",) and train.TRAINABLE_ENTRIES == ("lateral_entries",)
    assert train.TRAINABLE_BLOCKS == ("lateral_blocks",) and train.TRAINABLE_STAGES == ("readout_tail", "readout", "fusion")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="MI355X"):
        train.main(["--trainable", "adapter"])
    with pytest.raises(MspiError, match="--trainable inception: only readout_tail, readout can be trained on a frozen pyramid.*adapter"):
        train.main(["--trainable", "inception"])
    doc = train.__doc__
    assert "--trainable adapter" in doc and "Still frozen in all six: the SyncBlock, the contrastive projectors and every encoder" in doc


# ------------------------------------------------------------------------------------------------------------- GPU
def _geom(C, Co):
    from mspi_amd import autograd as A
    return A._geometry(*WIDTHS[(C, Co)], C, Co)


def _kernel(dev, x, dy, C, Co, bias=True, xld=None, dyld=None, dyoff=None):
    """dW [Co,Ci,kt,kh,kw] and db of the kernel; xld: x is the last C channels of rows xld wide, NaN elsewhere; dyld / dyoff: dy
    lies at channel dyoff of rows dyld wide, NaN elsewhere."""
    from mspi_amd import engine as E
    xc = _cl(x, dev, xld)
    if dyld is None:
        dc = _cl(dy, dev)
    else:
        N, _, T, H, W = dy.shape
        buf = torch.full((N, T, H, W, dyld), float("nan"), device=dev)
        buf[..., dyoff:dyoff + Co] = dy.permute(0, 2, 3, 4, 1).to(dev)
        dc = E.CL(buf.view(-1), dyoff, N, T, H, W, Co, dyld)
    return E.conv_wgrad_t16(xc, dc, _geom(C, Co), bias=bias)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C,Co", list(WIDTHS), ids=["%d_%d" % k for k in WIDTHS])
def test_hip_t16_wgrad_kernel_vs_fp64(dev, shape, C, Co):
    """dW and db of the kernel against float64 on every shape and width; twice, for equal bits; db NULL leaves dW its bits."""
    from mspi_amd import engine as E
    x, dy, (rW, rb) = _wcase(shape, C, Co)
    assert E.conv_wgrad_t16_variant(_cl(x, dev), _cl(dy, dev), _geom(C, Co)) == 64
    dW, db = _kernel(dev, x, dy, C, Co)
    assert torch.isfinite(dW).all() and torch.isfinite(db).all()
    eW, eb = _err(dW, rW), _err(db, rb)
    print("%s %d -> %d %s: dW %.2e db %.2e" % (shape, C, Co, WIDTHS[(C, Co)][0], eW, eb))
    assert eW <= GRAD_TOL and eb <= GRAD_TOL
    dW2, db2 = _kernel(dev, x, dy, C, Co)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)        # bitwise repeatable
    dW3, none = _kernel(dev, x, dy, C, Co, bias=False)
    assert none is None and torch.equal(dW, dW3)


@pytest.mark.gpu
def test_hip_t16_wgrad_neighbouring_image_does_not_leak(dev):
    """(2,2,2,3): with the second clip (and, for (1,3,3), every frame but the first) poisoned, the gradient computed from the
    first alone is what the poison leaves finite -- checked through dy = 0 there: a tap that crossed the boundary would read NaN."""
    shape = (2, 2, 2, 3)
    for (C, Co), (k, pad) in WIDTHS.items():
        x, dy, _ = _wcase(shape, C, Co)
        x, dy = x.clone(), dy.clone()
        keep = (slice(0, 1), slice(None), slice(0, 1)) if k == (1, 3, 3) else (slice(0, 1),)
        rW, rb = AR.wgrad(x[keep], dy[keep], k, pad)
        # rows outside `keep` contribute dy = 0 exactly; their x is finite but huge, the kept rows' neighbours across the boundary
        big = torch.full_like(x, 1e30)
        big[keep] = x[keep]
        zero = torch.zeros_like(dy)
        zero[keep] = dy[keep]
        dW, db = _kernel(dev, big, zero, C, Co)
        eW, eb = _err(dW, rW), _err(db, rb)
        print("%d -> %d %s: dW %.2e db %.2e beside 1e30" % (C, Co, k, eW, eb))
        assert eW <= GRAD_TOL and eb <= GRAD_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("off", DY_OFFSETS)
def test_hip_t16_wgrad_channel_slices(dev, off):
    """dy a slice of 512-wide rows at the offsets of the model's call sites, x a slice of wider rows, NaN outside both: the bits
    of the dense call."""
    C, Co = {192: (208, 208), 400: (48, 48), 448: (416, 16)}[off]
    x, dy, (rW, rb) = _wcase((2, 4, 3, 5), C, Co)
    dW, db = _kernel(dev, x, dy, C, Co)
    sW, sb = _kernel(dev, x, dy, C, Co, xld=C + 32, dyld=512, dyoff=off)
    eW, eb = _err(sW, rW), _err(sb, rb)
    print("dy at %d of 512, x the last %d of %d: dW %.2e db %.2e" % (off, C, C + 32, eW, eb))
    assert eW <= GRAD_TOL and eb <= GRAD_TOL
    assert torch.equal(sW, dW) and torch.equal(sb, db)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(VARIANTS))
def test_hip_t16_wgrad_further_variants(dev, key):
    from mspi_amd import engine as E
    shape, (C, Co), code = VARIANTS[key]
    x, dy, (rW, rb) = _wcase(shape, C, Co, seed=7)
    assert E.conv_wgrad_t16_variant(_cl(x, dev), _cl(dy, dev), _geom(C, Co)) == code and code in E.WGRAD_T16_SLICES
    dW, db = _kernel(dev, x, dy, C, Co)
    eW, eb = _err(dW, rW), _err(db, rb)
    print("%s: dW %.2e db %.2e" % (key, eW, eb))
    assert eW <= GRAD_TOL and eb <= GRAD_TOL
    dW2, db2 = _kernel(dev, x, dy, C, Co)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


@pytest.mark.gpu
@pytest.mark.parametrize("C,Co", [(96, 208), (208, 208), (416, 16)])
def test_hip_t16_wgrad_loss_scale(dev, C, Co):
    """dy x 1e-4, the scale SalLoss leaves on these layers: the same relative bar."""
    x, dy, _ = _wcase((2, 4, 3, 5), C, Co)
    small = dy * 1e-4
    rW, rb = AR.wgrad(x, small, *WIDTHS[(C, Co)])
    dW, db = _kernel(dev, x, small, C, Co)
    eW, eb = _err(dW, rW), _err(db, rb)
    print("%d -> %d x 1e-4: dW %.2e db %.2e" % (C, Co, eW, eb))
    assert eW <= GRAD_TOL and eb <= GRAD_TOL


def _taps_of(k, pad, dims, pos):
    """The taps (kt, kh, kw) through which input position pos = (t, h, w) is read by an output position inside dims."""
    taps = []
    for a in range(k[0]):
        for b in range(k[1]):
            for c in range(k[2]):
                out = (pos[0] - a + pad[0], pos[1] - b + pad[1], pos[2] - c + pad[2])
                if all(0 <= o < d for o, d in zip(out, dims)):
                    taps.append((a, b, c))
    return taps


@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("C,Co", [(16, 48), (208, 208), (416, 192)])
def test_hip_t16_wgrad_nonfinite_operands_propagate(dev, C, Co, value):
    """A poison in a used x[r][ci] reaches exactly dW[:, ci, tap] for the taps that read r, and not db; one in dy[r][co] exactly
    dW[co] and db[co]."""
    shape = (2, 4, 3, 5)
    B, T, h, w = shape
    k, pad = WIDTHS[(C, Co)]
    x, dy, (rW, rb) = _wcase(shape, C, Co)
    for ci, pos in ((1, (0, 0, 0)), (C - 1, (T - 1, h - 1, w // 2)), (C // 2, (1, 1, 2))):
        dW, db = _kernel(dev, _poisoned(x, (B - 1, ci) + pos, value), dy, C, Co)
        ref = rW.clone()
        taps = _taps_of(k, pad, (T, h, w), pos)
        assert taps
        for tap in taps:
            ref[(slice(None), ci) + tap] = float("nan")
        _judge("%d -> %d x[ci %d, %s] -> dW" % (C, Co, ci, pos), dW, ref)
        assert torch.isfinite(db).all() and _err(db, rb) <= GRAD_TOL
    for co in (0, Co // 2 + 1, Co - 1):
        dW, db = _kernel(dev, x, _poisoned(dy, (0, co, 0, h // 2, w - 1), value), C, Co)
        refW, refb = rW.clone(), rb.clone()
        refW[co] = float("nan")
        refb[co] = float("nan")
        _judge("%d -> %d dy[co %d] -> dW" % (C, Co, co), dW, refW)
        _judge("%d -> %d dy[co %d] -> db" % (C, Co, co), db, refb)


@pytest.mark.gpu
def test_hip_t16_wgrad_capture_and_replay(dev):
    """The raw entry point, the first call included: operands and the host descriptor overwritten between capture and replay."""
    from mspi_amd import _lib
    lib = _lib.load()
    shape = (2, 4, 3, 5)
    B, T, h, w = shape
    for (C, Co) in ((96, 208), (48, 48), (416, 16)):
        k, pad = WIDTHS[(C, Co)]

        def operands(seed):
            x, dy, _ = _wcase(shape, C, Co, seed=seed)
            return {"x": x.permute(0, 2, 3, 4, 1).contiguous(), "dy": dy.permute(0, 2, 3, 4, 1).contiguous()}

        def launch(t, host):
            d = _desc(N=B, T=T, H=h, W=w, C=C, Cout=Co, k=k, pad=pad)
            host.append(d)                                          # the descriptor: read during the call, overwritten before the replay
            dW, db = torch.empty(Co, k[0] * k[1] * k[2] * C, device=dev), torch.empty(Co, device=dev)
            ws = torch.empty(lib.mspi_conv_wgrad_t16_ws_bytes(ctypes.byref(d)) // 4, device=dev)
            _lib.check(lib.mspi_conv_wgrad_t16(ctypes.byref(d), t["x"].data_ptr(), t["dy"].data_ptr(), dW.data_ptr(), db.data_ptr(),
                                               ws.data_ptr(), _stream()), "mspi_conv_wgrad_t16")
            return {"dW": dW, "db": db}
        _replayed(dev, {"A": operands(41), "B": operands(42)}, launch)


@pytest.mark.gpu
def test_hip_adapter_wgrad_routes(dev):
    """adapter_wgrad goes to the wide kernel from 8192 rows on where that kernel takes the layer, to the new one everywhere
    else; at the threshold, on the narrowest layer that switches (416 -> 64), both routes against float64."""
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    assert E.WGRAD_T16_ROWS == (1024, 8192)
    for c, co in ((416, 192), (416, 96), (416, 64)):
        assert A.adapter_wgrad_route(8191, c, co) == "t16" and A.adapter_wgrad_route(8192, c, co) == "wide"
    for c, co in ((96, 208), (208, 208), (416, 16), (16, 48), (48, 48)):
        assert A.adapter_wgrad_route(1 << 20, c, co) == "t16"
    gen = torch.Generator().manual_seed(5)
    x, dy = torch.randn(1, 416, 2, 64, 64, generator=gen), torch.randn(1, 64, 2, 64, 64, generator=gen)
    rW, _ = AR.wgrad(x, dy, *K111)
    geo = A._geometry(*K111, 416, 64)
    xc, dc = _cl(x, dev), _cl(dy, dev)
    with E.Profiler() as prof:
        routed = A.adapter_wgrad(xc, dc, geo)
        torch.cuda.synchronize()
    assert "conv_wgrad_wide" in prof.summary() and "conv_wgrad_t16" not in prof.summary()
    new = E.conv_wgrad_t16(xc, dc, geo)[0]
    e_w, e_n = _err(routed, rW), _err(new, rW)
    print("8192 rows 416 -> 64: wide %.2e t16 %.2e" % (e_w, e_n))
    assert e_w <= GRAD_TOL and e_n <= GRAD_TOL
    with E.Profiler() as prof:
        A.adapter_wgrad(_cl(x[:, :, :1], dev), _cl(dy[:, :, :1], dev), geo)
        torch.cuda.synchronize()
    assert "conv_wgrad_t16" in prof.summary() and "conv_wgrad_wide" not in prof.summary()


# ---- the stages
def _fusion_run(fp, dev, masks_grad):
    """One forward and backward of autograd.Fusion on sum_j <s_j, G_j>: ({name: gradient of the 19 others}, dmasks or None)."""
    from mspi_amd.autograd import Fusion
    lats, masks, sa, bn = _fusion_args(fp, dev)
    masks.requires_grad_(masks_grad)
    maps = Fusion.apply(*lats, masks, *sa, *bn)
    Gs = [torch.from_numpy(fp[g]).to(dev).permute(0, 2, 3, 4, 1).contiguous() for g in FR.GRADS]
    sum((s * g).sum() for s, g in zip(maps, Gs)).backward()
    grads = {k: p.grad for k, p in zip(FR.SA_PARAMS + FR.LATERALS, sa + lats)}
    return grads, (masks.grad.permute(0, 4, 1, 2, 3) if masks_grad else None)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["fusion_tiny", "fusion_odd"])
def test_hip_fusion_returns_the_gradient_of_masks(dev, key):
    fp, ref = _fusion_case(key)
    plain, none = _fusion_run(fp, dev, False)
    grads, dm = _fusion_run(fp, dev, True)
    assert none is None and dm is not None and torch.isfinite(dm).all()
    e = _err(dm, ref)
    print("%s: dmasks %.2e" % (key, e))
    assert e <= GRAD_TOL
    assert len(plain) == 19
    for k in plain:                                                # the other 19 keep their bits
        assert torch.equal(grads[k], plain[k]), k


def _adapter_args(case, dev, buffers=True):
    """(cat, the 24 tensors as leaves, the eight buffer triples) on the device, fresh buffers (0, 1, 0)."""
    cat = torch.from_numpy(case["cat"]).to(dev).permute(0, 2, 3, 4, 1).contiguous()
    ts = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in AR.PARAMS]
    bns = [(torch.zeros(case["gam_%s" % l].shape[0], device=dev), torch.ones(case["gam_%s" % l].shape[0], device=dev),
            torch.zeros((), dtype=torch.long, device=dev)) for l in AR.LAYERS] if buffers else [None] * 8
    return cat, ts, bns


def _adapter_run(case, dev):
    from mspi_amd.autograd import Adapter
    cat, ts, bns = _adapter_args(case, dev)
    keep = cat.clone()
    masks = Adapter.apply(cat, *ts, *bns)
    masks.backward(torch.from_numpy(case["G"]).to(dev).permute(0, 2, 3, 4, 1).contiguous())
    assert torch.equal(cat, keep) and cat.grad is None
    return masks.detach(), {k: p.grad for k, p in zip(AR.PARAMS, ts)}, bns


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(CASES))
def test_hip_adapter_end_to_end(dev, key):
    """masks, all 24 gradients and the eight updated running-statistic triples against the restatement; twice the same bits."""
    case, sv, ref = _restated(key)
    masks, grads, bns = _adapter_run(case, dev)
    e = _err(masks.permute(0, 4, 1, 2, 3), sv["masks"])
    print("%s: masks %.2e" % (key, e))
    assert e <= GRAD_TOL
    for k in AR.PARAMS:
        assert grads[k] is not None and grads[k].shape == ref[k].shape and torch.isfinite(grads[k]).all(), k
        e = _err(grads[k], ref[k])
        print("%s: d %s %.2e" % (key, k, e))
        assert e <= GRAD_TOL, k
    for l, (rm, rv, nbt) in zip(AR.LAYERS, bns):
        want_m, want_v = AR.running_stats(sv[l])
        e_m, e_v = (rm.double().cpu() - want_m).abs().max().item(), _err(rv, want_v)
        print("%s %s: running mean %.2e (absolute), running var %.2e" % (key, l, e_m, e_v))
        assert e_m <= GRAD_TOL * max(1.0, want_m.abs().max().item()) and e_v <= GRAD_TOL and int(nbt) == 1
    masks2, grads2, _ = _adapter_run(case, dev)
    assert torch.equal(masks2, masks) and all(torch.equal(grads2[k], grads[k]) for k in AR.PARAMS)


@pytest.mark.gpu
def test_hip_adapter_refuses_by_name(dev):
    from mspi_amd.autograd import Adapter
    from mspi_amd._lib import MspiError
    case = _restated("tiny")[0]
    cat, ts, bns = _adapter_args(case, dev)
    with pytest.raises(MspiError, match="expected 24 tensors and 8 BatchNorm buffer triples after cat, got 31"):
        Adapter.apply(cat, *ts, *bns[:7])
    with pytest.raises(MspiError, match="GPU only"):
        Adapter.apply(cat.cpu(), *[t.detach().cpu() for t in ts], *[None] * 8)
    with pytest.raises(MspiError, match="cat must be fp32 \\[B,T,h,w,C\\]"):
        Adapter.apply(cat[0], *ts, *bns)
    with pytest.raises(MspiError, match="layer b0 has conv.weight .* it reads 48 channels"):
        Adapter.apply(torch.cat([cat, cat[..., :16]], 4), *ts, *bns)
    bad = list(ts)
    bad[3 * 2] = torch.randn(32, 16, 3, 1, 1, device=dev)          # b1s with conv_t's kernel
    with pytest.raises(MspiError, match="layer b1s has conv.weight"):
        Adapter.apply(cat, *bad, *bns)
    narrow = AR.make_case(1, 2, 2, 3, 1, (24, 16, 16, 32, 16, 16, 16))
    c2, t2, b2 = _adapter_args(narrow, dev)
    with pytest.raises(MspiError, match="layer b0 is 24 -> 16 wide; the widths must be multiples of 16"):
        Adapter.apply(c2, *t2, *b2)
    out = Adapter.apply(cat, *ts, *[None] * 8)                      # without buffers: nothing to update
    assert tuple(out.shape) == (1, 2, 2, 3, 80) and out.requires_grad


# ---- the whole model
@pytest.mark.gpu
@pytest.mark.parametrize("case,name,cls,entries_total", MODELS, ids=[m[0] for m in MODELS])
def test_hip_whole_model_trains_its_adapter(dev, golden_dir, monkeypatch, case, name, cls, entries_total):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    from mspi_amd import metrics as M
    from mspi_amd._lib import MspiError
    from mspi_amd.model import model_utils as pm
    from test_readout_tail import _batches, _build
    total = entries_total + 24
    E.autotune(False)          # bits are compared, and an empty cache pins the library's own kernel choices
    monkeypatch.setitem(E.AUTOTUNE, "cache", {})      # (tests/test_lateral_train.py::test_hip_whole_model_trains_its_lateral_blocks says why)
    sound = cls == "AudioVisualSaliencyModel"
    g, cfg, make, clips, audio = _build(golden_dir, case, name, cls, dev)
    args = (clips, audio) if sound else (clips,)
    m = make().to(dev)
    off = m(*args)[0]
    label = _batches(clips, audio, 1, True)[0][2].to(dev)
    m.trainable("adapter")
    m.eval()
    with pytest.raises(MspiError, match="trainable\\('adapter'\\): a forward with grad runs .*adapter.conv.branch0.0.bn.*frozen_encoder"):
        m(*args)
    m.train()
    m.frozen_encoder()
    with torch.no_grad():      # the switch on under no_grad: the launches of inference, the switch-off map's bits
        quiet = m(*args)[0]
    assert torch.equal(quiet, off) and not quiet.requires_grad

    calls = []

    class Recorded:
        @staticmethod
        def apply(cat, *rest):
            masks = A.Adapter.apply(cat, *rest)
            rec = {"cat": cat.detach().clone()}
            masks.register_hook(lambda gr, rec=rec: rec.__setitem__("G", gr.detach().clone()))
            calls.append(rec)
            return masks
    monkeypatch.setattr(pm, "AdapterTrain", Recorded)

    def step_grads():
        for p in m.parameters():
            p.grad = None
        out = m(*args)[0]
        assert out.requires_grad
        M.SalLoss()(out, label).backward()
        return out.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    start = {k: v.clone() for k, v in m.state_dict().items()}
    params = [p for p in m.parameters() if p.requires_grad]
    assert len(params) == total
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0)
    out1, grads = step_grads()
    out2, grads2 = step_grads()
    monkeypatch.setattr(pm, "AdapterTrain", A.Adapter)
    assert sorted(grads) == _trained_names(m) and len(grads) == total and len(calls) == 2
    assert all(torch.isfinite(gr).all() for gr in grads.values())
    assert torch.equal(out1, out2) and all(torch.equal(grads2[n], grads[n]) for n in grads)      # twice the same bits
    # the adapter's 24 gradients against the float64 restatement, fed this very run's cat and dmasks
    rec = calls[0]
    state = {k: v for k, v in start.items()}
    p = {"widths": AR.WIDTHS, "cat": rec["cat"].permute(0, 4, 1, 2, 3).cpu().numpy()}
    p.update({k: state[AR.STATE_KEYS[k]].cpu().numpy() for k in AR.PARAMS})
    ref = AR.backward(p, AR.forward(p), G=rec["G"].permute(0, 4, 1, 2, 3).cpu())
    for k in AR.PARAMS:
        e = _err(grads[AR.STATE_KEYS[k]], ref[k])
        print("%s d %s: %.2e" % (case, k, e))
        assert e <= GRAD_TOL, k
    opt.step()
    moved = set(_trained_names(m)) | {"%s.%s" % (mod, n) for mod in BN_NAMES for n in ("running_mean", "running_var", "num_batches_tracked")}
    # AdamW without weight decay leaves a tensor whose gradient is exactly zero where it is; the true gradient of
    # readout.12.bias IS zero (tests/test_entry_train.py says why): only that tensor may stand still
    still = {n for n in _trained_names(m) if not grads[n].any()}
    print("%s: gradient exactly zero: %s" % (case, sorted(still)))
    assert still <= {"readout.12.bias"}
    for k, v in m.state_dict().items():
        assert torch.equal(v, start[k]) == (k not in moved - still), k
    with torch.no_grad():
        trained = m(*args)[0]
    assert not torch.equal(trained, off) and torch.isfinite(trained).all()
    fresh = make()
    fresh.load_state_dict(m.state_dict())
    again = fresh.to(dev)(*args)[0]
    assert torch.equal(again, trained)             # the no-grad forward uses the stepped values and the new running statistics
    m.trainable(None)
    m.eval()
    plain = m(*args)[0]
    assert torch.equal(plain, trained) and not plain.requires_grad
