"""The trainable SA gating and top-down fusion: csrc/fusion_bwd.hip (mspi_rowgate_bwd, mspi_upsample_sum_bwd, declared in
include/mspi_train_hip.h), engine.rowgate_bwd / upsample_sum_bwd, autograd.Fusion, the map gradients of autograd.ReadoutHead,
_SaliencyBase.trainable("fusion"), mspi_amd.train --trainable fusion.

Yardsticks: tests/golden/fusion.npz holds "tiny" ((B, T, a, b) = (1, 1, 1, 2), D = Cm = mid = 32) as its seed and, in float64,
the four maps and the gradients of sum_j <s_j, G_j> for the 15 SA tensors and the four laterals that torch autograd gives
through torch.nn layers with upstream's arguments (tools/gen_fusion_golden.py), and the seed of "odd" ((2, 2, 2, 3));
tests/fusion_restate.py is the float64 restatement in this project's order with its analytic backward, pinned to that fixture
and, here, to torch autograd on "odd".

Bounds.  Every gradient tensor: max |got - ref| / max |ref| <= GRAD_TOL = 2e-5, the project's bar for gradients
(tests/test_readout_train.py); every test prints its figure before it asserts.  Maps: MAP_TOL.  Adjoint identities: 1e-5 of
the sum of the absolute terms, accumulated in float64 on the host.  The ledger part holds the two entry points to what
tests/test_capi_host.py, tests/test_launch_ledger.py and tests/test_nonfinite_ledger.py hold every entry point of mspi_hip.h
to: declared = exported = bound, capture + replay with the operands and host arrays overwritten in between, and a NaN / +Inf in
each floating operand reaching every output that depends on it and no other.

ReLU kinks.  End to end only inputs are compared on which torch fp32 on the CPU agrees with float64 (no unit on its kink):
"tiny" and "odd" (2.8e-7, 4.6e-7) and the product's channel counts on (1, 1, 1, 2) with seed 0 (3.7e-6, rounding of the 13824-term
sums)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import fusion_restate as FR
import readout_restate as R
from test_parity_gpu import MAP_TOL
from test_readout_train import GRAD_TOL, _cl, _dot, _err, _ncdhw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_rowgate_bwd", "mspi_upsample_sum_bwd")
CASES = ("tiny", "odd")
SHAPES = {"tiny": (1, 1, 1, 2), "odd": (2, 2, 2, 3)}
NAMES = FR.SA_PARAMS + FR.LATERALS
PRODUCT = dict(D=192, Cm=512, mid=32)


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fusion.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _restated(key):
    """(case, saved, grads) in float64, computed once: a fixture case by name, or "product" (the product's channel counts)."""
    if key == "product":
        case = FR.make_case(1, 1, 1, 2, seed=0, zeros=True, **PRODUCT)
    else:
        case = FR.make_case(*SHAPES[key], seed=int(_gold()["%s_seed" % key]))
    saved = FR.forward(case)
    return case, saved, FR.backward(case, saved, [case[g] for g in FR.GRADS])


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["cases"]) == CASES
    for c in CASES:
        assert tuple(g["%s_shape" % c]) == SHAPES[c]
    shapes = FR.param_shapes(32, 32)
    case = _restated("tiny")[0]
    for k in FR.SA_PARAMS:
        assert g["tiny_d_%s" % k].shape == shapes[k] and g["tiny_d_%s" % k].dtype == np.float64
    for j in range(4):
        assert g["tiny_d_l%d" % j].shape == case["l%d" % j].shape == g["tiny_s%d" % j].shape and g["tiny_s%d" % j].dtype == np.float64
    assert len(FR.SA_PARAMS) == 15
    golden = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(golden, "fusion.npz")) <= os.path.getsize(os.path.join(golden, "readout.npz"))


def test_restatement_matches_the_fixture():
    g = _gold()
    case, saved, grads = _restated("tiny")
    for j in range(4):
        assert (saved["s%d" % j] - torch.from_numpy(g["tiny_s%d" % j])).abs().max().item() <= 1e-12
    for k in NAMES:
        assert _err(grads[k], g["tiny_d_%s" % k]) <= 1e-12, k


def test_restatement_matches_torch_autograd_on_odd():
    """ "odd" is stored as its seed: torch.nn layers with upstream's arguments, .train() BatchNorm, float64, built here."""
    case, saved, grads = _restated("odd")
    maps, ref, mods = FR.upstream_grads(case)
    for j in range(4):
        assert (saved["s%d" % j] - maps[j]).abs().max().item() <= 1e-12
    for k in NAMES:
        assert _err(grads[k], ref[k]) <= 1e-12, k
    rm, rv = FR.running_stats(saved["bn"], saved["pre"].numel() // saved["pre"].shape[1])
    for k in range(3):
        bn = mods[k][0].bn
        assert _err(rm[32 * k:32 * k + 32], bn.running_mean) <= 1e-12 and _err(rv[32 * k:32 * k + 32], bn.running_var) <= 1e-12
        assert (bn.eps, bn.momentum, int(bn.num_batches_tracked)) == (FR.EPS, FR.MOMENTUM, 1)


def test_the_model_builds_the_gates_the_restatement_assumes():
    from mspi_amd import autograd as A
    m = _model()
    for k in range(3):
        sa = getattr(m, "sa_%d" % k)
        assert (sa.k, sa.conv_mask[0].bn.eps, sa.conv_mask[0].bn.momentum) == (FR.FACTORS[k], FR.EPS, FR.MOMENTUM)
    assert (A.SA_FACTORS, A.SA_BN_EPS, A.SA_BN_MOMENTUM) == (FR.FACTORS, FR.EPS, FR.MOMENTUM)
    assert sorted(FR.STATE_KEYS.values()) == sorted(n for n, _ in m.named_parameters() if n.startswith("sa_"))


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(mspi_[a-z0-9_]+)\s*\(", text)), text


def test_new_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    from mspi_amd import engine as E
    train, _ = _declared("mspi_train_hip.h")
    base, base_text = _declared("mspi_hip.h")
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert train == set(NEW_SYMBOLS) == set(_lib.TRAIN_EXPORTS) == set(_lib._TRAIN_SIGNATURES)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _lib._TRAIN_SIGNATURES[name][1], name
    # the pinned symbol set is as it was: no new name in mspi_hip.h or EXPORTS, the ABI version unchanged
    assert base == set(_lib.EXPORTS) and not base & set(NEW_SYMBOLS) and not set(_lib.EXPORTS) & set(NEW_SYMBOLS)
    assert re.search(r"#define MSPI_ABI_VERSION 2\b", base_text) and lib.mspi_version() == 2
    for name in ("rowgate_bwd", "upsample_sum_bwd"):
        assert callable(getattr(E, name)) and name in E.__all__
    src = open(os.path.join(ROOT, "mspi_amd", "csrc", "fusion_bwd.hip")).read()
    assert "atomic" not in src.lower().replace("no float atomics", "")
    mk = open(os.path.join(ROOT, "mspi_amd", "csrc", "Makefile")).read()
    assert "fusion_bwd.hip" in mk and "mspi_train_hip.h" in mk and "-fno-slp-vectorize" in mk


def test_host_refusals():
    from mspi_amd import _lib
    lib = _lib.load()

    def rgb(dy=4096, lddy=8, x=8192, ldx=8, gate=12288, dx=16384, lddx=8, dz=20480, M=3, C=8):
        return lib.mspi_rowgate_bwd(dy, lddy, x, ldx, gate, dx, lddx, dz, M, C, None), lib.mspi_last_error().decode()

    def usb(factors=(2,), ptrs=None, lds=None, dx=4096, lddx=8, NT=1, H=1, W=1, C=8, J=None):
        J = len(factors) if J is None else J
        n = max(len(factors), 1)
        p = (ctypes.c_void_p * n)(*(ptrs or [8192 + 4096 * j for j in range(n)]))
        ld = (ctypes.c_int64 * n)(*(lds or [C] * n))
        ks = (ctypes.c_int32 * n)(*factors)
        return lib.mspi_upsample_sum_bwd(p, ld, ks, J, dx, lddx, NT, H, W, C, 0, None), lib.mspi_last_error().decode()

    for rc, why in (rgb(C=6), rgb(lddy=6), rgb(ldx=4), rgb(lddx=10), rgb(dy=4100), rgb(x=8200), rgb(dx=16388)):
        assert rc == -1 and "mspi_rowgate_bwd" in why and "multiples of 4" in why, (rc, why)
    for rc, why in (rgb(dz=None), rgb(gate=None), rgb(dy=None)):
        assert rc == -1 and "null argument" in why, (rc, why)
    assert rgb(M=0)[0] == -1 and "bad extent" in rgb(M=0)[1]
    for rc, why in (usb(C=6, lddx=6), usb(lds=[6]), usb(lddx=4), usb(dx=4100), usb(ptrs=[8200])):
        assert rc == -1 and "mspi_upsample_sum_bwd" in why and "multiples of 4" in why, (rc, why)
    rc, why = usb(factors=(2, 2, 2, 2))
    assert rc == -1 and "1 to 3 sources" in why
    assert usb(factors=(2,), J=0)[0] == -1
    for f in (3, 1, 16):
        rc, why = usb(factors=(2, f))
        assert rc == -1 and "2, 4 or 8" in why, (f, rc, why)
    assert usb(ptrs=[None])[0] == -1 and usb(dx=None)[0] == -1
    assert usb(NT=1 << 20, H=64, W=64, C=64, lddx=64)[0] == -1 and "2^31" in lib.mspi_last_error().decode()


def _model():
    from mspi_amd import testing as T
    from mspi_amd.model.model_utils import AudioVisualSaliencyModel
    return T.seeded(lambda: AudioVisualSaliencyModel(T.make_cfg("x3dl")), 0)


BATCH_STAT = ["readout.2", "readout.5", "sa_0.conv_mask.0.bn", "sa_1.conv_mask.0.bn", "sa_2.conv_mask.0.bn"]


def test_trainable_fusion_flags_modes_and_restore(monkeypatch):
    from mspi_amd._lib import MspiError
    from mspi_amd.model import model_utils as pm
    m = _model()
    first = next(m.visnet.parameters())
    first.requires_grad_(False)
    before = {n: p.requires_grad for n, p in m.named_parameters()}
    assert m.trainable("fusion") is m
    on = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert on == sorted(list(R.STATE_KEYS.values()) + list(FR.STATE_KEYS.values())) and len(on) == 31
    m.train()
    m.frozen_encoder()
    assert sorted(n for n, s in m.named_modules() if s.training) == BATCH_STAT and not m.training
    m._check_eval()                                             # the forward's guard lets exactly these five through
    for other in (m.readout[1], m.sa_0, m.sa_1.conv_mask[0], m.latlayer_0, m.adapter):
        other.train()
        with pytest.raises(MspiError, match="under trainable\\('fusion'\\) only readout.2, readout.5 and the three"):
            m._check_eval()
        m.frozen_encoder()                                      # back to the five
    m._check_eval()
    m.trainable("readout")                                      # switching over: the readout's own guard and message
    m.frozen_encoder()
    assert sorted(n for n, s in m.named_modules() if s.training) == ["readout.2", "readout.5"]
    m.sa_0.conv_mask[0].bn.train()
    with pytest.raises(MspiError, match="only readout.2 and readout.5"):
        m._check_eval()
    m.trainable("fusion")
    for bad in ("decoder", "all", ""):
        with pytest.raises(MspiError, match="readout_tail"):
            m.trainable(bad)
    m.trainable(None)
    assert {n: p.requires_grad for n, p in m.named_parameters()} == before and not first.requires_grad
    monkeypatch.setattr(pm, "DECODER_FUSED", False)
    with pytest.raises(MspiError, match="MSPI_DECODER_FUSED"):
        m.trainable("fusion")


def test_sa_key_follows_parameters_and_running_statistics():
    m = _model()
    assert m._PK_SELF_KEYED == ("readout", "sa_0", "sa_1", "sa_2")
    key = m._sa_key()
    assert m._sa_key() == key and len(key) == 15
    with torch.no_grad():
        m.sa_1.conv_mask[0].bn.running_var.mul_(2.0)
    k2 = m._sa_key()
    assert k2 != key
    with torch.no_grad():
        m.sa_2.conv_mask[0].conv.weight.add_(1.0)
    k3, h3 = m._sa_key(), m._head_key()
    assert k3 != k2
    with torch.no_grad():
        m.sa_0.conv_mask[2].bias.add_(1.0)                      # the gate's second conv is sa_0's own plan, not the shared fold
    assert m._sa_key() == k3 and m._head_key() == h3


def test_train_accepts_fusion_up_to_the_gpu_check(monkeypatch):
    from mspi_amd import train
    from mspi_amd._lib import MspiError
    assert train.TRAINABLE == ("readout_tail", "readout") and train.TRAINABLE_STAGES == train.TRAINABLE + ("fusion",)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="MI355X"):
        train.main(["--trainable", "fusion"])
    with pytest.raises(MspiError, match="--trainable decoder: only readout_tail, readout can be trained on a frozen pyramid, and fusion"):
        train.main(["--trainable", "decoder"])
    assert "--trainable fusion" in train.__doc__ and "Still frozen" in train.__doc__


# ------------------------------------------------------------------------------------------------------------- GPU
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rgb_case(M, C, seed):
    """dy, x [M, C] and gate [M] in fp32 (from four rows on: gates at 0, 1 and 0.5 on the first three) and the float64 (dx, dz)."""
    gen = torch.Generator().manual_seed(seed)
    dy, x, gate = torch.randn(M, C, generator=gen), torch.randn(M, C, generator=gen), torch.rand(M, generator=gen)
    if M >= 4:
        gate[:3] = torch.tensor([0.0, 1.0, 0.5])
    return dy, x, gate, _rgb_ref(dy, x, gate)


def _rgb_ref(dy, x, gate):
    g = gate.double()
    return dy.double() * (1 + g)[:, None], g * (1 - g) * (dy.double() * x.double()).sum(1)


def _rgb_raw(dy, lddy, x, ldx, gate, dx, lddx, M, C):
    """mspi_rowgate_bwd on device buffers as they stand (dx None: the NULL form); returns dz."""
    from mspi_amd import _lib
    lib = _lib.load()
    dz = torch.full((M,), float("nan"), device=gate.device)
    _lib.check(lib.mspi_rowgate_bwd(dy.data_ptr(), lddy, x.data_ptr(), ldx, gate.data_ptr(), None if dx is None else dx.data_ptr(),
                                    lddx, dz.data_ptr(), M, C, _stream()), "mspi_rowgate_bwd")
    return dz


@pytest.mark.gpu
@pytest.mark.parametrize("C", [4, 36, 192])
@pytest.mark.parametrize("M", [1, 255, 257, 4099])
def test_hip_rowgate_bwd_vs_fp64(dev, M, C):
    from mspi_amd import engine as E
    dy, x, gate, (rdx, rdz) = _rgb_case(M, C, 100 * C + M)
    d, v, g = (E.CL(t.to(dev).reshape(-1), 0, M, 1, 1, 1, c, c) for t, c in ((dy, C), (x, C), (gate, 1)))
    runs = [E.rowgate_bwd(d, v, g) for _ in range(2)]
    dx, dz = runs[0]
    e_dx, e_dz = _err(dx.as_rows(), rdx), _err(dz, rdz)
    print("M=%d C=%d: dx %.2e, dz %.2e of the largest entry" % (M, C, e_dx, e_dz))
    assert e_dx <= GRAD_TOL and e_dz <= GRAD_TOL
    if M >= 4:
        assert torch.equal(dz[:2], torch.zeros(2, device=dev))                      # gates at 0 and 1: g (1 - g) is exactly 0
    assert torch.equal(runs[1][0].buf, dx.buf) and torch.equal(runs[1][1], dz)      # repeatable
    none, dz2 = E.rowgate_bwd(d, v, g, need_dx=False)
    assert none is None and torch.equal(dz2, dz)


@pytest.mark.gpu
def test_hip_rowgate_bwd_strides_alias_and_null(dev):
    M, C = 257, 36
    dy, x, gate, (rdx, rdz) = _rgb_case(M, C, 7)
    wide = {}
    for name, t, ld in (("dy", dy, 40), ("x", x, 48), ("dx", torch.zeros(M, C), 44)):
        buf = torch.full((M, ld), float("nan"), device=dev)      # NaN in the padding: nothing may read or write it
        buf[:, :C] = t.to(dev)
        wide[name] = buf
    g = gate.to(dev)
    dz = _rgb_raw(wide["dy"], 40, wide["x"], 48, g, wide["dx"], 44, M, C)
    torch.cuda.synchronize()
    e_dx, e_dz = _err(wide["dx"][:, :C], rdx), _err(dz, rdz)
    print("strided: dx %.2e, dz %.2e" % (e_dx, e_dz))
    assert e_dx <= GRAD_TOL and e_dz <= GRAD_TOL and torch.isnan(wide["dx"][:, C:]).all()
    dense_dx = wide["dx"][:, :C].clone()
    # dx == NULL: the same dz, nothing else written; dx == dy: the same dx, in place
    keep = wide["dy"].clone()
    dz_null = _rgb_raw(wide["dy"], 40, wide["x"], 48, g, None, 0, M, C)
    assert torch.equal(dz_null, dz) and torch.equal(wide["dy"].nan_to_num(7.0), keep.nan_to_num(7.0))
    dz_alias = _rgb_raw(wide["dy"], 40, wide["x"], 48, g, wide["dy"], 40, M, C)
    assert torch.equal(dz_alias, dz) and torch.equal(wide["dy"][:, :C], dense_dx) and torch.isnan(wide["dy"][:, C:]).all()


def _usb_case(factors, H, W, C, seed, NT=2):
    gen = torch.Generator().manual_seed(seed)
    dys = [torch.randn(NT, C, 1, H * k, W * k, generator=gen) for k in factors]
    prev = torch.randn(NT, C, 1, H, W, generator=gen)
    ref = sum(R.up_t(d.double(), k) for d, k in zip(dys, factors))
    return dys, prev, ref


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5)])
@pytest.mark.parametrize("factors", [(2,), (4,), (8,), (2, 4), (8, 2), (2, 4, 8), (4, 4, 2)], ids=lambda f: "k" + "_".join(map(str, f)))
def test_hip_upsample_sum_bwd_is_the_adjoint(dev, factors, H, W):
    """sum_j <up_kj(x), dy_j> = <x, upsample_sum_bwd(dys)>, the result against float64, against the chain of upsample_bwd
    launches and adds it replaces, with and without accumulate, twice."""
    from mspi_amd import engine as E
    for C in (4, 36):
        dys, prev, ref = _usb_case(factors, H, W, C, 1000 * C + 10 * H + len(factors))
        srcs = [(_cl(d, dev), k) for d, k in zip(dys, factors)]
        got = E.upsample_sum_bwd(None, srcs)
        e = _err(_ncdhw(got), ref)
        x = torch.randn(2, C, 1, H, W, generator=torch.Generator().manual_seed(C))
        xc = _cl(x, dev)
        lhs = sum(_dot(_ncdhw(E.upsample(xc, k)), d) for d, k in zip(dys, factors))
        rhs = _dot(x, _ncdhw(got))
        f64 = sum(_dot(R.up(x.double(), k), d) for d, k in zip(dys, factors))
        scale = sum((R.up(x.double(), k) * d.double()).abs().sum().item() for d, k in zip(dys, factors))
        print("k=%s %dx%d C=%d: %.2e of the largest entry; <up x, dy> = %.9e, <x, adjoint> = %.9e, float64 %.9e"
              % (factors, H, W, C, e, lhs, rhs, f64))
        assert e <= GRAD_TOL and abs(lhs - rhs) <= 1e-5 * scale and abs(rhs - f64) <= 1e-5 * scale
        chain = [E.upsample_bwd(s, k) for s, k in srcs]
        if len(factors) == 1:
            assert torch.equal(got.buf, chain[0].buf)           # one source: mspi_upsample_bwd's bits
        acc = _cl(prev, dev)
        summed = acc.buf.clone()
        for t in chain:
            summed = summed + t.buf
        out = E.upsample_sum_bwd(acc, srcs, accumulate=True)
        assert out is acc
        e_acc, e_chain = _err(_ncdhw(acc), prev.double() + ref), _err(acc.buf, summed.double().cpu())
        print("    accumulate: %.2e against float64, %.2e against the chain" % (e_acc, e_chain))
        assert e_acc <= GRAD_TOL and e_chain <= 2.0 ** -21      # the same terms added in the same order: fp32 rounding at most
        again = E.upsample_sum_bwd(None, srcs)
        acc2 = _cl(prev, dev)
        E.upsample_sum_bwd(acc2, srcs, accumulate=True)
        assert torch.equal(again.buf, got.buf) and torch.equal(acc2.buf, acc.buf)


@pytest.mark.gpu
def test_hip_engine_wrappers_refuse_by_name(dev):
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    d = _cl(torch.zeros(1, 8, 1, 4, 4), dev)
    with pytest.raises(MspiError, match="rowgate_bwd: gate must hold one value per row"):
        E.rowgate_bwd(d, d, d)
    with pytest.raises(MspiError, match="rowgate_bwd: dy"):
        E.rowgate_bwd(d, _cl(torch.zeros(1, 4, 1, 4, 4), dev), E.CL(torch.zeros(16, device=dev), 0, 1, 1, 4, 4, 1, 1))
    with pytest.raises(MspiError, match="upsample_sum_bwd: 1 to 3 sources"):
        E.upsample_sum_bwd(None, [])
    with pytest.raises(MspiError, match="upsample_sum_bwd: factor 3"):
        E.upsample_sum_bwd(None, [(d, 3)])
    with pytest.raises(MspiError, match="upsample_sum_bwd: accumulate needs"):
        E.upsample_sum_bwd(None, [(d, 2)], accumulate=True)
    with pytest.raises(MspiError, match="upsample_sum_bwd: a dense gradient"):
        E.upsample_sum_bwd(None, [(d, 2), (d, 4)])
    with pytest.raises(MspiError, match="GPU only"):
        E.rowgate_bwd(_cl(torch.zeros(1, 8, 1, 4, 4), "cpu"), d, d)


# ---- autograd.Fusion
def _fusion_args(case, dev, buffers=True, lat_grad=True):
    """(laterals, masks, the 15 SA tensors as leaves, the three buffer triples) on the device, fresh buffers (0, 1, 0)."""
    lats = [torch.from_numpy(case[k]).to(dev).permute(0, 2, 3, 4, 1).contiguous().requires_grad_(lat_grad) for k in FR.LATERALS]
    masks = torch.from_numpy(case["masks"]).to(dev).permute(0, 2, 3, 4, 1).contiguous()
    sa = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in FR.SA_PARAMS]
    mid = case["gam_0"].shape[0]
    bn = [(torch.zeros(mid, device=dev), torch.ones(mid, device=dev), torch.zeros((), dtype=torch.long, device=dev))
          for _ in range(3)] if buffers else [None] * 3
    return lats, masks, sa, bn


def _fusion(case, dev, gscale=1.0, lat_grad=True):
    """One forward and backward of autograd.Fusion on sum_j <s_j, G_j> * gscale: (maps in NCDHW, {name: gradient})."""
    from mspi_amd.autograd import Fusion
    lats, masks, sa, bn = _fusion_args(case, dev, lat_grad=lat_grad)
    keep = [t.detach().clone() for t in lats]
    maps = Fusion.apply(*lats, masks, *sa, *bn)
    Gs = [torch.from_numpy(case[g]).to(dev).permute(0, 2, 3, 4, 1).contiguous() * gscale for g in FR.GRADS]
    Gkeep = [g.clone() for g in Gs]
    sum((s * g).sum() for s, g in zip(maps, Gs)).backward()
    assert all(torch.equal(a, b.detach()) for a, b in zip(keep, lats)), "the ungated laterals were written"
    assert all(torch.equal(a, b) for a, b in zip(Gkeep, Gs)), "an incoming gradient was written"
    grads = {k: p.grad for k, p in zip(FR.SA_PARAMS, sa)}
    grads.update({k: (None if p.grad is None else p.grad.permute(0, 4, 1, 2, 3)) for k, p in zip(FR.LATERALS, lats)})
    return [s.detach().permute(0, 4, 1, 2, 3) for s in maps], grads, bn


def _assert_fusion_grads(got, ref, what, scale=1.0):
    for k in NAMES:
        e = _err(got[k], torch.as_tensor(ref[k]).double() * scale)
        print("%s %s: %.2e of the largest entry" % (what, k, e))
    for k in NAMES:
        assert _err(got[k], torch.as_tensor(ref[k]).double() * scale) <= GRAD_TOL, (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["tiny", "odd", "product"])
def test_hip_fusion_end_to_end(dev, key):
    """ "product": Cm = 512, mid = 32, D = 192 as in the model -- the weight gradient in three input-channel slices -- with half
    of sa_0's units dead, so that the premask and its up-samples hold whole planes of exact zeros (the mask of conv_c1_bwd)."""
    case, saved, grads = _restated(key)
    maps, got, _ = _fusion(case, dev)
    g = _gold()
    for j in range(4):
        ref = torch.from_numpy(g["tiny_s%d" % j]) if key == "tiny" else saved["s%d" % j]
        err = (maps[j].double().cpu() - ref).abs().max().item()
        print("%s: map s%d error %.2e" % (key, j, err))
        assert err < MAP_TOL
    if key == "product":
        assert (saved["m"][0] == 0).double().mean().item() > 0.25
    _assert_fusion_grads(got, {k: g["tiny_d_%s" % k] for k in NAMES} if key == "tiny" else grads, key)


@pytest.mark.gpu
@pytest.mark.parametrize("exp", [-20, 12])
def test_hip_fusion_gradients_at_the_scale_of_a_loss(dev, exp):
    case, saved, grads = _restated("tiny")
    _, got, _ = _fusion(case, dev, gscale=2.0 ** exp)
    _assert_fusion_grads(got, grads, "g * 2^%d" % exp, scale=2.0 ** exp)


@pytest.mark.gpu
def test_hip_fusion_is_repeatable_and_skips_unasked_lateral_gradients(dev):
    case, _, _ = _restated("odd")
    _, a, _ = _fusion(case, dev)
    _, b, _ = _fusion(case, dev)
    _, c, _ = _fusion(case, dev, lat_grad=False)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k
    for k in FR.SA_PARAMS:
        assert torch.equal(a[k], c[k]), k
    assert all(c[k] is None for k in FR.LATERALS)


@pytest.mark.gpu
def test_hip_fusion_running_statistics_after_two_forwards(dev):
    from mspi_amd.autograd import Fusion
    case, saved, _ = _restated("odd")
    mods = FR.upstream_modules(case)
    masks64 = torch.from_numpy(case["masks"]).double()
    with torch.no_grad():
        for seq in mods:
            seq(masks64), seq(masks64)
    lats, masks, sa, bn = _fusion_args(case, dev)
    with torch.no_grad():
        Fusion.apply(*lats, masks, *sa, *bn)
        first = Fusion.apply(*lats, masks, *sa, *bn)
    for k, (rm, rv, nbt) in enumerate(bn):
        ref = mods[k][0].bn
        e_m = (rm.double().cpu() - ref.running_mean).abs().max().item()
        print("sa_%d: running mean %.2e (absolute), running var %.2e" % (k, e_m, _err(rv, ref.running_var)))
        assert e_m <= GRAD_TOL * max(1.0, ref.running_mean.abs().max().item()) and _err(rv, ref.running_var) <= GRAD_TOL
        assert int(nbt) == int(ref.num_batches_tracked) == 2
    without = Fusion.apply(*[t.detach() for t in lats], masks, *[p.detach() for p in sa], None, None, None)
    assert all(torch.equal(a, b) for a, b in zip(first, without)) and int(bn[0][2]) == 2


# ---- autograd.ReadoutHead: the maps' gradients
@pytest.mark.gpu
def test_hip_readout_head_map_gradients(dev):
    """The four maps' gradients against torch autograd in float64 through upstream's layers on the readout fixture's inputs;
    asking for them leaves the ten parameter gradients bit for bit as they are without."""
    from mspi_amd.autograd import ReadoutHead, ReadoutTail
    import readout_tail_restate as RT
    import test_readout_train as TR
    case = TR._restated("tiny")[0]

    def run(map_grad):
        maps, head, bn = TR._head_args(case, dev)
        maps = [m.requires_grad_(map_grad) for m in maps]
        tail = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in RT.PARAMS]
        out = ReadoutTail.apply(ReadoutHead.apply(*maps, *head, bn[0], bn[1]), *tail)
        (out * torch.from_numpy(case["g"]).to(dev)).sum().backward()
        return [m.grad for m in maps], [p.grad for p in head]
    dmaps, with_maps = run(True)
    none, without = run(False)
    assert all(g is None for g in none)
    for name, a, b in zip(R.HEAD, with_maps, without):
        assert torch.equal(a, b), name
    r = R.upstream_readout(case)
    s = [torch.from_numpy(case[k]).double().requires_grad_(True) for k in R.MAPS]
    ups = [torch.nn.Upsample(scale_factor=(1, k, k), mode="trilinear", align_corners=False)(t) for k, t in ((2, s[1]), (4, s[2]), (8, s[3]))]
    z = r(torch.cat([s[0] + ups[0] + ups[1] + ups[2]] + ups, 1))[:, 0, 0]
    out = z - torch.logsumexp(z.flatten(1), 1).view(-1, 1, 1)
    ref = torch.autograd.grad((out * torch.from_numpy(case["g"]).double()).sum(), s)
    for j in range(4):
        e = _err(dmaps[j].permute(0, 4, 1, 2, 3), ref[j])
        print("d s%d: %.2e of the largest entry" % (j, e))
    for j in range(4):
        assert _err(dmaps[j].permute(0, 4, 1, 2, 3), ref[j]) <= GRAD_TOL, j


# ---- the whole model
@pytest.mark.gpu
def test_hip_whole_model_trains_its_fusion(dev, golden_dir):
    from mspi_amd import engine as E
    from mspi_amd import metrics as M
    from mspi_amd._lib import MspiError
    from test_readout_tail import _batches, _build
    E.autotune(False)          # an earlier test (inference.build_model) may have left tuning on: a forward that tunes a shape on
    #                            first sight keeps the last candidate's result, not the chosen tile's, and bits are compared here
    g, cfg, make, clips, audio = _build(golden_dir, "av_x3dl_64", "x3dl", "AudioVisualSaliencyModel", dev)
    m = make().to(dev)
    off, _ = m(clips, audio)
    m.trainable("fusion")
    with pytest.raises(MspiError, match="frozen_encoder"):      # eval() BatchNorm and a graph: batch statistics would be a surprise
        m(clips, audio)
    m.train()
    m.frozen_encoder()
    with torch.no_grad():
        quiet, _ = m(clips, audio)
    assert torch.equal(quiet, off) and not quiet.requires_grad  # the switch-on map under no_grad is the switch-off map
    lat, sa_cat, sa_own = m.pk["lat"], m.pk["sa_cat"], m.sa_0.pk
    start = {k: v.clone() for k, v in m.state_dict().items()}
    params = [p for p in m.parameters() if p.requires_grad]
    assert len(params) == 31
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0)
    label = _batches(clips, audio, 1, True)[0][2].to(dev)
    out, aux = m(clips, audio)
    assert out.requires_grad and not aux.requires_grad
    opt.zero_grad()
    M.SalLoss()(out, label).backward()
    trained_names = set(R.STATE_KEYS.values()) | set(FR.STATE_KEYS.values())
    for name, p in m.named_parameters():                        # exactly the SA and readout parameters are filled
        assert (p.grad is not None) == (name in trained_names), name
        assert p.grad is None or torch.isfinite(p.grad).all(), name
    opt.step()
    moved = trained_names | {"%s.%s" % (mod, n) for mod in BATCH_STAT for n in ("running_mean", "running_var", "num_batches_tracked")}
    for k, v in m.state_dict().items():
        assert torch.equal(v, start[k]) == (k not in moved), k
    with torch.no_grad():
        trained, _ = m(clips, audio)
    pk = m.pk
    assert pk["lat"] is lat and all(a is b for a, b in zip(pk["lat"], lat))      # the step did not rebuild the laterals' packs
    assert pk["sa_cat"] is not sa_cat and m.sa_0.pk is not sa_own               # ... and did replace the SA fold and sa_0's plan
    assert not torch.equal(trained, off) and torch.isfinite(trained).all()
    fresh = make()
    fresh.load_state_dict(m.state_dict())
    again, _ = fresh.to(dev)(clips, audio)
    assert torch.equal(again, trained)
    m.trainable(None)
    m.eval()
    plain, _ = m(clips, audio)
    assert torch.equal(plain, trained) and not plain.requires_grad


# ---- the ledger of the two entry points
def _poisoned(t, idx, value):
    t = t.clone()
    t[idx] = value
    return t


def _judge(what, got, ref):
    """Non-finite contract PROPAGATE: where the float64 reference computed from the poisoned operand is non-finite the output
    is, and everywhere else it is within the bar."""
    got, ref = got.detach().double().cpu(), ref.double()
    bad = ~torch.isfinite(ref)
    assert bad.any(), "%s: the poison reaches nothing" % what
    assert (~torch.isfinite(got[bad])).all(), "%s: %d dependent outputs came out finite" % (what, int(torch.isfinite(got[bad]).sum()))
    e = ((got[~bad] - ref[~bad]).abs().max() / ref[~bad].abs().max()).item() if (~bad).any() else 0.0
    print("%s: %d non-finite outputs, the others within %.2e" % (what, int(bad.sum()), e))
    assert e <= GRAD_TOL, what


def _up_t_sparse(dy, k):
    """The up-sample's adjoint in float64 as torch autograd scatters it, tap by tap: unlike the dense matrices of
    readout_restate.up_t, a NaN in dy reaches only the cells it is a tap of (the reference tests/test_nonfinite_ledger.py uses)."""
    N, Cc, T, Ho, Wo = dy.shape
    x = torch.zeros(N, Cc, T, Ho // k, Wo // k, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.interpolate(x, scale_factor=(1, k, k), mode="trilinear", align_corners=False)
    return torch.autograd.grad(y, x, dy.double())[0]


@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_hip_ledger_nonfinite_operands_propagate(dev, value):
    from mspi_amd import engine as E
    M, C = 70, 36
    dy, x, gate, _ = _rgb_case(M, C, 11)
    for name, idx in (("dy", (5, 9)), ("x", (66, 35)), ("gate", (37,))):
        ops = {"dy": dy, "x": x, "gate": gate}
        ops[name] = _poisoned(ops[name], idx, value)
        rdx, rdz = _rgb_ref(ops["dy"], ops["x"], ops["gate"])
        d, v, g = (E.CL(ops[k].to(dev).reshape(-1), 0, M, 1, 1, 1, c, c) for k, c in (("dy", C), ("x", C), ("gate", 1)))
        dx, dz = E.rowgate_bwd(d, v, g)
        _judge("rowgate_bwd %s -> dz" % name, dz, rdz)
        if name == "x":                                        # dx does not read x
            assert _err(dx.as_rows(), rdx) <= GRAD_TOL
        else:
            _judge("rowgate_bwd %s -> dx" % name, dx.as_rows(), rdx)
    factors, H, W, Cc = (2, 4, 8), 3, 5, 8
    dys, prev, _ = _usb_case(factors, H, W, Cc, 12)
    for j, k in enumerate(factors):                            # interior cells: both of their taps per axis carry weight
        ops = list(dys)
        ops[j] = _poisoned(ops[j], (1, 3, 0, k + 1, 2 * k), value)
        ref = prev.double() + sum(_up_t_sparse(d, kk) for d, kk in zip(ops, factors))
        acc = _cl(prev, dev)
        E.upsample_sum_bwd(acc, [(_cl(d, dev), kk) for d, kk in zip(ops, factors)], accumulate=True)
        _judge("upsample_sum_bwd dy_%d (k = %d)" % (j, k), _ncdhw(acc), ref)
    bad_prev = _poisoned(prev, (0, 2, 0, 1, 1), value)
    acc = _cl(bad_prev, dev)
    E.upsample_sum_bwd(acc, [(_cl(d, dev), kk) for d, kk in zip(dys, factors)], accumulate=True)
    _judge("upsample_sum_bwd dx (accumulate)", _ncdhw(acc), bad_prev.double() + sum(R.up_t(d.double(), kk) for d, kk in zip(dys, factors)))


def _replayed(dev, sets, launch):
    """The capture rules, as tests/test_launch_ledger.py holds them: eager on operand set A; capture on a side stream with set
    B in the static operands; then A copied in, the host arrays the launch handed over overwritten and the outputs filled with a
    sentinel; one replay must give the eager bits."""
    import test_launch_ledger as LL
    static = {k: v.to(dev).clone() for k, v in sets["A"].items()}
    want = {k: v.clone() for k, v in launch(static, []).items()}
    torch.cuda.synchronize()
    for k, v in sets["B"].items():
        static[k].copy_(v)
    host = []
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = launch(static, host)
    for k, v in sets["A"].items():
        static[k].copy_(v)
    LL._scribble(host)
    for v in outs.values():
        LL._fill(v)
    graph.replay()
    torch.cuda.synchronize()
    for k in want:
        assert LL._bits_equal(outs[k], want[k]), "output %s of the replay differs from the eager launch" % k


@pytest.mark.gpu
def test_hip_ledger_capture_and_replay(dev):
    from mspi_amd import _lib
    lib = _lib.load()
    M, C = 300, 36
    sets = {w: dict(zip(("dy", "x", "gate"), _rgb_case(M, C, s)[:3])) for w, s in (("A", 21), ("B", 22))}

    def rowgate(t, host):
        dx, dz = torch.empty(M, C, device=dev), torch.empty(M, device=dev)
        _lib.check(lib.mspi_rowgate_bwd(t["dy"].data_ptr(), C, t["x"].data_ptr(), C, t["gate"].data_ptr(), dx.data_ptr(), C,
                                        dz.data_ptr(), M, C, _stream()), "mspi_rowgate_bwd")
        return {"dx": dx, "dz": dz}
    _replayed(dev, sets, rowgate)

    factors, NT, H, W, Cc = (2, 4, 8), 2, 3, 5, 8

    def operands(seed):
        dys, prev, _ = _usb_case(factors, H, W, Cc, seed, NT)
        t = {"dy%d" % j: d.permute(0, 2, 3, 4, 1).contiguous() for j, d in enumerate(dys)}
        t["prev"] = prev.permute(0, 2, 3, 4, 1).contiguous()
        return t

    def upsum(t, host):
        ptrs = (ctypes.c_void_p * 3)(*[t["dy%d" % j].data_ptr() for j in range(3)])
        lds = (ctypes.c_int64 * 3)(Cc, Cc, Cc)
        ks = (ctypes.c_int32 * 3)(*factors)
        host.extend([ptrs, lds, ks])                          # host arrays: read during the call, overwritten before the replay
        dx = t["prev"].clone()
        _lib.check(lib.mspi_upsample_sum_bwd(ptrs, lds, ks, 3, dx.data_ptr(), Cc, NT, H, W, Cc, 1, _stream()), "mspi_upsample_sum_bwd")
        return {"dx": dx}
    _replayed(dev, {"A": operands(31), "B": operands(32)}, upsum)
