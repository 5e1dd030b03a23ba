"""The trainable ConvNextBlock at the end of each lateral: csrc/block_bwd.hip (mspi_gelu_bwd, mspi_layernorm_bwd,
mspi_dwconv_wgrad, declared in include/mspi_block_train_hip.h), engine.gelu_bwd / layernorm_bwd / dwconv_wgrad,
autograd.LateralBlock, _SaliencyBase.trainable("lateral_blocks"), mspi_amd.train --trainable lateral_blocks.

Yardsticks: tests/golden/lateral_block.npz holds "tiny" ((B, T, h, w) = (1, 1, 1, 2), D = 32) as its seed and, in float64, the
output and the 11 gradients of <y, G> that torch autograd gives through torch.nn layers with upstream's arguments
(tools/gen_lateral_golden.py), and the seed of "odd" ((2, 3, 5, 3)); tests/lateral_restate.py is the float64 restatement in
this project's order with its analytic backward, pinned to that fixture and, here, to torch autograd on "odd".

Bounds.  Every gradient tensor: max |got - ref| / max |ref| <= GRAD_TOL = 2e-5, the project's bar for gradients
(tests/test_readout_train.py); every test prints its figure before it asserts.  Torch FLOAT32 on the CPU agrees with float64
on all 12 tensors to 4.2e-7 on the fixture's "tiny" seed and to 4.3e-7 on its "odd" seed (tools/gen_lateral_golden.py prints
both), so the bar leaves a factor of ten.  The block has no ReLU: no kink caveats.  Adjoint identity: 1e-5 of the sum of the
absolute terms, accumulated in float64 on the host.  The ledger part holds the three entry points to what
tests/test_fusion_train.py holds its two: declared = exported = bound, capture + replay with the operands and the host
descriptor overwritten in between, and a NaN / +Inf in each floating operand reaching every output that depends on it and no
other.

Cases: "tiny" (every 7x7 and 7-tap window clipped on all sides), "odd" (odd extents, T < 7, rows no multiple of any workgroup
size), "s3" ((1, 4, 7, 12) at D = 192: the product's channels and s3's extent) and "switch" ((1, 4, 32, 32) at D = 192: 4096
rows, the fused-mlp side of ConvNextBlock's switch)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import fusion_restate as FR
import lateral_restate as LR
import readout_restate as R
from test_fusion_train import BATCH_STAT, _declared, _judge, _poisoned, _replayed, _stream
from test_readout_train import GRAD_TOL, _cl, _dot, _err, _ncdhw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_gelu_bwd", "mspi_layernorm_bwd_ws_bytes", "mspi_layernorm_bwd", "mspi_dwconv_wgrad_supported",
               "mspi_dwconv_wgrad_ws_bytes", "mspi_dwconv_wgrad")
CASES = ("tiny", "odd")
SHAPES = {"tiny": (1, 1, 1, 2), "odd": (2, 3, 5, 3), "s3": (1, 4, 7, 12), "switch": (1, 4, 32, 32)}
DIMS = {"tiny": 32, "odd": 32, "s3": 192, "switch": 192}
SEEDS = {"s3": 9501, "switch": 9502}
ALL = ("tiny", "odd", "s3", "switch")


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "lateral_block.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _restated(key):
    """(case, saved, grads) in float64, computed once and left unchanged."""
    seed = int(_gold()["%s_seed" % key]) if key in CASES else SEEDS[key]
    case = LR.make_case(*SHAPES[key], seed=seed, D=DIMS[key])
    saved = LR.forward(case)
    return case, saved, LR.backward(case, saved, case["G"])


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["cases"]) == CASES
    for c in CASES:
        assert tuple(g["%s_shape" % c]) == SHAPES[c]
    shapes = dict(LR.param_shapes(32), x=(1, 32, 1, 1, 2))
    assert len(LR.NAMES) == 11 and len(LR.PARAMS) == 10
    for k in LR.NAMES:
        assert g["tiny_d_%s" % k].shape == shapes[k] and g["tiny_d_%s" % k].dtype == np.float64
    assert g["tiny_y"].shape == shapes["x"] and g["tiny_y"].dtype == np.float64
    golden = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(golden, "lateral_block.npz")) <= os.path.getsize(os.path.join(golden, "fusion.npz"))


def test_restatement_matches_the_fixture():
    g = _gold()
    case, saved, grads = _restated("tiny")
    assert (saved["y"] - torch.from_numpy(g["tiny_y"])).abs().max().item() <= 1e-12
    for k in LR.NAMES:
        assert _err(grads[k], g["tiny_d_%s" % k]) <= 1e-12, k


def test_restatement_matches_torch_autograd_on_odd():
    """ "odd" is stored as its seed: torch.nn layers with upstream's arguments, float64, built here."""
    case, saved, grads = _restated("odd")
    y, ref = LR.upstream_grads(case)
    assert (saved["y"] - y).abs().max().item() <= 1e-12
    for k in LR.NAMES:
        assert _err(grads[k], ref[k]) <= 1e-12, k


def test_block_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    from mspi_amd import engine as E
    block, _ = _declared("mspi_block_train_hip.h")
    train, _ = _declared("mspi_train_hip.h")
    base, base_text = _declared("mspi_hip.h")
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert block == set(NEW_SYMBOLS) == set(_lib.BLOCK_EXPORTS) == set(_lib._BLOCK_SIGNATURES)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _lib._BLOCK_SIGNATURES[name][1], name
    # the pinned symbol sets are as they were, the ABI version unchanged
    assert train == set(_lib.TRAIN_EXPORTS) == {"mspi_rowgate_bwd", "mspi_upsample_sum_bwd"}
    assert base == set(_lib.EXPORTS) and not (base | train) & set(NEW_SYMBOLS)
    assert re.search(r"#define MSPI_ABI_VERSION 2\b", base_text) and lib.mspi_version() == 2
    for name in ("gelu_bwd", "layernorm_bwd", "dwconv_wgrad"):
        assert callable(getattr(E, name)) and name in E.__all__
    src = open(os.path.join(ROOT, "mspi_amd", "csrc", "block_bwd.hip")).read()
    assert "atomic" not in src.lower()
    mk = open(os.path.join(ROOT, "mspi_amd", "csrc", "Makefile")).read()
    assert "block_bwd.hip" in mk and mk.count("mspi_block_train_hip.h") == 2 and "-fno-slp-vectorize" in mk


def _dw_desc(N=1, T=2, H=3, W=4, C=8, k=(1, 7, 7), stride=(1, 1, 1), pad=(0, 3, 3), ldx=None, ldy=None):
    from mspi_amd import _lib
    d = _lib.DwConvDesc()
    d.N, d.T, d.H, d.W, d.C = N, T, H, W, C
    d.ldx, d.ldy = (C if ldx is None else ldx), (C if ldy is None else ldy)
    d.kT, d.kH, d.kW = k
    d.strT, d.strH, d.strW = stride
    d.padT, d.padH, d.padW = pad
    d.To, d.Ho, d.Wo = [(n + 2 * p - kk) // s + 1 for n, p, kk, s in zip((T, H, W), pad, k, stride)]
    return d


def test_host_refusals():
    from mspi_amd import _lib
    lib = _lib.load()

    def err():
        return lib.mspi_last_error().decode()

    def gelu(z=4096, ldz=8, dg=8192, lddg=8, g=12288, ldg=8, dz=16384, lddz=8, M=3, C=8):
        return lib.mspi_gelu_bwd(z, ldz, dg, lddg, g, ldg, dz, lddz, M, C, None), err()

    def lnb(x=4096, ldx=8, dy=8192, lddy=8, gamma=12288, eps=1e-5, dx=16384, lddx=8, dgam=20480, dbet=24576, ws=28672, M=3, C=8):
        return lib.mspi_layernorm_bwd(x, ldx, dy, lddy, gamma, eps, dx, lddx, dgam, dbet, ws, M, C, None), err()

    def dwg(d=None, x=4096, dy=8192, dW=12288, db=16384, ws=20480, **kw):
        d = _dw_desc(**kw) if d is None else d
        return lib.mspi_dwconv_wgrad(ctypes.byref(d), x, dy, dW, db, ws, None), err()

    for rc, why in (gelu(C=6), gelu(ldz=6), gelu(lddg=4), gelu(ldg=10), gelu(lddz=6), gelu(z=4100), gelu(dg=8200), gelu(g=12292),
                    gelu(dz=16388)):
        assert rc == -1 and "mspi_gelu_bwd" in why and "multiples of 4" in why, (rc, why)
    for rc, why in (gelu(z=None), gelu(dg=None), gelu(dz=None)):
        assert rc == -1 and "null argument" in why, (rc, why)
    assert gelu(M=0)[0] == -1 and "bad extent" in gelu(M=0)[1] and gelu(C=0)[0] == -1
    assert gelu(M=1 << 31)[0] == -1 and "2^31" in gelu(M=1 << 31)[1]

    for rc, why in (lnb(ldx=6), lnb(lddy=4), lnb(lddx=10), lnb(x=4100), lnb(dy=8200), lnb(dx=16388)):
        assert rc == -1 and "mspi_layernorm_bwd" in why and "multiples of 4" in why, (rc, why)
    for rc, why in (lnb(C=6), lnb(C=260), lnb(C=0)):
        assert rc == -1 and "multiple of 4, at most 256" in why, (rc, why)
    for rc, why in (lnb(x=None), lnb(dy=None), lnb(gamma=None), lnb(dx=None), lnb(dgam=None), lnb(dbet=None), lnb(ws=None)):
        assert rc == -1 and "null argument" in why, (rc, why)
    assert lnb(gamma=12292)[0] == -1 and lnb(ws=28676)[0] == -1 and lnb(eps=-1.0)[0] == -1
    assert lnb(M=0)[0] == -1 and "no rows" in lnb(M=0)[1]
    assert lnb(M=1 << 31)[0] == -1 and "2^31" in lnb(M=1 << 31)[1]
    assert lib.mspi_layernorm_bwd_ws_bytes(0, 8) == 0 and lib.mspi_layernorm_bwd_ws_bytes(3, 6) == 0
    assert lib.mspi_layernorm_bwd_ws_bytes(257, 192) == 2 * 2 * 192 * 4          # one record [dbeta | dgamma] per 256 rows

    good = _dw_desc()
    assert lib.mspi_dwconv_wgrad_supported(ctypes.byref(good)) == 1
    assert lib.mspi_dwconv_wgrad_supported(ctypes.byref(_dw_desc(k=(7, 1, 1), pad=(3, 0, 0)))) == 1
    assert lib.mspi_dwconv_wgrad_ws_bytes(ctypes.byref(good)) == 2 * 1 * 50 * 8 * 4   # 2 frames x 1 band of 4 rows, [49 + 1][C]
    refused = {"stride must be 1": _dw_desc(stride=(1, 2, 2)), "kernel must be": _dw_desc(k=(3, 3, 3), pad=(1, 1, 1)),
               "multiples of 4": _dw_desc(C=6), "bad extent": _dw_desc(W=0), "2^31": _dw_desc(N=1 << 11, T=1 << 10, H=32, W=32)}
    refused["multiples of 4 "] = _dw_desc(ldx=10)
    refused["multiples of 4  "] = _dw_desc(ldy=4)
    refused["kernel must be "] = _dw_desc(pad=(0, 2, 2))
    for text, d in refused.items():
        assert lib.mspi_dwconv_wgrad_supported(ctypes.byref(d)) == 0 and text.strip() in err(), (text, err())
        assert lib.mspi_dwconv_wgrad_ws_bytes(ctypes.byref(d)) == 0
        rc, why = dwg(d=d)
        assert rc == -1 and "mspi_dwconv_wgrad" in why and text.strip() in why, (text, rc, why)
    assert lib.mspi_dwconv_wgrad_supported(None) == 0
    for rc, why in (dwg(x=None), dwg(dy=None), dwg(dW=None), dwg(db=None), dwg(ws=None)):
        assert rc == -1 and "null argument" in why, (rc, why)
    for rc, why in (dwg(x=4100), dwg(dy=8200), dwg(ws=20484)):
        assert rc == -1 and "16-byte aligned" in why, (rc, why)


def _model():
    from mspi_amd import testing as T
    from mspi_amd.model.model_utils import AudioVisualSaliencyModel
    return T.seeded(lambda: AudioVisualSaliencyModel(T.make_cfg("x3dl")), 0)


def _block_names(m):
    return ["latlayer_%d.%d.%s" % (k, len(getattr(m, "latlayer_%d" % k)) - 1, n) for k in range(4) for n in LR.STATE_KEYS.values()]


def _trained_names(m):
    return sorted(list(R.STATE_KEYS.values()) + list(FR.STATE_KEYS.values()) + _block_names(m))


def test_trainable_lateral_blocks_flags_modes_and_restore(monkeypatch):
    from mspi_amd._lib import MspiError
    from mspi_amd.model import model_utils as pm
    m = _model()
    first = next(m.visnet.parameters())
    first.requires_grad_(False)
    before = {n: p.requires_grad for n, p in m.named_parameters()}
    assert m.trainable("lateral_blocks") is m
    on = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert on == _trained_names(m) and len(on) == 71 and len(_block_names(m)) == 40
    assert not any(p.requires_grad for k in range(4) for p in getattr(m, "latlayer_%d" % k)[0].parameters())
    m.train()
    m.frozen_encoder()
    assert sorted(n for n, s in m.named_modules() if s.training) == BATCH_STAT and not m.training
    m._check_eval()
    for other in (m.latlayer_0[0], m.adapter, m.latlayer_3[-1]):
        other.train()
        with pytest.raises(MspiError, match="under trainable\\('lateral_blocks'\\) only readout.2, readout.5 and the three"):
            m._check_eval()
        m.frozen_encoder()
    m._check_eval()
    m.trainable("fusion")                                       # switching over and back
    assert len([n for n, p in m.named_parameters() if p.requires_grad]) == 31
    m.adapter.train()
    with pytest.raises(MspiError, match="under trainable\\('fusion'\\) only readout.2, readout.5 and the three"):
        m._check_eval()
    m.frozen_encoder()
    m.trainable("lateral_blocks")
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == on
    for bad in ("laterals", "decoder", ""):
        with pytest.raises(MspiError, match="readout_tail"):
            m.trainable(bad)
    m.trainable(None)
    assert {n: p.requires_grad for n, p in m.named_parameters()} == before and not first.requires_grad
    monkeypatch.setattr(pm, "DECODER_FUSED", False)
    with pytest.raises(MspiError, match="MSPI_DECODER_FUSED"):
        m.trainable("lateral_blocks")


def test_train_accepts_lateral_blocks_up_to_the_gpu_check(monkeypatch):
    from mspi_amd import train
    from mspi_amd._lib import MspiError
    assert train.TRAINABLE_BLOCKS == ("lateral_blocks",)
    assert train.TRAINABLE == ("readout_tail", "readout") and train.TRAINABLE_STAGES == train.TRAINABLE + ("fusion",)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="MI355X"):
        train.main(["--trainable", "lateral_blocks"])
    with pytest.raises(MspiError, match="--trainable laterals: only readout_tail, readout can be trained on a frozen pyramid, and "
                                        "fusion.*lateral_blocks"):
        train.main(["--trainable", "laterals"])
    assert "--trainable lateral_blocks" in train.__doc__ and "Still frozen" in train.__doc__


# ------------------------------------------------------------------------------------------------------------- GPU
def _rows_cl(t, dev, ld=None):
    """[M, C] -> CL of M rows (ld > C: inside a wider buffer that holds NaN elsewhere)."""
    return _cl(t[:, :, None, None, None], dev, ld)


def _gelu_case(M, C, seed):
    gen = torch.Generator().manual_seed(seed)
    z, dg = 2.0 * torch.randn(M, C, generator=gen), torch.randn(M, C, generator=gen)
    z.view(-1)[:6] = torch.tensor([0.0, -0.0, 6.0, -6.0, 1e-3, -12.0])
    return z, dg


@pytest.mark.gpu
@pytest.mark.parametrize("M,C", [(2, 128), (90, 128), (336, 768), (4096, 768), (257, 4)])
def test_hip_gelu_bwd_vs_fp64(dev, M, C):
    from mspi_amd import engine as E
    z, dg = _gelu_case(M, C, 40 + M)
    rg, rdz = LR.gelu_bwd(z.double(), dg.double())
    g, dz = E.gelu_bwd(_rows_cl(z, dev), _rows_cl(dg, dev))
    eg, ed = _err(g.as_rows(), rg), _err(dz.as_rows(), rdz)
    print("gelu_bwd M=%d C=%d: g %.2e dz %.2e" % (M, C, eg, ed))
    assert eg <= GRAD_TOL and ed <= GRAD_TOL
    g2, dz2 = E.gelu_bwd(_rows_cl(z, dev), _rows_cl(dg, dev))
    assert torch.equal(g2.buf, g.buf) and torch.equal(dz2.buf, dz.buf)
    none, dz3 = E.gelu_bwd(_rows_cl(z, dev), _rows_cl(dg, dev), need_g=False)
    assert none is None and torch.equal(dz3.buf, dz.buf)
    # in place, inside buffers wider than C whose other columns hold NaN: g over z, dz over dg, the same bits
    zc, dc = _rows_cl(z, dev, ld=C + 8), _rows_cl(dg, dev, ld=C + 4)
    gi, dzi = E.gelu_bwd(zc, dc, inplace=True)
    assert gi is zc and dzi is dc
    assert torch.equal(zc.as_rows(), g.as_rows()) and torch.equal(dc.as_rows(), dz.as_rows())
    assert torch.isnan(zc.buf.view(M, C + 8)[:, :8]).all() and torch.isnan(dc.buf.view(M, C + 4)[:, :4]).all()


def _ln_case(M, C, seed):
    gen = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(M, C, generator=gen) + torch.randn(M, 1, generator=gen)
    return x, torch.randn(M, C, generator=gen), 1.0 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)


def _ln_judge(what, got, ref):
    for name, a, b in zip(("dx", "dgamma", "dbeta"), got, ref):
        e = _err(a.as_rows() if hasattr(a, "as_rows") else a, b)
        print("%s %s: %.2e" % (what, name, e))
        assert e <= GRAD_TOL, (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("M,C", [(2, 32), (90, 32), (336, 192), (4096, 192), (257, 64), (513, 132), (255, 256), (17, 4)])
def test_hip_layernorm_bwd_vs_fp64(dev, M, C):
    from mspi_amd import engine as E
    x, dy, gam, bet = _ln_case(M, C, 50 + M)
    ref = LR.layernorm_bwd(dy.double(), x.double(), gam.double())
    got = E.layernorm_bwd(_rows_cl(dy, dev), _rows_cl(x, dev), gam.to(dev))
    _ln_judge("layernorm_bwd M=%d C=%d" % (M, C), got, ref)
    again = E.layernorm_bwd(_rows_cl(dy, dev), _rows_cl(x, dev), gam.to(dev))
    assert all(torch.equal(a.buf if hasattr(a, "buf") else a, b.buf if hasattr(b, "buf") else b) for a, b in zip(got, again))
    wide = E.layernorm_bwd(_rows_cl(dy, dev, ld=C + 4), _rows_cl(x, dev, ld=C + 12), gam.to(dev))      # NaN in the pad columns
    assert all(torch.equal(a.buf if hasattr(a, "buf") else a, b.buf if hasattr(b, "buf") else b) for a, b in zip(got, wide))
    # the recomputed x^ is the forward's: gamma x^ + beta from this kernel's mean / rstd order equals layernorm's output bits
    # (checked through dgamma with dy = 1 on one row: dgamma = x^ of that row)
    if M >= 2:
        one = torch.zeros(M, C)
        one[1] = 1.0
        xh = E.layernorm_bwd(_rows_cl(one, dev), _rows_cl(x, dev), gam.to(dev))[1]
        y = E.layernorm(_rows_cl(x, dev), torch.ones(C, device=dev), torch.zeros(C, device=dev), 1e-5)
        assert torch.equal(xh, y.as_rows()[1])


def _dw_case(shape, C, k, seed):
    gen = torch.Generator().manual_seed(seed)
    N, T, H, W = shape
    return torch.randn(N, C, T, H, W, generator=gen), torch.randn(N, C, T, H, W, generator=gen), torch.randn(C, 1, *k, generator=gen)


KERNELS = {"t": ((7, 1, 1), (3, 0, 0)), "s": ((1, 7, 7), (0, 3, 3))}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["t", "s"])
@pytest.mark.parametrize("key,C", [("tiny", 32), ("odd", 32), ("s3", 192), ("switch", 192), ("odd", 4), ("odd", 148), ("long", 8)])
def test_hip_dwconv_wgrad_vs_fp64(dev, key, C, which):
    from mspi_amd import engine as E
    shape = SHAPES.get(key, (2, 9, 10, 17))            # "long": lines longer than the 7-step unroll along both axes
    k, pad = KERNELS[which]
    x, dy, w = _dw_case(shape, C, k, 60 + C)
    rW, rb = LR.dwconv_wgrad(x.double(), dy.double(), k, pad)
    pk = E.pack_dwconv(w, None, None, (1, 1, 1), pad)
    dW, db = E.dwconv_wgrad(_cl(x, dev), _cl(dy, dev), pk)
    eW, eb = _err(dW, rW), _err(db, rb)
    print("dwconv_wgrad %s %s C=%d: dW %.2e db %.2e" % (k, shape, C, eW, eb))
    assert eW <= GRAD_TOL and eb <= GRAD_TOL and dW.shape == w.shape
    dW2, db2 = E.dwconv_wgrad(_cl(x, dev), _cl(dy, dev), pk)
    assert torch.equal(dW2, dW) and torch.equal(db2, db)
    dW3, db3 = E.dwconv_wgrad(_cl(x, dev, ld=C + 4), _cl(dy, dev, ld=C + 8), pk)                     # NaN in the pad columns
    assert torch.equal(dW3, dW) and torch.equal(db3, db)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["t", "s"])
@pytest.mark.parametrize("key", ["tiny", "odd", "s3"])
def test_hip_flipped_dwconv_is_the_adjoint(dev, key, which):
    """<dw(x), y> = <x, dw^T(y)> with dw^T the same conv on the flipped taps without bias, as LateralBlock.backward packs it."""
    from mspi_amd import engine as E
    k, pad = KERNELS[which]
    x, y, w = _dw_case(SHAPES[key], DIMS[key], k, 70)
    fwd = _ncdhw(E.dwconv(_cl(x, dev), E.pack_dwconv(w, None, None, (1, 1, 1), pad, device=dev)))
    adj = _ncdhw(E.dwconv(_cl(y, dev), E.pack_dwconv(w.flip(2, 3, 4), None, None, (1, 1, 1), pad, device=dev)))
    lhs, rhs = _dot(fwd, y), _dot(x, adj)
    scale = (fwd.double().cpu() * y.double()).abs().sum().item() + (x.double() * adj.double().cpu()).abs().sum().item()
    print("dwconv adjoint %s %s: |lhs - rhs| / sum|terms| = %.2e" % (k, key, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-5 * scale


@pytest.mark.gpu
def test_hip_engine_wrappers_refuse_by_name(dev):
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    z, dg = _gelu_case(6, 8, 1)
    with pytest.raises(MspiError, match="gelu_bwd: dg must match"):
        E.gelu_bwd(_rows_cl(z, dev), _rows_cl(dg[:5], dev))
    with pytest.raises(MspiError, match="GPU only"):
        E.gelu_bwd(_rows_cl(z, "cpu"), _rows_cl(dg, "cpu"))
    x, dy, gam, _ = _ln_case(6, 8, 2)
    with pytest.raises(MspiError, match="layernorm_bwd: dy must match"):
        E.layernorm_bwd(_rows_cl(dy[:, :4], dev), _rows_cl(x, dev), gam.to(dev))
    with pytest.raises(MspiError, match="layernorm_bwd: gamma must be a contiguous fp32"):
        E.layernorm_bwd(_rows_cl(dy, dev), _rows_cl(x, dev), gam[:4].to(dev))
    big = torch.zeros(2, 260)
    with pytest.raises(MspiError, match="at most 256"):
        E.layernorm_bwd(_rows_cl(big, dev), _rows_cl(big, dev), torch.ones(260, device=dev))
    xs, ds, w = _dw_case((1, 2, 3, 4), 8, (3, 3, 3), 3)
    with pytest.raises(MspiError, match="dwconv_wgrad: .*kernel must be"):
        E.dwconv_wgrad(_cl(xs, dev), _cl(ds, dev), E.pack_dwconv(w, None, None, (1, 1, 1), (1, 1, 1)))
    w7 = torch.randn(8, 1, 1, 7, 7)
    with pytest.raises(MspiError, match="dwconv_wgrad: .*stride must be 1"):
        E.dwconv_wgrad(_cl(xs, dev), _cl(ds, dev), E.pack_dwconv(w7, None, None, (1, 2, 2), (0, 3, 3)))
    with pytest.raises(MspiError, match="must be dense and have the extent of x"):
        E.dwconv_wgrad(_cl(xs, dev), _cl(ds[:, :, :1], dev), E.pack_dwconv(w7, None, None, (1, 1, 1), (0, 3, 3)))


# ---- autograd.LateralBlock
def _rows5(t, dev):
    return torch.as_tensor(t).float().permute(0, 2, 3, 4, 1).contiguous().to(dev)


def _block(case, dev, gscale=1.0, x_grad=True):
    """(y, {name: gradient}) of autograd.LateralBlock on the case, gradients of <y, gscale G>; x's in NCDHW."""
    from mspi_amd import autograd as A
    x = _rows5(case["x"], dev).requires_grad_(x_grad)
    ps = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in LR.PARAMS]
    y = A.LateralBlock.apply(x, *ps)
    wrt = ([x] if x_grad else []) + ps
    grads = dict(zip(LR.NAMES if x_grad else LR.PARAMS, torch.autograd.grad(y, wrt, _rows5(case["G"], dev) * gscale)))
    if x_grad:
        grads["x"] = grads["x"].permute(0, 4, 1, 2, 3)
    return y.detach(), grads


def _assert_block_grads(got, ref, what, scale=1.0):
    for k, g in got.items():
        e = _err(g, torch.as_tensor(ref[k]).double() * scale)
        print("%s d %s: %.2e" % (what, k, e))
        assert e <= GRAD_TOL, (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ALL)
def test_hip_lateral_block_end_to_end(dev, key):
    from mspi_amd import engine as E
    from mspi_amd.model import model_utils as pm
    E.autotune(False)
    case, saved, grads = _restated(key)
    D = DIMS[key]
    y, got = _block(case, dev)
    # the forward has the bits of the inference path on the same parameters, on both sides of the 4096-row switch
    blk = pm.ConvNextBlock(dim=D)
    blk.load_state_dict({LR.STATE_KEYS[k]: torch.from_numpy(case[k]) for k in LR.PARAMS})
    blk = blk.to(dev).eval()
    B, T, h, w = SHAPES[key]
    run = blk.run(E.CL(_rows5(case["x"], dev).view(-1), 0, B, T, h, w, D, D))
    assert (blk.pk["fused"] is not None and run.M >= 4096) == (key == "switch")
    assert torch.equal(run.buf.view(B, T, h, w, D), y)
    ref_y = torch.from_numpy(_gold()["tiny_y"]) if key == "tiny" else saved["y"]
    ey = _err(y.permute(0, 4, 1, 2, 3), ref_y)
    print("LateralBlock %s y: %.2e" % (key, ey))
    assert ey <= GRAD_TOL
    ref = {k: _gold()["tiny_d_%s" % k] for k in LR.NAMES} if key == "tiny" else grads
    _assert_block_grads(got, ref, "LateralBlock %s" % key)


@pytest.mark.gpu
@pytest.mark.parametrize("exp", [-20, 12])
@pytest.mark.parametrize("key", ["odd", "s3"])
def test_hip_lateral_block_gradients_at_the_scale_of_a_loss(dev, key, exp):
    from mspi_amd import engine as E
    E.autotune(False)
    case, _, grads = _restated(key)
    _assert_block_grads(_block(case, dev, gscale=2.0 ** exp)[1], grads, "LateralBlock %s, G x 2^%d" % (key, exp), scale=2.0 ** exp)


@pytest.mark.gpu
def test_hip_lateral_block_is_repeatable_and_skips_an_unasked_dx(dev):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    E.autotune(False)
    case = _restated("s3")[0]
    y1, g1 = _block(case, dev)
    y2, g2 = _block(case, dev)
    assert torch.equal(y1, y2) and all(torch.equal(g1[k], g2[k]) for k in LR.NAMES)
    y3, g3 = _block(case, dev, x_grad=False)
    assert "x" not in g3 and torch.equal(y3, y1) and all(torch.equal(g1[k], g3[k]) for k in LR.PARAMS)
    calls = []
    orig = E.dwconv
    try:
        E.dwconv = lambda *a, **k: calls.append(1) or orig(*a, **k)
        _block(case, dev, x_grad=False)
        without = len(calls)
        _block(case, dev)
    finally:
        E.dwconv = orig
    assert (without, len(calls) - without) == (3, 4)             # two forward + one adjoint; dx costs one more launch
    ps = [torch.from_numpy(case[k]).to(dev) for k in LR.PARAMS]
    x = _rows5(case["x"], dev)
    with pytest.raises(MspiError, match="GPU only"):
        A.LateralBlock.apply(x.cpu(), *[p.cpu() for p in ps])
    with pytest.raises(MspiError, match="x must be fp32 \\[B,T,h,w,D\\]"):
        A.LateralBlock.apply(x[0], *ps)
    with pytest.raises(MspiError, match="D % 32 != 0"):
        A.LateralBlock.apply(x[..., :40].contiguous(), *ps)
    with pytest.raises(MspiError, match="pwconv1.weight is"):
        A.LateralBlock.apply(x, *ps[:6], ps[6][:, :96].contiguous(), *ps[7:])


# ---- the ledger of the three entry points
@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_hip_ledger_nonfinite_operands_propagate(dev, value):
    from mspi_amd import engine as E
    M, C = 70, 36
    z, dg = _gelu_case(M, C, 11)
    for name, idx in (("z", (5, 9)), ("dg", (66, 35))):
        ops = {"z": z, "dg": dg}
        ops[name] = _poisoned(ops[name], idx, value)
        rg, rdz = LR.gelu_bwd(ops["z"].double(), ops["dg"].double())
        g, dz = E.gelu_bwd(_rows_cl(ops["z"], dev), _rows_cl(ops["dg"], dev))
        _judge("gelu_bwd %s -> dz" % name, dz.as_rows(), rdz)
        if name == "z":
            _judge("gelu_bwd z -> g", g.as_rows(), rg)
        else:
            assert _err(g.as_rows(), rg) <= GRAD_TOL               # g does not read dg
    x, dy, gam, _ = _ln_case(M, C, 12)
    for name, idx in (("x", (37, 20)), ("dy", (69, 35)), ("gam", (7,))):
        ops = {"x": x, "dy": dy, "gam": gam}
        ops[name] = _poisoned(ops[name], idx, value)
        ref = LR.layernorm_bwd(ops["dy"].double(), ops["x"].double(), ops["gam"].double())
        dx, dgam, dbet = E.layernorm_bwd(_rows_cl(ops["dy"], dev), _rows_cl(ops["x"], dev), ops["gam"].to(dev))
        _judge("layernorm_bwd %s -> dx" % name, dx.as_rows(), ref[0])
        if name == "gam":                                           # neither sum reads gamma
            assert _err(dgam, ref[1]) <= GRAD_TOL and _err(dbet, ref[2]) <= GRAD_TOL
        else:
            _judge("layernorm_bwd %s -> dgamma" % name, dgam, ref[1])
            if name == "dy":
                _judge("layernorm_bwd dy -> dbeta", dbet, ref[2])
            else:
                assert _err(dbet, ref[2]) <= GRAD_TOL               # dbeta does not read x
    for which, shape in (("t", (2, 3, 5, 3)), ("s", (2, 3, 9, 10))):
        k, pad = KERNELS[which]
        xs, ds, w = _dw_case(shape, 8, k, 13)
        pk = E.pack_dwconv(w, None, None, (1, 1, 1), pad)
        for name, idx in (("x", (1, 5, 1, 2, 1)), ("dy", (0, 3, 2, 4, 2))):
            ops = {"x": xs, "dy": ds}
            ops[name] = _poisoned(ops[name], idx, value)
            rW, rb = LR.dwconv_wgrad(ops["x"].double(), ops["dy"].double(), k, pad)
            dW, db = E.dwconv_wgrad(_cl(ops["x"], dev), _cl(ops["dy"], dev), pk)
            _judge("dwconv_wgrad %s %s -> dW" % (k, name), dW, rW)
            if name == "dy":
                _judge("dwconv_wgrad %s dy -> db" % (k,), db, rb)
            else:
                assert _err(db, rb) <= GRAD_TOL                     # db does not read x


@pytest.mark.gpu
def test_hip_ledger_capture_and_replay(dev):
    from mspi_amd import _lib
    lib = _lib.load()
    M, C = 300, 36

    def gelu(t, host):
        g, dz = torch.empty(M, C, device=dev), torch.empty(M, C, device=dev)
        _lib.check(lib.mspi_gelu_bwd(t["z"].data_ptr(), C, t["dg"].data_ptr(), C, g.data_ptr(), C, dz.data_ptr(), C, M, C, _stream()),
                   "mspi_gelu_bwd")
        return {"g": g, "dz": dz}
    _replayed(dev, {w: dict(zip(("z", "dg"), _gelu_case(M, C, s))) for w, s in (("A", 21), ("B", 22))}, gelu)

    def lnb(t, host):
        dx, dgb = torch.empty(M, C, device=dev), torch.empty(2, C, device=dev)
        ws = torch.empty(lib.mspi_layernorm_bwd_ws_bytes(M, C) // 4, device=dev)
        _lib.check(lib.mspi_layernorm_bwd(t["x"].data_ptr(), C, t["dy"].data_ptr(), C, t["gam"].data_ptr(), 1e-5, dx.data_ptr(), C,
                                          dgb[0].data_ptr(), dgb[1].data_ptr(), ws.data_ptr(), M, C, _stream()), "mspi_layernorm_bwd")
        return {"dx": dx, "dgb": dgb}
    _replayed(dev, {w: dict(zip(("x", "dy", "gam"), _ln_case(M, C, s)[:3])) for w, s in (("A", 23), ("B", 24))}, lnb)

    for which, shape in (("t", (2, 3, 5, 3)), ("s", (2, 3, 9, 10))):
        k, pad = KERNELS[which]
        N, T, H, W = shape
        Cc, taps = 8, k[0] * k[1] * k[2]

        def operands(seed):
            x, dy, _ = _dw_case(shape, Cc, k, seed)
            return {"x": x.permute(0, 2, 3, 4, 1).contiguous(), "dy": dy.permute(0, 2, 3, 4, 1).contiguous()}

        def dwg(t, host):
            d = _dw_desc(N=N, T=T, H=H, W=W, C=Cc, k=k, pad=pad)
            host.append(d)                                          # the descriptor: read during the call, overwritten before the replay
            dW, db = torch.empty(taps, Cc, device=dev), torch.empty(Cc, device=dev)
            ws = torch.empty(lib.mspi_dwconv_wgrad_ws_bytes(ctypes.byref(d)) // 4, device=dev)
            _lib.check(lib.mspi_dwconv_wgrad(ctypes.byref(d), t["x"].data_ptr(), t["dy"].data_ptr(), dW.data_ptr(), db.data_ptr(),
                                             ws.data_ptr(), _stream()), "mspi_dwconv_wgrad")
            return {"dW": dW, "db": db}
        _replayed(dev, {"A": operands(25), "B": operands(26)}, dwg)


# ---- the whole model
@pytest.mark.gpu
@pytest.mark.parametrize("case,cls", [("av_x3dl_64", "AudioVisualSaliencyModel"), ("vis_x3dl_64", "VisualSaliencyModel")], ids=["av", "vis"])
def test_hip_whole_model_trains_its_lateral_blocks(dev, golden_dir, monkeypatch, case, cls):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    from mspi_amd import metrics as M
    from mspi_amd._lib import MspiError
    from mspi_amd.model import model_utils as pm
    from test_readout_tail import _batches, _build
    E.autotune(False)          # bits are compared (tests/test_fusion_train.py::test_hip_whole_model_trains_its_fusion says why)
    # ... and with tuning off engine._choose still takes what an earlier test's tuning left in the cache: tile choices made by
    # timing, so the forward's last bits would follow the tests that ran before.  The gradient of readout.12.bias is a sum that
    # cancels to rounding level (the log-softmax is shift invariant), and whether AdamW moves that tensor hangs on those bits.
    # An empty cache (put back afterwards) pins the library's own choices.
    monkeypatch.setitem(E.AUTOTUNE, "cache", {})
    sound = cls == "AudioVisualSaliencyModel"
    g, cfg, make, clips, audio = _build(golden_dir, case, "x3dl", cls, dev)
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

    m.trainable("fusion")
    m.train()
    m.frozen_encoder()
    f_out, f_grads = step_grads()
    assert len(f_grads) == 31

    m.trainable("lateral_blocks")
    m.eval()
    with pytest.raises(MspiError, match="frozen_encoder"):      # eval() BatchNorm and a graph: batch statistics would be a surprise
        m(*args)
    m.train()
    m.frozen_encoder()
    # no_grad under the switch: the launches of inference.  (The fusion step above has moved the five layers' running statistics,
    # so the map to compare with is this model's own switch-off map now, taken under trainable(None) below.)
    with torch.no_grad():
        quiet = m(*args)[0]
    assert not quiet.requires_grad

    calls = []

    class Recorded:
        @staticmethod
        def apply(x, *ps):
            y = A.LateralBlock.apply(x, *ps)
            rec = {"x": x.detach().clone()}
            y.register_hook(lambda gr, rec=rec: rec.__setitem__("G", gr.detach().clone()))
            calls.append(rec)
            return y
    monkeypatch.setattr(pm, "LateralBlock", Recorded)
    start = {k: v.clone() for k, v in m.state_dict().items()}
    params = [p for p in m.parameters() if p.requires_grad]
    assert len(params) == 71
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0)
    b_out, b_grads = step_grads()
    monkeypatch.undo()
    # on identical weights and input: the map and the 31 SA and readout gradients have the bits of trainable("fusion")
    assert torch.equal(b_out, f_out)
    assert sorted(b_grads) == _trained_names(m) and len(calls) == 4
    for n, gr in f_grads.items():
        assert torch.equal(b_grads[n], gr), n
    # the 40 block gradients against the float64 backward, fed the block inputs and the d l_k of this very run
    for k, rec in enumerate(calls):
        blk = getattr(m, "latlayer_%d" % k)[-1]
        prefix = "latlayer_%d.%d." % (k, len(getattr(m, "latlayer_%d" % k)) - 1)
        c = {n: p.detach().cpu().numpy() for n, p in zip(LR.PARAMS, blk.tensors())}
        c["x"], c["G"] = (rec[n].permute(0, 4, 1, 2, 3).cpu().numpy() for n in ("x", "G"))
        ref = LR.backward(c, LR.forward(c), c["G"])
        for n in LR.PARAMS:
            got = b_grads[prefix + LR.STATE_KEYS[n]]
            assert torch.isfinite(got).all()
            e = _err(got, ref[n])
            print("%s latlayer_%d d %s: %.2e" % (case, k, n, e))
            assert e <= GRAD_TOL, (k, n)
    opt.step()
    moved = set(_trained_names(m)) | {"%s.%s" % (mod, n) for mod in BATCH_STAT for n in ("running_mean", "running_var", "num_batches_tracked")}
    for k, v in m.state_dict().items():
        assert torch.equal(v, start[k]) == (k not in moved), k
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
@pytest.mark.parametrize("case,cls", [("av_x3dl_64", "AudioVisualSaliencyModel"), ("vis_x3dl_64", "VisualSaliencyModel")], ids=["av", "vis"])
def test_hip_switch_on_under_no_grad_is_the_switch_off_map(dev, golden_dir, case, cls):
    from mspi_amd import engine as E
    from test_readout_tail import _build
    E.autotune(False)
    g, cfg, make, clips, audio = _build(golden_dir, case, "x3dl", cls, dev)
    args = (clips, audio) if cls == "AudioVisualSaliencyModel" else (clips,)
    m = make().to(dev)
    off = m(*args)[0]
    m.trainable("lateral_blocks")
    m.train()
    m.frozen_encoder()
    with torch.no_grad():
        quiet = m(*args)[0]
    assert torch.equal(quiet, off) and not quiet.requires_grad
