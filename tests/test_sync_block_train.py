"""The transformer Block of the SyncBlock differentiated by hand: csrc/sync_bwd.hip (mspi_attn_bwd, mspi_layernorm_bwd_wide,
declared in include/mspi_sync_train_hip.h), engine.attention_bwd / layernorm_bwd_wide, autograd.TransformerBlock,
pack_transformer_block and Block.tensors().  No stage of the training ladder reaches the block yet, and Block._pack and
Block.run are untouched: the Function's forward restates their launches and the end-to-end tests hold it to their bits.

Yardsticks: tests/golden/sync_block.npz holds "tiny" ((B, R) = (1, 1)) with the float64 output and twelve gradients of <y, G>
that torch autograd gives through torch.nn layers with upstream's arguments (tools/gen_sync_block_golden.py; the six weight
gradients, rank one at one row, as their two factors) and the seed of "odd" ((2, 37)); tests/sync_block_restate.py is the
float64 restatement in this project's order with its analytic backward, pinned to that fixture and, here, to torch autograd on
"odd".

Bounds.  Every tensor: max |got - ref| / max |ref| <= GRAD_TOL = 2e-5, the project's bar for gradients
(tests/test_readout_train.py); every test prints its figure before it asserts.  Torch FLOAT32 on the CPU agrees with float64
on all twelve tensors to 6.1e-7 .. 7.4e-7 on the generator's seeds, so the bar leaves a factor of about thirty.  One reference
is identically zero: with a single key the softmax is 1, dS = dP - Delta cancels exactly and dq = dk = 0; there the error is
measured against what cancelled, scale * sum_d |dO_d v_d| * max |k| (or max |q|), the size of the terms whose difference it is.
The ledger part holds the two entry points to what tests/test_lateral_train.py holds its three."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import sync_block_restate as SR
from test_fusion_train import _declared, _judge, _poisoned, _replayed, _stream
from test_readout_train import GRAD_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_attn_bwd_ws_bytes", "mspi_attn_bwd_variant", "mspi_attn_bwd", "mspi_layernorm_bwd_wide_ws_bytes",
               "mspi_layernorm_bwd_wide")
CASES = ("odd", "tiny")
SHAPES = {"tiny": (1, 1), "odd": (2, 37), "tile": (1, 130), "default": (1, 372)}      # 372 = 336 + 36, the reference default
SEEDS = {"tile": 9601, "default": 9602}
ATTN_CASES = [(1, 1, 1, 1), (1, 1, 31, 33), (1, 2, 33, 95), (2, 4, 130, 130), (1, 4, 820, 820)]
LN_CASES = [(2, 512), (90, 512), (257, 260), (513, 388), (372, 512)]
D = 128


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "sync_block.npz"))
    return {k: z[k] for k in z.files}


def _gold_grad(k):
    g = _gold()
    if "tiny.d%s.u" % k in g:
        return np.outer(g["tiny.d%s.u" % k], g["tiny.d%s.v" % k])
    return g["tiny.d" + k]


@functools.lru_cache(maxsize=None)
def _restated(key):
    """(case, saved, grads) in float64, computed once and left unchanged."""
    seed = int(_gold()[key + ".shape"][2]) if key in CASES else SEEDS[key]
    case = SR.make_case(*SHAPES[key], seed=seed)
    return case, SR.forward(case), SR.backward(case)


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["names"]) == CASES and tuple(g["grads"]) == SR.GRADS and len(SR.GRADS) == 12
    for c in CASES:
        assert tuple(g[c + ".shape"][:2]) == SHAPES[c]
    assert g["tiny.y"].shape == (1, 1, 512) and g["tiny.y"].dtype == np.float64
    case = SR.make_case(1, 1, 0)
    for k in SR.GRADS:
        assert _gold_grad(k).shape == case[k].shape and _gold_grad(k).dtype == np.float64, k
    golden = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(golden, "sync_block.npz")) <= os.path.getsize(os.path.join(golden, "fusion.npz"))


def test_restatement_matches_the_fixture():
    case, saved, grads = _restated("tiny")
    assert SR.rel_err(saved["y"], _gold()["tiny.y"]) <= 1e-12
    for k in SR.GRADS:
        assert SR.rel_err(grads[k], _gold_grad(k)) <= 1e-12, k


def test_restatement_matches_torch_autograd_on_odd():
    """ "odd" is stored as its seed: torch.nn layers with upstream's arguments, float64, built here."""
    case, saved, grads = _restated("odd")
    y, ref = SR.upstream_grads(case)
    assert SR.rel_err(saved["y"], y) <= 1e-12
    for k in SR.GRADS:
        assert SR.rel_err(grads[k], ref[k]) <= 1e-12, k


def test_sync_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    from mspi_amd import engine as E
    sync, _ = _declared("mspi_sync_train_hip.h")
    base, base_text = _declared("mspi_hip.h")
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert sync == set(NEW_SYMBOLS) == set(_lib.SYNC_EXPORTS) == set(_lib._SYNC_SIGNATURES)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _lib._SYNC_SIGNATURES[name][1], name
    older = set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.BLOCK_EXPORTS) | set(_lib.ENTRY_EXPORTS) | set(_lib.ADAPTER_EXPORTS)
    for header in ("mspi_train_hip.h", "mspi_block_train_hip.h", "mspi_entry_train_hip.h", "mspi_adapter_train_hip.h"):
        older |= _declared(header)[0]
    assert base == set(_lib.EXPORTS) and not (older | base) & set(NEW_SYMBOLS)
    assert re.search(r"#define MSPI_ABI_VERSION 2\b", base_text) and lib.mspi_version() == 2
    for name in ("attention_bwd", "layernorm_bwd_wide"):
        assert callable(getattr(E, name)) and name in E.__all__
    src = open(os.path.join(ROOT, "mspi_amd", "csrc", "sync_bwd.hip")).read()
    assert "atomic" not in src.lower()
    mk = open(os.path.join(ROOT, "mspi_amd", "csrc", "Makefile")).read()
    assert "sync_bwd.hip" in mk and mk.count("mspi_sync_train_hip.h") == 2 and "-fno-slp-vectorize" in mk


def _attn_desc(B=1, Hh=2, Nq=5, Nk=7, Dq=D, Dv=D, prec=0, nmask=0, nwin=0, pad=0):
    from mspi_amd import _lib
    d = _lib.AttnDesc()
    d.B, d.Hh, d.Nq, d.Nk, d.D, d.Dv, d.nmask, d.nwin = B, Hh, Nq, Nk, Dq, Dv, nmask, nwin
    d.q_sB, d.q_sH, d.q_sT = Hh * Nq * Dq + pad, Nq * Dq, Dq
    d.k_sB, d.k_sH, d.k_sT = Hh * Nk * Dq, Nk * Dq, Dq
    d.v_sB, d.v_sH, d.v_sT = Hh * Nk * Dv, Nk * Dv, Dv
    d.o_sB, d.o_sH, d.o_sT = Hh * Nq * Dv, Nq * Dv, Dv
    d.scale, d.prec = D ** -0.5, prec
    return d


def test_host_refusals():
    from mspi_amd import _lib
    lib = _lib.load()

    def err():
        return lib.mspi_last_error().decode()
    ptrs = dict(q=4096, k=8192, v=12288, o=16384, dO=20480, dq=24576, dk=28672, dv=32768, ws=36864)

    def bwd(d=None, **kw):
        p = dict(ptrs, **kw)
        d = _attn_desc() if d is None else d
        rc = lib.mspi_attn_bwd(ctypes.byref(d), p["q"], p["k"], p["v"], p["o"], p["dO"], p["dq"], p["dk"], p["dv"], p["ws"], None)
        return rc, err()
    for name in ptrs:
        rc, why = bwd(**{name: None})
        assert rc == -1 and "mspi_attn_bwd: null argument" in why, (name, rc, why)
        rc, why = bwd(**{name: ptrs[name] + 4})
        assert rc == -1 and "mspi_attn_bwd" in why and "16-B aligned" in why, (name, rc, why)
    assert lib.mspi_attn_bwd(None, *([4096] * 9), None) == -1 and "null argument" in err()
    refused = {"(D=64, Dv=64) not in {(128,128)}": _attn_desc(Dq=64, Dv=64), "(D=128, Dv=96) not in {(128,128)}": _attn_desc(Dv=96),
               "prec = 1": _attn_desc(prec=_lib.PREC_F16X3), "empty extent": _attn_desc(Nq=0), "empty extent ": _attn_desc(Nk=0),
               "no mask and no token index": _attn_desc(nmask=1), "no mask and no token index ": _attn_desc(nwin=2),
               "multiples of 4": _attn_desc(pad=2), "B*H too large": _attn_desc(B=1 << 14, Hh=4)}
    for text, d in refused.items():
        rc, why = bwd(d=d)
        assert rc == -1 and "mspi_attn_bwd: " in why and text.strip() in why, (text, rc, why)
        assert lib.mspi_attn_bwd_variant(ctypes.byref(d)) == -1 and text.strip() in err(), (text, err())
        assert lib.mspi_attn_bwd_ws_bytes(ctypes.byref(d)) == 0
    good = _attn_desc()
    assert lib.mspi_attn_bwd_variant(ctypes.byref(good)) == 10000000 + 128 * 10000 + 128 * 10
    assert lib.mspi_attn_bwd_variant(None) == -1 and lib.mspi_attn_bwd_ws_bytes(None) == 0
    assert lib.mspi_attn_bwd_ws_bytes(ctypes.byref(good)) == 1 * 2 * 5 * 2 * 4          # [lse | Delta] per (sequence, head, query)

    def lnw(x=4096, ldx=512, dy=8192, lddy=512, gamma=12288, eps=1e-5, dx=16384, lddx=512, dgam=20480, dbet=24576, ws=28672, M=3, C=512):
        return lib.mspi_layernorm_bwd_wide(x, ldx, dy, lddy, gamma, eps, dx, lddx, dgam, dbet, ws, M, C, None), err()
    for C_ in (256, 516, 8, 262, 0):
        rc, why = lnw(C=C_, ldx=520, lddy=520, lddx=520)
        assert rc == -1 and "mspi_layernorm_bwd_wide: C=%d" % C_ in why and "256 < C <= 512" in why, (C_, rc, why)
        assert lib.mspi_layernorm_bwd_wide_ws_bytes(3, C_) == 0
    for rc, why in (lnw(ldx=510), lnw(lddy=256), lnw(lddx=514), lnw(x=4100), lnw(dy=8200), lnw(dx=16388)):
        assert rc == -1 and "mspi_layernorm_bwd_wide" in why and "multiples of 4" in why, (rc, why)
    for rc, why in (lnw(x=None), lnw(dy=None), lnw(gamma=None), lnw(dx=None), lnw(dgam=None), lnw(dbet=None), lnw(ws=None)):
        assert rc == -1 and "null argument" in why, (rc, why)
    assert lnw(gamma=12292)[0] == -1 and lnw(ws=28676)[0] == -1 and lnw(eps=-1.0)[0] == -1
    assert lnw(M=0)[0] == -1 and "no rows" in lnw(M=0)[1]
    assert lnw(M=1 << 31)[0] == -1 and "2^31" in lnw(M=1 << 31)[1]
    assert lib.mspi_layernorm_bwd_wide_ws_bytes(0, 512) == 0
    assert lib.mspi_layernorm_bwd_wide_ws_bytes(257, 388) == 2 * 2 * 388 * 4            # one record [dbeta | dgamma] per 256 rows
    # the older entry point keeps its limit
    assert lib.mspi_layernorm_bwd(4096, 512, 8192, 512, 12288, 1e-5, 16384, 512, 20480, 24576, 28672, 3, 512, None) == -1
    assert "at most 256" in err()


def test_block_tensors_order():
    from mspi_amd import autograd as A
    from mspi_amd.model import model_utils as pm
    blk = pm.Block(dim=512, num_heads=4)
    a, m = blk.attn, blk.mlp
    want = (blk.norm1.weight, blk.norm1.bias, a.qkv.weight, a.proj.weight, a.proj.bias, blk.norm2.weight, blk.norm2.bias, m.fc1.weight,
            m.fc1.bias, m.fc2.weight, m.fc2.bias)
    got = blk.tensors()
    assert len(got) == 11 == len(A.BLOCK_TENSORS) and all(x is y for x, y in zip(got, want)) and a.qkv.bias is None
    names = dict(blk.named_parameters())
    assert all(names[n] is t for n, t in zip(A.BLOCK_TENSORS, got))
    assert tuple(SR.make_case(1, 1, 0)[k].shape for k in SR.NAMES) == tuple(tuple(t.shape) for t in got)


# ------------------------------------------------------------------------------------------------------------- GPU
def _judge_grad(what, got, ref, den=None):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    e = (got - ref).abs().max().item() / (ref.abs().max().item() if den is None else den)
    print("%s: %.2e" % (what, e))
    assert e <= GRAD_TOL, what
    return e


@functools.lru_cache(maxsize=None)
def _attn_case(shape, mult):
    """fp32 q, k, v, dO [B, H, N, 128], o in fp32 from float64, and the float64 (dq, dk, dv); computed once."""
    B, H, Nq, Nk = shape
    gen = torch.Generator().manual_seed(7000 + Nq * 3 + Nk + int(mult))
    q, dO = torch.randn(B, H, Nq, D, generator=gen), torch.randn(B, H, Nq, D, generator=gen)
    k, v = torch.randn(B, H, Nk, D, generator=gen), torch.randn(B, H, Nk, D, generator=gen)
    scale = mult * D ** -0.5
    o = SR.attention(q.double(), k.double(), v.double(), scale)
    ref = SR.attention_bwd(q.double(), k.double(), v.double(), dO.double(), scale, o=o.float().double())
    # a single key: dq and dk are zero but for the float64 rounding of the reference itself; judged against what cancels
    cancel = scale * (dO.double().abs() * o.abs()).sum(-1).max().item()
    dens = (cancel * k.abs().max().item(), cancel * q.abs().max().item(), None) if Nk == 1 else (None, None, None)
    return {"q": q, "k": k, "v": v, "dO": dO, "o": o.float(), "scale": scale}, ref, dens


def _attn_launch(dev, ops, shape, slab, desc_out=None, static=None):
    """mspi_attn_bwd on the operands: dense [B, H, N, 128] tensors, or every operand inside a [rows][3][H][128] (+ 8 columns)
    slab -- o and dO inside [rows][H][128] (+ 4) -- with NaN in every cell the kernel has no business with, dqkv written in
    place into such a slab.  Returns (dq, dk, dv) as [B, H, N, 128] views and the output buffer."""
    from mspi_amd import _lib
    lib = _lib.load()
    B, H, Nq, Nk = shape
    d = _lib.AttnDesc()
    d.B, d.Hh, d.Nq, d.Nk, d.D, d.Dv, d.nmask, d.nwin = B, H, Nq, Nk, D, D, 0, 0
    d.scale, d.prec = ops["scale"], _lib.PREC_F32
    t = {n: (static[n] if static is not None else ops[n].to(dev)) for n in ("q", "k", "v", "o", "dO")}
    if not slab:
        d.q_sB, d.q_sH, d.q_sT = H * Nq * D, Nq * D, D
        d.k_sB, d.k_sH, d.k_sT = d.v_sB, d.v_sH, d.v_sT = H * Nk * D, Nk * D, D
        d.o_sB, d.o_sH, d.o_sT = H * Nq * D, Nq * D, D
        out = torch.full((B * H * (Nq + 2 * Nk) * D,), float("nan"), device=dev)
        dq, dk, dv = out[:B * H * Nq * D].view(B, H, Nq, D), out[B * H * Nq * D:B * H * (Nq + Nk) * D].view(B, H, Nk, D), \
            out[B * H * (Nq + Nk) * D:].view(B, H, Nk, D)
        src = t
    else:
        rows, ld, ldo = max(Nq, Nk), 3 * H * D + 8, H * D + 4
        d.q_sB = d.k_sB = d.v_sB = rows * ld
        d.q_sH = d.k_sH = d.v_sH = D
        d.q_sT = d.k_sT = d.v_sT = ld
        d.o_sB, d.o_sH, d.o_sT = rows * ldo, D, ldo
        qkv = torch.full((B, rows, ld), float("nan"), device=dev)
        out = torch.full((B, rows, ld), float("nan"), device=dev)
        os_, gs = torch.full((B, rows, ldo), float("nan"), device=dev), torch.full((B, rows, ldo), float("nan"), device=dev)

        def view(buf, which, n):      # [B, H, n, D] view of part `which` of a slab
            return buf[:, :n, which * H * D:(which + 1) * H * D].view(B, n, H, D).permute(0, 2, 1, 3)
        view(qkv, 0, Nq).copy_(t["q"]); view(qkv, 1, Nk).copy_(t["k"]); view(qkv, 2, Nk).copy_(t["v"])
        view(os_, 0, Nq).copy_(t["o"]); view(gs, 0, Nq).copy_(t["dO"])
        src = {"q": view(qkv, 0, Nq), "k": view(qkv, 1, Nk), "v": view(qkv, 2, Nk), "o": view(os_, 0, Nq), "dO": view(gs, 0, Nq)}
        dq, dk, dv = view(out, 0, Nq), view(out, 1, Nk), view(out, 2, Nk)
    if desc_out is not None:
        desc_out.append(d)
    ws = torch.empty(lib.mspi_attn_bwd_ws_bytes(ctypes.byref(d)) // 4, device=dev)
    assert ws.numel() == 2 * B * H * Nq
    ptrs = [x.data_ptr() for x in (src["q"], src["k"], src["v"], src["o"], src["dO"], dq, dk, dv)]      # a view's pointer is its first cell
    _lib.check(lib.mspi_attn_bwd(ctypes.byref(d), *ptrs, ws.data_ptr(), _stream()), "mspi_attn_bwd")
    return (dq, dk, dv), out


@pytest.mark.gpu
@pytest.mark.parametrize("mult", [1.0, 4.0], ids=["std1", "peaked"])
@pytest.mark.parametrize("shape", ATTN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_hip_attention_bwd_vs_fp64(dev, shape, mult):
    ops, ref, dens = _attn_case(shape, mult)
    B, H, Nq, Nk = shape
    for slab in (False, True):
        got, out = _attn_launch(dev, ops, shape, slab)
        torch.cuda.synchronize()
        for name, g, r, den in zip(("dq", "dk", "dv"), got, ref, dens):
            _judge_grad("attention_bwd %s scale x%g %s %s" % (shape, mult, "slab" if slab else "dense", name), g, r, den)
        # every other cell of the output buffer is as it was: NaN in the slab's pads and in rows past Nq / Nk
        assert int(torch.isfinite(out).sum()) == B * H * (Nq + 2 * Nk) * D
        again, _ = _attn_launch(dev, ops, shape, slab)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs differ"
    zero = dict(ops, dO=torch.zeros_like(ops["dO"]))
    (dq, dk, dv), _ = _attn_launch(dev, zero, shape, False)
    assert not dv.any() and not dq.any() and not dk.any()                     # dv = P^T 0 exactly; dS = P (0 - 0)


@pytest.mark.gpu
def test_hip_engine_attention_bwd_writes_a_slab_in_place_and_refuses_by_name(dev):
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    shape = (2, 4, 130, 130)
    ops, ref, _ = _attn_case(shape, 1.0)
    B, H, N, _ = shape

    def rows(t):      # [B, H, N, D] -> [B * N, H * D]
        return t.permute(0, 2, 1, 3).reshape(B * N, H * D)
    qkv = E.from_rows(torch.cat([rows(ops[n]) for n in ("q", "k", "v")], 1).contiguous().to(dev)).reshape(B, N, 1, 1)
    o, dO = (E.from_rows(rows(ops[n]).contiguous().to(dev)).reshape(B, N, 1, 1) for n in ("o", "dO"))
    out = E.alloc(B, N, 1, 1, 3 * H * D, dev)
    assert E.attention_bwd(qkv, o, dO, B, N, H, D, ops["scale"], out=out) is out
    fresh = E.attention_bwd(qkv, o, dO, B, N, H, D, ops["scale"])
    assert torch.equal(fresh.as_rows(), out.as_rows())
    for i, name in enumerate(("dq", "dk", "dv")):
        _judge_grad("engine.attention_bwd %s" % name, out.as_rows()[:, i * H * D:(i + 1) * H * D], rows(ref[i]))
    with pytest.raises(MspiError, match="GPU only"):
        E.attention_bwd(E.from_rows(qkv.as_rows().cpu()), o, dO, B, N, H, D, 1.0)
    with pytest.raises(MspiError, match="attention_bwd: dO is"):
        E.attention_bwd(qkv, o, E.from_rows(dO.as_rows()[:-1].contiguous()), B, N, H, D, 1.0)
    with pytest.raises(MspiError, match="attention_bwd: qkv is"):
        E.attention_bwd(qkv, o, dO, B, N - 1, H, D, 1.0)
    with pytest.raises(MspiError, match=r"attention_bwd: head dim \(D=64, Dv=64\) not in"):
        E.attention_bwd(qkv, o, dO, B, N, 2 * H, 64, 1.0)
    with pytest.raises(MspiError, match="attention_bwd: out is"):
        E.attention_bwd(qkv, o, dO, B, N, H, D, 1.0, out=o)


def _ln_case(M, C, seed):
    gen = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(M, C, generator=gen) + torch.randn(M, 1, generator=gen)
    return x, torch.randn(M, C, generator=gen), 1.0 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)


def _rows_cl(t, dev, ld=None):
    """[M, C] -> CL of M rows (ld > C: inside a wider buffer that holds NaN elsewhere)."""
    from mspi_amd import engine as E
    M, C = t.shape
    if ld is None:
        return E.CL(t.contiguous().to(dev).view(-1), 0, M, 1, 1, 1, C, C)
    buf = torch.full((M, ld), float("nan"), device=dev)
    buf[:, ld - C:] = t.to(dev)
    return E.CL(buf.view(-1), ld - C, M, 1, 1, 1, C, ld)


@pytest.mark.gpu
@pytest.mark.parametrize("M,C", LN_CASES)
def test_hip_layernorm_bwd_wide_vs_fp64(dev, M, C):
    from mspi_amd import _lib
    from mspi_amd import engine as E
    lib = _lib.load()
    x, dy, gam, bet = _ln_case(M, C, 100 + M)
    ref = SR.layernorm_bwd(dy.double(), x.double(), gam.double())
    got = E.layernorm_bwd_wide(_rows_cl(dy, dev), _rows_cl(x, dev), gam.to(dev))
    for name, a, b in zip(("dx", "dgamma", "dbeta"), got, ref):
        _judge_grad("layernorm_bwd_wide (%d, %d) %s" % (M, C, name), a.as_rows() if hasattr(a, "as_rows") else a, b)
    again = E.layernorm_bwd_wide(_rows_cl(dy, dev), _rows_cl(x, dev), gam.to(dev))
    assert torch.equal(again[0].as_rows(), got[0].as_rows()) and torch.equal(again[1], got[1]) and torch.equal(again[2], got[2])
    # padded row strides with NaN in the pads change nothing (the raw entry point: the wrapper takes dense rows)
    ld = C + 12
    xs, ds = _rows_cl(x, dev, ld), _rows_cl(dy, dev, ld)
    dxs = torch.full((M, ld), float("nan"), device=dev)
    dgb = torch.empty(2, C, device=dev)
    ws = torch.empty(lib.mspi_layernorm_bwd_wide_ws_bytes(M, C) // 4, device=dev)
    _lib.check(lib.mspi_layernorm_bwd_wide(xs.ptr, ld, ds.ptr, ld, gam.to(dev).data_ptr(), 1e-5, dxs.data_ptr(), ld, dgb[0].data_ptr(),
                                           dgb[1].data_ptr(), ws.data_ptr(), M, C, _stream()), "mspi_layernorm_bwd_wide")
    assert torch.equal(dxs[:, :C], got[0].as_rows()) and torch.isnan(dxs[:, C:]).all()
    assert torch.equal(dgb[0], got[1]) and torch.equal(dgb[1], got[2])
    # x^ has the forward's bits: under a one-hot dy, dgamma is that row's x^, which E.layernorm gives with gamma 1, beta 0
    r = M // 2
    hot = torch.zeros(M, C)
    hot[r] = 1.0
    one, nul = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    _, dgam, dbet = E.layernorm_bwd_wide(_rows_cl(hot, dev), _rows_cl(x, dev), one)
    fwd = E.layernorm(_rows_cl(x, dev), one, nul, 1e-5)
    assert torch.equal(dgam, fwd.as_rows()[r]) and torch.equal(dbet, one)


@pytest.mark.gpu
def test_hip_engine_layernorm_bwd_wide_refuses_by_name(dev):
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    x, dy, gam, _ = _ln_case(6, 512, 2)
    with pytest.raises(MspiError, match="layernorm_bwd_wide: dy must match"):
        E.layernorm_bwd_wide(_rows_cl(dy[:, :388], dev), _rows_cl(x, dev), gam.to(dev))
    with pytest.raises(MspiError, match="layernorm_bwd_wide: gamma must be a contiguous fp32"):
        E.layernorm_bwd_wide(_rows_cl(dy, dev), _rows_cl(x, dev), gam[:4].to(dev))
    with pytest.raises(MspiError, match="GPU only"):
        E.layernorm_bwd_wide(_rows_cl(dy, "cpu"), _rows_cl(x, "cpu"), gam)
    for C in (256, 516):
        z = torch.zeros(2, C)
        with pytest.raises(MspiError, match="layernorm_bwd_wide: rows of %d channels" % C):
            E.layernorm_bwd_wide(_rows_cl(z, dev), _rows_cl(z, dev), torch.ones(C, device=dev))
    with pytest.raises(MspiError, match="at most 256"):                      # the older wrapper keeps its limit
        E.layernorm_bwd(_rows_cl(dy, dev), _rows_cl(x, dev), gam.to(dev))


# ---- autograd.TransformerBlock
def _params(case, dev, grad=True):
    return [torch.from_numpy(case[k]).float().to(dev).requires_grad_(grad) for k in SR.NAMES]


def _block(case, dev, gscale=1.0, wrt=None):
    """(y, {name: gradient}) of autograd.TransformerBlock on the case, gradients of <y, gscale G>."""
    from mspi_amd import autograd as A
    wrt = SR.GRADS if wrt is None else wrt
    x = torch.from_numpy(case["x"]).float().to(dev).requires_grad_("x" in wrt)
    ps = _params(case, dev, False)
    for k, p in zip(SR.NAMES, ps):
        p.requires_grad_(k in wrt)
    y = A.TransformerBlock.apply(x, *ps)
    y.backward(torch.from_numpy(case["G"]).float().to(dev) * gscale)
    return y.detach(), dict(zip(SR.GRADS, [x.grad] + [p.grad for p in ps]))


def _assert_block_grads(got, ref, what, scale=1.0):
    for k in SR.GRADS:
        _judge_grad("%s d %s" % (what, k), got[k], torch.as_tensor(ref[k]).double() * scale)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["tiny", "odd", "tile", "default"])
def test_hip_transformer_block_end_to_end(dev, key):
    from mspi_amd import engine as E
    from mspi_amd.model import model_utils as pm
    E.autotune(False)
    case, saved, grads = _restated(key)
    B, R = SHAPES[key]
    y, got = _block(case, dev)
    # the forward has the bits of the inference path on the same tensors
    blk = pm.Block(dim=512, num_heads=4)
    with torch.no_grad():
        for p, k in zip(blk.tensors(), SR.NAMES):
            p.copy_(torch.from_numpy(case[k]))
    blk = blk.to(dev).eval()
    run = blk.run(E.CL(torch.from_numpy(case["x"]).float().to(dev).view(-1), 0, B, R, 1, 1, 512, 512), B, R)
    assert torch.equal(run.as_rows().view(B, R, 512), y)
    _judge_grad("TransformerBlock %s y" % key, y, torch.from_numpy(_gold()["tiny.y"]) if key == "tiny" else saved["y"])
    ref = {k: _gold_grad(k) for k in SR.GRADS} if key == "tiny" else grads
    _assert_block_grads(got, ref, "TransformerBlock %s" % key)


@pytest.mark.gpu
@pytest.mark.parametrize("exp", [-20, 12])
def test_hip_transformer_block_gradients_at_the_scale_of_a_loss(dev, exp):
    from mspi_amd import engine as E
    E.autotune(False)
    case, _, grads = _restated("odd")
    _assert_block_grads(_block(case, dev, gscale=2.0 ** exp)[1], grads, "TransformerBlock odd, G x 2^%d" % exp, scale=2.0 ** exp)


@pytest.mark.gpu
def test_hip_three_blocks_chained(dev):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    E.autotune(False)
    B, R = SHAPES["odd"]
    blocks = [SR.make_case(1, 1, 9700 + i) for i in range(3)]
    first = SR.make_case(B, R, 9710)
    ref_y, ref = SR.chain(blocks, first["x"], first["G"])
    x = torch.from_numpy(first["x"]).float().to(dev).requires_grad_(True)
    ps = [_params(c, dev) for c in blocks]
    y = x
    for p in ps:
        y = A.TransformerBlock.apply(y, *p)
    y.backward(torch.from_numpy(first["G"]).float().to(dev))
    _judge_grad("three blocks y", y, ref_y)
    _judge_grad("three blocks d x", x.grad, ref[0]["x"])
    for i, p in enumerate(ps):
        for k, t in zip(SR.NAMES, p):
            _judge_grad("three blocks, block %d d %s" % (i, k), t.grad, ref[i][k])


@pytest.mark.gpu
def test_hip_transformer_block_is_repeatable_asks_only_and_refuses_by_name(dev):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    E.autotune(False)
    case = _restated("odd")[0]
    y1, g1 = _block(case, dev)
    y2, g2 = _block(case, dev)
    assert torch.equal(y1, y2) and all(torch.equal(g1[k], g2[k]) for k in SR.GRADS)
    y3, g3 = _block(case, dev, wrt=("w2",))
    assert torch.equal(y3, y1) and torch.equal(g3["w2"], g1["w2"]) and all(g3[k] is None for k in SR.GRADS if k != "w2")
    x = torch.from_numpy(case["x"]).float().to(dev)
    ps = _params(case, dev, False)
    with pytest.raises(MspiError, match="GPU only"):
        A.TransformerBlock.apply(x.cpu(), *[p.cpu() for p in ps])
    with pytest.raises(MspiError, match=r"x must be fp32 \[B,R,512\]"):
        A.TransformerBlock.apply(x[0], *ps)
    with pytest.raises(MspiError, match=r"x must be fp32 \[B,R,512\]"):
        A.TransformerBlock.apply(x[..., :256].contiguous(), *ps)
    with pytest.raises(MspiError, match=r"x must be fp32 \[B,R,512\]"):
        A.TransformerBlock.apply(x.double(), *ps)
    with pytest.raises(MspiError, match=r"attn.qkv.weight is \(1024, 512\).* has \(1536, 512\)"):
        A.TransformerBlock.apply(x, ps[0], ps[1], ps[2][:1024].contiguous(), *ps[3:])
    with pytest.raises(MspiError, match="mlp.fc1.bias is"):
        A.TransformerBlock.apply(x, *ps[:8], ps[8].cpu(), *ps[9:])
    leaf = x.clone().requires_grad_(True)
    gx, = torch.autograd.grad(A.TransformerBlock.apply(leaf, *ps).sum(), leaf, create_graph=True)
    with pytest.raises(RuntimeError):       # no double backward: the gradient carries no graph, or one that refuses
        torch.autograd.grad(gx.sum(), leaf)


# ---- the ledger of the two entry points
@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_hip_ledger_nonfinite_operands_propagate(dev, value):
    from mspi_amd import engine as E
    shape = (1, 2, 33, 95)
    ops, _, _ = _attn_case(shape, 1.0)
    spots = {"q": (0, 1, 7, 40), "k": (0, 0, 90, 3), "v": (0, 1, 50, 127), "o": (0, 0, 32, 64), "dO": (0, 1, 0, 5)}
    for name, idx in spots.items():
        bad = dict(ops)
        bad[name] = _poisoned(ops[name], idx, value)
        if name != "o":           # the stored o is the forward's on the poisoned operands
            bad["o"] = SR.attention(bad["q"].double(), bad["k"].double(), bad["v"].double(), ops["scale"]).float()
        ref = SR.attention_bwd(bad["q"].double(), bad["k"].double(), bad["v"].double(), bad["dO"].double(), ops["scale"], o=bad["o"].double())
        E._need_gpu(torch.empty(1, device=dev))
        E.range_flag()
        got, _ = _attn_launch(dev, bad, shape, False)
        torch.cuda.synchronize()
        assert E.range_flag(), "attention_bwd %s: a poisoned output did not set the status word" % name
        for out, g, r in zip(("dq", "dk", "dv"), got, ref):
            if torch.isfinite(r).all():                                       # dv reads neither q's Delta nor o
                _judge_grad("attention_bwd %s -> %s (independent)" % (name, out), g, r)
            else:
                _judge("attention_bwd %s -> %s" % (name, out), g, r)
        other = 1 - idx[1]                                                    # the other head of the sequence is untouched
        assert all(torch.isfinite(g[0, other]).all() for g in got)
    M, C = 70, 388
    x, dy, gam, _ = _ln_case(M, C, 12)
    for name, idx in (("x", (37, 200)), ("dy", (69, 387)), ("gam", (300,))):
        t = {"x": x, "dy": dy, "gam": gam}
        t[name] = _poisoned(t[name], idx, value)
        ref = SR.layernorm_bwd(t["dy"].double(), t["x"].double(), t["gam"].double())
        dx, dgam, dbet = E.layernorm_bwd_wide(_rows_cl(t["dy"], dev), _rows_cl(t["x"], dev), t["gam"].to(dev))
        _judge("layernorm_bwd_wide %s -> dx" % name, dx.as_rows(), ref[0])
        if name == "gam":                                                     # neither sum reads gamma
            _judge_grad("layernorm_bwd_wide gam -> dgamma", dgam, ref[1]); _judge_grad("layernorm_bwd_wide gam -> dbeta", dbet, ref[2])
        else:
            _judge("layernorm_bwd_wide %s -> dgamma" % name, dgam, ref[1])
            if name == "dy":
                _judge("layernorm_bwd_wide dy -> dbeta", dbet, ref[2])
            else:
                _judge_grad("layernorm_bwd_wide x -> dbeta", dbet, ref[2])    # dbeta does not read x
    E.range_flag()


@pytest.mark.gpu
def test_hip_ledger_capture_and_replay(dev):
    from mspi_amd import _lib
    lib = _lib.load()
    shape = (1, 2, 33, 95)

    def operands(mult):
        ops = _attn_case(shape, mult)[0]
        return {n: ops[n] for n in ("q", "k", "v", "o", "dO")}

    def attn(t, host):
        (dq, dk, dv), _ = _attn_launch(dev, {"scale": D ** -0.5}, shape, False, desc_out=host, static=t)
        return {"dq": dq, "dk": dk, "dv": dv}
    _replayed(dev, {"A": operands(1.0), "B": operands(4.0)}, attn)

    M, C = 300, 388

    def lnw(t, host):
        dx, dgb = torch.empty(M, C, device=dev), torch.empty(2, C, device=dev)
        ws = torch.empty(lib.mspi_layernorm_bwd_wide_ws_bytes(M, C) // 4, device=dev)
        _lib.check(lib.mspi_layernorm_bwd_wide(t["x"].data_ptr(), C, t["dy"].data_ptr(), C, t["gam"].data_ptr(), 1e-5, dx.data_ptr(), C,
                                               dgb[0].data_ptr(), dgb[1].data_ptr(), ws.data_ptr(), M, C, _stream()),
                   "mspi_layernorm_bwd_wide")
        return {"dx": dx, "dgb": dgb}
    _replayed(dev, {w: dict(zip(("x", "dy", "gam"), _ln_case(M, C, s)[:3])) for w, s in (("A", 23), ("B", 24))}, lnw)
