"""The whole SyncBlock differentiated by hand: csrc/linear_wgrad.hip (mspi_linear_wgrad, declared in
include/mspi_linear_train_hip.h), engine.linear_wgrad, autograd.linear_wgrad_route, SyncEmbed, sync_block and
SyncBlock.tensors().  No stage of the training ladder reaches the SyncBlock yet, and SyncBlock._pack / run and Block._pack / run
are untouched: the Functions' forwards restate their launches and the end-to-end tests hold them to their bits.

Yardsticks: tests/golden/sync_tokens.npz holds "tiny" (B = 1, one visual and one audio token, C4 = 192) with the float64 slab of
the embedding, the output y of the three blocks and the embedding's eight gradients of <slab, G> ("tiny.e.*") and of <y, G>
("tiny.d.*") that torch autograd gives through torch.nn layers with upstream's arguments (tools/gen_sync_tokens_golden.py;
dW_proj, rank one at one token, as its two factors), and the seed of "odd" (B = 2, vis 1x3x2, aud 1x1x5, C4 = 784);
tests/sync_tokens_restate.py is the float64 restatement in this project's order with its analytic backward, pinned to that
fixture and, here, to torch autograd on "odd".

Bounds.  Every tensor: max |got - ref| / max |ref| <= GRAD_TOL = 2e-5, the project's bar for gradients
(tests/test_readout_train.py); every test prints its figure before it asserts.  The fp32 MFMA is a k-ordered fmaf chain, about
1e-7 of sum |a b|, and torch FLOAT32 on the CPU agrees with float64 on all 47 tensors of the two cases to 7.4e-7 .. 7.7e-7 on the
generator's seeds, so the bar leaves a factor of about twenty-five.  The kernel is judged against float64 dy^T x."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import sync_block_restate as SR
import sync_tokens_restate as TR
from test_fusion_train import _declared, _judge, _poisoned, _replayed, _stream
from test_readout_train import GRAD_TOL
from test_sync_block_train import _judge_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_linear_wgrad_ws_bytes", "mspi_linear_wgrad_variant", "mspi_linear_wgrad")
OLDER_HEADERS = ("mspi_hip.h", "mspi_train_hip.h", "mspi_block_train_hip.h", "mspi_entry_train_hip.h", "mspi_adapter_train_hip.h",
                 "mspi_sync_train_hip.h")
CASES = ("odd", "tiny")
# name: (B, vis (t, h, w), aud (F, T'), C4)
SHAPES = {"tiny": (1, (1, 1, 1), (1, 1), 192), "odd": (2, (1, 3, 2), (1, 5), 784)}
# (M, N, K, extra columns of the buffers the operands are read from in the "slab" pass); the fifth case is sized from the variant
KERNEL_CASES = [(1, 32, 4, 12), (37, 32, 36, 12), (130, 96, 784, 12), (257, 1536, 512, 8), "slices"]


def _slice_rows(M, N, K):
    """The header's formula, restated."""
    blocks = -(-N // 128) * -(-K // 128)
    want = max(1, 512 // blocks)
    return min(max(128, 32 * -(-(-(-M // want)) // 32)), (1 << 31) - 32)


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "sync_tokens.npz"))
    return {k: z[k] for k in z.files}


def _gold_grad(tag, k):
    g = _gold()
    if k == "wp":
        return np.outer(g["tiny.%s.wp.u" % tag], g["tiny.%s.wp.v" % tag])
    return g["tiny.%s.%s" % (tag, k)]


@functools.lru_cache(maxsize=None)
def _restated(key):
    """(case, embedding slab, embedding gradients of <slab, G>, (y, embedding gradients, block gradients) of <y, G>) in float64,
    computed once and left unchanged."""
    B, thw, ft, C4 = SHAPES[key]
    case = TR.make_case(B, thw, ft, C4, int(_gold()[key + ".shape"][-1]))
    return case, TR.embed_forward(case)[0], TR.embed_backward(case), TR.backward(case)


# ------------------------------------------------------------------------------------------------------------- CPU
def test_linear_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    from mspi_amd import engine as E
    linear, _ = _declared("mspi_linear_train_hip.h")
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert linear == set(NEW_SYMBOLS) == set(_lib.LINEAR_EXPORTS) == set(_lib._LINEAR_SIGNATURES)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _lib._LINEAR_SIGNATURES[name][1], name
    older = set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.BLOCK_EXPORTS) | set(_lib.ENTRY_EXPORTS) | \
        set(_lib.ADAPTER_EXPORTS) | set(_lib.SYNC_EXPORTS)
    for header in OLDER_HEADERS:
        older |= _declared(header)[0]
    assert not older & set(NEW_SYMBOLS)
    base, base_text = _declared("mspi_hip.h")
    assert base == set(_lib.EXPORTS)
    assert re.search(r"#define MSPI_ABI_VERSION 2\b", base_text) and lib.mspi_version() == 2
    for name in ("linear_wgrad", "linear_wgrad_variant"):
        assert callable(getattr(E, name)) and name in E.__all__
    src = open(os.path.join(ROOT, "mspi_amd", "csrc", "linear_wgrad.hip")).read()
    assert "atomic" not in src.lower()
    mk = open(os.path.join(ROOT, "mspi_amd", "csrc", "Makefile")).read()
    assert "linear_wgrad.hip" in mk and mk.count("mspi_linear_train_hip.h") == 2 and "-fno-slp-vectorize" in mk


def test_host_refusals_and_slice_arithmetic():
    from mspi_amd import _lib
    lib = _lib.load()

    def err():
        return lib.mspi_last_error().decode()
    base = dict(x=4096, ldx=36, dy=8192, lddy=64, dW=12288, db=16384, ws=20480, M=70, N=64, K=36)

    def run(**kw):
        p = dict(base, **kw)
        rc = lib.mspi_linear_wgrad(p["x"], p["ldx"], p["dy"], p["lddy"], p["dW"], p["db"], p["ws"], p["M"], p["N"], p["K"], None)
        return rc, err()

    def variant(**kw):
        p = dict(base, **kw)
        return lib.mspi_linear_wgrad_variant(p["x"], p["ldx"], p["dy"], p["lddy"], p["M"], p["N"], p["K"]), err()
    for name in ("x", "dy", "dW", "ws"):
        rc, why = run(**{name: None})
        assert rc == -1 and "mspi_linear_wgrad: null argument" in why, (name, rc, why)
    for name in ("x", "dy", "dW", "db", "ws"):
        rc, why = run(**{name: base[name] + 4})
        assert rc == -1 and "mspi_linear_wgrad" in why and "16-byte aligned" in why, (name, rc, why)
    # by shape: the launch, the variant and the workspace size refuse the same things
    shapes = {"N must be a multiple of 32": dict(N=48, lddy=48), "N must be a multiple of 32 ": dict(N=0),
              "K must be a multiple of 4": dict(K=38, ldx=40), "K must be a multiple of 4 ": dict(K=0),
              "at most 4096": dict(N=4128, lddy=4128), "at most 4096 ": dict(K=4100, ldx=4100),
              "no rows": dict(M=0), "no rows ": dict(M=-5), "2^31": dict(M=1 << 31), "2^31 ": dict(M=(1 << 31) + 7)}
    for text, kw in shapes.items():
        rc, why = run(**kw)
        assert rc == -1 and "mspi_linear_wgrad: " in why and text.strip() in why, (text, rc, why)
        v, why = variant(**kw)
        assert v == -1 and text.strip() in why, (text, v, why)
        p = dict(base, **kw)
        assert lib.mspi_linear_wgrad_ws_bytes(p["M"], p["N"], p["K"]) == 0, text
    # by operand: strides below the width or not multiples of 4
    for text, kw in {"multiples of 4": dict(ldx=38), "multiples of 4 ": dict(lddy=66), ">= the width": dict(ldx=32),
                     ">= the width ": dict(lddy=60)}.items():
        rc, why = run(**kw)
        assert rc == -1 and "mspi_linear_wgrad: " in why and text.strip() in why, (text, rc, why)
        v, why = variant(**kw)
        assert v == -1 and text.strip() in why, (text, v, why)
    assert variant(x=None)[0] == -1 and "null argument" in err()
    assert variant(dy=8196)[0] == -1 and "16-byte aligned" in err()
    # the largest accepted extents, and the slice arithmetic on a handful of shapes: the model's and the edges of the formula
    assert variant(M=(1 << 31) - 1, N=4096, K=4096, ldx=4096, lddy=4096)[0] == _slice_rows((1 << 31) - 1, 4096, 4096)
    for M, N, K in [(70, 64, 36), (1, 32, 4), (1640, 512, 512), (1640, 1536, 512), (11472, 2048, 512), (11472, 512, 2048), (2868, 512, 784),
                    (5736, 512, 192), (128 * 512 + 1, 32, 4), (300, 4096, 4096), (293, 160, 132)]:
        L = _slice_rows(M, N, K)
        assert L % 32 == 0 and L >= 128
        assert variant(M=M, N=N, K=K, ldx=K, lddy=N)[0] == L, (M, N, K)
        assert lib.mspi_linear_wgrad_ws_bytes(M, N, K) == -(-M // L) * (N * K + N) * 4, (M, N, K)


def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["names"]) == CASES and tuple(g["grads"]) == TR.EMBED_GRADS and len(TR.EMBED_GRADS) == 8
    for c in CASES:
        B, thw, ft, C4 = SHAPES[c]
        assert tuple(g[c + ".shape"][:-1]) == (B,) + thw + ft + (C4,)
    assert g["tiny.slab"].shape == g["tiny.y"].shape == (1, 2, 512) and g["tiny.slab"].dtype == g["tiny.y"].dtype == np.float64
    case = _restated("tiny")[0]
    for tag in ("e", "d"):
        for k in TR.EMBED_GRADS:
            assert _gold_grad(tag, k).shape == case[k].shape and _gold_grad(tag, k).dtype == np.float64, (tag, k)
    assert not any(k.startswith("odd.") and k != "odd.shape" for k in g)          # "odd" is its seed
    golden = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(golden, "sync_tokens.npz")) <= os.path.getsize(os.path.join(golden, "sync_block.npz"))


def test_restatement_matches_the_fixture():
    case, slab, alone, (y, through, _) = _restated("tiny")
    assert SR.rel_err(slab, _gold()["tiny.slab"]) <= 1e-12 and SR.rel_err(y, _gold()["tiny.y"]) <= 1e-12
    for k in TR.EMBED_GRADS:
        assert SR.rel_err(alone[k], _gold_grad("e", k)) <= 1e-12, k
        assert SR.rel_err(through[k], _gold_grad("d", k)) <= 1e-12, k


def test_restatement_matches_torch_autograd_on_odd():
    """ "odd" is stored as its seed: torch.nn layers with upstream's arguments, float64, built here."""
    case, slab, alone, (y, through, blocks) = _restated("odd")
    ref_slab, ref_alone, _ = TR.upstream_grads(case, blocks=False)
    ref_y, ref_through, ref_blocks = TR.upstream_grads(case)
    assert SR.rel_err(slab, ref_slab) <= 1e-12 and SR.rel_err(y, ref_y) <= 1e-12
    for k in TR.EMBED_GRADS:
        assert SR.rel_err(alone[k], ref_alone[k]) <= 1e-12, k
        assert SR.rel_err(through[k], ref_through[k]) <= 1e-12, k
    for i in range(TR.NBLOCKS):
        for k in SR.NAMES:
            assert SR.rel_err(blocks[i][k], ref_blocks[i][k]) <= 1e-12, (i, k)


def test_sync_block_tensors_order():
    from mspi_amd import autograd as A
    from mspi_amd.model import model_utils as pm
    m = pm.SyncBlock(num_blocks=3, num_vis_tokens=6, num_aud_tokens=5, vis_in_embed=784)
    want = (m.vis_proj.weight, m.vis_proj.bias, m.vis_norm.weight, m.vis_norm.bias, m.aud_norm.weight, m.aud_norm.bias)
    got = m.tensors()
    assert len(got) == 6 == len(A.SYNC_EMBED_TENSORS) and all(x is y for x, y in zip(got, want))
    names = dict(m.named_parameters())
    assert all(names[n] is t for n, t in zip(A.SYNC_EMBED_TENSORS, got))
    assert len(names) == 6 + 3 * 11 == 39
    case = _restated("odd")[0]
    assert tuple(case[k].shape for k in TR.EMBED) == tuple(tuple(t.shape) for t in got)
    assert A.linear_wgrad_route(1640, 1536, 512) in ("linear", "sliced")


# ------------------------------------------------------------------------------------------------------------- GPU, kernel
@functools.lru_cache(maxsize=None)
def _kernel_case(which):
    """(M, N, K, pad), fp32 x [M, K] and dy [M, N] and the float64 (dW, db); computed once."""
    from mspi_amd import _lib
    if which == "slices":
        lib = _lib.load()
        N, K, pad = 160, 132, 12
        L = lib.mspi_linear_wgrad_variant(4096, K, 8192, N, 1, N, K)
        M = 2 * L + 37
        assert lib.mspi_linear_wgrad_variant(4096, K, 8192, N, M, N, K) == L and -(-M // L) >= 3 and M % L
    else:
        M, N, K, pad = which
    gen = torch.Generator().manual_seed(8000 + M + N + K)
    x, dy = torch.randn(M, K, generator=gen), torch.randn(M, N, generator=gen)
    return (M, N, K, pad), x, dy, (dy.double().t() @ x.double(), dy.double().sum(0))


def _lw_launch(dev, x, dy, pad=0, bias=True, static=None):
    """mspi_linear_wgrad on x [M, K] and dy [M, N]: dense with pad = 0; otherwise each inside a [M + 3][width + pad] buffer, 8
    columns in, with NaN in every cell the kernel has no business with, the three rows after M included.  dW and db are
    written into NaN-filled buffers with 64 cells to spare.  Returns (dW [N, K], db [N] or None, the two whole buffers)."""
    from mspi_amd import _lib
    lib = _lib.load()
    M, K = x.shape
    N = dy.shape[1]

    def place(t, name):
        if static is not None:
            return static[name], t.shape[1]
        if not pad:
            return t.contiguous().to(dev), t.shape[1]
        buf = torch.full((M + 3, t.shape[1] + pad), float("nan"), device=dev)
        buf[:M, 8:8 + t.shape[1]] = t.to(dev)
        return buf[:, 8:], t.shape[1] + pad
    xs, ldx = place(x, "x")
    ds, lddy = place(dy, "dy")
    wbuf = torch.full((N * K + 64,), float("nan"), device=dev)
    bbuf = torch.full((N + 64,), float("nan"), device=dev)
    ws = torch.empty(lib.mspi_linear_wgrad_ws_bytes(M, N, K) // 4, device=dev)
    assert ws.numel() == -(-M // _slice_rows(M, N, K)) * (N * K + N)
    _lib.check(lib.mspi_linear_wgrad(xs.data_ptr(), ldx, ds.data_ptr(), lddy, wbuf.data_ptr(), bbuf.data_ptr() if bias else None,
                                     ws.data_ptr(), M, N, K, _stream()), "mspi_linear_wgrad")
    return wbuf[:N * K].view(N, K), (bbuf[:N] if bias else None), (wbuf, bbuf)


@pytest.mark.gpu
@pytest.mark.parametrize("which", KERNEL_CASES, ids=lambda c: c if isinstance(c, str) else "x".join(map(str, c[:3])))
def test_hip_linear_wgrad_vs_fp64(dev, which):
    (M, N, K, pad), x, dy, (rW, rb) = _kernel_case(which)
    print("linear_wgrad case %s: M=%d N=%d K=%d, %d rows a slice" % (which, M, N, K, _slice_rows(M, N, K)))
    first = None
    for p in (0, pad):
        what = "linear_wgrad (%d, %d, %d) %s" % (M, N, K, "in a wider buffer" if p else "dense")
        dW, db, (wbuf, bbuf) = _lw_launch(dev, x, dy, p)
        torch.cuda.synchronize()
        _judge_grad(what + " dW", dW, rW)
        _judge_grad(what + " db", db, rb)
        # every cell of dW and db written and nothing else
        assert torch.isnan(wbuf[N * K:]).all() and torch.isnan(bbuf[N:]).all()
        again = _lw_launch(dev, x, dy, p)
        assert torch.equal(again[0], dW) and torch.equal(again[1], db), "two runs differ"
        if first is None:
            first = (dW.clone(), db.clone())
        else:          # where the operands lie changes nothing
            assert torch.equal(dW, first[0]) and torch.equal(db, first[1])
        # db = NULL: dW as before, db untouched
        dW0, none, (_, bbuf0) = _lw_launch(dev, x, dy, p, bias=False)
        assert none is None and torch.equal(dW0, dW) and torch.isnan(bbuf0).all()
    dWz, dbz, _ = _lw_launch(dev, x, torch.zeros_like(dy), pad)
    assert not dWz.any() and not dbz.any()                                    # dy = 0: exact zeros


@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_hip_linear_wgrad_nonfinite_operands_propagate(dev, value):
    from mspi_amd import engine as E
    (M, N, K, pad), x, dy, _ = _kernel_case((130, 96, 784, 12))
    E._need_gpu(torch.empty(1, device=dev))
    for name, idx in (("x", (77, 770)), ("dy", (129, 65))):
        ops = {"x": x, "dy": dy}
        ops[name] = _poisoned(ops[name], idx, value)
        rW, rb = ops["dy"].double().t() @ ops["x"].double(), ops["dy"].double().sum(0)
        E.range_flag()
        dW, db, _ = _lw_launch(dev, ops["x"], ops["dy"], pad)
        torch.cuda.synchronize()
        assert E.range_flag(), "linear_wgrad %s: a poisoned output did not set the status word" % name
        _judge("linear_wgrad %s -> dW" % name, dW, rW)
        bad = ~torch.isfinite(dW.cpu())
        if name == "x":           # column k of dW and never db
            assert bad[:, idx[1]].all() and int(bad.sum()) == N
            _judge_grad("linear_wgrad x -> db (independent)", db, rb)
        else:                     # row n of dW and db[n]
            assert bad[idx[1]].all() and int(bad.sum()) == K
            _judge("linear_wgrad dy -> db", db, rb)
            assert int((~torch.isfinite(db.cpu())).sum()) == 1
    E.range_flag()
    dW, db, _ = _lw_launch(dev, x, dy, pad)
    torch.cuda.synchronize()
    assert not E.range_flag() and torch.isfinite(dW).all() and torch.isfinite(db).all()


@pytest.mark.gpu
def test_hip_linear_wgrad_capture_and_replay(dev):
    (M, N, K, pad), x, dy, _ = _kernel_case("slices")
    gen = torch.Generator().manual_seed(77)
    other = {"x": torch.randn(M, K, generator=gen), "dy": torch.randn(M, N, generator=gen)}

    def launch(t, host):
        dW, db, _ = _lw_launch(dev, x, dy, static=t)
        return {"dW": dW, "db": db}
    _replayed(dev, {"A": {"x": x, "dy": dy}, "B": other}, launch)


@pytest.mark.gpu
def test_hip_engine_linear_wgrad_reads_a_slab_and_refuses_by_name(dev):
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    (M, N, K, pad), x, dy, (rW, rb) = _kernel_case((257, 1536, 512, 8))
    xc = E.from_rows(x.to(dev))
    slab = torch.full((M, N + 8), float("nan"), device=dev)                   # the [rows][3][4][128] (+ 8) slab attention_bwd writes
    slab[:, :N] = dy.to(dev)
    dc = E.CL(slab.view(-1), 0, M, 1, 1, 1, N, N + 8)
    assert E.linear_wgrad_variant(xc, dc) == _slice_rows(M, N, K)
    dW, db = E.linear_wgrad(xc, dc)
    _judge_grad("engine.linear_wgrad dW", dW, rW)
    _judge_grad("engine.linear_wgrad db", db, rb)
    dW0, none = E.linear_wgrad(xc, E.from_rows(dy.to(dev)), bias=False)
    assert none is None and torch.equal(dW0, dW) and tuple(dW.shape) == (N, K) and tuple(db.shape) == (N,)
    with pytest.raises(MspiError, match="GPU only"):
        E.linear_wgrad(E.from_rows(x), dc)
    with pytest.raises(MspiError, match="GPU only"):
        E.linear_wgrad(xc, E.from_rows(dy))
    with pytest.raises(MspiError, match="linear_wgrad: x has 257 rows, dy 256"):
        E.linear_wgrad(xc, E.from_rows(dy[:-1].contiguous().to(dev)))
    with pytest.raises(MspiError, match="linear_wgrad: .*N must be a multiple of 32"):
        E.linear_wgrad(xc, E.from_rows(dy[:, :48].contiguous().to(dev)))
    with pytest.raises(MspiError, match="linear_wgrad: .*at most 4096"):
        E.linear_wgrad(E.from_rows(torch.zeros(4, 4100, device=dev)), E.from_rows(torch.zeros(4, 32, device=dev)))
    with pytest.raises(MspiError, match="linear_wgrad: .*row strides must be multiples of 4"):
        E.linear_wgrad(E.CL(torch.zeros(M * 514, device=dev), 0, M, 1, 1, 1, K, 514), dc)
    with pytest.raises(MspiError, match="linear_wgrad: .*16-byte aligned"):
        E.linear_wgrad(E.CL(torch.zeros(M * K + 4, device=dev), 2, M, 1, 1, 1, K, K), dc)
    with pytest.raises(MspiError, match="no sample stride"):
        E.linear_wgrad(E.CL(torch.zeros(2 * M * K, device=dev), 0, 1, M, 1, 1, K, K, 2 * M * K), dc)


# ------------------------------------------------------------------------------------------------------------- GPU, Functions
def _module(case, dev, nblocks):
    """A SyncBlock with the case's tensors (its first nblocks blocks), on the GPU in eval mode."""
    from mspi_amd.model import model_utils as pm
    m = pm.SyncBlock(num_blocks=nblocks, num_vis_tokens=case["Rv"], num_aud_tokens=case["Ra"], vis_in_embed=case["C4"])
    with torch.no_grad():
        for p, k in zip(m.tensors(), TR.EMBED):
            p.copy_(torch.from_numpy(case[k]))
        for blk, c in zip(m.blocks, case["blocks"]):
            for p, k in zip(blk.tensors(), SR.NAMES):
                p.copy_(torch.from_numpy(c[k]))
    return m.to(dev).eval()


def _inputs(case, dev, wrt=("vis", "aud")):
    return (torch.from_numpy(case[k]).float().to(dev).requires_grad_(k in wrt) for k in ("vis", "aud"))


def _embed(case, dev, gscale=1.0, wrt=TR.EMBED_GRADS):
    """(slab, {name: gradient}) of autograd.SyncEmbed on the case, gradients of <slab, gscale G>."""
    from mspi_amd import autograd as A
    vis, aud = _inputs(case, dev, wrt)
    ps = [torch.from_numpy(case[k]).float().to(dev).requires_grad_(k in wrt) for k in TR.EMBED]
    tabs = [torch.from_numpy(case[k]).float().to(dev) for k in ("vpos", "apos")]
    slab = A.SyncEmbed.apply(vis, aud, *ps, *tabs)
    slab.backward(torch.from_numpy(case["G"]).float().to(dev) * gscale)
    return slab.detach(), dict(zip(TR.EMBED_GRADS, [vis.grad, aud.grad] + [p.grad for p in ps]))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["tiny", "odd"])
def test_hip_sync_embed_end_to_end(dev, key):
    from mspi_amd import engine as E
    E.autotune(False)
    case, ref_slab, alone, _ = _restated(key)
    slab, got = _embed(case, dev)
    # the forward has the bits of the inference path on the same tensors (a SyncBlock without blocks is its embedding)
    m = _module(case, dev, 0)
    vis, aud = _inputs(case, dev, ())
    run = m.run(E.CL(vis.view(-1), 0, *vis.shape, vis.shape[4]), E.CL(aud.view(-1), 0, *aud.shape, aud.shape[4]))
    assert torch.equal(run.as_rows().view(slab.shape), slab)
    _judge_grad("SyncEmbed %s slab" % key, slab, torch.from_numpy(_gold()["tiny.slab"]) if key == "tiny" else ref_slab)
    ref = {k: _gold_grad("e", k) for k in TR.EMBED_GRADS} if key == "tiny" else alone
    for k in TR.EMBED_GRADS:
        _judge_grad("SyncEmbed %s d %s" % (key, k), got[k], ref[k])
    # at the scale of a loss
    s = 2.0 ** -20
    for k, g in _embed(case, dev, gscale=s)[1].items():
        _judge_grad("SyncEmbed %s, G x 2^-20, d %s" % (key, k), g, torch.as_tensor(ref[k]).double() * s)


@pytest.mark.gpu
def test_hip_sync_embed_asks_only_and_refuses_by_name(dev):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    E.autotune(False)
    case = _restated("odd")[0]
    _, full = _embed(case, dev)
    _, one = _embed(case, dev, wrt=("ga",))
    assert torch.equal(one["ga"], full["ga"]) and all(one[k] is None for k in TR.EMBED_GRADS if k != "ga")
    vis, aud = _inputs(case, dev, ())
    ps = [torch.from_numpy(case[k]).float().to(dev) for k in TR.EMBED]
    vpos, apos = (torch.from_numpy(case[k]).float().to(dev) for k in ("vpos", "apos"))
    wp = ps[0].clone().requires_grad_(True)
    slab = A.SyncEmbed.apply(vis, aud, wp, *ps[1:], vpos, apos)
    with E.Profiler() as prof:                                                # the frozen encoders' gradients cost no launch
        slab.backward(torch.from_numpy(case["G"]).float().to(dev))
    assert [r[0] for r in prof.records] == ["layernorm_bwd_wide", "linear_wgrad"] and torch.equal(wp.grad, full["wp"])
    with pytest.raises(MspiError, match="GPU only"):
        A.SyncEmbed.apply(vis.cpu(), aud.cpu(), *[p.cpu() for p in ps], vpos.cpu(), apos.cpu())
    with pytest.raises(MspiError, match="SyncBlock: got 6 visual / 5 audio tokens but the positional tables hold 5 / 5 rows"):
        A.SyncEmbed.apply(vis, aud, *ps, vpos[:5].contiguous(), apos)
    with pytest.raises(MspiError, match="SyncBlock: got 6 visual / 5 audio tokens but the positional tables hold 6 / 6 rows"):
        A.SyncEmbed.apply(vis, aud, *ps, vpos, vpos)
    with pytest.raises(MspiError, match=r"SyncEmbed: vis must be fp32 \[B,t,h,w,C4\]"):
        A.SyncEmbed.apply(vis[0], aud, *ps, vpos, apos)
    with pytest.raises(MspiError, match=r"SyncEmbed: aud is .* expected \[2,1,F,T',512\]"):
        A.SyncEmbed.apply(vis, aud[..., :256].contiguous(), *ps, vpos, apos)
    with pytest.raises(MspiError, match=r"SyncEmbed: vis_proj.weight is \(512, 192\)"):
        A.SyncEmbed.apply(vis, aud, ps[0][:, :192].contiguous(), *ps[1:], vpos, apos)
    leaf = aud.clone().requires_grad_(True)
    gx, = torch.autograd.grad(A.SyncEmbed.apply(vis, leaf, *ps, vpos, apos).sum(), leaf, create_graph=True)
    with pytest.raises(RuntimeError):       # no double backward: the gradient carries no graph, or one that refuses
        torch.autograd.grad(gx.sum(), leaf)


def _sync(case, dev, m, wrt=None):
    """(y, vis.grad, aud.grad, {parameter name: gradient}) of autograd.sync_block on the module m, gradients of <y, G>; wrt: the
    parameter names (and "vis" / "aud") that require grad, default all."""
    from mspi_amd import autograd as A
    names = dict(m.named_parameters())
    for n, p in names.items():
        p.grad = None
        p.requires_grad_(wrt is None or n in wrt)
    vis, aud = _inputs(case, dev, ("vis", "aud") if wrt is None else wrt)
    y = A.sync_block(m, vis, aud)
    y.backward(torch.from_numpy(case["G"]).float().to(dev))
    return y.detach(), vis.grad, aud.grad, {n: (None if p.grad is None else p.grad.clone()) for n, p in names.items()}


@pytest.mark.gpu
def test_hip_sync_block_end_to_end(dev):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    E.autotune(False)
    case, _, _, (ref_y, ref_e, ref_b) = _restated("odd")
    m = _module(case, dev, TR.NBLOCKS)
    y, dvis, daud, got = _sync(case, dev, m)
    assert len(got) == 39 and all(g is not None for g in got.values())
    # the bits of the inference path: SyncBlock.forward on the NCDHW views of the same inputs
    vis, aud = _inputs(case, dev, ())
    with torch.no_grad():
        fwd = m(vis.permute(0, 4, 1, 2, 3), aud.permute(0, 4, 1, 2, 3))
    assert torch.equal(fwd, y)
    _judge_grad("sync_block odd y", y, ref_y)
    _judge_grad("sync_block odd d vis", dvis, ref_e["vis"])
    _judge_grad("sync_block odd d aud", daud, ref_e["aud"])
    for n, k in zip(A.SYNC_EMBED_TENSORS, TR.EMBED):
        _judge_grad("sync_block odd d %s" % n, got[n], ref_e[k])
    for i in range(TR.NBLOCKS):
        for n, k in zip(A.BLOCK_TENSORS, SR.NAMES):
            _judge_grad("sync_block odd d blocks.%d.%s" % (i, n), got["blocks.%d.%s" % (i, n)], ref_b[i][k])
    # repeatable to the bit
    y2, dvis2, daud2, got2 = _sync(case, dev, m)
    assert torch.equal(y2, y) and torch.equal(dvis2, dvis) and torch.equal(daud2, daud)
    assert all(torch.equal(got2[n], got[n]) for n in got)
    # asking for one tensor returns None for the rest and the same bits for that one
    for only in ("vis_norm.weight", "blocks.1.mlp.fc1.weight"):
        y3, dvis3, daud3, got3 = _sync(case, dev, m, wrt=(only,))
        assert torch.equal(y3, y) and dvis3 is None and daud3 is None
        assert torch.equal(got3[only], got[only]) and all(g is None for n, g in got3.items() if n != only)


@pytest.mark.gpu
def test_hip_transformer_block_backward_launches_no_sliced_wgrad(dev, monkeypatch):
    """The Block's four weight gradients are four mspi_linear_wgrad launch pairs under the "linear" route; the "sliced" route
    is the path the Block had before, with the same gradients within the bar."""
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    E.autotune(False)
    case = SR.make_case(2, 37, 12)
    ref = SR.backward(case)

    def run():
        x = torch.from_numpy(case["x"]).float().to(dev).requires_grad_(True)
        ps = [torch.from_numpy(case[k]).float().to(dev).requires_grad_(True) for k in SR.NAMES]
        y = A.TransformerBlock.apply(x, *ps)
        with E.Profiler() as prof:
            y.backward(torch.from_numpy(case["G"]).float().to(dev))
        return [r[0] for r in prof.records], dict(zip(SR.GRADS, [x.grad] + [p.grad for p in ps]))
    assert all(A.linear_wgrad_route(2 * 37, n, k) == "linear" for n, k in ((512, 2048), (2048, 512), (512, 512), (1536, 512)))
    names, got = run()
    print("TransformerBlock.backward launches:", names)
    assert names.count("linear_wgrad") == 4 and not any(n.startswith("conv_wgrad_wide") for n in names), names
    monkeypatch.setattr(A, "linear_wgrad_route", lambda M, N, K: "sliced")
    sliced_names, sliced = run()
    assert "linear_wgrad" not in sliced_names and sliced_names.count("conv_wgrad_wide") == 99, sliced_names
    for k in ("wqkv", "wproj", "bproj", "w1", "b1", "w2", "b2"):
        _judge_grad("TransformerBlock linear route d %s" % k, got[k], ref[k])
        _judge_grad("TransformerBlock sliced route d %s" % k, sliced[k], ref[k])
        assert got[k].shape == sliced[k].shape
