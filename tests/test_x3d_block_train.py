"""The X3D residual block's training path: mspi_x3d_train_hip.h (csrc/x3d_bwd.hip), its engine wrappers, autograd.X3DBlock and
autograd.x3d_blocks.

CPU: the float64 restatement (tests/x3d_block_restate.py) against the stored fixture and against torch autograd through
torch.nn layers built with upstream's arguments; the ninth header's symbols declared = exported = bound and disjoint from the
older headers'; the refusals that need no GPU.
GPU: every new kernel against float64, autograd.X3DBlock against the restatement at GRAD_TOL = 2e-5 of each tensor's largest
entry (torch's own fp32 loses 4e-7 .. 2e-6 on these cases: tools/gen_x3d_block_golden.py prints it), the running statistics,
repeatability, x3d_blocks over three blocks, and the two ledgers (non-finite operands propagate; capture and replay)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import x3d_block_restate as XR
from test_fusion_train import _judge, _replayed
from test_readout_train import GRAD_TOL, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_dwconv3_wgrad_supported", "mspi_dwconv3_wgrad_ws_bytes", "mspi_dwconv3_wgrad", "mspi_bn_gate_act_fwd",
               "mspi_gate_swish_bwd_ws_bytes", "mspi_gate_swish_bwd", "mspi_se_train_fwd", "mspi_se_train_bwd_ws_bytes",
               "mspi_se_train_bwd", "mspi_relu_mask_add")
OLDER_HEADERS = ("mspi_train_hip.h", "mspi_block_train_hip.h", "mspi_entry_train_hip.h", "mspi_adapter_train_hip.h",
                 "mspi_sync_train_hip.h", "mspi_linear_train_hip.h", "mspi_contrast_train_hip.h")
WRAPPERS = ("dwconv3_wgrad", "bn_gate_act", "gate_swish_bwd", "se_train_fwd", "se_train_bwd", "relu_mask_add")
# name: (dim_out, dim_inner, B, T, h, w, se); the seeds are the fixture's
CASES = {"tiny": (32, 72, 1, 2, 2, 2, 1), "odd_se": (32, 72, 2, 3, 5, 7, 1), "odd": (32, 72, 2, 3, 5, 7, 0),
         "s4": (96, 216, 1, 2, 3, 4, 1), "s5": (192, 432, 1, 2, 3, 4, 0), "s5_map": (192, 432, 1, 16, 7, 12, 1),
         "chain0": (32, 72, 2, 2, 3, 5, 1), "chain1": (32, 72, 2, 2, 3, 5, 0), "chain2": (32, 72, 2, 2, 3, 5, 1)}
BLOCK_CASES = ("tiny", "odd_se", "odd", "s4", "s5", "s5_map")
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "x3d_block.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _restated(key):
    """(case, forward dict, {name: float64 gradient}) of the restatement; computed once and left unchanged."""
    spec = [int(v) for v in _gold()[key + ".shape"]]
    case = XR.make_case(*spec[:6], bool(spec[6]), spec[7])
    fwd = XR.forward(case)
    return case, fwd, XR.backward(case, fwd)


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases():
    g = _gold()
    assert sorted(g["names"].tolist()) == sorted(CASES)
    assert tuple(g["grads"].tolist()) == XR.GRADS == ("x",) + XR.PARAMS and len(XR.PARAMS) == 13
    for name, spec in CASES.items():
        assert tuple(int(v) for v in g[name + ".shape"][:7]) == spec, name
    D, Ci, B, T, h, w, _ = CASES["tiny"]
    assert g["tiny.y"].shape == g["tiny.x"].shape == (B, T, h, w, D) and g["tiny.y"].dtype == np.float64
    assert g["tiny.wb"].shape == (Ci, 1, 3, 3, 3) and g["tiny.w1"].shape == (XR.se_width(Ci), Ci, 1, 1, 1)
    assert B * T * h * w > 2                     # with two rows BatchNorm's x^ is +-1 and dx cancels to zero
    path = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(os.path.join(path, "x3d_block.npz")) <= os.path.getsize(os.path.join(path, "fusion.npz"))


def test_restatement_matches_the_fixture():
    g = _gold()
    case, fwd, grads = _restated("tiny")
    assert XR.rel_err(fwd["y"], g["tiny.y"]) <= 1e-12
    for k in XR.GRADS:
        assert XR.rel_err(grads[k], g["tiny." + k]) <= 1e-12, k


@pytest.mark.parametrize("key", ["odd_se", "odd"])
def test_restatement_matches_torch_autograd_in_float64(key):
    case, fwd, grads = _restated(key)
    y, ref = XR.upstream_grads(case)
    assert sorted(ref) == sorted(grads) == sorted(("x",) + XR.params(case))
    assert XR.rel_err(fwd["y"], y) <= 1e-12
    for k in ref:
        assert XR.rel_err(grads[k], ref[k]) <= 1e-12, k


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(mspi_[a-z0-9_]+)\s*\(", text)), text


def test_x3d_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    from mspi_amd import engine as E
    declared, _ = _declared("mspi_x3d_train_hip.h")
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert declared == set(NEW_SYMBOLS) == set(_lib.X3D_EXPORTS) == set(_lib._X3D_SIGNATURES)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _lib._X3D_SIGNATURES[name][1], name
    older = set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.BLOCK_EXPORTS) | set(_lib.ENTRY_EXPORTS) | \
        set(_lib.ADAPTER_EXPORTS) | set(_lib.SYNC_EXPORTS) | set(_lib.LINEAR_EXPORTS) | set(_lib.CONTRAST_EXPORTS)
    for header in OLDER_HEADERS:
        older |= _declared(header)[0]
    assert not older & set(NEW_SYMBOLS)
    base, base_text = _declared("mspi_hip.h")
    assert base == set(_lib.EXPORTS)
    assert re.search(r"#define MSPI_ABI_VERSION 2\b", base_text) and lib.mspi_version() == 2
    for name in WRAPPERS:
        assert callable(getattr(E, name)) and name in E.__all__, name
    src = open(os.path.join(ROOT, "mspi_amd", "csrc", "x3d_bwd.hip")).read()
    assert "atomic" not in src.lower()
    mk = open(os.path.join(ROOT, "mspi_amd", "csrc", "Makefile")).read()
    assert "x3d_bwd.hip" in mk and mk.count("mspi_x3d_train_hip.h") == 2 and "-fno-slp-vectorize" in mk
    for header in OLDER_HEADERS[1:]:
        assert mk.count(header) == 2, header


def _dw_desc(N=1, T=2, H=3, W=4, C=8, ldx=None, ldy=None, k=(3, 3, 3), s=(1, 1, 1), p=(1, 1, 1), out=None):
    from mspi_amd import _lib
    d = _lib.DwConvDesc()
    d.N, d.T, d.H, d.W, d.C = N, T, H, W, C
    d.ldx, d.ldy = C if ldx is None else ldx, C if ldy is None else ldy
    d.kT, d.kH, d.kW = k
    d.strT, d.strH, d.strW = s
    d.padT, d.padH, d.padW = p
    d.To, d.Ho, d.Wo = (T, H, W) if out is None else out
    return d


def test_band_rule_and_workspace_sizes_are_host_arithmetic():
    from mspi_amd import _lib
    from mspi_amd import engine as E
    lib = _lib.load()
    assert (E.DWCONV3_WGRAD_RECORDS, E.GATE_SWISH_BWD_ROWS, E.SE_TRAIN_MAX_F, E.X3D_TRAIN_MAX_CH) == (256, 32, 64, 4096)
    # (N, T, H, W, C) -> records: band = max(1, ceil(N T H / 256)) lines, records = ceil(N T H / band)
    for shape, records in (((8, 16, 7, 12, 432), 224), ((2, 16, 7, 12, 432), 224), ((8, 16, 14, 24, 216), 256),
                           ((2, 16, 14, 24, 216), 224), ((1, 1, 1, 1, 4), 1), ((1, 3, 86, 5, 8), 129)):
        N, T, H, W, Cc = shape
        lines = N * T * H
        band = max(1, -(-lines // E.DWCONV3_WGRAD_RECORDS))
        assert -(-lines // band) == records
        d = _dw_desc(N, T, H, W, Cc)
        assert lib.mspi_dwconv3_wgrad_supported(ctypes.byref(d)) == 1
        assert lib.mspi_dwconv3_wgrad_ws_bytes(ctypes.byref(d)) == records * 28 * Cc * 4, shape
    assert lib.mspi_gate_swish_bwd_ws_bytes(2, 70, 72) == 2 * -(-70 // E.GATE_SWISH_BWD_ROWS) * 72 * 4
    assert lib.mspi_gate_swish_bwd_ws_bytes(8, 1344, 432) == 8 * 42 * 432 * 4
    assert lib.mspi_se_train_bwd_ws_bytes(8, 432, 32) == 8 * (432 + 32) * 4
    for bad in ((0, 70, 72), (2, 0, 72), (2, 70, 70), (2, 70, 4100), (65536, 1, 4)):
        assert lib.mspi_gate_swish_bwd_ws_bytes(*bad) == 0, bad
    for bad in ((0, 72, 8), (2, 70, 8), (2, 72, 0), (2, 72, 65), (2, 4100, 8)):
        assert lib.mspi_se_train_bwd_ws_bytes(*bad) == 0, bad


def test_host_refusals():
    from mspi_amd import _lib
    lib = _lib.load()

    def err():
        return lib.mspi_last_error().decode()

    # ---- mspi_dwconv3_wgrad: the descriptor
    for kw, why in ((dict(k=(7, 1, 1), p=(3, 0, 0)), r"kernel must be \(3,3,3\)"), (dict(k=(1, 7, 7), p=(0, 3, 3)), r"kernel must be \(3,3,3\)"),
                    (dict(p=(0, 1, 1)), r"padding \(1,1,1\)"), (dict(s=(1, 2, 2), out=(2, 2, 2)), "stride must be 1"),
                    (dict(C=6), "multiples of 4"), (dict(ldx=4), "ld >= C"), (dict(ldy=10), "multiples of 4"), (dict(C=4100), "4096 channels"),
                    (dict(N=0), "bad extent"), (dict(out=(2, 3, 3)), "output extent"), (dict(N=1 << 14, T=1 << 7, H=1 << 5, W=1 << 5), "2\\^31")):
        d = _dw_desc(**kw)
        assert lib.mspi_dwconv3_wgrad_supported(ctypes.byref(d)) == 0 and re.search("mspi_dwconv3_wgrad: .*" + why, err()), (kw, err())
        assert lib.mspi_dwconv3_wgrad_ws_bytes(ctypes.byref(d)) == 0
        assert lib.mspi_dwconv3_wgrad(ctypes.byref(d), 4096, 8192, 12288, None, 16384, None) == -1
    d = _dw_desc()
    assert lib.mspi_dwconv3_wgrad(ctypes.byref(d), None, 8192, 12288, None, 16384, None) == -1 and "null argument" in err()
    assert lib.mspi_dwconv3_wgrad(ctypes.byref(d), 4096, 8192, 12288, None, None, None) == -1 and "null argument" in err()
    assert lib.mspi_dwconv3_wgrad(ctypes.byref(d), 4100, 8192, 12288, None, 16384, None) == -1 and "16-byte aligned" in err()
    assert lib.mspi_dwconv3_wgrad(None, 4096, 8192, 12288, None, 16384, None) == -1 and "null descriptor" in err()
    # the older entry point still refuses this kernel shape
    assert lib.mspi_dwconv_wgrad_supported(ctypes.byref(d)) == 0

    # ---- mspi_bn_gate_act_fwd
    def bga(x=4096, ldx=8, vec=8192, gate=None, res=None, ldr=0, y=12288, ldy=8, M=6, R=3, C=8, act=_lib.ACT_SWISH):
        return lib.mspi_bn_gate_act_fwd(x, ldx, vec, vec, vec, vec, gate, res, ldr, y, ldy, M, R, C, act, None)
    for kw, why in ((dict(x=None), "null argument"), (dict(y=None), "null argument"), (dict(M=0), "0 < M"), (dict(C=6, ldx=6, ldy=6), "multiple of 4"),
                    (dict(C=4100, ldx=4100, ldy=4100), "C <= 4096"), (dict(R=4), "must divide"), (dict(R=0), "must divide"),
                    (dict(act=_lib.ACT_GELU), "MSPI_ACT_NONE, MSPI_ACT_RELU or MSPI_ACT_SWISH"), (dict(ldx=4), ">= C"), (dict(ldy=10), "multiples of 4"),
                    (dict(res=16384, ldr=4), ">= C"), (dict(x=4100), "16-byte aligned"), (dict(gate=20484), "16-byte aligned")):
        assert bga(**kw) == -1 and re.search("mspi_bn_gate_act_fwd: .*" + why, err()), (kw, err())

    # ---- mspi_gate_swish_bwd
    def gsb(ds=4096, ldds=8, v0=8192, ldv=8, vec=12288, gate=16384, dv=20480, lddv=8, dgate=24576, ws=28672, N=2, R=3, C=8):
        return lib.mspi_gate_swish_bwd(ds, ldds, v0, ldv, vec, vec, vec, vec, gate, dv, lddv, dgate, ws, N, R, C, None)
    for kw, why in ((dict(ds=None), "null argument"), (dict(dv=None), "null argument"), (dict(dgate=None), "with a gate, dgate and ws"),
                    (dict(ws=None), "with a gate, dgate and ws"), (dict(N=0), "0 < N < 65536"), (dict(N=65536), "0 < N < 65536"), (dict(R=0), "no rows"),
                    (dict(N=40000, R=60000), "2\\^31"), (dict(C=6, ldds=6, ldv=6, lddv=6), "multiple of 4"), (dict(ldv=4), ">= C"),
                    (dict(lddv=10), "multiples of 4"), (dict(v0=8200), "16-byte aligned"), (dict(dgate=24580), "16-byte aligned")):
        assert gsb(**kw) == -1 and re.search("mspi_gate_swish_bwd: .*" + why, err()), (kw, err())

    # ---- mspi_se_train_fwd / _bwd
    def sef(p0=4096, N=2, C=8, F=8, **kw):
        a = dict(pool0=p0, mean=8192, rstd=8192, gamma=8192, beta=8192, w1=12288, b1=16384, w2=20480, b2=24576, p=28672, h=32768, gate=36864)
        a.update(kw)
        return lib.mspi_se_train_fwd(*[a[k] for k in ("pool0", "mean", "rstd", "gamma", "beta", "w1", "b1", "w2", "b2", "p", "h", "gate")], N, C, F, None)

    def seb(N=2, C=8, F=8, **kw):
        a = dict(dgate=4096, gate=8192, h=12288, p=16384, w1=20480, w2=24576, dw1=28672, db1=32768, dw2=36864, db2=40960, dp=45056, ws=49152)
        a.update(kw)
        return lib.mspi_se_train_bwd(*[a[k] for k in ("dgate", "gate", "h", "p", "w1", "w2", "dw1", "db1", "dw2", "db2", "dp", "ws")], N, C, F, None)
    for fn, name in ((sef, "mspi_se_train_fwd"), (seb, "mspi_se_train_bwd")):
        for kw, why in ((dict(N=0), "0 < N < 65536"), (dict(C=6), "multiple of 4"), (dict(C=4100), "C <= 4096"), (dict(F=0), "0 < F <= 64"),
                        (dict(F=65), "0 < F <= 64"), (dict(w1=None), "null argument"), (dict(w2=20484), "16-byte aligned")):
            assert fn(**kw) == -1 and re.search(name + ": .*" + why, err()), (name, kw, err())
    assert seb(ws=None) == -1 and "null argument" in err()

    # ---- mspi_relu_mask_add
    def rma(dx=4096, lddx=8, g=8192, ldg=8, y=12288, ldy=8, M=3, C=8):
        return lib.mspi_relu_mask_add(dx, lddx, g, ldg, y, ldy, M, C, None)
    for kw, why in ((dict(dx=None), "null argument"), (dict(y=None), "null argument"), (dict(M=0), "0 < M"), (dict(C=6, lddx=6, ldg=6, ldy=6), "multiple of 4"),
                    (dict(ldg=4), ">= C"), (dict(ldy=10), "multiples of 4"), (dict(g=8196), "16-byte aligned")):
        assert rma(**kw) == -1 and re.search("mspi_relu_mask_add: .*" + why, err()), (kw, err())


def _block_args(case, dev, grad=True, buffers=False):
    """The arguments of autograd.X3DBlock.apply behind x for a restatement case."""
    ts = [torch.from_numpy(case[k]).to(dev).requires_grad_(grad) if k in case else None for k in XR.PARAMS]
    D, Ci = case["x"].shape[-1], case["wa"].shape[0]
    bns = [(torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.long, device=dev)) if buffers else None
           for c in (Ci, Ci, D)]
    return ts, bns


def test_x3d_block_refuses_by_name_without_a_gpu():
    """The refusals that precede the first launch: they need no GPU, so the tensors are on the CPU."""
    from mspi_amd import autograd as A
    from mspi_amd._lib import MspiError
    for D, Ci in ((24, 54), (48, 108)):                       # stages 2 and 3 of X3D-L
        case = XR.make_case(D, Ci, 1, 2, 2, 2, True, 1)
        ts, bns = _block_args(case, "cpu")
        with pytest.raises(MspiError, match=r"X3DBlock: dim_out / dim_inner = %d / %d: dim_out must be a multiple of 32" % (D, Ci)):
            A.X3DBlock.apply(torch.from_numpy(case["x"]), *ts, *bns)
    case = XR.make_case(32, 72, 1, 1, 1, 1, True, 2)
    ts, bns = _block_args(case, "cpu")
    with pytest.raises(MspiError, match=r"X3DBlock: BatchNorm on batch statistics needs more than one row \(B T h w = 1\)"):
        A.X3DBlock.apply(torch.from_numpy(case["x"]), *ts, *bns)
    case = _restated("tiny")[0]
    ts, bns = _block_args(case, "cpu")
    x = torch.from_numpy(case["x"])
    with pytest.raises(MspiError, match="GPU only"):
        A.X3DBlock.apply(x, *ts, *bns)
    i = XR.PARAMS.index("w1")
    with pytest.raises(MspiError, match=r"X3DBlock: se.fc1.weight is \(8, 36, 1, 1, 1\).* has \(8, 72, 1, 1, 1\)"):
        A.X3DBlock.apply(x, *ts[:i], ts[i][:, :36].contiguous(), *ts[i + 1:], *bns)
    with pytest.raises(MspiError, match="se.fc1 / se.fc2 must be given whole"):
        A.X3DBlock.apply(x, *ts[:i], None, *ts[i + 1:], *bns)
    with pytest.raises(MspiError, match=r"X3DBlock: b.weight is \(72, 1, 1, 3, 3\)"):
        A.X3DBlock.apply(x, *ts[:3], ts[3][:, :, :1].contiguous(), *ts[4:], *bns)
    with pytest.raises(MspiError, match=r"X3DBlock: x must be fp32 \[B,T,h,w,dim_out\]"):
        A.X3DBlock.apply(x[0], *ts, *bns)
    with pytest.raises(MspiError, match=r"X3DBlock: x must be fp32 \[B,T,h,w,dim_out\]"):
        A.X3DBlock.apply(x.double(), *ts, *bns)


def _stage(blocks=5):
    """A one-pathway X3D ResStage 32 / 72 wide: block 0 is the head (stride 2, branch1), `se` on the even blocks."""
    from mspi_amd.backbones.blocks3d import ResStage
    return ResStage([32], [32], [2], [[3]], [blocks], [72], [72], [blocks], [[]], trans_func_name="x3d_transform")


def test_resblock_tensors_and_x3d_blocks_refusals_without_a_gpu():
    from mspi_amd import autograd as A
    from mspi_amd._lib import MspiError
    from mspi_amd.backbones.blocks3d import ResStage
    assert len(A.X3D_BLOCK_TENSORS) == len(XR.PARAMS) == 13
    stage = _stage()
    for i, blk in enumerate(stage.blocks(0)):
        t, ts = blk.branch2, blk.tensors()
        assert len(ts) == 16 and hasattr(t, "se") == (i % 2 == 0)
        named = dict(zip(XR.PARAMS, ts))
        assert named["wa"] is t.a.weight and named["ga"] is t.a_bn.weight and named["ba"] is t.a_bn.bias and named["wb"] is t.b.weight
        assert named["gb"] is t.b_bn.weight and named["bb"] is t.b_bn.bias and named["wc"] is t.c.weight
        assert named["gc"] is t.c_bn.weight and named["bc"] is t.c_bn.bias
        if i % 2 == 0:
            assert named["w1"] is t.se.fc1.weight and named["b1"] is t.se.fc1.bias and named["w2"] is t.se.fc2.weight and named["b2"] is t.se.fc2.bias
            assert tuple(named["w1"].shape) == (XR.se_width(72), 72, 1, 1, 1)
        else:
            assert [named[k] for k in XR.SE_PARAMS] == [None] * 4
        for bufs, bn in zip(ts[13:], (t.a_bn, t.b_bn, t.c_bn)):
            assert bufs[0] is bn.running_mean and bufs[1] is bn.running_var and bufs[2] is bn.num_batches_tracked
    x = torch.zeros(1, 2, 4, 4, 32)
    with pytest.raises(MspiError, match="x3d_blocks: pathway0_res0 has branch1"):
        A.x3d_blocks(stage, x, start=0)
    with pytest.raises(MspiError, match="x3d_blocks: blocks 3 .. 6 of a stage of 5"):
        A.x3d_blocks(stage, x, start=3, stop=7)
    with pytest.raises(MspiError, match="GPU only"):
        A.x3d_blocks(stage, x)
    two = ResStage([32, 32], [32, 32], [1, 1], [[3], [3]], [1, 1], [72, 72], [72, 72], [1, 1], [[], []], trans_func_name="x3d_transform")
    with pytest.raises(MspiError, match="x3d_blocks: the stage has 2 pathways"):
        A.x3d_blocks(two, x, start=0)
    plain = ResStage([32], [32], [1], [[3]], [1], [16], [1], [1], [[]])
    with pytest.raises(MspiError, match="ResBlock.tensors: branch2 is a BottleneckTransform"):
        plain.blocks(0)[0].tensors()


# ------------------------------------------------------------------------------------------------------------- GPU: kernels
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cl(t, dev, ld=None, c0=0):
    """[N,T,H,W,C] tensor -> CL on the device; ld > C: the rows sit at channel c0 of a wider buffer filled with NaN elsewhere."""
    from mspi_amd import engine as E
    t = torch.as_tensor(t).float()
    N, T, H, W, Cc = t.shape
    if ld is None:
        return E.CL(t.contiguous().to(dev).view(-1), 0, N, T, H, W, Cc, Cc)
    buf = torch.full((N, T, H, W, ld), float("nan"), device=dev)
    buf[..., c0:c0 + Cc] = t.to(dev)
    return E.CL(buf.view(-1), c0, N, T, H, W, Cc, ld)


def _dw3_case(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=gen)
    dy = torch.randn(*shape, generator=gen)
    return x, dy, XR.dwconv3_wgrad(x.double(), dy.double()), dy.double().reshape(-1, shape[-1]).sum(0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 4), (1, 2, 1, 3, 8), (2, 3, 5, 7, 72), (1, 4, 14, 24, 216), (1, 16, 7, 12, 432), (3, 31, 3, 4, 116)],
                         ids=lambda s: "x".join(map(str, s)))
def test_hip_dwconv3_wgrad_vs_fp64(dev, shape):
    """The last shape has 279 lines: bands of 2 with a short last band, and two channel groups of 15 and 14 quads."""
    from mspi_amd import engine as E
    x, dy, ref, rdb = _dw3_case(shape, 5)
    for bias in (False, True):                                  # db NULL and given
        dW, db = E.dwconv3_wgrad(_cl(x, dev), _cl(dy, dev), bias=bias)
        dW2, db2 = E.dwconv3_wgrad(_cl(x, dev), _cl(dy, dev), bias=bias)
        assert tuple(dW.shape) == (shape[-1], 1, 3, 3, 3) and torch.equal(dW, dW2), "two runs differ"
        e = _err(dW, ref)
        print("dwconv3_wgrad %s bias=%s: dW %.2e" % (shape, bias, e))
        assert e <= GRAD_TOL
        if bias:
            eb = _err(db, rdb)
            print("dwconv3_wgrad %s: db %.2e" % (shape, eb))
            assert eb <= GRAD_TOL and torch.equal(db, db2)
        else:
            assert db is None
    if shape == (1, 1, 1, 1, 4):                                # one position: only the centre tap sees it, the other 26 are exact zeros
        flat = dW.cpu().reshape(4, 27)
        assert (flat[:, 13] != 0).all() and (flat[:, :13] == 0).all() and (flat[:, 14:] == 0).all()


@pytest.mark.gpu
def test_hip_dwconv3_wgrad_reads_channel_slices_of_wider_buffers(dev):
    from mspi_amd import engine as E
    shape = (2, 3, 5, 7, 72)
    x, dy, ref, rdb = _dw3_case(shape, 6)
    dW, db = E.dwconv3_wgrad(_cl(x, dev, ld=96, c0=8), _cl(dy, dev, ld=80, c0=4), bias=True)     # NaN beside the slices
    e, eb = _err(dW, ref), _err(db, rdb)
    print("dwconv3_wgrad slices ld 96 / 80: dW %.2e db %.2e" % (e, eb))
    assert e <= GRAD_TOL and eb <= GRAD_TOL
    dense, _ = E.dwconv3_wgrad(_cl(x, dev), _cl(dy, dev))
    assert torch.equal(dW, dense)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 72), (3, 31, 3, 4, 116)], ids=lambda s: "x".join(map(str, s)))
def test_hip_dwconv3_wgrad_stays_inside_the_workspace_it_asks_for(dev, shape):
    from mspi_amd import _lib
    lib = _lib.load()
    x, dy, ref, rdb = _dw3_case(shape, 7)
    d = _dw_desc(*shape)
    n = lib.mspi_dwconv3_wgrad_ws_bytes(ctypes.byref(d)) // 4
    guard = 1024
    buf = torch.full((n + 2 * guard,), SENTINEL, device=dev)
    xs, dys = x.to(dev), dy.to(dev)
    outs = torch.full((28 * shape[-1] + 2 * guard,), SENTINEL, device=dev)
    dW, db = outs[guard:guard + 27 * shape[-1]], outs[guard + 27 * shape[-1]:guard + 28 * shape[-1]]
    _lib.check(lib.mspi_dwconv3_wgrad(ctypes.byref(d), xs.data_ptr(), dys.data_ptr(), dW.data_ptr(), db.data_ptr(),
                                      buf[guard:].data_ptr(), _stream()), "mspi_dwconv3_wgrad")
    torch.cuda.synchronize()
    assert (buf[:guard] == SENTINEL).all() and (buf[guard + n:] == SENTINEL).all(), "a store outside the workspace"
    assert (outs[:guard] == SENTINEL).all() and (outs[guard + 28 * shape[-1]:] == SENTINEL).all(), "a store outside dW | db"
    assert (buf[guard:guard + n] != SENTINEL).all(), "a record element was left unwritten"
    assert _err(dW.view(shape[-1], 1, 3, 3, 3), ref) <= GRAD_TOL and _err(db, rdb) <= GRAD_TOL


def _bn_case(N, R, C, seed, F=None):
    gen = torch.Generator().manual_seed(seed)
    t = {"x": 2.0 * torch.randn(N, 1, 1, R, C, generator=gen) + 0.5, "res": torch.randn(N, 1, 1, R, C, generator=gen),
         "d": torch.randn(N, 1, 1, R, C, generator=gen), "mean": 0.5 + 0.2 * torch.randn(C, generator=gen),
         "rstd": 0.5 + 0.1 * torch.rand(C, generator=gen), "gamma": 1.0 + 0.3 * torch.randn(C, generator=gen),
         "beta": 0.3 * torch.randn(C, generator=gen), "gate": torch.sigmoid(torch.randn(N, C, generator=gen))}
    return t


def _bga_ref(t, gate, res, act):
    from mspi_amd import engine as E
    x = t["x"].double()
    v = (x - t["mean"].double()) * t["rstd"].double() * t["gamma"].double() + t["beta"].double()
    if gate:
        v = v * t["gate"].double().view(x.shape[0], 1, 1, 1, -1)
    if res:
        v = t["res"].double() + v
    return torch.relu(v) if act == E.ACT_RELU else (v * torch.sigmoid(v) if act == E.ACT_SWISH else v)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [72, 432])
@pytest.mark.parametrize("use", ["gate_swish", "swish", "res_relu", "gate_res_relu", "plain"])
def test_hip_bn_gate_act_vs_fp64(dev, use, C):
    from mspi_amd import engine as E
    gate, res = "gate" in use, "res" in use
    act = E.ACT_SWISH if "swish" in use else (E.ACT_RELU if "relu" in use else E.ACT_NONE)
    t = _bn_case(3, 35, C, 8)
    vec = [t[k].to(dev) for k in ("mean", "rstd", "gamma", "beta")]
    ref = _bga_ref(t, gate, res, act)
    x = _cl(t["x"], dev, ld=C + 8, c0=4)
    y = E.bn_gate_act(x, *vec, gate=t["gate"].to(dev) if gate else None, res=_cl(t["res"], dev) if res else None, act=act)
    e = _err(y.as_nthwc(), ref)
    print("bn_gate_act %s C=%d: %.2e" % (use, C, e))
    assert e <= GRAD_TOL
    out = _cl(torch.zeros_like(t["x"]), dev, ld=C + 4)          # into a slice of a wider buffer; twice the same bits
    E.bn_gate_act(x, *vec, gate=t["gate"].to(dev) if gate else None, res=_cl(t["res"], dev) if res else None, act=act, out=out)
    assert torch.equal(out.as_nthwc(), y.as_nthwc()) and torch.isnan(out.buf.view(-1, C + 4)[:, C:]).all()


def _gsb_ref(t, gate):
    N = t["x"].shape[0]
    v = (t["x"].double() - t["mean"].double()) * t["rstd"].double() * t["gamma"].double() + t["beta"].double()
    g = t["gate"].double().view(N, 1, 1, 1, -1) if gate else torch.ones(1, dtype=torch.float64)
    w = v * g
    sg = torch.sigmoid(w)
    dw = t["d"].double() * sg * (1 + w * (1 - sg))
    return dw * g, (dw * v).reshape(N, -1, v.shape[-1]).sum(1)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [72, 432])
@pytest.mark.parametrize("gate", [True, False], ids=["gate", "nogate"])
def test_hip_gate_swish_bwd_vs_fp64(dev, gate, C):
    """70 rows a sample: two whole 32-row bands and one of 6; 432 channels: two channel groups of 64 and 44 quads."""
    from mspi_amd import engine as E
    t = _bn_case(3, 70, C, 9)
    vec = [t[k].to(dev) for k in ("mean", "rstd", "gamma", "beta")]
    rdv, rdg = _gsb_ref(t, gate)
    runs = [E.gate_swish_bwd(_cl(t["d"], dev, ld=C + 4), _cl(t["x"], dev), *vec, gate=t["gate"].to(dev) if gate else None) for _ in range(2)]
    dv, dgate = runs[0]
    e = _err(dv.as_nthwc(), rdv)
    print("gate_swish_bwd gate=%s C=%d: dv %.2e" % (gate, C, e))
    assert e <= GRAD_TOL and torch.equal(dv.as_nthwc(), runs[1][0].as_nthwc())
    if gate:
        eg = _err(dgate, rdg)
        print("gate_swish_bwd C=%d: dgate %.2e" % (C, eg))
        assert eg <= GRAD_TOL and torch.equal(dgate, runs[1][1])
    else:
        assert dgate is None
    ds = _cl(t["d"], dev)                                        # in place: dv over ds
    dv2, _ = E.gate_swish_bwd(ds, _cl(t["x"], dev), *vec, gate=t["gate"].to(dev) if gate else None, inplace=True)
    assert dv2 is ds and torch.equal(ds.as_nthwc(), dv.as_nthwc())


def _se_case(N, C, seed):
    gen = torch.Generator().manual_seed(seed)
    F = XR.se_width(C)
    t = _bn_case(N, 1, C, seed)
    t.update({"pool0": 0.5 + torch.randn(N, C, generator=gen), "w1": torch.randn(F, C, 1, 1, 1, generator=gen) / C ** 0.5,
              "b1": 0.3 * torch.randn(F, generator=gen), "w2": torch.randn(C, F, 1, 1, 1, generator=gen) / F ** 0.5,
              "b2": 0.3 * torch.randn(C, generator=gen), "dgate": torch.randn(N, C, generator=gen)})
    return t, F


def _se_ref(t, F):
    d = {k: v.double() for k, v in t.items()}
    C = d["pool0"].shape[1]
    W1, W2 = d["w1"].view(F, C), d["w2"].view(C, F)
    p = (d["pool0"] - d["mean"]) * d["rstd"] * d["gamma"] + d["beta"]
    h = torch.relu(p @ W1.t() + d["b1"])
    gate = torch.sigmoid(h @ W2.t() + d["b2"])
    dz2 = d["dgate"] * gate * (1 - gate)
    dh = dz2 @ W2
    dz1 = torch.where(h > 0, dh, torch.zeros_like(dh))
    return {"p": p, "h": h, "gate": gate, "dw1": (dz1.t() @ p).view(F, C, 1, 1, 1), "db1": dz1.sum(0),
            "dw2": (dz2.t() @ h).view(C, F, 1, 1, 1), "db2": dz2.sum(0), "dp": dz1 @ W1}


def _se_run(t, dev):
    from mspi_amd import engine as E
    g = {k: v.to(dev) for k, v in t.items()}
    p, h, gate = E.se_train_fwd(g["pool0"], g["mean"], g["rstd"], g["gamma"], g["beta"], g["w1"], g["b1"], g["w2"], g["b2"])
    dw1, db1, dw2, db2, dp = E.se_train_bwd(g["dgate"], gate, h, p, g["w1"], g["w2"])
    return {"p": p, "h": h, "gate": gate, "dw1": dw1, "db1": db1, "dw2": dw2, "db2": db2, "dp": dp}


@pytest.mark.gpu
@pytest.mark.parametrize("C", [72, 432])
@pytest.mark.parametrize("N", [1, 2, 8])
def test_hip_se_train_fwd_and_bwd_vs_fp64(dev, N, C):
    t, F = _se_case(N, C, 10 + N)
    ref = _se_ref(t, F)
    if N == 8:
        assert (ref["h"] > 0).any() and (ref["h"] == 0).any()      # both sides of the ReLU's mask
    got, again = _se_run(t, dev), _se_run(t, dev)
    for k in ref:
        e = _err(got[k], ref[k])
        print("se_train N=%d C=%d F=%d: %s %.2e" % (N, C, F, k, e))
        assert e <= GRAD_TOL, k
        assert torch.equal(got[k], again[k]), k


@pytest.mark.gpu
def test_hip_relu_mask_add_takes_zero_and_negative_outputs_as_masked(dev):
    from mspi_amd import engine as E
    gen = torch.Generator().manual_seed(11)
    shape = (2, 1, 3, 37, 72)
    dx, g, y = (torch.randn(*shape, generator=gen) for _ in range(3))
    y[0, 0, 0, :5] = 0.0                                          # exactly zero: masked, like the negative ones
    y[1, 0, 2, 3:9] = -0.0
    y = torch.where(y.abs() < 0.2, torch.zeros_like(y), y)
    assert (y == 0).sum() > 100 and (y < 0).sum() > 100 and (y > 0).sum() > 100
    ref = dx.double() + torch.where(y > 0, g, torch.zeros_like(g)).double()
    acc = _cl(dx, dev, ld=80, c0=4)
    out = E.relu_mask_add(acc, _cl(g, dev, ld=76), _cl(y, dev))
    e = _err(out.as_nthwc(), ref)
    print("relu_mask_add: %.2e" % e)
    assert out is acc and e <= 1e-7
    masked = (y <= 0)
    assert torch.equal(out.as_nthwc().cpu()[masked], dx[masked])  # masked cells keep their bits


@pytest.mark.gpu
def test_hip_engine_wrappers_refuse_by_name(dev):
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    t = _bn_case(2, 6, 8, 12)
    vec = [t[k].to(dev) for k in ("mean", "rstd", "gamma", "beta")]
    x, d = _cl(t["x"], dev), _cl(t["d"], dev)
    with pytest.raises(MspiError, match="GPU only"):
        E.dwconv3_wgrad(_cl(t["x"], "cpu"), _cl(t["d"], "cpu"))
    with pytest.raises(MspiError, match=r"dwconv3_wgrad: dy \[2,1,1,3,8\] must match \[2,1,1,6,8\]"):
        E.dwconv3_wgrad(x, _cl(t["d"][:, :, :, :3], dev))
    with pytest.raises(MspiError, match="bn_gate_act: act must be ACT_NONE, ACT_RELU or ACT_SWISH"):
        E.bn_gate_act(x, *vec, act=E.ACT_GELU)
    with pytest.raises(MspiError, match="bn_gate_act: gamma must be a contiguous fp32"):
        E.bn_gate_act(x, vec[0], vec[1], vec[2][:4], vec[3])
    with pytest.raises(MspiError, match="bn_gate_act: gate must be a contiguous fp32 tensor of 2 x 8"):
        E.bn_gate_act(x, *vec, gate=t["gate"][:1].to(dev))
    with pytest.raises(MspiError, match=r"bn_gate_act: res \[2,1,1,3,8\] must match"):
        E.bn_gate_act(x, *vec, res=_cl(t["res"][:, :, :, :3], dev))
    with pytest.raises(MspiError, match=r"gate_swish_bwd: ds \[2,1,1,3,8\] must match"):
        E.gate_swish_bwd(_cl(t["d"][:, :, :, :3], dev), x, *vec)
    with pytest.raises(MspiError, match="gate_swish_bwd: gate must be a contiguous fp32 tensor of 2 x 8"):
        E.gate_swish_bwd(d, x, *vec, gate=t["gate"].to(dev).t())
    s, F = _se_case(2, 8, 13)
    g = {k: v.to(dev) for k, v in s.items()}
    with pytest.raises(MspiError, match="se_train_fwd: fc1.weight must be a contiguous fp32 tensor of 8 x 8"):
        E.se_train_fwd(g["pool0"], g["mean"], g["rstd"], g["gamma"], g["beta"], g["w1"][:4], g["b1"], g["w2"], g["b2"])
    with pytest.raises(MspiError, match=r"se_train_fwd: N=2 C=8 F=65"):
        E.se_train_fwd(g["pool0"], g["mean"], g["rstd"], g["gamma"], g["beta"], g["w1"], torch.zeros(65, device=dev), g["w2"], g["b2"])
    with pytest.raises(MspiError, match="se_train_bwd: h must be a contiguous fp32 tensor of 2 x 8"):
        E.se_train_bwd(g["dgate"], g["gate"], torch.zeros(3, 8, device=dev), g["pool0"], g["w1"], g["w2"])
    with pytest.raises(MspiError, match="relu_mask_add: g must be dense rows"):
        E.relu_mask_add(x, _cl(t["d"][:, :, :, :3], dev), x)


# ------------------------------------------------------------------------------------------------------------- GPU: the Function
def _block(case, dev, grad_x=True, only=None, buffers=False, G=None):
    """(y, {name: gradient}, buffer triples) of autograd.X3DBlock on a restatement case; only: the names that require grad."""
    from mspi_amd import autograd as A
    ts, bns = _block_args(case, dev, grad=False, buffers=buffers)
    names = ("x",) + XR.PARAMS
    x = torch.from_numpy(case["x"]).to(dev)
    leaves = dict(zip(names, [x] + ts))
    ask = [k for k in names if leaves[k] is not None and (k in only if only is not None else (grad_x or k != "x"))]
    for k in ask:
        leaves[k].requires_grad_(True)
    y = A.X3DBlock.apply(x, *ts, *bns)
    G = torch.from_numpy(case["G"]).to(dev) if G is None else G
    gs = torch.autograd.grad(y, [leaves[k] for k in ask], G, allow_unused=True)
    return y.detach(), dict(zip(ask, gs)), bns


@pytest.mark.gpu
@pytest.mark.parametrize("key", BLOCK_CASES)
def test_hip_x3d_block_vs_the_restatement(dev, key):
    from mspi_amd import engine as E
    E.autotune(False)
    case, fwd, ref = _restated(key)
    y, got, _ = _block(case, dev)
    assert sorted(got) == sorted(ref)
    errs = {"y": _err(y, fwd["y"])}
    errs.update({k: _err(got[k], ref[k]) for k in ref})
    for k, e in errs.items():
        print("X3DBlock %-6s %-2s: %.2e of max|ref| = %.2e" % (key, k, e, float((fwd["y"] if k == "y" else ref[k]).abs().max())))
    for k, e in errs.items():
        assert e <= GRAD_TOL, (key, k, e)


@pytest.mark.gpu
def test_hip_x3d_block_tiny_vs_the_stored_torch_gradients(dev):
    case = _restated("tiny")[0]
    g = _gold()
    y, got, _ = _block(case, dev)
    assert _err(y, g["tiny.y"]) <= GRAD_TOL
    for k in XR.GRADS:
        e = _err(got[k], g["tiny." + k])
        print("X3DBlock tiny %-2s vs torch float64: %.2e" % (k, e))
        assert e <= GRAD_TOL, k


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["odd_se", "s5"])
def test_hip_x3d_block_running_statistics_like_batchnorm3d_train(dev, key):
    """Two forwards on the same input: running_mean, running_var (unbiased, momentum 0.1) and num_batches_tracked against
    upstream's layers in float64."""
    from mspi_amd import autograd as A
    case = _restated(key)[0]
    m, _ = XR.upstream_block(case)
    xt = torch.from_numpy(case["x"]).double().permute(0, 4, 1, 2, 3)
    ts, bns = _block_args(case, dev, grad=False, buffers=True)
    x = torch.from_numpy(case["x"]).to(dev)
    for _ in range(2):
        with torch.no_grad():
            m(xt)
        A.X3DBlock.apply(x, *ts, *bns)
    for name, bufs, bn in zip("abc", bns, (m.a_bn, m.b_bn, m.c_bn)):
        em, ev = _err(bufs[0], bn.running_mean), _err(bufs[1], bn.running_var)
        print("X3DBlock %s bn_%s: running_mean %.2e running_var %.2e" % (key, name, em, ev))
        assert em <= GRAD_TOL and ev <= GRAD_TOL
        assert int(bufs[2]) == int(bn.num_batches_tracked) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["odd_se", "odd"])
def test_hip_x3d_block_is_repeatable_and_skips_what_is_not_asked(dev, key):
    case = _restated(key)[0]
    y1, g1, _ = _block(case, dev)
    y2, g2, _ = _block(case, dev)
    assert torch.equal(y1, y2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), "two backward passes differ in %s" % k
    for only in (("wc", "gc"), ("w1", "b2") if case["se"] else ("gb",), ("wb", "bb"), ("wa",), ("x",), ("ga", "bc")):
        _, part, _ = _block(case, dev, only=only)
        assert sorted(part) == sorted(only)
        for k in only:
            assert part[k] is not None and torch.equal(part[k], g1[k]), "asked alone, %s has other bits" % k


@pytest.mark.gpu
def test_hip_x3d_block_has_no_double_backward(dev):
    from mspi_amd import autograd as A
    case = _restated("tiny")[0]
    ts, bns = _block_args(case, dev)
    leaf = torch.from_numpy(case["x"]).to(dev).requires_grad_(True)
    gx, = torch.autograd.grad(A.X3DBlock.apply(leaf, *ts, *bns).sum(), leaf, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gx.sum(), leaf)


@pytest.mark.gpu
def test_hip_x3d_blocks_chains_three_blocks(dev):
    """Blocks 2, 3, 4 of a five-block stage (se, no se, se) against three chained restatements."""
    from mspi_amd import autograd as A
    cases = [dict(_restated("chain%d" % i)[0]) for i in range(3)]
    fwds = []
    for i, c in enumerate(cases):                               # block i reads block i - 1's float64 output
        if i:
            c["x"] = fwds[-1]["y"].numpy()
        fwds.append(XR.forward(c))
    refs, G = [None] * 3, cases[2]["G"]
    for i in (2, 1, 0):
        cases[i]["G"] = G
        refs[i] = XR.backward(cases[i], fwds[i])
        G = refs[i]["x"].numpy()
    stage = _stage(5).to(dev)
    for blk, c in zip(stage.blocks(0)[2:], cases):
        for k, p in zip(XR.PARAMS, blk.tensors()[:13]):
            assert (p is None) == (k not in c)
            if p is not None:
                with torch.no_grad():
                    p.copy_(torch.from_numpy(c[k]))
    x = torch.from_numpy(cases[0]["x"]).to(dev).requires_grad_(True)
    y = A.x3d_blocks(stage, x, start=2)
    params = [(i, k, p) for i, blk in enumerate(stage.blocks(0)[2:]) for k, p in zip(XR.PARAMS, blk.tensors()[:13]) if p is not None]
    gs = torch.autograd.grad(y, [x] + [p for _, _, p in params], torch.from_numpy(cases[2]["G"]).float().to(dev))
    errs = {"y": _err(y, fwds[2]["y"]), "x": _err(gs[0], refs[0]["x"])}
    errs.update({"block%d.%s" % (i, k): _err(g, refs[i][k]) for (i, k, _), g in zip(params, gs[1:])})
    for k, e in errs.items():
        print("x3d_blocks %-10s: %.2e" % (k, e))
    assert len(params) == 13 + 9 + 13
    for k, e in errs.items():
        assert e <= GRAD_TOL, (k, e)
    for blk in stage.blocks(0)[2:]:                             # train(): every BatchNorm of the three blocks has seen one batch
        assert all(int(b[2]) == 1 for b in blk.tensors()[13:])
    assert all(int(b[2]) == 0 for b in stage.blocks(0)[1].tensors()[13:])


# ------------------------------------------------------------------------------------------------------------- GPU: the ledgers
def _nan_at(t, idx):
    t = t.clone()
    t[idx] = float("nan")
    return t


@pytest.mark.gpu
def test_hip_ledger_nonfinite_operands_propagate(dev):
    """One case per entry point: a NaN in x or dy, the float64 reference computed from the poisoned operand."""
    from mspi_amd import engine as E
    shape = (2, 3, 5, 7, 72)
    x, dy, _, _ = _dw3_case(shape, 21)
    for name, idx in (("x", (1, 1, 2, 3, 9)), ("dy", (0, 2, 4, 6, 70))):
        ops = {"x": x, "dy": dy}
        ops[name] = _nan_at(ops[name], idx)
        dW, db = E.dwconv3_wgrad(_cl(ops["x"], dev), _cl(ops["dy"], dev), bias=True)
        _judge("dwconv3_wgrad %s -> dW" % name, dW, XR.dwconv3_wgrad(ops["x"].double(), ops["dy"].double()))
        if name == "dy":
            _judge("dwconv3_wgrad dy -> db", db, ops["dy"].double().reshape(-1, 72).sum(0))
    t = _bn_case(3, 70, 72, 22)
    vec = [t[k].to(dev) for k in ("mean", "rstd", "gamma", "beta")]
    bad = dict(t, x=_nan_at(t["x"], (1, 0, 0, 40, 5)))
    y = E.bn_gate_act(_cl(bad["x"], dev), *vec, gate=t["gate"].to(dev), res=_cl(t["res"], dev), act=E.ACT_RELU)
    _judge("bn_gate_act x -> y (ReLU)", y.as_nthwc(), _bga_ref(bad, True, True, E.ACT_RELU))
    bad = dict(t, d=_nan_at(t["d"], (2, 0, 0, 69, 71)))
    dv, dgate = E.gate_swish_bwd(_cl(bad["d"], dev), _cl(t["x"], dev), *vec, gate=t["gate"].to(dev))
    rdv, rdg = _gsb_ref(bad, True)
    _judge("gate_swish_bwd ds -> dv", dv.as_nthwc(), rdv)
    _judge("gate_swish_bwd ds -> dgate", dgate, rdg)
    s, F = _se_case(3, 72, 23)
    bad = dict(s, pool0=_nan_at(s["pool0"], (1, 17)))
    got, ref = _se_run(bad, dev), _se_ref(bad, F)
    for k in ("p", "h", "gate"):
        _judge("se_train_fwd pool0 -> %s" % k, got[k], ref[k])
    bad = dict(s, dgate=_nan_at(s["dgate"], (2, 30)))
    got, ref = _se_run(bad, dev), _se_ref(bad, F)
    for k in ("dw1", "db1", "dw2", "db2", "dp"):
        _judge("se_train_bwd dgate -> %s" % k, got[k], ref[k])
    gen = torch.Generator().manual_seed(24)
    dx, g, yy = (torch.randn(2, 1, 3, 37, 72, generator=gen) for _ in range(3))
    yy[1, 0, 1, 5, 7] = 1.0
    g = _nan_at(g, (1, 0, 1, 5, 7))
    out = E.relu_mask_add(_cl(dx, dev), _cl(g, dev), _cl(yy, dev))
    _judge("relu_mask_add g -> dx", out.as_nthwc(), dx.double() + torch.where(yy > 0, g, torch.zeros_like(g)).double())


@pytest.mark.gpu
def test_hip_ledger_capture_and_replay(dev):
    """One case per entry point, on the C ABI: eager on one operand set, captured with another, replayed on the first."""
    from mspi_amd import _lib
    lib = _lib.load()
    shape = (2, 3, 5, 7, 72)
    N, T, H, W, C = shape

    def dw_ops(seed):
        x, dy, _, _ = _dw3_case(shape, seed)
        return {"x": x, "dy": dy}

    def dw(t, host):
        d = _dw_desc(*shape)
        host.append(d)                                            # the descriptor: read during the call only
        dW, db = torch.empty(C, 27, device=dev), torch.empty(C, device=dev)
        ws = torch.empty(lib.mspi_dwconv3_wgrad_ws_bytes(ctypes.byref(d)) // 4, device=dev)
        _lib.check(lib.mspi_dwconv3_wgrad(ctypes.byref(d), t["x"].data_ptr(), t["dy"].data_ptr(), dW.data_ptr(), db.data_ptr(),
                                          ws.data_ptr(), _stream()), "mspi_dwconv3_wgrad")
        return {"dW": dW, "db": db}
    _replayed(dev, {"A": dw_ops(31), "B": dw_ops(32)}, dw)

    R, M = 70, 3 * 70
    keys = ("x", "res", "d", "mean", "rstd", "gamma", "beta", "gate")

    def bn_ops(seed):
        t = _bn_case(3, R, C, seed)
        return {k: t[k].contiguous() for k in keys}

    def bga(t, host):
        y = torch.empty(M, C, device=dev)
        _lib.check(lib.mspi_bn_gate_act_fwd(t["x"].data_ptr(), C, t["mean"].data_ptr(), t["rstd"].data_ptr(), t["gamma"].data_ptr(),
                                            t["beta"].data_ptr(), t["gate"].data_ptr(), t["res"].data_ptr(), C, y.data_ptr(), C, M, R, C,
                                            _lib.ACT_SWISH, _stream()), "mspi_bn_gate_act_fwd")
        return {"y": y}
    _replayed(dev, {"A": bn_ops(33), "B": bn_ops(34)}, bga)

    def gsb(t, host):
        dv, dgate = torch.empty(M, C, device=dev), torch.empty(3, C, device=dev)
        ws = torch.empty(lib.mspi_gate_swish_bwd_ws_bytes(3, R, C) // 4, device=dev)
        _lib.check(lib.mspi_gate_swish_bwd(t["d"].data_ptr(), C, t["x"].data_ptr(), C, t["mean"].data_ptr(), t["rstd"].data_ptr(),
                                           t["gamma"].data_ptr(), t["beta"].data_ptr(), t["gate"].data_ptr(), dv.data_ptr(), C,
                                           dgate.data_ptr(), ws.data_ptr(), 3, R, C, _stream()), "mspi_gate_swish_bwd")
        return {"dv": dv, "dgate": dgate}
    _replayed(dev, {"A": bn_ops(35), "B": bn_ops(36)}, gsb)

    F = XR.se_width(C)
    se_keys = ("pool0", "mean", "rstd", "gamma", "beta", "w1", "b1", "w2", "b2", "dgate")

    def se_ops(seed):
        s, _ = _se_case(3, C, seed)
        return {k: s[k].contiguous() for k in se_keys}

    def se(t, host):
        p, gate, dp = (torch.empty(3, C, device=dev) for _ in range(3))
        h = torch.empty(3, F, device=dev)
        _lib.check(lib.mspi_se_train_fwd(*[t[k].data_ptr() for k in se_keys[:9]], p.data_ptr(), h.data_ptr(), gate.data_ptr(), 3, C, F,
                                         _stream()), "mspi_se_train_fwd")
        dw1, dw2, db1, db2 = torch.empty(F, C, device=dev), torch.empty(C, F, device=dev), torch.empty(F, device=dev), torch.empty(C, device=dev)
        ws = torch.empty(lib.mspi_se_train_bwd_ws_bytes(3, C, F) // 4, device=dev)
        _lib.check(lib.mspi_se_train_bwd(t["dgate"].data_ptr(), gate.data_ptr(), h.data_ptr(), p.data_ptr(), t["w1"].data_ptr(),
                                         t["w2"].data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), dp.data_ptr(),
                                         ws.data_ptr(), 3, C, F, _stream()), "mspi_se_train_bwd")
        return {"p": p, "h": h, "gate": gate, "dw1": dw1, "db1": db1, "dw2": dw2, "db2": db2, "dp": dp}
    _replayed(dev, {"A": se_ops(37), "B": se_ops(38)}, se)

    def rma(t, host):
        dx = t["x"].clone()
        _lib.check(lib.mspi_relu_mask_add(dx.data_ptr(), C, t["d"].data_ptr(), C, t["res"].data_ptr(), C, M, C, _stream()),
                   "mspi_relu_mask_add")
        return {"dx": dx}
    _replayed(dev, {"A": bn_ops(39), "B": bn_ops(40)}, rma)
