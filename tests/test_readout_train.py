"""The trainable readout: csrc/readout_train.hip (wide weight gradient, BatchNorm on batch statistics), engine.conv_wgrad_wide /
bn_stats / bn_apply / bn_bwd, autograd.ReadoutHead, _SaliencyBase.trainable("readout"), mspi_amd.train --trainable readout.

Yardsticks: tests/golden/readout.npz holds "tiny" (pyramid base (B, a, b) = (1, 1, 2), decoder width 32) with the float64 value
and the 16 gradients torch autograd gives through torch.nn layers with upstream's arguments, BatchNorm in .train() mode
(tools/gen_readout_golden.py), and the seed of "odd" ((2, 2, 3)); tests/readout_restate.py is the float64 restatement in
this project's order with its analytic backward, pinned to that fixture and, here, to torch autograd on "odd".

Bounds.  Every gradient tensor: max |got - ref| / max |ref| <= GRAD_TOL = 2e-5, the project's bar for gradients; torch fp32 on
the CPU sits at 1e-6 .. 4e-6 on these inputs.  The gradients of readout[1].bias, readout[4].bias (a BatchNorm on batch
statistics ignores a shift of its input) and readout[12].bias (so does the log-softmax) are zero in exact arithmetic: they are
computed like any other bias gradient and checked as |db| <= 2e-5 * sum|g| over the gradient tensor they are the sum of,
never against their own size.  bn_stats: variance within 2e-5 relative and mean within 2e-5 * max(1, |mean|) of float64 on
means spread over +-1000 with deviations 0.1 .. 10, where a one-pass E[x^2] - E[x]^2 in fp32 is off by 10 to 100 times that.
Adjoint identities: 1e-5 relative, the sums accumulated in float64 on the host.

ReLU kinks.  Kernel-level tests feed the backward entry points the restatement's own activations cast to fp32, so the masks
agree by construction.  End to end only kink-free inputs are compared ("tiny", whose seed was searched for that, and width 192
on (1, 1, 2) with seed 0)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import readout_restate as R
import readout_tail_restate as RT
from test_parity_gpu import MAP_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_conv_wgrad_wide_supported", "mspi_conv_wgrad_wide_variant", "mspi_conv_wgrad_wide_ws_bytes",
               "mspi_conv_wgrad_wide_fwd", "mspi_bn_ws_bytes", "mspi_bn_stats", "mspi_bn_apply", "mspi_bn_bwd")
CASES = ("tiny", "odd")
SHAPES = {"tiny": (1, 1, 2), "odd": (2, 2, 3)}
GRAD_TOL = 2e-5
ZERO_BIASES = ("b1", "b4", "b12")

# the split constants of csrc/readout_train.hip
BOX = 128              # WW_ROWS: output rows per staged box (a 1x1x1 kernel over dense rows: 128 consecutive rows)
BPS, BPS_BIG = 4, 32   # WW_BPS_SMALL / WW_BPS_BIG: boxes per slice
BIG_BOXES = 512        # WW_BIG_BOXES: boxes from which the long slice is taken
BN_ROWS = 512          # rows per workgroup record of the BatchNorm kernels
# rows of a 1x1x1 layer one below, at and one above: a box, a short slice, the last row count with short slices, the first
# with long ones, and a whole number of long slices
WIDE_BOUNDARY = (BOX - 1, BOX, BOX + 1, BPS * BOX - 1, BPS * BOX, BPS * BOX + 1, (BIG_BOXES - 1) * BOX - 1, (BIG_BOXES - 1) * BOX,
                 (BIG_BOXES - 1) * BOX + 1, BIG_BOXES * BOX - 1, BIG_BOXES * BOX, BIG_BOXES * BOX + 1)


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "readout.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _restated(key, D=32):
    """(case, saved, grads) in float64, computed once: a fixture case by name, or a seeded (B, a, b) shape at width D."""
    g = _gold()
    if key == "tiny" and D == 32:
        case = {k: g["tiny_%s" % k] for k in R.MAPS + R.PARAMS + ("g",)}
    elif isinstance(key, str):
        case = R.make_case(*SHAPES[key], seed=int(g["%s_seed" % key]) if D == 32 else 0, D=D)
    else:
        case = R.make_case(*key, seed=0, D=D)
    saved = R.forward(case)
    return case, saved, R.backward(case, saved, case["g"])


def _err(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / ref.abs().max()).item()


def _gsum(t):
    return torch.as_tensor(t).double().abs().sum().item()


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["cases"]) == CASES
    for c in CASES:
        assert tuple(g["%s_shape" % c]) == SHAPES[c]
    B, a, b = SHAPES["tiny"]
    shapes = R.param_shapes(32)
    for j in range(4):
        assert g["tiny_s%d" % j].shape == (B, 32, 4, (8 >> j) * a, (8 >> j) * b) and g["tiny_s%d" % j].dtype == np.float32
    for k in R.PARAMS:
        assert g["tiny_%s" % k].shape == shapes[k] and g["tiny_%s" % k].dtype == np.float32
        assert g["tiny_d_%s" % k].shape == shapes[k] and g["tiny_d_%s" % k].dtype == np.float64
    assert g["tiny_g"].shape == (B, 32 * a, 32 * b) and g["tiny_out"].shape == (B, 32 * a, 32 * b) and g["tiny_out"].dtype == np.float64
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "readout.npz")) < (1 << 20)


def _assert_pinned(grads, ref, case, what):
    for k in R.PARAMS:
        if k in ZERO_BIASES:
            assert (grads[k] - torch.as_tensor(ref[k])).abs().max().item() <= 1e-12 * _gsum(case["g"]), (what, k)
        else:
            assert _err(grads[k], ref[k]) <= 1e-12, (what, k)


def test_restatement_matches_the_fixture():
    g = _gold()
    case, saved, grads = _restated("tiny")
    assert (saved["out"] - torch.from_numpy(g["tiny_out"])).abs().max().item() <= 1e-12
    _assert_pinned(grads, {k: g["tiny_d_%s" % k] for k in R.PARAMS}, case, "tiny")


def test_restatement_matches_torch_autograd_on_odd():
    """ "odd" is stored as its seed: torch.nn layers with upstream's arguments, .train() BatchNorm, float64, built here."""
    case, saved, grads = _restated("odd")
    out, ref, seq = R.upstream_grads(case)
    assert (saved["out"] - out).abs().max().item() <= 1e-12
    _assert_pinned(grads, ref, case, "odd")
    M = case["s0"].size // case["s0"].shape[1]
    for i, key in ((2, "bn2"), (5, "bn5")):
        rm, rv = R.running_stats(saved["head"][key], M)
        assert _err(rm, seq[i].running_mean) <= 1e-12 and _err(rv, seq[i].running_var) <= 1e-12
        assert int(seq[i].num_batches_tracked) == 1


def test_new_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mspi_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name) and getattr(lib, name).argtypes is not None, name
    from mspi_amd import engine as E
    for name in ("conv_wgrad_wide", "conv_wgrad_wide_variant", "bn_stats", "bn_apply", "bn_bwd"):
        assert callable(getattr(E, name)) and name in E.__all__
    assert (E.WGRAD_WIDE_BOX_ROWS, E.WGRAD_WIDE_SLICES, E.WGRAD_WIDE_BIG_BOXES, E.BN_ROWS) == (BOX, (BPS, BPS_BIG), BIG_BOXES, BN_ROWS)
    src = open(os.path.join(ROOT, "mspi_amd", "csrc", "readout_train.hip")).read()
    assert "atomic" not in src.lower().replace("no float atomics", "")


def _desc(N, T, H, W, Cin, Cout, k, pad, stride=(1, 1, 1), ld=None):
    from mspi_amd._lib import ConvDesc
    ld = Cin if ld is None else ld
    d = ConvDesc()
    d.N, d.T, d.H, d.W, d.C = N, T, H, W, Cin
    d.sN, d.sT, d.sH, d.sW, d.sC = T * H * W * ld, H * W * ld, W * ld, ld, 1
    d.kT, d.kH, d.kW = k
    d.strT, d.strH, d.strW = stride
    d.padT, d.padH, d.padW = pad
    d.To, d.Ho, d.Wo = [(n + 2 * p - kk) // s + 1 for n, p, kk, s in zip((T, H, W), pad, k, stride)]
    d.Cout, d.ldy = Cout, Cout
    return d


def _wide_host(d, x=4096, dy=8192):
    from mspi_amd import _lib
    lib = _lib.load()
    return (lib.mspi_conv_wgrad_wide_supported(ctypes.byref(d)), lib.mspi_conv_wgrad_wide_variant(ctypes.byref(d), x, dy),
            lib.mspi_conv_wgrad_wide_ws_bytes(ctypes.byref(d)), lib.mspi_last_error().decode())


def _record(Cout, taps, Cin):
    return 4 * (Cout * taps * Cin + Cout)


def test_wide_wgrad_host_arithmetic():
    # the three production layers at 8 clips of 224 x 384: maps [8, 4, 56, 96]; boxes of 4 x 4 x 8 positions, 1 x 14 x 12 per
    # clip = 1344 boxes >= BIG_BOXES, so 42 slices of 32; the 1x1x1 layer takes its 172032 dense rows as 1344 boxes of 128
    for Cin, Cout, k, pad in ((192, 192, (3, 3, 3), (1, 1, 1)), (192, 64, (1, 3, 3), (0, 1, 1)), (192, 192, (1, 1, 1), (0, 0, 0))):
        taps = k[0] * k[1] * k[2]
        assert _wide_host(_desc(8, 4, 56, 96, Cin, Cout, k, pad))[:3] == (1, BPS_BIG, 42 * _record(Cout, taps, Cin)), (Cin, Cout, k)
    # at cfg.TRAIN.BATCH_SIZE-like one clip: 168 boxes, short slices
    assert _wide_host(_desc(1, 4, 56, 96, 192, 192, (3, 3, 3), (1, 1, 1)))[:3] == (1, BPS, 42 * _record(192, 27, 192))
    # both sides of every slice constant, on the 1x1x1 layer (rows = boxes of 128)
    for M in WIDE_BOUNDARY:
        boxes = (M + BOX - 1) // BOX
        bps = BPS_BIG if boxes >= BIG_BOXES else BPS
        assert _wide_host(_desc(1, 1, 1, M, 32, 32, (1, 1, 1), (0, 0, 0)))[:3] == (1, bps, (boxes + bps - 1) // bps * _record(32, 1, 32)), M
    # a 1x1x1 layer takes its rows as one line while they are evenly spaced (ld > C included): 3 x 4 x 4 x 9 = 432 rows, 4 boxes,
    # one slice; with a gap between the samples it keeps its geometry, 2 boxes of 4 x 4 x 8 positions per sample, 6 boxes, two slices
    d = _desc(3, 4, 4, 9, 32, 32, (1, 1, 1), (0, 0, 0), ld=64)
    assert _wide_host(d)[:3] == (1, BPS, _record(32, 1, 32))
    d.sN *= 2
    assert _wide_host(d)[:3] == (1, BPS, 2 * _record(32, 1, 32))
    # refusals, each with its reason
    for d, why in ((_desc(1, 4, 8, 16, 36, 32, (1, 3, 3), (0, 1, 1)), "Cin must be a multiple of 32"),
                   (_desc(1, 4, 8, 16, 32, 200, (1, 3, 3), (0, 1, 1)), "Cout must be a multiple of 32, at most 192"),
                   (_desc(1, 4, 8, 16, 224, 32, (1, 3, 3), (0, 1, 1)), "Cin must be a multiple of 32, at most 192"),
                   (_desc(1, 4, 8, 16, 32, 32, (1, 3, 3), (0, 1, 1), stride=(1, 2, 2)), "stride must be 1"),
                   (_desc(1, 4, 8, 16, 32, 32, (4, 3, 3), (0, 1, 1)), "more than 27 taps")):
        ok, variant, ws, msg = _wide_host(d)
        assert (ok, variant, ws) == (0, -1, 0) and why in msg and msg.startswith("mspi_conv_wgrad_wide"), msg
    good = _desc(1, 4, 8, 16, 32, 32, (1, 3, 3), (0, 1, 1))
    for x, dy in ((4096 + 4, 8192), (4096, 8192 + 8)):
        ok, variant, ws, msg = _wide_host(good, x, dy)
        assert ok == 1 and variant == -1 and ws > 0 and "16-byte aligned" in msg
    # the narrow entry points keep their answers
    from mspi_amd import _lib
    lib = _lib.load()
    assert lib.mspi_conv_wgrad_supported(ctypes.byref(_desc(1, 4, 8, 16, 192, 192, (3, 3, 3), (1, 1, 1)))) == 0
    assert lib.mspi_conv_wgrad_supported(ctypes.byref(_desc(1, 1, 8, 16, 32, 32, (1, 3, 3), (0, 1, 1)))) == 1


def test_bn_argument_checks():
    from mspi_amd import _lib
    lib = _lib.load()
    p = 4096                                                    # never dereferenced: every call below is refused on the host
    assert lib.mspi_bn_ws_bytes(1, 64) == 0 and lib.mspi_bn_ws_bytes(2, 64) == 2 * 64 * 4
    assert lib.mspi_bn_ws_bytes(BN_ROWS, 192) == 2 * 192 * 4 and lib.mspi_bn_ws_bytes(BN_ROWS + 1, 192) == 2 * 2 * 192 * 4
    assert lib.mspi_bn_ws_bytes(8, 6) == 0 and lib.mspi_bn_ws_bytes(8, 196) == 0 and lib.mspi_bn_ws_bytes(0, 64) == 0

    def stats(M, Cc, x=p, ld=None, eps=1e-5):
        rc = lib.mspi_bn_stats(x, Cc if ld is None else ld, M, Cc, eps, p, p, p, p, None)
        return rc, lib.mspi_last_error().decode()
    for args, why in (((1, 64), "M = 1"), ((0, 64), "no rows"), ((8, 6), "multiple of 4"), ((8, 196), "at most 192"),
                      ((8, 64, p + 4), "16-byte aligned"), ((8, 64, p, 62), "multiple of 4"), ((8, 64, p, 60), ">= C"),
                      ((8, 64, p, None, -1.0), "negative eps")):
        rc, msg = stats(*args)
        assert rc != 0 and why in msg and msg.startswith("mspi_bn_stats"), (args, msg)
    rc = lib.mspi_bn_apply(p, 64, p, p, p, p, p, 64, 1, 64, 0, None)
    assert rc != 0 and "M = 1" in lib.mspi_last_error().decode()
    rc = lib.mspi_bn_apply(p, 64, p, p, p, p, p, 64, 8, 64, 2, None)            # MSPI_ACT_GELU
    assert rc != 0 and "act must be" in lib.mspi_last_error().decode()
    rc = lib.mspi_bn_apply(p, 64, p, p + 8, p, p, p, 64, 8, 64, 0, None)
    assert rc != 0 and "16-byte aligned" in lib.mspi_last_error().decode()
    rc = lib.mspi_bn_bwd(p, 64, p, 64, None, 0, p, p, p, p, 64, p, p, p, 1, 64, None)
    assert rc != 0 and "M = 1" in lib.mspi_last_error().decode()
    rc = lib.mspi_bn_bwd(p, 64, p, 64, p + 4, 64, p, p, p, p, 64, p, p, p, 8, 64, None)
    assert rc != 0 and "16-byte aligned" in lib.mspi_last_error().decode()
    rc = lib.mspi_bn_bwd(p, 64, p, 64, None, 0, p, p, p, p, 64, p, p, None, 8, 64, None)
    assert rc != 0 and "ws not null" in lib.mspi_last_error().decode()


def _model():
    from mspi_amd import testing as T
    from mspi_amd.model.model_utils import AudioVisualSaliencyModel
    return T.seeded(lambda: AudioVisualSaliencyModel(T.make_cfg("x3dl")), 0)


def test_trainable_readout_flags_modes_and_restore(monkeypatch):
    from mspi_amd._lib import MspiError
    from mspi_amd.model import model_utils as pm
    m = _model()
    first = next(m.visnet.parameters())
    first.requires_grad_(False)                                 # a flag the caller had set: must come back as it was
    before = {n: p.requires_grad for n, p in m.named_parameters()}
    assert m.trainable("readout") is m
    on = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert on == sorted(R.STATE_KEYS.values()) and len(on) == 16
    assert on == sorted("readout." + n for n, _ in m.readout.named_parameters())
    m.train()
    m.frozen_encoder()
    training = sorted(n for n, s in m.named_modules() if s.training)
    assert training == ["readout.2", "readout.5"] and not m.training
    m._check_eval()                                             # the forward's guard lets exactly these two through
    for other in (m.readout[1], m.sa_0, m.latlayer_0):
        other.train()
        with pytest.raises(MspiError, match="only readout.2 and readout.5"):
            m._check_eval()
        other.eval()
    m.readout[2].train(), m.readout[5].train()                  # .eval() of a parent does not reach back: still the two
    m._check_eval()
    m.trainable("readout_tail")                                 # switching over: the saved flags are still the original ones
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == sorted(RT.STATE_KEYS.values())
    m.frozen_encoder()
    assert not any(s.training for s in m.modules())
    m.trainable("readout")
    for bad in ("decoder", "all", ""):
        with pytest.raises(MspiError, match="readout_tail"):
            m.trainable(bad)
    m.trainable(None)
    assert {n: p.requires_grad for n, p in m.named_parameters()} == before and not first.requires_grad
    m.train()
    m.frozen_encoder()                                          # switch off: upstream's behaviour, only the two encoders
    assert m.training and m.readout[2].training and not m.audnet.training and not m.image_encoder.training
    with pytest.raises(MspiError, match="inference engine"):
        m._check_eval()
    monkeypatch.setattr(pm, "DECODER_FUSED", False)
    with pytest.raises(MspiError, match="MSPI_DECODER_FUSED"):
        m.trainable("readout")
    assert m.trainable("readout_tail") is m                     # the tail does not need the fused path


def test_head_key_follows_parameters_and_running_statistics():
    m = _model()
    key = m._head_key()
    assert m._head_key() == key and len(key) == 14
    with torch.no_grad():
        m.readout[2].running_var.mul_(2.0)
    k2 = m._head_key()
    assert k2 != key
    with torch.no_grad():
        m.readout[0].weight.add_(1.0)
    k3 = m._head_key()
    assert k3 != k2
    m.load_state_dict(m.state_dict())
    assert m._head_key() != k3
    k4, t4 = m._head_key(), m._tail_key()
    with torch.no_grad():
        m.readout[12].bias.add_(1.0)                            # the tail's business, not the head's
    assert m._head_key() == k4 and m._tail_key() != t4


def test_train_accepts_readout_up_to_the_gpu_check(monkeypatch):
    from mspi_amd import train
    from mspi_amd._lib import MspiError
    assert train.TRAINABLE == ("readout_tail", "readout")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for value in train.TRAINABLE:
        with pytest.raises(SystemExit, match="MI355X"):
            train.main(["--trainable", value])
    for value in ("decoder", "all", ""):
        with pytest.raises(MspiError, match="--trainable %s: only readout_tail, readout can" % value):
            train.main(["--trainable", value])
    assert "--trainable readout" in train.__doc__ and "Still frozen" in train.__doc__


# ------------------------------------------------------------------------------------------------------------- GPU
def _cl(t, dev, ld=None):
    """[N,C,T,H,W] tensor -> CL on the device; ld > C: the rows sit in a wider buffer filled with NaN elsewhere."""
    from mspi_amd import engine as E
    t = torch.as_tensor(t).float()
    N, Cc, T, H, W = t.shape
    rows = t.permute(0, 2, 3, 4, 1).contiguous().to(dev)
    if ld is None:
        return E.CL(rows.view(-1), 0, N, T, H, W, Cc, Cc)
    buf = torch.full((N, T, H, W, ld), float("nan"), device=dev)
    buf[..., ld - Cc:] = rows
    return E.CL(buf.view(-1), ld - Cc, N, T, H, W, Cc, ld)


def _ncdhw(cl):
    return cl.as_ncdhw()


def _wide_case(dev, shape, Cin, Cout, k, pad, seed, ld=None):
    from mspi_amd import engine as E
    gen = torch.Generator().manual_seed(seed)
    N, T, H, W = shape
    x = torch.randn(N, Cin, T, H, W, generator=gen)
    w = torch.randn(Cout, Cin, *k, generator=gen)
    To, Ho, Wo = [n + 2 * p - kk + 1 for n, p, kk in zip((T, H, W), pad, k)]
    dy = torch.randn(N, Cout, To, Ho, Wo, generator=gen)
    pk = E.pack_conv(w, torch.zeros(Cout), None, (1, 1, 1), pad, E.ACT_NONE, device=dev)
    xc, dyc = _cl(x, dev, ld), _cl(dy, dev)
    variant = E.conv_wgrad_wide_variant(xc, dyc, pk)
    dW, db = E.conv_wgrad_wide(xc, dyc, pk)
    if k == (1, 1, 1):
        ref = torch.einsum("bothw,bithw->oi", dy.double(), x.double())[:, :, None, None, None]
    else:
        ref = torch.nn.grad.conv3d_weight(x.double(), w.shape, dy.double(), padding=pad)
    return variant, (dW, ref), (db, dy.double().sum((0, 2, 3, 4)))


WIDE_GEOMETRIES = {
    # the three layers at width 192 on the pyramid (1, 1, 2): s0 is [1, 4, 8, 16]; the 1x1x1 layer on s3, 8 rows
    "r1_27tap": ((1, 4, 8, 16), 192, 192, (3, 3, 3), (1, 1, 1), None),
    "r4_9tap": ((1, 4, 8, 16), 192, 64, (1, 3, 3), (0, 1, 1), None),
    "r0_on_s3": ((1, 4, 1, 2), 192, 192, (1, 1, 1), (0, 0, 0), None),
    # channel pairs, on maps that are no multiple of the box (4 x 4 x 8) and hold several boxes and slices
    "32_32": ((2, 3, 5, 19), 32, 32, (3, 3, 3), (1, 1, 1), None),
    "192_64": ((2, 4, 9, 7), 192, 64, (1, 3, 3), (0, 1, 1), None),
    "64_192": ((1, 5, 6, 9), 64, 192, (1, 3, 3), (0, 1, 1), None),
    "taps_2": ((1, 4, 6, 9), 32, 64, (2, 1, 1), (0, 0, 0), None),
    "taps_27_flat": ((2, 1, 1, 9), 32, 32, (1, 1, 27), (0, 0, 13), None),
    # an input with ld > C: a channel slice of a wider buffer
    "ld_gt_c_9tap": ((1, 4, 8, 16), 64, 32, (1, 3, 3), (0, 1, 1), 96),
    "ld_gt_c_1tap": ((1, 4, 8, 17), 32, 64, (1, 1, 1), (0, 0, 0), 160),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WIDE_GEOMETRIES))
def test_hip_wide_wgrad_vs_fp64(dev, name):
    shape, Cin, Cout, k, pad, ld = WIDE_GEOMETRIES[name]
    variant, (dW, ref), (db, bref) = _wide_case(dev, shape, Cin, Cout, k, pad, 8800 + Cin + Cout, ld)
    print("%s: dW %.2e, db %.2e of the largest entry; %d boxes per slice" % (name, _err(dW, ref), _err(db, bref), variant))
    assert variant == BPS
    assert _err(dW, ref) <= GRAD_TOL and _err(db, bref) <= GRAD_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("M", WIDE_BOUNDARY)
def test_hip_wide_wgrad_slice_boundaries(dev, M):
    variant, (dW, ref), (db, bref) = _wide_case(dev, (1, 1, 1, M), 32, 32, (1, 1, 1), (0, 0, 0), 8900 + M % 97)
    print("M = %d: dW %.2e, db %.2e of the largest entry; %d boxes per slice" % (M, _err(dW, ref), _err(db, bref), variant))
    assert variant == (BPS_BIG if (M + BOX - 1) // BOX >= BIG_BOXES else BPS)
    assert _err(dW, ref) <= GRAD_TOL and _err(db, bref) <= GRAD_TOL


@pytest.mark.gpu
def test_hip_wide_wgrad_long_slices_with_taps(dev):
    """The long slice on a kernel with taps: 2 x 2 x 13 x 10 = 520 boxes of 4 x 4 x 8 positions."""
    variant, (dW, ref), (db, bref) = _wide_case(dev, (2, 8, 52, 80), 32, 32, (1, 3, 3), (0, 1, 1), 8990)
    print("520 boxes: dW %.2e, db %.2e of the largest entry" % (_err(dW, ref), _err(db, bref)))
    assert variant == BPS_BIG and _err(dW, ref) <= GRAD_TOL and _err(db, bref) <= GRAD_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("M", [2, 255, 4096])
def test_hip_bn_stats_on_shifted_channels(dev, M):
    from mspi_amd import engine as E
    gen = torch.Generator().manual_seed(9000 + M)
    mu, sd = torch.linspace(-1000.0, 1000.0, 64), torch.logspace(-1.0, 1.0, 64)
    x = torch.randn(M, 64, generator=gen) * sd[torch.randperm(64, generator=gen)] + mu
    mean, var, rstd = E.bn_stats(E.from_rows(x.to(dev)), eps=1e-5)
    xd = x.double()
    rm, rv = xd.mean(0), xd.var(0, unbiased=False)
    e_mean = ((mean.double().cpu() - rm).abs() / rm.abs().clamp_min(1.0)).max().item()
    e_var = ((var.double().cpu() - rv).abs() / rv).max().item()
    e_rstd = _err(rstd, 1.0 / torch.sqrt(rv + 1e-5))
    naive = ((x * x).mean(0) - x.mean(0) ** 2).double()
    print("M = %d: mean %.2e, var %.2e, rstd %.2e (fp32 one-pass var: %.2e)" % (M, e_mean, e_var, e_rstd, ((naive - rv).abs() / rv).max().item()))
    assert e_mean <= 2e-5 and e_var <= 2e-5 and e_rstd <= 2e-5


def _bn_layers():
    """(label, key, D, which BatchNorm): C of 32 and 64 on both cases, 192 on "tiny" at width 192."""
    return [("tiny_c32", "tiny", 32, 2), ("tiny_c64", "tiny", 32, 5), ("odd_c32", "odd", 32, 2), ("odd_c64", "odd", 32, 5),
            ("tiny_c192", "tiny", 192, 2), ("odd_c192", "odd", 192, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("label,key,D,which", _bn_layers(), ids=[b[0] for b in _bn_layers()])
def test_hip_bn_apply_and_bwd_vs_restatement(dev, label, key, D, which):
    from mspi_amd import engine as E
    case, saved, grads = _restated(key, D)
    head = saved["head"]
    hb = R.head_backward(case, head, grads["y4"])
    xk, ak, gk, bk, dyk, dxk, wk, biask = (("x1", "a1", "g2", "be2", "da1", "d1", "w1", "b1") if which == 2 else
                                           ("x4", "y4", "g5", "be5", None, "d4", "w4", "b4"))
    x = _cl(head[xk], dev)
    gamma, beta = torch.from_numpy(case[gk]).to(dev), torch.from_numpy(case[bk]).to(dev)
    mean, var, rstd = E.bn_stats(x)
    m_ref, v_ref, r_ref = head["bn%d" % which]
    y = E.bn_apply(x, mean, rstd, gamma, beta, act=E.ACT_RELU)
    errs = {"mean": (mean.double().cpu() - m_ref).abs().max().item(), "var": _err(var, v_ref), "rstd": _err(rstd, r_ref),
            "y": _err(_ncdhw(y), head[ak])}
    dy_ref = grads["y4"] if dyk is None else hb[dyk]
    dx, dgamma, dbeta = E.bn_bwd(_cl(dy_ref, dev), x, mean, rstd, gamma, y=_cl(head[ak], dev))      # the restatement's mask
    errs.update(dx=_err(_ncdhw(dx), hb[dxk]), dgamma=_err(dgamma, hb[gk]), dbeta=_err(dbeta, hb[bk]))
    # no ReLU: y = NULL, every row counts
    plain = E.bn_apply(x, mean, rstd, gamma, beta)
    v = lambda t: t.view(1, -1, 1, 1, 1)
    errs["y_plain"] = _err(_ncdhw(plain), head["p%d" % which])
    dx2, dg2, db2 = E.bn_bwd(_cl(dy_ref, dev), x, mean, rstd, gamma)
    ref2 = R.bn_backward(dy_ref, head[xk], m_ref, r_ref, torch.from_numpy(case[gk]).double(), torch.ones_like(dy_ref))
    errs.update(dx_plain=_err(_ncdhw(dx2), ref2[0]), dgamma_plain=_err(dg2, ref2[1]), dbeta_plain=_err(db2, ref2[2]))
    # the bias in front of the BatchNorm: its gradient is the sum of dx, zero in exact arithmetic
    pad = (1, 1, 1) if which == 2 else (0, 1, 1)
    pk = E.pack_conv(torch.from_numpy(case[wk]), torch.from_numpy(case[biask]), None, (1, 1, 1), pad, E.ACT_NONE, device=dev)
    src = _cl(head["y0"] if which == 2 else head["a1"], dev)
    dW, db = E.conv_wgrad_wide(src, _cl(hb[dxk], dev), pk)
    errs["dW"] = _err(dW, hb[wk])
    zero = db.abs().max().item() / _gsum(hb[dxk])
    print("%s: %s; |d %s| = %.2e of sum|g|" % (label, ", ".join("%s %.2e" % kv for kv in errs.items()), biask, zero))
    assert errs.pop("mean") <= GRAD_TOL * max(1.0, m_ref.abs().max().item())
    assert all(e <= GRAD_TOL for e in errs.values()), errs
    assert zero <= GRAD_TOL


def _head_args(case, dev, buffers=True):
    """(maps, the ten head parameters as leaves, the two buffer triples) on the device, fresh buffers (0, 1, 0)."""
    maps = [torch.from_numpy(case[k]).to(dev).permute(0, 2, 3, 4, 1).contiguous() for k in R.MAPS]
    params = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in R.HEAD]
    bn = [(torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.long, device=dev))
          for c in (case["g2"].shape[0], 64)] if buffers else [None, None]
    return maps, params, bn


def _readout(case, dev, gscale=1.0, bn=None):
    """One forward and backward of ReadoutHead + ReadoutTail: (out, {name: gradient})."""
    from mspi_amd.autograd import ReadoutHead, ReadoutTail
    maps, head, fresh = _head_args(case, dev)
    bn = fresh if bn is None else bn
    tail = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in RT.PARAMS]
    y4 = ReadoutHead.apply(*maps, *head, bn[0], bn[1])
    assert y4.requires_grad and not any(m.requires_grad for m in maps)
    out = ReadoutTail.apply(y4, *tail)
    (out * (torch.from_numpy(case["g"]).to(dev) * gscale)).sum().backward()
    return out.detach(), dict(zip(R.PARAMS, [p.grad for p in head + tail]))


def _assert_grads(got, grads, case, what, scale=1.0):
    gsum = _gsum(case["g"])
    for k in R.PARAMS:
        if k in ZERO_BIASES:
            e = got[k].double().abs().max().item() / (gsum * scale)
            print("%s %s: %.2e of sum|g|" % (what, k, e))
        else:
            e = _err(got[k], grads[k] * scale)
            print("%s %s: %.2e of the largest entry" % (what, k, e))
        assert e <= GRAD_TOL, (what, k, e)


@pytest.mark.gpu
@pytest.mark.parametrize("key,D", [("tiny", 32), ((1, 1, 2), 192)], ids=["fixture_tiny", "live_width_192"])
def test_hip_readout_end_to_end(dev, key, D):
    case, saved, grads = _restated(key, D)
    out, got = _readout(case, dev)
    ref = torch.from_numpy(_gold()["tiny_out"]) if key == "tiny" else saved["out"]
    err = (out.double().cpu() - ref).abs().max().item()
    print("%s: map error %.2e" % (key, err))
    assert err < MAP_TOL
    ref_grads = {k: torch.from_numpy(_gold()["tiny_d_%s" % k]) for k in R.PARAMS} if key == "tiny" else grads
    _assert_grads(got, ref_grads, case, str(key))


@pytest.mark.gpu
@pytest.mark.parametrize("exp", [-20, -30, 12])
def test_hip_readout_gradients_at_the_scale_of_a_loss(dev, exp):
    case, saved, grads = _restated("tiny")
    _, got = _readout(case, dev, gscale=2.0 ** exp)
    _assert_grads(got, grads, case, "g * 2^%d" % exp, scale=2.0 ** exp)


@pytest.mark.gpu
def test_hip_readout_backward_is_repeatable(dev):
    case, _, _ = _restated((1, 1, 2), 192)
    _, a = _readout(case, dev)
    _, b = _readout(case, dev)
    for k in R.PARAMS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_hip_running_statistics_after_two_forwards(dev):
    from mspi_amd.autograd import ReadoutHead
    case, saved, _ = _restated("odd")
    seq = R.upstream_readout(case)
    s = [torch.from_numpy(case[k]).double() for k in R.MAPS]
    ups = [torch.nn.Upsample(scale_factor=(1, k, k), mode="trilinear", align_corners=False)(t) for k, t in ((2, s[1]), (4, s[2]), (8, s[3]))]
    cat = torch.cat([s[0] + ups[0] + ups[1] + ups[2]] + ups, 1)
    with torch.no_grad():
        seq(cat), seq(cat)
    maps, head, bn = _head_args(case, dev)
    with torch.no_grad():
        ReadoutHead.apply(*maps, *head, bn[0], bn[1])
        ReadoutHead.apply(*maps, *head, bn[0], bn[1])
    for i, (rm, rv, nbt) in zip((2, 5), bn):
        print("readout[%d]: running mean %.2e (absolute), running var %.2e" % (i, (rm.double().cpu() - seq[i].running_mean).abs().max().item(),
                                                                               _err(rv, seq[i].running_var)))
        assert (rm.double().cpu() - seq[i].running_mean).abs().max().item() <= GRAD_TOL * max(1.0, seq[i].running_mean.abs().max().item())
        assert _err(rv, seq[i].running_var) <= GRAD_TOL
        assert int(nbt) == int(seq[i].num_batches_tracked) == 2
    # without buffers (the module in eval()): nothing to update, same output
    y_a = ReadoutHead.apply(*maps, *[p.detach() for p in head], bn[0], bn[1])
    y_b = ReadoutHead.apply(*maps, *[p.detach() for p in head], None, None)
    assert torch.equal(y_a, y_b) and int(bn[0][2]) == 3


def _dot(a, b):
    return (a.double().cpu() * b.double().cpu()).sum().item()


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,k,pad", [(192, 192, (3, 3, 3), (1, 1, 1)), (64, 192, (1, 3, 3), (0, 1, 1))], ids=["27tap_192_192", "9tap_64_192"])
def test_hip_conv_transpose_is_the_adjoint(dev, Cin, Cout, k, pad):
    """<conv(x), d> = <x, conv_T(d)> with the flipped, transposed pack ReadoutHead.backward builds, both at PREC_F32."""
    from mspi_amd import engine as E
    gen = torch.Generator().manual_seed(9100 + Cin)
    w = torch.randn(Cout, Cin, *k, generator=gen) / (Cin * k[0] * k[1] * k[2]) ** 0.5
    x, d = torch.randn(2, Cin, 4, 6, 9, generator=gen), torch.randn(2, Cout, 4, 6, 9, generator=gen)
    pk = E.pack_conv(w, None, None, (1, 1, 1), pad, E.ACT_NONE, device=dev, prec=E.PREC_F32)
    pkt = E.pack_conv(w.transpose(0, 1).flip(2, 3, 4), None, None, (1, 1, 1), pad, E.ACT_NONE, device=dev, prec=E.PREC_F32)
    lhs = _dot(_ncdhw(E.conv(_cl(x, dev), pk)), d)
    rhs = _dot(x, _ncdhw(E.conv(_cl(d, dev), pkt)))
    ref = _dot(torch.nn.functional.conv3d(x.double(), w.double(), padding=pad), d)
    print("<conv x, d> = %.9e, <x, conv_T d> = %.9e, float64 %.9e" % (lhs, rhs, ref))
    scale = (torch.nn.functional.conv3d(x.double(), w.double(), padding=pad) * d.double()).abs().sum().item()
    assert abs(lhs - rhs) <= 1e-5 * scale and abs(lhs - ref) <= 1e-5 * scale


@pytest.mark.gpu
def test_hip_dw0_is_the_wgrad_over_the_concat(dev):
    """ReadoutHead's dW0, assembled from four 1x1x1 wide weight gradients on the coarse maps, against a wide weight gradient
    over the explicitly built 768-channel concat (four 192-channel slices of it, ld 768) with the same dy0."""
    from mspi_amd import engine as E
    case, saved, grads = _restated((1, 1, 2), 192)
    _, got = _readout(case, dev)
    head = saved["head"]
    hb = R.head_backward(case, head, grads["y4"])
    s = [torch.from_numpy(case[k]).double() for k in R.MAPS]
    ups = [R.up(t, kk) for kk, t in ((2, s[1]), (4, s[2]), (8, s[3]))]
    cat = _cl(torch.cat([s[0] + ups[0] + ups[1] + ups[2]] + ups, 1), dev)
    assert cat.C == 768
    dy0 = _cl(hb["dy0"], dev)
    pk = E.pack_conv(torch.zeros(192, 192, 1, 1, 1), torch.zeros(192), device=dev)
    blocks = [E.conv_wgrad_wide(cat.slice(192 * j, 192), dy0, pk) for j in range(4)]
    dW0 = torch.cat([b[0] for b in blocks], 1)
    print("dW0: concat against float64 %.2e, ReadoutHead against float64 %.2e, against the concat %.2e"
          % (_err(dW0, hb["w0"]), _err(got["w0"], hb["w0"]), _err(got["w0"], dW0.double().cpu())))
    assert _err(dW0, hb["w0"]) <= GRAD_TOL and _err(got["w0"], dW0.double().cpu()) <= GRAD_TOL
    assert _err(blocks[0][1], hb["b0"]) <= GRAD_TOL


@pytest.mark.gpu
def test_hip_whole_model_trains_its_readout(dev, golden_dir):
    from mspi_amd import metrics as M
    from test_readout_tail import _batches, _build
    g, cfg, make, clips, audio = _build(golden_dir, "av_x3dl_64", "x3dl", "AudioVisualSaliencyModel", dev)
    m = make().to(dev)
    off, _ = m(clips, audio)
    m.trainable("readout")
    from mspi_amd._lib import MspiError
    with pytest.raises(MspiError, match="frozen_encoder"):      # eval() BatchNorm and a graph: batch statistics would be a surprise
        m(clips, audio)
    m.train()
    m.frozen_encoder()
    with torch.no_grad():
        quiet, _ = m(clips, audio)
    assert torch.equal(quiet, off) and not quiet.requires_grad
    start = {k: v.clone() for k, v in m.state_dict().items()}
    params = [p for p in m.parameters() if p.requires_grad]
    assert len(params) == 16
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0)
    label = _batches(clips, audio, 1, True)[0][2].to(dev)
    out, aux = m(clips, audio)
    assert out.requires_grad and not aux.requires_grad
    opt.zero_grad()
    M.SalLoss()(out, label).backward()
    opt.step()
    moved = set(R.STATE_KEYS.values()) | {"readout.%d.%s" % (i, n) for i in (2, 5) for n in ("running_mean", "running_var", "num_batches_tracked")}
    for k, v in m.state_dict().items():
        assert torch.equal(v, start[k]) == (k not in moved), k
    assert int(m.readout[2].num_batches_tracked) == int(start["readout.2.num_batches_tracked"]) + 1
    with torch.no_grad():
        trained, _ = m(clips, audio)
    assert not torch.equal(trained, off) and torch.isfinite(trained).all()
    fresh = make()
    fresh.load_state_dict(m.state_dict())
    again, _ = fresh.to(dev)(clips, audio)
    assert torch.equal(again, trained)
    m.trainable(None)
    m.eval()
    plain, _ = m(clips, audio)
    assert torch.equal(plain, trained) and not plain.requires_grad
