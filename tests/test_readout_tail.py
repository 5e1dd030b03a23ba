"""The trainable readout tail: csrc/readout_bwd.hip, engine.conv_wgrad / conv_c1_bwd / upsample_bwd / logsumexp_sub_bwd,
autograd.ReadoutTail, _SaliencyBase.trainable("readout_tail"), mspi_amd.train.

Yardsticks: tests/golden/readout_tail.npz holds two small cases with the float64 value and the seven gradients torch autograd
gives through UPSTREAM's order of the tail (tools/gen_readout_tail_golden.py); tests/readout_tail_restate.py is the float64 CPU
restatement in this project's order with its analytic backward, which the generator pinned to the fixture and which stands
in for it on other shapes.

Bounds.  Every gradient tensor: max |got - ref| / max |ref| <= 2e-5, the project's bar for gradients
(tests/test_sal_loss_grad.py); a float32 CPU evaluation of the same tail sits at 1.7e-7 .. 1.3e-6, so the bar leaves room for
the summation order and nothing else (both data-gradient convs run on the fp32 MFMA path, not on f16x3).  readout.12.bias: its gradient is zero in exact
arithmetic (the log-softmax ignores a shift), checked as |db12| <= 1e-6 sum|g|.  Adjoint identities: 1e-5 relative, the sums
accumulated in float64 on the host, once per factor with an independent random y (relative to the value itself) and on further
shapes with a random y that carries the signs of A x (relative to the sum of the terms' magnitudes: no cancellation).

ReLU kinks.  Kernel-level tests feed the backward entry points the restatement's own saved activations cast to fp32, so the
masks agree by construction.  The end-to-end test hands the DEVICE's masks to the restatement's backward and asserts that
every cell where they differ from the float64 masks has |float64 pre-activation| <= 1e-5."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import readout_tail_restate as RT
import sal_loss_restate as S
from test_parity_gpu import MAP_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_logsumexp_sub_bwd", "mspi_conv_c1_bwd_ws_bytes", "mspi_conv_c1_bwd", "mspi_conv_wgrad_supported",
               "mspi_conv_wgrad_ws_bytes", "mspi_conv_wgrad_variant", "mspi_conv_wgrad_fwd", "mspi_upsample_bwd")
CASES = ("tiny", "odd")
SHAPES = {"tiny": (1, 2, 3), "odd": (2, 5, 7)}            # (B, h, w); H = 4h, W = 4w
MULTI = (2, 8, 12)                                         # 3072 rows at full resolution: several slices and workgroups
GRAD_TOL = 2e-5
NAMES = ("y4",) + RT.PARAMS

# the split constants of csrc/readout_bwd.hip and the extents (N, H, W) on both sides of each
SLICE = 256            # WG_SLICE_SMALL: rows per slice of mspi_conv_wgrad_fwd below BIG_M rows (a wave takes a quarter, 64)
SLICE_BIG = 2048       # WG_SLICE_BIG: rows per slice from BIG_M rows on
BIG_M = 65536          # WG_BIG_M
WGRAD_BOUNDARY = {SLICE - 1: (1, 15, 17), SLICE: (1, 16, 16), SLICE + 1: (1, 1, 257),
                  BIG_M - 1: (1, 255, 257), BIG_M: (1, 256, 256), BIG_M + 1: (1, 1, 65537)}
C1_ROWS = 1024         # C1_ROWS: rows per workgroup of mspi_conv_c1_bwd
C1_BOUNDARY = {C1_ROWS - 1: (1, 33, 31), C1_ROWS: (1, 32, 32), C1_ROWS + 1: (1, 25, 41)}


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "readout_tail.npz"))
    return {k: z[k] for k in z.files}


def _fixture_case(name):
    g = _gold()
    return {k: g["%s_%s" % (name, k)] for k in ("y4", "g") + RT.PARAMS}


@functools.lru_cache(maxsize=None)
def _restated(key):
    """(case, saved, grads) of a fixture case (by name) or of a seeded (B, h, w) shape, computed once in float64."""
    case = _fixture_case(key) if isinstance(key, str) else RT.make_case(*key, seed=8500 + sum(key))
    saved = RT.forward(case["y4"], case)
    return case, saved, RT.backward(case["y4"], case, saved, case["g"])


def _err(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / ref.abs().max()).item()


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["cases"]) == CASES
    for c in CASES:
        B, h, w = SHAPES[c]
        assert g["%s_y4" % c].shape == (B, 64, 4, h, w) and g["%s_y4" % c].dtype == np.float32
        assert g["%s_g" % c].shape == (B, 4 * h, 4 * w) and g["%s_g" % c].dtype == np.float32
        zero = float((g["%s_y4" % c] == 0).mean())
        assert (g["%s_y4" % c] >= 0).all() and 0.2 <= zero <= 0.4, zero
        for k in RT.PARAMS:
            assert g["%s_%s" % (c, k)].shape == RT.PARAM_SHAPES[k] and g["%s_%s" % (c, k)].dtype == np.float32
        assert g["%s_out" % c].dtype == np.float64 and g["%s_out" % c].shape == (B, 4 * h, 4 * w)
        for k in NAMES:
            assert g["%s_d_%s" % (c, k)].dtype == np.float64 and g["%s_d_%s" % (c, k)].shape == g["%s_%s" % (c, k)].shape
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "readout_tail.npz")) < (1 << 20)
    assert RT.min_preactivation(_restated("tiny")[1]) >= 1e-4            # the kink-free case


def test_restatement_matches_the_fixture():
    g = _gold()
    for c in CASES:
        case, saved, grads = _restated(c)
        assert (saved["out"] - torch.from_numpy(g["%s_out" % c])).abs().max().item() <= 1e-12
        gsum = np.abs(case["g"]).astype(np.float64).sum()
        for k in NAMES:
            ref = torch.from_numpy(g["%s_d_%s" % (c, k)])
            if k == "b12":
                assert (grads[k] - ref).abs().max().item() <= 1e-12 * gsum
            else:
                assert _err(grads[k], ref) <= 1e-12, (c, k)


def test_restated_gradient_is_autograd_of_the_restated_forward():
    """On a shape the fixture does not hold, (1, 9, 4)."""
    case, saved, grads = _restated((1, 9, 4))
    leaves = {k: torch.from_numpy(case[k]).double().requires_grad_(True) for k in NAMES}
    out = RT.forward(leaves["y4"], leaves)["out"]
    got = torch.autograd.grad((out * torch.from_numpy(case["g"]).double()).sum(), [leaves[k] for k in NAMES])
    gsum = np.abs(case["g"]).astype(np.float64).sum()
    for k, t in zip(NAMES, got):
        if k == "b12":
            assert (grads[k] - t).abs().max().item() <= 1e-12 * gsum
        else:
            assert _err(grads[k], t) <= 1e-12, k


def test_new_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mspi_hip.h")).read()
    assert int(re.search(r"#define\s+MSPI_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mspi_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib._SIGNATURES and name in _lib.EXPORTS
        assert getattr(raw, name) is not None and getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]
    assert lib.mspi_version() == 2
    mk = open(os.path.join(ROOT, "mspi_amd", "csrc", "Makefile")).read()
    assert "readout_bwd.hip" in mk


def _desc(N, T, H, W, Cin, Cout, k, s, p):
    from mspi_amd import _lib
    d = _lib.ConvDesc()
    d.N, d.T, d.H, d.W, d.C = N, T, H, W, Cin
    d.sN, d.sT, d.sH, d.sW, d.sC = T * H * W * Cin, H * W * Cin, W * Cin, Cin, 1
    d.kT, d.kH, d.kW = k
    d.strT, d.strH, d.strW = s
    d.padT, d.padH, d.padW = p
    d.To, d.Ho, d.Wo = [(e + 2 * pp - kk) // ss + 1 for e, kk, ss, pp in zip((T, H, W), k, s, p)]
    d.Cout, d.ldy = Cout, Cout
    return d


R10 = dict(k=(1, 3, 3), s=(1, 1, 1), p=(0, 1, 1))
R8 = dict(k=(4, 1, 1), s=(4, 1, 1), p=(0, 0, 0))


def test_wgrad_host_answers_and_workspace_arithmetic():
    """_supported / _variant / _ws_bytes are host arithmetic.  A slice record holds 32 x (tiles x 32) partial products and 32
    bias sums; tiles = taps x ceil(Cin / 32); slices = ceil(M / 256), ceil(M / 2048) from 65536 rows on."""
    from mspi_amd import _lib, engine as E
    lib = _lib.load()
    assert E.WGRAD_SLICES == (SLICE, SLICE_BIG) and E.WGRAD_BIG_M == BIG_M and E.C1_BWD_ROWS == C1_ROWS
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    base = (p.value + 15) // 16 * 16
    al, mis = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def ws(d):
        return lib.mspi_conv_wgrad_ws_bytes(ctypes.byref(d))

    def rec(tiles):
        return 4 * (32 * tiles * 32 + 32)
    # the two layers of the tail at 8 x 224 x 384 and on the fixture shapes
    for B, h, w in ((8, 56, 96),) + tuple(SHAPES.values()) + (MULTI,):
        d10, d8 = _desc(B, 1, 4 * h, 4 * w, 32, 32, **R10), _desc(B, 4, h, w, 64, 32, **R8)
        for d, tiles in ((d10, 9), (d8, 8)):
            M = d.N * d.To * d.Ho * d.Wo
            sl = SLICE_BIG if M >= BIG_M else SLICE
            assert lib.mspi_conv_wgrad_supported(ctypes.byref(d)) == 1
            assert lib.mspi_conv_wgrad_variant(ctypes.byref(d), al, al) == sl
            assert ws(d) == -(-M // sl) * rec(tiles), (B, h, w)
    for M, (N, H, W) in WGRAD_BOUNDARY.items():
        d = _desc(N, 1, H, W, 36, 12, **R10)
        assert lib.mspi_conv_wgrad_variant(ctypes.byref(d), al, al) == (SLICE_BIG if M >= BIG_M else SLICE)
        assert ws(d) == -(-M // (SLICE_BIG if M >= BIG_M else SLICE)) * rec(18)
    # refusals: each answers 0 / -1 with a message, and the launch refuses the same
    good = lambda: _desc(2, 1, 20, 28, 32, 32, **R10)      # noqa: E731
    bad = {"Cout": good(), "Cin": good(), "sC": good()}
    bad["Cout"].Cout = bad["Cout"].ldy = 36
    bad["Cin"].C = 68
    bad["sC"].sC = 2
    for key, d in bad.items():
        assert lib.mspi_conv_wgrad_supported(ctypes.byref(d)) == 0 and b"mspi_conv_wgrad" in lib.mspi_last_error(), key
        assert lib.mspi_conv_wgrad_variant(ctypes.byref(d), al, al) == -1 and ws(d) == 0
        assert lib.mspi_conv_wgrad_fwd(ctypes.byref(d), al, al, al, al, al, None) == -1
    d = good()
    assert lib.mspi_conv_wgrad_supported(ctypes.byref(d)) == 1
    for x, dy in ((mis, al), (al, mis)):
        assert lib.mspi_conv_wgrad_variant(ctypes.byref(d), x, dy) == -1 and b"aligned" in lib.mspi_last_error()
        assert lib.mspi_conv_wgrad_fwd(ctypes.byref(d), x, dy, al, al, al, None) == -1
    # the last conv's workspace: one record of 9 x 64 + 4 floats per 1024 rows
    c1 = lib.mspi_conv_c1_bwd_ws_bytes
    assert c1(0, 4, 4) == 0 and c1(1, 0, 4) == 0 and c1(1, 4, -1) == 0
    for M, (N, H, W) in C1_BOUNDARY.items():
        assert c1(N, H, W) == -(-M // C1_ROWS) * 4 * (9 * 64 + 4)
    assert c1(8, 224, 384) == 672 * 4 * 580
    # argument checks of the other entry points, no launch
    assert lib.mspi_logsumexp_sub_bwd(None, al, al, 1, 8, None) == -1 and b"mspi_logsumexp_sub_bwd" in lib.mspi_last_error()
    assert lib.mspi_upsample_bwd(al, 4, None, 0, al, 4, 1, 2, 2, 4, 3, 0, None) == -1 and b"factor" in lib.mspi_last_error()
    assert lib.mspi_upsample_bwd(al, 4, None, 0, al, 4, 1, 2, 2, 4, 4, 1, None) == -1 and b"RELU" in lib.mspi_last_error()
    assert lib.mspi_upsample_bwd(al, 6, None, 0, al, 6, 1, 2, 2, 6, 4, 0, None) == -1
    assert lib.mspi_conv_c1_bwd(al, 68, al, al, al, 68, al, al, al, 1, 4, 4, 68, None) == -1 and b"C must" in lib.mspi_last_error()
    assert lib.mspi_conv_c1_bwd(mis, 32, al, al, al, 32, al, al, al, 1, 4, 4, 32, None) == -1


def test_lr_by_epoch_is_upstreams_list():
    from mspi_amd import testing as T
    from mspi_amd.train import lr_by_epoch
    for max_epoch in (120, 180):
        cfg = T.make_cfg("x3dl")
        cfg.SOLVER.MAX_EPOCH = max_epoch
        lr = cfg.SOLVER.LR
        want = [lr] * 60 + [lr * 0.1] * 60 + ([lr * 0.1 * 0.1] * 60 if max_epoch == 180 else [])
        assert lr_by_epoch(cfg) == want and len(want) == max_epoch


def test_train_refuses_other_trainable_values_and_more_ranks(monkeypatch):
    from mspi_amd import train
    from mspi_amd._lib import MspiError
    for value in ("decoder", "all", ""):
        with pytest.raises(MspiError, match="--trainable %s: only readout_tail" % value):
            train.main(["--trainable", value])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(MspiError, match="one rank"):
        train.main(["--trainable", "readout_tail"])
    args = train.build_parser().parse_args([])
    for name in ("split", "dataset", "weights", "log_dir", "save_ckpt_freq", "gamma", "start_epoch", "trainable"):
        assert hasattr(args, name)


def test_train_loop_schedule_checkpoints_and_log(tmp_path, monkeypatch):
    """train() with a stub model and a stubbed epoch: the learning rate each epoch sees, which checkpoints are written and
    that they load, one JSON line per epoch."""
    import json
    from mspi_amd import engine_train, testing as T, train
    from mspi_amd._lib import MspiError
    cfg = T.make_cfg("x3dl")
    cfg.SOLVER.MAX_EPOCH = 63
    model = torch.nn.Linear(2, 1)
    seen = []

    def fake_epoch(model, criterion, data, optimizer, device, epoch, cfg, gamma=1.0, **kw):
        assert not kw and type(criterion).__name__ == "SalLoss" and isinstance(optimizer, torch.optim.AdamW)
        assert [g["weight_decay"] for g in optimizer.param_groups] == [0]
        seen.append((epoch, optimizer.param_groups[0]["lr"], gamma, data))
        with torch.no_grad():
            model.weight.add_(1.0)
        return {"loss": 1.0 / (epoch + 1), "lr": optimizer.param_groups[0]["lr"]}
    monkeypatch.setattr(engine_train, "train_one_epoch", fake_epoch)
    logs = train.train(model, "batches", cfg, torch.device("cpu"), str(tmp_path), start_epoch=58, save_ckpt_freq=2, gamma=0.5)
    lr = cfg.SOLVER.LR
    assert seen == [(58, lr, 0.5, "batches"), (59, lr, 0.5, "batches")] + [(e, lr * 0.1, 0.5, "batches") for e in (60, 61, 62)]
    assert sorted(os.listdir(tmp_path / "checkpoints")) == ["ckpt_60.pth", "ckpt_62.pth", "ckpt_63.pth"]
    sd = torch.load(tmp_path / "checkpoints" / "ckpt_63.pth")
    assert set(sd) == {"weight", "bias"} and torch.equal(sd["weight"], model.weight.detach())
    lines = [json.loads(line) for line in open(tmp_path / "log.txt")]
    assert lines == logs and [line["epoch"] for line in lines] == [58, 59, 60, 61, 62]
    assert lines[0] == {"train_loss": 1.0 / 59, "train_lr": lr, "epoch": 58, "n_parameters": 3}
    for p in model.parameters():
        p.requires_grad_(False)
    with pytest.raises(MspiError, match="no parameter requires grad"):
        train.train(model, "batches", cfg, torch.device("cpu"), str(tmp_path))


def test_trainable_switch_sets_and_restores_flags():
    from mspi_amd import testing as T
    from mspi_amd._lib import MspiError
    from mspi_amd.model.model_utils import AudioVisualSaliencyModel
    m = T.seeded(lambda: AudioVisualSaliencyModel(T.make_cfg("x3dl")), 0)
    first = next(m.visnet.parameters())
    first.requires_grad_(False)                                 # a flag the caller had set: must come back as it was
    before = {n: p.requires_grad for n, p in m.named_parameters()}
    assert m.trainable("readout_tail") is m
    on = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert on == sorted(RT.STATE_KEYS.values()) and len(on) == 6
    m.trainable("readout_tail")                                 # twice: the saved flags are still the original ones
    m.train()
    m.frozen_encoder()
    assert not m.training and not any(s.training for s in m.modules())
    with pytest.raises(MspiError, match="readout_tail"):
        m.trainable("decoder")
    m.trainable(None)
    assert {n: p.requires_grad for n, p in m.named_parameters()} == before and not first.requires_grad
    m.train()
    m.frozen_encoder()                                          # switch off: upstream's behaviour, only the two encoders
    assert m.training and not m.audnet.training and not m.image_encoder.training


# ------------------------------------------------------------------------------------------------------------- GPU
def _cl(t, dev):
    """[N,C,T,H,W] (or [N,C,H,W]) tensor -> dense CL on the device, C a multiple of 4."""
    from mspi_amd import engine as E
    t = torch.as_tensor(t).float()
    if t.dim() == 4:
        t = t[:, :, None]
    N, Cc, T, H, W = t.shape
    return E.CL(t.permute(0, 2, 3, 4, 1).contiguous().to(dev).view(-1), 0, N, T, H, W, Cc, Cc)


def _nchw(cl):
    return cl.as_ncdhw().squeeze(2)


def _tail_packs(case, dev):
    from mspi_amd.autograd import pack_readout_tail
    return pack_readout_tail(*[torch.from_numpy(case[k]).to(dev) for k in RT.PARAMS])


def _entry_points(dev, key):
    """Every backward entry point on the restatement's own saved activations: {name: (got, ref)}."""
    from mspi_amd import engine as E
    case, saved, grads = _restated(key)
    pk8, pk10, _ = _tail_packs(case, dev)
    w10 = torch.from_numpy(case["w10"]).to(dev)
    u, y10 = _cl(saved["u"], dev), _cl(saved["y10"], dev)
    res = {}
    res["dz"] = (E.logsumexp_sub_bwd(saved["out"].float().to(dev), torch.from_numpy(case["g"]).to(dev)), grads["dz"])
    d10, dw12, db12 = E.conv_c1_bwd(y10, grads["dz"].float().to(dev), torch.from_numpy(case["w12"]).to(dev))
    res["d10"], res["w12"], res["b12"] = (_nchw(d10), grads["d10"]), (dw12, grads["w12"]), (db12, grads["b12"])
    d10r = _cl(grads["d10"], dev)
    assert E.conv_wgrad_variant(u, d10r, pk10) == (SLICE_BIG if u.M >= BIG_M else SLICE)
    dw10, db10 = E.conv_wgrad(u, d10r, pk10)
    res["w10"], res["b10"] = (dw10, grads["w10"]), (db10, grads["b10"])
    pk10t = E.pack_conv(w10.transpose(0, 1).flip(3, 4), None, None, (1, 1, 1), (0, 1, 1), E.ACT_NONE, prec=E.PREC_F32)
    res["du_raw"] = (_nchw(E.conv(d10r, pk10t)), grads["du_raw"])
    d8 = E.upsample_bwd(_cl(grads["du_raw"], dev), 4, u=u, act=E.ACT_RELU)
    res["d8"] = (_nchw(d8), grads["d8"])
    dw8, db8 = E.conv_wgrad(_cl(case["y4"], dev), _cl(grads["d8"], dev), pk8)
    res["w8"], res["b8"] = (dw8, grads["w8"]), (db8, grads["b8"])
    return res, np.abs(case["g"]).astype(np.float64).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["tiny", "odd", MULTI], ids=str)
def test_hip_each_entry_point_vs_restatement(dev, key):
    res, gsum = _entry_points(dev, key)
    for name, (got, ref) in res.items():
        if name == "b12":
            print("%s b12: %.2e of sum|g|" % (key, got.abs().item() / gsum))
            assert got.abs().item() <= 1e-6 * gsum
            continue
        err = _err(got, ref)
        print("%s %s: %.2e of the largest entry" % (key, name, err))
        assert err <= GRAD_TOL, (name, err)


def _wgrad_case(dev, N, T, H, W, Cin, Cout, k, s, p, seed):
    from mspi_amd import engine as E
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, T, H, W, generator=gen).clamp_min(0)
    To, Ho, Wo = [(e + 2 * pp - kk) // ss + 1 for e, kk, ss, pp in zip((T, H, W), k, s, p)]
    dy = torch.randn(N, Cout, To, Ho, Wo, generator=gen)
    pk = E.pack_conv(torch.zeros(Cout, Cin, *k), None, None, s, p, device=dev)
    ref_w = torch.nn.grad.conv3d_weight(x.double(), (Cout, Cin) + tuple(k), dy.double(), stride=s, padding=p)
    xc, dyc = _cl(x, dev), _cl(dy, dev)
    dw, db = E.conv_wgrad(xc, dyc, pk)
    return E.conv_wgrad_variant(xc, dyc, pk), _err(dw, ref_w), _err(db, dy.double().sum((0, 2, 3, 4)))


@pytest.mark.gpu
@pytest.mark.parametrize("M", sorted(WGRAD_BOUNDARY))
def test_hip_wgrad_either_side_of_the_slice_constants(dev, M):
    """36 -> 12 channels: a second, partly filled channel block and fewer than 32 output channels; both variant codes."""
    N, H, W = WGRAD_BOUNDARY[M]
    assert N * H * W == M
    code, ew, eb = _wgrad_case(dev, N, 1, H, W, 36, 12, seed=M, **R10)
    print("M = %d: variant %d, dW %.2e, db %.2e" % (M, code, ew, eb))
    assert code == (SLICE_BIG if M >= BIG_M else SLICE) and ew <= GRAD_TOL and eb <= GRAD_TOL


@pytest.mark.gpu
def test_hip_wgrad_other_geometries(dev):
    """A (3,3,3) conv with stride 2 and padding, and the temporal (4,1,1)/4 conv on a width that is no multiple of 32."""
    for geom in (dict(N=2, T=5, H=9, W=7, Cin=8, Cout=4, k=(3, 3, 3), s=(1, 2, 2), p=(1, 1, 1)),
                 dict(N=3, T=8, H=5, W=7, Cin=44, Cout=32, **R8)):
        code, ew, eb = _wgrad_case(dev, seed=5, **geom)
        assert code == SLICE and ew <= GRAD_TOL and eb <= GRAD_TOL, (geom, ew, eb)


@pytest.mark.gpu
@pytest.mark.parametrize("M,Cc", [(m, 32) for m in sorted(C1_BOUNDARY)] + [(C1_ROWS - 1, 12), (C1_ROWS + 1, 64)])
def test_hip_conv_c1_bwd_either_side_of_the_workgroup_rows(dev, M, Cc):
    """Also 12 channels (three vectors per row: 85 rows per pass, one idle thread) and the widest, 64."""
    from mspi_amd import engine as E
    N, H, W = C1_BOUNDARY[M]
    gen = torch.Generator().manual_seed(M + Cc)
    y = torch.randn(N, Cc, H, W, generator=gen).clamp_min(0)
    dz = torch.randn(N, H, W, generator=gen)
    w = torch.randn(1, Cc, 1, 3, 3, generator=gen)
    w2, dz1 = w[:, :, 0].double(), dz[:, None].double()
    ref_d = torch.nn.grad.conv2d_input(y.shape, w2, dz1, padding=1) * (y > 0)
    ref_w = torch.nn.grad.conv2d_weight(y.double(), w2.shape, dz1, padding=1)[:, :, None]
    d, dw, db = E.conv_c1_bwd(_cl(y, dev), dz.to(dev), w.to(dev))
    errs = (_err(_nchw(d), ref_d), _err(dw, ref_w), abs(db.item() - dz.double().sum().item()) / dz.double().abs().sum().item())
    print("M = %d, C = %d: d %.2e, dW %.2e, db %.2e of sum|dz|" % (M, Cc, *errs))
    assert errs[0] <= GRAD_TOL and errs[1] <= GRAD_TOL and errs[2] <= 1e-6


def _dot(a, b):
    return (a.detach().double().cpu() * b.detach().double().cpu()).sum().item()


def _signed_like(ax, gen):
    """A random y for an adjoint identity <A x, y> = <x, A^T y>: uniform magnitudes in [0.5, 1.5) with the signs of A x.  The
    identity holds for every y; with this one the left side is a sum of non-negative terms, so an error bound relative to
    the value does not depend on how much a sum of random signs happens to cancel."""
    from mspi_amd import engine as E
    mag = (torch.rand(ax.buf.numel(), generator=gen) + 0.5).to(ax.buf.device)
    sign = torch.where(ax.buf < 0, -torch.ones_like(ax.buf), torch.ones_like(ax.buf))
    return E.CL(mag * sign, 0, ax.N, ax.T, ax.H, ax.W, ax.C, ax.ld)


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [2, 4, 8])
def test_hip_upsample_adjoint_identity(dev, factor):
    """<up(x), y> = <x, up_bwd(y)> on random x and y, on the device's own forward; without ReLU the two are adjoint maps.
    y has random magnitudes and the signs of up(x) (_signed_like), so 1e-5 of the value is a well-conditioned bound."""
    from mspi_amd import engine as E
    gen = torch.Generator().manual_seed(factor)
    # an independent random y, seed fixed: the bound is relative to the value, whatever cancels in it
    x = _cl(torch.randn(2, 32, 1, 5, 7, generator=gen), dev)
    y = _cl(torch.randn(2, 32, 1, 5 * factor, 7 * factor, generator=gen), dev)
    lhs, rhs = _dot(E.upsample(x, factor).buf, y.buf), _dot(x.buf, E.upsample_bwd(y, factor).buf)
    print("factor %d, independent y: %.9g vs %.9g" % (factor, lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (factor, lhs, rhs)
    for N, T, H, W, Cc in ((2, 1, 5, 7, 32), (1, 3, 1, 6, 4), (1, 1, 9, 1, 8)):
        x = _cl(torch.randn(N, Cc, T, H, W, generator=gen), dev)
        ux = E.upsample(x, factor)
        y = _signed_like(ux, gen)
        lhs, rhs = _dot(ux.buf, y.buf), _dot(x.buf, E.upsample_bwd(y, factor).buf)
        assert lhs > 0 and abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (factor, N, T, H, W, lhs, rhs)
        # with the ReLU: <relu(up(x)), y> = <x, up_bwd(y; mask of u)> since relu(v) = mask * v
        u = E.upsample(x, factor, act=E.ACT_RELU)
        lhs, rhs = _dot(u.buf, y.buf), _dot(x.buf, E.upsample_bwd(y, factor, u=u, act=E.ACT_RELU).buf)
        assert lhs > 0 and abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (factor, "relu", lhs, rhs)


@pytest.mark.gpu
def test_hip_conv_data_gradient_adjoint_identity(dev):
    """<conv(x), y> = <x, conv_T(y)> for readout[10] without bias and activation: conv_T is the same conv with w'[ci][-tap][co]."""
    from mspi_amd import engine as E
    case = _restated("odd")[0]
    w10 = torch.from_numpy(case["w10"]).to(dev)
    fwd = E.pack_conv(w10, None, None, (1, 1, 1), (0, 1, 1), E.ACT_NONE)
    bwd = E.pack_conv(w10.transpose(0, 1).flip(3, 4), None, None, (1, 1, 1), (0, 1, 1), E.ACT_NONE, prec=E.PREC_F32)
    gen = torch.Generator().manual_seed(10)
    x, y = _cl(torch.randn(2, 32, 20, 28, generator=gen), dev), _cl(torch.randn(2, 32, 20, 28, generator=gen), dev)
    lhs, rhs = _dot(E.conv(x, fwd).buf, y.buf), _dot(x.buf, E.conv(y, bwd).buf)       # an independent random y, seed fixed
    print("conv, independent y: %.9g vs %.9g" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    for N, H, W in ((2, 20, 28), (1, 9, 33)):
        x = _cl(torch.randn(N, 32, H, W, generator=gen), dev)
        cx = E.conv(x, fwd)
        y = _signed_like(cx, gen)
        lhs, rhs = _dot(cx.buf, y.buf), _dot(x.buf, E.conv(y, bwd).buf)
        assert lhs > 0 and abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (lhs, rhs)


@pytest.mark.gpu
def test_hip_backward_is_bitwise_repeatable(dev):
    """Each entry point twice on (2, 8, 12), and a third time after an unrelated launch."""
    first = {k: v[0].clone() for k, v in _entry_points(dev, MULTI)[0].items()}
    second = _entry_points(dev, MULTI)[0]
    a = torch.randn(512, 512, device=dev)
    (a @ a).sum().item()
    third = _entry_points(dev, MULTI)[0]
    for k in first:
        assert torch.equal(first[k], second[k][0]) and torch.equal(first[k], third[k][0]), k


def _device_tail(dev, case, y4_grad=True, g_scale=1.0):
    """ReadoutTail on a case: (out, grads by name, mask_u, mask_10) with the masks of the device's own forward."""
    from mspi_amd import engine as E
    from mspi_amd.autograd import ReadoutTail, readout_tail_forward
    y4 = torch.from_numpy(case["y4"]).permute(0, 2, 3, 4, 1).contiguous().to(dev).requires_grad_(y4_grad)
    params = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in RT.PARAMS]
    out = ReadoutTail.apply(y4, *params)
    assert out.requires_grad and out.grad_fn is not None
    out.backward(torch.from_numpy(case["g"]).to(dev) * g_scale)
    B, _, h, w, _ = y4.shape
    with torch.no_grad():
        same, u, y10 = readout_tail_forward(E.CL(y4.detach().view(-1), 0, B, 4, h, w, 64, 64), *_tail_packs(case, dev))
    assert torch.equal(same, out.detach())                     # the same launches: bit-identical to the inference path
    grads = dict(zip(RT.PARAMS, (p.grad for p in params)))
    grads["y4"] = None if y4.grad is None else y4.grad.permute(0, 4, 1, 2, 3)
    return out.detach(), grads, (_nchw(u) > 0).cpu(), (_nchw(y10) > 0).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_readout_tail_end_to_end_vs_fixture(dev, name):
    gold = _gold()
    case, saved, own = _restated(name)
    out, grads, mask_u, mask_10 = _device_tail(dev, case)
    assert (out.double().cpu() - torch.from_numpy(gold["%s_out" % name])).abs().max().item() <= 1e-4
    # mask rule: the device may sit on the other side of a ReLU kink only where the float64 pre-activation is within 1e-5
    for mask, pre in ((mask_u, saved["up"]), (mask_10, saved["p10"])):
        differ = mask != (pre > 0)
        worst = pre[differ].abs().max().item() if differ.any() else 0.0
        print("%s: %d mask cells differ, largest |pre-activation| among them %.1e" % (name, int(differ.sum()), worst))
        assert worst <= 1e-5
    ref = RT.backward(case["y4"], case, saved, case["g"], masks=(mask_u, mask_10))
    if name == "tiny":                                          # kink-free: the masks agree and the fixture itself is the reference
        assert torch.equal(mask_u, saved["up"] > 0) and torch.equal(mask_10, saved["p10"] > 0)
        ref = {k: torch.from_numpy(gold["%s_d_%s" % (name, k)]) for k in NAMES}
    gsum = np.abs(case["g"]).astype(np.float64).sum()
    for k in NAMES:
        if k == "b12":
            print("%s b12: %.2e of sum|g|" % (name, grads[k].abs().item() / gsum))
            assert grads[k].abs().item() <= 1e-6 * gsum
            continue
        err = _err(grads[k], ref[k])
        print("%s d %s: %.2e of the largest entry" % (name, k, err))
        assert err <= GRAD_TOL, (k, err)


@pytest.mark.gpu
@pytest.mark.parametrize("exp", [-20, -30, 12])
def test_hip_readout_tail_gradients_at_the_scale_of_a_loss(dev, exp):
    """The upstream gradient of a training loss is tiny (SalLoss at 8 x 224 x 384: 1e-5 and below), far under the window in
    which an f16x3 activation split is exact.  The backward is linear in g, so with g scaled by a power of two every
    gradient must be the scaled reference, to the same 2e-5, and must stay within rounding of the scaled unit-g result."""
    case, saved, _ = _restated("odd")
    scale = 2.0 ** exp
    _, unit, mask_u, mask_10 = _device_tail(dev, case)
    _, grads, mu2, m2 = _device_tail(dev, case, g_scale=scale)
    assert torch.equal(mask_u, mu2) and torch.equal(mask_10, m2)
    ref = RT.backward(case["y4"], case, saved, case["g"], masks=(mask_u, mask_10))
    for k in NAMES:
        if k == "b12":
            continue
        err, drift = _err(grads[k], ref[k] * scale), _err(grads[k], unit[k].double().cpu() * scale)
        print("g x 2^%d, d %s: %.2e of the largest entry (%.2e from the scaled unit-g result)" % (exp, k, err, drift))
        assert err <= GRAD_TOL and drift <= 2e-6, (k, err, drift)


@pytest.mark.gpu
def test_hip_readout_tail_skips_the_feature_gradient(dev):
    case = _restated("odd")[0]
    _, with_y4, _, _ = _device_tail(dev, case, y4_grad=True)
    _, grads, _, _ = _device_tail(dev, case, y4_grad=False)
    assert grads["y4"] is None and with_y4["y4"] is not None
    for k in RT.PARAMS:
        assert torch.equal(grads[k], with_y4[k]), k
    # frozen parameters get none either
    from mspi_amd.autograd import ReadoutTail
    y4 = torch.from_numpy(case["y4"]).permute(0, 2, 3, 4, 1).contiguous().to(dev)
    params = [torch.from_numpy(case[k]).to(dev).requires_grad_(k in ("w12", "b12")) for k in RT.PARAMS]
    ReadoutTail.apply(y4, *params).backward(torch.from_numpy(case["g"]).to(dev))
    assert [p.grad is not None for p in params] == [False, False, False, False, True, True]
    assert torch.equal(params[4].grad, with_y4["w12"])


def _build(golden_dir, case, name, cls, dev):
    from mspi_amd import testing as T
    from mspi_amd.model import model_utils as pm
    g = np.load(os.path.join(golden_dir, case + ".npz"))
    cfg = T.golden_cfg(g, name)
    make = lambda: T.condition_(T.seeded(lambda: getattr(pm, cls)(cfg), int(g["seed"])), name)      # noqa: E731
    H, W = T.golden_hw(g)
    clips, audio = T.synth_inputs(int(g["batch"]), 16, H, W, Wa=int(g["wa"]), seed=int(g["seed"]), device=dev)
    return g, cfg, make, clips, audio


def _batches(clips, audio, n, sound):
    """n batches of different clips (frames rolled in time) that share one density map: the steps then pull the tail the same
    way, so the loss of a second pass over them must come out lower if the gradients point downhill."""
    out = []
    label = torch.from_numpy(S.make_case(clips.shape[0], clips.shape[3], clips.shape[4], 900)[1])
    for i in range(n):
        c = clips.roll(i, dims=2) if i else clips
        out.append((c, audio, label) if sound else (c, label))
    return out


@pytest.mark.gpu
def test_hip_whole_model_trains_its_tail(dev, golden_dir):
    from mspi_amd import engine_train as ET
    from mspi_amd import metrics as M
    g, cfg, make, clips, audio = _build(golden_dir, "av_x3dl_64", "x3dl", "AudioVisualSaliencyModel", dev)
    m = make().to(dev)
    off, _ = m(clips, audio)
    assert (off.cpu() - torch.as_tensor(g["out"])).abs().max().item() < MAP_TOL and not off.requires_grad
    m.trainable("readout_tail")
    with torch.no_grad():
        quiet, _ = m(clips, audio)
    assert torch.equal(quiet, off) and not quiet.requires_grad
    loud, aux = m(clips, audio)
    assert loud.requires_grad and torch.equal(loud.detach(), off) and not aux.requires_grad
    start = {k: v.clone() for k, v in m.state_dict().items()}
    tail = set(RT.STATE_KEYS.values())
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0)
    assert sum(len(gr["params"]) for gr in opt.param_groups) == 6
    batches = _batches(clips, audio, 2, True)
    cfg.DATA.USE_SOUND = True
    first = ET.train_one_epoch(m, M.SalLoss(), batches, opt, dev, 0, cfg)
    second = ET.train_one_epoch(m, M.SalLoss(), batches, opt, dev, 1, cfg)
    print("whole model: loss %.5f -> %.5f" % (first["loss"], second["loss"]))
    assert second["loss"] < first["loss"] and second["grad_norm"] > 0
    assert not m.training                                       # frozen_encoder() put the whole model into eval()
    for k, v in m.state_dict().items():
        if k in tail:
            assert not torch.equal(v, start[k]), k
        else:
            assert torch.equal(v, start[k]), k
    # the unusual order: grad forward, a no_grad peek (repacks), backward, step, no_grad forward -- the last one must see the step
    out, _ = m(clips, audio)
    with torch.no_grad():
        peek, _ = m(clips, audio)
    opt.zero_grad()
    M.SalLoss()(out, batches[0][2].to(dev)).backward()
    opt.step()
    with torch.no_grad():
        after, _ = m(clips, audio)
    assert torch.equal(peek, out.detach()) and not torch.equal(after, peek)
    # a fresh model from the state dict gives the trained model's inference output: no stale pack on either side
    with torch.no_grad():
        trained, _ = m(clips, audio)
    assert not torch.equal(trained, off)
    fresh = make()
    fresh.load_state_dict(m.state_dict())
    again, _ = fresh.to(dev)(clips, audio)
    assert torch.equal(again, trained)
    m.trainable(None)
    plain, _ = m(clips, audio)
    assert torch.equal(plain, trained) and not plain.requires_grad
    # without the switch the model is the inference engine it was: the loop's model.train() is refused by the forward
    from mspi_amd._lib import MspiError
    with pytest.raises(MspiError, match="inference engine"):
        ET.train_one_epoch(m, M.SalLoss(), batches[:1], opt, dev, 2, cfg)


@pytest.mark.gpu
def test_hip_visual_model_trains_its_tail(dev, golden_dir):
    from mspi_amd import engine_train as ET
    from mspi_amd import metrics as M
    g, cfg, make, clips, _ = _build(golden_dir, "vis_x3dl_64", "x3dl", "VisualSaliencyModel", dev)
    m = make().to(dev)
    off, zero = m(clips)
    assert zero == 0 and (off.cpu() - torch.as_tensor(g["out"])).abs().max().item() < MAP_TOL
    m.trainable("readout_tail")
    start = {k: v.clone() for k, v in m.state_dict().items()}
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0)
    cfg.DATA.USE_SOUND = False
    stats = ET.train_one_epoch(m, M.SalLoss(), _batches(clips, None, 1, False), opt, dev, 0, cfg)
    assert np.isfinite(stats["loss"])
    tail = set(RT.STATE_KEYS.values())
    for k, v in m.state_dict().items():
        assert torch.equal(v, start[k]) == (k not in tail), k
    with torch.no_grad():
        trained, _ = m(clips)
    fresh = make()
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(fresh.to(dev)(clips)[0], trained) and not torch.equal(trained, off)
