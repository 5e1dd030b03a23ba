"""AUC-Judd, shuffled AUC and information gain (utils/compute_saliency_metrics.py:111-308 of the reference).

Yardsticks: tests/golden/saliency_auc.npz holds small inputs, the injected jitter noise and the scores of the reference's
own functions (tools/gen_auc_golden.py); tests/saliency_auc_restate.py is the vectorised CPU restatement that the
generator pinned to the reference and that stands in for it on maps too large to commit.

Bounds.  AUC-Judd: the device counts are integers and exact, the only freedom is the summation order of the float64
trapezoid: n + 1 <= P terms of magnitude <= P / (P - n) <= 2 for n <= P / 2, so 2 * P * 2^-53 = 7e-11 at P = 307200;
tested at 1e-9 absolute.  Shuffled AUC: counts exact, score 1e-12 absolute (the reference averages 100 equal doubles).
IG: the sibling kernel's yardstick (tests/test_metrics.py), relative 2e-5 with a 1e-3 floor on the fixture, 1e-4 at full
size.  NaN is a value: it must appear exactly where the yardstick has it, all other entries are compared."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import saliency_auc_restate as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_saliency_auc_ws_bytes", "mspi_saliency_auc_judd", "mspi_saliency_sauc_counts", "mspi_saliency_ig")
JUDD_CASES = ("cont", "u8", "u8_jitter", "dense", "dense_jitter", "nofix", "const")
SAUC_CASES = ("pin", "wide", "square", "noother", "nofix")


def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "saliency_auc.npz"))
    return {k: z[k] for k in z.files}


def _close(got, ref, tol):
    """NaN exactly where ref has it, every other entry within tol; returns the largest difference for the message."""
    got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(ref, np.float64))
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    ok = ~np.isnan(ref)
    err = float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0
    assert err <= tol, (err, got, ref)
    return err


def _bits_equal(a, b):
    return a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["judd_cases"]) == JUDD_CASES and tuple(g["sauc_cases"]) == SAUC_CASES
    nan_cases = [c for c in JUDD_CASES if math.isnan(float(g["judd_%s_score" % c]))]
    assert nan_cases == ["nofix", "const"]
    assert [c for c in SAUC_CASES if math.isnan(float(g["sauc_%s_score" % c]))] == ["nofix"]
    assert g["judd_dense_fix"].mean() >= 0.25 and len(np.unique(g["judd_u8_sal"])) <= 256
    for c in JUDD_CASES:
        assert g["judd_%s_sal" % c].dtype == np.float32 and g["judd_%s_fix" % c].dtype == np.uint8
    # the >= / > pin: fixations and other-fixation reads sit exactly on float32(k / 10)
    s, gt, other = g["sauc_pin_sal"], g["sauc_pin_gt"], g["sauc_pin_other"]
    tenths = (np.arange(1, 10) / 10).astype(np.float32)
    assert s.min() == 0.0 and s.max() == 1.0 and np.isin(s[gt == 1], tenths).all()
    x, y = np.where(other == 1)
    k = x * s.shape[0] + y
    assert np.isin(s[k % s.shape[0] - 1, k // s.shape[0]], np.concatenate([tenths, [0, 1]]).astype(np.float32)).mean() > 0.9


def test_restatement_matches_reference_scores():
    g = _gold()
    for c in JUDD_CASES:
        got, n = A.auc_judd(g["judd_%s_sal" % c], g["judd_%s_fix" % c], g.get("judd_%s_noise" % c))
        _close(got, g["judd_%s_score" % c], 1e-12)
        assert n == int(g["judd_%s_fix" % c].sum())
    for c in SAUC_CASES:
        _close(A.auc_shuff(g["sauc_%s_sal" % c], g["sauc_%s_gt" % c], g["sauc_%s_other" % c]), g["sauc_%s_score" % c], 1e-12)
    per = A.ig_per_sample(g["ig_pred"], g["ig_gt"], g["ig_base"])
    assert torch.equal(per, torch.from_numpy(g["ig_per_sample"]))
    assert abs(per.mean().item() - float(g["ig_ref_mean"])) < 1e-6


def test_restatement_jitter_changes_a_quantised_map():
    g = _gold()
    assert abs(float(g["judd_u8_score"]) - float(g["judd_u8_jitter_score"])) > 1e-3


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


def test_argument_validation_without_gpu():
    from mspi_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # workspace query: pure host arithmetic; room for L thresholds as double and L + 1 counters per map
    assert lib.mspi_saliency_auc_ws_bytes(0, 100) == 0 and lib.mspi_saliency_auc_ws_bytes(2, 1) == 0
    assert lib.mspi_saliency_auc_ws_bytes(1, 100) >= 100 * 8 + 101 * 4
    assert lib.mspi_saliency_auc_ws_bytes(8, 480 * 640) == 8 * lib.mspi_saliency_auc_ws_bytes(1, 480 * 640)
    for bad in ((None, 0, p, p, p, p, 1, 100), (p, 0, None, p, p, p, 1, 100), (p, 0, p, None, p, p, 1, 100),
                (p, 1, p, p, None, p, 1, 100), (p, 1, p, p, p, None, 1, 100), (p, 0, p, p, p, p, 0, 100),
                (p, 0, p, p, p, p, -3, 100), (p, 0, p, p, p, p, 1, 1), (p, 1, p, p, p, p, 1, 0)):
        assert lib.mspi_saliency_auc_judd(*bad, None) == -1
        assert b"mspi_saliency_auc_judd" in lib.mspi_last_error()
    for bad in ((None, p, p, p, 1, 4, 8), (p, None, p, p, 1, 4, 8), (p, p, None, p, 1, 4, 8), (p, p, p, None, 1, 4, 8),
                (p, p, p, p, 0, 4, 8), (p, p, p, p, 1, 0, 8), (p, p, p, p, 1, 1, 1)):
        assert lib.mspi_saliency_sauc_counts(*bad, None) == -1
    assert lib.mspi_saliency_sauc_counts(p, p, p, p, 1, 8, 4, None) == -1          # H > W: upstream raises IndexError
    assert b"H = 8 > W = 4" in lib.mspi_last_error()
    for bad in ((None, p, p, p, 1, 100), (p, None, p, p, 1, 100), (p, p, None, p, 1, 100), (p, p, p, None, 1, 100),
                (p, p, p, p, 0, 100), (p, p, p, p, 1, 1)):
        assert lib.mspi_saliency_ig(*bad, None) == -1
        assert b"mspi_saliency_ig" in lib.mspi_last_error()


def test_python_entry_points_refuse_cpu_tensors_and_shape_mismatch():
    from mspi_amd import metrics as M
    from mspi_amd._lib import MspiError
    a = torch.rand(1, 8, 12)
    for call in (lambda: M.auc_judd(a, a), lambda: M.auc_shuff(a, a, a), lambda: M.ig(a, a, a),
                 lambda: M.auc_judd_per_sample(a, a, jitter=False)):
        with pytest.raises(MspiError, match="no CPU fallback"):
            call()


def test_sauc_host_steps_match_restatement():
    """The product's host part of shuffled AUC (round, sort, trapezoid) on the fixture's counts."""
    from mspi_amd import metrics as M
    g = _gold()
    for c in SAUC_CASES:
        counts = A.sauc_counts(g["sauc_%s_sal" % c], g["sauc_%s_gt" % c], g["sauc_%s_other" % c])
        _close(M._sauc_score([int(v) for v in counts]), g["sauc_%s_score" % c], 1e-12)


# ------------------------------------------------------------------------------------------------------------- GPU
def _seeded_batch(B, H, W, nfix, seed, levels=None):
    """Seeded CPU inputs: smooth maps with a little noise (levels: quantised to that many values, like postprocess_u8's
    output), fixation maps with exactly nfix[b] fixations, other-fixation maps, densities, baselines, jitter noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    sal = np.zeros((B, H, W), np.float32)
    for b in range(B):
        for _ in range(5):
            cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(H / 16, H / 4)
            sal[b] += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32)
        sal[b] += rng.random((H, W), dtype=np.float32) * 0.02
    if levels:
        sal = np.round(sal / sal.max() * (levels - 1)).astype(np.float32)
    fix = np.zeros((B, H * W), np.float32)
    other = np.zeros((B, H * W), np.float32)
    for b in range(B):
        fix[b, rng.choice(H * W, size=nfix[b], replace=False)] = 1
        other[b, rng.choice(H * W, size=1497, replace=False)] = 1
    dens = rng.random((B, H, W), dtype=np.float32) ** 4
    base = rng.random((B, H, W), dtype=np.float32) + 0.1
    noise = rng.random((B, H, W))
    return sal, fix.reshape(B, H, W), other.reshape(B, H, W), dens, base, noise


@pytest.mark.gpu
def test_hip_auc_judd_vs_fixture(dev):
    from mspi_amd import metrics as M
    g = _gold()
    for c in JUDD_CASES:
        sal = torch.from_numpy(g["judd_%s_sal" % c])[None].to(dev)
        fix = torch.from_numpy(g["judd_%s_fix" % c])[None].to(dev)
        noise = g.get("judd_%s_noise" % c)
        jit = False if noise is None else torch.from_numpy(noise)[None].to(dev)
        score, n = M.auc_judd_per_sample(sal, fix, jitter=jit, return_counts=True)
        assert score.dtype == torch.float64 and n.dtype == torch.int32
        err = _close(score.cpu().numpy(), [float(g["judd_%s_score" % c])], 1e-9)
        print("auc_judd %-13s |hip - reference| = %.2e" % (c, err))
        assert n.item() == int(g["judd_%s_fix" % c].sum())
        _close(M.auc_judd(sal, fix, jitter=jit).item(), float(g["judd_%s_score" % c]), 1e-9)


@pytest.mark.gpu
def test_hip_auc_judd_default_jitter_is_seeded_and_float64(dev):
    """jitter=True draws float64 noise on the device from the given generator: repeatable, and on a quantised map
    different from jitter=False (the reason the jitter path exists)."""
    from mspi_amd import metrics as M
    g = _gold()
    sal = torch.from_numpy(g["judd_u8_sal"])[None].to(dev)
    fix = torch.from_numpy(g["judd_u8_fix"])[None].to(dev)
    a = M.auc_judd(sal, fix, generator=torch.Generator(device=dev).manual_seed(7))
    b = M.auc_judd(sal, fix, jitter=True, generator=torch.Generator(device=dev).manual_seed(7))
    assert _bits_equal(a, b) and a.dtype == torch.float64
    noise = torch.rand(sal.shape, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    ref, _ = A.auc_judd(g["judd_u8_sal"], g["judd_u8_fix"], noise[0].cpu().numpy())
    _close(a.item(), ref, 1e-9)
    assert abs(a.item() - M.auc_judd(sal, fix, jitter=False).item()) > 1e-3


@pytest.mark.gpu
def test_hip_sauc_vs_fixture(dev):
    from mspi_amd import metrics as M
    g = _gold()
    for c in SAUC_CASES:
        s, gt, other = (torch.from_numpy(g["sauc_%s_%s" % (c, k)].astype(np.float32))[None].to(dev) for k in ("sal", "gt", "other"))
        counts = M.sauc_counts(s, gt, other).cpu().numpy()
        ref_counts = A.sauc_counts(g["sauc_%s_sal" % c], g["sauc_%s_gt" % c], g["sauc_%s_other" % c])
        assert np.array_equal(counts[0], ref_counts), (c, counts[0], ref_counts)
        _close(M.auc_shuff_per_sample(s, gt, other).cpu().numpy(), [float(g["sauc_%s_score" % c])], 1e-12)
        _close(M.auc_shuff(s, gt, other, splits=3, stepsize=0.5).item(), float(g["sauc_%s_score" % c]), 1e-12)


@pytest.mark.gpu
def test_hip_sauc_refuses_tall_maps(dev):
    from mspi_amd import metrics as M
    from mspi_amd._lib import MspiError
    t = torch.rand(1, 12, 8, device=dev)
    with pytest.raises(MspiError, match="H = 12 > W = 8"):
        M.auc_shuff(t, t, t)
    with pytest.raises(MspiError, match="equal"):
        M.auc_judd(torch.rand(1, 6, 8, device=dev), t)


@pytest.mark.gpu
def test_hip_ig_vs_fixture(dev):
    from mspi_amd import metrics as M
    g = _gold()
    p, d, b = (torch.from_numpy(g[k]).to(dev) for k in ("ig_pred", "ig_gt", "ig_base"))
    got = M.ig_per_sample(p, d, b)
    ref = torch.from_numpy(g["ig_per_sample"])
    assert ((got.cpu() - ref).abs() / ref.abs().clamp_min(1e-3)).max().item() < 2e-5
    m = float(g["ig_ref_mean"])
    assert abs(M.ig(p, d, b).item() - m) < 2e-5 * max(1.0, abs(m))
    assert _bits_equal(got, M.ig_per_sample(p, d, b))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(224, 384), (480, 640)])
def test_hip_full_size_batch_vs_restatement(dev, H, W):
    """8 maps whose fixation counts differ, one of them without any (NaN in place, the others unaffected): float32 path on
    continuous and on 256-level maps, float64 path with injected noise; shuffled-AUC counts and scores; IG.  Every launch
    twice, bitwise equal."""
    from mspi_amd import metrics as M
    nfix = [300, 50, 0, 1000, 328, 2000, 17, 4000]
    for levels in (None, 256):
        sal, fix, other, dens, base, noise = _seeded_batch(8, H, W, nfix, seed=H + (levels or 0), levels=levels)
        ts, tf, to, td, tb = (torch.from_numpy(a).to(dev) for a in (sal, fix, other, dens, base))
        tn = torch.from_numpy(noise).to(dev)
        for jit, nz in ((False, [None] * 8), (tn, noise)):
            score, n = M.auc_judd_per_sample(ts, tf, jitter=jit, return_counts=True)
            score2, n2 = M.auc_judd_per_sample(ts, tf, jitter=jit, return_counts=True)
            assert _bits_equal(score, score2) and torch.equal(n, n2)
            ref = [A.auc_judd(sal[b], fix[b], nz[b])[0] for b in range(8)]
            assert math.isnan(ref[2]) and sum(math.isnan(r) for r in ref) == 1
            err = _close(score.cpu().numpy(), ref, 1e-9)
            print("auc_judd %dx%d levels=%s f64=%s: max |hip - restatement| = %.2e" % (H, W, levels, jit is not False, err))
            assert n.cpu().tolist() == nfix
            _close(M.auc_judd(ts, tf, jitter=jit).item(), A.nanmean(ref)[0], 1e-9)
        counts = M.sauc_counts(ts, tf, to)
        assert torch.equal(counts, M.sauc_counts(ts, tf, to))
        ref_counts = np.stack([A.sauc_counts(sal[b], fix[b], other[b]) for b in range(8)])
        assert np.array_equal(counts.cpu().numpy(), ref_counts)
        ref = [A.sauc_from_counts(c) for c in ref_counts]
        assert math.isnan(ref[2]) and sum(math.isnan(r) for r in ref) == 1
        _close(M.auc_shuff_per_sample(ts, tf, to).cpu().numpy(), ref, 1e-12)
        _close(M.auc_shuff(ts, tf, to).item(), A.nanmean(ref)[0], 1e-12)
        if levels is None:
            got = M.ig_per_sample(ts, td, tb)
            assert _bits_equal(got, M.ig_per_sample(ts, td, tb))
            ref = A.ig_per_sample(sal, dens, base)
            assert ((got.cpu() - ref).abs() / ref.abs().clamp_min(1e-3)).max().item() < 1e-4


@pytest.mark.gpu
def test_hip_auc_judd_more_fixations_than_the_lds_list(dev):
    """The thresholds of a map are sorted and searched in LDS up to 4096 of them; beyond that in the caller's workspace.
    4097 is the first count on that path, 100000 (a third of the pixels) a dense one; a sparse map shares the batch."""
    from mspi_amd import metrics as M
    H, W, nfix = 480, 640, [4097, 100000, 300, 4096]
    sal, fix, _, _, _, noise = _seeded_batch(4, H, W, nfix, seed=99, levels=256)
    ts, tf, tn = torch.from_numpy(sal).to(dev), torch.from_numpy(fix).to(dev), torch.from_numpy(noise).to(dev)
    for jit, nz in ((False, [None] * 4), (tn, noise)):
        score, n = M.auc_judd_per_sample(ts, tf, jitter=jit, return_counts=True)
        assert n.cpu().tolist() == nfix
        _close(score.cpu().numpy(), [A.auc_judd(sal[b], fix[b], nz[b])[0] for b in range(4)], 1e-9)
        assert _bits_equal(score, M.auc_judd_per_sample(ts, tf, jitter=jit))


@pytest.mark.gpu
def test_hip_launches_inside_graph_capture(dev):
    """No synchronisation, allocation or copy inside the entry points: captured and replayed they give the eager result."""
    from mspi_amd import metrics as M
    nfix = [300, 0, 5000, 77]
    sal, fix, other, dens, base, noise = _seeded_batch(4, 224, 384, nfix, seed=5)
    ts, tf, to, td, tb = (torch.from_numpy(a).to(dev) for a in (sal, fix, other, dens, base))
    tn = torch.from_numpy(noise).to(dev)

    def launches():
        return (M.auc_judd_per_sample(ts, tf, jitter=False), M.auc_judd_per_sample(ts, tf, jitter=tn),
                M.sauc_counts(ts, tf, to), M.ig_per_sample(ts, td, tb))
    eager = launches()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = launches()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        assert _bits_equal(e, c)
    assert math.isnan(eager[0][1].item()) and not math.isnan(eager[0][0].item())


@pytest.mark.gpu
def test_sal_eval_over_two_batches(dev):
    from mspi_amd import metrics as M
    from oracle import restate as R
    H, W = 96, 128
    batches = [_seeded_batch(3, H, W, [40, 0, 200], seed=1), _seeded_batch(2, H, W, [90, 10], seed=2)]
    ev = M.SalEval(jitter=False)
    per = {k: [] for k in M.SalEval.KEYS}
    for sal, fix, other, dens, base, _ in batches:
        logmap = torch.log_softmax(torch.from_numpy(sal).flatten(1) * 3, 1).view(-1, H, W)
        ev.update(logmap.to(dev), torch.from_numpy(dens).to(dev), torch.from_numpy(fix).to(dev), torch.from_numpy(other).to(dev),
                  torch.from_numpy(base).to(dev))
        # the map SalEval scores is torch's float32 exp on the device; AUC is a rank statistic, so the yardstick gets the same bits
        s = logmap.to(dev).exp().cpu()
        four = R.saliency_metrics(s, torch.from_numpy(dens), torch.from_numpy(fix))
        for i, k in enumerate(("kl", "cc", "sim", "nss")):
            per[k] += four[:, i].double().tolist()
        per["auc_j"] += [A.auc_judd(s[b].numpy(), fix[b])[0] for b in range(len(sal))]
        per["s_auc"] += [A.auc_shuff(s[b].numpy(), fix[b], other[b]) for b in range(len(sal))]
        per["ig"] += A.ig_per_sample(s, fix, base).double().tolist()
    res = ev.result()
    assert set(res) == set(M.SalEval.KEYS)
    for k in M.SalEval.KEYS:
        mean, n_nan = A.nanmean(per[k])
        assert ev.nan[k] == n_nan and ev.count[k] == 5 - n_nan, (k, ev.nan[k], n_nan)
        tol = {"auc_j": 1e-9, "s_auc": 1e-12}.get(k, 1e-4 * max(1.0, abs(mean)))
        assert abs(res[k] - mean) <= tol, (k, res[k], mean)
    assert ev.nan["auc_j"] == 1 and ev.nan["s_auc"] == 1 and ev.nan["nss"] == 1
    # without fixations only the density metrics are fed
    ev2 = M.SalEval()
    ev2.update(logmap.to(dev), torch.from_numpy(dens).to(dev))
    assert set(ev2.result()) == {"kl", "cc", "sim"}


@pytest.mark.gpu
def test_validation_one_epoch_matches_model_plus_salloss(dev):
    from mspi_amd import metrics as M
    from mspi_amd import testing as T
    from mspi_amd.model.model_utils import AudioVisualSaliencyModel
    size = 64
    cfg = T.make_cfg("x3dl", num_aud_tokens=36, num_vis_tokens=16 * (size // 32) ** 2)
    model = T.seeded(lambda: AudioVisualSaliencyModel(cfg), 0).to(dev)
    loader, extended = [], []
    for seed in (0, 1):
        clips, audio = T.synth_inputs(2, 16, size, size, Wa=111, seed=seed)
        _, fix, other, dens, base, _ = _seeded_batch(2, size, size, [30, 12], seed=seed)
        loader.append((clips, audio, torch.from_numpy(dens)))
        extended.append((clips, audio, torch.from_numpy(dens), torch.from_numpy(fix), torch.from_numpy(other)))
    assert cfg.DATA.USE_SOUND
    got = M.validation_one_epoch(model, loader, dev, cfg)
    assert set(got) == {"loss", "kld", "cc", "sim"}                       # engine_train.py:116-119
    crit, vals, ev = M.SalLoss(), {k: [] for k in ("loss", "kl", "cc", "sim")}, M.SalEval()
    with torch.no_grad():
        for (clips, audio, dens), ext in zip(loader, extended):
            out, _ = model(clips.to(dev), audio.to(dev))
            assert out.shape == dens.shape
            before = {k: crit.log[k].sum for k in ("kl", "cc", "sim")}
            vals["loss"].append(crit(out, dens.to(dev)).item())
            for k in ("kl", "cc", "sim"):
                vals[k].append(crit.log[k].sum - before[k])
            ev.update(out, dens.to(dev), ext[3].to(dev), ext[4].to(dev))
    for key, k in (("loss", "loss"), ("kld", "kl"), ("cc", "cc"), ("sim", "sim")):
        assert abs(got[key] - sum(vals[k]) / 2) <= 1e-6 * max(1.0, abs(got[key])), (key, got[key], vals[k])
    got2 = M.validation_one_epoch(model, extended, dev, cfg)
    assert set(got2) == {"loss", "kld", "cc", "sim", "nss", "auc_j", "s_auc"}
    for key in ("loss", "kld", "cc", "sim"):
        assert abs(got2[key] - got[key]) <= 1e-6 * max(1.0, abs(got[key]))
    ref = ev.result()
    for key in ("nss", "s_auc"):
        assert abs(got2[key] - ref[key]) <= 1e-6 * max(1.0, abs(ref[key]))
    assert 0.0 <= got2["auc_j"] <= 1.0                                     # default jitter: unseeded noise, value in range
