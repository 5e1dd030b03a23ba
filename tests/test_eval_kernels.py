"""saliency_metrics_kernel and saliency_ig_kernel (csrc/metrics.hip) against float64.

Yardstick: tests/saliency_metrics_restate.py, the reference's kldiv / cc / similarity / nss / ig term by term in
float64.  The CPU tests pin it to the reference's own float32 results in tests/golden (relative distance measured when
this module was written: 3.1e-6 on the four metrics, whose smallest value is 1.3e-3, and 1.8e-7 on IG; its float32
evaluation reproduces both fixtures bit for bit).

Shapes: batch 3 and map sizes either side of the kernel's stride of 1024 threads (one partial wave, 1023 / 1024 / 1025,
a prime, 2049, 4095, a ragged frame-like 48 x 85); with odd L the second and third sample start at unaligned addresses.
Forms: saliency_metrics_restate.make_case.

Bar: 2e-5 of each value's own magnitude, no floor (the project's bar for these metrics, tests/test_sal_loss_grad.py).
The seed is chosen so that every compared float64 value is at least 0.05 in magnitude (asserted below), and a plain
float32 torch evaluation of the same formulas sits at least 4x inside the bar on every case (asserted below; measured
1.5e-7 .. 1.2e-6), so a failing kernel case is never mended with friendlier inputs.

Degenerate maps follow the restatement's NaN pattern.  torch.min hands a NaN on, so upstream's SIM of a constant
prediction, or against an all-zero density, is NaN; the kernel's fminf dropped the NaN and returned SIM = 1.0 there
until this module was written, and so did the chunked kernels of csrc/salloss.hip that report the same terms."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import saliency_auc_restate as A
import saliency_metrics_restate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5
MIN_MAG = 0.05
BIG = 1.0e6           # neighbours of the inputs: finite, and ruinous to any result that reads them
SHAPES = ((1, 63), (31, 33), (32, 32), (25, 41), (1, 1087), (3, 683), (45, 91), (48, 85))
CASES = [(H, W, form) for H, W in SHAPES for form in S.FORMS]
IG_CASES = [(H, W, form, gt) for H, W in SHAPES for form in S.FORMS if form != "nofix" for gt in ("gt", "fix")]
DEGENERATE = ("constant_pred", "zero_density", "no_fixations")


def _id(case):
    return "%dx%d-%s" % case[:3] + ("-%s" % case[3] if len(case) > 3 else "")


@functools.lru_cache(maxsize=None)
def _case(H, W, form):
    """Inputs and their float64 yardsticks, computed once: the case's maps, "ref" [3,4], "ig_pred" (probabilities) and
    "ig_gt" / "ig_fix" [3] (information gain with the density / the fixation map as ground truth)."""
    c = S.make_case(form, H, W)
    c["ref"] = S.metrics(c["pred"], c["gt"], c["fix"], c["is_log"])
    c["cols"] = 3 if c["fix"] is None else 4
    c["ig_pred"] = c["pred"].double().exp().float() if c["is_log"] else c["pred"]
    for name in ("gt", "fix"):
        if c[name] is not None:
            c["ig_" + name] = S.ig(c["ig_pred"], c[name], c["base"])
    return c


@functools.lru_cache(maxsize=None)
def _degenerate(kind):
    """The 25 x 41 `prob` case with one degenerate sample; (pred, gt, fix, float64 metrics, (sample, NaN columns))."""
    c = S.make_case("prob", 25, 41)
    pred, gt, fix = c["pred"].clone(), c["gt"].clone(), c["fix"].clone()
    if kind == "constant_pred":
        pred[1] = 0.5             # a power of two: its sums and its mean are exact in float32 and in float64
        where = (1, (1, 2))
    elif kind == "zero_density":
        gt[0] = 0.0
        where = (0, (0, 1, 2))    # SIM too: 0 / 0 in the normalised density, and torch.min hands the NaN on
    else:
        fix[2] = 0.0
        where = (2, (3,))
    return pred, gt, fix, S.metrics(pred, gt, fix), where


# ------------------------------------------------------------------------------------------------------------- CPU
def test_restatement_reproduces_the_reference_fixtures():
    """float64 against the reference's own float32 results: float32's distance (3.1e-6 and 1.8e-7 relative, measured),
    bars a factor 3 and 5 above; the float32 evaluation of the restatement gives the fixtures' bits."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "saliency_metrics.npz"))
    g = {k: torch.from_numpy(z[k]) for k in z.files}
    d = S.rel_err(g["per_sample"], S.metrics(g["pred"], g["gt"], g["fix"]))
    print("four metrics: float32 reference within %.2e of the float64 restatement" % d)
    assert d <= 1e-5
    assert torch.equal(S.metrics(g["pred"], g["gt"], g["fix"], dtype=torch.float32), g["per_sample"])
    none = S.metrics(g["pred"], g["gt"])
    assert torch.equal(none[:, :3], S.metrics(g["pred"], g["gt"], g["fix"])[:, :3]) and (none[:, 3] == 0).all()
    logged = S.metrics(g["pred"].double().log(), g["gt"], g["fix"], pred_is_log=True)
    assert S.rel_err(logged, S.metrics(g["pred"], g["gt"], g["fix"])) <= 1e-12
    z = np.load(os.path.join(ROOT, "tests", "golden", "saliency_auc.npz"))
    p, gt, b, ref = (torch.from_numpy(z[k]) for k in ("ig_pred", "ig_gt", "ig_base", "ig_per_sample"))
    d = S.rel_err(ref, S.ig(p, gt, b))
    print("information gain: float32 reference within %.2e of the float64 restatement" % d)
    assert d <= 1e-6
    assert torch.equal(S.ig(p, gt, b, dtype=torch.float32), ref) and torch.equal(A.ig_per_sample(p, gt, b), ref)
    assert abs(S.ig(p, gt, b).mean().item() - float(z["ig_ref_mean"])) <= 1e-6


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_inputs_are_what_the_forms_promise(case):
    H, W, form = case
    c = _case(*case)
    L = H * W
    pred, gt, fix = c["pred"].flatten(1), c["gt"].flatten(1), c["fix"]
    assert pred.shape == (3, L) and not torch.equal(pred[0], pred[1]) and not torch.equal(gt[1], gt[2])
    if form == "log":
        assert (pred.double().exp().sum(1) - 1).abs().max() < 1e-5 and pred.min() < -38 and pred.max() > -9
    else:
        assert (pred >= 0).all() and ((pred == 0).any(1).all() if form == "pred0" else (pred > 0).all())
    assert (gt >= 0).all() and ((gt == 0).any(1).all() if form == "gt0" else (gt > 0).all())
    assert (fix is None) == (form == "nofix")
    if fix is not None:
        f = fix.flatten(1)
        assert set(f.unique().tolist()) == {0.0, 1.0} and (f[:, 0] == 1).all() and (f[:, L - 1] == 1).all()
        assert (f.sum(1) >= 6).all()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_compared_values_are_well_conditioned_and_float32_sits_inside_the_bar(case):
    """Every compared float64 value is at least 0.05 in magnitude, and float32 torch is at least 4x inside the bar."""
    c = _case(*case)
    n = c["cols"]
    ref = c["ref"][:, :n]
    assert torch.isfinite(ref).all() and ref.abs().min().item() >= MIN_MAG
    e32 = S.rel_err(S.metrics(c["pred"], c["gt"], c["fix"], c["is_log"], dtype=torch.float32)[:, :n], ref)
    assert e32 <= TOL / 4, e32
    if c["fix"] is None:
        assert (c["ref"][:, 3] == 0).all()
        return
    for name in ("gt", "fix"):
        ref = c["ig_" + name]
        assert torch.isfinite(ref).all() and ref.abs().min().item() >= MIN_MAG
        e32 = S.rel_err(S.ig(c["ig_pred"], c[name], c["base"], dtype=torch.float32), ref)
        assert e32 <= TOL / 4, (name, e32)


def test_restated_nan_pattern_of_degenerate_maps():
    for kind in DEGENERATE:
        ref, (n, cols) = _degenerate(kind)[3:]
        want = torch.zeros(3, 4, dtype=torch.bool)
        want[n, list(cols)] = True
        assert torch.equal(torch.isnan(ref), want), kind
        assert torch.isfinite(ref[~want]).all(), kind
    # the float32 evaluation of the reference's formulas has the same pattern
    for kind in DEGENERATE:
        pred, gt, fix, ref, _ = _degenerate(kind)
        assert torch.equal(torch.isnan(S.metrics(pred, gt, fix, dtype=torch.float32)), torch.isnan(ref)), kind


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_hip_metrics_vs_float64(dev, case):
    from mspi_amd import metrics as M
    c = _case(*case)
    n = c["cols"]
    args = (c["pred"].to(dev), c["gt"].to(dev), None if c["fix"] is None else c["fix"].to(dev))
    got = M.per_sample(*args, pred_is_log=c["is_log"])
    assert torch.equal(got, M.per_sample(*args, pred_is_log=c["is_log"]))            # bitwise repeatable
    err = S.rel_err(got[:, :n], c["ref"][:, :n])
    e32 = S.rel_err(S.metrics(c["pred"], c["gt"], c["fix"], c["is_log"], dtype=torch.float32)[:, :n], c["ref"][:, :n])
    print("metrics %s: kernel %.2e, float32 torch %.2e of each value" % (_id(case), err, e32))
    assert err <= TOL
    if c["fix"] is None:
        assert torch.equal(got[:, 3].cpu(), torch.zeros(3))                          # exactly 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", IG_CASES, ids=_id)
def test_hip_ig_vs_float64(dev, case):
    from mspi_amd import metrics as M
    H, W, form, name = case
    c = _case(H, W, form)
    args = (c["ig_pred"].to(dev), c[name].to(dev), c["base"].to(dev))
    got = M.ig_per_sample(*args)
    assert torch.equal(got, M.ig_per_sample(*args))
    ref = c["ig_" + name]
    err = S.rel_err(got, ref)
    e32 = S.rel_err(S.ig(c["ig_pred"], c[name], c["base"], dtype=torch.float32), ref)
    print("ig %s: kernel %.2e, float32 torch %.2e of each value" % (_id(case), err, e32))
    assert err <= TOL


def _embedded(t, dev, pad=256):
    """t's values inside a larger buffer whose other values are BIG; (buffer, pointer to the first value)."""
    buf = torch.full((pad + t.numel() + pad,), BIG, dtype=torch.float32, device=dev)
    buf[pad:pad + t.numel()] = t.flatten().to(dev)
    return buf, buf.data_ptr() + 4 * pad


@pytest.mark.gpu
def test_hip_raw_abi_writes_its_own_floats_only(dev):
    """Both entry points once, N = 3 and L = 1023 (two rows at odd offsets): the output sits in a NaN-filled buffer, the
    inputs between large finite neighbours.  Only the output's own floats change, and no neighbour enters a result."""
    from mspi_amd import _lib, metrics as M
    lib = _lib.load()
    N, L, G = 3, 1023, 64
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for form in ("prob", "log"):
        c = _case(31, 33, form)
        keep = [_embedded(c[k], dev) for k in ("pred", "gt", "fix")]
        out = torch.full((G + N * 4 + G,), float("nan"), dtype=torch.float32, device=dev)
        assert lib.mspi_saliency_metrics(keep[0][1], keep[1][1], keep[2][1], out.data_ptr() + 4 * G, N, L, int(c["is_log"]), st) == 0
        torch.cuda.synchronize()
        assert torch.isnan(out[:G]).all() and torch.isnan(out[G + N * 4:]).all()
        got = out[G:G + N * 4].view(N, 4)
        assert torch.equal(got, M.per_sample(c["pred"].to(dev), c["gt"].to(dev), c["fix"].to(dev), pred_is_log=c["is_log"]))
        assert S.rel_err(got, c["ref"]) <= TOL
        out.fill_(float("nan"))                                                      # fix == NULL through the raw ABI
        assert lib.mspi_saliency_metrics(keep[0][1], keep[1][1], None, out.data_ptr() + 4 * G, N, L, int(c["is_log"]), st) == 0
        torch.cuda.synchronize()
        assert torch.isnan(out[:G]).all() and torch.isnan(out[G + N * 4:]).all()
        assert torch.equal(out[G:G + N * 4].view(N, 4)[:, :3], got[:, :3]) and (out[G:G + N * 4].view(N, 4)[:, 3] == 0).all()
        for b, _ in keep:
            assert (b[:256] == BIG).all() and (b[-256:] == BIG).all()
    c = _case(31, 33, "pred0")
    keep = [_embedded(c[k], dev) for k in ("ig_pred", "fix", "base")]
    out = torch.full((G + N + G,), float("nan"), dtype=torch.float32, device=dev)
    assert lib.mspi_saliency_ig(keep[0][1], keep[1][1], keep[2][1], out.data_ptr() + 4 * G, N, L, st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out[:G]).all() and torch.isnan(out[G + N:]).all()
    assert torch.equal(out[G:G + N], M.ig_per_sample(c["ig_pred"].to(dev), c["fix"].to(dev), c["base"].to(dev)))
    assert S.rel_err(out[G:G + N], c["ig_fix"]) <= TOL
    for b, _ in keep:
        assert (b[:256] == BIG).all() and (b[-256:] == BIG).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", DEGENERATE)
def test_hip_degenerate_maps_follow_the_restated_nan_pattern(dev, kind):
    """NaN exactly where the float64 restatement has NaN, finite everywhere else; the two ordinary samples of the batch
    stay inside the bar."""
    from mspi_amd import metrics as M
    pred, gt, fix, ref, (n, cols) = _degenerate(kind)
    got = M.per_sample(pred.to(dev), gt.to(dev), fix.to(dev)).cpu()
    print("%s: kernel %s, float64 %s" % (kind, got[n].tolist(), ref[n].tolist()))
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.isfinite(got[~torch.isnan(ref)]).all()
    others = [i for i in range(3) if i != n]
    assert S.rel_err(got[others], ref[others]) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("constant_pred", "zero_density"))
def test_hip_chunked_loss_terms_follow_the_same_nan_pattern(dev, kind):
    """csrc/salloss.hip reports the same four terms from its chunked kernels (SalLoss with grad logs them).  A log map of
    zeros is the constant prediction 1.0; the terms have NaN exactly where the float64 restatement and the evaluation
    kernel have it, and the ordinary samples stay inside the bar.  Its SIM also came from fminf and was 1.0 here."""
    from mspi_amd import metrics as M
    c = S.make_case("prob", 25, 41)
    log_map, gt, fix = c["pred"].log(), c["gt"].clone(), c["fix"]
    if kind == "constant_pred":
        log_map[1] = 0.0
        n = 1
    else:
        gt[0] = 0.0
        n = 0
    ref = S.metrics(log_map, gt, fix, pred_is_log=True)
    assert torch.isnan(ref[n]).any() and torch.isnan(ref).sum() == torch.isnan(ref[n]).sum()
    got = M.sal_loss_terms(log_map.to(dev), gt.to(dev), fix.to(dev)).cpu()
    ev = M.per_sample(log_map.to(dev), gt.to(dev), fix.to(dev), pred_is_log=True).cpu()
    print("chunked %s: kernel %s, evaluation kernel %s, float64 %s" % (kind, got[n].tolist(), ev[n].tolist(), ref[n].tolist()))
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isnan(ev), torch.isnan(ref))
    assert torch.isfinite(got[~torch.isnan(ref)]).all()
    others = [i for i in range(3) if i != n]
    assert S.rel_err(got[others], ref[others]) <= TOL


@pytest.mark.gpu
def test_sal_eval_counts_degenerate_samples_and_leaves_them_out(dev):
    """SalEval takes log maps: a log map of zeros is the constant prediction 1.0.  Its CC and SIM are NaN, counted in
    .nan and left out of the means; a sample without fixations does the same to NSS."""
    from mspi_amd import metrics as M
    c = S.make_case("prob", 25, 41)
    log_map = c["pred"].log()
    log_map[1] = 0.0
    fix = c["fix"].clone()
    fix[2] = 0.0
    ref = S.metrics(log_map, c["gt"], fix, pred_is_log=True)
    assert torch.isnan(ref[1, 1]) and torch.isnan(ref[1, 2]) and torch.isnan(ref[2, 3]) and torch.isnan(ref).sum() == 3
    ev = M.SalEval(jitter=False)
    ev.update(log_map.to(dev), c["gt"].to(dev), fix.to(dev))
    assert {k: ev.nan[k] for k in ("kl", "cc", "sim", "nss")} == {"kl": 0, "cc": 1, "sim": 1, "nss": 1}
    assert {k: ev.count[k] for k in ("kl", "cc", "sim", "nss")} == {"kl": 3, "cc": 2, "sim": 2, "nss": 2}
    res = ev.result()
    for col, k in enumerate(("kl", "cc", "sim", "nss")):
        want = ref[:, col][~torch.isnan(ref[:, col])].mean().item()
        assert not math.isnan(res[k]) and abs(res[k] - want) <= TOL * abs(want), (k, res[k], want)
