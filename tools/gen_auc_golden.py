"""Writes tests/golden/saliency_auc.npz: small inputs, the injected jitter noise and the scores of the REFERENCE's own
auc_judd / auc_shuff / ig (utils/compute_saliency_metrics.py:111-308), and asserts tests/saliency_auc_restate.py
against them on the way.  Needs the reference checkout (oracle.ref_harness); run from the repository root:

    python tools/gen_auc_golden.py
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness as rh  # noqa: E402
import saliency_auc_restate as A  # noqa: E402

if not hasattr(np, "trapz"):          # the reference calls the deprecated alias
    np.trapz = np.trapezoid


def _reference():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))       # imported at the top of the file, used by a resize only
    cwd = os.getcwd()
    rh.enter_reference()
    from utils import compute_saliency_metrics as M
    os.chdir(cwd)
    return M


def _same(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or (not np.isnan(a) and not np.isnan(b) and abs(a - b) <= tol)


def main():
    M = _reference()
    rng = np.random.default_rng(20240)
    out = {}

    # ---- AUC-Judd ----
    def smooth(H, W):
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        m = np.zeros((H, W), np.float32)
        for _ in range(4):
            cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(3, 9)
            m += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32)
        return m

    def fixations(H, W, p):
        return (rng.random((H, W)) < p).astype(np.uint8)

    judd = []
    m = smooth(32, 48) + rng.random((32, 48), dtype=np.float32) * 0.05
    judd.append(("cont", m, fixations(32, 48, 0.03), None))
    u8 = np.round(smooth(48, 64) / 4 * 255).clip(0, 255).astype(np.float32)      # 256 levels, large tied regions
    fx = fixations(48, 64, 0.02)
    judd.append(("u8", u8, fx, None))
    judd.append(("u8_jitter", u8, fx, rng.random((48, 64))))
    md = smooth(24, 40) + rng.random((24, 40), dtype=np.float32) * 0.2
    judd.append(("dense", md, fixations(24, 40, 0.3), None))
    judd.append(("dense_jitter", md, fixations(24, 40, 0.3), rng.random((24, 40))))
    judd.append(("nofix", m, np.zeros((32, 48), np.uint8), None))
    judd.append(("const", np.full((24, 40), 0.25, np.float32), fixations(24, 40, 0.05), None))
    for name, sal, fix, noise in judd:
        keep = np.random.random
        if noise is not None:
            np.random.random = lambda shape, _n=noise: _n.copy()
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref = float(M.auc_judd(torch.from_numpy(sal)[None], torch.from_numpy(fix.astype(np.float32))[None],
                                       jitter=noise is not None))
        finally:
            np.random.random = keep
        got, n = A.auc_judd(sal, fix, noise)
        assert _same(got, ref, 1e-12), (name, got, ref)
        assert np.isnan(ref) == (name in ("nofix", "const")), (name, ref)
        assert n == int(fix.sum()) and (name == "nofix" or n <= sal.size // 2)
        print("[auc_judd] %-13s n=%4d  reference %.17g  restatement - reference %.1e" % (name, n, ref, got - ref))
        out["judd_%s_sal" % name] = sal
        out["judd_%s_fix" % name] = fix
        if noise is not None:
            out["judd_%s_noise" % name] = noise
        out["judd_%s_score" % name] = np.float64(ref)
    out["judd_cases"] = np.array([j[0] for j in judd])

    # ---- shuffled AUC ----
    def other_targets(H, other):
        x, y = np.where(other == 1)
        k = x * H + y
        return k % H - 1, k // H

    sauc = []
    H, W = 24, 40
    tenths = (np.arange(11) / 10).astype(np.float32)
    pin = rng.random((H, W), dtype=np.float32)
    pick = rng.random((H, W)) < 0.4
    pin[pick] = tenths[rng.integers(0, 11, size=int(pick.sum()))]
    pin[0, 0], pin[0, 1] = 0.0, 1.0                               # min 0, max 1: the normalisation is the identity
    gt = fixations(H, W, 0.06)
    gt[0, :2] = 0
    other = fixations(H, W, 0.1)
    fy, fx_ = np.where(gt == 1)
    pin[fy, fx_] = tenths[rng.integers(1, 10, size=fy.size)]      # exactly float32(k / 10) at the fixations ...
    ry, rx = other_targets(H, other)
    keep_ = ~((ry % H == 0) & (rx <= 1))
    pin[ry[keep_] % H, rx[keep_]] = tenths[rng.integers(1, 10, size=int(keep_.sum()))]   # ... and where other-fixations read
    assert pin.min() == 0.0 and pin.max() == 1.0
    sauc.append(("pin", pin, gt, other))
    sauc.append(("wide", smooth(24, 40) + rng.random((24, 40), dtype=np.float32) * 0.1, fixations(24, 40, 0.04), fixations(24, 40, 0.15)))
    sauc.append(("square", smooth(32, 32) + rng.random((32, 32), dtype=np.float32) * 0.1, fixations(32, 32, 0.05), fixations(32, 32, 0.05)))
    sauc.append(("noother", smooth(24, 40), fixations(24, 40, 0.04), np.zeros((24, 40), np.uint8)))
    sauc.append(("nofix", smooth(24, 40), np.zeros((24, 40), np.uint8), fixations(24, 40, 0.05)))
    for name, sal, gt, other in sauc:
        t = lambda a: torch.from_numpy(a.astype(np.float32))[None]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            np.random.seed(1)
            ref = float(M.auc_shuff(t(sal), t(gt), t(other)))
            np.random.seed(2)
            ref2 = float(M.auc_shuff(t(sal), t(gt), t(other)))
        assert _same(ref, ref2, 0.0), (name, ref, ref2)           # the splits are equal: no dependence on the random state
        counts = A.sauc_counts(sal, gt, other)
        got = A.sauc_from_counts(counts)
        assert _same(got, ref, 1e-12), (name, got, ref)
        assert np.isnan(ref) == (name == "nofix"), (name, ref)
        print("[auc_shuff] %-8s reference %.17g  restatement - reference %.1e  counts %s" % (name, ref, got - ref, counts.tolist()))
        out["sauc_%s_sal" % name] = sal.astype(np.float32)
        out["sauc_%s_gt" % name] = gt
        out["sauc_%s_other" % name] = other
        out["sauc_%s_score" % name] = np.float64(ref)
    out["sauc_cases"] = np.array([s[0] for s in sauc])
    # the pin must bite: with > in place of >= (or the other way round) its counts change
    s, g, o = sauc[0][1:]
    n_eq = sum(int(((s == th) & (g == 1)).sum()) for th in tenths[1:10])
    assert n_eq > 0

    # ---- information gain ----
    g = torch.Generator().manual_seed(5)
    B, H, W = 3, 24, 40
    pred = torch.softmax((torch.rand(B, H * W, generator=g) * 6), 1).view(B, H, W)
    dens = torch.rand(B, H, W, generator=g) ** 4
    base = torch.softmax((torch.rand(B, H * W, generator=g) * 2), 1).view(B, H, W)
    ref = M.ig(pred, dens, base)
    per = A.ig_per_sample(pred, dens, base)
    assert abs(per.mean().item() - ref.item()) < 1e-6
    print("[ig] reference %.9g  restatement mean %.9g" % (ref.item(), per.mean().item()))
    out.update(ig_pred=pred.numpy(), ig_gt=dens.numpy(), ig_base=base.numpy(), ig_ref_mean=ref.numpy(), ig_per_sample=per.numpy())

    path = os.path.join(ROOT, "tests", "golden", "saliency_auc.npz")
    np.savez_compressed(path, **out)
    print("[golden] %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
