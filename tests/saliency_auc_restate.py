"""CPU restatement of the reference's auc_judd, auc_shuff and ig (utils/compute_saliency_metrics.py:111-308), vectorised
numpy / torch with float64 scores.  It is the yardstick of tests/test_saliency_auc.py where the reference's own scores
are not in the fixture (full-size maps), and tools/gen_auc_golden.py asserts it against the reference's functions.  It is
not imported by mspi_amd."""
import numpy as np
import torch

_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def auc_judd(sal, fix, noise=None):
    """One map.  sal [H,W] float32, fix [H,W] (fixation where > 0); noise: the float64 array the reference would draw with
    np.random.random (jitter=True, :148-150) or None (jitter=False).  Returns (score float64, number of fixations)."""
    S = np.asarray(sal)
    F = np.asarray(fix).ravel()
    n = int((F > 0).sum())
    if n == 0:
        return float("nan"), 0
    if noise is not None:
        S = S + np.asarray(noise, dtype=np.float64) / 10 ** 7
    with np.errstate(invalid="ignore", divide="ignore"):
        S = (S - S.min()) / (S.max() - S.min())
    if np.isnan(S).all():
        return float("nan"), n
    s = S.ravel()
    P = s.size
    th = np.sort(s[F > 0])[::-1]
    above = P - np.searchsorted(np.sort(s), th, side="left")
    tp = np.concatenate([[0.0], np.arange(1, n + 1) / float(n), [1.0]])
    fp = np.concatenate([[0.0], (above - np.arange(n)).astype(np.float64) / (P - n), [1.0]])
    return float(_trapezoid(tp, x=fp)), n


def sauc_counts(sal, gt, other):
    """The 20 integers of one map: #{s >= th_k and gt == 1} (k = 1..9), #{r > th_k}, #{gt == 1}, #{other == 1}; float32
    normalisation as normalize_map (:33-43), other-fixations looked up with the reference's index arithmetic (:226, :246)."""
    s = torch.as_tensor(sal, dtype=torch.float32)
    s = ((s - s.min()) / (s.max() - s.min() * 1.0)).numpy()
    gt = np.asarray(gt, dtype=np.float32)
    other = np.asarray(other, dtype=np.float32)
    H = s.shape[0]
    x, y = np.where(other == 1)
    k = x * H + y
    r = s[k % H - 1, k // H] if k.size else np.zeros(0, np.float32)
    out = np.zeros(20, np.int64)
    for i in range(9):
        th = np.float32((i + 1) / 10)
        out[i] = int(((s >= th).astype(np.float32) + gt == 2).sum())
        out[9 + i] = int((r > th).sum())
    out[18] = int((gt == 1).sum())
    out[19] = k.size
    return out


def sauc_from_counts(c):
    """:254-276 on the counts.  The reference's num_fixations is np.sum of a float32 map, a float32 scalar, so tp and fp are
    float32 quotients before round(x, 4); the arithmetic is repeated here with the same numpy scalar types."""
    c = [int(v) for v in c]
    if c[18] == 0:
        return float("nan")
    nf = np.float32(c[18])
    area = [(0.0, 0.0)]
    for i in range(9):
        area.append((round(c[i] / (nf * 1.0), 4), round(c[9 + i] / (nf * 1.0), 4)))
    area.append((1.0, 1.0))
    area.sort(key=lambda p: p[0])
    return float(_trapezoid(np.array([p[0] for p in area]), np.array([p[1] for p in area])))


def auc_shuff(sal, gt, other):
    return sauc_from_counts(sauc_counts(sal, gt, other))


def ig_per_sample(s_map, gt, baseline):
    """[B] float32: the per-map sums whose mean the reference returns (:278-308)."""
    s, g, b = (torch.as_tensor(t, dtype=torch.float32).flatten(1) for t in (s_map, gt, baseline))
    s, g, b = s / s.sum(1, keepdim=True), g / g.sum(1, keepdim=True), b / b.sum(1, keepdim=True)
    eps = 2.2204e-16
    return (g * (torch.log(eps + s) - torch.log(eps + b))).sum(1)


def nanmean(v):
    """Mean over the entries that are not NaN (NaN if there is none) and the number of NaN entries."""
    v = np.asarray(v, dtype=np.float64)
    ok = ~np.isnan(v)
    return (float(v[ok].mean()) if ok.any() else float("nan")), int((~ok).sum())
