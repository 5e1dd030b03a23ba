"""CPU restatement of the evaluation metrics behind csrc/metrics.hip's saliency_metrics_kernel and saliency_ig_kernel:
kldiv / cc / similarity / nss (utils/compute_saliency_metrics.py:9-108 of the reference) and ig (:278-308), term by term
in torch and in the dtype the caller chooses, float64 by default.  Same eps, unbiased std, min-max normalisation before
SIM; torch.min hands a NaN on, as upstream.  It is the yardstick of tests/test_eval_kernels.py, which also
pins it to the reference's own float32 results (tests/golden/saliency_metrics.npz, the ig_* entries of saliency_auc.npz).
`make_case` builds the seeded inputs both modules share.  It is not imported by mspi_amd."""
import numpy as np
import torch

EPS = 2.2204e-16


def metrics(pred, gt, fix=None, pred_is_log=False, dtype=torch.float64):
    """[B,4] per-sample (KL, CC, SIM, NSS) of [B,H,W] maps; column 3 is 0 without a fixation map.  pred_is_log: pred is
    a log map and is exponentiated in `dtype` first."""
    B = pred.shape[0]
    s, g = pred.reshape(B, -1).to(dtype), gt.reshape(B, -1).to(dtype)
    if pred_is_log:
        s = s.exp()
    sp, gp = s / s.sum(1, keepdim=True), g / g.sum(1, keepdim=True)
    kl = (gp * torch.log(EPS + gp / (sp + EPS))).sum(1)                                    # kldiv :9-31
    sz = (s - s.mean(1, keepdim=True)) / s.std(1, keepdim=True)
    gz = (g - g.mean(1, keepdim=True)) / g.std(1, keepdim=True)
    cc = (sz * gz).sum(1) / torch.sqrt((sz * sz).sum(1) * (gz * gz).sum(1))                # cc :73-90
    sn = (s - s.min(1, keepdim=True)[0]) / (s.max(1, keepdim=True)[0] - s.min(1, keepdim=True)[0])
    gn = (g - g.min(1, keepdim=True)[0]) / (g.max(1, keepdim=True)[0] - g.min(1, keepdim=True)[0])
    sim = torch.min(sn / sn.sum(1, keepdim=True), gn / gn.sum(1, keepdim=True)).sum(1)     # similarity :46-70
    if fix is None:
        ns = torch.zeros(B, dtype=dtype)
    else:
        f = fix.reshape(B, -1).to(dtype)
        ns = (((s - s.mean(1, keepdim=True)) / (s.std(1, keepdim=True) + EPS)) * f).sum(1) / f.sum(1)   # nss :93-107
    return torch.stack([kl, cc, sim, ns], 1)


def ig(pred, gt, baseline, dtype=torch.float64):
    """[B] per-sample information gain of pred over baseline (:278-308)."""
    s, g, b = (torch.as_tensor(t).flatten(1).to(dtype) for t in (pred, gt, baseline))
    s, g, b = s / s.sum(1, keepdim=True), g / g.sum(1, keepdim=True), b / b.sum(1, keepdim=True)
    return (g * (torch.log(EPS + s) - torch.log(EPS + b))).sum(1)


def rel_err(got, ref):
    """max |got - ref| / |ref|: relative to each value's own magnitude, no floor."""
    got, ref = got.detach().double().cpu(), ref.double()
    return ((got - ref).abs() / ref.abs()).max().item()


# ------------------------------------------------------------------------------------------------------ seeded inputs
FORMS = ("prob", "log", "gt0", "pred0", "fix", "nofix")


def _bumps(rng, t, n, lo, hi):
    """A positive smooth profile over the flattened map: n Gaussian bumps of widths lo .. hi (fractions of the map)."""
    m = np.zeros_like(t)
    for _ in range(n):
        c, w, a = rng.uniform(0.05, 0.95), rng.uniform(lo, hi), rng.uniform(0.5, 1.0)
        m += a * np.exp(-(t - c) ** 2 / (2 * w * w))
    return m


SEED = 21      # chosen so that every value the GPU tests compare is at least 0.05 in magnitude (test_eval_kernels.py asserts it)


def make_case(form, H, W, B=3, seed=SEED):
    """{"pred", "gt", "fix" (or None), "base", "is_log"} of float32 [B,H,W] tensors with different content per sample.

    Every map is a profile over the flattened index, so a shape only decides L and the rows' alignment.
      prob   probabilities without zeros, a dense density
      log    a log-softmax map that follows the density and falls by a further 36 over one stretch (about -40 there)
      gt0    the density's values below 5 % of its peak, and at least its lowest quarter, are exactly 0
      pred0  the prediction's values below 10 % of its peak are exactly 0
      fix    as prob, with five times the fixations
      nofix  as prob, without a fixation map
    A fixation map always holds pixel 0 and pixel L - 1; the others are drawn where the density is high."""
    assert form in FORMS
    L = H * W
    rng = np.random.default_rng([seed, L, FORMS.index(form)])
    t = (np.arange(L) + 0.5) / L
    pred, gt, fix, base = (np.zeros((B, L)) for _ in range(4))
    for b in range(B):
        d = _bumps(rng, t, 3, 0.03, 0.10)
        d = d / d.max()
        other = _bumps(rng, t, 2, 0.05, 0.15)
        noise = rng.normal(0, 1, L)
        logits = 4.0 * d + 1.0 * other / other.max() + 0.3 * noise
        if form == "log":
            inner = (t > 0.1) & (t < 0.9)
            c = t[inner][np.argmin(d[inner])]                          # where the density is lowest
            logits = logits - 36.0 * np.clip(1.0 - np.abs(t - c) / 0.08, 0.0, 1.0)
        logits = logits - logits.max()
        p = np.exp(logits) / np.exp(logits).sum()
        dens = d + 0.02
        if form == "gt0":
            dens = np.where(d < max(0.05, np.quantile(d, 0.25)), 0.0, d)
        if form == "pred0":
            p = np.where(p < 0.10 * p.max(), 0.0, p)
        pred[b] = logits - np.log(np.exp(logits).sum()) if form == "log" else p
        gt[b] = dens
        base[b] = 1.25 - d + 0.3 * _bumps(rng, t, 1, 0.2, 0.4)         # a baseline that is low where the density is high
        nfix = max(6, int(L * (0.05 if form == "fix" else 0.01)))
        w = d ** 4 / (d ** 4).sum()
        fix[b, rng.choice(L, size=nfix, replace=False, p=w)] = 1.0
        fix[b, 0] = fix[b, L - 1] = 1.0
    out = {k: torch.from_numpy(v.astype(np.float32)).view(B, H, W) for k, v in
           (("pred", pred), ("gt", gt), ("fix", fix), ("base", base))}
    if form == "nofix":
        out["fix"] = None
    out["is_log"] = form == "log"
    return out
