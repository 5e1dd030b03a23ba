"""CPU restatement of the training criterion (utils/loss.py:26-49 over utils/compute_saliency_metrics.py:9-108) and of
its ANALYTIC gradient with respect to the log map, in torch and in the dtype the caller chooses.  It is the yardstick of
tests/test_sal_loss_grad.py where the fixture has no entry (full-size maps, training loops); tools/gen_loss_golden.py
asserts it against autograd of the reference's own functions.  In float32 `terms` repeats oracle.restate.saliency_metrics
operation by operation.  It is not imported by mspi_amd."""
import numpy as np
import torch

EPS = 2.2204e-16


def terms(log_map, density, fixations=None, dtype=torch.float64):
    """[B,4] per-sample (KL, CC, SIM, NSS); NSS is 0 without fixations."""
    B = log_map.shape[0]
    s, g = log_map.reshape(B, -1).to(dtype).exp(), density.reshape(B, -1).to(dtype)
    sp, gp = s / s.sum(1, keepdim=True), g / g.sum(1, keepdim=True)
    kl = (gp * torch.log(EPS + gp / (sp + EPS))).sum(1)
    sz = (s - s.mean(1, keepdim=True)) / s.std(1, keepdim=True)
    gz = (g - g.mean(1, keepdim=True)) / g.std(1, keepdim=True)
    cc = (sz * gz).sum(1) / torch.sqrt((sz * sz).sum(1) * (gz * gz).sum(1))
    sn = (s - s.min(1, keepdim=True)[0]) / (s.max(1, keepdim=True)[0] - s.min(1, keepdim=True)[0])
    gn = (g - g.min(1, keepdim=True)[0]) / (g.max(1, keepdim=True)[0] - g.min(1, keepdim=True)[0])
    sim = torch.min(sn / sn.sum(1, keepdim=True), gn / gn.sum(1, keepdim=True)).sum(1)
    if fixations is None:
        ns = torch.zeros(B, dtype=dtype)
    else:
        f = fixations.reshape(B, -1).to(dtype)
        ns = (((s - s.mean(1, keepdim=True)) / (s.std(1, keepdim=True) + EPS)) * f).sum(1) / f.sum(1)
    return torch.stack([kl, cc, sim, ns], 1)


def loss_from_terms(t, with_nss, w_kl=1.0, w_cc=1.0, w_nss=0.1):
    """The batch mean of w_kl KL - w_cc CC [- w_nss NSS]."""
    m = t.mean(0)
    return w_kl * m[0] - w_cc * m[1] - (w_nss * m[3] if with_nss else 0.0)


def loss(log_map, density, fixations=None, dtype=torch.float64, **w):
    return loss_from_terms(terms(log_map, density, fixations, dtype), fixations is not None, **w)


def term_grads(log_map, density, fixations=None, dtype=torch.float64):
    """(dKL, dCC, dNSS) / d log_map, each of the log map's shape, per sample (no batch mean); dNSS is None without fixations."""
    B = log_map.shape[0]
    x, g = log_map.reshape(B, -1).to(dtype), density.reshape(B, -1).to(dtype)
    L = x.shape[1]
    s = x.exp()
    P, G = s.sum(1, keepdim=True), g.sum(1, keepdim=True)
    sp, gp = s / P, g / G
    ds, dg = s - s.mean(1, keepdim=True), g - g.mean(1, keepdim=True)
    Qs, Qg, A = (ds * ds).sum(1, keepdim=True), (dg * dg).sum(1, keepdim=True), (ds * dg).sum(1, keepdim=True)
    a = -gp * gp / ((sp + EPS) * (EPS * (sp + EPS) + gp))
    T = (a * sp).sum(1, keepdim=True)
    d_kl = s * (a - T) / P
    d_cc = s * (dg - (A / Qs) * ds) / torch.sqrt(Qs * Qg)
    d_nss = None
    if fixations is not None:
        f = fixations.reshape(B, -1).to(dtype)
        sd = torch.sqrt(Qs / (L - 1))
        F, D = f.sum(1, keepdim=True), (ds * f).sum(1, keepdim=True)
        d_nss = (s * ((f - F / L) / (sd + EPS) - D * ds / ((sd + EPS) ** 2 * (L - 1) * sd)) / F).view(log_map.shape)
    return d_kl.view(log_map.shape), d_cc.view(log_map.shape), d_nss


def loss_grad(log_map, density, fixations=None, dtype=torch.float64, w_kl=1.0, w_cc=1.0, w_nss=0.1):
    """d loss / d log_map of `loss` (the batch mean's 1/B included)."""
    d_kl, d_cc, d_nss = term_grads(log_map, density, fixations, dtype)
    out = w_kl * d_kl - w_cc * d_cc
    if d_nss is not None:
        out = out - w_nss * d_nss
    return out / log_map.shape[0]


def make_case(B, H, W, seed):
    """Seeded inputs, shared with tests/test_sal_loss_grad.py: a log-softmax map, a Gaussian-blob density whose values
    below 1e-3 are exactly 0, a binary fixation map with at least one fixation per sample."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)

    def blobs(n, lo, hi):
        m = np.zeros((B, H, W), np.float32)
        for b in range(B):
            for _ in range(n):
                cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(lo, hi) * min(H, W)
                m[b] += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32)
        return m
    logits = 4 * blobs(3, 0.1, 0.4) + rng.normal(0, 0.5, (B, H, W)).astype(np.float32)
    log_map = torch.log_softmax(torch.from_numpy(logits).flatten(1), 1).view(B, H, W).numpy()
    dens = blobs(2, 0.05, 0.15)
    dens = dens / dens.reshape(B, -1).max(1).reshape(B, 1, 1)
    dens[dens < 1e-3] = 0
    fix = (rng.random((B, H, W)) < np.clip(dens * 0.05 + 0.002, 0, 1)).astype(np.float32)
    for b in range(B):
        if fix[b].sum() == 0:
            fix[b].reshape(-1)[int(dens[b].argmax())] = 1
    assert (fix.reshape(B, -1).sum(1) >= 1).all() and set(np.unique(fix)) <= {0.0, 1.0}
    assert (dens == 0).any() and (dens.reshape(B, -1).max(1) == 1).all()
    return log_map.astype(np.float32), dens.astype(np.float32), fix
