"""Float64 restatement of the contrastive head (model/model_utils.py:545-552 upstream) in this project's order: the mean over
each modality's tokens of the SyncBlock's slab, projector (Linear-LN-ReLU x2, Linear-LN), predictor (Linear-LN-ReLU, Linear) and
loss_av = 0.5 mean -cos(p_vis, z_aud) + 0.5 mean -cos(p_aud, z_vis) with the embeddings z detached, and its analytic backward in
the launch order of mspi_amd.autograd.ContrastHead; also the three new kernels' formulas on their own (neg_cosine_bwd,
layernorm_act_bwd, mean_rows_bwd).  No GPU, no project code: the tests hold the kernels to this file, and this file to torch
autograd (upstream_grads, tools/gen_contrast_golden.py)."""
import math

import numpy as np
import torch

DIM, HIDDEN, EPS, COS_EPS = 512, 2048, 1e-5, 1e-8
SIDES = ("vis", "aud")
# one modality's 18 tensors in module order (mspi_amd.autograd.CONTRAST_TENSORS): Linear i is (w{i}, b{i}), LayerNorm i (g{i}, e{i})
TENSORS = ("w0", "b0", "g0", "e0", "w1", "b1", "g1", "e1", "w2", "b2", "g2", "e2", "w3", "b3", "g3", "e3", "w4", "b4")
WIDTHS = ((DIM, HIDDEN), (HIDDEN, HIDDEN), (HIDDEN, HIDDEN), (HIDDEN, DIM), (DIM, HIDDEN))      # (in, out) of the five Linears
RELU = (True, True, False, True)                  # behind the four LayerNorms
NAMES = tuple("%s.%s" % (s, t) for s in SIDES for t in TENSORS)      # ContrastHead's 36 tensors in argument order


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def rel_err(got, ref):
    got, ref = _t(got), _t(ref)
    return ((got - ref).abs().max() / ref.abs().max()).item()


def make_case(B, Rv, Ra, seed):
    """slab [B, Rv+Ra, 512] standard normal; every Linear as nn.Linear initialises it (weight and bias uniform in
    +-1/sqrt(fan_in)), LayerNorm weights 1 + N(0, 0.1^2) and biases N(0, 0.1^2), drawn from RandomState(seed) in a fixed
    order.  The LayerNorm inputs then have a per-row spread of order 1 (0.2 to 0.6)."""
    rs = np.random.RandomState(seed)
    c = {"B": B, "Rv": Rv, "Ra": Ra, "seed": seed, "slab": rs.standard_normal((B, Rv + Ra, DIM))}
    for s in SIDES:
        for i, (k, n) in enumerate(WIDTHS):
            a = 1.0 / math.sqrt(k)
            c["%s.w%d" % (s, i)], c["%s.b%d" % (s, i)] = rs.uniform(-a, a, (n, k)), rs.uniform(-a, a, n)
            if i < 4:
                c["%s.g%d" % (s, i)], c["%s.e%d" % (s, i)] = 1.0 + 0.1 * rs.standard_normal(n), 0.1 * rs.standard_normal(n)
    return c


# ---- the three kernels' formulas
def layernorm(x, g, e):
    m = x.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(((x - m) ** 2).mean(-1, keepdim=True) + EPS)
    return (x - m) * r * g + e


def layernorm_act_bwd(dy, x, g, y=None):
    """(dx, dgamma, dbeta) of act(layernorm(x) g + e) over rows [M, C]: act the ReLU where y (the forward's output) is given --
    dy counts where y > 0, is 0 where y <= 0, and a NaN in y stays one -- the identity otherwise."""
    if y is not None:
        dy = torch.where(y > 0, dy, torch.where(y <= 0, torch.zeros_like(dy), y))
    m = x.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(((x - m) ** 2).mean(-1, keepdim=True) + EPS)
    xh = (x - m) * r
    a = dy * g
    dx = r * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def neg_cosine(p, z, scale):
    npn, nzn = p.norm(dim=-1).clamp_min(COS_EPS), z.norm(dim=-1).clamp_min(COS_EPS)
    return -scale * ((p * z).sum(-1) / (npn * nzn)).mean()


def neg_cosine_bwd(p, z, g, scale):
    """dp of neg_cosine(p, z, scale) times g, z a constant; the second term only where |p| >= 1e-8 (the clamp's derivative)."""
    N = p.shape[0]
    raw = p.norm(dim=-1, keepdim=True)
    npn, nzn = raw.clamp_min(COS_EPS), z.norm(dim=-1, keepdim=True).clamp_min(COS_EPS)
    dot = (p * z).sum(-1, keepdim=True)
    second = torch.where(raw < COS_EPS, torch.zeros_like(p), dot * p / (npn ** 3 * nzn))
    return -g * scale / N * (z / (npn * nzn) - second)


def mean_rows_bwd(g, R):
    """[N, C] -> [N, R, C]: the adjoint of the mean over R rows."""
    return (g / R)[:, None, :].expand(-1, R, -1)


# ---- the head
def _side(case, s, x):
    """One modality's projector and predictor on the pooled rows x: (emb, pred, zs, ys) as contrast_embed_forward keeps them."""
    zs, ys = [], []
    for i in range(4):
        zs.append(x @ _t(case["%s.w%d" % (s, i)]).t() + _t(case["%s.b%d" % (s, i)]))
        x = layernorm(zs[-1], _t(case["%s.g%d" % (s, i)]), _t(case["%s.e%d" % (s, i)]))
        if RELU[i]:
            x = torch.relu(x)
        ys.append(x)
    return ys[2], x @ _t(case["%s.w4" % s]).t() + _t(case["%s.b4" % s]), zs, ys


def forward(case):
    """(loss_av, {side: (pooled, emb, pred, zs, ys)}) in float64."""
    slab, Rv = _t(case["slab"]), case["Rv"]
    kept = {}
    for s, rows in (("vis", slab[:, :Rv]), ("aud", slab[:, Rv:])):
        pooled = rows.mean(1)
        kept[s] = (pooled,) + _side(case, s, pooled)
    loss = neg_cosine(kept["vis"][2], kept["aud"][1], 0.5) + neg_cosine(kept["aud"][2], kept["vis"][1], 0.5)
    return loss, kept


def backward(case, g=1.0):
    """(loss_av, {"slab": dslab, "vis.w0": ..}) for the loss's gradient g, in ContrastHead.backward's order: per modality
    neg_cosine_bwd against the OTHER modality's detached embedding, then down predictor and projector, then mean_rows_bwd."""
    loss, kept = forward(case)
    B, Rv, Ra = case["B"], case["Rv"], case["Ra"]
    out = {"slab": torch.zeros(B, Rv + Ra, DIM, dtype=torch.float64)}
    for s, o, r0, R in (("vis", "aud", 0, Rv), ("aud", "vis", Rv, Ra)):
        pooled, _, pred, zs, ys = kept[s]
        xs = [pooled] + ys
        d = neg_cosine_bwd(pred, kept[o][1], g, 0.5)
        for i in range(4, -1, -1):
            out["%s.w%d" % (s, i)], out["%s.b%d" % (s, i)] = d.t() @ xs[i], d.sum(0)
            d = d @ _t(case["%s.w%d" % (s, i)])
            if i == 0:
                out["slab"][:, r0:r0 + R] = mean_rows_bwd(d, R)
                break
            d, out["%s.g%d" % (s, i - 1)], out["%s.e%d" % (s, i - 1)] = layernorm_act_bwd(
                d, zs[i - 1], _t(case["%s.g%d" % (s, i - 1)]), ys[i - 1] if RELU[i - 1] else None)
    return loss, out


def upstream_grads(case, dtype=torch.float64):
    """(loss_av, gradients by "slab" and NAMES) from torch autograd through torch.nn layers built with upstream's arguments
    (model/model_utils.py:401-436, 285-290, 541-551): AdaptiveAvgPool over the tokens, the two projectors, the two predictors,
    D(p, z) = -cosine_similarity(p, z.detach()).mean()."""
    import torch.nn as nn
    import torch.nn.functional as F
    h, Rv = HIDDEN, case["Rv"]

    def projector():
        return nn.Sequential(nn.Linear(DIM, h), nn.LayerNorm(h), nn.ReLU(inplace=True), nn.Linear(h, h), nn.LayerNorm(h),
                             nn.ReLU(inplace=True), nn.Linear(h, h), nn.LayerNorm(h))

    def predictor():
        return nn.Sequential(nn.Linear(h, 512), nn.LayerNorm(512), nn.ReLU(), nn.Linear(512, h))

    def D(p, z):
        return -F.cosine_similarity(p, z.detach(), dim=-1).mean()
    mods, where = {}, {}
    for s in SIDES:
        mods[s] = (projector().to(dtype), predictor().to(dtype))
        params = list(mods[s][0].parameters()) + list(mods[s][1].parameters())
        assert len(params) == len(TENSORS)
        with torch.no_grad():
            for t, prm in zip(TENSORS, params):
                prm.copy_(_t(case["%s.%s" % (s, t)]).to(dtype))
                where["%s.%s" % (s, t)] = prm
    slab = _t(case["slab"]).to(dtype).requires_grad_(True)
    # b (t h w) c -> b c t h w and b (h w) c -> b c h w, then the adaptive average pools to one cell
    vis_fea = slab[:, :Rv].permute(0, 2, 1)[:, :, :, None, None]
    aud_fea = slab[:, Rv:].permute(0, 2, 1)[:, :, :, None]
    vis_emb = mods["vis"][0](nn.AdaptiveAvgPool3d((1, 1, 1))(vis_fea).flatten(1))
    aud_emb = mods["aud"][0](nn.AdaptiveAvgPool2d((1, 1))(aud_fea).flatten(1))
    vis_pred, aud_pred = mods["vis"][1](vis_emb), mods["aud"][1](aud_emb)
    loss = (D(vis_pred, aud_emb) + D(aud_pred, vis_emb)) * 0.5
    loss.backward()
    grads = {"slab": slab.grad}
    grads.update({k: prm.grad for k, prm in where.items()})
    return loss.detach(), grads
