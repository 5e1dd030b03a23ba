"""Float64 CPU restatement of the decoder stage between the lateral outputs and readout[0] -- the three SA gates
(model/model_utils.py:155-170) and the top-down sums of model/model_utils.py:566-567 -- in this project's order, with the
analytic backward that mirrors autograd.Fusion's launch sequence: the yardstick of tests/test_fusion_train.py.
tools/gen_fusion_golden.py pins it to torch autograd through torch.nn layers built with upstream's arguments (BasicConv3d's
BatchNorm3d(eps=1e-3, momentum=0.001), backbones/s3d.py:41-52, in .train() mode).

    l0 [B,D,T,8a,8b]  l1 [B,D,T,4a,4b]  l2 [B,D,T,2a,2b]  l3 [B,D,T,a,b]   masks [B,Cm,T,2a,2b]            (NCDHW)
    pre = conv (3,3,3) pad 1 of masks with cat(wc_0, wc_1, wc_2), no bias      [B, 3 mid, T, 2a, 2b]
    p   = relu(gam (pre - mean) rstd + bet)      batch statistics, biased variance, eps 1e-3
    m_k = up_{4,2,1}(p[:, k mid : (k + 1) mid])   gate_k = sigmoid(conv (1,3,3) pad (0,1,1) of m_k with w2_k, b2_k)
    s0 = l0 (1 + gate_0)    s2 = l2 (1 + gate_2) + up2(l3)    s1 = l1 (1 + gate_1) + up2(s2) + up4(l3)    s3 = l3
The value is the four maps autograd.ReadoutHead takes (s0 gated and not yet summed); the scalar differentiated is
sum_j <s_j, G_j> for four stored G_j."""
import numpy as np
import torch
import torch.nn.functional as F

import readout_restate as R

LATERALS = ("l0", "l1", "l2", "l3")
SA_PARAMS = tuple("%s_%d" % (n, k) for k in range(3) for n in ("wc", "gam", "bet", "w2", "b2"))      # sa_0, sa_1, sa_2
GRADS = ("G0", "G1", "G2", "G3")
MAPS = ("s0", "s1", "s2", "s3")
FACTORS = (4, 2, 1)                       # sa_k up-samples its premask by FACTORS[k]
EPS, MOMENTUM = 1e-3, 0.001
STATE_KEYS = {}
for _k in range(3):
    STATE_KEYS.update({"wc_%d" % _k: "sa_%d.conv_mask.0.conv.weight" % _k, "gam_%d" % _k: "sa_%d.conv_mask.0.bn.weight" % _k,
                       "bet_%d" % _k: "sa_%d.conv_mask.0.bn.bias" % _k, "w2_%d" % _k: "sa_%d.conv_mask.2.weight" % _k,
                       "b2_%d" % _k: "sa_%d.conv_mask.2.bias" % _k})


def param_shapes(Cm, mid):
    s = {}
    for k in range(3):
        s.update({"wc_%d" % k: (mid, Cm, 3, 3, 3), "gam_%d" % k: (mid,), "bet_%d" % k: (mid,), "w2_%d" % k: (1, mid, 1, 3, 3),
                  "b2_%d" % k: (1,)})
    return s


def make_case(B, T, a, b, seed, D=32, Cm=32, mid=32, zeros=False):
    """fp32 numpy inputs: laterals (signed, unit scale), masks (non-negative with exact zeros, as the adapter's ReLU leaves
    them), the 15 SA tensors at the scale of torch's default initialisation, and four upstream gradients G_j.
    zeros=True also clears whole 3 x 3 x 3 neighbourhoods of masks, so that the premask and its up-samples hold exact zeros."""
    rng = np.random.RandomState(seed)
    out = {"l%d" % j: rng.randn(B, D, T, (8 >> j) * a, (8 >> j) * b).astype(np.float32) for j in range(4)}
    out["masks"] = np.maximum(rng.randn(B, Cm, T, 2 * a, 2 * b), 0).astype(np.float32)
    for k, shape in param_shapes(Cm, mid).items():
        n = k.split("_")[0]
        if n == "gam":
            out[k] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif n == "bet":
            out[k] = (0.1 * rng.randn(*shape)).astype(np.float32)
        elif n == "b2":
            out[k] = rng.uniform(-0.2, 0.2, shape).astype(np.float32)
        else:
            out[k] = (rng.uniform(-1.0, 1.0, shape) / np.sqrt(27 * Cm if n == "wc" else 9 * mid)).astype(np.float32)
    for j in range(4):
        out["G%d" % j] = rng.randn(*out["l%d" % j].shape).astype(np.float32)
    if zeros:
        out["bet_0"][::2] = -4.0          # half of sa_0's units are dead everywhere: their post-ReLU premask is exactly 0
    return out


def _d(t):
    return torch.as_tensor(t).double()


def _cat(p, name, dtype=torch.float64):
    return torch.cat([torch.as_tensor(p["%s_%d" % (name, k)]).to(dtype) for k in range(3)], 0)


def bn_forward(x, gamma, beta):
    mean = x.mean((0, 2, 3, 4))
    var = ((x - mean.view(1, -1, 1, 1, 1)) ** 2).mean((0, 2, 3, 4))
    rstd = 1.0 / torch.sqrt(var + EPS)
    v = lambda t: t.view(1, -1, 1, 1, 1)
    return v(gamma) * (x - v(mean)) * v(rstd) + v(beta), mean, var, rstd


def forward(p, dtype=torch.float64):
    """The saved tensors: pre, p (post-ReLU premask), the statistics, and per gate m (up-sampled premask), gate; the maps."""
    q = {k: torch.as_tensor(p[k]).to(dtype) for k in LATERALS + ("masks",) + SA_PARAMS}
    mid = q["wc_0"].shape[0]
    pre = F.conv3d(q["masks"], _cat(p, "wc", dtype), None, padding=1)
    pb, mean, var, rstd = bn_forward(pre, _cat(p, "gam", dtype), _cat(p, "bet", dtype))
    pm = pb.clamp_min(0)
    sv = {"pre": pre, "p": pm, "bn": (mean, var, rstd), "m": [], "gate": []}
    gated = []
    for k in range(3):
        m = pm[:, k * mid:(k + 1) * mid]
        if FACTORS[k] != 1:
            m = R.up(m, FACTORS[k], dtype)
        gate = torch.sigmoid(F.conv3d(m, q["w2_%d" % k], q["b2_%d" % k], padding=(0, 1, 1)))
        sv["m"].append(m)
        sv["gate"].append(gate)
        gated.append(q["l%d" % k] * (1 + gate))
    s2 = gated[2] + R.up(q["l3"], 2, dtype)
    s1 = gated[1] + R.up(s2, 2, dtype) + R.up(q["l3"], 4, dtype)
    sv.update({"s0": gated[0], "s1": s1, "s2": s2, "s3": q["l3"]})
    return sv


def backward(p, sv, G):
    """Gradients of sum_j <s_j, G_j> for the 15 SA tensors and the four laterals, in the order autograd.Fusion launches:
    the two up-sample-sum adjoints, the row gate's backward, the (1,3,3) conv's backward with the mask m > 0 (the ReLU's for
    sa_2; for the up-sampled premasks exact as well, see autograd.Fusion), the up-sample adjoints, BatchNorm, the weight gradient."""
    q = {k: _d(p[k]) for k in LATERALS + ("masks",) + SA_PARAMS}
    G = [_d(g) for g in G]
    mid = q["wc_0"].shape[0]
    gr = {}
    D2 = G[2] + R.up_t(G[1], 2)
    gr["l3"] = G[3] + R.up_t(G[1], 4) + R.up_t(D2, 2)
    dp = torch.zeros_like(_d(sv["p"]))
    for k, Gk in enumerate((G[0], G[1], D2)):
        gate, m = _d(sv["gate"][k]), _d(sv["m"][k])
        gr["l%d" % k] = Gk * (1 + gate)
        dz = gate * (1 - gate) * (Gk * q["l%d" % k]).sum(1, keepdim=True)
        gr["w2_%d" % k] = torch.nn.grad.conv3d_weight(m, q["w2_%d" % k].shape, dz, padding=(0, 1, 1))
        gr["b2_%d" % k] = dz.sum().view(1)
        dm = torch.nn.grad.conv3d_input(m.shape, q["w2_%d" % k], dz, padding=(0, 1, 1)) * (m > 0)
        dp[:, k * mid:(k + 1) * mid] = dm if FACTORS[k] == 1 else R.up_t(dm, FACTORS[k])
    mean, _, rstd = (_d(t) for t in sv["bn"])
    pre = _d(sv["pre"])
    v = lambda t: t.view(1, -1, 1, 1, 1)
    M = pre.numel() // pre.shape[1]
    dym = dp * (_d(sv["p"]) > 0)
    xh = (pre - v(mean)) * v(rstd)
    dbeta, dgamma = dym.sum((0, 2, 3, 4)), (dym * xh).sum((0, 2, 3, 4))
    dpre = v(_cat(p, "gam")) * v(rstd) * (dym - v(dbeta) / M - xh * v(dgamma) / M)
    dW = torch.nn.grad.conv3d_weight(q["masks"], (3 * mid,) + tuple(q["wc_0"].shape[1:]), dpre, padding=1)
    for k in range(3):
        sl = slice(k * mid, (k + 1) * mid)
        gr["wc_%d" % k], gr["gam_%d" % k], gr["bet_%d" % k] = dW[sl], dgamma[sl], dbeta[sl]
    gr.update({"D2": D2, "dp": dp, "dpre": dpre})
    return gr


def running_stats(stats, M, steps=1):
    """running_mean, running_var [3 mid] after `steps` identical forwards from (0, 1): momentum 0.001, unbiased variance."""
    mean, var, _ = stats
    rm, rv = torch.zeros_like(mean), torch.ones_like(var)
    for _ in range(steps):
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1 - MOMENTUM) * rv + MOMENTUM * var * M / (M - 1)
    return rm, rv


def upstream_modules(p, dtype=torch.float64):
    """sa_0, sa_1, sa_2 as upstream builds them (model/model_utils.py:155-166 over backbones/s3d.py:41-52), .train(), holding p."""
    import torch.nn as nn
    mid, Cm = p["wc_0"].shape[:2]
    mods = []
    for k in range(3):
        f = FACTORS[k]
        basic = nn.Sequential()
        basic.conv = nn.Conv3d(Cm, mid, kernel_size=3, stride=1, padding=1, bias=False)
        basic.bn = nn.BatchNorm3d(mid, eps=1e-3, momentum=0.001, affine=True)
        basic.relu = nn.ReLU()
        seq = nn.Sequential(
            basic,
            nn.Upsample(scale_factor=(1, f, f), align_corners=False, mode="trilinear") if f != 1 else nn.Identity(),
            nn.Conv3d(mid, 1, kernel_size=(1, 3, 3), stride=1, padding=(0, 1, 1)),
            nn.Sigmoid(),
        ).to(dtype).train()
        with torch.no_grad():
            for name, dst in (("wc", basic.conv.weight), ("gam", basic.bn.weight), ("bet", basic.bn.bias), ("w2", seq[2].weight),
                              ("b2", seq[2].bias)):
                dst.copy_(torch.as_tensor(p["%s_%d" % (name, k)]).to(dtype))
        mods.append(seq)
    return mods


def upstream_grads(p, dtype=torch.float64):
    """(maps, {name: gradient}, modules): the four maps by upstream's lines (x * mask + x, model/model_utils.py:167-170, and
    the sums of :566-567) and torch autograd's gradients of sum_j <s_j, G_j> for the SA tensors and the laterals."""
    import torch.nn as nn
    mods = upstream_modules(p, dtype)
    lat = [torch.as_tensor(p[k]).to(dtype).requires_grad_() for k in LATERALS]
    masks = torch.as_tensor(p["masks"]).to(dtype)
    up2 = nn.Upsample(scale_factor=(1, 2, 2), mode="trilinear", align_corners=False)
    up4 = nn.Upsample(scale_factor=(1, 4, 4), mode="trilinear", align_corners=False)

    def sa(k, x):
        m = mods[k](masks)
        return x * m + x
    s2 = sa(2, lat[2]) + up2(lat[3])
    s1 = sa(1, lat[1]) + up2(s2) + up4(lat[3])
    maps = [sa(0, lat[0]), s1, s2, lat[3]]
    leaves = []
    for k in range(3):
        leaves += [mods[k][0].conv.weight, mods[k][0].bn.weight, mods[k][0].bn.bias, mods[k][2].weight, mods[k][2].bias]
    loss = sum((s * torch.as_tensor(p["G%d" % j]).to(dtype)).sum() for j, s in enumerate(maps))
    grads = torch.autograd.grad(loss, leaves + lat)
    return [s.detach() for s in maps], dict(zip(SA_PARAMS + LATERALS, grads)), mods
