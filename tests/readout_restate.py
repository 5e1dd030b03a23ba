"""Float64 CPU restatement of the whole readout in this project's order with its analytic backward: the yardstick of
tests/test_readout_train.py.  The head (autograd.ReadoutHead) is restated here, the tail in tests/readout_tail_restate.py.
tools/gen_readout_golden.py pins both to torch autograd through torch.nn layers built with upstream's arguments
(model/model_utils.py:490-504, BatchNorm in .train() mode) on the 4 D-channel concat upstream builds.

    s0 [B,D,4,8a,8b]  s1 [B,D,4,4a,4b]  s2 [B,D,4,2a,2b]  s3 [B,D,4,a,b]       (NCDHW; s1, s2 already summed top-down)
    y0 = W0 s0 + b0 + up2((W0+W1) s1) + up4((W0+W2) s2) + up8((W0+W3) s3)      W = [W0|W1|W2|W3] = readout[0].weight
    x1 = conv (3,3,3) pad 1 + b1          a1 = relu(g2 (x1 - mean) rstd + be2)   batch statistics, biased variance, eps 1e-5
    x4 = conv (1,3,3) pad (0,1,1) + b4    y4 = relu(g5 (x4 - mean) rstd + be5)
    out = tail(y4)
"""
import numpy as np
import torch
import torch.nn.functional as F

import readout_tail_restate as RT

HEAD = ("w0", "b0", "w1", "b1", "g2", "be2", "w4", "b4", "g5", "be5")
PARAMS = HEAD + RT.PARAMS
MAPS = ("s0", "s1", "s2", "s3")
EPS, MOMENTUM = 1e-5, 0.1
STATE_KEYS = dict({"w0": "readout.0.weight", "b0": "readout.0.bias", "w1": "readout.1.weight", "b1": "readout.1.bias",
                   "g2": "readout.2.weight", "be2": "readout.2.bias", "w4": "readout.4.weight", "b4": "readout.4.bias",
                   "g5": "readout.5.weight", "be5": "readout.5.bias"}, **RT.STATE_KEYS)


def param_shapes(D):
    s = {"w0": (D, 4 * D, 1, 1, 1), "b0": (D,), "w1": (D, D, 3, 3, 3), "b1": (D,), "g2": (D,), "be2": (D,),
         "w4": (64, D, 1, 3, 3), "b4": (64,), "g5": (64,), "be5": (64,)}
    s.update(RT.PARAM_SHAPES)
    return s


def make_case(B, a, b, seed, D=32):
    """fp32 numpy inputs: the four maps (signed, unit scale), the 16 parameters at the scale of torch's default
    initialisation (BatchNorm weights in [0.5, 1.5], biases small) and an upstream gradient g [B,32a,32b]."""
    rng = np.random.RandomState(seed)
    out = {"s%d" % j: rng.randn(B, D, 4, (8 >> j) * a, (8 >> j) * b).astype(np.float32) for j in range(4)}
    fan = {"0": 4 * D, "1": 27 * D, "4": 9 * D, "8": 256, "10": 288, "12": 288}
    for k, shape in param_shapes(D).items():
        if k[0] == "g":
            out[k] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif k[:2] == "be":
            out[k] = (0.1 * rng.randn(*shape)).astype(np.float32)
        else:
            out[k] = (rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan[k[1:]])).astype(np.float32)
    out["g"] = rng.randn(B, 32 * a, 32 * b).astype(np.float32)
    return out


def _d(t):
    return torch.as_tensor(t).double()


def up(x, k, dtype=torch.float64):
    """Bilinear up-sample by k of the last two axes of [B,C,T,h,w] (align_corners=False), as a pair of matrices."""
    return torch.einsum("Hh,bcthw,Ww->bctHW", RT.up_matrix(x.shape[3], k).to(dtype), x, RT.up_matrix(x.shape[4], k).to(dtype))


def up_t(x, k):
    """Its adjoint: [B,C,T,kh,kw] -> [B,C,T,h,w]."""
    return torch.einsum("Hh,bctHW,Ww->bcthw", RT.up_matrix(x.shape[3] // k, k), x, RT.up_matrix(x.shape[4] // k, k))


def bn_forward(x, gamma, beta):
    """(pre-ReLU output, mean, biased var, rstd) on batch statistics over (B, T, H, W)."""
    mean = x.mean((0, 2, 3, 4))
    var = ((x - mean.view(1, -1, 1, 1, 1)) ** 2).mean((0, 2, 3, 4))
    rstd = 1.0 / torch.sqrt(var + EPS)
    v = lambda t: t.view(1, -1, 1, 1, 1)
    return v(gamma) * (x - v(mean)) * v(rstd) + v(beta), mean, var, rstd


def bn_backward(dy, x, mean, rstd, gamma, mask):
    """(dx, dgamma, dbeta) for the gradient dy of the post-ReLU output whose mask is `mask`."""
    v = lambda t: t.view(1, -1, 1, 1, 1)
    M = x.numel() // x.shape[1]
    dym = dy * mask
    xh = (x - v(mean)) * v(rstd)
    dbeta, dgamma = dym.sum((0, 2, 3, 4)), (dym * xh).sum((0, 2, 3, 4))
    return v(gamma) * v(rstd) * (dym - v(dbeta) / M - xh * v(dgamma) / M), dgamma, dbeta


def head_forward(p, dtype=torch.float64):
    """The saved tensors of the head: y0, x1, p2 (before the ReLU), a1, x4, p5, y4 and the statistics (mean, var, rstd) x 2."""
    q = {k: torch.as_tensor(p[k]).to(dtype) for k in HEAD + MAPS}
    D = q["w0"].shape[0]
    W = q["w0"].flatten(1)
    y0 = F.conv3d(q["s0"], W[:, :D, None, None, None], q["b0"])
    for j in (1, 2, 3):
        y0 = y0 + up(F.conv3d(q["s%d" % j], (W[:, :D] + W[:, j * D:(j + 1) * D])[:, :, None, None, None]), 1 << j, dtype)
    x1 = F.conv3d(y0, q["w1"], q["b1"], padding=1)
    p2, m2, v2, r2 = bn_forward(x1, q["g2"], q["be2"])
    a1 = p2.clamp_min(0)
    x4 = F.conv3d(a1, q["w4"], q["b4"], padding=(0, 1, 1))
    p5, m5, v5, r5 = bn_forward(x4, q["g5"], q["be5"])
    return {"y0": y0, "x1": x1, "p2": p2, "a1": a1, "x4": x4, "p5": p5, "y4": p5.clamp_min(0),
            "bn2": (m2, v2, r2), "bn5": (m5, v5, r5)}


def head_backward(p, saved, dy4, masks=None):
    """Analytic gradients of the ten head parameters for the gradient dy4 of y4.  masks = (mask_a1, mask_y4): the ReLU masks
    to use in place of the restatement's own (a1 > 0, y4 > 0) -- the activations the backward is handed."""
    q = {k: _d(p[k]) for k in HEAD + MAPS}
    D = q["w0"].shape[0]
    mask1, mask4 = (saved["a1"] > 0, saved["y4"] > 0) if masks is None else masks
    y0, x1, a1, x4 = (_d(saved[k]) for k in ("y0", "x1", "a1", "x4"))
    m2, _, r2 = (_d(t) for t in saved["bn2"])
    m5, _, r5 = (_d(t) for t in saved["bn5"])
    gr = {}
    d4, gr["g5"], gr["be5"] = bn_backward(_d(dy4), x4, m5, r5, q["g5"], mask4)
    gr["w4"], gr["b4"] = torch.nn.grad.conv3d_weight(a1, q["w4"].shape, d4, padding=(0, 1, 1)), d4.sum((0, 2, 3, 4))
    da1 = torch.nn.grad.conv3d_input(a1.shape, q["w4"], d4, padding=(0, 1, 1))
    d1, gr["g2"], gr["be2"] = bn_backward(da1, x1, m2, r2, q["g2"], mask1)
    gr["w1"], gr["b1"] = torch.nn.grad.conv3d_weight(y0, q["w1"].shape, d1, padding=1), d1.sum((0, 2, 3, 4))
    dy0 = torch.nn.grad.conv3d_input(y0.shape, q["w1"], d1, padding=1)
    gr["b0"] = dy0.sum((0, 2, 3, 4))
    G = [torch.einsum("bothw,bithw->oi", dy0, q["s0"])]
    G += [torch.einsum("bothw,bithw->oi", up_t(dy0, 1 << j), q["s%d" % j]) for j in (1, 2, 3)]
    gr["w0"] = torch.cat([G[0] + G[1] + G[2] + G[3], G[1], G[2], G[3]], 1)[:, :, None, None, None]
    gr.update({"d4": d4, "da1": da1, "d1": d1, "dy0": dy0, "G": G})
    return gr


def forward(p, dtype=torch.float64):
    """Head then tail: a dict with "head" and "tail" (the two saved dicts) and "out" [B,H,W]."""
    head = head_forward(p, dtype)
    tail = RT.forward(head["y4"], p, dtype)
    return {"head": head, "tail": tail, "out": tail["out"]}


def backward(p, saved, g, head_masks=None, tail_masks=None):
    """The 16 parameter gradients of sum(out * g), plus "y4" (the gradient the head receives)."""
    tail = RT.backward(saved["head"]["y4"], p, saved["tail"], g, masks=tail_masks)
    head = head_backward(p, saved["head"], tail["y4"], masks=head_masks)
    out = {k: tail[k] for k in RT.PARAMS + ("y4",)}
    out.update({k: head[k] for k in HEAD})
    return out


def running_stats(stats, M, steps=1, mean0=None, var0=None):
    """running_mean, running_var after `steps` identical forwards from (0, 1): momentum 0.1, unbiased variance."""
    mean, var, _ = stats
    rm = torch.zeros_like(mean) if mean0 is None else mean0
    rv = torch.ones_like(var) if var0 is None else var0
    for _ in range(steps):
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1 - MOMENTUM) * rv + MOMENTUM * var * M / (M - 1)
    return rm, rv


def upstream_readout(p, dtype=torch.float64):
    """nn.Sequential with upstream's arguments (model/model_utils.py:490-504) at decoder width D, in .train() mode, holding p."""
    import torch.nn as nn
    D = p["w0"].shape[0]
    r = nn.Sequential(
        nn.Conv3d(D * 4, D, 1, 1, 0),
        nn.Conv3d(D, D, kernel_size=3, stride=1, padding=1),
        nn.BatchNorm3d(D),
        nn.ReLU(inplace=True),
        nn.Conv3d(D, 64, kernel_size=(1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1)),
        nn.BatchNorm3d(64),
        nn.ReLU(inplace=True),
        nn.Upsample(scale_factor=(1, 4, 4), mode="trilinear", align_corners=False),
        nn.Conv3d(64, 32, kernel_size=(4, 1, 1), stride=(4, 1, 1), padding=0),
        nn.ReLU(inplace=True),
        nn.Conv3d(32, 32, kernel_size=(1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1)),
        nn.ReLU(inplace=True),
        nn.Conv3d(32, 1, kernel_size=(1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1)),
    ).to(dtype).train()
    with torch.no_grad():
        for k, name in STATE_KEYS.items():
            i, attr = name.split(".")[1:]
            getattr(r[int(i)], attr).copy_(torch.as_tensor(p[k]).to(dtype))
    return r


def upstream_forward(p, dtype=torch.float64):
    """(out [B,H,W], the nn.Sequential) through upstream's order: s0' = s0 + up2(s1) + up4(s2) + up8(s3), the 4 D-channel
    concat, the Sequential, x - logsumexp(x)."""
    import torch.nn as nn
    r = upstream_readout(p, dtype)
    s = [torch.as_tensor(p[k]).to(dtype) for k in MAPS]
    ups = [nn.Upsample(scale_factor=(1, k, k), mode="trilinear", align_corners=False)(t) for k, t in ((2, s[1]), (4, s[2]), (8, s[3]))]
    z = r(torch.cat([s[0] + ups[0] + ups[1] + ups[2]] + ups, 1))[:, 0, 0]
    return z - torch.logsumexp(z.flatten(1), 1).view(-1, 1, 1), r


def upstream_grads(p, dtype=torch.float64):
    """(out, {name: gradient}) of sum(out * g) by torch autograd through upstream_forward."""
    out, r = upstream_forward(p, dtype)
    leaves = []
    for k in PARAMS:
        i, attr = STATE_KEYS[k].split(".")[1:]
        leaves.append(getattr(r[int(i)], attr))
    grads = torch.autograd.grad((out * torch.as_tensor(p["g"]).to(dtype)).sum(), leaves)
    return out.detach(), dict(zip(PARAMS, grads)), r
