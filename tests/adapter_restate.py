"""Float64 restatement of the adapter's Inception (Adapter.conv: backbones/s3d.py upstream, eight conv -> BatchNorm3d(eps 1e-3,
momentum 0.001) -> ReLU layers on BATCH statistics) in this project's launch order -- the unfolded conv, the statistics, the
normalisation with its ReLU, branch by branch into the channel slices of one output -- with the analytic backward
autograd.Adapter launches: per layer the BatchNorm backward under the ReLU mask, the weight gradient, and for the two
SepConv3d the data gradients through conv_t and conv_s.  The input `cat` gets no gradient.  Plus the gradient of `masks` of
the Fusion stage (fusion_dmasks): the data gradient of the concatenated 3x3x3 conv behind fusion_restate's dpre.

The branch widths are parameters: WIDTHS is the model's (416 -> 192 | 96 -> 208 -> 208 | 16 -> 48 -> 48 | 64), SMALL a
scaled-down set of multiples of 16 for the stored fixture."""
import numpy as np
import torch
import torch.nn.functional as F

import fusion_restate as FR

EPS, MOMENTUM = 1e-3, 0.001
WIDTHS = (416, 192, 96, 208, 16, 48, 64)         # cin, branch0, branch1 (1x1x1, SepConv3d), branch2 (1x1x1, SepConv3d), branch3
SMALL = (32, 16, 16, 32, 16, 16, 16)
LAYERS = ("b0", "b1a", "b1s", "b1t", "b2a", "b2s", "b2t", "b3")     # launch order
_MODULE = {"b0": ("branch0.0", "conv", "bn"), "b1a": ("branch1.0", "conv", "bn"), "b1s": ("branch1.1", "conv_s", "bn_s"),
           "b1t": ("branch1.1", "conv_t", "bn_t"), "b2a": ("branch2.0", "conv", "bn"), "b2s": ("branch2.1", "conv_s", "bn_s"),
           "b2t": ("branch2.1", "conv_t", "bn_t"), "b3": ("branch3.1", "conv", "bn")}
PARAMS = tuple("%s_%s" % (n, l) for l in LAYERS for n in ("w", "gam", "bet"))      # the order of autograd.Adapter's 24 tensors
STATE_KEYS = {}
BN_KEYS = {}
for _l, (_m, _c, _b) in _MODULE.items():
    STATE_KEYS.update({"w_%s" % _l: "adapter.conv.%s.%s.weight" % (_m, _c), "gam_%s" % _l: "adapter.conv.%s.%s.weight" % (_m, _b),
                       "bet_%s" % _l: "adapter.conv.%s.%s.bias" % (_m, _b)})
    BN_KEYS[_l] = "adapter.conv.%s.%s" % (_m, _b)


def geometry(widths=WIDTHS):
    """{layer: (cin, cout, kernel, padding)}."""
    cin, c0, c1a, c1, c2a, c2, c3 = widths
    return {"b0": (cin, c0, (1, 1, 1), (0, 0, 0)), "b1a": (cin, c1a, (1, 1, 1), (0, 0, 0)), "b1s": (c1a, c1, (1, 3, 3), (0, 1, 1)),
            "b1t": (c1, c1, (3, 1, 1), (1, 0, 0)), "b2a": (cin, c2a, (1, 1, 1), (0, 0, 0)), "b2s": (c2a, c2, (1, 3, 3), (0, 1, 1)),
            "b2t": (c2, c2, (3, 1, 1), (1, 0, 0)), "b3": (cin, c3, (1, 1, 1), (0, 0, 0))}


def slices(widths=WIDTHS):
    """{branch's last layer: (first channel, width)} in the output."""
    _, c0, _, c1, _, c2, c3 = widths
    return {"b0": (0, c0), "b1t": (c0, c1), "b2t": (c0 + c1, c2), "b3": (c0 + c1 + c2, c3)}


def make_case(B, T, h, w, seed, widths=WIDTHS):
    """fp32 numpy inputs: cat (non-negative: max-pools and an up-sample of post-ReLU maps), the 24 tensors at the scale of
    torch's default initialisation, and the gradient G of the output."""
    rng = np.random.RandomState(seed)
    out = {"cat": np.abs(rng.randn(B, widths[0], T, h, w)).astype(np.float32), "widths": tuple(widths)}
    for l, (cin, cout, k, _) in geometry(widths).items():
        out["w_%s" % l] = (rng.uniform(-1.0, 1.0, (cout, cin) + k) / np.sqrt(cin * k[0] * k[1] * k[2])).astype(np.float32)
        out["gam_%s" % l] = rng.uniform(0.5, 1.5, (cout,)).astype(np.float32)
        out["bet_%s" % l] = (0.1 * rng.randn(cout)).astype(np.float32)
    out["G"] = rng.randn(B, sum(s[1] for s in slices(widths).values()), T, h, w).astype(np.float32)
    return out


def _d(t):
    return torch.as_tensor(t).double()


def _v(t):
    return t.view(1, -1, 1, 1, 1)


def _layer(x, p, l, pad):
    z = F.conv3d(x, _d(p["w_%s" % l]), None, padding=pad)
    mean = z.mean((0, 2, 3, 4))
    var = ((z - _v(mean)) ** 2).mean((0, 2, 3, 4))
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = (_v(_d(p["gam_%s" % l])) * (z - _v(mean)) * _v(rstd) + _v(_d(p["bet_%s" % l]))).clamp_min(0)
    return {"x": x, "z": z, "mean": mean, "var": var, "rstd": rstd, "y": y}


def forward(p, cat=None):
    """{layer: saved tensors} and "masks", the concatenated output."""
    geo = geometry(p["widths"])
    cat = _d(p["cat"]) if cat is None else _d(cat)
    pooled = F.max_pool3d(cat, 3, 1, 1)
    sv = {}
    src = {"b0": None, "b1a": None, "b1s": "b1a", "b1t": "b1s", "b2a": None, "b2s": "b2a", "b2t": "b2s", "b3": None}
    for l in LAYERS:
        x = pooled if l == "b3" else (cat if src[l] is None else sv[src[l]]["y"])
        sv[l] = _layer(x, p, l, geo[l][3])
    sv["masks"] = torch.cat([sv[l]["y"] for l in ("b0", "b1t", "b2t", "b3")], 1)
    return sv


def _layer_bwd(s, p, l, dy, pad, need_dx):
    M = s["z"].numel() // s["z"].shape[1]
    dym = dy * (s["y"] > 0)
    xh = (s["z"] - _v(s["mean"])) * _v(s["rstd"])
    dbeta, dgamma = dym.sum((0, 2, 3, 4)), (dym * xh).sum((0, 2, 3, 4))
    dz = _v(_d(p["gam_%s" % l])) * _v(s["rstd"]) * (dym - _v(dbeta) / M - xh * _v(dgamma) / M)
    w = _d(p["w_%s" % l])
    dW = torch.nn.grad.conv3d_weight(s["x"], w.shape, dz, padding=pad)
    dx = torch.nn.grad.conv3d_input(s["x"].shape, w, dz, padding=pad) if need_dx else None
    return {"w_%s" % l: dW, "gam_%s" % l: dgamma, "bet_%s" % l: dbeta}, dx, dz


def backward(p, sv, G=None):
    """{name: gradient} of <masks, G> for the 24 tensors, and "dz_<layer>", the gradient in front of each BatchNorm."""
    geo = geometry(p["widths"])
    G = _d(p["G"] if G is None else G)
    gr = {}
    for last, chain in (("b0", ("b0",)), ("b1t", ("b1t", "b1s", "b1a")), ("b2t", ("b2t", "b2s", "b2a")), ("b3", ("b3",))):
        c0, c = slices(p["widths"])[last]
        dy = G[:, c0:c0 + c]
        for i, l in enumerate(chain):
            g, dy, dz = _layer_bwd(sv[l], p, l, dy, geo[l][3], need_dx=i + 1 < len(chain))
            gr.update(g)
            gr["dz_%s" % l] = dz
    return gr


def running_stats(s, steps=1):
    """running_mean, running_var of a layer after `steps` identical forwards from (0, 1): unbiased variance, momentum 0.001."""
    M = s["z"].numel() // s["z"].shape[1]
    rm, rv = torch.zeros_like(s["mean"]), torch.ones_like(s["var"])
    for _ in range(steps):
        rm = (1 - MOMENTUM) * rm + MOMENTUM * s["mean"]
        rv = (1 - MOMENTUM) * rv + MOMENTUM * s["var"] * M / (M - 1)
    return rm, rv


def upstream_inception(p, dtype=torch.float64):
    """Inception as upstream builds it (BasicConv3d / SepConv3d of backbones/s3d.py: Conv3d without bias,
    BatchNorm3d(eps=1e-3, momentum=0.001, affine=True), ReLU), .train(), holding p.  Returns (module, {layer: (conv, bn)})."""
    import torch.nn as nn
    cin, c0, c1a, c1, c2a, c2, c3 = p["widths"]

    def basic(i, o):
        m = nn.Sequential()
        m.conv = nn.Conv3d(i, o, kernel_size=1, stride=1, padding=0, bias=False)
        m.bn = nn.BatchNorm3d(o, eps=1e-3, momentum=0.001, affine=True)
        m.relu = nn.ReLU()
        return m

    def sep(i, o):
        m = nn.Sequential()
        m.conv_s = nn.Conv3d(i, o, (1, 3, 3), (1, 1, 1), (0, 1, 1), bias=False)
        m.bn_s = nn.BatchNorm3d(o, eps=1e-3, momentum=0.001, affine=True)
        m.relu_s = nn.ReLU()
        m.conv_t = nn.Conv3d(o, o, (3, 1, 1), (1, 1, 1), (1, 0, 0), bias=False)
        m.bn_t = nn.BatchNorm3d(o, eps=1e-3, momentum=0.001, affine=True)
        m.relu_t = nn.ReLU()
        return m
    b0 = nn.Sequential(basic(cin, c0))
    b1 = nn.Sequential(basic(cin, c1a), sep(c1a, c1))
    b2 = nn.Sequential(basic(cin, c2a), sep(c2a, c2))
    b3 = nn.Sequential(nn.MaxPool3d(kernel_size=(3, 3, 3), stride=1, padding=1), basic(cin, c3))
    mod = nn.ModuleList([b0, b1, b2, b3]).to(dtype).train()
    layers = {"b0": (b0[0].conv, b0[0].bn), "b1a": (b1[0].conv, b1[0].bn), "b1s": (b1[1].conv_s, b1[1].bn_s),
              "b1t": (b1[1].conv_t, b1[1].bn_t), "b2a": (b2[0].conv, b2[0].bn), "b2s": (b2[1].conv_s, b2[1].bn_s),
              "b2t": (b2[1].conv_t, b2[1].bn_t), "b3": (b3[1].conv, b3[1].bn)}
    with torch.no_grad():
        for l, (conv, bn) in layers.items():
            conv.weight.copy_(torch.as_tensor(p["w_%s" % l]).to(dtype))
            bn.weight.copy_(torch.as_tensor(p["gam_%s" % l]).to(dtype))
            bn.bias.copy_(torch.as_tensor(p["bet_%s" % l]).to(dtype))
    return mod, layers


def upstream_grads(p, dtype=torch.float64):
    """(masks, {name: gradient}, layers): Inception.forward's torch.cat of the four branches and torch autograd's gradients of
    <masks, G> for the 24 tensors; the layers' running statistics have taken one step."""
    mod, layers = upstream_inception(p, dtype)
    cat = torch.as_tensor(p["cat"]).to(dtype)
    masks = torch.cat([b(cat) for b in mod], 1)
    leaves = [t for l in LAYERS for t in (layers[l][0].weight, layers[l][1].weight, layers[l][1].bias)]
    grads = torch.autograd.grad((masks * torch.as_tensor(p["G"]).to(dtype)).sum(), leaves)
    return masks.detach(), dict(zip(PARAMS, grads)), layers


def wgrad(x, dy, k, pad):
    """dW [Co,Ci,kt,kh,kw] and db [Co] in float64 of a stride-1 conv for x [N,Ci,T,H,W] and dy [N,Co,T,H,W]."""
    x, dy = _d(x), _d(dy)
    return torch.nn.grad.conv3d_weight(x, (dy.shape[1], x.shape[1]) + tuple(k), dy, padding=pad), dy.sum((0, 2, 3, 4))


def fusion_dmasks(fp, grads=None):
    """The gradient of `masks` of the Fusion stage on a fusion_restate case: the data gradient of the concatenated 3x3x3 conv
    Cm -> 3 mid for fusion_restate.backward's dpre."""
    if grads is None:
        grads = FR.backward(fp, FR.forward(fp), [fp[g] for g in FR.GRADS])
    return torch.nn.grad.conv3d_input(_d(fp["masks"]).shape, FR._cat(fp, "wc"), grads["dpre"], padding=1)


def fusion_dmasks_upstream(fp, dtype=torch.float64):
    """The same by torch autograd through upstream's SA modules."""
    mods = FR.upstream_modules(fp, dtype)
    import torch.nn as nn
    lat = [torch.as_tensor(fp[k]).to(dtype) for k in FR.LATERALS]
    masks = torch.as_tensor(fp["masks"]).to(dtype).requires_grad_()
    up2 = nn.Upsample(scale_factor=(1, 2, 2), mode="trilinear", align_corners=False)
    up4 = nn.Upsample(scale_factor=(1, 4, 4), mode="trilinear", align_corners=False)

    def sa(k, x):
        return x * mods[k](masks) + x
    s2 = sa(2, lat[2]) + up2(lat[3])
    s1 = sa(1, lat[1]) + up2(s2) + up4(lat[3])
    maps = [sa(0, lat[0]), s1, s2, lat[3]]
    loss = sum((s * torch.as_tensor(fp["G%d" % j]).to(dtype)).sum() for j, s in enumerate(maps))
    return torch.autograd.grad(loss, masks)[0]
