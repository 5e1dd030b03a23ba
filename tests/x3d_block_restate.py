"""Float64 restatement of one stride-1 X3D residual block without branch1 (SlowFast/resnet_helper.py:213-360 and 490-616
upstream) with its three BatchNorm3d(eps 1e-5, momentum 0.1) layers on BATCH statistics, in this project's launch order, and
the analytic backward autograd.X3DBlock launches:

    z_a = a(x); t = relu(bn_a(z_a)); v0 = b(t); v = bn_b(v0); g = sigmoid(fc2(relu(fc1(p)))), p = bn_b(mean_THW(v0)) -- the mean
    of a per-channel affine map is the affine map of the mean --; s = swish(v g); z_c = c(s); y = relu(x + bn_c(z_c)).

Activations are channels-last [B,T,h,w,C] numpy arrays, the parameters in their nn layouts.  upstream_grads builds the same
block from torch.nn layers with upstream's arguments and differentiates <y, G> by torch autograd."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

EPS, MOMENTUM, SE_RATIO = 1e-5, 0.1, 0.0625
# the order of autograd.X3DBlock's 13 tensors (autograd.X3D_BLOCK_TENSORS); the four se ones are absent without `se`
PARAMS = ("wa", "ga", "ba", "wb", "gb", "bb", "w1", "b1", "w2", "b2", "wc", "gc", "bc")
SE_PARAMS = ("w1", "b1", "w2", "b2")
GRADS = ("x",) + PARAMS


def se_width(width, ratio=SE_RATIO, min_width=8, divisor=8):
    """fc1.out_channels of upstream's SE (SlowFast/resnet_helper.py:34-46)."""
    width *= ratio
    out = max(min_width, int(width + divisor / 2) // divisor * divisor)
    if out < 0.9 * width:
        out += divisor
    return int(out)


def params(case):
    return tuple(k for k in PARAMS if k in case)


def make_case(dim_out, dim_inner, B, T, h, w, se, seed):
    """fp32 numpy inputs: x the ReLU of a normal draw (a block input is post-ReLU), the conv weights uniform at the scale of
    torch's default initialisation, BatchNorm gamma ~ 1 + 0.3 N(0,1) and beta ~ 0.3 N(0,1), and the gradient G ~ N(0,1) of y."""
    rng = np.random.RandomState(seed)
    D, Ci = dim_out, dim_inner

    def uni(shape, fan):
        return (rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan)).astype(np.float32)

    def bn(c):
        return (1.0 + 0.3 * rng.randn(c)).astype(np.float32), (0.3 * rng.randn(c)).astype(np.float32)
    out = {"x": np.maximum(rng.randn(B, T, h, w, D), 0.0).astype(np.float32), "se": bool(se)}
    out["wa"] = uni((Ci, D, 1, 1, 1), D)
    out["ga"], out["ba"] = bn(Ci)
    out["wb"] = uni((Ci, 1, 3, 3, 3), 27)
    out["gb"], out["bb"] = bn(Ci)
    if se:
        Fc = se_width(Ci)
        out["w1"], out["b1"] = uni((Fc, Ci, 1, 1, 1), Ci), uni((Fc,), Ci)
        out["w2"], out["b2"] = uni((Ci, Fc, 1, 1, 1), Fc), uni((Ci,), Fc)
    out["wc"] = uni((D, Ci, 1, 1, 1), Ci)
    out["gc"], out["bc"] = bn(D)
    out["G"] = rng.randn(B, T, h, w, D).astype(np.float32)
    return out


def _d(t):
    return torch.as_tensor(np.asarray(t)).double()


def _stats(z):
    """Per-channel mean, biased variance and rstd over the rows of [B,T,h,w,C]."""
    r = z.reshape(-1, z.shape[-1])
    mean = r.mean(0)
    var = ((r - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def dwconv3(t, wb):
    """Depthwise (3,3,3), padding (1,1,1), stride 1 on channels-last t [B,T,h,w,C] with wb [C,1,3,3,3], tap by tap."""
    B, T, H, W, C = t.shape
    tp = F.pad(t, (0, 0, 1, 1, 1, 1, 1, 1))
    out = torch.zeros_like(t)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                out = out + tp[:, kt:kt + T, kh:kh + H, kw:kw + W] * wb[:, 0, kt, kh, kw]
    return out


def dwconv3_wgrad(t, dy):
    """dW[c][kt][kh][kw] = sum dy[n,t,h,w,c] x[n,t+kt-1,h+kh-1,w+kw-1,c], zeros outside the frame: [C,1,3,3,3]; any dtype."""
    B, T, H, W, C = t.shape
    tp = F.pad(t, (0, 0, 1, 1, 1, 1, 1, 1))
    dW = torch.zeros(C, 1, 3, 3, 3, dtype=t.dtype)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                dW[:, 0, kt, kh, kw] = (dy * tp[:, kt:kt + T, kh:kh + H, kw:kw + W]).reshape(-1, C).sum(0)
    return dW


def forward(case):
    """Every intermediate of the block in float64, as a dict; running-statistics inputs: the biased variances va, vb, vc."""
    c = {k: _d(v) for k, v in case.items() if k not in ("se",)}
    x = c["x"]
    B, T, h, w, D = x.shape
    Ci = c["wa"].shape[0]
    R = T * h * w
    o = {}
    o["z_a"] = x @ c["wa"].reshape(Ci, D).t()
    o["ma"], o["va"], o["ra"] = _stats(o["z_a"])
    o["xh_a"] = (o["z_a"] - o["ma"]) * o["ra"]
    o["t"] = torch.relu(o["xh_a"] * c["ga"] + c["ba"])
    o["v0"] = dwconv3(o["t"], c["wb"])
    o["mb"], o["vb"], o["rb"] = _stats(o["v0"])
    o["xh_b"] = (o["v0"] - o["mb"]) * o["rb"]
    o["v"] = o["xh_b"] * c["gb"] + c["bb"]
    if case["se"]:
        Fc = c["b1"].numel()
        pool0 = o["v0"].reshape(B, R, Ci).mean(1)
        o["p"] = (pool0 - o["mb"]) * o["rb"] * c["gb"] + c["bb"]
        o["h"] = torch.relu(o["p"] @ c["w1"].reshape(Fc, Ci).t() + c["b1"])
        o["gate"] = torch.sigmoid(o["h"] @ c["w2"].reshape(Ci, Fc).t() + c["b2"])
        g = o["gate"].reshape(B, 1, 1, 1, Ci)
    else:
        g = torch.ones(1, dtype=torch.float64)
    o["g"] = g
    o["w"] = o["v"] * g
    o["s"] = o["w"] * torch.sigmoid(o["w"])
    o["z_c"] = o["s"] @ c["wc"].reshape(D, Ci).t()
    o["mc"], o["vc"], o["rc"] = _stats(o["z_c"])
    o["xh_c"] = (o["z_c"] - o["mc"]) * o["rc"]
    o["y"] = torch.relu(x + o["xh_c"] * c["gc"] + c["bc"])
    return o


def _bn_bwd(d, xh, rstd, gamma):
    """(dx, dgamma, dbeta) of gamma xh + beta on batch statistics for the gradient d: mspi_bn_bwd's formula."""
    C = d.shape[-1]
    M = d.numel() // C
    dbeta = d.reshape(-1, C).sum(0)
    dgamma = (d * xh).reshape(-1, C).sum(0)
    return gamma * rstd * (d - dbeta / M - xh * dgamma / M), dgamma, dbeta


def backward(case, fwd=None):
    """{name: float64 gradient} for GRADS of <y, G>, in the order autograd.X3DBlock.backward works."""
    o = forward(case) if fwd is None else fwd
    c = {k: _d(v) for k, v in case.items() if k not in ("se",)}
    x, G = c["x"], c["G"]
    B, T, h, w, D = x.shape
    Ci = c["wa"].shape[0]
    R = T * h * w
    g = {}
    Gm = torch.where(o["y"] > 0, G, torch.zeros_like(G))
    dz_c, g["gc"], g["bc"] = _bn_bwd(Gm, o["xh_c"], o["rc"], c["gc"])
    g["wc"] = (dz_c.reshape(-1, D).t() @ o["s"].reshape(-1, Ci)).reshape(D, Ci, 1, 1, 1)
    ds = dz_c @ c["wc"].reshape(D, Ci)
    sg = torch.sigmoid(o["w"])
    dw = ds * sg * (1 + o["w"] * (1 - sg))
    dv = dw * o["g"]
    if case["se"]:
        Fc = c["b1"].numel()
        W1, W2 = c["w1"].reshape(Fc, Ci), c["w2"].reshape(Ci, Fc)
        dgate = (dw * o["v"]).reshape(B, R, Ci).sum(1)
        dz2 = dgate * o["gate"] * (1 - o["gate"])
        dh = dz2 @ W2
        dz1 = torch.where(o["h"] > 0, dh, torch.zeros_like(dh))
        g["w2"], g["b2"] = (dz2.t() @ o["h"]).reshape(Ci, Fc, 1, 1, 1), dz2.sum(0)
        g["w1"], g["b1"] = (dz1.t() @ o["p"]).reshape(Fc, Ci, 1, 1, 1), dz1.sum(0)
        dp = dz1 @ W1
        dv = dv + (dp / R).reshape(B, 1, 1, 1, Ci)
    dv0, g["gb"], g["bb"] = _bn_bwd(dv, o["xh_b"], o["rb"], c["gb"])
    g["wb"] = dwconv3_wgrad(o["t"], dv0)
    dt = dwconv3(dv0, c["wb"].flip(2, 3, 4))
    dtm = torch.where(o["t"] > 0, dt, torch.zeros_like(dt))
    dz_a, g["ga"], g["ba"] = _bn_bwd(dtm, o["xh_a"], o["ra"], c["ga"])
    g["wa"] = (dz_a.reshape(-1, Ci).t() @ x.reshape(-1, D)).reshape(Ci, D, 1, 1, 1)
    g["x"] = dz_a @ c["wa"].reshape(Ci, D) + Gm
    return g


def rel_err(got, ref):
    got, ref = torch.as_tensor(np.asarray(got)).double(), torch.as_tensor(np.asarray(ref)).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / ref.abs().max()).item()


class _SE(nn.Module):
    """SlowFast/resnet_helper.py:27-73: x * sigmoid(fc2(relu(fc1(avg_pool(x)))))."""

    def __init__(self, dim_in, ratio):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool3d((1, 1, 1))
        dim_fc = se_width(dim_in, ratio)
        self.fc1 = nn.Conv3d(dim_in, dim_fc, 1, bias=True)
        self.fc1_act = nn.ReLU()
        self.fc2 = nn.Conv3d(dim_fc, dim_in, 1, bias=True)
        self.fc2_sig = nn.Sigmoid()

    def forward(self, x):
        return x * self.fc2_sig(self.fc2(self.fc1_act(self.fc1(self.avg_pool(x)))))


class _Block(nn.Module):
    """ResBlock with an X3DTransform branch2, dim_in == dim_out, stride 1: upstream's layers with upstream's arguments."""

    def __init__(self, D, Ci, se):
        super().__init__()
        self.a = nn.Conv3d(D, Ci, (1, 1, 1), (1, 1, 1), 0, bias=False)
        self.a_bn = nn.BatchNorm3d(Ci, eps=EPS, momentum=MOMENTUM)
        self.b = nn.Conv3d(Ci, Ci, (3, 3, 3), (1, 1, 1), (1, 1, 1), groups=Ci, bias=False)
        self.b_bn = nn.BatchNorm3d(Ci, eps=EPS, momentum=MOMENTUM)
        self.se = _SE(Ci, SE_RATIO) if se else None
        self.c = nn.Conv3d(Ci, D, 1, 1, 0, bias=False)
        self.c_bn = nn.BatchNorm3d(D, eps=EPS, momentum=MOMENTUM)

    def forward(self, x):
        u = torch.relu(self.a_bn(self.a(x)))
        u = self.b_bn(self.b(u))
        if self.se is not None:
            u = self.se(u)
        u = u * torch.sigmoid(u)                      # Swish
        return torch.relu(x + self.c_bn(self.c(u)))


def upstream_block(case, dtype=torch.float64):
    """The torch.nn block in train() mode holding the case's tensors."""
    D, Ci = case["x"].shape[-1], case["wa"].shape[0]
    m = _Block(D, Ci, case["se"]).to(dtype).train()
    mods = {"wa": m.a.weight, "ga": m.a_bn.weight, "ba": m.a_bn.bias, "wb": m.b.weight, "gb": m.b_bn.weight, "bb": m.b_bn.bias,
            "wc": m.c.weight, "gc": m.c_bn.weight, "bc": m.c_bn.bias}
    if case["se"]:
        mods.update({"w1": m.se.fc1.weight, "b1": m.se.fc1.bias, "w2": m.se.fc2.weight, "b2": m.se.fc2.bias})
    with torch.no_grad():
        for k, p in mods.items():
            p.copy_(torch.as_tensor(case[k]).to(dtype))
    return m, mods


def upstream_grads(case, dtype=torch.float64):
    """(y [B,T,h,w,D], {name: gradient} for GRADS) of the torch.nn block by torch autograd on <y, G>, in `dtype`."""
    m, mods = upstream_block(case, dtype)
    x = torch.as_tensor(case["x"]).to(dtype).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    G = torch.as_tensor(case["G"]).to(dtype).permute(0, 4, 1, 2, 3)
    y = m(x)
    names = ["x"] + list(mods)
    gs = torch.autograd.grad(y, [x] + [mods[k] for k in mods], G)
    out = {k: v for k, v in zip(names, gs)}
    out["x"] = out["x"].permute(0, 2, 3, 4, 1)
    return y.detach().permute(0, 2, 3, 4, 1), out
