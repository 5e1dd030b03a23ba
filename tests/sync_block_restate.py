"""Float64 restatement of the SyncBlock's transformer Block (model/model_utils.py:84-152 upstream) in this project's order, with
the analytic backward in the launch order of mspi_amd.autograd.TransformerBlock.  No GPU, no project code: the tests hold the
kernels to this file, and this file to torch autograd (upstream_grads, tools/gen_sync_block_golden.py)."""
import math

import numpy as np
import torch

DIM, HEADS, HD, HIDDEN, EPS = 512, 4, 128, 2048, 1e-5
NAMES = ("n1w", "n1b", "wqkv", "wproj", "bproj", "n2w", "n2b", "w1", "b1", "w2", "b2")      # the Function's argument order
GRADS = ("x",) + NAMES


def make_case(B, R, seed, scale_x=1.0):
    """x and G standard normal (x times scale_x), weights xavier-uniform, biases N(0, 0.1^2), LayerNorm weights 1 + N(0, 0.1^2);
    float64 numpy arrays drawn from RandomState(seed) in a fixed order."""
    rs = np.random.RandomState(seed)

    def xavier(o, i):
        a = math.sqrt(6.0 / (i + o))
        return rs.uniform(-a, a, (o, i))
    c = {"B": B, "R": R, "seed": seed}
    c["x"] = rs.standard_normal((B, R, DIM)) * scale_x
    c["G"] = rs.standard_normal((B, R, DIM))
    c["n1w"], c["n1b"] = 1.0 + 0.1 * rs.standard_normal(DIM), 0.1 * rs.standard_normal(DIM)
    c["wqkv"] = xavier(3 * DIM, DIM)
    c["wproj"], c["bproj"] = xavier(DIM, DIM), 0.1 * rs.standard_normal(DIM)
    c["n2w"], c["n2b"] = 1.0 + 0.1 * rs.standard_normal(DIM), 0.1 * rs.standard_normal(DIM)
    c["w1"], c["b1"] = xavier(HIDDEN, DIM), 0.1 * rs.standard_normal(HIDDEN)
    c["w2"], c["b2"] = xavier(DIM, HIDDEN), 0.1 * rs.standard_normal(DIM)
    return c


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def layernorm(x, g, b):
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    return (x - mean) * rstd * g + b


def layernorm_bwd(dy, x, g):
    """(dx, dgamma, dbeta) of layernorm(x, g, b) over the last axis, rows = every other axis."""
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    xh = (x - mean) * rstd
    a = dy * g
    dx = rstd * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).flatten(0, -2).sum(0), dy.flatten(0, -2).sum(0)


def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def attention(q, k, v, scale):
    """q [..., Nq, D], k [..., Nk, D], v [..., Nk, Dv] -> o [..., Nq, Dv]."""
    return torch.softmax(scale * q @ k.transpose(-2, -1), -1) @ v


def attention_bwd(q, k, v, dO, scale, o=None):
    """(dq, dk, dv) of o = softmax(scale q k^T) v in the kernel's formulation; o: the stored forward output, if it is to be
    read instead of computed (the kernel reads it for Delta)."""
    q, k, v, dO = _t(q), _t(k), _t(v), _t(dO)
    P = torch.softmax(scale * q @ k.transpose(-2, -1), -1)
    o = P @ v if o is None else _t(o)
    delta = (dO * o).sum(-1, keepdim=True)
    dv = P.transpose(-2, -1) @ dO
    dS = P * (dO @ v.transpose(-2, -1) - delta)
    return scale * dS @ k, scale * dS.transpose(-2, -1) @ q, dv


def _heads(t, B, R):      # [B, R, 3 * DIM] -> three [B, HEADS, R, HD]
    return t.reshape(B, R, 3, HEADS, HD).permute(2, 0, 3, 1, 4)


def forward(case):
    """y and what the Function keeps or recomputes, float64 torch."""
    p = {k: _t(case[k]) for k in ("x",) + NAMES}
    B, R = case["B"], case["R"]
    s = {}
    s["h"] = layernorm(p["x"], p["n1w"], p["n1b"])
    s["qkv"] = s["h"] @ p["wqkv"].t()
    q, k, v = _heads(s["qkv"], B, R)
    s["o"] = attention(q, k, v, HD ** -0.5).transpose(1, 2).reshape(B, R, DIM)
    s["x1"] = p["x"] + s["o"] @ p["wproj"].t() + p["bproj"]
    s["n"] = layernorm(s["x1"], p["n2w"], p["n2b"])
    s["z"] = s["n"] @ p["w1"].t() + p["b1"]
    s["y"] = s["x1"] + gelu(s["z"]) @ p["w2"].t() + p["b2"]
    return s


def backward(case, G=None):
    """The twelve gradients (dict by GRADS) for the output gradient G (default case["G"]), in the Function's launch order."""
    p = {k: _t(case[k]) for k in ("x",) + NAMES}
    B, R = case["B"], case["R"]
    G = _t(case["G"] if G is None else G)
    s = forward(case)
    rows = lambda t: t.reshape(B * R, -1)                                     # noqa: E731
    n, z = s["n"], s["z"]
    dg = G @ p["w2"]
    g, dz = gelu(z), dg * gelu_grad(z)
    out = {"w2": rows(G).t() @ rows(g), "b2": rows(G).sum(0)}
    out["w1"], out["b1"] = rows(dz).t() @ rows(n), rows(dz).sum(0)
    d, out["n2w"], out["n2b"] = layernorm_bwd(dz @ p["w1"], s["x1"], p["n2w"])
    dx1 = G + d
    out["wproj"], out["bproj"] = rows(dx1).t() @ rows(s["o"]), rows(dx1).sum(0)
    do = (dx1 @ p["wproj"]).reshape(B, R, HEADS, HD).transpose(1, 2)
    q, k, v = _heads(s["qkv"], B, R)
    dq, dk, dv = attention_bwd(q, k, v, do, HD ** -0.5)
    dqkv = torch.stack((dq, dk, dv), 0).permute(1, 3, 0, 2, 4).reshape(B, R, 3 * DIM)
    out["wqkv"] = rows(dqkv).t() @ rows(s["h"])
    d, out["n1w"], out["n1b"] = layernorm_bwd(dqkv @ p["wqkv"], p["x"], p["n1w"])
    out["x"] = dx1 + d
    return out


def build_upstream(case, dtype=torch.float64):
    """The Block from torch.nn layers with upstream's arguments (qkv_bias=False, exact GELU, LayerNorm eps 1e-5) holding the
    case's tensors: (modules dict, forward function)."""
    import torch.nn as nn
    m = {"norm1": nn.LayerNorm(DIM, eps=EPS), "qkv": nn.Linear(DIM, 3 * DIM, bias=False), "proj": nn.Linear(DIM, DIM),
         "norm2": nn.LayerNorm(DIM, eps=EPS), "fc1": nn.Linear(DIM, HIDDEN), "act": nn.GELU(), "fc2": nn.Linear(HIDDEN, DIM)}
    where = {"n1w": m["norm1"].weight, "n1b": m["norm1"].bias, "wqkv": m["qkv"].weight, "wproj": m["proj"].weight,
             "bproj": m["proj"].bias, "n2w": m["norm2"].weight, "n2b": m["norm2"].bias, "w1": m["fc1"].weight, "b1": m["fc1"].bias,
             "w2": m["fc2"].weight, "b2": m["fc2"].bias}
    for mod in m.values():
        mod.to(dtype)
    with torch.no_grad():
        for k, prm in where.items():
            prm.copy_(_t(case[k]).to(dtype))

    def fwd(x):
        B, N, C = x.shape
        qkv = m["qkv"](m["norm1"](x)).reshape(B, N, 3, HEADS, C // HEADS).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        attn = ((q @ k.transpose(-2, -1)) * (C // HEADS) ** -0.5).softmax(dim=-1)
        x = x + m["proj"]((attn @ v).transpose(1, 2).reshape(B, N, C))
        return x + m["fc2"](m["act"](m["fc1"](m["norm2"](x))))
    return where, fwd


def upstream_grads(case, dtype=torch.float64):
    """(y, the twelve gradients by GRADS) from torch autograd through the torch.nn Block."""
    where, fwd = build_upstream(case, dtype)
    x = _t(case["x"]).to(dtype).requires_grad_(True)
    y = fwd(x)
    y.backward(_t(case["G"]).to(dtype))
    grads = {"x": x.grad}
    grads.update({k: prm.grad for k, prm in where.items()})
    return y.detach(), grads


def chain(cases_params, x, G):
    """Blocks chained: cases_params a list of cases (their x and G ignored); returns (y, [grads per block]) in float64, the
    gradient of each block's input handed to the block before."""
    B, R = x.shape[0], x.shape[1]
    xs, cur = [], np.asarray(x, dtype=np.float64)
    for c in cases_params:
        cc = dict(c, x=cur, B=B, R=R)
        xs.append(cc)
        cur = forward(cc)["y"].numpy()
    grads, g = [None] * len(xs), np.asarray(G, dtype=np.float64)
    for i in reversed(range(len(xs))):
        grads[i] = backward(xs[i], g)
        g = grads[i]["x"].numpy()
    return torch.as_tensor(cur), grads


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    den = ref.abs().max().item()
    return (got - ref).abs().max().item() / (den if den > 0 else 1.0)
