"""Float64 CPU restatement of the ConvNextBlock at the end of each lateral (model/model_utils.py:306-354) in this project's
order, with the analytic backward that mirrors autograd.LateralBlock's launch sequence: the yardstick of
tests/test_lateral_train.py.  tools/gen_lateral_golden.py pins it to torch autograd through torch.nn layers built with
upstream's arguments.

    x [B,D,T,h,w]                                                                                                   (NCDHW)
    a = dw (7,1,1) pad (3,0,0) of x with wt, bt        b = dw (1,7,7) pad (0,3,3) of a with ws, bs
    n = gam (b - mean_c) rstd_c + bet                  per position over the D channels, biased variance, eps 1e-5
    z = W1 n + b1 [4D]      g = z Phi(z)      y = x + W2 g + b2
The scalar differentiated is <y, G> for a stored G."""
import math

import numpy as np
import torch
import torch.nn.functional as F

PARAMS = ("wt", "bt", "ws", "bs", "gam", "bet", "w1", "b1", "w2", "b2")       # the order of autograd.LateralBlock's arguments
NAMES = ("x",) + PARAMS                                                       # the 11 gradients
EPS = 1e-5
STATE_KEYS = {"wt": "dwconv_t.weight", "bt": "dwconv_t.bias", "ws": "dwconv_s.weight", "bs": "dwconv_s.bias",
              "gam": "norm.norm.weight", "bet": "norm.norm.bias", "w1": "pwconv1.weight", "b1": "pwconv1.bias",
              "w2": "pwconv2.weight", "b2": "pwconv2.bias"}                    # below latlayer_k[-1]


def param_shapes(D):
    return {"wt": (D, 1, 7, 1, 1), "bt": (D,), "ws": (D, 1, 1, 7, 7), "bs": (D,), "gam": (D,), "bet": (D,),
            "w1": (4 * D, D, 1, 1, 1), "b1": (4 * D,), "w2": (D, 4 * D, 1, 1, 1), "b2": (D,)}


def make_case(B, T, h, w, seed, D=32):
    """fp32 numpy inputs: x and G standard normal, weights N(0, 0.3^2), biases N(0, 0.1^2), the LayerNorm weight 1 + N(0, 0.1^2)."""
    rng = np.random.RandomState(seed)
    out = {"x": rng.randn(B, D, T, h, w).astype(np.float32)}
    for k, shape in param_shapes(D).items():
        if k == "gam":
            out[k] = (1.0 + 0.1 * rng.randn(*shape)).astype(np.float32)
        else:
            out[k] = ((0.3 if k.startswith("w") else 0.1) * rng.randn(*shape)).astype(np.float32)
    out["G"] = rng.randn(B, D, T, h, w).astype(np.float32)
    return out


def _rows(t):
    return t.permute(0, 2, 3, 4, 1)


def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def gelu_parts(z):
    """(Phi(z), phi(z)) of the standard normal."""
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))), torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def layernorm_rows(b, eps=EPS):
    """Rows [..., C] -> (x^, mean, rstd), biased variance."""
    mean = b.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((b - mean) ** 2).mean(-1, keepdim=True) + eps)
    return (b - mean) * rstd, mean, rstd


def forward(p, dtype=torch.float64):
    """The block's intermediates and its output y (NCDHW); a, b as the forward saves them, the rest as the backward recomputes."""
    q = {k: torch.as_tensor(p[k]).to(dtype) for k in NAMES}
    D = q["x"].shape[1]
    a = F.conv3d(q["x"], q["wt"], q["bt"], padding=(3, 0, 0), groups=D)
    b = F.conv3d(a, q["ws"], q["bs"], padding=(0, 3, 3), groups=D)
    xh, mean, rstd = layernorm_rows(_rows(b))
    n = xh * q["gam"] + q["bet"]
    z = n @ q["w1"].flatten(1).t() + q["b1"]
    g = z * gelu_parts(z)[0]
    y = q["x"] + _ncdhw(g @ q["w2"].flatten(1).t() + q["b2"])
    return {"a": a, "b": b, "xh": xh, "rstd": rstd, "n": n, "z": z, "g": g, "y": y}


def gelu_bwd(z, dg):
    cdf, pdf = gelu_parts(z)
    return z * cdf, dg * (cdf + z * pdf)


def layernorm_bwd(dy, x, gamma, eps=EPS):
    """Rows [..., C]: (dx, dgamma, dbeta) of y = gamma x^ + beta."""
    xh, _, rstd = layernorm_rows(x, eps)
    a = dy * gamma
    dx = rstd * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
    C = x.shape[-1]
    return dx, (dy * xh).reshape(-1, C).sum(0), dy.reshape(-1, C).sum(0)


def dwconv_wgrad(x, dy, k, pad):
    """dW[c,0,kt,kh,kw] = sum dy[p] x[p + tap - pad] with x zero outside the frame, db[c] = sum dy; NCDHW, stride 1, "same"."""
    xp = F.pad(x, (pad[2], pad[2], pad[1], pad[1], pad[0], pad[0]))
    _, Cc, T, H, W = dy.shape
    dW = torch.zeros(Cc, 1, *k, dtype=dy.dtype)
    for t in range(k[0]):
        for i in range(k[1]):
            for j in range(k[2]):
                dW[:, 0, t, i, j] = (dy * xp[:, :, t:t + T, i:i + H, j:j + W]).sum((0, 2, 3, 4))
    return dW, dy.sum((0, 2, 3, 4))


def backward(p, sv, G, dtype=torch.float64):
    """The 11 gradients of <y, G> in autograd.LateralBlock.backward's order of launches."""
    q = {k: torch.as_tensor(p[k]).to(dtype) for k in NAMES}
    D = q["x"].shape[1]
    G = torch.as_tensor(G).to(dtype)
    Gr = _rows(G)
    w1, w2 = q["w1"].flatten(1), q["w2"].flatten(1)
    dg = Gr @ w2
    g, dz = gelu_bwd(sv["z"], dg)
    out = {"w2": (Gr.reshape(-1, D).t() @ g.reshape(-1, 4 * D)).view_as(q["w2"]), "b2": Gr.reshape(-1, D).sum(0)}
    out["w1"] = (dz.reshape(-1, 4 * D).t() @ sv["n"].reshape(-1, D)).view_as(q["w1"])
    out["b1"] = dz.reshape(-1, 4 * D).sum(0)
    dn = dz @ w1
    db_rows, out["gam"], out["bet"] = layernorm_bwd(dn, _rows(sv["b"]), q["gam"])
    db = _ncdhw(db_rows).contiguous()
    da = F.conv3d(db, q["ws"].flip(2, 3, 4), None, padding=(0, 3, 3), groups=D)
    out["ws"], out["bs"] = dwconv_wgrad(sv["a"], db, (1, 7, 7), (0, 3, 3))
    out["wt"], out["bt"] = dwconv_wgrad(q["x"], da, (7, 1, 1), (3, 0, 0))
    out["x"] = G + F.conv3d(da, q["wt"].flip(2, 3, 4), None, padding=(3, 0, 0), groups=D)
    return out


def upstream_block(p, dtype=torch.float64):
    """torch.nn layers with upstream's arguments (model/model_utils.py:318-327), loaded with the case's parameters."""
    D = p["x"].shape[1]
    mods = {"dwconv_t": torch.nn.Conv3d(D, D, kernel_size=(7, 1, 1), padding=(3, 0, 0), groups=D),
            "dwconv_s": torch.nn.Conv3d(D, D, kernel_size=(1, 7, 7), padding=(0, 3, 3), groups=D),
            "norm": torch.nn.LayerNorm(D), "pwconv1": torch.nn.Conv3d(D, 4 * D, 1), "act": torch.nn.GELU(),
            "pwconv2": torch.nn.Conv3d(4 * D, D, 1)}
    assert mods["norm"].eps == EPS and mods["act"].approximate == "none"
    named = {"wt": mods["dwconv_t"].weight, "bt": mods["dwconv_t"].bias, "ws": mods["dwconv_s"].weight, "bs": mods["dwconv_s"].bias,
             "gam": mods["norm"].weight, "bet": mods["norm"].bias, "w1": mods["pwconv1"].weight, "b1": mods["pwconv1"].bias,
             "w2": mods["pwconv2"].weight, "b2": mods["pwconv2"].bias}
    for m in mods.values():
        m.to(dtype)
    with torch.no_grad():
        for k, t in named.items():
            t.copy_(torch.as_tensor(p[k]).to(dtype))
    return mods, named


def upstream_grads(p, dtype=torch.float64):
    """(y, {name: gradient of <y, G>}) by torch autograd through upstream's layers in upstream's order."""
    mods, named = upstream_block(p, dtype)
    x = torch.as_tensor(p["x"]).to(dtype).requires_grad_(True)
    t = mods["dwconv_s"](mods["dwconv_t"](x))
    t = mods["norm"](t.permute(0, 2, 3, 4, 1)).permute(0, 4, 1, 2, 3)
    y = x + mods["pwconv2"](mods["act"](mods["pwconv1"](t)))
    (y * torch.as_tensor(p["G"]).to(dtype)).sum().backward()
    grads = {k: t.grad.detach() for k, t in named.items()}
    grads["x"] = x.grad.detach()
    return y.detach(), grads
