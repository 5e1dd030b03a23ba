"""Float64 CPU restatement of the decoder's readout tail in this project's order (conv, then up-sample) with its analytic
backward: the yardstick of tests/test_readout_tail.py.  tools/gen_readout_tail_golden.py pins it to upstream's order
(up-sample, then conv; model/model_utils.py:403-409) built from torch.nn layers, values and all seven gradients.

    y4  [B,64,4,h,w]                                  (NCDHW, as torch holds it)
    a8  = conv (4,1,1)/(4,1,1) 64 -> 32 + b8          [B,32,h,w]
    up  = bilinear x4 (align_corners=False) of a8     [B,32,H,W]      u   = relu(up)
    p10 = conv (3,3) pad 1, 32 -> 32 + b10                            y10 = relu(p10)
    z   = conv (3,3) pad 1, 32 -> 1 + b12             [B,H,W]
    out = z - logsumexp(z) per sample
"""
import numpy as np
import torch
import torch.nn.functional as F

PARAMS = ("w8", "b8", "w10", "b10", "w12", "b12")
PARAM_SHAPES = {"w8": (32, 64, 4, 1, 1), "b8": (32,), "w10": (32, 32, 1, 3, 3), "b10": (32,), "w12": (1, 32, 1, 3, 3), "b12": (1,)}
STATE_KEYS = {"w8": "readout.8.weight", "b8": "readout.8.bias", "w10": "readout.10.weight", "b10": "readout.10.bias",
              "w12": "readout.12.weight", "b12": "readout.12.bias"}


def make_case(B, h, w, seed):
    """fp32 numpy inputs: y4 [B,64,4,h,w] non-negative with about 30 % exact zeros (a ReLU output), the six parameters at the
    scale of torch's default initialisation, and an upstream gradient g [B,4h,4w]."""
    rng = np.random.RandomState(seed)
    out = {"y4": np.maximum(rng.randn(B, 64, 4, h, w) + 0.5244, 0.0).astype(np.float32)}
    for k in PARAMS:
        shape = PARAM_SHAPES[k]
        fan_in = {"8": 256, "10": 288, "12": 288}[k[1:]]
        out[k] = (rng.uniform(-1.0, 1.0, shape) / np.sqrt(fan_in)).astype(np.float32)
    out["g"] = rng.randn(B, 4 * h, 4 * w).astype(np.float32)
    return out


def up_matrix(n, k):
    """[n k, n] float64 matrix of the bilinear up-sample by k along one axis: align_corners=False, source coordinate
    max(0, (dst + 0.5) / k - 0.5), second tap clamped to n - 1."""
    m = torch.zeros(n * k, n, dtype=torch.float64)
    for o in range(n * k):
        f = max(0.0, (o + 0.5) / k - 0.5)
        i0 = int(f)
        i1 = min(i0 + 1, n - 1)
        lam = f - i0
        m[o, i0] += 1.0 - lam
        m[o, i1] += lam
    return m


def _d(t):
    return torch.as_tensor(t).double()


def forward(y4, p, dtype=torch.float64):
    """Returns a dict: out [B,H,W] and the saved tensors a8, up (before its ReLU), u, p10 (before its ReLU), y10, z."""
    y4 = torch.as_tensor(y4).to(dtype)
    q = {k: torch.as_tensor(p[k]).to(dtype) for k in PARAMS}
    B, _, _, h, w = y4.shape
    a8 = F.conv3d(y4, q["w8"], q["b8"], stride=(4, 1, 1))[:, :, 0]
    uh, uw = up_matrix(h, 4).to(dtype), up_matrix(w, 4).to(dtype)
    up = torch.einsum("Hh,bchw,Ww->bcHW", uh, a8, uw)
    u = up.clamp_min(0)
    p10 = F.conv2d(u, q["w10"][:, :, 0], q["b10"], padding=1)
    y10 = p10.clamp_min(0)
    z = F.conv2d(y10, q["w12"][:, :, 0], q["b12"], padding=1)[:, 0]
    out = z - torch.logsumexp(z.flatten(1), 1).view(-1, 1, 1)
    return {"out": out, "a8": a8, "up": up, "u": u, "p10": p10, "y10": y10, "z": z}


def backward(y4, p, saved, g, masks=None):
    """Analytic gradients of sum(out * g): a dict with y4 and the six parameters.  masks = (mask_u, mask_10), boolean
    [B,32,H,W] each: the ReLU masks to use in place of the restatement's own (up > 0, p10 > 0)."""
    y4, g = _d(y4), _d(g)
    q = {k: _d(p[k]) for k in PARAMS}
    B, _, _, h, w = y4.shape
    mask_u, mask_10 = (saved["up"] > 0, saved["p10"] > 0) if masks is None else masks
    out, u, y10 = _d(saved["out"]), _d(saved["u"]), _d(saved["y10"])
    dz = g - out.exp() * g.flatten(1).sum(1).view(-1, 1, 1)
    dz1 = dz[:, None]
    w12, w10 = q["w12"][:, :, 0], q["w10"][:, :, 0]
    grads = {"b12": dz.sum().view(1), "w12": torch.nn.grad.conv2d_weight(y10, w12.shape, dz1, padding=1)[:, :, None]}
    d10 = torch.nn.grad.conv2d_input(y10.shape, w12, dz1, padding=1) * mask_10
    grads["b10"] = d10.sum((0, 2, 3))
    grads["w10"] = torch.nn.grad.conv2d_weight(u, w10.shape, d10, padding=1)[:, :, None]
    grads["du_raw"] = torch.nn.grad.conv2d_input(u.shape, w10, d10, padding=1)     # in front of the up-sample's ReLU mask
    du = grads["du_raw"] * mask_u
    d8 = torch.einsum("Hh,bcHW,Ww->bchw", up_matrix(h, 4), du, up_matrix(w, 4))
    grads["b8"] = d8.sum((0, 2, 3))
    grads["w8"] = torch.einsum("bohw,bithw->oit", d8, y4)[:, :, :, None, None]
    grads["y4"] = torch.einsum("bohw,oit->bithw", d8, q["w8"][:, :, :, 0, 0])
    grads["dz"], grads["d10"], grads["du"], grads["d8"] = dz, d10, du, d8
    return grads


def min_preactivation(saved):
    """Smallest |pre-activation| of the two ReLUs: how close the case sits to a kink."""
    return min(saved["up"].abs().min().item(), saved["p10"].abs().min().item())
