"""Float64 CPU restatement of the laterals' entry conv(s) (model/model_utils.py:440-470 upstream) in this project's order, with
the analytic backward that mirrors autograd.LateralEntry: the yardstick of tests/test_entry_train.py.
tools/gen_lateral_entry_golden.py pins it to torch autograd through nn.Conv3d(C, 192, 1) followed by
nn.Conv3d(192, 192, (s,1,1), (s,1,1), bias=False).

    x [B,C,T,h,w] (NCDHW), the concat of the two inputs where there are two
    compose:   Wc[co,ci,t] = sum_m W1[co,m,t] W0[m,ci],   bc[co] = sum_{m,t} W1[co,m,t] b0[m]        (no W1: Wc = W0, bc = b0)
    one conv:  y[n,co,to,h,w] = bc[co] + sum_{ci,t} Wc[co,ci,t] x[n,ci,to s + t,h,w],   To = floor(T / s)
    backward:  dWc[co,ci,t] = sum_r G[r][co] x[n,ci,to s + t,h,w],   dbc[co] = sum_r G[r][co]          (frames >= To s unread)
               dW1[co,m,t] = sum_ci dWc[co,ci,t] W0[m,ci] + dbc[co] b0[m]
               dW0[m,ci]   = sum_{co,t} W1[co,m,t] dWc[co,ci,t],   db0[m] = sum_{co,t} W1[co,m,t] dbc[co]
The scalar differentiated is <y, G> for a stored G.  x gets no gradient: the entry convs' inputs are frozen."""
import numpy as np
import torch

MID = 192
NAMES = ("w0", "b0", "w1")                                  # the gradients; "w1" is absent where there is no second conv
STATE_KEYS = {"w0": "0.weight", "b0": "0.bias", "w1": "1.weight"}       # below latlayer_k


def make_case(B, T, h, w, C, s, seed, second=True, mid=MID):
    """fp32 numpy inputs: x and G standard normal, W0 ~ N(0, 1 / C), W1 ~ N(0, 1 / (mid s)), b0 ~ N(0, 0.1^2).  second False:
    no second conv (s must be 1)."""
    rng = np.random.RandomState(seed)
    out = {"x": rng.randn(B, C, T, h, w).astype(np.float32),
           "w0": (rng.randn(mid, C, 1, 1, 1) / np.sqrt(C)).astype(np.float32),
           "b0": (0.1 * rng.randn(mid)).astype(np.float32)}
    if second:
        out["w1"] = (rng.randn(mid, mid, s, 1, 1) / np.sqrt(mid * s)).astype(np.float32)
    else:
        assert s == 1
    out["G"] = rng.randn(B, mid, T // s, h, w).astype(np.float32)
    out["s"] = s
    return out


def _t(case, k, dtype=torch.float64):
    return torch.from_numpy(case[k]).to(dtype)


def compose(case, dtype=torch.float64):
    """(Wc [co,ci,s], bc [co]) of the case."""
    w0, b0 = _t(case, "w0", dtype).flatten(1), _t(case, "b0", dtype)
    if "w1" not in case:
        return w0[:, :, None], b0
    w1 = _t(case, "w1", dtype)[:, :, :, 0, 0]
    return torch.einsum("omt,mi->oit", w1, w0), torch.einsum("omt,m->o", w1, b0)


def _lines(x, s):
    """x [B,C,T,h,w] -> [B,To,h,w,C,s]: the taps of every output row; trailing frames dropped."""
    B, C, T, h, w = x.shape
    To = T // s
    return x[:, :, :To * s].reshape(B, C, To, s, h, w).permute(0, 2, 4, 5, 1, 3)


def forward(case, x=None):
    """y [B,co,To,h,w] in float64.  x: another input than the case's (same shape)."""
    wc, bc = compose(case)
    x = _t(case, "x") if x is None else x.double()
    y = torch.einsum("nthwis,ois->nthwo", _lines(x, case["s"]), wc) + bc
    return y.permute(0, 4, 1, 2, 3)


def composed_grads(x, G, s):
    """(dWc [co,ci,s], dbc [co]) for x [B,C,T,h,w] and G [B,co,To,h,w], both float64."""
    Gr = G.permute(0, 2, 3, 4, 1)
    return torch.einsum("nthwo,nthwis->ois", Gr, _lines(x, s)), Gr.sum((0, 1, 2, 3))


def backward(case, G=None, x=None):
    """{name: gradient} in the parameters' nn layouts, float64."""
    x = _t(case, "x") if x is None else x.double()
    G = _t(case, "G") if G is None else G.double()
    dwc, dbc = composed_grads(x, G, case["s"])
    if "w1" not in case:
        return {"w0": dwc[:, :, :, None, None], "b0": dbc}
    w0, b0, w1 = _t(case, "w0").flatten(1), _t(case, "b0"), _t(case, "w1")[:, :, :, 0, 0]
    dw1 = torch.einsum("oit,mi->omt", dwc, w0) + dbc[:, None, None] * b0[None, :, None]
    dw0 = torch.einsum("omt,oit->mi", w1, dwc)
    db0 = torch.einsum("omt,o->m", w1, dbc)
    return {"w0": dw0[:, :, None, None, None], "b0": db0, "w1": dw1[:, :, :, None, None]}


def upstream_grads(case, dtype=torch.float64):
    """(y, {name: gradient}) by torch autograd through the two nn.Conv3d layers as upstream builds them."""
    s, mid, C = case["s"], case["w0"].shape[0], case["w0"].shape[1]
    c0 = torch.nn.Conv3d(C, mid, 1, 1, 0).to(dtype)
    layers = [c0]
    with torch.no_grad():
        c0.weight.copy_(_t(case, "w0", dtype))
        c0.bias.copy_(_t(case, "b0", dtype))
        if "w1" in case:
            c1 = torch.nn.Conv3d(mid, mid, kernel_size=(s, 1, 1), stride=(s, 1, 1), bias=False).to(dtype)
            c1.weight.copy_(_t(case, "w1", dtype))
            layers.append(c1)
    y = torch.nn.Sequential(*layers)(_t(case, "x", dtype))
    (y * _t(case, "G", dtype)).sum().backward()
    grads = {"w0": c0.weight.grad, "b0": c0.bias.grad}
    if "w1" in case:
        grads["w1"] = layers[1].weight.grad
    return y.detach(), grads
