"""Float64 restatement of the whole SyncBlock (model/model_utils.py:223-282 upstream) in this project's order: the embedding in
front of the blocks -- vis_norm(vis_proj(vis)) + table, aud_norm(aud) + table, concatenated along the tokens -- with its analytic
backward in the launch order of mspi_amd.autograd.SyncEmbed, and the three transformer Blocks behind it from
tests/sync_block_restate.py, which is imported as it stands.  No GPU, no project code: the tests hold the kernels to this file,
and this file to torch autograd (upstream_grads, tools/gen_sync_tokens_golden.py)."""
import math

import numpy as np
import torch

import sync_block_restate as SR

DIM, EPS, NBLOCKS = SR.DIM, SR.EPS, 3
EMBED = ("wp", "bp", "gv", "bv", "ga", "ba")      # SyncEmbed's argument order behind vis and aud
EMBED_GRADS = ("vis", "aud") + EMBED


def sinusoid(n):
    """The positional table [n, 512] the module holds: sin on the even columns, cos on the odd, of pos / 10000^(2 (c // 2) / 512),
    rounded to float32 as the module stores it, handed back in float64."""
    pos = np.arange(n, dtype=np.float64)[:, None]
    col = np.arange(DIM)[None, :]
    ang = pos / np.power(10000.0, 2 * (col // 2) / DIM)
    tab = np.where(col % 2 == 0, np.sin(ang), np.cos(ang))
    return tab.astype(np.float32).astype(np.float64)


def make_case(B, vis_thw, aud_ft, C4, seed):
    """vis [B,t,h,w,C4], aud [B,1,F,T',512] and G [B,Rv+Ra,512] standard normal, vis_proj xavier-uniform with a N(0, 0.1^2) bias,
    LayerNorm weights 1 + N(0, 0.1^2) and biases N(0, 0.1^2), drawn from RandomState(seed) in a fixed order; the three blocks'
    tensors are those of sync_block_restate.make_case(1, 1, seed + 1 + i)."""
    rs = np.random.RandomState(seed)
    t, h, w = vis_thw
    F, T = aud_ft
    Rv, Ra = t * h * w, F * T
    c = {"B": B, "thw": tuple(vis_thw), "ft": tuple(aud_ft), "C4": C4, "Rv": Rv, "Ra": Ra, "seed": seed}
    c["vis"] = rs.standard_normal((B, t, h, w, C4))
    c["aud"] = rs.standard_normal((B, 1, F, T, DIM))
    c["G"] = rs.standard_normal((B, Rv + Ra, DIM))
    a = math.sqrt(6.0 / (C4 + DIM))
    c["wp"], c["bp"] = rs.uniform(-a, a, (DIM, C4)), 0.1 * rs.standard_normal(DIM)
    c["gv"], c["bv"] = 1.0 + 0.1 * rs.standard_normal(DIM), 0.1 * rs.standard_normal(DIM)
    c["ga"], c["ba"] = 1.0 + 0.1 * rs.standard_normal(DIM), 0.1 * rs.standard_normal(DIM)
    c["vpos"], c["apos"] = sinusoid(Rv), sinusoid(Ra)
    c["blocks"] = [SR.make_case(1, 1, seed + 1 + i) for i in range(NBLOCKS)]
    return c


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def embed_forward(case):
    """(slab [B, Rv+Ra, 512], p = vis_proj(vis) [B, Rv, 512]) in float64."""
    B, Rv, Ra = case["B"], case["Rv"], case["Ra"]
    p = _t(case["vis"]).reshape(B, Rv, -1) @ _t(case["wp"]).t() + _t(case["bp"])
    v = SR.layernorm(p, _t(case["gv"]), _t(case["bv"])) + _t(case["vpos"])
    a = SR.layernorm(_t(case["aud"]).reshape(B, Ra, DIM), _t(case["ga"]), _t(case["ba"])) + _t(case["apos"])
    return torch.cat([v, a], 1), p


def embed_backward(case, G=None):
    """The eight gradients (dict by EMBED_GRADS) for the slab's gradient G (default case["G"]), in SyncEmbed's launch order."""
    B, Rv, Ra, C4 = case["B"], case["Rv"], case["Ra"], case["C4"]
    G = _t(case["G"] if G is None else G)
    _, p = embed_forward(case)
    out = {}
    dp, out["gv"], out["bv"] = SR.layernorm_bwd(G[:, :Rv], p, _t(case["gv"]))
    rows = dp.reshape(B * Rv, DIM)
    out["wp"], out["bp"] = rows.t() @ _t(case["vis"]).reshape(B * Rv, C4), rows.sum(0)
    da, out["ga"], out["ba"] = SR.layernorm_bwd(G[:, Rv:], _t(case["aud"]).reshape(B, Ra, DIM), _t(case["ga"]))
    out["vis"] = (dp @ _t(case["wp"])).reshape(case["vis"].shape)
    out["aud"] = da.reshape(case["aud"].shape)
    return out


def forward(case):
    """(embedding slab, output of the three blocks) in float64."""
    slab, _ = embed_forward(case)
    cur = slab
    for c in case["blocks"]:
        cur = SR.forward(dict(c, x=cur.numpy(), B=case["B"], R=case["Rv"] + case["Ra"]))["y"]
    return slab, cur


def backward(case):
    """(y, the embedding's eight gradients, [the twelve of each block]) for the output gradient case["G"]."""
    slab, _ = embed_forward(case)
    y, blocks = SR.chain(case["blocks"], slab.numpy(), case["G"])
    return y, embed_backward(case, blocks[0]["x"]), blocks


def upstream_grads(case, blocks=True, dtype=torch.float64):
    """(y, embedding gradients by EMBED_GRADS, [block gradients by SR.NAMES]) from torch autograd through nn.Linear, nn.LayerNorm
    and the torch.nn Blocks of sync_block_restate.build_upstream, with upstream's arguments; blocks=False: the embedding alone."""
    import torch.nn as nn
    B, Rv, Ra, C4 = case["B"], case["Rv"], case["Ra"], case["C4"]
    proj, vn, an = nn.Linear(C4, DIM).to(dtype), nn.LayerNorm(DIM, eps=EPS).to(dtype), nn.LayerNorm(DIM, eps=EPS).to(dtype)
    where = {"wp": proj.weight, "bp": proj.bias, "gv": vn.weight, "bv": vn.bias, "ga": an.weight, "ba": an.bias}
    with torch.no_grad():
        for k, prm in where.items():
            prm.copy_(_t(case[k]).to(dtype))
    vis = _t(case["vis"]).to(dtype).requires_grad_(True)
    aud = _t(case["aud"]).to(dtype).requires_grad_(True)
    v = vn(proj(vis.reshape(B, Rv, C4))) + _t(case["vpos"]).to(dtype)
    a = an(aud.reshape(B, Ra, DIM)) + _t(case["apos"]).to(dtype)
    y = torch.cat([v, a], dim=1)
    built = [SR.build_upstream(c, dtype) for c in case["blocks"]] if blocks else []
    for _, fwd in built:
        y = fwd(y)
    y.backward(_t(case["G"]).to(dtype))
    grads = {"vis": vis.grad, "aud": aud.grad}
    grads.update({k: prm.grad for k, prm in where.items()})
    return y.detach(), grads, [{k: prm.grad for k, prm in w.items()} for w, _ in built]
