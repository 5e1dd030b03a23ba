"""The SyncBlock in training, on one GPU: (a) the attention backward alone, (b) one Block forward + backward with all twelve
gradients, (c) the linear weight gradient alone, (d) the whole SyncBlock forward + backward with all 39 gradients.

    python tools/sync_block_bench.py [--reps 10] [--rounds 3] [--parts abcd] [--json OUT]

At x3dl's shapes: 8 clips and 2 clips, 224 x 384 with the 257 x 300 spectrogram (16 * 7 * 12 + 90 = 1 434 tokens) and 224 x 224
with 36 audio tokens (820), dim 512, 4 heads of 128.  (a) engine.attention_bwd on a [rows][3][4][128] slab against torch's
autograd through softmax(scale q k^T) v on the same operands (backward only: the graph is built once and kept), timed in the
same rounds, alternating; FLOPs from shapes (five N x N x 128 products a head, the recomputed scores of the statistics pass
and of the second launch not counted) over time, against the 157 TFLOP/s of the fp32 MFMA.  (b) autograd.TransformerBlock
forward + backward under both routes of autograd.linear_wgrad_route -- "linear", mspi_linear_wgrad, and "sliced", the path the
Block had before -- against the same block in torch ops with torch autograd, the three alternating in every round; the
per-launch split of the hand-written path comes from engine.Profiler in a separate pass.  (c) engine.linear_wgrad on the
Block's four layers and on vis_proj (x3dl: 192 -> 512, on the visual tokens) against autograd.wgrad_wide_sliced and torch's
dy.t() @ x on the same operands, alternating; 2 M N K FLOP over time against the same peak.  (d) autograd.sync_block forward +
backward with all 39 gradients against the same layers in torch ops with torch autograd.  One warm-up call each, then `reps`
calls inside one pair of device events, in rounds.  Prints one JSON line.  Needs the GPU."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from entry_bench import spread  # noqa: E402
from readout_tail_bench import timed  # noqa: E402

PEAK_F32_TFLOPS = 157.0
SHAPES = [("8 x 224x384 + 257x300", 8, 1434), ("2 x 224x384 + 257x300", 2, 1434), ("8 x 224x224 + 36", 8, 820), ("2 x 224x224 + 36", 2, 820)]
HEADS, HD, DIM = 4, 128, 512


def attention_alone(E, dev, B, N, reps, rounds):
    gen = torch.Generator().manual_seed(7)
    qkv_t = torch.randn(B * N, 3 * DIM, generator=gen).to(dev)
    dO_t = torch.randn(B * N, DIM, generator=gen).to(dev)
    scale = HD ** -0.5
    qkv = E.from_rows(qkv_t).reshape(B, N, 1, 1)
    dO = E.from_rows(dO_t).reshape(B, N, 1, 1)
    q, k, v = (t.detach().requires_grad_(True) for t in qkv_t.view(B, N, 3, HEADS, HD).permute(2, 0, 3, 1, 4))
    o_t = torch.softmax(scale * q @ k.transpose(-2, -1), -1) @ v
    g_t = dO_t.view(B, N, HEADS, HD).transpose(1, 2)
    o = E.from_rows(o_t.detach().transpose(1, 2).reshape(B * N, DIM).contiguous()).reshape(B, N, 1, 1)
    out = E.alloc(B, N, 1, 1, 3 * DIM, dev)
    paths = {"hip": lambda: E.attention_bwd(qkv, o, dO, B, N, HEADS, HD, scale, out=out),
             "torch": lambda: torch.autograd.grad(o_t, (q, k, v), g_t, retain_graph=True)}
    got, want = paths["hip"](), paths["torch"]()                                          # warm-up, and a check
    want = torch.stack(want, 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * DIM)
    diff = ((got.as_rows() - want).abs().max() / want.abs().max()).item()
    del want
    times = {n: [] for n in paths}
    for _ in range(rounds):
        for n, fn in paths.items():
            times[n].append(timed(fn, reps))
    flops = 5 * 2.0 * B * HEADS * N * N * HD
    ms = min(times["hip"])
    return {"B": B, "tokens": N, "ms": {n: round(min(v), 4) for n, v in times.items()}, "ms_spread": {n: spread(v) for n, v in times.items()},
            "TFLOP_per_s": round(flops / (1e9 * ms), 2), "of_fp32_mfma_peak": round(flops / (1e9 * ms) / PEAK_F32_TFLOPS, 3),
            "rel_diff_vs_torch_fp32": diff}


def block_step(E, A, SR, dev, B, N, reps, rounds):
    case = SR.make_case(B, N, 3)
    where, fwd = SR.build_upstream(case, torch.float32)
    for p in where.values():
        p.data = p.data.to(dev)
    ps = [torch.from_numpy(case[k]).float().to(dev).requires_grad_(True) for k in SR.NAMES]
    x = torch.from_numpy(case["x"]).float().to(dev).requires_grad_(True)
    G = torch.from_numpy(case["G"]).float().to(dev)
    ref_wrt = [x] + [where[k] for k in SR.NAMES]

    route = {"now": "linear"}
    A.linear_wgrad_route = lambda M, N_, K: route["now"]                                  # both routes in one process

    def hip(which):
        def run():
            route["now"] = which
            return torch.autograd.grad(A.TransformerBlock.apply(x, *ps), [x] + ps, G)
        return run

    def ref():
        return torch.autograd.grad(fwd(x), ref_wrt, G)
    paths = {"linear": hip("linear"), "sliced": hip("sliced"), "torch": ref}
    got, old, want = paths["linear"](), paths["sliced"](), ref()                          # warm-up, and a check
    diffs = {n: ((got[i] - want[i]).abs().max() / want[i].abs().max().clamp_min(1e-30)).item() for i, n in enumerate(SR.GRADS)}
    diffs_sliced = {n: ((old[i] - want[i]).abs().max() / want[i].abs().max().clamp_min(1e-30)).item() for i, n in enumerate(SR.GRADS)}
    del got, old, want
    torch.cuda.synchronize()
    times = {n: [] for n in paths}
    for _ in range(rounds):
        for n, fn in paths.items():
            times[n].append(timed(fn, reps))
    launches = {}
    for which in ("linear", "sliced"):
        with E.Profiler() as prof:
            paths[which]()
            torch.cuda.synchronize()
        launches[which] = {k: [v["calls"], round(v["ms"], 4)] for k, v in sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])}
    route["now"] = "linear"
    return {"B": B, "tokens": N, "ms": {k: round(min(v), 3) for k, v in times.items()},
            "ms_rounds": {k: [round(t, 3) for t in v] for k, v in times.items()}, "ms_spread": {k: spread(v) for k, v in times.items()},
            "launch_calls_ms": launches, "grad_rel_diff_vs_torch_fp32": diffs, "sliced_grad_rel_diff_vs_torch_fp32": diffs_sliced}


def linear_alone(E, A, dev, B, N, reps, rounds):
    """Part (c): the Block's four layers on B * N rows and vis_proj on the visual tokens (x3dl: C4 = 192)."""
    Rv = N - (90 if N == 1434 else 36)
    layers = [("qkv", B * N, 3 * DIM, DIM), ("proj", B * N, DIM, DIM), ("fc1", B * N, 4 * DIM, DIM), ("fc2", B * N, DIM, 4 * DIM),
              ("vis_proj", B * Rv, DIM, 192)]
    gen = torch.Generator().manual_seed(11)
    rows = []
    for name, M, No, K in layers:
        x_t, dy_t = torch.randn(M, K, generator=gen).to(dev), torch.randn(M, No, generator=gen).to(dev)
        x, dy = E.from_rows(x_t), E.from_rows(dy_t)
        paths = {"linear": lambda: E.linear_wgrad(x, dy), "sliced": lambda: A.wgrad_wide_sliced(x, dy, (1, 1, 1), (0, 0, 0)),
                 "torch": lambda: (dy_t.t() @ x_t, dy_t.sum(0))}
        got, old, want = (fn() for fn in paths.values())                                  # warm-up, and a check
        diff = ((got[0] - want[0]).abs().max() / want[0].abs().max()).item()
        same = bool(torch.equal(E.linear_wgrad(x, dy)[0], got[0]))
        del got, old, want
        times = {n: [] for n in paths}
        for _ in range(rounds):
            for n, fn in paths.items():
                times[n].append(timed(fn, reps))
        flops, ms = 2.0 * M * No * K, min(times["linear"])
        rows.append({"layer": name, "M": M, "N": No, "K": K, "rows_per_slice": E.linear_wgrad_variant(x, dy),
                     "ws_MB": round(E._lib.load().mspi_linear_wgrad_ws_bytes(M, No, K) / 2 ** 20, 2),
                     "ms": {n: round(min(v), 4) for n, v in times.items()}, "ms_spread": {n: spread(v) for n, v in times.items()},
                     "TFLOP_per_s": round(flops / (1e9 * ms), 2), "of_fp32_mfma_peak": round(flops / (1e9 * ms) / PEAK_F32_TFLOPS, 3),
                     "rel_diff_vs_torch_fp32": diff, "repeatable": same})
    return rows


def sync_step(E, A, TR, dev, B, N, reps, rounds):
    """Part (d): autograd.sync_block forward + backward, all 39 gradients, against the same layers in torch ops."""
    import torch.nn as nn
    from mspi_amd.model import model_utils as pm
    Ra = 90 if N == 1434 else 36
    thw = (16, 7, 12) if N == 1434 else (16, 7, 7)
    case = TR.make_case(B, thw, (1, Ra), 192, 5)
    m = pm.SyncBlock(num_blocks=3, num_vis_tokens=N - Ra, num_aud_tokens=Ra, vis_in_embed=192).to(dev).eval()
    vis, aud = (torch.from_numpy(case[k]).float().to(dev) for k in ("vis", "aud"))
    G = torch.from_numpy(case["G"]).float().to(dev)
    params = list(m.parameters())
    vpos, apos = m.vis_pos_embed[0].to(dev), m.aud_pos_embed[0].to(dev)

    def torch_block(blk, x):
        Bq, Nq, Cq = x.shape
        qkv = nn.functional.linear(nn.functional.layer_norm(x, (Cq,), blk.norm1.weight, blk.norm1.bias), blk.attn.qkv.weight)
        q, k, v = qkv.reshape(Bq, Nq, 3, HEADS, HD).permute(2, 0, 3, 1, 4).unbind(0)
        o = (torch.softmax(q @ k.transpose(-2, -1) * HD ** -0.5, -1) @ v).transpose(1, 2).reshape(Bq, Nq, Cq)
        x = x + nn.functional.linear(o, blk.attn.proj.weight, blk.attn.proj.bias)
        h = nn.functional.gelu(nn.functional.linear(nn.functional.layer_norm(x, (Cq,), blk.norm2.weight, blk.norm2.bias),
                                                    blk.mlp.fc1.weight, blk.mlp.fc1.bias))
        return x + nn.functional.linear(h, blk.mlp.fc2.weight, blk.mlp.fc2.bias)

    def ref():
        v = nn.functional.layer_norm(m.vis_proj(vis.view(B, N - Ra, 192)), (DIM,), m.vis_norm.weight, m.vis_norm.bias) + vpos
        a = nn.functional.layer_norm(aud.view(B, Ra, DIM), (DIM,), m.aud_norm.weight, m.aud_norm.bias) + apos
        x = torch.cat([v, a], 1)
        for blk in m.blocks:
            x = torch_block(blk, x)
        return torch.autograd.grad(x, params, G)

    def hip():
        return torch.autograd.grad(A.sync_block(m, vis, aud), params, G)
    paths = {"hip": hip, "torch": ref}
    got, want = hip(), ref()                                                              # warm-up, and a check
    worst = max(((g - w).abs().max() / w.abs().max().clamp_min(1e-30)).item() for g, w in zip(got, want))
    del got, want
    torch.cuda.synchronize()
    times = {n: [] for n in paths}
    for _ in range(rounds):
        for n, fn in paths.items():
            times[n].append(timed(fn, reps))
    return {"B": B, "tokens": N, "ms": {k: round(min(v), 3) for k, v in times.items()},
            "ms_rounds": {k: [round(t, 3) for t in v] for k, v in times.items()}, "worst_grad_rel_diff_vs_torch_fp32": worst}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", type=str, default="abcd")
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sync_block_bench needs an MI355X (no CPU fallback)")
    import sync_block_restate as SR
    import sync_tokens_restate as TR
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    E.autotune(False)
    dev = torch.device("cuda", 0)
    out = {"reps": args.reps, "rounds": args.rounds, "shapes": {}, "device": torch.cuda.get_device_name(0)}
    for name, B, N in SHAPES:
        row = out["shapes"][name] = {}
        if "a" in args.parts:
            row["attention_bwd"] = attention_alone(E, dev, B, N, args.reps, args.rounds)
        if "b" in args.parts:
            row["block"] = block_step(E, A, SR, dev, B, N, args.reps, args.rounds)
        if "c" in args.parts:
            row["linear_wgrad"] = linear_alone(E, A, dev, B, N, args.reps, args.rounds)
        if "d" in args.parts:
            row["sync_block"] = sync_step(E, A, TR, dev, B, N, args.reps, args.rounds)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
