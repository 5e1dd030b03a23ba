"""The SyncBlock's transformer Block in training, on one GPU: (a) the attention backward alone, (b) one Block forward + backward
with all twelve gradients.

    python tools/sync_block_bench.py [--reps 10] [--rounds 3] [--json OUT]

At x3dl's shapes: 8 clips and 2 clips, 224 x 384 with the 257 x 300 spectrogram (16 * 7 * 12 + 90 = 1 434 tokens) and 224 x 224
with 36 audio tokens (820), dim 512, 4 heads of 128.  (a) engine.attention_bwd on a [rows][3][4][128] slab against torch's
autograd through softmax(scale q k^T) v on the same operands (backward only: the graph is built once and kept), timed in the
same rounds, alternating; FLOPs from shapes (five N x N x 128 products a head, the recomputed scores of the statistics pass
and of the second launch not counted) over time, against the 157 TFLOP/s of the fp32 MFMA.  (b) autograd.TransformerBlock
forward + backward against the same block in torch ops with torch autograd; the per-launch split of the hand-written path
comes from engine.Profiler in a separate pass.  One warm-up call each, then `reps` calls inside one pair of device events, in
rounds.  Prints one JSON line.  Needs the GPU."""
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

    def hip():
        return torch.autograd.grad(A.TransformerBlock.apply(x, *ps), [x] + ps, G)

    def ref():
        return torch.autograd.grad(fwd(x), ref_wrt, G)
    got, want = hip(), ref()                                                              # warm-up, and a check
    diffs = {n: ((got[i] - want[i]).abs().max() / want[i].abs().max().clamp_min(1e-30)).item() for i, n in enumerate(SR.GRADS)}
    del got, want
    torch.cuda.synchronize()
    times = {"hip": [], "torch": []}
    for _ in range(rounds):
        times["hip"].append(timed(hip, reps))
        times["torch"].append(timed(ref, reps))
    with E.Profiler() as prof:
        hip()
        torch.cuda.synchronize()
    launches = {k: round(v["ms"], 4) for k, v in sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])}
    return {"B": B, "tokens": N, "ms": {k: round(min(v), 3) for k, v in times.items()},
            "ms_rounds": {k: [round(t, 3) for t in v] for k, v in times.items()}, "launch_ms": launches,
            "grad_rel_diff_vs_torch_fp32": diffs}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sync_block_bench needs an MI355X (no CPU fallback)")
    import sync_block_restate as SR
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    E.autotune(False)
    dev = torch.device("cuda", 0)
    out = {"reps": args.reps, "rounds": args.rounds, "shapes": {}, "device": torch.cuda.get_device_name(0)}
    for name, B, N in SHAPES:
        out["shapes"][name] = {"attention_bwd": attention_alone(E, dev, B, N, args.reps, args.rounds),
                               "block": block_step(E, A, SR, dev, B, N, args.reps, args.rounds)}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
