"""One stride-1 X3D residual block in training, on one GPU: (a) autograd.X3DBlock forward + backward with all gradients against
the same block in torch ops with torch autograd, (b) the depthwise (3,3,3) weight gradient alone against torch's grouped-conv
weight gradient.

    python tools/x3d_block_bench.py [--reps 10] [--rounds 3] [--parts ab] [--json OUT]

At X3D-L's two last stages on 224 x 384 frames: (dim_out, dim_inner) = (192, 432) on 16 x 7 x 12 maps and (96, 216) on
16 x 14 x 24, 8 clips and 2 clips, with and without `se`.  (a) the block of tests/x3d_block_restate.py (upstream's torch.nn
layers in train() mode, fp32) on the same tensors, once on NCDHW-contiguous input ("torch") and once on channels_last_3d memory
("torch_cl"), the three alternating in every round; the per-launch split of the hand-written path comes from engine.Profiler in
a separate pass.  (b) engine.dwconv3_wgrad on [rows][dim_inner] operands against torch.autograd.grad of F.conv3d(groups = C)
with respect to its weight on the same operands (backward only: the graph is built once and kept), alternating; the bytes the
gradient needs (x and dy read once) over time.  One warm-up call each, then `reps` calls inside one pair of device events, in
rounds; the minimum and the spread over the rounds are reported.  The warm-up call's gradients are compared with torch's fp32
ones, in the largest entry of each tensor: a sanity figure, not a test -- at these row counts an element of bn_a's output within
fp32 rounding of zero can take the other side of the ReLU on either side, which a max-norm sees as 1e-2 on dx
(profiles/r24_x3d_block.txt section 2 holds both sides against float64).  Prints one JSON line.  Needs the GPU."""
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

# label, dim_out, dim_inner, clips, T, h, w
SHAPES = [("s5 192/432 8 x 16x7x12", 192, 432, 8, 16, 7, 12), ("s5 192/432 2 x 16x7x12", 192, 432, 2, 16, 7, 12),
          ("s4 96/216 8 x 16x14x24", 96, 216, 8, 16, 14, 24), ("s4 96/216 2 x 16x14x24", 96, 216, 2, 16, 14, 24)]


def rounds_of(paths, reps, rounds):
    times = {n: [] for n in paths}
    for _ in range(rounds):
        for n, fn in paths.items():
            times[n].append(timed(fn, reps))
    return times


def block_step(E, A, XR, dev, D, Ci, B, T, h, w, se, reps, rounds):
    case = XR.make_case(D, Ci, B, T, h, w, se, 3)
    m, mods = XR.upstream_block(case, torch.float32)
    m = m.to(dev)                                                                         # in place: mods still names its parameters
    names = [k for k in XR.PARAMS if k in case]
    ps = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) if k in case else None for k in XR.PARAMS]
    x = torch.from_numpy(case["x"]).to(dev).requires_grad_(True)
    G = torch.from_numpy(case["G"]).to(dev)
    x_nc = x.detach().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    x_cl = x.detach().permute(0, 4, 1, 2, 3).requires_grad_(True)                         # channels-last memory, NCDHW view: no copy
    G_nc, G_cl = G.permute(0, 4, 1, 2, 3).contiguous(), G.permute(0, 4, 1, 2, 3)
    wrt = [mods[k] for k in names]

    def hip():
        return torch.autograd.grad(A.X3DBlock.apply(x, *ps, None, None, None), [x] + [p for p in ps if p is not None], G)

    def ref(xt, Gt):
        return lambda: torch.autograd.grad(m(xt), [xt] + wrt, Gt)
    paths = {"hip": hip, "torch": ref(x_nc, G_nc), "torch_cl": ref(x_cl, G_cl)}
    got, want = hip(), paths["torch"]()                                                   # warm-up, and a check
    paths["torch_cl"]()
    diffs = {"x": ((got[0] - want[0].permute(0, 2, 3, 4, 1)).abs().max() / want[0].abs().max()).item()}
    diffs.update({k: ((g - r).abs().max() / r.abs().max().clamp_min(1e-30)).item() for k, g, r in zip(names, got[1:], want[1:])})
    del got, want
    torch.cuda.synchronize()
    times = rounds_of(paths, reps, rounds)
    with E.Profiler() as prof:
        hip()
        torch.cuda.synchronize()
    launches = {k: [v["calls"], round(v["ms"], 4)] for k, v in sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])}
    return {"se": bool(se), "rows": B * T * h * w, "ms": {k: round(min(v), 3) for k, v in times.items()},
            "ms_rounds": {k: [round(t, 3) for t in v] for k, v in times.items()}, "ms_spread": {k: spread(v) for k, v in times.items()},
            "launch_calls_ms": launches, "worst_grad_rel_diff_vs_torch_fp32": max(diffs.values()), "grad_rel_diff_vs_torch_fp32": diffs}


def wgrad_alone(E, A, dev, Ci, B, T, h, w, reps, rounds):
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, h, w, Ci, generator=gen).to(dev)
    dy = torch.randn(B, T, h, w, Ci, generator=gen).to(dev)
    xc, dc = A._cl5(x), A._cl5(dy)
    wt = torch.zeros(Ci, 1, 3, 3, 3, device=dev, requires_grad=True)
    out = {}
    refs = {}
    for name, xt, dt in (("torch", x.permute(0, 4, 1, 2, 3).contiguous(), dy.permute(0, 4, 1, 2, 3).contiguous()),
                         ("torch_cl", x.permute(0, 4, 1, 2, 3), dy.permute(0, 4, 1, 2, 3))):
        y = torch.nn.functional.conv3d(xt, wt, None, 1, 1, 1, Ci)
        refs[name] = (lambda y=y, dt=dt: torch.autograd.grad(y, wt, dt, retain_graph=True))
    paths = {"hip": lambda: E.dwconv3_wgrad(xc, dc), **refs}
    got, want = paths["hip"]()[0], paths["torch"]()[0]                                    # warm-up, and a check
    paths["torch_cl"]()
    out["rel_diff_vs_torch_fp32"] = ((got - want).abs().max() / want.abs().max()).item()
    out["repeatable"] = bool(torch.equal(E.dwconv3_wgrad(xc, dc)[0], got))
    torch.cuda.synchronize()
    times = rounds_of(paths, reps, rounds)
    d = E._dw_desc(xc, (3, 3, 3), (1, 1, 1), (1, 1, 1), dc.ld)
    ws = E._lib.load().mspi_dwconv3_wgrad_ws_bytes(E.C.byref(d))
    nbytes, ms = 8.0 * xc.M * Ci, min(times["hip"])
    out.update({"rows": xc.M, "C": Ci, "records": ws // (28 * Ci * 4), "ws_MB": round(ws / 2 ** 20, 2),
                "ms": {n: round(min(v), 4) for n, v in times.items()}, "ms_spread": {n: spread(v) for n, v in times.items()},
                "needed_GB_per_s": round(nbytes / (1e6 * ms), 1)})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", type=str, default="ab")
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("x3d_block_bench needs an MI355X (no CPU fallback)")
    import x3d_block_restate as XR
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    E.autotune(False)
    dev = torch.device("cuda", 0)
    out = {"reps": args.reps, "rounds": args.rounds, "shapes": {}, "device": torch.cuda.get_device_name(0)}
    for label, D, Ci, B, T, h, w in SHAPES:
        row = out["shapes"][label] = {}
        if "a" in args.parts:
            row["block"] = [block_step(E, A, XR, dev, D, Ci, B, T, h, w, se, args.reps, args.rounds) for se in (True, False)]
        if "b" in args.parts:
            row["dwconv3_wgrad"] = wgrad_alone(E, A, dev, Ci, B, T, h, w, args.reps, args.rounds)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
