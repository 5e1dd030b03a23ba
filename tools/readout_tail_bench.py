"""Forward + backward of the readout tail at the training shape, hand-written path against torch ops on the same GPU.

    python tools/readout_tail_bench.py [--batch 8] [--height 224] [--width 384] [--reps 20] [--json OUT]

Code under test: mspi_amd.autograd.ReadoutTail (four forward launches, the backward of csrc/readout_bwd.hip and the two
data-gradient convs), gradients for the six parameters and for the features y4.  Baseline, never the code under test: the same
tail in this project's order written in torch ops (F.conv3d, F.interpolate, F.conv2d, logsumexp) with torch autograd.  One
warm-up call each, then `reps` calls inside one pair of device events, the two paths alternating in rounds; the per-launch
split of the hand-written path comes from engine.Profiler in a separate pass.  Prints one JSON line.  Needs the GPU."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_tail(y4, w8, b8, w10, b10, w12, b12):
    """y4 [B,64,4,h,w] (NCDHW, channels-last memory is up to torch) -> log map [B,H,W]."""
    a8 = F.conv3d(y4, w8, b8, stride=(4, 1, 1))[:, :, 0]
    u = F.relu(F.interpolate(a8, scale_factor=4, mode="bilinear", align_corners=False))
    y10 = F.relu(F.conv2d(u, w10[:, :, 0], b10, padding=1))
    z = F.conv2d(y10, w12[:, :, 0], b12, padding=1)[:, 0]
    return z - torch.logsumexp(z.flatten(1), 1).view(-1, 1, 1)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=224)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("readout_tail_bench needs an MI355X (no CPU fallback)")
    import readout_tail_restate as RT
    from mspi_amd import engine as E
    from mspi_amd.autograd import ReadoutTail
    dev = torch.device("cuda", 0)
    B, h, w = args.batch, args.height // 4, args.width // 4
    case = RT.make_case(B, h, w, 1)
    params = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in RT.PARAMS]
    y4_nc = torch.from_numpy(case["y4"]).to(dev)
    y4_cl = y4_nc.permute(0, 2, 3, 4, 1).contiguous().requires_grad_(True)
    y4_nc.requires_grad_(True)
    g = torch.from_numpy(case["g"]).to(dev)

    def hip():
        torch.autograd.grad((ReadoutTail.apply(y4_cl, *params) * g).sum(), [y4_cl] + params)

    def hip_params_only():
        torch.autograd.grad((ReadoutTail.apply(y4_cl.detach(), *params) * g).sum(), params)

    def ref():
        torch.autograd.grad((torch_tail(y4_nc, *params) * g).sum(), [y4_nc] + params)

    got = torch.autograd.grad((ReadoutTail.apply(y4_cl, *params) * g).sum(), [y4_cl] + params)      # warm-up, and a check
    want = torch.autograd.grad((torch_tail(y4_nc, *params) * g).sum(), [y4_nc] + params)
    worst = 0.0
    for name, a, b in zip(("y4",) + RT.PARAMS, got, want):
        if name == "b12":
            continue
        a = a.permute(0, 4, 1, 2, 3) if name == "y4" else a
        worst = max(worst, ((a - b).abs().max() / b.abs().max()).item())
    hip_params_only()
    torch.cuda.synchronize()
    t_hip, t_ref, t_par = [], [], []
    for _ in range(args.rounds):
        t_hip.append(timed(hip, args.reps))
        t_ref.append(timed(ref, args.reps))
        t_par.append(timed(hip_params_only, args.reps))
    with E.Profiler() as prof:
        hip()
        torch.cuda.synchronize()
    launches = {k: round(v["ms"], 4) for k, v in sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])}
    out = {"shape": [B, args.height, args.width], "reps": args.reps, "hip_ms": min(t_hip), "hip_ms_rounds": t_hip,
           "hip_params_only_ms": min(t_par), "torch_ms": min(t_ref), "torch_ms_rounds": t_ref,
           "grad_rel_diff_vs_torch_fp32": worst, "hip_launch_ms": launches, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
