"""Forward + backward of the whole readout at the training shape, hand-written path against torch ops on the same GPU.

    python tools/readout_bench.py [--batch 8] [--height 224] [--width 384] [--reps 20] [--rounds 3] [--json OUT]

Code under test: mspi_amd.autograd.ReadoutHead + ReadoutTail over the four fused pyramid maps at decoder width 192, gradients
for the 16 parameters.  Baseline, never the code under test: the same layers in torch ops (this project's order of readout[0],
F.conv3d, F.batch_norm(training=True), F.interpolate, logsumexp) with torch autograd.  One warm-up call each, then `reps` calls
inside one pair of device events, the two paths alternating in rounds; the per-launch split of the hand-written path comes
from engine.Profiler in a separate pass.  Prints one JSON line.  Needs the GPU."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from readout_tail_bench import timed, torch_tail  # noqa: E402


def torch_head(s, w0, b0, w1, b1, g2, be2, w4, b4, g5, be5):
    """s: the four maps NCDHW -> y4 [B,64,4,h,w]; BatchNorm on batch statistics (running statistics left alone)."""
    D = w0.shape[0]
    W = w0.flatten(1)
    y0 = F.conv3d(s[0], W[:, :D, None, None, None], b0)
    for j in (1, 2, 3):
        part = F.conv3d(s[j], (W[:, :D] + W[:, j * D:(j + 1) * D])[:, :, None, None, None])
        y0 = y0 + F.interpolate(part, scale_factor=(1, 1 << j, 1 << j), mode="trilinear", align_corners=False)
    a1 = F.relu(F.batch_norm(F.conv3d(y0, w1, b1, padding=1), None, None, g2, be2, True, 0.1, 1e-5))
    return F.relu(F.batch_norm(F.conv3d(a1, w4, b4, padding=(0, 1, 1)), None, None, g5, be5, True, 0.1, 1e-5))


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
        raise SystemExit("readout_bench needs an MI355X (no CPU fallback)")
    import readout_restate as R
    import readout_tail_restate as RT
    from mspi_amd import engine as E
    from mspi_amd.autograd import ReadoutHead, ReadoutTail
    dev = torch.device("cuda", 0)
    B, a, b = args.batch, args.height // 32, args.width // 32
    case = R.make_case(B, a, b, 1, D=192)
    head = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in R.HEAD]
    tail = [torch.from_numpy(case[k]).to(dev).requires_grad_(True) for k in RT.PARAMS]
    s_nc = [torch.from_numpy(case[k]).to(dev) for k in R.MAPS]
    s_cl = [t.permute(0, 2, 3, 4, 1).contiguous() for t in s_nc]
    g = torch.from_numpy(case["g"]).to(dev)
    bn = [(torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.long, device=dev)) for c in (192, 64)]

    def hip():
        return torch.autograd.grad((ReadoutTail.apply(ReadoutHead.apply(*s_cl, *head, bn[0], bn[1]), *tail) * g).sum(), head + tail)

    def ref():
        return torch.autograd.grad((torch_tail(torch_head(s_nc, *head), *tail) * g).sum(), head + tail)

    got, want = hip(), ref()                                                                  # warm-up, and a check
    diffs = {}
    for name, x, y in zip(R.PARAMS, got, want):
        if name not in ("b1", "b4", "b12"):
            diffs[name] = ((x - y).abs().max() / y.abs().max()).item()
    torch.cuda.synchronize()
    t_hip, t_ref = [], []
    for _ in range(args.rounds):
        t_hip.append(timed(hip, args.reps))
        t_ref.append(timed(ref, args.reps))
    with E.Profiler() as prof:
        hip()
        torch.cuda.synchronize()
    launches = {k: round(v["ms"], 4) for k, v in sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])}
    details = [(r[5], round(r[3].elapsed_time(r[4]), 4)) for r in prof.records if r[0] == "conv_wgrad_wide"]
    out = {"shape": [B, args.height, args.width], "reps": args.reps, "hip_ms": min(t_hip), "hip_ms_rounds": t_hip,
           "torch_ms": min(t_ref), "torch_ms_rounds": t_ref, "grad_rel_diff_vs_torch_fp32": diffs, "hip_launch_ms": launches,
           "wide_wgrad_calls": details, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
