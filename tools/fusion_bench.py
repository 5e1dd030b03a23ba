"""Forward + backward of the SA gating, the top-down fusion and the whole readout at the training shape, hand-written path
against torch ops on the same GPU.

    python tools/fusion_bench.py [--batch 8] [--height 224] [--width 384] [--reps 20] [--rounds 3] [--json OUT]

Code under test: mspi_amd.autograd.Fusion + ReadoutHead + ReadoutTail over the four lateral outputs and the adapter's masks at
the product's channel counts (D = 192, Cm = 512, mid = 32), gradients for the 15 SA tensors, the 16 readout tensors and the four
laterals.  Baseline, never the code under test: the same layers in torch ops (one F.conv3d for the three first convs,
F.batch_norm(training=True, eps 1e-3), F.interpolate, F.conv3d, sigmoid, this project's order of readout[0]) with torch
autograd.  One warm-up call each, then `reps` calls inside one pair of device events, the two paths alternating in rounds; the
per-launch split of the hand-written path comes from engine.Profiler in a separate pass, and for the launches of
csrc/fusion_bwd.hip also bytes moved / time.  Prints one JSON line.  Needs the GPU."""
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

from readout_bench import torch_head  # noqa: E402
from readout_tail_bench import timed, torch_tail  # noqa: E402


def torch_fusion(lat, masks, sa):
    """lat: the four laterals NCDHW, sa: the 15 tensors -> the four maps ReadoutHead takes; BatchNorm on batch statistics."""
    import fusion_restate as FR
    mid = sa[0].shape[0]
    pre = F.conv3d(masks, torch.cat(sa[0::5], 0), None, padding=1)
    pm = F.relu(F.batch_norm(pre, None, None, torch.cat(sa[1::5]), torch.cat(sa[2::5]), True, FR.MOMENTUM, FR.EPS))
    gated = []
    for k in range(3):
        m = pm[:, k * mid:(k + 1) * mid]
        if FR.FACTORS[k] != 1:
            m = F.interpolate(m, scale_factor=(1, FR.FACTORS[k], FR.FACTORS[k]), mode="trilinear", align_corners=False)
        gate = torch.sigmoid(F.conv3d(m, sa[5 * k + 3], sa[5 * k + 4], padding=(0, 1, 1)))
        gated.append(lat[k] * gate + lat[k])

    def up(x, k):
        return F.interpolate(x, scale_factor=(1, k, k), mode="trilinear", align_corners=False)
    s2 = gated[2] + up(lat[3], 2)
    s1 = gated[1] + up(s2, 2) + up(lat[3], 4)
    return [gated[0], s1, s2, lat[3]]


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
        raise SystemExit("fusion_bench needs an MI355X (no CPU fallback)")
    import fusion_restate as FR
    import readout_restate as R
    import readout_tail_restate as RT
    from mspi_amd import engine as E
    from mspi_amd.autograd import Fusion, ReadoutHead, ReadoutTail
    dev = torch.device("cuda", 0)
    B, a, b = args.batch, args.height // 32, args.width // 32
    fcase = FR.make_case(B, 4, a, b, 1, D=192, Cm=512, mid=32)
    rcase = R.make_case(1, 1, 1, 1, D=192)                                                    # the readout's parameters
    sa = [torch.from_numpy(fcase[k]).to(dev).requires_grad_(True) for k in FR.SA_PARAMS]
    head = [torch.from_numpy(rcase[k]).to(dev).requires_grad_(True) for k in R.HEAD]
    tail = [torch.from_numpy(rcase[k]).to(dev).requires_grad_(True) for k in RT.PARAMS]
    l_nc = [torch.from_numpy(fcase[k]).to(dev).requires_grad_(True) for k in FR.LATERALS]
    l_cl = [t.detach().permute(0, 2, 3, 4, 1).contiguous().requires_grad_(True) for t in l_nc]
    m_nc = torch.from_numpy(fcase["masks"]).to(dev)
    m_cl = m_nc.permute(0, 2, 3, 4, 1).contiguous()
    g = torch.randn(B, 32 * a, 32 * b, generator=torch.Generator().manual_seed(2)).to(dev)
    del fcase
    bn_sa = [(torch.zeros(32, device=dev), torch.ones(32, device=dev), torch.zeros((), dtype=torch.long, device=dev)) for _ in range(3)]
    bn = [(torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.long, device=dev)) for c in (192, 64)]

    def hip():
        maps = Fusion.apply(*l_cl, m_cl, *sa, *bn_sa)
        out = ReadoutTail.apply(ReadoutHead.apply(*maps, *head, bn[0], bn[1]), *tail)
        return torch.autograd.grad((out * g).sum(), sa + head + tail + l_cl)

    def ref():
        out = torch_tail(torch_head(torch_fusion(l_nc, m_nc, sa), *head), *tail)
        return torch.autograd.grad((out * g).sum(), sa + head + tail + l_nc)

    got, want = hip(), ref()                                                                  # warm-up, and a check
    names = FR.SA_PARAMS + R.PARAMS + FR.LATERALS
    diffs = {}
    for name, x, y in zip(names, got, want):
        if name not in ("b1", "b4", "b12"):
            x = x.permute(0, 4, 1, 2, 3) if name in FR.LATERALS else x
            diffs[name] = ((x - y).abs().max() / y.abs().max()).item()
    del got, want
    torch.cuda.synchronize()
    t_hip, t_ref = [], []
    for _ in range(args.rounds):
        t_hip.append(timed(hip, args.reps))
        t_ref.append(timed(ref, args.reps))
    with E.Profiler() as prof:
        hip()
        torch.cuda.synchronize()
    launches = {k: round(v["ms"], 4) for k, v in sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])}
    new = [{"launch": r[0], "detail": r[5], "us": round(1e3 * r[3].elapsed_time(r[4]), 1), "MB": round(r[2] / 1e6, 1),
            "TB_per_s": round(r[2] / (1e9 * r[3].elapsed_time(r[4])), 3)} for r in prof.records if r[0] in ("rowgate_bwd", "upsample_sum_bwd")]
    out = {"shape": [B, args.height, args.width], "reps": args.reps, "hip_ms": min(t_hip), "hip_ms_rounds": t_hip,
           "torch_ms": min(t_ref), "torch_ms_rounds": t_ref, "grad_rel_diff_vs_torch_fp32": diffs, "hip_launch_ms": launches,
           "fusion_bwd_launches": new, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
