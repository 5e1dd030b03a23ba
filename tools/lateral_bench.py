"""Forward + backward of the laterals' four ConvNextBlocks, the SA gating, the top-down fusion and the whole readout at the
training shape, hand-written path against torch ops on the same GPU.

    python tools/lateral_bench.py [--batch 8] [--height 224] [--width 384] [--reps 10] [--rounds 3] [--json OUT]

Code under test: mspi_amd.autograd.LateralBlock (four times) + Fusion + ReadoutHead + ReadoutTail over the four entry-conv
outputs and the adapter's masks at the product's channel counts (D = 192, Cm = 512, mid = 32), gradients for all 71 tensors
that trainable("lateral_blocks") trains.  Baseline, never the code under test: the same layers in torch ops (F.conv3d with
groups, F.layer_norm, exact F.gelu, and tools/fusion_bench.py's torch path behind them) with torch autograd.  One warm-up call
each, then `reps` calls inside one pair of device events, the two paths alternating in rounds; the per-launch split of the
hand-written path comes from engine.Profiler in a separate pass, and for the launches of csrc/block_bwd.hip also bytes moved /
time, next to the rate of a device-to-device copy of level 0's activation.  Also timed, on the host with a synchronise on
either side: building the four blocks' packs from the live tensors, which LateralBlock.forward does at every step.  Prints one
JSON line.  Needs the GPU."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fusion_bench import torch_fusion  # noqa: E402
from readout_bench import torch_head  # noqa: E402
from readout_tail_bench import timed, torch_tail  # noqa: E402

NEW = ("gelu_bwd", "layernorm_bwd", "dwconv_wgrad")


def torch_block(x, wt, bt, ws, bs, gam, bet, w1, b1, w2, b2):
    """x NCDHW -> the ConvNextBlock in torch ops, upstream's order (model/model_utils.py:339-354)."""
    D = x.shape[1]
    t = F.conv3d(F.conv3d(x, wt, bt, padding=(3, 0, 0), groups=D), ws, bs, padding=(0, 3, 3), groups=D)
    t = F.layer_norm(t.permute(0, 2, 3, 4, 1), (D,), gam, bet, 1e-5).permute(0, 4, 1, 2, 3)
    return x + F.conv3d(F.gelu(F.conv3d(t, w1, b1)), w2, b2)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=224)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lateral_bench needs an MI355X (no CPU fallback)")
    import fusion_restate as FR
    import lateral_restate as LR
    import readout_restate as R
    import readout_tail_restate as RT
    from mspi_amd import engine as E
    from mspi_amd.autograd import Fusion, LateralBlock, ReadoutHead, ReadoutTail, pack_convnext_block
    dev = torch.device("cuda", 0)
    B, a, b = args.batch, args.height // 32, args.width // 32
    fcase = FR.make_case(B, 4, a, b, 1, D=192, Cm=512, mid=32)
    rcase = R.make_case(1, 1, 1, 1, D=192)                                                    # the readout's parameters
    sa = [torch.from_numpy(fcase[k]).to(dev).requires_grad_(True) for k in FR.SA_PARAMS]
    head = [torch.from_numpy(rcase[k]).to(dev).requires_grad_(True) for k in R.HEAD]
    tail = [torch.from_numpy(rcase[k]).to(dev).requires_grad_(True) for k in RT.PARAMS]
    blocks = []
    for k in range(4):                                                                        # upstream's init is N(0, 0.02^2): a tenth of the tests' scale
        bcase = LR.make_case(1, 1, 1, 1, 10 + k, D=192)
        blocks.append([(torch.from_numpy(bcase[n]) * (0.1 if n.startswith("w") else 1.0)).to(dev).requires_grad_(True) for n in LR.PARAMS])
    e_nc = [torch.from_numpy(fcase[k]).to(dev) for k in FR.LATERALS]                          # the entry convs' outputs: no grad
    e_cl = [t.permute(0, 2, 3, 4, 1).contiguous() for t in e_nc]
    m_nc = torch.from_numpy(fcase["masks"]).to(dev)
    m_cl = m_nc.permute(0, 2, 3, 4, 1).contiguous()
    g = torch.randn(B, 32 * a, 32 * b, generator=torch.Generator().manual_seed(2)).to(dev)
    del fcase
    bn_sa = [(torch.zeros(32, device=dev), torch.ones(32, device=dev), torch.zeros((), dtype=torch.long, device=dev)) for _ in range(3)]
    bn = [(torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.long, device=dev)) for c in (192, 64)]
    wrt = [p for blk in blocks for p in blk] + sa + head + tail
    assert len(wrt) == 71

    def hip():
        lats = [LateralBlock.apply(x, *blk) for x, blk in zip(e_cl, blocks)]
        maps = Fusion.apply(*lats, m_cl, *sa, *bn_sa)
        out = ReadoutTail.apply(ReadoutHead.apply(*maps, *head, bn[0], bn[1]), *tail)
        return torch.autograd.grad((out * g).sum(), wrt)

    def ref():
        lats = [torch_block(x, *blk) for x, blk in zip(e_nc, blocks)]
        out = torch_tail(torch_head(torch_fusion(lats, m_nc, sa), *head), *tail)
        return torch.autograd.grad((out * g).sum(), wrt)

    got, want = hip(), ref()                                                                  # warm-up, and a check
    names = ["lat%d_%s" % (k, n) for k in range(4) for n in LR.PARAMS] + list(FR.SA_PARAMS + R.PARAMS)
    diffs = {}
    for name, x, y in zip(names, got, want):
        if name not in ("b1", "b4", "b12"):
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
            "TB_per_s": round(r[2] / (1e9 * r[3].elapsed_time(r[4])), 3)} for r in prof.records if r[0] in NEW]
    src = e_cl[0]
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), 20)
    copy = {"MB": round(8.0 * src.numel() / 1e6, 1), "us": round(1e3 * copy_ms, 1), "TB_per_s": round(8.0 * src.numel() / (1e9 * copy_ms), 3)}
    packs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for blk in blocks:
                pack_convnext_block(*blk)
        torch.cuda.synchronize()
        packs.append(1e3 * (time.perf_counter() - t0))
    out = {"shape": [B, args.height, args.width], "reps": args.reps, "hip_ms": min(t_hip), "hip_ms_rounds": t_hip,
           "torch_ms": min(t_ref), "torch_ms_rounds": t_ref, "grad_rel_diff_vs_torch_fp32": diffs, "hip_launch_ms": launches,
           "block_bwd_launches": new, "device_copy": copy, "host_pack_four_blocks_ms": packs,
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
