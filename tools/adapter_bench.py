"""The adapter's Inception in training, on one GPU: (a) the 16-tile weight-gradient kernel alone on the eight layer shapes,
(b) the training step with and without the adapter stage.

    python tools/adapter_bench.py [--batch 8] [--height 224] [--width 384] [--reps 10] [--rounds 3] [--json OUT]

(a) mspi_conv_wgrad_t16 on each of the eight layers (rows = batch x 4 x H/16 x W/16), bytes from shapes (x once + dy once) over
time, next to a device-to-device copy of the same bytes and to what the older kernels can do, timed in the same rounds,
alternating: on the three layers mspi_conv_wgrad_wide_fwd takes (416 -> 192, 416 -> 96, 416 -> 64) that kernel on input slices
of at most 192 channels; on the other five zero-padded dense copies of x and dy to multiples of 32 (the copies are timed with
it) and the wide kernel on slices of at most 192 channels of either.  (b) Adapter + LateralEntry (four) + LateralBlock (four)
+ Fusion + ReadoutHead + ReadoutTail at x3dl's shapes with gradients for all 107 tensors, against the same without the adapter
stage (the 83 tensors of trainable("lateral_entries"), masks given) and against the same layers in torch ops with torch
autograd; the per-launch split of both hand-written paths comes from engine.Profiler in a separate pass.  One warm-up call
each, then `reps` calls inside one pair of device events, in rounds.  Prints one JSON line.  Needs the GPU."""
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

from entry_bench import entry_shapes, spread  # noqa: E402
from fusion_bench import torch_fusion  # noqa: E402
from lateral_bench import torch_block  # noqa: E402
from readout_bench import torch_head  # noqa: E402
from readout_tail_bench import timed, torch_tail  # noqa: E402

PEAK_TB_S = 8.0
WIDE_MAX = 192


def older_route(E, A, x, dy, k, pad):
    """The weight gradient from mspi_conv_wgrad_wide_fwd: x [B,T,h,w,C] and dy [B,T,h,w,Co] zero-padded to multiples of 32 in
    dense copies where they are not, then slices of at most 192 channels of either.  Returns dW [Co,C,kt,kh,kw]."""
    C, Co = x.shape[4], dy.shape[4]
    if C % 32:
        x = F.pad(x, (0, 32 - C % 32))
    if Co % 32:
        dy = F.pad(dy, (0, 32 - Co % 32))
    return A.wgrad_wide_sliced(A._cl5(x), A._cl5(dy), k, pad)[0][:Co, :C]


def kernel_alone(E, A, AR, dev, B, H, W, reps, rounds):
    out = []
    h, w = H // 16, W // 16
    for l, (c, co, k, pad) in AR.geometry().items():
        gen = torch.Generator().manual_seed(7)
        x = torch.randn(B, 4, h, w, c, generator=gen).to(dev)
        G = torch.randn(B, 4, h, w, co, generator=gen).to(dev)
        xc, Gc, geo = A._cl5(x), A._cl5(G), A._geometry(k, pad, c, co)
        paths = {"t16": lambda: E.conv_wgrad_t16(xc, Gc, geo)[0], "older": lambda: older_route(E, A, x, G, k, pad)}
        got = {n: fn() for n, fn in paths.items()}                                  # warm-up, and a check
        diff = ((got["t16"] - got["older"]).abs().max() / got["t16"].abs().max()).item()
        del got
        times = {n: [] for n in paths}
        for _ in range(rounds):
            for n, fn in paths.items():
                times[n].append(timed(fn, reps))
        nbytes = 4.0 * Gc.M * (c + co)
        src = torch.empty(int(nbytes // 8), device=dev)
        dst = torch.empty_like(src)
        copy_ms = min(timed(lambda: dst.copy_(src), reps) for _ in range(rounds))
        ms = min(times["t16"])
        taps = k[0] * k[1] * k[2]
        out.append({"layer": l, "C": c, "Cout": co, "kernel": list(k), "rows": Gc.M, "variant": E.conv_wgrad_t16_variant(xc, Gc, geo),
                    "route": A.adapter_wgrad_route(Gc.M, c, co),
                    "older_is": "wide" if not (c % 32 or co % 32 or co > WIDE_MAX) else "pad + wide", "MB": round(nbytes / 1e6, 2),
                    "ms": {n: round(min(v), 4) for n, v in times.items()}, "ms_spread": {n: spread(v) for n, v in times.items()},
                    "TB_per_s": round(nbytes / (1e9 * ms), 3), "TFLOP_per_s": round(2.0 * Gc.M * taps * c * co / (1e9 * ms), 2),
                    "copy_same_bytes_ms": round(copy_ms, 4), "rel_diff_older": diff})
        del x, G, src, dst
    return out


def step(E, A, AR, dev, B, H, W, reps, rounds):
    import fusion_restate as FR
    import lateral_entry_restate as ER
    import lateral_restate as LR
    import readout_restate as R
    import readout_tail_restate as RT
    a, b = H // 32, W // 32
    shapes, s = entry_shapes("x3dl", B, H, W)
    fcase = FR.make_case(1, 1, 1, 1, 1, D=192, Cm=512, mid=32)
    rcase = R.make_case(1, 1, 1, 1, D=192)
    acase = AR.make_case(B, 4, 2 * a, 2 * b, 3)
    sa = [torch.from_numpy(fcase[k]).to(dev).requires_grad_(True) for k in FR.SA_PARAMS]
    head = [torch.from_numpy(rcase[k]).to(dev).requires_grad_(True) for k in R.HEAD]
    tail = [torch.from_numpy(rcase[k]).to(dev).requires_grad_(True) for k in RT.PARAMS]
    ad = [torch.from_numpy(acase[k]).to(dev).requires_grad_(True) for k in AR.PARAMS]
    cat_nc = torch.from_numpy(acase["cat"]).to(dev)
    cat_cl = cat_nc.permute(0, 2, 3, 4, 1).contiguous()
    inception, layers = AR.upstream_inception(acase, torch.float32)
    inception = inception.to(dev)
    ad_torch = [t for l in AR.LAYERS for t in (layers[l][0].weight, layers[l][1].weight, layers[l][1].bias)]
    blocks, entries, xs_cl = [], [], []
    gen = torch.Generator().manual_seed(5)
    for k in range(4):
        bcase = LR.make_case(1, 1, 1, 1, 10 + k, D=192)
        blocks.append([(torch.from_numpy(bcase[n]) * (0.1 if n.startswith("w") else 1.0)).to(dev).requires_grad_(True) for n in LR.PARAMS])
        ins = [sh for sh in shapes if sh[0].startswith("x3dl k=%d" % k)]
        ecase = ER.make_case(1, s, 1, 1, sum(c for _, _, c in ins), s, 20 + k)
        entries.append([torch.from_numpy(ecase[n]).to(dev).requires_grad_(True) for n in ER.NAMES])
        xs_cl.append([torch.randn(*shape, c, generator=gen).to(dev) for _, shape, c in ins])
    xs_nc = [torch.cat([t.permute(0, 4, 1, 2, 3) for t in ts], 1).contiguous() for ts in xs_cl]
    g = torch.randn(B, H, W, generator=torch.Generator().manual_seed(2)).to(dev)

    def buffers(widths):
        return [(torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.long, device=dev)) for c in widths]
    bn_sa, bn, bn_ad = buffers((32, 32, 32)), buffers((192, 64)), buffers([acase["gam_%s" % l].shape[0] for l in AR.LAYERS])
    wrt_entries = [p for e in entries for p in e] + [p for blk in blocks for p in blk] + sa + head + tail
    wrt = ad + wrt_entries
    assert len(wrt_entries) == 83 and len(wrt) == 107
    with torch.no_grad():
        m_cl = A.Adapter.apply(cat_cl, *ad, *bn_ad).clone()

    def rest(masks, wrt_):
        lats = [A.LateralBlock.apply(A.LateralEntry.apply(ts[0], ts[1] if len(ts) == 2 else None, *e), *blk)
                for ts, e, blk in zip(xs_cl, entries, blocks)]
        maps = A.Fusion.apply(*lats, masks, *sa, *bn_sa)
        out = A.ReadoutTail.apply(A.ReadoutHead.apply(*maps, *head, bn[0], bn[1]), *tail)
        return torch.autograd.grad((out * g).sum(), wrt_)

    def hip_adapter():
        return rest(A.Adapter.apply(cat_cl, *ad, *bn_ad), wrt)

    def hip_entries():
        return rest(m_cl, wrt_entries)

    def ref():
        masks = torch.cat([br(cat_nc) for br in inception], 1)
        lats = [torch_block(F.conv3d(F.conv3d(x, e[0], e[1]), e[2], stride=(s, 1, 1)), *blk) for x, e, blk in zip(xs_nc, entries, blocks)]
        out = torch_tail(torch_head(torch_fusion(lats, masks, sa), *head), *tail)
        return torch.autograd.grad((out * g).sum(), ad_torch + wrt_entries)

    got, want = hip_adapter(), ref()                                                          # warm-up, and a check
    diffs = {n: ((got[i] - want[i]).abs().max() / want[i].abs().max().clamp_min(1e-30)).item() for i, n in enumerate(AR.PARAMS)}
    del got, want
    hip_entries()
    torch.cuda.synchronize()
    times = {"hip_adapter": [], "hip_entries": [], "torch": []}
    for _ in range(rounds):
        times["hip_adapter"].append(timed(hip_adapter, reps))
        times["hip_entries"].append(timed(hip_entries, reps))
        times["torch"].append(timed(ref, reps))
    launches = {}
    for name, fn in (("hip_adapter", hip_adapter), ("hip_entries", hip_entries)):
        with E.Profiler() as prof:
            fn()
            torch.cuda.synchronize()
        launches[name] = {k: round(v["ms"], 4) for k, v in sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])}
    added = {k: round(v - launches["hip_entries"].get(k, 0.0), 4) for k, v in launches["hip_adapter"].items()
             if abs(v - launches["hip_entries"].get(k, 0.0)) >= 0.005}
    return {"ms": {k: round(min(v), 3) for k, v in times.items()}, "ms_rounds": {k: [round(t, 3) for t in v] for k, v in times.items()},
            "added_ms": round(min(times["hip_adapter"]) - min(times["hip_entries"]), 3), "added_by_launch_ms": added,
            "launch_ms": launches, "adapter_grad_rel_diff_vs_torch_fp32": diffs}


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
        raise SystemExit("adapter_bench needs an MI355X (no CPU fallback)")
    import adapter_restate as AR
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    E.autotune(False)
    dev = torch.device("cuda", 0)
    out = {"shape": [args.batch, args.height, args.width], "reps": args.reps, "rounds": args.rounds,
           "kernel": kernel_alone(E, A, AR, dev, args.batch, args.height, args.width, args.reps, args.rounds),
           "step": step(E, A, AR, dev, args.batch, args.height, args.width, args.reps, args.rounds),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
