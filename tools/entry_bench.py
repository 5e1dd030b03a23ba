"""The laterals' entry convs in training, on one GPU: (a) the weight-gradient kernel alone, (b) the training step with and
without the entry stage, (c) what rebuilding the model's root plan costs after a step.

    python tools/entry_bench.py [--batch 8] [--height 224] [--width 384] [--reps 10] [--rounds 3] [--json OUT]

(a) mspi_conv_wgrad_entry on the entry shapes of x3dl (C = 24, 48, 96, 192 | 512, s = 4, 16 frames) and videoswins (96, 192, 384,
768 | 512, s = 2, 8 frames), bytes from shapes (x once + dy once) over time, next to a device-to-device copy of the same
bytes and to two alternatives timed in the same rounds, alternating: torch's convolution_backward of the composed conv
(weight and bias gradient only), and what the older kernels can do where they can do it at all (C % 32 == 0): a dense copy
of each tap's frames, then mspi_conv_wgrad_wide_fwd on slices of at most 192 channels.  (b) LateralEntry (four) + LateralBlock
(four) + Fusion + ReadoutHead + ReadoutTail at x3dl's shapes with gradients for all 83 tensors, against the same without the
entry stage (the 71 tensors of trainable("lateral_blocks"), entry outputs given) and against the same layers in torch ops with
torch autograd; the per-launch split of both hand-written paths comes from engine.Profiler in a separate pass.  (c) the
audio-visual x3dl model: `model.pk` after an in-place change of one entry conv, a synchronise on either side.  One warm-up
call each, then `reps` calls inside one pair of device events, in rounds.  Prints one JSON line.  Needs the GPU."""
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
from lateral_bench import torch_block  # noqa: E402
from readout_bench import torch_head  # noqa: E402
from readout_tail_bench import timed, torch_tail  # noqa: E402

ENCODERS = {"x3dl": ((24, 48, 96, 192), 4, 16), "videoswins": ((96, 192, 384, 768), 2, 8)}      # widths, s, frames
SYNC_WIDTH = 512                                                                                # the SyncBlock's tokens, second input of k = 3
PEAK_TB_S = 8.0                                                                                 # HBM3E, the chip's peak


def entry_shapes(name, B, H, W):
    """[(label, (B, T, h, w), C)] of the tensors the four entry convs read."""
    widths, s, T = ENCODERS[name]
    out = []
    for k, c in enumerate(widths):
        shape = (B, T, H >> (2 + k), W >> (2 + k))
        out.append(("%s k=%d" % (name, k), shape, c))
        if k == 3:
            out.append(("%s k=3 sync" % name, shape, SYNC_WIDTH))
    return out, s


def spread(ts):
    return round(max(ts) - min(ts), 4)


def kernel_alone(E, A, dev, B, H, W, reps, rounds):
    rows = []
    for name in ENCODERS:
        shapes, s = entry_shapes(name, B, H, W)
        for label, (b, T, h, w), c in shapes:
            gen = torch.Generator().manual_seed(7)
            x = torch.randn(b, T, h, w, c, generator=gen).to(dev)
            G = torch.randn(b, T // s, h, w, 192, generator=gen).to(dev)
            xc, Gc = A._cl5(x), A._cl5(G)
            geo = A._geometry((s, 1, 1), (0, 0, 0), c, 192, (s, 1, 1))
            x_nc, G_nc = x.permute(0, 4, 1, 2, 3), G.permute(0, 4, 1, 2, 3)       # channels-last memory, NCDHW view: no copy
            wc = torch.zeros(192, c, s, 1, 1, device=dev)

            def new():
                return E.conv_wgrad_entry(xc, Gc, geo)

            def torch_bwd():
                return torch.ops.aten.convolution_backward(G_nc, x_nc, wc, [192], [s, 1, 1], [0, 0, 0], [1, 1, 1], False, [0, 0, 0], 1,
                                                           [False, True, True])

            def older():      # a dense copy of each tap's frames, then the wide kernel on <= 192-channel slices
                return [A.wgrad_wide_sliced(A._cl5(x[:, t::s].contiguous()), Gc, (1, 1, 1), (0, 0, 0)) for t in range(s)]
            paths = {"entry": new, "torch": torch_bwd}
            if c % 32 == 0:
                paths["copy_wide"] = older
            got, failed = {}, {}
            for k, fn in list(paths.items()):                                      # warm-up, and a check
                try:
                    got[k] = fn()
                except RuntimeError as e:                                          # a baseline torch cannot run at this shape is reported, not timed
                    if k == "entry":
                        raise
                    failed[k] = str(e)[:200]
                    del paths[k]
            dW = got["entry"][0]
            check = {}
            if "torch" in got:
                check["torch"] = ((dW - got["torch"][1]).abs().max() / dW.abs().max()).item()
            if "copy_wide" in got:
                old = torch.stack([p[0][:, :, 0, 0, 0] for p in got["copy_wide"]], 2)
                check["copy_wide"] = ((dW[:, :, :, 0, 0] - old).abs().max() / dW.abs().max()).item()
            del got
            times = {k: [] for k in paths}
            for _ in range(rounds):
                for k, fn in paths.items():
                    times[k].append(timed(fn, reps))
            nbytes = 4.0 * Gc.M * (s * c + 192)
            src = torch.empty(int(nbytes // 8), device=dev)
            dst = torch.empty_like(src)
            copy_ms = min(timed(lambda: dst.copy_(src), reps) for _ in range(rounds))
            ms = min(times["entry"])
            rows.append({"shape": label, "x": [b, T, h, w, c], "s": s, "rows": Gc.M, "variant": E.conv_wgrad_entry_variant(xc, Gc, geo),
                         "MB": round(nbytes / 1e6, 1), "ms": {k: round(min(v), 4) for k, v in times.items()},
                         "ms_spread": {k: spread(v) for k, v in times.items()}, "TB_per_s": round(nbytes / (1e9 * ms), 3),
                         "share_of_peak": round(nbytes / (1e9 * ms) / PEAK_TB_S, 3), "copy_same_bytes_ms": round(copy_ms, 4),
                         "share_of_copy_rate": round(copy_ms / ms, 3), "rel_diff": check, "not_run": failed})
            del x, G, src, dst
    return rows


def step(E, A, dev, B, H, W, reps, rounds):
    import fusion_restate as FR
    import lateral_entry_restate as ER
    import lateral_restate as LR
    import readout_restate as R
    import readout_tail_restate as RT
    a, b = H // 32, W // 32
    shapes, s = entry_shapes("x3dl", B, H, W)
    fcase = FR.make_case(B, 4, a, b, 1, D=192, Cm=512, mid=32)
    rcase = R.make_case(1, 1, 1, 1, D=192)
    sa = [torch.from_numpy(fcase[k]).to(dev).requires_grad_(True) for k in FR.SA_PARAMS]
    head = [torch.from_numpy(rcase[k]).to(dev).requires_grad_(True) for k in R.HEAD]
    tail = [torch.from_numpy(rcase[k]).to(dev).requires_grad_(True) for k in RT.PARAMS]
    m_nc = torch.from_numpy(fcase["masks"]).to(dev)
    m_cl = m_nc.permute(0, 2, 3, 4, 1).contiguous()
    del fcase
    blocks, entries, xs_cl = [], [], []
    gen = torch.Generator().manual_seed(5)
    for k in range(4):
        bcase = LR.make_case(1, 1, 1, 1, 10 + k, D=192)
        blocks.append([(torch.from_numpy(bcase[n]) * (0.1 if n.startswith("w") else 1.0)).to(dev).requires_grad_(True) for n in LR.PARAMS])
        ins = [sh for sh in shapes if sh[0].startswith("x3dl k=%d" % k)]
        cin = sum(c for _, _, c in ins)
        ecase = ER.make_case(1, s, 1, 1, cin, s, 20 + k)
        entries.append([torch.from_numpy(ecase[n]).to(dev).requires_grad_(True) for n in ER.NAMES])
        xs_cl.append([torch.randn(*shape, c, generator=gen).to(dev) for _, shape, c in ins])
    xs_nc = [torch.cat([t.permute(0, 4, 1, 2, 3) for t in ts], 1).contiguous() for ts in xs_cl]
    g = torch.randn(B, H, W, generator=torch.Generator().manual_seed(2)).to(dev)
    bn_sa = [(torch.zeros(32, device=dev), torch.ones(32, device=dev), torch.zeros((), dtype=torch.long, device=dev)) for _ in range(3)]
    bn = [(torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.long, device=dev)) for c in (192, 64)]
    wrt_blocks = [p for blk in blocks for p in blk] + sa + head + tail
    wrt = [p for e in entries for p in e] + wrt_blocks
    assert len(wrt_blocks) == 71 and len(wrt) == 83
    with torch.no_grad():
        e_cl = [A.LateralEntry.apply(ts[0], ts[1] if len(ts) == 2 else None, *e).clone() for ts, e in zip(xs_cl, entries)]

    def rest(lats_in, wrt_):
        lats = [A.LateralBlock.apply(x, *blk) for x, blk in zip(lats_in, blocks)]
        maps = A.Fusion.apply(*lats, m_cl, *sa, *bn_sa)
        out = A.ReadoutTail.apply(A.ReadoutHead.apply(*maps, *head, bn[0], bn[1]), *tail)
        return torch.autograd.grad((out * g).sum(), wrt_)

    def hip_entries():
        return rest([A.LateralEntry.apply(ts[0], ts[1] if len(ts) == 2 else None, *e) for ts, e in zip(xs_cl, entries)], wrt)

    def hip_blocks():
        return rest(e_cl, wrt_blocks)

    def ref():
        lats = [torch_block(F.conv3d(F.conv3d(x, e[0], e[1]), e[2], stride=(s, 1, 1)), *blk) for x, e, blk in zip(xs_nc, entries, blocks)]
        out = torch_tail(torch_head(torch_fusion(lats, m_nc, sa), *head), *tail)
        return torch.autograd.grad((out * g).sum(), wrt)

    got, want = hip_entries(), ref()                                                          # warm-up, and a check
    diffs = {"lat%d_%s" % (k, n): ((got[3 * k + i] - want[3 * k + i]).abs().max() / want[3 * k + i].abs().max()).item()
             for k in range(4) for i, n in enumerate(ER.NAMES)}
    del got, want
    hip_blocks()
    torch.cuda.synchronize()
    times = {"hip_entries": [], "hip_blocks": [], "torch": []}
    for _ in range(rounds):
        times["hip_entries"].append(timed(hip_entries, reps))
        times["hip_blocks"].append(timed(hip_blocks, reps))
        times["torch"].append(timed(ref, reps))
    launches = {}
    for name, fn in (("hip_entries", hip_entries), ("hip_blocks", hip_blocks)):
        with E.Profiler() as prof:
            fn()
            torch.cuda.synchronize()
        launches[name] = {k: round(v["ms"], 4) for k, v in sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])}
    added = {k: round(v - launches["hip_blocks"].get(k, 0.0), 4) for k, v in launches["hip_entries"].items()
             if abs(v - launches["hip_blocks"].get(k, 0.0)) >= 0.005}
    packs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for e in entries:
                A.pack_lateral_entry(e[0], e[1], e[2], (s, 1, 1))
        torch.cuda.synchronize()
        packs.append(round(1e3 * (time.perf_counter() - t0), 3))
    return {"ms": {k: round(min(v), 3) for k, v in times.items()}, "ms_rounds": {k: [round(t, 3) for t in v] for k, v in times.items()},
            "added_ms": round(min(times["hip_entries"]) - min(times["hip_blocks"]), 3), "added_by_launch_ms": added,
            "launch_ms": launches, "entry_grad_rel_diff_vs_torch_fp32": diffs, "host_pack_four_entries_ms": packs}


def plan_rebuild(dev, H, W):
    """model.pk of the audio-visual x3dl model after an in-place change of one entry conv (what an optimiser step leaves
    behind): the root plan's key covers the entry convs, so every pack of the root is built again."""
    from mspi_amd import testing as T
    from mspi_amd.model.model_utils import AudioVisualSaliencyModel
    cfg = T.make_cfg("x3dl", num_vis_tokens=16 * (H // 32) * (W // 32))
    m = T.seeded(lambda: AudioVisualSaliencyModel(cfg), 0).to(dev)
    m.pk
    out = {"moved_entry_conv_ms": [], "nothing_moved_ms": []}
    for _ in range(3):
        for key, move in (("moved_entry_conv_ms", True), ("nothing_moved_ms", False)):
            if move:
                with torch.no_grad():
                    m.latlayer_0[0].weight.mul_(1.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.pk
            torch.cuda.synchronize()
            out[key].append(round(1e3 * (time.perf_counter() - t0), 3))
    return out


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
        raise SystemExit("entry_bench needs an MI355X (no CPU fallback)")
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    E.autotune(False)
    dev = torch.device("cuda", 0)
    out = {"shape": [args.batch, args.height, args.width], "reps": args.reps, "rounds": args.rounds,
           "kernel": kernel_alone(E, A, dev, args.batch, args.height, args.width, args.reps, args.rounds),
           "step": step(E, A, dev, args.batch, args.height, args.width, args.reps, args.rounds),
           "root_plan": plan_rebuild(dev, args.height, args.width), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
