"""trainable("adapter", sync=True) in training, on one GPU: (a) the whole training step of the audio-visual x3dl model with and
without sync=True, (b) the layers of the 75 added tensors alone against torch ops.

    python tools/sync_train_bench.py [--batches 8 2] [--height 224] [--width 384] [--wa 300] [--reps 5] [--rounds 3] [--json OUT]

(a) One step = forward with grad + criterion + backward with every gradient of the switch: model.trainable("adapter") -- 107
tensors, metrics.SalLoss -- and model.trainable("adapter", sync=True) -- 182 tensors, SalLoss + loss_av -- on ONE model in one
process, the two alternating inside every round (the switch only moves requires_grad flags; no optimiser step, so no plan is
rebuilt).  Clips of 16 x H x W, a 257 x wa spectrogram (wa = 300: 90 audio tokens, 1 434 tokens in all at 224 x 384, the shape
tools/sync_block_bench.py measures).  (b) autograd.sync_block + autograd.ContrastHead on random v4 / audio maps of the model's
shapes, with a fixed random gradient standing in for the one latlayer_3's entry conv returns to the visual tokens, gradients for
the 75 tensors; against the same layers in torch ops (explicit softmax attention, the model's own nn.Sequential projectors
called as torch modules, F.cosine_similarity) with torch autograd, alternating.  One warm-up call each, then `reps` calls inside
one pair of device events, in rounds; best and spread.  Prints one JSON line.  No speed bar is set.  Needs the GPU."""
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

from entry_bench import spread  # noqa: E402
from readout_tail_bench import timed  # noqa: E402
from train_step_digest import density  # noqa: E402

HEADS, HD, DIM = 4, 128, 512


def rounds_of(paths, reps, rounds):
    times = {n: [] for n in paths}
    for _ in range(rounds):
        for n, fn in paths.items():
            times[n].append(timed(fn, reps))
    return {"ms": {k: round(min(v), 3) for k, v in times.items()}, "spread_ms": {k: spread(v) for k, v in times.items()},
            "ms_rounds": {k: [round(t, 3) for t in v] for k, v in times.items()}}


def whole_step(m, M, clips, audio, label, reps, rounds):
    crit = M.SalLoss()

    def step(sync):
        m.trainable("adapter", sync=sync)
        for p in m.parameters():
            p.grad = None
        out, aux = m(clips, audio)
        (crit(out, label) + aux if sync else crit(out, label)).backward()
        return sum(p.grad is not None for p in m.parameters())
    paths = {"adapter": lambda: step(False), "adapter+sync": lambda: step(True)}
    counts = {n: fn() for n, fn in paths.items()}                 # warm-up, and the number of gradients
    torch.cuda.synchronize()
    return dict(rounds_of(paths, reps, rounds), gradients=counts)


def added_layers(m, A, dev, B, thw, ft, reps, rounds):
    sb = m.aud_vis_sync_block
    t, h, w = thw
    Rv, Ra, C4 = t * h * w, ft[0] * ft[1], sb.vis_proj.weight.shape[1]
    gen = torch.Generator().manual_seed(11)
    vis = torch.randn(B, t, h, w, C4, generator=gen).to(dev)
    aud = torch.randn(B, 1, ft[0], ft[1], DIM, generator=gen).to(dev)
    Gv = (torch.randn(B, Rv, DIM, generator=gen) * 1e-3).to(dev)
    head = m._contrast_tensors()
    params = list(sb.parameters()) + head
    vpos, apos = sb.vis_pos_embed[0].to(dev), sb.aud_pos_embed[0].to(dev)

    def torch_block(blk, x):
        Bq, Nq, Cq = x.shape
        qkv = F.linear(F.layer_norm(x, (Cq,), blk.norm1.weight, blk.norm1.bias), blk.attn.qkv.weight)
        q, k, v = qkv.reshape(Bq, Nq, 3, HEADS, HD).permute(2, 0, 3, 1, 4).unbind(0)
        o = (torch.softmax(q @ k.transpose(-2, -1) * HD ** -0.5, -1) @ v).transpose(1, 2).reshape(Bq, Nq, Cq)
        x = x + F.linear(o, blk.attn.proj.weight, blk.attn.proj.bias)
        hid = F.gelu(F.linear(F.layer_norm(x, (Cq,), blk.norm2.weight, blk.norm2.bias), blk.mlp.fc1.weight, blk.mlp.fc1.bias))
        return x + F.linear(hid, blk.mlp.fc2.weight, blk.mlp.fc2.bias)

    def D(p, z):
        return -F.cosine_similarity(p, z.detach(), dim=-1).mean()

    def ref():
        v = F.layer_norm(sb.vis_proj(vis.view(B, Rv, C4)), (DIM,), sb.vis_norm.weight, sb.vis_norm.bias) + vpos
        a = F.layer_norm(aud.view(B, Ra, DIM), (DIM,), sb.aud_norm.weight, sb.aud_norm.bias) + apos
        x = torch.cat([v, a], 1)
        for blk in sb.blocks:
            x = torch_block(blk, x)
        ve, ae = m.vis_projector(x[:, :Rv].mean(1)), m.aud_projector(x[:, Rv:].mean(1))
        loss = 0.5 * (D(m.mlp_vis(ve), ae) + D(m.mlp_aud(ae), ve))
        return torch.autograd.grad(loss + (x[:, :Rv] * Gv).sum(), params)

    def hip():
        x = A.sync_block(sb, vis, aud)
        return torch.autograd.grad(A.ContrastHead.apply(x, Rv, *head) + (x[:, :Rv] * Gv).sum(), params)
    for p in params:
        p.requires_grad_(True)
    paths = {"hip": hip, "torch": ref}
    got, want = hip(), ref()                                      # warm-up, and a check
    worst = max(((g - w_).abs().max() / w_.abs().max().clamp_min(1e-30)).item() for g, w_ in zip(got, want))
    del got, want
    torch.cuda.synchronize()
    return dict(rounds_of(paths, reps, rounds), tensors=len(params), tokens=Rv + Ra, worst_grad_rel_diff_vs_torch_fp32=worst)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 2])
    ap.add_argument("--height", type=int, default=224)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--wa", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sync_train_bench needs an MI355X (no CPU fallback)")
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    from mspi_amd import inference as I
    from mspi_amd import metrics as M
    from mspi_amd import testing as T
    dev = torch.device("cuda", 0)
    I.device = dev
    H, W = args.height, args.width
    m = T.randomize_(I.build_model("x3dl", (H, W), wa=args.wa), 0)
    E.autotune(False)                  # as mspi_amd.train: the trained layers are re-packed at every step, nothing to tune once
    m.trainable("adapter", sync=True)
    m.train()
    m.frozen_encoder()
    out = {"reps": args.reps, "rounds": args.rounds, "model": "x3dl", "frame": [H, W], "wa": args.wa,
           "device": torch.cuda.get_device_name(0), "batches": {}}
    thw, ft = (16, H // 32, W // 32), (9, (args.wa + 31) // 32)
    for B in args.batches:
        clips, audio = T.synth_inputs(B, 16, H, W, Wa=args.wa, seed=100, device=dev)
        label = density(B, H, W).to(dev)
        row = out["batches"][str(B)] = {"step": whole_step(m, M, clips, audio, label, args.reps, args.rounds)}
        for p in m.parameters():
            p.grad = None
        del clips, audio, label
        m.trainable("adapter", sync=True)
        row["added_layers"] = added_layers(m, A, dev, B, thw, ft, args.reps, args.rounds)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
