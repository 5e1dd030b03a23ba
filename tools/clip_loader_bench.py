"""Device time of assembling one validation batch of clips -- 128 decoded frames 480x640 -> fp32 [8,3,16,224,384] -- through
preproc.assemble_clips (one launch of mspi_clip_resize_norm_fwd) and through the per-frame path it replaces: 128 x
preproc.resize_normalize (two launches and a torch.empty each), then torch.stack + permute + contiguous per clip batch.
Upload excluded; both paths start from the same uint8 frames on the device and are checked to produce equal bits first.

  * idle: HIP events around one assembly, median of --iters after --warmup, the two paths alternating, nothing else queued;
  * loaded: the same with bench.py's model (x3dl, batch 8, 224x224, eager launches) running on a second stream: --load
    forwards are queued first, then --loaded-iters assemblies are timed as one window; a window only counts when the model
    was still running at its end.  This project ranks kernels under load.

Measurement only:   python tools/clip_loader_bench.py [--iters 30] [--warmup 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mspi_amd import preproc as P  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def event_us(fn, n=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def summary(times):
    return {"median_us": statistics.median(times), "min_us": min(times), "max_us": max(times), "n": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--load", type=int, default=4, help="model forwards queued on the second stream per loaded window")
    ap.add_argument("--loaded-iters", type=int, default=8, help="assemblies timed per loaded window")
    ap.add_argument("--windows", type=int, default=5, help="loaded windows per path")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_loader_bench.py needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda:0")
    B, T, Hin, Win, Hout, Wout = 8, 16, 480, 640, 224, 384
    N = B * T
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (N, Hin, Win, 3), dtype=np.uint8)).to(dev)
    slots = np.arange(N, dtype=np.int32)
    slots_dev = torch.from_numpy(slots).to(dev)
    out = torch.empty(B, 3, T, Hout, Wout, device=dev)

    def new():
        return P.assemble_clips(frames, slots, out, MEAN, STD, slots_dev=slots_dev)

    def parent():
        per = [P.resize_normalize(frames[i], (Hout, Wout), MEAN, STD) for i in range(N)]
        return torch.stack([torch.stack(per[b * T:(b + 1) * T]).permute(1, 0, 2, 3) for b in range(B)])

    assert torch.equal(new(), parent()), "the two paths differ"
    res = {"frames": N, "src": [Hin, Win], "dst": [Hout, Wout], "plan": P.clip_tile_plan(Hin, Win, Hout, Wout),
           "iters": args.iters, "warmup": args.warmup, "launches": {"assemble_clips": 1, "per_frame": 2 * N},
           "bytes": {"read_u8": frames.numel(), "written_f32": out.numel() * 4}}
    for _ in range(args.warmup):
        new(), parent()
    torch.cuda.synchronize()
    t_new, t_par = [], []
    for _ in range(args.iters):                                  # alternating, same process, same frames
        t_new.append(event_us(new))
        t_par.append(event_us(parent))
    res["idle"] = {"assemble_clips": summary(t_new), "per_frame": summary(t_par)}
    res["idle"]["speedup"] = res["idle"]["per_frame"]["median_us"] / res["idle"]["assemble_clips"]["median_us"]
    res["idle"]["assemble_clips"]["frames_per_s"] = N / res["idle"]["assemble_clips"]["median_us"] * 1e6
    res["idle"]["per_frame"]["frames_per_s"] = N / res["idle"]["per_frame"]["median_us"] * 1e6
    res["idle"]["assemble_clips"]["TB_per_s"] = (frames.numel() + out.numel() * 4) / res["idle"]["assemble_clips"]["median_us"] * 1e-6

    # loaded: bench.py's model on a second stream
    from mspi_amd import engine as E
    from mspi_amd import testing as Tm
    from mspi_amd.model.model_utils import AudioVisualSaliencyModel
    cfg = Tm.make_cfg("x3dl", num_aud_tokens=9 * ((300 + 31) // 32), num_vis_tokens=16 * 7 * 7)
    so, sys.stdout = sys.stdout, open(os.devnull, "w")
    try:
        model = Tm.seeded(lambda: AudioVisualSaliencyModel(cfg), 0).to(dev)
    finally:
        sys.stdout = so
    clips, audio = Tm.synth_inputs(8, 16, 224, 224, Wa=300, seed=100, device=dev)
    E.autotune(False)
    with torch.no_grad():
        model(clips, audio)
        torch.cuda.synchronize()
        res["model_forward_us"] = event_us(lambda: model(clips, audio), 3)
        side, main = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        loaded = {"assemble_clips": [], "per_frame": []}
        dropped = 0
        for _ in range(args.windows):
            for name, fn in (("assemble_clips", new), ("per_frame", parent)):
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(args.load):
                        model(clips, audio)
                    done = torch.cuda.Event()
                    done.record()
                with torch.cuda.stream(main):                    # not the NULL stream: it would order itself behind the model
                    us = event_us(fn, args.loaded_iters)
                if done.query():                                # the model had finished: not a loaded window
                    dropped += 1
                else:
                    loaded[name].append(us)
                torch.cuda.synchronize()
    res["loaded"] = {k: (summary(v) if v else None) for k, v in loaded.items()}
    res["loaded"]["windows_dropped"] = dropped
    for k in ("assemble_clips", "per_frame"):
        if res["loaded"][k]:
            res["loaded"][k]["frames_per_s"] = N / res["loaded"][k]["median_us"] * 1e6
    if res["loaded"]["assemble_clips"] and res["loaded"]["per_frame"]:
        res["loaded"]["speedup"] = res["loaded"]["per_frame"]["median_us"] / res["loaded"]["assemble_clips"]["median_us"]
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
