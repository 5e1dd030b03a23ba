"""Device time of the evaluate step (mspi_amd/evaluate.py) for one batch of 8 frames at 480x640, upload excluded: the
resize of the prediction and of the density plus all seven metrics, next to the resize kernels on their own (time and
bytes / time) and to the frames/s of a whole evaluate_dataset run over a synthetic tree of 480x640 JPEG files.  HIP events,
median of --iters iterations after --warmup warm-up iterations, on an otherwise idle device.  Measurement only:

    python tools/eval_step_bench.py [--iters 30] [--warmup 10] [--frames 32] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mspi_amd import _lib  # noqa: E402
from mspi_amd import evaluate as E  # noqa: E402
from mspi_amd import metrics as M  # noqa: E402


def event_us(fn, iters, warmup, inner=1):
    """Median over `iters` of the HIP-event time of `inner` back-to-back calls of fn, per call, in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(times), min(times), max(times)


def smooth_u8(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    m = np.zeros((H, W), np.float32)
    for _ in range(5):
        cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(H / 16, H / 4)
        m += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32)
    return np.round(8 + 247 * m / m.max()).astype(np.uint8)


def toy_tree(root, rng, videos, frames, hw):
    from PIL import Image
    import scipy.io
    data, pred = os.path.join(root, "data"), os.path.join(root, "pred")
    os.makedirs(os.path.join(data, "fold_lists"))
    with open(os.path.join(data, "fold_lists", "TOY_list_test_2_fps.txt"), "w") as f:
        for v in range(videos):
            f.write("clip%d %d 25\n" % (v, frames))
    for v in range(videos):
        ann = os.path.join(data, "annotations", "TOY", "clip%d" % v)
        os.makedirs(os.path.join(ann, "maps"))
        os.makedirs(os.path.join(pred, "clip%d" % v))
        for i in range(1, frames + 1):
            Image.fromarray(smooth_u8(rng, *hw)).save(os.path.join(ann, "maps", "eyeMap_%05d.jpg" % i))
            Image.fromarray(smooth_u8(rng, *hw)).save(os.path.join(pred, "clip%d" % v, "img_%05d.jpg" % i))
            fix = np.zeros(hw, np.uint8)
            fix.reshape(-1)[rng.choice(hw[0] * hw[1], size=300, replace=False)] = 1
            scipy.io.savemat(os.path.join(ann, "fixMap_%05d.mat" % i), {"eyeMap": fix}, do_compression=True)
    return pred, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=32, help="frames per video of the synthetic tree (3 videos)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_step_bench.py needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rng = np.random.default_rng(0)
    B, H, W = 8, 480, 640
    pred = torch.from_numpy(np.stack([smooth_u8(rng, H, W) for _ in range(B)])).to(dev)
    dens = torch.from_numpy(np.stack([smooth_u8(rng, H, W) for _ in range(B)])).to(dev)
    fix = np.zeros((B, H * W), np.float32)
    other = np.zeros((B, H * W), np.float32)
    for b in range(B):
        fix[b, rng.choice(H * W, size=300, replace=False)] = 1
        other[b, rng.choice(H * W, size=1497, replace=False)] = 1
    fix, other = torch.from_numpy(fix).view(B, H, W).to(dev), torch.from_numpy(other).view(B, H, W).to(dev)
    base = (torch.rand(B, H, W, device=dev) + 0.1)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {"batch": B, "size": [H, W], "iters": args.iters, "warmup": args.warmup}

    def step():
        s = E.resize_maps(pred, (H, W))
        d = E.resize_maps(dens, (H, W))
        return (M.per_sample(s, d, fix=fix), M.auc_judd_per_sample(s, fix, True, gen), M.sauc_counts(s, fix, other),
                M.ig_per_sample(s, fix, base))

    def step_small():                 # a prediction kept at the model's size, brought to the annotation's size
        s = E.resize_maps(pred_small, (H, W))
        d = E.resize_maps(dens, (H, W))
        return (M.per_sample(s, d, fix=fix), M.auc_judd_per_sample(s, fix, True, gen), M.sauc_counts(s, fix, other),
                M.ig_per_sample(s, fix, base))

    pred_small = torch.from_numpy(np.stack([smooth_u8(rng, 224, 384) for _ in range(B)])).to(dev)
    s, d = E.resize_maps(pred, (H, W)), E.resize_maps(dens, (H, W))
    res["step_us"] = event_us(step, args.iters, args.warmup)
    res["step_from_224x384_us"] = event_us(step_small, args.iters, args.warmup)
    res["metrics_only_us"] = event_us(lambda: (M.per_sample(s, d, fix=fix), M.auc_judd_per_sample(s, fix, True, gen),
                                               M.sauc_counts(s, fix, other), M.ig_per_sample(s, fix, base)), args.iters, args.warmup)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kernels = {}
    for name, src, (Ho, Wo) in (("u8 480x640 -> 480x640 (conversion)", pred, (H, W)),
                                ("u8 224x384 -> 480x640", pred_small, (H, W)),
                                ("u8 480x640 -> 224x384", pred, (224, 384)),
                                ("u8 480x640 -> 720x1280", pred, (720, 1280)),
                                ("f32 480x640 -> 720x1280", s, (720, 1280))):
        out = torch.empty(B, Ho, Wo, dtype=torch.float32, device=dev)
        u8 = 1 if src.dtype == torch.uint8 else 0
        call = lambda: lib.mspi_resize_bilinear_fwd(src.data_ptr(), u8, out.data_ptr(), B, src.shape[1], src.shape[2], Ho, Wo, stream)
        med, lo, hi = event_us(call, args.iters, args.warmup, inner=20)
        nbytes = src.numel() * src.element_size() + out.numel() * 4
        kernels[name] = {"us": med, "min_us": lo, "max_us": hi, "bytes": nbytes, "TB_per_s": nbytes / med * 1e-6}
    for name, (row, col) in (("fixation 480x640 -> 224x384", (224, 384)), ("fixation 480x640 -> 720x1280", (720, 1280))):
        out = torch.empty(B, row, col, dtype=torch.float32, device=dev)
        call = lambda: lib.mspi_resize_fixation_fwd(fix.data_ptr(), out.data_ptr(), B, H, W, row, col, stream)
        med, lo, hi = event_us(call, args.iters, args.warmup, inner=20)
        nbytes = fix.numel() * 4 + out.numel() * 4
        kernels[name] = {"us": med, "min_us": lo, "max_us": hi, "bytes": nbytes, "TB_per_s": nbytes / med * 1e-6}
    res["kernels"] = kernels
    # a copy of the same 8 x 480 x 640 floats, the yardstick of the memory-bound kernels
    a, b = torch.empty(B, H, W, device=dev), torch.empty(B, H, W, device=dev)
    med, _, _ = event_us(lambda: b.copy_(a), args.iters, args.warmup, inner=20)
    res["copy_8x480x640_f32"] = {"us": med, "TB_per_s": 2 * a.numel() * 4 / med * 1e-6}

    with tempfile.TemporaryDirectory() as tmp:
        p, dset = toy_tree(tmp, rng, 3, args.frames, (H, W))
        for kw in ({}, {"other": 3, "baseline": "mean"}):
            E.evaluate_dataset(p, dset, "TOY", 2, device=dev, batch=B, **kw)          # warm: file cache, code objects
            torch.cuda.synchronize()
            t0 = time.time()
            r = E.evaluate_dataset(p, dset, "TOY", 2, device=dev, batch=B, **kw)
            torch.cuda.synchronize()
            dt = time.time() - t0
            res["toy_run" + ("_other3_mean" if kw else "")] = {"frames": r["frames"], "seconds": dt, "frames_per_s": r["frames"] / dt}
        t0 = time.time()
        n = 0
        for _, frames in E.host_batches(E.plan(p, dset, "TOY", 2), batch=B, prefetch=False):
            n += len(frames)
        res["host_decode_only"] = {"frames": n, "seconds": time.time() - t0, "frames_per_s": n / (time.time() - t0)}
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
