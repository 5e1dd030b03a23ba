#!/usr/bin/env python3
"""What decoding the input JPEG frames costs, on the device and on the host.  Measurement only, no threshold.

(a) engine.jpeg_decode_rgb on N = 8 and N = 16 frames of 480x640, 4:2:0, quality 90: HIP events around the whole call (packing
    on the host, the H2D copy, five launches), median of 30 after 10 warm-ups, the synchronisation passes seen and the
    per-kernel split (torch.profiler's device times of the jpegdec_* kernels over 10 calls).  Beside it PIL's decoder on this
    box's host with 1 and with 8 threads, and the bytes uploaded each way (the scans + tables / the pixels).
(b) files -> files windows/s of inference.inference_dataset on a generated 480x640 JPEG toy video, x3dl, batch 8: four runs
    in one process -- flags off, --device_decode, --workers 8, all three flags -- after one untimed run that tunes the kernels.

  python tools/jpeg_decode_bench.py [--frames 80] [--out profiles/r06_jpeg_decode.txt]
"""
import argparse
import io
import os
import sys
import tempfile
import time
import types
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from mspi_amd import engine as E, inference as I, testing as T

dev = torch.device("cuda")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def frame(i, base):
    """A smooth, moving texture: frames that decode at the cost of a real video's."""
    return Image.fromarray(np.roll(base, i, axis=1)).resize((640, 480), Image.BILINEAR)


def frame_bytes(i, base):
    b = io.BytesIO()
    frame(i, base).save(b, format="JPEG", quality=90)
    return b.getvalue()


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def kernel_split(files, calls=10):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                E.jpeg_decode_rgb(files)
            torch.cuda.synchronize()
        rows = {}
        for ev in prof.events():
            if "jpegdec_" in ev.name:
                name = ev.name[ev.name.index("jpegdec_"):].split("(")[0].split("E")[0]
                rows[name] = rows.get(name, 0.0) + (ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {k: v / calls for k, v in rows.items()}
    except Exception as e:      # the split is a nicety; the event times above stand without it
        say("    (per-kernel split unavailable: %s)" % e)
        return {}


def part_a():
    base = np.random.RandomState(0).randint(0, 255, (60, 80, 3), dtype=np.uint8)
    for n in (8, 16):
        files = [frame_bytes(i, base) for i in range(n)]
        ms = []
        for it in range(40):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rgb, status, passes = E.jpeg_decode_rgb(files)
            e1.record()
            e1.synchronize()
            if it >= 10:
                ms.append(e0.elapsed_time(e1))
        same = all(np.array_equal(rgb[k].cpu().numpy(), pil_decode(files[k])) for k in range(n))
        info = E.jpeg_probe(files[0])
        cap = (max(E.jpeg_probe(f).scan_len for f in files) + 15) // 16 * 16
        say("(a) %d frames 480x640, 4:2:0, quality 90 (files of %d...%d bytes, S = %d)" % (
            n, min(map(len, files)), max(map(len, files)), E.jpeg_subseq_bits(cap)))
        say("    device decode (5 launches + copy): median %.3f ms per batch, min %.3f, max %.3f; pixels %s PIL's; status %s; passes %s" % (
            float(np.median(ms)), min(ms), max(ms), "==" if same else "!=", sorted(set(status.tolist())), sorted(set(passes.tolist()))))
        split = kernel_split(files)
        if split:
            say("    per kernel, us per batch         : " + ", ".join("%s %.1f" % (k.replace("jpegdec_", "").replace("_kernel", ""), v)
                                                                       for k, v in sorted(split.items())))
        for threads in (1, 8):
            ts = []
            with ThreadPoolExecutor(threads) as pool:
                for it in range(20):
                    t0 = time.perf_counter()
                    list(pool.map(pil_decode, files))
                    if it >= 5:
                        ts.append(1e3 * (time.perf_counter() - t0))
            say("    PIL on the host, %d thread%s      : median %.3f ms per batch" % (threads, " " if threads == 1 else "s", float(np.median(ts))))
        say("    H2D per batch                    : scans + tables %d bytes, pixels %d bytes" % (
            n * (cap + 1488), n * info.H * info.W * 3))


def make_video(root, n_frames, name="clip1", fps=25, sr=16000):
    from scipy.io import wavfile
    rng = np.random.RandomState(0)
    fdir = os.path.join(root, "video_frames", "TOY", name)
    adir = os.path.join(root, "video_audio", "TOY", name)
    os.makedirs(fdir), os.makedirs(adir), os.makedirs(os.path.join(root, "fold_lists"))
    base = rng.randint(0, 255, (60, 80, 3), dtype=np.uint8)
    for i in range(n_frames):
        frame(i, base).save(os.path.join(fdir, "img_%05d.jpg" % (i + 1)), quality=90)
    t = np.arange(int(sr * n_frames / fps) + sr) / sr
    wavfile.write(os.path.join(adir, name + ".wav"), sr, (0.3 * np.sin(2 * np.pi * 440 * t)).astype(np.float32))
    with open(os.path.join(root, "fold_lists", "TOY_list_test_2_fps.txt"), "w") as f:
        f.write("%s %d %d\n" % (name, n_frames, fps))


def part_b(n_frames):
    res = (224, 384)
    I.device = dev
    I._RESOLUTION[:] = list(res)
    so, sys.stdout = sys.stdout, open(os.devnull, "w")
    model = I.build_model("x3dl", res)
    T.randomize_(model.cpu(), 0)
    model = model.to(dev).eval()
    sys.stdout = so
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "data")
        make_video(root, n_frames)
        runs = (("warm-up (tuning)", {}), ("flags off", {}), ("--device_decode", dict(device_decode=True)),
                ("--workers 8", dict(workers=8)),
                ("--device_decode --device_jpeg --workers 8", dict(device_decode=True, device_jpeg=True, workers=8)))
        say("(b) inference_dataset, x3dl %dx%d, batch 8, %d frames of 480x640 JPEG in, %d maps of 480x640 JPEG out" % (
            res[0], res[1], n_frames, n_frames))
        trees, base = {}, None
        for k, (tag, kw) in enumerate(runs):
            args = types.SimpleNamespace(clip_size=16, dataset="TOY", split=2, path_data=root, save_path=os.path.join(tmp, "out%d" % k),
                                         use_sound=True, batch=8, **kw)
            so, sys.stdout = sys.stdout, open(os.devnull, "w")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            I.inference_dataset(model, args)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            sys.stdout = so
            d = os.path.join(args.save_path, "clip1")
            trees[tag] = {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}
            if k == 0:
                continue
            rate = n_frames / dt
            base = rate if base is None else base
            say("    %-42s: %7.1f windows/s (x%.2f of flags off), files %s" % (
                tag, rate, rate / base, "identical to flags off" if trees[tag] == trees["flags off"] else "DIFFERENT"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip_loop", action="store_true")
    a = ap.parse_args()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        part_a()
    if not a.skip_loop:
        part_b(a.frames)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
