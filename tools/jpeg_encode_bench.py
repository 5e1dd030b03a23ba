#!/usr/bin/env python3
"""What writing the saliency maps as JPEG costs, on the device and on the host.  Measurement only, no threshold.

(a) engine.jpeg_encode_gray on 8 blob maps of 480x640 at quality 95: HIP events, median of 30 after 10 warm-ups.  Beside it
    PIL's encoder on this box's host with 1 and with 8 threads, and the D2H bytes of both forms (the files / the pixels).
(b) files -> files windows/s of inference.inference_dataset on a generated 480x640 JPEG toy video, x3dl, batch 8: four runs
    in one process -- flags off, --device_jpeg, --workers 8, both -- after one untimed run that tunes the kernels.

  python tools/jpeg_encode_bench.py [--frames 80] [--out profiles/r05_jpeg_encode.txt]
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


def blob(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g = np.zeros((h, w))
    for _ in range(4):
        cy, cx, s, a = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.2) * max(h, w), rng.uniform(0.3, 1.0)
        g += a * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return np.round(255 * g / g.max()).astype(np.uint8)


def pil_encode(m):
    b = io.BytesIO()
    Image.fromarray(m).save(b, format="JPEG", quality=95)
    return b.getvalue()


def part_a():
    maps = np.stack([blob(480, 640, s) for s in range(8)])
    dmaps = torch.from_numpy(maps).to(dev)
    ms = []
    for it in range(40):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        files, lengths = E.jpeg_encode_gray(dmaps, 95)
        e1.record()
        e1.synchronize()
        if it >= 10:
            ms.append(e0.elapsed_time(e1))
    lens = lengths.cpu().numpy()
    same = all(files[b, : lens[b]].cpu().numpy().tobytes() == pil_encode(maps[b]) for b in range(8))
    say("(a) 8 blob maps 480x640, quality 95")
    say("    device encode (4 launches)       : median %.3f ms per batch, min %.3f, max %.3f; files %s PIL's" % (
        float(np.median(ms)), min(ms), max(ms), "==" if same else "!="))
    for threads in (1, 8):
        ts = []
        with ThreadPoolExecutor(threads) as pool:
            for it in range(40):
                t0 = time.perf_counter()
                list(pool.map(pil_encode, maps))
                if it >= 10:
                    ts.append(1e3 * (time.perf_counter() - t0))
        say("    PIL on the host, %d thread%s      : median %.3f ms per batch" % (threads, " " if threads == 1 else "s", float(np.median(ts))))
    say("    D2H per batch                    : files %d bytes (longest file x 8: %d), pixels %d bytes" % (
        int(lens.sum()), int(lens.max()) * 8, maps.size))


def make_video(root, n_frames, name="clip1", fps=25, sr=16000):
    from scipy.io import wavfile
    rng = np.random.RandomState(0)
    fdir = os.path.join(root, "video_frames", "TOY", name)
    adir = os.path.join(root, "video_audio", "TOY", name)
    os.makedirs(fdir), os.makedirs(adir), os.makedirs(os.path.join(root, "fold_lists"))
    base = rng.randint(0, 255, (60, 80, 3), dtype=np.uint8)
    for i in range(n_frames):        # a smooth, moving texture: frames that decode at the cost of a real video's
        img = Image.fromarray(np.roll(base, i, axis=1)).resize((640, 480), Image.BILINEAR)
        img.save(os.path.join(fdir, "img_%05d.jpg" % (i + 1)), quality=90)
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
        runs = (("warm-up (tuning)", {}), ("flags off", {}), ("--device_jpeg", dict(device_jpeg=True)),
                ("--workers 8", dict(workers=8)), ("--device_jpeg --workers 8", dict(device_jpeg=True, workers=8)))
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
            say("    %-28s: %7.1f windows/s (x%.2f of flags off), files %s" % (
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
