"""CRC32 digests of one training step per model and stage: what a change of the training path's Python must leave bit for bit.

    python tools/train_step_digest.py [--launches]

For each of the four models of tests/test_entry_train.py::MODELS and each of the six stages model.trainable() takes, on a fresh
model built as tests/test_readout_tail._build builds it: trainable(stage), train(), frozen_encoder(), one forward with grad,
metrics.SalLoss against a seeded Gaussian density, backward.  On the audio-visual models a seventh case, "adapter+sync":
trainable("adapter", sync=True), and loss_av added to the criterion before the backward (its own line, `out loss_av`).  On a
commit whose trainable() has no such keyword that case is left out.  Autotuning is off and the autotune cache empty, so the library's
own kernel choices hold.  One line per case, stage and tensor -- `case stage kind name crc32 numel` -- for the output map,
every gradient and every buffer the step moved (the BatchNorm running statistics).  --launches: also the engine.Profiler
summary of one more trainable("adapter") step on av_x3dl_64, one `launch kernel calls` line per kernel name.  Only the public
surface is used, so the same file runs on an older commit; two outputs are compared with diff.  Needs the GPU."""
import argparse
import contextlib
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = ("readout_tail", "readout", "fusion", "lateral_blocks", "lateral_entries", "adapter")
SYNC = "adapter+sync"                    # trainable("adapter", sync=True): the audio-visual models only


def crc(t):
    return "%08x" % zlib.crc32(t.detach().cpu().contiguous().numpy().tobytes())


def density(B, H, W, seed=900):
    """Two Gaussian blobs per sample, the peak at 1, values below 1e-3 exactly 0."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    m = np.zeros((B, H, W), np.float32)
    for b in range(B):
        for _ in range(2):
            cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.05, 0.15) * min(H, W)
            m[b] += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32)
    m = m / m.reshape(B, -1).max(1).reshape(B, 1, 1)
    m[m < 1e-3] = 0
    return torch.from_numpy(m)


def step(m, args, label, loss, sync=False):
    for p in m.parameters():
        p.grad = None
    out, aux = m(*args)
    assert out.requires_grad and (not sync or aux.requires_grad)
    (loss(out, label) + aux if sync else loss(out, label)).backward()
    torch.cuda.synchronize()
    return out, aux


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true")
    opts = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_step_digest needs an MI355X (no CPU fallback)")
    from mspi_amd import engine as E
    from mspi_amd import metrics as M
    from test_entry_train import MODELS
    from test_readout_tail import _build
    E.autotune(False)
    E.AUTOTUNE["cache"].clear()
    dev = torch.device("cuda", 0)
    golden = os.path.join(ROOT, "tests", "golden")
    for case, name, cls, _ in MODELS:
        _, _, make, clips, audio = _build(golden, case, name, cls, dev)
        args = (clips, audio) if cls == "AudioVisualSaliencyModel" else (clips,)
        label = density(clips.shape[0], clips.shape[3], clips.shape[4]).to(dev)
        for stage in STAGES + ((SYNC,) if len(args) == 2 else ()):
            with contextlib.redirect_stdout(sys.stderr):      # the constructors announce their encoder
                m = make().to(dev)
            sync = stage == SYNC
            if sync:
                try:
                    m.trainable("adapter", sync=True)
                except TypeError:                             # an older commit: no keyword, no case
                    continue
            else:
                m.trainable(stage)
            m.train()
            m.frozen_encoder()
            before = {k: v.clone() for k, v in m.named_buffers()}
            out, aux = step(m, args, label, M.SalLoss(), sync)
            print("%s %s out map %s %d" % (case, stage, crc(out), out.numel()))
            if sync:
                print("%s %s out loss_av %s %d" % (case, stage, crc(aux), aux.numel()))
            for n, p in sorted(m.named_parameters()):
                if p.grad is not None:
                    print("%s %s grad %s %s %d" % (case, stage, n, crc(p.grad), p.grad.numel()))
            for n, b in sorted(m.named_buffers()):
                if not torch.equal(b, before[n]):
                    print("%s %s buffer %s %s %d" % (case, stage, n, crc(b), b.numel()))
            if opts.launches and (case, stage) == ("av_x3dl_64", "adapter"):
                with E.Profiler() as prof:
                    step(m, args, label, M.SalLoss())
                for k, v in sorted(prof.summary().items()):
                    print("launch %s %d" % (k, v["calls"]))
            sys.stdout.flush()
            del m


if __name__ == "__main__":
    main()
