"""Writes tests/golden/saliency_eval.npz: binary fixation maps and what the REFERENCE's own resize_fixation
(avsp_dataloader.py:16-31) makes of them, and asserts tests/saliency_eval_restate.py against it on the way.  The function
is imported from the reference checkout (oracle.ref_harness.REF), never restated here; the third-party modules that file
imports at its top and that are absent offline are inert stubs.  Run from the repository root:

    python tools/gen_eval_golden.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness as rh  # noqa: E402
import saliency_eval_restate as E  # noqa: E402

# name, (H, W), (row, col), fixation probability
CASES = (
    ("real", (480, 640), (224, 384), 0.004),     # the loader's case; the last row rounds to `row` and is stepped back
    ("ties", (448, 640), (224, 320), 0.02),      # ratio 1/2: every odd row / column lands on .5
    ("up", (100, 120), (224, 384), 0.02),        # enlarging
    ("odd", (37, 53), (17, 20), 0.3),            # many fixations per target
    ("hd", (720, 1280), (224, 384), 0.002),      # shrinking from HD
    ("empty", (48, 64), (24, 40), 0.0),
    ("same", (60, 80), (60, 80), 0.05),
)


def _stub(name, **attrs):
    if name not in sys.modules:
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    return sys.modules[name]


def _reference():
    """avsp_dataloader.resize_fixation of the reference; cv2, torchaudio, torchvision and timm are only named at import."""
    _stub("cv2")
    _stub("torchaudio")
    _stub("torchvision", transforms=_stub("torchvision.transforms"))
    _stub("timm")
    _stub("timm.data")
    _stub("timm.data.constants", IMAGENET_DEFAULT_MEAN=(0.485, 0.456, 0.406), IMAGENET_DEFAULT_STD=(0.229, 0.224, 0.225))
    cwd = os.getcwd()
    rh.enter_reference()
    import avsp_dataloader
    os.chdir(cwd)
    return avsp_dataloader.resize_fixation


def main():
    resize_fixation = _reference()
    rng = np.random.default_rng(20241)
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, (H, W), (row, col), p in CASES:
        fix = (rng.random((H, W)) < p).astype(np.uint8)
        if p > 0:
            fix[H - 1, 0] = fix[H - 1, W - 1] = 1           # bottom corners: the `== row` / `== col` step back is taken
        ref = resize_fixation(fix, row, col)
        assert ref.shape == (row, col) and ref.dtype == np.float64 and set(np.unique(ref)) <= {0.0, 1.0}
        got = E.resize_fixation(fix, row, col)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), name
        assert np.array_equal(E.resize_fixation(fix.astype(np.float32), row, col), ref), name
        r = np.arange(H) * (row / H)
        print("[resize_fixation] %-5s %4dx%-4d -> %3dx%-3d  %5d fixations -> %5d   tie rows %3d, rows stepped back %d" % (
            name, H, W, row, col, int(fix.sum()), int(ref.sum()), int((r % 1 == 0.5).sum()), int((np.rint(r) == row).sum())))
        out["%s_fix" % name] = fix
        out["%s_to" % name] = np.array([row, col], np.int32)
        out["%s_out" % name] = ref.astype(np.uint8)          # binary: uint8 holds it exactly
    path = os.path.join(ROOT, "tests", "golden", "saliency_eval.npz")
    np.savez_compressed(path, **out)
    print("[golden] %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
