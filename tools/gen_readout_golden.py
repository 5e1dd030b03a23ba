"""Writes tests/golden/readout.npz: fp32 inputs and parameters of the whole readout at decoder width 32 (128 -> 32 -> 32 -> 64
-> tail) and, in float64, the value and the 16 parameter gradients that torch autograd gives through torch.nn layers built
with upstream's arguments (model/model_utils.py:490-504, BatchNorm in .train() mode) over the 128-channel concat.  Asserts
tests/readout_restate.py (this project's order, readout[0] split over the coarse maps, analytic backward) against it to 1e-12
on the way, for "tiny" (pyramid base (B, a, b) = (1, 1, 2)) and for "odd" ((2, 2, 3)).

Only "tiny" is stored with its gradients.  Its seed is searched until torch FLOAT32 on the CPU agrees with float64 to 2e-6 on
every gradient, so that no ReLU unit sits on its kink and an fp32 device can be compared end to end.  On "odd" fp32 and
float64 differ by flipped masks (about 3e-3): it is stored as its seed alone, rebuilt by readout_restate.make_case, and
goes through the per-entry-point tests with the masks it is given.  Run from the repository root:

    python tools/gen_readout_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import readout_restate as R  # noqa: E402

CASES = (("tiny", 1, 1, 2), ("odd", 2, 2, 3))
FP32_AGREES = 2e-6


def rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def grad_err(k, got, ref, gsum):
    """Gradients that are zero in exact arithmetic (the biases in front of a BatchNorm, the bias in front of the log-softmax)
    are measured against sum|g|, the others against their own largest entry."""
    if k in ("b1", "b4", "b12"):
        return (got - ref).abs().max().item() / gsum
    return rel(got, ref)


def pinned(case, name):
    saved = R.forward(case)
    grads = R.backward(case, saved, case["g"])
    ref_out, ref, _ = R.upstream_grads(case)
    gsum = float(np.abs(case["g"]).astype(np.float64).sum())
    assert (saved["out"] - ref_out).abs().max().item() <= 1e-12, name
    for k in R.PARAMS:
        err = grad_err(k, grads[k], ref[k], gsum)
        assert err <= 1e-12, (name, k, err)
    return ref_out, ref, gsum


def main():
    out = {"cases": np.array([c[0] for c in CASES])}
    for i, (name, B, a, b) in enumerate(CASES):
        for seed in range(8600 + 100 * i, 8600 + 100 * i + 40):
            case = R.make_case(B, a, b, seed)
            if name != "tiny":
                break
            _, ref, gsum = pinned(case, name)
            _, g32, _ = R.upstream_grads(case, torch.float32)
            worst = max(grad_err(k, g32[k].double(), ref[k], gsum) for k in R.PARAMS)
            if worst <= FP32_AGREES:
                break
        else:
            raise SystemExit("%s: no seed on which fp32 agrees with float64 to %g" % (name, FP32_AGREES))
        ref_out, ref, gsum = pinned(case, name)
        out["%s_seed" % name] = np.array(seed)
        out["%s_shape" % name] = np.array([B, a, b])
        if name == "tiny":
            print("[%s] seed %d: fp32 CPU against float64, worst gradient %.1e" % (name, seed, worst))
            out.update({"%s_%s" % (name, k): v for k, v in case.items()})
            out["%s_out" % name] = ref_out.numpy()
            out.update({"%s_d_%s" % (name, k): ref[k].numpy() for k in R.PARAMS})
        else:
            _, g32, _ = R.upstream_grads(case, torch.float32)
            print("[%s] seed %d: fp32 CPU against float64, worst gradient %.1e (flipped masks: not compared end to end)"
                  % (name, seed, max(grad_err(k, g32[k].double(), ref[k], gsum) for k in R.PARAMS)))
    path = os.path.join(ROOT, "tests", "golden", "readout.npz")
    np.savez_compressed(path, **out)
    print("[golden] %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
