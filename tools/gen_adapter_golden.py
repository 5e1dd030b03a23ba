"""Writes tests/golden/adapter.npz: for the adapter's Inception (eight conv -> BatchNorm3d -> ReLU layers on batch statistics),
in float64, the output `masks` and the gradients of <masks, G> for its 24 tensors as torch autograd gives them through
torch.nn layers built with upstream's arguments (BasicConv3d / SepConv3d of backbones/s3d.py: Conv3d without bias,
BatchNorm3d(eps=1e-3, momentum=0.001) in .train() mode, ReLU; MaxPool3d(3, 1, 1) in front of branch3).  Asserts
tests/adapter_restate.py (this project's launch order, analytic backward) against it to 1e-12 on the way, and the restated
gradient of the Fusion stage's `masks` against torch autograd through upstream's SA modules likewise.

Cases.  "tiny" (B, T, h, w) = (1, 2, 2, 3), 12 rows, at the scaled-down widths adapter_restate.SMALL (at the model's widths the
float64 weight gradients are about 3.8 MB; the file must stay below readout.npz, the largest fixture) is stored with its
float64 results.  "odd" (2, 2, 3, 5) at the same widths and "full" (1, 4, 3, 4) at the model's widths are stored as seeds
alone, and so are "fusion_tiny" and "fusion_odd", the fusion_restate cases (1, 1, 1, 2) and (2, 2, 2, 3) on which the gradient
of `masks` is checked: adapter_restate.make_case / fusion_restate.make_case rebuild the fp32 inputs from the seed (numpy's
RandomState stream is frozen).  Every seed is searched until torch FLOAT32 on the CPU agrees with float64 to 2e-6 of every
gradient's largest entry, so that no ReLU unit sits on its kink and an fp32 device can be compared end to end; the figure
of every case is printed.  Run from the repository root:

    python tools/gen_adapter_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adapter_restate as AR  # noqa: E402
import fusion_restate as FR  # noqa: E402

CASES = (("tiny", (1, 2, 2, 3), AR.SMALL), ("odd", (2, 2, 3, 5), AR.SMALL), ("full", (1, 4, 3, 4), AR.WIDTHS))
FUSION_CASES = (("fusion_tiny", (1, 1, 1, 2)), ("fusion_odd", (2, 2, 2, 3)))
FP32_AGREES = 2e-6
SEEDS = 400


def rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def pinned(case, name):
    sv = AR.forward(case)
    grads = AR.backward(case, sv)
    masks, ref, layers = AR.upstream_grads(case)
    assert (sv["masks"] - masks).abs().max().item() <= 1e-12, name
    for k in AR.PARAMS:
        assert rel(grads[k], ref[k]) <= 1e-12, (name, k, rel(grads[k], ref[k]))
    for l, (_, bn) in layers.items():
        rm, rv = AR.running_stats(sv[l])
        assert rel(rm, bn.running_mean) <= 1e-12 and rel(rv, bn.running_var) <= 1e-12, (name, l)
    return masks, ref


def main():
    out = {"cases": np.array([c[0] for c in CASES]), "fusion_cases": np.array([c[0] for c in FUSION_CASES])}
    for i, (name, shape, widths) in enumerate(CASES):
        for seed in range(9300 + 1000 * i, 9300 + 1000 * i + SEEDS):
            case = AR.make_case(*shape, seed, widths)
            m32, g32, _ = AR.upstream_grads(case, torch.float32)
            m64, g64, _ = AR.upstream_grads(case)
            worst = max([rel(m32.double(), m64)] + [rel(g32[k].double(), g64[k]) for k in AR.PARAMS])
            if worst <= FP32_AGREES:
                break
        else:
            raise SystemExit("%s: no seed on which fp32 agrees with float64 to %g" % (name, FP32_AGREES))
        masks, ref = pinned(case, name)
        out["%s_seed" % name] = np.array(seed)
        out["%s_shape" % name] = np.array(shape)
        out["%s_widths" % name] = np.array(widths)
        print("[%s] seed %d: fp32 CPU against float64, worst of masks and the 24 gradients %.1e" % (name, seed, worst))
        if name == "tiny":
            out["tiny_masks"] = masks.numpy()
            out.update({"tiny_d_%s" % k: ref[k].numpy() for k in AR.PARAMS})
    for i, (name, shape) in enumerate(FUSION_CASES):
        for seed in range(9700 + 1000 * i, 9700 + 1000 * i + SEEDS):
            fp = FR.make_case(*shape, seed)
            d64 = AR.fusion_dmasks_upstream(fp)
            _, g64, _ = FR.upstream_grads(fp)
            _, g32, _ = FR.upstream_grads(fp, torch.float32)
            worst = max([rel(AR.fusion_dmasks_upstream(fp, torch.float32).double(), d64)] +
                        [rel(g32[k].double(), g64[k]) for k in FR.SA_PARAMS + FR.LATERALS])
            if worst <= FP32_AGREES:
                break
        else:
            raise SystemExit("%s: no seed on which fp32 agrees with float64 to %g" % (name, FP32_AGREES))
        assert rel(AR.fusion_dmasks(fp), d64) <= 1e-12, name
        out["%s_seed" % name] = np.array(seed)
        out["%s_shape" % name] = np.array(shape)
        print("[%s] seed %d: fp32 CPU against float64, worst of dmasks and the 19 other gradients %.1e" % (name, seed, worst))
    path = os.path.join(ROOT, "tests", "golden", "adapter.npz")
    np.savez_compressed(path, **out)
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(ROOT, "tests", "golden", "readout.npz"))
    print("[golden] %s: %d bytes" % (path, size))
    if size > cap:
        raise SystemExit("adapter.npz (%d bytes) is larger than readout.npz (%d)" % (size, cap))


if __name__ == "__main__":
    main()
