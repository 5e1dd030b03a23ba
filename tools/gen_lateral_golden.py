"""Writes tests/golden/lateral_block.npz: for the ConvNextBlock at the end of each lateral, in float64, the output y and the
11 gradients of <y, G> (x and the block's ten tensors) as torch autograd gives them through torch.nn layers built with
upstream's arguments (model/model_utils.py:306-354: Conv3d(groups=dim) (7,1,1) then (1,7,7), nn.LayerNorm(dim) with eps 1e-5,
exact nn.GELU, two 1x1x1 convs, the residual).  Asserts tests/lateral_restate.py (this project's order, analytic backward in
autograd.LateralBlock's launch sequence) against it to 1e-12 on the way, for "tiny" (B, T, h, w) = (1, 1, 1, 2) and for "odd"
(2, 3, 5, 3), both at D = 32.

The fp32 inputs are not stored: lateral_restate.make_case rebuilds them from the stored seed (numpy's RandomState stream is
frozen).  "tiny" is stored with its float64 results, "odd" as its seed alone.  The block has no ReLU, so there is no kink to
steer the seeds around; how far torch FLOAT32 on the CPU is from float64 on each seed is printed.  Run from the repository root:

    python tools/gen_lateral_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lateral_restate as LR  # noqa: E402

CASES = (("tiny", 1, 1, 1, 2, 9300), ("odd", 2, 3, 5, 3, 9400))


def rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def main():
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, B, T, h, w, seed in CASES:
        case = LR.make_case(B, T, h, w, seed)
        sv = LR.forward(case)
        grads = LR.backward(case, sv, case["G"])
        y, ref = LR.upstream_grads(case)
        assert (sv["y"] - y).abs().max().item() <= 1e-12, name
        for k in LR.NAMES:
            assert rel(grads[k], ref[k]) <= 1e-12, (name, k, rel(grads[k], ref[k]))
        y32, g32 = LR.upstream_grads(case, torch.float32)
        worst = max([rel(y32.double(), y)] + [rel(g32[k].double(), ref[k]) for k in LR.NAMES])
        print("[%s] seed %d: fp32 CPU against float64, worst of the 12 tensors %.1e" % (name, seed, worst))
        out["%s_seed" % name] = np.array(seed)
        out["%s_shape" % name] = np.array([B, T, h, w])
        if name == "tiny":
            out["tiny_y"] = y.numpy()
            out.update({"tiny_d_%s" % k: ref[k].numpy() for k in LR.NAMES})
    path = os.path.join(ROOT, "tests", "golden", "lateral_block.npz")
    np.savez_compressed(path, **out)
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(ROOT, "tests", "golden", "fusion.npz"))
    print("[golden] %s: %d bytes" % (path, size))
    if size > cap:
        raise SystemExit("lateral_block.npz (%d bytes) is larger than fusion.npz (%d)" % (size, cap))


if __name__ == "__main__":
    main()
