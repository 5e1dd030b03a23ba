#!/usr/bin/env python
"""Writes tests/golden/x3d_block.npz for tests/test_x3d_block_train.py (CPU only, float64).

Case "tiny" -- (dim_out, dim_inner) = (32, 72) at B,T,h,w = 1,2,2,2 with `se` -- is stored with what torch autograd gives in
float64 through torch.nn layers built with upstream's arguments (tests/x3d_block_restate.upstream_grads): y, dx and the 13
tensors' gradients.  The other cases are stored as their shapes and seeds.
The restatement is asserted against torch autograd in float64 to 1e-12 on every case, what torch itself loses in fp32 is
printed per case -- the figure the GPU tests' bar GRAD_TOL = 2e-5 is read against -- and asserted to stay below GRAD_TOL / 5: a
case that does not has inputs too ill-conditioned for the bar and is replaced, the bar is not loosened."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import x3d_block_restate as XR      # noqa: E402

GRAD_TOL = 2e-5                     # tests/test_readout_train.py
# name: (dim_out, dim_inner, B, T, h, w, se, seed); chain0..2: the three blocks tests chain through autograd.x3d_blocks
CASES = {
    "tiny": (32, 72, 1, 2, 2, 2, 1, 61),
    "odd_se": (32, 72, 2, 3, 5, 7, 1, 62),
    "odd": (32, 72, 2, 3, 5, 7, 0, 63),
    "s4": (96, 216, 1, 2, 3, 4, 1, 64),
    "s5": (192, 432, 1, 2, 3, 4, 0, 65),
    "s5_map": (192, 432, 1, 16, 7, 12, 1, 66),
    "chain0": (32, 72, 2, 2, 3, 5, 1, 67),
    "chain1": (32, 72, 2, 2, 3, 5, 0, 68),
    "chain2": (32, 72, 2, 2, 3, 5, 1, 69),
}


def main():
    torch.manual_seed(0)
    out = {"names": np.array(sorted(CASES)), "grads": np.array(XR.GRADS)}
    for name, spec in CASES.items():
        case = XR.make_case(*spec[:6], bool(spec[6]), spec[7])
        y64, g64 = XR.upstream_grads(case)
        fwd = XR.forward(case)
        mine = XR.backward(case, fwd)
        assert sorted(mine) == sorted(g64), (sorted(mine), sorted(g64))
        errs = {"y": XR.rel_err(fwd["y"], y64)}
        errs.update({k: XR.rel_err(mine[k], g64[k]) for k in g64})
        assert max(errs.values()) <= 1e-12, (name, errs)
        y32, g32 = XR.upstream_grads(case, dtype=torch.float32)
        f32 = {"y": XR.rel_err(y32, y64)}
        f32.update({k: XR.rel_err(g32[k], g64[k]) for k in g64})
        worst = max(f32, key=f32.get)
        small = min(float(g64[k].abs().max()) for k in g64)
        print("%-7s %s: restatement vs torch float64 %.2e, torch fp32 vs float64 %.2e (%s), smallest max|ref| %.2e"
              % (name, spec, max(errs.values()), f32[worst], worst, small))
        assert f32[worst] < GRAD_TOL / 5, (name, worst, f32[worst])
        out[name + ".shape"] = np.array(spec)
        if name == "tiny":
            out["tiny.y"] = y64.numpy()
            for k in XR.GRADS:
                out["tiny." + k] = g64[k].numpy()
    path = os.path.join(ROOT, "tests", "golden", "x3d_block.npz")
    np.savez_compressed(path, **out)
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(ROOT, "tests", "golden", "fusion.npz"))
    print("wrote %s, %d bytes (fusion.npz: %d)" % (path, size, cap))
    assert size <= cap


if __name__ == "__main__":
    main()
