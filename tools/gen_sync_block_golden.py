#!/usr/bin/env python
"""Writes tests/golden/sync_block.npz for tests/test_sync_block_train.py (CPU only, float64).

Case "tiny" (B, R) = (1, 1) is stored with its float64 y and twelve gradients from torch autograd through torch.nn layers
(tests/sync_block_restate.upstream_grads).  With one row every weight gradient is the outer product of two vectors, so the six
matrices are stored as those two factors (taken from the autograd result through its largest entry and checked to reproduce
it to 1e-15 of its size): 25 MB of float64 as 100 KB, nothing lost.  Case "odd" (2, 37) is stored as its seed.
The restatement is asserted against torch autograd to 1e-12 on every seed, and what torch itself loses in fp32 is printed: the
figure the GPU tests' bar is read against."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sync_block_restate as R      # noqa: E402

CASES = {"tiny": (1, 1, 11), "odd": (2, 37, 12)}
EXTRA = {"tile": (1, 130, 13)}      # checked and printed, not stored


def factor(dW):
    """u, v with dW = outer(u, v), exact for a rank-one dW."""
    i, j = np.unravel_index(np.abs(dW).argmax(), dW.shape)
    u, v = dW[:, j] / dW[i, j], dW[i, :].copy()
    assert np.abs(np.outer(u, v) - dW).max() <= 1e-15 * np.abs(dW).max(), "not rank one"
    return u, v


def main():
    torch.manual_seed(0)
    out = {"names": np.array(sorted(CASES)), "grads": np.array(R.GRADS)}
    for name, (B, Rr, seed) in list(CASES.items()) + list(EXTRA.items()):
        case = R.make_case(B, Rr, seed)
        y64, g64 = R.upstream_grads(case, torch.float64)
        mine, y = R.backward(case), R.forward(case)["y"]
        worst = max([R.rel_err(y, y64)] + [R.rel_err(mine[k], g64[k]) for k in R.GRADS])
        assert worst <= 1e-12, (name, worst)
        y32, g32 = R.upstream_grads(case, torch.float32)
        f32 = max([R.rel_err(y32, y64)] + [R.rel_err(g32[k], g64[k]) for k in R.GRADS])
        print("%-5s (B, R) = (%d, %d) seed %d: restatement vs torch float64 %.2e, torch fp32 vs float64 %.2e" % (name, B, Rr, seed, worst, f32))
        if name not in CASES:
            continue
        out[name + ".shape"] = np.array([B, Rr, seed])
        if name == "tiny":
            out["tiny.y"] = y64.numpy()
            for k in R.GRADS:
                g = g64[k].numpy()
                if g.ndim == 2:
                    out["tiny.d%s.u" % k], out["tiny.d%s.v" % k] = factor(g)
                else:
                    out["tiny.d" + k] = g
    path = os.path.join(ROOT, "tests", "golden", "sync_block.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
