#!/usr/bin/env python
"""Writes tests/golden/contrast_head.npz for tests/test_sync_train.py (CPU only, float64).

Case "tiny" -- B = 1, one visual and one audio token -- is stored with what torch autograd gives in float64 through torch.nn
layers built with upstream's arguments (tests/contrast_restate.upstream_grads): loss_av, the slab's gradient and the 36
tensors' gradients.  With one row a Linear's dW is the outer product of its db and its input row, so each is stored as those two
factors (db under its own name, the row as "tiny.<side>.w<i>.v"; checked to reproduce dW to 1e-15 of its size).  Case "odd" -- B = 2,
6 visual and 5 audio tokens -- is stored as its seed.
The restatement is asserted against torch autograd to 1e-12 on both cases, and what torch itself loses in fp32 is printed: the
figure the GPU tests' bar is read against."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contrast_restate as CR      # noqa: E402

# name: (B, Rv, Ra, seed)
CASES = {"tiny": (1, 1, 1, 41), "odd": (2, 6, 5, 42)}


def factor(dW, db):
    """v with dW = outer(db, v), exact for the dW of one row."""
    i = np.abs(db).argmax()
    v = dW[i, :] / db[i]
    assert np.abs(np.outer(db, v) - dW).max() <= 1e-15 * np.abs(dW).max(), "not the outer product of db and a row"
    return v


def main():
    torch.manual_seed(0)
    out = {"names": np.array(sorted(CASES)), "grads": np.array(("slab",) + CR.NAMES)}
    for name, (B, Rv, Ra, seed) in CASES.items():
        case = CR.make_case(B, Rv, Ra, seed)
        l64, g64 = CR.upstream_grads(case)
        loss, mine = CR.backward(case)
        errs = [abs(loss.item() - l64.item()) / abs(l64.item())] + [CR.rel_err(mine[k], g64[k]) for k in g64]
        assert max(errs) <= 1e-12, (name, max(errs))
        l32, g32 = CR.upstream_grads(case, dtype=torch.float32)
        f32 = max([abs(l32.item() - l64.item()) / abs(l64.item())] + [CR.rel_err(g32[k], g64[k]) for k in g64])
        print("%-5s B = %d, Rv = %d, Ra = %d, seed %d: restatement vs torch float64 %.2e, torch fp32 vs float64 %.2e"
              % (name, B, Rv, Ra, seed, max(errs), f32))
        out[name + ".shape"] = np.array([B, Rv, Ra, seed])
        if name == "tiny":
            out["tiny.loss"], out["tiny.slab"] = l64.numpy(), g64["slab"].numpy()
            for k in CR.NAMES:
                g = g64[k].numpy()
                if g.ndim == 2:
                    out["tiny.%s.v" % k] = factor(g, g64[k.replace(".w", ".b")].numpy())
                else:
                    out["tiny.%s" % k] = g
    path = os.path.join(ROOT, "tests", "golden", "contrast_head.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
