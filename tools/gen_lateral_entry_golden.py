"""Writes tests/golden/lateral_entry.npz: for the laterals' entry conv(s), in float64, the output y and the gradients of <y, G>
with respect to latlayer_k[0].weight, latlayer_k[0].bias and latlayer_k[1].weight as torch autograd gives them through
nn.Conv3d(C, 192, 1) followed by nn.Conv3d(192, 192, (s,1,1), (s,1,1), bias=False) (model/model_utils.py:440-470 upstream).
Asserts tests/lateral_entry_restate.py (this project's order: compose, one conv, the chain rule through the composition)
against it to 1e-12 on the way, for every case.

The fp32 inputs are not stored: lateral_entry_restate.make_case rebuilds them from the stored seed (numpy's RandomState stream
is frozen).  "tiny" is stored with its float64 results, every other case as its seed and geometry alone.  The stored "tiny"
is TINY_MID = 32 channels wide behind the first conv, not 192: at 192 the float64 gradient of latlayer_k[1].weight alone is
590 KB, eight times lateral_block.npz, which this file must not outgrow; 32 is the narrowest output the kernel takes.  Every
case, "tiny" included, is also checked at 192 here and stored as its seed.  The layers have no
nonlinearity, so there is no kink to steer the seeds around; how far torch FLOAT32 on the CPU is from float64 on each case is
printed.  Torch only.  Run from the repository root:

    python tools/gen_lateral_entry_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lateral_entry_restate as ER  # noqa: E402

# name, (B, T, h, w), C (the two inputs' widths summed), s, second conv, seed
CASES = (("tiny", (1, 2, 1, 2), 24, 2, True, 9600), ("odd", (2, 6, 5, 3), 24, 2, True, 9601), ("tail", (1, 5, 3, 3), 48, 2, True, 9602),
         ("s4", (1, 8, 7, 12), 48, 4, True, 9603), ("ragged112", (1, 4, 3, 5), 112, 2, True, 9604),
         ("ragged44", (1, 4, 3, 5), 44, 2, True, 9605), ("split", (2, 4, 2, 3), 192 + 512, 4, True, 9606),
         ("plain", (1, 2, 3, 5), 320, 1, False, 9607), ("widest", (1, 1, 2, 2), 2048 + 512, 1, False, 9608),
         ("slice", (1, 2, 4, 4), 32, 2, True, 9609))


TINY_MID = 32


def rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def main():
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, shape, C, s, second, seed in CASES:
        case = ER.make_case(*shape, C, s, seed, second)
        y, ref = ER.upstream_grads(case)
        grads = ER.backward(case)
        assert rel(ER.forward(case), y) <= 1e-12, name
        for k in ref:
            assert rel(grads[k], ref[k]) <= 1e-12, (name, k, rel(grads[k], ref[k]))
        y32, g32 = ER.upstream_grads(case, torch.float32)
        worst = max([rel(y32.double(), y)] + [rel(g32[k].double(), ref[k]) for k in ref])
        print("[%s] seed %d: fp32 CPU against float64, worst of the %d tensors %.1e" % (name, seed, 1 + len(ref), worst))
        out["%s_seed" % name] = np.array(seed)
        out["%s_geom" % name] = np.array(list(shape) + [C, s, int(second)])
        if name == "tiny":
            case = ER.make_case(*shape, C, s, seed, second, mid=TINY_MID)
            y, ref = ER.upstream_grads(case)
            grads = ER.backward(case)
            for k in ref:
                assert rel(grads[k], ref[k]) <= 1e-12, (name, k, rel(grads[k], ref[k]))
            out["tiny_mid"] = np.array(TINY_MID)
            out["tiny_y"] = y.numpy()
            out.update({"tiny_d_%s" % k: ref[k].numpy() for k in ref})
    path = os.path.join(ROOT, "tests", "golden", "lateral_entry.npz")
    np.savez_compressed(path, **out)
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(ROOT, "tests", "golden", "lateral_block.npz"))
    print("[golden] %s: %d bytes" % (path, size))
    if size > cap:
        raise SystemExit("lateral_entry.npz (%d bytes) is larger than lateral_block.npz (%d)" % (size, cap))


if __name__ == "__main__":
    main()
