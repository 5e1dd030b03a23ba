"""Writes tests/golden/readout_tail.npz: fp32 inputs and parameters of the decoder's readout tail and, in float64, the
value and the seven gradients that torch autograd gives through UPSTREAM's order of the tail, built from torch.nn layers
with the arguments of model/model_utils.py:403-409: trilinear Upsample (1,4,4), Conv3d(64,32,(4,1,1),(4,1,1)), ReLU,
Conv3d(32,32,(1,3,3)), ReLU, Conv3d(32,1,(1,3,3)), then x - logsumexp(x).  Asserts tests/readout_tail_restate.py (this
project's order, conv then up-sample, with its analytic backward) against it to 1e-12 on the way.  Run from the
repository root:

    python tools/gen_readout_tail_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import readout_tail_restate as T  # noqa: E402

CASES = (("tiny", 1, 2, 3), ("odd", 2, 5, 7))
KINK_FREE = {"tiny": 1e-4}        # smallest |pre-activation| asked of the case's seed (none exists on the larger case)


def upstream_tail(p):
    tail = nn.Sequential(
        nn.Upsample(scale_factor=(1, 4, 4), mode="trilinear", align_corners=False),
        nn.Conv3d(64, 32, kernel_size=(4, 1, 1), stride=(4, 1, 1), padding=0),
        nn.ReLU(inplace=True),
        nn.Conv3d(32, 32, kernel_size=(1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1)),
        nn.ReLU(inplace=True),
        nn.Conv3d(32, 1, kernel_size=(1, 3, 3), stride=(1, 1, 1), padding=(0, 1, 1)),
    ).double()
    with torch.no_grad():
        for i, k in ((1, "8"), (3, "10"), (5, "12")):
            tail[i].weight.copy_(torch.from_numpy(p["w" + k]).double())
            tail[i].bias.copy_(torch.from_numpy(p["b" + k]).double())
    return tail


def rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def main():
    out = {"cases": np.array([c[0] for c in CASES])}
    for i, (name, B, h, w) in enumerate(CASES):
        for seed in range(8200 + 100 * i, 8200 + 100 * i + 40):
            case = T.make_case(B, h, w, seed)
            saved = T.forward(case["y4"], case)
            if T.min_preactivation(saved) >= KINK_FREE.get(name, 0.0):
                break
        else:
            raise SystemExit("%s: no seed with |pre-activation| >= %g" % (name, KINK_FREE[name]))
        tail = upstream_tail(case)
        y4 = torch.from_numpy(case["y4"]).double().requires_grad_(True)
        g = torch.from_numpy(case["g"]).double()
        z = tail(y4)[:, 0, 0]
        ref_out = z - torch.logsumexp(z.flatten(1), 1).view(-1, 1, 1)
        names = ("y4",) + T.PARAMS
        leaves = [y4] + [getattr(tail[j], a) for j in (1, 3, 5) for a in ("weight", "bias")]
        ref = dict(zip(names, torch.autograd.grad((ref_out * g).sum(), leaves)))
        grads = T.backward(case["y4"], case, saved, case["g"])
        assert (saved["out"] - ref_out).abs().max().item() <= 1e-12, name
        gsum = g.abs().sum().item()
        for k in names:
            err = (grads[k] - ref[k]).abs().max().item() / gsum if k == "b12" else rel(grads[k], ref[k])
            assert err <= 1e-12, (name, k, err)
        print("[%s] seed %d, (B, h, w) = %s: smallest |pre-activation| %.1e, zero share of y4 %.2f, |d b12| / sum|g| = %.1e"
              % (name, seed, (B, h, w), T.min_preactivation(saved), float((case["y4"] == 0).mean()),
                 ref["b12"].abs().item() / gsum))
        out.update({"%s_%s" % (name, k): v for k, v in case.items()})
        out["%s_out" % name] = ref_out.detach().numpy()
        out.update({"%s_d_%s" % (name, k): ref[k].numpy() for k in names})
    path = os.path.join(ROOT, "tests", "golden", "readout_tail.npz")
    np.savez_compressed(path, **out)
    print("[golden] %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
