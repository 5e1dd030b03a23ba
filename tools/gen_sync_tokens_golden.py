#!/usr/bin/env python
"""Writes tests/golden/sync_tokens.npz for tests/test_sync_tokens_train.py (CPU only, float64).

Case "tiny" -- B = 1, one visual and one audio token, C4 = 192 -- is stored with what torch autograd gives in float64 through
nn.Linear / nn.LayerNorm with upstream's arguments, the sinusoid tables and the three torch.nn Blocks of
tests/sync_block_restate.build_upstream (tests/sync_tokens_restate.upstream_grads): the embedding's slab, the output y of the
three blocks, and the embedding's eight gradients twice -- of <slab, G> ("tiny.e.*", the embedding alone, what SyncEmbed is held
to) and of <y, G> ("tiny.d.*", through the three blocks).  With one visual token dW_proj is the outer product of two vectors and
is stored as those two factors (checked to reproduce it to 1e-15 of its size).  Case "odd" -- B = 2, vis 1x3x2, aud 1x1x5,
C4 = 784 -- is stored as its seed.
The restatement is asserted against torch autograd to 1e-12 on both cases, and what torch itself loses in fp32 is printed: the
figure the GPU tests' bar is read against."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sync_block_restate as SR      # noqa: E402
import sync_tokens_restate as TR      # noqa: E402

# name: (B, vis (t, h, w), aud (F, T'), C4, seed)
CASES = {"tiny": (1, (1, 1, 1), (1, 1), 192, 31), "odd": (2, (1, 3, 2), (1, 5), 784, 32)}


def factor(dW):
    """u, v with dW = outer(u, v), exact for a rank-one dW."""
    i, j = np.unravel_index(np.abs(dW).argmax(), dW.shape)
    u, v = dW[:, j] / dW[i, j], dW[i, :].copy()
    assert np.abs(np.outer(u, v) - dW).max() <= 1e-15 * np.abs(dW).max(), "not rank one"
    return u, v


def main():
    torch.manual_seed(0)
    out = {"names": np.array(sorted(CASES)), "grads": np.array(TR.EMBED_GRADS)}
    for name, (B, thw, ft, C4, seed) in CASES.items():
        case = TR.make_case(B, thw, ft, C4, seed)
        y64, e64, b64 = TR.upstream_grads(case)
        s64, a64, _ = TR.upstream_grads(case, blocks=False)
        slab, y = TR.forward(case)
        my_y, mine, mine_b = TR.backward(case)
        alone = TR.embed_backward(case)
        errs = [SR.rel_err(slab, s64), SR.rel_err(y, y64), SR.rel_err(my_y, y64)]
        errs += [SR.rel_err(mine[k], e64[k]) for k in TR.EMBED_GRADS] + [SR.rel_err(alone[k], a64[k]) for k in TR.EMBED_GRADS]
        errs += [SR.rel_err(mine_b[i][k], b64[i][k]) for i in range(TR.NBLOCKS) for k in SR.NAMES]
        assert max(errs) <= 1e-12, (name, max(errs))
        y32, e32, b32 = TR.upstream_grads(case, dtype=torch.float32)
        f32 = max([SR.rel_err(y32, y64)] + [SR.rel_err(e32[k], e64[k]) for k in TR.EMBED_GRADS] +
                  [SR.rel_err(b32[i][k], b64[i][k]) for i in range(TR.NBLOCKS) for k in SR.NAMES])
        print("%-5s B = %d, vis %s, aud %s, C4 = %d, seed %d: restatement vs torch float64 %.2e, torch fp32 vs float64 %.2e"
              % (name, B, thw, ft, C4, seed, max(errs), f32))
        out[name + ".shape"] = np.array([B, *thw, *ft, C4, seed])
        if name == "tiny":
            out["tiny.slab"], out["tiny.y"] = s64.numpy(), y64.numpy()
            for tag, grads in (("e", a64), ("d", e64)):
                for k in TR.EMBED_GRADS:
                    g = grads[k].numpy()
                    if k == "wp":
                        out["tiny.%s.wp.u" % tag], out["tiny.%s.wp.v" % tag] = factor(g)
                    else:
                        out["tiny.%s.%s" % (tag, k)] = g
    path = os.path.join(ROOT, "tests", "golden", "sync_tokens.npz")
    np.savez_compressed(path, **out)
    ref = os.path.join(ROOT, "tests", "golden", "sync_block.npz")
    print("wrote %s, %d bytes (sync_block.npz: %d)" % (path, os.path.getsize(path), os.path.getsize(ref)))
    assert os.path.getsize(path) <= os.path.getsize(ref)


if __name__ == "__main__":
    main()
