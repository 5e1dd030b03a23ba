"""Writes tests/golden/saliency_loss.npz: small log maps, densities and fixation maps, the four per-sample terms of the
REFERENCE's own kldiv / cc / similarity / nss (utils/compute_saliency_metrics.py:9-108) in float64, and the gradients
that autograd gives through them for the two losses of utils/loss.py:26-49, kl - cc and kl - cc - 0.1 nss.  Asserts
tests/sal_loss_restate.py (terms and analytic gradient) against both on the way.  Needs the reference checkout
(oracle.ref_harness); run from the repository root:

    python tools/gen_loss_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness as rh  # noqa: E402
from oracle import restate as R  # noqa: E402
import sal_loss_restate as S  # noqa: E402

CASES = (("tiny", 1, 5, 7), ("odd", 3, 33, 31), ("quad", 2, 40, 52))


def _reference():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))       # imported at the top of the file, used by a resize only
    cwd = os.getcwd()
    rh.enter_reference()
    from utils import compute_saliency_metrics as M
    os.chdir(cwd)
    return M


def main():
    M = _reference()
    out = {"cases": np.array([c[0] for c in CASES])}
    for i, (name, B, H, W) in enumerate(CASES):
        log_map, dens, fix = S.make_case(B, H, W, 7100 + i)
        x = torch.from_numpy(log_map).double().requires_grad_(True)
        g, f = torch.from_numpy(dens).double(), torch.from_numpy(fix).double()
        # per-sample terms: the reference's functions return batch means, so one sample at a time
        terms = torch.stack([torch.stack([M.kldiv(x[b:b + 1].exp(), g[b:b + 1]), M.cc(x[b:b + 1].exp(), g[b:b + 1]),
                                          M.similarity(x[b:b + 1].exp(), g[b:b + 1]), M.nss(x[b:b + 1].exp(), f[b:b + 1])])
                             for b in range(B)]).detach()
        loss2 = M.kldiv(x.exp(), g) - M.cc(x.exp(), g)                                   # utils/loss.py:32
        loss3 = M.kldiv(x.exp(), g) - M.cc(x.exp(), g) - 0.1 * M.nss(x.exp(), f)         # utils/loss.py:40
        grad2, = torch.autograd.grad(loss2, x)
        grad3, = torch.autograd.grad(loss3, x)
        xd = x.detach()
        t = S.terms(xd, g, f)
        assert (t - terms).abs().max().item() <= 1e-12, (name, (t - terms).abs().max().item())
        assert abs(S.loss(xd, g).item() - loss2.item()) <= 1e-12 and abs(S.loss(xd, g, f).item() - loss3.item()) <= 1e-12
        for ref, got in ((grad2, S.loss_grad(xd, g)), (grad3, S.loss_grad(xd, g, f))):
            err = ((got - ref).flatten(1).abs().max(1)[0] / ref.flatten(1).abs().max(1)[0]).max().item()
            assert err <= 1e-12, (name, err)
            print("[%s] analytic gradient vs autograd of the reference: %.1e of the largest entry" % (name, err))
        t32 = S.terms(torch.from_numpy(log_map), torch.from_numpy(dens), torch.from_numpy(fix), dtype=torch.float32)
        assert torch.equal(t32, R.saliency_metrics(torch.from_numpy(log_map).exp(), torch.from_numpy(dens), torch.from_numpy(fix)))
        print("[%s] %dx%dx%d  loss %.9f / %.9f  fixations %s" % (name, B, H, W, loss2.item(), loss3.item(),
                                                                 fix.reshape(B, -1).sum(1).astype(int).tolist()))
        out.update({"%s_log_map" % name: log_map, "%s_density" % name: dens, "%s_fix" % name: fix.astype(np.uint8),
                    "%s_terms" % name: terms.numpy(), "%s_loss" % name: np.array([loss2.item(), loss3.item()]),
                    "%s_grad" % name: grad2.numpy(), "%s_grad_fix" % name: grad3.numpy()})
    path = os.path.join(ROOT, "tests", "golden", "saliency_loss.npz")
    np.savez_compressed(path, **out)
    print("[golden] %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
