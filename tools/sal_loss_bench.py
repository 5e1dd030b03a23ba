#!/usr/bin/env python3
"""The criterion's forward and backward at the training shape (8 x 224 x 384, with fixations): HIP-event medians of 30
calls after 10 warm-ups of
  (a) mspi_saliency_loss_fwd and (b) mspi_saliency_loss_bwd, with the bytes each moves and the fraction of what a plain
      device copy of the same number of bytes reaches (the yardstick of tools/hbm_reference.py, measured here at that size);
  (c) mspi_saliency_metrics(pred_is_log = 1), the evaluation launch that computes the same four values;
  (d) torch autograd of the restated formulas on the same device, forward plus backward: what a user writes without (a), (b).
Measurement only; run from the repository root:  python tools/sal_loss_bench.py [B H W]"""
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sal_loss_restate as S  # noqa: E402
from mspi_amd import _lib  # noqa: E402

WARMUP, RUNS = 10, 30


def median_us(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    B, H, W = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (8, 224, 384)
    dev = torch.device("cuda")
    lib = _lib.load()
    L = H * W
    x, g, f = (torch.from_numpy(a).to(dev) for a in S.make_case(B, H, W, 3))
    terms = torch.empty(B, 4, device=dev)
    ws = torch.empty(lib.mspi_saliency_loss_ws_bytes(B, L), dtype=torch.uint8, device=dev)
    dlog = torch.empty_like(x)
    out = torch.empty(B, 4, device=dev)
    one = torch.ones((), device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd():
        _lib.check(lib.mspi_saliency_loss_fwd(x.data_ptr(), g.data_ptr(), f.data_ptr(), terms.data_ptr(), ws.data_ptr(), B, L, st), "fwd")

    def bwd():
        _lib.check(lib.mspi_saliency_loss_bwd(x.data_ptr(), g.data_ptr(), f.data_ptr(), ws.data_ptr(), one.data_ptr(), 1 / B, 1 / B,
                                              0.1 / B, dlog.data_ptr(), B, L, st), "bwd")

    def metrics():
        _lib.check(lib.mspi_saliency_metrics(x.data_ptr(), g.data_ptr(), f.data_ptr(), out.data_ptr(), B, L, 1, st), "metrics")

    xt = x.clone().requires_grad_(True)

    def torch_autograd():
        xt.grad = None
        S.loss(xt, g, f, dtype=torch.float32).backward()

    def copy_rate(nbytes):
        """GB/s (read + write) of a device copy that moves nbytes in all."""
        n = nbytes // 8
        a, b = torch.empty(n, device=dev).normal_(), torch.empty(n, device=dev)
        us = median_us(lambda: b.copy_(a))[0]
        return 2.0 * n * 4 / us / 1e3, us

    fwd_bytes = B * L * (12 + 8) + ws.numel()            # pass one reads three maps, pass two two; partials are noise
    bwd_bytes = B * L * 16                               # three maps read, one written
    print("saliency loss at %d x %d x %d with fixations, medians of %d after %d warm-ups (min .. max), %s" % (
        B, H, W, RUNS, WARMUP, torch.cuda.get_device_name(0)))
    rows = (("(a) mspi_saliency_loss_fwd (3 launches)", fwd, fwd_bytes), ("(b) mspi_saliency_loss_bwd (1 launch)", bwd, bwd_bytes),
            ("(c) mspi_saliency_metrics, pred_is_log", metrics, None), ("(d) torch autograd of the restated formulas", torch_autograd, None))
    res = {}
    for name, fn, nbytes in rows:
        med, lo, hi = median_us(fn)
        res[name[:3]] = med
        line = "%-46s %8.1f us  (%.1f .. %.1f)" % (name, med, lo, hi)
        if nbytes:
            rate, cus = copy_rate(nbytes)
            line += "  %.2f MB moved, %.0f GB/s = %.2f of a copy of as many bytes (%.0f GB/s, %.1f us)" % (
                nbytes / 1e6, nbytes / med / 1e3, nbytes / med / 1e3 / rate, rate, cus)
        print(line)
    torch.cuda.synchronize()
    ref = S.terms(x.cpu(), g.cpu(), f.cpu())
    print("terms: max rel err vs float64  chunked %.2e  one-workgroup %.2e" % tuple(
        ((t.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-3)).max().item() for t in (terms, out)))
    print("(a) / (c) = %.2f   ((a) + (b)) / (d) = %.3f" % (res["(a)"] / res["(c)"], (res["(a)"] + res["(b)"]) / res["(d)"]))


if __name__ == "__main__":
    main()
