#!/usr/bin/env python3
"""One fused X3D a+b launch per stage shape (batch 8), timed as a hipGraph of 20 dependent launches, against the thin GEMM +
depthwise pair it replaces: the stride-1 blocks (x3d_block.hip) and the first, stride-2 block of stages 2 and 3 (x3d_head.hip).
MSPI_X3D_DBG: 1 no GEMM phase, 2 no depthwise phase, 4 no x loads.  MSPI_X3D_TSEG: frames per T segment.
X3D_AB_SHAPES=s2 (or s1, stem): only the stride-2 (stride-1) shapes (the stem: 3 -> 24 from 224 x 224, the fused launch and the
single (5,3,3) conv it could also be, against the pair of launches)."""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mspi_amd import engine as E
from mspi_amd.module import to_cl

dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
SHAPES = [(24, 54, 56, 1), (48, 108, 28, 1), (96, 216, 14, 1), (192, 432, 7, 1), (24, 54, 112, 2), (24, 108, 56, 2)]
only = os.environ.get("X3D_AB_SHAPES", "")
for (Cin, Cmid, HW, stride) in SHAPES:
    if only and only != "s%d" % stride:
        continue
    x = to_cl(torch.randn(8, Cin, 16, HW, HW, generator=g).to(dev))
    wa = torch.randn(Cmid, Cin, 1, 1, 1, generator=g) / math.sqrt(Cin)
    wb = torch.randn(Cmid, 1, 3, 3, 3, generator=g) / math.sqrt(27)
    pa = E.pack_conv(wa, torch.randn(Cmid, generator=g), act=E.ACT_RELU, cin_stored=x.Cs, device=dev)
    pb = E.pack_dwconv(wb, torch.randn(Cmid, generator=g), None, (1, stride, stride), (1, 1, 1), E.ACT_SWISH, device=dev)
    pk = E.pack_x3d_ab(pa, pb) if stride == 1 else E.pack_x3d_ab_s2(pa, pb)
    fused = E.x3d_ab if stride == 1 else E.x3d_ab_s2
    def run():
        for _ in range(20):
            fused(x, pk)
    def run_unfused():
        for _ in range(20):
            E.dwconv(E.conv(x, pa), pb)
    res = []
    for fn in (run, run_unfused):
        fn(); torch.cuda.synchronize()
        s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            fn()
        gr.replay(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            gr.replay()
        e1.record(); torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / 100 * 1e3)
    out_hw = HW // stride
    must = 4.0 * 8 * 16 * (HW * HW * x.Cs + out_hw * out_hw * E.rup4(Cmid))      # x once in, u once out
    print("Cin %3d Cmid %3d %3dx%3d stride %d: fused %6.1f us (%.2f TB/s of the %.0f MB it must move)   unfused a + b %6.1f us   (dbg=%s tseg=%s)" % (
        Cin, Cmid, HW, HW, stride, res[0], must / res[0] * 1e-6, must * 1e-6, res[1],
        os.environ.get("MSPI_X3D_DBG", "0"), os.environ.get("MSPI_X3D_TSEG", "auto")), flush=True)


def graph_time(fn, reps=20):
    """us per call of fn, from a hipGraph of `reps` calls replayed five times."""
    fn(); torch.cuda.synchronize()
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        for _ in range(reps):
            fn()
    gr.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        gr.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (5 * reps) * 1e3


if only in ("", "stem"):
    # The X3D stem, 3 -> 24 from 224 x 224 (batch 8): conv_xy (1,3,3)/s2 + temporal depthwise (5,1,1) + BN + ReLU as the two
    # launches X3DStem.run makes, against the SAME map as one (5,3,3) conv (conv_xy has no bias and nothing non-linear follows
    # it, so w[c,ci,kt,kh,kw] = wt[c,kt] * wxy[c,ci,kh,kw], K = 135), both with the tuner's tile choice.
    clip = torch.randn(8, 3, 16, 224, 224, generator=g).to(dev)
    wxy = torch.randn(24, 3, 1, 3, 3, generator=g) / math.sqrt(27)
    wt = torch.randn(24, 1, 5, 1, 1, generator=g) / math.sqrt(5)
    bn = torch.nn.BatchNorm3d(24).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.2, 0.2); bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 1.5)
    pxy = E.pack_conv(wxy, None, None, (1, 2, 2), (0, 1, 1), E.ACT_NONE, device=dev)
    pt = E.pack_dwconv(wt, None, bn, (1, 1, 1), (2, 0, 0), E.ACT_RELU, device=dev)
    w5 = wt.view(24, 1, 5, 1, 1) * wxy.view(24, 3, 1, 3, 3)
    p5 = E.pack_conv(w5, None, bn, (1, 2, 2), (2, 1, 1), E.ACT_RELU, device=dev)
    E.autotune(True)
    a = E.dwconv(E.conv(clip, pxy), pt)
    b = E.conv(clip, p5)
    E.autotune(False)
    torch.cuda.synchronize()
    err = (a.as_ncdhw() - b.as_ncdhw()).abs().max().item()
    t_pair = graph_time(lambda: E.dwconv(E.conv(clip, pxy), pt))
    t_fold = graph_time(lambda: E.conv(clip, p5))
    pk = E.pack_x3d_stem(wxy, wt, bn)
    c = E.x3d_stem(clip, pk)
    torch.cuda.synchronize()
    err_f = (a.as_ncdhw() - c.as_ncdhw()).abs().max().item()
    t_fused = graph_time(lambda: E.x3d_stem(clip, pk))
    must = 4.0 * 8 * 16 * (3 * 224 * 224 + 24 * 112 * 112)
    print("stem 3 -> 24 from 224x224: conv_xy + temporal dw %6.1f us   fused stem %6.1f us (%.2f TB/s of the %.0f MB it must move, max |diff| %.2e)"
          "   one (5,3,3) conv, K = 135 %6.1f us (max |diff| %.2e)" % (t_pair, t_fused, must / t_fused * 1e-6, must * 1e-6, err_f, t_fold, err), flush=True)
