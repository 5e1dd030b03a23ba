"""The head end of the X3D path: mspi_x3d_ab_s2_fwd, the first block of a stage (`a` 1x1x1 + ReLU, then the channel-wise
3x3x3 conv at spatial stride 2) in one launch (csrc/x3d_head.hip).  Reference: float64 torch on the CPU.  The bar is the one
test_ops_gpu.py::test_x3d_ab_fused holds the stride-1 kernel to (2e-5 of max(1, max|ref|)): the arithmetic is the same, an
f16x3 GEMM with K <= 96 followed by 27 fp32 FMAs.  The host-side tests (symbols, supported / variant answers, argument
rejection) need no GPU.  Second half: mspi_x3d_stem_fwd, the X3D stem (conv_xy + temporal depthwise conv + BN + ReLU) as one
launch of fp32 FMAs."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

TOL = 2e-5
SENTINEL = -777.25


def _close(got, ref, tol, what=""):
    err = (got.cpu() - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    print("%s: max abs err %.3e (scale %.2f, bar %.1e)" % (what, err, scale, tol * scale))
    assert err <= tol * scale, "%s: max abs err %.3e (scale %.2f)" % (what, err, scale)


def _desc(N, T, H, W, Cin, Cmid, act=0, scale=1.0, ldx=None, ldu=None):
    from mspi_amd import _lib as L
    d = L.X3dAbS2Desc()
    d.N, d.T, d.H, d.W, d.Cin, d.Cmid = N, T, H, W, Cin, Cmid
    d.ldx, d.ldu, d.act, d.wa_scale = Cin if ldx is None else ldx, Cmid if ldu is None else ldu, act, scale
    return d


# ----------------------------------------------------------------------------- host only

def test_s2_symbols_declared_exported_bound():
    import os
    import re
    from mspi_amd import _lib as L
    names = {"mspi_x3d_ab_s2_supported", "mspi_x3d_ab_s2_pool_rows", "mspi_x3d_ab_s2_variant", "mspi_x3d_ab_s2_fwd"}
    assert names <= set(L.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mspi_hip.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(mspi_[a-z0-9_]+)\s*\(", hdr)) and "MspiX3dAbS2Desc" in hdr
    lib = L.load()
    for n in names:
        assert getattr(lib, n).argtypes is not None
    assert lib.mspi_version() == 2
    # the stride-1 descriptor is untouched: the new one is a type of its own with the same layout
    assert C.sizeof(L.X3dAbS2Desc) == C.sizeof(L.X3dAbDesc) == 48


def test_s2_supported_and_variant_answers():
    from mspi_amd import _lib as L
    lib = L.load()
    sup = lambda *a: lib.mspi_x3d_ab_s2_supported(C.byref(_desc(*a)))
    var = lambda *a: lib.mspi_x3d_ab_s2_variant(C.byref(_desc(*a)))
    # production: X3D-L stage 2 and stage 3, first block, batch 8
    assert sup(8, 16, 112, 112, 24, 56) == 1 and var(8, 16, 112, 112, 24, 56) == 17071
    assert sup(8, 16, 56, 56, 24, 108) == 1 and var(8, 16, 56, 56, 24, 108) == 17071
    assert lib.mspi_x3d_ab_s2_pool_rows(C.byref(_desc(8, 16, 112, 112, 24, 56))) == 64          # 8 x 8 tiles, one T segment
    assert var(1, 4, 14, 28, 48, 108) == 27071 and var(1, 4, 14, 28, 96, 216) == 37071
    # refused: odd extent, an output that 7 does not divide, K > 96, channel counts off the 8 / 4 grid, no frames
    for bad in ((1, 4, 15, 28, 24, 56), (1, 4, 28, 15, 24, 56), (1, 4, 16, 28, 24, 56), (1, 4, 28, 20, 24, 56),
                (1, 4, 14, 14, 104, 56), (1, 4, 14, 14, 192, 432), (1, 4, 14, 14, 20, 56), (1, 4, 14, 14, 24, 54),
                (1, 0, 14, 14, 24, 56), (1, 4, 0, 14, 24, 56)):
        assert sup(*bad) == 0, bad
        assert lib.mspi_x3d_ab_s2_pool_rows(C.byref(_desc(*bad))) == 0
        assert var(*bad) == -1 and b"outside" in lib.mspi_last_error()
    assert lib.mspi_x3d_ab_s2_supported(None) == 0
    # T segments: a small grid is cut along T (two frames per segment at the least), a full one is not
    assert lib.mspi_x3d_ab_s2_pool_rows(C.byref(_desc(1, 16, 14, 28, 24, 56))) == 2 * 8


def test_s2_host_rejects_bad_arguments():
    from mspi_amd import _lib as L
    lib = L.load()
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)
    d = _desc(1, 2, 14, 14, 24, 56, act=L.ACT_SWISH)
    fwd = lambda dd, *a: lib.mspi_x3d_ab_s2_fwd(C.byref(dd), *a)
    assert lib.mspi_x3d_ab_s2_fwd(None, p, p, p, p, p, p, None, None) == -1 and b"null" in lib.mspi_last_error()
    for hole in range(6):
        args = [p] * 6
        args[hole] = None
        assert fwd(d, *args, None, None) == -1 and b"null" in lib.mspi_last_error()
    for (ix, what) in ((0, "x"), (1, "wa"), (3, "wb"), (4, "bias_b"), (5, "u")):
        args = [p] * 6
        args[ix] = odd
        assert fwd(d, *args, None, None) == -1 and b"alignment" in lib.mspi_last_error(), what
    assert fwd(_desc(1, 2, 15, 14, 24, 56), p, p, p, p, p, p, None, None) == -1 and b"outside" in lib.mspi_last_error()
    assert fwd(_desc(1, 2, 14, 14, 24, 56, ldx=20), p, p, p, p, p, p, None, None) == -1 and b"strides" in lib.mspi_last_error()
    assert fwd(_desc(1, 2, 14, 14, 24, 56, ldu=58), p, p, p, p, p, p, None, None) == -1 and b"strides" in lib.mspi_last_error()
    assert fwd(_desc(1, 2, 14, 14, 24, 56, act=L.ACT_RELU), p, p, p, p, p, p, None, None) == -1 and b"act" in lib.mspi_last_error()
    assert fwd(_desc(1, 2, 14, 14, 24, 56, scale=0.0), p, p, p, p, p, p, None, None) == -1 and b"wa_scale" in lib.mspi_last_error()
    assert fwd(_desc(0, 2, 14, 14, 24, 56), p, p, p, p, p, p, None, None) == -1


def test_pack_refuses_other_strides():
    from mspi_amd import engine as E
    if E.DEFAULT_PREC != E.PREC_F16X3:
        pytest.skip("the fused X3D kernel is an f16x3 kernel")
    g = torch.Generator().manual_seed(1)
    pa = E.pack_conv(torch.randn(56, 24, 1, 1, 1, generator=g), torch.randn(56, generator=g), act=E.ACT_RELU, cin_stored=24)
    wb = torch.randn(56, 1, 3, 3, 3, generator=g)
    assert E.pack_x3d_ab_s2(pa, E.pack_dwconv(wb, None, None, (1, 1, 1), (1, 1, 1))) is None
    assert E.pack_x3d_ab_s2(pa, E.pack_dwconv(wb, None, None, (2, 2, 2), (1, 1, 1))) is None
    assert E.pack_x3d_ab_s2(pa, E.pack_dwconv(wb, None, None, (1, 2, 2), (0, 1, 1))) is None
    pk = E.pack_x3d_ab_s2(pa, E.pack_dwconv(wb, None, None, (1, 2, 2), (1, 1, 1)))
    assert pk is not None and tuple(pk.wa.shape) == (2, 1, 2, 2, 64, 8)
    assert E.pack_x3d_ab(pa, E.pack_dwconv(wb, None, None, (1, 2, 2), (1, 1, 1))) is None      # the stride-1 pack still refuses it


def _stem_desc(N, T, H, W, strides=None, ldy=24):
    from mspi_amd import _lib as L
    d = L.X3dStemDesc()
    d.N, d.T, d.H, d.W = N, T, H, W
    d.sN, d.sC, d.sT, d.sH, d.sW = strides if strides is not None else (3 * T * H * W, T * H * W, H * W, W, 1)
    d.ldy = ldy
    return d


def test_stem_symbols_answers_and_rejection():
    from mspi_amd import _lib as L
    names = {"mspi_x3d_stem_supported", "mspi_x3d_stem_variant", "mspi_x3d_stem_fwd"}
    assert names <= set(L.EXPORTS)
    lib = L.load()
    sup = lambda d: lib.mspi_x3d_stem_supported(C.byref(d))
    var = lambda d: lib.mspi_x3d_stem_variant(C.byref(d))
    assert sup(_stem_desc(8, 16, 224, 224)) == 1 and var(_stem_desc(8, 16, 224, 224)) == 16     # production: one T segment
    assert sup(_stem_desc(1, 16, 28, 28)) == 1 and var(_stem_desc(1, 16, 28, 28)) == 4          # a small grid is cut along T
    assert var(_stem_desc(1, 1, 16, 20)) == 1 and var(_stem_desc(1, 3, 17, 19)) == 3
    assert sup(_stem_desc(1, 4, 28, 28, strides=(9408, 3136, 784, -28, 1))) == 0                # a flipped view
    assert sup(_stem_desc(1, 4, 28, 28, strides=(0, 0, 0, 1 << 27, 1))) == 0                    # a tap offset beyond 32 bits
    assert sup(_stem_desc(0, 4, 28, 28)) == 0 and sup(_stem_desc(1, 0, 28, 28)) == 0 and sup(_stem_desc(1, 4, 0, 28)) == 0
    assert lib.mspi_x3d_stem_supported(None) == 0
    assert var(_stem_desc(0, 4, 28, 28)) == -1 and b"outside" in lib.mspi_last_error()
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)
    d = _stem_desc(1, 2, 4, 4)
    fwd = lambda dd, *a: lib.mspi_x3d_stem_fwd(C.byref(dd), *a)
    assert lib.mspi_x3d_stem_fwd(None, p, p, p, p, p, None) == -1 and b"null" in lib.mspi_last_error()
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        assert fwd(d, *args, None) == -1 and b"null" in lib.mspi_last_error()
    assert fwd(d, p, p, p, p, odd, None) == -1 and b"aligned" in lib.mspi_last_error()
    assert fwd(d, C.c_void_p(base + 2), p, p, p, p, None) == -1 and b"aligned" in lib.mspi_last_error()
    assert fwd(_stem_desc(1, 2, 4, 4, ldy=20), p, p, p, p, p, None) == -1 and b"stride" in lib.mspi_last_error()
    assert fwd(_stem_desc(1, 2, 4, 4, ldy=26), p, p, p, p, p, None) == -1 and b"stride" in lib.mspi_last_error()
    assert fwd(_stem_desc(1, 2, 4, 4, strides=(96, 32, 16, -4, 1)), p, p, p, p, p, None) == -1 and b"outside" in lib.mspi_last_error()


def test_stem_pack_only_for_the_x3d_stem():
    from mspi_amd import engine as E
    g = torch.Generator().manual_seed(2)
    bn = torch.nn.BatchNorm3d(24).eval()
    wxy, wt = torch.randn(24, 3, 1, 3, 3, generator=g), torch.randn(24, 1, 5, 1, 1, generator=g)
    pk = E.pack_x3d_stem(wxy, wt, bn)
    assert pk is not None and tuple(pk.wxy.shape) == (27, 24) and tuple(pk.wt.shape) == (5, 24) and not pk.wxy.is_cuda
    assert torch.equal(pk.wxy[1 * 9 + 2 * 3 + 1], wxy[:, 1, 0, 2, 1])
    assert E.pack_x3d_stem(torch.randn(24, 3, 1, 5, 5), wt, bn) is None
    assert E.pack_x3d_stem(wxy, torch.randn(24, 1, 3, 1, 1), bn) is None
    assert E.pack_x3d_stem(torch.randn(32, 3, 1, 3, 3), torch.randn(32, 1, 5, 1, 1), torch.nn.BatchNorm3d(32).eval()) is None


# ----------------------------------------------------------------------------- GPU

S2_CASES = [
    # (N, Cin, Cmid, T, H, W)
    (2, 24, 54, 5, 28, 28),      # 14 x 14 out: tile seams in both directions, 54 -> 56 stored, second chunk partial
    (1, 24, 108, 4, 14, 28),     # the stage-3 widths: four chunks, the last with 12 channels
    (1, 24, 54, 1, 14, 14),      # a single frame: both temporal neighbours are padding
    (1, 24, 54, 16, 14, 28),     # a long clip: several T segments
]


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs, weights and the float64 reference of one case: computed once, shared by the se / no-se tests, never modified."""
    N, Cin, Cmid, T, H, W = case
    g = torch.Generator().manual_seed(Cin + Cmid + T + H)
    x = torch.randn(N, Cin, T, H, W, generator=g)
    wa = torch.randn(Cmid, Cin, 1, 1, 1, generator=g) / math.sqrt(Cin)
    ba = torch.randn(Cmid, generator=g) * 0.3
    wb = torch.randn(Cmid, 1, 3, 3, 3, generator=g) / math.sqrt(27)
    bb = torch.randn(Cmid, generator=g) * 0.3
    t = F.relu(F.conv3d(x.double(), wa.double(), ba.double()))
    ref = F.conv3d(t, wb.double(), bb.double(), (1, 2, 2), 1, 1, Cmid)
    return x, wa, ba, wb, bb, ref


def _sentinel_out(E, dev, N, T, Ho, Wo, Cmid):
    """An output view with room before it, after it and beside every row, all holding the sentinel."""
    cs = E.rup4(Cmid)
    ld, off, rows = cs + 4, 64, N * T * Ho * Wo
    buf = torch.full((off + rows * ld + 64,), SENTINEL, dtype=torch.float32, device=dev)
    return E.CL(buf, off, N, T, Ho, Wo, Cmid, ld), (buf, off, rows, ld, cs)


def _untouched(lay):
    buf, off, rows, ld, cs = lay
    body = buf[off: off + rows * ld].view(rows, ld)
    return bool((buf[:off] == SENTINEL).all() and (buf[off + rows * ld:] == SENTINEL).all() and (body[:, cs:] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", S2_CASES)
@pytest.mark.parametrize("se", [False, True])
def test_x3d_ab_s2_fused(dev, case, se):
    from mspi_amd import engine as E
    from mspi_amd.module import to_cl
    if E.DEFAULT_PREC != E.PREC_F16X3:
        pytest.skip("the fused X3D kernel is an f16x3 kernel")
    N, Cin, Cmid, T, H, W = case
    x, wa, ba, wb, bb, ref = _case(case)
    Ho, Wo = H // 2, W // 2
    xc = to_cl(x.to(dev))
    pa = E.pack_conv(wa, ba, act=E.ACT_RELU, cin_stored=xc.Cs, device=dev)
    pb = E.pack_dwconv(wb, bb, None, (1, 2, 2), (1, 1, 1), E.ACT_NONE if se else E.ACT_SWISH, device=dev)
    pk = E.pack_x3d_ab_s2(pa, pb)
    assert pk is not None and E.x3d_ab_s2_supported(xc, pk)
    lib = E._lib.load()
    d = E._x3d_ab_s2_desc(xc, pk, pk.cmid_s, E.ACT_NONE)
    assert lib.mspi_x3d_ab_s2_variant(C.byref(d)) == 17071
    rows = lib.mspi_x3d_ab_s2_pool_rows(C.byref(d))
    tiles = (Ho // 7) * (Wo // 7)
    assert rows % tiles == 0
    if T == 16:
        assert rows // tiles > 1, "the long clip must be cut into T segments (tseg < T)"
    E.range_flag()
    o1, lay1 = _sentinel_out(E, dev, N, T, Ho, Wo, Cmid)
    o2, lay2 = _sentinel_out(E, dev, N, T, Ho, Wo, Cmid)
    if se:
        u, part = E.x3d_ab_s2(xc, pk, pool=True, out=o1)
        u2, part2 = E.x3d_ab_s2(xc, pk, pool=True, out=o2)
        assert tuple(part.shape) == (N, rows, pk.cmid_s)
        _close(u.as_ncdhw(Cmid), ref.float(), TOL, "s2 a+b")
        _close(part.sum(1)[:, :Cmid], ref.sum((2, 3, 4)).float(), TOL, "s2 a+b: se partial sums")
        assert torch.equal(part, part2)
        assert (part[:, :, Cmid:] == 0).all()
    else:
        u = E.x3d_ab_s2(xc, pk, out=o1)
        u2 = E.x3d_ab_s2(xc, pk, out=o2)
        _close(u.as_ncdhw(Cmid), F.silu(ref).float(), TOL, "s2 a+b + swish")
    assert torch.equal(u.buf, u2.buf), "second call differs"
    assert _untouched(lay1) and _untouched(lay2), "wrote outside [rows, :Cs]"
    # the unfused pair of launches computes the same thing
    v = E.dwconv(E.conv(xc, pa), pb)
    _close(u.as_ncdhw(Cmid), v.as_ncdhw(Cmid).cpu(), TOL, "fused vs unfused")
    torch.cuda.synchronize()
    assert not E.range_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("H,fused_calls", [(15, 0), (28, 1)])
@pytest.mark.parametrize("block_idx", [0, 1])
def test_x3d_transform_takes_the_fused_path_only_where_supported(dev, monkeypatch, H, fused_calls, block_idx):
    """X3DTransform with `b` at stride 2: H = 15 is refused by mspi_x3d_ab_s2_supported and runs the unfused pair; H = 28 runs
    the fused launch.  Both against the module's own layers in float64 (block_idx 0 has squeeze-excite).  The block is a
    chain of layers (a, b, the SE gate, c), so its bar is the one test_parity_gpu.py holds chains of these layers to: 1e-4
    of the largest reference value."""
    from mspi_amd import engine as E, testing as T, _lib as L
    from mspi_amd.backbones import blocks3d as B
    from mspi_amd.module import to_cl
    if E.DEFAULT_PREC != E.PREC_F16X3:
        pytest.skip("the fused X3D kernel is an f16x3 kernel")
    W, Tn = 28, 3
    assert L.load().mspi_x3d_ab_s2_supported(C.byref(_desc(1, Tn, H, W, 24, 56))) == (1 if H == 28 else 0)
    m = T.seeded(lambda: B.X3DTransform(24, 24, 3, 2, 54, 54, block_idx=block_idx), 3)
    g = torch.Generator().manual_seed(H)
    x = torch.randn(1, 24, Tn, H, W, generator=g)
    md = m.double()
    u = md.b_bn(md.b(F.relu(md.a_bn(md.a(x.double())))))
    if hasattr(md, "se"):
        s = u.mean((2, 3, 4), keepdim=True)
        u = u * torch.sigmoid(md.se.fc2(F.relu(md.se.fc1(s))))
    ref = F.relu(md.c_bn(md.c(F.silu(u))))
    m = m.float().to(dev)
    calls = []
    real = E.x3d_ab_s2
    monkeypatch.setattr(E, "x3d_ab_s2", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(B, "FUSE_S2", "1")
    y = m.run(to_cl(x.to(dev)), None)
    assert len(calls) == fused_calls
    assert tuple(y.as_ncdhw().shape) == tuple(ref.shape)
    _close(y.as_ncdhw(), ref.float(), 1e-4, "X3DTransform H=%d" % H)
    monkeypatch.setattr(B, "FUSE_S2", "0")
    calls.clear()
    y0 = m.run(to_cl(x.to(dev)), None)
    assert not calls
    _close(y.as_ncdhw(), y0.as_ncdhw().cpu(), 1e-4, "X3DTransform fused vs unfused H=%d" % H)


@pytest.mark.gpu
def test_x3dl_backbone_fused_head_vs_unfused(dev, monkeypatch):
    """X3D-L, seeded and conditioned as bench.py does: the four features with the stride-2 fusion (stages 2-5) and the fused
    stem forced on against both forced off, at the relative bar test_parity_gpu.py holds the X3D features to (1e-4 of the feature's largest value)."""
    from mspi_amd import testing as T
    from mspi_amd.backbones import blocks3d as B
    from mspi_amd.backbones.X3D import X3D
    from mspi_amd.config import cfg
    m = T.condition_(T.seeded(lambda: X3D(cfg.MODEL.X3D.PATH_CFG), 0), "x3dl").to(dev)
    clips, _ = T.synth_inputs(1, 4, 112, 112, seed=0, device=dev)
    feats = {}
    for sw in ("0", "1"):
        monkeypatch.setattr(B, "FUSE_S2", sw)
        monkeypatch.setattr(B, "STEM_FUSED", sw)
        feats[sw] = [f.detach().float().cpu().clone() for f in m([clips])]
    worst = 0.0
    for i, (a, b) in enumerate(zip(feats["1"], feats["0"])):
        assert a.shape == b.shape
        rel = ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()
        print("feature v%d: fused vs unfused, relative max error %.3e" % (i + 1, rel))
        worst = max(worst, rel)
    print("X3D-L backbone, MSPI_X3D_FUSE_S2 and MSPI_X3D_STEM_FUSED 1 vs 0: worst relative error %.3e" % worst)
    assert worst < 1e-4


STEM_CASES = [
    # (N, T, H, W, view): view = slice of a larger tensor
    (2, 6, 28, 28, False),
    (1, 1, 16, 20, False),       # T below the 5 taps: every temporal neighbour but the frame itself is padding
    (1, 16, 28, 28, False),      # T segments
    (2, 6, 28, 28, True),        # a non-contiguous view of a larger tensor
    (1, 3, 17, 19, False),       # odd extent: the last output row / column has no padding tap on its far side
]


@functools.lru_cache(maxsize=None)
def _stem_case(case):
    N, T, H, W, view = case
    g = torch.Generator().manual_seed(T + H + W)
    if view:
        big = torch.randn(N + 2, 3, T + 4, H + 6, W + 8, generator=g)
        x = big[1:N + 1, :, 2:T + 2, 3:H + 3, 5:W + 5]
    else:
        big = x = torch.randn(N, 3, T, H, W, generator=g)
    wxy = torch.randn(24, 3, 1, 3, 3, generator=g) / math.sqrt(27)
    wt = torch.randn(24, 1, 5, 1, 1, generator=g) / math.sqrt(5)
    bn = torch.nn.BatchNorm3d(24).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(24, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(24, generator=g) * 0.4 - 0.2)
        bn.running_mean.copy_(torch.rand(24, generator=g) * 0.4 - 0.2)
        bn.running_var.copy_(torch.rand(24, generator=g) + 0.5)
        y = F.conv3d(x.double(), wxy.double(), None, (1, 2, 2), (0, 1, 1))
        y = F.conv3d(y, wt.double(), None, 1, (2, 0, 0), 1, 24)
        sc = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        ref = F.relu(y * sc.view(1, -1, 1, 1, 1) + (bn.bias.double() - bn.running_mean.double() * sc).view(1, -1, 1, 1, 1))
    return big, wxy, wt, bn, ref


@pytest.mark.gpu
@pytest.mark.parametrize("case", STEM_CASES)
def test_x3d_stem_fused(dev, case):
    """mspi_x3d_stem_fwd against float64 conv3d -> depthwise conv3d -> eval BN -> ReLU, against the unfused pair of launches,
    and bit for bit against itself.  Bar 2e-5: the fused kernel's products are fp32 FMAs (K = 27, then 5 taps), at least as
    exact as the f16x3 pair it replaces, which test_ops_gpu.py holds to 2e-5."""
    from mspi_amd import engine as E
    N, T, H, W, view = case
    big, wxy, wt, bn, ref = _stem_case(case)
    xb = big.to(dev)
    x = xb[1:N + 1, :, 2:T + 2, 3:H + 3, 5:W + 5] if view else xb
    assert x.is_contiguous() != view
    pk = E.pack_x3d_stem(wxy, wt, bn)
    assert pk is not None and E.x3d_stem_supported(x, pk)
    tseg = E._lib.load().mspi_x3d_stem_variant(C.byref(E._x3d_stem_desc(x, 24)))
    if T == 16:
        assert 1 <= tseg < T, "the long clip must be cut into T segments"
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    o1, lay1 = _sentinel_out(E, dev, N, T, Ho, Wo, 24)
    o2, lay2 = _sentinel_out(E, dev, N, T, Ho, Wo, 24)
    y = E.x3d_stem(x, pk, out=o1)
    y2 = E.x3d_stem(x, pk, out=o2)
    _close(y.as_ncdhw(24), ref.float(), TOL, "stem")
    assert torch.equal(y.buf, y2.buf), "second call differs"
    assert _untouched(lay1) and _untouched(lay2), "wrote outside [rows, :24]"
    pxy = E.pack_conv(wxy, None, None, (1, 2, 2), (0, 1, 1), E.ACT_NONE, device=dev)
    pt = E.pack_dwconv(wt, None, bn, (1, 1, 1), (2, 0, 0), E.ACT_RELU, device=dev)
    v = E.dwconv(E.conv(x, pxy), pt)
    _close(y.as_ncdhw(24), v.as_ncdhw(24).cpu(), TOL, "stem: fused vs unfused")
    yd = E.x3d_stem(x, pk)                       # the default output allocation
    assert torch.equal(yd.as_ncdhw(24), y.as_ncdhw(24))
