"""Coverage ledger of the depthwise-convolution and attention dispatchers: one case per kernel instantiation that
mspi_dwconv_fwd / mspi_attn_fwd(_ws) can launch under the default environment, named by the host-only queries
mspi_dwconv_variant / mspi_attn_variant (include/mspi_hip.h), which the launches themselves switch on.

CPU: every ledger row selects its code, and a sweep over many descriptors finds no reachable code without a row -- a new
instantiation, or a heuristic change that moves a model shape onto another kernel, fails here before any GPU run.
GPU: every row against a float64 torch reference (tolerance relative to the output's own magnitude, no floor), plus the
range-guard and per-layer precision routing of the attention kernels."""
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

# ----------------------------------------------------------------------------------------------------------- the ledger
# depthwise: code -> (N, C, T, H, W, kernel, stride, pad).  code = kind * 1000 + K * 100 + stride * 10 + SW, kind 1 = LDS-staged,
# 2 = register tile, 3 = strip, 4 = generic.  The shapes carry the edges where these kernels go wrong: odd Ho (row pairs of the
# tile kernel), Wo not a multiple of SW, C / 4 = 37 (channel groups of one) or 33 (groups of 11), C / 4 = 40 (two groups),
# N > 1 and T > 1 with kT = 1.
DW_LEDGER = {
    1717: (2, 96, 2, 13, 14, (1, 7, 7), (1, 1, 1), (0, 3, 3)),       # 7x7 on a 14-wide map (ConvNeXt stage 3)
    1714: (1, 148, 1, 12, 12, (1, 7, 7), (1, 1, 1), (0, 3, 3)),      # Wo 12: ragged 7-strips -> SW 4; C/4 = 37
    1517: (1, 64, 3, 7, 7, (5, 5, 5), (1, 1, 1), (2, 2, 2)),         # UniFormer's local "attention"
    1514: (2, 64, 4, 9, 10, (5, 5, 5), (1, 1, 1), (2, 2, 2)),
    2717: (2, 148, 2, 29, 28, (1, 7, 7), (1, 1, 1), (0, 3, 3)),      # fusion head dwconv_s / ConvNeXt stage 1-2; Ho 29, C/4 = 37
    2714: (2, 160, 3, 15, 30, (1, 7, 7), (1, 1, 1), (0, 3, 3)),      # Wo 30 = 7 strips of 4 + 2; C/4 = 40: two channel groups
    2317: (2, 132, 3, 9, 14, (3, 3, 3), (1, 1, 1), (1, 1, 1)),       # X3D b; C/4 = 33: groups of 11
    2314: (2, 56, 4, 9, 10, (3, 3, 3), (1, 1, 1), (1, 1, 1)),
    2327: (2, 148, 2, 13, 14, (3, 3, 3), (1, 2, 2), (1, 1, 1)),      # X3D b, first block of a stage: Ho 7 (odd), Wo 7
    2324: (1, 108, 3, 11, 11, (3, 3, 3), (1, 2, 2), (1, 1, 1)),      # Wo 6
    3714: (2, 148, 2, 7, 7, (1, 7, 7), (1, 1, 1), (0, 3, 3)),        # ConvNeXt stage 4 / fusion head at 7x7
    3314: (2, 56, 3, 9, 10, (3, 3, 3), (1, 2, 1), (1, 1, 1)),        # square 3x3, unequal H/W strides: no tile kernel
    3324: (2, 56, 3, 9, 10, (3, 3, 3), (1, 1, 2), (1, 1, 1)),
    3514: (1, 64, 6, 9, 10, (5, 5, 5), (2, 1, 1), (2, 2, 2)),        # temporal stride: no LDS kernel
    4000: (1, 16, 2, 6, 9, (2, 5, 4), (1, 1, 2), (0, 2, 1)),         # non-square: the generic kernel
}
# reachable only through an A/B switch (or not at all without one): never selected under the default environment
DW_EXCLUDED = {
    1317: "LDS-staged 3x3: only with MSPI_DW_LDS=1 (measured slower than the tile kernel on every 3x3x3 shape)",
    1314: "LDS-staged 3x3: only with MSPI_DW_LDS=1",
}
# MSPI_DW_STRIP, MSPI_DW_TILE3=0, MSPI_DW_TILE_ALL and MSPI_DW_LDS=0 only move shapes between the codes above.

# attention: code -> (B, Hh, Nq, Nk, D, Dv, prec, bias, mask, tok, ws, res).  code = kind * 10^7 + D * 10^4 + Dv * 10 + merge,
# kind 1 = fp32, 2 = f16x3 without planes (mspi_attn_fwd), 3 = f16x3 on prefetched planes (bias / mask / token index),
# 5 = software pipeline (no bias, mask or token index); merge = key split + merge pass (>= 24 key tiles, few query tiles).
_PAIRS = ((32, 32), (64, 64), (96, 96), (128, 128), (128, 96), (144, 96), (160, 96))
F32, F16X3 = 0, 1


def _attn_ledger():
    rows = {}
    for i, (D, Dv) in enumerate(_PAIRS):
        pair = D * 10000 + Dv * 10
        res = D != Dv                       # MViT form: residual pooling rides along as `res`
        swin = i % 2 == 0                   # alternate the Swin form (bias + mask + token index) and the plain form
        rows[10000000 + pair] = (2, 2, 77, 77, D, Dv, F32, swin, swin, swin, False, res)
        rows[20000000 + pair] = (2, 2, 97, 97, D, Dv, F16X3, swin, swin, swin, False, res)
        rows[30000000 + pair] = (4, 2, 71, 71, D, Dv, F16X3, True, i % 3 != 1, i % 3 != 2, True, res)
        rows[50000000 + pair] = (2, 2, 300, 300, D, Dv, F16X3, False, False, False, True, res)
        rows[50000000 + pair + 1] = (1, 1, 100, 900 if i % 2 else 790, D, Dv, F16X3, False, False, False, True, res)
    return rows


ATTN_LEDGER = _attn_ledger()
ATTN_EXCLUDED = {}
for _D, _Dv in _PAIRS:
    ATTN_EXCLUDED[40000000 + _D * 10000 + _Dv * 10] = "planes without register prefetch: only with MSPI_ATTN_PF=0"
    ATTN_EXCLUDED[30000000 + _D * 10000 + _Dv * 10 + 1] = "key split on the non-pipelined kernel: only with MSPI_ATTN_PIPE=0"
# MSPI_ATTN_KSPLIT=0 only drops the merge pass (codes above); MSPI_ATTN_PLANES=0 (engine) only routes f16x3 to kind 2.


# environment switches that move calls between the kernels of this ledger (test_gemm_ledger.py passes its own prefixes)
SWITCHES = ("MSPI_DW_", "MSPI_ATTN_")


def _switches(prefixes=SWITCHES):
    return sorted(k for k in os.environ if k.startswith(prefixes))


def _no_switches(prefixes=SWITCHES):
    if _switches(prefixes):
        pytest.skip("dispatch switches set in the environment: %s" % ", ".join(_switches(prefixes)))


def _dw_desc(N, Cc, T, H, W, k, s, p, ldx=None, ldy=None):
    from mspi_amd import _lib
    d = _lib.DwConvDesc()
    d.N, d.T, d.H, d.W, d.C = N, T, H, W, Cc
    d.ldx, d.ldy = ldx or Cc, ldy or Cc
    d.kT, d.kH, d.kW = k
    d.strT, d.strH, d.strW = s
    d.padT, d.padH, d.padW = p
    d.To, d.Ho, d.Wo = ((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip((T, H, W), k, s, p))
    return d


def _attn_desc(B, Hh, Nq, Nk, D, Dv, prec):
    from mspi_amd import _lib
    d = _lib.AttnDesc()
    d.B, d.Hh, d.Nq, d.Nk, d.D, d.Dv, d.prec = B, Hh, Nq, Nk, D, Dv, prec
    return d


def _dw_code(*case):
    from mspi_amd import _lib
    return _lib.load().mspi_dwconv_variant(C.byref(_dw_desc(*case)))


def _attn_code(row):
    from mspi_amd import _lib
    B, Hh, Nq, Nk, D, Dv, prec, bias, mask, tok, ws, _ = row
    return _lib.load().mspi_attn_variant(C.byref(_attn_desc(B, Hh, Nq, Nk, D, Dv, prec)), bias, mask, tok, ws)


def _dw_sweep():
    """Every code mspi_dwconv_variant returns over a grid of kernels, strides, map sizes and channel counts."""
    seen = {}
    kernels = [(1, 7, 7), (7, 1, 1), (3, 3, 3), (1, 3, 3), (5, 5, 5), (1, 5, 5), (3, 5, 5), (9, 7, 7), (2, 5, 4), (3, 1, 1),
               (1, 1, 1), (3, 7, 7)]
    strides = [(1, 1, 1), (2, 1, 1), (1, 2, 2), (1, 2, 1), (1, 1, 2), (2, 2, 2), (1, 3, 3)]
    for k in kernels:
        for s in strides:
            for W in (5, 7, 8, 10, 12, 14, 15, 20, 28, 30, 56):
                for H in (7, 14):
                    for Cc in (64, 148):
                        case = (2, Cc, 9, H, W, k, s, tuple(kk // 2 for kk in k))
                        code = _dw_code(*case)
                        if code > 0:
                            seen.setdefault(code, case)
    return seen


def _attn_sweep():
    seen = {}
    for D in range(16, 257, 16):
        for Dv in range(16, 257, 16):
            for prec in (F32, F16X3):
                for B, Hh, Nq, Nk in ((2, 2, 300, 300), (1, 1, 100, 900), (8, 4, 874, 874)):
                    for flags in range(16):
                        row = (B, Hh, Nq, Nk, D, Dv, prec, flags & 1, (flags >> 1) & 1, (flags >> 2) & 1, (flags >> 3) & 1, False)
                        code = _attn_code(row)
                        if code > 0:
                            seen.setdefault(code, row)
    return seen


# ------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("code", sorted(DW_LEDGER))
def test_dw_ledger_row_selects_its_kernel(code):
    _no_switches()
    assert _dw_code(*DW_LEDGER[code]) == code


@pytest.mark.parametrize("code", sorted(ATTN_LEDGER))
def test_attn_ledger_row_selects_its_kernel(code):
    _no_switches()
    assert _attn_code(ATTN_LEDGER[code]) == code


def test_dw_ledger_covers_every_reachable_kernel():
    _no_switches()
    seen = _dw_sweep()
    missing = {c: case for c, case in seen.items() if c not in DW_LEDGER}
    assert not missing, "depthwise kernels without a ledger case (code: a descriptor that selects it): %s" % missing
    assert not set(seen) & set(DW_EXCLUDED), "an excluded variant is reachable by default: %s" % (set(seen) & set(DW_EXCLUDED))
    assert set(DW_LEDGER) == set(seen), "ledger rows the sweep never reaches: %s" % (set(DW_LEDGER) - set(seen))


def test_attn_ledger_covers_every_reachable_kernel():
    _no_switches()
    seen = _attn_sweep()
    missing = {c: row for c, row in seen.items() if c not in ATTN_LEDGER}
    assert not missing, "attention kernels without a ledger case (code: a descriptor that selects it): %s" % missing
    assert not set(seen) & set(ATTN_EXCLUDED), "an excluded variant is reachable by default: %s" % (set(seen) & set(ATTN_EXCLUDED))
    assert set(ATTN_LEDGER) == set(seen), "ledger rows the sweep never reaches: %s" % (set(ATTN_LEDGER) - set(seen))


def test_variant_queries_reject_bad_descriptors():
    from mspi_amd import _lib
    lib = _lib.load()
    assert lib.mspi_dwconv_variant(C.byref(_dw_desc(1, 6, 1, 5, 5, (1, 3, 3), (1, 1, 1), (0, 1, 1)))) == -1    # C % 4
    bad = _dw_desc(1, 8, 1, 5, 5, (1, 3, 3), (1, 1, 1), (0, 1, 1))
    bad.Wo = 4
    assert lib.mspi_dwconv_variant(C.byref(bad)) == -1 and b"does not match" in lib.mspi_last_error()
    assert lib.mspi_attn_variant(C.byref(_attn_desc(1, 1, 64, 64, 48, 48, F32)), 0, 0, 0, 0) == -1
    assert lib.mspi_attn_variant(C.byref(_attn_desc(1, 1, 64, 64, 64, 64, 7)), 0, 0, 0, 1) == -1


def test_production_shapes_keep_their_kernels():
    """Model shapes pinned to the kernel they run today: a heuristic change that moves one of them onto another (possibly
    less tested) instantiation must show up here."""
    _no_switches()
    # fusion head ConvNextBlock.dwconv_s (1,7,7) at its wide levels (56, 28) and at 7x7
    for W in (56, 28):
        assert _dw_code(8, 96, 4, W, W, (1, 7, 7), (1, 1, 1), (0, 3, 3)) == 2717
    assert _dw_code(8, 96, 4, 7, 7, (1, 7, 7), (1, 1, 1), (0, 3, 3)) == 3714
    # ConvNeXt-T (per frame, T = 1): stages 1-2 on the tile kernel, stage 3 LDS-staged, stage 4 strip
    assert _dw_code(16, 96, 1, 56, 56, (1, 7, 7), (1, 1, 1), (0, 3, 3)) == 2717
    assert _dw_code(16, 384, 1, 14, 14, (1, 7, 7), (1, 1, 1), (0, 3, 3)) == 1717
    assert _dw_code(16, 768, 1, 7, 7, (1, 7, 7), (1, 1, 1), (0, 3, 3)) == 3714
    # X3D-L (3,3,3) depthwise convs: stride-2 entry of stage 2 (112 -> 56) and the stride-1 blocks of stages 2 and 5
    assert _dw_code(8, 56, 16, 112, 112, (3, 3, 3), (1, 2, 2), (1, 1, 1)) == 2327
    assert _dw_code(8, 56, 16, 56, 56, (3, 3, 3), (1, 1, 1), (1, 1, 1)) == 2317
    assert _dw_code(8, 432, 16, 7, 7, (3, 3, 3), (1, 1, 1), (1, 1, 1)) == 2317
    # sync-block attention of the bench line (8 clips, 4 heads of 128, 16 x 7^2 visual + 90 audio tokens): pipeline + merge
    assert _attn_code((8, 4, 874, 874, 128, 128, F16X3, False, False, False, True, False)) == 51281281


def _attn_ksplit(B, Hh, Nq, Nk):
    """attn_ksplit of csrc/attn.hip restated: key slices so that the grid reaches 512 workgroups, none under 12 tiles, <= 8."""
    wgs = (Nq + 127) // 128 * B * Hh
    ntile = (Nk + 31) // 32
    split = min(512 // max(wgs, 1), ntile // 12, 8)
    while split > 1 and (split - 1) * ((ntile + split - 1) // split) >= ntile:      # every slice non-empty
        split -= 1
    return split if split > 1 else 1


def _attn_ws_bytes(B, Hh, Nq, Nk, D, Dv):
    """The workspace of mspi_attn_fwd_ws restated: f16 hi / lo planes of K and V (the larger of the plain layout and the
    per-tile LDS images, padded to 16 B), then the key split's partial O and (max, sum)."""
    nkp = (Nk + 31) // 32 * 32
    plain = B * Hh * 2 * nkp * (D + Dv) * 2
    kti, vti = 64 * (D + 8), (144 * Dv + 1023) // 1024 * 512
    img = B * Hh * (nkp // 32) * (kti + vti) * 2
    planes = (max(plain, img) + 15) // 16 * 16
    split = _attn_ksplit(B, Hh, Nq, Nk)
    return planes + (split * B * Hh * Nq * (Dv + 2) * 4 if split > 1 else 0)


def test_attn_workspace_size_matches_its_layout():
    """mspi_attn_ws_bytes against the layout restated above (MSPI_ATTN_KSPLIT unset): every workspace row of the ledger, the
    sync block's shape, MViT's key-split and many-query stages, and pairs without kernels (the size query does not check
    the pair).  fp32 needs no workspace."""
    from mspi_amd import _lib
    _no_switches()
    lib = _lib.load()
    shapes = [row[:6] for row in ATTN_LEDGER.values() if row[10]]
    shapes += [(8, 4, 874, 874, 128, 128), (8, 8, 392, 1568, 160, 96), (8, 1, 25088, 392, 128, 96)]
    shapes += [(2, 3, 50, 2000, 48, 80), (1, 2, 130, 33, 256, 16)]
    assert len(shapes) == 3 * len(_PAIRS) + 5
    splits = set()
    for B, Hh, Nq, Nk, D, Dv in shapes:
        assert lib.mspi_attn_ws_bytes(C.byref(_attn_desc(B, Hh, Nq, Nk, D, Dv, F16X3))) == _attn_ws_bytes(B, Hh, Nq, Nk, D, Dv), \
            (B, Hh, Nq, Nk, D, Dv)
        assert lib.mspi_attn_ws_bytes(C.byref(_attn_desc(B, Hh, Nq, Nk, D, Dv, F32))) == 0
        splits.add(_attn_ksplit(B, Hh, Nq, Nk))
    assert {1, 2}.issubset(splits) and max(splits) > 2      # the cases hold unsplit, two-slice and wider key splits


def test_attn_refusal_names_every_instantiated_pair():
    """A (D, Dv) without kernels is refused by both launches with the full list of pairs, in order; the variant query says -1.
    Nothing launches: the pair is checked on the host."""
    import ctypes
    from mspi_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 72)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    listed = ",".join("(%d,%d)" % pair for pair in _PAIRS)
    for D, Dv in ((48, 48), (96, 128), (128, 64), (160, 160)):
        for prec in (F32, F16X3):
            d = _attn_desc(1, 1, 1, 1, D, Dv, prec)
            want = ("mspi_attn_fwd: (D=%d, Dv=%d) not in {%s}" % (D, Dv, listed)).encode()
            assert lib.mspi_attn_fwd(C.byref(d), p, p, p, None, None, None, None, p, None) == -1
            assert lib.mspi_last_error() == want
            assert lib.mspi_attn_fwd_ws(C.byref(d), p, p, p, None, None, None, None, p, p, None) == -1
            assert lib.mspi_last_error() == want
            for flags in range(16):
                assert lib.mspi_attn_variant(C.byref(d), flags & 1, (flags >> 1) & 1, (flags >> 2) & 1, flags >> 3) == -1


# ------------------------------------------------------------------------------------------------------------ GPU tests
def _rel_close(got, ref, tol, what):
    """max |got - ref| <= tol * max |ref| (no floor: down-scaled outputs keep their relative bar)."""
    err = (got.cpu().double() - ref.double()).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= tol * scale, "%s: max abs err %.3e, %.1e of max|ref| %.3e" % (what, err, err / max(scale, 1e-300), scale)


def _guard(E, dev):
    """Register the range-guard word and clear it."""
    E._need_gpu(torch.empty(1, device=dev))
    E.range_flag()


def _pool_supported(k, s):
    return k[1] == k[2] and (k[2], s[2]) in ((3, 1), (3, 2), (5, 1), (7, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("code", sorted(DW_LEDGER))
def test_dw_ledger_kernel_vs_fp64(dev, code):
    """Each depthwise instantiation against F.conv3d(groups=C) in float64: swish and no activation, dense and from a channel
    slice of a wider buffer (MViT's qkv.slice) into a channel slice of another (columns outside it untouched), pooled
    partial sums (bitwise reproducible) where the kernel has them."""
    from mspi_amd import engine as E
    _no_switches()
    N, Cc, T, H, W, k, s, p = DW_LEDGER[code]
    g = torch.Generator().manual_seed(code)
    x = torch.randn(N, Cc, T, H, W, generator=g)
    w = torch.randn(Cc, 1, *k, generator=g) / math.sqrt(k[0] * k[1] * k[2])
    b = torch.randn(Cc, generator=g)
    ref = F.conv3d(x.double(), w.double(), b.double(), s, p, 1, Cc)
    pk = E.pack_dwconv(w, b, None, s, p, E.ACT_SWISH, device=dev)
    xd = E.alloc(N, T, H, W, Cc, dev)
    xd.as_ncdhw().copy_(x.to(dev))
    assert E.dwconv_variant(xd, pk) == code
    _guard(E, dev)
    _rel_close(E.dwconv(xd, pk).as_ncdhw(), ref * torch.sigmoid(ref), 1e-5, "dwconv %d swish" % code)
    _rel_close(E.dwconv(xd, pk, act=E.ACT_NONE).as_ncdhw(), ref, 1e-5, "dwconv %d" % code)
    # input: columns [Cc + 4, 2 Cc + 4) of rows 2 Cc + 8 wide; output: columns [8, Cc + 8) of rows Cc + 12 wide
    wide_in = E.alloc(N, T, H, W, 2 * Cc + 8, dev)
    wide_in.buf.fill_(1e3)
    xs = wide_in.slice(Cc + 4, Cc)
    xs.as_ncdhw().copy_(x.to(dev))
    assert xs.ld > xs.C and E.dwconv_variant(xs, pk) == code
    To, Ho, Wo = ref.shape[2:]
    wide_out = E.alloc(N, To, Ho, Wo, Cc + 12, dev)
    wide_out.buf.fill_(-3.0)
    E.dwconv(xs, pk, out=wide_out.slice(8, Cc), act=E.ACT_NONE)
    got = wide_out.as_ncdhw()
    _rel_close(got[:, 8:Cc + 8], ref, 1e-5, "dwconv %d, channel slices" % code)
    assert (got[:, :8] == -3.0).all() and (got[:, Cc + 8:] == -3.0).all(), "dwconv %d wrote outside its output slice" % code
    if _pool_supported(k, s):
        out, part = E.dwconv(xd, pk, pool=True, act=E.ACT_NONE)
        _rel_close(out.as_ncdhw(), ref, 1e-5, "dwconv %d (pool)" % code)
        _rel_close(part.sum(1)[:, :Cc], ref.sum((2, 3, 4)), 1e-5, "dwconv %d pooled sums" % code)
        out2, part2 = E.dwconv(xd, pk, pool=True, act=E.ACT_NONE)
        assert torch.equal(part, part2) and torch.equal(out.buf, out2.buf)      # no atomics: bitwise reproducible
    torch.cuda.synchronize()
    assert not E.range_flag()


def _attn_inputs(row, seed):
    """Random operands of a ledger row (float32, CPU) and the float64 reference output.  Layout per sample [S][Hh][R][d]:
    with a token index, B = S * nwin sequences are windows of S samples whose token t lives at row tok[win][t]."""
    B, Hh, Nq, Nk, D, Dv, prec, bias, mask, tok, ws, res = row
    g = torch.Generator().manual_seed(seed)
    nwin = 2 if tok else 1
    S = B // nwin
    Rq, Rk = nwin * Nq, nwin * Nk
    q = torch.randn(S, Hh, Rq, D, generator=g)
    k = torch.randn(S, Hh, Rk, D, generator=g)
    v = torch.randn(S, Hh, Rk, Dv, generator=g)
    r = torch.randn(S, Hh, Rq, Dv, generator=g) if res else None
    bT = torch.randn(Hh, Nk, Nq, generator=g) if bias else None
    nmask = 2
    mT = torch.where(torch.rand(nmask, Nk, Nq, generator=g) < 0.3, torch.tensor(-100.0), torch.tensor(0.0)) if mask else None
    ti = torch.randperm(Rq, generator=g).view(nwin, Nq).to(torch.int32) if tok else None
    t = dict(q=q, k=k, v=v, res=r, biasT=bT, maskT=mT, tok=ti, nwin=nwin, nmask=nmask, scale=D ** -0.5)
    return t, _attn_ref(row, t)


def _attn_ref(row, t):
    """Explicit float64 softmax attention of the operands `t` of a ledger row (test_nonfinite_ledger.py evaluates it on
    poisoned operands too)."""
    B, Hh, Nq, Nk, D, Dv, prec, bias, mask, tok, ws, res = row
    q, k, v, r, bT, mT, ti = (t[n] for n in ("q", "k", "v", "res", "biasT", "maskT", "tok"))
    nwin, nmask, scale = t["nwin"], t["nmask"], t["scale"]
    S, Rq = q.shape[0], q.shape[2]
    ref = torch.zeros(S, Hh, Rq, Dv, dtype=torch.float64)
    for bb in range(B):
        smp, win = bb // nwin, bb % nwin
        rows = ti[win].long() if tok else torch.arange(Nq)
        krows = ti[win].long() if tok else torch.arange(Nk)
        logit = (q[smp][:, rows].double() @ k[smp][:, krows].double().transpose(-1, -2)) * scale
        if bias:
            logit = logit + bT.double().transpose(1, 2)
        if mask:
            logit = logit + mT[bb % nmask].double().t()
        o = logit.softmax(-1) @ v[smp][:, krows].double()
        if res:
            o = o + r[smp][:, rows].double()
        ref[smp][:, rows] = o
    return ref


def _attn_direct(E, row, t, dev, fill=float("nan")):
    """mspi_attn_fwd / mspi_attn_fwd_ws straight from a ledger row into an output prefilled with `fill`.  Returns (output
    [S,Hh,Rq,Dv] on the GPU, variant)."""
    B, Hh, Nq, Nk, D, Dv, prec, bias, mask, tok, ws, res = row
    lib = E._lib.load()
    gq, gk, gv = (t[n].to(dev).contiguous() for n in ("q", "k", "v"))
    S, _, Rq, _ = gq.shape
    Rk = gk.shape[2]
    o = torch.full((S, Hh, Rq, Dv), fill, device=dev)
    d = _attn_desc(B, Hh, Nq, Nk, D, Dv, prec)
    d.nmask = t["nmask"] if mask else 0
    d.nwin = t["nwin"] if tok else 0
    d.q_sB, d.q_sH, d.q_sT = Hh * Rq * D, Rq * D, D
    d.k_sB, d.k_sH, d.k_sT = Hh * Rk * D, Rk * D, D
    d.v_sB, d.v_sH, d.v_sT = Hh * Rk * Dv, Rk * Dv, Dv
    d.o_sB, d.o_sH, d.o_sT = Hh * Rq * Dv, Rq * Dv, Dv
    d.scale = t["scale"]
    keep = [t[n].to(dev).contiguous() if t[n] is not None else None for n in ("res", "biasT", "maskT", "tok")]
    ptrs = [x.data_ptr() if x is not None else None for x in keep]
    variant = lib.mspi_attn_variant(C.byref(d), bias, mask, tok, ws)
    if ws:
        nbytes = lib.mspi_attn_ws_bytes(C.byref(d))
        assert nbytes > 0
        wsb = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        E.check(lib.mspi_attn_fwd_ws(C.byref(d), gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), *ptrs, o.data_ptr(), wsb.data_ptr(),
                                     E._stream()), "mspi_attn_fwd_ws")
    else:
        E.check(lib.mspi_attn_fwd(C.byref(d), gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), *ptrs, o.data_ptr(), E._stream()),
                "mspi_attn_fwd")
    torch.cuda.synchronize()
    return o, variant


@pytest.mark.gpu
@pytest.mark.parametrize("code", sorted(ATTN_LEDGER))
def test_attn_ledger_kernel_vs_fp64(dev, code):
    """Each attention instantiation (kernel x (D, Dv) x merge pass) against explicit float64 softmax attention: ragged query
    and key counts, bias + mask + token index where the row has them, residual for the MViT widths; the range guard stays
    clear on in-range data (padded query rows and key tiles are never flagged)."""
    from mspi_amd import engine as E
    _no_switches()
    row = ATTN_LEDGER[code]
    t, ref = _attn_inputs(row, code % 100003)
    _guard(E, dev)
    out, variant = _attn_direct(E, row, t, dev)
    assert variant == code
    _rel_close(out, ref, 1e-5, "attention variant %d" % code)
    assert not E.range_flag(), "in-range attention flagged as non-finite"


@pytest.mark.gpu
@pytest.mark.parametrize("D,Dv", _PAIRS)
def test_attn_forms_bit_identical(dev, D, Dv):
    """The f16x3 forms of one (D, Dv) give the same bits: K / V split by every query tile (kind 2) against the software
    pipeline on plane images (kind 5), and, with token index + bias + mask, against prefetched plain planes (kind 3).
    97 keys = three full tiles plus one key, 71 = two tiles plus 7 (both lane halves of the key tail), ragged query tiles,
    several sequences and heads; residual for the MViT widths."""
    from mspi_amd import engine as E
    _no_switches()
    pair = D * 10000 + Dv * 10
    res = D != Dv
    for shape, form, with_ws in (((2, 2, 97, 97), False, 50000000), ((4, 2, 71, 71), True, 30000000)):
        row = shape + (D, Dv, F16X3, form, form, form, False, res)
        t, _ = _attn_inputs(row, pair + form)
        direct, code = _attn_direct(E, row, t, dev)
        assert code == 20000000 + pair
        planes, code = _attn_direct(E, row[:10] + (True, res), t, dev)
        assert code == with_ws + pair
        assert not torch.isnan(direct).any() and torch.equal(direct, planes)


def _mvit_case(q_thw, k_thw, heads, B, seed, hd=96):
    """Operands of MViT pooled attention and the float64 reference (decomposed rel-pos + residual pooling)."""
    g = torch.Generator().manual_seed(seed)
    Nq, Nk = math.prod(q_thw), math.prod(k_thw)
    q = torch.randn(B, Nq, heads * hd, generator=g)
    k = torch.randn(B, Nk, heads * hd, generator=g)
    v = torch.randn(B, Nk, heads * hd, generator=g)
    tabs, dists = [], []
    for i in range(3):
        n = 2 * max(q_thw[i], k_thw[i]) - 1
        tabs.append(torch.randn(n, hd, generator=g) * 0.3)
        qr, kr = max(k_thw[i] / q_thw[i], 1.0), max(q_thw[i] / k_thw[i], 1.0)
        dists.append((torch.arange(q_thw[i])[:, None] * qr - torch.arange(k_thw[i])[None, :] * kr + (k_thw[i] - 1) * kr).long())
    Rt, Rh, Rw = (tabs[i][dists[i]] for i in range(3))
    qh = q.view(B, Nq, heads, hd).transpose(1, 2).double()
    kh = k.view(B, Nk, heads, hd).transpose(1, 2).double()
    vh = v.view(B, Nk, heads, hd).transpose(1, 2).double()
    rq = qh.reshape(B, heads, *q_thw, hd)
    att = (qh * hd ** -0.5) @ kh.transpose(-2, -1)
    att = (att.view(B, heads, *q_thw, *k_thw)
           + torch.einsum("bythwc,hkc->bythwk", rq, Rh.double())[:, :, :, :, :, None, :, None]
           + torch.einsum("bythwc,wkc->bythwk", rq, Rw.double())[:, :, :, :, :, None, None, :]
           + torch.einsum("bythwc,tkc->bythwk", rq, Rt.double())[:, :, :, :, :, :, None, None]).view(B, heads, Nq, Nk)
    ref = (att.softmax(-1) @ vh + qh).transpose(1, 2).reshape(B, Nq, heads * hd)
    return dict(q=q, k=k, v=v, Rh=Rh, Rw=Rw, Rt=Rt, tabs=tabs, dists=dists), ref


def _run_mvit(E, c, q_thw, k_thw, heads, B, dev, rel, slot=None, hd=96):
    def cl(t, thw):
        return E.CL(t.to(dev).contiguous().view(-1), 0, B, thw[0], thw[1], thw[2], heads * hd, heads * hd)

    rel_gemm = None
    if rel:
        stack = torch.cat([c["tabs"][1], c["tabs"][2], c["tabs"][0]], 0)           # h, w, t
        offs = (0, c["tabs"][1].shape[0], c["tabs"][1].shape[0] + c["tabs"][2].shape[0])
        idx = [(c["dists"][a].to(torch.int32) + o).contiguous().to(dev) for a, o in zip((1, 2, 0), offs)]
        rel_gemm = (E.pack_conv(stack, None, device=dev), idx[0], idx[1], idx[2])
    out = E.mvit_attention(cl(c["q"], q_thw), cl(c["k"], k_thw), cl(c["v"], k_thw), B, heads, hd, hd ** -0.5, q_thw, k_thw,
                           c["Rh"].to(dev).contiguous(), c["Rw"].to(dev).contiguous(), c["Rt"].to(dev).contiguous(),
                           rel_gemm=rel_gemm, slot=slot)
    return out.as_rows().view(B, math.prod(q_thw), heads * hd)


@pytest.mark.gpu
@pytest.mark.parametrize("rel", [False, True], ids=["dot-kernel", "rel-gemm"])
@pytest.mark.parametrize("q_thw,k_thw,code", [((2, 14, 14), (2, 28, 28), 51600961), ((1, 24, 24), (1, 24, 24), 51600960)])
def test_mvit_attention_160_on_the_pipeline(dev, q_thw, k_thw, code, rel):
    """A key grid with 49 <= kT + kH + kW <= 64 makes the augmented width 160: attn_pipe_kernel<160, 96>, with (2, 28, 28)
    keys also split + merged.  Both forms of the rel-pos dot products."""
    from mspi_amd import engine as E
    _no_switches()
    if E.DEFAULT_PREC != E.PREC_F16X3:
        pytest.skip("f16x3 only")
    B, heads = 2, 1
    c, ref = _mvit_case(q_thw, k_thw, heads, B, sum(k_thw))
    _guard(E, dev)
    E.autotune(False)
    out = _run_mvit(E, c, q_thw, k_thw, heads, B, dev, rel, slot={})
    assert E.attn_variant() == code
    _rel_close(out, ref, 1e-5, "mvit attention (160, 96)")
    torch.cuda.synchronize()
    assert not E.range_flag()


def _qkv_case(B, Ntok, heads, hd, seed, q_mul=1.0, k_mul=1.0, rows=None):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * (rows or Ntok), 3 * heads * hd, generator=g)
    qkv[:, : heads * hd] *= q_mul
    qkv[:, heads * hd: 2 * heads * hd] *= k_mul
    return qkv


def _qkv_ref(qkv, B, Ntok, heads, hd, scale):
    q, k, v = [t.reshape(B, Ntok, heads, hd).permute(0, 2, 1, 3).double() for t in qkv.chunk(3, 1)]
    return (torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v).permute(0, 2, 1, 3).reshape(B * Ntok, heads * hd)


def _slot_f32(key):
    from mspi_amd import engine as E
    return {key: E.PREC_F32}


@pytest.mark.gpu
@pytest.mark.parametrize("hd,Ntok", [(32, 77), (64, 201), (96, 130), (128, 300)])
def test_attention_fp32_route_plain(dev, hd, Ntok):
    """The fp32 kernel as the model reaches it: a layer whose slot holds the F32 decision (what the first-sight range check
    leaves behind), plain qkv at a ragged token count."""
    from mspi_amd import engine as E
    _no_switches()
    B, heads = 2, 2
    qkv = _qkv_case(B, Ntok, heads, hd, hd + Ntok)
    ref = _qkv_ref(qkv, B, Ntok, heads, hd, hd ** -0.5)
    cl = E.CL(qkv.to(dev).view(-1), 0, B, 1, 1, Ntok, 3 * heads * hd, 3 * heads * hd)
    _guard(E, dev)
    out = E.attention(cl, B, Ntok, heads, hd, hd ** -0.5, slot=_slot_f32(("qkv", heads, hd, Ntok, 0)))
    assert E.attn_variant() == 10000000 + hd * 10000 + hd * 10
    _rel_close(out.as_rows(), ref, 1e-5, "fp32 attention hd %d" % hd)
    torch.cuda.synchronize()
    assert not E.range_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f16x3"])
@pytest.mark.parametrize("hd", [32, 64])
def test_attention_swin_padded_grid(dev, prec, hd):
    """Swin form on a grid that is not a multiple of the window: bias + shifted-window mask + token index, every padding token
    on ONE extra row per sample (rows_per_sample = D*H*W + 1).  fp32 through a seeded F32 slot, f16x3 through an empty one."""
    from mspi_amd import engine as E
    from mspi_amd.backbones import video_swin_transformer as S
    _no_switches()
    if prec == 1 and E.DEFAULT_PREC != E.PREC_F16X3:
        pytest.skip("f16x3 only")
    B, D, H, W, heads = 2, 3, 9, 10, 3
    ws, ss = (2, 7, 7), (1, 3, 3)
    Dp, Hp, Wp = 4, 14, 14
    N, R, Cc = ws[0] * ws[1] * ws[2], D * H * W, heads * hd
    g = torch.Generator().manual_seed(hd + prec)
    qkv = torch.randn(B, R + 1, 3 * Cc, generator=g)
    tok = S.window_token_index(D, H, W, ws, ss, (Dp, Hp, Wp))
    nW = tok.shape[0]
    assert (tok == R).any()
    bias = torch.randn(heads, N, N, generator=g)
    mask = S.compute_mask(Dp, Hp, Wp, ws, ss)
    ref = torch.zeros(B, R + 1, Cc, dtype=torch.float64)
    for b in range(B):
        for w in range(nW):
            rows = tok[w].long()
            q, k, v = (qkv[b, rows, i * Cc:(i + 1) * Cc].double().view(N, heads, hd).transpose(0, 1) for i in range(3))
            att = q @ k.transpose(-1, -2) * hd ** -0.5 + bias.double() + mask[w].double()
            o = (att.softmax(-1) @ v).transpose(0, 1).reshape(N, Cc)
            real = rows < R
            ref[b, rows[real]] = o[real]
    xc = E.CL(qkv.to(dev).contiguous().view(-1), 0, B, R + 1, 1, 1, 3 * Cc, 3 * Cc)
    slot = _slot_f32(("qkv", heads, hd, N, nW)) if prec == 0 else {}
    _guard(E, dev)
    E.autotune(False)
    out = E.attention(xc, B * nW, N, heads, hd, hd ** -0.5, biasT=bias.transpose(1, 2).contiguous().to(dev),
                      maskT=mask.transpose(1, 2).contiguous().to(dev), tok_idx=tok.to(dev), rows_per_sample=R + 1, slot=slot)
    assert E.attn_variant() == (10000000 if prec == 0 else 30000000) + hd * 10000 + hd * 10
    got = out.buf.view(B, R + 1, Cc)[:, :R]
    _rel_close(got, ref[:, :R], 1e-5, "swin padded grid")
    torch.cuda.synchronize()
    assert not E.range_flag(), "masked / padded Swin windows flagged as non-finite"


@pytest.mark.gpu
@pytest.mark.parametrize("k_thw,DA", [((2, 3, 3), 128), ((8, 14, 14), 144), ((2, 28, 28), 160)])
def test_mvit_attention_fp32_route(dev, k_thw, DA):
    """MViT form (augmented width 128 / 144 / 160, residual pooling as `res`) on the fp32 kernel through a seeded F32 slot."""
    from mspi_amd import engine as E
    _no_switches()
    B, heads = 2, 1
    q_thw = (k_thw[0], 7, 7)
    c, ref = _mvit_case(q_thw, k_thw, heads, B, DA)
    slot = _slot_f32(("mvit", heads, 96, math.prod(q_thw), math.prod(k_thw)))
    _guard(E, dev)
    out = _run_mvit(E, c, q_thw, k_thw, heads, B, dev, rel=False, slot=slot)
    assert E.attn_variant() == 10000000 + DA * 10000 + 960
    _rel_close(out, ref, 1e-5, "fp32 mvit attention DA %d" % DA)
    torch.cuda.synchronize()
    assert not E.range_flag()


# ----------------------------------------------------------------------------------- per-layer routing and the range guard
@pytest.mark.gpu
def test_attention_range_decision_is_per_layer(dev):
    """Two attention layers of the same shape, the second with |q * scale| ~ 2e3 (inf in the f16x3 hi half): on first sight
    while tuning only the second moves to fp32 -- the decision is the layer's, not the shape's -- and both match fp64."""
    from mspi_amd import engine as E
    _no_switches()
    if E.DEFAULT_PREC != E.PREC_F16X3:
        pytest.skip("f16x3 only")
    B, Ntok, heads, hd, scale = 2, 77, 2, 32, 0.5
    key = ("qkv", heads, hd, Ntok, 0)
    normal = _qkv_case(B, Ntok, heads, hd, 1)
    large = _qkv_case(B, Ntok, heads, hd, 2, q_mul=4e3, k_mul=1e-3)
    slots = ({}, {})
    moved = len(E.RANGE_CHECK["moved"])
    _guard(E, dev)
    outs = []
    E.autotune(True)
    try:
        for qkv, slot in ((normal, slots[0]), (large, slots[1])):
            cl = E.CL(qkv.to(dev).view(-1), 0, B, 1, 1, Ntok, 3 * heads * hd, 3 * heads * hd)
            outs.append(E.attention(cl, B, Ntok, heads, hd, scale, slot=slot).as_rows().cpu())
    finally:
        E.autotune(False)
    assert slots[0][key] == E.PREC_F16X3 and slots[1][key] == E.PREC_F32
    assert len(E.RANGE_CHECK["moved"]) == moved + 1
    for out, qkv in zip(outs, (normal, large)):
        _rel_close(out, _qkv_ref(qkv, B, Ntok, heads, hd, scale), 1e-5, "per-layer attention")
    E.check_range()


@pytest.mark.gpu
def test_swin_blocks_of_one_shape_decide_separately(dev):
    """The same through a real module class: two Swin blocks of identical shape, the second's q projection scaled so that
    |q * scale| ~ 2e3.  While tuning only the second block's attention moves to fp32 (RANGE_CHECK["moved"]); both blocks
    match the float64 reference block; a weight reload gives the layer a fresh decision."""
    from mspi_amd import engine as E
    from mspi_amd.backbones.video_swin_transformer import SwinTransformerBlock3D
    from oracle import restate as R
    _no_switches()
    if E.DEFAULT_PREC != E.PREC_F16X3:
        pytest.skip("f16x3 only")
    dim, heads, window, shift = 96, 3, (2, 7, 7), (1, 3, 3)
    B, D, H, W = 1, 2, 14, 14
    torch.manual_seed(3)
    blocks = [SwinTransformerBlock3D(dim, heads, window, shift).eval() for _ in range(2)]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, D, H, W, dim, generator=g)
    with torch.no_grad():
        for blk in blocks:
            blk.attn.relative_position_bias_table.copy_(torch.randn(blk.attn.relative_position_bias_table.shape, generator=g))
        hn = F.layer_norm(x, (dim,), blocks[1].norm1.weight, blocks[1].norm1.bias, 1e-5)
        qmax = F.linear(hn, blocks[1].attn.qkv.weight[:dim], blocks[1].attn.qkv.bias[:dim]).abs().max().item()
        s = 2e3 / (qmax * (dim // heads) ** -0.5)
        blocks[1].attn.qkv.weight[:dim] *= s
        blocks[1].attn.qkv.bias[:dim] *= s
    refs = []
    for blk in blocks:
        sd = {"b." + kk: vv.double() if vv.is_floating_point() else vv for kk, vv in blk.state_dict().items()}
        ws, ss = R._swin_window_size((D, H, W), window, shift)
        mask = R._swin_mask(D, H, W, ws, ss).double()
        refs.append(R.swin_block(sd, "b", x.double(), heads, window, shift, mask))
        blk.to(dev)
    xc = E.CL(x.to(dev).contiguous().view(-1), 0, B, D, H, W, dim, dim)
    moved = len(E.RANGE_CHECK["moved"])
    _guard(E, dev)
    E.autotune(True)
    try:
        outs = [blk.run(xc).buf.view(B, D, H, W, dim).cpu() for blk in blocks]
    finally:
        E.autotune(False)
    precs = [list(blk.pk["attn_prec"].values()) for blk in blocks]
    assert precs == [[E.PREC_F16X3], [E.PREC_F32]], precs
    new = E.RANGE_CHECK["moved"][moved:]
    assert len([m for m in new if m[0].startswith("attention")]) == 1, new
    # whole blocks (LayerNorms, f16x3 GEMMs, MLP) around the attention; block 1's q projection reaches ~1e4, so fp32 rounding of
    # its logits alone is ~1e-4 absolute: measured 1.3e-5 of max|ref| there, 1e-4 keeps a margin (an f16x3 run is NaN)
    for i, (out, ref) in enumerate(zip(outs, refs)):
        _rel_close(out, ref, 1e-5 if i == 0 else 1e-4, "swin block %d" % i)
    E.check_range()
    blocks[1].load_state_dict(blocks[1].state_dict())          # weights reloaded: the plan and its decisions are rebuilt
    assert "attn_prec" not in blocks[1].pk


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["pipe", "merge", "bias-mask"])
def test_untuned_attention_overflow_is_reported(dev, form):
    """Untuned (no first-sight check), |q| ~ 1.6e4 is inf in the f16x3 hi half (q is pre-scaled by 64): the attention kernels
    themselves report the non-finite output through the range guard, so check_range() raises instead of NaN flowing on
    silently -- for the software pipeline, the key split's merge pass and the bias / mask kernel."""
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    _no_switches()
    if E.DEFAULT_PREC != E.PREC_F16X3:
        pytest.skip("f16x3 only")
    B, Ntok, heads, hd = {"pipe": (2, 201, 2, 64), "merge": (1, 900, 1, 96), "bias-mask": (2, 98, 2, 32)}[form]
    qkv = _qkv_case(B, Ntok, heads, hd, 11, q_mul=4e3, k_mul=1e-3)
    cl = E.CL(qkv.to(dev).view(-1), 0, B, 1, 1, Ntok, 3 * heads * hd, 3 * heads * hd)
    extra = {}
    if form == "bias-mask":
        g = torch.Generator().manual_seed(12)
        extra = dict(biasT=torch.randn(heads, Ntok, Ntok, generator=g).to(dev),
                     maskT=torch.where(torch.rand(2, Ntok, Ntok, generator=g) < 0.3, -100.0, 0.0).to(dev))
    E.autotune(False)
    _guard(E, dev)
    out = E.attention(cl, B, Ntok, heads, hd, hd ** -0.5, slot={}, **extra)
    code = E.attn_variant()
    assert code // 10000000 == (3 if form == "bias-mask" else 5) and code % 10 == (1 if form == "merge" else 0), code
    torch.cuda.synchronize()
    assert not torch.isfinite(out.as_rows()).all()
    with pytest.raises(MspiError, match="f16x3 range"):
        E.check_range()
    assert not E.range_flag()
