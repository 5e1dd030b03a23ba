"""The decoder tail: the readout's 1x1x1 conv r0 moved below the top-down fusion's up-samples, and the sum-of-up-samples
kernel (mspi_upsample_sum_fwd) that replaces the chains of accumulating mspi_upsample_fwd launches.

r0 reads cat(s0', up2(s1'), up4(s2'), up8(s3)) with s0' = s0 + up2(s1') + up4(s2') + up8(s3).  A 1x1x1 conv mixes channels
at one position, a bilinear up-sample mixes positions of one channel: they commute, so with W = [W0|W1|W2|W3]
    r0(cat) = W0 s0 + b + up2((W0+W1) s1') + up4((W0+W2) s2') + up8((W0+W3) s3).

CPU: the identity in fp64 and fp32, the four composed weight blocks against F.conv3d of the concat, the refusals of the new
entry point.  GPU: the kernel bit-equal to the chain it replaces and against fp64 at the ledgers' 1e-5 of max|ref|, and the
whole tail with the rewrite on against off.

The halo-staged conv kernel (mspi_conv_halo_fwd) has its coverage ledger here, in the manner of test_gemm_ledger.py: the
host-only query mspi_conv_halo_variant names the instantiation (kT * 1000 + BN) and the launch switches on it.  CPU: every
code has a ledger row, a sweep reaches no code without one, the refusals carry their messages.  GPU: every case against
F.conv3d in float64 at 1e-5 of max|ref| on shapes ragged in every brick dimension, from a NaN-fenced slab into a slab."""
import ctypes as C
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from test_kernel_ledger import _guard, _rel_close      # the tolerance rule of the ledgers

TOL = 1e-5
BIG = 1.0e3           # neighbour columns of every slab: finite, and ruinous to any result that reads them
NAN = float("nan")


def _up(x, k):
    return F.interpolate(x, scale_factor=(1, k, k), mode="trilinear", align_corners=False)


def _levels(dt, seed=0):
    """s0..s3 after their gates at [2,192,2,16,24] and the three coarser levels, and r0's weight and bias."""
    g = torch.Generator().manual_seed(seed)
    s = [torch.randn(2, 192, 2, 16 >> j, 24 >> j, generator=g, dtype=torch.float64).to(dt) for j in range(4)]
    w = (torch.randn(192, 768, generator=g, dtype=torch.float64) / 768 ** 0.5).to(dt)
    b = torch.randn(192, generator=g, dtype=torch.float64).to(dt)
    return s, w, b


def _tail_old(s, w, b):
    s0, s1, s2, s3 = s
    s2 = s2 + _up(s3, 2)
    s1 = s1 + _up(s2, 2) + _up(s3, 4)
    s0 = s0 + _up(s1, 2) + _up(s2, 4) + _up(s3, 8)
    cat = torch.cat([s0, _up(s1, 2), _up(s2, 4), _up(s3, 8)], 1)
    return F.conv3d(cat, w[:, :, None, None, None], b)


def _tail_new(s, parts):
    s0, s1, s2, s3 = s
    s2 = s2 + _up(s3, 2)
    s1 = s1 + _up(s2, 2) + _up(s3, 4)
    z = [F.conv3d(x, wj[:, :, None, None, None], bj) for x, (wj, bj) in zip((s0, s1, s2, s3), parts)]
    return z[0] + _up(z[1], 2) + _up(z[2], 4) + _up(z[3], 8)


def _parts(w, b):
    from mspi_amd.model.model_utils import _SaliencyBase
    return _SaliencyBase._r0_parts(w[:, :, None, None, None], b)


def _relerr(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_r0_commutes_with_the_upsamples():
    """fp64: the identity to 1e-12 relative.  fp32: the new order is no worse than 4x the old order against fp64."""
    s, w, b = _levels(torch.float64)
    ref = _tail_old(s, w, b)
    d = w.shape[1] // 4
    parts64 = [(w[:, :d], b)] + [(w[:, :d] + w[:, j * d:(j + 1) * d], None) for j in (1, 2, 3)]
    e64 = _relerr(_tail_new(s, parts64), ref)
    assert e64 <= 1e-12, e64
    s32, w32, b32 = [v.float() for v in s], w.float(), b.float()
    ref32 = _tail_old([v.double() for v in s32], w32.double(), b32.double())      # fp64 of the fp32 inputs
    e_old = _relerr(_tail_old(s32, w32, b32), ref32)
    e_new = _relerr(_tail_new(s32, _parts(w32, b32)), ref32)
    print("fp64 identity %.2e; fp32 against fp64: old order %.2e, new order %.2e" % (e64, e_old, e_new))
    assert e_new <= 4 * e_old, (e_new, e_old)


def test_r0_parts_reproduce_the_concat_conv():
    """The four blocks _pack_decoder packs (W0 with the bias; W0+W1, W0+W2, W0+W3 without, summed in fp32), applied to four
    maps of ONE resolution, equal F.conv3d of cat(a0+a1+a2+a3, a1, a2, a3).  The only error is the fp32 rounding of W0+Wj,
    2^-24 relative per weight, over K = 192 products per block: held to 1e-6 of max|ref|."""
    g = torch.Generator().manual_seed(3)
    a = [torch.randn(2, 192, 2, 5, 7, generator=g) for _ in range(4)]
    w = torch.randn(192, 768, generator=g) / 768 ** 0.5
    b = torch.randn(192, generator=g)
    parts = _parts(w, b)
    assert [tuple(p[0].shape) for p in parts] == [(192, 192)] * 4 and all(p[0].dtype == torch.float32 for p in parts)
    assert torch.equal(parts[0][0], w[:, :192]) and torch.equal(parts[0][1], b) and all(p[1] is None for p in parts[1:])
    for j in (1, 2, 3):
        assert torch.equal(parts[j][0], w[:, :192] + w[:, 192 * j:192 * (j + 1)])
    a64 = [v.double() for v in a]
    ref = F.conv3d(torch.cat([a64[0] + a64[1] + a64[2] + a64[3]] + a64[1:], 1), w.double()[:, :, None, None, None], b.double())
    got = sum(F.conv3d(x, p[0].double()[:, :, None, None, None], None if p[1] is None else p[1].double()) for x, p in zip(a64, parts))
    _rel_close(got, ref, 1e-6, "composed r0 blocks")


def _sum_call(lib, J, ks, c, ldd=None, lds=None, ptr=4096):
    n = max(J, 1)
    srcs = (C.c_void_p * n)(*([ptr] * n))
    ld = (C.c_int64 * n)(*([c if lds is None else lds] * n))
    kk = (C.c_int32 * n)(*(list(ks) + [1] * n)[:n])
    return lib.mspi_upsample_sum_fwd(srcs, ld, kk, J, C.c_void_p(ptr), c if ldd is None else ldd, 2, 8, 8, c, 1, 0, None)


def test_upsample_sum_refusals():
    """Refused before any launch (no GPU needed), each with its message."""
    from mspi_amd import _lib
    lib = _lib.load()

    def refused(rc, text):
        assert rc != 0
        msg = lib.mspi_last_error().decode()
        assert text in msg, msg

    refused(_sum_call(lib, 0, (), 8), "1 to 3 sources")
    refused(_sum_call(lib, 4, (2, 2, 2, 2), 8), "1 to 3 sources")
    refused(_sum_call(lib, 2, (2, 0), 8), "every factor must be >= 1")
    refused(_sum_call(lib, 1, (3,), 8), "divide Ho and Wo")
    refused(_sum_call(lib, 1, (2,), 6), "multiples of 4")
    refused(_sum_call(lib, 1, (2,), 8, ldd=4), "multiples of 4")           # ld < C
    refused(_sum_call(lib, 1, (2,), 8, lds=4), "multiples of 4")
    refused(_sum_call(lib, 1, (2,), 8, ptr=4100), "16-B aligned")
    refused(lib.mspi_upsample_sum_fwd(None, None, None, 1, None, 8, 2, 8, 8, 8, 1, 0, None), "null argument")


# ---------------------------------------------------------------------------------------------------------------- GPU
SUM_FACTORS = {1: (2,), 2: (2, 4), 3: (2, 4, 8)}
SUM_CASES = [(J, c, acc) for J in (1, 2, 3) for c in (4, 192) for acc in (False, True)]
SUM_BASE = (2, 3, 5, 7)      # N, T and the coarsest source's H, W: odd extents, several workgroups at C = 192


def _slab(E, t5, dev, left, right):
    """NCDHW cpu tensor -> columns [left, left + C) of a wider buffer whose other columns hold BIG."""
    N, Cc, T, H, W = t5.shape
    wide = E.alloc(N, T, H, W, left + Cc + right, dev, ld=left + Cc + right)
    wide.buf.fill_(BIG)
    view = wide.slice(left, Cc)
    view.as_ncdhw().copy_(t5.to(dev))
    return wide, view


def _outside(wide, left, Cc):
    rows = wide.buf.view(-1, wide.ld)
    return torch.cat([rows[:, :left].reshape(-1), rows[:, left + Cc:].reshape(-1)])


@pytest.mark.gpu
@pytest.mark.parametrize("J,c,acc", SUM_CASES, ids=["J%d-C%d-acc%d" % (J, c, acc) for J, c, acc in SUM_CASES])
def test_upsample_sum_equals_the_chain_and_fp64(dev, J, c, acc):
    """Sources and destination as channel slabs of wider buffers; = and +=; no activation and ReLU.  Bit-equal to the chain of
    E.upsample(..., accumulate=True) launches, 1e-5 of max|ref| against fp64, columns outside the slab untouched."""
    from mspi_amd import engine as E
    _guard(E, dev)
    n, t, h, w = SUM_BASE
    ks = SUM_FACTORS[J]
    kmax = ks[-1]
    g = torch.Generator().manual_seed(100 * J + c + int(acc))
    srcs = [torch.randn(n, c, t, h * kmax // k, w * kmax // k, generator=g) for k in ks]
    base = torch.randn(n, c, t, h * kmax, w * kmax, generator=g)
    ref = sum(_up(s.double(), k) for s, k in zip(srcs, ks))
    if acc:
        ref = base.double() + ref
    dsrc = [_slab(E, s, dev, 8, 4)[1] for s in srcs]
    for act in (E.ACT_NONE, E.ACT_RELU):
        r = F.relu(ref) if act == E.ACT_RELU else ref
        wide, dst = _slab(E, base if acc else torch.full_like(base, NAN), dev, c, 12)
        wide2, chain = _slab(E, base if acc else torch.full_like(base, NAN), dev, c, 12)
        assert dst.ld > dst.C and all(s.ld > s.C for s in dsrc)
        E.upsample_sum(dst, list(zip(dsrc, ks)), accumulate=acc, act=act)
        for j, (s, k) in enumerate(zip(dsrc, ks)):
            E.upsample(s, k, dst=chain, accumulate=acc if j == 0 else True, act=act if j == J - 1 else E.ACT_NONE)
        what = "upsample_sum J=%d C=%d acc=%d act=%d" % (J, c, acc, act)
        assert torch.equal(dst.as_ncdhw(), chain.as_ncdhw()), what + ": differs from the chain of accumulate launches"
        _rel_close(dst.as_ncdhw(), r, TOL, what)
        assert (_outside(wide, c, c) == BIG).all(), what + ": wrote outside its channel slab"
        print("%s: error %.2e of max|ref|" % (what, _relerr(dst.as_ncdhw().cpu(), r)))


@pytest.mark.gpu
def test_decoder_tail_rewrite_on_against_off(dev, monkeypatch):
    """The whole model with the rewritten tail against the original sequence, same weights and inputs: the maps are
    log-probabilities (parity bar 1e-3); the two orders agree within 1e-5 absolute."""
    from mspi_amd import engine as E
    from mspi_amd import testing as T
    from mspi_amd.model import model_utils as MU
    from mspi_amd.model.model_utils import AudioVisualSaliencyModel
    _guard(E, dev)
    size, B = 64, 2
    cfg = T.make_cfg("x3dl", num_aud_tokens=36, num_vis_tokens=16 * (size // 32) ** 2)
    model = T.seeded(lambda: AudioVisualSaliencyModel(cfg), 0).to(dev)
    clips, audio = T.synth_inputs(B, 16, size, size, Wa=111, seed=0)
    clips, audio = clips.to(dev), audio.to(dev)
    maps = {}
    for on in (True, False):
        monkeypatch.setattr(MU, "DECODER_FUSED", on)
        out, _ = model(clips, audio)
        maps[on] = out.clone()
    torch.cuda.synchronize()
    assert not E.range_flag()
    err = (maps[True] - maps[False]).abs().max().item()
    print("decoder tail rewrite on against off: max abs difference %.2e (map range %.2f .. %.2f)"
          % (err, maps[False].min().item(), maps[False].max().item()))
    assert torch.isfinite(maps[True]).all() and err <= 1e-5, err


# ------------------------------------------------------------------------------------------------- halo-staged conv kernel
F16X3, F32 = 1, 0
ACTS = (0, 1, 2, 3, 4)      # none, ReLU, GELU (erf), sigmoid, swish
# code = kT * 1000 + BN -> (Cin, Cout) rows run on the GPU.  Cout 44 / 204: a partial column tile (204: two tiles of 192);
# Cin 32 / 192: one and six channel chunks; Cout 96: the 128-column instantiation.
HALO_LEDGER = {
    1064: ((32, 44), (192, 44)),
    1128: ((32, 96),),
    1192: ((32, 204), (192, 204)),
    3064: ((32, 44), (192, 44)),
    3128: ((32, 96),),
    3192: ((32, 204), (192, 204)),
}
# N = 2 (a brick must not cross a sample); (T, H, W) ragged in every brick dimension (4 x 8 x 8), T below the brick depth,
# more than one brick along H
HALO_GEOMS = ((3, 9, 11), (1, 5, 7), (4, 17, 9))
HALO_CASES = [(code, cc, co, g) for code in sorted(HALO_LEDGER) for cc, co in HALO_LEDGER[code] for g in HALO_GEOMS]


def _halo_desc(N, T, H, W, Cc, Co, kT, ld=None, k=None, s=(1, 1, 1), p=None, prec=F16X3, sC=1, ldy=None, ldr=0, act=0):
    from mspi_amd import _lib
    d = _lib.ConvDesc()
    k = (kT, 3, 3) if k is None else k
    p = (k[0] // 2, k[1] // 2, k[2] // 2) if p is None else p
    ld = Cc if ld is None else ld
    d.N, d.T, d.H, d.W, d.C = N, T, H, W, Cc
    if sC == 1:
        d.sN, d.sT, d.sH, d.sW, d.sC = T * H * W * ld, H * W * ld, W * ld, ld, 1
    else:      # NCDHW
        d.sN, d.sC, d.sT, d.sH, d.sW = Cc * T * H * W, T * H * W, H * W, W, 1
    d.kT, d.kH, d.kW = k
    d.strT, d.strH, d.strW = s
    d.padT, d.padH, d.padW = p
    d.To, d.Ho, d.Wo = ((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip((T, H, W), k, s, p))
    d.Cout = Co
    d.ldy, d.ldw, d.ldr = (Co if ldy is None else ldy), k[0] * k[1] * k[2] * Cc, ldr
    d.act, d.prec, d.w_scale, d.tile = act, prec, 1.0, -1
    d.w_blocked = 4096      # the queries look at it for NULL and alignment only
    return d


def _halo_code(d, x=4096):
    from mspi_amd import _lib
    return _lib.load().mspi_conv_halo_variant(C.byref(d), x)


@pytest.mark.parametrize("code", sorted(HALO_LEDGER))
def test_halo_ledger_row_selects_its_kernel(code):
    for cc, co in HALO_LEDGER[code]:
        for t, h, w in HALO_GEOMS:
            assert _halo_code(_halo_desc(2, t, h, w, cc, co, code // 1000)) == code
            assert _halo_code(_halo_desc(2, t, h, w, cc, co, code // 1000, ld=cc + 12), 4096 + 32) == code      # a channel slab


def test_halo_ledger_covers_every_reachable_kernel():
    """kT x C x Cout x layout x stride x pad: whatever the query accepts is a ledger code, and every ledger code is reached."""
    from mspi_amd import _lib
    lib = _lib.load()
    seen = set()
    for kT, cc, co, layout, st, pad in itertools.product((1, 3), (32, 64, 96, 192, 20), (4, 44, 64, 68, 128, 132, 192, 204, 400),
                                                         ("dense", "slab", "ncdhw"), (1, 2), ("same", "none")):
        d = _halo_desc(2, 4, 9, 11, cc, co, kT, ld=cc + 8 if layout == "slab" else None, s=(1, st, st),
                       p=None if pad == "same" else (0, 0, 0), sC=1 if layout != "ncdhw" else 0)
        code = _halo_code(d)
        assert lib.mspi_conv_halo_supported(C.byref(d)) == (1 if code > 0 else 0)
        if code < 0:
            assert st == 2 or pad == "none" or cc == 20 or layout == "ncdhw", (kT, cc, co, layout, st, pad)
            continue
        assert code in HALO_LEDGER, "halo code %d has no ledger row" % code
        assert code == kT * 1000 + (64 if co <= 64 else 128 if co <= 128 else 192)
        seen.add(code)
    assert seen == set(HALO_LEDGER)


def test_halo_refusals():
    from mspi_amd import _lib
    lib = _lib.load()

    def refused(d, text, x=4096):
        assert _halo_code(d, x) == -1
        msg = lib.mspi_last_error().decode()
        assert text in msg, msg

    ok = dict(N=2, T=4, H=9, W=11, Cc=64, Co=64, kT=3)
    assert _halo_code(_halo_desc(**ok)) == 3064
    refused(_halo_desc(**ok, s=(1, 2, 2)), "stride (1,2,2) is not 1")
    refused(_halo_desc(**{**ok, "Cc": 20}), "C = 20 is not a multiple of 32")
    refused(_halo_desc(**ok, sC=0), "channels-last input only")
    refused(_halo_desc(**ok), "16-B aligned", x=4100)
    refused(_halo_desc(**ok, k=(3, 5, 5)), "kernel (3,5,5) is not (1|3,3,3)")
    refused(_halo_desc(**ok, k=(5, 3, 3)), "kernel (5,3,3) is not (1|3,3,3)")
    refused(_halo_desc(**ok, prec=F32), "f16x3 only")
    refused(_halo_desc(**ok, p=(0, 1, 1)), "pad (0,1,1) is not (kT/2,1,1)")
    d = _halo_desc(**ok)
    d.w_blocked = None
    refused(d, "blocked weight planes")
    # a gate is refused by the launch itself, before anything reaches the GPU
    d = _halo_desc(**ok)
    assert lib.mspi_conv_halo_fwd(C.byref(d), 4096, None, None, 4096, 4096, None) != 0
    assert "no gate" in lib.mspi_last_error().decode()


def _halo_run(E, lib, dev, geom, cc, co, kT, acts, code=None):
    """One conv through mspi_conv_halo_fwd: (a) slab input fenced with NaN rows, slab output, residual with ldr > Cout, act
    acts[0]; (b) the same input, dense output, no residual, act acts[1].  Returns the operands for further comparisons."""
    N = 2
    T, H, W = geom
    g = torch.Generator().manual_seed(kT * 100000 + cc * 1000 + co + T * 7 + H)
    x = torch.randn(N, cc, T, H, W, generator=g)
    w = torch.randn(co, cc, kT, 3, 3, generator=g) / math.sqrt(cc * kT * 9)
    b = torch.randn(co, generator=g)
    ref = F.conv3d(x.double(), w.double(), b.double(), 1, (kT // 2, 1, 1)).permute(0, 2, 3, 4, 1).reshape(-1, co)
    M = ref.shape[0]
    res = torch.randn(M, co + 8, generator=g)
    pk = E.pack_conv(w, b, None, (1, 1, 1), (kT // 2, 1, 1), device=dev)
    assert pk.cout_s == co and pk.prec == F16X3
    # input: columns [8, 8 + C) of rows C + 12 wide (the others hold 1e3); a plane of NaN rows before the first sample and
    # after every sample, so that a halo read outside the frame is NaN and not luck
    ld, plane, rows = cc + 12, H * W, T * H * W
    buf = torch.full(((N * (rows + plane) + plane), ld), NAN, device=dev)
    xs = x.permute(0, 2, 3, 4, 1).reshape(N, rows, cc).to(dev)
    for n in range(N):
        r0 = plane + n * (rows + plane)
        buf[r0:r0 + rows] = BIG
        buf[r0:r0 + rows, 8:8 + cc] = xs[n]
    xp = buf.data_ptr() + 4 * (plane * ld + 8)

    def run(act, with_res, ldy):
        y = torch.full((M, ldy), -3.0, device=dev)
        c0 = 4 if ldy > co else 0
        rd = res.to(dev) if with_res else None
        d = _halo_desc(N, T, H, W, cc, co, kT, ld=ld, ldy=ldy, ldr=co + 8 if with_res else 0, act=act)
        d.sN = (rows + plane) * ld
        d.w_scale = pk.w_scale
        assert d.ldw == pk.ldw
        d.w_blocked = E.sp_weights(pk).data_ptr()
        if code is not None:
            assert lib.mspi_conv_halo_variant(C.byref(d), xp) == code
        E.check(lib.mspi_conv_halo_fwd(C.byref(d), xp, pk.bias.data_ptr(), rd.data_ptr() if rd is not None else None, None,
                                       y.data_ptr() + 4 * c0, E._stream()), "mspi_conv_halo_fwd")
        torch.cuda.synchronize()
        return y.cpu(), c0

    what = "conv_halo kT=%d %d->%d on %s" % (kT, cc, co, geom)
    y, c0 = run(acts[0], True, co + 12)
    want = _act64(ref + res[:, :co].double(), acts[0])
    print("%s act %d + res: error %.2e of max|ref|" % (what, acts[0], _relerr(y[:, c0:c0 + co], want)))
    _rel_close(y[:, c0:c0 + co], want, TOL, what + " act %d + res" % acts[0])
    assert (y[:, :c0] == -3.0).all() and (y[:, c0 + co:] == -3.0).all(), what + ": wrote outside its output slab"
    y1, _ = run(acts[1], False, co)
    want = _act64(ref, acts[1])
    print("%s act %d: error %.2e of max|ref|" % (what, acts[1], _relerr(y1, want)))
    _rel_close(y1, want, TOL, what + " act %d" % acts[1])
    return pk, buf, xp, ld, (rows + plane) * ld, ref, y1


def _act64(v, a):
    return (v, v.clamp_min(0), F.gelu(v), torch.sigmoid(v), v * torch.sigmoid(v))[a]


@pytest.mark.gpu
@pytest.mark.parametrize("code,cc,co,geom", HALO_CASES, ids=["%d-C%d-Co%d-%dx%dx%d" % ((c, a, b) + g) for c, a, b, g in HALO_CASES])
def test_halo_ledger_kernel_vs_fp64(dev, code, cc, co, geom):
    from mspi_amd import engine as E
    lib = E._lib.load()
    _guard(E, dev)
    i = HALO_CASES.index((code, cc, co, geom))
    _halo_run(E, lib, dev, geom, cc, co, code // 1000, (ACTS[i % 5], ACTS[(i + 2) % 5]), code)
    torch.cuda.synchronize()
    assert not E.range_flag()


@pytest.mark.gpu
def test_halo_matches_the_tap_major_kernel_at_the_readout_widths(dev):
    """192 -> 192, 3x3x3, on (4,14,14): against fp64 as above, and against mspi_conv_fwd's own choice (tile -1) on the same
    operands at 2e-5 of max|ref| (two fp32-accurate sums in different orders)."""
    from mspi_amd import engine as E
    lib = E._lib.load()
    _guard(E, dev)
    geom, cc, co = (4, 14, 14), 192, 192
    pk, buf, xp, ld, sN, ref, y_halo = _halo_run(E, lib, dev, geom, cc, co, 3, (1, 0), 3192)
    T, H, W = geom
    d = _halo_desc(2, T, H, W, cc, co, 3, ld=ld)
    d.sN, d.w_scale, d.tile = sN, pk.w_scale, -1
    d.w_blocked = E.sp_weights(pk).data_ptr()
    y = torch.full((ref.shape[0], co), -3.0, device=dev)
    E.check(lib.mspi_conv_fwd(C.byref(d), xp, pk.w.data_ptr(), pk.bias.data_ptr(), None, None, y.data_ptr(), E._stream()), "mspi_conv_fwd")
    torch.cuda.synchronize()
    _rel_close(y_halo, y.cpu(), 2e-5, "conv_halo against mspi_conv_fwd")
    assert not E.range_flag()
