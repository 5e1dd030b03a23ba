"""Weight packs on the CPU (mspi_amd/packs.py): every fragment layout against a restatement in plain index loops, written
from the sentence that states the layout (the function's docstring, include/mspi_hip.h, `plane_off` of csrc/common.h), and
pack_conv's folds, tap order, pre-scale and f16 split.  Seeded weights; every layout comparison is bit equality."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

U = 2.0 ** -24      # unit roundoff of fp32


def _rnd(seed, *shape):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 0.5


def _bits(a):
    a = a.detach().cpu().contiguous().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same_bits(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _split(ws):
    """(hi, lo) of a float32 array: hi = f16(ws), lo = f16(ws - f32(hi))."""
    hi = ws.astype(np.float16)
    return hi, (ws - hi.astype(np.float32)).astype(np.float16)


def _pad(w, rows, cols):
    out = np.zeros((rows, cols), np.float32)
    out[:w.shape[0], :w.shape[1]] = w
    return out


def _scaled(pk):
    """The scaled weight a fused pack is built from: f32(hi) + f32(lo) of the conv pack's planes."""
    w = pk.w.numpy()
    return w[0].astype(np.float32) + w[1].astype(np.float32)


def _conv1(co, ci, seed, cin_stored=None):
    """A packed 1x1x1 conv + bias + ReLU, the form X3D's `a` and `c` convs take."""
    from mspi_amd import packs as P
    return P.pack_conv(_rnd(seed, co, ci, 1, 1, 1), _rnd(seed + 1, co), act=P.ACT_RELU, cin_stored=cin_stored)


# ------------------------------------------------------------------------------- restatements
def first_layer_restated(ws):
    """[chunk j][k-step s][hi,lo][lane l][e] = Ws[32 j + l % 32][16 s + 8 (l / 32) + e]"""
    halves = _split(ws)
    n, k = ws.shape
    out = np.zeros((n // 32, k // 16, 2, 64, 8), np.float16)
    for j in range(n // 32):
        for s in range(k // 16):
            for p in range(2):
                for l in range(64):
                    for e in range(8):
                        out[j, s, p, l, e] = halves[p][32 * j + l % 32, 16 * s + 8 * (l // 32) + e]
    return out


def second_layer_restated(ws, nch):
    """[chunk j][s < 2][tile t][hi,lo][lane l][e] = Ws[32 t + l % 32][32 j + (2 s + e / 4) 8 + 4 (l / 32) + e % 4]"""
    halves = _split(ws)
    ct = ws.shape[0] // 32
    out = np.zeros((nch, 2, ct, 2, 64, 8), np.float16)
    for j in range(nch):
        for s in range(2):
            for t in range(ct):
                for p in range(2):
                    for l in range(64):
                        for e in range(8):
                            out[j, s, t, p, l, e] = halves[p][32 * t + l % 32, 32 * j + (2 * s + e // 4) * 8 + 4 * (l // 32) + e % 4]
    return out


def two_layer_restated(w1s, w2s):
    """mspi_mlp_fwd's operand: per chunk of 32 hidden units its W1 part, then its W2 part."""
    nch = w1s.shape[0] // 32
    a, b = first_layer_restated(w1s), second_layer_restated(w2s, nch)
    return np.stack([np.concatenate([a[j].reshape(-1), b[j].reshape(-1)]) for j in range(nch)])


def x3d_ab_restated(ws):
    """[chunk][k32 step][16-row half][hi,lo][lane l][e] = W[chunk*32 + half*16 + (l & 15)][32*step + 8*(l >> 4) + e]"""
    halves = _split(ws)
    n, k = ws.shape
    out = np.zeros((n // 32, k // 32, 2, 2, 64, 8), np.float16)
    for j in range(n // 32):
        for s in range(k // 32):
            for h in range(2):
                for p in range(2):
                    for l in range(64):
                        for e in range(8):
                            out[j, s, h, p, l, e] = halves[p][j * 32 + h * 16 + (l & 15), 32 * s + 8 * (l >> 4) + e]
    return out


def plane_off(m, k, kt):
    return ((m >> 4) * kt + (k >> 5)) * 512 + (m & 15) * 32 + (k & 31)


def f16_scale_restated(w):
    mx = float(np.abs(w).max())
    return 2.0 ** max(-10, min(24, math.floor(math.log2(16384.0 / mx))))


# ------------------------------------------------------------------------------- rowgemm
@pytest.mark.parametrize("k_s,n_s,ksb", [(24, 56, 2), (200, 36, 14)])
def test_rowgemm_fragment_order(k_s, n_s, ksb):
    from mspi_amd import packs as P
    pk = _conv1(n_s, k_s, 100 + k_s)
    assert P.rowgemm_ksb(k_s) == ksb and pk.thin is not None and pk.thin.dtype == torch.float16
    ws = pk.w32.numpy()[:, :k_s] * np.float32(pk.w_scale)
    assert _same_bits(pk.thin, first_layer_restated(_pad(ws, (n_s + 31) // 32 * 32, ksb * 16)))


def test_rowgemm_is_not_packed_beyond_224_columns():
    from mspi_amd import packs as P
    assert _conv1(36, 232, 110).thin is None and not P.rowgemm_supported(232, 36)


# ------------------------------------------------------------------------------- fused X3D a + b
def _ab_layers(cin_s, co, stride=(1, 1, 1), seed=200):
    from mspi_amd import packs as P
    pa = _conv1(co, cin_s, seed + cin_s)
    pb = P.pack_dwconv(_rnd(seed + 2, co, 1, 3, 3, 3), _rnd(seed + 3, co), stride=stride, pad=(1, 1, 1))
    return pa, pb


@pytest.mark.parametrize("cin_s,co,cout_s,ks", [(24, 54, 56, 1), (168, 36, 36, 6)])
def test_x3d_ab_fragment_order(cin_s, co, cout_s, ks):
    from mspi_amd import packs as P
    pa, pb = _ab_layers(cin_s, co)
    p = P.pack_x3d_ab(pa, pb)
    assert pa.cout_s == cout_s and (p.cin_s, p.cmid, p.cmid_s, p.wa_scale) == (cin_s, co, cout_s, pa.w_scale)
    assert p.ba is pa.bias and p.wb is pb.w and p.bb is pb.bias
    assert _same_bits(p.wa, x3d_ab_restated(_pad(_scaled(pa)[:, :cin_s], (cout_s + 31) // 32 * 32, ks * 32)))
    assert P.pack_x3d_ab_s2(pa, pb) is None                 # a stride-1 `b` is not the stride-2 kernel's


def test_x3d_ab_refuses_four_k_steps():
    from mspi_amd import packs as P
    assert P.pack_x3d_ab(*_ab_layers(104, 36)) is None
    assert P.pack_x3d_ab_s2(*_ab_layers(104, 36, stride=(1, 2, 2))) is None


def test_x3d_ab_s2_is_the_same_pack_from_a_stride_2_b():
    from mspi_amd import packs as P
    pa, pb = _ab_layers(24, 54, stride=(1, 2, 2))
    p = P.pack_x3d_ab_s2(pa, pb)
    assert _same_bits(p.wa, x3d_ab_restated(_pad(_scaled(pa)[:, :24], 64, 32))) and p.wb is pb.w and pb.stride == (1, 2, 2)
    assert P.pack_x3d_ab(pa, pb) is None


# ------------------------------------------------------------------------------- fused X3D c + next a
@pytest.mark.parametrize("d,d_s,cx_s,c", [(54, 56, 24, 128), (216, 216, 96, 224)])
def test_x3d_ca_is_the_two_layer_order(d, d_s, cx_s, c):
    from mspi_amd import packs as P
    pc, pa = _conv1(cx_s, d, 300 + d, cin_stored=d_s), _conv1(d, cx_s, 310 + d)
    p = P.pack_x3d_ca(pc, pa)
    hid = (cx_s + 31) // 32 * 32
    assert (p.d, p.d_s, p.cx, p.cx_s, p.wc_scale, p.wa_scale) == (d, d_s, cx_s, cx_s, pc.w_scale, pa.w_scale)
    assert p.bc is pc.bias and p.ba is pa.bias
    assert _same_bits(p.w, two_layer_restated(_pad(_scaled(pc)[:, :d_s], hid, c), _pad(_scaled(pa)[:, :cx_s], c, hid)))


# ------------------------------------------------------------------------------- fused MLP
@pytest.mark.parametrize("c,hidden,gamma", [(96, 64, True), (192, 32, False)])
def test_mlp_is_the_two_layer_order(c, hidden, gamma):
    from mspi_amd import packs as P
    w1, b1, w2, b2 = _rnd(400, hidden, c), _rnd(401, hidden), _rnd(402, c, hidden), _rnd(403, c)
    g = _rnd(404, c) if gamma else None
    p = P.pack_mlp(w1, b1, w2, b2, out_scale=g)
    w2g, b2g = (w2.numpy() * g.numpy()[:, None], b2.numpy() * g.numpy()) if gamma else (w2.numpy(), b2.numpy())
    assert (p.c, p.hidden) == (c, hidden)
    assert (p.s1, p.s2) == (f16_scale_restated(w1.numpy()), f16_scale_restated(w2g))
    assert _same_bits(p.b1, b1.numpy()) and _same_bits(p.b2, b2g)            # gamma reaches fc2 and b2 only
    assert _same_bits(p.w, two_layer_restated(w1.numpy() * np.float32(p.s1), w2g * np.float32(p.s2)))


# ------------------------------------------------------------------------------- blocked planes
def test_sp_weights_follow_plane_off():
    from mspi_amd import packs as P
    pk = P.pack_conv(_rnd(500, 54, 64), _rnd(501, 54))
    assert (pk.cout_s, pk.ldw) == (56, 64)
    wsp = P.sp_weights(pk)
    assert wsp.dtype == torch.float16 and wsp.numel() == 2 * 64 * 64 and wsp.is_contiguous() and P.sp_weights(pk) is wsp
    got, src = _bits(wsp).reshape(2, -1), _bits(pk.w)
    want = np.full_like(got, 0xFFFF)
    for p in range(2):
        for m in range(64):
            for k in range(64):
                want[p, plane_off(m, k, 64 // 32)] = src[p, m, k] if m < 56 else 0
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------- pack_conv
@pytest.fixture(scope="module")
def folded():
    """A (2,3,3) conv 5 -> 6 channels, stored input channels 8, with BatchNorm and an output scale."""
    from mspi_amd import packs as P
    from mspi_amd import testing as T
    w, b, g = _rnd(600, 6, 5, 2, 3, 3), _rnd(601, 6), _rnd(602, 6) + 1.0
    bn = T.randomize_(nn.BatchNorm3d(6), 7).eval()
    pk = P.pack_conv(w, b, bn=bn, stride=(1, 2, 2), pad=(0, 1, 1), cin_stored=8, out_scale=g)
    return {"w": w, "b": b, "g": g, "bn": bn, "pk": pk}


def test_pack_conv_tap_order_and_padding():
    from mspi_amd import packs as P
    w = _rnd(610, 6, 5, 2, 3, 3)
    pk = P.pack_conv(w, None, cin_stored=8)
    K = 2 * 3 * 3 * 8
    assert (pk.cin, pk.cin_s, pk.cout, pk.cout_s, pk.k, pk.ldw, pk.ldw32, pk.bias) == (5, 8, 6, 8, (2, 3, 3), 160, K, None)
    want = np.zeros((8, K), np.float32)
    for o in range(6):
        for ci in range(5):
            for t in range(2):
                for h in range(3):
                    for x in range(3):
                        want[o, ((t * 3 + h) * 3 + x) * 8 + ci] = w[o, ci, t, h, x]
    assert _same_bits(pk.w32, want)                                          # w32: the unscaled padded weight


def test_pack_conv_folds_bn_and_out_scale(folded):
    w, b, g, bn, pk = (folded[k] for k in ("w", "b", "g", "bn", "pk"))
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    ref = (w.double() * s.view(-1, 1, 1, 1, 1) * g.double().view(-1, 1, 1, 1, 1)).permute(0, 2, 3, 4, 1)
    got = pk.w32[:6].view(6, 2, 3, 3, 8)[..., :5].double()
    # s: var + eps, sqrt, divide = 2.5 U; times w, times g: 4.5 U to first order
    assert bool(((got - ref).abs() <= 6 * U * ref.abs()).all())
    terms = (bn.bias.detach().double().abs() + (bn.running_mean.double() * s).abs() + (b.double() * s).abs()) * g.double().abs()
    bref = (bn.bias.detach().double() - bn.running_mean.double() * s + b.double() * s) * g.double()
    assert bool(((pk.bias[:6].double() - bref).abs() <= 8 * U * terms).all()) and float(pk.bias[6:].abs().max()) == 0.0


def test_pack_conv_scale_and_split(folded):
    pk = folded["pk"]
    wf = _pad(pk.w32.numpy(), 8, pk.ldw)
    assert math.frexp(pk.w_scale)[0] == 0.5 and 2.0 ** 13 <= float(np.abs(wf).max()) * pk.w_scale < 2.0 ** 14
    ws = wf * np.float32(pk.w_scale)
    hi, lo = pk.w.numpy()
    assert pk.w.dtype == torch.float16 and pk.w.shape == (2, 8, pk.ldw)
    assert np.array_equal(_bits(hi), _bits(ws.astype(np.float16)))
    assert np.array_equal(_bits(lo), _bits((ws - hi.astype(np.float32)).astype(np.float16)))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_pack_conv_refuses_non_finite_weights(bad):
    from mspi_amd import packs as P
    w = _rnd(620, 8, 8)
    w[3, 2] = bad
    with pytest.raises(P.MspiError):
        P.pack_conv(w)


# ------------------------------------------------------------------------------- import surface
MOVED = ["rup4", "fold_bn", "DEFAULT_PREC", "PackedConv", "pack_conv", "PackedDw", "pack_dwconv", "rowgemm_ksb",
         "rowgemm_supported", "_pack_rowgemm", "PackedMlp", "mlp_supported", "pack_mlp", "pack_mlp_tail", "PackedX3dAb",
         "pack_x3d_ab", "pack_x3d_ab_s2", "PackedX3dStem", "pack_x3d_stem", "PackedX3dCa", "x3d_ca_supported", "pack_x3d_ca",
         "sp_weights", "_pad_vec", "SP_ENABLED", "sp_supported"]


def test_engine_keeps_its_names():
    from mspi_amd import engine as E
    from mspi_amd import packs as P
    assert len(set(E.__all__)) == len(E.__all__) and all(hasattr(E, n) for n in E.__all__)
    assert all(getattr(E, n) is getattr(P, n) for n in MOVED)
    assert all(getattr(v, "__name__", "") != "mspi_amd.engine" for v in vars(P).values())      # packs stands below engine
