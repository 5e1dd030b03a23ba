"""Weight packing, the one place that turns parameters into kernel operands: eval-mode BatchNorm folded in, taps channel-minor,
channels padded to a multiple of 4 and, for f16x3, the power-of-two pre-scale (`f16_scale`), the hi/lo split (`split_f16`) and
one function per order a kernel reads the halves in (`frag_*`, `blocked_planes`; tests/test_packs.py restates each).  Host only."""
import math
import os

import torch

from ._lib import ACT_GELU, ACT_NONE, ACT_RELU, PREC_F16X3, PREC_F32, MspiError

# GEMM arithmetic for every dense conv / Linear: "f16x3" (default; fp32-accurate split product on the f16 matrix
# pipe, see include/mspi_hip.h) or "f32" (v_mfma_f32_32x32x2_f32).  Read when weights are packed.
DEFAULT_PREC = {"f32": PREC_F32, "f16x3": PREC_F16X3}[os.environ.get("MSPI_GEMM_PREC", "f16x3")]
SP_ENABLED = os.environ.get("MSPI_PRESPLIT", "1") != "0"   # A/B switch: pre-split activations between LN / GEMM / GEMM


def rup4(c):
    return (c + 3) // 4 * 4


def sp_supported(c):
    """Channel counts the pre-split GEMM takes as its K: multiples of the 32-deep stage (then ldw == K)."""
    return SP_ENABLED and DEFAULT_PREC == PREC_F16X3 and c % 32 == 0


def fold_bn(weight, bias, bn):
    """Fold an eval-mode BatchNorm (running stats) into the preceding conv: returns (w, b)."""
    w = weight.detach().float()
    b = None if bias is None else bias.detach().float()
    if bn is not None:
        s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        w = w * s.view(-1, *([1] * (w.dim() - 1)))
        b0 = bn.bias.detach().float() - bn.running_mean.detach().float() * s
        b = b0 if b is None else b0 + b * s
    return w, b


def _pad_vec(v, n):
    out = torch.zeros(n, dtype=torch.float32, device=v.device)
    out[: v.numel()] = v.detach().float().view(-1)
    return out


def f16_scale(w):
    """The power of two that puts max|w| in [2^13, 2^14): the lo halves of typical weights are then normal f16."""
    mx = float(w.abs().max())
    if not math.isfinite(mx):
        raise MspiError("pack: non-finite weights")
    e = 0 if mx == 0.0 else max(-10, min(24, int(math.floor(math.log2(16384.0 / mx)))))
    return float(2.0 ** e)


def split_f16(ws):
    """Scaled fp32 weights -> (hi, lo) f16 halves: hi = f16(ws), lo = f16(ws - f32(hi))."""
    hi = ws.to(torch.float16)
    return hi, (ws - hi.float()).to(torch.float16)


def _padded(w, rows, cols):
    """The fp32 matrix w in the top-left corner of a zero [rows, cols] host matrix."""
    out = torch.zeros(rows, cols, dtype=torch.float32)
    out[: w.shape[0], : w.shape[1]] = w.cpu()
    return out


def _scaled(pk, cols):
    """The first `cols` columns of the scaled fp32 weight of an f16x3 PackedConv: hi + lo is its 22 bits."""
    return (pk.w[0].float() + pk.w[1].float()).cpu()[:, :cols]


def _frag(ws, view, perm, shape):
    """Both halves of ws as view -> permute -> reshape, the plane axis (0: hi, 1: lo) in front of [lane][e]."""
    return torch.stack([pl.view(view).permute(perm).reshape(shape) for pl in split_f16(ws)], -3)


# ----------------------------------------------------------------------------- fragment layouts: plane 0 = hi, 1 = lo
def frag_k16(ws):
    """First-layer order, "32 outputs x k16 steps" (mspi_rowgemm_fwd, W1 of mspi_mlp_fwd, the `c` conv of mspi_x3d_ca_fwd).
    ws: fp32 [n, k], n % 32 == 0, k % 16 == 0.  Result f16 [n/32][k/16][2][64][8]:
    element e of lane l of plane p of k-step s of chunk j = half p of ws[32 j + l % 32][16 s + 8 (l / 32) + e]."""
    n, k = ws.shape
    return _frag(ws, (n // 32, 32, k // 16, 2, 8), (0, 2, 3, 1, 4), (n // 32, k // 16, 64, 8))


def frag_second(ws, nch):
    """Second-layer order (W2 of mspi_mlp_fwd, the `a` conv of mspi_x3d_ca_fwd), the contraction over the first layer's nch
    chunks of 32 outputs in two steps of 16.  ws: fp32 [c, 32 nch], c % 32 == 0.  Result f16 [nch][2][c/32][2][64][8]: element e of
    lane l of plane p of tile t of step s of chunk j = half p of ws[32 t + l % 32][32 j + 16 s + 8 (e / 4) + 4 (l / 32) + e % 4]."""
    ct = ws.shape[0] // 32
    return _frag(ws, (ct, 32, nch, 2, 2, 2, 4), (2, 3, 0, 5, 1, 4, 6), (nch, 2, ct, 64, 8))


def frag_x3d_ab(ws):
    """The order of mspi_x3d_ab_fwd / mspi_x3d_ab_s2_fwd: 16-row halves x k32 steps.  ws: fp32 [n, k], n % 32 == 0,
    k % 32 == 0.  Result f16 [n/32][k/32][2][2][64][8]:
    element e of lane l of plane p of half h of k-step s of chunk j = half p of ws[32 j + 16 h + l % 16][32 s + 8 (l / 16) + e]."""
    n, k = ws.shape
    return _frag(ws, (n // 32, 2, 16, k // 32, 4, 8), (0, 3, 1, 4, 2, 5), (n // 32, k // 32, 2, 64, 8))


def blocked_planes(w):
    """The blocked plane order of mspi_gemm_sp_fwd (`plane_off` of csrc/common.h): 16 rows x 32 k = 1 KB contiguous per block,
    blocks k-fastest.  w: [2][n][k] hi / lo planes, n % 16 == 0, k % 32 == 0.  Result [2][n/16][k/32][16][32]:
    element ((m / 16) (k / 32) + c / 32) 512 + 32 (m % 16) + c % 32 of plane p = w[p][m][c]."""
    return w.view(2, w.shape[1] // 16, 16, w.shape[2] // 32, 32).permute(0, 1, 3, 2, 4).contiguous()


class PackedConv:
    __slots__ = ("w", "bias", "k", "stride", "pad", "cin", "cin_s", "cout", "cout_s", "ldw", "act", "prec", "w_scale", "thin",
                 "w32", "ldw32", "checked", "wsp")


def pack_conv(weight, bias=None, bn=None, stride=(1, 1, 1), pad=(0, 0, 0), act=ACT_NONE, cin_stored=None,
              out_scale=None, device=None, prec=None):
    """weight: [Co,Ci] (Linear), [Co,Ci,kh,kw] (2-D) or [Co,Ci,kt,kh,kw].  Result rows are
    [Co_s][ldw] with k = (kt,kh,kw,ci) ci fastest, Ci padded to cin_stored, Co to a multiple of 4."""
    w, b = fold_bn(weight, bias, bn)
    if w.dim() == 2:
        w = w[:, :, None, None, None]
    elif w.dim() == 4:
        w = w[:, :, None]
    if out_scale is not None:  # e.g. ConvNeXt layer-scale gamma folded into the producing conv
        s = out_scale.detach().float().view(-1)
        w = w * s.view(-1, 1, 1, 1, 1)
        b = None if b is None else b * s
    co, ci, kt, kh, kw = w.shape
    cin_s = ci if cin_stored is None else cin_stored
    assert cin_s >= ci
    cout_s = rup4(co) if co > 1 else 1
    K = kt * kh * kw * cin_s
    prec = DEFAULT_PREC if prec is None else prec
    ldw = rup4(K) if prec == PREC_F32 else (K + 31) // 32 * 32
    wp = torch.zeros(cout_s, kt, kh, kw, cin_s, dtype=torch.float32, device=w.device)
    wp[:co, :, :, :, :ci] = w.permute(0, 2, 3, 4, 1)
    wf = torch.zeros(cout_s, ldw, dtype=torch.float32, device=w.device)
    wf[:, :K] = wp.reshape(cout_s, K)
    p = PackedConv()
    p.prec, p.w_scale, p.thin, p.wsp, p.checked = prec, 1.0, None, None, False
    dev = w.device if device is None else device
    if prec == PREC_F16X3:
        p.w_scale = f16_scale(wf)
        ws = wf * p.w_scale
        p.w = torch.stack(split_f16(ws)).to(dev).contiguous()
        p.ldw32 = rup4(K)                                   # the fp32 form, for layers the range check moves off f16x3
        p.w32 = wf[:, :p.ldw32].to(dev).contiguous()
        if (kt, kh, kw) == (1, 1, 1) and tuple(stride) == (1, 1, 1) and tuple(pad) == (0, 0, 0):
            p.thin = _pack_rowgemm(ws[:, :K], cin_s, cout_s, dev)
    else:
        p.w = wf.to(dev).contiguous()
        p.w32, p.ldw32 = p.w, ldw
    p.bias = None if b is None else _pad_vec(b, cout_s).to(dev)
    p.k, p.stride, p.pad = (kt, kh, kw), tuple(stride), tuple(pad)
    p.cin, p.cin_s, p.cout, p.cout_s, p.ldw, p.act = ci, cin_s, co, cout_s, ldw, act
    return p


def sp_weights(pk):
    """The weights of an f16x3 pack in the form mspi_gemm_sp_fwd takes: blocked like the activation planes (rows zero-padded
    to a multiple of 16), so that every LDS-DMA piece of a stage is 8 full cache lines.  Built on first use, kept on the pack."""
    if pk.wsp is None:
        w = torch.zeros(2, (pk.cout_s + 15) // 16 * 16, pk.ldw, dtype=torch.float16, device=pk.w.device)
        w[:, : pk.cout_s] = pk.w
        pk.wsp = blocked_planes(w)
    return pk.wsp


def rowgemm_ksb(k):
    """k-steps of 16 the row-stationary thin GEMM keeps in registers for K stored input columns (0: not covered)."""
    return 2 if k <= 32 else 4 if k <= 64 else 8 if k <= 128 else 14 if k <= 224 else 0


def rowgemm_supported(k, n):
    """Mirror of mspi_rowgemm_supported."""
    return bool(rowgemm_ksb(k)) and 4 <= n <= 1024


def _pack_rowgemm(ws, k_s, n_s, dev):
    """Scaled weights ws [n_s, k_s] -> frag_k16 planes of mspi_rowgemm_fwd; None when the shape is outside the kernel's range."""
    if not rowgemm_supported(k_s, n_s):
        return None
    return frag_k16(_padded(ws, (n_s + 31) // 32 * 32, rowgemm_ksb(k_s) * 16)).contiguous().to(dev)


def _two_layer(w1s, w2s):
    """mspi_mlp_fwd's operand from scaled w1s [hidden, c], w2s [c, hidden]: per 32 hidden units frag_k16(w1s), then frag_second(w2s)."""
    nch = w1s.shape[0] // 32
    return torch.cat([frag_k16(w1s).reshape(nch, -1), frag_second(w2s, nch).reshape(nch, -1)], 1).contiguous()


class PackedMlp:
    __slots__ = ("w", "b1", "b2", "c", "hidden", "s1", "s2", "act", "src", "checked", "fallback")


def mlp_supported(c, hidden):
    """Shapes mspi_mlp_fwd covers (the rows stay in registers as MFMA fragments: C <= 192)."""
    fused = os.environ.get("MSPI_MLP_FUSED", "1") != "0"   # A/B switch
    return fused and DEFAULT_PREC == PREC_F16X3 and c in (96, 192) and hidden % 32 == 0 and hidden <= 1024


def pack_mlp(fc1_w, fc1_b, fc2_w, fc2_b, out_scale=None, act=ACT_GELU, device=None):
    """Fragment-order f16 hi/lo packing of a Linear(C, hidden) -> act -> Linear(hidden, C) pair for mspi_mlp_fwd.
    out_scale (ConvNeXt layer-scale gamma) is folded into the second layer."""
    w1, w2, b2 = (t.detach().float().cpu() for t in (fc1_w, fc2_w, fc2_b))
    if out_scale is not None:
        g = out_scale.detach().float().cpu().view(-1)
        w2, b2 = w2 * g[:, None], b2 * g
    hidden, c = w1.shape
    if w2.shape != (c, hidden) or c % 32 or hidden % 32:
        raise MspiError("pack_mlp: shapes %s / %s" % (tuple(w1.shape), tuple(w2.shape)))
    p = PackedMlp()
    p.s1, p.s2 = f16_scale(w1), f16_scale(w2)
    dev = fc1_w.device if device is None else device
    p.w = _two_layer(w1 * p.s1, w2 * p.s2).to(dev)
    p.b1 = fc1_b.detach().float().contiguous().to(dev)
    p.b2 = b2.contiguous().to(dev)
    p.c, p.hidden, p.act = c, hidden, act
    # first-sight range check (engine.mlp): the layer pair as two GEMM packs, built from these when the check needs them
    p.src, p.checked, p.fallback = (fc1_w, fc1_b, fc2_w, fc2_b, out_scale), False, None
    return p


def pack_mlp_tail(fc1, fc2, out_scale=None):
    """LN -> Linear -> GELU -> Linear (+ residual) tail of a ConvNeXt / Swin / MViT block: the fused kernel where it
    applies (C in {96, 192}, f16x3), else the two GEMM packs.  Use with engine.mlp_tail()."""
    if mlp_supported(fc1.in_features, fc1.out_features) and fc2.out_features == fc1.in_features:
        return ("fused", pack_mlp(fc1.weight, fc1.bias, fc2.weight, fc2.bias, out_scale=out_scale))
    return ("split", pack_conv(fc1.weight, fc1.bias, act=ACT_GELU), pack_conv(fc2.weight, fc2.bias, out_scale=out_scale))


class PackedX3dCa:
    __slots__ = ("w", "bc", "ba", "d", "cx", "cx_s", "d_s", "wc_scale", "wa_scale")


def x3d_ca_supported(d_s, cx_s):
    """Mirror of mspi_x3d_ca_supported."""
    return 4 <= d_s <= 224 and d_s % 4 == 0 and 4 <= cx_s <= 256 and cx_s % 4 == 0


def pack_x3d_ca(pc, pa):
    """Operands of the fused X3D block seam (mspi_x3d_ca_fwd): this block's `c` conv `pc` and the next block's `a` conv `pa`
    (both PackedConv, 1x1x1, f16x3, ReLU), packed as mspi_mlp_fwd's pair with C = the inner width padded to 128 or 224 and
    hidden = the block width padded to 32; None when the pair is outside the kernel's range."""
    ok = all(q.prec == PREC_F16X3 and q.k == (1, 1, 1) and q.stride == (1, 1, 1) and q.pad == (0, 0, 0) and q.act == ACT_RELU
             and q.bias is not None for q in (pc, pa))
    if not ok or pc.cout_s != pa.cin_s or pc.cin_s != pa.cout_s or not x3d_ca_supported(pc.cin_s, pc.cout_s):
        return None
    d_s, cx_s = pc.cin_s, pc.cout_s
    c, hid = 128 if d_s <= 128 else 224, (cx_s + 31) // 32 * 32
    p = PackedX3dCa()
    p.w = _two_layer(_padded(_scaled(pc, d_s), hid, c), _padded(_scaled(pa, cx_s), c, hid)).to(pc.w.device)
    p.bc, p.ba = pc.bias, pa.bias
    p.d, p.d_s, p.cx, p.cx_s, p.wc_scale, p.wa_scale = pc.cin, d_s, pc.cout, cx_s, pc.w_scale, pa.w_scale
    return p


class PackedDw:
    __slots__ = ("w", "bias", "k", "stride", "pad", "c", "c_s", "act")


def pack_dwconv(weight, bias=None, bn=None, stride=(1, 1, 1), pad=(0, 0, 0), act=ACT_NONE, device=None):
    """weight: [C,1,kt,kh,kw] or [C,1,kh,kw] depthwise.  Packed as [taps][C_s]."""
    w, b = fold_bn(weight, bias, bn)
    if w.dim() == 4:
        w = w[:, :, None]
    c, one, kt, kh, kw = w.shape
    assert one == 1
    c_s = rup4(c)
    wp = torch.zeros(kt * kh * kw, c_s, dtype=torch.float32, device=w.device)
    wp[:, :c] = w.reshape(c, kt * kh * kw).t()
    bp = torch.zeros(c_s, dtype=torch.float32, device=w.device) if b is None else _pad_vec(b, c_s)
    p = PackedDw()
    dev = w.device if device is None else device
    p.w, p.bias = wp.to(dev).contiguous(), bp.to(dev)
    p.k, p.stride, p.pad, p.c, p.c_s, p.act = (kt, kh, kw), tuple(stride), tuple(pad), c, c_s, act
    return p


class PackedX3dAb:
    __slots__ = ("wa", "ba", "wb", "bb", "wa_scale", "cin_s", "cmid", "cmid_s")


def pack_x3d_ab(pa, pb, stride=(1, 1, 1)):
    """Operands of the fused X3D `a` + `b` kernel (mspi_x3d_ab_fwd) from the packed 1x1x1 conv `pa` (PackedConv, f16x3: BN
    folded, scaled hi/lo planes) and the packed 3x3x3 depthwise conv `pb` (PackedDw) of that stride; None when the layer
    pair is outside the kernel's range."""
    ks = (pa.cin_s + 31) // 32
    if pa.prec != PREC_F16X3 or pa.k != (1, 1, 1) or pa.stride != (1, 1, 1) or pb.k != (3, 3, 3) or pb.stride != stride \
            or pb.pad != (1, 1, 1) or pa.cout_s != pb.c_s or pa.cin_s % 8 or pa.act != ACT_RELU or pa.bias is None \
            or ks not in (1, 2, 3, 6):
        return None
    p = PackedX3dAb()
    p.wa = frag_x3d_ab(_padded(_scaled(pa, pa.cin_s), (pa.cout_s + 31) // 32 * 32, ks * 32)).contiguous().to(pa.w.device)
    p.ba, p.wb, p.bb = pa.bias, pb.w, pb.bias
    p.wa_scale, p.cin_s, p.cmid, p.cmid_s = pa.w_scale, pa.cin_s, pb.c, pb.c_s
    return p


def pack_x3d_ab_s2(pa, pb):
    """Operands of the stride-2 fused X3D `a` + `b` kernel (mspi_x3d_ab_s2_fwd, the first block of a stage): the same pack as
    pack_x3d_ab, from a depthwise conv `pb` with stride (1,2,2); None when the layer pair is outside the kernel's range."""
    return pack_x3d_ab(pa, pb, stride=(1, 2, 2)) if (pa.cin_s + 31) // 32 <= 3 else None


class PackedX3dStem:
    __slots__ = ("wxy", "wt", "bias")


def pack_x3d_stem(w_xy, w_t, bn):
    """Operands of the fused X3D stem (mspi_x3d_stem_fwd): conv_xy's weight [24,3,1,3,3] (no bias) and the temporal depthwise
    weight [24,1,5,1,1] with `bn` folded, as HOST arrays (they travel as kernel arguments); None for any other stem."""
    if tuple(w_xy.shape) != (24, 3, 1, 3, 3) or tuple(w_t.shape) != (24, 1, 5, 1, 1):
        return None
    wt, b = fold_bn(w_t, None, bn)
    p = PackedX3dStem()
    p.wxy = w_xy.detach().float().cpu().reshape(24, 27).t().contiguous()      # [(ci,kh,kw)][c]
    p.wt = wt.detach().float().cpu().reshape(24, 5).t().contiguous()          # [kt][c]
    p.bias = (b if b is not None else torch.zeros(24)).detach().float().cpu().contiguous()
    return p
