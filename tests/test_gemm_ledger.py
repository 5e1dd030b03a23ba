"""Coverage ledger of the GEMM family: one case per kernel instantiation that mspi_conv_fwd / mspi_conv_splitk_fwd,
mspi_gemm_sp_fwd, mspi_rowgemm_fwd, mspi_mlp_fwd, mspi_x3d_ab_fwd and mspi_x3d_ca_fwd can launch under the default
environment, named by the host-only queries mspi_*_variant (include/mspi_hip.h), which the launches themselves switch on.

The autotuner (engine.conv, engine._conv_sp) times every candidate tile, so which instantiation a production layer runs
differs from box to box: every one of them must be right for every operand form.

CPU: every ledger row selects its code, the rows sit on the edges they claim (ragged M and Cout, K not a multiple of 32, all
activations per kind), and a sweep over many descriptors finds no reachable code without a row.
GPU: every row against a float64 torch reference at 1e-5 of the output's magnitude, no floor (test_kernel_ledger._rel_close)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import test_kernel_ledger as KL
from test_kernel_ledger import _guard, _rel_close      # the tolerance rule and the range-guard reset of both ledgers

F32, F16X3 = 0, 1
NONE, RELU, GELU, SIGMOID, SWISH = 0, 1, 2, 3, 4
ACTS = (NONE, RELU, GELU, SIGMOID, SWISH)

# ------------------------------------------------------------------------------------------------------ conv / split-K / DMA
# geometries: kernel, stride, pad (and the input extent N, T, H, W that gives M = 378 output rows: ragged for BM 64 / 128 / 256)
DENSE = ((1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 3, 7, 9))
DENSE3 = ((1, 1, 1), (1, 1, 1), (0, 0, 0), (3, 3, 7, 9))               # three samples: the gate rows
TAPS = ((1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 3, 13, 17))               # strided 3x3 with pads
CUBE = ((3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 3, 7, 9))                 # 27 taps


def _row(geom, Cc, Co, layout, prec, tile, ksplit=1, gate=False):
    k, s, p, (N, T, H, W) = geom
    return dict(N=N, T=T, H=H, W=W, C=Cc, Cout=Co, k=k, s=s, p=p, layout=layout, prec=prec, tile=tile, ksplit=ksplit, gate=gate)


def _conv_ledger():
    """code -> row.  code = kind * 10^7 + BM * 10^4 + BN * 10 + form (include/mspi_hip.h, mspi_conv_variant).  layout: "cl"
    dense channels-last rows, "slab" a channel slice of a wider token buffer (ld > C), "ncdhw" a raw NCDHW tensor (sC != 1).
    Register forms: v4 f32 = strided 3x3 on a slab, v4 f16x3 = 1x1x1 on a slab, scalar f32 = raw NCDHW 3x3x3, scalar f16x3 =
    C % 4 != 0.  Cout = BN + 12 leaves the last column tile partial; C = 20 / 5 / 6 keep K off multiples of 32."""
    rows = {}
    reg = {0: (128, 128), 1: (128, 64), 2: (128, 32), 3: (64, 64), 4: (128, 128), 5: (256, 128)}
    forms = ((TAPS, 20, "slab"), (DENSE, 20, "slab"), (CUBE, 5, "ncdhw"), (TAPS, 6, "cl"))
    for tile, (bm, bn) in reg.items():
        for form, (geom, Cc, layout) in enumerate(forms):
            code = (2 if tile >= 4 else 1) * 10 ** 7 + bm * 10 ** 4 + bn * 10 + form
            rows[code] = _row(geom, Cc, bn + 12, layout, form & 1, tile)
    # split-K: 27 taps (K = 540 / 135 / 162: 17 / 5 / 6 k-steps), slices 2..8, Cout 76 = 64 + 12
    splitk = ((CUBE, 20, "slab", 2), (CUBE, 20, "cl", 8), (CUBE, 5, "ncdhw", 4), (CUBE, 6, "cl", 3))
    for form, (geom, Cc, layout, S) in enumerate(splitk):
        rows[30000000 + 640640 + form] = _row(geom, Cc, 76, layout, form & 1, 3, ksplit=S)
    # LDS-DMA, 128 rows: BN 32..256 by tile 11 / 7 / 9 / 6 / 8 / 10; BN 160 / 224 / 256 only as tile 8 ("all columns") with
    # Cout in 129..160 / 193..224 / 225..256
    dma = {32: (11, 44), 64: (7, 76), 96: (9, 108), 128: (6, 140), 160: (8, 148), 192: (10, 204), 224: (8, 212), 256: (8, 244)}
    for bn, (tile, Co) in dma.items():
        rows[41280000 + bn * 10 + 0] = _row(TAPS, 20, Co, "slab", F16X3, tile)
        rows[41280000 + bn * 10 + 1] = _row(DENSE, 20, Co, "slab", F16X3, tile)
        rows[41280000 + bn * 10 + 2] = _row(DENSE3, 20, Co, "cl", F16X3, tile, gate=True)
    # the heuristic's deep_conv path (taps > 1, K >= 2048, M >= 16384): 3x3x3 over 76 channels, M = 16884, BN 64
    rows[41280640] = _row(((3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 4, 63, 67)), 76, 76, "cl", F16X3, -1)
    # LDS-DMA, 256 rows / 8 waves: tiles 12 / 13 / 14
    for tile, bn in ((12, 256), (13, 192), (14, 128)):
        rows[52560000 + bn * 10 + 0] = _row(TAPS, 20, bn + 12, "slab", F16X3, tile)
        rows[52560000 + bn * 10 + 1] = _row(DENSE, 20, bn + 12, "slab", F16X3, tile)
        rows[52560000 + bn * 10 + 2] = _row(DENSE3, 20, bn + 12, "cl", F16X3, tile, gate=True)
    # 256-row tile at the M the autotuner offers it (>= 16384), last row tile ragged (17298 = 67 x 256 + 146)
    rows[52561281] = _row(((1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 9, 31, 31)), 20, 140, "slab", F16X3, 14)
    return rows


CONV_LEDGER = _conv_ledger()
CONV_EXCLUDED = {}
# MSPI_CONV_TILE, MSPI_CONV_4WAVE, MSPI_CONV_DMA and MSPI_CONV_BN only move heuristic calls between the codes above.

# pre-split GEMM (mspi_gemm_sp_fwd): code = kind * 10^7 + BM * 10^4 + BN * 10 + form, kind 6 = 128 rows, 7 = 256 rows, form 0 =
# fp32 rows out, 1 = blocked planes out.  row: (N, T, H, W, K, Cout, tile); K a multiple of 32 (the planes' contract), planes out
# need Cout % 32 == 0 (Cout = BN + 32: partial last tile), rows out Cout = BN + 12.  M = 378: ragged for 16 / 128 / 256.
_SP_TILES = {(128, 128): 6, (128, 64): 7, (128, 96): 9, (128, 192): 10, (128, 256): 11, (256, 256): 12, (256, 192): 13,
             (256, 128): 14}


def _sp_ledger():
    rows = {}
    for (bm, bn), tile in _SP_TILES.items():
        base = (6 if bm == 128 else 7) * 10 ** 7 + bm * 10 ** 4 + bn * 10
        rows[base] = (2, 3, 7, 9, 64 if bn != 96 else 96, bn + 12, tile)
        rows[base + 1] = (2, 3, 7, 9, 96 if bn != 96 else 64, bn + 32, tile)
    rows[61280640] = (2, 3, 7, 9, 64, 44, -1)               # the heuristic: Cout <= 64 -> 128 x 64
    return rows


SP_LEDGER = _sp_ledger()

# row-stationary thin GEMM: code = KSB * 10 + gate -> (M, K, N).  K stored columns (not multiples of 32), N = 44: a partial chunk.
ROWGEMM_LEDGER = {
    20: (378, 28, 44), 21: (378, 28, 44),
    40: (501, 60, 44), 41: (501, 60, 76),
    80: (378, 108, 44), 81: (378, 108, 44),
    140: (501, 216, 44), 141: (378, 216, 108),
}

# fused MLP: code = C * 1000 + TM * 100 + NS * 10 + NWV -> (M, C, hidden).  The 8-wave form at M just over 65536 (ragged
# last 256-row tile) with the smallest legal hidden.
MLP_LEDGER = {
    96134: (1001, 96, 64),
    192134: (777, 192, 96),
    192138: (65536 + 77, 192, 32),
}
MLP_EXCLUDED = {96244: "mlp_fused_kernel<96, 2, 4>: only with MSPI_MLP_TM=2"}

# fused X3D a + b: code = KS * 10000 + TH * 1000 + TW * 10 + SL -> (N, T, H, W, Cin, Cmid).  Cmid 52: a partial chunk.
X3D_AB_LEDGER = {
    17142: (2, 3, 14, 28, 24, 52),
    27142: (2, 2, 7, 14, 48, 52),
    37142: (1, 3, 14, 14, 88, 36),
    17071: (2, 3, 14, 7, 24, 52),
    27071: (2, 2, 7, 7, 48, 20),
    37071: (1, 3, 14, 7, 88, 52),
    67071: (2, 2, 7, 7, 176, 52),
}

# fused X3D c + next a: code = C * 10 + gate -> (N, rows per sample, D, Cx).  D, Cx stored widths (Cx not a multiple of 32).
X3D_CA_LEDGER = {
    1280: (2, 189, 56, 44),
    1281: (3, 126, 100, 44),
    2240: (2, 189, 216, 100),
    2241: (3, 126, 148, 60),
}


SWITCHES = ("MSPI_CONV_", "MSPI_MLP_", "MSPI_X3D_")


def _no_switches():
    KL._no_switches(SWITCHES)


def _acts(i):
    """The two epilogue activations of the i-th row of a kind: over any three rows all five appear."""
    return ACTS[i % 5], ACTS[(i + 2) % 5]


def _row_index(ledger, code):
    kind = code // 10 ** 7
    return sorted(c for c in ledger if c // 10 ** 7 == kind).index(code)


# ---------------------------------------------------------------------------------------------------------------- queries
def _lib():
    from mspi_amd import _lib as L
    return L, L.load()


def _out_extent(r):
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip((r["T"], r["H"], r["W"]), r["k"], r["s"], r["p"]))


def _ldx(r):
    return r["C"] + 12 if r["layout"] == "slab" else r["C"]


def _conv_desc(r, ldy=None, ldr=0, act=NONE):
    L, _ = _lib()
    d = L.ConvDesc()
    N, T, H, W, Cc = r["N"], r["T"], r["H"], r["W"], r["C"]
    d.N, d.T, d.H, d.W, d.C = N, T, H, W, Cc
    if r["layout"] == "ncdhw":
        d.sN, d.sT, d.sH, d.sW, d.sC = Cc * T * H * W, H * W, W, 1, T * H * W
    else:
        ld = _ldx(r)
        d.sN, d.sT, d.sH, d.sW, d.sC = T * H * W * ld, H * W * ld, W * ld, ld, 1
    d.kT, d.kH, d.kW = r["k"]
    d.strT, d.strH, d.strW = r["s"]
    d.padT, d.padH, d.padW = r["p"]
    d.To, d.Ho, d.Wo = _out_extent(r)
    K = r["k"][0] * r["k"][1] * r["k"][2] * Cc
    d.Cout = r["Cout"]
    d.ldy = ldy or r["Cout"]
    d.ldw = (K + 3) // 4 * 4 if r["prec"] == F32 else (K + 31) // 32 * 32
    d.ldr = ldr
    d.act, d.prec, d.w_scale, d.tile = act, r["prec"], 1.0, r["tile"]
    return d


_X_ALIGNED, _G_ALIGNED = 1 << 20, 1 << 21        # the queries look at pointers for 16-B alignment only, never through them


def _conv_code(r):
    _, lib = _lib()
    return lib.mspi_conv_variant(C.byref(_conv_desc(r)), _X_ALIGNED, _G_ALIGNED if r["gate"] else None, r["ksplit"])


def _sp_desc(row, planes_out=False):
    L, _ = _lib()
    N, T, H, W, K, Co, tile = row
    d = L.ConvDesc()
    d.N, d.T, d.H, d.W, d.C = N, T, H, W, K
    d.kT = d.kH = d.kW = d.strT = d.strH = d.strW = 1
    d.To, d.Ho, d.Wo, d.Cout = T, H, W, Co
    d.ldy, d.ldw, d.prec, d.w_scale, d.tile = 0 if planes_out else Co, K, F16X3, 1.0, tile
    return d


def _sp_code(code_or_row, planes_out):
    _, lib = _lib()
    return lib.mspi_gemm_sp_variant(C.byref(_sp_desc(code_or_row, planes_out)), _X_ALIGNED if planes_out else None)


def _rg_desc(M, K, N, rps=1, act=NONE):
    L, _ = _lib()
    d = L.RowGemmDesc()
    d.M, d.K, d.N, d.ldx, d.ldy, d.ldr, d.ldg = M, K, N, K, N, N, K
    d.act, d.rows_per_sample, d.w_scale = act, rps, 1.0
    return d


def _rg_code(M, K, N, gate):
    _, lib = _lib()
    return lib.mspi_rowgemm_variant(C.byref(_rg_desc(M, K, N)), int(gate))


def _mlp_desc(M, Cc, hidden, ln=0):
    L, _ = _lib()
    d = L.MlpDesc()
    d.M, d.C, d.hidden, d.ldx, d.ldy, d.ldr = M, Cc, hidden, Cc, Cc, Cc
    d.ln, d.act, d.eps, d.w1_scale, d.w2_scale = ln, GELU, 1e-6, 1.0, 1.0
    return d


def _mlp_code(M, Cc, hidden):
    _, lib = _lib()
    return lib.mspi_mlp_variant(C.byref(_mlp_desc(M, Cc, hidden)))


def _ab_desc(N, T, H, W, Cin, Cmid, act=SWISH):
    L, _ = _lib()
    d = L.X3dAbDesc()
    d.N, d.T, d.H, d.W, d.Cin, d.Cmid, d.ldx, d.ldu, d.act, d.wa_scale = N, T, H, W, Cin, Cmid, Cin, Cmid, act, 1.0
    return d


def _ab_code(N, T, H, W, Cin, Cmid):
    _, lib = _lib()
    return lib.mspi_x3d_ab_variant(C.byref(_ab_desc(N, T, H, W, Cin, Cmid)))


def _ca_desc(M, D, Cx, rps=1):
    L, _ = _lib()
    d = L.X3dCaDesc()
    d.M, d.D, d.Cx, d.ldu, d.ldr, d.ldy, d.ldt, d.ldg = M, D, Cx, D, Cx, Cx, D, D
    d.rows_per_sample, d.wc_scale, d.wa_scale = rps, 1.0, 1.0
    return d


def _ca_code(M, D, Cx, gate):
    _, lib = _lib()
    return lib.mspi_x3d_ca_variant(C.byref(_ca_desc(M, D, Cx)), int(gate))


# ---------------------------------------------------------------------------------------------------------------- sweeps
def _conv_sweep():
    """Every code mspi_conv_variant returns over geometries, input layouts, channel counts, M, precisions, tiles, split-K and
    gate."""
    seen = {}
    geoms = [((1, 1, 1), (1, 1, 1), (0, 0, 0)), ((1, 1, 1), (1, 2, 2), (0, 0, 0)), ((1, 3, 3), (1, 2, 2), (0, 1, 1)),
             ((3, 3, 3), (1, 1, 1), (1, 1, 1)), ((3, 1, 1), (1, 1, 1), (1, 0, 0)), ((1, 1, 1), (1, 1, 1), (0, 1, 1))]
    sizes = [(2, 3, 7, 9), (2, 8, 33, 33), (4, 16, 33, 33)]            # M small, >= 16384, >= 65536
    for k, s, p in geoms:
        for N, T, H, W in sizes:
            for Cc, layout in ((20, "cl"), (20, "slab"), (80, "cl"), (256, "slab"), (5, "ncdhw"), (6, "cl")):
                for Co in (4, 20, 44, 100, 148, 212, 244, 300, 512):
                    for prec in (F32, F16X3):
                        r = dict(N=N, T=T, H=H, W=W, C=Cc, Cout=Co, k=k, s=s, p=p, layout=layout, prec=prec, tile=-1,
                                 ksplit=1, gate=False)
                        for gate in (False, True):
                            for tile in range(-1, 15):
                                r.update(tile=tile, gate=gate, ksplit=1)
                                code = _conv_code(r)
                                if code > 0:
                                    seen.setdefault(code, dict(r))
                        r.update(tile=3, gate=False)
                        for S in range(2, 9):
                            r["ksplit"] = S
                            code = _conv_code(r)
                            if code > 0:
                                seen.setdefault(code, dict(r))
    return seen


def _sp_sweep():
    seen = {}
    for K in (32, 64, 96, 256):
        for Co in (4, 32, 44, 64, 96, 100, 192, 288, 384, 512):
            for T, H, W in ((3, 7, 9), (8, 33, 33)):
                for tile in range(-1, 15):
                    for planes in (False, True):
                        row = (2, T, H, W, K, Co, tile)
                        code = _sp_code(row, planes)
                        if code > 0:
                            seen.setdefault(code, row)
    return seen


# ------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("code", sorted(CONV_LEDGER))
def test_conv_ledger_row_selects_its_kernel(code):
    _no_switches()
    assert _conv_code(CONV_LEDGER[code]) == code


@pytest.mark.parametrize("code", sorted(SP_LEDGER))
def test_gemm_sp_ledger_row_selects_its_kernel(code):
    _no_switches()
    assert _sp_code(SP_LEDGER[code], code % 10 == 1) == code


def test_fused_ledger_rows_select_their_kernels():
    _no_switches()
    for code, (M, K, N) in ROWGEMM_LEDGER.items():
        assert _rg_code(M, K, N, code % 10) == code
    for code, (M, Cc, hidden) in MLP_LEDGER.items():
        assert _mlp_code(M, Cc, hidden) == code
    for code, (N, T, H, W, Cin, Cmid) in X3D_AB_LEDGER.items():
        assert _ab_code(N, T, H, W, Cin, Cmid) == code
    for code, (N, rps, D, Cx) in X3D_CA_LEDGER.items():
        assert _ca_code(N * rps, D, Cx, code % 10) == code


def test_ledger_rows_sit_on_the_edges():
    """The rows carry what they claim: M not a multiple of BM, a partial last column tile, K off multiples of 32 where the
    kernel allows it, and all five activations within each kind."""
    for code, r in CONV_LEDGER.items():
        bm, bn = (code // 10 ** 4) % 1000, (code // 10) % 1000
        M = r["N"] * math.prod(_out_extent(r))
        K = math.prod(r["k"]) * r["C"]
        assert M % bm and r["Cout"] % bn and K % 32, (code, M, r["Cout"], K)
        assert not r["gate"] or r["C"] % 8 == 4, code      # the gate's last 8-channel chunk is half outside the row
    for code, (N, T, H, W, K, Co, tile) in SP_LEDGER.items():
        bm, bn = (code // 10 ** 4) % 1000, (code // 10) % 1000
        assert (N * T * H * W) % bm and (N * T * H * W) % 16 and Co % bn, code
    for code, (M, K, N) in ROWGEMM_LEDGER.items():
        assert M % 128 and N % 32 and K % 32, code
    assert all(M % 128 for M, _, _ in MLP_LEDGER.values()) and MLP_LEDGER[192138][0] > 65536
    for ledger in (CONV_LEDGER, SP_LEDGER, ROWGEMM_LEDGER):
        for kind in {c // 10 ** 7 for c in ledger}:
            codes = [c for c in ledger if c // 10 ** 7 == kind]
            got = {a for c in codes for a in _acts(_row_index(ledger, c))}
            assert got == set(ACTS), (kind, got)


def test_conv_ledger_covers_every_reachable_kernel():
    _no_switches()
    seen = _conv_sweep()
    missing = {c: r for c, r in seen.items() if c not in CONV_LEDGER}
    assert not missing, "conv kernels without a ledger row (code: a descriptor that selects it): %s" % missing
    assert not set(seen) & set(CONV_EXCLUDED)
    assert set(CONV_LEDGER) == set(seen), "ledger rows the sweep never reaches: %s" % (set(CONV_LEDGER) - set(seen))


def test_gemm_sp_ledger_covers_every_reachable_kernel():
    _no_switches()
    seen = _sp_sweep()
    missing = {c: r for c, r in seen.items() if c not in SP_LEDGER}
    assert not missing, "pre-split GEMM kernels without a ledger row: %s" % missing
    assert set(SP_LEDGER) == set(seen), "ledger rows the sweep never reaches: %s" % (set(SP_LEDGER) - set(seen))


def test_fused_ledgers_cover_every_reachable_kernel():
    _no_switches()
    seen = {}
    for K in range(4, 232, 4):
        for N in (4, 44, 100, 1024):
            for gate in (0, 1):
                seen.setdefault(_rg_code(1000, K, N, gate), (K, N))
    seen.pop(-1, None)
    assert set(seen) == set(ROWGEMM_LEDGER), seen
    seen = {}
    for Cc in (64, 96, 128, 192):
        for hidden in (32, 96, 384, 512, 768, 1024):
            for M in (1, 1000, 65535, 65536, 10 ** 6):
                seen.setdefault(_mlp_code(M, Cc, hidden), (M, Cc, hidden))
    seen.pop(-1, None)
    assert set(seen) == set(MLP_LEDGER) and not set(seen) & set(MLP_EXCLUDED), seen
    seen = {}
    for Cin in range(8, 257, 8):
        for H, W in ((7, 7), (14, 14), (7, 28), (56, 56), (14, 21), (6, 14)):
            seen.setdefault(_ab_code(2, 4, H, W, Cin, 52), (H, W, Cin))
    seen.pop(-1, None)
    assert set(seen) == set(X3D_AB_LEDGER), seen
    seen = {}
    for D in range(4, 260, 4):
        for Cx in (4, 44, 256, 260):
            for gate in (0, 1):
                seen.setdefault(_ca_code(500, D, Cx, gate), (D, Cx))
    seen.pop(-1, None)
    assert set(seen) == set(X3D_CA_LEDGER), seen


def test_variant_queries_refuse_what_the_launch_refuses():
    """The selection functions hold the launches' checks; the refusals come with their messages.  The gated conv with
    padding or stride is refused through the query only: launched on a build without the check, the gated LDS-DMA form
    (which has no spatial bounds check) would read outside x."""
    _no_switches()
    _, lib = _lib()
    gated = dict(CONV_LEDGER[41281282])
    for k, s, p in (((1, 1, 1), (1, 1, 1), (0, 1, 1)), ((1, 1, 1), (1, 2, 2), (0, 0, 0)), ((1, 3, 3), (1, 1, 1), (0, 1, 1))):
        for tile in (-1, 3, 6, 12):
            r = dict(gated, k=k, s=s, p=p, tile=tile)
            assert _conv_code(r) == -1 and b"gate needs a 1x1x1 stride-1 unpadded conv" in lib.mspi_last_error(), (k, s, p, tile)
    assert _conv_code(dict(gated, ksplit=4)) == -1 and b"no gate" in lib.mspi_last_error()
    # the LDS-DMA tiles need f16x3 and the 16-B gather
    for tile in range(6, 15):
        for r in (dict(CONV_LEDGER[11281280], tile=tile), dict(CONV_LEDGER[11281282], tile=tile), dict(CONV_LEDGER[11281283], tile=tile)):
            assert _conv_code(r) == -1 and (b"tile %d not available" % tile) in lib.mspi_last_error()
    # a misaligned input pointer is a scalar gather: DMA refused, register tile takes the scalar form
    r = dict(CONV_LEDGER[41281281])
    d = _conv_desc(r)
    assert lib.mspi_conv_variant(C.byref(d), _X_ALIGNED + 4, None, 1) == -1
    d.tile = 3
    assert lib.mspi_conv_variant(C.byref(d), _X_ALIGNED + 4, None, 1) == 10640643
    # tile 8 holds every column in one tile: Cout <= 256
    assert _conv_code(dict(CONV_LEDGER[41282561], Cout=260)) == -1 and b"tile 8 not available" in lib.mspi_last_error()
    assert _conv_code(dict(CONV_LEDGER[41282561], tile=15)) == -1
    assert _conv_code(dict(CONV_LEDGER[30640640], ksplit=65)) == -1 and b"ksplit" in lib.mspi_last_error()
    assert _conv_code(dict(CONV_LEDGER[30640640], Cout=74)) == -1
    assert lib.mspi_conv_variant(C.byref(_conv_desc(CONV_LEDGER[11281280])), None, None, 1) == -1      # NULL input
    assert b"null" in lib.mspi_last_error()
    bad = _conv_desc(CONV_LEDGER[11281280])
    bad.Wo += 1
    assert lib.mspi_conv_variant(C.byref(bad), _X_ALIGNED, None, 1) == -1 and b"does not match" in lib.mspi_last_error()
    assert lib.mspi_gemm_sp_variant(C.byref(_sp_desc((2, 3, 7, 9, 64, 44, 6), True)), _X_ALIGNED) == -1   # planes: Cout % 32
    assert b"Cout % 32" in lib.mspi_last_error()
    assert lib.mspi_gemm_sp_variant(C.byref(_sp_desc((2, 3, 7, 9, 48, 44, 6))), None) == -1              # K % 32
    assert _rg_code(100, 232, 44, 0) == -1 and b"outside" in lib.mspi_last_error()
    assert lib.mspi_rowgemm_variant(C.byref(_rg_desc(100, 60, 44, rps=0)), 1) == -1 and b"gate" in lib.mspi_last_error()
    assert _mlp_code(100, 128, 384) == -1 and b"not supported" in lib.mspi_last_error()
    assert _mlp_code(100, 96, 1024) == -1 and b"> 512" in lib.mspi_last_error()
    assert lib.mspi_mlp_variant(C.byref(_mlp_desc(100, 96, 384, ln=1))) == 96134    # the query takes the LN parameters as given
    assert _ab_code(2, 4, 14, 14, 176, 52) == -1 and b"outside" in lib.mspi_last_error()     # K > 96 on 14-wide tiles
    assert _ca_code(100, 228, 44, 0) == -1 and _ca_code(100, 56, 260, 1) == -1
    assert lib.mspi_x3d_ca_variant(C.byref(_ca_desc(100, 56, 44, rps=0)), 1) == -1 and b"gate" in lib.mspi_last_error()


def test_production_shapes_keep_their_kernels():
    """Model shapes whose kernel is not timed, pinned to the instantiation they run today."""
    _no_switches()
    # ConvNeXt-T fused MLP (per frame, 8 clips x 16 frames): stage 1 at 56^2, stage 2 at 28^2 on the 8-wave form (M = 100352)
    assert _mlp_code(8 * 16 * 56 * 56, 96, 384) == 96134
    assert _mlp_code(8 * 16 * 28 * 28, 192, 768) == 192138
    assert _mlp_code(1 * 16 * 28 * 28, 192, 768) == 192134          # batch 1: the 4-wave form
    # X3D-L rowgemm: `a` convs (block width 24 / 48 / 96 / 192 -> inner 54 / 108 / 216 / 432, stored 56 / 108 / 216 / 432) and the
    # gated `c` convs back (inner -> block width)
    M = 8 * 16 * 56 * 56
    assert [_rg_code(M, K, N, 0) for K, N in ((24, 56), (48, 108), (96, 216), (192, 432))] == [20, 40, 80, 140]
    assert [_rg_code(M, K, N, 1) for K, N in ((56, 24), (108, 48), (216, 96))] == [41, 81, 141]
    # X3D-L at 224^2: fused a + b per stage (56^2 / 28^2 / 14^2 / 7^2, block widths 24 / 48 / 96 / 192) and the c + a seam
    assert [_ab_code(8, 16, hw, hw, cin, cm) for hw, cin, cm in ((56, 24, 56), (28, 48, 108), (14, 96, 216), (7, 192, 432))] == \
        [17142, 27142, 37142, 67071]
    assert [_ca_code(8 * 16 * hw * hw, d, cx, g) for hw, d, cx in ((56, 56, 24), (28, 108, 48), (14, 216, 96)) for g in (0, 1)] == \
        [1280, 1281, 1280, 1281, 2240, 2241]
    # fusion-head SA mask conv (32 -> 1, (1,3,3), SIGMOID) at its three levels, and the 27-tap readout conv (192 -> 192)
    mask = dict(N=8, T=16, H=56, W=56, C=32, Cout=1, k=(1, 3, 3), s=(1, 1, 1), p=(0, 1, 1), layout="cl", prec=F16X3, tile=-1,
                ksplit=1, gate=False)
    assert [_conv_code(dict(mask, H=hw, W=hw)) for hw in (56, 28, 14)] == [11280321, 10640641, 10640641]
    readout = dict(mask, C=192, Cout=192, k=(3, 3, 3), p=(1, 1, 1))
    assert [_conv_code(dict(readout, H=hw, W=hw)) for hw in (56, 28)] == [41280640, 41280640]      # deep_conv: DMA, BN 64


def _old_profiler_name(c, presplit):
    """The name engine.conv / engine._conv_sp built from the bitfield mspi_conv_last_config() returned, before the variant
    code took its place: the same shifts, masks and format strings."""
    if presplit:
        return "conv_gemm<%d,%d,dma-presplit,f16x3>" % (c >> 16, (c >> 4) & 0xFFF)
    return "conv_gemm<%d,%d,%s,%s>" % (c >> 16, (c >> 4) & 0xFFF,
                                       "dma" if c & 4 else ("s" if c & 1 else "v4") + ("w8" if c & 8 else ""),
                                       "f16x3" if (c >> 1) & 1 else "f32")


def test_gemm_kernel_name_is_the_name_the_last_launch_bitfield_gave():
    """engine.gemm_kernel_name(code) for every conv and pre-split ledger row against the old path restated: the bitfield
    (BM << 16) | (BN << 4) | (8 if 8 waves) | (prec << 1) | (4 if LDS-DMA else 1 if scalar gather) the launches used to
    leave behind, built from the row, decoded as engine.py decoded it.  Split-K (kind 3) is named from the kernel choice: GPU
    test below."""
    from mspi_amd import engine as E
    for code, r in CONV_LEDGER.items():
        kind, bm, bn = code // 10 ** 7, (code // 10 ** 4) % 1000, (code // 10) % 1000
        if kind == 3:
            continue
        dma = kind in (4, 5)
        scalar = r["layout"] == "ncdhw" or r["C"] % 4 != 0
        w8 = kind == 2 or (dma and bm == 256)
        c = (bm << 16) | (bn << 4) | (8 if w8 else 0) | (r["prec"] << 1) | (4 if dma else 1 if scalar else 0)
        assert E.gemm_kernel_name(code) == _old_profiler_name(c, False), code
    for code in SP_LEDGER:
        bm, bn = (code // 10 ** 4) % 1000, (code // 10) % 1000
        c = (bm << 16) | (bn << 4) | (8 if bm == 256 else 0) | (F16X3 << 1) | 4
        assert E.gemm_kernel_name(code) == _old_profiler_name(c, True), code


def test_engine_tiles_restate_the_library_table():
    """engine.TILES (code -> kind, BM, BN) against the codes the library's own table gives the ledger rows: every tile code has
    a row, and the pre-split codes are engine.SP_TILES with code 11 as 128 x 256."""
    from mspi_amd import engine as E
    seen = set()
    for code, r in CONV_LEDGER.items():
        kind, bm, bn = code // 10 ** 7, (code // 10 ** 4) % 1000, (code // 10) % 1000
        if kind == 3 or r["tile"] < 0:
            continue
        want = E.TILES[r["tile"]]
        assert (kind, bm) == want[:2] and (bn == want[2] or (want[2] == 0 and bn == (r["Cout"] + 31) // 32 * 32)), (code, want)
        seen.add(r["tile"])
    assert seen == set(E.TILES) == set(range(15))
    sp = {row[6]: ((code // 10 ** 7) - 2, (code // 10 ** 4) % 1000, (code // 10) % 1000) for code, row in SP_LEDGER.items() if row[6] >= 0}
    assert set(sp) == set(E.SP_TILES)
    assert all(sp[t] == (E.TILES[t] if t != 11 else (E.DMA128, 128, 256)) for t in sp)


def test_autotune_candidate_lists():
    """engine._conv_kernels and engine._sp_tiles, built from engine.TILES, are the literal lists the autotuner has timed so far."""
    from types import SimpleNamespace as NS
    from mspi_amd import engine as E

    def cands(prec, cout, M, sC=1, Cc=20):
        return E._conv_kernels(NS(prec=prec, cout_s=cout, ldw=32), NS(sC=sC, C=Cc), M, None, False, None)

    assert cands(F32, 192, 378) == [1, 2, 3, 4]
    assert cands(F16X3, 192, 378) == [1, 2, 3, 4, 6, 7, 9, 10, 8]
    assert cands(F16X3, 192, 16383) == [1, 2, 3, 4, 6, 7, 9, 10, 8]
    assert cands(F16X3, 192, 16384) == [1, 2, 3, 4, 6, 7, 9, 10, 8, 12, 13, 14]
    assert cands(F16X3, 256, 378) == [1, 2, 3, 4, 6, 7, 9, 10, 8]
    assert cands(F16X3, 320, 378) == [1, 2, 3, 4, 6, 7, 9, 10]
    assert cands(F16X3, 320, 16384) == [1, 2, 3, 4, 6, 7, 9, 10, 12, 13, 14]
    assert cands(F16X3, 192, 16384, sC=63) == [1, 2, 3, 4] and cands(F16X3, 192, 16384, Cc=6) == [1, 2, 3, 4]      # scalar gather
    assert E._sp_tiles(4095) == [6, 7, 9, 10, 11]
    assert E._sp_tiles(4096) == [6, 7, 9, 10, 11, 12, 13, 14]
    assert E.SP_TILES == (6, 7, 9, 10, 11, 12, 13, 14) and (E.THIN, E.SPLITK, E.HALO) == (100, 200, 300)
    # extra candidates keep their places behind the tile codes
    pk, d = NS(prec=F16X3, cout_s=76, ldw=32 * 32), NS(sC=1, C=20)
    assert E._conv_kernels(pk, d, 378, object(), True, None) == [1, 2, 3, 4, 6, 7, 9, 10, 8, E.THIN, E.HALO] + \
        ([E.SPLITK + 2, E.SPLITK + 4] if E.SPLITK_ENABLED else [])


# ------------------------------------------------------------------------------------------------------------ GPU tests
def _act64(v, a):
    return (v, v.clamp_min(0), F.gelu(v), torch.sigmoid(v), v * torch.sigmoid(v))[a]


def _nan_tail(t, dev):
    """t on the device at the head of a NaN-filled buffer: a gate read past the last sample's row turns the output into NaN
    instead of landing in allocator slack (64 floats of tail keep any such read inside the allocation)."""
    buf = torch.full((t.numel() + 64,), float("nan"), device=dev)
    buf[:t.numel()] = t.reshape(-1).to(dev)
    return buf[:t.numel()].view(t.shape)


def _swish_gate(x, g):
    """x' = swish(x * gate[n, c]) for x [N, C, ...] (float64)."""
    xg = x * g.view(*g.shape, *([1] * (x.dim() - 2)))
    return xg * torch.sigmoid(xg)


def _conv_input(r, x, dev):
    """The row's input form on the GPU: (pointer, keep-alive)."""
    if r["layout"] == "ncdhw":
        t = x.to(dev).contiguous()
        return t.data_ptr(), t
    N, Cc, T, H, W = x.shape
    ld = _ldx(r)
    buf = torch.full((N * T * H * W, ld), 1e3, device=dev)        # columns outside the slice: large junk, never read
    c0 = 8 if r["layout"] == "slab" else 0
    buf[:, c0:c0 + Cc] = x.permute(0, 2, 3, 4, 1).reshape(-1, Cc).to(dev)
    return buf.data_ptr() + 4 * c0, buf


@pytest.mark.gpu
@pytest.mark.parametrize("code", sorted(CONV_LEDGER))
def test_conv_ledger_kernel_vs_fp64(dev, code):
    """Each conv instantiation (register tile x loader x precision, split-K, LDS-DMA tile x form) against F.conv3d in float64:
    bias, a residual with ldr > Cout and the output in a channel slice of a wider buffer (columns outside untouched) under one
    activation, dense output without residual under another.  Gate rows: the SE gate + Swish prologue over three samples,
    the gate followed by NaN in memory.
    LDS-DMA rows: blocked and row-major weights give the same bits.  Split-K rows: bitwise repeatable."""
    from mspi_amd import engine as E
    _no_switches()
    r = CONV_LEDGER[code]
    lib = E._lib.load()
    g = torch.Generator().manual_seed(code % 100003)
    N, Cc, Co, k = r["N"], r["C"], r["Cout"], r["k"]
    x = torch.randn(N, Cc, r["T"], r["H"], r["W"], generator=g)
    w = torch.randn(Co, Cc, *k, generator=g) / math.sqrt(Cc * math.prod(k))
    b = torch.randn(Co, generator=g)
    gt = torch.rand(N, Cc, generator=g) * 2 if r["gate"] else None
    xr = _swish_gate(x.double(), gt.double()) if r["gate"] else x.double()
    ref = F.conv3d(xr, w.double(), b.double(), r["s"], r["p"]).permute(0, 2, 3, 4, 1).reshape(-1, Co)
    M = ref.shape[0]
    pk = E.pack_conv(w, b, None, r["s"], r["p"], device=dev, prec=r["prec"])
    assert pk.cout_s == Co
    xp, keep = _conv_input(r, x, dev)
    gd = _nan_tail(gt, dev) if r["gate"] else None      # C = 20: the last k chunk's second float4 lies past a sample's row
    kind = code // 10 ** 7
    a0, a1 = _acts(_row_index(CONV_LEDGER, code))
    res = torch.randn(M, Co + 8, generator=g)

    def run(act, with_res, ldy, blocked=True):
        y = torch.full((M, ldy), -3.0, device=dev)
        c0 = 4 if ldy > Co else 0
        rd = res.to(dev) if with_res else None
        d = _conv_desc(r, ldy=ldy, ldr=Co + 8 if with_res else 0, act=act)
        d.w_scale = pk.w_scale
        assert d.ldw == pk.ldw
        d.w_blocked = E.sp_weights(pk).data_ptr() if (blocked and r["prec"] == F16X3) else None
        assert lib.mspi_conv_variant(C.byref(d), xp, gd.data_ptr() if gd is not None else None, r["ksplit"]) == code
        bias = pk.bias.data_ptr()
        if r["ksplit"] > 1:
            ws = torch.empty(r["ksplit"] * M * Co, device=dev)
            E.check(lib.mspi_conv_splitk_fwd(C.byref(d), xp, pk.w.data_ptr(), bias, rd.data_ptr() if rd is not None else None,
                                             y.data_ptr() + 4 * c0, ws.data_ptr(), r["ksplit"], E._stream()), "mspi_conv_splitk_fwd")
        else:
            E.check(lib.mspi_conv_fwd(C.byref(d), xp, pk.w.data_ptr(), bias, rd.data_ptr() if rd is not None else None,
                                      gd.data_ptr() if gd is not None else None, y.data_ptr() + 4 * c0, E._stream()), "mspi_conv_fwd")
        torch.cuda.synchronize()
        return y, c0

    _guard(E, dev)
    y, c0 = run(a0, True, Co + 12)
    got = y.cpu()
    _rel_close(got[:, c0:c0 + Co], _act64(ref + res[:, :Co].double(), a0), 1e-5, "conv %d act %d + res" % (code, a0))
    assert (got[:, :c0] == -3.0).all() and (got[:, c0 + Co:] == -3.0).all(), "conv %d wrote outside its output slice" % code
    y1, _ = run(a1, False, Co)
    _rel_close(y1, _act64(ref, a1), 1e-5, "conv %d act %d" % (code, a1))
    if kind in (4, 5):
        y2, _ = run(a1, False, Co, blocked=False)
        assert torch.equal(y1, y2), "conv %d: blocked and row-major weights differ" % code
    if kind == 3:
        y3, _ = run(a0, True, Co + 12)
        assert torch.equal(y, y3), "split-K %d is not bitwise repeatable" % code
    torch.cuda.synchronize()
    assert not E.range_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("code", sorted(SP_LEDGER))
def test_gemm_sp_ledger_kernel_vs_fp64(dev, code):
    """Each pre-split GEMM instantiation on blocked f16 hi/lo activation planes against float64: bias and a residual with
    ldr > Cout under two activations; rows out into a channel slice of a wider buffer, or blocked planes out (joined back)."""
    from mspi_amd import engine as E
    _no_switches()
    N, T, H, W, K, Co, tile = SP_LEDGER[code]
    planes_out = code % 10 == 1
    lib = E._lib.load()
    g = torch.Generator().manual_seed(code % 100003)
    M = N * T * H * W
    x = torch.randn(M, K, generator=g)
    w = torch.randn(Co, K, generator=g) / math.sqrt(K)
    b = torch.randn(Co, generator=g)
    res = torch.randn(M, Co + 8, generator=g)
    ref = x.double() @ w.double().t() + b.double()
    pk = E.pack_conv(w, b, device=dev, prec=F16X3)
    assert pk.ldw == K and pk.cout_s == Co
    xs = E.alloc_sp(N, T, H, W, K, dev)
    xd = x.to(dev).contiguous()
    E.check(lib.mspi_split_planes_fwd(xd.data_ptr(), K, M, K, xs.ptr, xs.ld, xs.plane, E._stream()), "mspi_split_planes_fwd")
    _guard(E, dev)
    for i, act in enumerate(_acts(_row_index(SP_LEDGER, code))):
        with_res = i == 0
        rd = res.to(dev) if with_res else None
        d = _sp_desc(SP_LEDGER[code], planes_out)
        d.act, d.w_scale, d.ldr = act, pk.w_scale, (Co + 8 if with_res else 0)
        want = _act64(ref + (res[:, :Co].double() if with_res else 0), act)
        if planes_out:
            ys = E.alloc_sp(N, T, H, W, Co, dev)
            assert lib.mspi_gemm_sp_variant(C.byref(d), ys.ptr) == code
            E.check(lib.mspi_gemm_sp_fwd(C.byref(d), xs.ptr, xs.ld, xs.plane, E.sp_weights(pk).data_ptr(), pk.bias.data_ptr(),
                                         rd.data_ptr() if rd is not None else None, None, ys.ptr, ys.ld, ys.plane, E._stream()),
                    "mspi_gemm_sp_fwd")
            _rel_close(E.join_planes(ys).as_rows()[:, :Co], want, 1e-5, "pre-split %d act %d -> planes" % (code, act))
        else:
            d.ldy = Co + 12
            y = torch.full((M, Co + 12), -3.0, device=dev)
            assert lib.mspi_gemm_sp_variant(C.byref(d), None) == code
            E.check(lib.mspi_gemm_sp_fwd(C.byref(d), xs.ptr, xs.ld, xs.plane, E.sp_weights(pk).data_ptr(), pk.bias.data_ptr(),
                                         rd.data_ptr() if rd is not None else None, y.data_ptr() + 16, None, 0, 0, E._stream()),
                    "mspi_gemm_sp_fwd")
            got = y.cpu()
            _rel_close(got[:, 4:4 + Co], want, 1e-5, "pre-split %d act %d" % (code, act))
            assert (got[:, :4] == -3.0).all() and (got[:, 4 + Co:] == -3.0).all(), "pre-split %d wrote outside its slice" % code
    torch.cuda.synchronize()
    assert not E.range_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("code", sorted(ROWGEMM_LEDGER))
def test_rowgemm_ledger_kernel_vs_fp64(dev, code):
    """Each thin-GEMM instantiation against float64: input from a channel slice (ldx > K), bias + residual (ldr > N) into an
    output slice under one activation, plain under another; gate rows apply swish(x * gate[sample]) over three samples."""
    from mspi_amd import engine as E
    _no_switches()
    M, K, Nn = ROWGEMM_LEDGER[code]
    gate = code % 10 == 1
    lib = E._lib.load()
    g = torch.Generator().manual_seed(code)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(Nn, K, generator=g) / math.sqrt(K)
    b = torch.randn(Nn, generator=g)
    res = torch.randn(M, Nn + 8, generator=g)
    S = 3
    rps = -(-M // S)
    gt = torch.rand(S, K, generator=g) * 2
    xr = x.double()
    if gate:
        xr = _swish_gate(xr, gt.double()[torch.arange(M) // rps])
    ref = xr @ w.double().t() + b.double()
    pk = E.pack_conv(w, b, device=dev, prec=F16X3)
    assert pk.thin is not None
    xb = torch.full((M, K + 8), 1e3, device=dev)
    xb[:, 4:4 + K] = x.to(dev)
    gd = _nan_tail(gt, dev)
    _guard(E, dev)
    for i, act in enumerate(_acts(_row_index(ROWGEMM_LEDGER, code))):
        with_res = i == 0
        ldy = Nn + 12 if with_res else Nn
        d = _rg_desc(M, K, Nn, rps, act)
        d.ldx, d.ldy, d.ldr, d.w_scale = K + 8, ldy, Nn + 8, pk.w_scale
        assert lib.mspi_rowgemm_variant(C.byref(d), int(gate)) == code
        y = torch.full((M, ldy), -3.0, device=dev)
        c0 = 4 if with_res else 0
        rd = res.to(dev) if with_res else None
        E.check(lib.mspi_rowgemm_fwd(C.byref(d), xb.data_ptr() + 16, pk.thin.data_ptr(), pk.bias.data_ptr(),
                                     rd.data_ptr() if rd is not None else None, gd.data_ptr() if gate else None,
                                     y.data_ptr() + 4 * c0, E._stream()), "mspi_rowgemm_fwd")
        got = y.cpu()
        want = _act64(ref + (res[:, :Nn].double() if with_res else 0), act)
        _rel_close(got[:, c0:c0 + Nn], want, 1e-5, "rowgemm %d act %d" % (code, act))
        assert (got[:, :c0] == -3.0).all() and (got[:, c0 + Nn:] == -3.0).all(), "rowgemm %d wrote outside its slice" % code
    torch.cuda.synchronize()
    assert not E.range_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("code", sorted(MLP_LEDGER))
def test_mlp_ledger_kernel_vs_fp64(dev, code):
    """Each fused-MLP instantiation (GELU between the layers is the kernel's only activation) against float64: LayerNorm on,
    input / output / residual in wider buffers (ldx, ldy, ldr > C; columns outside the output slice untouched), then LayerNorm
    off without residual."""
    from mspi_amd import engine as E
    _no_switches()
    M, Cc, hidden = MLP_LEDGER[code]
    lib = E._lib.load()
    g = torch.Generator().manual_seed(code)
    x = torch.randn(M, Cc, generator=g) * 1.5 + 0.25
    w1 = torch.randn(hidden, Cc, generator=g) / math.sqrt(Cc)
    b1 = torch.randn(hidden, generator=g) * 0.5
    w2 = torch.randn(Cc, hidden, generator=g) / math.sqrt(hidden)
    b2 = torch.randn(Cc, generator=g)
    gam = torch.randn(Cc, generator=g) * 0.5 + 1
    bet = torch.randn(Cc, generator=g) * 0.5
    res = torch.randn(M, Cc, generator=g)
    pk = E.pack_mlp(w1, b1, w2, b2, device=dev)
    xb = torch.full((M, Cc + 8), 1e3, device=dev)
    xb[:, 4:4 + Cc] = x.to(dev)
    rb = torch.zeros(M, Cc + 4, device=dev)
    rb[:, :Cc] = res.to(dev)
    gd, bd = gam.to(dev), bet.to(dev)
    _guard(E, dev)
    for ln in (1, 0):
        h = F.layer_norm(x.double(), (Cc,), gam.double(), bet.double(), 1e-6) if ln else x.double()
        want = F.gelu(h @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double() + (res.double() if ln else 0)
        d = _mlp_desc(M, Cc, hidden, ln)
        d.ldx, d.ldy, d.ldr, d.w1_scale, d.w2_scale = Cc + 8, Cc + 12 if ln else Cc, Cc + 4, pk.s1, pk.s2
        assert lib.mspi_mlp_variant(C.byref(d)) == code
        y = torch.full((M, d.ldy), -3.0, device=dev)
        c0 = 4 if ln else 0
        E.check(lib.mspi_mlp_fwd(C.byref(d), xb.data_ptr() + 16, gd.data_ptr() if ln else None, bd.data_ptr() if ln else None,
                                 pk.w.data_ptr(), pk.b1.data_ptr(), pk.b2.data_ptr(), rb.data_ptr() if ln else None,
                                 y.data_ptr() + 4 * c0, E._stream()), "mspi_mlp_fwd")
        got = y.cpu()
        _rel_close(got[:, c0:c0 + Cc], want, 1e-5, "mlp %d ln=%d" % (code, ln))
        assert (got[:, :c0] == -3.0).all() and (got[:, c0 + Cc:] == -3.0).all(), "mlp %d wrote outside its slice" % code
    torch.cuda.synchronize()
    assert not E.range_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("code", sorted(X3D_AB_LEDGER))
def test_x3d_ab_ledger_kernel_vs_fp64(dev, code):
    """Each fused X3D a + b instantiation against float64 relu(conv1x1) -> depthwise 3x3x3: Swish out, then no activation with
    the squeeze-excite partial sums (bitwise repeatable)."""
    from mspi_amd import engine as E
    _no_switches()
    N, T, H, W, Cin, Cmid = X3D_AB_LEDGER[code]
    g = torch.Generator().manual_seed(code)
    x = torch.randn(N, Cin, T, H, W, generator=g)
    wa = torch.randn(Cmid, Cin, 1, 1, 1, generator=g) / math.sqrt(Cin)
    ba = torch.randn(Cmid, generator=g) * 0.5
    wb = torch.randn(Cmid, 1, 3, 3, 3, generator=g) / math.sqrt(27)
    bb = torch.randn(Cmid, generator=g)
    a = F.conv3d(x.double(), wa.double(), ba.double()).clamp_min(0)
    u = F.conv3d(a, wb.double(), bb.double(), 1, 1, 1, Cmid)
    pa = E.pack_conv(wa, ba, None, act=E.ACT_RELU, device=dev, prec=F16X3)
    pb = E.pack_dwconv(wb, bb, None, (1, 1, 1), (1, 1, 1), device=dev)
    pk = E.pack_x3d_ab(pa, pb)
    assert pk is not None
    xc = E.alloc(N, T, H, W, Cin, dev)
    xc.as_ncdhw().copy_(x.to(dev))
    assert E.x3d_ab_supported(xc, pk)
    lib = E._lib.load()
    assert lib.mspi_x3d_ab_variant(C.byref(E._x3d_ab_desc(xc, pk, pk.cmid_s, SWISH))) == code
    _guard(E, dev)
    _rel_close(E.x3d_ab(xc, pk).as_ncdhw(), u * torch.sigmoid(u), 1e-5, "x3d_ab %d swish" % code)
    out, part = E.x3d_ab(xc, pk, pool=True)
    _rel_close(out.as_ncdhw(), u, 1e-5, "x3d_ab %d" % code)
    _rel_close(part.sum(1)[:, :Cmid], u.sum((2, 3, 4)), 1e-5, "x3d_ab %d pooled sums" % code)
    out2, part2 = E.x3d_ab(xc, pk, pool=True)
    assert torch.equal(part, part2) and torch.equal(out.buf, out2.buf)
    torch.cuda.synchronize()
    assert not E.range_flag()


@pytest.mark.gpu
@pytest.mark.parametrize("code", sorted(X3D_CA_LEDGER))
def test_x3d_ca_ledger_kernel_vs_fp64(dev, code):
    """Each X3D c + next-a seam instantiation (ReLU is the kernel's activation) against float64: y = relu(c(u') + bc + res),
    t = relu(a(y) + ba), u' = swish(u * gate[sample]) over three samples on gate rows."""
    from mspi_amd import engine as E
    _no_switches()
    N, rps, D, Cx = X3D_CA_LEDGER[code]
    gate = code % 10 == 1
    M = N * rps
    g = torch.Generator().manual_seed(code)
    u = torch.randn(M, D, generator=g)
    wc = torch.randn(Cx, D, generator=g) / math.sqrt(D)
    bc = torch.randn(Cx, generator=g) * 0.5
    wa = torch.randn(D, Cx, generator=g) / math.sqrt(Cx)
    ba = torch.randn(D, generator=g) * 0.5
    res = torch.randn(M, Cx, generator=g)
    gt = torch.rand(N, D, generator=g) * 2
    ur = _swish_gate(u.double(), gt.double()[torch.arange(M) // rps]) if gate else u.double()
    y_ref = (ur @ wc.double().t() + bc.double() + res.double()).clamp_min(0)
    t_ref = (y_ref @ wa.double().t() + ba.double()).clamp_min(0)
    pc = E.pack_conv(wc, bc, act=E.ACT_RELU, device=dev, prec=F16X3)
    pa = E.pack_conv(wa, ba, act=E.ACT_RELU, device=dev, prec=F16X3)
    pk = E.pack_x3d_ca(pc, pa)
    assert pk is not None
    uc = E.alloc(N, 1, 1, rps, D, dev)
    uc.as_rows()[:, :D] = u.to(dev)
    rc = E.alloc(N, 1, 1, rps, Cx, dev)
    rc.as_rows()[:, :Cx] = res.to(dev)
    d = _ca_desc(M, D, Cx, rps)
    assert E._lib.load().mspi_x3d_ca_variant(C.byref(d), int(gate)) == code
    _guard(E, dev)
    y, t = E.x3d_ca(uc, pk, rc, gate=_nan_tail(gt, dev) if gate else None)
    _rel_close(y.as_rows()[:, :Cx], y_ref, 1e-5, "x3d_ca %d y" % code)
    _rel_close(t.as_rows()[:, :D], t_ref, 1e-5, "x3d_ca %d t" % code)
    torch.cuda.synchronize()
    assert not E.range_flag()


@pytest.mark.gpu
def test_profiler_names_of_forced_launches(dev):
    """The names engine.Profiler records for one forced launch of each naming path, on the ledger's small geometries
    (M = 378): register tiles, LDS-DMA tiles and pre-split tiles through engine.gemm_kernel_name and the variant queries,
    THIN / split-K / HALO from the kernel choice.  bench.py's roofline line and the tools key on these strings."""
    from mspi_amd import engine as E
    lib = E._lib.load()
    g = torch.Generator().manual_seed(7)

    def conv_row(r, tile, want=None):
        """One E.conv launch of ledger-style row r with the forced kernel choice; returns (recorded names, pack, input)."""
        x = torch.randn(r["N"], r["C"], r["T"], r["H"], r["W"], generator=g)
        w = torch.randn(r["Cout"], r["C"], *r["k"], generator=g) / math.sqrt(r["C"] * math.prod(r["k"]))
        pk = E.pack_conv(w, torch.randn(r["Cout"], generator=g), None, r["s"], r["p"], device=dev, prec=r["prec"])
        if r["layout"] == "ncdhw":
            xin = x.to(dev)
        else:
            ld = _ldx(r)
            buf = torch.zeros(r["N"] * r["T"] * r["H"] * r["W"] * ld, device=dev)
            c0 = 8 if r["layout"] == "slab" else 0
            buf.view(-1, ld)[:, c0:c0 + r["C"]] = x.permute(0, 2, 3, 4, 1).reshape(-1, r["C"]).to(dev)
            xin = E.CL(buf, c0, r["N"], r["T"], r["H"], r["W"], r["C"], ld)
        with E.Profiler() as prof:
            E.conv(xin, pk, tile=tile)
        torch.cuda.synchronize()
        names = [rec[0] for rec in prof.records]
        if want is not None:
            assert names == [want], (tile, names)
        return names, pk, xin

    _guard(E, dev)
    conv_row(CONV_LEDGER[10640641], 3, "conv_gemm<64,64,v4,f16x3>")               # f16x3 slab row
    conv_row(CONV_LEDGER[21281282], 4, "conv_gemm<128,128,sw8,f32>")              # raw NCDHW f32 row
    conv_row(CONV_LEDGER[41280641], 7, "conv_gemm<128,64,dma,f16x3>")             # LDS-DMA dense rows
    conv_row(_row(DENSE, 20, 140, "slab", F16X3, 14), 14, "conv_gemm<256,128,dma,f16x3>")
    conv_row(CONV_LEDGER[30640640], E.SPLITK + 2, "conv_gemm<64,64,splitk2>")
    names, pk, _ = conv_row(_row(DENSE, 20, 76, "cl", F16X3, -1), E.THIN)
    assert pk.thin is not None and names == ["rowgemm<%d,f16x3>" % E.rowgemm_ksb(pk.cin_s)], names
    # the smallest shape mspi_conv_halo_supported accepts: one output position, 32 channels, (1,3,3)
    r = _row(((1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1, 1)), 32, 4, "cl", F16X3, -1)
    names, pk, xin = conv_row(r, E.HALO)
    d = _conv_desc(r)
    d.w_scale, d.w_blocked = pk.w_scale, E.sp_weights(pk).data_ptr()
    v = lib.mspi_conv_halo_variant(C.byref(d), xin.ptr)
    assert v > 0 and names == ["conv_halo<%d,%d,f16x3>" % (v // 1000, v % 1000)], (v, names)
    # pre-split planes in: tile 6 with fp32 rows out, tile 13 with planes out
    for code, want in ((61281280, "conv_gemm<128,128,dma-presplit,f16x3>"), (72561921, "conv_gemm<256,192,dma-presplit,f16x3>")):
        N, T, H, W, K, Co, tile = SP_LEDGER[code]
        pk = E.pack_conv(torch.randn(Co, K, generator=g) / math.sqrt(K), torch.randn(Co, generator=g), device=dev, prec=F16X3)
        xd = torch.randn(N * T * H * W, K, generator=g).to(dev)
        xs = E.alloc_sp(N, T, H, W, K, dev)
        E.check(lib.mspi_split_planes_fwd(xd.data_ptr(), K, xd.shape[0], K, xs.ptr, xs.ld, xs.plane, E._stream()), "mspi_split_planes_fwd")
        with E.Profiler() as prof:
            out = E.conv(xs, pk, tile=tile, sp_out=code % 10 == 1)
        torch.cuda.synchronize()
        assert isinstance(out, E.SP) == (code % 10 == 1)
        assert [rec[0] for rec in prof.records] == [want], (code, prof.records)
    assert not E.range_flag()
