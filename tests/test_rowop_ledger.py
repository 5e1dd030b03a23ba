"""Coverage ledger of the kernels between the GEMMs: LayerNorm, the squeeze-excite gate, bilinear up-sample, row gate,
space-to-depth, max-pool, the MViT q/k augment kernels, permute / gated sum, the small reductions, split / join of the f16
planes and the saliency post-process chain.

The three entry points that choose between instantiations on the host are named by host-only queries the launches
themselves switch on (include/mspi_hip.h): mspi_layernorm_variant (LPR * 100 + VPT), mspi_se_gate_variant (1 register
preloaded, 2 generic), mspi_permute_variant (4 vector, 1 scalar); mspi_mean_rows_slices plays that role for mean_rows.

CPU: every ledger row selects its code, a sweep reaches no code without a row, the rows sit on the bucket edges, the model
shapes are pinned to their kernels, the queries refuse what the launches refuse, and a plain fp32 torch evaluation of every
toleranced GPU case sits at least 4x inside its bar (so a failing kernel case is never "fixed" with friendlier inputs).
GPU: every row against a float64 reference at 1e-5 of max|ref| (no floor), into NaN-filled outputs, beside large finite
neighbours; data movement and single-rounding kernels exactly."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from test_kernel_ledger import _guard, _no_switches, _rel_close      # the tolerance rule of all three ledgers

TOL = 1e-5            # fp32 kernels against fp64: the bar test_kernel_ledger.py / test_gemm_ledger.py hold theirs to
SWITCHES = ("MSPI_LN_", "MSPI_SE_", "MSPI_PERMUTE_")      # none exists today: these dispatchers read no environment
BIG = 1.0e6           # input pads and neighbour columns: finite, and ruinous to any result that reads them
NAN = float("nan")
ACTS = (0, 1, 2, 3, 4)      # none, ReLU, GELU (erf), sigmoid, swish


def _act(v, act):
    return (v, F.relu(v), F.gelu(v), torch.sigmoid(v), v * torch.sigmoid(v))[act]


def _lib():
    from mspi_amd import _lib
    return _lib.load()


# ----------------------------------------------------------------------------------------------------------- the ledgers
# LayerNorm: code -> the widths C run on the GPU.  Each bucket holds its smallest and its largest C, one C whose C / 4 is not
# a multiple of the lanes per row (masked tail lanes) and the widths the models pass.
LN_LEDGER = {
    1601: (4, 36, 64),                    # UniFormer stage 1 (64)
    1602: (68, 96, 112, 128),             # ConvNeXt / Swin / MViT 96, MorphMLP 112, UniFormer 128
    1604: (132, 192, 224, 256),           # every C = 192 stage, the fusion head; MorphMLP 224
    3204: (260, 320, 384, 392, 512),      # stage 3 of ConvNeXt / Swin / MViT, UniFormer 320 / 512, MorphMLP 392, sync block
    6404: (516, 768, 784, 1024),          # stage 4 of ConvNeXt / Swin / MViT, MorphMLP 784
    6408: (1028, 1536, 2048),             # Swin PatchMerging on 4 * 384; the projectors (2048)
    6412: (2052, 2400, 3072),             # Swin PatchMerging on 4 * 768
}
LN_ROWS = [(code, c) for code in sorted(LN_LEDGER) for c in LN_LEDGER[code]]
LN_PLANE_ROWS = [(code, c) for code, c in LN_ROWS if c % 32 == 0]
LN_N, LN_R = 3, 13      # M = 39 rows: the last workgroup is ragged for 16, 8 and 4 rows per workgroup (LPR 16 / 32 / 64)

# squeeze-excite gate: code -> (C, F, rows, N)
SE_LEDGER = {
    1: ((54, 8, 37, 3), (108, 8, 5, 3), (216, 16, 700, 2), (432, 32, 23, 3),      # X3D-L's own gates (_se_width)
        (512, 32, 50, 2),         # C = 512 exactly: two row groups
        (100, 17, 24, 3),         # second hidden unit on one wave only; C not a multiple of 64
        (320, 32, 10, 3),         # C > 256, G * C = 960 < 1024: idle threads
        (216, 16, 5, 2),          # rows < 24: one partial batch
        (8, 1, 1, 1)),            # one row, one hidden unit
    2: ((768, 48, 30, 2),         # 512 < C <= 1024: one row group
        (2048, 128, 9, 2),        # C > 1024: the strided loops
        (256, 64, 40, 3),         # F > 32 with C <= 512: four row groups
        (520, 8, 100, 2)),        # just past the preload bound
}
SE_ROWS = [(code, case) for code in sorted(SE_LEDGER) for case in SE_LEDGER[code]]
X3D_L_GATES = ((54, 8), (108, 8), (216, 16), (432, 32))


def _morph_specs(BT, H, W, Cc, sd, T=8):
    from mspi_amd.backbones import MorphMLP as M
    B = BT // T
    return {"t_gather": M.t_gather(B, T, H * W, Cc), "t_scatter": M.t_scatter(B, T, H * W, Cc),
            "w_gather": M.w_gather(BT, H * W, Cc, sd), "w_scatter": M.w_scatter(BT, H * W, Cc, sd),
            "h_gather": M.h_gather(BT, H, W, Cc, sd), "h_scatter": M.h_scatter(BT, H, W, Cc, sd),
            "s2_gather": M.s2_gather(BT, H * W, Cc, sd), "s2_scatter": M.s2_scatter(BT, H * W, Cc, sd)}


def _morph_stages():
    """(C, segment_dim, H = W) of MorphMLP-S's four stages on 224 x 224 clips, from its config."""
    import os
    import yaml
    import mspi_amd
    with open(os.path.join(os.path.dirname(mspi_amd.__file__), "configs", "K400_MLP_S16x4.yaml")) as f:
        m = yaml.safe_load(f)["MORPH"]
    return [(c, sd, 224 // 4 // 2 ** i) for i, (c, sd) in enumerate(zip(m["EMBED_DIMS"], m["SEGMENT_DIM"]))]


def _permute_ledger():
    """code -> {name: (dims, strides, x offset in floats, y offset in floats)}"""
    m112, m224 = _morph_specs(8, 28, 14, 112, 14), _morph_specs(8, 28, 14, 224, 28)
    vec = {"morph_" + k: v + (0, 0) for k, v in m112.items() if not k.startswith("t_")}          # h_*: 6 real dimensions
    vec.update({"morph_" + k: v + (0, 0) for k, v in m224.items() if k.startswith("t_")})        # C / 8 = 28 floats per run
    vec["broadcast"] = ((5, 4, 8), (0, 8, 1), 0, 0)                                              # zero stride
    w = m112["w_gather"]
    sca = {"morph_t_gather": m112["t_gather"] + (0, 0),                   # MorphFC_T at C = 112: runs of C / 8 = 14 floats
           "morph_t_scatter": m112["t_scatter"] + (0, 0),
           "innermost_6": ((3, 5, 7, 6), (210, 6, 30, 1), 0, 0),          # innermost extent % 4 != 0
           "stride_10": ((4, 6, 8), (10, 40, 1), 0, 0),                   # an outer stride % 4 != 0
           "x_pointer": w + (1, 0),                                       # a source at an odd float offset
           "y_pointer": w + (0, 2),                                       # a destination 8 bytes off
           "broadcast": ((5, 3, 6), (0, 6, 1), 0, 0)}
    return {4: vec, 1: sca}


PERMUTE_LEDGER = _permute_ledger()
PERMUTE_ROWS = [(code, name) for code in sorted(PERMUTE_LEDGER) for name in sorted(PERMUTE_LEDGER[code])]

# mean over rows: form (1 = one stage, 2 = two stages through a workspace) -> (R, C, N)
MEAN_LEDGER = {
    1: ((1, 64, 2), (30, 100, 2), (1023, 129, 2)),
    2: ((1024, 64, 2), (1025, 100, 3), (3001, 65, 2), (25088, 112, 2)),      # 25088: MorphMLP's re-weighting at 8 x 56 x 56
}
MEAN_ROWS = [(form, case) for form in sorted(MEAN_LEDGER) for case in MEAN_LEDGER[form]]


def _ln_code(c, planes=0):
    return _lib().mspi_layernorm_variant(c, planes)


def _perm_desc(dims, strides, src_elems):
    from mspi_amd import _lib
    d = _lib.PermuteDesc()
    pad = 6 - len(dims)
    d.dims[:] = [1] * pad + list(dims)
    d.strides[:] = [0] * pad + list(strides)
    d.src_elems = src_elems
    return d


def _span(dims, strides):
    return sum((n - 1) * s for n, s in zip(dims, strides))


def _perm_code(dims, strides, xoff=0, yoff=0, src_elems=None):
    """mspi_permute_variant on made-up pointers (only their alignment is looked at)."""
    d = _perm_desc(dims, strides, _span(dims, strides) + 1 if src_elems is None else src_elems)
    return _lib().mspi_permute_variant(C.byref(d), 4096 + 4 * xoff, 8192 + 4 * yoff)


def _mean_form(r):
    s = _lib().mspi_mean_rows_slices(r)
    assert s == 0 or s == (r + 255) // 256
    return 2 if s else 1


# ------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("code,c", LN_ROWS, ids=["%d-C%d" % r for r in LN_ROWS])
def test_layernorm_ledger_row_selects_its_kernel(code, c):
    _no_switches(SWITCHES)
    assert _ln_code(c) == code
    assert _ln_code(c, 1) == (code if c % 32 == 0 else -1)


@pytest.mark.parametrize("code,case", SE_ROWS, ids=["se_gate-%d-C%d-F%d" % (r[0], r[1][0], r[1][1]) for r in SE_ROWS])
def test_se_gate_ledger_row_selects_its_kernel(code, case):
    _no_switches(SWITCHES)
    assert _lib().mspi_se_gate_variant(case[0], case[1]) == code


@pytest.mark.parametrize("code,name", PERMUTE_ROWS, ids=["permute-%d-%s" % r for r in PERMUTE_ROWS])
def test_permute_ledger_row_selects_its_kernel(code, name):
    _no_switches(SWITCHES)
    dims, strides, xoff, yoff = PERMUTE_LEDGER[code][name]
    assert _perm_code(dims, strides, xoff, yoff) == code


@pytest.mark.parametrize("form,case", MEAN_ROWS, ids=["mean_rows-%d-R%d" % (r[0], r[1][0]) for r in MEAN_ROWS])
def test_mean_rows_ledger_row_selects_its_form(form, case):
    assert _mean_form(case[0]) == form


def _ln_sweep():
    return {c: _ln_code(c) for c in range(4, 3073, 4)}


def test_ledgers_cover_every_reachable_kernel():
    _no_switches(SWITCHES)
    lib = _lib()
    seen = set(_ln_sweep().values())
    assert seen == set(LN_LEDGER), "LayerNorm codes without a row / rows never reached: %s" % (seen ^ set(LN_LEDGER))
    seen = {lib.mspi_se_gate_variant(c, f) for c in list(range(1, 1100, 7)) + [512, 513, 1024, 1025, 2048, 4096, 8000]
            for f in (1, 8, 16, 17, 32, 33, 64, 128, 512)}
    assert seen - {-1} == set(SE_LEDGER), "gate codes without a row / rows never reached: %s" % ((seen - {-1}) ^ set(SE_LEDGER))
    seen = set()
    for inner in (1, 3, 4, 6, 8, 12):
        for outer in ((5,), (3, 5), (2, 3, 4), (2, 1, 3, 2, 2)):
            for smul in (1, 2, 4, 5, 8):
                dims = outer + (inner,)
                strides, acc = [], inner
                for n in reversed(outer):
                    strides.insert(0, acc * smul)
                    acc *= n * smul
                for xoff in (0, 1, 2, 4):
                    for yoff in (0, 1, 4):
                        seen.add(_perm_code(dims, tuple(strides) + (1,), xoff, yoff))
    assert seen == set(PERMUTE_LEDGER), "permute codes without a row / rows never reached: %s" % (seen ^ set(PERMUTE_LEDGER))
    seen = {_mean_form(r) for r in range(1, 30001)}
    assert seen == set(MEAN_LEDGER)


def test_ledger_rows_sit_on_the_edges():
    """Each LayerNorm bucket holds its smallest C, its largest C and a C whose float4 count is not a multiple of the lanes per
    row; the gate rows straddle the preload bound; the mean rows straddle the switch between the forms."""
    sweep = _ln_sweep()
    for code, widths in LN_LEDGER.items():
        bucket = [c for c, v in sweep.items() if v == code]
        lpr = code // 100
        assert min(widths) == min(bucket) and max(widths) == max(bucket), (code, min(bucket), max(bucket))
        assert any((c // 4) % lpr for c in widths), "bucket %d has no row with masked tail lanes" % code
        assert all(sweep[c] == code for c in widths)
    lib = _lib()
    assert (512, 32) in {c[:2] for c in SE_LEDGER[1]} and lib.mspi_se_gate_variant(513, 32) == 2 == lib.mspi_se_gate_variant(512, 33)
    assert {c[0] for c in MEAN_LEDGER[1]} >= {1, 1023} and {c[0] for c in MEAN_LEDGER[2]} >= {1024, 1025}


def _model_layernorm_widths():
    """{encoder: {top-level module: widths}} of every nn.LayerNorm the audio-visual model holds, per motion encoder."""
    import torch.nn as nn
    from mspi_amd import config, testing as T
    from mspi_amd.model.model_utils import AudioVisualSaliencyModel
    out = {}
    for name in config._MOTION_ENCODERS:
        model = AudioVisualSaliencyModel(T.make_cfg(name))
        w = {}
        for n, m in model.named_modules():
            if isinstance(m, nn.LayerNorm):
                assert len(m.normalized_shape) == 1
                w.setdefault(n.split(".")[0], set()).add(m.normalized_shape[0])
        out[name] = w
    return out


def test_production_shapes_keep_their_kernels():
    """Model shapes pinned to the kernel they run today (read from the modules, not from a table): a dispatch change that
    moves one of them onto another instantiation must show up here."""
    _no_switches(SWITCHES)
    from mspi_amd.backbones.blocks3d import _se_width
    lib = _lib()
    widths = _model_layernorm_widths()
    assert len(widths) == 7
    pins = {"mvitv2s": {96: 1602, 192: 1604, 384: 3204, 768: 6404},
            "morphmlps": {112: 1602, 224: 1604, 392: 3204, 784: 6404},
            "uniformerb": {64: 1601, 128: 1602, 320: 3204, 512: 3204},
            "videoswins": {96: 1602, 192: 1604, 384: 3204, 768: 6404, 1536: 6408},
            "s3d": {}, "slowfast4x16": {}, "x3dl": {}}
    head = {"image_encoder": {96: 1602, 192: 1604, 384: 3204, 768: 6404},       # ConvNeXt-T
            "aud_vis_sync_block": {512: 3204}, "mlp_vis": {512: 3204}, "mlp_aud": {512: 3204},
            "vis_projector": {2048: 6408}, "aud_projector": {2048: 6408}}
    head.update({"latlayer_%d" % i: {192: 1604} for i in range(4)})              # fusion head ConvNextBlocks
    for name, mods in widths.items():
        want = dict(head)
        if pins[name]:
            want["visnet"] = pins[name]
        assert {k: sorted(v) for k, v in mods.items()} == {k: sorted(v) for k, v in want.items()}, name
        for mod, table in want.items():
            for c, code in table.items():
                assert _ln_code(c) == code, (name, mod, c)
                assert c in LN_LEDGER[code], "model width %d has no GPU row" % c
    # X3D-L's squeeze-excite pairs: the register-preloaded kernel, each also a GPU row
    for dim in (54, 108, 216, 432):
        pair = (dim, _se_width(dim, 0.0625))
        assert pair in X3D_L_GATES and pair in {c[:2] for c in SE_LEDGER[1]}
        assert lib.mspi_se_gate_variant(*pair) == 1
    # MorphMLP's regroupings at 224 x 224 (8 frames after the stem).  The spatial ones move runs of C / segment_dim = 8, 8, 14, 16
    # floats, MorphFC_T runs of C / 8 = 14, 28, 49, 98: a run that is not a multiple of 4 floats is on the scalar kernel
    stages = _morph_stages()
    assert stages == [(112, 14, 56), (224, 28, 28), (392, 28, 14), (784, 49, 7)]
    for (Cc, sd, hw), spatial, temporal in zip(stages, (4, 4, 1, 4), (1, 4, 1, 1)):
        for which, (dims, strides) in _morph_specs(16, hw, hw, Cc, sd).items():
            assert _perm_code(dims, strides) == (temporal if which.startswith("t_") else spatial), (Cc, which)
    assert _mean_form(8 * 56 * 56) == 2 and _mean_form(8 * 7 * 7) == 1


def test_variant_queries_refuse_what_the_launches_refuse():
    lib = _lib()
    for c in (0, -4, 2, 6, 98, 3073, 3076, 4096):
        assert lib.mspi_layernorm_variant(c, 0) == -1, c
    assert b"multiple of 4" in lib.mspi_last_error()
    for c in (4, 48, 100, 3056):
        assert lib.mspi_layernorm_variant(c, 0) > 0 and lib.mspi_layernorm_variant(c, 1) == -1      # planes need C % 32 == 0
    assert b"C % 32" in lib.mspi_last_error()
    assert lib.mspi_layernorm_variant(3072, 1) == 6412
    # the gate's LDS bound: (G * C + C + F) floats <= 64 KB with G = 1024 / C row groups (1 beyond C = 1024)
    for c, f, ok in ((0, 8, False), (8, 0, False), (512, 32, True), (1024, 14336, True), (1024, 14337, False),
                     (8000, 384, True), (8000, 385, False), (8192, 1, False), (1, 15359, True), (1, 15360, False)):
        g = 1024 // c if 0 < c <= 1024 else 1
        assert ok == (c > 0 and f > 0 and 4 * (g * c + c + f) <= 65536)
        assert (lib.mspi_se_gate_variant(c, f) > 0) == ok, (c, f)
    # permute: the reads must stay inside the declared source; innermost run contiguous; positive extents
    dims, strides = (4, 6, 8), (12, 48, 1)
    span = _span(dims, strides)
    assert _perm_code(dims, strides, src_elems=span + 1) == 4 and _perm_code(dims, strides, src_elems=span) == -1
    assert b"source" in lib.mspi_last_error()
    assert _perm_code((4, 8), (16, 2)) == -1 and b"contiguous" in lib.mspi_last_error()
    assert _perm_code((4, 0, 8), (16, 8, 1), src_elems=100) == -1
    assert _perm_code((4, 8), (-8, 1), src_elems=100) == -1
    d = _perm_desc((4, 8), (8, 1), 32)
    assert lib.mspi_permute_variant(C.byref(d), None, 4096) == -1 and lib.mspi_permute_variant(None, 4096, 4096) == -1
    assert lib.mspi_permute_variant(C.byref(d), 4096, 4096) == 4


def test_postprocess_refuses_maps_smaller_than_the_blur_radius():
    """H or W < 6: the kernel reflects once and then clamps, OpenCV reflects repeatedly, the oracle's reflect padding refuses
    the map outright -- no reference defines the result, so the entry point refuses (before any GPU call)."""
    lib = _lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    for h, w in ((5, 40), (40, 5), (1, 1), (2, 2)):
        assert lib.mspi_postprocess_u8(p, p, p, 1, h, w, 16, 16, None) == -1
        assert b"smaller than the blur radius" in lib.mspi_last_error() and b"no reference" in lib.mspi_last_error()
    assert lib.mspi_postprocess_u8(p, p, p, 0, 6, 6, 16, 16, None) == -1 and b"bad argument" in lib.mspi_last_error()


# ------------------------------------------------------------------------------------------- the cases and their references
# Every toleranced case is a function of a dtype: float64 gives the reference, float32 the "plain fp32 evaluation" that has to
# sit 4x inside the bar.  The operands are drawn in fp32 (what the kernel sees) and converted.
def _ln_inputs(c):
    g = torch.Generator().manual_seed(c)
    x = torch.randn(LN_N, LN_R, c, generator=g) * 3 + 1
    return x, torch.randn(c, generator=g), torch.randn(c, generator=g), torch.randn(LN_R, c, generator=g)


def _ln_eval(t, act, table, dt, eps=1e-5):
    x, gm, bt, tab = (v.to(dt) for v in t)
    y = _act(F.layer_norm(x, x.shape[-1:], gm, bt, eps), act)
    return y + tab if table else y


def _emulate_split(y):
    """fp32 -> f16 hi + f16 lo -> fp32, as the planes carry it."""
    hi = y.half()
    return hi.float() + (y - hi.float()).half().float()


def _se_inputs(case):
    c, f, rows, n = case
    g = torch.Generator().manual_seed(c * 131 + f)
    pool = torch.randn(n, rows, c, generator=g) * 50 / rows ** 0.5
    return (pool, torch.randn(f, c, generator=g) * c ** -0.5, torch.randn(f, generator=g),
            torch.randn(c, f, generator=g) * f ** -0.5, torch.randn(c, generator=g))


SE_INV = 1 / 100.0


def _se_eval(t, dt):
    pool, w1, b1, w2, b2 = (v.to(dt) for v in t)
    return torch.sigmoid(F.linear(F.relu(F.linear(pool.sum(1) * SE_INV, w1, b1)), w2, b2))


# up-sample: (NT, H, W, C, factor, accumulate, act)
UPSAMPLE_CASES = [(2, 7, 7, 192, 2, False, 0),       # fusion head: s1 -> cat.slice(192, 192)
                  (2, 5, 7, 192, 4, False, 0), (1, 3, 4, 192, 8, False, 0),
                  (3, 5, 6, 24, 1, False, 0),         # factor 1
                  (2, 1, 9, 16, 4, True, 1), (2, 9, 1, 16, 2, True, 2), (1, 1, 1, 8, 8, False, 3),      # H or W = 1
                  (2, 6, 5, 40, 2, True, 4), (2, 6, 5, 40, 2, False, 1), (2, 4, 5, 12, 8, True, 0)]


def _up_inputs(case):
    nt, h, w, c, k, acc, act = case
    g = torch.Generator().manual_seed(h * 100 + w * 10 + k)
    return torch.randn(nt, c, 1, h, w, generator=g), torch.randn(nt, c, 1, h * k, w * k, generator=g)


def _up_eval(t, case, dt):
    k, acc, act = case[4:]
    x, base = (v.to(dt) for v in t)
    y = F.interpolate(x, scale_factor=(1, k, k), mode="trilinear", align_corners=False) if k > 1 else x
    return _act(y + base if acc else y, act)


ROWGATE_CASES = [(2, 3, 5, 7, 24), (1, 1, 9, 9, 192), (3, 2, 1, 1, 4)]      # (N, T, H, W, C)


def _rowgate_inputs(case):
    n, t, h, w, c = case
    g = torch.Generator().manual_seed(c + h)
    return torch.randn(n, c, t, h, w, generator=g), torch.rand(n, 1, t, h, w, generator=g)


def _rowgate_eval(t, dt):
    x, m = (v.to(dt) for v in t)
    return x * (1 + m)


# MViT augment: (DA, k_thw): Dh = 96, J = kT + kH + kW relative-position columns, zero columns from Dh + J to DA
AUG_CASES = [(128, (2, 3, 3)), (128, (2, 5, 6)), (128, (8, 7, 7)), (144, (8, 14, 14)), (144, (3, 7, 9)), (160, (8, 21, 22)),
             (160, (4, 6, 6)), (160, (16, 24, 24))]
AUG_Q = (2, 3, 4)
AUG_B, AUG_HEADS, AUG_DH = 2, 2, 96


def _aug_inputs(case):
    da, k_thw = case
    g = torch.Generator().manual_seed(da + sum(k_thw))
    nq, nk = math.prod(AUG_Q), math.prod(k_thw)
    q = torch.randn(AUG_B, nq, AUG_HEADS * AUG_DH, generator=g)
    k = torch.randn(AUG_B, nk, AUG_HEADS * AUG_DH, generator=g)
    Rt, Rh, Rw = (torch.randn(AUG_Q[i], k_thw[i], AUG_DH, generator=g) * 0.3 for i in range(3))
    return q, k, Rh, Rw, Rt


def _aug_rel_eval(t, case, dt):
    """The J dot-product columns [B, heads, Nq, J] (order: kH, kW, kT)."""
    q, _, Rh, Rw, Rt = (v.to(dt) for v in t)
    qh = q.view(AUG_B, *AUG_Q, AUG_HEADS, AUG_DH)                       # [b, t, h, w, head, c]
    return torch.cat([torch.einsum("bthwyc,hkc->bythwk", qh, Rh), torch.einsum("bthwyc,wkc->bythwk", qh, Rw),
                      torch.einsum("bthwyc,tkc->bythwk", qh, Rt)], -1).reshape(AUG_B, AUG_HEADS, math.prod(AUG_Q), -1)


GATED_CASES = [(3, 50, 56, 2), (3, 50, 56, 3), (5, 1, 100, 3), (4, 1, 8, 2), (2, 392, 112, 3)]      # (N, rows per sample, C, J)


def _gated_inputs(case):
    n, r, c, j = case
    g = torch.Generator().manual_seed(n * 1000 + c + j)
    return [torch.randn(n, r, c, generator=g) for _ in range(j)] + [(torch.rand(n, c * j, generator=g) * 2 - 1) * 80]


def _gated_eval(t, case, dt):
    n, r, c, j = case
    a = t[-1].to(dt).reshape(n, c, j).permute(2, 0, 1).softmax(0)[:, :, None, :]
    return sum(a[i] * t[i].to(dt) for i in range(j))


LSE_CASES = [(3, 1), (2, 100), (2, 1023), (2, 1025), (3, 50176)]      # (N, L); L = 1: an all-zero result, asserted exactly


def _lse_inputs(case):
    g = torch.Generator().manual_seed(case[1])
    return (torch.rand(*case, generator=g) * 2 - 1) * 80


def _lse_eval(x, dt):
    x = x.to(dt)
    return x - torch.logsumexp(x, 1, keepdim=True)


def _mean_inputs(case):
    r, c, n = case
    g = torch.Generator().manual_seed(r + c)
    return torch.randn(n, r, c, generator=g) + 0.5


COS_CASES = [(4, 2048, False), (3, 100, True), (5, 260, True), (1, 4, False)]      # (N, C, one zero vector)


def _cos_inputs(case):
    n, c, zero = case
    g = torch.Generator().manual_seed(c)
    p, z = torch.randn(n, c, generator=g), torch.randn(n, c, generator=g)
    if zero:
        p[n // 2] = 0
    return p, z


def _cos_eval(t, dt):
    p, z = (v.to(dt) for v in t)
    return -F.cosine_similarity(p, z, dim=-1, eps=1e-8).mean().view(1)


def _toleranced_cases():
    """(name, tolerance, fp32 evaluation, fp64 reference) of every GPU case that has a tolerance."""
    for code, c in LN_ROWS:
        t = _ln_inputs(c)
        for act in ACTS:
            for table in (False, True):
                yield "layernorm %d C=%d act=%d table=%d" % (code, c, act, table), TOL, _ln_eval(t, act, table, torch.float32), \
                    _ln_eval(t, act, table, torch.float64)
    for code, c in LN_PLANE_ROWS:
        t = _ln_inputs(c)
        yield "layernorm planes %d C=%d" % (code, c), TOL, _emulate_split(_ln_eval(t, 0, False, torch.float32)), \
            _ln_eval(t, 0, False, torch.float64)
    for code, case in SE_ROWS:
        t = _se_inputs(case)
        yield "se_gate-%d %s" % (code, case), TOL, _se_eval(t, torch.float32), _se_eval(t, torch.float64)
    for case in UPSAMPLE_CASES:
        t = _up_inputs(case)
        yield "upsample %s" % (case,), TOL, _up_eval(t, case, torch.float32), _up_eval(t, case, torch.float64)
    for case in ROWGATE_CASES:
        t = _rowgate_inputs(case)
        yield "rowgate %s" % (case,), TOL, _rowgate_eval(t, torch.float32), _rowgate_eval(t, torch.float64)
    for case in AUG_CASES:
        t = _aug_inputs(case)
        yield "mvit augment %s" % (case,), TOL, _aug_rel_eval(t, case, torch.float32), _aug_rel_eval(t, case, torch.float64)
    for case in GATED_CASES:
        t = _gated_inputs(case)
        yield "gated_sum %s" % (case,), TOL, _gated_eval(t, case, torch.float32), _gated_eval(t, case, torch.float64)
    for case in LSE_CASES:
        if case[1] > 1:
            x = _lse_inputs(case)
            yield "logsumexp %s" % (case,), TOL, _lse_eval(x, torch.float32), _lse_eval(x, torch.float64)
    for form, case in MEAN_ROWS:
        x = _mean_inputs(case)
        yield "mean_rows-%d %s" % (form, case), TOL, x.mean(1), x.double().mean(1)
    for case in COS_CASES:
        t = _cos_inputs(case)
        yield "neg_cosine %s" % (case,), TOL, _cos_eval(t, torch.float32), _cos_eval(t, torch.float64)


def test_fp32_evaluation_is_4x_inside_every_bar():
    """The bar is reachable by a correct fp32 kernel: torch in fp32 on the CPU, against the fp64 reference, errs by at most a
    quarter of each GPU case's tolerance.  If this fails, change the inputs, not the tolerance."""
    n = 0
    for name, tol, got, ref in _toleranced_cases():
        scale = ref.abs().max().item()
        err = (got.double() - ref).abs().max().item()
        assert scale > 0 and err <= 0.25 * tol * scale, "%s: fp32 torch errs by %.2e of max|ref|" % (name, err / scale)
        n += 1
    assert n > 300


# post-process: (N, H, W, Ho, Wo); L = Ho * Wo % 16 = 0, 9, 1, 3, 4, 13 -- with N = 3 maps 1 and 2 of the unaligned sizes
# start at addresses that are not 16-byte aligned (the scalar path of quantize_kernel)
PP_CASES = [(3, 224, 224, 480, 640), (3, 224, 224, 45, 77), (3, 64, 96, 33, 33), (3, 6, 6, 33, 35), (3, 7, 12, 30, 30),
            (3, 224, 384, 37, 41)]


def _pp_maps(case):
    n, h, w = case[:3]
    return torch.randn(n, h, w, generator=torch.Generator().manual_seed(h + w)) * 2 - 9


def _pp_f64(logmap, out_hw):
    """oracle.restate.postprocess_u8 evaluated in float64."""
    k = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / 8.0)
    k = k / k.sum()
    x = F.pad(logmap[None, None].double(), (5, 5, 5, 5), mode="reflect")
    x = torch.exp(F.conv2d(F.conv2d(x, k.view(1, 1, 1, 11)), k.view(1, 1, 11, 1)))
    x = F.interpolate(x, size=out_hw, mode="bilinear", align_corners=False)[0, 0]
    return torch.round((x - x.min()) / (x.max() - x.min()) * 255).to(torch.uint8)


@pytest.mark.parametrize("case", PP_CASES, ids=["%dx%d-%dx%d" % c[1:] for c in PP_CASES])
def test_postprocess_reference_is_well_inside_its_cap(case):
    """The cap of the GPU test (1 grey level, < 2 % of the pixels) holds for the reference alone with room to spare: the fp32
    oracle against an fp64 evaluation of the same pipeline differs by one level on at most 0.5 % of the pixels (rounding ties)."""
    from oracle import restate as R
    assert (case[3] * case[4]) % 16 in (0, 9, 1, 3, 4, 13)
    maps = _pp_maps(case)
    for i in range(case[0]):
        d = (R.postprocess_u8(maps[i], case[3:]).int() - _pp_f64(maps[i], case[3:]).int()).abs()
        assert d.max() <= 1 and (d > 0).float().mean() <= 0.005, (case, i, d.max().item(), (d > 0).float().mean().item())


# ------------------------------------------------------------------------------------------------------------ GPU tests
def _poisoned(E, N, T, H, W, Cc, dev, ld, fill):
    t = E.alloc(N, T, H, W, Cc, dev, ld=ld)
    t.buf.fill_(fill)
    return t


def _put(E, t5, dev, left=0, right=0, fill=BIG):
    """NCDHW cpu tensor -> columns [left, left + C) of rows left + C + right wide; the other columns hold `fill`."""
    N, Cc, T, H, W = t5.shape
    wide = _poisoned(E, N, T, H, W, left + Cc + right, dev, left + Cc + right, fill)
    view = wide.slice(left, Cc)
    view.as_ncdhw().copy_(t5.to(dev))
    return wide, view


def _outside(wide, left, Cc):
    rows = wide.buf.view(-1, wide.ld)
    return torch.cat([rows[:, :left].reshape(-1), rows[:, left + Cc:].reshape(-1)])


@pytest.mark.gpu
@pytest.mark.parametrize("code,c", LN_ROWS, ids=["%d-C%d" % r for r in LN_ROWS])
def test_layernorm_ledger_kernel_vs_fp64(dev, code, c):
    """Each LayerNorm row x {dense, token-slab input, token-slab output, in place} x every activation x {table, none}: M = 39
    rows (ragged last workgroup), input pads at 1e6, outputs NaN-filled, rows and columns outside the slab untouched."""
    from mspi_amd import engine as E
    _no_switches(SWITCHES)
    assert _ln_code(c) == code
    t = _ln_inputs(c)
    x, gm, bt, tab = (v.to(dev) for v in t)
    N, R, pre = LN_N, LN_R, 4
    worst = 0.0
    for act in ACTS:
        for table in (False, True):
            ref = _ln_eval(t, act, table, torch.float64)
            for layout in ("dense", "slab_in", "slab_out", "in_place"):
                what = "layernorm %d C=%d act=%d table=%d %s" % (code, c, act, table, layout)
                if layout in ("slab_in", "in_place"):       # rows [4, 4 + R) of R + 9, columns [0, C) of C + 8
                    seq = _poisoned(E, N, R + 9, 1, 1, c, dev, c + 8, BIG)
                    seq.buf.view(N, R + 9, c + 8)[:, pre:pre + R, :c] = x
                    xin = seq.tokens(pre, R, 1, 1)
                    assert not xin.dense
                else:
                    xin = E.CL(x.reshape(-1).clone(), 0, N, R, 1, 1, c, c)
                if layout == "slab_out":
                    oseq = _poisoned(E, N, R + 9, 1, 1, c, dev, c + 4, -3.0)
                    out = oseq.tokens(pre, R, 1, 1)
                elif layout == "in_place":
                    out = xin
                else:
                    out = _poisoned(E, N, R, 1, 1, c, dev, c, NAN)
                E.layernorm(xin, gm, bt, 1e-5, out=out, act=act, table=tab if table else None)
                if layout == "slab_out":
                    full = oseq.buf.view(N, R + 9, c + 4)
                    got = full[:, pre:pre + R, :c]
                    keep = torch.ones_like(full, dtype=torch.bool)
                    keep[:, pre:pre + R, :c] = False
                    assert (full[keep] == -3.0).all(), what + ": wrote outside its slab"
                elif layout == "in_place":
                    full = seq.buf.view(N, R + 9, c + 8)
                    got = full[:, pre:pre + R, :c]
                    keep = torch.ones_like(full, dtype=torch.bool)
                    keep[:, pre:pre + R, :c] = False
                    assert (full[keep] == BIG).all(), what + ": wrote outside its slab"
                else:
                    got = out.buf.view(N, R, c)
                _rel_close(got, ref, TOL, what)
                worst = max(worst, ((got.cpu().double() - ref).abs().max() / ref.abs().max()).item())
    print("layernorm %d C=%d: worst error %.2e of max|ref| (bar %.0e)" % (code, c, worst, TOL))


@pytest.mark.gpu
@pytest.mark.parametrize("code,c", LN_PLANE_ROWS, ids=["%d-C%d" % r for r in LN_PLANE_ROWS])
def test_layernorm_planes_vs_fp64(dev, code, c):
    """mspi_layernorm_sp_fwd at M % 16 = 0, 1, 15 from a token slab, read back through mspi_join_planes_fwd: element for element
    against the fp64 LayerNorm; the rows that pad the last 16-row group stay zero, as alloc_sp left them."""
    from mspi_amd import engine as E
    _no_switches(SWITCHES)
    lib = _lib()
    assert _ln_code(c, 1) == code
    g = torch.Generator().manual_seed(c + 1)
    gm, bt = torch.randn(c, generator=g), torch.randn(c, generator=g)
    gmd, btd = gm.to(dev), bt.to(dev)      # named: a temporary's memory is handed to the next allocation before the launch
    for N, R in ((3, 16), (3, 11), (3, 21)):
        M = N * R
        x = torch.randn(N, R, c, generator=g) * 3 + 1
        ref = F.layer_norm(x.double(), (c,), gm.double(), bt.double(), 1e-5)
        seq = _poisoned(E, N, R + 5, 1, 1, c, dev, c + 4, BIG)
        seq.buf.view(N, R + 5, c + 4)[:, 2:2 + R, :c] = x.to(dev)
        xin = seq.tokens(2, R, 1, 1)
        sp = E.alloc_sp(N, R, 1, 1, c, dev)
        mp = (M + 15) // 16 * 16
        blocks = sp.buf.view(2, mp // 16, c // 32, 16, 32)
        if M % 16:
            assert (blocks[:, -1, :, M % 16:] == 0).all()
        blocks.fill_(NAN)
        if M % 16:
            blocks[:, -1, :, M % 16:] = 0
        E.check(lib.mspi_layernorm_sp_fwd(xin.ptr, xin.ld, xin.sN, sp.ptr, sp.ld, sp.plane, gmd.data_ptr(),
                                          btd.data_ptr(), 1e-5, N, R, c, 0, E._stream()), "mspi_layernorm_sp_fwd")
        out = _poisoned(E, N, R, 1, 1, c, dev, c + 4, -3.0)
        E.check(lib.mspi_join_planes_fwd(sp.ptr, sp.ld, sp.plane, M, c, out.ptr, out.ld, E._stream()), "mspi_join_planes_fwd")
        got = out.buf.view(M, c + 4)
        _rel_close(got[:, :c].reshape(N, R, c), ref, TOL, "layernorm planes %d C=%d M=%d" % (code, c, M))
        assert (got[:, c:] == -3.0).all()
        if M % 16:
            assert (blocks[:, -1, :, M % 16:] == 0).all(), "pad rows of the last 16-row group were written"
        assert not torch.isnan(blocks.float()).any()


@pytest.mark.gpu
@pytest.mark.parametrize("code,case", SE_ROWS, ids=["se_gate-%d-C%d-F%d-r%d" % ((r[0],) + r[1][:3]) for r in SE_ROWS])
def test_se_gate_ledger_kernel_vs_fp64(dev, code, case):
    from mspi_amd import engine as E
    _no_switches(SWITCHES)
    c, f, rows, n = case
    assert _lib().mspi_se_gate_variant(c, f) == code
    t = _se_inputs(case)
    ref = _se_eval(t, torch.float64)
    td = [v.to(dev) for v in t]
    gate = torch.full((n, c), NAN, device=dev)
    E.se_gate(td[0], SE_INV, *td[1:], gate=gate)
    _rel_close(gate, ref, TOL, "se_gate-%d %s" % (code, case))
    again = torch.full((n, c), NAN, device=dev)
    E.se_gate(td[0], SE_INV, *td[1:], gate=again)
    assert torch.equal(gate, again), "se_gate-%d %s: two launches differ" % (code, case)
    print("se_gate-%d %s: error %.2e of max|ref| (bar %.0e)" % (code, case, ((gate.cpu().double() - ref).abs().max() / ref.abs().max()).item(), TOL))


@pytest.mark.gpu
@pytest.mark.parametrize("case", UPSAMPLE_CASES, ids=["upsample-%dx%dx%d-C%d-k%d-acc%d-act%d" % c for c in UPSAMPLE_CASES])
def test_upsample_slices_vs_fp64(dev, case):
    """Source and destination as channel slices of wider buffers (the fusion head's cat.slice); columns outside untouched."""
    from mspi_amd import engine as E
    nt, h, w, c, k, acc, act = case
    t = _up_inputs(case)
    ref = _up_eval(t, case, torch.float64)
    _, src = _put(E, t[0], dev, left=8, right=4)
    if acc:
        wide, dst = _put(E, t[1], dev, left=c, right=12, fill=-3.0)
    else:
        wide = _poisoned(E, nt, 1, h * k, w * k, 2 * c + 12, dev, 2 * c + 12, -3.0)
        dst = wide.slice(c, c)
        dst.as_ncdhw().fill_(NAN)
    assert src.ld > src.C and dst.ld > dst.C
    E.upsample(src, k, dst=dst, accumulate=acc, act=act)
    _rel_close(dst.as_ncdhw(), ref, TOL, "upsample %s" % (case,))
    assert (_outside(wide, c, c) == -3.0).all(), "upsample wrote outside its channel slice"
    print("upsample %s: error %.2e of max|ref|" % (case, ((dst.as_ncdhw().cpu().double() - ref).abs().max() / ref.abs().max()).item()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROWGATE_CASES, ids=["rowgate-%dx%dx%dx%d-C%d" % c for c in ROWGATE_CASES])
def test_rowgate_slice_vs_fp64(dev, case):
    from mspi_amd import engine as E
    n, tt, h, w, c = case
    t = _rowgate_inputs(case)
    wide, x = _put(E, t[0], dev, left=4, right=8, fill=-3.0)
    mask = E.CL(t[1].to(dev).reshape(-1).contiguous(), 0, n, tt, h, w, 1, 1)
    E.rowgate(x, mask)
    _rel_close(x.as_ncdhw(), _rowgate_eval(t, torch.float64), TOL, "rowgate %s" % (case,))
    assert (_outside(wide, 4, c) == -3.0).all(), "rowgate wrote outside its channel slice"


S2D_CASES = [(2, 2, 4, 6, 24), (1, 3, 2, 2, 96), (3, 1, 6, 2, 4)]      # (N, T, H, W, C)


@pytest.mark.gpu
@pytest.mark.parametrize("case", S2D_CASES, ids=["s2d-%dx%dx%dx%d-C%d" % c for c in S2D_CASES])
def test_space_to_depth_slices_exact(dev, case):
    from mspi_amd import engine as E
    n, tt, h, w, c = case
    x = torch.randn(n, c, tt, h, w, generator=torch.Generator().manual_seed(c))
    _, xs = _put(E, x, dev, left=4, right=4)
    wide = _poisoned(E, n, tt, h // 2, w // 2, 4 * c + 12, dev, 4 * c + 12, -3.0)
    out = wide.slice(8, 4 * c)
    out.as_ncdhw().fill_(NAN)
    E.space_to_depth(xs, out=out)
    rows = x.permute(0, 2, 3, 4, 1).reshape(n, tt, h // 2, 2, w // 2, 2, c)                      # [n, t, ho, dh, wo, dw, c]
    ref = rows.permute(0, 1, 2, 4, 5, 3, 6).reshape(n, tt, h // 2, w // 2, 4 * c)                 # quadrant q = 2 dw + dh
    assert torch.equal(out.as_ncdhw().cpu(), ref.permute(0, 4, 1, 2, 3))
    assert (_outside(wide, 8, 4 * c) == -3.0).all(), "space_to_depth wrote outside its channel slice"


# max-pool: (N, C, T, H, W, kernel, stride, pad): the windows the models use, odd extents
MAXPOOL_CASES = [(2, 24, 4, 7, 9, (2, 2, 2), (2, 2, 2), (0, 0, 0)),       # S3D (pool, 2, 2) / (pool, 2, 2)
                 (2, 24, 4, 7, 9, (4, 2, 2), (4, 2, 2), (0, 0, 0)),
                 (2, 40, 8, 5, 7, (4, 1, 1), (4, 1, 1), (0, 0, 0)),       # fusion head (s, 1, 1) / (s, 1, 1)
                 (2, 40, 6, 5, 7, (2, 1, 1), (2, 1, 1), (0, 0, 0)),
                 (1, 16, 5, 9, 11, (3, 3, 3), (2, 2, 2), (1, 1, 1)),      # S3D base2, odd extents
                 (1, 16, 3, 7, 7, (3, 3, 3), (1, 1, 1), (1, 1, 1)),       # S3D / fusion head branch 3
                 (2, 96, 2, 7, 9, (1, 3, 3), (1, 2, 2), (0, 1, 1)),       # MViT kernel_skip, stems
                 (1, 8, 1, 1, 1, (1, 3, 3), (1, 2, 2), (0, 1, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", MAXPOOL_CASES, ids=["maxpool-k%d%d%d-s%d%d%d-C%d" % (c[5] + c[6] + (c[1],)) for c in MAXPOOL_CASES])
def test_maxpool_windows_exact(dev, case):
    """dw_kernel<true>: exact against F.max_pool3d for a mixed-sign and an all-negative input (the -inf identity against zero
    padding), from a channel slice into a channel slice (out=cat.slice(..)), neighbours untouched."""
    from mspi_amd import engine as E
    N, Cc, T, H, W, k, s, p = case
    g = torch.Generator().manual_seed(Cc + T + H)
    for x in (torch.randn(N, Cc, T, H, W, generator=g), -torch.rand(N, Cc, T, H, W, generator=g) - 1):
        ref = F.max_pool3d(x, k, s, p)
        _, xs = _put(E, x, dev, left=4, right=8)
        To, Ho, Wo = ref.shape[2:]
        wide = _poisoned(E, N, To, Ho, Wo, Cc + 20, dev, Cc + 20, -3.0)
        out = wide.slice(12, Cc)
        out.as_ncdhw().fill_(NAN)
        E.maxpool(xs, k, s, p, out=out)
        assert torch.equal(out.as_ncdhw().cpu(), ref), "maxpool %s" % (case,)
        assert (_outside(wide, 12, Cc) == -3.0).all(), "maxpool wrote outside its channel slice"
        dense = E.maxpool(xs, k, s, p)
        assert torch.equal(dense.as_ncdhw().cpu(), ref)


def _aug_desc(da, k_thw, ldq, ldk):
    from mspi_amd import _lib
    a = _lib.MvitAugDesc()
    a.B, a.heads, a.Dh, a.DA = AUG_B, AUG_HEADS, AUG_DH, da
    a.qT, a.qH, a.qW = AUG_Q
    a.kT, a.kH, a.kW = k_thw
    a.ldq, a.ldk, a.scale = ldq, ldk, AUG_DH ** -0.5
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["rel", "gather"])
@pytest.mark.parametrize("case", AUG_CASES, ids=["mvit_aug-DA%d-k%dx%dx%d" % ((c[0],) + c[1]) for c in AUG_CASES])
def test_mvit_augment_buffers(dev, case, entry):
    """mspi_mvit_qk_augment (copy + rel kernels) and mspi_mvit_qk_augment_p (copy + gather) into NaN-filled qa / ka: the copied
    columns, the one-hot columns and every column from Dh + J to DA exactly; the J dot products against fp64 (rel) or exactly
    (gather, from a P computed in fp64 and rounded on the host)."""
    from mspi_amd import engine as E
    lib = _lib()
    da, k_thw = case
    Dh, heads, B = AUG_DH, AUG_HEADS, AUG_B
    nq, nk, J = math.prod(AUG_Q), math.prod(k_thw), sum(k_thw)
    kT, kH, kW = k_thw
    t = _aug_inputs(case)
    q, k, Rh, Rw, Rt = t
    ld = heads * Dh + 8                                             # q / k rows as channel slices of wider rows
    qd = torch.full((B * nq, ld), BIG, device=dev)
    kd = torch.full((B * nk, ld), BIG, device=dev)
    qd[:, :heads * Dh] = q.reshape(B * nq, -1).to(dev)
    kd[:, :heads * Dh] = k.reshape(B * nk, -1).to(dev)
    qa = torch.full((B, heads, nq, da), NAN, device=dev)
    ka = torch.full((B, heads, nk, da), NAN, device=dev)
    a = _aug_desc(da, k_thw, ld, ld)
    rel64 = _aug_rel_eval(t, case, torch.float64)
    if entry == "rel":
        tabs = [v.to(dev).contiguous() for v in (Rh, Rw, Rt)]
        E.check(lib.mspi_mvit_qk_augment(C.byref(a), qd.data_ptr(), kd.data_ptr(), *[v.data_ptr() for v in tabs], qa.data_ptr(),
                                         ka.data_ptr(), E._stream()), "mspi_mvit_qk_augment")
    else:
        # P = q rows (b, token, head) x every table row, in fp64, rounded once; its columns shuffled so the indices matter
        g = torch.Generator().manual_seed(da)
        allrows = torch.cat([Rh.reshape(-1, Dh), Rw.reshape(-1, Dh), Rt.reshape(-1, Dh)])
        ncol = allrows.shape[0]
        perm = torch.randperm(ncol, generator=g)
        where = torch.empty(ncol, dtype=torch.int64)
        where[perm] = torch.arange(ncol)                                            # table row r sits in column where[r]
        P = (q.reshape(B * nq * heads, Dh).double() @ allrows.double().t()).float()[:, perm]
        ldp = (ncol + 3) // 4 * 4 + 4
        Pd = torch.full((B * nq * heads, ldp), BIG, device=dev)
        Pd[:, :ncol] = P.to(dev)
        nh, nw = AUG_Q[1] * kH, AUG_Q[2] * kW
        idx = [where[:nh].view(AUG_Q[1], kH), where[nh:nh + nw].view(AUG_Q[2], kW), where[nh + nw:].view(AUG_Q[0], kT)]
        idx = [v.to(torch.int32).to(dev).contiguous() for v in idx]
        E.check(lib.mspi_mvit_qk_augment_p(C.byref(a), qd.data_ptr(), kd.data_ptr(), Pd.data_ptr(), ldp, *[v.data_ptr() for v in idx],
                                           qa.data_ptr(), ka.data_ptr(), E._stream()), "mspi_mvit_qk_augment_p")
        # what the gather must deliver, bit for bit: the fp32 P entries
        tok = torch.arange(nq)
        wq, hq, tq = tok % AUG_Q[2], (tok // AUG_Q[2]) % AUG_Q[1], tok // (AUG_Q[2] * AUG_Q[1])
        cols = torch.cat([idx[0].cpu().long()[hq], idx[1].cpu().long()[wq], idx[2].cpu().long()[tq]], 1)      # [nq, J]
        Pv = P.view(B, nq, heads, ncol).permute(0, 2, 1, 3)
        relP = torch.gather(Pv, 3, cols[None, None].expand(B, heads, nq, J))
    qa, ka = qa.cpu(), ka.cpu()
    what = "mvit augment %s %s" % (case, entry)
    kh = k.view(B, nk, heads, Dh).transpose(1, 2)
    qh = q.view(B, nq, heads, Dh).transpose(1, 2)
    assert torch.equal(ka[..., :Dh], kh), what + ": ka[:, :Dh] != k"
    assert torch.equal(qa[..., :Dh], qh * torch.tensor(Dh ** -0.5, dtype=torch.float32)), what + ": qa[:, :Dh] != fl32(scale q)"
    tok = torch.arange(nk)
    onehot = torch.zeros(nk, J)
    onehot[tok, (tok // kW) % kH] = 1
    onehot[tok, kH + tok % kW] = 1
    onehot[tok, kH + kW + tok // (kW * kH)] = 1
    assert torch.equal(ka[..., Dh:Dh + J], onehot.expand(B, heads, nk, J)), what + ": one-hot columns"
    assert (ka[..., Dh + J:] == 0).all() and not torch.isnan(ka).any(), what + ": ka columns past Dh + J are not zero"
    assert (qa[..., Dh + J:] == 0).all() and not torch.isnan(qa).any(), what + ": qa columns past Dh + J are not zero"
    if entry == "rel":
        _rel_close(qa[..., Dh:Dh + J], rel64, TOL, what)
    else:
        assert torch.equal(qa[..., Dh:Dh + J], relP), what + ": gathered columns"


@pytest.mark.gpu
@pytest.mark.parametrize("code,name", PERMUTE_ROWS, ids=["permute-%d-%s" % r for r in PERMUTE_ROWS])
def test_permute_ledger_kernel_exact(dev, code, name):
    from mspi_amd import engine as E
    lib = _lib()
    dims, strides, xoff, yoff = PERMUTE_LEDGER[code][name]
    n_src, n = _span(dims, strides) + 1, math.prod(dims)
    src = torch.randn(n_src, generator=torch.Generator().manual_seed(n))
    xbuf = torch.full((n_src + xoff + 4,), BIG, device=dev)
    xbuf[xoff:xoff + n_src] = src.to(dev)
    ybuf = torch.full((n + yoff + 8,), NAN, device=dev)
    ybuf[:yoff] = -3.0
    ybuf[yoff + n:] = -3.0
    d = _perm_desc(dims, strides, n_src)
    xp, yp = xbuf.data_ptr() + 4 * xoff, ybuf.data_ptr() + 4 * yoff
    assert lib.mspi_permute_variant(C.byref(d), xp, yp) == code
    E.check(lib.mspi_permute_fwd(C.byref(d), xp, yp, E._stream()), "mspi_permute_fwd")
    assert torch.equal(ybuf[yoff:yoff + n].cpu(), src.as_strided(tuple(dims), tuple(strides)).reshape(-1)), "permute-%d %s" % (code, name)
    assert (ybuf[:yoff] == -3.0).all() and (ybuf[yoff + n:] == -3.0).all(), "permute-%d %s wrote outside its output" % (code, name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GATED_CASES, ids=["gated_sum-N%d-R%d-C%d-J%d" % c for c in GATED_CASES])
def test_gated_sum_wide_logits_vs_fp64(dev, case):
    from mspi_amd import engine as E
    n, r, c, j = case
    t = _gated_inputs(case)
    cls = [E.CL(s_.to(dev).reshape(-1), 0, n, 1, r, 1, c, c) for s_ in t[:j]]
    out = _poisoned(E, n, 1, r, 1, c, dev, c, NAN)
    E.gated_sum(cls, t[-1].to(dev), out=out)
    _rel_close(out.buf.view(n, r, c), _gated_eval(t, case, torch.float64), TOL, "gated_sum %s" % (case,))


@pytest.mark.gpu
@pytest.mark.parametrize("case", LSE_CASES, ids=["logsumexp-N%d-L%d" % c for c in LSE_CASES])
def test_logsumexp_edges_vs_fp64(dev, case):
    from mspi_amd import engine as E
    n, L = case
    x = _lse_inputs(case)
    buf = torch.full((n * L + 8,), -3.0, device=dev)
    buf[:n * L] = x.reshape(-1).to(dev)
    E.logsumexp_sub(buf, n, L)
    got = buf[:n * L].view(n, L)
    if L == 1:
        assert (got == 0).all(), "logsumexp of one element is the element: x - lse must be exactly 0"
    else:
        _rel_close(got, _lse_eval(x, torch.float64), TOL, "logsumexp %s" % (case,))
    assert (buf[n * L:] == -3.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("form,case", MEAN_ROWS, ids=["mean_rows-%d-R%d-C%d" % ((r[0],) + r[1][:2]) for r in MEAN_ROWS])
def test_mean_rows_ledger_vs_fp64(dev, form, case):
    """Both forms from a token slab of wider rows (sample stride and row stride not dense); the two-stage form twice,
    bit-identical."""
    from mspi_amd import engine as E
    r, c, n = case
    assert _mean_form(r) == form
    x = _mean_inputs(case)
    ld = (c + 3) // 4 * 4 + 4
    seq = torch.full((n, r + 3, ld), BIG, device=dev)
    seq[:, 2:2 + r, :c] = x.to(dev)
    slab = E.CL(seq.view(-1), 2 * ld, n, r, 1, 1, c, ld, (r + 3) * ld)
    out = torch.full((n * c + 4,), NAN, device=dev)
    out[n * c:] = -3.0
    E.mean_rows(slab, n, r, out)
    _rel_close(out[:n * c].view(n, c), x.double().mean(1), TOL, "mean_rows-%d %s" % (form, case))
    assert (out[n * c:] == -3.0).all()
    again = torch.full((n * c + 4,), NAN, device=dev)
    E.mean_rows(slab, n, r, again)
    assert torch.equal(out[:n * c], again[:n * c]), "mean_rows-%d %s: two launches differ" % (form, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", COS_CASES, ids=["neg_cosine-N%d-C%d-zero%d" % c for c in COS_CASES])
def test_neg_cosine_edges_vs_fp64(dev, case):
    from mspi_amd import engine as E
    t = _cos_inputs(case)
    ref = _cos_eval(t, torch.float64)
    p, z = (E.from_rows(v.to(dev)) for v in t)
    loss = torch.full((1,), NAN, device=dev)
    E.neg_cosine(p, z, loss, 0.5, False)
    E.neg_cosine(z, p, loss, 0.5, True)
    _rel_close(loss, ref, TOL, "neg_cosine %s" % (case,))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1003, 1024, 4099])
def test_add_exact(dev, n):
    from mspi_amd import engine as E
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y = torch.full((n + 12,), NAN, device=dev)
    y[n:] = -3.0
    E.add(a.to(dev), b.to(dev), y)
    assert torch.equal(y[:n].cpu(), a + b) and (y[n:] == -3.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(33, 32), (47, 96), (7, 64), (1000, 224)])
def test_split_join_round_trip(dev, M, K):
    """|join(split(x)) - x| <= 2^-21 |x| element-wise for 2^-4 <= |x| < 2^15: hi = f16(x) leaves a residual of at most 2^-11 |x|,
    lo = f16(residual) rounds it to 2^-11 of itself (2^-22 |x|; 2^-25 absolute where lo is an f16 subnormal, which 2^-21 |x|
    covers from |x| = 2^-4), and hi + lo is exact in fp32.  A property of the format, not a measurement."""
    from mspi_amd import engine as E
    lib = _lib()
    g = torch.Generator().manual_seed(M + K)
    x = torch.exp2(torch.rand(M, K, generator=g) * 19 - 4) * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1)
    x = x.clamp(-32767.0, 32767.0)
    xd = torch.full((M, K + 4), BIG, device=dev)
    xd[:, :K] = x.to(dev)
    sp = E.alloc_sp(1, 1, 1, M, K, dev)
    mp = (M + 15) // 16 * 16
    blocks = sp.buf.view(2, mp // 16, K // 32, 16, 32)
    blocks.fill_(NAN)
    if M % 16:
        blocks[:, -1, :, M % 16:] = 0
    E.check(lib.mspi_split_planes_fwd(xd.data_ptr(), K + 4, M, K, sp.ptr, sp.ld, sp.plane, E._stream()), "mspi_split_planes_fwd")
    y = torch.full((M, K + 8), -3.0, device=dev)
    E.check(lib.mspi_join_planes_fwd(sp.ptr, sp.ld, sp.plane, M, K, y.data_ptr(), K + 8, E._stream()), "mspi_join_planes_fwd")
    got = y[:, :K].cpu()
    assert ((got.double() - x.double()).abs() <= 2.0 ** -21 * x.double().abs()).all(), \
        "worst %.3e |x|" % ((got.double() - x.double()).abs() / x.double().abs()).max().item()
    assert (y[:, K:] == -3.0).all()
    if M % 16:
        assert (blocks[:, -1, :, M % 16:] == 0).all(), "pad rows of the last 16-row group were written"


@pytest.mark.gpu
@pytest.mark.parametrize("case", PP_CASES, ids=["postprocess-%dx%d-%dx%d" % c[1:] for c in PP_CASES])
def test_postprocess_sizes_vs_oracle(dev, case):
    """Against oracle.restate.postprocess_u8 (at most 1 grey level, fewer than 2 % of the pixels differing), and every map of
    the N = 3 batch byte-identical to the same map run alone: with L % 16 != 0 maps 1 and 2 take quantize_kernel's scalar
    path, alone they take the vector path."""
    from mspi_amd import engine as E
    from oracle import restate as R
    n, h, w, ho, wo = case
    maps = _pp_maps(case)
    out = torch.full((n * ho * wo + 16,), 77, dtype=torch.uint8, device=dev)
    batch = out[:n * ho * wo].view(n, ho, wo)
    E.postprocess_u8(maps.to(dev), (ho, wo), out=batch)
    assert (out[n * ho * wo:] == 77).all(), "postprocess wrote past its last map"
    for i in range(n):
        ref = R.postprocess_u8(maps[i], (ho, wo))
        d = (batch[i].cpu().int() - ref.int()).abs()
        print("postprocess %s map %d: max diff %d, %.3f %% of pixels differ" % (case, i, d.max().item(), 100 * (d > 0).float().mean().item()))
        assert d.max() <= 1 and (d > 0).float().mean() < 0.02
        alone = E.postprocess_u8(maps[i:i + 1].to(dev), (ho, wo))
        assert torch.equal(alone[0], batch[i]), "map %d of the batch differs from the same map run alone" % i


@pytest.mark.gpu
@pytest.mark.parametrize("value", [0.0, -9.0, 3.25])
def test_postprocess_constant_map_is_all_zeros(dev, value):
    """hi == lo: the kernel promises literal zeros (the reference's 0 / 0 is no reference)."""
    from mspi_amd import engine as E
    maps = torch.full((2, 24, 40), value)
    maps[1] = torch.randn(24, 40, generator=torch.Generator().manual_seed(0))
    out = E.postprocess_u8(maps.to(dev), (45, 77)).cpu()
    assert (out[0] == 0).all(), "constant map %.2f: %d non-zero pixels" % (value, int((out[0] != 0).sum()))
    assert int(out[1].min()) == 0 and int(out[1].max()) == 255
