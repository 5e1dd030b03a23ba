"""mspi_amd.evaluate: saved saliency maps + dataset annotations -> metric table, and the two device resizes under it.

Each stage has its own yardstick on the same inputs, so an error in one stage cannot hide in another.

resize_fixations.  tests/golden/saliency_eval.npz holds fixation maps and the output of the REFERENCE's own resize_fixation
(avsp_dataloader.py:16-31; tools/gen_eval_golden.py); tests/saliency_eval_restate.py is the vectorised restatement the
generator pinned to it.  The result is binary: equal bit for bit, no tolerance.

resize_maps.  Yardstick: torch.nn.functional.interpolate(x.double(), size, mode="bilinear", align_corners=False) on the CPU
(saliency_eval_restate.resize_bilinear).  OpenCV is absent where these tests run, so parity with cv2.resize itself stays
unpinned, as for oracle.restate.postprocess_u8.  Bound, derived and not fitted: the kernel computes the source index and
the fractional weight exactly (integers) and rounds each weight once to fp32; an output is then a convex combination of
four samples evaluated in fp32 with at most 15 roundings (two weights, two complements 1 - w, six products and three sums
of the horizontal pass, two products and one sum of the vertical pass: 13 here), each of magnitude <= 2^-24 max|x| because
every intermediate is a convex combination of samples.  So |hip - exact| <= 16 * 2^-24 * max|x| absolute, with room to
spare.  An observed error above that means the coordinate arithmetic is wrong; the bound is not to be loosened.

evaluate_dataset.  The device-resized maps of every batch are copied to the host and fed to oracle.restate.saliency_metrics
and tests/saliency_auc_restate.py; tolerances are the project's own (tests/test_metrics.py, tests/test_saliency_auc.py):
KL / CC / SIM / NSS / IG relative 2e-5 with a 1e-3 floor, AUC-Judd 1e-9 absolute, shuffled AUC 1e-12.  NaN is a value: it
must appear exactly where the yardstick has it."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import saliency_auc_restate as A
import saliency_eval_restate as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_resize_bilinear_fwd", "mspi_resize_fixation_fwd")
CASES = ("real", "ties", "up", "odd", "hd", "empty", "same")
SHAPES = {"real": ((480, 640), (224, 384)), "ties": ((448, 640), (224, 320)), "up": ((100, 120), (224, 384)),
          "odd": ((37, 53), (17, 20)), "hd": ((720, 1280), (224, 384))}


def _gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "saliency_eval.npz"))
    return {k: z[k] for k in z.files}


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases(golden_dir):
    g = _gold(golden_dir)
    assert tuple(g["cases"]) == CASES
    for c in CASES:
        fix, out, to = g["%s_fix" % c], g["%s_out" % c], tuple(g["%s_to" % c])
        assert fix.dtype == np.uint8 and out.dtype == np.uint8 and out.shape == to
        assert set(np.unique(fix)) <= {0, 1} and set(np.unique(out)) <= {0, 1}
        if c in SHAPES:
            assert (fix.shape, to) == SHAPES[c]
        if c != "empty":                      # bottom corners are fixations: the step back from `row` / `col` is exercised
            assert fix[-1, 0] == 1 and fix[-1, -1] == 1
            assert c == "up" or (out[-1, 0] == 1 and out[-1, -1] == 1)       # enlarging, the corner stays inside: 99 -> 222
    assert g["empty_fix"].sum() == 0 and g["empty_out"].sum() == 0
    assert g["same_fix"].shape == tuple(g["same_to"]) and np.array_equal(g["same_fix"], g["same_out"])
    assert g["up_out"].sum() == g["up_fix"].sum()                          # enlarging: no two fixations share a target
    # real: the last row rounds to `row` and is stepped back
    assert np.rint(479 * (224 / 480)) == 224
    # ties: ratio 1/2, every odd row and column lands on .5 (224 rows, 320 columns), and the last one rounds up to `row`
    H, W = g["ties_fix"].shape
    r, c = np.arange(H) * (224 / H), np.arange(W) * (320 / W)
    assert int((r % 1 == 0.5).sum()) == 224 and int((c % 1 == 0.5).sum()) == 320
    assert int((np.rint(r) == 224).sum()) == 1 and int((np.rint(c) == 320).sum()) == 1
    assert g["ties_fix"][1::2].sum() > 1000 and g["ties_fix"][:, 1::2].sum() > 1000   # fixations do sit on tie rows / columns
    # half to even, not half up: source rows 1 and 3 (0.5, 1.5) go to rows 0 and 2, nothing but row 2 itself goes to row 1
    rows = np.minimum(np.rint(np.argwhere(g["ties_fix"])[:, 0] * 0.5), 223)
    assert set(np.unique(rows[np.argwhere(g["ties_fix"])[:, 0] % 4 == 1] % 2)) == {0.0}
    # odd: many fixations merge into one target
    assert g["odd_fix"].sum() > 1.5 * g["odd_out"].sum() > 0


def test_restatement_equals_fixture(golden_dir):
    g = _gold(golden_dir)
    for c in CASES:
        row, col = (int(v) for v in g["%s_to" % c])
        got = ER.resize_fixation(g["%s_fix" % c], row, col)
        assert got.dtype == np.float64 and np.array_equal(got, g["%s_out" % c].astype(np.float64)), c
        assert np.array_equal(ER.resize_fixation(g["%s_fix" % c].astype(np.float32), row, col), got), c


def test_new_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mspi_hip.h")).read()
    assert int(re.search(r"#define\s+MSPI_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mspi_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib._SIGNATURES and name in _lib.EXPORTS
        assert getattr(raw, name) is not None and getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]
    assert lib.mspi_version() == 2
    assert os.path.exists(os.path.join(ROOT, "mspi_amd", "csrc", "evalprep.hip"))


def test_argument_validation_without_gpu():
    from mspi_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for bad in ((None, 0, p, 1, 4, 4, 4, 4), (p, 0, None, 1, 4, 4, 4, 4), (None, 1, p, 1, 4, 4, 4, 4)):
        assert lib.mspi_resize_bilinear_fwd(*bad, None) == -1
        assert b"mspi_resize_bilinear_fwd" in lib.mspi_last_error() and b"null" in lib.mspi_last_error()
    for bad in ((p, 0, p, 0, 4, 4, 4, 4), (p, 0, p, 1, 0, 4, 4, 4), (p, 1, p, 1, 4, 0, 4, 4), (p, 0, p, 1, 4, 4, 0, 4),
                (p, 0, p, 1, 4, 4, 4, 0), (p, 0, p, -2, 4, 4, 4, 4), (p, 0, p, 1, 4, 4, -1, 4)):
        assert lib.mspi_resize_bilinear_fwd(*bad, None) == -1
        assert b"mspi_resize_bilinear_fwd" in lib.mspi_last_error() and b"extent" in lib.mspi_last_error()
    for bad in ((None, p, 1, 4, 4, 4, 4), (p, None, 1, 4, 4, 4, 4)):
        assert lib.mspi_resize_fixation_fwd(*bad, None) == -1
        assert b"mspi_resize_fixation_fwd" in lib.mspi_last_error() and b"null" in lib.mspi_last_error()
    for bad in ((p, p, 0, 4, 4, 4, 4), (p, p, 1, 0, 4, 4, 4), (p, p, 1, 4, 0, 4, 4), (p, p, 1, 4, 4, 0, 4), (p, p, 1, 4, 4, 4, 0),
                (p, p, 1, 4, 4, -3, 4)):
        assert lib.mspi_resize_fixation_fwd(*bad, None) == -1
        assert b"mspi_resize_fixation_fwd" in lib.mspi_last_error() and b"extent" in lib.mspi_last_error()


def test_entry_points_refuse_cpu_tensors_and_cpu_devices(tmp_path):
    from mspi_amd import evaluate as E
    from mspi_amd._lib import MspiError
    a = torch.rand(1, 8, 12)
    for call in (lambda: E.resize_maps(a, (4, 6)), lambda: E.resize_maps(a.to(torch.uint8), (4, 6)),
                 lambda: E.resize_fixations(a, (4, 6)),
                 lambda: E.evaluate_dataset(str(tmp_path), str(tmp_path), "TOY", 2, device="cpu")):
        with pytest.raises(MspiError, match="no CPU fallback"):
            call()
    if not torch.cuda.is_available():
        with pytest.raises(MspiError, match="no CPU fallback"):
            E.evaluate_dataset(str(tmp_path), str(tmp_path), "TOY", 2)
        with pytest.raises(SystemExit, match=r"needs an MI355X \(no CPU fallback\)"):
            E.main(["--pred", str(tmp_path)])


def test_cli_arguments():
    from mspi_amd import evaluate as E
    a = E.build_parser().parse_args(["--pred", "out"])
    assert (a.pred, a.path_data, a.dataset, a.split, a.at, a.batch, a.other, a.baseline, a.jitter, a.seed, a.json) == (
        "out", "./AuViDataset", "AVAD", 2, "gt", 8, 0, None, True, 0, None)
    a = E.build_parser().parse_args("--pred o --path_data d --dataset DIEM --split 1 --at pred --batch 4 --other 10 "
                                    "--baseline mean --no_jitter --seed 7 --json r.json".split())
    assert (a.pred, a.path_data, a.dataset, a.split, a.at, a.batch, a.other, a.baseline, a.jitter, a.seed, a.json) == (
        "o", "d", "DIEM", 1, "pred", 4, 10, "mean", False, 7, "r.json")
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["--pred", "o", "--at", "model"])
    with pytest.raises(SystemExit):
        E.build_parser().parse_args([])


def _smooth(rng, H, W, blobs=4):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    m = np.zeros((H, W), np.float32)
    for _ in range(blobs):
        cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(H / 10, H / 3)
        m += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32)
    return m


def _u8(m, lo=16):
    """A smooth map as an 8-bit image with every value >= lo (no pixel is exactly zero after the JPEG round trip)."""
    return np.round(lo + (255 - lo) * m / m.max()).astype(np.uint8)


def _make_tree(root, videos, pred_hw, dataset="TOY", split=2, fix_ext=None, seed=0, empty=(), nofix=(), extra_pred=(),
               missing_pred=()):
    """path_data and pred_root under `root`.  videos: [(name, n_frames, (H, W))]; frames are numbered from 1.
    empty: {(video, frame)} whose density is all zero; nofix: {(video, frame)} without a fixation; extra_pred:
    {(video, frame)} predictions without an annotation; missing_pred: annotated frames without a prediction;
    fix_ext: {video: "mat" | "png"} (default mat)."""
    from PIL import Image
    import scipy.io
    rng = np.random.default_rng(seed)
    data, pred = os.path.join(root, "data"), os.path.join(root, "pred")
    os.makedirs(os.path.join(data, "fold_lists"))
    name = "DIEM_list_test_fps.txt" if dataset == "DIEM" else "%s_list_test_%d_fps.txt" % (dataset, split)
    with open(os.path.join(data, "fold_lists", name), "w") as f:
        for v, n, _ in reversed(videos):                               # unsorted on purpose: the reader sorts
            f.write("%s %d %d\n" % (v, n, 25))
    for v, n, (H, W) in videos:
        adir = os.path.join(data, "annotations", dataset, v)
        os.makedirs(os.path.join(adir, "maps"))
        os.makedirs(os.path.join(pred, v))
        for i in range(1, n + 1):
            dens = np.zeros((H, W), np.uint8) if (v, i) in empty else _u8(_smooth(rng, H, W))
            Image.fromarray(dens).save(os.path.join(adir, "maps", "eyeMap_%05d.jpg" % i), quality=95)
            fix = np.zeros((H, W), np.uint8)
            if (v, i) not in nofix:
                fix.reshape(-1)[rng.choice(H * W, size=int(rng.integers(5, 40)), replace=False)] = 1
            if (fix_ext or {}).get(v, "mat") == "mat":
                scipy.io.savemat(os.path.join(adir, "fixMap_%05d.mat" % i), {"eyeMap": fix * 255})
            else:
                Image.fromarray(fix * 255).save(os.path.join(adir, "fixMap_%05d.png" % i))
            if (v, i) not in missing_pred:
                Image.fromarray(_u8(_smooth(rng, pred_hw[0], pred_hw[1]))).save(os.path.join(pred, v, "img_%05d.jpg" % i), quality=95)
        for (pv, i) in extra_pred:
            if pv == v:
                Image.fromarray(_u8(_smooth(rng, pred_hw[0], pred_hw[1]))).save(os.path.join(pred, v, "img_%05d.jpg" % i))
    return pred, data


def test_plan_pairs_files_shards_and_counts(tmp_path, monkeypatch):
    """The host walk of evaluate_dataset, without a GPU: pairing by frame number, sharding, the missing-prediction error,
    the unannotated and empty_gt counts, .mat and .png fixation files, the seeded choice of other-frames."""
    from mspi_amd import evaluate as E
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    videos = [("va", 5, (12, 16)), ("vb", 3, (12, 16)), ("vc", 4, (10, 14))]
    pred, data = _make_tree(str(tmp_path), videos, (18, 24), fix_ext={"vb": "png"}, empty={("va", 2), ("vc", 4)},
                            extra_pred={("va", 9), ("vb", 7), ("vb", 8)})
    assert E.list_videos(data, "TOY", 2) == ["va", "vb", "vc"]
    work = E.plan(pred, data, "TOY", 2)
    assert [v["video"] for v in work["videos"]] == ["va", "vb", "vc"] and [v["index"] for v in work["videos"]] == [0, 1, 2]
    assert work["unannotated"] == 3 and work["seed"] == 0
    for v, (name, n, _) in zip(work["videos"], videos):
        assert [f["frame"] for f in v["frames"]] == list(range(1, n + 1))
        for f in v["frames"]:
            assert f["pred"] == os.path.join(pred, name, "img_%05d.jpg" % f["frame"])
            assert f["density"] == os.path.join(data, "annotations", "TOY", name, "maps", "eyeMap_%05d.jpg" % f["frame"])
            ext = "png" if name == "vb" else "mat"
            assert f["fixation"] == os.path.join(data, "annotations", "TOY", name, "fixMap_%05d.%s" % (f["frame"], ext))
            assert f["others"] == []
    # decoding on the host: uint8 arrays, binary fixations from both file types, empty densities counted and left out
    counters = {}
    batches = list(E.host_batches(work, batch=2, counters=counters))
    assert counters["empty_gt"] == 2
    assert [(v["video"], [f["frame"] for f in fr]) for v, fr in batches] == [
        ("va", [1, 3]), ("va", [4, 5]), ("vb", [1, 2]), ("vb", [3]), ("vc", [1, 2]), ("vc", [3])]
    for v, fr in batches:
        for f in fr:
            assert f["pred"].dtype == np.uint8 and f["pred"].shape == (18, 24)
            assert f["density"].dtype == np.uint8 and f["density"].shape == f["fixation"].shape and f["density"].max() > 0
            assert set(np.unique(f["fixation"])) == {0, 1} and 5 <= f["fixation"].sum() < 40
    assert [[f["frame"] for f in fr] for _, fr in E.host_batches(work, batch=2, prefetch=False)] == [
        [f["frame"] for f in fr] for _, fr in batches]
    # sharding by RANK / WORLD_SIZE as inference.py: rank r takes videos r, r + world, ... of the sorted list
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    w0 = E.plan(pred, data, "TOY", 2)
    monkeypatch.setenv("RANK", "1")
    w1 = E.plan(pred, data, "TOY", 2)
    assert [v["video"] for v in w0["videos"]] == ["va", "vc"] and [v["video"] for v in w1["videos"]] == ["vb"]
    assert [v["index"] for v in w0["videos"]] == [0, 2] and (w0["unannotated"], w1["unannotated"]) == (1, 2)
    # the choice of other-frames: seeded, repeatable, from OTHER videos, and the same whether the run is sharded or not
    monkeypatch.delenv("RANK")
    monkeypatch.delenv("WORLD_SIZE")
    a = E.plan(pred, data, "TOY", 2, other=3, generator=5)
    b = E.plan(pred, data, "TOY", 2, other=3, generator=5)
    c = E.plan(pred, data, "TOY", 2, other=3, generator=6)
    d = E.plan(pred, data, "TOY", 2, other=3, generator=np.random.default_rng(1))
    e = E.plan(pred, data, "TOY", 2, other=3, generator=np.random.default_rng(1))
    others = lambda w: [f["others"] for v in w["videos"] for f in v["frames"]]
    assert others(a) == others(b) and others(a) != others(c) and others(d) == others(e) and d["seed"] == e["seed"] != 0
    for v in a["videos"]:
        for f in v["frames"]:
            assert len(f["others"]) == 3
            for o in f["others"]:
                assert os.path.exists(o) and os.sep + v["video"] + os.sep not in o and "fixMap_" in o
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    s1 = E.plan(pred, data, "TOY", 2, other=3, generator=5)
    assert others(s1) == [f["others"] for f in a["videos"][1]["frames"]]
    dec = next(iter(E.host_batches(s1, batch=8, prefetch=False)))[1]
    assert len(dec[0]["others"]) == 3 and all(o.dtype == np.uint8 and o.ndim == 2 for o in dec[0]["others"])


def test_plan_names_the_missing_prediction(tmp_path, monkeypatch):
    from mspi_amd import evaluate as E
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    pred, data = _make_tree(str(tmp_path), [("va", 3, (12, 16)), ("vb", 2, (12, 16))], (18, 24), dataset="DIEM",
                            missing_pred={("vb", 2)})
    with pytest.raises(FileNotFoundError, match=re.escape(os.path.join(pred, "vb", "img_00002"))):
        E.plan(pred, data, "DIEM", 1)                     # DIEM's list has its special name; the split is not part of it
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    assert [v["video"] for v in E.plan(pred, data, "DIEM", 1)["videos"]] == ["va"]      # the other shard's files are not this rank's
    os.remove(os.path.join(data, "annotations", "DIEM", "va", "fixMap_00001.mat"))
    with pytest.raises(FileNotFoundError, match="fixMap_00001"):
        E.plan(pred, data, "DIEM", 1)


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_hip_resize_fixations_vs_fixture(dev, golden_dir):
    from mspi_amd import evaluate as E
    g = _gold(golden_dir)
    for c in CASES:
        size = tuple(int(v) for v in g["%s_to" % c])
        fix = torch.from_numpy(g["%s_fix" % c].astype(np.float32))[None].to(dev)
        got = E.resize_fixations(fix, size)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + size
        ref = torch.from_numpy(g["%s_out" % c].astype(np.float32))[None]
        assert _bits_equal(got.cpu(), ref), (c, int((got.cpu() != ref).sum()))
        assert _bits_equal(got, E.resize_fixations(fix * 255.0, size)), c             # any non-zero value is a fixation
    # a batch of 8 `real`-sized maps: the fixture's map rolled, so that every map of the batch differs
    base = g["real_fix"]
    maps = np.stack([np.roll(base, (17 * b, 29 * b), (0, 1)) for b in range(8)]).astype(np.float32)
    got = E.resize_fixations(torch.from_numpy(maps).to(dev), (224, 384)).cpu().numpy()
    for b in range(8):
        assert np.array_equal(got[b], ER.resize_fixation(maps[b], 224, 384).astype(np.float32)), b
    assert np.array_equal(got[0], g["real_out"].astype(np.float32))


@pytest.mark.gpu
def test_hip_resize_fixations_both_directions_vs_restatement(dev):
    from mspi_amd import evaluate as E
    rng = np.random.default_rng(3)
    for (H, W), (row, col), p in (((480, 640), (224, 384), 0.01), ((224, 384), (480, 640), 0.01), ((480, 640), (224, 384), 0.5),
                                  ((224, 384), (480, 640), 1.0), ((7, 5), (3, 9), 0.5)):
        maps = (rng.random((3, H, W)) < p).astype(np.float32)
        maps[1, H - 1, W - 1] = 1
        t = torch.from_numpy(maps).to(dev)
        got = E.resize_fixations(t, (row, col))
        assert _bits_equal(got, E.resize_fixations(t, (row, col)))
        for b in range(3):
            assert np.array_equal(got[b].cpu().numpy(), ER.resize_fixation(maps[b], row, col).astype(np.float32)), (H, W, row, col, b)


RESIZE_CASES = [((224, 384), (480, 640)), ((480, 640), (224, 384)), ((480, 640), (720, 1280)), ((37, 53), (101, 64)),
                ((1, 53), (7, 31)), ((37, 1), (9, 6)), ((48, 64), (1, 1)), ((480, 640), (270, 483))]


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_hip_resize_maps_vs_float64_interpolate(dev, src, dst):
    """|hip - float64 yardstick| <= 16 * 2^-24 * max|x| (the derivation is in the module docstring), uint8 and float32
    sources, B = 1 and 8; two runs are bit-equal."""
    from mspi_amd import evaluate as E
    rng = np.random.default_rng(src[0] * 7 + dst[1])
    for B in (1, 8):
        for kind in ("u8", "f32"):
            if kind == "u8":
                x = torch.from_numpy(rng.integers(0, 256, (B,) + src, dtype=np.uint8))
            else:
                x = torch.from_numpy((rng.standard_normal((B,) + src) * 3 + 1).astype(np.float32))
            got = E.resize_maps(x.to(dev), dst)
            assert got.dtype == torch.float32 and tuple(got.shape) == (B,) + dst
            ref = ER.resize_bilinear(x, dst)
            bound = 16 * 2.0 ** -24 * float(x.double().abs().max())
            err = float((got.cpu().double() - ref).abs().max())
            print("resize_maps %s B=%d %s -> %s: max |hip - float64| = %.3e (bound %.3e)" % (kind, B, src, dst, err, bound))
            assert err <= bound, (kind, B, err, bound)
            assert _bits_equal(got, E.resize_maps(x.to(dev), dst))


@pytest.mark.gpu
def test_hip_resize_maps_identity_and_constant(dev):
    from mspi_amd import evaluate as E
    rng = np.random.default_rng(11)
    for H, W in ((480, 640), (37, 53), (1, 7)):
        x = torch.from_numpy(rng.standard_normal((2, H, W)).astype(np.float32))
        x[0, 0, 0], x[1, -1, -1] = -0.0, float("inf")
        assert _bits_equal(E.resize_maps(x.to(dev), (H, W)).cpu(), x)
        u = torch.from_numpy(rng.integers(0, 256, (2, H, W), dtype=np.uint8))
        assert _bits_equal(E.resize_maps(u.to(dev), (H, W)).cpu(), u.float())
    for value in (0.1, 255.0, -3.7e5):
        for dst in ((480, 640), (101, 64), (10, 13)):
            got = E.resize_maps(torch.full((2, 37, 53), value, dtype=torch.float32, device=dev), dst).cpu().double()
            assert float((got - float(np.float32(value))).abs().max()) <= 16 * 2.0 ** -24 * abs(value)


@pytest.mark.gpu
def test_hip_resizes_inside_graph_capture(dev):
    """No synchronisation, allocation or copy inside the entry points: captured and replayed they give the eager result."""
    from mspi_amd import evaluate as E
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.standard_normal((4, 224, 384)).astype(np.float32)).to(dev)
    u = torch.from_numpy(rng.integers(0, 256, (4, 480, 640), dtype=np.uint8)).to(dev)
    f = torch.from_numpy((rng.random((4, 480, 640)) < 0.01).astype(np.float32)).to(dev)

    def launches():
        return E.resize_maps(x, (480, 640)), E.resize_maps(u, (224, 384)), E.resize_fixations(f, (224, 384))
    eager = launches()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = launches()
    for t in captured:
        t.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        assert _bits_equal(e, c)


def _rel(got, ref):
    return abs(got - ref) / max(abs(ref), 1e-3)


def _yardstick(s, d, f, o, b):
    """Per-frame values of the CPU yardsticks on host copies of one batch's device maps."""
    from oracle import restate as R
    four = R.saliency_metrics(s, d, f).double()
    ref = {k: four[:, i].tolist() for i, k in enumerate(("kl", "cc", "sim", "nss"))}
    ref["auc_j"] = [A.auc_judd(s[i].numpy(), f[i].numpy())[0] for i in range(len(s))]
    if o is not None:
        ref["s_auc"] = [A.auc_shuff(s[i].numpy(), f[i].numpy(), o[i].numpy()) for i in range(len(s))]
    if b is not None:
        ref["ig"] = A.ig_per_sample(s, f, b).double().tolist()
    return ref


TOL = {"auc_j": ("abs", 1e-9), "s_auc": ("abs", 1e-12)}


def _eval_tree(root):
    videos = [("clip_a", 5, (48, 64)), ("clip_b", 4, (48, 64)), ("clip_c", 5, (60, 80))]     # clip_c: another annotation size
    return _make_tree(root, videos, (72, 96), empty={("clip_a", 3)}, nofix={("clip_b", 2)}, extra_pred={("clip_c", 9)}, seed=4)


@pytest.mark.gpu
@pytest.mark.parametrize("at", ["gt", "pred"])
def test_evaluate_dataset_end_to_end(dev, tmp_path, monkeypatch, at):
    from mspi_amd import evaluate as E
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    pred, data = _eval_tree(str(tmp_path))
    kw = dict(at=at, batch=3, other=3, baseline="mean", jitter=False, generator=9, device=dev)
    res = E.evaluate_dataset(pred, data, "TOY", 2, **kw)
    assert res["frames"] == 13 and res["empty_gt"] == 1 and res["unannotated"] == 1
    assert set(res["per_video"]) == {"clip_a", "clip_b", "clip_c"}
    assert [res["per_video"][v]["frames"] for v in ("clip_a", "clip_b", "clip_c")] == [4, 4, 5]
    keys = ("kl", "cc", "sim", "nss", "auc_j", "s_auc", "ig")
    assert all(k in res for k in keys) and set(res["sum"]) == set(keys)

    # stage 1: the baseline is the mean of the device-resized densities, against the float64 yardstick of the resize
    base = E.mean_baseline(data, "TOY", 2, batch=3, device=dev)
    work = E.plan(pred, data, "TOY", 2, other=3, generator=9)
    dens = [f["density"] for _, fr in E.host_batches(work, batch=8) for f in fr]
    assert len(dens) == 13
    ref_base = torch.stack([ER.resize_bilinear(torch.from_numpy(x)[None], E.MEAN_BASELINE_SIZE)[0] for x in dens]).mean(0)
    assert tuple(base.shape) == E.MEAN_BASELINE_SIZE and float((base.cpu().double() - ref_base).abs().max()) <= 17 * 2.0 ** -24 * 255

    # stage 2: every batch's device maps against the host decode + the resize yardsticks; stage 3: the metric launches on
    # those maps against the CPU yardsticks fed with host copies of the SAME maps
    per_frame = {k: [] for k in keys}
    per_video = {}
    n_batches = 0
    for video, nos, s, d, f, o, b in E.device_batches(work, at, 3, base, dev):
        n_batches += 1
        size = tuple(s.shape[1:])
        by_no = {fr["frame"]: fr for fr in video["frames"]}
        raw_p = torch.stack([torch.from_numpy(E.load_gray(by_no[n]["pred"])) for n in nos])
        raw_d = torch.stack([torch.from_numpy(E.load_gray(by_no[n]["density"])) for n in nos])
        raw_f = np.stack([E.load_fixation(by_no[n]["fixation"]) for n in nos])
        assert size == (tuple(raw_d.shape[1:]) if at == "gt" else (72, 96))
        bound = 16 * 2.0 ** -24 * 255
        assert float((s.cpu().double() - ER.resize_bilinear(raw_p, size)).abs().max()) <= bound
        assert float((d.cpu().double() - ER.resize_bilinear(raw_d, size)).abs().max()) <= bound
        assert float((b.cpu().double() - ER.resize_bilinear(base.cpu()[None], size)).abs().max()) <= 16 * 2.0 ** -24 * float(base.max())
        ref_f = np.stack([ER.resize_fixation(x, *size) for x in raw_f]).astype(np.float32)
        assert np.array_equal(f.cpu().numpy(), ref_f)
        ref_o = np.stack([np.max([ER.resize_fixation(E.load_fixation(p), *size) for p in by_no[n]["others"]], 0) for n in nos])
        assert np.array_equal(o.cpu().numpy(), ref_o.astype(np.float32)) and o.sum() > 0
        got = E.score_batch(s, d, f, o, b, jitter=False)
        ref = _yardstick(s.cpu(), d.cpu(), f.cpu(), o.cpu(), b.cpu())
        for k in keys:
            for i, (gv, rv) in enumerate(zip(got[k], ref[k])):
                assert math.isnan(gv) == math.isnan(rv), (k, video["video"], nos[i], gv, rv)
                if not math.isnan(rv):
                    kind, tol = TOL.get(k, ("rel", 2e-5))
                    err = abs(gv - rv) if kind == "abs" else _rel(gv, rv)
                    assert err <= tol, (k, video["video"], nos[i], gv, rv, err)
            per_frame[k] += got[k]
            per_video.setdefault(video["video"], {kk: [] for kk in keys})[k] += got[k]
    assert n_batches == 6                                  # 2 + 2 + 2: batches never mix videos
    # clip_b frame 2 has no fixation: NaN for the fixation metrics, exactly there
    for k in ("nss", "auc_j", "s_auc", "ig"):
        assert res["nan"][k] == 1 and res["count"][k] == 12 and res["per_video"]["clip_b"]["nan"][k] == 1
    for k in ("kl", "cc", "sim"):
        assert res["nan"][k] == 0 and res["count"][k] == 13

    # stage 4: the bookkeeping -- sums, counts and means of evaluate_dataset are those of the per-frame values
    def check(entry, values):
        for k in keys:
            ok = [v for v in values[k] if not math.isnan(v)]
            assert entry["count"][k] == len(ok) and entry["nan"][k] == len(values[k]) - len(ok)
            assert entry["sum"][k] == pytest.approx(math.fsum(ok), rel=1e-14, abs=1e-14)      # <= 13 float64 additions
            mean = entry["mean"][k] if "mean" in entry else entry[k]
            assert mean == entry["sum"][k] / entry["count"][k]
    check(res, per_frame)
    for v in per_video:
        check(res["per_video"][v], per_video[v])
    for k in keys:
        assert res["sum"][k] == math.fsum(res["per_video"][v]["sum"][k] for v in per_video)
        assert res["count"][k] == sum(res["per_video"][v]["count"][k] for v in per_video)
    assert res == E.evaluate_dataset(pred, data, "TOY", 2, **kw)           # a second run: the same dict, bit for bit

    # two shards, one after the other in this process: their sums and counts add up to the unsharded ones exactly
    monkeypatch.setenv("WORLD_SIZE", "2")
    shards = []
    for rank in (0, 1):
        monkeypatch.setenv("RANK", str(rank))
        shards.append(E.evaluate_dataset(pred, data, "TOY", 2, **kw))
    assert set(shards[0]["per_video"]) == {"clip_a", "clip_c"} and set(shards[1]["per_video"]) == {"clip_b"}
    merged = {}
    for sh in shards:
        for v, pv in sh["per_video"].items():
            assert pv == res["per_video"][v], v                            # a video's entry does not depend on the sharding
            merged[v] = pv
    for k in keys:
        assert shards[0]["count"][k] + shards[1]["count"][k] == res["count"][k]
        assert shards[0]["nan"][k] + shards[1]["nan"][k] == res["nan"][k]
        # "sum" is math.fsum of the per-video sums -- independent of their grouping -- so the shards merge exactly ...
        assert math.fsum(pv["sum"][k] for pv in merged.values()) == res["sum"][k]
        assert shards[0]["sum"][k] == math.fsum(merged[v]["sum"][k] for v in ("clip_a", "clip_c")) and shards[1]["sum"][k] == merged["clip_b"]["sum"][k]
        # ... while a plain `+` of two shard totals rounds once more: equal to the last bit or two of a float64
        assert shards[0]["sum"][k] + shards[1]["sum"][k] == pytest.approx(res["sum"][k], rel=4 * 2.0 ** -53, abs=1e-300)
    assert shards[0]["frames"] + shards[1]["frames"] == 13
    assert shards[0]["empty_gt"] + shards[1]["empty_gt"] == 1 and shards[0]["unannotated"] + shards[1]["unannotated"] == 1


@pytest.mark.gpu
def test_evaluate_dataset_options(dev, tmp_path, monkeypatch, capsys):
    """Without other / baseline only the fed metrics are reported; a .npy and a tensor baseline; seeded jitter repeats;
    tall maps (H > W) are counted under nan['s_auc']; a missing prediction raises; the CLI prints the table and writes JSON."""
    import json
    from mspi_amd import evaluate as E
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    pred, data = _make_tree(str(tmp_path / "wide"), [("va", 3, (24, 32)), ("vb", 2, (24, 32))], (36, 48), seed=1)
    res = E.evaluate_dataset(pred, data, "TOY", 2, jitter=False, device=dev)
    assert {k for k in ("kl", "cc", "sim", "nss", "auc_j", "s_auc", "ig") if k in res} == {"kl", "cc", "sim", "nss", "auc_j"}
    assert res["frames"] == 5 and all(math.isfinite(res[k]) for k in ("kl", "cc", "sim", "nss", "auc_j"))
    a = E.evaluate_dataset(pred, data, "TOY", 2, generator=3, device=dev)
    b = E.evaluate_dataset(pred, data, "TOY", 2, generator=3, device=dev)
    assert a == b and math.isfinite(a["auc_j"]) and abs(a["auc_j"] - res["auc_j"]) < 0.05     # seeded jitter repeats; it only reorders ties
    base = torch.rand(30, 40, generator=torch.Generator().manual_seed(0)) + 0.1
    np.save(str(tmp_path / "base.npy"), base.numpy())
    r1 = E.evaluate_dataset(pred, data, "TOY", 2, baseline=str(tmp_path / "base.npy"), jitter=False, device=dev)
    r2 = E.evaluate_dataset(pred, data, "TOY", 2, baseline=base.to(dev), jitter=False, device=dev)
    assert r1["sum"] == r2["sum"] and math.isfinite(r1["ig"]) and r1["sum"]["kl"] == res["sum"]["kl"]
    from mspi_amd._lib import MspiError
    with pytest.raises(MspiError, match="no CPU fallback"):
        E.evaluate_dataset(pred, data, "TOY", 2, baseline=base, device=dev)
    out = E.main(["--pred", pred, "--path_data", data, "--dataset", "TOY", "--no_jitter", "--json", str(tmp_path / "r.json")])
    printed = capsys.readouterr().out
    assert "va" in printed and "auc_j" in printed and "frames/s" in printed
    assert json.load(open(str(tmp_path / "r.json")))["sum"] == out["sum"] == res["sum"]
    tall_pred, tall_data = _make_tree(str(tmp_path / "tall"), [("ta", 3, (32, 24)), ("tb", 2, (32, 24))], (48, 36), seed=2)
    t = E.evaluate_dataset(tall_pred, tall_data, "TOY", 2, other=2, jitter=False, device=dev)
    assert t["nan"]["s_auc"] == 5 and t["count"]["s_auc"] == 0 and math.isnan(t["s_auc"]) and t["count"]["auc_j"] == 5
    os.remove(os.path.join(pred, "vb", "img_00002.jpg"))
    with pytest.raises(FileNotFoundError, match="img_00002"):
        E.evaluate_dataset(pred, data, "TOY", 2, device=dev)


@pytest.mark.gpu
def test_round_trip_with_the_clip_loop(dev, tmp_path, monkeypatch):
    """inference_dataset writes the maps of a toy dataset with a small model, evaluate_dataset scores what it wrote: it
    completes, every metric is finite and every annotated frame is scored."""
    from PIL import Image
    import scipy.io
    from mspi_amd import evaluate as E
    from mspi_amd import inference as I
    from mspi_amd import testing as T
    from scipy.io import wavfile
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    root, rng = str(tmp_path / "data"), np.random.default_rng(0)
    n_frames, hw, sr = 34, (48, 64), 22050
    os.makedirs(os.path.join(root, "fold_lists"))
    names = ("clip1", "clip2")
    with open(os.path.join(root, "fold_lists", "TOY_list_test_2_fps.txt"), "w") as f:
        for name in names:
            f.write("%s %d %d\n" % (name, n_frames, 25))
    for name in names:
        fdir, adir = os.path.join(root, "video_frames", "TOY", name), os.path.join(root, "video_audio", "TOY", name)
        ann = os.path.join(root, "annotations", "TOY", name)
        os.makedirs(fdir), os.makedirs(adir), os.makedirs(os.path.join(ann, "maps"))
        for i in range(1, n_frames + 1):
            Image.fromarray(rng.integers(0, 255, hw + (3,), dtype=np.uint8)).save(os.path.join(fdir, "img_%05d.jpg" % i))
            Image.fromarray(_u8(_smooth(rng, *hw))).save(os.path.join(ann, "maps", "eyeMap_%05d.jpg" % i), quality=95)
            fix = np.zeros(hw, np.uint8)
            fix.reshape(-1)[rng.choice(hw[0] * hw[1], size=20, replace=False)] = 1
            scipy.io.savemat(os.path.join(ann, "fixMap_%05d.mat" % i), {"eyeMap": fix})
        t = np.arange(int(sr * n_frames / 25) + sr) / sr
        wav = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * rng.standard_normal(t.size)).astype(np.float32)
        wavfile.write(os.path.join(adir, name + ".wav"), sr, np.stack([wav, 0.5 * wav], 1))     # stereo
    res_hw = (64, 96)
    I.device = dev
    I._RESOLUTION[:] = list(res_hw)
    torch.manual_seed(0)
    model = I.build_model("x3dl", res_hw)
    T.randomize_(model.cpu(), 0)
    model = model.to(dev).eval()
    args = types.SimpleNamespace(clip_size=16, dataset="TOY", split=2, path_data=root, save_path=str(tmp_path / "out"),
                                 use_sound=True, batch=5)
    I.inference_dataset(model, args)
    torch.cuda.synchronize()
    for at in ("gt", "pred"):
        res = E.evaluate_dataset(args.save_path, root, "TOY", 2, at=at, other=2, baseline="mean", generator=1, device=dev)
        assert res["frames"] == 2 * n_frames and res["unannotated"] == 0 and res["empty_gt"] == 0
        for k in ("kl", "cc", "sim", "nss", "auc_j", "s_auc", "ig"):
            assert math.isfinite(res[k]) and res["count"][k] == 2 * n_frames and res["nan"][k] == 0, (at, k, res[k])
        assert 0.0 <= res["auc_j"] <= 1.0
