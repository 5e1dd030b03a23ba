"""Grey JPEG encoding on the device (csrc/jpegenc.hip, engine.jpeg_encode_gray, inference --device_jpeg / --workers).

The oracle is tests/jpeg_restate.py, a numpy restatement of libjpeg's baseline encoder; where PIL is built on libjpeg-turbo
it is itself pinned to PIL.Image.save(format="JPEG", quality=q), byte for byte.  Every comparison is exact."""
import ctypes
import functools
import io
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_restate as J  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mspi_jpeg_gray_header", "mspi_jpeg_gray_bound", "mspi_jpeg_gray_ws_bytes", "mspi_jpeg_gray_fwd")


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _blob(h, w, seed):
    """Four Gaussians of seeded place, width and height, scaled to 0...255: what a saliency map looks like."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g = np.zeros((h, w))
    for _ in range(4):
        cy, cx, s, a = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.05, 0.2) * max(h, w), rng.uniform(0.3, 1.0)
        g += a * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return np.round(255 * g / g.max()).astype(np.uint8)


def _cos77():
    y, x = np.mgrid[0:8, 0:16]
    return np.round(128 + 100 * np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16)).astype(np.uint8)


def _checker():
    y, x = np.mgrid[0:32, 0:48]
    return (((y // 8 + x // 8) % 2) * 255).astype(np.uint8)


# name: (image, quality, what the restatement must report about the stream -- so that no case goes soft).  The figures are
# those of PIL's own stream for these seeds (the restatement equals PIL on every row).
CASES = {
    "noise_8x8": (lambda: _noise(8, 8, 0), 95, dict(scan_bytes=64)),                                 # one block, first-block DC
    "noise_37x53": (lambda: _noise(37, 53, 1), 95, dict(stuffed=13, max_ac_size=9)),                 # edges, unaligned rows
    "blob_37x53": (lambda: _blob(37, 53, 39), 95, dict(zrl=1, stuffed=5)),                           # zero runs
    "blob_48x64": (lambda: _blob(48, 64, 1), 95, dict(stuffed=5)),
    "cos77_8x16": (_cos77, 95, dict(zrl=6, max_dc_size=0)),                                          # only coefficient 63 set
    "checker_q95": (_checker, 95, dict(max_dc_size=10, max_ac_size=0)),                              # DC-only blocks
    "checker_q100": (_checker, 100, dict(max_dc_size=11, max_ac_size=0)),
    "noise_40x40_q100": (lambda: _noise(40, 40, 2), 100, dict(stuffed=33)),                          # all divisors 8
    "noise_24x24_q30": (lambda: _noise(24, 24, 3), 30, dict()),
    "blob_224x384_q75": (lambda: _blob(224, 384, 4), 75, dict()),
    "blob_480x640": (lambda: _blob(480, 640, 5), 95, dict(stuffed=45, zrl=2)),                       # 4800 blocks
    "const255_16x24": (lambda: np.full((16, 24), 255, np.uint8), 95, dict()),
    "noise_16x16_aligned": (lambda: _noise(16, 16, 121), 95, dict(scan_bits=2072)),                  # bit count % 8 == 0: no padding
    "noise_16x16_padded": (lambda: _noise(16, 16, 100), 95, dict()),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(image, quality, the restatement's file, its stream statistics); computed once per session."""
    make, quality, _ = CASES[name]
    img, stats = make(), {}
    return img, quality, J.encode(img, quality, stats), stats


def _turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


def _pil(img, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=quality)
    return b.getvalue()


# ----------------------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reports_what_the_case_exercises(name):
    _, _, data, stats = _case(name)
    for k, v in CASES[name][2].items():
        assert stats[k] == v, (name, k, stats)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9" and len(data) == J.HEADER_LEN + stats["scan_bytes"] + stats["stuffed"] + 2


def test_padding_cases_cover_both_endings():
    assert _case("noise_16x16_aligned")[3]["scan_bits"] % 8 == 0
    assert _case("noise_16x16_padded")[3]["scan_bits"] % 8 != 0


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_pil(name):
    if not _turbo():
        pytest.skip("PIL is not built on libjpeg-turbo: its encoder is not the one restated")
    img, quality, data, _ = _case(name)
    assert data == _pil(img, quality)


def test_header_equals_pil():
    from PIL import Image
    from mspi_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_ubyte * 512)()
    n = lib.mspi_jpeg_gray_header(48, 64, 95, buf, 512)
    assert n == 328 and bytes(buf[:n]) == J.header(48, 64, 95)
    for quality in (1, 30, 49, 50, 75, 100):
        assert lib.mspi_jpeg_gray_header(37, 53, quality, buf, 512) == 328 and bytes(buf[:328]) == J.header(37, 53, quality)
    if not _turbo():
        pytest.skip("PIL is not built on libjpeg-turbo: nothing to pin the header to")
    lib.mspi_jpeg_gray_header(48, 64, 95, buf, 512)
    ref = _pil(_blob(48, 64, 1), 95)
    assert bytes(buf[:328]) == ref[:328]
    natural = np.zeros(64, dtype=int)
    natural[J.ZIGZAG] = list(buf[25:89])                   # the DQT payload is in zigzag order, PIL hands tables back de-zigzagged
    assert natural.tolist() == list(Image.open(io.BytesIO(ref)).quantization[0]) == J.quant_table(95).tolist()


def test_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mspi_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared and name in _lib._SIGNATURES and name in _lib.EXPORTS
        assert getattr(raw, name) is not None and getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]
    assert lib.mspi_version() == 2
    assert "MspiJpegDesc" in hdr and ctypes.sizeof(_lib.JpegDesc) == 4 * 4 + 4 * 8 + 64 * 2 + 8 + 8


def _desc(lib, H, W, quality=95, B=1, header_ptr=1):
    from mspi_amd import _lib
    buf = (ctypes.c_ubyte * 512)()
    d = _lib.JpegDesc()
    d.B, d.H, d.W, d.quality, d.pitch, d.map_stride = B, H, W, quality, W, H * W
    d.cap = d.file_stride = lib.mspi_jpeg_gray_bound(H, W)
    d.header_len = max(lib.mspi_jpeg_gray_header(H, W, quality, buf, 512), 0)
    for k in range(64):
        d.div[k] = 8 * buf[25 + k]
    d.header = header_ptr
    return d


def test_refusals():
    """Bad descriptors are refused on the host, before any launch, and say why."""
    from mspi_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_ubyte * 512)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(d, maps=p, files=p, lengths=p, ws=p):
        return lib.mspi_jpeg_gray_fwd(ctypes.byref(d), maps, files, lengths, ws, None)

    for H, W in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-1, 8)):
        assert lib.mspi_jpeg_gray_header(H, W, 95, buf, 512) == -1 and b"65535" in lib.mspi_last_error()
        assert lib.mspi_jpeg_gray_bound(H, W) == 0 and lib.mspi_jpeg_gray_ws_bytes(1, H, W) == 0
        d = _desc(lib, 8, 8)
        d.H, d.W = H, W
        assert fwd(d) == -1 and b"65535" in lib.mspi_last_error()
    for quality in (0, 101, -5):
        assert lib.mspi_jpeg_gray_header(8, 8, quality, buf, 512) == -1 and b"quality" in lib.mspi_last_error()
        d = _desc(lib, 8, 8)
        d.quality = quality
        assert fwd(d) == -1 and b"quality" in lib.mspi_last_error()
    assert lib.mspi_jpeg_gray_header(8, 8, 95, buf, 327) == -1 and b"cap" in lib.mspi_last_error()
    assert lib.mspi_jpeg_gray_header(8, 8, 95, None, 512) == -1 and b"null" in lib.mspi_last_error()
    d = _desc(lib, 37, 53)
    d.cap -= 1
    assert fwd(d) == -1 and b"cap" in lib.mspi_last_error()
    d = _desc(lib, 37, 53)
    for kw in (dict(maps=None), dict(files=None), dict(lengths=None), dict(ws=None)):
        assert fwd(d, **kw) == -1 and b"null" in lib.mspi_last_error()
    assert lib.mspi_jpeg_gray_fwd(None, p, p, p, p, None) == -1 and b"null" in lib.mspi_last_error()
    d.header = None
    assert fwd(d) == -1 and b"null" in lib.mspi_last_error()
    d = _desc(lib, 37, 53)
    d.div[5] += 8                                          # not the divisors of the declared quality
    assert fwd(d) == -1 and b"divisor" in lib.mspi_last_error()
    d = _desc(lib, 37, 53)
    d.pitch = 52
    assert fwd(d) == -1 and b"pitch" in lib.mspi_last_error()


def test_bound_covers_every_case():
    from mspi_amd import _lib
    lib = _lib.load()
    for name in CASES:
        img, _, data, _ = _case(name)
        assert lib.mspi_jpeg_gray_bound(*img.shape) == J.bound(*img.shape) >= len(data)
    assert lib.mspi_jpeg_gray_ws_bytes(8, 480, 640) % 8 == 0 and lib.mspi_jpeg_gray_ws_bytes(8, 480, 640) > 8 * 4800 * 12


def test_engine_refuses_cpu_tensors():
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    with pytest.raises(MspiError):
        E.jpeg_encode_gray(torch.zeros(1, 8, 8, dtype=torch.uint8))


def test_device_jpeg_with_graph_is_refused_before_any_work(tmp_path):
    from mspi_amd import inference as I
    _make_dataset(str(tmp_path))
    args = types.SimpleNamespace(clip_size=16, dataset="TOY", split=2, path_data=str(tmp_path), save_path=str(tmp_path / "o"),
                                 use_sound=True, batch=4, graph=True, device_jpeg=True)
    with pytest.raises(ValueError, match="graph"):
        I._inference_dataset(None, args)


def test_frame_decoder_hands_back_the_loop_s_own_frames(tmp_path):
    """--workers: frames decoded ahead on the pool are the arrays the loop's own decode gives, in any order of asking,
    asked twice, and never more than `ahead` of them in flight."""
    from mspi_amd import inference as I
    _make_dataset(str(tmp_path), n_frames=12)
    paths = sorted(os.path.join(str(tmp_path), "video_frames", "TOY", "clip1", n)
                   for n in os.listdir(os.path.join(str(tmp_path), "video_frames", "TOY", "clip1")))
    dec = I._FrameDecoder(paths, workers=3, ahead=4)
    try:
        for j in (0, 1, 2, 5, 3, 3, 11, 10):
            assert np.array_equal(dec.get(j), I._decode_rgb(paths[j]))
            assert len(dec.pending) <= 4
    finally:
        dec.close()


# ----------------------------------------------------------------------------- on the GPU
GUARD = 64


def _encode(dev, maps, quality):
    """maps: uint8 [B,H,W] device tensor, unit stride along W -> (rows [B, cap + GUARD] as numpy, lengths, cap).  Straight
    through the C ABI, with rows of cap + GUARD bytes pre-filled with 0xA5."""
    from mspi_amd import _lib
    lib = _lib.load()
    B, H, W = maps.shape
    d = _desc(lib, H, W, quality, B)
    hbuf = (ctypes.c_ubyte * 512)()
    lib.mspi_jpeg_gray_header(H, W, quality, hbuf, 512)
    header = torch.tensor(list(hbuf[:328]), dtype=torch.uint8).to(dev)
    d.header, d.pitch, d.map_stride = header.data_ptr(), maps.stride(1), maps.stride(0)
    d.file_stride = d.cap + GUARD
    files = torch.full((B, d.cap + GUARD), 0xA5, dtype=torch.uint8, device=dev)
    lengths = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mspi_jpeg_gray_ws_bytes(B, H, W), dtype=torch.uint8, device=dev)
    _lib.check(lib.mspi_jpeg_gray_fwd(ctypes.byref(d), maps.data_ptr(), files.data_ptr(), lengths.data_ptr(), ws.data_ptr(),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "mspi_jpeg_gray_fwd")
    torch.cuda.synchronize()
    return files.cpu().numpy(), lengths.cpu().numpy(), int(d.cap)


def _check_rows(rows, lengths, cap, want):
    for b, data in enumerate(want):
        n = int(lengths[b])
        assert n == len(data), (b, n, len(data))
        assert rows[b, :n].tobytes() == data, "map %d: first difference at byte %d" % (
            b, int(np.flatnonzero(np.frombuffer(data, np.uint8) != rows[b, :n])[0]))
        assert (rows[b, n:] == 0xA5).all(), "map %d: bytes written beyond the file" % b       # the guard bytes included
    assert rows.shape[1] == cap + GUARD


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_encoder_equals_restatement(dev, name):
    img, quality, data, _ = _case(name)
    rows, lengths, cap = _encode(dev, torch.from_numpy(img)[None].to(dev), quality)
    _check_rows(rows, lengths, cap, [data])
    if _turbo():
        assert rows[0, : lengths[0]].tobytes() == _pil(img, quality)


@pytest.mark.gpu
def test_three_maps_in_one_launch(dev):
    imgs = [_noise(37, 53, 1), _blob(37, 53, 39), np.full((37, 53), 200, np.uint8)]
    want = [J.encode(m, 95) for m in imgs]
    assert len({len(w) for w in want}) == 3
    rows, lengths, cap = _encode(dev, torch.from_numpy(np.stack(imgs)).to(dev), 95)
    _check_rows(rows, lengths, cap, want)


@pytest.mark.gpu
def test_strided_view_gives_the_same_bytes(dev):
    """A pitch and a map stride larger than dense: the maps are a window of a wider, taller buffer."""
    imgs = np.stack([_noise(37, 53, 1), _blob(37, 53, 39)])
    wide = torch.full((2, 45, 80), 77, dtype=torch.uint8, device=dev)
    view = wide[:, 3:40, 11:64]
    view.copy_(torch.from_numpy(imgs))
    assert view.stride() == (45 * 80, 80, 1)
    rows, lengths, cap = _encode(dev, view, 95)
    _check_rows(rows, lengths, cap, [J.encode(m, 95) for m in imgs])


@pytest.mark.gpu
def test_two_launches_are_identical_and_engine_wrapper(dev):
    from mspi_amd import engine as E
    img, quality, data, _ = _case("blob_480x640")
    maps = torch.from_numpy(np.stack([img, img[::-1]])).to(dev)
    f0, l0 = E.jpeg_encode_gray(maps, quality)
    f1, l1 = E.jpeg_encode_gray(maps, quality)
    assert f0.is_cuda and l0.is_cuda and f0.dtype == torch.uint8 and l0.dtype == torch.int32
    f0, l0, f1, l1 = f0.cpu().numpy(), l0.cpu().numpy(), f1.cpu().numpy(), l1.cpu().numpy()
    assert (l0 == l1).all()
    for b in range(2):
        assert (f0[b, : l0[b]] == f1[b, : l1[b]]).all()
    assert f0[0, : l0[0]].tobytes() == data
    wide = torch.zeros(2, 480, 700, dtype=torch.uint8, device=dev)
    wide[:, :, 30:670] = maps
    f2, l2 = E.jpeg_encode_gray(wide[:, :, 30:670], quality)                 # the wrapper passes a view's strides on
    assert f2.cpu().numpy()[0, : int(l2[0])].tobytes() == data


def _make_dataset(root, name="clip1", n_frames=34, hw=(48, 64), fps=25, sr=22050):
    """The toy dataset of tests/test_inference.py (a copy: test modules do not import from each other)."""
    from PIL import Image
    from scipy.io import wavfile
    rng = np.random.RandomState(0)
    fdir = os.path.join(root, "video_frames", "TOY", name)
    adir = os.path.join(root, "video_audio", "TOY", name)
    os.makedirs(fdir), os.makedirs(adir), os.makedirs(os.path.join(root, "fold_lists"))
    for i in range(n_frames):
        Image.fromarray(rng.randint(0, 255, (hw[0], hw[1], 3), dtype=np.uint8)).save(os.path.join(fdir, "img_%05d.jpg" % (i + 1)))
    t = np.arange(int(sr * n_frames / fps) + sr) / sr
    wav = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * rng.randn(t.size)).astype(np.float32)
    wavfile.write(os.path.join(adir, name + ".wav"), sr, np.stack([wav, 0.5 * wav], 1))     # stereo
    with open(os.path.join(root, "fold_lists", "TOY_list_test_2_fps.txt"), "w") as f:
        f.write("%s %d %d\n" % (name, n_frames, fps))
    return os.path.join(adir, name + ".wav")


@pytest.mark.gpu
def test_clip_loop_writes_the_same_files(dev, tmp_path):
    """inference_dataset with the flags off, with device_jpeg and with decode workers: the same names, the same bytes.
    A first run with the flags off comes before the three and is not compared: the first forwards of a freshly built model
    are not the later ones (engine.autotune times kernel candidates, and the operand-range check moves an out-of-range
    layer to the fp32 path "from the NEXT forward on"), so a first run's maps differ from every later run's by a grey level
    here and there whatever the flags are."""
    from mspi_amd import inference as I
    from mspi_amd import testing as T
    root = str(tmp_path / "data")
    _make_dataset(root)
    res = (64, 96)
    I.device = dev
    I._RESOLUTION[:] = list(res)
    model = I.build_model("x3dl", res)
    T.randomize_(model.cpu(), 0)
    model = model.to(dev).eval()
    trees = {}
    for tag, kw in (("first", {}), ("off", {}), ("device_jpeg", dict(device_jpeg=True)), ("workers", dict(workers=4))):
        args = types.SimpleNamespace(clip_size=16, dataset="TOY", split=2, path_data=root, save_path=str(tmp_path / tag),
                                     use_sound=True, batch=5, **kw)
        I.inference_dataset(model, args)
        names = sorted(os.listdir(os.path.join(args.save_path, "clip1")))
        trees[tag] = {n: open(os.path.join(args.save_path, "clip1", n), "rb").read() for n in names}
    assert len(trees["off"]) == 34
    for tag in ("device_jpeg", "workers"):
        assert sorted(trees[tag]) == sorted(trees["off"])
        bad = [n for n in trees["off"] if trees[tag][n] != trees["off"][n]]
        assert not bad, (tag, bad[:5])
    args = types.SimpleNamespace(clip_size=16, dataset="TOY", split=2, path_data=root, save_path=str(tmp_path / "refused"),
                                 use_sound=True, batch=5, device_jpeg=True, graph=True)
    with pytest.raises(ValueError, match="graph"):
        I.inference_dataset(model, args)
