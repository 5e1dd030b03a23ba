"""JPEG frame decoding on the device (csrc/jpegdec.hip, engine.jpeg_decode_rgb / jpeg_probe, preproc.decode_frames,
inference --device_decode, AudioVisualDataset(device_decode=True)).

The oracle is tests/jpeg_decode_restate.py, a numpy restatement of libjpeg-turbo's default decode and of the decoder's
self-synchronising pass rule; where PIL is built on libjpeg-turbo the restatement is itself pinned to
np.asarray(Image.open(f).convert("RGB")), pixel for pixel.  The arithmetic is integer only: every comparison is exact."""
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
import jpeg_decode_restate as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mspi_jpeg_dec_parse", "mspi_jpeg_dec_ws_bytes", "mspi_jpeg_dec_fwd")


def _noise(h, w, seed, grey=False):
    return np.random.default_rng(seed).integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)


def _smooth(h, w, seed):
    """Three slow waves plus a little seeded noise: what a video frame's statistics look like."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / 37.0 + rng.uniform(0, 3)) * np.cos(y / 23.0), 128 + 90 * np.cos(x / 51.0 + y / 13.0),
                    (x + y) / 5.0 % 256], 2)
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


def _checker():
    y, x = np.mgrid[0:128, 0:128]
    return np.repeat((((y // 8 + x // 8) % 2) * 255).astype(np.uint8)[:, :, None], 3, 2)


_QTABLES = [[3 + (5 * k) % 23 for k in range(64)], [2 + (7 * k) % 31 for k in range(64)]]

# name: (image, PIL save arguments, S or None for the engine's default, what the restatement must report about the stream
# -- so that no case goes soft).  lanes: subsequences; passes: behind the first, the confirming one included (1: the guesses
# were right); longest: the longest Huffman code met; zrl / stuffed: counts.  The figures are those of PIL's own files for
# these seeds.
CASES = {
    "noise_8x8_444": (lambda: _noise(8, 8, 0), dict(quality=95, subsampling=0), 128,      # one MCU
        dict(lanes=10, passes=10, longest_code=9, zrl=0, stuffed=0)),
    "noise_16x16_420": (lambda: _noise(16, 16, 1), dict(quality=95, subsampling=2), 128,      # one MCU of six blocks
        dict(lanes=19, passes=19, longest_code=10, zrl=0, stuffed=2)),
    "smooth_17x19_444": (lambda: _smooth(17, 19, 2), dict(quality=95, subsampling=0), 128,      # partial MCUs,
        dict(lanes=23, passes=5, longest_code=16, zrl=1, stuffed=9)),
    "smooth_17x19_422": (lambda: _smooth(17, 19, 2), dict(quality=95, subsampling=1), 128,      # odd chroma sizes
        dict(lanes=17, passes=9, longest_code=16, zrl=5, stuffed=9)),
    "smooth_17x19_420": (lambda: _smooth(17, 19, 2), dict(quality=95, subsampling=2), 128,
        dict(lanes=14, passes=10, longest_code=16, zrl=1, stuffed=4)),
    "smooth_33x95_444": (lambda: _smooth(33, 95, 3), dict(quality=95, subsampling=0), 128,
        dict(lanes=175, passes=12, longest_code=16, zrl=32, stuffed=39)),
    "smooth_33x95_422": (lambda: _smooth(33, 95, 3), dict(quality=95, subsampling=1), 128,
        dict(lanes=115, passes=12, longest_code=16, zrl=57, stuffed=20)),
    "smooth_33x95_420": (lambda: _smooth(33, 95, 3), dict(quality=95, subsampling=2), 128,
        dict(lanes=94, passes=22, longest_code=16, zrl=14, stuffed=15)),
    "grey_37x53": (lambda: _noise(37, 53, 4, grey=True), dict(quality=90), 128,
        dict(lanes=109, passes=49, longest_code=16, zrl=0, stuffed=1)),
    "toy_48x64_420_q75": (lambda: _noise(48, 64, 5), dict(quality=75), 128,      # the toy dataset's frame
        dict(lanes=115, passes=73, longest_code=15, zrl=1, stuffed=2)),
    "opt_48x64_q60": (lambda: _smooth(48, 64, 6), dict(quality=60, optimize=True), 128,      # the file's own Huffman tables
        dict(lanes=15, passes=6, longest_code=8, zrl=1, stuffed=0)),
    "qtables_48x64": (lambda: _smooth(48, 64, 7), dict(qtables=_QTABLES, subsampling=1), 128,
        dict(lanes=71, passes=15, longest_code=16, zrl=60, stuffed=46)),
    "noise_64x64_q100_444": (lambda: _noise(64, 64, 8), dict(quality=100, subsampling=0), 256,      # long codes, many passes
        dict(lanes=522, passes=147, longest_code=16, zrl=0, stuffed=102)),
    "const_128x128_420": (lambda: np.zeros((128, 128, 3), np.uint8), dict(subsampling=2), 128,      # never synchronises
        dict(lanes=17, passes=17, longest_code=6, zrl=0, stuffed=0)),
    "checker_128x128_444": (_checker, dict(quality=95, subsampling=0), 128,
        dict(lanes=59, passes=12, longest_code=8, zrl=0, stuffed=24)),
    "smooth_96x128_S128": (lambda: _smooth(96, 128, 9), dict(quality=75), 128,
        dict(lanes=94, passes=18, longest_code=16, zrl=0, stuffed=3)),
    "smooth_96x128_S1024": (lambda: _smooth(96, 128, 9), dict(quality=75), 1024,
        dict(lanes=12, passes=3, longest_code=16, zrl=0, stuffed=3)),
    "smooth_480x640_420_q90": (lambda: _smooth(480, 640, 10), dict(quality=90, subsampling=2), None,      # the only full-size case
        dict(lanes=622, passes=5, longest_code=16, zrl=1100, stuffed=700)),
}


def _jpeg(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", **kw)
    return b.getvalue()


def _pil(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(file, S, the restatement's pixels, its stream statistics incl. the simulated passes); computed once per session."""
    make, kw, S, _ = CASES[name]
    data, stats = _jpeg(make(), **kw), {}
    want = D.decode(data, stats)
    want.setflags(write=False)
    S = S if S is not None else D.default_subseq_bits((D.parse(data)["scan_len"] + 15) // 16 * 16)
    passes, counts, status = D.simulate(data, S)
    stats.update(lanes=len(counts), passes=passes, status=status, counts=counts)
    return data, S, want, stats


# ----------------------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reports_what_the_case_exercises(name):
    data, S, want, stats = _case(name)
    for k, v in CASES[name][3].items():
        assert stats[k] == v, (name, k, {k: stats[k] for k in stats if k != "counts"})
    info = D.parse(data)
    assert want.shape == (info["H"], info["W"], 3) and stats["status"] == 0 and sum(stats["counts"]) == stats["blocks"]
    assert stats["scan_bits"] - 8 < stats["end_bit"] <= stats["scan_bits"]


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_pil(name):
    if not _turbo():
        pytest.skip("PIL is not built on libjpeg-turbo: its decoder is not the one restated")
    data, _, want, _ = _case(name)
    assert np.array_equal(want, _pil(data))


def _parse(data):
    from mspi_amd import _lib
    lib = _lib.load()
    info = _lib.JpegDecInfo()
    rc = lib.mspi_jpeg_dec_parse(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), ctypes.byref(info))
    return rc, info, lib.mspi_last_error()


@pytest.mark.parametrize("name", list(CASES))
def test_parser_equals_restatement(name):
    data = _case(name)[0]
    rc, info, _ = _parse(data)
    ref = D.parse(data)
    assert rc == 0
    assert (info.H, info.W, info.ncomp, info.hs, info.vs) == (ref["H"], ref["W"], ref["ncomp"], ref["hs"], ref["vs"])
    assert (info.scan_off, info.scan_len, info.tables.scan_len) == (ref["scan_off"], ref["scan_len"], ref["scan_len"])
    assert data[info.scan_off + info.scan_len:info.scan_off + info.scan_len + 2] == b"\xff\xd9"
    for c in range(ref["ncomp"]):
        assert list(info.tables.quant[c]) == ref["quant"][c].tolist()
        assert (info.tables.comp_dc[c], info.tables.comp_ac[c]) == (ref["comp_dc"][c], ref["comp_ac"][c])
    for t in range(4):
        if ref["counts"][t] is not None:
            assert list(info.tables.counts[t]) == ref["counts"][t]
            assert list(info.tables.vals[t])[:len(ref["vals"][t])] == ref["vals"][t]


def test_custom_tables_are_in_the_files():
    """The optimize=True and qtables cases carry tables of their own, not Annex K's."""
    std = D.parse(_case("toy_48x64_420_q75")[0])
    assert D.parse(_case("opt_48x64_q60")[0])["counts"][2] != std["counts"][2]
    q = D.parse(_case("qtables_48x64")[0])["quant"]
    assert q[0].tolist() == _QTABLES[0] and q[1].tolist() == q[2].tolist() == _QTABLES[1]      # PIL takes them in natural order


def _refused():
    from PIL import Image
    img, good = _smooth(48, 64, 6), _case("toy_48x64_420_q75")[0]
    b = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(b, format="JPEG")
    return {"progressive": (_jpeg(img, progressive=True), b"progressive"),
            "restart": (_jpeg(img, restart_marker_blocks=1), b"restart"),
            "cmyk": (b.getvalue(), b"4 components"),
            "cut_header": (good[:200], b"truncated"),
            "empty": (b"", b"empty")}


@pytest.mark.parametrize("what", ["progressive", "restart", "cmyk", "cut_header", "empty"])
def test_parser_refuses_with_a_reason(what):
    from mspi_amd import engine as E
    data, reason = _refused()[what]
    rc, _, err = _parse(data)
    assert rc == -1 and reason in err, err
    assert E.jpeg_probe(data) is None
    assert E.jpeg_probe(_case("toy_48x64_420_q75")[0]).W == 64


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
    for name in ("MspiJpegDecTables", "MspiJpegDecInfo", "MspiJpegDecDesc"):
        assert name in hdr
    assert ctypes.sizeof(_lib.JpegDecTables) == 8 + 3 * 64 * 2 + 8 + 4 * 16 + 4 * 256
    assert ctypes.sizeof(_lib.JpegDecInfo) == 32 + ctypes.sizeof(_lib.JpegDecTables)
    assert ctypes.sizeof(_lib.JpegDecDesc) == 8 * 4 + 4 * 8


def _desc(H=37, W=53, B=1, ncomp=3, hs=2, vs=2, S=128, cap=1024, pitch=None):
    from mspi_amd import _lib
    d = _lib.JpegDecDesc()
    d.B, d.H, d.W, d.ncomp, d.hs, d.vs, d.S = B, H, W, ncomp, hs, vs, S
    d.scan_stride = d.scan_cap = cap
    d.pitch = 3 * W if pitch is None else pitch
    d.img_stride = d.pitch * H
    return d


def test_refusals():
    """Bad descriptors are refused on the host, before any launch, and say why."""
    from mspi_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_ubyte * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16)

    def fwd(d, scans=p, tables=p, rgb=p, status=p, passes=p, ws=p):
        return lib.mspi_jpeg_dec_fwd(ctypes.byref(d), scans, tables, rgb, status, passes, ws, None)

    for kw in (dict(scans=None), dict(tables=None), dict(rgb=None), dict(status=None), dict(passes=None), dict(ws=None)):
        assert fwd(_desc(), **kw) == -1 and b"null" in lib.mspi_last_error()
    assert lib.mspi_jpeg_dec_fwd(None, p, p, p, p, p, p, None) == -1 and b"null" in lib.mspi_last_error()
    for H, W in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        d = _desc(H=H, W=W)
        assert fwd(d) == -1 and b"65535" in lib.mspi_last_error() and lib.mspi_jpeg_dec_ws_bytes(ctypes.byref(d)) == 0
    assert fwd(_desc(pitch=3 * 53 - 1)) == -1 and b"pitch" in lib.mspi_last_error()
    for S in (0, 96, 160 + 16, -128):
        assert fwd(_desc(S=S)) == -1 and b"S = " in lib.mspi_last_error()
    assert fwd(_desc(S=128, cap=16 * 1024 + 16)) == -1 and b"subsequences" in lib.mspi_last_error()      # 1025 of them
    assert lib.mspi_jpeg_dec_ws_bytes(ctypes.byref(_desc(S=128, cap=16 * 1024))) > 0                      # 1024
    for kw in (dict(ncomp=2), dict(ncomp=4), dict(hs=1, vs=2), dict(hs=4, vs=1), dict(ncomp=1, hs=2, vs=2)):
        assert fwd(_desc(**kw)) == -1 and (b"sampling" in lib.mspi_last_error() or b"components" in lib.mspi_last_error())
    assert fwd(_desc(W=2, hs=2, vs=1)) == -1 and b"chroma width" in lib.mspi_last_error()
    assert fwd(_desc(B=0)) == -1 and b"batch" in lib.mspi_last_error()
    assert fwd(_desc(), ws=ctypes.c_void_p(p.value + 4)) == -1 and b"aligned" in lib.mspi_last_error()
    d = _desc(480, 640, B=8, cap=96 * 1024, S=1024)
    assert lib.mspi_jpeg_dec_ws_bytes(ctypes.byref(d)) % 16 == 0
    assert lib.mspi_jpeg_dec_ws_bytes(ctypes.byref(d)) >= 8 * (96 * 1024 + 7200 * 128 + 480 * 640 * 3 // 2)


def test_engine_refuses_mixed_geometry_and_unsupported_files():
    from mspi_amd import engine as E
    from mspi_amd._lib import MspiError
    with pytest.raises(MspiError, match="mixed geometry"):
        E.jpeg_decode_rgb([_case("smooth_17x19_444")[0], _case("smooth_17x19_420")[0]])
    with pytest.raises(MspiError, match="mixed geometry"):
        E.jpeg_decode_rgb([_case("toy_48x64_420_q75")[0], _case("smooth_96x128_S128")[0]])
    with pytest.raises(MspiError, match="progressive"):
        E.jpeg_decode_rgb([_refused()["progressive"][0]])
    with pytest.raises(MspiError):
        E.jpeg_decode_rgb([])
    assert E.jpeg_subseq_bits(80 * 1024) == D.default_subseq_bits(80 * 1024) == 1024
    assert E.jpeg_subseq_bits(1 << 20) == D.default_subseq_bits(1 << 20) == 8192


# ----------------------------------------------------------------------------- on the GPU
GUARD = 64


def _decode(dev, files, S, scan_lens=None):
    """Straight through the C ABI: the output rows have a pitch of 3 * W + 16 and are pre-filled with 0xA5, GUARD bytes of 0xA5
    lie behind the last image and behind the workspace.  Returns (rgb [B,H,W,3], status, passes) as numpy after checking that
    no byte outside the images was written.  scan_lens: override the scan length of each file (truncation)."""
    from mspi_amd import _lib
    lib = _lib.load()
    infos = []
    for f in files:
        rc, info, err = _parse(f)
        assert rc == 0, err
        infos.append(info)
    if scan_lens is not None:
        for info, n in zip(infos, scan_lens):
            info.tables.scan_len = n
    B, H, W = len(files), infos[0].H, infos[0].W
    cap = (max(i.scan_len for i in infos) + 15) // 16 * 16
    tsz = ctypes.sizeof(_lib.JpegDecTables)
    host = np.zeros(B * (tsz + cap), dtype=np.uint8)
    for k, (f, info) in enumerate(zip(files, infos)):
        host[k * tsz:(k + 1) * tsz] = np.frombuffer(ctypes.string_at(ctypes.addressof(info.tables), tsz), dtype=np.uint8)
        host[B * tsz + k * cap:B * tsz + k * cap + info.scan_len] = np.frombuffer(f, np.uint8, info.scan_len, info.scan_off)
    inp = torch.from_numpy(host).to(dev)
    d = _desc(H, W, B, infos[0].ncomp, infos[0].hs, infos[0].vs, S, cap, pitch=3 * W + 16)
    need = lib.mspi_jpeg_dec_ws_bytes(ctypes.byref(d))
    assert need > 0, lib.mspi_last_error()
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((B * d.img_stride + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.full((B,), -7, dtype=torch.int32, device=dev)
    passes = torch.full((B,), -7, dtype=torch.int32, device=dev)
    _lib.check(lib.mspi_jpeg_dec_fwd(ctypes.byref(d), inp.data_ptr() + B * tsz, inp.data_ptr(), out.data_ptr(), status.data_ptr(),
                                     passes.data_ptr(), ws.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "mspi_jpeg_dec_fwd")
    torch.cuda.synchronize()
    assert (ws[need:] == 0xA5).all(), "bytes written behind the workspace"
    out = out.cpu().numpy()
    assert (out[B * d.img_stride:] == 0xA5).all(), "bytes written behind the last image"
    rows = out[:B * d.img_stride].reshape(B, H, 3 * W + 16)
    assert (rows[:, :, 3 * W:] == 0xA5).all(), "bytes written between the rows"
    return rows[:, :, :3 * W].reshape(B, H, W, 3), status.cpu().numpy(), passes.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_decoder_equals_restatement(dev, name):
    data, S, want, stats = _case(name)
    rgb, status, passes = _decode(dev, [data], S)
    print(name, "S", S, "lanes", stats["lanes"], "passes", int(passes[0]), "simulated", stats["passes"], "status", int(status[0]))
    assert status[0] == 0 and passes[0] == stats["passes"]
    bad = np.argwhere((rgb[0] != want).any(2))
    assert bad.size == 0, "%d pixels differ, the first at %s" % (len(bad), bad[0])
    if _turbo():
        assert np.array_equal(rgb[0], _pil(data))


@pytest.mark.gpu
def test_three_files_of_one_geometry_in_one_launch(dev):
    """Different Huffman and quantiser tables, different scan lengths."""
    img = _smooth(48, 64, 6)
    files = [_jpeg(img, quality=60, optimize=True), _jpeg(img[::-1].copy(), quality=95),
             _jpeg(_noise(48, 64, 5), qtables=_QTABLES, subsampling=2)]
    assert len({D.parse(f)["scan_len"] for f in files}) == 3
    rgb, status, passes = _decode(dev, files, 128)
    for k, f in enumerate(files):
        assert status[k] == 0 and passes[k] == D.simulate(f, 128)[0]
        assert np.array_equal(rgb[k], D.decode(f)), k


@pytest.mark.gpu
def test_two_launches_are_identical_and_engine_wrapper(dev):
    from mspi_amd import engine as E
    data, S, want, stats = _case("smooth_96x128_S128")
    other = _jpeg(_smooth(96, 128, 11), quality=85)
    a = E.jpeg_decode_rgb([data, other], device=dev)
    b = E.jpeg_decode_rgb([data, other], device=dev)
    c = E.jpeg_decode_rgb([data], subseq_bits=128, device=dev)
    assert a[0].is_cuda and a[0].dtype == torch.uint8 and tuple(a[0].shape) == (2, 96, 128, 3) and a[1].dtype == torch.int32
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[1].tolist() == [0, 0] and c[1].tolist() == [0] and c[2].tolist() == [stats["passes"]]
    assert np.array_equal(a[0][0].cpu().numpy(), want) and np.array_equal(c[0][0].cpu().numpy(), want)
    assert np.array_equal(a[0][1].cpu().numpy(), D.decode(other))


@pytest.mark.gpu
def test_damaged_scans_are_reported_and_stay_inside(dev):
    """A scan cut by a third and one with 40 bytes of seeded noise: the clamps keep every access inside the image's own
    buffers (the guards of _decode), the cut one is reported, and the next launch on a good file is exact."""
    data, S, want, _ = _case("smooth_96x128_S128")
    info = D.parse(data)
    rgb, status, _ = _decode(dev, [data], S, scan_lens=[info["scan_len"] * 2 // 3])
    assert status[0] != 0
    noisy = bytearray(data)
    at = info["scan_off"] + info["scan_len"] // 2
    noisy[at:at + 40] = np.random.default_rng(12).integers(0, 255, 40, dtype=np.uint8).tobytes()      # no FF: the scan keeps its length
    rgb, status, _ = _decode(dev, [bytes(noisy)], S)
    assert np.array_equal(rgb[0, :8], want[:8])                     # the rows in front of the damage
    rgb, status, _ = _decode(dev, [data], S)
    assert status[0] == 0 and np.array_equal(rgb[0], want)


@pytest.mark.gpu
def test_decode_frames_routes_refused_and_damaged_files_to_the_host(dev):
    from mspi_amd import preproc
    good, img = _case("toy_48x64_420_q75")[0], _smooth(48, 64, 6)
    info = D.parse(good)
    cut = good[:info["scan_off"] + info["scan_len"] // 2] + b"\xff\xd9"          # PIL decodes what is there; the device reports it
    blobs = [good, _jpeg(img, progressive=True), _case("grey_37x53")[0], cut, _jpeg(img, restart_marker_blocks=1), good]
    stats = {}
    frames = preproc.decode_frames(blobs, dev, stats)
    assert stats == {"device": 3, "host": 3}
    for f, t in zip(blobs, frames):
        assert t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), _pil(f))


def _make_dataset(root, name="clip1", n_frames=34, hw=(48, 64), fps=25, sr=22050, progressive=(7,)):
    """The toy dataset of tests/test_inference.py (a copy: test modules do not import from each other), with the frames in
    `progressive` saved as progressive JPEG: the device decoder hands those to the host."""
    from PIL import Image
    from scipy.io import wavfile
    rng = np.random.RandomState(0)
    fdir = os.path.join(root, "video_frames", "TOY", name)
    adir = os.path.join(root, "video_audio", "TOY", name)
    os.makedirs(fdir), os.makedirs(adir), os.makedirs(os.path.join(root, "fold_lists"))
    for i in range(n_frames):
        Image.fromarray(rng.randint(0, 255, (hw[0], hw[1], 3), dtype=np.uint8)).save(os.path.join(fdir, "img_%05d.jpg" % (i + 1)),
                                                                                     progressive=i in progressive)
    t = np.arange(int(sr * n_frames / fps) + sr) / sr
    wav = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * rng.randn(t.size)).astype(np.float32)
    wavfile.write(os.path.join(adir, name + ".wav"), sr, np.stack([wav, 0.5 * wav], 1))     # stereo
    with open(os.path.join(root, "fold_lists", "TOY_list_test_2_fps.txt"), "w") as f:
        f.write("%s %d %d\n" % (name, n_frames, fps))


def test_device_frame_decoder_reads_bytes_without_a_gpu(tmp_path, monkeypatch):
    """--device_decode's frame source: chunks of `chunk` frames, each asked once in increasing order, bytes read on the pool
    one chunk ahead; the decode itself is replaced by a recorder here."""
    from mspi_amd import inference as I
    from mspi_amd import preproc
    _make_dataset(str(tmp_path), n_frames=12)
    fdir = os.path.join(str(tmp_path), "video_frames", "TOY", "clip1")
    paths = sorted(os.path.join(fdir, n) for n in os.listdir(fdir))
    calls = []
    monkeypatch.setattr(preproc, "decode_frames",
                        lambda blobs, device, stats=None, host_decode=None: calls.append(len(blobs)) or list(blobs))
    for workers in (0, 3):
        dec = I._DeviceFrameDecoder(paths, workers, 5)
        try:
            for j in range(12):
                assert dec.get(j) == open(paths[j], "rb").read()
                assert len(dec.pending) <= 5
        finally:
            dec.close()
    assert calls == [5, 5, 2, 5, 5, 2]
    assert I._device_decode(types.SimpleNamespace(device_decode=True)) and not I._device_decode(types.SimpleNamespace())


@pytest.mark.gpu
def test_clip_loop_writes_the_same_files(dev, tmp_path):
    """inference_dataset with the flags off, with device_decode, and with device_decode + device_jpeg + workers: the same
    names, the same bytes.  A first run with the flags off comes before the three and is not compared: the first forwards of a
    freshly built model are not the later ones (engine.autotune times kernel candidates, and the operand-range check moves
    an out-of-range layer to the fp32 path from the next forward on)."""
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
    for tag, kw in (("first", {}), ("off", {}), ("device_decode", dict(device_decode=True)),
                    ("all", dict(device_decode=True, device_jpeg=True, workers=4))):
        args = types.SimpleNamespace(clip_size=16, dataset="TOY", split=2, path_data=root, save_path=str(tmp_path / tag),
                                     use_sound=True, batch=5, **kw)
        I.inference_dataset(model, args)
        names = sorted(os.listdir(os.path.join(args.save_path, "clip1")))
        trees[tag] = {n: open(os.path.join(args.save_path, "clip1", n), "rb").read() for n in names}
    assert len(trees["off"]) == 34
    for tag in ("device_decode", "all"):
        assert sorted(trees[tag]) == sorted(trees["off"])
        bad = [n for n in trees["off"] if trees[tag][n] != trees["off"][n]]
        assert not bad, (tag, bad[:5])


@pytest.mark.gpu
def test_dataset_batch_with_device_decode_is_the_same_batch(dev, tmp_path):
    from PIL import Image
    import scipy.io
    from mspi_amd.avsp_dataloader import AudioVisualDataset
    root, rng, T = str(tmp_path), np.random.default_rng(3), 4
    os.makedirs(os.path.join(root, "fold_lists"))
    with open(os.path.join(root, "fold_lists", "TOY_list_val_2_fps.txt"), "w") as f:
        f.write("v1 9 25\nv2 9 25\n")
    for v, (H, W) in (("v1", (48, 64)), ("v2", (37, 53))):
        adir, fdir = os.path.join(root, "annotations", "TOY", v), os.path.join(root, "video_frames", "TOY", v)
        os.makedirs(os.path.join(adir, "maps")), os.makedirs(fdir)
        for i in range(1, 10):
            Image.fromarray(rng.integers(1, 256, (H, W), dtype=np.uint8)).save(os.path.join(adir, "maps", "eyeMap_%05d.jpg" % i))
            fix = np.zeros((H, W), np.uint8)
            fix.reshape(-1)[rng.choice(H * W, size=9, replace=False)] = 255
            scipy.io.savemat(os.path.join(adir, "fixMap_%05d.mat" % i), {"eyeMap": fix})
        for i in range(1, 11):
            Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(fdir, "img_%05d.jpg" % i),
                                                                                progressive=(i == 3))
    kw = dict(batch_size=4, with_fixations=True, workers=2, device=dev)
    off = list(AudioVisualDataset(root, "TOY", 2, T, "val", False, (32, 48), **kw))
    on = list(AudioVisualDataset(root, "TOY", 2, T, "val", False, (32, 48), device_decode=True, **kw))
    assert len(off) == len(on) == 1 and off[0][0].shape == (2, 3, T, 32, 48)
    for a, b in zip(off[0], on[0]):
        assert torch.equal(a, b)
