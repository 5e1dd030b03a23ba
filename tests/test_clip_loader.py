"""Clip assembly (mspi_clip_resize_norm_fwd / preproc.assemble_clips) and the dataset that feeds it
(mspi_amd.avsp_dataloader).  Without a GPU: the symbol, the argument checks, the tile planner with a numpy emulation of the
tiled two-pass algorithm against PIL, the clip list on a toy tree.  On the GPU: exact equality with PIL + ToTensor +
Normalize and with the per-frame path, graph capture, a dataset batch against a per-sample restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (Hin, Win, Hout, Wout): the vertical cases the planner has to cover, each with a width of its own
SIZES = [(480, 640, 224, 384), (360, 640, 224, 384), (100, 150, 224, 384), (224, 384, 224, 384), (481, 641, 64, 94),
         (1080, 1920, 224, 384)]


# ------------------------------------------------------------------------------------------------ symbols, arguments
def test_clip_symbol_is_declared_exported_and_bound():
    from mspi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mspi_hip.h")).read()
    assert re.search(r"\bint\s+mspi_clip_resize_norm_fwd\s*\(", hdr)
    assert "mspi_clip_resize_norm_fwd" in _lib.EXPORTS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert raw.mspi_clip_resize_norm_fwd is not None
    lib = _lib.load()
    assert lib.mspi_clip_resize_norm_fwd.restype is ctypes.c_int and len(lib.mspi_clip_resize_norm_fwd.argtypes) == 26
    assert lib.mspi_version() == 2


class _Call:
    """A well-formed argument list of mspi_clip_resize_norm_fwd over HOST buffers: every test changes one thing, and the
    entry point has to refuse before it launches (it never dereferences the device pointers on the host)."""

    def __init__(self, N=4, B=2, T=4, Hin=20, Win=30, Hout=8, Wout=12):
        from mspi_amd.preproc import pil_bilinear_coeffs
        self.hb, self.hk, self.hks = pil_bilinear_coeffs(Win, Wout)
        self.vb, self.vk, self.vks = pil_bilinear_coeffs(Hin, Hout)
        self.frames = np.zeros(max(N, 1) * Hin * Win * 3 + 16, np.uint8)
        self.out = np.zeros(B * 3 * T * Hout * Wout, np.float32)
        self.slots = np.arange(max(N, 1), dtype=np.int32)
        self.mean, self.std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
        self.a = dict(frames=self.frames.ctypes.data, N=N, Hin=Hin, Win=Win, slots=self.slots.ctypes.data,
                      slots_host=self.slots.ctypes.data, out=self.out.ctypes.data, B=B, T=T, sB=3 * T * Hout * Wout,
                      sC=T * Hout * Wout, sT=Hout * Wout, sH=Wout, Hout=Hout, Wout=Wout, hb=self.hb.ctypes.data,
                      hb_host=self.hb.ctypes.data, hk=self.hk.ctypes.data, hks=self.hks, vb=self.vb.ctypes.data,
                      vb_host=self.vb.ctypes.data, vk=self.vk.ctypes.data, vks=self.vks, mean=self.mean, std=self.std, stream=None)

    def __call__(self, **change):
        from mspi_amd import _lib
        lib = _lib.load()
        a = dict(self.a, **change)
        rc = lib.mspi_clip_resize_norm_fwd(*[a[k] for k in self.a])
        return rc, lib.mspi_last_error().decode()


def test_clip_arguments_are_refused_before_launch():
    c = _Call()
    for name in ("frames", "slots", "slots_host", "out", "hb", "hb_host", "hk", "vb", "vb_host", "vk", "mean", "std"):
        rc, msg = c(**{name: None})
        assert rc == -1 and "null" in msg, (name, rc, msg)
    for name in ("N", "Hin", "Win", "Hout", "Wout", "B", "T", "hks", "vks"):
        rc, msg = c(**{name: 0})
        assert rc == -1 and "extent" in msg, (name, rc, msg)
    assert c(N=-3)[0] == -1
    for name, v in (("sH", 11), ("sT", 8 * 12 - 1), ("sC", 4 * 8 * 12 - 1), ("sB", 3 * 4 * 8 * 12 - 1)):
        rc, msg = c(**{name: v})
        assert rc == -1 and "strides" in msg, (name, rc, msg)
    for bad in (8, -1, 2 ** 31 - 1):
        s = np.array([0, 1, bad, 3], np.int32)
        rc, msg = c(slots_host=s.ctypes.data)
        assert rc == -1 and "outside" in msg, (bad, rc, msg)
    s = np.array([0, 5, 2, 5], np.int32)
    rc, msg = c(slots_host=s.ctypes.data)
    assert rc == -1 and "twice" in msg
    rc, msg = c(N=9)                                    # more frames than slots
    assert rc == -1
    rc, msg = c(frames=c.frames.ctypes.data + 1)
    assert rc == -1 and "aligned" in msg
    # bounds tables that point outside the frame
    vb = c.vb.copy()
    vb[-1, 1] += 1
    rc, msg = c(vb_host=vb.ctypes.data)
    assert rc == -1 and "vertical" in msg
    hb = c.hb.copy()
    hb[3, 0] = -1
    rc, msg = c(hb_host=hb.ctypes.data)
    assert rc == -1 and "horizontal" in msg
    # nothing fits: the entry point says so and points at the per-frame call
    big = _Call(N=1, B=1, T=1, Hin=4000, Win=30, Hout=2, Wout=12000)
    rc, msg = big()
    assert rc == -1 and "fits" in msg


# ------------------------------------------------------------------------------------------------ tile planner
def _h_pass(rows, hb, hk):
    """uint8 [r, Wout, 3] from uint8 [r, Win, 3]: PIL's horizontal pass, vectorised over the taps."""
    ks = hk.shape[1]
    idx = np.minimum(hb[:, :1] + np.arange(ks)[None], rows.shape[1] - 1)          # taps beyond n have weight 0
    w = np.where(np.arange(ks)[None] < hb[:, 1:], hk, 0).astype(np.int64)
    s = (rows[:, idx, :].astype(np.int64) * w[None, :, :, None]).sum(2) + (1 << 21)
    return np.clip(s >> 22, 0, 255).astype(np.uint8)


def _emulate_tiled(img, Hout, Wout, plan):
    """The kernel's algorithm in numpy: per tile, the staged rows [r0, r0 + staged_rows) are resampled horizontally in
    batches of batch_rows, and the vertical pass reads ONLY that staging buffer."""
    from mspi_amd.preproc import pil_bilinear_coeffs
    Hin, Win = img.shape[:2]
    hb, hk, _ = pil_bilinear_coeffs(Win, Wout)
    vb, vk, _ = pil_bilinear_coeffs(Hin, Hout)
    TH, R, RB = plan["tile_rows"], plan["staged_rows"], plan["batch_rows"]
    out = np.zeros((Hout, Wout, 3), np.uint8)
    for y0 in range(0, Hout, TH):
        y1 = min(Hout, y0 + TH)
        r0 = int(vb[y0, 0])
        r1 = int(vb[y1 - 1, 0] + vb[y1 - 1, 1])
        assert r1 - r0 <= R and r1 <= Hin
        hbuf = np.full((R, Wout, 3), 0xEE, np.uint8)
        for rb in range(r0, r1, RB):
            nb = min(RB, r1 - rb)
            hbuf[rb - r0:rb - r0 + nb] = _h_pass(img[rb:rb + nb], hb, hk)
        for y in range(y0, y1):
            ymin, n = int(vb[y, 0]), int(vb[y, 1])
            assert r0 <= ymin and ymin + n <= r1
            s = (hbuf[ymin - r0:ymin - r0 + n].astype(np.int64) * vk[y, :n].astype(np.int64)[:, None, None]).sum(0) + (1 << 21)
            out[y] = np.clip(s >> 22, 0, 255)
    return out


@pytest.mark.parametrize("Hin,Win,Hout,Wout", SIZES)
def test_tile_plan_covers_every_row_and_emulation_equals_pil(Hin, Win, Hout, Wout):
    from PIL import Image
    from mspi_amd.preproc import clip_tile_plan, pil_bilinear_coeffs
    plan = clip_tile_plan(Hin, Win, Hout, Wout)
    assert plan is not None, "the planner refuses a size the clip loop meets"
    TH, R, RB = plan["tile_rows"], plan["staged_rows"], plan["batch_rows"]
    assert 1 <= TH <= Hout and 1 <= RB <= R
    WP = (Wout + 3) // 4 * 4
    assert RB * Win * 3 + 8 <= 8 * 1024 and R * 3 * WP <= 32 * 1024          # the two LDS images
    assert plan["lds_bytes"] <= 40 * 1024 and plan["lds_bytes"] >= RB * Win * 3 + R * 3 * WP
    vb, _, _ = pil_bilinear_coeffs(Hin, Hout)
    for y in range(Hout):
        r0 = vb[y // TH * TH, 0]
        assert r0 <= vb[y, 0] and vb[y, 0] + vb[y, 1] <= min(r0 + R, Hin), y
    rng = np.random.default_rng(Hin * 7 + Hout)
    for img in (rng.integers(0, 256, (Hin, Win, 3), dtype=np.uint8), np.full((Hin, Win, 3), 255, np.uint8)):
        ref = np.asarray(Image.fromarray(img).resize((Wout, Hout), Image.BILINEAR))
        assert np.array_equal(_emulate_tiled(img, Hout, Wout, plan), ref)


def test_tile_plan_refuses_what_does_not_fit():
    from mspi_amd.preproc import clip_tile_plan
    assert clip_tile_plan(100000, 64, 1, 64) is None            # one output row taps every input row
    assert clip_tile_plan(20000, 640, 8, 384) is None
    assert clip_tile_plan(480, 3000, 224, 384) is None          # a row of the frame is larger than the load buffer
    assert clip_tile_plan(480, 640, 224, 11000) is None         # a single staged row is larger than the staging buffer
    assert clip_tile_plan(2 ** 18, 2700, 3, 10900) is None      # large extents: no overflow on the way to the refusal
    assert clip_tile_plan(48, 64, 32, 48) is not None


# ------------------------------------------------------------------------------------------------ clip list
def _smooth(rng, H, W):
    y, x = np.mgrid[0:H, 0:W]
    cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
    return np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * (0.2 * min(H, W)) ** 2))


def _make_tree(root, videos, dataset="TOY", split=2, mode="val", empty=(), frames=True, audio=True, seed=0, fps=25):
    """A dataset directory.  videos: [(name, n annotated frames, (H, W) of frames and maps)]; frames are numbered from 1
    and there is one frame more than maps (clips read img_%05d up to start + len_clip).  empty: {(video, frame)} whose
    density is all zero.  The fold list is written in REVERSE order: the reader sorts."""
    from PIL import Image
    import scipy.io
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "fold_lists"), exist_ok=True)
    name = "DIEM_list_%s_fps.txt" % mode if dataset == "DIEM" else "%s_list_%s_%d_fps.txt" % (dataset, mode, split)
    with open(os.path.join(root, "fold_lists", name), "w") as f:
        for v, n, _ in reversed(videos):
            f.write("%s %d %d\n" % (v, n, fps))
    for v, n, (H, W) in videos:
        adir = os.path.join(root, "annotations", dataset, v)
        os.makedirs(os.path.join(adir, "maps"))
        for i in range(1, n + 1):
            dens = np.zeros((H, W), np.uint8) if (v, i) in empty else np.round(255 * _smooth(rng, H, W)).astype(np.uint8)
            Image.fromarray(dens).save(os.path.join(adir, "maps", "eyeMap_%05d.jpg" % i), quality=95)
            fix = np.zeros((H, W), np.uint8)
            fix.reshape(-1)[rng.choice(H * W, size=int(rng.integers(5, 40)), replace=False)] = 1
            scipy.io.savemat(os.path.join(adir, "fixMap_%05d.mat" % i), {"eyeMap": fix * 255})
        if frames:
            fdir = os.path.join(root, "video_frames", dataset, v)
            os.makedirs(fdir)
            for i in range(1, n + 2):
                Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(fdir, "img_%05d.jpg" % i))
        if audio:
            wdir = os.path.join(root, "video_audio", dataset, v)
            os.makedirs(wdir)
            sr = 22050
            t = np.arange(int(sr * (n + 2) / fps) + sr) / sr
            wav = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.1 * rng.standard_normal(t.size)).astype(np.float32)
            wavfile.write(os.path.join(wdir, v + ".wav"), sr, np.stack([wav, 0.5 * wav], 1))
    return root


def _reference_val_list(root, dataset, names, len_snippet):
    """avsp_dataloader.py:118-133 restated: sorted names, starts range(0, len(frames) - len_snippet, 2 * len_snippet), kept
    where eyeMap_%05d.jpg % (i + len_snippet) is not all zero (check_frame, :137-139, with PIL in cv2.imread's place)."""
    from PIL import Image
    out = []
    for v in sorted(names):
        maps = os.path.join(root, "annotations", dataset, v, "maps")
        frames = sorted(os.listdir(maps))
        for i in range(0, len(frames) - len_snippet, 2 * len_snippet):
            img = np.asarray(Image.open(os.path.join(maps, "eyeMap_%05d.jpg" % (i + len_snippet))).convert("L"))
            if img.max() != 0:
                out.append((v, i))
    return out


def test_clip_list_on_a_toy_tree(tmp_path):
    from mspi_amd.avsp_dataloader import AudioVisualDataset
    T = 4
    videos = [("vb", 21, (12, 16)), ("va", 30, (12, 16)), ("short", 3, (12, 16)), ("vc", 9, (10, 14))]
    empty = {("va", 12), ("vb", 4), ("vb", 20)}               # va: start 8; vb: starts 0 and 16
    root = _make_tree(str(tmp_path / "d"), videos, empty=empty, frames=False, audio=False)
    ds = AudioVisualDataset(root, "TOY", 2, T, "val", True, (8, 8))
    assert ds.list_indata == ["short", "va", "vb", "vc"]                       # the fold list was written unsorted
    want = _reference_val_list(root, "TOY", [v[0] for v in videos], T)
    assert ds.list_num_frame == want and ds.clip_list() == want and len(ds) == len(want)
    assert ("va", 8) not in want and ("vb", 0) not in want and ("vb", 16) not in want
    assert ("va", 0) in want and ("va", 24) in want and ("vb", 8) in want and ("vc", 0) in want
    assert not [c for c in want if c[0] == "short"]                            # shorter than a clip: no start at all
    assert ds.videos_fps["va"].strip() == "25"
    # DIEM: the list name carries no split
    root2 = _make_tree(str(tmp_path / "e"), [("d1", 9, (10, 14))], dataset="DIEM", mode="test", frames=False, audio=False)
    assert AudioVisualDataset(root2, "DIEM", 7, T, "test", True, (8, 8)).list_num_frame == [("d1", 0)]
    with pytest.raises(FileNotFoundError):
        AudioVisualDataset(root2, "DIEM", 7, T, "val", True, (8, 8))
    # a missing annotation is named
    os.remove(os.path.join(root, "annotations", "TOY", "vc", "maps", "eyeMap_00004.jpg"))
    with pytest.raises(FileNotFoundError, match="eyeMap_00004.jpg"):
        AudioVisualDataset(root, "TOY", 2, T, "val", True, (8, 8))


def test_train_starts_come_from_the_generator(tmp_path):
    """avsp_dataloader.py:144-156: one start per video in [0, n - len_snippet], drawn again while the clip's label is all
    zero -- from the Generator handed in, so two equal generators give equal lists and the global state is not touched."""
    from mspi_amd.avsp_dataloader import AudioVisualDataset
    from mspi_amd._lib import MspiError
    T = 4
    videos = [("vb", 7, (12, 16)), ("va", 12, (12, 16))]
    empty = {("vb", i) for i in (4, 5, 6)} | {("va", i) for i in range(4, 12)}      # vb: only start 3 is left; va: only 8
    root = _make_tree(str(tmp_path / "d"), videos, mode="train", empty=empty, frames=False, audio=False)
    state = np.random.get_state()[1].copy()
    lists = []
    for _ in range(2):
        ds = AudioVisualDataset(root, "TOY", 2, T, "train", True, (8, 8), generator=np.random.default_rng(5))
        assert len(ds) == 2 and ds.list_num_frame == [12, 7]
        lists.append([ds.clip_list() for _ in range(3)])
    assert lists[0] == lists[1]
    for epoch in lists[0]:
        assert epoch == [("va", 8), ("vb", 3)]                   # never on a zero map
    assert np.array_equal(np.random.get_state()[1], state)
    # starts cover the whole range where every map is defined
    root2 = _make_tree(str(tmp_path / "e"), [("vd", 6, (12, 16))], mode="train", frames=False, audio=False)
    ds = AudioVisualDataset(root2, "TOY", 2, T, "train", True, (8, 8), generator=np.random.default_rng(1))
    seen = {ds.clip_list()[0][1] for _ in range(200)}
    assert seen == {0, 1, 2}                                     # np.random.randint(0, 6 - 4 + 1)
    with pytest.raises(MspiError, match="Generator"):
        AudioVisualDataset(root2, "TOY", 2, T, "train", True, (8, 8)).clip_list()
    root3 = _make_tree(str(tmp_path / "f"), [("tiny", 3, (12, 16))], mode="train", frames=False, audio=False)
    with pytest.raises(ValueError, match="tiny"):
        AudioVisualDataset(root3, "TOY", 2, T, "train", True, (8, 8), generator=np.random.default_rng(1)).clip_list()


def test_dataset_refuses_a_cpu_device(tmp_path):
    from mspi_amd.avsp_dataloader import AudioVisualDataset
    from mspi_amd._lib import MspiError
    root = _make_tree(str(tmp_path / "d"), [("va", 9, (12, 16))], frames=False, audio=False)
    with pytest.raises(MspiError, match="GPU"):
        next(iter(AudioVisualDataset(root, "TOY", 2, 4, "val", True, (8, 8), device="cpu")))


# ------------------------------------------------------------------------------------------------ GPU: the kernel
GUARD = 64


def _guarded_u8(frames, dev):
    """The frames in the middle of a larger device buffer of 0xA5 bytes (GUARD on each side)."""
    n = frames.size
    big = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    big[GUARD:GUARD + n] = torch.from_numpy(frames.reshape(-1)).to(dev)
    return big, big[GUARD:GUARD + n].view(frames.shape)


def _guarded_out(shape, dev):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), 12345.0, dtype=torch.float32, device=dev)
    big[GUARD:GUARD + n] = float("nan")
    return big, big[GUARD:GUARD + n].view(shape)


def _slot_orders(N, B, T, rng):
    return {"forward": np.arange(N), "reversed": np.arange(N)[::-1].copy(), "scattered": rng.permutation(B * T)[:N]}


@pytest.mark.gpu
@pytest.mark.parametrize("Hin,Win,Hout,Wout", SIZES)
def test_assemble_clips_equals_pil_and_the_per_frame_path(dev, Hin, Win, Hout, Wout):
    from mspi_amd import preproc as P
    from oracle import restate as R
    rng = np.random.default_rng(Hin + Wout)
    T = 16
    frames = rng.integers(0, 256, (37, Hin, Win, 3), dtype=np.uint8)
    frames[5] = 255                                                # the value that overflows a sloppy accumulator
    ref = torch.stack([R.frame_transform(f, (Hout, Wout), MEAN, STD) for f in frames])        # PIL + ToTensor + Normalize
    assert P.clip_tile_plan(Hin, Win, Hout, Wout) is not None
    for N in (1, 16, 37):
        B = N // T + 1
        for order, slots in _slot_orders(N, B, T, rng).items():
            in_big, fr = _guarded_u8(frames[:N], dev)
            out_big, out = _guarded_out((B, 3, T, Hout, Wout), dev)
            got = P.assemble_clips(fr, slots, out, MEAN, STD)
            assert got.data_ptr() == out.data_ptr()
            torch.cuda.synchronize()
            host = out.cpu()
            written = np.zeros(B * T, bool)
            for i, s in enumerate(slots.tolist()):
                assert torch.equal(host[s // T, :, s % T], ref[i]), (N, order, i)
                written[s] = True
            for s in np.flatnonzero(~written).tolist():
                assert torch.isnan(host[s // T, :, s % T]).all(), (N, order, s)
            assert (out_big[:GUARD] == 12345.0).all() and (out_big[-GUARD:] == 12345.0).all()
            assert (in_big[:GUARD] == 0xA5).all() and (in_big[-GUARD:] == 0xA5).all()
            assert torch.equal(fr.cpu(), torch.from_numpy(frames[:N]))
    # bit for bit what the per-frame path assembles: resize_normalize per frame, stack, permute
    fr = torch.from_numpy(frames[:32]).to(dev)
    parent = torch.stack([P.resize_normalize(fr[i], (Hout, Wout), MEAN, STD) for i in range(32)]).view(2, T, 3, Hout, Wout).permute(0, 2, 1, 3, 4)
    out = torch.full((2, 3, T, Hout, Wout), float("nan"), device=dev)
    P.assemble_clips(fr, np.arange(32), out, MEAN, STD)
    assert torch.equal(out, parent.contiguous())


@pytest.mark.gpu
def test_assemble_clips_strided_output_and_refusals(dev):
    """A clip tensor whose rows are padded (the scalar-store variant) and the wrapper's own checks."""
    from mspi_amd import preproc as P
    from mspi_amd._lib import MspiError
    from oracle import restate as R
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (5, 37, 53, 3), dtype=np.uint8)
    store = torch.full((2, 3, 4, 21, 31 + 3), float("nan"), device=dev)
    out = store[..., :31]
    P.assemble_clips(torch.from_numpy(frames).to(dev), [7, 0, 3, 4, 2], out, MEAN, STD)
    for i, s in enumerate([7, 0, 3, 4, 2]):
        assert torch.equal(out[s // 4, :, s % 4].cpu(), R.frame_transform(frames[i], (21, 31), MEAN, STD))
    assert torch.isnan(store[..., 31:]).all() and torch.isnan(out[0, :, 1]).all()
    with pytest.raises(MspiError, match="twice"):
        P.assemble_clips(torch.from_numpy(frames).to(dev), [0, 1, 2, 1, 3], out, MEAN, STD)
    with pytest.raises(MspiError, match="outside"):
        P.assemble_clips(torch.from_numpy(frames).to(dev), [0, 1, 2, 8, 3], out, MEAN, STD)
    with pytest.raises(MspiError, match="GPU"):
        P.assemble_clips(torch.from_numpy(frames), [0, 1, 2, 4, 3], out, MEAN, STD)
    # where no tile fits, the wrapper takes the per-frame path: same result
    tall = rng.integers(0, 256, (2, 1500, 24, 3), dtype=np.uint8)
    assert P.clip_tile_plan(1500, 24, 2, 3000) is None
    out = torch.full((1, 3, 2, 2, 3000), float("nan"), device=dev)
    P.assemble_clips(torch.from_numpy(tall).to(dev), [1, 0], out, MEAN, STD)
    for i, s in enumerate([1, 0]):
        assert torch.equal(out[0, :, s].cpu(), R.frame_transform(tall[i], (2, 3000), MEAN, STD))


@pytest.mark.gpu
def test_assemble_clips_in_a_captured_graph(dev):
    from mspi_amd import preproc as P
    from oracle import restate as R
    rng = np.random.default_rng(9)
    N, T, Hin, Win, Hout, Wout = 16, 16, 120, 160, 64, 96
    data = [rng.integers(0, 256, (N, Hin, Win, 3), dtype=np.uint8) for _ in range(3)]
    slots = rng.permutation(N).astype(np.int32)
    slots_dev = torch.from_numpy(slots).to(dev)
    fr = torch.from_numpy(data[0]).to(dev)
    out = torch.full((1, 3, T, Hout, Wout), float("nan"), device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # warm-up: coefficient tables are built and uploaded here
        P.assemble_clips(fr, slots, out, MEAN, STD, slots_dev=slots_dev)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        # counted around the call itself: entering the capture makes torch register its generator state with the graph,
        # which allocates two tensors of torch's own before anything of this project runs
        before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
        P.assemble_clips(fr, slots, out, MEAN, STD, slots_dev=slots_dev)
        after = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    assert after == before, "assemble_clips allocated inside the capture"
    for d in data[1:]:
        fr.copy_(torch.from_numpy(d).to(dev))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        host = out.cpu()
        for i, s in enumerate(slots.tolist()):
            assert torch.equal(host[0, :, s], R.frame_transform(d[i], (Hout, Wout), MEAN, STD))


# ------------------------------------------------------------------------------------------------ GPU: the dataset
def _sample(root, dataset, v, start, T, size, fps, dev, use_sound=True):
    """One sample as avsp_dataloader.py:158-193 builds it, from the per-frame functions of this repository."""
    from PIL import Image
    import scipy.io
    from mspi_amd import evaluate as EV
    from mspi_amd import inference as I
    from oracle import restate as R
    from saliency_eval_restate import resize_fixation
    clip = torch.stack([R.frame_transform(np.asarray(Image.open(os.path.join(root, "video_frames", dataset, v, "img_%05d.jpg" % (start + i + 1))).convert("RGB")), size, MEAN, STD)
                        for i in range(T)]).permute(1, 0, 2, 3)
    ann = os.path.join(root, "annotations", dataset, v)
    gt = np.asarray(Image.open(os.path.join(ann, "maps", "eyeMap_%05d.jpg" % (start + T))).convert("L"))
    lab = EV.resize_maps(torch.from_numpy(gt.copy())[None].to(dev), size)[0]
    if lab.max() > 1.0:
        lab = lab / 255.0
    fix = resize_fixation(np.asarray(scipy.io.loadmat(os.path.join(ann, "fixMap_%05d.mat" % (start + T)))["eyeMap"]), size[0], size[1])
    aud = I.get_audio_feature(os.path.join(root, "video_audio", dataset, v, v + ".wav"), start, fps, len_snippet=T)
    return clip, aud, lab.cpu(), torch.from_numpy(fix).float()


@pytest.mark.gpu
def test_dataset_batches_equal_the_per_sample_restatement(dev, tmp_path):
    """Two source sizes in one batch, a video without a wav, a last partial batch, fixations appended."""
    import shutil
    from mspi_amd.avsp_dataloader import AudioVisualDataset
    T, size = 4, (32, 48)
    videos = [("va", 25, (48, 64)), ("vb", 13, (37, 53)), ("vc", 9, (48, 64))]
    root = _make_tree(str(tmp_path / "d"), videos, empty={("va", 12)})
    shutil.rmtree(os.path.join(root, "video_audio", "TOY", "vc"))
    ds = AudioVisualDataset(root, "TOY", 2, T, "val", True, size, batch_size=3, with_fixations=True, workers=3, device=dev)
    want = [("va", 0), ("va", 16), ("vb", 0), ("vb", 8), ("vc", 0)]
    assert ds.clip_list() == want
    batches = list(ds)
    assert [b[0].shape[0] for b in batches] == [3, 2] and all(len(b) == 4 for b in batches)
    k = 0
    for clips, audio, label, fix in batches:
        assert clips.is_cuda and audio.is_cuda and label.is_cuda and fix.is_cuda
        assert tuple(clips.shape[1:]) == (3, T, 32, 48) and tuple(audio.shape[1:]) == (1, 257, 111)
        for b in range(clips.shape[0]):
            v, start = want[k]
            c, a, l, f = _sample(root, "TOY", v, start, T, size, "25", dev)
            assert torch.equal(clips[b].cpu(), c), (v, start)
            assert torch.equal(label[b].cpu(), l) and 0 < l.max() <= 1.0
            assert torch.equal(fix[b].cpu(), f) and f.sum() > 0
            err = (audio[b].cpu() - a).abs().max().item()
            assert err < 2e-3, "%s %d: audio max abs err %.3e" % (v, start, err)
            if v == "vc":
                assert torch.equal(audio[b].cpu(), torch.full((1, 257, 111), 0.02))
            k += 1
    assert k == len(want)
    # without sound and without fixations: (clips, label), equal clips
    ds2 = AudioVisualDataset(root, "TOY", 2, T, "val", False, size, batch_size=8, device=dev)
    (clips2, label2), = list(ds2)
    assert torch.equal(clips2[:3], batches[0][0]) and torch.equal(label2[3:], batches[1][2])
    # a missing frame is named
    os.remove(os.path.join(root, "video_frames", "TOY", "vb", "img_00010.jpg"))
    with pytest.raises(FileNotFoundError, match="img_00010.jpg"):
        list(AudioVisualDataset(root, "TOY", 2, T, "val", False, size, batch_size=8, device=dev))
