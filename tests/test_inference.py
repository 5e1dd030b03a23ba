"""inference.py surface: host-side front end on CPU; post-process kernel and the clip loop on the GPU."""
import math
import os
import types

import numpy as np
import pytest
import torch


def _make_dataset(root, name="clip1", n_frames=34, hw=(48, 64), fps=25, sr=22050):
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


def test_audio_front_end(tmp_path):
    from mspi_amd import inference as I
    wav = _make_dataset(str(tmp_path))
    a = I.get_audio_feature(wav, start_idx=3, fps=25)
    assert tuple(a.shape) == (1, 257, 111) and torch.isfinite(a).all()
    assert a.mean(1).abs().max() < 1e-4                       # per time-column standardised over the 257 bins
    r = I.get_audio_feature(wav, start_idx=3, fps=25, mode=True)
    assert not torch.allclose(a, r)
    assert torch.allclose(I.get_audio_feature(str(tmp_path / "missing.wav"), 0, 25), torch.full((1, 257, 111), 0.02))
    # sinc resampler: a 1 kHz tone survives 48 kHz -> 16 kHz
    t = torch.arange(48000) / 48000.0
    y = I._sinc_resample(torch.sin(2 * math.pi * 1000 * t)[None], 48000, 16000)
    ref = torch.sin(2 * math.pi * 1000 * torch.arange(16000) / 16000.0)
    assert y.shape[-1] == 16000 and (y[0, 200:-200] - ref[200:-200]).abs().max() < 2e-3


def test_blur_and_transform(tmp_path):
    from mspi_amd import inference as I
    from oracle import restate as R
    _make_dataset(str(tmp_path))
    x = torch.randn(40, 52)
    k = torch.exp(-(torch.arange(11.0) - 5) ** 2 / 8)
    k = k / k.sum()
    ref = torch.nn.functional.conv2d(torch.nn.functional.conv2d(torch.nn.functional.pad(x[None, None], (5, 5, 5, 5), mode="reflect"),
                                                                k.view(1, 1, 1, 11)), k.view(1, 1, 11, 1))[0, 0]
    assert np.abs(I.blur(x.numpy()) - ref.numpy()).max() < 1e-5
    assert I.normalize(np.array([1.0, 3.0])).tolist() == [0.0, 1.0]
    u8 = R.postprocess_u8(torch.randn(20, 30), (48, 64))
    assert u8.dtype == torch.uint8 and int(u8.min()) == 0 and int(u8.max()) == 255


def test_preprocessing_oracle_and_tables(tmp_path):
    """Host side of the GPU pre-processing: the fixed-point tap tables reproduce PIL's resize bit for bit (numpy emulation of
    the two integer passes), the oracle's spectrogram window equals the reference-signature host function, and
    audio_segment cuts what get_audio_feature cuts."""
    from PIL import Image
    from mspi_amd import inference as I
    from mspi_amd.preproc import pil_bilinear_coeffs
    from oracle import restate as R
    rng = np.random.default_rng(0)
    for Hin, Win, Hout, Wout in ((48, 64, 32, 48), (100, 150, 224, 384), (333, 517, 96, 160)):
        img = rng.integers(0, 256, (Hin, Win, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).resize((Wout, Hout), Image.BILINEAR))
        hb, hk, _ = pil_bilinear_coeffs(Win, Wout)
        vb, vk, _ = pil_bilinear_coeffs(Hin, Hout)
        tmp = np.stack([np.clip(((img[:, x0:x0 + n].astype(np.int64) * hk[x, :n][None, :, None]).sum(1) + (1 << 21)) >> 22, 0, 255)
                        for x, (x0, n) in enumerate(hb)], 1)
        out = np.stack([np.clip(((tmp[y0:y0 + n] * vk[y, :n][:, None, None]).sum(0) + (1 << 21)) >> 22, 0, 255)
                        for y, (y0, n) in enumerate(vb)], 0)
        assert np.array_equal(out, ref)
        t = R.frame_transform(img, (Hout, Wout))
        assert tuple(t.shape) == (3, Hout, Wout) and -2.2 < t.min() < t.max() < 2.7
    wav = _make_dataset(str(tmp_path))
    wave = I._load_wav_16k(wav).reshape(-1)
    for first, rev in ((3, False), (3, True), (20, False)):
        st, ln = I.audio_segment(wave.numel(), first, "25")
        a = R.log_spectrogram_window(wave, st, ln, rev)
        assert torch.equal(a, I.get_audio_feature(wav, first, "25", mode=rev))
    assert I.audio_segment(16000, 100, 25) == (0, 0)                   # window past the end of the wave: "no audio"
    assert torch.equal(R.log_spectrogram_window(wave, 0, 0), torch.full((1, 257, 111), 0.02))


@pytest.mark.gpu
def test_gpu_preprocessing(dev, tmp_path):
    """frame resize + normalise (bit-exact to PIL / torchvision's ops) and the batched log-spectrogram
    kernel (vs the torch.stft oracle) on the GPU."""
    from PIL import Image
    from mspi_amd import inference as I
    from mspi_amd import preproc as P
    from mspi_amd._lib import MspiError
    from oracle import restate as R
    rng = np.random.default_rng(1)
    for Hin, Win, Hout, Wout in ((480, 640, 224, 384), (48, 64, 32, 48), (100, 150, 224, 384), (224, 384, 224, 384)):
        img = rng.integers(0, 256, (Hin, Win, 3), dtype=np.uint8)
        got = P.resize_normalize(torch.from_numpy(img).to(dev), (Hout, Wout), I.IMAGENET_DEFAULT_MEAN, I.IMAGENET_DEFAULT_STD).cpu()
        assert torch.equal(got, R.frame_transform(img, (Hout, Wout))), (Hin, Win, Hout, Wout)
    _make_dataset(str(tmp_path))
    I.device = dev
    I._RESOLUTION[:] = [32, 48]
    path = os.path.join(str(tmp_path), "video_frames", "TOY", "clip1", "img_00001.jpg")
    t, sz = I.torch_transform(path)
    assert t.is_cuda and sz == (64, 48)
    assert torch.equal(t.cpu(), R.frame_transform(np.asarray(Image.open(path).convert("RGB")), (32, 48)))
    # spectrogram windows: tone + noise, a chirp-free silent stretch, reversed windows, a short window (pads with 0.02)
    g = torch.Generator().manual_seed(0)
    n = 16000 * 3
    tt = torch.arange(n) / 16000.0
    wave = 0.3 * torch.sin(2 * math.pi * 440 * tt) + 0.05 * torch.randn(n, generator=g)
    wave[20000:24000] *= 1e-3
    segs = [(0, 21120, 0), (1234, 21120, 1), (16000, 21121, 0), (30000, 5000, 0), (40000, 8000, 1), (0, 0, 0), (47000, 300, 0)]
    out = P.log_spectrogram(wave.to(dev), segs, 111).cpu()
    assert tuple(out.shape) == (len(segs), 1, 257, 111)
    for b, (st, ln, rev) in enumerate(segs):
        ref = R.log_spectrogram_window(wave, st, ln, bool(rev))
        err = (out[b] - ref).abs().max().item()
        assert err < 2e-3, "window %d: max abs err %.3e" % (b, err)      # fp32 FFT (oracle) vs fp64-accumulated DFT
    with pytest.raises(MspiError, match="outside"):
        P.log_spectrogram(wave.to(dev), [(n - 100, 300, 0)])
    with pytest.raises(MspiError, match="reflect"):
        P.log_spectrogram(wave.to(dev), [(0, 200, 0)])


@pytest.mark.gpu
def test_postprocess_kernel(dev):
    from mspi_amd import engine as E
    from oracle import restate as R
    g = torch.Generator().manual_seed(1)
    maps = torch.randn(3, 224, 224, generator=g) * 2 - 9
    out = E.postprocess_u8(maps.to(dev), (480, 640)).cpu()
    for i in range(3):
        ref = R.postprocess_u8(maps[i], (480, 640))
        d = (out[i].int() - ref.int()).abs()
        assert d.max() <= 1 and (d > 0).float().mean() < 0.02      # rounding ties only
    assert torch.equal(out, E.postprocess_u8(maps.to(dev), (480, 640)).cpu())


@pytest.mark.gpu
def test_clip_loop_end_to_end(dev, tmp_path):
    """Synthetic dataset directory -> one grey map per frame, equal to oracle model + oracle post-process."""
    from PIL import Image
    from mspi_amd import inference as I
    from mspi_amd import testing as T
    from oracle import restate as R
    root = str(tmp_path / "data")
    _make_dataset(root)
    res = (64, 96)
    I.device = dev
    I._RESOLUTION[:] = list(res)
    torch.manual_seed(0)
    model = I.build_model("x3dl", res)
    T.randomize_(model.cpu(), 0)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev).eval()
    args = types.SimpleNamespace(clip_size=16, dataset="TOY", split=2, path_data=root, save_path=str(tmp_path / "out"),
                                 use_sound=True, batch=5)
    I.inference_dataset(model, args)
    outs = sorted(os.listdir(os.path.join(args.save_path, "clip1")))
    assert len(outs) == 34 and outs[0] == "img_00001.jpg"
    # frame 20 (window frames 5..20) against the oracle pipeline
    frames = [I.torch_transform(os.path.join(root, "video_frames", "TOY", "clip1", "img_%05d.jpg" % (i + 1)))[0] for i in range(4, 20)]
    clip = torch.stack(frames).permute(1, 0, 2, 3)[None].cpu()
    aud = I.get_audio_feature(os.path.join(root, "video_audio", "TOY", "clip1", "clip1.wav"), 4, "25")[None]
    cfg = model.cfg
    with torch.no_grad():
        ref, _ = R.audio_visual_forward(sd, clip, aud, "x3dl", cfg.MODEL.LATERAL_BOOL, cfg.MODEL.LATERAL_STRIDE)
    want = R.postprocess_u8(ref[0], (480, 640)).numpy().astype(int)
    # the file went through a JPEG encode: compare the device output before encoding instead
    from mspi_amd import engine as E
    got = E.postprocess_u8(model(clip.to(dev), aud.to(dev))[0], (480, 640))[0].cpu().numpy().astype(int)
    assert np.abs(got - want).max() <= 2
    img = np.asarray(Image.open(os.path.join(args.save_path, "clip1", "img_00020.jpg")))
    assert img.shape == (480, 640) and np.abs(img.astype(int) - want).mean() < 3.0


@pytest.mark.gpu
def test_frame_feature_cache(dev, tmp_path):
    """per-frame image-branch features cached across overlapping windows.  (a) forward with
    frame_feats == forward without, for two windows that share 15 frames and a time-reversed one; (b) the clip loop with
    the cache writes the same maps as the loop that re-encodes every window."""
    from PIL import Image
    from mspi_amd import inference as I
    from mspi_amd import testing as T
    root = str(tmp_path / "data")
    _make_dataset(root, n_frames=36)
    res = (64, 96)
    I.device = dev
    I._RESOLUTION[:] = list(res)
    model = I.build_model("x3dl", res)
    T.randomize_(model.cpu(), 0)
    model = model.to(dev).eval()
    frames = torch.stack([I.torch_transform(os.path.join(root, "video_frames", "TOY", "clip1", "img_%05d.jpg" % (i + 1)))[0]
                          for i in range(17)]).to(dev)                                        # [17,3,H,W]
    wav = os.path.join(root, "video_audio", "TOY", "clip1", "clip1.wav")
    idx = [list(range(0, 16)), list(range(1, 17)), list(range(15, -1, -1))]
    clips = torch.stack([frames[i].permute(1, 0, 2, 3) for i in idx])                         # [3,3,16,H,W]
    aud = torch.stack([I.get_audio_feature(wav, 0, "25"), I.get_audio_feature(wav, 1, "25"),
                       I.get_audio_feature(wav, 0, "25", mode=True)]).to(dev)
    f1, f0 = model.encode_frames(frames)
    flat = [j for w in idx for j in w]
    a = model(clips, aud)[0]
    b = model(clips, aud, frame_feats=(f1[flat], f0[flat]))[0]
    assert (a - b).abs().max().item() < 1e-5
    # the clip loop's runner returns u8 maps; the fp32 map in front of its post-processing, replayed from the runner's kind of
    # pipeline (hipGraphs of the cached-frames forward, two in flight), is the eager forward of the same windows bit for bit
    from mspi_amd.runtime import GraphPipeline
    ff = (f1[flat], f0[flat])
    b = b.clone()
    pipe = GraphPipeline(lambda c, s, g1, g0: model(c, s, frame_feats=(g1, g0))[0], (clips, aud) + ff, depth=2, layouts=1, watch=model)
    rev = (clips.flip(0), aud.flip(0)) + tuple(t.view(3, 16, *t.shape[1:]).flip(0).reshape(t.shape) for t in ff)      # windows in reverse order
    b_rev = model(rev[0], rev[1], frame_feats=rev[2:])[0].clone()
    tickets = [pipe.submit(clips, aud, *ff), pipe.submit(*rev)]
    assert torch.equal(pipe.fetch(tickets[0]), b) and torch.equal(pipe.fetch(tickets[1]), b_rev)
    assert not torch.equal(b, b_rev)
    pipe.drain()
    del pipe
    out = {}
    for tag, cache, graph in (("cached", True, True), ("plain", False, True), ("eager", True, False)):
        args = types.SimpleNamespace(clip_size=16, dataset="TOY", split=2, path_data=root, save_path=str(tmp_path / tag),
                                     use_sound=True, batch=4, cache_frames=cache, graph=graph)
        I.inference_dataset(model, args)
        names = sorted(os.listdir(os.path.join(args.save_path, "clip1")))
        assert len(names) == 36
        out[tag] = np.stack([np.asarray(Image.open(os.path.join(args.save_path, "clip1", n))).astype(int) for n in names])
    # the two loops batch the image branch differently (16-frame chunks vs whole windows), so a map value can round to the
    # neighbouring grey level; the files went through a JPEG encode, which can turn that one level into two on a few pixels
    d = np.abs(out["cached"] - out["plain"])
    assert d.max() <= 2 and (d > 1).mean() < 1e-3
    # hipGraph replay (runtime.GraphPipeline, two batches in flight, padded last batch) == eager launches, file for file
    assert np.array_equal(out["cached"], out["eager"])
