"""python -m mspi_amd.validate: the CLI surface without a GPU, and on the GPU validate() against
metrics.validation_one_epoch fed by a loader that the test builds from the per-frame functions."""
import os
import types

import numpy as np
import pytest
import torch

from test_clip_loader import MEAN, STD, _make_tree


def test_cli_parses_and_refuses_what_it_cannot_do(monkeypatch, tmp_path):
    from mspi_amd import validate as V
    from mspi_amd._lib import MspiError
    a = V.build_parser().parse_args([])
    assert (a.dataset, a.split, a.mode, a.clip_size, a.batch, a.use_sound, a.fixations, a.resolution) == \
        ("AVAD", 2, "val", 16, 8, True, False, [224, 384])
    a = V.build_parser().parse_args("--weight w.pt --path_data /d --dataset DIEM --split 1 --mode test --model x3dl --resolution 64 96 "
                                    "--clip_size 8 --batch 3 --no_sound --fixations".split())
    assert (a.weight, a.path_data, a.dataset, a.split, a.mode, a.model) == ("w.pt", "/d", "DIEM", 1, "test", "x3dl")
    assert (a.resolution, a.clip_size, a.batch, a.use_sound, a.fixations) == ([64, 96], 8, 3, False, True)
    with pytest.raises(SystemExit):
        V.build_parser().parse_args(["--mode", "train"])
    assert V.format_line({"kld": 1.23456, "cc": 0.5, "sim": 0.25, "loss": 0.73456}) == "* Kldiv 1.2346 CC 0.5000 SIM 0.2500 loss 0.7346"
    root = _make_tree(str(tmp_path / "d"), [("va", 9, (12, 16))], frames=False, audio=False)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(MspiError, match="WORLD_SIZE"):
        V.validate(torch.nn.Identity(), root, "TOY", 2, clip_size=4, device="cuda")
    with pytest.raises(MspiError, match="WORLD_SIZE"):
        V.main(["--path_data", root, "--dataset", "TOY"])
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(MspiError, match="GPU"):
        V.validate(torch.nn.Identity(), root, "TOY", 2, clip_size=4, device="cpu")


def _per_frame_loader(root, dataset, clip_list, T, size, fps, dev, batch, use_sound, fixations):
    """The batches validate() has to reproduce, built from the per-frame functions: resize_normalize per frame + stack +
    permute, one log_spectrogram launch per clip, resize_maps / resize_fixations per sample."""
    from PIL import Image
    from mspi_amd import evaluate as EV
    from mspi_amd import inference as I
    from mspi_amd import preproc as P
    out = []
    for i in range(0, len(clip_list), batch):
        clips, auds, labs, fixs = [], [], [], []
        for v, start in clip_list[i:i + batch]:
            frames = []
            for j in range(T):
                img = np.asarray(Image.open(os.path.join(root, "video_frames", dataset, v, "img_%05d.jpg" % (start + j + 1))).convert("RGB"))
                frames.append(P.resize_normalize(torch.from_numpy(img.copy()).to(dev), size, MEAN, STD))
            clips.append(torch.stack(frames).permute(1, 0, 2, 3))
            ann = os.path.join(root, "annotations", dataset, v)
            lab = EV.resize_maps(torch.from_numpy(EV.load_gray(os.path.join(ann, "maps", "eyeMap_%05d.jpg" % (start + T))))[None].to(dev), size)[0]
            labs.append(lab / 255.0 if lab.max() > 1.0 else lab)
            fix = EV.load_fixation(os.path.join(ann, "fixMap_%05d.mat" % (start + T)))
            fixs.append(EV.resize_fixations(torch.from_numpy(fix)[None].to(dev).float(), size)[0])
            wave = I._load_wav_16k(os.path.join(root, "video_audio", dataset, v, v + ".wav")).reshape(-1).to(dev)
            auds.append(P.log_spectrogram(wave, [I.audio_segment(wave.numel(), start, fps, len_snippet=T) + (0,)], 111)[0])
        b = [torch.stack(clips)] + ([torch.stack(auds)] if use_sound else []) + [torch.stack(labs)]
        out.append(tuple(b + ([torch.stack(fixs)] if fixations else [])))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("use_sound,fixations", [(True, False), (False, False), (True, True)])
def test_validate_equals_validation_one_epoch_on_per_frame_batches(dev, tmp_path, use_sound, fixations):
    """Seeded x3dl at 64 x 64 as in the av_x3dl_64 golden, autotune off: the dataset's batches are bit-equal to the per-frame
    ones and the launches are the same, so the numbers are required to be EQUAL."""
    from mspi_amd import engine as E
    from mspi_amd import metrics as M
    from mspi_amd import testing as T
    from mspi_amd import validate as V
    from mspi_amd.model import model_utils as pm
    E.autotune(False)
    size, Tc = (64, 64), 16
    videos = [("va", 49, (48, 64)), ("vb", 17, (37, 53))]
    root = _make_tree(str(tmp_path / "d"), videos)
    clip_list = [("va", 0), ("va", 32), ("vb", 0)]
    cfg = T.make_cfg("x3dl", num_aud_tokens=36, num_vis_tokens=16 * 2 * 2)
    cls = pm.AudioVisualSaliencyModel if use_sound else pm.VisualSaliencyModel
    model = T.seeded(lambda: cls(cfg), 0).to(dev)
    torch.manual_seed(11)                 # AUC-Judd's jitter noise comes from the device's default generator
    got = V.validate(model, root, "TOY", 2, "val", size, Tc, batch=2, use_sound=use_sound, fixations=fixations, workers=4, device=dev)
    loader = _per_frame_loader(root, "TOY", clip_list, Tc, size, "25", dev, 2, use_sound, fixations)
    torch.manual_seed(11)
    want = M.validation_one_epoch(model, loader, dev, types.SimpleNamespace(DATA=types.SimpleNamespace(USE_SOUND=use_sound)))
    print("validate:", got, "per-frame:", want)
    assert set(got) == set(want) and {"loss", "kld", "cc", "sim"} <= set(got)
    assert ("nss" in got and "auc_j" in got) == fixations
    for k in want:
        assert np.isfinite(got[k]) and got[k] == want[k], (k, got[k], want[k])
