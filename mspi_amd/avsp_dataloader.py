"""The dataset of the reference's avsp_dataloader.py:83-193 (AudioVisualDataset) for validation on the MI355X.

Same constructor arguments, same files under data_root (fold_lists/, video_frames/, annotations/<dataset>/<video>/maps,
video_audio/), same clip list.  What differs: iterating it yields BATCHES THAT ARE ALREADY ON THE DEVICE, not samples for
a DataLoader to collate --

  * frames img_%05d.jpg are decoded with PIL on a small pool of host threads (one batch ahead of the consumer), uploaded as
    uint8 -- or, with device_decode=True, only read by the pool and decoded on the device (`preproc.decode_frames`, the same
    pixels; files the device does not take fall back to PIL) --, grouped by source size and written into the [B,3,T,H,W]
    clip tensor by one `preproc.assemble_clips` launch per
    size group (PIL's resize + ToTensor + Normalize, bit for bit);
  * the label eyeMap_%05d.jpg is resized on the device (`evaluate.resize_maps`, cv2.resize upstream) and divided by 255
    where its maximum exceeds 1 (:176-182);
  * the fixation map is resized with `evaluate.resize_fixations` to `size` -- upstream resizes it to a hard-coded
    224 x 384 (:186) whatever `size` is, and then does not return it; here it follows `size` and is appended to the batch
    with with_fixations=True, which is what metrics.validation_one_epoch scores NSS / AUC-Judd from;
  * the wav is read and resampled once per video and its windows (`inference.audio_segment(..., len_snippet=len_clip)`:
    upstream's dataset cuts len_clip + 1 frames of audio, unlike its inference.py) are one `preproc.log_spectrogram`
    launch per batch per video;
  * train mode draws its start frames from a numpy Generator handed in, not from numpy's global state.

A batch is (clips, audio, label) with sound and (clips, label) without, plus the fixations when asked for.  A missing frame
or annotation raises FileNotFoundError naming the file.  There is no CPU fallback."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import evaluate as EV
from . import preproc
from ._lib import MspiError

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


def load_rgb(path):
    """uint8 [H,W,3]: the frame as upstream reads it (PIL, convert('RGB'))."""
    from PIL import Image
    if not os.path.exists(path):
        raise FileNotFoundError("avsp_dataloader: missing frame %s" % path)
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def read_frame(path):
    """The bytes of a frame file (device_decode: the frame is decoded on the device)."""
    if not os.path.exists(path):
        raise FileNotFoundError("avsp_dataloader: missing frame %s" % path)
    with open(path, "rb") as f:
        return f.read()


def _gray(path):
    if not os.path.exists(path):
        raise FileNotFoundError("avsp_dataloader: missing annotation %s" % path)
    return EV.load_gray(path)


def _fixation(root, no):
    path = os.path.join(root, "fixMap_%05d.mat" % no)
    if not os.path.exists(path):
        png = path[:-4] + ".png"
        if not os.path.exists(png):
            raise FileNotFoundError("avsp_dataloader: missing annotation %s (or .png)" % path)
        path = png
    return EV.load_fixation(path)


class AudioVisualDataset:
    def __init__(self, data_root, dataset_name="DIEM", split=1, len_clip=32, mode="train", use_sound=True, size=(224, 224),
                 batch_size=8, with_fixations=False, generator=None, workers=8, device=None, device_decode=False):
        if mode not in ("train", "val", "test"):
            raise MspiError("avsp_dataloader: mode must be train, val or test, got %r" % (mode,))
        self.path_data, self.dataset_name, self.mode = data_root, dataset_name, mode
        self.use_sound, self.len_snippet, self.size = use_sound, int(len_clip), (int(size[0]), int(size[1]))
        self.batch_size, self.with_fixations = max(1, int(batch_size)), with_fixations
        self.generator, self.workers, self.device = generator, max(1, int(workers)), device
        self.device_decode = bool(device_decode)
        if dataset_name == "DIEM":
            file_name = "DIEM_list_{}_fps.txt".format(mode)
        else:
            file_name = "{}_list_{}_{}_fps.txt".format(dataset_name, mode, split)
        self.videos_fps, self.videos_frame_num, self.list_indata = {}, {}, []
        with open(os.path.join(data_root, "fold_lists", file_name), "r") as f:
            for line in f.readlines():
                if not line.strip():
                    continue
                name, frame_num, fps = line.split(" ")
                self.list_indata.append(name)
                self.videos_frame_num[name] = frame_num
                self.videos_fps[name] = fps
        self.list_indata.sort()
        n_maps = [len(os.listdir(self._maps(v))) for v in self.list_indata]
        if mode == "train":
            self.list_num_frame = n_maps
        else:
            self.list_num_frame = []
            for v, n in zip(self.list_indata, n_maps):
                for i in range(0, n - self.len_snippet, 2 * self.len_snippet):
                    if self.check_frame(os.path.join(self._maps(v), "eyeMap_%05d.jpg" % (i + self.len_snippet))):
                        self.list_num_frame.append((v, i))
        self._waves = {}

    def _maps(self, video):
        return os.path.join(self.path_data, "annotations", self.dataset_name, video, "maps")

    def check_frame(self, path):
        return _gray(path).max() != 0

    def __len__(self):
        return len(self.list_num_frame)

    def clip_list(self):
        """[(video, start frame)] of one pass.  val / test: the fixed list.  train: one start per video, drawn from the
        generator and drawn again until the label of its clip is not all zero (:147-154)."""
        if self.mode != "train":
            return list(self.list_num_frame)
        if not isinstance(self.generator, np.random.Generator):
            raise MspiError("avsp_dataloader: train mode draws its start frames from a numpy.random.Generator; pass generator=")
        out = []
        for v, n in zip(self.list_indata, self.list_num_frame):
            if n - self.len_snippet + 1 <= 0:
                raise ValueError("avsp_dataloader: %s has %d annotated frames, fewer than a clip of %d" % (v, n, self.len_snippet))
            while True:
                start = int(self.generator.integers(0, n - self.len_snippet + 1))
                if self.check_frame(os.path.join(self._maps(v), "eyeMap_%05d.jpg" % (start + self.len_snippet))):
                    break
            out.append((v, start))
        return out

    # ------------------------------------------------------------------------------------------------ host side
    def _submit(self, pool, items):
        T = self.len_snippet
        frames, labels, fixes = [], [], []
        for v, start in items:
            clip_dir = os.path.join(self.path_data, "video_frames", self.dataset_name, v)
            frames += [pool.submit(read_frame if self.device_decode else load_rgb,
                                   os.path.join(clip_dir, "img_%05d.jpg" % (start + i + 1))) for i in range(T)]
            labels.append(pool.submit(_gray, os.path.join(self._maps(v), "eyeMap_%05d.jpg" % (start + T))))
            if self.with_fixations:
                fixes.append(pool.submit(_fixation, os.path.join(self.path_data, "annotations", self.dataset_name, v), start + T))
        return items, frames, labels, fixes

    # ------------------------------------------------------------------------------------------------ device side
    def _by_shape(self, arrays, device):
        """[(indices, uint8 CUDA tensor [n, ...])] of the arrays grouped by shape, in order of first appearance."""
        groups = {}
        for i, a in enumerate(arrays):
            groups.setdefault(a.shape, []).append(i)
        return [(idx, torch.from_numpy(np.stack([arrays[i] for i in idx])).to(device)) for idx in groups.values()]

    def _frames_by_shape(self, frames, device):
        """_by_shape of the batch's frames; with device_decode they arrive as file bytes and are decoded on the device."""
        if not self.device_decode:
            return self._by_shape(frames, device)
        groups = {}
        for i, t in enumerate(preproc.decode_frames(frames, device)):
            groups.setdefault(tuple(t.shape), []).append((i, t))
        return [([i for i, _ in g], torch.stack([t for _, t in g])) for g in groups.values()]

    def _wave(self, video, device):
        if video not in self._waves:
            from . import inference as I
            path = os.path.join(self.path_data, "video_audio", self.dataset_name, video, video + ".wav")
            if len(self._waves) >= 2:
                self._waves.clear()
            self._waves[video] = I._load_wav_16k(path).reshape(-1).to(device) if os.path.exists(path) else None
        return self._waves[video]

    def _audio(self, items, device):
        from . import inference as I
        out = torch.empty(len(items), 1, 257, 111, dtype=torch.float32, device=device)
        by_video = {}
        for b, (v, start) in enumerate(items):
            by_video.setdefault(v, []).append((b, start))
        for v, rows in by_video.items():
            wave = self._wave(v, device)
            idx = torch.tensor([b for b, _ in rows], device=device)
            if wave is None:                  # no wav file: the constant upstream feeds (:78-79)
                out[idx] = 0.02
                continue
            segs = [I.audio_segment(wave.numel(), start, self.videos_fps[v], len_snippet=self.len_snippet) + (0,) for _, start in rows]
            out[idx] = preproc.log_spectrogram(wave, segs, 111)
        return out

    def _assemble(self, job, device):
        items, frames, labels, fixes = job
        frames = [f.result() for f in frames]
        B, T = len(items), self.len_snippet
        clips = torch.empty(B, 3, T, self.size[0], self.size[1], dtype=torch.float32, device=device)
        for idx, dev_frames in self._frames_by_shape(frames, device):
            preproc.assemble_clips(dev_frames, idx, clips, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
        label = torch.empty(B, self.size[0], self.size[1], dtype=torch.float32, device=device)
        for idx, maps in self._by_shape([f.result() for f in labels], device):
            gt = EV.resize_maps(maps, self.size)
            gt = torch.where(gt.amax((1, 2), keepdim=True) > 1.0, gt / 255.0, gt)
            label[torch.tensor(idx, device=device)] = gt
        batch = [clips] + ([self._audio(items, device)] if self.use_sound else []) + [label]
        if self.with_fixations:
            fix = torch.empty_like(label)
            for idx, maps in self._by_shape([f.result() for f in fixes], device):
                fix[torch.tensor(idx, device=device)] = EV.resize_fixations(maps.float(), self.size)
            batch.append(fix)
        return tuple(batch)

    def __iter__(self):
        device = EV._device(self.device)
        todo = self.clip_list()
        chunks = [todo[i:i + self.batch_size] for i in range(0, len(todo), self.batch_size)]
        if not chunks:
            return
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            job = self._submit(pool, chunks[0])
            for nxt in chunks[1:] + [None]:
                ahead = self._submit(pool, nxt) if nxt is not None else None      # the pool decodes one batch ahead
                yield self._assemble(job, device)
                job = ahead
