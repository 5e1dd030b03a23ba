"""float64 restatement of oracle.restate.log_spectrogram_window (inference.py:41-58 upstream): the wave promoted to
float64, a float64 periodic Hann window, torch.stft in float64, log(p + 1e-6), per-column standardisation with the
unbiased std, crop / pad with 0.02.  It also returns the per-column std, which says where the standardisation divides
by (almost) nothing.  `make_wave` and `WINDOWS` are the inputs tests/test_logspec_kernel.py and its CPU pins share.
It is not imported by mspi_amd."""
import math

import torch

PAD = 0.02
SR = 16000
N_WAVE = 3 * SR
ATTENUATED = (12000, 16000)          # scaled by 1e-3
SILENCE = (30000, 32400)             # exact zeros

# (start, length, reversed).  nframes = 1 + length // 160.
WINDOWS = (
    (100, 257, 0),                   # the smallest legal window: 2 frames, both reflect at both ends
    (5000, 319, 0),                  # 2 frames
    (5000, 320, 0),                  # 3 frames: the last one is centred on the sample after the window
    (5000, 321, 0),                  # 3 frames
    (7001, 1599, 0),                 # 10 frames
    (7001, 1600, 0),                 # 11 frames
    (7001, 1601, 1),                 # 11 frames, reversed
    (0, 17599, 0),                   # 110 frames: one pad column at Wa = 111
    (0, 0, 0),                       # no audio: every column is padding
    (1000, 17600, 0),                # exactly 111 frames
    (2000, 17760, 1),                # 112 frames: cropped at Wa = 111
    (N_WAVE - 3000, 3000, 0),        # ends on the last sample of the wave
    (12345, 2001, 0),                # odd start, inside the attenuated stretch
    (12345, 2001, 1),                # its reversed twin
    (30200, 1600, 0),                # inside the silence: every frame is exact zeros
    (28896, 2881, 0),                # straddles the start of the silence: frames 9 .. 18 are exact zeros, frame 8 keeps
                                     # 80 samples of signal under the window's rising edge (weights up to 0.22)
)
SILENT_WINDOWS = (14, 15)
WAS = (111, 37, 300)


def make_wave():
    """float32 [48000]: a 440 Hz tone plus noise, one stretch attenuated by 1e-3, one stretch of exact zeros."""
    g = torch.Generator().manual_seed(0)
    tt = torch.arange(N_WAVE) / float(SR)
    wave = 0.3 * torch.sin(2 * math.pi * 440 * tt) + 0.05 * torch.randn(N_WAVE, generator=g)
    wave[ATTENUATED[0]:ATTENUATED[1]] *= 1e-3
    wave[SILENCE[0]:SILENCE[1]] = 0.0
    return wave


def log_spectrogram_window(wave, start, length, reverse=False, Wa=111):
    """(out float64 [1,257,Wa], std float64 [Wa]); std is NaN on the pad columns."""
    out = torch.full((1, 257, Wa), PAD, dtype=torch.float64)
    std = torch.full((Wa,), float("nan"), dtype=torch.float64)
    if length == 0:
        return out, std
    a = wave[start:start + length][None].double()
    if reverse:
        a = torch.flip(a, [1])
    spec = torch.stft(a, n_fft=512, hop_length=160, win_length=512, window=torch.hann_window(512, dtype=torch.float64),
                      center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    a = torch.log(spec.abs().pow(2.0) + 1e-6)
    sd = a.std(dim=1, keepdim=True)
    a = (a - a.mean(dim=1, keepdim=True)) / (sd + 1e-6)
    n = min(a.shape[-1], Wa)
    out[:, :, :n] = a[:, :, :n]
    std[:n] = sd[0, 0, :n]
    return out, std
