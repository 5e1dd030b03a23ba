"""logspec_kernel (csrc/preproc.hip, behind preproc.log_spectrogram) against float64.

Yardstick: tests/logspec_restate.py, oracle.restate.log_spectrogram_window with the wave and the Hann window in float64.
Wave and windows: logspec_restate.make_wave / WINDOWS -- three seconds of tone plus noise with an attenuated stretch and a
stretch of exact zeros; the smallest legal window, lengths either side of a multiple of the hop, 110 / 111 / 112 frames
(one pad column, none, cropped at Wa = 111), a window ending on the wave's last sample, an odd start and its reversed
twin, an empty window in the middle of the list, one window inside the zeros and one across their start.  One launch
over the whole list, at Wa = 111, 37 and 300, into a NaN-filled larger buffer.

Bar: max |kernel - float64| <= BAR = 2.6e-4.  It is measured, not chosen: twice the worst distance of the float32
torch.stft oracle (oracle.restate.log_spectrogram_window) to the float64 restatement over this same window list, which
was 1.27e-4 (window 9, the 111-frame one; the others 4e-6 .. 8e-5) when this module was written, rounded up to two
digits.  The kernel accumulates its DFT in float64 and has no reason to do worse than a float32 FFT; the factor 2 covers
logf and the reduction order.  A CPU test recomputes the oracle's distance and asserts it is still at most BAR / 2.
That pin has little room (1.27e-4 against 1.3e-4 here; the same oracle sat at 9.6e-5 on another CPU): a float32 FFT's
rounding can move with the torch or FFT-library build.  If it fails with nothing changed in this project, the cure is to
measure the oracle's distance again over the same windows and set BAR to twice that, in this docstring and the
constant together -- never to raise BAR because the kernel misses it.

Columns whose float64 std is below 1e-3 are left out of the toleranced comparison.  They occur only in the two windows
over the zeros, where all 257 log(0 + 1e-6) values of a column are bit-equal and their float64 std is exactly 0
(asserted on the CPU).  The value of the formula there is exactly 0.0, and that is what the kernel must return; the
float32 oracle returns rounding noise of up to 2.9 on those columns.  The kernel forms its mean as sum / 257, which
need not give the common value back in general; for the one value digital silence produces, logf(1e-6f), summed in the
kernel's fixed order, it does, and all 21 silent columns came out as exact zeros on an MI355X at every Wa when this
module was written (kernel 1.0e-4, float32 oracle 9.6e-5 from float64 on the other columns).  Pad columns are exactly
0.02."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import logspec_restate as LS
from oracle import restate as R

BAR = 2.6e-4
LOW_STD = 1e-3
GUARD = 1024          # floats on either side of the output


@functools.lru_cache(maxsize=None)
def _wave():
    return LS.make_wave()


@functools.lru_cache(maxsize=None)
def _reference(Wa):
    """(float64 [B,1,257,Wa], std [B,Wa]) of the whole window list, computed once per Wa."""
    pairs = [LS.log_spectrogram_window(_wave(), st, ln, bool(rev), Wa) for st, ln, rev in LS.WINDOWS]
    return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


def _nframes(length, Wa):
    return min(Wa, 1 + length // 160) if length else 0


# ------------------------------------------------------------------------------------------------------------- CPU
def test_wave_and_windows_hold_the_named_edges():
    wave = _wave()
    assert wave.dtype == torch.float32 and wave.numel() == LS.N_WAVE == 48000
    z0, z1 = LS.SILENCE
    assert z1 - z0 >= 2000 and (wave[z0:z1] == 0).all() and wave[z0 - 1] != 0 and wave[z1] != 0
    a0, a1 = LS.ATTENUATED
    assert wave[a0:a1].abs().max() < 1e-3 < 0.1 < wave[:a0].abs().max()
    lens = [w[1] for w in LS.WINDOWS]
    assert min(ln for ln in lens if ln) == 257 and {319, 320, 321, 1599, 1600, 1601, 17599, 17600, 17760} <= set(lens)
    assert [1 + ln // 160 for ln in (17599, 17600, 17760)] == [110, 111, 112]
    assert any(st + ln == wave.numel() for st, ln, _ in LS.WINDOWS) and any(st % 2 and ln for st, ln, _ in LS.WINDOWS)
    assert any((st, ln, 1 - rev) in LS.WINDOWS for st, ln, rev in LS.WINDOWS if rev)
    assert (0, 0, 0) in LS.WINDOWS[1:-1]
    inside, across = (LS.WINDOWS[i] for i in LS.SILENT_WINDOWS)
    assert z0 <= inside[0] and inside[0] + inside[1] <= z1
    assert across[0] < z0 < across[0] + across[1] <= z1
    assert all(0 <= st and st + ln <= wave.numel() and (ln == 0 or ln > 256) for st, ln, _ in LS.WINDOWS)


def test_restatement_follows_the_float32_oracle_within_half_the_bar():
    """The measurement behind BAR, repeated: the float32 oracle's worst distance to float64 over the window list."""
    worst = 0.0
    for Wa in LS.WAS:
        ref, std = _reference(Wa)
        for i, (st, ln, rev) in enumerate(LS.WINDOWS):
            ora = R.log_spectrogram_window(_wave(), st, ln, bool(rev), Wa)
            keep = ~(std[i] < LOW_STD)
            d = (ora.double() - ref[i])[:, :, keep].abs().max().item()
            if Wa == LS.WAS[0]:
                print("window %2d %-18s float32 oracle within %.2e of float64" % (i, (st, ln, rev), d))
            worst = max(worst, d)
            n = _nframes(ln, Wa)
            assert torch.equal(ref[i][:, :, n:], torch.full((1, 257, Wa - n), LS.PAD, dtype=torch.float64))
            assert torch.isnan(std[i, n:]).all() and not torch.isnan(std[i, :n]).any()
    print("worst %.3e; BAR = %.1e" % (worst, BAR))
    assert worst <= BAR / 2


def test_low_std_columns_are_the_silent_frames_only():
    """float64 std < 1e-3 happens only in the two windows over the zeros, only on frames whose 512 samples are all
    zero, and is then exactly 0 with a value of exactly 0; every other column has a std of at least 0.5."""
    ref, std = _reference(300)
    z0, z1 = LS.SILENCE
    for i, (st, ln, rev) in enumerate(LS.WINDOWS):
        low = (std[i] < LOW_STD).nonzero().flatten().tolist()
        if i not in LS.SILENT_WINDOWS:
            assert low == []
            continue
        silent = []
        for f in range(1 + ln // 160):
            j = (torch.arange(512) + f * 160 - 256).abs()                            # centre + reflect padding
            j = torch.where(j >= ln, 2 * (ln - 1) - j, j)
            if (_wave()[st + j] == 0).all():
                silent.append(f)
        assert low == silent and len(low) >= 10
        assert (std[i, low] == 0).all() and (ref[i][:, :, low] == 0).all()
    ok = std[~torch.isnan(std) & ~(std < LOW_STD)]
    assert ok.min().item() >= 0.5


# ------------------------------------------------------------------------------------------------------------- GPU
def _launch(dev, Wa):
    """One raw mspi_logspec_fwd over the whole list into the middle of a NaN-filled buffer; (out [B,1,257,Wa], buffer)."""
    from mspi_amd import _lib
    lib = _lib.load()
    wave = _wave().to(dev)
    seg_host = np.ascontiguousarray(np.asarray(LS.WINDOWS, dtype=np.int32))
    seg = torch.from_numpy(seg_host).to(dev)
    B = seg_host.shape[0]
    win = torch.hann_window(512, dtype=torch.float32).to(dev)
    n = B * 257 * Wa
    buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    rc = lib.mspi_logspec_fwd(wave.data_ptr(), wave.numel(), seg.data_ptr(), seg_host.ctypes.data, B, win.data_ptr(),
                              buf.data_ptr() + 4 * GUARD, Wa, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mspi_last_error()
    torch.cuda.synchronize()
    return buf[GUARD:GUARD + n].view(B, 1, 257, Wa), buf


@pytest.mark.gpu
@pytest.mark.parametrize("Wa", LS.WAS)
def test_hip_logspec_vs_float64(dev, Wa):
    from mspi_amd import preproc as P
    out, buf = _launch(dev, Wa)
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all()
    assert not torch.isnan(out).any()
    out2, _ = _launch(dev, Wa)
    assert torch.equal(out, out2)                                                    # bitwise repeatable
    assert torch.equal(out, P.log_spectrogram(_wave().to(dev), list(LS.WINDOWS), Wa))
    out = out.cpu()
    ref, std = _reference(Wa)
    pad = torch.tensor(LS.PAD, dtype=torch.float32)
    failures = []
    for i, (st, ln, rev) in enumerate(LS.WINDOWS):
        n = _nframes(ln, Wa)
        assert (out[i][:, :, n:] == pad).all(), "window %d: pad columns" % i
        low = std[i] < LOW_STD
        keep = ~low & ~torch.isnan(std[i])
        err = (out[i].double() - ref[i])[:, :, keep].abs().max().item() if keep.any() else 0.0
        ora = R.log_spectrogram_window(_wave(), st, ln, bool(rev), Wa)
        e32 = (ora.double() - ref[i])[:, :, keep].abs().max().item() if keep.any() else 0.0
        silent = out[i][:, :, low].abs().max().item() if low.any() else 0.0
        print("Wa %3d window %2d %-18s kernel %.2e, float32 oracle %.2e%s" % (
            Wa, i, (st, ln, rev), err, e32, ", %d silent columns: max |kernel| %.3g" % (int(low.sum()), silent) if low.any() else ""))
        if err > BAR:
            failures.append("window %d: max abs err %.3e" % (i, err))
        if low.any() and not (out[i][:, :, low] == 0).all():
            failures.append("window %d: up to %.3g on silent columns, where the formula's value is exactly 0" % (i, silent))
    assert not failures, failures
