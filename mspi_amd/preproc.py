"""Clip-loop pre-processing on the GPU: log-spectrogram windows and frame
resize + normalise through the C ABI (csrc/preproc.hip).  Host code here only builds small tables."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import MspiError, check

PRECISION_BITS = 32 - 8 - 2          # PIL's fixed point for 8-bit resampling


def pil_bilinear_coeffs(in_size, out_size):
    """PIL's precompute_coeffs (bilinear, support 1 scaled by the shrink factor = antialiasing) followed by
    normalize_coeffs_8bpc: (bounds int32 [out][2] = (first input index, taps), kk int32 [out][ksize], ksize)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = np.zeros(xmax, np.float64)
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            k[x] = 1.0 - t if t < 1.0 else 0.0
        ww = k.sum()
        if ww != 0.0:
            k = k / ww
        bounds[xx] = (xmin, xmax)
        kk[xx, :xmax] = [int(v * (1 << PRECISION_BITS) + (0.5 if v >= 0 else -0.5)) for v in k]
    return bounds, kk, ksize


_COEFFS = {}


def _coeffs(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    if key not in _COEFFS:
        b, k, ks = pil_bilinear_coeffs(in_size, out_size)
        _COEFFS[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), ks)
    return _COEFFS[key]


def resize_normalize(rgb_u8, out_hw, mean, std, out=None):
    """rgb_u8: uint8 [Hin, Win, 3] on the GPU -> fp32 [3, Hout, Wout]: PIL bilinear resize (bit-exact), /255, -mean, /std."""
    lib = _lib.load()
    if not rgb_u8.is_cuda:
        raise MspiError("resize_normalize runs on the GPU only (tensor on %s)" % rgb_u8.device)
    assert rgb_u8.dtype == torch.uint8 and rgb_u8.dim() == 3 and rgb_u8.shape[2] == 3 and rgb_u8.is_contiguous()
    Hin, Win = rgb_u8.shape[:2]
    Hout, Wout = out_hw
    dev = rgb_u8.device
    hb, hk, hks = _coeffs(Win, Wout, dev)
    vb, vk, vks = _coeffs(Hin, Hout, dev)
    tmp = torch.empty(Hin * Wout * 3, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(3, Hout, Wout, dtype=torch.float32, device=dev)
    assert out.shape == (3, Hout, Wout) and out.stride(2) == 1 and out.stride(1) == Wout
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    check(lib.mspi_resize_norm_fwd(rgb_u8.data_ptr(), Hin, Win, tmp.data_ptr(), out.data_ptr(), out.stride(0), Hout, Wout,
                                   hb.data_ptr(), hk.data_ptr(), hks, vb.data_ptr(), vk.data_ptr(), vks, m, s,
                                   torch.cuda.current_stream().cuda_stream), "mspi_resize_norm_fwd")
    return out


_WINDOW = {}


def log_spectrogram(wave, segments, Wa=111):
    """wave: fp32 [n] 16 kHz mono on the GPU; segments: list of (start, length, reversed) -> [B, 1, 257, Wa] standardised
    log-spectrogram windows (inference.py:24-63 upstream), padded with 0.02."""
    lib = _lib.load()
    if not wave.is_cuda:
        raise MspiError("log_spectrogram runs on the GPU only (tensor on %s)" % wave.device)
    wave = wave.reshape(-1).contiguous()
    seg_host = np.ascontiguousarray(np.asarray(segments, dtype=np.int32).reshape(-1, 3))
    B = seg_host.shape[0]
    dev = wave.device
    if str(dev) not in _WINDOW:
        _WINDOW[str(dev)] = torch.hann_window(512, dtype=torch.float32).to(dev)
    seg = torch.from_numpy(seg_host).to(dev)
    out = torch.empty(B, 1, 257, Wa, dtype=torch.float32, device=dev)
    check(lib.mspi_logspec_fwd(wave.data_ptr(), wave.numel(), seg.data_ptr(), seg_host.ctypes.data, B, _WINDOW[str(dev)].data_ptr(),
                               out.data_ptr(), Wa, torch.cuda.current_stream().cuda_stream), "mspi_logspec_fwd")
    return out


_COEFFS_HOST = {}


def _coeffs_host(in_size, out_size):
    key = (in_size, out_size)
    if key not in _COEFFS_HOST:
        b, _, ks = pil_bilinear_coeffs(in_size, out_size)
        _COEFFS_HOST[key] = (np.ascontiguousarray(b), ks)
    return _COEFFS_HOST[key]


def clip_tile_plan(Hin, Win, Hout, Wout):
    """What one workgroup of mspi_clip_resize_norm_fwd stages for frames Hin x Win -> Hout x Wout, planned on the host from
    the vertical bounds table: {"tile_rows", "staged_rows", "batch_rows", "lds_bytes"}, or None where no tile fits the LDS
    budget (extreme shrink factors, very wide frames).  No GPU call."""
    lib = _lib.load()
    vb, vks = _coeffs_host(Hin, Hout)
    plan = (C.c_int32 * 4)()
    if lib.mspi_clip_resize_plan(vb.ctypes.data, Hin, Win, Hout, Wout, vks, plan) != 0:
        return None
    return {"tile_rows": plan[0], "staged_rows": plan[1], "batch_rows": plan[2], "lds_bytes": plan[3]}


def assemble_clips(frames_u8, slots, out, mean, std, slots_dev=None):
    """frames_u8: uint8 [N, Hin, Win, 3] on the GPU (N decoded frames of one source size); out: fp32 [B, 3, T, Hout, Wout]
    on the GPU; slots: N integers, frame i is written to out[b, :, t] with b * T + t = slots[i].  Each frame gets
    resize_normalize's result (PIL bilinear resize bit for bit, /255, -mean, /std) straight in its slot: one launch for
    the N frames, no temporary.  Slots that are not named keep what they held.  slots_dev: the same table as an int32 CUDA
    tensor, for callers that may not allocate (graph capture); built here otherwise.  Where no tile of the batched kernel
    fits (clip_tile_plan() is None) the frames go through resize_normalize one by one.  Returns out."""
    lib = _lib.load()
    if not (frames_u8.is_cuda and out.is_cuda):
        raise MspiError("assemble_clips runs on the GPU only (tensors on %s, %s)" % (frames_u8.device, out.device))
    assert frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[3] == 3 and frames_u8.is_contiguous()
    assert out.dtype == torch.float32 and out.dim() == 5 and out.shape[1] == 3 and out.stride(4) == 1
    N, Hin, Win = frames_u8.shape[:3]
    B, _, T, Hout, Wout = out.shape
    slots_host = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
    if slots_host.shape[0] != N:
        raise MspiError("assemble_clips: %d slots for %d frames" % (slots_host.shape[0], N))
    dev = frames_u8.device
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    if N > 0 and clip_tile_plan(Hin, Win, Hout, Wout) is None:        # the per-frame path, two launches and a temporary each
        if slots_host.min() < 0 or slots_host.max() >= B * T or np.unique(slots_host).size != N:
            raise MspiError("assemble_clips: slots must be distinct and inside the %d x %d clip tensor" % (B, T))
        for i, sl in enumerate(slots_host.tolist()):
            out[sl // T, :, sl % T].copy_(resize_normalize(frames_u8[i], (Hout, Wout), mean, std))
        return out
    hb, hk, hks = _coeffs(Win, Wout, dev)
    vb, vk, vks = _coeffs(Hin, Hout, dev)
    hb_host, vb_host = _coeffs_host(Win, Wout)[0], _coeffs_host(Hin, Hout)[0]
    if slots_dev is None:
        slots_dev = torch.from_numpy(slots_host).to(dev)
    assert slots_dev.dtype == torch.int32 and slots_dev.is_cuda and slots_dev.numel() == N and slots_dev.is_contiguous()
    check(lib.mspi_clip_resize_norm_fwd(frames_u8.data_ptr(), N, Hin, Win, slots_dev.data_ptr(), slots_host.ctypes.data,
                                        out.data_ptr(), B, T, out.stride(0), out.stride(1), out.stride(2), out.stride(3), Hout, Wout,
                                        hb.data_ptr(), hb_host.ctypes.data, hk.data_ptr(), hks, vb.data_ptr(), vb_host.ctypes.data,
                                        vk.data_ptr(), vks, m, s, torch.cuda.current_stream().cuda_stream),
          "mspi_clip_resize_norm_fwd")
    return out


def decode_rgb_bytes(data):
    """uint8 [H,W,3]: the frame as upstream reads it (PIL, convert('RGB'), inference.py:154-165), from the file's bytes."""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def decode_frames(blobs, device, stats=None, host_decode=None):
    """Input frames given as the bytes of their JPEG files -> a list of uint8 [H,W,3] tensors on `device`, what PIL decodes
    pixel for pixel.  Files the device decoder takes (`engine.jpeg_probe`) are grouped by geometry and decoded by one
    `engine.jpeg_decode_rgb` launch sequence per group on the current stream; only their bytes are uploaded.  A file the
    parser refuses (progressive, restart markers, CMYK, ...) and a file whose scan the device reports as truncated or corrupt
    (status != 0) are decoded with PIL on the host and uploaded as pixels.  Reading the status words synchronises the stream
    once per call.  stats: a dict whose "device" / "host" counters are advanced; host_decode(k): the caller's own host decode
    of frame k (default: PIL on blobs[k])."""
    from . import engine as E
    out, groups, infos = [None] * len(blobs), {}, [E.jpeg_probe(b) for b in blobs]
    for k, info in enumerate(infos):
        if info is not None:
            groups.setdefault((info.H, info.W, info.ncomp, info.hs, info.vs), []).append(k)
    done = []
    for idx in groups.values():
        rgb, status, _ = E.jpeg_decode_rgb([blobs[k] for k in idx], device=device, infos=[infos[k] for k in idx])
        done.append((idx, rgb, status))
    for idx, rgb, status in done:
        for j, (k, bad) in enumerate(zip(idx, status.tolist())):
            if not bad:
                out[k] = rgb[j]
    host = [k for k in range(len(blobs)) if out[k] is None]
    for k in host:
        out[k] = torch.from_numpy(decode_rgb_bytes(blobs[k]) if host_decode is None else host_decode(k)).to(device, non_blocking=True)
    if stats is not None:
        stats["device"] = stats.get("device", 0) + len(blobs) - len(host)
        stats["host"] = stats.get("host", 0) + len(host)
    return out
