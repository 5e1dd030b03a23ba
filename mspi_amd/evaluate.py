"""From a directory of written saliency maps plus a dataset's annotations to the metric table, on the GPU.

inference.py writes one map per frame to save_path/<video>/<frame>; metrics.py scores equal-shaped device maps.  This
module is the step between them: it pairs the files, decodes them on the host (PIL / scipy.io), uploads uint8 and does
everything after that on the device -- the two resizes upstream does with cv2.resize and resize_fixation
(utils/compute_saliency_metrics.py:119-122, avsp_dataloader.py:16-31,176,186; csrc/evalprep.hip here) and the seven metric
launches of metrics.py.  The maps come from files, so they are linear, not the log maps SalEval.update() takes: the
launches are called directly and SalEval only keeps the sums.

    python -m mspi_amd.evaluate --pred ./output --path_data ./AuViDataset --dataset AVAD --split 2 [--at gt|pred]
        [--batch N] [--other N] [--baseline PATH|mean] [--no_jitter] [--seed S] [--json OUT]

plan() and host_batches() are the host side and touch no GPU; device_batches() yields the resized device maps of each batch
and evaluate_dataset() scores them.  There is no CPU fallback."""
import argparse
import ctypes as C
import glob
import json
import math
import os
import re
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from . import metrics as M
from ._lib import MspiError, check

MEAN_BASELINE_SIZE = (224, 384)      # baseline="mean" averages the densities at the model's size (config.py DATA.RESOLUTION)
_FRAME_NO = re.compile(r"_(\d+)\.[^.]+$")


# --------------------------------------------------------------------------------------------------- device resizes
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda_maps(what, t, dtypes):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise MspiError("mspi_amd.evaluate.%s runs on the GPU only; there is no CPU fallback" % what)
    if t.dim() != 3 or t.dtype not in dtypes:
        raise MspiError("%s: maps must be a [B,H,W] tensor of %s, got %s %s" % (
            what, " or ".join(str(d) for d in dtypes), tuple(t.shape), t.dtype))
    return t.contiguous()


def _size(what, size):
    if len(size) != 2 or int(size[0]) <= 0 or int(size[1]) <= 0:
        raise MspiError("%s: size must be two positive extents, got %s" % (what, (size,)))
    return int(size[0]), int(size[1])


def resize_maps(maps, size):
    """float32 [B,Ho,Wo] from [B,H,W] uint8 (values used as 0..255) or float32 CUDA maps: bilinear, cv2.INTER_LINEAR's
    convention (pixel centres aligned, edges clamped, no antialiasing); the same size is a bit-exact copy / conversion."""
    lib = _lib.load()
    x = _cuda_maps("resize_maps", maps, (torch.uint8, torch.float32))
    Ho, Wo = _size("resize_maps", size)
    B, H, W = x.shape
    out = torch.empty(B, Ho, Wo, dtype=torch.float32, device=x.device)
    check(lib.mspi_resize_bilinear_fwd(x.data_ptr(), 1 if x.dtype == torch.uint8 else 0, out.data_ptr(), B, H, W, Ho, Wo, _stream()),
          "mspi_resize_bilinear_fwd")
    return out


def resize_fixations(fix, size):
    """float32 [B,row,col] binary maps from [B,H,W] float32 CUDA fixation maps: the reference's resize_fixation
    (avsp_dataloader.py:16-31), bit for bit."""
    lib = _lib.load()
    x = _cuda_maps("resize_fixations", fix, (torch.float32,))
    row, col = _size("resize_fixations", size)
    B, H, W = x.shape
    out = torch.empty(B, row, col, dtype=torch.float32, device=x.device)
    check(lib.mspi_resize_fixation_fwd(x.data_ptr(), out.data_ptr(), B, H, W, row, col, _stream()), "mspi_resize_fixation_fwd")
    return out


# --------------------------------------------------------------------------------------------------- host: pairing files
def list_videos(path_data, dataset, split, shard=True):
    """The sorted video names of fold_lists/<dataset>_list_test_<split>_fps.txt (DIEM: DIEM_list_test_fps.txt), as
    inference.py reads them; shard: this rank's slice by RANK / WORLD_SIZE, as inference.py shards."""
    file_name = "DIEM_list_test_fps.txt" if dataset == "DIEM" else "{}_list_test_{}_fps.txt".format(dataset, split)
    names = []
    with open(os.path.join(path_data, "fold_lists", file_name), "r") as f:
        for line in f.readlines():
            if line.strip():
                names.append(line.split(" ")[0])
    names.sort()
    if shard:
        rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        names = names[rank::world]
    return names


def _numbered(pattern):
    """{frame number: path} of the files matching pattern (the number is what follows the last underscore)."""
    out = {}
    for p in sorted(glob.glob(pattern)):
        m = _FRAME_NO.search(os.path.basename(p))
        if m:
            out.setdefault(int(m.group(1)), p)
    return out


def _annotations(path_data, dataset, video):
    """[(frame number, density path, fixation path)] of one video, by frame number.  The fixation map is fixMap_%05d.mat,
    or fixMap_%05d.png where there is no .mat."""
    root = os.path.join(path_data, "annotations", dataset, video)
    out = []
    for no, dens in sorted(_numbered(os.path.join(root, "maps", "eyeMap_*.*")).items()):
        fix = os.path.join(root, "fixMap_%05d.mat" % no)
        if not os.path.exists(fix):
            fix = os.path.join(root, "fixMap_%05d.png" % no)
            if not os.path.exists(fix):
                raise FileNotFoundError("evaluate: %s has no fixation map %s (.mat or .png)" % (dens, fix[:-4]))
        out.append((no, dens, fix))
    return out


def _seed_of(generator):
    if generator is None:
        return 0
    if isinstance(generator, np.random.Generator):
        return int(generator.integers(0, 2 ** 62))
    return int(generator)


def plan(pred_root, path_data, dataset, split, other=0, generator=None):
    """The work of this rank as plain data, without decoding a file or touching the GPU:
    {"videos": [{"video", "index", "frames": [{"frame", "pred", "density", "fixation", "others": [fixation paths]}]}],
     "unannotated": n, "seed": s}.
    The three files of a frame carry the same number (avsp_dataloader.py:150-186, inference.py:370).  An annotated frame
    without a prediction raises FileNotFoundError naming the missing file; a predicted frame without an annotation is
    counted in "unannotated".  other = N > 0: every frame gets the fixation files of N frames of the OTHER videos of the
    whole list, drawn by numpy's Generator seeded with (seed, video's index in the whole list, frame number) -- a frame's
    draw does not depend on the sharding or on the frames before it.  generator: None (seed 0), an int seed or a
    numpy Generator (one draw from it is the seed)."""
    seed = _seed_of(generator)
    everything = list_videos(path_data, dataset, split, shard=False)
    mine = set(list_videos(path_data, dataset, split, shard=True))
    annotations = {}

    def ann(v):
        if v not in annotations:
            annotations[v] = _annotations(path_data, dataset, v)
        return annotations[v]

    pool = []        # (video index, fixation path) of every annotated frame of the list, in list order
    if other > 0:
        for vi, v in enumerate(everything):
            pool += [(vi, a[2]) for a in ann(v)]
        pool_video = np.array([p[0] for p in pool], dtype=np.int64)
    videos, unannotated = [], 0
    for vi, v in enumerate(everything):
        if v not in mine:
            continue
        preds = _numbered(os.path.join(pred_root, v, "img_*.*"))
        frames = []
        for no, dens, fix in ann(v):
            if no not in preds:
                raise FileNotFoundError("evaluate: no prediction %s for the annotated frame %s" % (
                    os.path.join(pred_root, v, "img_%05d.*" % no), dens))
            others = []
            if other > 0:
                cand = np.flatnonzero(pool_video != vi)
                if cand.size == 0:
                    raise MspiError("evaluate: other=%d needs annotated frames in another video than %s" % (other, v))
                rng = np.random.default_rng([seed, vi, no])
                others = [pool[i][1] for i in rng.choice(cand, size=other, replace=cand.size < other)]
            frames.append({"frame": no, "pred": preds[no], "density": dens, "fixation": fix, "others": others})
        unannotated += len(set(preds) - {a[0] for a in ann(v)})
        videos.append({"video": v, "index": vi, "frames": frames})
    return {"videos": videos, "unannotated": unannotated, "seed": seed}


# --------------------------------------------------------------------------------------------------- host: decoding
def load_gray(path):
    """uint8 [H,W]: the file as upstream reads it (PIL, convert('L'))."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("L"), dtype=np.uint8)


def load_fixation(path):
    """uint8 [H,W] of 0 / 1: a .mat's `eyeMap` (scipy.io.loadmat, avsp_dataloader.py:184-185) or an image; non-zero is a
    fixation (np.argwhere upstream)."""
    if path.lower().endswith(".mat"):
        import scipy.io
        a = np.asarray(scipy.io.loadmat(path)["eyeMap"])
    else:
        a = load_gray(path)
    if a.ndim != 2:
        raise MspiError("evaluate: fixation map %s is not two-dimensional: %s" % (path, a.shape))
    return (a != 0).astype(np.uint8)


def _decode(item, with_pred=True):
    dens = load_gray(item["density"])
    if dens.max() == 0:                     # avsp_dataloader.py:137-139,182: no saliency defined for this frame
        return None
    out = {"frame": item["frame"], "density": dens}
    if with_pred:
        out["pred"] = load_gray(item["pred"])
        out["fixation"] = load_fixation(item["fixation"])
        out["others"] = [load_fixation(p) for p in item["others"]]
    return out


def _decode_batches(work, batch, with_pred, counters):
    for video in work["videos"]:
        cur, shape = [], None
        for item in video["frames"]:
            d = _decode(item, with_pred)
            if d is None:
                counters["empty_gt"] += 1
                continue
            s = (d["density"].shape,) + ((d["pred"].shape, d["fixation"].shape) if with_pred else ())
            if cur and (s != shape or len(cur) >= batch):
                yield video, cur
                cur = []
            shape = s
            cur.append(d)
        if cur:
            yield video, cur


def host_batches(work, batch=8, with_pred=True, counters=None, prefetch=True):
    """(video, [decoded frames]) per batch: at most `batch` consecutive frames of ONE video whose maps have equal shapes,
    decoded to uint8 numpy arrays.  A frame whose density is all zero is left out and counted in counters["empty_gt"].
    prefetch: ONE background thread decodes the next batch while the caller works on this one (never more: the decode is
    the host's share and is not sized by the machine's CPU count)."""
    counters = counters if counters is not None else {}
    counters.setdefault("empty_gt", 0)
    it = _decode_batches(work, max(1, int(batch)), with_pred, counters)
    if not prefetch:
        yield from it
        return
    end = object()
    with ThreadPoolExecutor(max_workers=1) as ex:
        nxt = ex.submit(next, it, end)
        while True:
            got = nxt.result()
            if got is end:
                return
            nxt = ex.submit(next, it, end)
            yield got


# --------------------------------------------------------------------------------------------------- device
def _up(arrays, device):
    return torch.from_numpy(np.stack(arrays)).to(device, non_blocking=False)


def _others_union(frames, size, device):
    """float32 [B,H,W]: per frame the union of its other-fixation maps, each brought to `size` with resize_fixations (one
    launch per distinct source shape)."""
    out = torch.zeros((len(frames),) + tuple(size), dtype=torch.float32, device=device)
    by_shape = {}
    for b, fr in enumerate(frames):
        for o in fr["others"]:
            by_shape.setdefault(o.shape, []).append((b, o))
    for group in by_shape.values():
        r = resize_fixations(_up([o for _, o in group], device).float(), size)
        for k, (b, _) in enumerate(group):
            torch.maximum(out[b], r[k], out=out[b])
    return out


def mean_baseline(path_data, dataset, split, batch=8, device=None):
    """float32 [224,384] on the device: the mean of the non-empty densities of the WHOLE list (every rank of a sharded run
    computes the same map, so that the shards score against one baseline), each resized on the device and summed in
    float64 in list order."""
    device = _device(device)
    work = {"videos": [{"video": v, "frames": [{"frame": no, "density": d} for no, d, _ in _annotations(path_data, dataset, v)]}
                       for v in list_videos(path_data, dataset, split, shard=False)]}
    acc = torch.zeros(MEAN_BASELINE_SIZE, dtype=torch.float64, device=device)
    n = 0
    for _, frames in host_batches(work, batch, with_pred=False):
        acc += resize_maps(_up([f["density"] for f in frames], device), MEAN_BASELINE_SIZE).double().sum(0)
        n += len(frames)
    if n == 0:
        raise MspiError("evaluate: baseline='mean' found no non-empty density")
    return (acc / n).float()


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise MspiError("mspi_amd.evaluate needs an MI355X; there is no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise MspiError("mspi_amd.evaluate runs on the GPU only; there is no CPU fallback (device %s)" % device)
    return device


def _baseline(baseline, path_data, dataset, split, batch, device):
    if baseline is None:
        return None
    if isinstance(baseline, str) and baseline == "mean":
        return mean_baseline(path_data, dataset, split, batch, device)
    if isinstance(baseline, (str, os.PathLike)):
        baseline = torch.from_numpy(np.load(baseline).astype(np.float32)).to(device)
    if not (torch.is_tensor(baseline) and baseline.is_cuda):
        raise MspiError("evaluate: baseline must be None, 'mean', a .npy path or a CUDA tensor; there is no CPU fallback")
    if baseline.dim() != 2:
        raise MspiError("evaluate: the baseline density must be [H,W], got %s" % (tuple(baseline.shape),))
    return baseline.float()


def device_batches(work, at="gt", batch=8, baseline=None, device=None, counters=None):
    """Per batch of host_batches(): (video, frame numbers, s, d, f, o, b) -- prediction, density, fixations, other-fixations
    (None without) and baseline (None without) as equal-shaped float32 [B,H,W] device maps, ready for metrics.py.
    at="gt": everything at the annotation's size, the prediction resized (compute_saliency_metrics.py:119-122);
    at="pred": everything at the prediction's size, density and fixations resized as upstream's loader does."""
    if at not in ("gt", "pred"):
        raise MspiError("evaluate: at must be 'gt' or 'pred', got %r" % (at,))
    device = _device(device)
    for video, frames in host_batches(work, batch, counters=counters):
        pred = _up([f["pred"] for f in frames], device)
        dens = _up([f["density"] for f in frames], device)
        fix = _up([f["fixation"] for f in frames], device).float()
        size = tuple(dens.shape[1:]) if at == "gt" else tuple(pred.shape[1:])
        s = resize_maps(pred, size)
        d = resize_maps(dens, size)
        f = fix if tuple(fix.shape[1:]) == size else resize_fixations(fix, size)
        o = _others_union(frames, size, device) if frames[0]["others"] else None
        b = None if baseline is None else resize_maps(baseline[None], size).expand(len(frames), -1, -1).contiguous()
        yield video, [fr["frame"] for fr in frames], s, d, f, o, b


def score_batch(s, d, f, o=None, b=None, jitter=True, generator=None):
    """{metric: list of per-frame floats} for one batch of equal-shaped linear maps -- SalEval.update()'s launches without
    its exp().  s_auc is left out for H > W (the kernel refuses such maps, as upstream raises)."""
    vals = {}
    m = M.per_sample(s, d, fix=f)
    vals["kl"], vals["cc"], vals["sim"], vals["nss"] = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    vals["auc_j"] = M.auc_judd_per_sample(s, f, jitter, generator)
    if o is not None and s.shape[1] <= s.shape[2]:
        vals["s_auc"] = M.sauc_counts(s, f, o)
    if b is not None:
        vals["ig"] = M.ig_per_sample(s, f, b)
    out = {}
    for k, v in vals.items():                # every launch is queued before the first copy to the host waits
        v = v.cpu().tolist()
        out[k] = [M._sauc_score(c) for c in v] if k == "s_auc" else v
    return out


def _summary(ev):
    res = ev.result()
    fed = list(res)
    return {"mean": res, "sum": {k: ev.sum[k] for k in fed}, "count": {k: ev.count[k] for k in fed},
            "nan": {k: ev.nan[k] for k in fed}}


def evaluate_dataset(pred_root, path_data, dataset, split, at="gt", batch=8, other=0, baseline=None, jitter=True,
                     generator=None, device=None):
    """Score the maps under pred_root/<video>/img_%05d.* against annotations/<dataset>/<video>/ of path_data.

    Returns {metric: mean over its frames that are not NaN} for kl, cc, sim, nss, auc_j, s_auc (other > 0) and ig
    (baseline given), plus "frames" (frames scored), "sum" / "count" / "nan" per metric (a sharded run -- RANK /
    WORLD_SIZE -- reports its own shard; the per-video entries of the shards are those of the unsharded run and "sum" is
    math.fsum of the per-video sums, so the shards add up; merging them is the caller's),
    "per_video" ({video: {"frames", "mean", "sum", "count", "nan"}}), "unannotated" (predicted frames without an
    annotation, skipped) and "empty_gt" (frames whose density is all zero, skipped).
    other: N > 0 scores shuffled AUC against the union of N other frames' fixations (see plan()); frames with H > W are
    counted under nan["s_auc"].  baseline: a .npy path, a [H,W] CUDA tensor or "mean" (mean_baseline()) turns on IG.
    jitter / generator: AUC-Judd's tie-breaking noise (metrics.auc_judd) is drawn per video from a device generator
    seeded with (seed, video's index in the list), so it is repeatable and independent of the sharding; generator is
    None (seed 0), an int or a numpy Generator, and also seeds the choice of other-frames."""
    device = _device(device)
    work = plan(pred_root, path_data, dataset, split, other=other, generator=generator)
    base = _baseline(baseline, path_data, dataset, split, batch, device)
    per_video, frames_of = {}, {}
    counters = {"empty_gt": 0}
    gen, gen_video = None, None
    for video, nos, s, d, f, o, b in device_batches(work, at, batch, base, device, counters):
        name = video["video"]
        if name not in per_video:
            per_video[name], frames_of[name] = M.SalEval(), 0
        if jitter is True and gen_video != name:
            gen = torch.Generator(device=device).manual_seed((work["seed"] * 1000003 + video["index"]) % (2 ** 63))
            gen_video = name
        vals = score_batch(s, d, f, o, b, jitter=bool(jitter), generator=gen)
        if o is not None and "s_auc" not in vals:
            vals["s_auc"] = [float("nan")] * len(nos)
        for k, v in vals.items():
            per_video[name]._add(k, v)
        frames_of[name] += len(nos)
    result = {"per_video": {}}
    for v in work["videos"]:                 # in list order; a video whose frames were all skipped still shows up
        name = v["video"]
        pv = _summary(per_video.get(name, M.SalEval()))
        pv["frames"] = frames_of.get(name, 0)
        result["per_video"][name] = pv
    # The totals are the correctly rounded sums (math.fsum) of the per-video sums, so they do not depend on the order or
    # the grouping of the videos: math.fsum over the per-video sums of all shards gives the unsharded total bit for bit.
    fed = [k for k in M.SalEval.KEYS if any(k in pv["sum"] for pv in result["per_video"].values())]
    pvs = list(result["per_video"].values())
    result["sum"] = {k: math.fsum(pv["sum"].get(k, 0.0) for pv in pvs) for k in fed}
    result["count"] = {k: sum(pv["count"].get(k, 0) for pv in pvs) for k in fed}
    result["nan"] = {k: sum(pv["nan"].get(k, 0) for pv in pvs) for k in fed}
    for k in fed:
        result[k] = result["sum"][k] / result["count"][k] if result["count"][k] else float("nan")
    result["frames"] = sum(pv["frames"] for pv in pvs)
    result["unannotated"] = work["unannotated"]
    result["empty_gt"] = counters["empty_gt"]
    return result


# --------------------------------------------------------------------------------------------------- CLI
def format_table(result):
    keys = [k for k in M.SalEval.KEYS if k in result]
    lines = ["%-28s %7s " % ("video", "frames") + " ".join("%9s" % k for k in keys)]
    for name, pv in sorted(result["per_video"].items()):
        lines.append("%-28s %7d " % (name[:28], pv["frames"]) + " ".join("%9.4f" % pv["mean"].get(k, float("nan")) for k in keys))
    lines.append("%-28s %7d " % ("all", result["frames"]) + " ".join("%9.4f" % result[k] for k in keys))
    lines.append("NaN frames left out: " + (", ".join("%s %d" % (k, result["nan"][k]) for k in keys if result["nan"][k]) or "none")
                 + "; unannotated predictions %d, empty densities %d" % (result["unannotated"], result["empty_gt"]))
    return "\n".join(lines)


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m mspi_amd.evaluate", description=__doc__.split("\n")[0])
    parser.add_argument("--pred", required=True, type=str, help="inference.py's --save_path: <pred>/<video>/img_%%05d.jpg")
    parser.add_argument("--path_data", default="./AuViDataset", type=str)
    parser.add_argument("--dataset", default="AVAD", type=str)
    parser.add_argument("--split", default=2, type=int)
    parser.add_argument("--at", default="gt", choices=("gt", "pred"), help="score at the annotation's or at the prediction's size")
    parser.add_argument("--batch", default=8, type=int, help="frames of one video per launch")
    parser.add_argument("--other", default=0, type=int, help="N > 0: shuffled AUC against N other frames' fixations")
    parser.add_argument("--baseline", default=None, type=str, help="a .npy density or 'mean': turns on information gain")
    parser.add_argument("--no_jitter", dest="jitter", action="store_false", help="AUC-Judd without the tie-breaking noise")
    parser.add_argument("--seed", default=0, type=int, help="seeds the other-frames and the jitter noise")
    parser.add_argument("--json", default=None, type=str, help="also write the result dict to this file")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    if not torch.cuda.is_available():
        raise SystemExit("mspi_amd.evaluate needs an MI355X (no CPU fallback)")
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    t0 = time.time()
    result = evaluate_dataset(args.pred, args.path_data, args.dataset, args.split, at=args.at, batch=args.batch, other=args.other,
                              baseline=args.baseline, jitter=args.jitter, generator=args.seed, device=device)
    dt = time.time() - t0
    print(format_table(result))
    print("%d frames in %.1f s (%.1f frames/s; the host's image decoding bounds this)" % (result["frames"], dt,
                                                                                        result["frames"] / max(dt, 1e-9)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1, allow_nan=True)
    return result


if __name__ == "__main__":
    main()
