"""Score a checkpoint on a val / test split: the reference's AudioVisualDataset + validation_one_epoch pair
(avsp_dataloader.py:83-193, engine_train.py:84-125) on the MI355X.

    python -m mspi_amd.validate --weight w.pt --path_data ./AuViDataset --dataset AVAD --split 2 --mode test --model x3dl
        [--resolution H W] [--clip_size 16] [--batch 8] [--no_sound] [--fixations] [--workers 8] [--device_decode] [--json OUT]

inference.build_model builds the model, avsp_dataloader.AudioVisualDataset yields device batches (frames decoded on the
host, clips assembled by one launch per batch) and metrics.validation_one_epoch scores them.  Prints upstream's line
(engine_train.py:122) and the result dict as JSON.  One process, one GPU: the numbers are means of per-batch means, which
do not merge across shards, so WORLD_SIZE > 1 is refused.  There is no CPU fallback."""
import argparse
import json
import os
import types

import torch

from ._lib import MspiError


def _single_rank():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise MspiError("mspi_amd.validate runs on one rank: its numbers are means of per-batch means, which do not merge "
                        "across shards (WORLD_SIZE=%s)" % os.environ["WORLD_SIZE"])


def _cuda(device):
    if device is None:
        if not torch.cuda.is_available():
            raise MspiError("mspi_amd.validate needs an MI355X; there is no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise MspiError("mspi_amd.validate runs on the GPU only; there is no CPU fallback (device %s)" % device)
    return device


def format_line(stats):
    """engine_train.py:122's line from validation_one_epoch's dict."""
    return "* Kldiv {:.4f} CC {:.4f} SIM {:.4f} loss {:.4f}".format(stats["kld"], stats["cc"], stats["sim"], stats["loss"])


@torch.no_grad()
def validate(model, data_root, dataset="AVAD", split=2, mode="val", resolution=(224, 384), clip_size=16, batch=8, use_sound=True,
             fixations=False, workers=8, device=None, generator=None, device_decode=False):
    """{"loss", "kld", "cc", "sim"[, "nss", "auc_j"]} of `model` (on the device, eval) over the clips of the split, as
    metrics.validation_one_epoch computes them from the batches of avsp_dataloader.AudioVisualDataset.  fixations: also
    NSS / AUC-Judd against the fixation maps.  The f16x3 range guard is read once at the end and raises."""
    from . import engine as E
    from . import metrics as M
    from .avsp_dataloader import AudioVisualDataset
    _single_rank()
    device = _cuda(device)
    data = AudioVisualDataset(data_root, dataset, split, clip_size, mode, use_sound, tuple(resolution), batch_size=batch,
                              with_fixations=fixations, generator=generator, workers=workers, device=device,
                              device_decode=device_decode)
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(USE_SOUND=bool(use_sound)))
    stats = M.validation_one_epoch(model, data, device, cfg)
    E.check_range(sync=True)                 # raise rather than report numbers computed from inf / NaN activations
    return stats


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m mspi_amd.validate", description=__doc__.split("\n")[0])
    parser.add_argument("--weight", default="./output/mvitv2_small_224_384_16_s2.pt", type=str)
    parser.add_argument("--path_data", default="./AuViDataset", type=str)
    parser.add_argument("--dataset", default="AVAD", type=str)
    parser.add_argument("--split", default=2, type=int)
    parser.add_argument("--mode", default="val", choices=("val", "test"), help="which fold list: <dataset>_list_<mode>_<split>_fps.txt")
    parser.add_argument("--model", default=os.environ.get("MSPI_MOTION_ENCODER", "mvitv2s"), type=str)
    parser.add_argument("--resolution", default=[224, 384], type=int, nargs=2, help="H W the frames are resized to")
    parser.add_argument("--clip_size", default=16, type=int)
    parser.add_argument("--batch", default=8, type=int, help="clips per forward")
    parser.add_argument("--no_sound", dest="use_sound", action="store_false", help="the visual-only model")
    parser.add_argument("--fixations", action="store_true", help="also NSS / AUC-Judd against the fixation maps")
    parser.add_argument("--workers", default=8, type=int, help="host threads decoding JPEGs")
    parser.add_argument("--device_decode", action="store_true", default=os.environ.get("MSPI_DEVICE_DECODE") == "1",
                        help="decode the frames on the GPU (the same pixels); the host threads then only read the files")
    parser.add_argument("--json", default=None, type=str, help="also write the result dict to this file")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    _single_rank()
    if not torch.cuda.is_available():
        raise SystemExit("mspi_amd.validate needs an MI355X (no CPU fallback)")
    from . import inference as I
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    I.device = device
    I._RESOLUTION[:] = args.resolution
    model = I.build_model(args.model, args.resolution, weight=args.weight, use_sound=args.use_sound)
    stats = validate(model, args.path_data, args.dataset, args.split, args.mode, args.resolution, args.clip_size, args.batch,
                     args.use_sound, args.fixations, args.workers, device, device_decode=args.device_decode)
    print(format_line(stats))
    print(json.dumps(stats))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(stats, f, indent=1)
    return stats


if __name__ == "__main__":
    main()
