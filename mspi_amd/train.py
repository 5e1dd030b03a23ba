"""Fine-tune the readout (or only its tail, or the SA gates with it) of a checkpoint: the reference's train.py as far as the readout needs it, on the MI355X.

    python -m mspi_amd.train --trainable readout|readout_tail|fusion|lateral_blocks|lateral_entries|adapter --weights w.pt --dataset AVAD --split 1 --model x3dl
        [--path_data ./AuViDataset] [--log_dir ./training_logs] [--save_ckpt_freq 10] [--gamma 1] [--start_epoch 0]
        [--resolution H W] [--batch 2] [--no_sound] [--workers 8] [--sync]

--trainable readout_tail: only readout[8], readout[10] and readout[12] train (model.trainable("readout_tail")); everything in
front of them is frozen and runs as in inference, with eval BatchNorm folded into the convolutions.
--trainable readout: the whole readout Sequential trains, all 16 of its tensors; readout[2] and readout[5] run on batch
statistics and update their running statistics as upstream's decoder training does (autograd.ReadoutHead).
--trainable fusion: the three SA gates train with the whole readout, 31 tensors; the gates' BatchNorm layers run on batch
statistics too, and the backward reaches the lateral outputs through the gating and the top-down sums (autograd.Fusion).
--trainable lateral_blocks: on top of that the ConvNextBlock at the end of each lateral trains, 71 tensors (autograd.LateralBlock:
the depthwise convs', LayerNorm's and GELU's backward); the laterals' entry convs stay frozen.
--trainable lateral_entries: on top of that the laterals' entry convs train, latlayer_k[0] and where present latlayer_k[1] --
83 tensors with x3dl, 81 with s3d, 79 with slowfast (autograd.LateralEntry: the weight gradient of the composed conv, then the
chain rule through the composition); with it every lateral parameter moves, as in upstream's training.
--trainable adapter: on top of that the adapter's Inception trains, its eight conv -> BatchNorm -> ReLU layers on batch
statistics -- 107 tensors with x3dl, 105 with s3d, 103 with slowfast (autograd.Adapter; autograd.Fusion returns the gradient
of the masks); with it the visual-only model trains everything upstream trains except the motion encoder.
Still frozen in all six: the SyncBlock, the contrastive projectors and every encoder (below --trainable adapter also the
adapter, below --trainable lateral_entries also the laterals' entry convs, with --trainable fusion also the laterals' blocks,
with --trainable readout and readout_tail also the SA gating).
--sync, a flag beside the ladder (model.trainable(stage, sync=True)), takes the first two off that list: with --trainable
lateral_entries or adapter on the audio-visual model the SyncBlock (39 tensors) and the contrastive projectors and predictors
(36) train too -- 182 tensors with x3dl on adapter, 180 with s3d, 178 with slowfast -- the SyncBlock through latlayer_3's entry
conv (autograd.sync_block, the data gradient of autograd.LateralEntry) and loss_av, the projectors through loss_av alone
(autograd.ContrastHead), which train_one_epoch adds to the criterion times --gamma.  With it the audio-visual model trains
everything upstream trains except the three encoders.  It is refused with --no_sound and below --trainable lateral_entries.
That is fine-tuning of a released checkpoint's decoder head, not upstream's full training.  As upstream: the training split of
avsp_dataloader.AudioVisualDataset, AdamW over the parameters that require grad with weight decay 0, cfg.SOLVER.LR for 60
epochs then a tenth of it every 60 (lr_by_epoch), a state_dict checkpoint every --save_ckpt_freq epochs and at the end
(inference.build_model loads them), one JSON line per epoch, printed and appended to <log_dir>/log.txt.  One process, one GPU."""
import argparse
import json
import os

import torch

from ._lib import MspiError
from .autograd import STAGE_NAMES

TRAINABLE = STAGE_NAMES[:2]                       # what trains on a frozen pyramid
TRAINABLE_STAGES = STAGE_NAMES[:3]                # ... and on frozen laterals
TRAINABLE_BLOCKS = STAGE_NAMES[3:4]               # ... and with the laterals' ConvNextBlocks
TRAINABLE_ENTRIES = STAGE_NAMES[4:5]              # ... and with the laterals' entry convs
TRAINABLE_ADAPTER = STAGE_NAMES[5:]               # ... and with the adapter's Inception: every value --trainable takes


def lr_by_epoch(cfg):
    """train.py:161-166: cfg.SOLVER.LR for the first 60 epochs, then a tenth of it, divided by ten again every 60 epochs; one
    value per epoch up to cfg.SOLVER.MAX_EPOCH."""
    values = [cfg.SOLVER.LR for _ in range(60)]
    lr = cfg.SOLVER.LR * 0.1
    for i in range(cfg.SOLVER.MAX_EPOCH - 60):
        values.append(lr)
        if (i + 1) % 60 == 0:
            lr = lr * 0.1
    return values


def _single_rank():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise MspiError("mspi_amd.train runs on one rank: multi-rank training is not built (WORLD_SIZE=%s)" % os.environ["WORLD_SIZE"])


def check_trainable(value):
    if value not in STAGE_NAMES:
        raise MspiError("--trainable %s: only %s can be trained on a frozen pyramid, and %s on frozen laterals, and %s on frozen "
                        "entry convs, and %s on a frozen adapter, and %s on frozen encoders (the models' backward stops behind the "
                        "laterals' entry convs and the adapter's Inception: the SyncBlock, the contrastive projectors and the "
                        "encoders do not train)"
                        % (value, ", ".join(TRAINABLE), TRAINABLE_STAGES[-1], ", ".join(TRAINABLE_BLOCKS), ", ".join(TRAINABLE_ENTRIES),
                           ", ".join(TRAINABLE_ADAPTER)))
    return value


def check_sync(trainable, sync, use_sound):
    """--sync beside --trainable: only on the audio-visual model and only from lateral_entries on."""
    if sync and not use_sound:
        raise MspiError("--sync with --no_sound: the visual-only model has neither a SyncBlock nor a contrastive head to train")
    if sync and trainable not in STAGE_NAMES[4:]:
        raise MspiError("--sync with --trainable %s: the SyncBlock reaches the map only through latlayer_3's entry conv, so --sync "
                        "needs --trainable %s" % (trainable, " or ".join(STAGE_NAMES[4:])))
    return bool(sync)


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m mspi_amd.train", description=__doc__.split("\n")[0])
    parser.add_argument("--trainable", default="readout_tail", type=str, help="the part of the model that trains: %s or %s" % (", ".join(STAGE_NAMES[:-1]), STAGE_NAMES[-1]))
    parser.add_argument("--start_epoch", default=0, type=int)
    parser.add_argument("--split", default=1, type=int)
    parser.add_argument("--dataset", default="AVAD", type=str)
    parser.add_argument("--weights", default="", type=str, help="checkpoint to start from (a state_dict)")
    parser.add_argument("--log_dir", default="./training_logs", type=str)
    parser.add_argument("--save_ckpt_freq", default=10, type=int)
    parser.add_argument("--gamma", default=1.0, type=float)
    parser.add_argument("--path_data", default="./AuViDataset", type=str)
    parser.add_argument("--model", default=os.environ.get("MSPI_MOTION_ENCODER", "mvitv2s"), type=str)
    parser.add_argument("--resolution", default=[224, 384], type=int, nargs=2, help="H W the frames are resized to")
    parser.add_argument("--clip_size", default=16, type=int)
    parser.add_argument("--batch", default=None, type=int, help="clips per step (default cfg.TRAIN.BATCH_SIZE)")
    parser.add_argument("--no_sound", dest="use_sound", action="store_false", help="the visual-only model")
    parser.add_argument("--sync", action="store_true", help="also train the SyncBlock and the contrastive head (model.trainable(stage, "
                        "sync=True)): audio-visual model, --trainable lateral_entries or adapter")
    parser.add_argument("--workers", default=8, type=int, help="host threads decoding JPEGs")
    parser.add_argument("--seed", default=2023, type=int)
    return parser


def train(model, data, cfg, device, log_dir, start_epoch=0, save_ckpt_freq=10, gamma=1.0):
    """The epoch loop of train.py:158-200 over `data` (an iterable of device batches).  Returns the per-epoch dicts."""
    from .engine_train import train_one_epoch
    from .metrics import SalLoss
    params = [p for p in model.parameters() if p.requires_grad]
    if not params:
        calls = ["model.trainable('%s')" % n for n in STAGE_NAMES]
        raise MspiError("train: no parameter requires grad; call %s or %s first" % (", ".join(calls[:-1]), calls[-1]))
    optimizer = torch.optim.AdamW(params, cfg.SOLVER.LR, weight_decay=0)
    schedule = lr_by_epoch(cfg)
    ckpt_dir = os.path.join(log_dir, "checkpoints")
    os.makedirs(ckpt_dir, exist_ok=True)
    n_parameters = sum(p.numel() for p in params)
    logs = []
    for epoch in range(start_epoch, cfg.SOLVER.MAX_EPOCH):
        for group in optimizer.param_groups:
            group["lr"] = schedule[epoch]
        stats = train_one_epoch(model, SalLoss(), data, optimizer, device, epoch, cfg, gamma=gamma)
        if (epoch + 1) % save_ckpt_freq == 0 or epoch + 1 == cfg.SOLVER.MAX_EPOCH:
            torch.save(model.state_dict(), os.path.join(ckpt_dir, "ckpt_%d.pth" % (epoch + 1)))
        line = dict({"train_%s" % k: v for k, v in stats.items()}, epoch=epoch, n_parameters=n_parameters)
        logs.append(line)
        print(json.dumps(line))
        with open(os.path.join(log_dir, "log.txt"), mode="a", encoding="utf-8") as f:
            f.write(json.dumps(line) + "\n")
    return logs


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    check_trainable(args.trainable)
    check_sync(args.trainable, args.sync, args.use_sound)
    _single_rank()
    if not torch.cuda.is_available():
        raise SystemExit("mspi_amd.train needs an MI355X (no CPU fallback)")
    import numpy as np
    from . import engine as E
    from . import inference as I
    from .avsp_dataloader import AudioVisualDataset
    torch.manual_seed(args.seed)
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    I.device = device
    I._RESOLUTION[:] = args.resolution
    model = I.build_model(args.model, args.resolution, weight=args.weights or None, use_sound=args.use_sound)
    E.autotune(False)      # the tail is re-packed at every step: nothing to tune once
    model.trainable(args.trainable, sync=args.sync)
    cfg = model.cfg
    cfg.DATA.USE_SOUND = bool(args.use_sound)
    batch = cfg.TRAIN.BATCH_SIZE if args.batch is None else args.batch
    data = AudioVisualDataset(args.path_data, args.dataset, args.split, args.clip_size, "train", args.use_sound,
                              tuple(args.resolution), batch_size=batch, generator=np.random.default_rng(args.seed),
                              workers=args.workers, device=device)
    os.makedirs(args.log_dir, exist_ok=True)
    return train(model, data, cfg, device, args.log_dir, args.start_epoch, args.save_ckpt_freq, args.gamma)


if __name__ == "__main__":
    main()
