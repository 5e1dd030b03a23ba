"""The loops of the reference's engine_train.py: train_one_epoch (:11-81) and validation_one_epoch (:84-125, in
mspi_amd.metrics).  The criterion's backward runs on hand-written kernels (metrics.SalLoss); mspi_amd's own models have no
backward yet, so train_one_epoch serves models whose forward is differentiable by other means, for example a torch
module over frozen mspi_amd features.  Single process, single device."""
import math

import torch

from ._lib import MspiError
from .metrics import SalLoss, _Avg, validation_one_epoch  # noqa: F401  (SalLoss, validation_one_epoch: upstream's names here)


def get_grad_norm(parameters):
    """utils/log.py:163-175 at its default norm_type: the 2-norm of the parameters' present gradients, 0 if there is none.
    The per-parameter norms are gathered on the first gradient's device."""
    grads = [p.grad.detach() for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.)
    return torch.norm(torch.stack([torch.norm(g).to(grads[0].device) for g in grads]))


_CRITERION_KEYS = (("kld", "kl"), ("cc", "cc"), ("sim", "sim"), ("nss", "nss"))      # returned key, SalLoss.log key


def _optimizer_stats(optimizer):
    """lr (largest of the groups, at least 0), min_lr (smallest, at most 10) and weight_decay (the last group's that is
    above 0, else None): the three values upstream's loop logs from the optimizer at every step."""
    lrs = [group["lr"] for group in optimizer.param_groups]
    decays = [group["weight_decay"] for group in optimizer.param_groups if group["weight_decay"] > 0]
    return {"lr": max([0.] + lrs), "min_lr": min([10.] + lrs), "weight_decay": decays[-1] if decays else None}


def train_one_epoch(model, criterion, data_loader, optimizer, device, epoch, cfg, start_steps=None, update_freq=1, gamma=1.0):
    """engine_train.py:11-81: the same loop over (imgs, audio, label) batches -- (imgs, label) without cfg.DATA.USE_SOUND --
    and the same returned keys, averages over the batches: loss, kld, cc, sim, nss, lr, min_lr, grad_norm, and weight_decay
    if a parameter group has one above 0 (upstream's logger skips a None).  With sound the model's second output, times
    gamma, is added to the criterion's loss.  As upstream, grad_norm is read before zero_grad, so it reports the gradients
    of the previous step (0 at the first), and start_steps / update_freq only number the iterations.  A NaN loss raises.
    One summary line is printed."""
    model.train()
    if hasattr(model, "frozen_encoder"):
        model.frozen_encoder()
    meters = {}
    n_in = 2 if cfg.DATA.USE_SOUND else 1
    for batch_data in data_loader:
        batch = [t.to(device, non_blocking=True) for t in batch_data]
        output, aux = model(*batch[:n_in])
        loss = criterion(output, batch[n_in])
        if cfg.DATA.USE_SOUND:
            loss = loss + gamma * aux
        if not (torch.is_tensor(loss) and loss.requires_grad):
            raise MspiError("train_one_epoch: the loss has no grad_fn, so there is nothing to train: mspi_amd's own models have "
                            "no backward yet (their forward runs outside autograd); train a differentiable torch module, for "
                            "example one over frozen mspi_amd features")
        stats = {"loss": loss.item()}
        if math.isnan(stats["loss"]):
            raise Exception("Loss is NaN.")
        stats.update({k: criterion.log[name].val for k, name in _CRITERION_KEYS})
        stats.update(_optimizer_stats(optimizer))
        stats["grad_norm"] = get_grad_norm(model.parameters()).item()       # before zero_grad: the previous step's
        for k, v in stats.items():
            if v is not None:
                meters.setdefault(k, _Avg()).update(v)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
    out = {k: m.avg for k, m in meters.items()}
    print("Epoch: [%s] Averaged stats: %s" % (epoch, "  ".join("%s: %.6g" % kv for kv in out.items())))
    return out
