"""Saliency metrics on the GPU: the reference's `utils/compute_saliency_metrics.py`
functions `kldiv`, `cc`, `similarity`, `nss` (same names, same [B,H,W] arguments, same batch-mean results) and the
bookkeeping of `utils/loss.py:SalLoss` -- all four metrics of a batch come from ONE launch of mspi_saliency_metrics.
`auc_judd`, `auc_shuff` and `ig` (:111-308 of the same file) have launches of their own; `SalEval` keeps all seven and
`validation_one_epoch` is the loop of the reference's `engine_train.py:84-125`.
The criterion is differentiable with respect to the log map (sal_loss, sal_loss_terms, SalLoss on an input that requires
grad: csrc/salloss.hip); everything else is evaluation only.  There is no CPU fallback."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import MspiError, check


def per_sample(pred, gt, fix=None, pred_is_log=False):
    """[B,4] tensor of (KL, CC, SIM, NSS) per sample; pred / gt / fix: [B,H,W] fp32 CUDA tensors."""
    lib = _lib.load()
    if not pred.is_cuda:
        raise MspiError("mspi_amd.metrics runs on the GPU only; there is no CPU fallback")
    if pred.shape != gt.shape or (fix is not None and fix.shape != pred.shape) or pred.dim() != 3:
        raise MspiError("metrics: pred %s, gt %s, fix %s must be equal [B,H,W] shapes" % (
            tuple(pred.shape), tuple(gt.shape), None if fix is None else tuple(fix.shape)))
    p, g = pred.float().contiguous(), gt.float().contiguous()
    f = None if fix is None else fix.float().contiguous()
    B, L = p.shape[0], p.shape[1] * p.shape[2]
    out = torch.empty(B, 4, dtype=torch.float32, device=p.device)
    check(lib.mspi_saliency_metrics(p.data_ptr(), g.data_ptr(), None if f is None else f.data_ptr(), out.data_ptr(), B, L,
                                    1 if pred_is_log else 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "mspi_saliency_metrics")
    return out


def kldiv(s_map, gt):
    return per_sample(s_map, gt)[:, 0].mean()


def cc(s_map, gt):
    return per_sample(s_map, gt)[:, 1].mean()


def similarity(s_map, gt):
    return per_sample(s_map, gt)[:, 2].mean()


def nss(s_map, gt):
    """gt is the fixation map here (compute_saliency_metrics.py:93-107)."""
    return per_sample(s_map, gt, fix=gt)[:, 3].mean()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _maps(what, *maps):
    """The float32, contiguous forms of equal-shaped [B,H,W] CUDA maps."""
    first = maps[0]
    if not all(torch.is_tensor(m) and m.is_cuda for m in maps):
        raise MspiError("mspi_amd.metrics.%s runs on the GPU only; there is no CPU fallback" % what)
    if first.dim() != 3 or any(m.shape != first.shape for m in maps):
        raise MspiError("%s: maps must have equal [B,H,W] shapes, got %s (resizing the saliency map to the fixation map's "
                        "size, cv2.resize upstream, is not done here)" % (what, [tuple(m.shape) for m in maps]))
    return [m.float().contiguous() for m in maps]


def auc_judd_per_sample(saliencyMap, fixationMap, jitter=True, generator=None, return_counts=False):
    """float64 [B]: AUC-Judd of every map (compute_saliency_metrics.py:111-203; upstream looks at sample 0 only), NaN for a
    map without fixations or a constant map.  A pixel is a fixation where fixationMap > 0.  See auc_judd for `jitter`.
    return_counts: also the int32 [B] numbers of fixations."""
    lib = _lib.load()
    s, f = _maps("auc_judd", saliencyMap, fixationMap)
    B, L = s.shape[0], s.shape[1] * s.shape[2]
    if jitter is False or jitter is None:
        is_f64 = 0
    else:
        if jitter is True:
            noise = torch.rand(s.shape, dtype=torch.float64, device=s.device, generator=generator)
        else:
            noise = jitter
            if not (torch.is_tensor(noise) and noise.is_cuda and noise.dtype == torch.float64 and noise.shape == s.shape):
                raise MspiError("auc_judd: jitter must be False, True or a float64 CUDA tensor of the maps' shape")
        s = (s.double() + noise / 10 ** 7).contiguous()          # :150 -- numpy promotes the map to float64 there
        is_f64 = 1
    score = torch.empty(B, dtype=torch.float64, device=s.device)
    nfix = torch.empty(B, dtype=torch.int32, device=s.device)
    ws = torch.empty(lib.mspi_saliency_auc_ws_bytes(B, L), dtype=torch.uint8, device=s.device)
    check(lib.mspi_saliency_auc_judd(s.data_ptr(), is_f64, f.data_ptr(), score.data_ptr(), nfix.data_ptr(), ws.data_ptr(), B, L,
                                     _stream()), "mspi_saliency_auc_judd")
    return (score, nfix) if return_counts else score


def auc_judd(saliencyMap, fixationMap, jitter=True, generator=None):
    """compute_saliency_metrics.py:111-203: the mean AUC-Judd over the samples whose score is not NaN (for B = 1 the
    reference's value; NaN if every sample is NaN), a float64 scalar tensor on the device.

    jitter=True (the default, as upstream) adds noise / 10**7 to the map before it is normalised, which breaks the ties of
    quantised maps: a 256-level map scores differently with and without it.  Upstream draws the noise from numpy's global
    RNG (np.random.random); here it is torch.rand(float64) on the device from `generator` (a CUDA generator; None: the
    device's default one), so a seeded generator makes the score repeatable.  jitter=<float64 CUDA tensor [B,H,W]> uses
    that noise (the reference's own draw, for a bit-level comparison); jitter=False keeps the map in float32, as upstream."""
    return torch.nanmean(auc_judd_per_sample(saliencyMap, fixationMap, jitter, generator))


def sauc_counts(s_map, gt, other_map):
    """int32 [B,20] from one launch of mspi_saliency_sauc_counts: per map #{s >= k/10 and gt == 1} for k = 1..9, #{r > k/10}
    over the other-fixations' looked-up values r, #{gt == 1}, #{other_map == 1}.  gt and other_map are binary maps."""
    lib = _lib.load()
    s, g, o = _maps("auc_shuff", s_map, gt, other_map)
    B, H, W = s.shape
    counts = torch.empty(B, 20, dtype=torch.int32, device=s.device)
    check(lib.mspi_saliency_sauc_counts(s.data_ptr(), g.data_ptr(), o.data_ptr(), counts.data_ptr(), B, H, W, _stream()),
          "mspi_saliency_sauc_counts")
    return counts


_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def _sauc_score(c):
    """compute_saliency_metrics.py:254-274 on one map's counts, in the reference's own scalar types: its num_fixations is
    np.sum of a float32 map, so tp and fp are float32 quotients before round(x, 4)."""
    if c[18] == 0:
        return float("nan")
    nf = np.float32(c[18])
    area = [(0.0, 0.0)]
    for k in range(9):
        area.append((round(c[k] / (nf * 1.0), 4), round(c[9 + k] / (nf * 1.0), 4)))
    area.append((1.0, 1.0))
    area.sort(key=lambda p: p[0])
    return float(_trapezoid(np.array([p[0] for p in area]), np.array([p[1] for p in area])))


def auc_shuff_per_sample(s_map, gt, other_map, splits=100, stepsize=0.1):
    """float64 [B] on the maps' device: shuffled AUC of every map (compute_saliency_metrics.py:206-276; upstream looks at
    sample 0 only), NaN for a map without fixations.  The counting is one launch; round(x, 4), the sort of the 11 ROC
    points and the trapezoid are host float64 arithmetic on the 20 counts, so this call synchronises."""
    counts = sauc_counts(s_map, gt, other_map).cpu().tolist()
    return torch.tensor([_sauc_score(c) for c in counts], dtype=torch.float64, device=s_map.device)


def auc_shuff(s_map, gt, other_map, splits=100, stepsize=0.1):
    """compute_saliency_metrics.py:206-276: the mean over the samples that are not NaN.  `splits` and `stepsize` are
    accepted and ignored: every split of the reference permutes ALL other-fixations and then only counts how many of
    their values exceed each threshold, so the 100 splits are equal and the result does not depend on the random state;
    `stepsize` is never read upstream (the thresholds are the literals 0.1 .. 0.9).  As upstream, fp is divided by the
    number of true fixations, so the score can leave [0, 1]; H > W is refused (upstream raises IndexError)."""
    return torch.nanmean(auc_shuff_per_sample(s_map, gt, other_map))


def ig_per_sample(s_map, gt, baseline):
    """float32 [B]: information gain of every map over the baseline map (compute_saliency_metrics.py:278-308)."""
    lib = _lib.load()
    s, g, b = _maps("ig", s_map, gt, baseline)
    B, L = s.shape[0], s.shape[1] * s.shape[2]
    out = torch.empty(B, dtype=torch.float32, device=s.device)
    check(lib.mspi_saliency_ig(s.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), B, L, _stream()), "mspi_saliency_ig")
    return out


def ig(s_map, gt, baseline):
    return ig_per_sample(s_map, gt, baseline).mean()


class _Avg:
    def __init__(self):
        self.sum, self.count, self.val = 0.0, 0, 0.0

    def update(self, v, n=1):
        self.val = float(v)
        self.sum += float(v) * n
        self.count += n

    @property
    def avg(self):
        return self.sum / max(self.count, 1)


SAL_LOSS_CHUNK = 2048      # values per workgroup of mspi_saliency_loss_fwd (csrc/salloss.hip SL_C)


def _loss_fwd(x, g, f):
    """(terms [B,4], ws) of one mspi_saliency_loss_fwd; x / g / f: contiguous float32 [B,H,W] CUDA tensors (f may be None)."""
    lib = _lib.load()
    B, L = x.shape[0], x.shape[1] * x.shape[2]
    terms = torch.empty(B, 4, dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.mspi_saliency_loss_ws_bytes(B, L), dtype=torch.uint8, device=x.device)
    check(lib.mspi_saliency_loss_fwd(x.data_ptr(), g.data_ptr(), None if f is None else f.data_ptr(), terms.data_ptr(),
                                     ws.data_ptr(), B, L, _stream()), "mspi_saliency_loss_fwd")
    return terms, ws


def _loss_bwd(x, g, f, ws, grad_out, w_kl, w_cc, w_nss):
    """dlog [B,H,W] of one mspi_saliency_loss_bwd; grad_out: a float32 scalar on the device."""
    lib = _lib.load()
    B, L = x.shape[0], x.shape[1] * x.shape[2]
    go = grad_out.to(torch.float32).contiguous()
    dlog = torch.empty_like(x)
    check(lib.mspi_saliency_loss_bwd(x.data_ptr(), g.data_ptr(), None if f is None else f.data_ptr(), ws.data_ptr(), go.data_ptr(),
                                     w_kl, w_cc, w_nss, dlog.data_ptr(), B, L, _stream()), "mspi_saliency_loss_bwd")
    return dlog


def _no_double_backward():
    if torch.is_grad_enabled():        # the engine enables grad inside backward only for create_graph=True
        raise MspiError("mspi_amd.metrics: the saliency loss has no double backward (create_graph=True is not supported)")


def _loss_inputs(what, log_map, density, fixations):
    if not torch.is_tensor(log_map) or log_map.dtype != torch.float32:
        raise MspiError("%s: the log map must be a float32 tensor" % what)
    maps = _maps(what, log_map, density) if fixations is None else _maps(what, log_map, density, fixations)
    return maps[0], maps[1], (maps[2] if fixations is not None else None)


class _SalLossFn(torch.autograd.Function):
    """loss = sum_n (w_kl KL_n - w_cc CC_n - w_nss NSS_n) and the [B,4] terms (not differentiable here: the loss carries
    the gradient), one forward and one backward launch group.  The gradient goes to the log map only."""

    @staticmethod
    def forward(ctx, log_map, density, fixations, w_kl, w_cc, w_nss):
        x, g, f = _loss_inputs("sal_loss", log_map, density, fixations)
        terms, ws = _loss_fwd(x, g, f)
        t = terms.sum(0)
        loss = t[0] * w_kl - t[1] * w_cc
        if f is not None:
            loss = loss - t[3] * w_nss
        ctx.save_for_backward(x, g, f, ws)
        ctx.weights = (float(w_kl), float(w_cc), float(w_nss) if f is not None else 0.0)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        _no_double_backward()
        x, g, f, ws = ctx.saved_tensors
        return _loss_bwd(x, g, f, ws, grad_loss, *ctx.weights), None, None, None, None, None


class _SalTermsFn(torch.autograd.Function):
    """The [B,4] terms with a gradient of their own: any weighting per sample and term.  The kernel takes one device scalar
    and three host weights, so the backward is one launch per term (KL, CC, NSS) scaled by that term's column of the
    incoming gradient.  SIM is a reported value without a gradient, as in the loss."""

    @staticmethod
    def forward(ctx, log_map, density, fixations):
        x, g, f = _loss_inputs("sal_loss_terms", log_map, density, fixations)
        terms, ws = _loss_fwd(x, g, f)
        ctx.save_for_backward(x, g, f, ws)
        return terms

    @staticmethod
    def backward(ctx, grad_terms):
        _no_double_backward()
        x, g, f, ws = ctx.saved_tensors
        one = torch.ones((), dtype=torch.float32, device=x.device)
        out = None
        for col, w in ((0, (1.0, 0.0, 0.0)), (1, (0.0, -1.0, 0.0)), (3, (0.0, 0.0, -1.0))):
            if col == 3 and f is None:
                continue
            d = _loss_bwd(x, g, f, ws, one, *w).mul_(grad_terms[:, col].to(torch.float32).view(-1, 1, 1))
            out = d if out is None else out.add_(d)
        return out, None, None


def sal_loss(log_map, density, fixations=None, w_kl=1.0, w_cc=1.0, w_nss=0.1):
    """(loss, terms): loss = mean over the batch of w_kl KL - w_cc CC [- w_nss NSS] as a 0-dim device tensor with a
    grad_fn, terms the [B,4] per-sample (KL, CC, SIM, NSS) without one.  No host synchronisation: the pair of launches can
    be captured in a graph.  Non-contiguous inputs are made contiguous; the gradient comes back in the input's shape."""
    B = log_map.shape[0] if torch.is_tensor(log_map) and log_map.dim() else 1
    return _SalLossFn.apply(log_map, density, fixations, w_kl / B, w_cc / B, w_nss / B)


def sal_loss_terms(log_map, density, fixations=None):
    """[B,4] per-sample (KL, CC, SIM, NSS) of a log map, connected to the graph: the values of
    per_sample(..., pred_is_log=True) from the chunked kernels, differentiable with respect to the log map in the KL, CC
    and NSS columns (SIM counts as a constant)."""
    return _SalTermsFn.apply(log_map, density, fixations)


class SalLoss:
    """utils/loss.py:6-49: forward(log_map, density[, fixations]) -> kl - cc [- 0.1 nss], with running averages of every
    term in .log (timm's AverageMeter upstream).  With grad enabled and a log map that requires grad the result is a
    0-dim device tensor with a grad_fn (sal_loss: hand-written forward and backward kernels); otherwise it is the
    evaluation path, one launch of mspi_saliency_metrics and a tensor without a graph."""

    def __init__(self):
        self.reset_records()

    def reset_records(self):
        self.log = {k: _Avg() for k in ("kl", "cc", "sim", "nss", "loss")}

    def forward(self, inputs, targets, fixations=None, targets2=None):
        graph = torch.is_grad_enabled() and torch.is_tensor(inputs) and inputs.requires_grad
        if graph:
            out, terms = sal_loss(inputs, targets, fixations)
            m = terms.mean(0)
        else:
            m = per_sample(inputs, targets, fix=fixations, pred_is_log=True).mean(0)
        kl, c, sim, ns = (float(v) for v in m.tolist())          # the one host read (upstream's .item() calls)
        loss = kl - c - (0.1 * ns if fixations is not None else 0.0)
        self.log["kl"].update(kl)
        self.log["cc"].update(c)
        self.log["sim"].update(sim)
        if fixations is not None:
            self.log["nss"].update(ns)
        self.log["loss"].update(loss)
        return out if graph else torch.tensor(loss, device=inputs.device)

    __call__ = forward


class SalEval:
    """Running means of all seven metrics over a dataset.  update() takes the model's LOG map, exponentiates it once on
    the device and runs the launches; per metric, samples whose value is NaN (AUC without fixations, constant maps) are
    left out of the mean and counted in .nan.  Keys: kl, cc, sim (always); nss, auc_j (with fixations); s_auc (with
    fixations and other-fixations); ig (with a baseline map; its `gt` is the fixation map if given, else the density)."""
    KEYS = ("kl", "cc", "sim", "nss", "auc_j", "s_auc", "ig")

    def __init__(self, jitter=True, generator=None):
        self.jitter, self.generator = jitter, generator
        self.reset()

    def reset(self):
        self.sum = {k: 0.0 for k in self.KEYS}
        self.count = {k: 0 for k in self.KEYS}
        self.nan = {k: 0 for k in self.KEYS}

    def _add(self, key, values):
        for v in values:
            if math.isnan(v):
                self.nan[key] += 1
            else:
                self.sum[key] += v
                self.count[key] += 1

    def update(self, log_map, density, fixations=None, other=None, baseline=None):
        s = log_map.float().exp()
        vals = {}
        m = per_sample(s, density, fix=fixations)
        vals["kl"], vals["cc"], vals["sim"] = m[:, 0], m[:, 1], m[:, 2]
        if fixations is not None:
            vals["nss"] = m[:, 3]
            vals["auc_j"] = auc_judd_per_sample(s, fixations, self.jitter, self.generator)
            if other is not None:
                vals["s_auc"] = sauc_counts(s, fixations, other)
        if baseline is not None:
            vals["ig"] = ig_per_sample(s, density if fixations is None else fixations, baseline)
        for k, v in vals.items():            # the launches are all queued before the first copy to the host waits
            v = v.cpu().tolist()
            self._add(k, [_sauc_score(c) for c in v] if k == "s_auc" else v)

    def result(self):
        """{metric: mean over its samples that were not NaN} for every metric that has been fed."""
        return {k: (self.sum[k] / self.count[k] if self.count[k] else float("nan"))
                for k in self.KEYS if self.count[k] + self.nan[k]}


@torch.no_grad()
def validation_one_epoch(model, data_loader, device, cfg):
    """engine_train.py:84-125: the same loop over (imgs, audio, label) batches -- (imgs, label) without cfg.DATA.USE_SOUND --
    and the same returned keys, loss / kld / cc / sim as averages over the batches of SalLoss's per-batch values.  A
    loader whose batches go on with (fixations[, other_fixations[, baseline]]) after the label also gets SalEval's
    per-sample means under nss / auc_j / s_auc / ig."""
    criterion = SalLoss()
    extra = SalEval()
    meters = {k: _Avg() for k in ("loss", "kld", "cc", "sim")}
    model.eval()
    n_in = 2 if cfg.DATA.USE_SOUND else 1
    for batch_data in data_loader:
        batch = [t.to(device, non_blocking=True) for t in batch_data]
        inputs, label, rest = batch[:n_in], batch[n_in], batch[n_in + 1:]
        output, _ = model(*inputs)
        loss = criterion(output, label)
        meters["loss"].update(loss.item())
        meters["kld"].update(criterion.log["kl"].val)
        meters["cc"].update(criterion.log["cc"].val)
        meters["sim"].update(criterion.log["sim"].val)
        if rest:
            extra.update(output, label, *rest[:3])
    out = {k: m.avg for k, m in meters.items()}
    out.update({k: v for k, v in extra.result().items() if k not in ("kl", "cc", "sim")})
    return out
