"""The shared pieces of the training path (mspi_amd/autograd.py): the stage ladder, the sliced wide weight gradient and the
BatchNorm-train helper.

CPU: the cutters' arithmetic, with the model's own widths pinned (they fix the launch count of a training step), and the ladder
against the counts the per-stage tests assert one by one.  GPU: wgrad_wide_sliced against float64 torch autograd on the CPU at
30 rows (B=1, T=2, h=3, w=5: less than one 128-row box) with the error measure and bound of tests/test_readout_train.py --
max |got - ref| / max |ref| <= GRAD_TOL = 2e-5 -- on widths that cut x, dy, both, and a strided view; bn_relu_train against
float64 batch norm + ReLU and nn.BatchNorm3d's running statistics with that file's BatchNorm bounds (GRAD_TOL relative, the mean
within GRAD_TOL * max(1, |mean|))."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_readout_train import GRAD_TOL, _cl, _err

NAMES = ("readout_tail", "readout", "fusion", "lateral_blocks", "lateral_entries", "adapter")
STOPS = (True, "maps", "laterals", "entries", "inputs", "cat")
SHAPE = (1, 2, 3, 5)                            # B, T, h, w: 30 rows


def test_wide_cut_tiles_every_width():
    from mspi_amd import autograd as A
    for c in range(32, 1025, 32):
        cut = A._wide_cut(c)
        assert [c0 for c0, _ in cut] == [sum(w for _, w in cut[:i]) for i in range(len(cut))] and sum(w for _, w in cut) == c, (c, cut)
        assert all(w % 32 == 0 and 0 < w <= A.WGRAD_WIDE_MAX_CH for _, w in cut), (c, cut)
        assert len(cut) == math.ceil(c / 192), (c, cut)


def test_wide_cut_of_the_models_widths():
    """What the 192-step loops gave on the widths the model has: the launches of a training step."""
    from mspi_amd import autograd as A
    assert [w for _, w in A._wide_cut(384)] == [192, 192]
    assert [w for _, w in A._wide_cut(416)] == [160, 160, 96]
    assert [w for _, w in A._wide_cut(512)] == [192, 192, 128]
    assert [w for _, w in A._wide_cut(768)] == [192, 192, 192, 192]
    assert all(A._wide_cut(c) == [(0, c)] for c in range(32, 193, 32))


def test_bn_slices_tile_every_width():
    from mspi_amd import autograd as A
    for c in range(16, 417, 4):
        cut = A._bn_slices(c)
        assert [c0 for c0, _ in cut] == [sum(w for _, w in cut[:i]) for i in range(len(cut))] and sum(w for _, w in cut) == c, (c, cut)
        assert all(w % 4 == 0 and 0 < w <= A.BN_MAX_CH for _, w in cut), (c, cut)
    assert A._bn_slices(208) == [(0, 104), (104, 104)]


def test_stage_ladder_and_what_follows_from_it():
    from mspi_amd import autograd as A
    from mspi_amd import testing as T
    from mspi_amd import train
    from mspi_amd.model import model_utils as pm
    assert A.STAGE_NAMES == NAMES and tuple(s.name for s in A.STAGES) == NAMES
    assert tuple(s.stop for s in A.STAGES) == STOPS and A.STAGES[0].stop is True
    assert [A.stage_rank(n) for n in NAMES] == [A.stage_rank(s) for s in STOPS] == list(range(6))
    assert A.stage_rank(None) == A.stage_rank(False) == -1 and not A.reaches(False, "readout_tail") and A.reaches("cat", "adapter")
    assert train.TRAINABLE == NAMES[:2] == ("readout_tail", "readout") and train.TRAINABLE_STAGES == NAMES[:3]
    assert train.TRAINABLE_BLOCKS == NAMES[3:4] == ("lateral_blocks",) and train.TRAINABLE_ENTRIES == NAMES[4:5] == ("lateral_entries",)
    assert train.TRAINABLE_ADAPTER == NAMES[5:] == ("adapter",)
    m = T.seeded(lambda: pm.AudioVisualSaliencyModel(T.make_cfg("x3dl")), 0)
    assert m.TAIL_PARAMS == A.STAGES[0].params and len(m.TAIL_PARAMS) == 6
    for name, stop, params, batch_stat in zip(NAMES, STOPS, (6, 16, 31, 71, 83, 107), (0, 2, 5, 5, 5, 13)):
        m.trainable(name)
        assert sum(p.requires_grad for p in m.parameters()) == params, name
        mods = m._batch_stat_modules()
        assert len(mods) == batch_stat and all(isinstance(b, torch.nn.BatchNorm3d) for b in mods.values()), name
        assert m._training_tail() == stop and (stop is not True or m._training_tail() is True), name
    m.trainable(None)
    assert m._training_tail() is False and not m._batch_stat_modules()


# name: (Ci, Co, kernel, padding, ld of the buffer x is a channel slice of, calls of the kernel)
WGRAD = {"x_sliced_uneven": (224, 32, (1, 1, 1), (0, 0, 0), None, 2), "dy_sliced": (32, 224, (1, 1, 1), (0, 0, 0), None, 2),
         "strided_view_333": (224, 96, (3, 3, 3), (1, 1, 1), 256, 2), "both_sliced_133": (224, 224, (1, 3, 3), (0, 1, 1), None, 4)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(WGRAD))
def test_hip_wgrad_wide_sliced_vs_fp64_autograd(dev, monkeypatch, case):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    Ci, Co, k, pad, ld, calls = WGRAD[case]
    B, T, h, w = SHAPE
    gen = torch.Generator().manual_seed(2100 + sorted(WGRAD).index(case))
    x, dy = torch.randn(B, Ci, T, h, w, generator=gen), torch.randn(B, Co, T, h, w, generator=gen)
    wt = torch.zeros(Co, Ci, *k, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    (F.conv3d(x.double(), wt, bias, padding=pad) * dy.double()).sum().backward()
    launched = []
    inner = E.conv_wgrad_wide
    monkeypatch.setattr(E, "conv_wgrad_wide", lambda xs, ds, geo: launched.append((xs.C, ds.C)) or inner(xs, ds, geo))
    dW, db = A.wgrad_wide_sliced(_cl(x, dev, ld), _cl(dy, dev), k, pad)
    torch.cuda.synchronize()
    assert torch.isfinite(dW).all() and torch.isfinite(db).all()
    e_w, e_b = _err(dW, wt.grad), _err(db, bias.grad)
    print("%s: dW %.2e, db %.2e of the largest entry; slices %s" % (case, e_w, e_b, launched))
    assert launched == [(ci, co) for _, co in A._wide_cut(Co) for _, ci in A._wide_cut(Ci)] and len(launched) == calls
    assert e_w <= GRAD_TOL and e_b <= GRAD_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("eps,momentum", [(1e-5, 0.1), (1e-3, 0.001)])
@pytest.mark.parametrize("C", [96, 208])
def test_hip_bn_relu_train_vs_fp64_batch_norm(dev, monkeypatch, C, eps, momentum):
    from mspi_amd import autograd as A
    from mspi_amd import engine as E
    B, T, h, w = SHAPE
    gen = torch.Generator().manual_seed(2200 + C)
    x = torch.randn(B, C, T, h, w, generator=gen) * torch.logspace(-1.0, 1.0, C).view(1, C, 1, 1, 1) + torch.linspace(-5.0, 5.0, C).view(1, C, 1, 1, 1)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    bn = torch.nn.BatchNorm3d(C, eps=eps, momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        ref = torch.relu(bn(x.double()))
    xd = x.double().transpose(0, 1).flatten(1)
    m_ref, v_ref = xd.mean(1), xd.var(1, unbiased=False)
    seen = []
    inner = E.bn_stats
    monkeypatch.setattr(E, "bn_stats", lambda xs, e: seen.append(inner(xs, e)) or seen[-1])
    wide = None
    if C > A.BN_MAX_CH:       # out: a channel slice of a 512-wide buffer, as the adapter's branches write theirs
        wide = E.alloc(B, T, h, w, 512, dev)
        wide.buf.fill_(float("nan"))
    y, mean, var, rstd = A.bn_relu_train(_cl(x, dev), gamma.to(dev), beta.to(dev), eps, out=None if wide is None else wide.slice(192, C))
    buffers = (torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), dtype=torch.long, device=dev))
    A._bn_running(buffers, mean, var, B * T * h * w, momentum)
    torch.cuda.synchronize()
    if wide is None:          # one slice: the kernel's own vectors, no copies
        assert len(seen) == 1 and mean is seen[0][0] and var is seen[0][1] and rstd is seen[0][2]
    else:
        assert [s[0].numel() for s in seen] == [104, 104] and y.buf is wide.buf
        rest = wide.as_rows(512)
        assert torch.isnan(rest[:, :192]).all() and torch.isnan(rest[:, 192 + C:]).all()
    errs = {"y": _err(y.as_ncdhw(), ref), "var": _err(var, v_ref), "rstd": _err(rstd, 1.0 / torch.sqrt(v_ref + eps)),
            "running_var": _err(buffers[1], bn.running_var)}
    e_mean = (mean.double().cpu() - m_ref).abs().max().item()
    e_rm = (buffers[0].double().cpu() - bn.running_mean).abs().max().item()
    print("C = %d eps %g: %s, mean %.2e, running_mean %.2e" % (C, eps, {k: "%.2e" % v for k, v in errs.items()}, e_mean, e_rm))
    assert e_mean <= GRAD_TOL * max(1.0, m_ref.abs().max().item())
    assert e_rm <= GRAD_TOL * max(1.0, bn.running_mean.abs().max().item())
    assert all(e <= GRAD_TOL for e in errs.values()), errs
    assert int(buffers[2]) == int(bn.num_batches_tracked) == 1
