"""Packed plans (HipModule.pk) must follow the parameters: whatever changes a parameter or a buffer -- a load_state_dict
into the model, a sub-module or a plain container, a backbone's load_weight, .to() / .double().float(), an optimiser step,
any in-place write -- the next `pk` access and the next forward use plans built from the present values.

Every comparison is an equality.  On the CPU a crc32 fingerprint of every tensor of every plan is compared with that of
a fresh model (a copy of a model that never built a plan) which was given the same parameters before its first `pk`; on the
GPU the forward is compared bit for bit with such a fresh model's, autotune off, so that the same parameters launch the same
kernels."""
import contextlib
import copy
import io
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn


# ------------------------------------------------------------------------------- helpers
def _owners(model):
    from mspi_amd.module import HipModule
    return [(n, m) for n, m in model.named_modules() if isinstance(m, HipModule) and type(m)._pack is not HipModule._pack]


def _crc(o, acc, path):
    """crc32 over the bytes of every tensor reachable from plan object `o`, in walk order: dicts, lists, tuples and pack
    objects (through __slots__ / __dict__); never into an nn.Module."""
    if isinstance(o, nn.Module) or o is None or isinstance(o, (str, bytes, int, float, bool, type)) or callable(o):
        return acc
    if torch.is_tensor(o):
        a = np.ascontiguousarray(o.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy()) if o.numel() else b""
        return zlib.crc32(a, acc)
    if id(o) in path:
        return acc
    path = path | {id(o)}
    if isinstance(o, dict):
        items = list(o.values())
    elif isinstance(o, (list, tuple)):
        items = list(o)
    else:
        items = [getattr(o, s) for c in type(o).__mro__ for s in getattr(c, "__slots__", ()) if hasattr(o, s)]
        items += list(getattr(o, "__dict__", {}).values())
    for v in items:
        acc = _crc(v, acc, path)
    return acc


def pack_fingerprint(model):
    """{module name: crc32 of its plan's tensors} for every HipModule of `model` that has a _pack (builds missing plans)."""
    return {n: _crc(m.pk, 0, frozenset()) for n, m in _owners(model)}


def _plan_tensors(o, out, path=frozenset()):
    """The plan's tensor OBJECTS, in the fingerprint's walk order."""
    if isinstance(o, nn.Module) or o is None or isinstance(o, (str, bytes, int, float, bool, type)) or callable(o):
        return out
    if torch.is_tensor(o):
        out.append(o)
        return out
    if id(o) in path:
        return out
    path = path | {id(o)}
    if isinstance(o, dict):
        items = list(o.values())
    elif isinstance(o, (list, tuple)):
        items = list(o)
    else:
        items = [getattr(o, s) for c in type(o).__mro__ for s in getattr(c, "__slots__", ()) if hasattr(o, s)]
        items += list(getattr(o, "__dict__", {}).values())
    for v in items:
        _plan_tensors(v, out, path)
    return out


def _packed(plan):
    """Tensors of a plan that the plan owns (a LayerNorm's weight, float and contiguous already, is handed on as it is)."""
    return [t for t in _plan_tensors(plan, []) if not isinstance(t, nn.Parameter)]


def _get(model, name):
    return model.get_submodule(name) if name else model


def _quiet(build):
    with contextlib.redirect_stdout(io.StringIO()):
        return build()


def _templates(golden_dir, case, cls):
    """Two models of the 64 x 64 fixture geometry, seeded 0 (A) and 1 (B), that never build a plan: a deepcopy of one is a
    fresh model."""
    from mspi_amd import testing as T
    from mspi_amd.model import model_utils as pm
    g = np.load(os.path.join(golden_dir, case + ".npz"))
    cfg = T.golden_cfg(g, "x3dl")
    a, b = (_quiet(lambda: T.seeded(lambda: getattr(pm, cls)(cfg), seed)) for seed in (0, 1))
    return {"g": g, "cfg": cfg, "A": a, "B": b}


@pytest.fixture(scope="module")
def vis(golden_dir):
    return _templates(golden_dir, "vis_x3dl_64", "VisualSaliencyModel")


@pytest.fixture(scope="module")
def av(golden_dir):
    return _templates(golden_dir, "av_x3dl_64", "AudioVisualSaliencyModel")


def _fresh(template, like=None):
    """A model without plans; like: give it that model's present parameters and buffers, tensor by tensor."""
    m = copy.deepcopy(template)
    assert not any("_pk" in x.__dict__ for x in m.modules())
    if like is not None:
        src = like.state_dict()
        with torch.no_grad():
            for k, v in m.state_dict().items():
                v.copy_(src[k])
    return m


def _check_follows(tpl, change, expect_change=True):
    """Steps 1-5 of every CPU case.  change(B, A) alters B's tensors; returns B."""
    B = _fresh(tpl["B"])
    before = pack_fingerprint(B)                     # touches every plan
    change(B, tpl["A"])
    after = pack_fingerprint(B)
    want = pack_fingerprint(_fresh(tpl["B"], like=B))
    stale = sorted(n for n in want if after[n] != want[n])
    assert not stale, "plans that do not follow the parameters: %r" % stale
    if expect_change:
        assert after != before, "the fingerprint does not see this change"
    return B


def _load_sub(name, strict=True):
    def change(B, A):
        _get(B, name).load_state_dict(_get(A, name).state_dict(), strict=strict)
    return change


# ------------------------------------------------------------------------------- CPU: load_state_dict
VIS_LOADS = ["", "sa_0", "latlayer_3", "readout", "visnet", "visnet.s3.pathway0_res2", "visnet.s3.pathway0_res2.branch2.a",
             "visnet.s1", "image_encoder", "adapter"]


@pytest.mark.parametrize("name", VIS_LOADS, ids=[n or "whole_model" for n in VIS_LOADS])
def test_plans_follow_load_state_dict(vis, name):
    _check_follows(vis, _load_sub(name))


@pytest.mark.parametrize("name", ["vis_projector", "mlp_aud", "aud_vis_sync_block", "audnet"])
def test_plans_follow_load_state_dict_audio_visual(av, name):
    _check_follows(av, _load_sub(name))


def test_plans_follow_load_weight(vis, tmp_path):
    """The PySlowFast '.pyth' layout ({'model_state': state_dict}, as tests/test_weights.py writes it) through
    visnet.load_weight after the plans exist: the root's laterals and every stage follow."""
    path = str(tmp_path / "x3d_l.pyth")
    torch.save({"model_state": {k: v.clone() for k, v in vis["A"].visnet.state_dict().items()}, "epoch": 300}, path)
    B = _check_follows(vis, lambda B, A: B.visnet.load_weight(path))
    for k, v in vis["A"].visnet.state_dict().items():
        assert torch.equal(B.visnet.state_dict()[k], v), k


# ------------------------------------------------------------------------------- CPU: _apply on a sub-module
@pytest.mark.parametrize("name", ["sa_1", "latlayer_2"])
def test_plans_are_rebuilt_after_apply_on_a_sub_module(vis, name):
    """.double().float() on a HipModule (sa_1) and on a plain Sequential that holds one (latlayer_2; nn.Module.to() takes no
    copy=True): the values stay, the storage is new.  Every plan that read the sub-module's tensors -- the root's sa_cat and
    lat, and the sub-module's own -- is built again, and no plan keeps a tensor that lies in the replaced storage."""
    B = _fresh(vis["B"])
    before = pack_fingerprint(B)
    sub = _get(B, name)
    floats = [t for t in list(sub.parameters()) + list(sub.buffers()) if t.is_floating_point()]
    old_ptrs = {t.data_ptr() for t in floats}
    old_storage = [t.untyped_storage() for t in floats]      # stays allocated: whatever lies at old_ptrs later is an alias of it
    inner = [m for _, m in _owners(sub)]
    assert inner
    kept = [t for m in inner for t in _packed(m.pk)] + _packed(B.pk["lat"]) + _packed(B.pk["sa_cat"])
    old = {id(t) for t in kept}                  # `kept` keeps them alive: no new tensor object can take one of these ids
    other = B.sa_0 if name != "sa_0" else B.sa_2
    untouched = _packed(other.pk)
    sub.double().float()
    live = {t.data_ptr() for t in list(B.parameters()) + list(B.buffers())}
    assert not (old_ptrs & live), "the storage was not re-created"
    for m in inner:
        assert not any(id(t) in old for t in _packed(m.pk)), type(m).__name__
    assert not any(id(t) in old for t in _packed(B.pk["lat"]) + _packed(B.pk["sa_cat"]))
    for n, m in _owners(B):
        assert not any(t.data_ptr() in old_ptrs for t in _plan_tensors(m.pk, [])), "%r keeps a tensor in the replaced storage" % n
    assert len(old_storage) == len(floats)
    assert all(a is b for a, b in zip(_packed(other.pk), untouched))      # and nothing else was rebuilt for it
    assert pack_fingerprint(B) == before                                   # same values: same plans


# ------------------------------------------------------------------------------- CPU: in-place writes
def test_plans_follow_an_in_place_scale_of_a_folded_conv(vis):
    def change(B, A):
        with torch.no_grad():
            B.sa_2.conv_mask[0].conv.weight.mul_(0.5)
    _check_follows(vis, change)


def test_plans_follow_a_write_to_a_folded_running_var(vis):
    def change(B, A):
        with torch.no_grad():
            B.sa_2.conv_mask[0].bn.running_var.copy_(A.sa_2.conv_mask[0].bn.running_var * 2.0)
    _check_follows(vis, change)


def test_plans_follow_an_optimiser_step_on_a_plain_container(vis):
    def change(B, A):
        params = list(B.latlayer_1.parameters())
        g = torch.Generator().manual_seed(5)
        for p in params:
            p.grad = torch.rand(p.shape, generator=g) - 0.5
        torch.optim.SGD(params, lr=0.1).step()
    _check_follows(vis, change)


def test_plans_follow_the_weight_broadcast(vis, monkeypatch):
    """sharding.broadcast_weights on a sub-module, single process: the collective is replaced by one that delivers model A's
    values for sa_1 (what rank 0 would send); the flat message is then written back in place, as on every rank."""
    from mspi_amd import sharding

    def change(B, A):
        sent = torch.cat([t.detach().reshape(-1) for t in list(A.sa_1.parameters()) + list(A.sa_1.buffers()) if t.is_floating_point()])
        monkeypatch.setattr(sharding.dist, "broadcast", lambda flat, src: flat.copy_(sent))
        assert sharding.broadcast_weights(B.sa_1) == sent.numel()
    _check_follows(vis, change)


# ------------------------------------------------------------------------------- CPU: no rebuild without a change
def test_no_rebuild_without_a_change(vis):
    B = _fresh(vis["B"])
    pack_fingerprint(B)
    for m in (B, B.visnet.s3, B.latlayer_3[2], B.image_encoder):
        first = _plan_tensors(m.pk, [])
        second = _plan_tensors(m.pk, [])
        assert len(first) > 0 and len(first) == len(second) and all(a is b for a, b in zip(first, second)), type(m).__name__
    # ... and the validated entry point of a forward does not rebuild either
    held = [_plan_tensors(m.pk, []) for m in (B, B.visnet.s3)]
    with getattr(B, "plans_checked", contextlib.nullcontext)():
        inside = [_plan_tensors(m.pk, []) for m in (B, B.visnet.s3)]
    for was, now in zip(held, inside):
        assert len(was) == len(now) and all(a is b for a, b in zip(was, now))


def test_a_load_into_one_model_leaves_the_other_models_plans(vis):
    A, B = _fresh(vis["A"]), _fresh(vis["B"])
    pack_fingerprint(A), pack_fingerprint(B)
    held = {n: _plan_tensors(m.pk, []) for n, m in _owners(B)}
    A.load_state_dict(B.state_dict())
    A.sa_0.load_state_dict(vis["A"].sa_0.state_dict())
    pack_fingerprint(A)
    for n, m in _owners(B):
        now = _plan_tensors(m.pk, [])
        assert len(now) == len(held[n]) and all(a is b for a, b in zip(now, held[n])), n


def test_pipeline_watch_is_optional_and_needs_no_gpu_to_refuse_host_inputs():
    from mspi_amd.runtime import GraphPipeline
    with pytest.raises(ValueError, match="device-resident"):
        GraphPipeline(lambda x: x, (torch.zeros(4),), watch=nn.Linear(2, 2))


# ------------------------------------------------------------------------------- GPU
def _inputs(tpl, dev):
    from mspi_amd import testing as T
    g = tpl["g"]
    H, W = T.golden_hw(g)
    return T.synth_inputs(int(g["batch"]), 16, H, W, Wa=int(g["wa"]), seed=int(g["seed"]), device=dev)


def _fwd(model, tpl, dev, sound):
    """(map, loss) of the 64 x 64 fixture inputs, clones (the next forward may reuse the memory)."""
    clips, audio = _inputs(tpl, dev)
    with torch.no_grad():
        y, loss = model(clips, audio) if sound else model(clips)
    return y.clone(), (loss.clone() if torch.is_tensor(loss) else loss)


def _same(a, b):
    return torch.equal(a[0], b[0]) and (torch.equal(a[1], b[1]) if torch.is_tensor(a[1]) else a[1] == b[1])


@pytest.fixture(scope="module")
def gpu_models(dev, vis, av):
    """One model A (seed 0) and one model B (seed 1) of each kind on the device, with B's seed-1 state kept for restoring."""
    from mspi_amd import engine as E
    E.autotune(False)
    out = {}
    for kind, tpl in (("vis", vis), ("av", av)):
        out[kind] = {"tpl": tpl, "A": _fresh(tpl["A"]).to(dev), "B": _fresh(tpl["B"]).to(dev), "sound": kind == "av",
                     "B0": {k: v.clone() for k, v in tpl["B"].state_dict().items()}}
    return out


def _restored_b(k):
    """Model B back at its seed-1 values, through the whole-model load (the owner's own subtree)."""
    k["B"].load_state_dict(k["B0"])
    return k["B"]


def _fresh_fwd(k, like, dev):
    return _fwd(_fresh(k["tpl"]["B"], like=like).to(dev), k["tpl"], dev, k["sound"])


@pytest.mark.gpu
def test_hip_loaders_reach_the_forward(dev, gpu_models, tmp_path):
    """VERDICT item 8 (f1 on the device): visnet.load_weight and the whole-model load_state_dict after the packs exist."""
    from mspi_amd import engine as E
    E.autotune(False)
    k = gpu_models["av"]
    A, B, tpl = k["A"], _restored_b(k), k["tpl"]
    pyth, plain = str(tmp_path / "x3d_l.pyth"), str(tmp_path / "ckpt.pth")
    torch.save({"model_state": {n: v.cpu() for n, v in A.visnet.state_dict().items()}}, pyth)
    torch.save({n: v.cpu() for n, v in A.state_dict().items()}, plain)
    want = _fwd(A, tpl, dev, True)
    first = _fwd(B, tpl, dev, True)                  # B's packs exist now
    assert not _same(first, want)
    with contextlib.redirect_stdout(io.StringIO()):
        B.visnet.load_weight(pyth)
    mixed = _fwd(B, tpl, dev, True)
    assert not _same(mixed, first) and not _same(mixed, want)
    assert _same(mixed, _fresh_fwd(k, B, dev)), "after load_weight the forward is not a fresh model's with B's weights + A's visnet"
    B.load_state_dict(torch.load(plain, map_location="cpu"))
    got = _fwd(B, tpl, dev, True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    E.check_range()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,name", [("vis", "sa_0"), ("vis", "latlayer_3"), ("vis", "visnet.s3.pathway0_res2"),
                                       ("av", "vis_projector")])
def test_hip_sub_module_load_changes_the_forward(dev, gpu_models, kind, name):
    from mspi_amd import engine as E
    E.autotune(False)
    k = gpu_models[kind]
    A, B, tpl, sound = k["A"], _restored_b(k), k["tpl"], k["sound"]
    before = _fwd(B, tpl, dev, sound)
    _get(B, name).load_state_dict(_get(A, name).state_dict())
    after = _fwd(B, tpl, dev, sound)
    want = _fresh_fwd(k, B, dev)
    if name == "vis_projector":                      # the contrastive branch: its value is the loss, the map does not read it
        assert torch.equal(after[1], want[1]) and not torch.equal(after[1], before[1])
        assert torch.equal(after[0], want[0])
    else:
        assert _same(after, want) and not torch.equal(after[0], before[0])
    E.check_range()


@pytest.mark.gpu
def test_hip_in_place_write_and_readout_step_reach_the_forward(dev, gpu_models, golden_dir):
    from mspi_amd import engine as E
    from mspi_amd import metrics as M
    from test_readout_tail import _batches
    E.autotune(False)
    k = gpu_models["vis"]
    B, tpl = _restored_b(k), k["tpl"]
    before = _fwd(B, tpl, dev, False)
    with torch.no_grad():
        B.sa_2.conv_mask[0].conv.weight.mul_(0.5)
    scaled = _fwd(B, tpl, dev, False)
    assert _same(scaled, _fresh_fwd(k, B, dev)) and not torch.equal(scaled[0], before[0])
    # one readout step as train.py takes it: trainable("readout"), AdamW over what requires grad, SalLoss
    clips, _ = _inputs(tpl, dev)
    B.trainable("readout")
    B.train()
    B.frozen_encoder()
    params = [p for p in B.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=0)
    label = _batches(clips, None, 1, False)[0][1].to(dev)
    out, _ = B(clips)
    opt.zero_grad()
    M.SalLoss()(out, label).backward()
    opt.step()
    B.trainable(None)
    B.eval()
    trained = _fwd(B, tpl, dev, False)
    assert not torch.equal(trained[0], scaled[0])
    fresh = _fresh(tpl["B"])
    fresh.load_state_dict(B.state_dict())
    assert _same(trained, _fwd(fresh.to(dev), tpl, dev, False))
    E.check_range()
    for p in params:
        p.grad = None


@pytest.mark.gpu
def test_hip_pipeline_refuses_to_replay_after_a_load(dev, gpu_models):
    from mspi_amd import engine as E
    from mspi_amd.runtime import GraphPipeline
    E.autotune(False)
    k = gpu_models["vis"]
    A, B, tpl = k["A"], _restored_b(k), k["tpl"]
    clips, _ = _inputs(tpl, dev)
    fn = lambda c: B(c)[0]                                        # noqa: E731
    eager = _fwd(B, tpl, dev, False)[0]
    pipe = GraphPipeline(fn, (clips,), depth=2, layouts=1, watch=B)
    assert torch.equal(pipe.fetch(pipe.submit()), eager)
    assert torch.equal(pipe.fetch(pipe.submit(clips)), eager)
    unwatched = GraphPipeline(fn, (clips,), depth=2, layouts=1)
    keep = [m.pk for _, m in _owners(B)]      # the buffers the captured graphs read stay allocated while they may be replayed
    B.sa_0.load_state_dict(A.sa_0.state_dict())
    for call in (lambda: pipe.submit(), lambda: pipe.submit_build(lambda ins: ins[0].copy_(clips)), lambda: pipe.submit(clips)):
        with pytest.raises(RuntimeError, match="changed after the capture.*build a new GraphPipeline"):
            call()
    pipe.drain()
    # without a watch nothing is compared: the old graphs replay the old packs, as they always did
    assert torch.equal(unwatched.fetch(unwatched.submit()), eager)
    unwatched.drain()
    del keep
    new = GraphPipeline(fn, (clips,), depth=2, layouts=1, watch=[B])
    want = _fresh_fwd(k, B, dev)[0]
    got = new.fetch(new.submit(clips))
    assert torch.equal(got, want) and not torch.equal(got, eager)
    new.drain()
    E.check_range()
