"""Whole models through the production launch path: hipGraph capture with the model's _Fork side streams as parallel
branches, replayed with several batches in flight (mspi_amd.runtime.GraphPipeline -- what bench.py and inference.py --graph
run; neither ever launches eagerly).

For every motion encoder and the visual-only model, on the configuration and inputs of its smallest model-level fixture
(test_parity_gpu._build), with three input sets (seeds s, s + 1, s + 2) and BOTH results of the forward, the fp32 log map and
the loss tensor (the loss is the value computed on the re-forked side stream; bench's lambda drops it):
  1. eager, forked (_Fork.ENABLED, the default)  ==  eager, linear (MSPI_STREAMS=0): streams change scheduling, never arithmetic;
  2. eager forked on the fixture's own inputs is inside the golden bar of test_audio_visual_model_vs_golden: the chain of
     equalities below is tied to the reference;
  3. forked graphs, depth 2 (bench.py's single-process path, the clip loop): sets 0, 1, 2, 0, 1 with two in flight, allocator
     churned between submits, every fetched map and loss bit-equal to the eager result of its input set;
  4. linear graphs, depth 3 (bench.py's multi-rank path): the same.
All comparisons are torch.equal: the kernels are bitwise repeatable and a replay runs the same kernels on the same data.
layouts=1 and the machine's default hardware-queue count throughout: no queue or graph setting is touched here.

The 224-pixel fixtures (mvit, swin, morphmlp) are already batch 1, and av_swin_t_224 carries the Swin depth override in its
fixture (swin_depths): nothing is cut further here."""
import time

import pytest
import torch

FIXTURES = [("av_x3dl_64", "x3dl", "AudioVisualSaliencyModel"), ("av_slowfast_64", "slowfast4x16", "AudioVisualSaliencyModel"),
            ("av_s3d_64", "s3d", "AudioVisualSaliencyModel"), ("av_uniformer_64", "uniformerb", "AudioVisualSaliencyModel"),
            ("av_mvit_224", "mvitv2s", "AudioVisualSaliencyModel"), ("av_swin_t_224", "videoswins", "AudioVisualSaliencyModel"),
            ("av_morphmlp_224", "morphmlps", "AudioVisualSaliencyModel"), ("vis_x3dl_64", "x3dl", "VisualSaliencyModel")]
ORDER = (0, 1, 2, 0, 1)      # input set of each submit: every slot of a depth-2 and of a depth-3 pipeline is reused


def test_fixture_list_covers_every_motion_encoder():
    """One fixture per motion encoder the model factory knows, plus the visual-only model."""
    from mspi_amd.config import cfg
    encoders = set(cfg.MODEL.MOTION_ENCODER_EMBEDS)
    named = {name for _, name, _ in FIXTURES}
    assert named <= encoders, "fixtures name unknown encoders: %s" % sorted(named - encoders)
    families = {"x3dl": "x3d", "slowfast4x16": "slowfast", "s3d": "s3d", "uniformerb": "uniformer", "mvitv2s": "mvit",
                "videoswins": "swin", "morphmlps": "morphmlp"}
    assert set(families) == named and len(set(families.values())) == 7
    assert sum(1 for _, _, cls in FIXTURES if cls == "VisualSaliencyModel") == 1
    assert len({case for case, _, _ in FIXTURES}) == len(FIXTURES)
    assert set(ORDER) == {0, 1, 2} and len(ORDER) > 3


def _churn(junk, i, dev):
    """test_full_size_determinism_under_allocator_churn's churn: odd-sized buffers come and go."""
    junk.append(torch.full((1 + (i * 7919) % 5000, 1031), float(i), device=dev))
    if len(junk) > 3:
        junk.pop(0)


def _same(got, want, what):
    for g, w, part in zip(got, want, ("map", "loss")):
        assert g.shape == w.shape and g.dtype == w.dtype, "%s %s: %s %s, eager %s %s" % (what, part, tuple(g.shape), g.dtype, tuple(w.shape), w.dtype)
        assert torch.equal(g, w), "%s: %s differs from the eager forward (max |d| %.3e)" % (what, part, (g.float() - w.float()).abs().max().item())


def _through_pipeline(fn, sets, want, depth, model, dev, what):
    from mspi_amd.runtime import GraphPipeline
    pipe = GraphPipeline(fn, sets[0], depth=depth, layouts=1, watch=model)
    assert pipe.depth == depth and pipe.layout == 0
    junk, tickets = [], []
    for i, k in enumerate(ORDER):      # up to `depth` in flight: fetch submit i-1 after submitting i, as test_runtime.py does
        tickets.append(pipe.submit(*sets[k]))
        _churn(junk, i, dev)
        if i:
            got = pipe.fetch(tickets[i - 1])
            _same(got if isinstance(got, tuple) else (got,), want[ORDER[i - 1]], "%s submit %d (set %d)" % (what, i - 1, ORDER[i - 1]))
    got = pipe.fetch(tickets[-1])
    _same(got if isinstance(got, tuple) else (got,), want[ORDER[-1]], "%s submit %d (set %d)" % (what, len(ORDER) - 1, ORDER[-1]))
    pipe.drain()
    return pipe


@pytest.mark.gpu
@pytest.mark.parametrize("case,name,cls", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_model_replay_equals_eager_forked_and_linear(dev, golden_dir, monkeypatch, case, name, cls):
    import test_parity_gpu as PG
    from mspi_amd import engine as E
    from mspi_amd import testing as T
    from mspi_amd.model.model_utils import _Fork
    from test_kernel_ledger import _guard
    g = PG._g(golden_dir, case)
    visual = cls == "VisualSaliencyModel"
    _guard(E, dev)
    moved, cache, attn = len(E.RANGE_CHECK["moved"]), dict(E.AUTOTUNE["cache"]), dict(E.ATTN_PREC)
    try:
        E.autotune(False)
        assert _Fork.ENABLED, "MSPI_STREAMS=0 in the environment: the forked forward is what this test is about"
        cfg, m, clips, audio = PG._build(g, name, cls, dev)
        H, W = T.golden_hw(g)
        seed = int(g["seed"])
        sets = [(clips,) if visual else (clips, audio)]
        for s in (seed + 1, seed + 2):
            c, a = T.synth_inputs(int(g["batch"]), 16, H, W, Wa=int(g["wa"]), seed=s, device=dev)
            sets.append((c,) if visual else (c, a))
        assert not torch.equal(sets[0][0], sets[1][0]) and not torch.equal(sets[1][0], sets[2][0])

        def fn(*t):      # the map and the loss tensor; the visual-only model has no loss (it returns the integer 0)
            out, loss = m(*t)
            return (out,) if visual else (out, loss)

        def eager():
            res = [tuple(t.clone() for t in fn(*s)) for s in sets]
            torch.cuda.synchronize()
            return res

        forked = eager()
        with monkeypatch.context() as mp:
            mp.setattr(_Fork, "ENABLED", False)
            linear = eager()
        for k in range(3):
            _same(linear[k], forked[k], "%s eager linear vs forked, set %d" % (case, k))
        assert not torch.equal(forked[0][0], forked[1][0]), "two input sets give one map: the comparisons below would be vacuous"

        # the golden bar of test_parity_gpu.py on the fixture's own inputs
        err = (forked[0][0].cpu() - torch.as_tensor(g["out"])).abs().max().item()
        assert err < PG.MAP_TOL, "max-abs map error %.3e" % err
        if not visual:
            loss = forked[0][1].item()
            assert abs(loss - float(g["loss"])) < 1e-3 * max(abs(float(g["loss"])), 1e-2), (loss, float(g["loss"]))

        t0 = time.perf_counter()
        _through_pipeline(fn, sets, forked, 2, m, dev, "%s forked depth 2" % case)
        t1 = time.perf_counter()
        with monkeypatch.context() as mp:      # linear at capture time; a replay reads no switch
            mp.setattr(_Fork, "ENABLED", False)
            pipe = _through_pipeline(fn, sets, forked, 3, m, dev, "%s linear depth 3" % case)
        t2 = time.perf_counter()
        E.check_range(sync=False)
        assert not E.range_flag()
        del pipe
        print("%s: eager forked == eager linear; golden %.2f of the bar; forked depth 2 replays == eager (%.2f s capture + replay); "
              "linear depth 3 replays == eager (%.2f s)" % (case, err / PG.MAP_TOL, t1 - t0, t2 - t1))
    finally:
        E.autotune(False)
        del E.RANGE_CHECK["moved"][moved:]
        E.AUTOTUNE["cache"].clear()
        E.AUTOTUNE["cache"].update(cache)
        E.ATTN_PREC.clear()
        E.ATTN_PREC.update(attn)
