"""submit() of a watch=-ed GraphPipeline against the same pipeline with the comparison switched off: 64 x 64 visual x3dl
model, depth 2, resident inputs, two batches in flight.
usage: python tools/pipeline_watch_time.py"""
import contextlib, io, json, os, statistics, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np, torch
from mspi_amd import engine as E
from mspi_amd import testing as T
from mspi_amd.model.model_utils import VisualSaliencyModel
from mspi_amd.runtime import GraphPipeline
dev = torch.device("cuda:0")
g = np.load(os.path.join(root, "tests", "golden", "vis_x3dl_64.npz"))
cfg = T.golden_cfg(g, "x3dl")
with contextlib.redirect_stdout(io.StringIO()):
    model = T.seeded(lambda: VisualSaliencyModel(cfg), 0).to(dev)
clips, _ = T.synth_inputs(int(g["batch"]), 16, 64, 64, Wa=111, seed=0, device=dev)
E.autotune(False)
fn = lambda c: model(c)[0]
fn(clips); torch.cuda.synchronize()
pipe = GraphPipeline(fn, (clips,), depth=2, layouts=1, watch=model)
watch = pipe._watch      # ONE pipeline (two captures land on different hardware queues and differ by 5 %): the check switched on / off
def loop(pipe, n=200):
    """steady state, two in flight: per-batch wall time and the host time of submit() alone"""
    t = [pipe.submit(), pipe.submit()]
    pipe.drain(); torch.cuda.synchronize()
    sub = []
    t0 = time.perf_counter()
    prev = None
    for i in range(n):
        a = time.perf_counter()
        tk = pipe.submit()
        sub.append(1e6 * (time.perf_counter() - a))
        if prev is not None:
            pipe.fetch(prev)
        prev = tk
    pipe.drain(); torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n, statistics.median(sub)
res = {"unwatched": [], "watched": []}
for rep in range(5):
    for k in ("unwatched", "watched"):
        pipe._watch = watch if k == "watched" else None
        res[k].append(loop(pipe))
for k, v in res.items():
    print(json.dumps({"pipeline": k, "reps": 5, "batches_per_rep": 200, "ms_per_batch": [round(a, 4) for a, _ in v],
                      "submit_host_us_median": [round(b, 1) for _, b in v]}))
