"""Median eager forward of the x3dl audio-visual model, batch 8, 224 x 224, wa 300 (the bench geometry).
Two figures: each forward synchronised on its own (latency of one call) and forwards back to back with one synchronise
at the end (bench.py --eager's way).  TREE_ROOT: the checkout whose mspi_amd is measured, so that two commits can be timed
alternately in one session.
usage: python tools/eager_forward_time.py TREE_ROOT LABEL [N]"""
import contextlib, io, json, statistics, sys, time
root, label = sys.argv[1], sys.argv[2]
n = int(sys.argv[3]) if len(sys.argv) > 3 else 60
sys.path.insert(0, root)
import torch
from mspi_amd import engine as E
from mspi_amd import testing as T
from mspi_amd.model.model_utils import AudioVisualSaliencyModel
import mspi_amd
assert mspi_amd.__file__.startswith(root), mspi_amd.__file__
dev = torch.device("cuda:0")
S, wa, B = 224, 300, 8
cfg = T.make_cfg("x3dl", num_aud_tokens=9 * ((wa + 31) // 32), num_vis_tokens=16 * (S // 32) ** 2)
with contextlib.redirect_stdout(io.StringIO()):
    model = T.seeded(lambda: AudioVisualSaliencyModel(cfg), 0).to(dev)
clips, audio = T.synth_inputs(B, 16, S, S, Wa=wa, seed=100, device=dev)
E.autotune(True)
model(clips, audio)
E.autotune(False)
for _ in range(8):
    model(clips, audio)
torch.cuda.synchronize()
wall, host = [], []
for _ in range(n):
    t0 = time.perf_counter()
    model(clips, audio)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    wall.append(1e3 * (t2 - t0)); host.append(1e3 * (t1 - t0))
# bench.py --eager's way: forwards back to back, one synchronize at the end
b2b = []
for _ in range(7):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(40):
        model(clips, audio)
    torch.cuda.synchronize()
    b2b.append(1e3 * (time.perf_counter() - t0) / 40)
q = statistics.quantiles(wall, n=4)
print(json.dumps({"label": label, "n": n, "wall_ms_median": round(statistics.median(wall), 3), "wall_ms_q1": round(q[0], 3),
                  "wall_ms_q3": round(q[2], 3), "wall_ms_min": round(min(wall), 3), "host_ms_median": round(statistics.median(host), 3),
                  "back_to_back_ms": [round(v, 3) for v in b2b], "back_to_back_ms_median": round(statistics.median(b2b), 3)}))
