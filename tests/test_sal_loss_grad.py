"""The differentiable criterion (csrc/salloss.hip, metrics.sal_loss / sal_loss_terms / SalLoss, engine_train.train_one_epoch).

Yardsticks: tests/golden/saliency_loss.npz holds three small cases with the float64 terms of the reference's own
kldiv / cc / similarity / nss and the gradients autograd gives through them (tools/gen_loss_golden.py);
tests/sal_loss_restate.py is the CPU restatement (terms and ANALYTIC gradient) that the generator pinned to both and
that stands in for them on shapes too large to commit.

Bounds.  Terms: the sibling kernel's bar (tests/test_metrics.py), relative 2e-5 with a 1e-3 floor on small shapes, 1e-4 at
full size.  Gradient: max |dlog - ref| / max |ref| per sample <= 2e-5, the project's bar for these metrics; a float32
evaluation of the same formulas on the CPU sits at 1e-7 .. 1.2e-6 on every shape here, so the bar leaves room for
__expf and the reduction order and nothing else.  Losses of training loops: 1e-4 against float64, the project's
tolerance on the loss."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import sal_loss_restate as S
from oracle import restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mspi_saliency_loss_ws_bytes", "mspi_saliency_loss_fwd", "mspi_saliency_loss_bwd")
CASES = ("tiny", "odd", "quad")
SHAPES = {"tiny": (1, 5, 7), "odd": (3, 33, 31), "quad": (2, 40, 52)}
CHUNK = 2048
# either side of the chunk size: L = CHUNK - 1, CHUNK, CHUNK + 1
BOUNDARY = {CHUNK - 1: (23, 89), CHUNK: (32, 64), CHUNK + 1: (3, 683)}


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "saliency_loss.npz"))
    return {k: z[k] for k in z.files}


def _case(name):
    g = _gold()
    return (torch.from_numpy(g["%s_log_map" % name]), torch.from_numpy(g["%s_density" % name]),
            torch.from_numpy(g["%s_fix" % name].astype(np.float32)))


@functools.lru_cache(maxsize=None)
def _seeded(B, H, W, seed):
    """Inputs and their float64 yardsticks, computed once: (x, g, f, terms, grad, grad with fixations)."""
    x, g, f = (torch.from_numpy(a) for a in S.make_case(B, H, W, seed))
    return x, g, f, S.terms(x, g, f), S.loss_grad(x, g), S.loss_grad(x, g, f)


def _grad_err(got, ref):
    """max |got - ref| / max |ref| per sample, the largest over the batch."""
    got, ref = got.detach().double().cpu().flatten(1), ref.double().flatten(1)
    return ((got - ref).abs().max(1)[0] / ref.abs().max(1)[0]).max().item()


def _terms_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return ((got - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()


# ------------------------------------------------------------------------------------------------------------- CPU
def test_fixture_holds_the_named_cases():
    g = _gold()
    assert tuple(g["cases"]) == CASES
    for c in CASES:
        x, d, f = _case(c)
        assert tuple(x.shape) == SHAPES[c] and x.dtype == torch.float32 and g["%s_fix" % c].dtype == np.uint8
        assert (x.double().exp().flatten(1).sum(1) - 1).abs().max() < 1e-5          # a log-softmax map
        assert (d == 0).any() and d[d > 0].min() >= 1e-3                            # exact zeros in the density
        assert (f.flatten(1).sum(1) >= 1).all() and set(f.unique().tolist()) <= {0.0, 1.0}
        assert g["%s_terms" % c].dtype == np.float64 and g["%s_grad_fix" % c].dtype == np.float64


def test_restatement_matches_reference_values_and_gradients():
    g = _gold()
    for c in CASES:
        x, d, f = _case(c)
        assert (S.terms(x, d, f) - torch.from_numpy(g["%s_terms" % c])).abs().max().item() <= 1e-12
        assert abs(S.loss(x, d).item() - g["%s_loss" % c][0]) <= 1e-12
        assert abs(S.loss(x, d, f).item() - g["%s_loss" % c][1]) <= 1e-12
        assert _grad_err(S.loss_grad(x, d), torch.from_numpy(g["%s_grad" % c])) <= 1e-12
        assert _grad_err(S.loss_grad(x, d, f), torch.from_numpy(g["%s_grad_fix" % c])) <= 1e-12
        assert torch.equal(S.terms(x, d, f, dtype=torch.float32), R.saliency_metrics(x.exp(), d, f))
        assert torch.equal(S.terms(x, d, None, dtype=torch.float32), R.saliency_metrics(x.exp(), d))


def test_restated_gradient_is_autograd_of_the_restated_terms():
    """The analytic gradient against torch autograd through the restated terms, on a chunk-boundary shape that the
    fixture does not hold."""
    x, g, f, _, grad, grad_fix = _seeded(2, 3, 683, 11)
    for fx, ref in ((None, grad), (f, grad_fix)):
        xv = x.double().requires_grad_(True)
        got, = torch.autograd.grad(S.loss(xv, g, fx), xv)
        assert _grad_err(ref, got) <= 1e-12


def test_new_symbols_declared_exported_and_bound():
    from mspi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mspi_hip.h")).read()
    assert int(re.search(r"#define\s+MSPI_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mspi_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib._SIGNATURES and name in _lib.EXPORTS
        assert getattr(raw, name) is not None and getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]
    assert lib.mspi_version() == 2


def test_ws_bytes_arithmetic():
    """64 bytes of statistics per sample and 64 per chunk (48 of pass one, 16 of pass two); pure host arithmetic."""
    from mspi_amd import _lib, metrics as M
    lib = _lib.load()
    assert M.SAL_LOSS_CHUNK == CHUNK
    ws = lib.mspi_saliency_loss_ws_bytes
    assert ws(0, 100) == 0 and ws(-1, 100) == 0 and ws(2, 1) == 0 and ws(2, 0) == 0
    for N, L in ((1, 2), (1, 35), (3, 1023), (2, CHUNK - 1), (2, CHUNK), (2, CHUNK + 1), (8, 224 * 384), (5, 480 * 640)):
        assert ws(N, L) == N * 64 * (1 + (L + CHUNK - 1) // CHUNK), (N, L)
    assert ws(1, CHUNK + 1) == ws(1, CHUNK) + 64 == ws(1, 2) + 64


def test_argument_validation_without_gpu():
    from mspi_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for bad in ((None, p, p, p, p, 1, 100), (p, None, p, p, p, 1, 100), (p, p, p, None, p, 1, 100), (p, p, p, p, None, 1, 100),
                (p, p, None, p, None, 1, 100), (p, p, p, p, p, 0, 100), (p, p, p, p, p, -2, 100), (p, p, p, p, p, 1, 1),
                (p, p, None, p, p, 1, 0)):
        assert lib.mspi_saliency_loss_fwd(*bad, None) == -1
        assert b"mspi_saliency_loss_fwd" in lib.mspi_last_error()
    w = (1.0, 1.0, 0.1)
    for bad in ((None, p, p, p, p, *w, p, 1, 100), (p, None, p, p, p, *w, p, 1, 100), (p, p, p, None, p, *w, p, 1, 100),
                (p, p, p, p, None, *w, p, 1, 100), (p, p, p, p, p, *w, None, 1, 100), (p, p, None, p, p, *w, None, 1, 100),
                (p, p, p, p, p, *w, p, 0, 100), (p, p, p, p, p, *w, p, -1, 100), (p, p, p, p, p, *w, p, 1, 1)):
        assert lib.mspi_saliency_loss_bwd(*bad, None) == -1
        assert b"mspi_saliency_loss_bwd" in lib.mspi_last_error()


def test_python_entry_points_refuse_cpu_tensors():
    from mspi_amd import metrics as M
    from mspi_amd._lib import MspiError
    x, d, f = _case("tiny")
    xr = x.clone().requires_grad_(True)
    for call in (lambda: M.SalLoss()(xr, d), lambda: M.SalLoss()(xr, d, f), lambda: M.sal_loss(xr, d, f),
                 lambda: M.sal_loss_terms(xr, d), lambda: M.SalLoss()(x, d)):
        with pytest.raises(MspiError, match="no CPU fallback"):
            call()


def test_train_one_epoch_refuses_a_loss_without_graph():
    """What mspi_amd's own models give today: an output outside autograd.  The loop says so instead of torch's
    'element 0 of tensors does not require grad'."""
    from mspi_amd import engine_train as E
    from mspi_amd._lib import MspiError
    assert E.validation_one_epoch is not None and E.SalLoss is not None
    lin = torch.nn.Linear(4, 4)

    class Frozen(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin, self.calls = lin, []

        def frozen_encoder(self):
            self.calls.append("frozen_encoder")

        def forward(self, imgs):
            with torch.no_grad():
                return self.lin(imgs), None

    class Crit:
        log = {k: types.SimpleNamespace(val=0.0) for k in ("kl", "cc", "sim", "nss", "loss")}

        def __call__(self, out, label):
            return (out - label).pow(2).mean()
    model = Frozen()
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(USE_SOUND=False))
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    with pytest.raises(MspiError, match="no backward yet"):
        E.train_one_epoch(model, Crit(), [(torch.rand(2, 4), torch.rand(2, 4))], opt, torch.device("cpu"), 0, cfg)
    assert model.calls == ["frozen_encoder"] and model.training


# ------------------------------------------------------------------------------------------------------------- GPU
def _gpu_loss_and_grad(dev, x, g, f, scale=1.0):
    from mspi_amd import metrics as M
    xg = x.to(dev).requires_grad_(True)
    crit = M.SalLoss()
    loss = crit(xg, g.to(dev), None if f is None else f.to(dev))
    assert loss.dim() == 0 and loss.is_cuda and loss.grad_fn is not None and loss.dtype == torch.float32
    (scale * loss).backward()
    assert xg.grad.shape == x.shape
    return loss, xg.grad, crit


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_hip_terms_and_gradient_vs_fixture(dev, case):
    from mspi_amd import metrics as M
    gold = _gold()
    x, g, f = _case(case)
    ref = torch.from_numpy(gold["%s_terms" % case])
    terms = M.sal_loss_terms(x.to(dev), g.to(dev), f.to(dev))
    err = _terms_err(terms, ref)
    print("%s terms: rel err %.2e" % (case, err))
    assert err <= 2e-5
    nofix = M.sal_loss_terms(x.to(dev), g.to(dev))
    assert torch.equal(nofix[:, :3], terms[:, :3]) and (nofix[:, 3] == 0).all()
    for fx, key, li in ((None, "%s_grad", 0), (f, "%s_grad_fix", 1)):
        loss, grad, crit = _gpu_loss_and_grad(dev, x, g, fx)
        err = _grad_err(grad, torch.from_numpy(gold[key % case]))
        print("%s gradient (fixations: %s): %.2e of the largest entry" % (case, fx is not None, err))
        assert err <= 2e-5
        assert abs(loss.item() - gold["%s_loss" % case][li]) <= 1e-4
        assert abs(crit.log["loss"].val - loss.item()) <= 1e-6 * max(1.0, abs(loss.item()))
        assert abs(crit.log["kl"].val - ref[:, 0].mean().item()) <= 2e-5 * max(1.0, ref[:, 0].mean().abs().item())
        assert crit.log["nss"].count == (1 if fx is not None else 0) and crit.log["sim"].count == 1
        loss2, grad2, _ = _gpu_loss_and_grad(dev, x, g, fx)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


@pytest.mark.gpu
@pytest.mark.parametrize("L", sorted(BOUNDARY))
def test_hip_either_side_of_the_chunk_size(dev, L):
    from mspi_amd import metrics as M
    H, W = BOUNDARY[L]
    assert H * W == L
    x, g, f, terms, grad, grad_fix = _seeded(2, H, W, 11)
    got = M.sal_loss_terms(x.to(dev), g.to(dev), f.to(dev))
    et = _terms_err(got, terms)
    e2 = _grad_err(_gpu_loss_and_grad(dev, x, g, None)[1], grad)
    e3 = _grad_err(_gpu_loss_and_grad(dev, x, g, f)[1], grad_fix)
    print("L = %d: terms %.2e, gradient %.2e / %.2e with fixations" % (L, et, e2, e3))
    assert et <= 2e-5 and e2 <= 2e-5 and e3 <= 2e-5


@pytest.mark.gpu
def test_hip_training_shape_vs_float64_restatement(dev):
    from mspi_amd import metrics as M
    x, g, f, terms, grad, grad_fix = _seeded(8, 224, 384, 3)
    got = M.sal_loss_terms(x.to(dev), g.to(dev), f.to(dev))
    assert torch.equal(got, M.sal_loss_terms(x.to(dev), g.to(dev), f.to(dev)))
    et = _terms_err(got, terms)
    # the evaluation launch computes the same four values
    ev = M.per_sample(x.to(dev), g.to(dev), f.to(dev), pred_is_log=True)
    assert _terms_err(got, ev.cpu()) <= 2e-4
    res = {}
    for fx, ref in ((None, grad), (f, grad_fix)):
        loss, gr, _ = _gpu_loss_and_grad(dev, x, g, fx)
        loss2, gr2, _ = _gpu_loss_and_grad(dev, x, g, fx)
        assert torch.equal(gr, gr2) and torch.equal(loss, loss2)
        res[fx is not None] = _grad_err(gr, ref)
        assert abs(loss.item() - S.loss_from_terms(terms, fx is not None).item()) <= 1e-4
    print("8x224x384: terms %.2e, gradient %.2e / %.2e with fixations" % (et, res[False], res[True]))
    assert et <= 1e-4 and res[False] <= 2e-5 and res[True] <= 2e-5


@pytest.mark.gpu
def test_hip_scaled_loss_and_accumulation(dev):
    from mspi_amd import metrics as M
    x, g, f = _case("odd")
    ref = torch.from_numpy(_gold()["odd_grad_fix"])
    _, g1, _ = _gpu_loss_and_grad(dev, x, g, f)
    _, g25, _ = _gpu_loss_and_grad(dev, x, g, f, scale=2.5)
    assert _grad_err(g25, 2.5 * ref) <= 2e-5
    assert _grad_err(g25, 2.5 * g1.cpu()) <= 2e-6           # the scale enters once, in the per-sample coefficients
    # a second backward through a fresh graph accumulates into .grad
    xg = x.to(dev).requires_grad_(True)
    crit = M.SalLoss()
    crit(xg, g.to(dev), f.to(dev)).backward()
    assert torch.equal(xg.grad, g1)
    crit(xg, g.to(dev), f.to(dev)).backward()
    assert torch.equal(xg.grad, g1 + g1)
    assert crit.log["loss"].count == 2


@pytest.mark.gpu
def test_hip_per_term_gradients_and_double_backward(dev):
    """sal_loss_terms takes any weighting per sample and term; SIM carries no gradient.  Double backward is refused."""
    from mspi_amd import metrics as M
    from mspi_amd._lib import MspiError
    x, g, f = _case("odd")
    d_kl, d_cc, d_nss = S.term_grads(x, g, f)
    coef = torch.tensor([[0.5, -1.0, 3.0, 0.25], [2.0, 0.5, -7.0, -1.0], [-1.0, 1.5, 0.0, 2.0]])
    ref = (coef[:, 0].view(3, 1, 1) * d_kl + coef[:, 1].view(3, 1, 1) * d_cc + coef[:, 3].view(3, 1, 1) * d_nss)
    xg = x.to(dev).requires_grad_(True)
    (M.sal_loss_terms(xg, g.to(dev), f.to(dev)) * coef.to(dev)).sum().backward()
    assert _grad_err(xg.grad, ref) <= 2e-5
    xg = x.to(dev).requires_grad_(True)
    loss, terms = M.sal_loss(xg, g.to(dev), f.to(dev))
    assert not terms.requires_grad and loss.requires_grad
    with pytest.raises(MspiError, match="double backward"):
        torch.autograd.grad(loss, xg, create_graph=True)


@pytest.mark.gpu
def test_hip_without_grad_keeps_the_evaluation_bits(dev):
    from mspi_amd import metrics as M
    x, g, f = (t.to(dev) for t in _case("quad"))
    for fx in (None, f):
        m = M.per_sample(x, g, fix=fx, pred_is_log=True).mean(0).tolist()
        want = float(m[0]) - float(m[1]) - (0.1 * float(m[3]) if fx is not None else 0.0)
        a = M.SalLoss()(x, g, fx)                                   # the input does not require grad
        with torch.no_grad():
            b = M.SalLoss()(x.clone().requires_grad_(True), g, fx)
        for t in (a, b):
            assert t.grad_fn is None and not t.requires_grad and t.is_cuda and t.dim() == 0
            assert torch.equal(t.cpu(), torch.tensor(want))


@pytest.mark.gpu
def test_hip_non_contiguous_input(dev):
    from mspi_amd import metrics as M
    x, g, f = (t.to(dev) for t in _case("quad"))
    B, H, W = x.shape
    wide = torch.zeros(B, H, 2 * W, device=dev)
    wide[:, :, ::2] = x
    wide.requires_grad_(True)
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    loss = M.SalLoss()(view, g, f)
    loss.backward()
    xc = x.clone().requires_grad_(True)
    loss_c = M.SalLoss()(xc, g, f)
    loss_c.backward()
    assert torch.equal(loss, loss_c)
    assert wide.grad.shape == wide.shape and torch.equal(wide.grad[:, :, ::2], xc.grad)
    assert (wide.grad[:, :, 1::2] == 0).all()
    gv, = torch.autograd.grad(M.SalLoss()(view, g, f), view)
    assert gv.shape == view.shape and torch.equal(gv, xc.grad)


@pytest.mark.gpu
def test_hip_raw_abi_keeps_guard_bytes(dev):
    """terms, ws and dlog sit inside buffers filled with 0xA5: both calls write their own bytes only.  N = 3, L = 1023:
    a vector row with a 3-value tail and two misaligned rows."""
    from mspi_amd import _lib, metrics as M
    lib = _lib.load()
    x, g, f = (t.to(dev).contiguous() for t in _case("odd"))
    N, L = 3, 1023
    G = 256
    sizes = {"terms": N * 4 * 4, "ws": lib.mspi_saliency_loss_ws_bytes(N, L), "dlog": N * L * 4}
    assert sizes["ws"] == N * 64 * 2
    bufs = {k: torch.full((G + n + G,), 0xA5, dtype=torch.uint8, device=dev) for k, n in sizes.items()}
    ptr = {k: b.data_ptr() + G for k, b in bufs.items()}
    one = torch.ones((), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mspi_saliency_loss_fwd(x.data_ptr(), g.data_ptr(), f.data_ptr(), ptr["terms"], ptr["ws"], N, L, st) == 0
    assert lib.mspi_saliency_loss_bwd(x.data_ptr(), g.data_ptr(), f.data_ptr(), ptr["ws"], one.data_ptr(), 1 / 3, 1 / 3, 0.1 / 3,
                                      ptr["dlog"], N, L, st) == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert (b[:G] == 0xA5).all() and (b[G + sizes[k]:] == 0xA5).all(), k
    dlog = bufs["dlog"][G:G + sizes["dlog"]].view(torch.float32).view(N, 33, 31)
    terms = bufs["terms"][G:G + sizes["terms"]].view(torch.float32).view(N, 4)
    assert not torch.isnan(dlog).any() and not torch.isnan(terms).any()
    _, grad, _ = _gpu_loss_and_grad(dev, x.cpu(), g.cpu(), f.cpu())
    assert torch.equal(dlog, grad) and torch.equal(terms, M.sal_loss_terms(x, g, f))


@pytest.mark.gpu
def test_hip_forward_and_backward_inside_graph_capture(dev):
    """No synchronisation or allocation inside the two entry points: one capture, two replays with new input values, each
    bitwise equal to the eager gradient."""
    from mspi_amd import metrics as M
    sets = [_seeded(2, 40, 52, s)[:3] for s in (21, 22, 23)]
    eager = []
    for x, g, f in sets:
        xg = x.to(dev).requires_grad_(True)
        loss, terms = M.sal_loss(xg, g.to(dev), f.to(dev))
        grad, = torch.autograd.grad(loss, xg)
        eager.append((loss.detach().clone(), terms.clone(), grad.clone()))
    xs, gs, fs = (t.to(dev).clone() for t in sets[0])
    xs.requires_grad_(True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, terms = M.sal_loss(xs, gs, fs)
        grad, = torch.autograd.grad(loss, xs)
    for i in (1, 2):
        with torch.no_grad():
            xs.copy_(sets[i][0])
            gs.copy_(sets[i][1])
            fs.copy_(sets[i][2])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), eager[i][0]) and torch.equal(terms, eager[i][1]) and torch.equal(grad, eager[i][2])
    assert not torch.equal(eager[1][2], eager[2][2])


@pytest.mark.gpu
def test_hip_adam_on_free_logits_follows_the_float64_loop(dev):
    """End to end through autograd: x = z - logsumexp(z) in torch ops, 20 Adam steps at lr 0.05 on the loss with
    fixations; every step's loss within 1e-4 of the same loop in float64 with the restatement on the CPU."""
    from mspi_amd import metrics as M
    x0, g, f = _seeded(2, 24, 40, 31)[:3]
    z0 = (x0 * 0.5).clone()

    def run(z, loss_fn, steps=20):
        z = z.clone().requires_grad_(True)
        opt = torch.optim.Adam([z], lr=0.05)
        out = []
        for _ in range(steps):
            x = z - torch.logsumexp(z.flatten(1), 1).view(-1, 1, 1)
            loss = loss_fn(x)
            out.append(loss.item())
            opt.zero_grad()
            loss.backward()
            opt.step()
        return out
    ref = run(z0.double(), lambda x: S.loss(x, g, f))
    crit = M.SalLoss()
    gd, fd = g.to(dev), f.to(dev)
    got = run(z0.to(dev), lambda x: crit(x, gd, fd))
    err = max(abs(a - b) for a, b in zip(got, ref))
    print("adam: loss %.4f -> %.4f (float64 %.4f -> %.4f), max |diff| %.2e" % (got[0], got[-1], ref[0], ref[-1], err))
    assert ref[-1] < ref[0] - 0.5 and err <= 1e-4
    assert crit.log["loss"].count == 20


class _Readout(torch.nn.Module):
    """The smallest trainable saliency model: a 3-D convolution over the clip, then the log-normalisation."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv3d(3, 1, (4, 3, 3), padding=(0, 1, 1))

    def forward(self, imgs, audio=None):
        y = self.conv(imgs).squeeze(2).squeeze(1)
        out = y - torch.logsumexp(y.flatten(1), 1).view(-1, 1, 1)
        return out, self.conv.weight.pow(2).mean()


def _train_batches():
    gen = torch.Generator().manual_seed(77)
    batches = []
    for i in range(3):
        imgs = torch.randn(2, 3, 4, 16, 24, generator=gen)
        audio = torch.randn(2, 1, 8, 8, generator=gen)
        label = torch.from_numpy(S.make_case(2, 16, 24, 500 + i)[1])
        batches.append((imgs, audio, label))
    return batches


def _restated_epoch(model, batches, dtype, lr, gamma):
    """The loop of train_one_epoch with the restated criterion on the CPU; returns the per-key averages."""
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    logs = {k: [] for k in ("loss", "kld", "cc", "sim")}
    for imgs, audio, label in batches:
        out, va = model(imgs.to(dtype), audio.to(dtype))
        t = S.terms(out, label, None, dtype=dtype)
        loss = S.loss_from_terms(t, False) + gamma * va
        m = t.detach().mean(0)
        for k, v in zip(("loss", "kld", "cc", "sim"), (loss.item(), m[0].item(), m[1].item(), m[2].item())):
            logs[k].append(v)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return {k: sum(v) / len(v) for k, v in logs.items()}


@pytest.mark.gpu
def test_train_one_epoch_follows_the_float64_loop(dev):
    """Three batches of 2x3x4x16x24 as sound-style triples, SGD without momentum, gamma = 0.5.  The parameter change over
    the epoch is within 1e-3 of its largest entry of a float64 CPU run of the restated loop, loss / kld / cc / sim within
    1e-4.  The float32 CPU version of the same loop stays at 5e-7 of the largest entry and 2e-7 on the averages (seed 5 of
    the model, measured when the test was written), far more than the 10x margin the bounds need."""
    from mspi_amd import engine_train as E
    from mspi_amd import metrics as M
    torch.manual_seed(5)
    model = _Readout()
    start = {k: v.clone() for k, v in model.state_dict().items()}
    ref_model = _Readout().double()
    ref_model.load_state_dict({k: v.double() for k, v in start.items()})
    batches = _train_batches()
    lr, gamma = 0.5, 0.5
    ref = _restated_epoch(ref_model, batches, torch.float64, lr, gamma)
    model = model.to(dev)
    cfg = types.SimpleNamespace(DATA=types.SimpleNamespace(USE_SOUND=True))
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    got = E.train_one_epoch(model, M.SalLoss(), batches, opt, dev, 0, cfg, start_steps=0, gamma=gamma)
    assert set(got) == {"loss", "kld", "cc", "sim", "nss", "lr", "min_lr", "grad_norm"}      # no weight decay: no such key
    assert got["lr"] == lr and got["min_lr"] == lr and got["nss"] == 0.0 and got["grad_norm"] > 0
    for k in ("loss", "kld", "cc", "sim"):
        assert abs(got[k] - ref[k]) <= 1e-4, (k, got[k], ref[k])
    # all parameters as one vector: the bias alone does not move (the log-normalisation removes it from the output)
    d_got = torch.cat([(v.detach().cpu().double() - start[k].double()).flatten() for k, v in model.state_dict().items()])
    d_ref = torch.cat([(v - start[k].double()).flatten() for k, v in ref_model.state_dict().items()])
    assert d_ref.abs().max() > 1e-2
    worst = ((d_got - d_ref).abs().max() / d_ref.abs().max()).item()
    print("train_one_epoch: parameter change within %.2e of its largest entry" % worst)
    assert worst <= 1e-3
