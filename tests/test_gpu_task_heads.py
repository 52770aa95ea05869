"""csrc/task_head.hip on the device: the wide fine-tune head (16 < C <= 1024)
and the NaN-masked task losses against torch in float64, their edge cases
(no kept element, padding rows, an all-NaN column), run-to-run determinism,
the model-level tail against the torch tail, and the captured step with NaN
labels that the boolean-index path cannot give."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import check_grads_model, rel_err

pytestmark = pytest.mark.gpu

KINDS = ("bce", "bce_logits", "mae", "rmse")
LOSS_TOL, LOSS_GRAD_TOL = 1e-5, 1e-4   # the project's BCE bars (test_predict_head_and_bce_vs_torch)
ACT_TOL, MODEL_LOSS_TOL, MODEL_GRAD_TOL = 1e-4, 1e-4, 1e-3  # tests/test_gpu_parity.py's


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------
# the wide head
# ---------------------------------------------------------------------------
def _head_case(n, k, c, sig):
    """Inputs, the float64 result and the float32 CPU result of one head case:
    [out, dx, dW1, db1, dW2, db2] each."""
    torch.manual_seed(n * 1000 + k + c)
    seq = nn.Sequential(nn.Linear(k, 64), nn.ReLU(), nn.Linear(64, c))
    x = torch.randn(n, k)
    up = torch.rand(n, c)
    res = []
    for dt in (torch.float64, torch.float32):
        s = copy.deepcopy(seq).to(dt)
        xx = x.to(dt).clone().requires_grad_(True)
        o = s(xx)
        o = torch.sigmoid(o) if sig else o
        (o * up.to(dt)).sum().backward()
        res.append([o.detach(), xx.grad] + [p.grad for p in s.parameters()])
    return seq, x, up, res[0], res[1]


def _run_head(pkg, dev, seq, x, up, sig):
    seqd = copy.deepcopy(seq).to(dev)
    xd = x.to(dev).requires_grad_(True)
    assert pkg.ops.predict_head_ok(xd, seqd)
    out = pkg.ops.predict_head(xd, seqd, sig)
    (out * up.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return [out.detach(), xd.grad] + [p.grad for p in seqd.parameters()]


HEAD_CASES = [(1, 128, 17, True), (33, 128, 128, True), (70, 64, 65, False), (5, 12, 27, True),
              (64, 128, 617, True), (0, 128, 128, True)]


@pytest.mark.parametrize("n,k,c,sig", HEAD_CASES)
def test_wide_head_vs_torch(pkg, dev, n, k, c, sig):
    """scgib_head_wide_fwd / _bwd against torch in float64: the output and the
    five gradients.  Bound per tensor: four times the error of the same head
    evaluated in float32 by torch on the CPU (a different but legitimate
    summation order), never below the project's 1e-5.  Measured float32 CPU
    figures (rel_err against float64; out, dx, dW1, db1, dW2, db2), largest
    over the six cases: 2.2e-7, 3.4e-7, 3.9e-7, 1.1e-7, 3.3e-7, 1.3e-7 — so
    the 1e-5 floor is the bound in every case.  Covers: one row; two row
    workgroups + a partial third (33) and the slab reduce; C not a multiple of
    the 64-column tile nor of the 16-column dW2 groups (17, 65, 27, 617);
    K = 12 / 64 (reads past column K stay unused); n = 0."""
    seq, x, up, ref, f32 = _head_case(n, k, c, sig)
    got = _run_head(pkg, dev, seq, x, up, sig)
    assert got[0].shape == (n, c)
    for name, g, r, f in zip(("out", "dx", "dW1", "db1", "dW2", "db2"), got, ref, f32):
        cpu32 = rel_err(f.numpy(), r.numpy())
        tol = max(4 * cpu32, 1e-5)
        err = rel_err(g.cpu().numpy(), r.numpy())
        print(f"{name}: err {err:.2e} fp32-cpu {cpu32:.2e} tol {tol:.2e}")
        assert g.shape == r.shape, name
        assert err < tol, (name, err, tol)
    if n == 0:
        assert all(float(g.abs().max()) == 0.0 for g in got[2:])


def test_wide_head_refusals(pkg, dev):
    """Outside 16 < C <= 1024, K <= 128, K % 4 == 0 the kernels refuse loudly
    (and predict_head_ok is False, so the model keeps torch's head)."""
    for k, c in ((128, 1025), (9, 17)):
        seq = nn.Sequential(nn.Linear(k, 64), nn.ReLU(), nn.Linear(64, c)).to(dev)
        x = torch.randn(4, k, device=dev)
        assert not pkg.ops.predict_head_ok(x, seq)
        with pytest.raises(pkg._lib.ScgibError):
            pkg.ops.predict_head(x, seq, True)
    seq = nn.Sequential(nn.Linear(128, 64), nn.ReLU(), nn.Linear(64, 1024)).to(dev)
    assert pkg.ops.predict_head_ok(torch.randn(4, 128, device=dev), seq)


# ---------------------------------------------------------------------------
# the masked losses
# ---------------------------------------------------------------------------
# (shape, NaN share) -> elements kept with the mask drawn first from
# torch.Generator().manual_seed(0) as torch.rand(shape) < p
LOSS_SHAPES = [((1, 1), 0.0, 1), ((33, 12), 0.2, 314), ((70, 128), 0.6, 3580),
               ((300, 617), 0.3, 129818)]


def _torch_loss(kind, s, t):
    if kind == "bce":
        return F.binary_cross_entropy(s, t)
    if kind == "bce_logits":
        return F.binary_cross_entropy_with_logits(s, t)
    if kind == "mae":
        return F.l1_loss(s, t)
    return torch.sqrt(F.mse_loss(s, t))


def _loss_inputs(kind, shape, p, seed=0):
    """scores, clean targets, NaN mask (CPU fp32 / bool)."""
    gen = torch.Generator().manual_seed(seed)
    nan = torch.rand(shape, generator=gen) < p
    if kind == "bce":
        s = torch.rand(shape, generator=gen).clamp(1e-6, 1 - 1e-6)
    else:
        s = torch.randn(shape, generator=gen)
    if kind in ("bce", "bce_logits"):
        t = torch.randint(0, 2, shape, generator=gen).float()
    else:
        t = torch.randn(shape, generator=gen)
    return s, t, nan


def _ref_masked(kind, s, t, nan):
    """metric(s[~nan], t[~nan]) in float64 and its gradient over s."""
    s64 = s.double().requires_grad_(True)
    loss = _torch_loss(kind, s64[~nan], t.double()[~nan])
    loss.backward()
    return loss.detach(), s64.grad


def _dev_loss(pkg, dev, kind, s, t, nan):
    sd = s.to(dev).requires_grad_(True)
    td = torch.where(nan, torch.full_like(t, float("nan")), t).to(dev)
    loss, count = pkg.ops.task_loss(sd, td, kind, return_count=True)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), sd.grad.cpu(), int(count)


@pytest.fixture(scope="module")
def loss_refs():
    """The float64 references, computed once per (kind, shape, masked)."""
    cache = {}

    def get(kind, shape, p, masked):
        key = (kind, shape, masked)
        if key not in cache:
            s, t, nan = _loss_inputs(kind, shape, p)
            if not masked:
                nan = torch.zeros_like(nan)
            cache[key] = (s, t, nan) + _ref_masked(kind, s, t, nan)
        return cache[key]
    return get


@pytest.mark.parametrize("masked", [True, False], ids=["nan", "clean"])
@pytest.mark.parametrize("shape,p,kept", LOSS_SHAPES, ids=["1x1", "33x12", "70x128", "300x617"])
@pytest.mark.parametrize("kind", KINDS)
def test_task_loss_vs_torch(pkg, dev, loss_refs, kind, shape, p, kept, masked):
    """Every loss kind against torch in float64 on metric(s[~nan], t[~nan])
    (masked) and on the plain loss (no NaN target): loss within 1e-5,
    d_scores within 1e-4, d_scores exactly 0 at masked elements, the loss
    finite (m > 0 in every case), the device count = elements kept.
    1x1: one thread's worth; 300x617: 64 workgroups, the last-arriver sum."""
    s, t, nan, ref, gref = loss_refs(kind, shape, p, masked)
    assert int((~nan).sum()) == (kept if masked else s.numel())
    assert torch.isfinite(ref)
    loss, grad, count = _dev_loss(pkg, dev, kind, s, t, nan)
    print(f"loss {float(loss):.8g} ref {float(ref):.8g} err {rel_err(loss, ref):.2e} "
          f"grad err {rel_err(grad, gref):.2e}")
    assert count == int((~nan).sum())
    assert torch.isfinite(loss)
    assert rel_err(loss.numpy(), ref.numpy()) < LOSS_TOL
    assert rel_err(grad.numpy(), gref.numpy()) < LOSS_GRAD_TOL
    if nan.any():
        assert float(grad[nan].abs().max()) == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_task_loss_all_nan_column(pkg, dev, kind):
    """A task with no label in the batch (one whole column NaN)."""
    s, t, nan = _loss_inputs(kind, (33, 12), 0.2)
    nan[:, 3] = True
    ref, gref = _ref_masked(kind, s, t, nan)
    loss, grad, count = _dev_loss(pkg, dev, kind, s, t, nan)
    assert count == int((~nan).sum()) and torch.isfinite(loss)
    assert rel_err(loss.numpy(), ref.numpy()) < LOSS_TOL
    assert rel_err(grad.numpy(), gref.numpy()) < LOSS_GRAD_TOL
    assert float(grad[:, 3].abs().max()) == 0.0 and float(grad[nan].abs().max()) == 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_task_loss_no_element_kept(pkg, dev, kind):
    """m = 0: the loss is NaN (torch's mean over an empty tensor) and d_scores
    is all zeros."""
    s, t, _ = _loss_inputs(kind, (4, 3), 0.0)
    loss, grad, count = _dev_loss(pkg, dev, kind, s, t, torch.ones(4, 3, dtype=torch.bool))
    assert count == 0 and bool(torch.isnan(loss))
    assert torch.equal(grad, torch.zeros(4, 3))


def _ulp_close(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b))))


@pytest.mark.parametrize("kind", KINDS)
def test_task_loss_padding_rows(pkg, dev, kind):
    """A short batch in capacity mode: 7 padding rows with NaN targets change
    nothing — loss and the real rows' gradients within one fp32 ulp (fp64 sums,
    one final rounding), the padding rows' gradients exactly zero."""
    s, t, nan = _loss_inputs(kind, (33, 12), 0.2)
    la, ga, ca = _dev_loss(pkg, dev, kind, s, t, nan)
    pad_s = torch.full((7, 12), 0.5)
    lb, gb, cb = _dev_loss(pkg, dev, kind, torch.cat([s, pad_s]), torch.cat([t, torch.zeros(7, 12)]),
                           torch.cat([nan, torch.ones(7, 12, dtype=torch.bool)]))
    assert ca == cb
    assert _ulp_close(lb.numpy(), la.numpy())
    assert _ulp_close(gb[:33].numpy(), ga.numpy())
    assert float(gb[33:].abs().max()) == 0.0


def test_kernels_are_deterministic(pkg, dev):
    """Two runs of every kernel on the same inputs: bitwise equal."""
    seq, x, up, _, _ = _head_case(33, 128, 128, True)
    a, b = (_run_head(pkg, dev, seq, x, up, True) for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    for kind in KINDS:
        s, t, nan = _loss_inputs(kind, (70, 128), 0.6)
        (la, ga, _), (lb, gb, _) = (_dev_loss(pkg, dev, kind, s, t, nan) for _ in range(2))
        assert torch.equal(la, lb) and torch.equal(ga, gb), kind


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
N_MOLS = 37


def _finetune(pkg, dev, num_classes, F_in):
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=N_MOLS, gin_layers=4, task="graph_classification",
                           dataset="ogbg-molpcba", device=dev)
    torch.manual_seed(5)
    inner = pkg.models.Mainmodel(args, F_in, 64, 4, 4, 1, "GIN")
    pre = pkg.models.Mainmodel_continue(args, F_in, 64, 4, 4, 1, num_classes, inner, "GIN")
    ft = pkg.models.Mainmodel_finetuning(args, F_in, 64, 4, 4, 1, num_classes, pre, "GIN")
    return ft.to(dev).train()


@pytest.fixture(scope="module")
def batch(pkg, dev):
    mols = pkg.synth.molecules(N_MOLS, "molpcba", seed=11)
    gh, _ = pkg.graph.collate_pyg(mols)
    g = gh.to(dev)
    x = F.normalize(g.ndata["x"].float())
    gen = torch.Generator().manual_seed(3)
    n = g.num_nodes()
    noise = (torch.rand(n, generator=gen).to(dev), torch.rand(n, 64, generator=gen).to(dev))
    return g, x, noise


def _targets(c, seed, p=0.3):
    gen = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 2, (N_MOLS, c), generator=gen).float()
    t[torch.rand(N_MOLS, c, generator=gen) < p] = float("nan")
    return t


@pytest.mark.parametrize("c", [128, 12])
def test_model_tail_matches_torch_tail(pkg, dev, batch, c, monkeypatch):
    """Mainmodel_finetuning with 128 tasks (the wide head) and 12 (head.hip's),
    loss through MetricWrapper(model.loss, "ignore-flatten") on NaN labels:
    models.FUSE_HEAD on (device head + ops.task_loss) against off (torch's
    head, the wrapper's boolean-index path) — scores, loss, every trainable
    gradient, at tests/test_gpu_parity.py's tolerances."""
    g, x, noise = batch
    base = _finetune(pkg, dev, c, x.shape[1])
    tg = _targets(c, 7).to(dev)
    runs = []
    for fuse in (False, True):
        monkeypatch.setattr(pkg.models, "FUSE_HEAD", fuse)
        ft = copy.deepcopy(base)
        wrapped = pkg.MetricWrapper(metric=ft.loss, target_nan_mask="ignore-flatten")
        scores, *_ = ft(g, x, None, None, 1, None, 1, dev, N_MOLS, noise=noise)
        loss = wrapped(scores, tg)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((scores.detach().cpu(), float(loss.detach()),
                     {n: p.grad.cpu().numpy() for n, p in ft.named_parameters() if p.grad is not None}))
    (s0, l0, g0), (s1, l1, g1) = runs
    assert s1.shape == (N_MOLS, c) and np.isfinite(l0)
    assert rel_err(s1.numpy(), s0.numpy()) < ACT_TOL
    assert rel_err(l1, l0) < MODEL_LOSS_TOL
    assert set(g0) == set(g1) and any(n.startswith("predict.") for n in g0)
    check_grads_model(g0, lambda n: torch.from_numpy(g1[n]), tol=MODEL_GRAD_TOL)


def test_masked_step_captures_and_replays(pkg, dev, batch):
    """The molpcba-shaped tail as a captured graph: the head at C = 128,
    MetricWrapper(model.loss, "ignore-flatten") on NaN labels and the backward
    are captured after one eager step (a path that synchronises would fail the
    capture itself), then replayed on a different NaN pattern written into the
    static target buffer: loss and predict.2.weight.grad are bitwise those of
    an eager run on these targets."""
    ft = _finetune(pkg, dev, 128, batch[1].shape[1])
    wrapped = pkg.MetricWrapper(metric=ft.loss, target_nan_mask="ignore-flatten")
    gen = torch.Generator().manual_seed(9)
    xs = torch.randn(N_MOLS, 128, generator=gen).to(dev)
    tg = _targets(128, 1).to(dev)
    tg2 = _targets(128, 2, p=0.6).to(dev)
    assert not torch.equal(torch.isnan(tg), torch.isnan(tg2))

    def step():
        scores = pkg.ops.predict_head(xs, ft.predict, True)
        loss = wrapped(scores, tg)
        loss.backward()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # eager: allocator warm-up, the loss's arrival counter
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ft.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    tg.copy_(tg2)
    graph.replay()
    torch.cuda.synchronize()
    got = loss.clone(), ft.predict[2].weight.grad.clone()
    ft.zero_grad(set_to_none=True)
    want = step(), ft.predict[2].weight.grad
    torch.cuda.synchronize()
    assert torch.isfinite(got[0])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ref = F.binary_cross_entropy(pkg.ops.predict_head(xs, ft.predict, True).detach()[~torch.isnan(tg2)],
                                 tg2[~torch.isnan(tg2)])
    assert rel_err(float(got[0]), float(ref)) < LOSS_TOL
