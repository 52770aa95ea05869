"""csrc/class_loss.hip on the device: the class-index cross-entropy and the
accuracy_TU count against torch on the CPU in float64 over the kept rows
(F.cross_entropy and its gradient, s.argmax(1) for the hits), the masking,
tie and NaN rules, refused labels, determinism, the captured step with the
epoch accumulator, an evaluation pass over DeviceEvalLoader with ClassEpoch,
and the model switch models.DEVICE_CE."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import check_grads_model, rel_err, rel_l2

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL = 1e-5, 1e-4   # tests/test_gpu_task_heads.py:20 (loss relative, d_scores relative L2)
MODEL_LOSS_TOL, MODEL_GRAD_TOL = 1e-4, 1e-3  # tests/test_gpu_parity.py's LOSS_TOL / GRAD_TOL
DTYPES = {"f32": torch.float32, "i32": torch.int32, "i64": torch.int64}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _inputs(b, c, seed=0):
    """Post-sigmoid scores of seeded normals scaled by 4 and class labels."""
    gen = torch.Generator().manual_seed(seed * 100003 + b * 1031 + c)
    s = torch.sigmoid(4 * torch.randn(b, c, generator=gen))
    y = torch.randint(0, c, (b,), generator=gen)
    mask = torch.rand(b, generator=gen) < 0.3
    mask[0] = False  # (the batch without a kept row has a test of its own)
    return s, y, mask


def _ref(s, y, keep):
    """float64 on the CPU over the kept rows: loss, d loss / d s [B, C] (zero
    rows where not kept), hits."""
    s64 = s.double().requires_grad_(True)
    loss = F.cross_entropy(s64[keep], y[keep])
    loss.backward()
    hits = int((s.argmax(1)[keep] == y[keep]).sum())
    return loss.detach(), s64.grad, hits


def _labels(y, keep, dtype, dev):
    """Device labels of ``dtype`` with the rows outside ``keep`` masked."""
    if dtype == torch.float32:
        lab = y.float()
        lab[~keep] = float("nan")
    else:
        lab = y.to(dtype)
        lab[~keep] = -100
    return lab.to(dev)


def _run(pkg, dev, s, lab, epoch=None):
    sd = s.to(dev).requires_grad_(True)
    loss, count, hits, invalid = pkg.ops.class_loss(sd, lab, epoch=epoch, return_stats=True)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), sd.grad.cpu(), int(count), int(hits), int(invalid)


def _ulp_close(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b))))


# ---------------------------------------------------------------------------
# 1. shapes
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """The float64 references, computed once per (B, C, masked)."""
    cache = {}

    def get(b, c, masked):
        if (b, c, masked) not in cache:
            s, y, mask = _inputs(b, c)
            keep = ~mask if masked else torch.ones(b, dtype=torch.bool)
            cache[b, c, masked] = (s, y, keep) + _ref(s, y, keep)
        return cache[b, c, masked]
    return get


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "clean"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("c", [1, 2, 3, 63, 64, 65, 130, 1024])
@pytest.mark.parametrize("b", [1, 3, 5, 256, 257])
def test_class_loss_vs_torch(pkg, dev, refs, b, c, dtype, masked):
    """B: one row, fewer rows than a workgroup's wavefronts, one full sweep of
    64 workgroups x 4 rows (a wavefront per row: C > 32), one row past it.
    C: below, at and past the 64 lanes, then several strides.  Loss within 1e-5, d_scores within 1e-4
    relative L2 and exactly 0 at masked rows; count, hits, invalid exact."""
    s, y, keep, ref, gref, hits = refs(b, c, masked)
    loss, grad, count, got_hits, invalid = _run(pkg, dev, s, _labels(y, keep, DTYPES[dtype], dev))
    print(f"loss {float(loss):.8g} ref {float(ref):.8g} err {rel_err(loss, ref):.2e} "
          f"grad err {rel_l2(grad, gref):.2e}")
    assert (count, got_hits, invalid) == (int(keep.sum()), hits, 0)
    assert rel_err(loss.numpy(), ref.numpy()) < LOSS_TOL
    assert rel_l2(grad.numpy(), gref.numpy()) < GRAD_TOL
    if not keep.all():
        assert float(grad[~keep].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", ["f32", "i64"])
@pytest.mark.parametrize("b,c", [(128, 2), (129, 2), (8193, 2), (32, 8), (33, 5), (2049, 8),
                                 (8, 32), (9, 17), (513, 20), (2, 33)])
def test_rows_sharing_a_wavefront(pkg, dev, refs, b, c, dtype):
    """Few classes put 32 (C <= 2), 8 (C <= 8) or 2 (C <= 32) rows in one
    wavefront.  Per width: one workgroup's sweep exactly full (128, 32, 8 rows:
    the path that finishes without the arrival), one row past it (a second
    workgroup with one row, lanes past the batch), and more rows than one
    sweep of the 64 workgroups (8193, 2049, 513); C = 17 and 20: classes that
    do not fill the 32 lanes; C = 33: back to a wavefront per row."""
    s, y, keep, ref, gref, hits = refs(b, c, True)
    loss, grad, count, got_hits, invalid = _run(pkg, dev, s, _labels(y, keep, DTYPES[dtype], dev))
    print(f"loss {float(loss):.8g} ref {float(ref):.8g} err {rel_err(loss, ref):.2e} "
          f"grad err {rel_l2(grad, gref):.2e}")
    assert (count, got_hits, invalid) == (int(keep.sum()), hits, 0)
    assert rel_err(loss.numpy(), ref.numpy()) < LOSS_TOL
    assert rel_l2(grad.numpy(), gref.numpy()) < GRAD_TOL
    if not keep.all():
        assert float(grad[~keep].abs().max()) == 0.0


def test_labels_as_a_column_and_refusals(pkg, dev):
    """[B, 1] labels are [B]'s; what the op refuses before any launch."""
    s, y, _ = _inputs(5, 3)
    keep = torch.ones(5, dtype=torch.bool)
    a = _run(pkg, dev, s, _labels(y, keep, torch.int64, dev))
    b = _run(pkg, dev, s, _labels(y, keep, torch.int64, dev).reshape(5, 1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]
    sd, yd = s.to(dev), y.to(dev)
    E = pkg._lib.ScgibError
    with pytest.raises(E, match="float32, int32 or int64"):
        pkg.ops.class_loss(sd, yd.double())
    with pytest.raises(E, match="float32, int32 or int64"):
        pkg.ops.class_loss(sd, yd.to(torch.int16))
    with pytest.raises(E, match="vs labels"):
        pkg.ops.class_loss(sd, yd[:4])
    with pytest.raises(E, match="non-empty"):
        pkg.ops.class_loss(sd[:0], yd[:0])
    with pytest.raises(E, match="at most 1024"):
        pkg.ops.class_loss(torch.zeros(2, 1025, device=dev), yd[:2])
    with pytest.raises(E, match="no CPU fallback"):
        pkg.ops.class_loss(sd, y)
    with pytest.raises(E, match="ClassEpoch"):
        pkg.ops.class_loss(sd, yd, epoch=torch.zeros(5, device=dev))
    # the C-ABI refuses the same shapes itself, without launching
    out = torch.zeros(4, dtype=torch.int32, device=dev)
    ws = torch.zeros(256, dtype=torch.float64, device=dev)
    p = pkg.ops._p
    for rows, classes, ltype in ((2, 1025, 2), (0, 3, 2), (2, 0, 2), (2, 3, 3), ((1 << 30) + 1, 3, 2)):
        with pytest.raises(E, match="scgib_class_loss_fwd failed"):
            pkg._lib.call("scgib_class_loss_fwd", p(sd), p(yd), ltype, rows, classes, p(ws),
                          p(out[3:]), p(ws), p(out[0:]), p(out[1:]), p(out[2:]), None,
                          pkg.ops._stream())
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------
# 2. ties and NaN scores
# ---------------------------------------------------------------------------
def _tie_rows(c):
    """(scores [R, c], torch's argmax per row): two and three classes at
    exactly 1.0f, all classes equal, a NaN before and after the numeric
    maximum, two NaNs.  c = 130 puts equal maxima in one lane's stride (3 and
    67), in different lanes (5 and 70) and past the second stride (129)."""
    one = float(torch.sigmoid(torch.tensor(20.0)))
    assert one == 1.0  # sigmoid saturates in fp32: ties are real
    gen = torch.Generator().manual_seed(c)
    base = 0.9 * torch.rand(7, c, generator=gen)
    nan = float("nan")
    far = [3, 67, 129] if c > 64 else [1, 2, 3]
    base[0, [far[0], far[1]]] = one
    base[1, far] = one
    base[2, :] = 0.7
    base[3, far[1]] = 0.95
    base[3, far[0]] = nan          # a NaN before the numeric maximum
    base[4, far[0]] = 0.95
    base[4, far[1]] = nan          # ... and after it
    base[5, [far[2], far[1]]] = nan
    if c > 64:
        base[6, [70, 5]] = one
    else:
        base[6, [0, c - 1]] = one
    want = [far[0], far[0], 0, far[0], far[1], far[1], 5 if c > 64 else 0]
    return base, want


@pytest.mark.parametrize("c", [5, 130])
def test_ties_and_nan_scores_follow_torch_argmax(pkg, dev, c):
    """Hits follow torch's rule — the lowest index among the maxima, a NaN
    above every number, the first NaN — and a row holding a NaN score has a
    NaN loss in both implementations."""
    s, want = _tie_rows(c)
    assert s.argmax(1).tolist() == want  # the expected values are torch's own
    rows = len(want)
    for shift in (0, 1):  # labels at the argmax, then one class further
        y = (torch.tensor(want) + shift) % c
        keep = torch.ones(rows, dtype=torch.bool)
        for dtype in DTYPES.values():
            _, _, count, hits, invalid = _run(pkg, dev, s, _labels(y, keep, dtype, dev))
            assert (count, hits, invalid) == (rows, rows if shift == 0 else 0, 0)
        for r in range(rows):  # per-row losses
            ref, gref, _ = _ref(s[r:r + 1], y[r:r + 1], keep[:1])
            loss, grad, _, hit, _ = _run(pkg, dev, s[r:r + 1], _labels(y[r:r + 1], keep[:1],
                                                                       torch.float32, dev))
            assert hit == 1 - shift
            assert bool(torch.isnan(loss)) == bool(torch.isnan(ref)) == bool(torch.isnan(s[r]).any())
            if not torch.isnan(ref):
                assert rel_err(loss.numpy(), ref.numpy()) < LOSS_TOL
                assert rel_l2(grad.numpy(), gref.numpy()) < GRAD_TOL


# ---------------------------------------------------------------------------
# 3. invalid labels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_invalid_labels_are_counted_and_index_nothing(pkg, dev, dtype):
    """1.5, -1.0, float(C), +-inf / int C and -1 among valid rows: counted in
    ``invalid``, no loss, no hit, no count, zero gradient; loss and gradient
    are those of the batch without these rows (the float64 reference at the
    bars above, and the device's own result on the shorter batch
    within one fp32 ulp: fp64 sums, one final rounding); ClassEpoch.result()
    raises.  A refusal: nothing here reaches torch's own loss on the device."""
    c, b = 4, 23
    s, y, mask = _inputs(b, c, seed=3)
    bad = [1.5, -1.0, float(c), float("inf"), float("-inf")] if dtype == "f32" else [c, -1, 1 << 20]
    at = [2, 7, 8, 15, 22][:len(bad)]
    lab = _labels(y, ~mask, DTYPES[dtype], dev)
    lab[at] = torch.tensor(bad, dtype=DTYPES[dtype], device=dev)
    keep = ~mask
    keep[at] = False
    ref, gref, hits = _ref(s, y, keep)
    ep = pkg.metrics.ClassEpoch(dev)
    loss, grad, count, got_hits, invalid = _run(pkg, dev, s, lab, epoch=ep)
    assert (count, got_hits, invalid) == (int(keep.sum()), hits, len(bad))
    assert rel_err(loss.numpy(), ref.numpy()) < LOSS_TOL
    assert rel_l2(grad.numpy(), gref.numpy()) < GRAD_TOL
    assert float(grad[~keep].abs().max()) == 0.0
    rest = torch.ones(b, dtype=torch.bool)
    rest[at] = False
    l2, g2, c2, h2, i2 = _run(pkg, dev, s[rest], _labels(y, ~mask, DTYPES[dtype], dev)[rest.to(dev)])
    assert (c2, h2, i2) == (count, hits, 0)
    assert _ulp_close(loss.numpy(), l2.numpy()) and _ulp_close(grad[rest].numpy(), g2.numpy())
    with pytest.raises(pkg._lib.ScgibError, match=f"{len(bad)} labels"):
        ep.result()
    ep.reset()
    with pytest.raises(ZeroDivisionError):
        ep.result()


# ---------------------------------------------------------------------------
# 4. no kept row
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_no_kept_row(pkg, dev, dtype):
    """The loss is NaN, the gradient all zero, and the accumulator moves only
    in ``invalid``."""
    s, y, mask = _inputs(9, 3, seed=4)
    ep = pkg.metrics.ClassEpoch(dev)
    _run(pkg, dev, s, _labels(y, ~mask, DTYPES[dtype], dev), epoch=ep)
    before = ep.state.cpu().clone()
    assert before[1] == 1 and before[3] == int((~mask).sum()) and before[4] == 0
    lab = _labels(y, torch.zeros(9, dtype=torch.bool), DTYPES[dtype], dev)
    loss, grad, count, hits, invalid = _run(pkg, dev, s, lab, epoch=ep)
    assert bool(torch.isnan(loss)) and (count, hits, invalid) == (0, 0, 0)
    assert torch.equal(grad, torch.zeros(9, 3))
    assert torch.equal(ep.state.cpu(), before)
    lab[4] = 7  # an invalid row among the masked ones
    loss, grad, count, hits, invalid = _run(pkg, dev, s, lab, epoch=ep)
    assert bool(torch.isnan(loss)) and (count, hits, invalid) == (0, 0, 1)
    assert torch.equal(grad, torch.zeros(9, 3))
    after = ep.state.cpu()
    assert torch.equal(after[:4], before[:4]) and after[4] == 1


# ---------------------------------------------------------------------------
# 5. determinism
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("b,c", [(257, 130), (2048, 6)])
def test_class_loss_is_deterministic(pkg, dev, b, c):
    """Two runs: equal bits in the loss and the gradient (2048 rows: eight
    sweeps of the 64 workgroups and the last-arriver sum)."""
    s, y, mask = _inputs(b, c, seed=5)
    lab = _labels(y, ~mask, torch.float32, dev)
    a, b2 = (_run(pkg, dev, s, lab) for _ in range(2))
    assert torch.isfinite(a[0])
    assert torch.equal(a[0], b2[0]) and torch.equal(a[1], b2[1]) and a[2:] == b2[2:]


# ---------------------------------------------------------------------------
# 6. capture
# ---------------------------------------------------------------------------
def test_step_with_epoch_captures_and_replays(pkg, dev):
    """predict_head + class_loss(epoch=) + backward captured after one eager
    step, replayed on three static batches: each replay's loss and gradients
    are bitwise the eager step's, and the accumulator holds the three."""
    B, K, C = 32, 128, 2
    torch.manual_seed(6)
    seq = nn.Sequential(nn.Linear(K, 64), nn.ReLU(), nn.Linear(64, C)).to(dev)
    gen = torch.Generator().manual_seed(16)
    batches = []
    for i in range(3):
        x = torch.randn(B, K, generator=gen)
        lab = torch.randint(0, C, (B,), generator=gen).float()
        lab[torch.rand(B, generator=gen) < 0.2 * i] = float("nan")
        batches.append((x.to(dev), lab.to(dev)))
    assert not torch.isnan(batches[0][1]).any() and torch.isnan(batches[2][1]).any()
    xs, labs = torch.zeros(B, K, device=dev), torch.zeros(B, device=dev)
    ep, ep_eager = pkg.metrics.ClassEpoch(dev), pkg.metrics.ClassEpoch(dev)

    def step(epoch):
        scores = pkg.ops.predict_head(xs, seq, True)
        loss, count, hits, _ = pkg.ops.class_loss(scores, labs, epoch=epoch, return_stats=True)
        loss.backward()
        return loss.detach(), count, hits

    def grads():
        return [p.grad.clone() for p in seq.parameters()]

    xs.copy_(batches[0][0])
    labs.copy_(batches[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(ep)  # eager: allocator warm-up, the loss's arrival counter
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ep.reset()
    seq.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(ep)
    got = []
    for x, lab in batches:
        xs.copy_(x)
        labs.copy_(lab)
        graph.replay()
        torch.cuda.synchronize()
        got.append(([t.clone() for t in out], grads()))
    total, n_hits, n_lab = 0.0, 0, 0
    for (x, lab), (o, g) in zip(batches, got):
        xs.copy_(x)
        labs.copy_(lab)
        seq.zero_grad(set_to_none=True)
        want = step(ep_eager)
        torch.cuda.synchronize()
        assert torch.isfinite(o[0])
        assert all(torch.equal(a, b) for a, b in zip(o, want))
        assert all(torch.equal(a, b) for a, b in zip(g, grads()))
        assert int(o[1]) == int((~torch.isnan(lab)).sum())
        total += float(o[0])  # the fp32 loss, summed in double
        n_hits += int(o[2])
        n_lab += int(o[1])
    assert torch.equal(ep.state, ep_eager.state)
    assert ep.state.cpu().tolist() == [total, 3.0, float(n_hits), float(n_lab), 0.0]
    r = ep.result()
    assert r == {"loss": total / 3, "acc": n_hits / n_lab, "hits": n_hits, "labelled": n_lab,
                 "batches": 3}


# ---------------------------------------------------------------------------
# 7. an evaluation epoch over DeviceEvalLoader
# ---------------------------------------------------------------------------
def test_eval_epoch_over_the_device_loader(pkg, dev):
    """150 Mutagenicity-like molecules with 0/1 class labels stored as floats,
    a 75-id subset in batches of 32 (a tail of 11 real rows and 21 fill rows):
    Mainmodel_finetuning in eval mode with fixed noise, then
    loss_CrossEntropy(..., epoch=ep).  ep.result() against the host loop over
    the same batches without the fill rows: per-batch F.cross_entropy in
    float64 and the argmax count."""
    import finetune_bench
    from eval_loader_cases import batches_of, eval_static, labels_of
    M, B = 150, 32
    mols = pkg.synth.molecules(M, "mutagenicity", seed=23)
    y = np.random.default_rng(23).integers(0, 2, size=(M, 1)).astype(np.float32)
    idx = np.random.default_rng(24).permutation(M)[:75]
    ft, k = finetune_bench.make_finetune_model(pkg, 14, B, dev, seed=5, dataset="Mutagenicity",
                                               num_classes=2)
    ft.eval()
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, k, labels=y)
    static = eval_static(pkg, ds, B, dev, idx)
    evl = pkg.graph.DeviceEvalLoader(ds, static, indices=idx)
    batches = batches_of(mols, idx, B)
    assert evl.steps == len(batches) == 3
    n_cap = static.n_cap
    gen = torch.Generator().manual_seed(25)
    noise = (torch.rand(n_cap, generator=gen).to(dev), torch.rand(n_cap, 64, generator=gen).to(dev))
    ep = pkg.metrics.ClassEpoch(dev)
    evl.prime()
    scores, labels = [], []
    for _ in range(evl.steps):
        static.load_next(evl.pool)
        evl.collate_ahead()
        with torch.no_grad():
            s, *_ = ft(static.graph, static.x, None, None, 1, None, k, dev, B, noise=noise)
            ft.loss_CrossEntropy(s, evl.labels, epoch=ep)
        scores.append(s.clone())
        labels.append(evl.labels.clone())
    torch.cuda.synchronize()
    assert evl.error() == 0 and static.ego_error() == 0
    losses, hits = [], 0
    for t, (ids, marked) in enumerate(batches):
        real = torch.from_numpy(marked >= 0)
        assert np.array_equal(labels[t].cpu().numpy(), labels_of(y, marked), equal_nan=True)
        s = scores[t].cpu()
        assert torch.isfinite(s).all()
        yb = torch.from_numpy(y[ids, 0]).long()[real]
        losses.append(float(F.cross_entropy(s.double()[real], yb)))
        hits += int((s.argmax(1)[real] == yb).sum())
    assert int(real.sum()) == 11
    r = ep.result()
    print(f"loss {r['loss']:.8g} host {sum(losses) / 3:.8g} acc {r['acc']:.4f} hits {hits}")
    assert (r["hits"], r["labelled"], r["batches"]) == (hits, len(idx), 3)
    assert r["acc"] == hits / len(idx)
    assert rel_err(r["loss"], sum(losses) / 3) < LOSS_TOL
    # the fill rows change nothing: the tail batch's loss is its 11 real rows'
    tail = pkg.ops.class_loss(scores[-1], labels[-1])
    short = pkg.ops.class_loss(scores[-1][:11].contiguous(), labels[-1][:11])
    assert _ulp_close(tail.cpu().numpy(), short.cpu().numpy())
    assert rel_err(float(tail), losses[-1]) < LOSS_TOL


# ---------------------------------------------------------------------------
# 8. the model switch
# ---------------------------------------------------------------------------
def test_model_switch_device_ce(pkg, dev, monkeypatch):
    """The Mutagenicity B = 32 case of tests/test_gpu_finetune_config.py.
    DEVICE_CE off: int64 targets give F.cross_entropy's bits on the device.
    On: loss and every trainable gradient agree with the torch tail at
    tests/test_gpu_parity.py's tolerances.  float32 targets take the kernel
    whatever the switch says."""
    import finetune_bench
    from test_gpu_finetune_config import B, CONFIGS, _loss
    workload, dataset, ncls, kind = CONFIGS["mutag_B32_ce"]
    F_in = pkg.synth.WORKLOADS[workload][2]
    base, k = finetune_bench.make_finetune_model(pkg, F_in, B, dev, seed=5, dataset=dataset,
                                                 num_classes=ncls)
    g = pkg.graph.collate_pyg(pkg.synth.molecules(B, workload, seed=41))[0].to(dev)
    x = F.normalize(g.ndata["x"].float())
    n = g.num_nodes()
    gen = torch.Generator().manual_seed(88)
    noise = (torch.rand(n, generator=gen).to(dev), torch.rand(n, 64, generator=gen).to(dev))
    targets = torch.randint(0, ncls, (B, 1), generator=gen).to(dev)
    assert pkg.models.DEVICE_CE is False
    runs = {}
    for name, switch, tg in (("torch", False, targets), ("device", True, targets),
                             ("float", False, targets.float())):
        monkeypatch.setattr(pkg.models, "DEVICE_CE", switch)
        ft = copy.deepcopy(base)
        scores, *_ = ft(g, x, None, None, 1, None, 2, dev, B, noise=noise)
        loss = ft.loss_CrossEntropy(scores, tg)
        if name == "torch":
            assert torch.equal(loss, _loss(kind, scores, targets))
        loss.backward()
        torch.cuda.synchronize()
        runs[name] = (scores.detach(), loss.detach(),
                      {nm: p.grad.cpu().numpy() for nm, p in ft.named_parameters()
                       if p.grad is not None})
    (s0, l0, g0), (s1, l1, g1), (s2, l2, g2) = runs["torch"], runs["device"], runs["float"]
    assert torch.equal(s0, s1) and torch.isfinite(l0)
    # the torch tail once more, by hand: same bits as the switch-off method
    ft = copy.deepcopy(base)
    scores, *_ = ft(g, x, None, None, 1, None, 2, dev, B, noise=noise)
    hand = F.cross_entropy(scores, targets.squeeze(-1))
    hand.backward()
    assert torch.equal(hand.detach(), l0)
    assert all(np.array_equal(p.grad.cpu().numpy(), g0[nm]) for nm, p in ft.named_parameters()
               if p.grad is not None)
    print(f"loss torch {float(l0):.8g} device {float(l1):.8g}")
    assert rel_err(float(l1), float(l0)) < MODEL_LOSS_TOL
    assert set(g0) == set(g1) and any(nm.startswith("predict.") for nm in g0)
    check_grads_model(g0, lambda nm: torch.from_numpy(g1[nm]), tol=MODEL_GRAD_TOL)
    assert torch.equal(l2, l1) and all(np.array_equal(g2[nm], g1[nm]) for nm in g1)
