"""graph.DeviceEvalLoader and DeviceLoader(indices=...) on the MI355X
(csrc/collate.hip): every ring slot against StaticBatch.pad of
the host-collated sequential batch (real molecules + fill), byte for byte over
two passes; labels and ids with NaN rows / -1 at the fill positions; subsets
that are no prefix of the dataset; set_subset under one captured graph;
overflow; and a whole evaluation pass against a fixed pool of the same batches."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eval_loader_cases import batches_of, eval_static, labels_of
from loader_cases import (handmade_set, labels_with_nans, pad_blob, same_bits, sized_set,
                          static_for, tiny_set)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


class _Expect:
    """The sequential batches of a subset: ids with fill, reported ids, labels
    and the pad(collate_pyg(...)) blob, computed once each."""

    def __init__(self, pkg, static, mols, y, indices):
        self.pkg, self.static, self.mols, self.y = pkg, static, mols, y
        self.batches = batches_of(mols, indices, static.B)
        self.steps = len(self.batches)
        self._blobs = {}

    def blob(self, j):
        j %= self.steps
        if j not in self._blobs:
            self._blobs[j] = pad_blob(self.pkg, self.static, self.mols, self.batches[j][0])
        return self._blobs[j]

    def marked(self, j):
        return self.batches[j % self.steps][1]

    def labels(self, j):
        return labels_of(self.y, self.marked(j))


def _check_primed(evl, exp):
    torch.cuda.synchronize()
    for s in range(3):
        assert torch.equal(evl.slots[s], exp.blob(s)), f"slot {s} after prime"
    assert evl.pool["cursor"].tolist() == [0, 0] and int(evl.state[0]) == 0


def _check_step(evl, static, exp, t, errors=0):
    """After step t's load_next + collate_ahead, t counted from prime(): the
    static batch holds batch t mod steps, the three slots in ring order hold
    batches t, t + 1, t + 2 mod steps, labels and ids are batch t's."""
    torch.cuda.synchronize()
    assert torch.equal(static.blob, exp.blob(t)), f"static batch at step {t}"
    c = int(evl.pool["cursor"][0]) - 1  # the slot load_next read
    for j in range(3):
        assert torch.equal(evl.slots[(c + j) % 3], exp.blob(t + j)), f"slot +{j} at step {t}"
    assert evl.ids.cpu().tolist() == exp.marked(t).tolist(), f"ids at step {t}"
    if exp.y is not None:
        assert same_bits(evl.labels.cpu().numpy(), exp.labels(t)), f"labels at step {t}"
    assert int(evl.state[0]) == (t + 1) % exp.steps
    assert evl.error() == errors


def _walk(pkg, dev, mols, y, B, indices, k=1, passes=2):
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, k, labels=y)
    static = eval_static(pkg, ds, B, dev, indices)
    evl = pkg.graph.DeviceEvalLoader(ds, static, indices=indices)
    exp = _Expect(pkg, static, mols, y, np.arange(len(mols)) if indices is None else indices)
    assert evl.steps == exp.steps
    evl.prime()
    _check_primed(evl, exp)
    for t in range(passes * exp.steps):
        static.load_next(evl.pool)
        evl.collate_ahead()
        _check_step(evl, static, exp, t)
    return evl, exp


@pytest.mark.parametrize("M,B", [(10, 3), (3, 5), (5, 5), (16, 8), (7, 8), (777, 259)])
def test_sequential_bitwise_tiny(pkg, dev, M, B):
    """steps of 4, 1, 1, 2, 1 and 3; a tail of 1, 3, 0, 0, 7 and 0 real rows;
    B = 259 puts the plan launch on two waves.  The static batch is sized
    exactly (capacities "sequential"), so the largest batch fills it."""
    mols, y = tiny_set(M)
    evl, exp = _walk(pkg, dev, mols, y, B, None)
    assert exp.steps == -(-M // B)
    assert (exp.marked(exp.steps - 1) < 0).sum() == exp.steps * B - M


@pytest.mark.parametrize("M,B", [(10, 3), (3, 5), (5, 5), (16, 8), (7, 8), (777, 259)])
def test_sequential_bitwise_f11(pkg, dev, M, B):
    """F = 11: feature rows that are no whole 16-byte words."""
    sizes = np.random.default_rng(M).integers(2, 5 if M > 100 else 9, size=M)
    mols, y = sized_set(sizes)
    _walk(pkg, dev, mols, y, B, None)


@pytest.mark.parametrize("k", [1, 2])
def test_sequential_bitwise_k(pkg, dev, k):
    mols, y = tiny_set(16)
    _walk(pkg, dev, mols, y, 8, None, k=k)


@pytest.mark.parametrize("T", [0, 1, 3])
def test_sequential_label_widths(pkg, dev, T):
    mols, _ = tiny_set(10)
    y = None if T == 0 else labels_with_nans(10, T, 5)
    evl, _ = _walk(pkg, dev, mols, y, 3, None)
    assert tuple(evl.labels.shape) == (3, T)


def test_subset_not_a_prefix_handmade(pkg, dev):
    """[5, 3, 0, 5]: a repeated id, and ids at or above the list's length (a
    clamp against the list's length instead of the dataset's would turn 5
    into 3).  Fill: molecule 0 (two atoms, one bond) before 3 (a self loop more)."""
    mols, y = handmade_set()
    evl, exp = _walk(pkg, dev, mols, y, 3, np.array([5, 3, 0, 5]))
    assert evl.fill_id == 0 and exp.marked(1).tolist() == [5, -1, -1]


def test_subset_not_a_prefix_tiny(pkg, dev):
    mols, y = tiny_set(40)
    _walk(pkg, dev, mols, y, 6, np.arange(39, 0, -2))


@pytest.mark.parametrize("case", ["handmade", "tiny"])
def test_training_loader_over_a_subset(pkg, dev, case):
    """DeviceLoader(indices=...): the shuffled batches of the subset's ids,
    byte for byte, with ids above the subset's length."""
    from test_gpu_loader import _Expect as TrainExpect, _check_step as check_train_step
    if case == "handmade":
        (mols, y), idx, B = handmade_set(), np.array([5, 3, 0, 5]), 1
    else:
        (mols, y), idx, B = tiny_set(40), np.arange(39, 0, -2), 3
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, 1, labels=y)
    static = static_for(pkg, ds, B, dev)
    loader = pkg.graph.DeviceLoader(ds, static, seed=6, indices=idx)
    exp = TrainExpect(pkg, static, mols, loader)
    loader.prime()
    S = loader.steps_per_epoch
    seen = []
    for t in range(2 * S + 1):
        if t and t % S == 0:
            loader.begin_epoch(t // S)
        static.load_next(loader.pool)
        loader.collate_ahead()
        check_train_step(loader, static, exp, y, t)
        seen += loader.ids.cpu().tolist()
    assert set(seen) <= set(idx.tolist()) and max(seen) >= len(idx)


def test_set_subset_under_one_captured_graph(pkg, dev):
    """load_next + collate_ahead captured once over subset A; set_subset to a
    longer and then a shorter list, each replayed for a pass and a step more,
    without recapture."""
    mols, y = tiny_set(40)
    a, b, c = np.arange(0, 20, 2), np.arange(39, 8, -1), np.array([7, 7, 30])
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, 1, labels=y)
    static = eval_static(pkg, ds, 4, dev, [a, b, c])
    evl = pkg.graph.DeviceEvalLoader(ds, static, indices=a, max_len=len(b))
    evl.prime()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static.load_next(evl.pool)
        evl.collate_ahead()
    torch.cuda.synchronize()
    for n, sub in enumerate((a, b, c)):
        if n:
            evl.set_subset(sub)
        exp = _Expect(pkg, static, mols, y, sub)
        assert evl.steps == exp.steps == -(-len(sub) // 4)
        _check_primed(evl, exp)
        for t in range(exp.steps + 1):
            graph.replay()
            _check_step(evl, static, exp, t)
    with pytest.raises(pkg._lib.ScgibError, match="max_len"):
        evl.set_subset(np.arange(40))


def test_overflow_marks_the_slot(pkg, dev):
    """Batch 3 (two 40-atom paths) is above the node capacity.  The step that
    would build it writes nothing: the whole ring allocation is unchanged, the
    count is 1.  The step that then scores slot 0's stale bytes (batch 0's)
    reports ids of -1 and NaN labels; batches 4 and 5 collate normally."""
    mols, y = sized_set([5, 6, 7, 4, 3, 8, 40, 40, 9, 3, 4, 5])
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, 1, labels=y)
    caps = ds.capacities(2, "sequential")
    assert caps[0] == 80
    static = pkg.graph.StaticBatch(2, 20, caps[1], ds.num_features, caps[2], caps[3], dev, 1)
    evl = pkg.graph.DeviceEvalLoader(ds, static)
    exp = _Expect(pkg, static, mols, y, np.arange(12))
    evl.prime()
    _check_primed(evl, exp)
    static.load_next(evl.pool)
    evl.collate_ahead()
    _check_step(evl, static, exp, 0)
    before = evl.ring.clone()
    static.load_next(evl.pool)
    evl.collate_ahead()  # step 1: batch 3 -> slot 0 does not fit
    torch.cuda.synchronize()
    assert evl.error() == 1 and torch.equal(evl.ring, before)
    assert torch.equal(static.blob, exp.blob(1)) and evl.ids.cpu().tolist() == [2, 3]
    assert same_bits(evl.labels.cpu().numpy(), y[[2, 3]])
    static.load_next(evl.pool)
    evl.collate_ahead()  # step 2: batch 4 -> slot 1
    torch.cuda.synchronize()
    assert evl.error() == 1 and evl.ids.cpu().tolist() == [4, 5]
    assert torch.equal(evl.slots[1], exp.blob(4)) and torch.equal(evl.slots[2], exp.blob(2))
    assert torch.equal(evl.slots[0], exp.blob(0))
    static.load_next(evl.pool)
    evl.collate_ahead()  # step 3 scores slot 0: batch 0's bytes, nothing labelled
    torch.cuda.synchronize()
    assert torch.equal(static.blob, exp.blob(0))
    assert evl.ids.cpu().tolist() == [-1, -1] and np.isnan(evl.labels.cpu().numpy()).all()
    assert torch.equal(evl.slots[2], exp.blob(5)) and evl.error() == 1
    static.load_next(evl.pool)
    evl.collate_ahead()  # step 4: batch 4 scored, batch 0 (the next pass) -> slot 0
    torch.cuda.synchronize()
    assert evl.ids.cpu().tolist() == [8, 9] and same_bits(evl.labels.cpu().numpy(), y[[8, 9]])
    assert torch.equal(evl.slots[0], exp.blob(0)) and evl.error() == 1
    # a primed batch that does not fit is refused eagerly; the count is kept
    with pytest.raises(pkg._lib.ScgibError, match="do not fit"):
        evl.set_subset([6, 7])
    assert evl.error() == 4  # the one batch, primed into each of the three slots


# ---------------------------------------------------------------------------
# an evaluation pass fed by the loader against the same pass fed by a fixed pool
# ---------------------------------------------------------------------------
B_E2E, T_E2E, K_E2E = 8, 2, 1


@pytest.fixture(scope="module")
def e2e(pkg, dev):
    """60 QM9-like molecules, binary labels with NaNs, a 27-id subset; a
    fine-tune model (GIN 64 x 5) after two training steps, in eval()."""
    mols = pkg.synth.molecules(60, "qm9", seed=5)
    mols = [(ei, F.normalize(torch.from_numpy(np.asarray(x, np.float32))).numpy()) for ei, x in mols]
    raw = labels_with_nans(60, T_E2E, 6)
    y = np.where(np.isnan(raw), np.nan, (raw > 0).astype(np.float32)).astype(np.float32)
    idx = np.random.default_rng(8).permutation(60)[:27]
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, K_E2E, labels=y)
    static = eval_static(pkg, ds, B_E2E, dev, idx)
    f_in = ds.num_features
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=B_E2E, gin_layers=5, task="graph_classification",
                           dataset="ogbg-molpcba", device=dev)
    torch.manual_seed(5)
    inner = pkg.models.Mainmodel(args, f_in, 64, 4, 4, K_E2E, "GIN")
    pre = pkg.models.Mainmodel_continue(args, f_in, 64, 4, 4, K_E2E, T_E2E, inner, "GIN")
    ft = pkg.models.Mainmodel_finetuning(args, f_in, 64, 4, 4, K_E2E, T_E2E, pre, "GIN")
    ft = ft.to(dev).train()
    opt = pkg.optim.Adam([p for p in ft.parameters() if p.requires_grad], lr=1e-3)
    pkg.ops.seed_noise(dev, 99)
    for ids in (np.arange(8), np.arange(8, 16)):  # running statistics off their initial values
        g = pkg.graph.collate_pyg([mols[i] for i in ids])[0].to(dev)
        opt.zero_grad(set_to_none=True)
        scores, *_ = ft(g, g.ndata["x"].float(), None, None, 1, None, K_E2E, dev, B_E2E)
        target = torch.from_numpy(np.nan_to_num(y[ids])).to(dev)
        ft.loss(scores, target).backward()
        opt.step()
    torch.cuda.synchronize()
    return SimpleNamespace(mols=mols, y=y, idx=idx, ds=ds, static=static, ft=ft.eval())


def _eval_pass(pkg, dev, c, pool, evl, labels_for, steps):
    """The captured evaluation step -- load_next, collate_ahead (loader-fed),
    forward under no_grad, EvalBuffer.append -- replayed ``steps`` times over
    ``pool``.  Pool-fed: the test writes each step's labels into the tensor the
    captured append reads.  Returns per-step scores and the buffer."""
    static, ft = c.static, c.ft
    pf = pkg.graph.EgoPrefetch(static, pool)
    buf = pkg.metrics.EvalBuffer(steps * B_E2E, T_E2E, dev)
    lab = evl.labels if evl is not None else torch.zeros(B_E2E, T_E2E, device=dev)

    def body():
        static.load_next(pool, pf)
        if evl is not None:
            evl.collate_ahead()
        with torch.no_grad():
            scores, *_ = ft(static.graph, static.x, None, None, 1, None, K_E2E, dev, B_E2E)
        buf.append(scores, lab)
        pf.join()
        return scores

    def rewind():
        if evl is not None:
            evl.prime()
        pool["cursor"].zero_()
        pf.prime()
        buf.reset()
        pkg.ops.seed_noise(dev, 4242)

    rewind()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up (allocator, lazy workspaces)
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    rewind()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body()
    scores = []
    for t in range(steps):
        if evl is None:
            lab.copy_(torch.from_numpy(labels_for(t)))
        graph.replay()
        torch.cuda.synchronize()
        scores.append(out.clone())
    assert static.ego_error() == 0 and pf.error() == 0
    return torch.stack(scores), buf


def _padded_pool(pkg, c, batch_ids):
    padded = [{"blob": pad_blob(pkg, c.static, c.mols, ids)} for ids in batch_ids]
    return padded, c.static.pool(padded)


@pytest.fixture(scope="module")
def e2e_runs(pkg, dev, e2e):
    c = e2e
    evl = pkg.graph.DeviceEvalLoader(c.ds, c.static, indices=c.idx)
    batches = batches_of(c.mols, c.idx, B_E2E)
    got = _eval_pass(pkg, dev, c, evl.pool, evl, None, evl.steps)
    assert evl.error() == 0
    keep, pool = _padded_pool(pkg, c, [ids for ids, _ in batches])
    ref = _eval_pass(pkg, dev, c, pool, None, lambda t: labels_of(c.y, batches[t][1]),
                     len(batches))
    return SimpleNamespace(evl=evl, batches=batches, got=got, ref=ref, keep=keep)


def test_eval_pass_fed_by_loader_equals_fixed_pool(pkg, dev, e2e, e2e_runs):
    """27 molecules in 4 batches of 8: scores and per-task metric tensors
    bitwise those of the pass over the host-padded batches, every molecule of
    the subset labelled once (the last three sit in the partial batch)."""
    from test_gpu_eval_metrics import same_bits as same_metric_bits
    c, r = e2e, e2e_runs
    (s_got, b_got), (s_ref, b_ref) = r.got, r.ref
    assert r.evl.steps == 4 and torch.isfinite(s_got).all()
    assert torch.equal(s_got, s_ref)
    assert b_got.rows() == b_ref.rows() == 4 * B_E2E
    assert torch.equal(b_got.scores, b_ref.scores)
    assert same_bits(b_got.labels.cpu().numpy(), b_ref.labels.cpu().numpy())
    m_got, m_ref = b_got.per_task(), b_ref.per_task()
    assert same_metric_bits(m_got, m_ref)
    want = (~np.isnan(c.y[c.idx])).sum(axis=0)
    assert m_got["labelled"].cpu().tolist() == want.tolist()
    assert want.sum() > (~np.isnan(c.y[c.idx[:24]])).sum()  # the tail carries labels


def test_eval_pass_metrics_equal_host_functions(pkg, dev, e2e, e2e_runs):
    """rocauc() / rmse() of the loader-fed buffer against metrics.eval_* on the
    same scores and the subset's labels (test_gpu_eval_metrics' bounds)."""
    pytest.importorskip("sklearn")
    from test_gpu_eval_metrics import ABS, REL
    c, (scores, buf) = e2e, e2e_runs.got
    s = scores.reshape(-1, T_E2E)[:27].cpu().numpy().astype(np.float64)
    y = c.y[c.idx]
    assert abs(buf.rocauc()["rocauc"] - pkg.metrics.eval_rocauc(y, s)["rocauc"]) <= ABS
    want = pkg.metrics.eval_rmse(y, s)["rmse"]
    assert abs(buf.rmse()["rmse"] - want) <= REL * want


def test_fill_molecule_does_not_touch_real_rows(pkg, dev, e2e, e2e_runs):
    """The tail batch scored with the loader's fill molecule and with another
    one (hand-padded): in eval mode the three real rows' scores are equal."""
    c, r = e2e, e2e_runs
    ids, marked = r.batches[-1]
    real = int((marked >= 0).sum())
    assert real == 3
    counts = c.ds.node_counts
    other = int(min((i for i in range(len(counts)) if counts[i] > counts[ids[-1]]),
                    key=lambda i: (counts[i], i)))  # the smallest molecule above the fill's size
    alt = ids.copy()
    alt[real:] = other
    out = []
    for batch in (ids, alt):
        keep, pool = _padded_pool(pkg, c, [batch])
        scores, _ = _eval_pass(pkg, dev, c, pool, None, lambda t: labels_of(c.y, marked), 1)
        out.append(scores[0])
    # (both are the first step after the same seed: the interaction's noise is
    # drawn per step, so the pass's fourth step is no reference for these)
    assert torch.equal(out[0][:real], out[1][:real])
    assert not torch.equal(out[0][real:], out[1][real:])


def test_training_fed_by_subset_loader_equals_fixed_pool(pkg, dev, monkeypatch):
    """The pattern of test_training_fed_by_loader_equals_fixed_pool at B = 3,
    six steps, with the loader over 10 ids of a 24-molecule dataset."""
    from test_gpu_graph_split import _assert_bitwise
    from test_gpu_loader import _train
    from loader_cases import qm9_set
    mols, y = qm9_set(pkg, M=24, seed=37, T=1)
    idx = np.array([23, 4, 17, 9, 22, 11, 0, 19, 14, 6])
    whole = pkg.graph.DeviceLoader
    # _train builds its loader as DeviceLoader(ds, static, seed=...): give it the subset
    monkeypatch.setattr(pkg.graph, "DeviceLoader",
                        lambda ds, static, **kw: whole(ds, static, indices=idx, **kw))
    ref = _train(pkg, dev, mols, y, "pool", split=False)
    got = _train(pkg, dev, mols, y, "loader", split=False)
    assert torch.isfinite(ref.losses).all()
    assert torch.equal(got.losses, ref.losses), (got.losses, ref.losses)
    _assert_bitwise(got.state, ref.state)
    assert set(got.ids) <= set(idx.tolist()) and got.ids == got.expected_ids
