"""graph.DeviceLoader on the MI355X (csrc/collate.hip): every
ring slot the two launches write against StaticBatch.pad of the host-collated
batch the sequence formula predicts, byte for byte over the whole slot; stale
tails, overflow, capture, a training run against the fixed pool, determinism."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from loader_cases import (handmade_set, pad_blob, qm9_set, same_bits, sized_set, static_for,
                          tiny_set)

pytestmark = pytest.mark.gpu
STEPS = 7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _setup(pkg, dev, mols, y, B, k=1, static=None, **kw):
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, k, labels=y)
    static = static or static_for(pkg, ds, B, dev)
    return ds, static, pkg.graph.DeviceLoader(ds, static, **kw)


def _ids(loader, j, repeat=False):
    """Molecule ids of global batch j; repeat: begin_epoch never called, so the
    two permutation buffers repeat."""
    if not repeat:
        return loader.batch_ids(j)
    S, B = loader.steps_per_epoch, loader.B
    return loader.epoch_permutation((j // S) % 2)[(j % S) * B:(j % S) * B + B]


class _Expect:
    """pad(collate_pyg(...)) blobs of the predicted batches, computed once each."""

    def __init__(self, pkg, static, mols, loader, repeat=False):
        self.pkg, self.static, self.mols, self.loader, self.repeat = pkg, static, mols, loader, repeat
        self._blobs = {}

    def ids(self, j):
        return _ids(self.loader, j, self.repeat)

    def __call__(self, j):
        if j not in self._blobs:
            self._blobs[j] = pad_blob(self.pkg, self.static, self.mols, self.ids(j))
        return self._blobs[j]


def _check_step(loader, static, exp, y, t):
    """After step t's load_next + collate_ahead: the static batch and slot
    t % 3 hold batch t, slot (t + 1) % 3 batch t + 1, and the slot just written
    batch t + 2; labels and ids are batch t's."""
    torch.cuda.synchronize()
    assert torch.equal(static.blob, exp(t)), f"static batch at step {t}"
    for j in (t, t + 1, t + 2):
        assert torch.equal(loader.slots[j % 3], exp(j)), f"slot {j % 3} at step {t}"
    ids = exp.ids(t)
    assert loader.ids.cpu().tolist() == ids.tolist()
    assert same_bits(loader.labels.cpu().numpy(), y[ids])
    assert loader.error() == 0


def _walk(pkg, dev, mols, y, B, k=1, steps=STEPS, seed=3):
    ds, static, loader = _setup(pkg, dev, mols, y, B, k, seed=seed)
    exp = _Expect(pkg, static, mols, loader)
    loader.prime()
    torch.cuda.synchronize()
    assert torch.equal(loader.slots[0], exp(0)) and torch.equal(loader.slots[1], exp(1))
    S = loader.steps_per_epoch
    for t in range(steps):
        if t and t % S == 0:
            loader.begin_epoch(t // S)
        static.load_next(loader.pool)
        loader.collate_ahead()
        _check_step(loader, static, exp, y, t)
    assert loader.pool["cursor"].tolist() == [steps, 0]
    return loader


def test_collation_bitwise_m10_b3(pkg, dev):
    """S = 3, one molecule dropped per epoch; 7 steps cross two epoch boundaries."""
    mols, y = qm9_set(pkg, M=10, seed=11, T=2)
    loader = _walk(pkg, dev, mols, y, 3)
    assert loader.steps_per_epoch == 3
    assert int(loader.state[0]) == STEPS % 6


@pytest.mark.parametrize("k", [1, 2])
def test_collation_bitwise_m60_b8(pkg, dev, k):
    mols, y = qm9_set(pkg)
    _walk(pkg, dev, mols, y, 8, k=k)


def test_collation_bitwise_b1(pkg, dev):
    mols, y = qm9_set(pkg, M=7, seed=17, T=1)
    _walk(pkg, dev, mols, y, 1)


def test_collation_bitwise_b1030(pkg, dev):
    """More molecules than the widest workgroup has threads (1,024): the plan
    launch's scan takes several molecules per thread and several waves."""
    mols, y = tiny_set(3 * 1030 + 5)
    _walk(pkg, dev, mols, y, 1030)


def test_collation_bitwise_handmade(pkg, dev):
    """Two atoms, an empty CSR row, a 512-atom path, a self loop; F = 8 takes
    the 16-byte feature path."""
    mols, y = handmade_set()
    _walk(pkg, dev, mols, y, 2)


def test_no_stale_tails_after_a_larger_batch(pkg, dev):
    """Slot 0 holds batch 0 (two 30-atom paths), then batch 3 (two 2-atom
    molecules): nothing of the larger batch survives in rowptr, col or x."""
    mols, y = sized_set([30, 30, 5, 6, 7, 4, 2, 2, 9, 3, 4, 5])
    ds, static, loader = _setup(pkg, dev, mols, y, 2, shuffle=False)
    exp = _Expect(pkg, static, mols, loader)
    loader.prime()
    for t in range(4):
        static.load_next(loader.pool)
        loader.collate_ahead()
        _check_step(loader, static, exp, y, t)
    torch.cuda.synchronize()
    assert torch.equal(loader.slots[0], exp(3))
    o = static._layout()
    rowptr = loader.slots[0][o[0]:o[0] + 4 * (static.n_cap + 1)].view(torch.int32).cpu()
    assert rowptr[4:].eq(4).all()  # n = 4, e = 4: the tail is e
    assert not loader.slots[0][o[1] + 4 * 4:o[2]].any() and not loader.slots[0][o[4] + 4 * 4 * 11:].any()


def test_overflow_leaves_the_ring_alone(pkg, dev):
    """Batch 3 (two 40-atom paths) is above the node capacity: its launch
    writes nothing — slot 0 keeps batch 0's bytes, slots 1 and 2 (neighbours in
    the one allocation) keep theirs — the error count is 1, labels and ids
    follow what the slot holds, and batch 4 collates normally."""
    mols, y = sized_set([5, 6, 7, 4, 3, 8, 40, 40, 9, 3, 4, 5])
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, 1, labels=y)
    caps = ds.capacities(2, "worst")
    static = pkg.graph.StaticBatch(2, 20, caps[1], ds.num_features, caps[2], caps[3], dev, 1)
    loader = pkg.graph.DeviceLoader(ds, static, shuffle=False)
    exp = _Expect(pkg, static, mols, loader)
    loader.prime()
    for t in (0,):
        static.load_next(loader.pool)
        loader.collate_ahead()
        _check_step(loader, static, exp, y, t)
    before = loader.ring.clone()
    static.load_next(loader.pool)
    loader.collate_ahead()  # step 1: batch 3 -> slot 0 does not fit
    torch.cuda.synchronize()
    assert loader.error() == 1
    assert torch.equal(loader.ring, before)
    assert torch.equal(static.blob, exp(1)) and loader.ids.cpu().tolist() == [2, 3]
    static.load_next(loader.pool)
    loader.collate_ahead()  # step 2: batch 4 -> slot 1
    torch.cuda.synchronize()
    assert loader.error() == 1
    assert torch.equal(loader.slots[1], exp(4)) and torch.equal(loader.slots[2], exp(2))
    assert torch.equal(loader.slots[0], exp(0))
    static.load_next(loader.pool)
    loader.collate_ahead()  # step 3 trains on slot 0: batch 0 again, with batch 0's labels
    torch.cuda.synchronize()
    assert torch.equal(static.blob, exp(0)) and loader.ids.cpu().tolist() == [0, 1]
    assert same_bits(loader.labels.cpu().numpy(), y[[0, 1]])
    assert torch.equal(loader.slots[2], exp(5)) and loader.error() == 1


@pytest.mark.parametrize("epochs", ["begin_epoch", "never"])
def test_captured_load_and_collate(pkg, dev, epochs):
    """load_next + collate_ahead under torch.cuda.graph, 7 replays at M = 10,
    B = 3; begin_epoch between epochs, or never (the two buffers repeat)."""
    mols, y = qm9_set(pkg, M=10, seed=23, T=2)
    ds, static, loader = _setup(pkg, dev, mols, y, 3, seed=8)
    exp = _Expect(pkg, static, mols, loader, repeat=epochs == "never")
    loader.prime()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static.load_next(loader.pool)
        loader.collate_ahead()
    torch.cuda.synchronize()
    assert loader.pool["cursor"].tolist() == [0, 0]  # (the capture ran nothing)
    for t in range(STEPS):
        if epochs == "begin_epoch" and t and t % 3 == 0:
            loader.begin_epoch(t // 3)
        graph.replay()
        _check_step(loader, static, exp, y, t)
    if epochs == "never":  # epoch 2 repeated epoch 0's batches
        assert torch.equal(exp(6), exp(0))


def test_two_loaders_same_seed_same_blobs(pkg, dev):
    mols, y = qm9_set(pkg, M=30, seed=29, T=1)
    rings = []
    for _ in range(2):
        ds, static, loader = _setup(pkg, dev, mols, y, 4, seed=12)
        loader.prime()
        got = []
        for t in range(STEPS):
            if t and t % loader.steps_per_epoch == 0:
                loader.begin_epoch(t // loader.steps_per_epoch)
            static.load_next(loader.pool)
            loader.collate_ahead()
            torch.cuda.synchronize()
            got.append((loader.ring.clone(), static.blob.clone(), loader.labels.clone(),
                        loader.ids.clone()))
        rings.append(got)
    for a, b in zip(*rings):
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.uint8).reshape(-1), v.view(torch.uint8).reshape(-1))
    other = _setup(pkg, dev, mols, y, 4, seed=13)[2]
    other.prime()
    torch.cuda.synchronize()
    assert not torch.equal(other.ring, rings[0][0][0])


# ---------------------------------------------------------------------------
# a training run fed by the loader against the same run fed by a fixed pool
# ---------------------------------------------------------------------------
def _train(pkg, dev, mols, y, feed, split, steps=6, warm=2, B=3, k=1, ride=False):
    """Mainmodel_continue (GIN-64x5), captured step with EgoPrefetch and Adam:
    ``warm`` eager steps, then the capture and steps - warm replays (whole
    graph, or as ops.SplitGraph's two lanes).  feed "loader": batches collated
    by the DeviceLoader; "pool": StaticBatch.pool of the same batches padded on
    the host.  Returns per-step losses and the final model / optimizer state."""
    from test_gpu_graph_split import _state
    from test_gpu_trajectory import _pretrain_model
    import torch.nn.functional as F
    mols = [(ei, F.normalize(torch.from_numpy(x)).numpy()) for ei, x in mols]
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, k, labels=y)
    static = static_for(pkg, ds, B, dev)
    loader = pkg.graph.DeviceLoader(ds, static, seed=31)
    model = _pretrain_model(pkg, ds.num_features, k, B, dev)
    opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
    pkg.ops.seed_noise(dev, 4242)
    padded = None
    if feed == "loader":
        loader.prime()
        pool = loader.pool
    else:
        padded = [{"blob": pad_blob(pkg, static, mols, loader.batch_ids(j))} for j in range(steps)]
        pool = static.pool(padded)
    pf = pkg.graph.EgoPrefetch(static, pool)
    pf.prime()
    if ride:  # collate_ahead on the ego prefetch's queue instead of the main one
        loader.ride(pf)
    one = torch.ones((), device=dev)

    def body():
        static.load_next(pool, pf)
        if feed == "loader" and not ride:
            loader.collate_ahead()
        _, kl, con, rec = model(static.graph, static.x, None, None, None, 1, None, k, dev, B)
        torch.autograd.backward((kl, rec, con), (one, one, one))
        pf.join()
        opt.step()
        return torch.stack([kl.detach(), rec.detach(), con.detach()])

    losses = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            opt.zero_grad(set_to_none=True)
            losses.append(body().clone())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        out = body()
    lanes = None
    try:
        if split:
            lanes = pkg.ops.SplitGraph(graph, dev)
        else:
            graph.instantiate()
        S = loader.steps_per_epoch
        for t in range(warm, steps):
            if feed == "loader" and t % S == 0:
                loader.begin_epoch(t // S)
            lanes.replay() if lanes is not None else graph.replay()
            torch.cuda.synchronize()
            losses.append(out.clone())
        assert pkg.ops.xq_timeouts(dev) == 0
        assert static.ego_error() == 0 and pf.error() == 0 and loader.error() == 0
        return SimpleNamespace(losses=torch.stack(losses), state=_state(model, opt), keep=(padded, one),
                               ids=loader.ids.cpu().tolist() if feed == "loader" else None,
                               expected_ids=loader.batch_ids(steps - 1).tolist())
    finally:
        torch.cuda.synchronize()
        if lanes is not None:
            lanes.close()


@pytest.fixture(scope="module")
def pool_run(pkg, dev):
    mols, y = qm9_set(pkg, M=10, seed=37, T=1)
    return mols, y, _train(pkg, dev, mols, y, "pool", split=False)


def test_training_fed_by_loader_equals_fixed_pool(pkg, dev, pool_run):
    """6 steps over M = 10, B = 3 (two epochs): per-step losses and the final
    parameters, BN buffers and Adam state bitwise equal to the same step fed
    by StaticBatch.pool of the six host-padded batches in the predicted order."""
    from test_gpu_graph_split import _assert_bitwise
    mols, y, ref = pool_run
    got = _train(pkg, dev, mols, y, "loader", split=False)
    assert torch.isfinite(ref.losses).all()
    assert torch.equal(got.losses, ref.losses), (got.losses, ref.losses)
    _assert_bitwise(got.state, ref.state)


@pytest.mark.parametrize("split", [False, True], ids=["whole", "lanes"])
def test_training_with_collate_on_the_prefetch_queue(pkg, dev, pool_run, split):
    """DeviceLoader.ride: collate_ahead behind the ego prefetch on its queue
    gives the same run, and the ids of the last step's batch after the join."""
    from test_gpu_graph_split import _assert_bitwise
    if split and not pkg.ops.xq_enabled():
        pytest.skip(f"hand-offs off here: {pkg.ops.XQ_REASON}")
    mols, y, ref = pool_run
    got = _train(pkg, dev, mols, y, "loader", split=split, ride=True)
    assert torch.equal(got.losses, ref.losses), (got.losses, ref.losses)
    _assert_bitwise(got.state, ref.state)
    assert got.ids == got.expected_ids


def test_training_fed_by_loader_split_replay(pkg, dev, pool_run):
    """... and replayed as ops.SplitGraph's two lanes: the same loss sequence."""
    from test_gpu_graph_split import _assert_bitwise
    if not pkg.ops.xq_enabled():
        pytest.skip(f"hand-offs off here: {pkg.ops.XQ_REASON}")
    mols, y, ref = pool_run
    got = _train(pkg, dev, mols, y, "loader", split=True)
    assert torch.equal(got.losses, ref.losses), (got.losses, ref.losses)
    _assert_bitwise(got.state, ref.state)
