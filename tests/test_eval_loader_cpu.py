"""graph.DeviceEvalLoader, DeviceLoader(indices=...) and
DeviceDataset.capacities("sequential") on the host: the
sequential batches with their fill molecule, the capacities against a brute
force over collate_pyg, the subset permutations, refusals, the entry points."""
import ctypes

import numpy as np
import pytest

from eval_loader_cases import batches_of, brute_capacities, eval_static, fill_of, labels_of
from loader_cases import pad_blob, qm9_set, same_bits, static_for, tiny_set


@pytest.mark.parametrize("M,B", [(16, 8), (9, 4), (7, 8), (15, 8), (3, 5), (5, 5)],
                         ids=["rem0", "rem1", "M=B-1", "remB-1", "M<B", "M=B"])
def test_sequential_ids_and_fill(pkg, M, B):
    """M % B in {0, 1, B - 1} and M < B: the host mirror's batch ids, fill id,
    labels and blob against collate_pyg + pad of the expected molecules."""
    G = pkg.graph
    mols, y = tiny_set(20)
    ds = G.DeviceDataset.from_molecules(mols, "cpu", 1, labels=y)
    sub = np.random.default_rng(M * 31 + B).permutation(20)[:M]
    want = batches_of(mols, sub, B)
    rows, marked = G.sequential_ids(ds, sub, B)
    assert rows.shape == marked.shape == (-(-M // B), B)
    assert G.sequential_fill_id(ds, sub) == fill_of(mols, sub)
    static = eval_static(pkg, ds, B, "cpu", sub)
    evl = G.DeviceEvalLoader(ds, static, indices=sub)
    assert evl.steps == len(want) and evl.M == M and evl.fill_id == fill_of(mols, sub)
    for j, (ids, rep) in enumerate(want):
        assert rows[j].tolist() == ids.tolist() and marked[j].tolist() == rep.tolist()
        got = evl.batch_ids(j + evl.steps)  # cyclic
        assert got[0].tolist() == ids.tolist() and got[1].tolist() == rep.tolist()
        blob, labels, out = G.sequential_blob_host(ds, sub, j, static)
        assert np.array_equal(blob, pad_blob(pkg, static, mols, ids).numpy())
        assert same_bits(labels, labels_of(y, rep))
        assert out.dtype == np.int32 and out.tolist() == rep.tolist()
    assert (marked[:-1] >= 0).all() and (marked[-1] < 0).sum() == len(want) * B - M


def test_fill_ties_break_by_edges_then_id(pkg):
    """Among equal atom counts the fewest edges win (a 4-atom chain before a
    4-atom ring), then the lowest id, not the first in list order."""
    G = pkg.graph
    mols, _ = tiny_set(30)
    ds = G.DeviceDataset.from_molecules(mols, "cpu", 1)
    four = [i for i in range(30) if ds.node_counts[i] == 4]
    ring = [i for i in four if ds.edge_counts[i] == 8]
    chain = [i for i in four if ds.edge_counts[i] == 6]
    assert ring and len(chain) >= 2
    sub = [ring[0], chain[-1], chain[0], chain[-1]]
    assert G.sequential_fill_id(ds, sub) == chain[0] == fill_of(mols, sub)


@pytest.mark.parametrize("k", [1, 2])
def test_sequential_capacities_are_the_brute_force_maxima(pkg, k):
    """M = 27, B = 8 of a 60-molecule set, one subset and two at once."""
    mols, y = qm9_set(pkg)
    ds = pkg.graph.DeviceDataset.from_molecules(mols, "cpu", k, labels=y)
    rng = np.random.default_rng(3)
    a, b = rng.permutation(60)[:27], rng.permutation(60)[:13]
    for subsets, arg in (([a], a), ([a, b], [a, b]), ([b], [b.tolist()])):
        n, e, mgn, (ns, es, dmax) = ds.capacities(8, "sequential", indices=arg)
        assert (n, e, ns, es) == brute_capacities(pkg, mols, subsets, 8, k)
        assert mgn == ds.max_graph_nodes
        assert dmax == (ds.max_in_degree if k == 1 else 1 << 30)
    one = ds.capacities(8, "sequential", indices=a)
    both = ds.capacities(8, "sequential", indices=[a, b])
    assert all(u <= v for u, v in zip(one[:2] + one[3][:2], both[:2] + both[3][:2]))
    whole = ds.capacities(8, "sequential")
    assert whole[:2] + whole[3][:2] == brute_capacities(pkg, mols, [np.arange(60)], 8, k)
    with pytest.raises(ValueError):
        ds.capacities(8, "worst", indices=a)


def test_epoch_permutation_over_a_subset(pkg):
    G = pkg.graph
    mols = pkg.synth.molecules(40, "qm9", seed=2)
    ds = G.DeviceDataset.from_molecules(mols, "cpu", 1)
    static = static_for(pkg, ds, 3, "cpu")
    idx = np.array([39, 37, 35, 33, 31, 29, 27, 25, 23, 21, 5, 5])
    sub = G.DeviceLoader(ds, static, seed=4, indices=idx)
    assert sub.M == 12 and sub.steps_per_epoch == 4
    for e in range(3):
        p = sub.epoch_permutation(e)
        assert sorted(p.tolist()) == sorted(idx.tolist())
        assert np.array_equal(p, idx[np.random.default_rng([4, e]).permutation(12)])
        assert sub.batch_ids(4 * e + 1).tolist() == p[3:6].tolist()
    plain = G.DeviceLoader(ds, static, shuffle=False, indices=idx)
    assert np.array_equal(plain.epoch_permutation(2), idx)
    whole = G.DeviceLoader(ds, static, seed=4)
    assert whole.indices is None and whole.M == 40
    for e in range(2):
        assert np.array_equal(whole.epoch_permutation(e),
                              np.random.default_rng([4, e]).permutation(40))
    # the descriptor: the permutation's length, and the dataset's for the clamp
    assert (sub._desc.M, sub._desc.S, sub._desc.D) == (12, 4, 40)
    assert (whole._desc.M, whole._desc.S, whole._desc.D) == (40, 13, 40)


def test_refusals(pkg):
    G, Err = pkg.graph, pkg._lib.ScgibError
    mols, y = tiny_set(12)
    ds = G.DeviceDataset.from_molecules(mols, "cpu", 1, labels=y)
    static = eval_static(pkg, ds, 4, "cpu")
    for bad in ([0, 12], [-1, 3]):
        with pytest.raises(Err, match="outside 0..11"):
            G.DeviceEvalLoader(ds, static, indices=bad)
        with pytest.raises(Err, match="outside 0..11"):
            G.DeviceLoader(ds, static, indices=bad * 6)
        with pytest.raises(Err, match="outside 0..11"):
            ds.capacities(4, "sequential", indices=bad)
    with pytest.raises(Err, match="empty subset"):
        G.DeviceEvalLoader(ds, static, indices=[])
    with pytest.raises(Err, match="1-D integer"):
        G.DeviceEvalLoader(ds, static, indices=[0.5, 1.0])
    with pytest.raises(Err, match="max_len"):
        G.DeviceEvalLoader(ds, static, indices=[0, 1, 2], max_len=2)
    evl = G.DeviceEvalLoader(ds, static, indices=[0, 1, 2], max_len=5)
    assert evl.max_len == 5 and evl.perm.numel() == 5
    with pytest.raises(Err, match="max_len"):
        evl.set_subset([0, 1, 2, 3, 4, 5])
    with pytest.raises(Err, match="empty subset"):
        evl.set_subset([])
    with pytest.raises(Err, match="HIP device"):  # a CPU device: no fallback
        evl.prime()
    with pytest.raises(Err, match="HIP device"):
        evl.set_subset([3, 4])
    assert evl.indices.tolist() == [0, 1, 2]  # a refused subset changes nothing
    assert G.DeviceEvalLoader(ds, static).M == 12  # the whole dataset, and steps < 3 is fine
    assert G.DeviceEvalLoader(ds, eval_static(pkg, ds, 12, "cpu")).steps == 1
    with pytest.raises(Err, match="at least 3"):  # the training loader still needs three batches
        G.DeviceLoader(ds, static, indices=np.arange(11))
    other = G.DeviceDataset.from_molecules(tiny_set(12, F=8)[0], "cpu", 1)
    with pytest.raises(Err, match="feature"):
        G.DeviceEvalLoader(other, static)


def test_sequential_entry_points_exported(pkg):
    """Entry points only: the ABI version and the descriptor's layout stay."""
    lib = pkg._lib.load()
    assert pkg._lib.ABI_VERSION == 24 and lib.scgib_abi_version() == 24
    for name in ("scgib_collate_seq_plan", "scgib_collate_seq_fill"):
        assert name in pkg._lib.SIGNATURES and getattr(lib, name) is not None
    assert ctypes.sizeof(pkg._lib.CollateDesc) == 16 * 8 + 12 * 8 + 4 * 4
    assert pkg._lib.CollateDesc.D.offset == 16 * 8 + 12 * 8 + 3 * 4
    # descriptors the entry points refuse before any launch
    assert lib.scgib_collate_seq_plan(ctypes.byref(pkg._lib.CollateDesc()), 0, 0, 0, None) == -1
    assert lib.scgib_collate_seq_fill(None, 0, None) == -1
    mols, y = tiny_set(12)
    ds = pkg.graph.DeviceDataset.from_molecules(mols, "cpu", 1, labels=y)
    evl = pkg.graph.DeviceEvalLoader(ds, eval_static(pkg, ds, 4, "cpu"))
    d = evl._desc
    assert (d.M, d.D) == (12, 12)
    assert lib.scgib_collate_seq_plan(ctypes.byref(d), 3, 0, 0, None) == -1  # ahead above 2
    d.D = 0  # a sequential descriptor names the dataset's size
    assert lib.scgib_collate_seq_plan(ctypes.byref(d), 0, 0, 0, None) == -1
    assert lib.scgib_collate_seq_fill(ctypes.byref(d), 0, None) == -1
