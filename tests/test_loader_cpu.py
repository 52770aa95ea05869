"""graph.DeviceDataset / DeviceLoader / collate_blob_host on the host
(DESIGN.md §14): the layout restatement against StaticBatch.pad byte for byte,
per-molecule ego bounds, capacities, the batch sequence, refusals, the ABI."""
import ctypes

import numpy as np
import pytest

from loader_cases import (handmade_set, pad_blob, path, qm9_set, same_bits, static_for)


@pytest.fixture(scope="module")
def qm9(pkg):
    mols, y = qm9_set(pkg)
    return mols, y, {k: pkg.graph.DeviceDataset.from_molecules(mols, "cpu", k, labels=y)
                     for k in (1, 2)}


def _check_blob(pkg, ds, mols, y, ids):
    static = static_for(pkg, ds, len(ids), "cpu")
    blob, labels, out_ids = pkg.graph.collate_blob_host(ds.host, ids, static)
    ref = pad_blob(pkg, static, mols, ids).numpy()
    assert blob.dtype == np.uint8 and blob.shape == ref.shape
    assert np.array_equal(blob, ref)
    assert same_bits(labels, y[np.asarray(ids)])
    assert np.isnan(labels).any() or len(ids) < 4
    assert out_ids.dtype == np.int32 and out_ids.tolist() == list(ids)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("ids", [[7], [59], [3, 17, 0, 44, 9, 21, 58, 30], [5, 5, 12, 5, 0, 12, 1, 2]],
                         ids=["B1", "B1-last", "B8", "B8-repeats"])
def test_blob_equals_pad_qm9(pkg, qm9, ids, k):
    mols, y, ds = qm9
    _check_blob(pkg, ds[k], mols, y, ids)


@pytest.mark.parametrize("ids", [[0, 1], [2, 0], [1, 2], [3, 4], [5, 2], [4, 4]])
def test_blob_equals_pad_handmade(pkg, ids):
    """A 2-atom molecule, an empty CSR row, a 512-atom path, a self loop."""
    mols, y = handmade_set()
    ds = pkg.graph.DeviceDataset.from_molecules(mols, "cpu", 1, labels=y)
    assert ds.max_graph_nodes == 512 and ds.num_tasks == 2
    _check_blob(pkg, ds, mols, y, ids)


def test_from_cache_equals_from_molecules(pkg, qm9, tmp_path):
    mols, y, ds = qm9
    cache = pkg.cache.write([(ei, x, yy) for (ei, x), yy in zip(mols, y)], str(tmp_path), "set")
    dc = pkg.graph.DeviceDataset.from_cache(cache, "cpu", 1)
    for key, v in ds[1].host.items():
        assert np.array_equal(np.asarray(dc.host[key]).view(np.uint8).reshape(-1),
                              np.asarray(v).view(np.uint8).reshape(-1)), key
    # ... and the stored rows reproduce CSRCache.collate
    ids = [4, 31, 4, 50]
    static = static_for(pkg, dc, len(ids), "cpu")
    g, labels, _ = cache.collate(ids)
    blob, lab, _ = pkg.graph.collate_blob_host(dc.host, ids, static)
    assert np.array_equal(blob, static.pad(g)["blob"].numpy())
    assert same_bits(lab, labels.numpy())


@pytest.mark.parametrize("k", [1, 2])
def test_molecule_ego_bounds_sum_to_batch_bounds(pkg, qm9, k):
    mols, _, ds = qm9
    hm, _ = handmade_set()
    dh = pkg.graph.DeviceDataset.from_molecules(hm, "cpu", k)
    for d, ms, idsets in ((ds[k], mols, ([0, 1, 2, 3, 4, 5, 6, 7], [9, 9, 40], list(range(60)))),
                          (dh, hm, ([0, 1, 3, 4, 5], [2, 3], [1]))):
        for ids in idsets:
            g, _ = pkg.graph.collate_pyg([ms[i] for i in ids])
            bn, be, dmax = pkg.graph.ego_bounds(g, k)
            assert int(d.host["ego_nodes"][ids].sum()) == bn
            assert int(d.host["ego_edges"][ids].sum()) == be
            assert dmax <= d.max_in_degree


def test_capacities_cover_sampled_batches(pkg, qm9):
    mols, _, ds = qm9
    d, B = ds[1], 8
    worst = d.capacities(B, "worst")
    rng = np.random.default_rng(0)
    for _ in range(20):
        ids = rng.choice(len(mols), B, replace=False)
        g, _ = pkg.graph.collate_pyg([mols[i] for i in ids])
        got = pkg.graph.StaticBatch.capacities([g], 1)
        assert got[0] <= worst[0] and got[1] <= worst[1] and got[2] <= worst[2]
        assert got[3][0] <= worst[3][0] and got[3][1] <= worst[3][1] and got[3][2] <= worst[3][2]
    for seed in range(4):
        s = d.capacities(B, "sampled", slack=1.0, seed=seed)
        assert s[0] <= worst[0] and s[1] <= worst[1] and s[2] == worst[2]
        assert s[3][0] <= worst[3][0] and s[3][1] <= worst[3][1] and s[3][2] == worst[3][2]
    assert ds[2].capacities(B, "worst")[3][2] == 1 << 30  # k >= 2: the bitmap builder
    assert d.capacities(B, "sampled", slack=1.5)[0] > d.capacities(B, "sampled", slack=1.0)[0]


def _loader(pkg, M, B, **kw):
    mols = pkg.synth.molecules(M, "qm9", seed=2)
    ds = pkg.graph.DeviceDataset.from_molecules(mols, "cpu", 1)
    return pkg.graph.DeviceLoader(ds, static_for(pkg, ds, B, "cpu"), **kw)


def test_epoch_permutations_and_batch_sequence(pkg):
    M, B = 10, 3
    a, b = _loader(pkg, M, B, seed=4), _loader(pkg, M, B, seed=4)
    other = _loader(pkg, M, B, seed=5)
    assert a.steps_per_epoch == 3
    perms = [a.epoch_permutation(e) for e in range(4)]
    for e, p in enumerate(perms):
        assert sorted(p.tolist()) == list(range(M))
        assert np.array_equal(p, b.epoch_permutation(e))
    assert len({tuple(p.tolist()) for p in perms}) == 4
    assert not np.array_equal(perms[0], other.epoch_permutation(0))
    for j in range(12):  # batch j = perm_{j // S}[(j mod S) * B : + B]; the tenth molecule is dropped
        e, s = divmod(j, 3)
        assert a.batch_ids(j).tolist() == perms[e][s * B:s * B + B].tolist()
    plain = _loader(pkg, M, B, shuffle=False)
    assert plain.epoch_permutation(3).tolist() == list(range(M))
    assert plain.batch_ids(4).tolist() == [3, 4, 5]
    # the pool has the shape StaticBatch.pool returns: three slots of one allocation
    assert a._ws.numel() == pkg._lib.load().scgib_collate_ws_words(B)
    assert a.pool["n"] == 3 and len(a.pool["batches"]) == 3 and a.pool["table"].numel() == 3
    nbytes = a.static.blob.numel()
    assert a.ring.numel() == 3 * nbytes
    assert [s["blob"].data_ptr() - a.ring.data_ptr() for s in a.pool["batches"]] == \
        [0, nbytes, 2 * nbytes]


def test_refusals(pkg):
    G = pkg.graph
    rng = np.random.default_rng(0)
    good = [path(3, 4, rng) for _ in range(4)]
    with pytest.raises(G.GraphIngestError, match="512"):
        G.DeviceDataset.from_molecules(good + [path(513, 4, rng)], "cpu", 1)
    one_atom = (np.array([[0], [0]], np.int64), rng.random((1, 4), dtype=np.float32))
    with pytest.raises(G.GraphIngestError, match="fewer than two"):
        G.DeviceDataset.from_molecules(good + [one_atom], "cpu", 1)
    ds = G.DeviceDataset.from_molecules(good[:2] + [one_atom] + good[2:], "cpu", 1,
                                        labels=np.arange(5, dtype=np.float32),
                                        drop_single_atom=True)
    assert ds.dropped == 1 and len(ds) == 4 and ds.host["y"].reshape(-1).tolist() == [0, 1, 3, 4]
    # an edge leaving its molecule (flat arrays, as a damaged cache would hold them)
    gptr, deg = np.array([0, 2, 4]), np.array([1, 1, 1, 1], np.int32)
    x = rng.random((4, 4), dtype=np.float32)
    G.DeviceDataset(gptr, deg, np.array([1, 0, 1, 0], np.int32), x, None, "cpu", 1)
    with pytest.raises(G.GraphIngestError, match="leaves its molecule"):
        G.DeviceDataset(gptr, deg, np.array([1, 0, 2, 0], np.int32), x, None, "cpu", 1)
    # S = M // B < 3
    ds8 = G.DeviceDataset.from_molecules([path(3, 4, rng) for _ in range(8)], "cpu", 1)
    with pytest.raises(pkg._lib.ScgibError, match="at least 3"):
        G.DeviceLoader(ds8, static_for(pkg, ds8, 3, "cpu"))
    loader = G.DeviceLoader(ds8, static_for(pkg, ds8, 2, "cpu"))
    with pytest.raises(pkg._lib.ScgibError, match="HIP device"):
        loader.prime()
    # a dataset whose in-degree or molecule size passes what the static batch was built for
    small = static_for(pkg, ds8, 2, "cpu")
    star = (np.array([[0, 0, 0, 0], [1, 2, 3, 4]], np.int64), rng.random((5, 4), dtype=np.float32))
    ds_star = G.DeviceDataset.from_molecules([path(3, 4, rng) for _ in range(7)] + [star], "cpu", 1)
    with pytest.raises(pkg._lib.ScgibError):
        G.DeviceLoader(ds_star, small)


def test_collate_entry_points_exported(pkg):
    lib = pkg._lib.load()
    assert pkg._lib.ABI_VERSION == 24 and lib.scgib_abi_version() == 24
    for name in ("scgib_collate_plan", "scgib_collate_fill", "scgib_collate_max_batch",
                 "scgib_collate_ws_words"):
        assert name in pkg._lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.scgib_collate_max_batch() == pkg.graph.COLLATE_MAX_BATCH == 4096
    assert lib.scgib_collate_ws_words(512) == 8 + 2 * 513 + 4 * 512
    # the host mirror of scgib_collate_desc: 16 pointers, 12 int64, 4 int32
    assert ctypes.sizeof(pkg._lib.CollateDesc) == 16 * 8 + 12 * 8 + 4 * 4
    # a descriptor the entry points must refuse before any launch
    assert lib.scgib_collate_plan(ctypes.byref(pkg._lib.CollateDesc()), 0, 0, 0, None) == -1
    assert lib.scgib_collate_fill(None, 0, None) == -1
