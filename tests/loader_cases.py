"""Datasets and references shared by test_loader_cpu.py and test_gpu_loader.py
(graph.DeviceDataset / graph.DeviceLoader)."""
import numpy as np


def labels_with_nans(M, T, seed):
    """[M, T] fp32 labels with about a fifth of them NaN (kept by the loader)."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((M, T)).astype(np.float32)
    y[rng.random((M, T)) < 0.2] = np.nan
    return y


def qm9_set(pkg, M=60, seed=5, T=3):
    return pkg.synth.molecules(M, "qm9", seed=seed), labels_with_nans(M, T, seed + 1)


def path(n, F, rng):
    """A path of n atoms, one direction stored (the ingest adds the other)."""
    ei = np.stack([np.arange(n - 1), np.arange(1, n)]).astype(np.int64)
    return ei, rng.random((n, F), dtype=np.float32)


def handmade_set(F=8, seed=9):
    """Six molecules around the layout's corners: two atoms, an isolated atom
    (an empty CSR row), a 512-atom path (the ego builder's limit), a self
    loop, a triangle and a star.  F = 8: feature rows of whole 16-byte words."""
    rng = np.random.default_rng(seed)
    x = lambda n: rng.random((n, F), dtype=np.float32)  # noqa: E731
    mols = [
        (np.array([[0], [1]], np.int64), x(2)),
        (np.array([[0], [2]], np.int64), x(3)),  # atom 1 has no bond
        path(512, F, rng),
        (np.array([[0, 1], [1, 1]], np.int64), x(2)),  # a self loop on atom 1
        (np.array([[0, 1, 2], [1, 2, 0]], np.int64), x(3)),
        (np.array([[0, 0, 0, 0], [1, 2, 3, 4]], np.int64), x(5)),
    ]
    return mols, labels_with_nans(len(mols), 2, seed + 1)


def tiny_set(M, F=4, seed=13):
    """M molecules of 2 to 4 atoms (paths; every third 4-atom one a ring)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 5, size=M)
    mols = []
    for i, n in enumerate(sizes):
        ei, x = path(int(n), F, rng)
        if n == 4 and i % 3 == 0:
            ei = np.concatenate([ei, np.array([[3], [0]], np.int64)], axis=1)
        mols.append((ei, x))
    return mols, labels_with_nans(M, 1, seed + 1)


def sized_set(sizes, F=11, seed=21):
    """Paths of the given atom counts, in order."""
    rng = np.random.default_rng(seed)
    return [path(int(n), F, rng) for n in sizes], labels_with_nans(len(sizes), 2, seed + 1)


def pad_blob(pkg, static, mols, ids):
    """The yardstick: the host-collated, host-padded blob of molecules ``ids``."""
    g, kept = pkg.graph.collate_pyg([mols[int(i)] for i in ids])
    assert len(kept) == len(ids)
    return static.pad(g)["blob"]


def static_for(pkg, ds, B, device, mode="worst"):
    caps = ds.capacities(B, mode)
    return pkg.graph.StaticBatch(B, caps[0], caps[1], ds.num_features, caps[2], caps[3], device,
                                 ds.k)


def same_bits(a, b):
    """Equality of fp32 arrays bit for bit (NaNs in place)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
