"""References shared by test_eval_loader_cpu.py and test_gpu_eval_loader.py
(graph.DeviceEvalLoader and DeviceLoader(indices=...)), written
without the code under test: the sequential batches of a subset with their
fill molecule, and their capacities by brute force over collate_pyg."""
import numpy as np


def fill_of(mols, indices):
    """The subset's smallest molecule: fewest atoms, then fewest stored edges
    (collate_pyg's count, both directions), then lowest id."""
    def key(i):
        ei, x = mols[i]
        pairs = {(int(a), int(b)) for a, b in ei.T} | {(int(b), int(a)) for a, b in ei.T}
        return len(x), len(pairs), i
    return min((int(i) for i in indices), key=key)


def batches_of(mols, indices, B):
    """[(molecule ids with fill [B], reported ids with -1 at the fill rows [B])]
    for the ceil(M / B) sequential batches of ``indices``."""
    indices = [int(i) for i in indices]
    fill = fill_of(mols, indices)
    out = []
    for a in range(0, len(indices), B):
        real = indices[a:a + B]
        pad = B - len(real)
        out.append((np.array(real + [fill] * pad, np.int64), np.array(real + [-1] * pad, np.int64)))
    return out


def labels_of(y, marked):
    """y[ids] with a NaN row where the reported id is -1."""
    out = y[np.maximum(marked, 0)].copy()
    out[marked < 0] = np.nan
    return out


def brute_capacities(pkg, mols, subsets, B, k):
    """StaticBatch.capacities' maxima over every sequential batch of every
    subset, without its + 1 (slack 1.0 adds one to each)."""
    hosts = [pkg.graph.collate_pyg([mols[int(i)] for i in rows])[0]
             for sub in subsets for rows, _ in batches_of(mols, sub, B)]
    n, e, mgn, (ns, es, _) = pkg.graph.StaticBatch.capacities(hosts, k)
    return n - 1, e - 1, ns - 1, es - 1


def eval_static(pkg, ds, B, device, indices=None):
    caps = ds.capacities(B, "sequential", indices=indices)
    return pkg.graph.StaticBatch(B, caps[0], caps[1], ds.num_features, caps[2], caps[3], device,
                                 ds.k)
