"""Shared inputs of the ingest tests (test_ingest_cpu.py, test_gpu_ingest.py)."""
import numpy as np
import torch


def handmade():
    """Three PyG-style molecules covering: a duplicated edge, edges given in
    one direction only, a self-loop, an isolated interior atom."""
    rng = np.random.default_rng(7)
    m0 = np.array([[0, 0, 1, 3, 2, 3, 0], [1, 1, 2, 3, 3, 2, 1]], np.int64)  # 4 atoms
    m1 = np.array([[0, 1, 3, 1], [1, 0, 4, 3]], np.int64)                    # 5 atoms, atom 2 isolated
    m2 = np.array([[0], [1]], np.int64)                                       # 2 atoms
    return [(m0, rng.random((4, 5), dtype=np.float32)), (m1, rng.random((5, 5), dtype=np.float32)),
            (m2, rng.random((2, 5), dtype=np.float32))]


def flat(mols):
    """(src, dst, graph_ptr, x) numpy arrays of the batch: the raw edges with
    node offsets added, nothing deduplicated or mirrored."""
    counts = np.array([x.shape[0] for _, x in mols], np.int64)
    gptr = np.concatenate([[0], np.cumsum(counts)])
    src = np.concatenate([np.asarray(ei, np.int64).reshape(2, -1)[0] + o
                          for (ei, _), o in zip(mols, gptr)])
    dst = np.concatenate([np.asarray(ei, np.int64).reshape(2, -1)[1] + o
                          for (ei, _), o in zip(mols, gptr)])
    x = np.concatenate([np.asarray(x, np.float32) for _, x in mols])
    return src, dst, gptr.astype(np.int32), x


def tensors(mols, device="cpu", dtype=torch.int64):
    src, dst, gptr, x = flat(mols)
    t = lambda a, dt=None: torch.from_numpy(a).to(device, dt)  # noqa: E731
    return t(src, dtype), t(dst, dtype), t(gptr), t(x)


def path_molecule(n, feat, seed=0):
    """A path of n atoms, bonds stored once (low -> high)."""
    ei = np.stack([np.arange(n - 1), np.arange(1, n)]).astype(np.int64)
    return ei, np.random.default_rng(seed).random((n, feat), dtype=np.float32)


class Duck:
    """The least a DGL-like graph offers: edges(), batch_num_nodes(),
    num_nodes(), ndata."""

    def __init__(self, src, dst, counts, ndata=None):
        self._src, self._dst, self._counts = src, dst, counts
        self.ndata = dict(ndata or {})

    def edges(self):
        return self._src, self._dst

    def batch_num_nodes(self):
        return self._counts

    def num_nodes(self):
        return int(self._counts.sum())

    @classmethod
    def of(cls, g, keys=("x",)):
        """The duck of a GraphBatch: its (src, dst)-sorted edges and counts."""
        src, dst = g.edges()
        gp = g.graph_ptr.to(torch.int64)
        return cls(src, dst, gp[1:] - gp[:-1], {k: g.ndata[k] for k in keys if k in g.ndata})


def same_graph(a, b):
    """CSR, graph_ptr and x of two batches are identical."""
    e = b.num_edges()
    ok = (torch.equal(a.rowptr.cpu(), b.rowptr.cpu()) and a.num_edges() == e and
          torch.equal(a.col.cpu()[:e], b.col.cpu()[:e]) and
          torch.equal(a.graph_ptr.cpu(), b.graph_ptr.cpu()) and a.rowptr.dtype == torch.int32 and
          a.col.dtype == torch.int32 and a.graph_ptr.dtype == torch.int32)
    if "x" in b.ndata and "x" in a.ndata:
        ok = ok and torch.equal(a.ndata["x"].cpu(), b.ndata["x"].cpu())
    return bool(ok)
