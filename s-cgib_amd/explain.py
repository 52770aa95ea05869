"""Dataset-level reading of graph cores and significant subgraphs
(csrc/explain.hip).

``model.explain(...)`` (models.py) explains one batch.  ``explain_dataset``
walks a subset of a ``graph.DeviceDataset`` with a ``graph.DeviceEvalLoader``:
one captured step — load_next, collate_ahead, the eval forward up to the
interaction, ops.explain_rank, ops.explain_store — replayed once per batch,
with no host read during the pass.  The per-batch cores are not stored: the
dataset-wide ``lam`` / ``lam_rank`` give every core rule (``core_mask``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import graph as G
from . import models
from . import ops

RANK_UNSET = -1  # rank of an atom no pass has written (a molecule outside the subset)


class DatasetExplanation:
    """Per-atom arrays over a whole DeviceDataset, addressed by its node
    offsets: atom a of molecule i is row ``node_off[i] + a``.  ``lam`` /
    ``alpha`` [total_nodes] fp32 (NaN where no pass wrote), ``lam_rank`` /
    ``alpha_rank`` int32 (-1 where no pass wrote); ``alpha`` / ``alpha_rank``
    None for a model without attention."""

    def __init__(self, dataset, use_att=True):
        dev = dataset.device
        self.dataset = dataset
        self.node_off = dataset.arrays["node_off"]
        self.total_nodes = int(dataset.host["node_off"][-1])
        n = self.total_nodes

        def f32():
            return torch.full((n,), float("nan"), dtype=torch.float32, device=dev)

        def i32():
            return torch.full((n,), RANK_UNSET, dtype=torch.int32, device=dev)

        self.lam, self.lam_rank = f32(), i32()
        self.alpha, self.alpha_rank = (f32(), i32()) if use_att else (None, None)

    def arrays(self):
        return self.lam, self.alpha, self.lam_rank, self.alpha_rank

    def molecule(self, i):
        """Host convenience (synchronises): (lam, alpha, lam_rank, alpha_rank)
        of molecule ``i`` as numpy arrays (None where there is no attention)."""
        off = self.dataset.host["node_off"]
        a, b = int(off[i]), int(off[i + 1])
        return tuple(None if t is None else t[a:b].cpu().numpy() for t in self.arrays())

    def core_mask(self, ratio=None, threshold=None):
        """The graph-core rule of ops.core_subgraph over the stored arrays
        (torch on the device, no kernel of its own): [total_nodes] bool."""
        if (ratio is None) == (threshold is None):
            raise ValueError("core_mask: exactly one of ratio and threshold")
        if threshold is not None:
            return self.lam >= float(np.float32(threshold))
        counts = np.diff(self.dataset.host["node_off"]).astype(np.float64)
        m = np.maximum(1.0, np.ceil(counts * float(ratio)))
        m = torch.from_numpy(np.repeat(m, counts.astype(np.int64)).astype(np.int32))
        return (self.lam_rank >= 0) & (self.lam_rank < m.to(self.lam_rank.device))


def explain_dataset(model, dataset, static, indices=None, *, u_gate=None, passes=1, out=None,
                    loader=None):
    """Fill a DatasetExplanation for the molecules ``indices`` of ``dataset``
    (default: all) with ``model`` in eval mode.

    ``static``: a graph.StaticBatch sized for the subset
    (``dataset.capacities(B, "sequential", indices=...)``).  One step —
    ``static.load_next``, ``collate_ahead``, the forward up to the
    interaction, explain_rank, explain_store — runs once eagerly (warm-up),
    is captured into a HIP graph and replayed ``steps`` times per pass;
    nothing is read back during the pass.  ``u_gate`` [n_cap] (or None: 0.5,
    the median gate) is the gate draw of every batch.  Fill molecules of the
    last batch write nothing.  Returns ``out`` (a new DatasetExplanation
    unless one is given)."""
    if model.training:
        raise RuntimeError("explain_dataset needs model.eval()")
    dev = static.blob.device
    if dev.type != "cuda":
        raise _lib.ScgibError("explain_dataset needs a HIP device (no CPU fallback)")
    owner, transfer, k = models._explain_route(model)
    use_att = bool(owner.useAtt)
    if out is None:
        out = DatasetExplanation(dataset, use_att)
    evl = loader if loader is not None else G.DeviceEvalLoader(dataset, static, indices=indices)

    def body():
        static.load_next(evl.pool)
        evl.collate_ahead()
        ex = models._explain(model, owner, transfer, k, static.graph, static.x, None, None, None,
                             None, 0, u_gate, with_core=False)
        ops.explain_store(ex.lam, ex.alpha, ex.lam_rank, ex.alpha_rank, static.graph, evl.ids,
                          out.node_off, out.arrays())

    evl.prime()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # warm-up (allocator, lazy workspaces): batch 0, stored once
        body()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    evl.prime()
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for _ in range(int(passes) * evl.steps):
        graph.replay()
    torch.cuda.synchronize(dev)
    if evl.error():
        raise _lib.ScgibError("explain_dataset: a batch did not fit the static batch's capacities")
    return out
