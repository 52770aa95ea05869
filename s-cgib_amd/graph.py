"""Batched molecular graphs for the S-CGIB hot path (DGL-duck-typed).

Reference surface reproduced: the model consumes a DGL
graph — ``batch_num_nodes()`` (models.py:665), ``ndata`` reads/writes
(exp_pretraining.py:304, models.py:683), ``edges()``, ``.to(device)``,
``adj().to_dense()`` (models.py:764), ``nodes()`` / ``num_nodes()``.

Storage, MI355X-first:
  * ``rowptr`` [N+1] / ``col`` [E] int32: dst-major CSR (row v lists the
    sources of v's in-edges, columns ascending) — the layout the GIN gather
    kernel reads; 4-byte indices halve index traffic vs int64;
  * ``rowptr_t`` / ``col_t``: the src-major CSR (the same tensors when the
    graph is symmetric, i.e. every to_bidirected molecule);
  * ``graph_ptr`` [B+1] int32: node range of every molecule;
  * host copies of the per-graph node/edge counts, so shape decisions never
    synchronise with the device.

Ingest restates ``util.load_dgl_fromPyG`` (util.py:277-325): ``dgl.graph``
infers ``num_nodes = max id + 1``, ``to_bidirected`` adds reverse edges and
rebuilds a simple graph with edges sorted by (src, dst); a molecule whose
``x`` row count differs from that node count (trailing isolated atoms, no
bonds) raises, which the reference's bare ``except`` turns into "skip"
(exp_pretraining.py:276-278).
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import torch

from . import _lib


class GraphIngestError(ValueError):
    """Raised where DGL raises on ``g.ndata['x'] = x`` (row-count mismatch)."""


class _NData(dict):
    def __init__(self, graph):
        super().__init__()
        self._g = graph

    def __setitem__(self, key, value):
        if value.shape[0] != self._g.num_nodes():
            raise GraphIngestError(
                f"Expect number of features to match number of nodes. Got {value.shape[0]} "
                f"and {self._g.num_nodes()} instead.")
        super().__setitem__(key, value)


class _Adj:
    def __init__(self, g):
        self._g = g

    def to_dense(self):
        src, dst = self._g.edges()
        n = self._g.num_nodes()
        a = torch.zeros(n, n, dtype=torch.float32, device=src.device)
        a[src, dst] = 1.0
        return a


def _csr_from_sorted(keys_major, minor, n):
    """CSR from edges already sorted by (major, minor)."""
    counts = np.bincount(keys_major, minlength=n) if n else np.zeros(0, np.int64)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=rowptr[1:])
    return rowptr.astype(np.int32), minor.astype(np.int32)


class GraphBatch:
    """A batch of B graphs with N nodes and E directed edges."""

    def __init__(self, rowptr, col, graph_ptr, batch_num_nodes, batch_num_edges=None,
                 rowptr_t=None, col_t=None, max_graph_nodes=None, n_edges=None,
                 host_info=None):
        self.rowptr = rowptr
        self.col = col
        self.rowptr_t = rowptr if rowptr_t is None else rowptr_t
        self.col_t = col if col_t is None else col_t
        self.symmetric = rowptr_t is None
        self.graph_ptr = graph_ptr
        self._bnn = None if batch_num_nodes is None else np.asarray(batch_num_nodes, np.int64)
        self._bne = None if batch_num_edges is None else np.asarray(batch_num_edges, np.int64)
        self._n = int(rowptr.shape[0] - 1)
        self._e = int(col.shape[0]) if n_edges is None else (None if n_edges < 0 else int(n_edges))
        self._B = int(graph_ptr.shape[0] - 1)
        if max_graph_nodes is None:
            max_graph_nodes = int(self._bnn.max()) if self._bnn is not None and len(self._bnn) else 0
        self.max_graph_nodes = int(max_graph_nodes)
        # host-side facts known at construction (no device sync to get them):
        # {"deg": in-degree per node (np.int64), "selfloops": per-node 0/1,
        #  "validated": edges never leave their graph}
        self.host_info = host_info
        # no edge leaves its graph_ptr segment (host-validated, or built so:
        # ego batches, StaticBatch) -- the chunked fused GIN backward needs it
        self.components_closed = bool(host_info is not None and host_info.get("validated"))
        # capacity mode: device int32 [actual nodes, actual edges]; the host
        # sizes above are then capacities (see StaticBatch)
        self.dims = None
        self.ego_caps = None  # (ego nodes cap, ego edges cap) for capacity mode
        self.seg_dims = None  # ego batches: device count of segments (= parent nodes)
        # device ingest (from_coo): (max in-degree, k = 1 ego nodes, k = 1 ego edge
        # bound) from its status record, what host_info gives a host batch
        self.ego_k1 = None
        self.ndata = _NData(self)
        self.edata = {}

    # ----- construction ---------------------------------------------------
    @classmethod
    def from_edges(cls, src, dst, num_nodes, symmetric_hint=False, batch_num_nodes=None,
                   batch_num_edges=None):
        """Graph from a COO edge list (kept as a multigraph-free CSR)."""
        src = np.asarray(src, np.int64)
        dst = np.asarray(dst, np.int64)
        n = int(num_nodes)
        order_out = np.lexsort((dst, src))
        rp_t, col_t = _csr_from_sorted(src[order_out], dst[order_out], n)
        if symmetric_hint:
            rp, col, rp_t2, col_t2 = rp_t, col_t, None, None
        else:
            order_in = np.lexsort((src, dst))
            rp, col = _csr_from_sorted(dst[order_in], src[order_in], n)
            rp_t2, col_t2 = torch.from_numpy(rp_t), torch.from_numpy(col_t)
        if batch_num_nodes is None:
            batch_num_nodes = np.array([n], np.int64)
            batch_num_edges = np.array([len(src)], np.int64)
        gptr = np.zeros(len(batch_num_nodes) + 1, np.int64)
        np.cumsum(batch_num_nodes, out=gptr[1:])
        # edges must stay inside their graph (the ego-net builder relies on it)
        owner = np.searchsorted(gptr, np.arange(n), side="right") - 1 if n else np.zeros(0, np.int64)
        validated = bool(len(src) == 0 or (owner[src] == owner[dst]).all())
        sl = np.zeros(n, np.int64)
        np.add.at(sl, src[src == dst], 1)
        info = {"deg": np.diff(rp.astype(np.int64)), "selfloops": sl, "validated": validated}
        return cls(torch.from_numpy(rp), torch.from_numpy(col),
                   torch.from_numpy(gptr.astype(np.int32)), batch_num_nodes, batch_num_edges,
                   rp_t2, col_t2, host_info=info)

    # ----- DGL surface ------------------------------------------------------
    def num_nodes(self, ntype=None):
        return self._n

    number_of_nodes = num_nodes

    def edge_capacity(self):
        """Host edge count to size launches: exact, or the capacity in capacity mode."""
        return int(self.col.shape[0]) if self.dims is not None else self.num_edges()

    def num_edges(self, etype=None):
        if self._e is None:  # ego batches sized by capacity: read the exact count once
            self._e = int(self.rowptr[-1].item())
        return self._e

    number_of_edges = num_edges

    @property
    def batch_size(self):
        return self._B

    @property
    def device(self):
        return self.rowptr.device

    def batch_num_nodes(self, ntype=None):
        if self._bnn is None:
            gp = self.graph_ptr.to("cpu", torch.int64)
            self._bnn = (gp[1:] - gp[:-1]).numpy()
        return torch.from_numpy(self._bnn)

    def batch_num_nodes_host(self):
        """Per-graph node counts as a host numpy array (no device sync)."""
        self.batch_num_nodes()
        return self._bnn

    def batch_num_edges(self, etype=None):
        if self._bne is None:
            rp_t = self.rowptr_t.to("cpu", torch.int64)
            gp = self.graph_ptr.to("cpu", torch.int64)
            self._bne = (rp_t[gp[1:]] - rp_t[gp[:-1]]).numpy()
        return torch.from_numpy(self._bne)

    def nodes(self, ntype=None):
        return torch.arange(self._n, dtype=torch.int64, device=self.device)

    def edges(self, form="uv", order="eid", etype=None):
        """(src, dst) int64 in DGL's order for to_bidirected graphs: (src, dst) sorted."""
        deg = (self.rowptr_t[1:] - self.rowptr_t[:-1]).to(torch.int64)
        src = torch.repeat_interleave(torch.arange(self._n, device=self.device), deg)
        return src, self.col_t[: self.num_edges()].to(torch.int64)

    def in_degrees(self):
        return (self.rowptr[1:] - self.rowptr[:-1]).to(torch.int64)

    def adj(self, etype=None, eweight_name=None):
        return _Adj(self)

    def to(self, device, non_blocking=False):
        def mv(t):
            return None if t is None else t.to(device, non_blocking=non_blocking)

        g = GraphBatch(mv(self.rowptr), mv(self.col), mv(self.graph_ptr), self._bnn, self._bne,
                       None if self.symmetric else mv(self.rowptr_t),
                       None if self.symmetric else mv(self.col_t), self.max_graph_nodes,
                       -1 if self._e is None else self._e, self.host_info)
        g.dims = mv(self.dims)
        g.components_closed = self.components_closed
        g.ego_caps = self.ego_caps
        g.seg_dims = mv(self.seg_dims)
        g.ego_k1 = self.ego_k1
        for k, v in self.ndata.items():
            dict.__setitem__(g.ndata, k, v.to(device, non_blocking=non_blocking))
        return g

    @contextlib.contextmanager
    def local_scope(self):
        saved = dict(self.ndata)
        try:
            yield
        finally:
            dict.clear(self.ndata)
            dict.update(self.ndata, saved)

    def __repr__(self):
        return (f"GraphBatch(num_graphs={self._B}, num_nodes={self._n}, num_edges={self._e}, "
                f"device={self.device})")


# ---------------------------------------------------------------------------
# ingest (A1) and collate (A3)
# ---------------------------------------------------------------------------
def bidirected_simple(src, dst, n):
    """dgl.to_bidirected(dgl.graph((src, dst))) edges: unique, (src, dst)-sorted."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    if len(src) == 0:
        return src, dst
    key = np.unique(np.concatenate([src * n + dst, dst * n + src]))
    return key // n, key % n


def pyg_num_nodes(edge_index):
    ei = np.asarray(edge_index)
    return int(ei.max()) + 1 if ei.size else 0


def from_pyg(edge_index, x=None):
    """util.load_dgl_fromPyG (util.py:277-325) for one molecule."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    n = pyg_num_nodes(ei)
    if x is not None and np.asarray(x).shape[0] != n:
        raise GraphIngestError(f"x has {np.asarray(x).shape[0]} rows, graph has {n} nodes")
    s, d = bidirected_simple(ei[0], ei[1], n)
    g = GraphBatch.from_edges(s, d, n, symmetric_hint=True)
    if x is not None:
        g.ndata["x"] = torch.as_tensor(np.asarray(x))
    return g


def collate_pyg(molecules, device=None, skip_invalid=True):
    """Batch a list of PyG-style ``(edge_index, x)`` molecules in one pass.

    Equivalent to ``dgl.batch([load_dgl_fromPyG(m) for m in molecules])`` with
    the reference's skip rule; vectorised over the batch (edges never cross
    molecules, so one global unique == per-molecule to_bidirected).
    Returns (GraphBatch, kept_indices).
    """
    srcs, dsts, xs, counts, kept = [], [], [], [], []
    off = 0
    for i, (ei, x) in enumerate(molecules):
        ei = np.asarray(ei, np.int64).reshape(2, -1)
        n = pyg_num_nodes(ei)
        if np.asarray(x).shape[0] != n:
            if skip_invalid:
                continue
            raise GraphIngestError(f"molecule {i}: x rows != inferred node count")
        srcs.append(ei[0] + off)
        dsts.append(ei[1] + off)
        xs.append(np.asarray(x, np.float32))
        counts.append(n)
        kept.append(i)
        off += n
    counts = np.asarray(counts, np.int64)
    src = np.concatenate(srcs) if srcs else np.zeros(0, np.int64)
    dst = np.concatenate(dsts) if dsts else np.zeros(0, np.int64)
    s, d = bidirected_simple(src, dst, max(off, 1))
    gptr = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=gptr[1:])
    e_counts = np.diff(np.searchsorted(s, gptr)) if len(counts) else np.zeros(0, np.int64)
    g = GraphBatch.from_edges(s, d, off, symmetric_hint=True, batch_num_nodes=counts,
                              batch_num_edges=e_counts)
    g.ndata["x"] = torch.from_numpy(np.concatenate(xs) if xs else np.zeros((0, 1), np.float32))
    if device is not None:
        g = g.to(device)
    return g, kept


def batch(graphs):
    """dgl.batch: concatenate GraphBatches with node-id offsets (host side)."""
    graphs = list(graphs)
    rps, cols, rpts, colts, bnn, bne = [], [], [], [], [], []
    noff = eoff = 0
    sym = all(g.symmetric for g in graphs)
    for g in graphs:
        rp = g.rowptr.cpu().numpy().astype(np.int64)
        rps.append(rp[:-1] + eoff)
        cols.append(g.col.cpu().numpy().astype(np.int64)[: g.num_edges()] + noff)
        if not sym:
            rpt = g.rowptr_t.cpu().numpy().astype(np.int64)
            rpts.append(rpt[:-1] + eoff)
            colts.append(g.col_t.cpu().numpy().astype(np.int64)[: g.num_edges()] + noff)
        bnn.append(g.batch_num_nodes_host())
        bne.append(g.batch_num_edges().numpy())
        noff += g.num_nodes()
        eoff += g.num_edges()
    rowptr = np.concatenate(rps + [np.array([eoff])]).astype(np.int32)
    col = (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int32)
    bnn = np.concatenate(bnn) if bnn else np.zeros(0, np.int64)
    bne = np.concatenate(bne) if bne else np.zeros(0, np.int64)
    gptr = np.zeros(len(bnn) + 1, np.int64)
    np.cumsum(bnn, out=gptr[1:])
    rp_t = col_t = None
    if not sym:
        rp_t = torch.from_numpy(np.concatenate(rpts + [np.array([eoff])]).astype(np.int32))
        col_t = torch.from_numpy(np.concatenate(colts).astype(np.int32))
    out = GraphBatch(torch.from_numpy(rowptr), torch.from_numpy(col),
                     torch.from_numpy(gptr.astype(np.int32)), bnn, bne, rp_t, col_t)
    out.components_closed = bool(graphs) and all(g.components_closed for g in graphs)
    if graphs:
        for k in graphs[0].ndata.keys():
            dict.__setitem__(out.ndata, k, torch.cat([g.ndata[k].cpu() for g in graphs], 0))
    dev = graphs[0].device if graphs else None
    return out.to(dev) if dev is not None and dev.type != "cpu" else out


# ---------------------------------------------------------------------------
# on-device ego-net builder (A2 + the per-step dgl.batch of A3)
# ---------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def egonet_batch(g: GraphBatch, k: int, x=None):
    """All k-hop in-subgraphs of ``g``, batched: ego j <-> node j of ``g``.

    Equivalent to ``dgl.batch(chain(*[[dgl.khop_in_subgraph(m, v, k)[0] for v
    in m.nodes()] for m in molecules]))`` (exp_pretraining.py:269-272,
    308-309).  Runs on ``g``'s HIP device through scgib_egonet_count/fill.  For
    k = 1 on a host-validated graph the output sizes are known on the host
    (no device sync); otherwise one 3-integer device->host read sizes them.
    The result carries ``ndata['_ID']`` (parent node id of every ego node)
    and, if ``x`` is given, ``ndata['x'] = x[_ID]``.
    """
    if g.device.type != "cuda":
        raise _lib.ScgibError("egonet_batch needs the graph on a HIP device (no CPU fallback)")
    if not g.symmetric:
        raise _lib.ScgibError("egonet_batch expects a symmetric (to_bidirected) graph")
    dev = g.device
    n = g.num_nodes()
    i32 = torch.int32
    ego_ptr = torch.empty(n + 1, dtype=i32, device=dev)
    ego_eptr = torch.empty(n + 1, dtype=i32, device=dev)
    ws = torch.empty(int(_lib.query("scgib_egonet_workspace_bytes", n)), dtype=torch.uint8,
                     device=dev)
    kb = _k1_bounds(g) if k == 1 else None
    if k == 1 and EGO_K1_FAST and n > 0:
        # two-launch k = 1 builder (sorted-list balls, batched loads): needs
        # the max in-degree bound and in-molecule edges, checked on the host
        kmax = int(_lib.query("scgib_egonet_k1_max_degree"))
        fits = g.max_graph_nodes <= int(_lib.query("scgib_egonet_k1_max_graph_nodes"))
        if g.dims is not None:
            caps = g.ego_caps or ()
            fast = fits and len(caps) > 2 and caps[2] <= kmax
        else:
            fast = fits and kb is not None and kb[0] <= kmax
        if fast:
            dmax = int(caps[2]) if g.dims is not None else kb[0]
            return _egonet_k1(g, ego_ptr, ego_eptr, ws, x, dmax, kb)
    err = getattr(g, "err_buf", None)
    if err is None:
        err = torch.zeros(1, dtype=i32, device=dev)
    st = _stream()
    mgn = max(g.max_graph_nodes, 1)
    _lib.call("scgib_egonet_count", _ptr(g.rowptr), _ptr(g.col), _ptr(g.graph_ptr), g.batch_size,
              n, k, mgn, _ptr(ego_ptr), _ptr(ego_eptr), _ptr(ws), _ptr(err), _ptr(g.dims), st)
    ego_dims = None
    if g.dims is not None:
        # capacity mode: outputs sized by the graph's capacities, actual sizes
        # stay on the device (ego_dims) — nothing is read back
        if g.ego_caps is None:
            raise _lib.ScgibError("capacity-mode graph without ego capacities (StaticBatch)")
        n_s, e_cap = g.ego_caps[:2]
        e_s = -1
        ego_dims = torch.empty(2, dtype=i32, device=dev)
    elif k == 1 and kb is not None and mgn <= 512:
        # sizes known on the host, no device sync: |ball(v)| = 1 + deg(v) - selfloop(v);
        # the induced-edge count is bounded by sum_{u in ball(v)} deg(u)
        _, n_s, e_cap = kb
        e_s = -1  # exact count read lazily (GraphBatch.num_edges)
    else:
        tot = torch.stack([ego_ptr[n], ego_eptr[n], err[0]]).cpu().tolist()
        n_s, e_s, e_code = int(tot[0]), int(tot[1]), int(tot[2])
        if e_code:
            raise _lib.ScgibError(f"scgib_egonet_count flagged error bits {e_code} "
                                  "(1: edge leaves its graph, 2: graph larger than max_graph_nodes)")
        e_cap = e_s
    ego_nodes = torch.empty(n_s, dtype=i32, device=dev)
    sub_rowptr = torch.empty(n_s + 1, dtype=i32, device=dev)
    sub_col = torch.empty(max(e_cap, 1), dtype=i32, device=dev)
    _lib.call("scgib_egonet_fill", _ptr(g.rowptr), _ptr(g.col), _ptr(g.graph_ptr), g.batch_size, n,
              k, mgn, _ptr(ego_ptr), _ptr(ego_eptr), _ptr(ego_nodes), _ptr(sub_rowptr),
              _ptr(sub_col), _ptr(err), n_s, _ptr(g.dims), _ptr(ego_dims), st)
    ego = GraphBatch(sub_rowptr, sub_col, ego_ptr, None, None, n_edges=e_s,
                     max_graph_nodes=mgn)
    ego.dims = ego_dims
    ego.components_closed = True  # induced subgraphs: edges stay in their ego-net
    ego.seg_dims = g.dims  # the ego batch's segments are g's nodes
    dict.__setitem__(ego.ndata, "_ID", ego_nodes)
    if x is not None:
        dict.__setitem__(ego.ndata, "x", x.index_select(0, ego_nodes))
    return ego


def _k1_bounds(g):
    """(max in-degree, ego nodes, ego edge bound) of ``g``'s k = 1 ego-nets
    where the host knows them without a device read -- from ``host_info`` of a
    validated host batch, or from the status record of the device ingest
    (``from_coo``) -- else None."""
    info = g.host_info
    if info is not None:
        if not info["validated"]:
            return None
        deg = info["deg"]
        ball = 1 + deg - info["selfloops"]
        return (int(deg.max()) if len(deg) else 0, int(ball.sum()), int((deg * ball).sum()))
    return g.ego_k1


def ego_bounds(g, k):
    """(ego-batch nodes, bound on ego-batch edges, max in-degree) of host
    batch ``g``'s k-hop ego-nets: nodes = sum_v |ball_k(v)|, edges <= sum_v
    sum_{u in ball_k(v)} deg(u).  k = 1: |ball(v)| = 1 + deg(v) - selfloop(v);
    k > 1: boolean reachability (I + A)^k on the host."""
    info = g.host_info
    deg = info["deg"].astype(np.int64)
    dmax = int(deg.max()) if len(deg) else 0
    if k == 1:
        ball = 1 + deg - info["selfloops"]
        return int(ball.sum()), int((deg * ball).sum()), dmax
    import scipy.sparse as sp
    n = g.num_nodes()
    rp = g.rowptr.cpu().numpy().astype(np.int64)
    col = g.col.cpu().numpy()[: rp[-1]].astype(np.int64)
    a = sp.csr_matrix((np.ones(len(col), np.int8), col, rp), shape=(n, n))
    step = (a + sp.identity(n, dtype=np.int8, format="csr")).astype(bool).astype(np.int32)
    r = step
    for _ in range(k - 1):
        r = (r @ step).astype(bool).astype(np.int32)
    return int(r.nnz), int((r @ deg).sum()), dmax


# k = 1 ego-nets through the sorted-list window builders when their bounds
# hold (in-degree <= 12, molecules <= the window), else the bitmap builder.
# On since round 1, session 4 (39 vs 46 us per QM9 B512 build alone; in the
# replayed step it first measured 0.5 % slower, which the later LDS-window
# one-pass form turned into 2.7 % faster).  Module attributes,
# not environment knobs: the tests compare every builder bit for bit.
EGO_K1_FAST = True
# ... in one launch (count + look-back scan + fill, egonet_k1_onepass_k)
# instead of two (count + block scan, fill)
EGO_K1_ONEPASS = True


def _egonet_k1(g, ego_ptr, ego_eptr, ws, x, max_in_degree=12, bounds=None):
    """egonet_batch for k = 1 via scgib_egonet_k1_build (sizes known on the
    host: |ball(v)| = 1 + deg(v) - selfloop(v); capacity mode: g.ego_caps)."""
    dev = g.device
    n = g.num_nodes()
    i32 = torch.int32
    ego_dims = None
    if g.dims is not None:
        n_s, e_cap = g.ego_caps[:2]
        ego_dims = torch.empty(2, dtype=i32, device=dev)
    else:
        _, n_s, e_cap = bounds if bounds is not None else _k1_bounds(g)
    ego_nodes = torch.empty(max(n_s, 1), dtype=i32, device=dev)
    sub_rowptr = torch.empty(n_s + 1, dtype=i32, device=dev)
    sub_col = torch.empty(max(e_cap, 1), dtype=i32, device=dev)
    if EGO_K1_ONEPASS:
        from . import ops  # (ops imports this module)
        state = ops.scan_state(dev, "egonet_k1_scan", int(_lib.query("scgib_egonet_k1_scan_words", n)))
        ops._launch("scgib_egonet_k1_build_onepass", {"n": n}, _ptr(g.rowptr), _ptr(g.col), n,
                  int(max_in_degree), _ptr(ego_ptr), _ptr(ego_eptr), _ptr(state), _ptr(ego_nodes),
                  _ptr(sub_rowptr), _ptr(sub_col), n_s, max(e_cap, 1),
                  _ptr(getattr(g, "err_buf", None)), _ptr(g.dims), _ptr(ego_dims), _stream())
    else:
        _lib.call("scgib_egonet_k1_build_deg", _ptr(g.rowptr), _ptr(g.col), n,
                  int(max_in_degree), _ptr(ego_ptr), _ptr(ego_eptr), _ptr(ws), _ptr(ego_nodes),
                  _ptr(sub_rowptr), _ptr(sub_col), n_s, _ptr(g.dims), _ptr(ego_dims), _stream())
    ego = _ego_graph(g, sub_rowptr, sub_col, ego_ptr, ego_nodes, n_s, ego_dims)
    if x is not None:
        dict.__setitem__(ego.ndata, "x", x.index_select(0, ego_nodes[:n_s]))
    return ego


def _ego_graph(g, sub_rowptr, sub_col, ego_ptr, ego_nodes, n_s, ego_dims):
    ego = GraphBatch(sub_rowptr, sub_col, ego_ptr, None, None, n_edges=-1,
                     max_graph_nodes=max(g.max_graph_nodes, 1))
    ego.dims = ego_dims
    ego.components_closed = True
    ego.seg_dims = g.dims
    dict.__setitem__(ego.ndata, "_ID", ego_nodes[:n_s])
    return ego


# ---------------------------------------------------------------------------
# device-side COO -> CSR ingest (csrc/ingest.hip)
# ---------------------------------------------------------------------------
INGEST_MAX_GRAPH_NODES = 512  # the ingest bitmap's widest molecule (= EGO_MAX_GRAPH_NODES)
_INGEST_WS = {}  # device -> (rows, workspace): zeroed once, the kernels reset it


def _ingest_raise(bits, where):
    names = "; ".join(f"{b}: {t}" for b, t in _lib.INGEST_ERRORS.items() if bits & b)
    raise _lib.ScgibError(f"{where} flagged error bits {bits} ({names})")


def _ingest_workspace(dev, n):
    """(rows, workspace) of the eager ingest on ``dev`` for at least ``n``
    rows: zero-filled when it is made or has to grow; between calls the
    kernels leave it zero.  Its layout follows the rows it was sized for."""
    have = _INGEST_WS.get(dev)
    if have is None or have[0] < n:
        nbytes = int(_lib.query("scgib_ingest_workspace_bytes", n, INGEST_MAX_GRAPH_NODES))
        have = (n, torch.zeros(nbytes, dtype=torch.uint8, device=dev))
        _INGEST_WS[dev] = have
    return have


def _index_pair(src, dst):
    src, dst = torch.as_tensor(src), torch.as_tensor(dst)
    if src.dtype not in (torch.int32, torch.int64):
        src = src.to(torch.int64)
    return src.reshape(-1).contiguous(), dst.to(src.device, src.dtype).reshape(-1).contiguous()


def _graph_ptr_of(graph_ptr, batch_num_nodes, dev):
    """graph_ptr as int32 [B+1] on ``dev`` (a cumsum where the per-graph counts
    are given; no device read)."""
    if graph_ptr is not None:
        return torch.as_tensor(graph_ptr).reshape(-1).to(dev, torch.int32).contiguous()
    if batch_num_nodes is None:
        raise ValueError("from_coo: graph_ptr or batch_num_nodes is needed")
    bnn = torch.as_tensor(batch_num_nodes).reshape(-1).to(torch.int64)
    gp = torch.zeros(bnn.numel() + 1, dtype=torch.int64, device=bnn.device)
    torch.cumsum(bnn, 0, out=gp[1:])
    return gp.to(dev, torch.int32)


def _from_coo_host(src, dst, gptr, n, bidirect, skip_rule):
    """from_coo on the host: the device route's checks in numpy, then
    bidirected_simple + from_edges (what collate_pyg runs)."""
    src, dst, gptr = src.numpy().astype(np.int64), dst.numpy().astype(np.int64), \
        gptr.numpy().astype(np.int64)
    counts = np.diff(gptr)
    bits = 0
    if len(gptr) < 1 or gptr[0] != 0 or gptr[-1] != n or (counts < 0).any():
        bits |= 64
    if (counts > INGEST_MAX_GRAPH_NODES).any():
        bits |= 2
    inside = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    if not bits and len(counts):
        owner = np.searchsorted(gptr, np.arange(n), side="right") - 1
        inside[inside] &= owner[src[inside]] == owner[dst[inside]]
    if not inside.all():
        bits |= 1
    if bits:
        _ingest_raise(bits, "from_coo")
    s, d = bidirected_simple(src, dst, max(n, 1))
    if not bidirect:
        key = src * max(n, 1) + dst
        if len(s) != len(src) or not np.array_equal(np.sort(key), s * max(n, 1) + d):
            bits |= 16  # duplicates, or an edge without its reverse
        s, d = np.unique(key) // max(n, 1), np.unique(key) % max(n, 1)
    deg = np.bincount(d, minlength=n)
    if skip_rule and len(counts) and (deg[gptr[1:][counts > 0] - 1] == 0).any():
        bits |= 8
    if bits:
        _ingest_raise(bits, "from_coo")
    e_counts = np.diff(np.searchsorted(s, gptr)) if len(counts) else np.zeros(0, np.int64)
    return GraphBatch.from_edges(s, d, n, symmetric_hint=True, batch_num_nodes=counts,
                                 batch_num_edges=e_counts)


def from_coo(src, dst, graph_ptr=None, num_nodes=None, x=None, bidirect=True, skip_rule=False,
             batch_num_nodes=None):
    """A GraphBatch from a batched COO edge list, on the tensors' device.

    ``src`` / ``dst`` [E] int32 or int64 (batch-global node ids),
    ``graph_ptr`` [B+1] node offsets or ``batch_num_nodes`` [B], ``num_nodes``
    rows (default: ``x``'s).  ``bidirect=True``: the union of the edges and
    their reverses, deduplicated -- ``dgl.to_bidirected`` per molecule, the CSR
    ``collate_pyg`` gives for the same molecules, bit for bit.
    ``bidirect=False``: the edges must already be simple and symmetric (a DGL
    batch built by the reference's ingest, an ego batch); that is verified,
    not repaired.  ``skip_rule``: refuse a molecule whose last atom has no
    edge, which the reference's ingest skips (util.py:317-321).

    HIP tensors go through scgib_ingest_csr (three launches) and one device ->
    host read per batch: the status record and graph_ptr together.  The result
    then carries the per-graph counts, the exact edge count, the largest
    molecule and the k = 1 ego bounds, so ``egonet_batch(g, 1)`` sizes its
    outputs without a second read.  CPU tensors take the host route with the
    same result.  Any error bit raises ScgibError naming it
    (``_lib.INGEST_ERRORS``)."""
    src, dst = _index_pair(src, dst)
    dev = src.device
    if num_nodes is None:
        if x is None:
            raise ValueError("from_coo: num_nodes or x is needed")
        num_nodes = x.shape[0]
    n = int(num_nodes)
    gptr = _graph_ptr_of(graph_ptr, batch_num_nodes, dev)
    B = int(gptr.numel()) - 1
    if src.numel() != dst.numel():
        raise ValueError("from_coo: src and dst differ in length")
    if dev.type != "cuda" or n == 0 or B < 1:
        g = _from_coo_host(src.cpu(), dst.cpu(), gptr.cpu(), n, bidirect, skip_rule)
        g = g if dev.type == "cpu" else g.to(dev)
    else:
        e_raw = int(src.numel())
        col_cap = max((2 if bidirect else 1) * e_raw, 1)
        i32 = torch.int32
        rowptr = torch.empty(n + 1, dtype=i32, device=dev)
        col = torch.empty(col_cap, dtype=i32, device=dev)
        status = torch.empty(int(_lib.query("scgib_ingest_status_words", B)), dtype=i32, device=dev)
        ws_rows, ws = _ingest_workspace(dev, n)
        _lib.call("scgib_ingest_csr", _ptr(src), _ptr(dst), src.element_size(), e_raw, _ptr(gptr),
                  B, n, INGEST_MAX_GRAPH_NODES, int(bool(bidirect)), int(bool(skip_rule)), _ptr(ws),
                  ws_rows, _ptr(rowptr), _ptr(col), col_cap, _ptr(status), _stream())
        st = status.cpu().numpy()  # the batch's one device -> host read
        if st[0]:
            _ingest_raise(int(st[0]), "scgib_ingest_csr")
        e = int(st[2])
        u64 = lambda lo, hi: (int(lo) & 0xffffffff) | ((int(hi) & 0xffffffff) << 32)  # noqa: E731
        g = GraphBatch(rowptr, col[:e], gptr, np.diff(st[16:16 + B + 1].astype(np.int64)), None,
                       max_graph_nodes=int(st[5]), n_edges=e)
        g.components_closed = True  # verified by the mark launch
        g.ego_k1 = (int(st[3]), u64(st[6], st[7]), u64(st[8], st[9]))
    if x is not None:
        g.ndata["x"] = x
    return g


def from_pyg_batch(batch, skip_rule=False):
    """A GraphBatch from a PyG-style batch: any object with ``edge_index``
    [2, E], ``ptr`` [B+1] and ``x`` (``from_coo`` with ``bidirect=True``;
    ``ndata['x']`` is set)."""
    ei = batch.edge_index
    return from_coo(ei[0], ei[1], batch.ptr, batch.x.shape[0], x=batch.x, bidirect=True,
                    skip_rule=skip_rule)


def as_graph_batch(obj):
    """``obj`` as a GraphBatch: a GraphBatch is returned as is; any other
    object with ``edges()``, ``batch_num_nodes()`` and ``num_nodes()`` (the DGL
    surface the reference's loops use) is converted by ``from_coo`` with
    ``bidirect=False`` -- such a graph is already bidirected and simple, which
    is verified -- and its ``ndata`` tensors are carried over.  The converted
    batch is cached on the object where it accepts attributes, so a loop that
    reuses a graph ingests it once (a graph mutated afterwards is not seen)."""
    if isinstance(obj, GraphBatch):
        return obj
    cached = getattr(obj, "_scgib_graph_batch", None)
    if cached is not None:
        return cached
    if not all(hasattr(obj, a) for a in ("edges", "batch_num_nodes", "num_nodes")):
        raise TypeError(f"{type(obj).__name__} is neither a GraphBatch nor a DGL-like graph "
                        "(edges(), batch_num_nodes(), num_nodes())")
    src, dst = obj.edges()
    g = from_coo(src, dst, None, int(obj.num_nodes()), bidirect=False,
                 batch_num_nodes=obj.batch_num_nodes())
    for key, value in dict(getattr(obj, "ndata", None) or {}).items():
        dict.__setitem__(g.ndata, key, value)
    try:
        obj._scgib_graph_batch = g
    except (AttributeError, TypeError):
        pass
    return g


class StaticBatch:
    """Capacity-sized device buffers of one molecule batch, for HIP-graph
    replay of the training step: every kernel reads the actual node/edge
    counts from ``dims`` (device), so a graph captured on these buffers
    serves every batch of ``B`` molecules that fits the capacities.

    ``load(src)`` copies a padded device batch (``pad(...)``) in with five
    device-to-device copies; nothing is read back to the host.
    """

    def __init__(self, B, n_cap, e_cap, n_feat, max_graph_nodes, ego_caps, device, k=1):
        self.B, self.n_cap, self.e_cap, self.n_feat = B, n_cap, e_cap, n_feat
        self.k = int(k)
        # one byte blob (rowptr | col | graph_ptr | dims | x, 256-B aligned
        # sections) so that loading a batch is a single device copy
        self.blob = torch.zeros(self._layout()[-1], dtype=torch.uint8, device=device)
        self.rowptr, self.col, self.graph_ptr, self.dims, self.err, self.x = \
            self._views(self.blob)
        self.graph = GraphBatch(self.rowptr, self.col, self.graph_ptr, None, None,
                                max_graph_nodes=max_graph_nodes, n_edges=-1)
        self.graph.dims = self.dims
        self.graph.components_closed = True  # pad() refuses batches whose edges leave a molecule
        # ego-net error word, zeroed by every load (no fill launch in the step)
        self.graph.err_buf = self.err
        self.graph.ego_caps = tuple(int(c) for c in ego_caps)

    def _layout(self):
        sizes = [4 * (self.n_cap + 1), 4 * max(self.e_cap, 1), 4 * (self.B + 1), 4 * 4,
                 4 * self.n_cap * self.n_feat]
        offs = [0]
        for sz in sizes:
            offs.append(offs[-1] + (sz + 255) // 256 * 256)
        return offs

    def _views(self, blob):
        o = self._layout()
        i32 = torch.int32
        return (blob[o[0]:o[0] + 4 * (self.n_cap + 1)].view(i32),
                blob[o[1]:o[1] + 4 * max(self.e_cap, 1)].view(i32),
                blob[o[2]:o[2] + 4 * (self.B + 1)].view(i32),
                blob[o[3]:o[3] + 8].view(i32),
                blob[o[3] + 8:o[3] + 12].view(i32),
                blob[o[4]:o[4] + 4 * self.n_cap * self.n_feat].view(torch.float32)
                .view(self.n_cap, self.n_feat))

    @staticmethod
    def capacities(host_batches, k, slack=1.0):
        """(n_cap, e_cap, max_graph_nodes, (ego nodes cap, ego edges cap, max
        in-degree)) covering every host-collated batch given,
        for k-hop ego-nets (k = 1 in closed form, k > 1 from the host
        reachability of each batch, as the reference's offline pass would)."""
        n = max(g.num_nodes() for g in host_batches)
        e = max(g.num_edges() for g in host_batches)
        mgn = max(g.max_graph_nodes for g in host_batches)
        ns = es = dmax = 0
        for g in host_batches:
            bn, be, bd = ego_bounds(g, k)
            ns, es, dmax = max(ns, bn), max(es, be), max(dmax, bd)
        f = lambda v: int(v * slack) + 1  # noqa: E731
        # ego caps: (nodes, edges, max in-degree — selects the k = 1 builder)
        return f(n), f(e), mgn, (f(ns), f(es), dmax if k == 1 else 1 << 30)

    def pad(self, g):
        """Device copy of host batch ``g`` padded to this batch's capacities."""
        n, e = g.num_nodes(), g.num_edges()
        if n > self.n_cap or e > self.e_cap or g.batch_size != self.B:
            raise _lib.ScgibError(f"batch (B={g.batch_size}, N={n}, E={e}) does not fit the "
                                  f"capacities (B={self.B}, N={self.n_cap}, E={self.e_cap})")
        if g.max_graph_nodes > self.graph.max_graph_nodes:
            raise _lib.ScgibError("batch has a larger molecule than the captured bitmap width")
        if not g.host_info["validated"]:
            raise _lib.ScgibError("batch edges leave their molecule")
        ns, es = self.graph.ego_caps[:2]
        bn, be, _ = ego_bounds(g, self.k)
        if bn > ns or be > es:
            raise _lib.ScgibError("batch's ego-nets exceed the ego capacities")
        if len(self.graph.ego_caps) > 2 and len(g.host_info["deg"]) and \
                int(g.host_info["deg"].max()) > self.graph.ego_caps[2]:
            raise _lib.ScgibError("batch's max degree exceeds the captured ego builder's bound")
        if self.B and g.batch_num_nodes_host().min() < 2:
            raise ValueError("Expected more than 1 value per channel when training "
                             "(a molecule with one atom; the reference skips those)")
        blob = np.zeros(self._layout()[-1], np.uint8)
        o = self._layout()
        rp = np.full(self.n_cap + 1, e, np.int32)
        rp[: n + 1] = g.rowptr.cpu().numpy()
        blob[o[0]:o[0] + rp.nbytes] = rp.view(np.uint8)
        col = g.col.cpu().numpy()[:e].astype(np.int32)
        blob[o[1]:o[1] + col.nbytes] = col.view(np.uint8)
        gp = g.graph_ptr.cpu().numpy().astype(np.int32)
        blob[o[2]:o[2] + gp.nbytes] = gp.view(np.uint8)
        blob[o[3]:o[3] + 8] = np.array([n, e], np.int32).view(np.uint8)
        x = np.ascontiguousarray(g.ndata["x"].cpu().numpy().astype(np.float32))
        blob[o[4]:o[4] + x.nbytes] = x.view(np.uint8).reshape(-1)
        dev = self.blob.device
        return {"blob": torch.from_numpy(blob).to(dev), "n": n, "e": e}

    def load(self, padded):
        """Copy a pad()-ed batch into the static buffers (one device copy)."""
        self.blob.copy_(padded["blob"], non_blocking=True)
        self._unload_prefetch()

    def ingest(self, src, dst, graph_ptr, x, counts=None, skip_rule=False):
        """Build a batch into the static buffers from its COO edge list on the
        device (scgib_ingest_blob: three launches, capturable, nothing
        allocated after the first call, nothing read back): afterwards the blob
        holds byte for byte what ``load(pad(collate_pyg(...)))`` leaves.

        ``src`` / ``dst`` [E] int32 or int64 device tensors (batch-global ids;
        reverses and duplicates are folded as ``to_bidirected`` does),
        ``graph_ptr`` [B+1] int32, ``x`` [n, n_feat] fp32.  ``counts=None``
        takes n and E from the tensor shapes.  A device ``counts`` int32 [2] =
        (n, E) makes ``src`` / ``dst`` / ``x`` capacity-sized staging buffers
        (``x`` of at least ``n_cap`` rows) whose contents change between the
        replays of a graph that captured this call.

        A batch that does not fit (``n_cap``, ``e_cap``, the ego capacities,
        the bitmap width), holds a molecule with fewer than two atoms or fails
        a check leaves the blob exactly as it was; its error bits
        (``_lib.INGEST_ERRORS``) are OR-ed into a sticky word:
        ``ingest_error()`` / ``reset_ingest_error()``.

        Limited to k = 1: the general ego builder has no capacity guard of its
        own and the k >= 2 ego bound needs reachability, which the ingest does
        not compute; a static batch with k >= 2 raises ScgibError."""
        if self.k != 1:
            raise _lib.ScgibError(f"StaticBatch.ingest is limited to k = 1 (this batch has k = "
                                  f"{self.k}): the k >= 2 ego bounds need reachability")
        dev = self.blob.device
        if dev.type != "cuda":
            raise _lib.ScgibError("StaticBatch.ingest needs a HIP device (no CPU fallback)")
        caps = self.graph.ego_caps
        if len(caps) < 3 or self.graph.max_graph_nodes > INGEST_MAX_GRAPH_NODES or \
                self.graph.max_graph_nodes < 1:
            raise _lib.ScgibError("StaticBatch.ingest needs (nodes, edges, max in-degree) ego "
                                  f"capacities and molecules of 1..{INGEST_MAX_GRAPH_NODES} atoms")
        i32 = torch.int32
        ok = (src.device == dev and dst.device == dev and src.dtype == dst.dtype and
              src.dtype in (i32, torch.int64) and src.dim() == 1 and src.shape == dst.shape and
              src.is_contiguous() and dst.is_contiguous() and
              graph_ptr.device == dev and graph_ptr.dtype == i32 and graph_ptr.is_contiguous() and
              tuple(graph_ptr.shape) == (self.B + 1,) and
              x.device == dev and x.dtype == torch.float32 and x.is_contiguous() and
              x.dim() == 2 and x.shape[1] == self.n_feat)
        if counts is not None:
            ok = ok and (counts.device == dev and counts.dtype == i32 and counts.numel() >= 2 and
                         counts.is_contiguous() and x.shape[0] >= self.n_cap)
        if not ok:
            raise _lib.ScgibError(
                "StaticBatch.ingest: src / dst (int32 or int64 [E]), graph_ptr (int32 [B+1]), x "
                "(fp32 [n, n_feat]; with counts at least n_cap rows) and counts (int32 [2]) must "
                "be contiguous tensors on the static batch's device")
        if getattr(self, "_ingest_ws", None) is None:
            self._ingest_ws = torch.zeros(
                int(_lib.query("scgib_ingest_workspace_bytes", self.n_cap,
                               self.graph.max_graph_nodes)), dtype=torch.uint8, device=dev)
            self._ingest_err = torch.zeros(1, dtype=i32, device=dev)
        o = self._layout()
        desc = _lib.IngestDesc(
            src=src.data_ptr(), dst=dst.data_ptr(), graph_ptr=graph_ptr.data_ptr(),
            x=x.data_ptr(), counts=None if counts is None else counts.data_ptr(),
            ws=self._ingest_ws.data_ptr(), status=None, sticky=self._ingest_err.data_ptr(),
            blob=self.blob.data_ptr(), e_raw=int(src.numel()), n=int(x.shape[0]),
            n_cap=self.n_cap, e_cap=self.e_cap, ego_n_cap=int(caps[0]), ego_e_cap=int(caps[1]),
            o_rowptr=o[0], o_col=o[1], o_gptr=o[2], o_dims=o[3], o_x=o[4],
            blob_bytes=self.blob.numel(), B=self.B, F=self.n_feat, idx_bytes=src.element_size(),
            max_graph_nodes=self.graph.max_graph_nodes, max_in_degree=min(int(caps[2]), 1 << 30),
            bidirect=1, skip_rule=int(bool(skip_rule)), pad_=0)
        # (a captured graph reads these buffers at every replay: keep them alive)
        self._ingest_keep = (src, dst, graph_ptr, x, counts)
        _lib.call("scgib_ingest_blob", ctypes.byref(desc), _stream())
        self._unload_prefetch()

    def ingest_error(self):
        """The sticky error bits of the ingests so far (0 = none;
        ``_lib.INGEST_ERRORS``) -- a device read, for outside the loop."""
        err = getattr(self, "_ingest_err", None)
        return 0 if err is None else int(err.item())

    def reset_ingest_error(self):
        err = getattr(self, "_ingest_err", None)
        if err is not None:
            err.zero_()

    def _unload_prefetch(self):
        pf = getattr(self.graph, "ego_prefetch", None)
        if pf is not None:
            pf.loaded = False  # its ego buffers no longer match the static batch

    def pool(self, padded):
        """Device state for load_next over the pad()-ed batches ``padded``: the
        table of their blobs and the cursor (kept alive by the caller along
        with ``padded``)."""
        dev = self.blob.device
        for p in padded:
            if p["blob"].numel() != self.blob.numel():
                raise _lib.ScgibError("pool batch was padded for other capacities")
        table = torch.tensor([p["blob"].data_ptr() for p in padded], dtype=torch.int64, device=dev)
        return {"table": table, "cursor": torch.zeros(2, dtype=torch.int32, device=dev),
                "n": len(padded), "batches": padded}

    def load_next(self, pool, prefetch=None):
        """Copy the pool's next batch in (one kernel, capturable: the replays of
        a graph holding it walk the pool in order, pool(...)[cursor] first).
        With an EgoPrefetch the same launch also moves the ego-nets it built
        for this batch into the step's ego buffers."""
        src2 = dst2 = None
        n2 = 0
        self._unload_prefetch()
        if prefetch is not None:
            if prefetch.pool is not pool:
                raise _lib.ScgibError("EgoPrefetch was made for another pool")
            # a prefetch no backward joined (a forward without backward) must
            # be done with the staging blob before this copy reads it
            prefetch.join()
            src2, dst2, n2 = _ptr(prefetch.staging), _ptr(prefetch.blob), prefetch.blob.numel()
            prefetch.loaded = True
        _lib.call("scgib_pool_copy2", ctypes.c_void_p(pool["table"].data_ptr()), pool["n"],
                  ctypes.c_void_p(pool["cursor"].data_ptr()), ctypes.c_void_p(self.blob.data_ptr()),
                  self.blob.numel(), src2, dst2, n2,
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def blob_offsets(self):
        """Byte offsets of (rowptr, col, graph_ptr, dims) inside each blob."""
        o = self._layout()
        return o[0], o[1], o[2], o[3]

    def ego_error(self):
        """Error bits the ego-net build of the last step flagged (0 = none; see
        egonet_batch) — a device read, for checks outside the timed loop."""
        return int(self.err.item())


class EgoPrefetch:
    """The ego-nets one batch ahead, for a replayed step over a StaticBatch
    pool (bench.py): step t builds the ego-nets of the batch step t + 1 will
    load — straight from that batch's pool blob, on the encoder pair's queue
    while it would otherwise idle through the loss section
    (models._encode_forked) — into a staging blob, and step t + 1's batch load
    (StaticBatch.load_next) moves them into the ego buffers the step reads.
    Every step still builds one batch's ego-nets (the reference's
    khop_in_subgraph pass, exp_pretraining.py:269-272); the build leaves the
    head of the step's critical path.  k = 1 within the one-pass builder's
    bounds: scgib_egonet_k1_build_onepass_pool; otherwise (k >= 2) the
    bitmap builder's count + fill, scgib_egonet_count_pool / _fill_pool.

    ``prime()`` builds the ego-nets of the pool's current batch once before
    the first step (eager).  ``ego`` is the step's ego batch (capacity mode,
    the same layout egonet_batch gives)."""

    def __init__(self, static, pool):
        g = static.graph
        caps = g.ego_caps or ()
        kmax = int(_lib.query("scgib_egonet_k1_max_degree"))
        self.onepass = (static.k == 1 and EGO_K1_FAST and len(caps) > 2 and caps[2] <= kmax and
                        g.max_graph_nodes <= int(_lib.query("scgib_egonet_k1_max_graph_nodes")))
        if len(caps) < 2 or g.max_graph_nodes > 512:
            raise _lib.ScgibError("EgoPrefetch needs ego capacities and molecules of <= 512 atoms")
        self.static, self.pool, self.k = static, pool, static.k
        self.n = g.num_nodes()
        self.n_s, self.e_cap = int(caps[0]), int(caps[1])
        self.dmax = int(caps[2]) if len(caps) > 2 else 0
        dev = static.blob.device
        # ego_ptr | ego_eptr | ego_nodes | sub_rowptr | sub_col | (ego dims, error bits)
        sizes = [4 * (self.n + 1), 4 * (self.n + 1), 4 * max(self.n_s, 1), 4 * (self.n_s + 1),
                 4 * max(self.e_cap, 1), 16]
        offs = [0]
        for sz in sizes:
            offs.append(offs[-1] + (sz + 255) // 256 * 256)
        self._offs, self._sizes = offs, sizes
        self.blob = torch.zeros(offs[-1], dtype=torch.uint8, device=dev)
        self.staging = torch.zeros(offs[-1], dtype=torch.uint8, device=dev)
        self.views = self._views(self.blob)
        self.next_views = self._views(self.staging)
        ego_ptr, _, ego_nodes, sub_rowptr, sub_col, ego_dims, self.err = self.views
        self.ego = _ego_graph(g, sub_rowptr, sub_col, ego_ptr, ego_nodes, self.n_s, ego_dims)
        self.ws = None if self.onepass else torch.empty(
            int(_lib.query("scgib_egonet_workspace_bytes", self.n)), dtype=torch.uint8, device=dev)
        self.loaded = False  # ego holds the static batch's ego-nets (load_next with this)
        self._side = None  # stream of a prefetch not yet joined back (join())
        g.ego_prefetch = self  # models._encode_forked takes ego from here when loaded

    def _views(self, blob):
        i32 = torch.int32
        v = [blob[o:o + sz].view(i32) for o, sz in zip(self._offs, self._sizes)]
        tail = v.pop()
        return (*v, tail[:2], tail[2:3])

    def prefetch(self):
        """Enqueue (current stream) the build of the ego-nets of the pool's
        batch at the cursor — the one the next load_next copies in — into the
        staging blob."""
        ego_ptr, ego_eptr, ego_nodes, sub_rowptr, sub_col, ego_dims, err = self.next_views
        o_rp, o_col, o_gptr, o_dims = self.static.blob_offsets()
        src = (_ptr(self.pool["table"]), self.pool["n"], _ptr(self.pool["cursor"]))
        if self.onepass:
            from . import ops  # (ops imports this module)
            state = ops.scan_state(self.blob.device, "egonet_k1_scan_prefetch",
                                   int(_lib.query("scgib_egonet_k1_scan_words", self.n)))
            _lib.call("scgib_egonet_k1_build_onepass_pool", *src, o_rp, o_col, o_dims, self.n,
                      self.dmax, _ptr(ego_ptr), _ptr(ego_eptr), _ptr(state), _ptr(ego_nodes),
                      _ptr(sub_rowptr), _ptr(sub_col), self.n_s, max(self.e_cap, 1), _ptr(err),
                      _ptr(ego_dims), _stream())
            return
        g = self.static.graph
        mgn = max(g.max_graph_nodes, 1)
        _lib.call("scgib_egonet_count_pool", *src, o_rp, o_col, o_gptr, o_dims, g.batch_size,
                  self.n, self.k, mgn, _ptr(ego_ptr), _ptr(ego_eptr), _ptr(self.ws), _ptr(err),
                  _stream())
        _lib.call("scgib_egonet_fill_pool", *src, o_rp, o_col, o_gptr, o_dims, g.batch_size,
                  self.n, self.k, mgn, _ptr(ego_ptr), _ptr(ego_eptr), _ptr(ego_nodes),
                  _ptr(sub_rowptr), _ptr(sub_col), _ptr(err), self.n_s, _ptr(ego_dims), _stream())

    def error(self):
        """Error bits any prefetched build flagged (sticky; 0 = none; see
        egonet_batch) — a device read, for checks outside the timed loop."""
        return int(self.err.item())

    def prime(self):
        """The ego-nets of the pool's batch at the cursor into staging, before
        the first load_next (eager, current stream)."""
        self.prefetch()

    def __call__(self):
        """The encoder pair's side tail: prefetch on the current stream, which
        the pair's backward joins back (joined()) — else join() does."""
        self.prefetch()
        self._side = torch.cuda.current_stream()

    def joined(self):
        self._side = None

    def join(self):
        """Order the current stream after a prefetch that no backward joined
        (e.g. a forward without backward); no-op otherwise."""
        if self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)
            self._side = None


# ---------------------------------------------------------------------------
# A15: logM reconstruction targets (host data preparation, like the
# reference's offline pass exp_tudataset.py:416-449)
# ---------------------------------------------------------------------------
def trans_logM(g, kstep):
    """util.getM_logM (util.py:74-91) + GetProbTranMat (:60-71) of one molecule:
    A^1..A^k of the dense adjacency, each column-normalised,
    log(A^i / colsum) - log(1/n), negatives / -inf / NaN set to 0; computed in
    float64 like the reference's numpy and returned as float32 [k, n, n]
    (exp_tudataset.py:433)."""
    n = g.num_nodes()
    A = g.adj().to_dense().cpu().numpy().astype(np.float32)
    Ak = np.identity(n)
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(kstep):
            Ak = Ak @ A
            colsum = np.repeat(Ak.sum(axis=0).reshape(1, -1), n, axis=0)
            P = np.log(np.divide(Ak, colsum)) - np.log(1.0 / n)
            P[P < 0] = 0
            P[np.isnan(P)] = 0
            out.append(P)
    return torch.from_numpy(np.array(out)).float()


class LogMBatch:
    """Device form of a batch's logM targets for scgib_recon_logm_*: per molecule
    S = sum_i logM_i ([n, n] fp32, packed at int64 offsets) and
    C = sum_i ||logM_i||_F^2 (fp64); kstep = k."""

    def __init__(self, logms, device):
        logms = [torch.as_tensor(m) for m in logms]
        if not logms:
            raise GraphIngestError("empty logM batch")
        self.kstep = int(logms[0].shape[0])
        sizes, S, C = [], [], []
        for m in logms:
            if m.dim() != 3 or m.shape[0] != self.kstep or m.shape[1] != m.shape[2]:
                raise GraphIngestError(f"logM target of shape {tuple(m.shape)}: expected "
                                       f"[{self.kstep}, n, n]")
            m64 = m.double()
            sizes.append(m.shape[1])
            S.append(m64.sum(0).float().reshape(-1))
            C.append(float((m64 * m64).sum()))
        off = np.zeros(len(sizes) + 1, np.int64)
        np.cumsum(np.asarray(sizes, np.int64) ** 2, out=off[1:])
        self.sizes = np.asarray(sizes, np.int64)
        self.S = torch.cat(S).to(device)
        self.offsets = torch.from_numpy(off).to(device)
        self.C = torch.tensor(C, dtype=torch.float64, device=device)


# ---------------------------------------------------------------------------
# A15 on the device: logM targets on the slots of the step's own ego-nets
# (csrc/logm.hip)
# ---------------------------------------------------------------------------
class LogMSparse:
    """A batch's logM targets on the slots of its k-hop ego batch (slot j of
    ball(c) <-> r = ego_nodes[j]): ``s_in`` = S[r, c], ``s_sym`` = S[r, c] +
    S[c, r] with S = sum_i logM_i (fp32), ``C`` [B] = sum_i ||logM_i||_F^2
    (fp64), ``kstep`` = k.  ``ego_ptr`` / ``ego_nodes`` are the ego batch's
    own tensors, ``graph_ptr`` the molecule batch's; ``err`` is the device
    error word (``error()``; shared with the ego builder's on a StaticBatch
    graph, where ``StaticBatch.ego_error()`` reads it).  ``dims``: the batch's
    device sizes in capacity mode, else None."""

    def __init__(self, s_in, s_sym, C, kstep, ego_ptr, ego_nodes, graph_ptr, err=None,
                 max_graph_nodes=512, dims=None):
        self.s_in, self.s_sym, self.C = s_in, s_sym, C
        self.kstep = int(kstep)
        self.ego_ptr, self.ego_nodes, self.graph_ptr = ego_ptr, ego_nodes, graph_ptr
        self.err = err
        self.max_graph_nodes = int(max_graph_nodes)
        self.dims = dims

    def error(self):
        """Error bits the target build flagged (0 = none; 1: an index leaves
        its molecule, 2: a molecule above 512 nodes, 4: a walk count outside
        the exact domain) — a device read."""
        return 0 if self.err is None else int(self.err.item())

    def to_dense(self):
        """Per-molecule dense S = sum_i logM_i ([n, n] fp32 numpy arrays) on
        the host, zeros outside the balls — for tests and debugging."""
        gp = self.graph_ptr.cpu().numpy().astype(np.int64)
        n = int(gp[-1])
        ep = self.ego_ptr.cpu().numpy().astype(np.int64)[: n + 1]
        n_s = int(ep[-1]) if n else 0
        rows = self.ego_nodes.cpu().numpy().astype(np.int64)[:n_s]
        vals = self.s_in.cpu().numpy()[:n_s]
        cols = np.repeat(np.arange(n), np.diff(ep))
        out = []
        for a, b in zip(gp[:-1], gp[1:]):
            S = np.zeros((b - a, b - a), np.float32)
            m = slice(int(ep[a]), int(ep[b]))
            S[rows[m] - a, cols[m] - a] = vals[m]
            out.append(S)
        return out


def logm_targets(g: GraphBatch, k: int, ego=None) -> LogMSparse:
    """The logM targets of ``g`` (util.getM_logM per molecule, k steps) built
    on ``g``'s HIP device from its k-hop ego batch (scgib_logm_targets); no
    host work, no n^2 buffer, capturable on a StaticBatch graph.  ``ego``: the
    ``egonet_batch(g, k)`` of the same graph if the caller already has it."""
    if g.device.type != "cuda":
        raise _lib.ScgibError("logm_targets needs the graph on a HIP device (no CPU fallback)")
    if not g.symmetric:
        raise _lib.ScgibError("logm_targets expects a symmetric (to_bidirected) graph")
    k = int(k)
    kmax = int(_lib.query("scgib_logm_max_k"))
    if not 1 <= k <= kmax:
        raise _lib.ScgibError(f"logm_targets: k = {k} outside the supported 1..{kmax}")
    if ego is None:
        ego = egonet_batch(g, k)
    dev = g.device
    ego_nodes = ego.ndata["_ID"]
    n_s = int(ego_nodes.shape[0])
    B, n = g.batch_size, g.num_nodes()
    if B == 0 or n == 0 or n_s == 0:
        raise _lib.ScgibError("logm_targets: empty batch")
    err = getattr(g, "err_buf", None)
    if err is None:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.empty(k * n_s, dtype=torch.int32, device=dev)
    s_in = torch.empty(n_s, dtype=torch.float32, device=dev)
    s_sym = torch.empty(n_s, dtype=torch.float32, device=dev)
    C = torch.empty(B, dtype=torch.float64, device=dev)
    _lib.call("scgib_logm_targets", _ptr(g.rowptr), _ptr(g.col), _ptr(g.graph_ptr), B, n,
              g.edge_capacity(), _ptr(ego.graph_ptr), _ptr(ego_nodes), n_s, k, _ptr(counts),
              _ptr(s_in), _ptr(s_sym), _ptr(C), _ptr(err), _ptr(g.dims), _stream())
    if g.dims is None:
        code = int(err.item())
        if code:
            raise _lib.ScgibError(f"scgib_logm_targets flagged error bits {code} (1: an index "
                                  "leaves its molecule, 2: a molecule above 512 nodes, 4: a "
                                  "walk count outside the exact domain)")
    return LogMSparse(s_in, s_sym, C, k, ego.graph_ptr, ego_nodes, g.graph_ptr, err,
                      max(g.max_graph_nodes, 1), g.dims)


# ---------------------------------------------------------------------------
# device-side collation of shuffled batches from a resident dataset
# (csrc/collate.hip)
# ---------------------------------------------------------------------------
COLLATE_MAX_BATCH = 4096  # scgib_collate_max_batch(): the plan launch is one workgroup
EGO_MAX_GRAPH_NODES = 512  # the ego builder's bitmap width
_DS_CHUNK = 2048  # molecules per host pass (ingest, k >= 2 ego bounds)


def _segment_sum(values, ptr):
    """Sums of ``values`` over the non-empty segments ptr[i]:ptr[i+1]."""
    if len(ptr) <= 1:
        return np.zeros(0, np.int64)
    return np.add.reduceat(np.asarray(values, np.int64), ptr[:-1])


def _molecule_ego_bounds(gptr, rowptr, deg, col, selfloops, k):
    """ego_bounds per molecule: (ego nodes [M], ego edge bound [M]) of flat
    molecule CSRs (molecule-local ``col``).  k = 1 in closed form; k >= 2 by
    the host reachability over chunks of molecules (block-diagonal, so one
    sparse product per chunk) with per-molecule segment sums."""
    deg64 = deg.astype(np.int64)
    if k == 1:
        ball = 1 + deg64 - selfloops
        return _segment_sum(ball, gptr), _segment_sum(deg64 * ball, gptr)
    import scipy.sparse as sp
    M = len(gptr) - 1
    nodes, edges = np.zeros(M, np.int64), np.zeros(M, np.int64)
    for a in range(0, M, _DS_CHUNK):
        b = min(a + _DS_CHUNK, M)
        n0, n1 = int(gptr[a]), int(gptr[b])
        e0, e1 = int(rowptr[n0]), int(rowptr[n1])
        n = n1 - n0
        local_ptr = gptr[a:b + 1] - n0
        owner_off = np.repeat(local_ptr[:-1], np.diff(local_ptr))  # node offset of each node's molecule
        indptr = rowptr[n0:n1 + 1] - e0
        cols = col[e0:e1].astype(np.int64) + np.repeat(owner_off, deg64[n0:n1])
        adj = sp.csr_matrix((np.ones(len(cols), np.int8), cols, indptr), shape=(n, n))
        step = (adj + sp.identity(n, dtype=np.int8, format="csr")).astype(bool).astype(np.int32)
        r = step
        for _ in range(k - 1):
            r = (r @ step).astype(bool).astype(np.int32)
        r.sort_indices()
        nodes[a:b] = _segment_sum(np.diff(r.indptr), local_ptr)
        edges[a:b] = _segment_sum(r @ deg64[n0:n1], local_ptr)
    return nodes, edges


class DeviceDataset:
    """A molecule dataset resident on the device as flat per-molecule CSRs,
    for device-side collation (DeviceLoader).  A collated batch is the offset
    concatenation of its molecules' rows, so the stored rows are exactly what
    ``collate_pyg`` / ``CSRCache.collate`` produce (the same ingest, once, on
    the host).  Features are stored as given (the caller normalises them).

    Device arrays (``arrays``; the same names on the host in ``host``):
    ``node_off`` / ``edge_off`` [M+1] int64, ``rp_local`` [nodes] int32 (row
    pointer of a node inside its molecule's edge range), ``col`` [edges] int32
    (molecule-local), ``x`` [nodes, F] fp32, ``y`` [M, T] fp32 or None (NaN
    kept), ``ego_nodes`` / ``ego_edges`` [M] int32 (``ego_bounds`` of each
    molecule for ``k``).  Host facts: ``node_counts`` / ``edge_counts`` [M],
    ``max_graph_nodes``, ``max_in_degree``, ``dropped`` (one-atom molecules
    left out under ``drop_single_atom``)."""

    def __init__(self, gptr, deg, col, x, y, device, k, drop_single_atom=False):
        gptr = np.asarray(gptr, np.int64)
        deg = np.asarray(deg, np.int32)
        col = np.asarray(col, np.int32)
        x = np.ascontiguousarray(np.asarray(x, np.float32))
        if x.ndim != 2 or x.shape[0] != gptr[-1] or len(deg) != gptr[-1] or \
                int(deg.astype(np.int64).sum()) != len(col):
            raise GraphIngestError("DeviceDataset: inconsistent flat arrays")
        if y is not None:
            y = np.asarray(y, np.float32)
            y = None if y.size == 0 else np.ascontiguousarray(y.reshape(len(gptr) - 1, -1))
        counts = np.diff(gptr)
        self.dropped = 0
        small = counts < 2
        if small.any():
            if not drop_single_atom:
                raise GraphIngestError(
                    f"DeviceDataset: molecule {int(np.flatnonzero(small)[0])} has fewer than two "
                    "atoms (StaticBatch.pad refuses those; drop_single_atom=True leaves them out, "
                    "as the reference skips them)")
            keep = ~small
            node_keep = np.repeat(keep, counts)
            edge_keep = np.repeat(node_keep, deg)
            deg, col, x = deg[node_keep], col[edge_keep], x[node_keep]
            y = None if y is None else y[keep]
            counts = counts[keep]
            gptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            self.dropped = int(small.sum())
        M = len(counts)
        if M == 0:
            raise GraphIngestError("DeviceDataset: no molecules")
        if int(counts.max()) > EGO_MAX_GRAPH_NODES:
            raise GraphIngestError(
                f"DeviceDataset: molecule {int(counts.argmax())} has {int(counts.max())} atoms, "
                f"above the ego builder's limit of {EGO_MAX_GRAPH_NODES}")
        rowptr = np.concatenate([[0], np.cumsum(deg, dtype=np.int64)])
        n_tot = int(gptr[-1])
        owner = np.repeat(np.arange(M), counts)
        node_count_of_edge = np.repeat(counts[owner], deg)
        if len(col) and (col.min() < 0 or (col >= node_count_of_edge).any()):
            raise GraphIngestError("DeviceDataset: an edge leaves its molecule")
        edge_off = rowptr[gptr]
        rp_local = (rowptr[:-1] - edge_off[owner]).astype(np.int32)
        local_row = np.arange(n_tot) - gptr[owner]
        rows = np.repeat(np.arange(n_tot), deg)
        selfloops = np.bincount(rows[col == local_row[rows]], minlength=n_tot).astype(np.int64)
        ego_n, ego_e = _molecule_ego_bounds(gptr, rowptr, deg, col, selfloops, int(k))
        if len(ego_e) and max(int(ego_n.max()), int(ego_e.max())) >= 2 ** 31:
            raise GraphIngestError("DeviceDataset: a molecule's ego bound passes int32")
        self.k = int(k)
        self.num_graphs, self.num_features = M, int(x.shape[1])
        self.num_tasks = 0 if y is None else int(y.shape[1])
        self.node_counts, self.edge_counts = counts, np.diff(edge_off)
        self.max_graph_nodes = int(counts.max())
        self.max_in_degree = int(deg.max()) if len(deg) else 0
        self.host = {"node_off": gptr, "edge_off": edge_off.astype(np.int64), "rp_local": rp_local,
                     "col": col, "x": x, "y": y, "ego_nodes": ego_n.astype(np.int32),
                     "ego_edges": ego_e.astype(np.int32)}
        self.device = torch.device(device)
        # (a memory-mapped cache array is read-only: torch wants a writable source)
        self.arrays = {key: None if v is None else
                       torch.from_numpy(v if v.flags.writeable else v.copy()).to(self.device)
                       for key, v in self.host.items()}

    def __len__(self):
        return self.num_graphs

    @classmethod
    def from_cache(cls, cache, device, k, drop_single_atom=False):
        """From a cache.CSRCache (its flat arrays are already in ingest order)."""
        return cls(np.asarray(cache.graph_ptr), np.asarray(cache.deg), np.asarray(cache.col),
                   np.asarray(cache.x), np.asarray(cache.y), device, k, drop_single_atom)

    @classmethod
    def from_molecules(cls, molecules, device, k, labels=None, drop_single_atom=False):
        """From PyG-style ``(edge_index, x)`` molecules, normalised through
        collate_pyg (to_bidirected, (src, dst)-sorted) in chunks; a molecule
        whose feature rows do not match its inferred node count raises."""
        molecules = list(molecules)
        counts, degs, cols, xs = [], [], [], []
        for a in range(0, len(molecules), _DS_CHUNK):
            g, _ = collate_pyg(molecules[a:a + _DS_CHUNK], skip_invalid=False)
            if not g.host_info["validated"]:
                raise GraphIngestError("DeviceDataset: an edge leaves its molecule")
            rp = g.rowptr.numpy().astype(np.int64)
            c = g.col.numpy().astype(np.int64)[: rp[-1]]
            bnn = g.batch_num_nodes_host().astype(np.int64)
            gp = np.concatenate([[0], np.cumsum(bnn)])
            node_off = np.repeat(gp[:-1], bnn)
            degs.append(np.diff(rp).astype(np.int32))
            cols.append((c - np.repeat(node_off, np.diff(rp))).astype(np.int32))
            xs.append(g.ndata["x"].numpy().astype(np.float32))
            counts.append(bnn)
        if not counts:
            raise GraphIngestError("DeviceDataset: no molecules")
        counts = np.concatenate(counts)
        y = None
        if labels is not None:
            y = np.asarray(labels, np.float32).reshape(len(molecules), -1)
        return cls(np.concatenate([[0], np.cumsum(counts)]), np.concatenate(degs),
                   np.concatenate(cols), np.concatenate(xs), y, device, k, drop_single_atom)

    def capacities(self, B, mode="worst", slack=1.0, samples=64, seed=0, indices=None):
        """The tuple StaticBatch.capacities returns, for batches of ``B``
        molecules of this dataset.  ``"worst"``: the sums of the B largest
        per-molecule node, edge and ego values, so no batch can overflow.
        ``"sampled"``: the maxima over ``samples`` seeded random batches times
        ``slack``, as StaticBatch.capacities takes them over host batches; a
        batch above them is skipped by the loader (DeviceLoader.error).
        ``"sequential"``: the exact maxima (no slack, nothing added) over
        every batch a DeviceEvalLoader builds from ``indices`` -- one id list
        or a list of id lists, default the whole dataset -- the last batch's
        fill rows included, so one static batch sized this way serves each of
        the subsets and cannot overflow."""
        B = int(B)
        per = [self.node_counts, self.edge_counts, self.host["ego_nodes"].astype(np.int64),
               self.host["ego_edges"].astype(np.int64)]
        dmax = self.max_in_degree if self.k == 1 else 1 << 30
        if mode == "sequential":
            if B < 1:
                raise _lib.ScgibError(f"capacities: batch size {B} below 1")
            if indices is None:
                subsets = [np.arange(self.num_graphs)]
            elif len(indices) and np.ndim(indices[0]) > 0:
                subsets = list(indices)
            else:
                subsets = [indices]
            tops = [0, 0, 0, 0]
            for sub in subsets:
                ids = sequential_ids(self, sub, B)[0]
                tops = [max(t, int(v[ids].sum(axis=1).max())) for t, v in zip(tops, per)]
            return tops[0], tops[1], self.max_graph_nodes, (tops[2], tops[3], dmax)
        if indices is not None:
            raise ValueError("capacities: indices go with mode \"sequential\"")
        if not 1 <= B <= self.num_graphs:
            raise _lib.ScgibError(f"capacities: batch size {B} outside 1..{self.num_graphs}")
        if mode == "worst":
            tops = [int(np.sort(v)[-B:].sum()) for v in per]
        elif mode == "sampled":
            rng = np.random.default_rng(seed)
            tops = [0, 0, 0, 0]
            for _ in range(int(samples)):
                ids = rng.choice(self.num_graphs, B, replace=False)
                tops = [max(t, int(v[ids].sum())) for t, v in zip(tops, per)]
        else:
            raise ValueError(f"capacities: mode {mode!r} (\"worst\", \"sampled\" or "
                             "\"sequential\")")
        f = lambda v: int(v * slack) + 1  # noqa: E731
        return f(tops[0]), f(tops[1]), self.max_graph_nodes, (f(tops[2]), f(tops[3]), dmax)


def collate_blob_host(host, ids, static):
    """The batch of molecules ``ids`` (in that order, repeats allowed) of a
    DeviceDataset's host arrays (``dataset.host``) as ``static``'s blob, in
    numpy: (blob uint8, labels [B, T] or None, ids int32).  What
    scgib_collate_fill writes into a ring slot, and byte for byte what
    ``static.pad(collate_pyg([...]))["blob"]`` holds:

      rowptr [n_cap+1]  edge offset of the molecule + the node's local row
                        pointer; rowptr[n..] = e
      col [max(e_cap,1)] molecule-local id + node offset of the molecule; 0 past e
      graph_ptr [B+1]   node offsets
      dims [4]          n, e, the ego error word (0), 0
      x [n_cap, F]      the molecules' feature rows; 0 past n
    each section at its 256-byte aligned offset (StaticBatch._layout)."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    node_off, edge_off = host["node_off"], host["edge_off"]
    if len(ids) != static.B or (len(ids) and (ids.min() < 0 or ids.max() >= len(node_off) - 1)):
        raise _lib.ScgibError("collate_blob_host: ids do not form one batch of the dataset")
    n_i = node_off[ids + 1] - node_off[ids]
    e_i = edge_off[ids + 1] - edge_off[ids]
    gptr = np.concatenate([[0], np.cumsum(n_i)])
    eoff = np.concatenate([[0], np.cumsum(e_i)])
    n, e = int(gptr[-1]), int(eoff[-1])
    ns, es = static.graph.ego_caps[:2]
    if n > static.n_cap or e > static.e_cap or int(host["ego_nodes"][ids].sum()) > ns or \
            int(host["ego_edges"][ids].sum()) > es:
        raise _lib.ScgibError("collate_blob_host: the batch does not fit the capacities")
    nodes = np.repeat(node_off[ids] - gptr[:-1], n_i) + np.arange(n)
    edges = np.repeat(edge_off[ids] - eoff[:-1], e_i) + np.arange(e)
    o = static._layout()
    blob = np.zeros(o[-1], np.uint8)
    rp = np.full(static.n_cap + 1, e, np.int32)
    rp[:n] = host["rp_local"][nodes] + np.repeat(eoff[:-1], n_i)
    blob[o[0]:o[0] + rp.nbytes] = rp.view(np.uint8)
    col = (host["col"][edges].astype(np.int64) + np.repeat(gptr[:-1], e_i)).astype(np.int32)
    blob[o[1]:o[1] + col.nbytes] = col.view(np.uint8)
    gp = gptr.astype(np.int32)
    blob[o[2]:o[2] + gp.nbytes] = gp.view(np.uint8)
    blob[o[3]:o[3] + 8] = np.array([n, e], np.int32).view(np.uint8)
    x = np.ascontiguousarray(host["x"][nodes])
    blob[o[4]:o[4] + x.nbytes] = x.view(np.uint8).reshape(-1)
    labels = None if host["y"] is None else host["y"][ids]
    return blob, labels, ids.astype(np.int32)


def _subset_ids(dataset, indices, who):
    """``indices`` (None: every molecule) as a checked int64 id list."""
    if indices is None:
        return np.arange(dataset.num_graphs, dtype=np.int64)
    ids = np.asarray(indices)
    if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
        raise _lib.ScgibError(f"{who}: indices must be a 1-D integer array of molecule ids")
    if ids.size == 0:
        raise _lib.ScgibError(f"{who}: an empty subset")
    ids = ids.astype(np.int64)
    if ids.min() < 0 or ids.max() >= dataset.num_graphs:
        bad = ids[(ids < 0) | (ids >= dataset.num_graphs)][0]
        raise _lib.ScgibError(f"{who}: molecule id {int(bad)} outside 0..{dataset.num_graphs - 1}")
    return ids


def sequential_fill_id(dataset, indices):
    """The molecule a DeviceEvalLoader fills the last batch of ``indices`` up
    with: the subset's smallest by atom count, then edge count, then id."""
    ids = _subset_ids(dataset, indices, "sequential_fill_id")
    order = np.lexsort((ids, dataset.edge_counts[ids], dataset.node_counts[ids]))
    return int(ids[order[0]])


def sequential_ids(dataset, indices, B):
    """The sequential batches of ``indices`` as (molecule ids [steps, B] with
    the fill molecule in the rows past the list's end, the same with -1
    there): what DeviceEvalLoader collates and what it reports in ``ids``."""
    ids = _subset_ids(dataset, indices, "sequential_ids")
    B = int(B)
    steps = -(-len(ids) // B)
    pad = steps * B - len(ids)
    rows = np.concatenate([ids, np.full(pad, sequential_fill_id(dataset, ids), np.int64)])
    marked = np.concatenate([ids, np.full(pad, -1, np.int64)])
    return rows.reshape(steps, B), marked.reshape(steps, B)


def sequential_blob_host(dataset, indices, j, static):
    """Batch ``j`` of the sequential batches of ``indices`` through
    collate_blob_host: (blob, labels with NaN rows at the fill positions or
    None, ids int32 with -1 there)."""
    rows, marked = sequential_ids(dataset, indices, static.B)
    blob, labels, _ = collate_blob_host(dataset.host, rows[j], static)
    if labels is not None:
        labels = labels.copy()
        labels[marked[j] < 0] = np.nan
    return blob, labels, marked[j].astype(np.int32)


def _loader_checks(who, ds, static):
    """What both loaders ask of a static batch; returns (ego caps, device)."""
    B = int(static.B)
    if not 1 <= B <= COLLATE_MAX_BATCH:
        raise _lib.ScgibError(f"{who}: batch size {B} outside 1..{COLLATE_MAX_BATCH}")
    caps = static.graph.ego_caps or ()
    if len(caps) < 2:
        raise _lib.ScgibError(f"{who}: the static batch has no ego capacities")
    if static.n_feat != ds.num_features or static.k != ds.k:
        raise _lib.ScgibError(f"{who}: static batch and dataset differ in feature "
                              "width or ego radius k")
    if ds.max_graph_nodes > static.graph.max_graph_nodes:
        raise _lib.ScgibError(f"{who}: the dataset has a larger molecule than the "
                              "static batch's bitmap width")
    if len(caps) > 2 and ds.max_in_degree > caps[2]:
        raise _lib.ScgibError(f"{who}: the dataset's max in-degree exceeds the "
                              "static batch's ego builder bound")
    dev = static.blob.device
    if ds.device != dev:
        raise _lib.ScgibError(f"{who}: dataset and static batch on different devices")
    return caps, dev


def _loader_ring(static, dev):
    """(ring, slots, pool): three blobs of ``static``'s layout in one
    allocation, as the pool StaticBatch.pool returns."""
    nbytes = static.blob.numel()
    ring = torch.zeros(3 * nbytes, dtype=torch.uint8, device=dev)
    slots = [ring[i * nbytes:(i + 1) * nbytes] for i in range(3)]
    pool = {"table": torch.tensor([s.data_ptr() for s in slots], dtype=torch.int64, device=dev),
            "cursor": torch.zeros(2, dtype=torch.int32, device=dev), "n": 3,
            "batches": [{"blob": s} for s in slots]}
    return ring, slots, pool


def _collate_desc(ds, static, caps, loader, M, S):
    a = ds.arrays
    o = static._layout()
    p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    return _lib.CollateDesc(
        node_off=p(a["node_off"]), edge_off=p(a["edge_off"]), rp_local=p(a["rp_local"]),
        col=p(a["col"]), x=p(a["x"]), y=p(a["y"]), ego_nodes=p(a["ego_nodes"]),
        ego_edges=p(a["ego_edges"]), perm=p(loader.perm), srcs=p(loader.pool["table"]),
        cursor=p(loader.pool["cursor"]), state=p(loader.state), ws=p(loader._ws),
        slot_ids=p(loader._slot_ids), labels=p(loader.labels), ids=p(loader.ids), M=M, S=S,
        n_cap=static.n_cap, e_cap=static.e_cap, ego_n_cap=int(caps[0]), ego_e_cap=int(caps[1]),
        o_rowptr=o[0], o_col=o[1], o_gptr=o[2], o_dims=o[3], o_x=o[4],
        blob_bytes=static.blob.numel(), B=int(static.B), F=ds.num_features, T=ds.num_tasks,
        D=ds.num_graphs)


class DeviceLoader:
    """Shuffled batches of a DeviceDataset collated on the device, one step
    ahead of a replayed step over ``static`` (csrc/collate.hip).

    ``pool`` is a ring of three blobs in ``static``'s layout (one allocation),
    shaped like ``StaticBatch.pool(...)``: ``static.load_next(loader.pool, pf)``
    and ``EgoPrefetch(static, loader.pool)`` consume it unchanged.  In step t,
    load_next reads slot t % 3, the ego prefetch reads slot (t + 1) % 3 and
    ``collate_ahead()`` — enqueued after load_next — builds batch t + 2 into
    slot (t + 2) % 3, the slot neither of them touches.

    Batch sequence: M molecules -- the whole dataset, or the subset
    ``indices`` (molecule ids, repeats allowed) -- in S = M // B steps per
    epoch (S >= 3); global batch j holds
    molecules ``epoch_permutation(j // S)[(j % S) * B : + B]``.  The M % B
    molecules at the end of each permutation are dropped that epoch (the
    reference trains on the partial batch; a captured graph has a fixed B).
    The permutations of even and odd epochs sit in two device buffers;
    ``begin_epoch(e)`` uploads epoch e + 1's.  If it is never called the two
    buffers repeat.

    ``labels`` [B, T] / ``ids`` [B]: the labels and molecule ids of the batch
    the step is training on, valid for work enqueued after ``collate_ahead()``
    (``ride(prefetch)`` moves that call onto the ego prefetch's queue, off the
    step's critical path, for steps that do not read the labels).
    A batch above the capacities of ``static`` is not written (its slot keeps
    the earlier batch, labels and ids follow the slot) and counted:
    ``error()``."""

    def __init__(self, dataset, static, seed=0, shuffle=True, indices=None):
        ds = dataset
        caps, dev = _loader_checks("DeviceLoader", ds, static)
        self.indices = None if indices is None else _subset_ids(ds, indices, "DeviceLoader")
        B, M = int(static.B), ds.num_graphs if indices is None else len(self.indices)
        S = M // B
        if S < 3:
            raise _lib.ScgibError(f"DeviceLoader: {M} molecules give {S} batches of {B} per epoch; "
                                  "the three-slot ring needs at least 3")
        self.dataset, self.static = ds, static
        self.seed, self.shuffle = int(seed), bool(shuffle)
        self.B, self.M, self.steps_per_epoch = B, M, S
        self.ring, self.slots, self.pool = _loader_ring(static, dev)
        i32 = torch.int32
        T = ds.num_tasks
        self.labels = torch.zeros(B, T, dtype=torch.float32, device=dev)
        self.ids = torch.zeros(B, dtype=i32, device=dev)
        self.state = torch.zeros(4, dtype=i32, device=dev)  # position in [0, 2S), overflow count
        self.perm = torch.zeros(2 * M, dtype=i32, device=dev)
        # scgib_collate_ws_words(B): header, graph_ptr, edge offsets, the molecules' 64-bit bases
        self._ws = torch.zeros((8 + 2 * (B + 1) + 1) // 2 * 2 + 4 * B, dtype=i32, device=dev)
        self._slot_ids = torch.zeros(3 * B, dtype=i32, device=dev)
        self._pinned = [None, None]  # begin_epoch's host staging and its copy's event
        self._desc = _collate_desc(ds, static, caps, self, M, S)

    # ----- the batch sequence (host side) ---------------------------------
    def epoch_permutation(self, e):
        """perm_e on the host (int64 numpy): drawn from a CPU generator seeded
        by (seed, e); the identity without shuffling.  Over a subset
        (``indices``) the same permutation of its positions, as molecule ids."""
        if not self.shuffle:
            perm = np.arange(self.M, dtype=np.int64)
        else:
            perm = np.random.default_rng([self.seed, int(e)]).permutation(self.M).astype(np.int64)
        return perm if self.indices is None else self.indices[perm]

    def batch_ids(self, j):
        """Molecule ids of global batch j (begin_epoch called every epoch)."""
        S, B = self.steps_per_epoch, self.B
        return self.epoch_permutation(j // S)[(j % S) * B:(j % S) * B + B]

    def _perm_slice(self, e):
        return self.perm[(e % 2) * self.M:(e % 2 + 1) * self.M]

    # ----- device side -------------------------------------------------------
    def _launch(self, ahead, slot, advance, labels):
        d = ctypes.byref(self._desc)
        _lib.call("scgib_collate_plan", d, ahead, slot, advance, _stream())
        _lib.call("scgib_collate_fill", d, labels, _stream())

    def prime(self):
        """Eager, before the capture: perm_0 and perm_1, batches 0 and 1 into
        slots 0 and 1 (slot 2 holds batch 0 until step 0 builds batch 2 over
        it), cursors reset."""
        if self.ring.device.type != "cuda":
            raise _lib.ScgibError("DeviceLoader.prime needs a HIP device (no CPU fallback)")
        for e in (0, 1):
            self._perm_slice(e).copy_(torch.from_numpy(self.epoch_permutation(e).astype(np.int32)))
        self.pool["cursor"].zero_()
        self.state.zero_()
        for ahead, slot in ((0, 2), (0, 0), (1, 1)):
            self._launch(ahead, slot, 0, 0)
        if self.error():
            raise _lib.ScgibError("DeviceLoader.prime: the first batches do not fit the "
                                  "capacities of the static batch")

    def collate_ahead(self):
        """Once per step after load_next, on a stream ordered after it
        (capturable; no host synchronisation): batch t + 2 into slot
        (t + 2) % 3, batch t's labels and ids into ``labels`` / ``ids``, and the
        position moves on."""
        self._launch(2, -1, 1, 1)

    def ride(self, prefetch):
        """Move collate_ahead onto the ego prefetch's queue: from now on every
        ``prefetch.prefetch()`` — the encoder pair's side tail, in the ego
        chain's idle stretch through the loss section — is followed by
        collate_ahead() on the same stream, which the backward joins back
        before the next load_next.  The step then makes no collate_ahead call
        of its own, and ``labels`` / ``ids`` are valid only after that join
        (a loss that reads the labels wants collate_ahead() on the main queue
        instead).  Call it after ``prefetch.prime()``."""
        if prefetch.pool is not self.pool:
            raise _lib.ScgibError("DeviceLoader.ride: the EgoPrefetch was made for another pool")
        build = prefetch.prefetch

        def prefetch_then_collate():
            build()
            self.collate_ahead()

        prefetch.prefetch = prefetch_then_collate

    def begin_epoch(self, e):
        """On the step's stream before the first step of epoch e >= 1 is
        enqueued: perm_{e+1} into buffer (e + 1) % 2, whose last reader (the
        collation of epoch e - 1's last batch) ran two steps earlier."""
        e = int(e)
        buf = (e + 1) % 2
        host = torch.from_numpy(self.epoch_permutation(e + 1).astype(np.int32))
        if self._pinned[buf] is not None:
            self._pinned[buf][1].synchronize()  # the staging's earlier copy has left it
            self._pinned[buf][0].copy_(host)
        else:
            self._pinned[buf] = [host.pin_memory(), torch.cuda.Event()]
        self._perm_slice(e + 1).copy_(self._pinned[buf][0], non_blocking=True)
        self._pinned[buf][1].record()

    def error(self):
        """How many batches did not fit the capacities and were skipped
        (sticky) — a device read, for checks outside the loop."""
        return int(self.state[1].item())


class DeviceEvalLoader:
    """The molecules of a subset of a DeviceDataset in order, every one exactly
    once per pass, collated on the device one step ahead of a replayed
    evaluation step over ``static`` (csrc/collate.hip).

    ``pool`` / ``labels`` / ``ids`` / ``error()`` as on DeviceLoader:
    ``static.load_next(evl.pool, pf)`` and ``EgoPrefetch(static, evl.pool)``
    consume the ring unchanged, and ``labels`` / ``ids`` describe the batch the
    step scores for work enqueued after ``collate_ahead()`` on its stream.

    Batch sequence: ``steps = ceil(M / B)`` (any steps >= 1); batch j holds
    ``indices[j * B : min((j + 1) * B, M)]`` in order and step t, counted from
    ``prime()``, scores batch t % steps.  The last batch is filled up to B with
    copies of the subset's smallest molecule (``sequential_fill_id``), so the
    step sees an ordinary batch; fill rows have ``ids`` -1 and a label row of
    NaN, which ops.task_loss and EvalBuffer ignore.  After ``steps`` steps
    the position is 0 again and the next pass needs no host call.

    A batch above the capacities of ``static`` is not written and counted
    (``error()``); its slot's ids become -1, so the step that scores the slot's
    stale bytes reports only NaN-labelled rows.  ``static`` sized by
    ``dataset.capacities(B, "sequential", indices=...)`` cannot overflow.

    The list, its length, the fill id and the position live in device memory:
    ``set_subset(indices)`` (up to ``max_len`` ids, default the first list's
    length) points a graph captured over the loader at another subset."""

    def __init__(self, dataset, static, indices=None, max_len=None):
        ds = dataset
        caps, dev = _loader_checks("DeviceEvalLoader", ds, static)
        ids = _subset_ids(ds, indices, "DeviceEvalLoader")
        self.max_len = len(ids) if max_len is None else int(max_len)
        if len(ids) > self.max_len:
            raise _lib.ScgibError(f"DeviceEvalLoader: {len(ids)} indices above max_len "
                                  f"{self.max_len}")
        self.dataset, self.static = ds, static
        B = self.B = int(static.B)
        self.ring, self.slots, self.pool = _loader_ring(static, dev)
        i32 = torch.int32
        self.labels = torch.zeros(B, ds.num_tasks, dtype=torch.float32, device=dev)
        self.ids = torch.zeros(B, dtype=i32, device=dev)
        # position in [0, steps), overflow count, list length, fill molecule id
        self.state = torch.zeros(4, dtype=i32, device=dev)
        self.perm = torch.zeros(self.max_len, dtype=i32, device=dev)  # the index list
        self._ws = torch.zeros((8 + 2 * (B + 1) + 1) // 2 * 2 + 4 * B, dtype=i32, device=dev)
        self._slot_ids = torch.zeros(3 * B, dtype=i32, device=dev)
        self._desc = _collate_desc(ds, static, caps, self, self.max_len, 1)
        self._set_host(ids)

    def _set_host(self, ids):
        self.indices, self.M = ids, len(ids)
        self.steps = -(-self.M // self.B)
        self.fill_id = sequential_fill_id(self.dataset, ids)

    def batch_ids(self, j):
        """(molecule ids collated into batch j % steps, fill included; the ids
        the loader reports for it, -1 at the fill rows)."""
        rows, marked = sequential_ids(self.dataset, self.indices, self.B)
        return rows[j % self.steps], marked[j % self.steps]

    def _launch(self, ahead, slot, advance, labels):
        d = ctypes.byref(self._desc)
        _lib.call("scgib_collate_seq_plan", d, ahead, slot, advance, _stream())
        _lib.call("scgib_collate_seq_fill", d, labels, _stream())

    def set_subset(self, indices):
        """Eager, on the current stream, between passes: the index list, its
        length and fill id, position 0, cursor 0 and batches 0, 1, 2 (mod
        steps) into slots 0, 1, 2.  The caller re-primes its EgoPrefetch; a
        graph captured over the loader then scores the new subset.  The
        overflow count is kept; a primed batch that does not fit raises."""
        ids = _subset_ids(self.dataset, indices, "DeviceEvalLoader.set_subset")
        if len(ids) > self.max_len:
            raise _lib.ScgibError(f"DeviceEvalLoader.set_subset: {len(ids)} indices above "
                                  f"max_len {self.max_len}")
        if self.ring.device.type != "cuda":
            raise _lib.ScgibError("DeviceEvalLoader needs a HIP device (no CPU fallback)")
        self._set_host(ids)
        before = self.error()
        self.perm[:self.M].copy_(torch.from_numpy(ids.astype(np.int32)))
        self.state.copy_(torch.tensor([0, before, self.M, self.fill_id], dtype=torch.int32))
        self.pool["cursor"].zero_()
        for slot in (0, 1, 2):
            self._launch(slot, slot, 0, 0)
        if self.error() != before:
            raise _lib.ScgibError("DeviceEvalLoader: the first batches do not fit the "
                                  "capacities of the static batch")

    def prime(self):
        """Eager, before the capture: ``set_subset`` of the current indices
        with the overflow count reset."""
        if self.ring.device.type != "cuda":
            raise _lib.ScgibError("DeviceEvalLoader.prime needs a HIP device (no CPU fallback)")
        self.state.zero_()
        self.set_subset(self.indices)

    def collate_ahead(self):
        """Once per step after load_next, on a stream ordered after it
        (capturable; no host synchronisation): batch (t + 2) % steps into slot
        (cursor + 1) % 3, batch t's labels and ids into ``labels`` / ``ids``,
        and the position moves on (cyclic)."""
        self._launch(2, -1, 1, 1)

    def error(self):
        """How many batches did not fit the capacities (sticky) — a device
        read, for checks outside the loop."""
        return int(self.state[1].item())
