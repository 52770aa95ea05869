"""CPU tests of the edge-list ingest: from_coo / from_pyg_batch / as_graph_batch
on the host route against collate_pyg, the errors it names, and the new
entry points in the binding table and the header.  No GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from ingest_util import Duck, handmade, same_graph, tensors

ENTRY_POINTS = ("scgib_ingest_workspace_bytes", "scgib_ingest_status_words", "scgib_ingest_csr",
                "scgib_ingest_blob")


def _cases(pkg):
    return {"handmade": handmade(), "synth7": pkg.synth.molecules(7, "qm9", seed=3),
            "one": pkg.synth.molecules(1, "molpcba", seed=1)}


@pytest.mark.parametrize("name", ["handmade", "synth7", "one"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_from_coo_matches_collate_pyg(pkg, name, dtype):
    G = pkg.graph
    mols = _cases(pkg)[name]
    ref, kept = G.collate_pyg(mols)
    assert len(kept) == len(mols)
    src, dst, gptr, x = tensors(mols, dtype=dtype)
    g = G.from_coo(src, dst, gptr, x.shape[0], x=x)
    assert isinstance(g, G.GraphBatch) and same_graph(g, ref)
    assert np.array_equal(g.batch_num_nodes_host(), ref.batch_num_nodes_host())
    assert torch.equal(g.batch_num_edges(), ref.batch_num_edges())
    # the per-graph counts in place of graph_ptr, and a shuffled edge order
    perm = torch.randperm(src.numel(), generator=torch.Generator().manual_seed(0))
    g2 = G.from_coo(src[perm], dst[perm], None, x.shape[0], x=x,
                    batch_num_nodes=gptr[1:] - gptr[:-1])
    assert same_graph(g2, ref)


def test_from_pyg_batch_matches_collate_pyg(pkg):
    G = pkg.graph
    mols = handmade()
    ref, _ = G.collate_pyg(mols)
    src, dst, gptr, x = tensors(mols)
    batch = SimpleNamespace(edge_index=torch.stack([src, dst]), ptr=gptr.to(torch.int64), x=x)
    g = G.from_pyg_batch(batch)
    assert same_graph(g, ref) and g.ndata["x"] is x


def test_as_graph_batch(pkg):
    G = pkg.graph
    ref, _ = G.collate_pyg(handmade())
    assert G.as_graph_batch(ref) is ref
    duck = Duck.of(ref)
    g = G.as_graph_batch(duck)
    assert same_graph(g, ref) and g.ndata["x"] is ref.ndata["x"]
    assert G.as_graph_batch(duck) is g  # cached on the object: ingested once
    with pytest.raises(TypeError):
        G.as_graph_batch(object())


def _raises(pkg, bit, *args, **kw):
    with pytest.raises(pkg._lib.ScgibError) as ei:
        pkg.graph.from_coo(*args, **kw)
    msg = str(ei.value)
    assert f"{bit}: {pkg._lib.INGEST_ERRORS[bit]}" in msg, msg
    return msg


def test_errors_name_their_bit(pkg):
    src, dst, gptr, x = tensors(handmade())
    n = x.shape[0]
    t = lambda *v: torch.tensor(v, dtype=torch.int64)  # noqa: E731
    _raises(pkg, 1, torch.cat([src, t(n)]), torch.cat([dst, t(0)]), gptr, n)       # index == n
    _raises(pkg, 1, torch.cat([src, t(-1)]), torch.cat([dst, t(0)]), gptr, n)      # negative
    _raises(pkg, 1, torch.cat([src, t(0)]), torch.cat([dst, t(5)]), gptr, n)       # leaves its graph
    big = torch.tensor([0, 513], dtype=torch.int32)
    _raises(pkg, 2, t(0), t(512), big, 513)                                          # 513 atoms
    bad = gptr.clone()
    bad[1], bad[2] = gptr[2], gptr[1]
    _raises(pkg, 64, src, dst, bad, n)                                               # not monotone
    _raises(pkg, 64, src, dst, gptr, n + 1)                                          # does not end at n
    # a molecule whose last atom is isolated: only under the skip rule
    s2, d2, g2 = t(0, 3), t(1, 4), torch.tensor([0, 3, 5], dtype=torch.int32)
    _raises(pkg, 8, s2, d2, g2, 5, skip_rule=True)
    assert pkg.graph.from_coo(s2, d2, g2, 5).num_edges() == 4
    # verify mode: one direction missing; a duplicate
    ref, _ = pkg.graph.collate_pyg(handmade())
    es, ed = ref.edges()
    pkg.graph.from_coo(es, ed, gptr, n, bidirect=False)
    keep = torch.ones(es.numel(), dtype=torch.bool)
    keep[int(torch.nonzero(es != ed)[0])] = False
    _raises(pkg, 16, es[keep], ed[keep], gptr, n, bidirect=False)
    _raises(pkg, 16, torch.cat([es, es[:1]]), torch.cat([ed, ed[:1]]), gptr, n, bidirect=False)


def test_static_ingest_refuses_k2_and_cpu(pkg):
    G = pkg.graph
    st = G.StaticBatch(3, 16, 32, 5, 8, (64, 256, 4), "cpu", k=2)
    src, dst, gptr, x = tensors(handmade())
    with pytest.raises(pkg._lib.ScgibError, match="k = 1"):
        st.ingest(src, dst, gptr, x)
    st1 = G.StaticBatch(3, 16, 32, 5, 8, (64, 256, 4), "cpu", k=1)
    with pytest.raises(pkg._lib.ScgibError, match="HIP device"):
        st1.ingest(src, dst, gptr, x)
    assert st1.ingest_error() == 0


def test_entry_points_bound_and_declared(pkg):
    L = pkg._lib
    header = open(os.path.join(ROOT, "include", "scgib.h")).read()
    lib = L.load()
    for name in ENTRY_POINTS:
        assert name in L.SIGNATURES, name
        assert re.search(rf"^\s*(?:int|int64_t)\s+{name}\(", header, re.M), name
        assert getattr(lib, name) is not None
    for bit, macro in ((1, "ERANGE"), (2, "EGRAPH"), (4, "ECAPACITY"), (8, "ELASTNODE"),
                       (16, "ESYMMETRY"), (32, "ESMALL"), (64, "EGPTR")):
        assert re.search(rf"#define SCGIB_INGEST_{macro} {bit}\b", header), macro
        assert bit in L.INGEST_ERRORS
    # argument errors are refused before any launch
    assert lib.scgib_ingest_csr(None, None, 8, 0, None, 1, 1, 512, 1, 0, None, 1, None, None, 1,
                                None, None) == -1
    assert lib.scgib_ingest_blob(None, None) == -1
    assert lib.scgib_ingest_workspace_bytes(1000, 512) >= 1000 * 64
    assert lib.scgib_ingest_workspace_bytes(1000, 513) == 0
    assert lib.scgib_ingest_status_words(3) == 16 + 4
    # the descriptor mirrors the header's struct: 9 pointers, 12 int64, 8 int32
    assert __import__("ctypes").sizeof(L.IngestDesc) == 9 * 8 + 12 * 8 + 8 * 4

