"""The device-side edge-list ingest on the MI355X (csrc/ingest.hip, DESIGN.md
§18): from_coo against collate_pyg, verify mode, refusals, StaticBatch.ingest
against StaticBatch.pad, a captured step fed from staging buffers, and the
model boundary's duck-typed graphs.  Everything is compared bit for bit."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ingest_util import Duck, handmade, path_molecule, same_graph, tensors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _raises(pkg, bit, fn, *args, **kw):
    with pytest.raises(pkg._lib.ScgibError) as ei:
        fn(*args, **kw)
    assert f"{bit}: {pkg._lib.INGEST_ERRORS[bit]}" in str(ei.value), str(ei.value)


# ---------------------------------------------------------------------------
# 1. from_coo against collate_pyg
# ---------------------------------------------------------------------------
def _molecules(pkg, name):
    if name == "handmade":
        return handmade()
    if name == "path512":  # the last bitmap word, among small molecules
        small = pkg.synth.molecules(4, "qm9", seed=2)
        return small[:2] + [path_molecule(512, 11)] + small[2:]
    if name == "rows70k":  # ~275 scan blocks of 256 rows
        return pkg.synth.molecules(3900, "qm9", seed=4)
    return pkg.synth.molecules(int(name[1:]), "qm9", seed=int(name[1:]))


@pytest.mark.parametrize("name", ["handmade", "B1", "B7", "B64", "B300", "rows70k", "path512"])
def test_from_coo_bitwise(pkg, dev, name):
    G = pkg.graph
    mols = _molecules(pkg, name)
    ref, kept = G.collate_pyg(mols)
    assert len(kept) == len(mols)
    if name == "rows70k":
        assert ref.num_nodes() > 256 * 256
    perm = torch.randperm(sum(ei.shape[1] for ei, _ in mols),
                          generator=torch.Generator().manual_seed(1)).to(dev)
    for dtype in (torch.int64, torch.int32):
        src, dst, gptr, x = tensors(mols, dev, dtype)
        runs = [G.from_coo(src, dst, gptr, x.shape[0], x=x) for _ in range(2)]
        runs.append(G.from_coo(src[perm], dst[perm], gptr, x.shape[0], x=x))
        for g in runs:
            assert g.device.type == "cuda" and same_graph(g, ref)
            assert g.num_edges() == ref.num_edges() and g.col.shape[0] == ref.num_edges()
            assert g.max_graph_nodes == ref.max_graph_nodes and g.components_closed
            assert np.array_equal(g.batch_num_nodes_host(), ref.batch_num_nodes_host())
            assert g.ego_k1 == G._k1_bounds(ref)
        assert torch.equal(runs[0].col, runs[1].col) and torch.equal(runs[0].rowptr, runs[1].rowptr)
    batch = SimpleNamespace(edge_index=torch.stack([src, dst]), ptr=gptr, x=x)
    assert same_graph(G.from_pyg_batch(batch), ref)


def test_from_coo_sizes_the_ego_batch_without_a_read(pkg, dev, monkeypatch):
    """egonet_batch(g, 1) on an ingested batch: the fast builder, and the same
    ego batch as on the host-collated one."""
    G = pkg.graph
    mols = pkg.synth.molecules(7, "qm9", seed=7)
    ref = G.collate_pyg(mols)[0].to(dev)
    src, dst, gptr, x = tensors(mols, dev)
    g = G.from_coo(src, dst, gptr, x.shape[0], x=x)
    names = []
    orig = pkg._lib.call
    monkeypatch.setattr(pkg._lib, "call", lambda n, *a: (names.append(n), orig(n, *a))[1])
    ego, ego_ref = G.egonet_batch(g, 1), G.egonet_batch(ref, 1)
    assert names and all(n.startswith("scgib_egonet_k1_build") for n in names), names
    assert torch.equal(ego.graph_ptr, ego_ref.graph_ptr)
    assert torch.equal(ego.rowptr, ego_ref.rowptr)
    assert torch.equal(ego.ndata["_ID"], ego_ref.ndata["_ID"])
    e = ego_ref.num_edges()
    assert torch.equal(ego.col[:e], ego_ref.col[:e])


# ---------------------------------------------------------------------------
# 2. verify mode
# ---------------------------------------------------------------------------
def test_verify_mode(pkg, dev):
    G = pkg.graph
    gd = G.collate_pyg(pkg.synth.molecules(7, "qm9", seed=5) + handmade_f11())[0].to(dev)
    n = gd.num_nodes()
    es, ed = gd.edges()
    for _ in range(2):
        g = G.from_coo(es, ed, gd.graph_ptr, n, bidirect=False)
        assert same_graph(g, gd)
    ego = G.egonet_batch(gd, 1)  # one graph per node
    e = ego.num_edges()
    s2, d2 = ego.edges()
    g2 = G.from_coo(s2, d2, ego.graph_ptr, ego.num_nodes(), bidirect=False)
    assert torch.equal(g2.rowptr, ego.rowptr) and torch.equal(g2.col, ego.col[:e])
    assert g2.batch_size == n
    g3 = G.as_graph_batch(Duck.of(ego, keys=("_ID",)))
    assert torch.equal(g3.rowptr, ego.rowptr) and g3.ndata["_ID"] is ego.ndata["_ID"]
    # one direction of one edge dropped; one edge given twice
    keep = torch.ones(es.numel(), dtype=torch.bool, device=dev)
    keep[int(torch.nonzero(es != ed)[3])] = False
    _raises(pkg, 16, G.from_coo, es[keep], ed[keep], gd.graph_ptr, n, bidirect=False)
    _raises(pkg, 16, G.from_coo, torch.cat([es, es[5:6]]), torch.cat([ed, ed[5:6]]), gd.graph_ptr,
            n, bidirect=False)
    assert same_graph(G.from_coo(es, ed, gd.graph_ptr, n, bidirect=False), gd)


# ---------------------------------------------------------------------------
# 3. refusals (validation paths: the values are rejected before they index)
# ---------------------------------------------------------------------------
def _bad_inputs(dev):
    src, dst, gptr, x = tensors(handmade(), dev)
    n = x.shape[0]
    t = lambda *v: torch.tensor(v, dtype=torch.int64, device=dev)  # noqa: E731
    swapped = gptr.clone()
    swapped[1], swapped[2] = gptr[2].clone(), gptr[1].clone()
    big = path_molecule(513, 5)
    bs, bd, bg, bx = tensors([big], dev)
    return {
        "index == n": (1, (torch.cat([src, t(n)]), torch.cat([dst, t(0)]), gptr, n), {}),
        "negative index": (1, (torch.cat([src, t(-1)]), torch.cat([dst, t(0)]), gptr, n), {}),
        "edge between molecules": (1, (torch.cat([src, t(0)]), torch.cat([dst, t(5)]), gptr, n), {}),
        "513 atoms": (2, (bs, bd, bg, 513), {}),
        "non-monotone graph_ptr": (64, (src, dst, swapped, n), {}),
        "last atom isolated": (8, (t(0, 3), t(1, 4), torch.tensor([0, 3, 5], dtype=torch.int32,
                                                                 device=dev), 5),
                               {"skip_rule": True}),
    }


@pytest.mark.parametrize("case", ["index == n", "negative index", "edge between molecules",
                                  "513 atoms", "non-monotone graph_ptr", "last atom isolated"])
def test_refusals(pkg, dev, case):
    G = pkg.graph
    valid = []
    for mols in (pkg.synth.molecules(64, "qm9", seed=64), handmade()):
        src, dst, gptr, x = tensors(mols, dev)
        valid.append(((src, dst, gptr, x.shape[0]), G.collate_pyg(mols)[0]))
    for args, ref in valid:  # (the larger batch first: it sizes the workspace the rest reuse)
        assert same_graph(G.from_coo(*args), ref)
    bit, args, kw = _bad_inputs(dev)[case]
    _raises(pkg, bit, G.from_coo, *args, **kw)
    # the same workspace afterwards: the bitmaps were cleared on the error path
    for args, ref in reversed(valid):
        assert same_graph(G.from_coo(*args), ref)


# ---------------------------------------------------------------------------
# 4. StaticBatch.ingest against StaticBatch.pad
# ---------------------------------------------------------------------------
def _static(pkg, dev, hosts, B, feat, n_cap=None, e_cap=None, ego_n=None, k=1):
    caps = pkg.graph.StaticBatch.capacities(hosts, 1, slack=1.1)
    ego = (caps[3][0] if ego_n is None else ego_n, caps[3][1], caps[3][2])
    return pkg.graph.StaticBatch(B, caps[0] if n_cap is None else n_cap,
                                 caps[1] if e_cap is None else e_cap, feat, caps[2], ego, dev, k)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_static_ingest_bitwise(pkg, dev, B):
    """Three batches in a row, the largest first, then the smallest: no stale
    tails; int64 and int32 indices."""
    G = pkg.graph
    sets = [pkg.synth.molecules(B, "qm9", seed=20 + i, mu=m) for i, m in enumerate((24, 6, 18))]
    if B == 3:
        sets.append(handmade_f11())
    hosts = [G.collate_pyg(m)[0] for m in sets]
    static = _static(pkg, dev, hosts, B, 11)
    for i, (mols, host) in enumerate(zip(sets, hosts)):
        src, dst, gptr, x = tensors(mols, dev, torch.int32 if i % 2 else torch.int64)
        static.ingest(src, dst, gptr, x)
        torch.cuda.synchronize()
        assert torch.equal(static.blob, static.pad(host)["blob"]), f"batch {i}"
    assert static.ingest_error() == 0 and static.ego_error() == 0
    ego, ego_ref = G.egonet_batch(static.graph, 1), G.egonet_batch(hosts[-1].to(dev), 1)
    n = hosts[-1].num_nodes()
    assert torch.equal(ego.graph_ptr[:n + 1], ego_ref.graph_ptr)


def handmade_f11():
    return [(ei, np.pad(x, ((0, 0), (0, 11 - x.shape[1])))) for ei, x in handmade()]


@pytest.mark.parametrize("what", ["n_cap", "e_cap", "ego nodes"])
def test_static_ingest_overflow_leaves_the_blob(pkg, dev, what):
    G = pkg.graph
    small, large = pkg.synth.molecules(3, "qm9", seed=31, mu=8), pkg.synth.molecules(3, "qm9", seed=32)
    hs, hl = G.collate_pyg(small)[0], G.collate_pyg(large)[0]
    assert hl.num_nodes() > hs.num_nodes() + 3
    bn = G.ego_bounds(hl, 1)[0]
    tight = {"n_cap": {"n_cap": hl.num_nodes() - 1}, "e_cap": {"e_cap": hl.num_edges() - 1},
             "ego nodes": {"ego_n": bn - 1}}[what]
    static = _static(pkg, dev, [hs, hl], 3, 11, **tight)
    with pytest.raises(pkg._lib.ScgibError):
        static.pad(hl)  # the host route refuses the same batch
    static.ingest(*tensors(small, dev))
    torch.cuda.synchronize()
    before = static.blob.clone()
    assert torch.equal(before, static.pad(hs)["blob"]) and static.ingest_error() == 0
    static.ingest(*tensors(large, dev))
    torch.cuda.synchronize()
    assert torch.equal(static.blob, before)
    assert static.ingest_error() == 4
    static.ingest(*tensors(small, dev))
    assert static.ingest_error() == 4  # sticky until reset
    assert torch.equal(static.blob, before)
    static.reset_ingest_error()
    assert static.ingest_error() == 0


def test_static_ingest_small_molecule_and_k2(pkg, dev):
    G = pkg.graph
    mols = pkg.synth.molecules(3, "qm9", seed=33)
    hosts = [G.collate_pyg(mols)[0]]
    static = _static(pkg, dev, hosts, 3, 11)
    static.ingest(*tensors(mols, dev))
    torch.cuda.synchronize()
    before = static.blob.clone()
    one = (np.array([[0], [0]], np.int64), mols[1][1][:1])  # one atom with a self-loop
    static.ingest(*tensors([mols[0], one, mols[2]], dev))
    assert static.ingest_error() == 32 and torch.equal(static.blob, before)
    k2 = _static(pkg, dev, hosts, 3, 11, k=2)
    with pytest.raises(pkg._lib.ScgibError, match="k = 1"):
        k2.ingest(*tensors(mols, dev))


# ---------------------------------------------------------------------------
# 5. a captured step fed from staging buffers
# ---------------------------------------------------------------------------
def _captured_run(pkg, dev, sets, hosts, feed, B=3, k=1):
    """Mainmodel_continue (GIN-64x5), Adam in the graph: one eager step on
    batch 0, the capture, then a replay per further batch.  feed "ingest":
    static.ingest(staging..., counts), the staging tensors refilled between
    replays; "load": static.load of a staging blob refilled with
    static.pad(...) of the same batches."""
    from test_gpu_graph_split import _state
    from test_gpu_trajectory import _pretrain_model
    static = _static(pkg, dev, hosts, B, 11)
    model = _pretrain_model(pkg, 11, k, B, dev)
    opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
    pkg.ops.seed_noise(dev, 4242)
    one = torch.ones((), device=dev)
    flats = [tensors(m, dev) for m in sets]
    e_max = max(f[0].numel() for f in flats)
    stage = SimpleNamespace(src=torch.zeros(e_max, dtype=torch.int64, device=dev),
                            dst=torch.zeros(e_max, dtype=torch.int64, device=dev),
                            gptr=torch.zeros(B + 1, dtype=torch.int32, device=dev),
                            x=torch.zeros(static.n_cap, 11, device=dev),
                            counts=torch.zeros(2, dtype=torch.int32, device=dev),
                            blob={"blob": torch.zeros_like(static.blob)})

    def refill(t):
        if feed == "load":
            stage.blob["blob"].copy_(static.pad(hosts[t])["blob"])
            return
        src, dst, gptr, x = flats[t]
        stage.src.fill_(-7)  # stale entries past the count are never read
        stage.src[:src.numel()].copy_(src)
        stage.dst[:dst.numel()].copy_(dst)
        stage.gptr.copy_(gptr)
        stage.x.fill_(3.0)
        stage.x[:x.shape[0]].copy_(x)
        stage.counts.copy_(torch.tensor([x.shape[0], src.numel()], dtype=torch.int32))

    def body():
        if feed == "load":
            static.load(stage.blob)
        else:
            static.ingest(stage.src, stage.dst, stage.gptr, stage.x, stage.counts)
        _, kl, con, rec = model(static.graph, static.x, None, None, None, 1, None, k, dev, B)
        torch.autograd.backward((kl, rec, con), (one, one, one))
        opt.step()
        return torch.stack([kl.detach(), rec.detach(), con.detach()])

    losses = []
    refill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.zero_grad(set_to_none=True)
        losses.append(body().clone())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    refill(1)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        out = body()
    for t in range(1, len(sets)):
        refill(t)
        graph.replay()
        torch.cuda.synchronize()
        losses.append(out.clone())
        assert torch.equal(static.blob, static.pad(hosts[t])["blob"])
    assert static.ego_error() == 0 and static.ingest_error() == 0
    return torch.stack(losses), _state(model, opt)


def test_captured_step_fed_by_ingest(pkg, dev):
    from test_gpu_graph_split import _assert_bitwise
    sets = [[(ei, F.normalize(torch.from_numpy(x)).numpy()) for ei, x in
             pkg.synth.molecules(3, "qm9", seed=40 + i)] for i in range(4)]
    hosts = [pkg.graph.collate_pyg(m)[0] for m in sets]
    ref_losses, ref_state = _captured_run(pkg, dev, sets, hosts, "load")
    losses, state = _captured_run(pkg, dev, sets, hosts, "ingest")
    assert torch.isfinite(ref_losses).all()
    assert torch.equal(losses, ref_losses), (losses, ref_losses)
    _assert_bitwise(state, ref_state)


# ---------------------------------------------------------------------------
# 6. the model boundary
# ---------------------------------------------------------------------------
def _models(pkg, dev, f_in, B):
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=B, gin_layers=4, task="graph_classification",
                           dataset="ogbg-molpcba", device=dev)
    torch.manual_seed(5)
    inner = pkg.models.Mainmodel(args, f_in, 64, 4, 4, 1, "GIN")
    pre = pkg.models.Mainmodel_continue(args, f_in, 64, 4, 4, 1, 2, inner, "GIN")
    ft = pkg.models.Mainmodel_finetuning(args, f_in, 64, 4, 4, 1, 2, copy.deepcopy(pre), "GIN")
    return pre.to(dev).train(), ft.to(dev).train()


def _run(model, call):
    model.zero_grad(set_to_none=True)
    outs = [o for o in call(model) if torch.is_tensor(o)]
    sum(o.sum() for o in outs).backward()
    torch.cuda.synchronize()
    return ([o.detach().clone() for o in outs],
            {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})


@pytest.mark.parametrize("ego_arg", ["device-built", "duck ego batch"])
def test_models_take_duck_graphs(pkg, dev, ego_arg, monkeypatch):
    G = pkg.graph
    B = 9
    mols = pkg.synth.molecules(B, "molpcba", seed=11)
    g = G.collate_pyg(mols)[0].to(dev)
    x = F.normalize(g.ndata["x"].float())
    n = g.num_nodes()
    gen = torch.Generator().manual_seed(3)
    noise = (torch.rand(n, generator=gen).to(dev), torch.rand(n, 64, generator=gen).to(dev))
    pre, ft = _models(pkg, dev, x.shape[1], B)
    ego = x_subs = None
    if ego_arg != "device-built":
        ego = G.egonet_batch(g, 1)
        x_subs = x.index_select(0, ego.ndata["_ID"])
    names = []
    orig = pkg._lib.call
    monkeypatch.setattr(pkg._lib, "call", lambda nm, *a: (names.append(nm), orig(nm, *a))[1])

    def calls(bg, be):
        return (lambda m: m(bg, x, be, None, x_subs, 1, None, 1, dev, B, noise=noise),
                lambda m: m(bg, x, be, x_subs, 1, None, 1, dev, B, noise=noise))

    ref = [_run(m, c) for m, c in zip((pre, ft), calls(g, ego))]
    assert not [nm for nm in names if "ingest" in nm]  # a GraphBatch is never ingested
    duck_g = Duck.of(g)
    duck_e = None if ego is None else Duck.of(ego, keys=("_ID",))
    got = [_run(m, c) for m, c in zip((pre, ft), calls(duck_g, duck_e))]
    # each duck object was ingested once, then served from its cache
    assert names.count("scgib_ingest_csr") == (1 if ego is None else 2)
    for (ro, rg), (go, gg) in zip(ref, got):
        assert len(ro) == len(go) and all(torch.equal(a, b) for a, b in zip(ro, go))
        assert rg.keys() == gg.keys() and rg
        assert not [k for k in rg if not torch.equal(rg[k], gg[k])]
