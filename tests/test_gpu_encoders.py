"""The GCN / GraphSAGE encoders on the fused graph-convolution layer
(csrc/conv_layer.hip) against an fp64 restatement of DGL 1.1.0's
GraphConv(norm='both') and SAGEConv('mean'), written here from the formulas
(index_add over the edge list):

  agg[v] = c_dst[v] * sum_{u -> v} c_src[u] x[u]
  out[v] = act(agg[v] Wn + x[v] Ws + b)

Tolerances are tests/test_gpu_parity.py's: activations rel_err < 1e-4, each
gradient tensor rel_l2 < 1e-3, losses within 1e-4.  Where a ReLU sits between
the compared quantity and a parameter, the fp64 side follows the kernels' own
decision at pre-activations within 1e-5 of zero (oracle.scgib_ref._relu, as
the GIN parity tests do): there two correct evaluations may decide either way.
"""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import big_graphs as BG
from conftest import check_grads_model, rel_err, rel_l2
from oracle import egonet
from oracle import scgib_ref as R

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4
ACT_TOL = 1e-4
GRAD_TOL = 1e-3
TIE = 1e-5
SHAPES = [(32, 128), (128, 128), (128, 64), (32, 64), (64, 64)]
MODES = ["gcn", "mean"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------
def ref_norm(src, dst, n, mode):
    din = torch.bincount(dst, minlength=n).clamp(min=1).double()
    dout = torch.bincount(src, minlength=n).clamp(min=1).double()
    if mode == "gcn":
        return dout.pow(-0.5), din.pow(-0.5)
    return torch.ones(n, dtype=torch.float64), 1.0 / din


def ref_layer(x, src, dst, wn, ws, b, mode, relu, mask=None):
    """One layer in fp64; wn [in, out] for 'gcn', wn / ws [out, in] for 'mean'."""
    n = x.shape[0]
    cs, cd = ref_norm(src, dst, n, mode)
    agg = cd[:, None] * torch.zeros_like(x).index_add(0, dst, cs[src, None] * x[src])
    z = agg @ (wn if mode == "gcn" else wn.t())
    if ws is not None:
        z = z + x @ ws.t()
    if b is not None:
        z = z + b
    return R._relu(z, mask, TIE) if relu else z


def make_weights(mode, d_in, d_out, seed):
    gen = torch.Generator().manual_seed(seed)
    sc = 1.0 / d_in ** 0.5
    shape = (d_in, d_out) if mode == "gcn" else (d_out, d_in)
    wn = torch.randn(shape, generator=gen) * sc
    ws = torch.randn(shape, generator=gen) * sc if mode == "mean" else None
    b = torch.randn(d_out, generator=gen) * 0.3
    return wn, ws, b


def run_layer(pkg, g, x, wn, ws, b, mode, relu, gout):
    """The HIP layer forward + backward; returns detached CPU results."""
    dev = g.rowptr.device
    leaves = [t.to(dev).requires_grad_(True) if t is not None else None for t in (x, wn, ws, b)]
    out = pkg.ops.conv_layer(leaves[0], g, leaves[1], leaves[2], leaves[3], mode, relu)
    out.backward(gout.to(dev))
    torch.cuda.synchronize()
    return out.detach(), [None if t is None else t.grad for t in leaves]


def check_layer(pkg, dev, gh, mode, d_in, d_out, relu, seed=0):
    g = gh.to(dev)
    n = gh.num_nodes()
    src, dst = gh.edges()
    gen = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(n, d_in, generator=gen)
    gout = torch.randn(n, d_out, generator=gen)
    wn, ws, b = make_weights(mode, d_in, d_out, seed)
    out, grads = run_layer(pkg, g, x, wn, ws, b, mode, relu, gout)
    ref_leaves = [t.double().requires_grad_(True) if t is not None else None
                  for t in (x, wn, ws, b)]
    ref = ref_layer(ref_leaves[0], src, dst, ref_leaves[1], ref_leaves[2], ref_leaves[3], mode,
                    relu, (out > 0).cpu() if relu else None)
    ref.backward(gout.double())
    assert out.shape == (n, d_out)
    assert rel_err(out.cpu(), ref.detach()) < ACT_TOL
    for name, mine, r in zip(("dx", "dWn", "dWs", "db"), grads, ref_leaves):
        if r is None:
            assert mine is None, name
            continue
        assert mine.shape == r.shape, name
        if float(r.grad.abs().max()) == 0.0:  # (an edgeless graph's dWn)
            assert float(mine.abs().max()) == 0.0, name
            continue
        err = rel_l2(mine.cpu(), r.grad)
        assert err < GRAD_TOL, (name, err)
    return out, grads


@pytest.fixture(scope="module")
def mols37(pkg):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(37, "qm9", seed=5))
    assert gh.num_nodes() % 64 != 0 and gh.num_nodes() > 3 * 64  # several tiles, ragged last
    return gh


# ---------------------------------------------------------------------------
# layer level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", MODES)
def test_layer_forward_backward(pkg, dev, mols37, mode, shape, relu):
    check_layer(pkg, dev, mols37, mode, shape[0], shape[1], relu, seed=shape[0] + shape[1])


def _path(n):
    a = np.arange(n - 1)
    return np.concatenate([a, a + 1]), np.concatenate([a + 1, a]), n


def _star(k):
    leaves = np.arange(1, k + 1)
    zeros = np.zeros(k, np.int64)
    return np.concatenate([leaves, zeros]), np.concatenate([zeros, leaves]), k + 1


def _hand_graphs():
    out = {"single": (np.zeros(0, np.int64), np.zeros(0, np.int64), 1)}
    out["path64"] = _path(64)
    out["path65"] = _path(65)
    # node 0 isolated (degree clamp, zero mean), then a path 1-2-3-4
    s, d, _ = _path(4)
    out["isolated_first"] = (s + 1, d + 1, 5)
    # star: 9 leaves <-> centre 0 (in-degree 9: gather rounds of 4 at 5 and 9)
    out["star9"] = _star(9)
    out["star33"] = _star(33)  # in-degree 33: nine gather rounds, the last one of a single edge
    # directed, non-symmetric: v -> v+1, v -> v+3, v -> 2v+5 (mod n), no reverse edges kept
    out["directed"] = BG.directed(70)
    return out


HAND = _hand_graphs()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(HAND))
def test_layer_hand_made_graphs(pkg, dev, name, mode):
    src, dst, n = HAND[name]
    gh = pkg.graph.GraphBatch.from_edges(src, dst, n, symmetric_hint=False)
    if name == "directed":
        din = np.bincount(dst, minlength=n)
        dout = np.bincount(src, minlength=n)
        assert (din != dout).mean() > 0.5  # a backward over the wrong CSR cannot pass
    # the reference's edge list is the input's, not read back from the CSR under test
    es, ed = gh.edges()
    assert sorted(zip(es.tolist(), ed.tolist())) == sorted(zip(src.tolist(), dst.tolist()))
    out, _ = check_layer(pkg, dev, gh, mode, 32, 64, True, seed=7)
    if name == "directed":
        check_layer(pkg, dev, gh, mode, 128, 64, False, seed=8)
    if name == "isolated_first" and mode == "mean":
        # no in-edges: zero neighbour term, the row is relu(x Ws^T + b)
        gen = torch.Generator().manual_seed(107)
        x = torch.randn(n, 32, generator=gen)
        wn, ws, b = make_weights(mode, 32, 64, 7)
        want = F.relu(x[0].double() @ ws.double().t() + b.double())
        assert rel_err(out[0].cpu(), want) < ACT_TOL


@pytest.fixture(scope="module")
def big(pkg):
    """name -> host graph of BG.big_directed(name), built once for the module."""
    cache = {}

    def get(name):
        if name not in cache:
            src, dst, n = BG.big_directed(name)
            gh = pkg.graph.GraphBatch.from_edges(src, dst, n, symmetric_hint=False)
            assert BG.degree_asymmetry(src, dst, n) > 0.5  # a backward over the wrong CSR cannot pass
            es, ed = gh.edges()  # the reference's edge list is the input's
            assert sorted(zip(es.tolist(), ed.tolist())) == sorted(zip(src.tolist(), dst.tolist()))
            cache[name] = gh
        return cache[name]
    return get


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(BG.BIG_SIZES))
def test_layer_past_256_tiles(pkg, dev, big, name, mode, shape):
    """conv_wgrad_k runs at most 256 workgroups.  big256: one full tile each,
    the boundary; big257: 258 tiles, workgroups 0 and 1 walk a second tile and
    the last one holds 6 rows.  A third of the edges leave their tile's
    neighbourhood, so the dx gather reads dz rows that other workgroups wrote."""
    gh = big(name)
    n = gh.num_nodes()
    assert pkg._lib.query("scgib_conv_slabs", n) == BG.GRID_CAP
    assert BG.tiles(n) == (BG.GRID_CAP if name == "big256" else BG.GRID_CAP + 2)
    check_layer(pkg, dev, gh, mode, shape[0], shape[1], True, seed=shape[0] + shape[1])


def _layer_twice(pkg, dev, gh, mode, shape):
    g = gh.to(dev)
    n = g.num_nodes()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(n, shape[0], generator=gen)
    gout = torch.randn(n, shape[1], generator=gen)
    wn, ws, b = make_weights(mode, shape[0], shape[1], 3)
    a = run_layer(pkg, g, x, wn, ws, b, mode, True, gout)
    c = run_layer(pkg, g, x, wn, ws, b, mode, True, gout)
    assert torch.equal(a[0], c[0])
    for ga, gc in zip(a[1], c[1]):
        assert (ga is None) == (gc is None)
        if ga is not None:
            assert torch.equal(ga, gc)


@pytest.mark.parametrize("mode,shape", [("gcn", (128, 128)), ("mean", (64, 64))])
def test_layer_deterministic(pkg, dev, mols37, mode, shape):
    _layer_twice(pkg, dev, mols37, mode, shape)


@pytest.mark.parametrize("mode,shape", [("gcn", (128, 128)), ("mean", (64, 64))])
def test_layer_deterministic_past_256_tiles(pkg, dev, big, mode, shape):
    _layer_twice(pkg, dev, big("big257"), mode, shape)


def test_unsupported_shapes_are_refused(pkg, dev, mols37):
    g = mols37.to(dev)
    x = torch.randn(g.num_nodes(), 48, device=dev)
    with pytest.raises(pkg._lib.ScgibError):
        pkg.ops.conv_layer(x, g, torch.randn(48, 64, device=dev), None, None, "gcn", False)
    x = torch.randn(g.num_nodes(), 64, device=dev)
    with pytest.raises(pkg._lib.ScgibError):
        pkg.ops.conv_layer(x, g, torch.randn(64, 32, device=dev), None, None, "gcn", False)


# ---------------------------------------------------------------------------
# encoder level
# ---------------------------------------------------------------------------
def make_encoder(pkg, name, seed=0):
    torch.manual_seed(seed)
    enc = pkg.models.GCN(32, 64) if name == "GCN" else pkg.models.GraphSAGE(32, 64)
    with torch.no_grad():  # DGL zero-initialises the biases: make them count
        for n_, p in enc.named_parameters():
            if n_.endswith("bias"):
                p.normal_(0.0, 0.2)
    return enc


def layer_plan(name):
    """[(conv name, relu)] of the reference's forwards (models.py:82-88, :98-104)."""
    if name == "GCN":
        return [("conv1", True), ("conv2", True), ("conv3", False)], "gcn"
    return [("conv1", True), ("conv2", True), ("conv2", False)], "mean"


def conv_weights(p, prefix, mode):
    if mode == "gcn":
        return p[prefix + ".weight"], None, p[prefix + ".bias"]
    return p[prefix + ".fc_neigh.weight"], p[prefix + ".fc_self.weight"], p[prefix + ".bias"]


def ref_encoder(p, prefix, name, src, dst, h, masks=None, split=None):
    """fp64 encoder over the parameter dict ``p``.  ``split``: a dict that
    receives one separate leaf copy of the weights per USE of a conv (to take
    the gradient of each use apart)."""
    plan, mode = layer_plan(name)
    for i, (conv, relu) in enumerate(plan):
        wn, ws, b = conv_weights(p, f"{prefix}.{conv}" if prefix else conv, mode)
        if split is not None:
            wn, ws, b = (None if t is None else t.detach().clone().requires_grad_(True)
                         for t in (wn, ws, b))
            split[i] = (wn, ws, b)
        h = ref_layer(h, src, dst, wn, ws, b, mode, relu, masks[i] if masks and relu else None)
    return h


def hip_relu_masks(pkg, enc, g, h):
    """The kernels' own ReLU decisions per layer, from the public layer op
    (the launches conv_encoder makes, so the same bits)."""
    plan, mode = layer_plan(type(enc).__name__)
    masks = []
    with torch.no_grad():
        for conv, relu in plan:
            wn, ws, b = getattr(enc, conv).conv_params()
            h = pkg.ops.conv_layer(h, g, wn, ws, b, mode, relu)
            masks.append((h > 0).cpu() if relu else None)
    return masks, h


def check_encoder(pkg, dev, name, gh):
    g = gh.to(dev)
    n = gh.num_nodes()
    src, dst = gh.edges()
    enc = make_encoder(pkg, name, 1).to(dev)
    gen = torch.Generator().manual_seed(2)
    h0 = torch.randn(n, 32, generator=gen)
    gout = torch.randn(n, 64, generator=gen)
    h = h0.to(dev).requires_grad_(True)
    out = enc(g, h)
    out.backward(gout.to(dev))
    torch.cuda.synchronize()
    masks, chained = hip_relu_masks(pkg, enc, g, h.detach())
    assert torch.equal(chained, out.detach())  # conv_encoder == the chained public op

    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in enc.state_dict().items()}
    hr = h0.double().requires_grad_(True)
    ref = ref_encoder(p, "", name, src, dst, hr, masks)
    ref.backward(gout.double())
    assert rel_err(out.detach().cpu(), ref.detach()) < ACT_TOL
    assert rel_l2(h.grad.cpu(), hr.grad) < GRAD_TOL
    mine = dict(enc.named_parameters())
    for k, r in p.items():
        if name == "GraphSAGE" and k.startswith("conv3."):
            assert mine[k].grad is None and r.grad is None, k  # built, never used
            continue
        err = rel_l2(mine[k].grad.cpu(), r.grad)
        assert err < GRAD_TOL, (k, err)

    if name == "GraphSAGE":  # conv2's gradient is the sum over its two uses
        split = {}
        hr2 = h0.double()
        ref_encoder({k: v.detach() for k, v in p.items()}, "", name, src, dst, hr2, masks,
                    split).backward(gout.double())
        for j, key in enumerate(("conv2.fc_neigh.weight", "conv2.fc_self.weight", "conv2.bias")):
            first, second = split[1][j].grad, split[2][j].grad
            got = mine[key].grad.cpu()
            assert rel_l2(got, first + second) < GRAD_TOL, key
            assert rel_l2(got, first) > 1e-2 and rel_l2(got, second) > 1e-2, key


@pytest.mark.parametrize("name", ["GCN", "GraphSAGE"])
def test_encoder_matches_fp64(pkg, dev, name):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(40, "qm9", seed=9))
    check_encoder(pkg, dev, name, gh)


@pytest.mark.parametrize("name", ["GCN", "GraphSAGE"])
def test_encoder_matches_fp64_past_256_tiles(pkg, dev, name):
    """258 tiles, the last of 30 rows: the inter-layer mask fusion, the
    256-slab reduce and "encoder == chained public op" at that size."""
    gh = BG.big_molecules(pkg)
    n = gh.num_nodes()
    assert n > 256 * 64 and n % 64 != 0
    assert pkg._lib.query("scgib_conv_slabs", n) == BG.GRID_CAP
    check_encoder(pkg, dev, name, gh)


def _encoder_step(enc, g, h, gout):
    for p in enc.parameters():
        p.grad = None
    h.grad = None
    out = enc(g, h)
    out.backward(gout)
    return out


def check_capacity_mode(pkg, dev, name, gh, capacities, oracle):
    """A StaticBatch with spare rows: live rows bitwise the unpadded run's,
    padded rows of out / dx zero, weight gradients bitwise equal.  ``oracle``:
    the capacity run's gradients against fp64 as well."""
    B = gh.batch_size
    n = gh.num_nodes()
    n_cap, e_cap, mgn, caps = capacities
    assert (n_cap + 63) // 64 > (n + 63) // 64  # whole spare tiles, and a partly live one
    static = pkg.graph.StaticBatch(B, n_cap, e_cap, gh.ndata["x"].shape[1], mgn, caps, dev)
    static.load(static.pad(gh))
    g = gh.to(dev)
    gen = torch.Generator().manual_seed(4)
    h_cap = torch.randn(n_cap, 32, generator=gen).to(dev)    # padded rows hold live-looking
    go_cap = torch.randn(n_cap, 64, generator=gen).to(dev)   # values: they must not count
    enc = make_encoder(pkg, name, 2).to(dev)

    h = h_cap[:n].clone().requires_grad_(True)
    out = _encoder_step(enc, g, h, go_cap[:n].contiguous())
    grads = {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    dx = h.grad.clone()

    hc = h_cap.clone().requires_grad_(True)
    out_c = _encoder_step(enc, static.graph, hc, go_cap)
    torch.cuda.synchronize()
    assert torch.equal(out_c[:n], out) and torch.equal(hc.grad[:n], dx)
    assert torch.count_nonzero(out_c[n:]) == 0 and torch.count_nonzero(hc.grad[n:]) == 0
    for k, p in enc.named_parameters():
        if k in grads:
            assert torch.equal(p.grad, grads[k]), k

    if oracle:  # not only a self-comparison: the capacity run against fp64
        masks, _ = hip_relu_masks(pkg, enc, g, h.detach())
        src, dst = gh.edges()
        pr = {k: v.detach().cpu().double().requires_grad_(True) for k, v in enc.state_dict().items()}
        hr = h_cap[:n].cpu().double().requires_grad_(True)
        ref = ref_encoder(pr, "", name, src, dst, hr, masks)
        ref.backward(go_cap[:n].cpu().double())
        assert rel_err(out_c[:n].detach().cpu(), ref.detach()) < ACT_TOL
        assert rel_l2(hc.grad[:n].cpu(), hr.grad) < GRAD_TOL
        for k, p in enc.named_parameters():
            if k in grads:
                err = rel_l2(p.grad.cpu(), pr[k].grad)
                assert err < GRAD_TOL, (k, err)

    # the public layer op with its own ReLU mask (dz materialised) likewise
    _, mode = layer_plan(name)
    wn, ws, b = enc.conv2.conv_params()
    d_in = wn.shape[0] if mode == "gcn" else wn.shape[1]
    d_out = wn.numel() // d_in
    xc = torch.randn(n_cap, d_in, generator=gen).to(dev)
    gc = torch.randn(n_cap, d_out, generator=gen).to(dev)
    res = []
    for graph, rows in ((g, n), (static.graph, n_cap)):
        leaves = [t.detach().clone().requires_grad_(True) for t in (xc[:rows], wn, b)]
        w_self = ws.detach() if ws is not None else None
        o = pkg.ops.conv_layer(leaves[0], graph, leaves[1], w_self, leaves[2], mode, True)
        o.backward(gc[:rows].contiguous())
        res.append((o.detach(), [t.grad for t in leaves]))
    torch.cuda.synchronize()
    (o_e, g_e), (o_c, g_c) = res
    assert torch.equal(o_c[:n], o_e) and torch.count_nonzero(o_c[n:]) == 0
    assert torch.equal(g_c[0][:n], g_e[0]) and torch.count_nonzero(g_c[0][n:]) == 0
    assert torch.equal(g_c[1], g_e[1]) and torch.equal(g_c[2], g_e[2])


@pytest.mark.parametrize("name", ["GCN", "GraphSAGE"])
def test_encoder_capacity_mode(pkg, dev, name):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(48, "qm9", seed=21))
    check_capacity_mode(pkg, dev, name, gh, pkg.graph.StaticBatch.capacities([gh], 1, slack=1.3),
                        False)


@pytest.mark.parametrize("split", list(BG.CAPACITY_SPLITS))
@pytest.mark.parametrize("name", ["GCN", "GraphSAGE"])
def test_encoder_capacity_mode_across_256_tiles(pkg, dev, name, split):
    """The same assertions with the 256-workgroup line between or behind the
    live tiles (BG.CAPACITY_SPLITS): a workgroup's second tile live, partly
    live or padded, and workgroups that meet padding only.  Tile -> workgroup
    is tile mod 256 in both runs and trailing zero slabs add +0.0 to their
    partition, so the bitwise claim carries over."""
    gh, capacities = BG.capacity_case(pkg, split)
    check_capacity_mode(pkg, dev, name, gh, capacities, True)


@pytest.mark.parametrize("name", ["GCN", "GraphSAGE"])
def test_encoder_captures(pkg, dev, name):
    """Forward + backward on a fixed graph under torch.cuda.graph, replayed
    twice: bitwise the eager run (no host sync anywhere on the path)."""
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(40, "qm9", seed=13))
    g = gh.to(dev)
    n = gh.num_nodes()
    gen = torch.Generator().manual_seed(6)
    h = torch.randn(n, 32, generator=gen).to(dev).requires_grad_(True)
    gout = torch.randn(n, 64, generator=gen).to(dev)
    enc = make_encoder(pkg, name, 3).to(dev)
    out_e = _encoder_step(enc, g, h, gout).detach().clone()
    want = {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    dx_e = h.grad.clone()
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up (allocator) off the capture
        _encoder_step(enc, g, h, gout)
    torch.cuda.current_stream().wait_stream(side)
    for p in enc.parameters():
        p.grad = None
    h.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = enc(g, h)
        out_s.backward(gout)
    for _ in range(2):
        with torch.no_grad():  # a replay must rewrite every result
            out_s.fill_(float("nan"))
            h.grad.fill_(float("nan"))
            for p in enc.parameters():
                if p.grad is not None:
                    p.grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_s.detach(), out_e) and torch.equal(h.grad, dx_e)
        got = {k: p.grad for k, p in enc.named_parameters() if p.grad is not None}
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
B_MODEL = 24


def _args():
    return SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=B_MODEL, gin_layers=5, task="graph_classification")


def _make_model(pkg, encoder, wrapped, f_in, dev):
    torch.manual_seed(17)
    model = pkg.models.Mainmodel(_args(), f_in, 64, 4, 4, 1, encoder)
    if wrapped:
        model = pkg.models.Mainmodel_continue(_args(), f_in, 64, 4, 4, 1, 1, model, encoder)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "Encoder" in k and k.endswith("bias"):
                p.normal_(0.0, 0.1)
            if "compressor.1" in k:
                p.add_(0.2 * torch.randn_like(p))
    return model.to(dev).train()


def _composed_oracle(model, encoder, wrapped, gh, u_gate, u_feat):
    """R.pretrain_forward's composition (fp64) around the fp64 encoders."""
    inner = "model." if wrapped else ""
    hot = ("transfer_d.", "MLP.", inner + "Encoder", inner + "compressor.", inner + "attn_layer.")
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith(hot)}
    p = {}
    for k, v in sd.items():
        t = v.clone()
        if t.is_floating_point():
            t = t.double()
            if "running" not in k:
                t.requires_grad_(True)
        p[k[len(inner):] if inner and k.startswith(inner) else k] = t
    sizes, ecount, nodes, esrc, edst = egonet.egonets(gh.rowptr.numpy(), gh.col.numpy(), 1)
    off = np.repeat(np.concatenate([[0], np.cumsum(sizes)[:-1]]), ecount)
    src, dst = gh.edges()
    counts = torch.from_numpy(gh.batch_num_nodes_host())
    es, ed = torch.from_numpy(esrc + off), torch.from_numpy(edst + off)
    x = F.normalize(gh.ndata["x"].double())
    xs = x[torch.from_numpy(nodes)]
    h0 = R._linear(x, p, "transfer_d", bias=False)
    hs0 = R._linear(xs, p, "transfer_d", bias=False)
    gf = ref_encoder(p, "Encoder1", encoder, src, dst, h0)
    sf = ref_encoder(p, "Encoder2", encoder, es, ed, hs0)
    readout = R.sum_nodes(gf, counts)
    noisy, _, kl_tensor = R.compression(p, gf, counts, u_gate.double(), u_feat.double(), None)
    im = R.attention(p, noisy, R.sum_nodes(sf, torch.from_numpy(sizes)), counts)
    im = R._linear(F.relu(R._linear(im, p, "MLP.0")), p, "MLP.2")
    kl = torch.mean(kl_tensor)
    con = R.semi_loss(R.sum_nodes(noisy, counts), readout, B_MODEL)
    rec = R.recon_adj_dense(im, src, dst)
    (kl + con + rec).backward()
    grads = {}
    for k in sd:
        sk = k[len(inner):] if inner and k.startswith(inner) else k
        if p[sk].requires_grad and p[sk].grad is not None:
            grads[k] = p[sk].grad.numpy()
    return [kl.item(), con.item(), rec.item()], grads


@pytest.mark.parametrize("wrapped", [False, True], ids=["Mainmodel", "Mainmodel_continue"])
@pytest.mark.parametrize("encoder", ["GCN", "GraphSAGE"])
def test_model_step_matches_composed_oracle(pkg, dev, encoder, wrapped):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(B_MODEL, "qm9", seed=31))
    f_in = gh.ndata["x"].shape[1]
    n = gh.num_nodes()
    gen = torch.Generator().manual_seed(77)
    u_gate, u_feat = torch.rand(n, generator=gen), torch.rand(n, 64, generator=gen)
    model = _make_model(pkg, encoder, wrapped, f_in, dev)
    losses_ref, grads_ref = _composed_oracle(copy.deepcopy(model).cpu(), encoder, wrapped, gh,
                                             u_gate, u_feat)
    g = gh.to(dev)
    x = F.normalize(g.ndata["x"].float())
    _, kl, con, rec = model(g, x, None, None, None, 1, None, 1, dev, B_MODEL,
                            noise=(u_gate.to(dev), u_feat.to(dev)))
    (kl + con + rec).backward()
    torch.cuda.synchronize()
    for name, a, b in zip(("kl", "contrastive", "recon"), (kl, con, rec), losses_ref):
        print(f"{encoder} wrapped={wrapped} {name}: {a.item():.8g} vs {b:.8g}")
        assert rel_err(a.item(), b) < LOSS_TOL, (name, a.item(), b)
    params = dict(model.named_parameters())
    inner = "model." if wrapped else ""
    enc_keys = [k for k in grads_ref if k.startswith((inner + "Encoder", "transfer_d."))]
    assert any("Encoder1" in k for k in enc_keys) and any("Encoder2" in k for k in enc_keys)
    errs = check_grads_model({k: grads_ref[k] for k in enc_keys}, lambda k: params[k].grad)
    print({k: f"{v:.2e}" for k, v in errs.items()})
    if encoder == "GraphSAGE":
        for e in ("Encoder1", "Encoder2"):
            for k in ("fc_self.weight", "fc_neigh.weight", "bias"):
                assert params[f"{inner}{e}.conv3.{k}"].grad is None
                assert f"{inner}{e}.conv3.{k}" not in grads_ref
    # one optimizer step (skips conv3's missing gradients)
    before = {k: p.detach().clone() for k, p in params.items()}
    opt = pkg.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-5)
    opt.step()
    torch.cuda.synchronize()
    for k, p in params.items():
        assert torch.isfinite(p).all(), k
        if p.grad is None:
            assert torch.equal(p, before[k]), k
    assert not torch.equal(params[inner + "Encoder1.conv1.bias"], before[inner + "Encoder1.conv1.bias"])
