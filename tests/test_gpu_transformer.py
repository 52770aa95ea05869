"""The Transformer encoder on the graph Transformer kernels (csrc/gt_layer.hip)
against an fp64 restatement of the reference's MultiHeadAttentionLayer /
GraphTransformerLayer / Transformer (models.py:807-918, :986-1005), written
here from the formulas with index_add over the input's own edge list:

  e = K[u,a,:] . Q[v,a,:] / sqrt(d_h);  s = exp(clamp(e, -5, 5))
  attn[v,a,:] = sum_{u->v} s V[u,a,:] / (sum_{u->v} s + 1e-6)
  h1 = LN1(h + attn Wo^T + bo);  out = LN2(h1 + dropout(relu(h1 W1^T + b1)) W2^T + b2)

Tolerances are tests/test_gpu_parity.py's, as tests/test_gpu_encoders.py uses
them: activations rel_err < 1e-4, each gradient tensor rel_l2 < 1e-3, losses
within 1e-4.  Where two correct evaluations may decide differently, the fp64
side follows the kernels' own decision: an FFN pre-activation within 1e-5 of
zero (aux["ffn_pos"], oracle.scgib_ref._relu) and a score within 1e-5 of +-5
(aux["score"]).
"""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import big_graphs as BG
from conftest import CANCELLED, check_grads_model, rel_err, rel_l2
from oracle import egonet
from oracle import scgib_ref as R

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4
ACT_TOL = 1e-4
GRAD_TOL = 1e-3
TIE = 1e-5
H, F2 = 64, 128
HEADS = [1, 4, 8]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
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
    s, d, _ = _path(4)  # node 0 isolated, then a path 1-2-3-4
    out["isolated_first"] = (s + 1, d + 1, 5)
    out["star9"] = _star(9)
    out["star33"] = _star(33)  # in-degree 33: beyond any small unroll
    # directed, non-symmetric: v -> v+1, v -> v+3, v -> 2v+5 (mod n), no reverse edges kept
    out["directed"] = BG.directed(70)
    return out


HAND = _hand_graphs()


class Case:
    """A host graph, its device copy and the edge list the fp64 side sums over.
    ``name``: "mols", a hand graph, or a BG.BIG_SIZES graph (the directed
    recipe just past 256 tiles)."""

    def __init__(self, pkg, dev, name):
        if name == "mols":
            self.gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(37, "qm9", seed=5))
            assert self.gh.num_nodes() % 64 != 0 and self.gh.num_nodes() > 3 * 64
            self.src, self.dst = self.gh.edges()
        else:
            src, dst, n = BG.big_directed(name) if name in BG.BIG_SIZES else HAND[name]
            self.gh = pkg.graph.GraphBatch.from_edges(src, dst, n, symmetric_hint=False)
            if name == "directed" or name in BG.BIG_SIZES:
                din, dout = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
                assert (din != dout).mean() > 0.5  # a backward over the wrong CSR cannot pass
            # the reference's edge list is the input's, not read back from the CSR under test
            es, ed = self.gh.edges()
            assert sorted(zip(es.tolist(), ed.tolist())) == sorted(zip(src.tolist(), dst.tolist()))
            self.src, self.dst = torch.from_numpy(src), torch.from_numpy(dst)
        self.n = self.gh.num_nodes()
        self.g = self.gh.to(dev)
        # row of the kernels' [E, heads] score (dst-major CSR order) for each listed edge
        rp, col = self.gh.rowptr.long(), self.gh.col.long()[: self.src.numel()]
        cdst = torch.repeat_interleave(torch.arange(self.n), rp[1:] - rp[:-1])
        key = cdst * self.n + col
        assert key.unique().numel() == key.numel()
        order = torch.argsort(key)
        want = self.dst * self.n + self.src
        self.score_row = order[torch.searchsorted(key[order], want)] if want.numel() else want
        assert torch.equal(key[self.score_row], want)


_CASES = {}


@pytest.fixture
def case(pkg, dev):
    def get(name):
        if name not in _CASES:
            _CASES[name] = Case(pkg, dev, name)
        return _CASES[name]
    return get


# ---------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------
def ref_attention(q, k, v, c, heads, score_hip=None, clamp=True):
    """(attn [n, 64], e [E, heads]) in fp64 over c's edge list.  score_hip: the
    kernels' scores in the edge list's order — followed within TIE of +-5."""
    n, dh = q.shape[0], H // heads
    Q, K, V = (t.view(n, heads, dh) for t in (q, k, v))
    e = (K[c.src] * Q[c.dst]).sum(-1) / dh ** 0.5
    ec = e
    if clamp:
        inside = (e >= -5) & (e <= 5)
        if score_hip is not None:
            near = (e.detach().abs() - 5).abs() < TIE
            inside = torch.where(near, score_hip.double().abs() <= 5, inside)
        ec = torch.where(inside, e, torch.sign(e.detach()) * 5.0)
    s = torch.exp(ec)
    wv = torch.zeros(n, heads, dh, dtype=q.dtype).index_add(0, c.dst, s.unsqueeze(-1) * V[c.src])
    z = torch.zeros(n, heads, dtype=q.dtype).index_add(0, c.dst, s)
    return (wv / (z.unsqueeze(-1) + 1e-6)).reshape(n, H), e


def ref_layer(h, p, pre, c, heads, training, keep=None, aux=None):
    """One GraphTransformerLayer in fp64 over the parameter dict p (prefix pre)."""
    lin = lambda x, name: F.linear(x, p[pre + name + ".weight"], p[pre + name + ".bias"])
    score = aux["score"][c.score_row].cpu() if aux is not None else None
    attn, _ = ref_attention(lin(h, "attention.Q"), lin(h, "attention.K"), lin(h, "attention.V"), c,
                            heads, score)
    h1 = F.layer_norm(h + lin(attn, "O"), (H,), p[pre + "layer_norm1.weight"],
                      p[pre + "layer_norm1.bias"], 1e-5)
    r = R._relu(lin(h1, "FFN_layer1"), aux["ffn_pos"].cpu() if aux is not None else None, TIE)
    if training:
        r = r * keep.double() * 2.0
    return F.layer_norm(h1 + lin(r, "FFN_layer2"), (H,), p[pre + "layer_norm2.weight"],
                        p[pre + "layer_norm2.bias"], 1e-5)


def ref_params(module):
    p = {}
    for k, v in module.state_dict().items():
        t = v.detach().cpu().clone()
        if t.is_floating_point():
            t = t.double()
            if "running" not in k:
                t.requires_grad_(True)
        p[k] = t
    return p


USED = ("attention.Q.", "attention.K.", "attention.V.", "O.", "layer_norm1.", "layer_norm2.",
        "FFN_layer1.", "FFN_layer2.")
UNUSED = ("attention.q_proj.", "attention.k_proj.", "attention.v_proj.", "batchnorm1.",
          "batchnorm2.")


# The K bias adds b_K . Q[v,a,:] / sqrt(d_h) to the score of EVERY in-edge of
# (v, a): all its s scale by one factor, which cancels in wV / (z + 1e-6) up to
# the 1e-6 — unless a score of that node is clamped.  Its gradient is then zero
# in real arithmetic and both sides hold rounding noise only; such tensors are
# held to conftest.check_grads's floor for cancelled gradients, 1e-3 of the
# sibling weight's gradient, instead of a relative error of noise.
CANCELLED_GT = ("attention.K.bias",)


def check_grad(name, mine, ref, sibling=None):
    assert mine is not None, name
    assert mine.shape == ref.shape, name
    if name.endswith(CANCELLED_GT):
        floor = 1e-3 * float(sibling.abs().max())
        if float(ref.abs().max()) <= floor:
            assert float(mine.abs().max()) <= floor, name
            return
    if float(ref.abs().max()) == 0.0:
        assert float(mine.abs().max()) == 0.0, name
        return
    err = rel_l2(mine.cpu(), ref)
    assert err < GRAD_TOL, (name, err)


# ---------------------------------------------------------------------------
# 1, 2: the attention op
# ---------------------------------------------------------------------------
def run_attention(pkg, c, heads, sigma, seed):
    gen = torch.Generator().manual_seed(seed)
    q0, k0 = (torch.randn(c.n, H, generator=gen) * sigma for _ in range(2))
    v0, gout = (torch.randn(c.n, H, generator=gen) for _ in range(2))
    dev = c.g.rowptr.device
    leaves = [t.to(dev).requires_grad_(True) for t in (q0, k0, v0)]
    attn, score = pkg.ops.graph_attention(*leaves, c.g, heads, return_score=True)
    attn.backward(gout.to(dev))
    torch.cuda.synchronize()
    assert score.shape == (c.g.col.numel(), heads) and not score.requires_grad
    return (q0, k0, v0, gout), attn.detach(), score.detach(), [t.grad for t in leaves]


def ref_attention_grads(inputs, c, heads, score, clamp=True):
    q0, k0, v0, gout = inputs
    leaves = [t.double().requires_grad_(True) for t in (q0, k0, v0)]
    attn, e = ref_attention(*leaves, c, heads, score, clamp)
    attn.backward(gout.double())
    return attn.detach(), e.detach(), [t.grad for t in leaves]


def check_attention_op(pkg, c, heads):
    inputs, attn, score, grads = run_attention(pkg, c, heads, 1.0, 11 + heads)
    sc = score[c.score_row].cpu()
    ref, e, rgrads = ref_attention_grads(inputs, c, heads, sc)
    if e.numel():
        assert rel_err(sc, e) < ACT_TOL  # the scaled pre-clamp scores, edge by edge
    assert rel_err(attn.cpu(), ref) < ACT_TOL
    for nm, mine, r in zip(("dQ", "dK", "dV"), grads, rgrads):
        check_grad(nm, mine, r)
    indeg = torch.bincount(c.dst, minlength=c.n)
    for v in torch.nonzero(indeg == 0).flatten().tolist():  # isolated: exact zeros
        assert torch.count_nonzero(attn[v]) == 0
        assert torch.count_nonzero(grads[0][v]) == 0


@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("name", ["mols"] + list(HAND))
def test_attention_op(pkg, case, name, heads):
    check_attention_op(pkg, case(name), heads)


@pytest.mark.parametrize("heads", HEADS)
def test_attention_op_past_256_tiles(pkg, case, heads):
    """16,454 rows: the 2v+5 edges make both backward walks (by destination,
    then by source over the transposed CSR) read rows of far workgroups."""
    c = case("big257")
    assert BG.tiles(c.n) > BG.GRID_CAP and c.n % BG.TILE == 6
    check_attention_op(pkg, c, heads)


@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("name", ["mols"] + list(HAND))
def test_attention_clamp(pkg, case, name, heads):
    """Q, K ~ N(0, 5): the scaled score has standard deviation about 5 for any
    heads, so a good part of the (edge, head) pairs sits on either side of
    the clamp, where its gradient is 0."""
    c = case(name)
    inputs, attn, score, grads = run_attention(pkg, c, heads, 5.0 ** 0.5, 23 + heads)
    sc = score[c.score_row].cpu()
    ref, e, rgrads = ref_attention_grads(inputs, c, heads, sc)
    assert rel_err(attn.cpu(), ref) < ACT_TOL
    for nm, mine, r in zip(("dQ", "dK", "dV"), grads, rgrads):
        check_grad(nm, mine, r)
    # With fewer than 200 (edge, head) pairs a 5 % floor on ~16 % events is not
    # a reliable statement about the sample; the parity above still holds there.
    if e.numel() >= 200:
        above, below = (e > 5).double().mean().item(), (e < -5).double().mean().item()
        inside = (e.abs() <= 5).double().mean().item()
        print(f"{name} heads={heads}: above {above:.3f} below {below:.3f} inside {inside:.3f}")
        assert above >= 0.05 and below >= 0.05 and inside >= 0.30
        # the case discriminates: without the clamp the fp64 gradients are out of tolerance
        _, _, ugrads = ref_attention_grads(inputs, c, heads, None, clamp=False)
        assert max(rel_l2(m.cpu(), r) for m, r in zip(grads[:2], ugrads[:2])) > GRAD_TOL


# ---------------------------------------------------------------------------
# 3, 6: one layer
# ---------------------------------------------------------------------------
def make_layer(pkg, dev, heads, seed, training):
    torch.manual_seed(seed)
    layer = pkg.models.GraphTransformerLayer(H, H, heads)
    with torch.no_grad():  # make the biases and the LayerNorm affines count
        for k, p in layer.named_parameters():
            if k.endswith("bias"):
                p.normal_(0.0, 0.2)
            if k.startswith("layer_norm") and k.endswith("weight"):
                p.add_(0.3 * torch.randn_like(p))
    return layer.to(dev).train(training)


def run_layer(pkg, c, layer, h0, gout, drop_mask=None, seed=None):
    dev = c.g.rowptr.device
    for p in layer.parameters():
        p.grad = None
    if seed is not None:
        pkg.ops.seed_dropout(dev, seed)
    h = h0.to(dev).requires_grad_(True)
    out, aux = pkg.ops.gt_layer(h, c.g, layer, drop_mask, return_aux=True)
    out.backward(gout.to(dev))
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None}
    return out.detach(), aux, h.grad.clone(), grads


def layer_inputs(c, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(c.n, H, generator=gen), torch.randn(c.n, H, generator=gen)


def layer_mode(pkg, c, mode, seed):
    """(layer, explicit mask or None, dropout seed or None) of a test mode."""
    layer = make_layer(pkg, c.g.rowptr.device, 4, seed, mode != "eval")
    mask = None
    if mode == "mask":
        gen = torch.Generator().manual_seed(seed + 1)
        mask = (torch.rand(c.n, F2, generator=gen) < 0.5).to(c.g.rowptr.device)
    return layer, mask, 4242 if mode == "drawn" else None


def check_layer_fp64(pkg, c, mode):
    layer, mask, seed = layer_mode(pkg, c, mode, 5)
    h0, gout = layer_inputs(c, 31)
    out, aux, dh, grads = run_layer(pkg, c, layer, h0, gout, mask, seed)
    assert aux["ffn_pos"].shape == (c.n, F2) and aux["keep"].shape == (c.n, F2)
    if mode == "mask":
        assert torch.equal(aux["keep"], mask)
    p = ref_params(layer)
    hr = h0.double().requires_grad_(True)
    ref = ref_layer(hr, p, "", c, 4, mode != "eval", aux["keep"].cpu(), aux)
    ref.backward(gout.double())
    assert rel_err(out.cpu(), ref.detach()) < ACT_TOL
    check_grad("dh", dh, hr.grad)
    for k, r in p.items():
        if k.startswith(USED):
            check_grad(k, grads.get(k), r.grad, p[k.rsplit(".", 1)[0] + ".weight"].grad)
        else:
            assert k.startswith(UNUSED) and k not in grads and (not r.requires_grad or r.grad is None), k
    assert len(grads) == 16


@pytest.mark.parametrize("mode", ["eval", "mask", "drawn"])
@pytest.mark.parametrize("name", ["mols", "directed"])
def test_layer_matches_fp64(pkg, case, name, mode):
    check_layer_fp64(pkg, case(name), mode)


@pytest.mark.parametrize("mode", ["eval", "mask"])
@pytest.mark.parametrize("name", list(BG.BIG_SIZES))
def test_layer_past_256_tiles(pkg, case, name, mode):
    """gt_lin_bwd_k runs at most 256 workgroups.  big256: one full tile each,
    the boundary; big257: 258 tiles, workgroups 0 and 1 walk a second tile
    (weight, bias and LayerNorm accumulators live across it) and the last one
    holds 6 rows."""
    c = case(name)
    assert pkg._lib.query("scgib_gt_slabs", c.n) == BG.GRID_CAP
    assert BG.tiles(c.n) == (BG.GRID_CAP if name == "big256" else BG.GRID_CAP + 2)
    check_layer_fp64(pkg, c, mode)


def _layer_twice(pkg, c, mode):
    layer, mask, seed = layer_mode(pkg, c, mode, 6)
    h0, gout = layer_inputs(c, 32)
    a = run_layer(pkg, c, layer, h0, gout, mask, seed)
    b = run_layer(pkg, c, layer, h0, gout, mask, seed)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert torch.equal(a[1]["keep"], b[1]["keep"])
    assert set(a[3]) == set(b[3])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("mode", ["eval", "mask", "drawn"])
def test_layer_deterministic(pkg, case, mode):
    _layer_twice(pkg, case("mols"), mode)


def test_layer_deterministic_past_256_tiles(pkg, case):
    _layer_twice(pkg, case("big257"), "drawn")


# ---------------------------------------------------------------------------
# 4: the encoder
# ---------------------------------------------------------------------------
def make_encoder(pkg, dev, seed):
    torch.manual_seed(seed)
    enc = pkg.models.Transformer(32, H, 4, 4, dev)
    with torch.no_grad():
        for k, p in enc.named_parameters():
            if k.endswith("bias"):
                p.normal_(0.0, 0.2)
    return enc.to(dev)


def ref_encoder(p, pre, c, h, n_layers, heads, training, keeps=None, auxes=None):
    h = F.linear(h, p[pre + "embedding_h.weight"])
    for i in range(n_layers):
        h = ref_layer(h, p, f"{pre}layers.{i}.", c, heads, training,
                      keeps[i] if keeps is not None else None,
                      auxes[i] if auxes is not None else None)
    return h


class EdgeList:
    """ref_* over a bare edge list (no kernel decisions to follow)."""

    def __init__(self, src, dst):
        self.src, self.dst = src, dst


def score_rows(gh, c):
    """Row of the kernels' [E, heads] score (dst-major CSR order) of each edge of c."""
    n = gh.num_nodes()
    rp, col = gh.rowptr.long(), gh.col.long()
    cdst = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    key = cdst * n + col
    order = torch.argsort(key)
    return order[torch.searchsorted(key[order], c.dst * n + c.src)]


def check_encoder_fp64(pkg, dev, gh):
    g, n = gh.to(dev), gh.num_nodes()
    enc = make_encoder(pkg, dev, 1).train()
    assert len(enc.layers) == 5
    gen = torch.Generator().manual_seed(2)
    h0, gout = torch.randn(n, 32, generator=gen), torch.randn(n, H, generator=gen)
    masks = [(torch.rand(n, F2, generator=gen) < 0.5).to(dev) for _ in enc.layers]
    buffers = {k: v.clone() for k, v in enc.named_buffers()}
    h = h0.to(dev).requires_grad_(True)
    out = enc(g, h, masks)
    out.backward(gout.to(dev))
    torch.cuda.synchronize()

    # the encoder is the chained public layer op, bit for bit
    auxes = []
    with torch.no_grad():
        x = F.linear(h.detach(), enc.embedding_h.weight)
        for layer, m in zip(enc.layers, masks):
            x, aux = pkg.ops.gt_layer(x, g, layer, m, return_aux=True)
            auxes.append(aux)
    assert torch.equal(x, out.detach())

    c = EdgeList(*gh.edges())
    c.score_row = score_rows(gh, c)
    p = ref_params(enc)
    hr = h0.double().requires_grad_(True)
    ref = ref_encoder(p, "", c, hr, 5, 4, True, [m.cpu() for m in masks], auxes)
    ref.backward(gout.double())
    assert rel_err(out.detach().cpu(), ref.detach()) < ACT_TOL
    check_grad("dh", h.grad, hr.grad)
    mine = dict(enc.named_parameters())
    for k, r in p.items():
        if not r.requires_grad:
            continue
        if any(u in k for u in UNUSED):  # built, never used
            assert mine[k].grad is None and r.grad is None, k
        else:
            check_grad(k, mine[k].grad, r.grad, p[k.rsplit(".", 1)[0] + ".weight"].grad)
    for k, v in enc.named_buffers():  # the BatchNorm statistics never move
        assert torch.equal(v, buffers[k]), k


def test_encoder_matches_fp64(pkg, dev):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(40, "qm9", seed=9))
    check_encoder_fp64(pkg, dev, gh)


def test_encoder_matches_fp64_past_256_tiles(pkg, dev):
    """258 tiles, the last of 30 rows: five layers, each with its three
    backward tile kernels and the 256-slab reduce, and "encoder == chained
    public op" at that size."""
    gh = BG.big_molecules(pkg)
    n = gh.num_nodes()
    assert n > 256 * 64 and n % 64 != 0
    assert pkg._lib.query("scgib_gt_slabs", n) == BG.GRID_CAP
    check_encoder_fp64(pkg, dev, gh)


def test_module_forwards(pkg, case, dev):
    """The sub-modules' own forwards (reference argument order: h, then g)."""
    c = case("mols")
    layer = make_layer(pkg, dev, 4, 9, False)
    h = torch.randn(c.n, H, generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        assert torch.equal(layer(h, c.g), pkg.ops.gt_layer(h, c.g, layer))
        a = layer.attention
        heads_out = a(h, c.g)
        want = pkg.ops.graph_attention(a.Q(h), a.K(h), a.V(h), c.g, 4)
    assert heads_out.shape == (c.n, 4, H // 4)
    assert torch.equal(heads_out.reshape(c.n, H), want)


# ---------------------------------------------------------------------------
# 5: dropout
# ---------------------------------------------------------------------------
def test_dropout_draws(pkg, case, dev):
    c = case("mols")
    layer = make_layer(pkg, dev, 4, 8, True)
    h = torch.randn(c.n, H, generator=torch.Generator().manual_seed(3)).to(dev)

    def keep():
        with torch.no_grad():
            return pkg.ops.gt_layer(h, c.g, layer, return_aux=True)[1]["keep"]

    st = pkg.ops.seed_dropout(dev, 99)
    k1 = keep()
    assert st.tolist() == [99, 1]  # the launch advanced the offset
    k2 = keep()
    assert st.tolist() == [99, 2]
    rate = k1.float().mean().item()
    bound = 6.0 * (0.25 / (c.n * F2)) ** 0.5
    print(f"keep rate {rate:.5f} (N = {c.n}, bound +-{bound:.5f})")
    assert abs(rate - 0.5) <= bound
    rows = k1.sum(1)
    assert int(rows.min()) > 0 and int(rows.max()) < F2  # no row all dropped / all kept
    assert not torch.equal(k1, k2)
    pkg.ops.seed_dropout(dev, 99)
    assert torch.equal(keep(), k1) and torch.equal(keep(), k2)  # reseeding reproduces both
    # eval draws nothing
    layer.eval()
    before = st.clone()
    k3 = keep()
    assert bool(k3.all()) and torch.equal(st, before)
    # the compression noise state is not touched by a Transformer forward
    noise = pkg.ops.seed_noise(dev, 7, 3)
    enc = make_encoder(pkg, dev, 4).train()
    with torch.no_grad():
        enc(c.g, torch.randn(c.n, 32, device=dev))
    torch.cuda.synchronize()
    assert noise.tolist() == [7, 3]
    assert st.tolist() == [99, int(before[1]) + len(enc.layers)]


# ---------------------------------------------------------------------------
# 7, 8: capacity mode and capture
# ---------------------------------------------------------------------------
def _encoder_step(pkg, enc, g, h, gout, seed):
    for p in enc.parameters():
        p.grad = None
    h.grad = None
    if seed is not None:
        pkg.ops.seed_dropout(h.device, seed)
    out = enc(g, h)
    out.backward(gout)
    return out


def check_capacity_mode(pkg, dev, gh, capacities, oracle, torch_gemm_bitwise=True):
    """A StaticBatch with spare rows: live rows bitwise the unpadded run's,
    padded rows of out / dx zero, weight gradients bitwise equal.  ``oracle``:
    the capacity run's gradients against fp64 as well.  ``torch_gemm_bitwise``
    off: the two results of torch's own GEMM (see below) within a reordered
    fp32 sum instead, and dh0 at the layer stack's input bitwise."""
    B = gh.batch_size
    n = gh.num_nodes()
    n_cap, e_cap, mgn, caps = capacities
    assert (n_cap + 63) // 64 > (n + 63) // 64  # whole spare tiles, and a partly live one
    static = pkg.graph.StaticBatch(B, n_cap, e_cap, gh.ndata["x"].shape[1], mgn, caps, dev)
    static.load(static.pad(gh))
    g = gh.to(dev)
    gen = torch.Generator().manual_seed(4)
    h_cap = torch.randn(n_cap, 32, generator=gen).to(dev)   # padded rows hold live-looking
    go_cap = torch.randn(n_cap, H, generator=gen).to(dev)   # values: they must not count
    enc = make_encoder(pkg, dev, 2).train()

    h = h_cap[:n].clone().requires_grad_(True)
    out = _encoder_step(pkg, enc, g, h, go_cap[:n].contiguous(), 77)
    grads = {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    dx = h.grad.clone()
    assert len(grads) == 1 + 16 * 5

    hc = h_cap.clone().requires_grad_(True)
    out_c = _encoder_step(pkg, enc, static.graph, hc, go_cap, 77)
    torch.cuda.synchronize()
    assert torch.equal(out_c[:n], out)
    assert torch.count_nonzero(out_c[n:]) == 0 and torch.count_nonzero(hc.grad[n:]) == 0
    differ = {}
    if not torch.equal(hc.grad[:n], dx):
        differ["dx"] = rel_l2(hc.grad[:n].cpu(), dx.cpu())
    for k, p in enc.named_parameters():
        if k not in grads:
            assert p.grad is None, k
        elif not torch.equal(p.grad, grads[k]):
            differ[k] = rel_l2(p.grad.cpu(), grads[k].cpu())
    print(f"n {n} n_cap {n_cap}: not bitwise {differ}")
    if torch_gemm_bitwise:
        assert not differ, differ
    else:
        # ops.gt_encoder's embedding_h is one torch F.linear, forward and
        # backward: dx = dh0 We sums 64 terms and dWe = dh0^T h sums one term
        # per row, in the order of the GEMM kernel that the BLAS library picks
        # for n rows, resp. n_cap.  Two fp32 sums of the same K terms in
        # different orders stay within about sqrt(K) 2^-24 of each other
        # (padded rows add exact zeros); twice that is the bar.  Every
        # gradient the project's own kernels write stays bitwise, and so does
        # dh0, which the layer stack run from a leaf h0 shows below.
        terms = {"dx": 64, "embedding_h.weight": n}
        assert set(differ) <= set(terms), differ
        for k, err in differ.items():
            assert err < 2 * terms[k] ** 0.5 * 2.0 ** -24, (k, err)
        res = []
        with torch.no_grad():
            h0_live = F.linear(h_cap[:n], enc.embedding_h.weight)
        for graph, rows in ((g, n), (static.graph, n_cap)):
            h0 = torch.cat([h0_live, go_cap[n:rows]]).requires_grad_(True)  # live-looking padding
            pkg.ops.seed_dropout(dev, 77)
            x = h0
            for layer in enc.layers:
                x = pkg.ops.gt_layer(x, graph, layer)
            (dh0,) = torch.autograd.grad(x, h0, go_cap[:rows].contiguous())
            res.append((x.detach(), dh0))
        torch.cuda.synchronize()
        (x_e, dh0_e), (x_c, dh0_c) = res
        assert torch.equal(x_e, out) and torch.equal(x_c[:n], out)
        assert torch.equal(dh0_c[:n], dh0_e) and torch.count_nonzero(dh0_c[n:]) == 0
        assert float(dh0_e.abs().max()) > 0

    if oracle:  # not only a self-comparison: the capacity run against fp64
        auxes = []
        pkg.ops.seed_dropout(dev, 77)  # the masks both runs drew, from the chained public op
        with torch.no_grad():
            x = F.linear(h.detach(), enc.embedding_h.weight)
            for layer in enc.layers:
                x, aux = pkg.ops.gt_layer(x, g, layer, return_aux=True)
                auxes.append(aux)
        assert torch.equal(x, out.detach())
        c = EdgeList(*gh.edges())
        c.score_row = score_rows(gh, c)
        pr = ref_params(enc)
        hr = h_cap[:n].cpu().double().requires_grad_(True)
        ref = ref_encoder(pr, "", c, hr, 5, 4, True, [a["keep"].cpu() for a in auxes], auxes)
        ref.backward(go_cap[:n].cpu().double())
        assert rel_err(out_c[:n].detach().cpu(), ref.detach()) < ACT_TOL
        check_grad("dh", hc.grad[:n], hr.grad)
        for k, p in enc.named_parameters():
            if k in grads:
                check_grad(k, p.grad, pr[k].grad, pr[k.rsplit(".", 1)[0] + ".weight"].grad)


def test_encoder_capacity_mode(pkg, dev):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(48, "qm9", seed=21))
    check_capacity_mode(pkg, dev, gh, pkg.graph.StaticBatch.capacities([gh], 1, slack=1.3), False)


@pytest.mark.parametrize("split", list(BG.CAPACITY_SPLITS))
def test_encoder_capacity_mode_across_256_tiles(pkg, dev, split):
    """The same assertions with the 256-workgroup line between or behind the
    live tiles (BG.CAPACITY_SPLITS): a workgroup's second tile live, partly
    live or padded, and workgroups that meet padding only.  Tile -> workgroup
    is tile mod 256 in both runs and trailing zero slabs add +0.0 to their
    partition, so the bitwise claim carries over for all 80 gradients of the
    layers' kernels and for dh0.  It does not for the torch F.linear in front
    of them (measured on its first run: embedding_h.weight 2.1e-6 apart at
    16,613 live / 17,112 capacity rows): at these row counts the BLAS library
    picks another kernel for n_cap rows than for n."""
    gh, capacities = BG.capacity_case(pkg, split)
    check_capacity_mode(pkg, dev, gh, capacities, True, torch_gemm_bitwise=False)


def test_encoder_captures(pkg, dev):
    """Forward + backward under torch.cuda.graph: with the dropout seed reset
    before a replay the result is bitwise the eager run's (no host sync on the
    path); a further replay draws a fresh mask (the offset advances in-graph)."""
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(40, "qm9", seed=13))
    g, n = gh.to(dev), gh.num_nodes()
    gen = torch.Generator().manual_seed(6)
    h = torch.randn(n, 32, generator=gen).to(dev).requires_grad_(True)
    gout = torch.randn(n, H, generator=gen).to(dev)
    enc = make_encoder(pkg, dev, 3).train()
    out_e = _encoder_step(pkg, enc, g, h, gout, 555).detach().clone()
    want = {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    dx_e = h.grad.clone()
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up (allocator) off the capture
        _encoder_step(pkg, enc, g, h, gout, None)
    torch.cuda.current_stream().wait_stream(side)
    for p in enc.parameters():
        p.grad = None
    h.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = enc(g, h)
        out_s.backward(gout)

    def replay():
        with torch.no_grad():  # a replay must rewrite every result
            out_s.fill_(float("nan"))
            h.grad.fill_(float("nan"))
            for p in enc.parameters():
                if p.grad is not None:
                    p.grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()

    pkg.ops.seed_dropout(dev, 555)
    torch.cuda.synchronize()
    replay()
    assert torch.equal(out_s.detach(), out_e) and torch.equal(h.grad, dx_e)
    got = {k: p.grad for k, p in enc.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    replay()  # no reseed: the offsets moved on
    assert torch.isfinite(out_s).all() and not torch.equal(out_s.detach(), out_e)
    assert pkg.ops.dropout_state(dev).tolist() == [555, 2 * len(enc.layers)]


# ---------------------------------------------------------------------------
# 9: model level
# ---------------------------------------------------------------------------
B_MODEL = 24


def _args():
    return SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=B_MODEL, gin_layers=5, task="graph_classification")


def _make_model(pkg, wrapped, f_in, dev):
    """A "GIN" model with fresh Transformer encoders installed by attribute."""
    torch.manual_seed(17)
    model = pkg.models.Mainmodel(_args(), f_in, 64, 4, 4, 1, "GIN")
    owners = [model]
    if wrapped:
        model = pkg.models.Mainmodel_continue(_args(), f_in, 64, 4, 4, 1, 1, model, "GIN")
        owners.append(model)
    for o in owners:
        for name in ("Encoder1", "Encoder2"):
            if hasattr(o, name):
                setattr(o, name, pkg.models.Transformer(32, H, 4, 4, dev))
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "Encoder" in k and k.endswith("bias"):
                p.normal_(0.0, 0.1)
            if "compressor.1" in k:
                p.add_(0.2 * torch.randn_like(p))
    model = model.to(dev).train()
    for m in model.modules():
        if isinstance(m, pkg.models.Transformer):
            m.eval()
    return model


def _composed_oracle(model, wrapped, gh, u_gate, u_feat):
    """R.pretrain_forward's composition (fp64) around the fp64 Transformers."""
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
    gf = ref_encoder(p, "Encoder1.", EdgeList(src, dst), h0, 5, 4, False)
    sf = ref_encoder(p, "Encoder2.", EdgeList(es, ed), hs0, 5, 4, False)
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
def test_model_step_matches_composed_oracle(pkg, dev, wrapped):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(B_MODEL, "qm9", seed=31))
    f_in, n = gh.ndata["x"].shape[1], gh.num_nodes()
    gen = torch.Generator().manual_seed(77)
    u_gate, u_feat = torch.rand(n, generator=gen), torch.rand(n, 64, generator=gen)
    model = _make_model(pkg, wrapped, f_in, dev)
    losses_ref, grads_ref = _composed_oracle(copy.deepcopy(model).cpu(), wrapped, gh, u_gate, u_feat)
    g = gh.to(dev)
    x = F.normalize(g.ndata["x"].float())
    _, kl, con, rec = model(g, x, None, None, None, 1, None, 1, dev, B_MODEL,
                            noise=(u_gate.to(dev), u_feat.to(dev)))
    (kl + con + rec).backward()
    torch.cuda.synchronize()
    for name, a, b in zip(("kl", "contrastive", "recon"), (kl, con, rec), losses_ref):
        print(f"Transformer wrapped={wrapped} {name}: {a.item():.8g} vs {b:.8g}")
        assert rel_err(a.item(), b) < LOSS_TOL, (name, a.item(), b)
    params = dict(model.named_parameters())
    inner = "model." if wrapped else ""
    enc_keys = [k for k in grads_ref if k.startswith((inner + "Encoder", "transfer_d."))]
    assert any("Encoder1" in k for k in enc_keys) and any("Encoder2" in k for k in enc_keys)
    errs = check_grads_model({k: grads_ref[k] for k in enc_keys}, lambda k: params[k].grad,
                             cancelled=CANCELLED + CANCELLED_GT)
    worst = max(errs, key=errs.get)
    print(f"worst gradient tensor: {worst} rel_l2 {errs[worst]:.2e}")
    for e in ("Encoder1", "Encoder2"):
        for i in range(5):
            for u in UNUSED:
                k = f"{inner}{e}.layers.{i}.{u}weight"
                assert params[k].grad is None and k not in grads_ref, k
    # one optimizer step (skips the missing gradients)
    before = {k: p.detach().clone() for k, p in params.items()}
    opt = pkg.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-5)
    opt.step()
    torch.cuda.synchronize()
    for k, p in params.items():
        assert torch.isfinite(p).all(), k
        if p.grad is None:
            assert torch.equal(p, before[k]), k
    k = inner + "Encoder1.layers.0.O.bias"
    assert not torch.equal(params[k], before[k])


# ---------------------------------------------------------------------------
# 10: refusals
# ---------------------------------------------------------------------------
def test_refusals(pkg, case, dev):
    c = case("mols")
    E = pkg._lib.ScgibError
    x = torch.randn(c.n, H, device=dev)
    with pytest.raises(E):
        pkg.ops.graph_attention(x, x, x, c.g, 3)
    layer = pkg.models.GraphTransformerLayer(H, H, 4).to(dev)
    layer.num_heads = 3
    with pytest.raises(E):
        pkg.ops.gt_layer(x, c.g, layer)
    x48 = torch.randn(c.n, 48, device=dev)
    with pytest.raises(E):
        pkg.ops.graph_attention(x48, x48, x48, c.g, 4)
    with pytest.raises(E):
        pkg.ops.gt_layer(x48, c.g, pkg.models.GraphTransformerLayer(H, H, 4).to(dev))
    with pytest.raises(E):  # the C entry point itself refuses the head count
        pkg._lib.call("scgib_gt_attn_fwd", None, None, None, None, None, 4, 3, None, None, None,
                      None, None)
    xc = x.cpu()
    with pytest.raises(E):
        pkg.ops.graph_attention(xc, xc, xc, c.g, 4)
    with pytest.raises(E):
        pkg.ops.gt_layer(xc, c.g, pkg.models.GraphTransformerLayer(H, H, 4).to(dev))
    with pytest.raises(E):
        pkg.ops.gt_encoder(torch.randn(c.n, 32), c.g, pkg.models.Transformer(32, H, 1, 4, dev).to(dev))
