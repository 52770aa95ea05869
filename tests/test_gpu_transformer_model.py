"""encoder="Transformer" as a model option on the folded entry
(csrc/gt_embed.hip, ops.gt_embed / ops.gt_encoder_x, models.GT_FOLD): the embed
kernels against fp64, the one-node encoder against the chained public ops bit
for bit, frozen layers, the training step against the composed fp64 oracle
with the dropout masks of both lanes restated from the Philox reference,
reproducible captured training, the fine-tune / domain-adaptation classes and
the refusals.

Tolerances are tests/test_gpu_transformer.py's: activations rel_err < 1e-4,
each gradient tensor rel_l2 < 1e-3, losses within 1e-4, and
conftest.check_grads_model's defaults for whole-model gradients.
"""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import philox_ref
from conftest import CANCELLED, check_grads_model, rel_err, rel_l2
from oracle import egonet
from oracle import scgib_ref as R
from test_gpu_transformer import (ACT_TOL, CANCELLED_GT, GRAD_TOL, HAND, LOSS_TOL, UNUSED, EdgeList,
                                  ref_encoder)

pytestmark = pytest.mark.gpu

H, F2, T = 64, 128, 32
USED = ("attention.Q.", "attention.K.", "attention.V.", "O.", "layer_norm1.", "layer_norm2.",
        "FFN_layer1.", "FFN_layer2.")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def all_encoder_strings(pkg, monkeypatch):
    monkeypatch.setattr(pkg.models, "ALL_ENCODER_STRINGS", True)


class CallCounter:
    """Counts _lib.call by entry point (the ops look the function up per call)."""

    def __init__(self, pkg, monkeypatch):
        self.n = {}
        real = pkg._lib.call

        def call(name, *args):
            self.n[name] = self.n.get(name, 0) + 1
            return real(name, *args)

        monkeypatch.setattr(pkg._lib, "call", call)

    def reset(self):
        self.n.clear()

    def __getitem__(self, name):
        return self.n.get(name, 0)


# ---------------------------------------------------------------------------
# 1, 2: the embed op
# ---------------------------------------------------------------------------
def embed_inputs(n, f, mapped, seed, rows_x=None):
    gen = torch.Generator().manual_seed(seed)
    if rows_x is None:
        rows_x = max(3, (2 * n) // 3 + 2) if mapped else n
    x = torch.randn(rows_x, f, generator=gen)
    wt = torch.randn(T, f, generator=gen) * f ** -0.5
    we = torch.randn(H, T, generator=gen) * T ** -0.5
    gout = torch.randn(n, H, generator=gen)
    # repeated and out-of-order parents
    nmap = torch.randint(0, rows_x, (n,), generator=gen).int() if mapped else None
    return x, wt, we, gout, nmap


def run_embed(pkg, dev, x, wt, we, gout, nmap, dims=None):
    lw = [t.to(dev).requires_grad_(True) for t in (wt, we)]
    h0 = pkg.ops.gt_embed(x.to(dev), lw[0], lw[1], None if nmap is None else nmap.to(dev), dims)
    h0.backward(gout.to(dev))
    torch.cuda.synchronize()
    return h0.detach(), lw[0].grad, lw[1].grad


def ref_embed(x, wt, we, gout, nmap):
    lw = [t.double().requires_grad_(True) for t in (wt, we)]
    xs = x.double() if nmap is None else x.double()[nmap.long()]
    h0 = (xs @ lw[0].T) @ lw[1].T
    h0.backward(gout.double())
    return h0.detach(), lw[0].grad, lw[1].grad


def check_embed(pkg, dev, n, f, mapped, seed):
    inputs = embed_inputs(n, f, mapped, seed)
    if mapped:
        assert inputs[0].shape[0] != n
    h0, dwt, dwe = run_embed(pkg, dev, *inputs)
    r0, rwt, rwe = ref_embed(*inputs)
    assert h0.shape == (n, H) and dwt.shape == (T, f) and dwe.shape == (H, T)
    assert rel_err(h0.cpu(), r0) < ACT_TOL
    assert rel_l2(dwt.cpu(), rwt) < GRAD_TOL and rel_l2(dwe.cpu(), rwe) < GRAD_TOL


@pytest.mark.parametrize("mapped", [False, True], ids=["identity", "mapped"])
@pytest.mark.parametrize("f", [1, 9, 11, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_embed_matches_fp64(pkg, dev, n, f, mapped):
    check_embed(pkg, dev, n, f, mapped, 100 * n + f)


@pytest.mark.parametrize("n", [256 * 64, 257 * 64 + 5], ids=["one_tile_each", "second_tile_partial"])
def test_embed_more_tiles_than_workgroups(pkg, dev, n):
    """The backward runs at most 256 workgroups: at 258 tiles two of them walk
    a second tile and the last tile holds 5 rows; 256 tiles beside it."""
    assert pkg._lib.query("scgib_gt_embed_slabs", n) == 256
    check_embed(pkg, dev, n, 11, False, 7)


@pytest.mark.parametrize("mapped", [False, True], ids=["identity", "mapped"])
def test_embed_capacity_mode(pkg, dev, mapped):
    n, cap = 70, 192
    x, wt, we, gout, nmap = embed_inputs(cap, 11, mapped, 5, rows_x=cap if not mapped else 50)
    dims = torch.tensor([n], dtype=torch.int32, device=dev)
    # the padded rows hold live-looking values: they must not count
    h_c, dwt_c, dwe_c = run_embed(pkg, dev, x, wt, we, gout, nmap, dims)
    h_e, dwt_e, dwe_e = run_embed(pkg, dev, x if mapped else x[:n], wt, we, gout[:n].contiguous(),
                                  None if nmap is None else nmap[:n].contiguous())
    assert h_c.shape == (cap, H)
    assert torch.equal(h_c[:n], h_e) and torch.count_nonzero(h_c[n:]) == 0
    assert torch.equal(dwt_c, dwt_e) and torch.equal(dwe_c, dwe_e)
    assert float(dwt_e.abs().max()) > 0 and float(dwe_e.abs().max()) > 0


# ---------------------------------------------------------------------------
# 3: gt_encoder_x is the chained path, bit for bit
# ---------------------------------------------------------------------------
B_MODEL = 24


def mol_batch(pkg, b=B_MODEL, seed=31):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(b, "qm9", seed=seed))
    return gh


def make_encoder(pkg, dev, seed, layers=4, heads=4):
    torch.manual_seed(seed)
    enc = pkg.models.Transformer(T, H, layers, heads, dev)
    with torch.no_grad():
        for k, p in enc.named_parameters():
            if k.endswith("bias"):
                p.normal_(0.0, 0.2)
    return enc.to(dev).train()


def encoder_case(pkg, dev, name):
    """(graph, x, node_map, readout) of a test graph."""
    gen = torch.Generator().manual_seed(3)
    if name in ("mols", "ego"):
        g = mol_batch(pkg).to(dev)
        x = F.normalize(g.ndata["x"].float())
        if name == "mols":
            return g, x, None, None
        ego = pkg.graph.egonet_batch(g, 1)
        return ego, x, ego.ndata["_ID"], (ego.graph_ptr, ego.batch_size, ego.seg_dims)
    src, dst, n = HAND[name]
    g = pkg.graph.GraphBatch.from_edges(src, dst, n, symmetric_hint=False).to(dev)
    return g, torch.randn(n, 11, generator=gen).to(dev), None, None


def grads_of(enc, td):
    out = {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    out["transfer_d.weight"] = td.weight.grad.clone()
    for p in list(enc.parameters()) + [td.weight]:
        p.grad = None
    return out


@pytest.mark.parametrize("name", ["mols", "ego"] + list(HAND))
def test_encoder_x_is_the_chained_path(pkg, dev, name, monkeypatch):
    ops = pkg.ops
    g, x, nmap, readout = encoder_case(pkg, dev, name)
    n = g.num_nodes()
    enc = make_encoder(pkg, dev, 2)
    L = len(enc.layers)
    torch.manual_seed(4)
    td = torch.nn.Linear(x.shape[1], T, bias=False).to(dev)
    gen = torch.Generator().manual_seed(8)
    masks = [(torch.rand(n, F2, generator=gen) < 0.5).to(dev) for _ in range(L)]
    gout = torch.randn(n, H, generator=gen).to(dev)
    gro = torch.randn(readout[1], H, generator=gen).to(dev) if readout else None

    h = ops.gt_embed(x, td.weight, enc.embedding_h.weight, nmap)
    for layer, m in zip(enc.layers, masks):
        h = ops.gt_layer(h, g, layer, m)
    if readout:
        ro = ops.segment_sum(h, *readout)
        torch.autograd.backward([h, ro], [gout, gro])
    else:
        h.backward(gout)
    want = grads_of(enc, td)
    assert len(want) == 16 * L + 2

    counter = CallCounter(pkg, monkeypatch)
    res = ops.gt_encoder_x(x, g, enc, td, nmap, readout=readout, drop_masks=masks)
    assert counter["scgib_gt_embed_fwd"] == 1
    counter.reset()
    if readout:
        out, ro_x = res
        assert torch.equal(ro_x, ro) and torch.equal(ro_x, ops.segment_sum(out.detach(), *readout))
        counter.reset()
        torch.autograd.backward([out, ro_x], [gout, gro])
    else:
        out = res
        out.backward(gout)
    torch.cuda.synchronize()
    assert counter["scgib_gt_embed_bwd"] == 1
    assert 1 <= counter["scgib_slab_reduce_multi_ex"] <= -(-(4 * L + 2) // 16)
    assert counter["scgib_gt_ffn_bwd"] == L
    assert torch.equal(out, h)
    got = grads_of(enc, td)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ---------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------
def _args(b=B_MODEL):
    return SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=b, gin_layers=5, task="graph_classification")


def make_model(pkg, wrapped, f_in, dev, b=B_MODEL):
    torch.manual_seed(17)
    model = pkg.models.Mainmodel(_args(b), f_in, 64, 4, 4, 1, "Transformer")
    if wrapped:
        model = pkg.models.Mainmodel_continue(_args(b), f_in, 64, 4, 4, 1, 1, model, "Transformer")
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "Encoder" in k and k.endswith("bias"):
                p.normal_(0.0, 0.1)
            if "compressor.1" in k:
                p.add_(0.2 * torch.randn_like(p))
    return model.to(dev).train()


def step_inputs(pkg, dev, b=B_MODEL, seed=31):
    gh = mol_batch(pkg, b, seed)
    n = gh.num_nodes()
    gen = torch.Generator().manual_seed(77)
    u_gate, u_feat = torch.rand(n, generator=gen), torch.rand(n, 64, generator=gen)
    g = gh.to(dev)
    return gh, g, F.normalize(g.ndata["x"].float()), u_gate, u_feat


def run_step(model, g, x, noise, dev, b=B_MODEL):
    model.zero_grad(set_to_none=True)
    _, kl, con, rec = model(g, x, None, None, None, 1, None, 1, dev, b, noise=noise)
    (kl + con + rec).backward()
    torch.cuda.synchronize()
    return [kl.item(), con.item(), rec.item()]


def seed_lanes(pkg, dev):
    pkg.ops.seed_dropout(dev, 99, 0, lane=0)
    pkg.ops.seed_dropout(dev, 1234, 7, lane=1)


# ---------------------------------------------------------------------------
# 4: frozen layers
# ---------------------------------------------------------------------------
def test_frozen_layers(pkg, dev, monkeypatch):
    gh, g, x, u_gate, u_feat = step_inputs(pkg, dev)
    noise = (u_gate.to(dev), u_feat.to(dev))
    model = make_model(pkg, False, x.shape[1], dev)
    counter = CallCounter(pkg, monkeypatch)

    seed_lanes(pkg, dev)
    run_step(model, g, x, noise, dev)
    full = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    assert counter["scgib_gt_embed_bwd"] == 2 and counter["scgib_gt_ffn_bwd"] == 10

    pkg.models.freeze_like_reference(model)
    model.transfer_d.weight.requires_grad = True
    want = {f"{e}.layers.2.{u}{t}" for e in ("Encoder1", "Encoder2") for u in USED
            for t in ("weight", "bias")} | {"transfer_d.weight"}
    counter.reset()
    seed_lanes(pkg, dev)
    run_step(model, g, x, noise, dev)
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(got) == want
    for k in want:
        assert torch.equal(got[k], full[k]), k
    # transfer_d trains: the chain runs down to the embed, one reduce per encoder
    assert counter["scgib_gt_embed_bwd"] == 2 and counter["scgib_gt_ffn_bwd"] == 10

    model.transfer_d.weight.requires_grad = False
    counter.reset()
    seed_lanes(pkg, dev)
    run_step(model, g, x, noise, dev)
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(got) == want - {"transfer_d.weight"}
    for k in got:
        assert torch.equal(got[k], full[k]), k
    # the chains stop at layer 2: layers 4, 3, 2 of both encoders, no embed backward
    assert counter["scgib_gt_embed_bwd"] == 0
    for name in ("scgib_gt_ffn_bwd", "scgib_gt_out_bwd", "scgib_gt_attn_bwd", "scgib_gt_qkv_bwd"):
        assert counter[name] == 6, name


# ---------------------------------------------------------------------------
# 5: the training step against the composed fp64 oracle
# ---------------------------------------------------------------------------
def composed_oracle(model, wrapped, gh, u_gate, u_feat, ego_ids, training, seeds=None):
    """R.pretrain_forward's composition (fp64) around the fp64 Transformers;
    training: layer i of Encoder1 keeps philox_ref.dropout_keep(seed1, off1 + i)
    over the batch's rows, of Encoder2 (seed2, off2 + i) over the ego rows."""
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
    # the masks are per row: the oracle's ego rows are the device batch's, in order
    assert np.array_equal(nodes, ego_ids.cpu().numpy())
    off = np.repeat(np.concatenate([[0], np.cumsum(sizes)[:-1]]), ecount)
    src, dst = gh.edges()
    counts = torch.from_numpy(gh.batch_num_nodes_host())
    es, ed = torch.from_numpy(esrc + off), torch.from_numpy(edst + off)
    x = F.normalize(gh.ndata["x"].double())
    xs = x[torch.from_numpy(nodes)]
    n, n_ego = x.shape[0], xs.shape[0]
    keeps1 = keeps2 = None
    if training:
        (s1, o1), (s2, o2) = seeds
        keeps1 = [torch.from_numpy(philox_ref.dropout_keep(s1, o1 + i, np.arange(n))) for i in range(5)]
        keeps2 = [torch.from_numpy(philox_ref.dropout_keep(s2, o2 + i, np.arange(n_ego)))
                  for i in range(5)]
    h0 = R._linear(x, p, "transfer_d", bias=False)
    hs0 = R._linear(xs, p, "transfer_d", bias=False)
    gf = ref_encoder(p, "Encoder1.", EdgeList(src, dst), h0, 5, 4, training, keeps1)
    sf = ref_encoder(p, "Encoder2.", EdgeList(es, ed), hs0, 5, 4, training, keeps2)
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
def test_training_step_matches_composed_oracle(pkg, dev, wrapped, monkeypatch):
    gh, g, x, u_gate, u_feat = step_inputs(pkg, dev)
    model = make_model(pkg, wrapped, x.shape[1], dev)
    assert all(m.training for m in model.modules() if isinstance(m, pkg.models.Transformer))
    ego_ids = pkg.graph.egonet_batch(g, 1).ndata["_ID"]
    losses_ref, grads_ref = composed_oracle(copy.deepcopy(model).cpu(), wrapped, gh, u_gate, u_feat,
                                            ego_ids, True, ((99, 0), (1234, 7)))
    counter = CallCounter(pkg, monkeypatch)
    seed_lanes(pkg, dev)
    losses = run_step(model, g, x, (u_gate.to(dev), u_feat.to(dev)), dev)
    assert counter["scgib_gt_embed_fwd"] == 2
    assert pkg.ops.dropout_state(dev, 0).tolist() == [99, 5]
    assert pkg.ops.dropout_state(dev, 1).tolist() == [1234, 12]
    for name, a, b in zip(("kl", "contrastive", "recon"), losses, losses_ref):
        print(f"Transformer training wrapped={wrapped} {name}: {a:.8g} vs {b:.8g}")
        assert rel_err(a, b) < LOSS_TOL, (name, a, b)
    params = dict(model.named_parameters())
    inner = "model." if wrapped else ""
    enc_keys = [k for k in grads_ref if k.startswith((inner + "Encoder", "transfer_d."))]
    assert any("Encoder1" in k for k in enc_keys) and any("Encoder2" in k for k in enc_keys)
    assert "transfer_d.weight" in enc_keys
    errs = check_grads_model({k: grads_ref[k] for k in enc_keys}, lambda k: params[k].grad,
                             cancelled=CANCELLED + CANCELLED_GT)
    worst = max(errs, key=errs.get)
    print(f"worst gradient tensor: {worst} rel_l2 {errs[worst]:.2e}")
    for e in ("Encoder1", "Encoder2"):
        for i in range(5):
            for u in UNUSED:
                k = f"{inner}{e}.layers.{i}.{u}weight"
                assert params[k].grad is None and k not in grads_ref, k


# ---------------------------------------------------------------------------
# 6: GT_FOLD off gives the same step within tolerance
# ---------------------------------------------------------------------------
def test_fold_off_is_the_same_step(pkg, dev, monkeypatch):
    gh, g, x, u_gate, u_feat = step_inputs(pkg, dev)
    noise = (u_gate.to(dev), u_feat.to(dev))
    model = make_model(pkg, True, x.shape[1], dev)
    for m in model.modules():
        if isinstance(m, pkg.models.Transformer):
            m.eval()
    counter = CallCounter(pkg, monkeypatch)
    monkeypatch.setattr(pkg.models, "GT_FOLD", False)
    off = run_step(model, g, x, noise, dev)
    assert counter["scgib_gt_embed_fwd"] == 0
    g_off = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()
             if p.grad is not None}
    monkeypatch.setattr(pkg.models, "GT_FOLD", True)
    on = run_step(model, g, x, noise, dev)
    assert counter["scgib_gt_embed_fwd"] == 2
    params = dict(model.named_parameters())
    assert {k for k, p in params.items() if p.grad is not None} == set(g_off)
    for name, a, b in zip(("kl", "contrastive", "recon"), on, off):
        assert rel_err(a, b) < LOSS_TOL, (name, a, b)
    keys = [k for k in g_off if k.startswith(("model.Encoder", "transfer_d."))]
    assert len(keys) == 2 * (16 * 5 + 1) + 1
    check_grads_model({k: g_off[k] for k in keys}, lambda k: params[k].grad,
                      cancelled=CANCELLED + CANCELLED_GT)


# ---------------------------------------------------------------------------
# 7: reproducible captured training
# ---------------------------------------------------------------------------
def test_captured_training_is_reproducible(pkg, dev, monkeypatch):
    from test_gpu_graph_split import _assert_bitwise, _state
    ops = pkg.ops
    monkeypatch.setattr(pkg.models, "FORK_ENCODERS", True)
    gh, g, x, _, _ = step_inputs(pkg, dev)
    one = torch.ones((), device=dev)

    def seed_all():
        ops.seed_noise(dev, 4242, 0)
        seed_lanes(pkg, dev)
        torch.cuda.synchronize()

    def capture():
        model = make_model(pkg, True, x.shape[1], dev)
        opt = pkg.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-5)

        def body():
            _, kl, con, rec = model(g, x, None, None, None, 1, None, 1, dev, B_MODEL)
            torch.autograd.backward((kl, rec, con), (one, one, one))
            opt.step()
            return torch.stack([kl.detach(), con.detach(), rec.detach()])

        seed_all()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up (allocator, Adam state) off the capture
            opt.zero_grad(set_to_none=True)
            body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        start = _state(model, opt)
        graph = torch.cuda.CUDAGraph()
        opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(graph):
            out = body()
        return model, opt, graph, out, start

    def restore(model, opt, start):
        with torch.no_grad():
            named = dict(model.named_parameters())
            bufs = dict(model.named_buffers())
            for k, v in start.items():
                if k.startswith("buf."):
                    bufs[k[4:]].copy_(v)
                elif k.startswith("opt."):
                    name, field = k[4:].rsplit(".", 1)
                    opt.state[named[name]][field].copy_(v)
                else:
                    named[k].copy_(v)
        seed_all()

    def replay3(graph, out):
        losses = []
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            losses.append(out.clone())
        return torch.stack(losses)

    model, opt, graph, out, start = capture()
    restore(model, opt, start)
    first = replay3(graph, out)
    end = _state(model, opt)
    assert torch.isfinite(first).all()
    assert ops.dropout_state(dev, 0).tolist() == [99, 15]
    assert ops.dropout_state(dev, 1).tolist() == [1234, 7 + 15]
    assert not torch.equal(first[0], first[1])  # the parameters and the masks moved on
    restore(model, opt, start)
    again = replay3(graph, out)
    assert torch.equal(again, first), (again, first)
    _assert_bitwise(_state(model, opt), end)

    # the same step with both chains on one stream: the same draws, the same bits
    monkeypatch.setattr(pkg.models, "FORK_ENCODERS", False)
    model2, opt2, graph2, out2, _ = capture()
    restore(model2, opt2, start)  # the forked run's initial state
    graph2.replay()
    torch.cuda.synchronize()
    assert torch.equal(out2, first[0]), (out2, first[0])


# ---------------------------------------------------------------------------
# 8: fine-tuning and domain adaptation
# ---------------------------------------------------------------------------
B_FT = 8


def ft_step(pkg, ft, g, x, y, dev):
    pkg.ops.seed_noise(dev, 11, 0)
    seed_lanes(pkg, dev)
    ft.zero_grad(set_to_none=True)
    scores = ft(g, x, None, None, 1, None, 1, dev, B_FT)[0]
    loss = ft.loss(scores, y)
    loss.backward()
    torch.cuda.synchronize()
    return scores.detach().clone(), loss.item()


def test_finetuning_on_a_transformer_model(pkg, dev, tmp_path):
    M = pkg.models
    gh, g, x, _, _ = step_inputs(pkg, dev, B_FT, 41)
    f_in = x.shape[1]
    y = (torch.arange(B_FT) % 2).float().view(B_FT, 1).to(dev)
    pre = make_model(pkg, True, f_in, dev, B_FT)
    path = tmp_path / "pre.pt"
    M.save_checkpoint(pre, path, _args(B_FT), in_dim=f_in)

    def build(cp):
        torch.manual_seed(23)
        return M.Mainmodel_finetuning(_args(B_FT), f_in, 64, 4, 4, 1, 1, cp, "Transformer") \
            .to(dev).train()

    ft = build(copy.deepcopy(pre))
    assert type(ft.Encoder1) is M.Transformer
    scores, loss = ft_step(pkg, ft, g, x, y, dev)
    assert scores.shape == (B_FT, 1) and np.isfinite(loss)
    assert torch.isfinite(scores).all() and bool(((scores > 0) & (scores < 1)).all())
    got = {k for k, p in ft.named_parameters() if p.grad is not None}
    head = {k for k, _ in ft.named_parameters()
            if k.startswith(("transfer_d.", "MLP.", "s2s.", "predict."))}
    inner = {f"model.{e}.layers.2.{u}{t}" for e in ("Encoder1", "Encoder2") for u in USED
             for t in ("weight", "bias")}
    assert "transfer_d.weight" in head and len(inner) == 32
    assert got == head | inner, (sorted(got - head - inner), sorted((head | inner) - got))
    for k, p in ft.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), k

    ft_file = build(path)  # the same weights through a save_checkpoint file
    assert type(ft_file.model) is M.Mainmodel_continue
    assert type(ft_file.model.Encoder1) is M.Transformer
    scores_file, _ = ft_step(pkg, ft_file, g, x, y, dev)
    assert torch.equal(scores_file, scores)


def test_domainadapt_around_a_gcn_model(pkg, dev):
    M = pkg.models
    gh, g, x, _, _ = step_inputs(pkg, dev, B_FT, 41)
    f_in = x.shape[1]
    torch.manual_seed(5)
    inner = M.Mainmodel(_args(B_FT), f_in, 64, 4, 4, 1, "GCN")
    da = M.Mainmodel_domainadapt(_args(B_FT), f_in, 64, 4, 4, 1, 1, inner, "GCN").to(dev).train()
    assert type(da.Encoder1) is M.GCN and type(da.model.Encoder1) is M.GCN
    pkg.ops.seed_noise(dev, 3, 0)
    loss = da(g, x, None, None, None, 1, None, 1, dev, B_FT)
    loss.backward()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and np.isfinite(loss.item())
    assert da.model.Encoder1.conv1.weight.grad is not None
    assert torch.isfinite(da.model.Encoder1.conv1.weight.grad).all()


# ---------------------------------------------------------------------------
# 9: refusals
# ---------------------------------------------------------------------------
def test_refusals(pkg, dev):
    E = pkg._lib.ScgibError
    ops = pkg.ops
    g, x, _, _ = encoder_case(pkg, dev, "mols")
    n = g.num_nodes()
    enc = make_encoder(pkg, dev, 1)
    td = torch.nn.Linear(x.shape[1], T, bias=False).to(dev)
    ops.gt_encoder_x(x, g, enc, td)  # the accepted call
    x17 = torch.randn(n, 17, device=dev)
    with pytest.raises(E):
        ops.gt_encoder_x(x17, g, enc, torch.nn.Linear(17, T, bias=False).to(dev))
    with pytest.raises(E):
        ops.gt_embed(x17, torch.randn(T, 17, device=dev), enc.embedding_h.weight)
    with pytest.raises(E):
        ops.gt_encoder_x(x, g, enc, torch.nn.Linear(x.shape[1], T, bias=True).to(dev))
    with pytest.raises(E):
        ops.gt_encoder_x(x.clone().requires_grad_(True), g, enc, td)
    empty = pkg.graph.GraphBatch.from_edges(np.zeros(0, np.int64), np.zeros(0, np.int64), 0,
                                            symmetric_hint=False).to(dev)
    with pytest.raises(E):
        ops.gt_encoder_x(x[:0], empty, enc, td)
    with pytest.raises(E):
        ops.gt_encoder_x(x.cpu(), g, enc, td)
    with pytest.raises(E):  # rows of x without a node_map must be the graph's
        ops.gt_encoder_x(x[: n - 1], g, enc, td)
    with pytest.raises(E):  # an int64 map
        ops.gt_embed(x, td.weight, enc.embedding_h.weight, torch.zeros(n, dtype=torch.int64, device=dev))
    with pytest.raises(E):  # the C entry point itself refuses the feature count
        pkg._lib.call("scgib_gt_embed_fwd", None, 17, 4, None, None, None, 4, None, None, None)
    torch.cuda.synchronize()
