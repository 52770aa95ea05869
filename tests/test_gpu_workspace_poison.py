"""Every device op against the contents of its fresh workspaces (DESIGN.md,
"Workspace contracts").

No kernel allocates: every byte a kernel reads is an input or a tensor that
ops.py / graph.py / metrics.py allocated with torch.empty.  Two contracts hold
the design together and nothing else in the suite tests them:

  1. a kernel writes every element that a later kernel, or the caller, reads;
  2. capacity mode: rows in [n, n_cap) are written as zeros or never read.

Each case runs its op three times through tests/poison.run_thrice -- on clean
memory, with every fresh fp32 / fp64 allocation filled with NaN, and with the
sentinel -7.0 -- and every output, input gradient, parameter gradient and
updated buffer must be torch.equal across the three runs (the reductions are
fixed-order, so the comparison is exact), and finite wherever the clean run
is.  Capacity-mode results are compared over the whole capacity.  Eager only:
replays are pinned against exact mode elsewhere.  Integer workspaces are never
poisoned (tests/poison.py), so a failure here is a wrong number, not a fault.
"""
import copy
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import test_gpu_encoders as ENC
import test_gpu_optim as OPT
import test_gpu_transformer as GT
from poison import assert_same, run_thrice
from test_gpu_parity import rand_graph
from test_gpu_trajectory import _pretrain_model

pytestmark = pytest.mark.gpu

N_MOLS = 40        # ~700 rows: 11 tiles of 64, the last one ragged
TILE = 64
KINDS = ["exact", "cap"]
K_FIN_BLOCKS = 256  # csrc/recon_fin.h kFinBlocks: past it the loss finish is recon_fin_k's launch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def check(build, run):
    results = run_thrice(build, run)
    clean = results[0]
    assert clean and any(v is not None and v.numel() for v in clean.values())
    assert_same(results)
    return clean


# ---------------------------------------------------------------------------
# the two shapes
# ---------------------------------------------------------------------------
_SHAPES = {}


def shape(pkg, dev, kind, k=1, n_mols=N_MOLS, seed=3):
    """The batch every case runs on.  'exact': synth.molecules(40, "qm9"), a
    ragged last tile and more than two tiles.  'cap': the same batch padded
    through StaticBatch.capacities(slack=1.5) as tests/test_gpu_capacity.py
    builds it -- one partly live tile, at least two tiles of padding only."""
    key = (kind, k, n_mols, seed)
    if key in _SHAPES:
        return _SHAPES[key]
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(n_mols, "qm9", seed=seed))
    dict.__setitem__(gh.ndata, "x", F.normalize(gh.ndata["x"].float()))
    n_live = gh.num_nodes()
    s = SimpleNamespace(gh=gh, n_live=n_live, B=gh.batch_size, kind=kind, k=k, static=None)
    if kind == "exact":
        if n_mols == N_MOLS:
            assert n_live % TILE != 0 and n_live > 2 * TILE
        s.g = gh.to(dev)
        s.x = s.g.ndata["x"]
        s.n = n_live
    else:
        n_cap, e_cap, mgn, caps = pkg.graph.StaticBatch.capacities([gh], k, slack=1.5)
        s.static = pkg.graph.StaticBatch(s.B, n_cap, e_cap, gh.ndata["x"].shape[1], mgn, caps,
                                         dev, k=k)
        s.static.load(s.static.pad(gh))
        s.g, s.x, s.n = s.static.graph, s.static.x, n_cap
        live_tiles, cap_tiles = -(-n_live // TILE), -(-n_cap // TILE)
        if n_mols == N_MOLS:
            assert n_live % TILE != 0            # one tile is partly live
            assert cap_tiles - live_tiles >= 2   # at least two tiles are padding only
    ego = pkg.graph.egonet_batch(s.g, k)
    torch.cuda.synchronize()
    s.ego_rows, s.ego_segments = ego.num_nodes(), ego.batch_size
    _SHAPES[key] = s
    return s


def randn(gen, *shape_, dev=None, scale=1.0):
    t = torch.randn(*shape_, generator=gen) * scale
    return t.to(dev) if dev is not None else t


def grads_of(prefix, module, out):
    for k, p in module.named_parameters():
        out[f"{prefix}grad.{k}"] = p.grad
    for k, b in module.named_buffers():
        out[f"{prefix}buf.{k}"] = b
    return out


def perturb_bn(module, gen):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.add_(0.2 * torch.randn(m.weight.shape, generator=gen))
                m.bias.add_(0.2 * torch.randn(m.bias.shape, generator=gen))
                m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))


# ---------------------------------------------------------------------------
# GIN encoder
# ---------------------------------------------------------------------------
GIN_CONFIGS = {
    "defaults": {},
    "agg_free": {"AGG_FREE_MIN_ROWS": 0},
    "recompute_r": {"STORE_R": False},
    "inline_bn": {"DEFER_BN": False, "DEFER_BN_FWD": False},
}


def _gin_base(pkg, d_in, layers, seed):
    torch.manual_seed(seed)
    gin = pkg.models.GIN(d_in, 64, layers)
    lin = torch.nn.Linear(11, 32, bias=False)
    perturb_bn(gin, torch.Generator().manual_seed(seed + 1))
    return gin, lin


def _gin_x_case(pkg, dev, s, training, via_ego, freeze=None):
    gin0, lin0 = _gin_base(pkg, 32, 5, 21)
    if freeze == "reference":
        pkg.models.freeze_like_reference(gin0)
        assert {k.split(".")[1] for k, p in gin0.named_parameters() if p.requires_grad} == {"2"}
    elif freeze == "0-3":
        for k, p in gin0.named_parameters():
            p.requires_grad = k.split(".")[1] == "4"
    rows = s.ego_rows if via_ego else s.n
    w = randn(torch.Generator().manual_seed(22), rows, 64, dev=dev)

    def build():
        return copy.deepcopy(gin0).to(dev).train(training), copy.deepcopy(lin0).to(dev)

    def run(state):
        gin, lin = state
        if via_ego:
            target = pkg.graph.egonet_batch(s.g, s.k)
            nmap = target.ndata["_ID"]
        else:
            target, nmap = s.g, None
        h = pkg.ops.gin_encoder_x(s.x, target, gin, lin, nmap)
        assert h.shape == (rows, 64)
        (h * w).sum().backward()
        return grads_of("gin.", gin, {"h": h, "dwt": lin.weight.grad})

    check(build, run)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("config", list(GIN_CONFIGS))
@pytest.mark.parametrize("via_ego", [False, True], ids=["direct", "via_ego"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_gin_encoder_x(pkg, dev, monkeypatch, training, via_ego, config, kind):
    for name, value in GIN_CONFIGS[config].items():
        monkeypatch.setattr(pkg.ops, name, value)
    _gin_x_case(pkg, dev, shape(pkg, dev, kind), training, via_ego)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("freeze", ["reference", "0-3"])
def test_gin_encoder_x_frozen_layers(pkg, dev, freeze, kind):
    """models.freeze_like_reference (only ginlayers.2 / batch_norms.2 train),
    and layers 0-3 frozen outright: the frozen layers' backward skips dW."""
    _gin_x_case(pkg, dev, shape(pkg, dev, kind), True, True, freeze)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layers", [2, 4])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_gin_encoder_from_h0(pkg, dev, training, layers, kind):
    s = shape(pkg, dev, kind)
    gin0, _ = _gin_base(pkg, 32, layers, 23)
    gen = torch.Generator().manual_seed(24)
    h0, w = randn(gen, s.n, 32, dev=dev), randn(gen, s.n, 64, dev=dev)

    def build():
        return copy.deepcopy(gin0).to(dev).train(training), h0.clone().requires_grad_(True)

    def run(state):
        gin, h = state
        out = pkg.ops.gin_encoder(h, s.g, gin)
        (out * w).sum().backward()
        return grads_of("gin.", gin, {"out": out, "dh0": h.grad})

    check(build, run)


# ---------------------------------------------------------------------------
# encoder pair
# ---------------------------------------------------------------------------
PAIR_GRADS = {"all": ("s", "ro", "f", "t"), "readout_t": ("ro", "t"), "f": ("f",),
              "no_t": ("s", "ro", "f")}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", list(PAIR_GRADS))
@pytest.mark.parametrize("with_lin0", [True, False], ids=["lin0", "nolin0"])
def test_gin_encoder_pair_x(pkg, dev, with_lin0, which, kind):
    s = shape(pkg, dev, kind)
    ego_gin0, lin_t0 = _gin_base(pkg, 32, 5, 31)
    core_gin0, _ = _gin_base(pkg, 32, 5, 32)
    torch.manual_seed(33)
    lin00 = torch.nn.Linear(64, 64)
    gen = torch.Generator().manual_seed(34)
    ws = {"s": randn(gen, s.ego_rows, 64, dev=dev), "ro": randn(gen, s.ego_segments, 64, dev=dev),
          "f": randn(gen, s.n, 64, dev=dev), "t": randn(gen, s.n, 64, dev=dev)}
    side = pkg.models._side_stream(dev)

    def build():
        mods = [copy.deepcopy(m).to(dev).train() for m in (ego_gin0, core_gin0, lin_t0, lin00)]
        return mods

    def run(state):
        ego_gin, core_gin, lin_t, lin0 = state
        ego = pkg.graph.egonet_batch(s.g, 1)
        outs = pkg.ops.gin_encoder_pair_x(s.x, ego, ego_gin, s.g, core_gin, lin_t,
                                          ego.ndata["_ID"], side, lin0 if with_lin0 else None)
        named = dict(zip(("s", "ro", "f", "t"), outs))
        assert ("t" in named) == with_lin0
        loss = sum((named[k] * ws[k]).sum() for k in PAIR_GRADS[which] if k in named)
        loss.backward()
        res = dict(named)
        res["dwt"] = lin_t.weight.grad
        grads_of("ego.", ego_gin, res)
        grads_of("core.", core_gin, res)
        return grads_of("lin0.", lin0, res)

    check(build, run)


# ---------------------------------------------------------------------------
# GCN / GraphSAGE layer, graph attention, Transformer layer and encoder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("mode", sorted(["gcn", "mean"]))
def test_conv_layer(pkg, dev, mode, relu, kind):
    assert set(pkg.ops.CONV_MODES) == {"gcn", "mean"}
    s = shape(pkg, dev, kind)
    wn, wself, b = ENC.make_weights(mode, 32, 64, 41)
    gen = torch.Generator().manual_seed(42)
    x, gout = randn(gen, s.n, 32, dev=dev), randn(gen, s.n, 64, dev=dev)

    def build():
        return [None if t is None else t.clone().to(dev).requires_grad_(True)
                for t in (x, wn, wself, b)]

    def run(leaves):
        out = pkg.ops.conv_layer(leaves[0], s.g, leaves[1], leaves[2], leaves[3], mode, relu)
        out.backward(gout)
        res = {"out": out}
        for name, t in zip(("dx", "dwn", "dws", "db"), leaves):
            res[name] = None if t is None else t.grad
        return res

    check(build, run)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["GCN", "GraphSAGE"])
def test_conv_encoder(pkg, dev, name, kind):
    s = shape(pkg, dev, kind)
    enc0 = ENC.make_encoder(pkg, name, 43)
    gen = torch.Generator().manual_seed(44)
    h0, gout = randn(gen, s.n, 32, dev=dev), randn(gen, s.n, 64, dev=dev)

    def build():
        return copy.deepcopy(enc0).to(dev), h0.clone().requires_grad_(True)

    def run(state):
        enc, h = state
        out = enc(s.g, h)
        out.backward(gout)
        return grads_of("enc.", enc, {"out": out, "dh": h.grad})

    check(build, run)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("heads", [1, 2, 4, 8, 16])
def test_graph_attention(pkg, dev, heads, kind):
    assert tuple(pkg.ops.GT_HEADS) == (1, 2, 4, 8, 16)
    s = shape(pkg, dev, kind)
    gen = torch.Generator().manual_seed(45 + heads)
    q, k, v, gout = (randn(gen, s.n, 64, dev=dev) for _ in range(4))

    def build():
        return [t.clone().requires_grad_(True) for t in (q, k, v)]

    def run(leaves):
        attn, score = pkg.ops.graph_attention(*leaves, s.g, heads, return_score=True)
        attn.backward(gout)
        return {"attn": attn, "score": score, "dq": leaves[0].grad, "dk": leaves[1].grad,
                "dv": leaves[2].grad}

    check(build, run)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("training", [True, False], ids=["dropout", "eval"])
def test_gt_layer(pkg, dev, training, kind):
    s = shape(pkg, dev, kind)
    layer0 = GT.make_layer(pkg, torch.device("cpu"), 4, 51, training)
    gen = torch.Generator().manual_seed(52)
    h0, gout = randn(gen, s.n, 64, dev=dev), randn(gen, s.n, 64, dev=dev)

    def build():
        pkg.ops.seed_dropout(dev, 4242)
        return copy.deepcopy(layer0).to(dev).train(training), h0.clone().requires_grad_(True)

    def run(state):
        layer, h = state
        out = pkg.ops.gt_layer(h, s.g, layer)
        out.backward(gout)
        res = grads_of("layer.", layer, {"out": out, "dh": h.grad})
        res["dropout_state"] = pkg.ops.dropout_state(dev)
        return res

    check(build, run)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("via_ego", [False, True], ids=["direct", "via_ego_readout"])
def test_gt_encoder_x(pkg, dev, via_ego, kind):
    s = shape(pkg, dev, kind)
    enc0 = GT.make_encoder(pkg, torch.device("cpu"), 53)
    torch.manual_seed(54)
    lin0 = torch.nn.Linear(11, 32, bias=False)
    gen = torch.Generator().manual_seed(55)
    rows = s.ego_rows if via_ego else s.n
    w, wro = randn(gen, rows, 64, dev=dev), randn(gen, s.ego_segments, 64, dev=dev)

    def build():
        pkg.ops.seed_dropout(dev, 777, lane=0)
        pkg.ops.seed_dropout(dev, 778, lane=1)
        return copy.deepcopy(enc0).to(dev).train(), copy.deepcopy(lin0).to(dev)

    def run(state):
        enc, lin = state
        res = {}
        if via_ego:
            ego = pkg.graph.egonet_batch(s.g, 1)
            out, ro = pkg.ops.gt_encoder_x(s.x, ego, enc, lin, ego.ndata["_ID"],
                                           readout=(ego.graph_ptr, ego.batch_size, ego.seg_dims),
                                           lane=1)
            ((out * w).sum() + (ro * wro).sum()).backward()
            res["readout"] = ro
        else:
            out = pkg.ops.gt_encoder_x(s.x, s.g, enc, lin)
            (out * w).sum().backward()
        res.update(out=out, dwt=lin.weight.grad)
        return grads_of("enc.", enc, res)

    check(build, run)


# ---------------------------------------------------------------------------
# interaction
# ---------------------------------------------------------------------------
def _interaction_modules(seed):
    torch.manual_seed(seed)
    comp = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.BatchNorm1d(64),
                               torch.nn.ReLU(), torch.nn.Linear(64, 1))
    attn = torch.nn.Linear(128, 1)
    perturb_bn(comp, torch.Generator().manual_seed(seed + 1))
    return comp, attn


INTERACTION_GRADS = {"all": ("im", "z1", "z2", "kl", "kl_mean"), "im": ("im",),
                     "kl": ("kl", "kl_mean")}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", list(INTERACTION_GRADS))
@pytest.mark.parametrize("use_att", [True, False], ids=["att", "noatt"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("op", ["interaction", "interaction_lin"])
def test_interaction(pkg, dev, op, training, use_att, which, kind):
    """``which`` = 'kl': gradients into the KL tensor and its mean only, so
    g_im is the buffer _interaction_backward zero-fills itself.  Capacity mode
    has no KL tensor (kl is empty): there the case is the mean alone."""
    s = shape(pkg, dev, kind)
    comp0, attn0 = _interaction_modules(61)
    gen = torch.Generator().manual_seed(62)
    f0, s0 = randn(gen, s.n, 64, dev=dev), randn(gen, s.n, 64, dev=dev)
    u_gate = torch.rand(s.n, generator=gen).to(dev)
    u_feat = torch.rand(s.n, 64, generator=gen).to(dev)
    n_last = int(s.gh.batch_num_nodes_host()[-1])
    ws = {"im": randn(gen, s.n, 128, dev=dev), "z1": randn(gen, s.B, 64, dev=dev),
          "z2": randn(gen, s.B, 64, dev=dev), "kl": randn(gen, 2 * n_last, 64, dev=dev),
          "kl_mean": randn(gen, 1, dev=dev)[0]}

    def build():
        return (copy.deepcopy(comp0).to(dev).train(training), copy.deepcopy(attn0).to(dev),
                f0.clone().requires_grad_(True), s0.clone().requires_grad_(True))

    def run(state):
        comp, attn, fd, sd = state
        if op == "interaction":
            outs = pkg.ops.interaction(fd, comp[0](fd), sd, u_gate, u_feat, comp[1], comp[3],
                                       attn, s.g, training, use_att)
        else:
            outs = pkg.ops.interaction_lin(fd, sd, u_gate, u_feat, comp, attn, s.g, training,
                                           use_att)
        named = dict(zip(("im", "z1", "z2", "kl", "kl_mean"), outs))
        assert named["kl"].shape[0] == (0 if kind == "cap" else 2 * n_last)
        loss = sum((named[k] * ws[k]).sum() for k in INTERACTION_GRADS[which]
                   if named[k].numel())
        loss.backward()
        res = dict(named)
        res.update(df=fd.grad, ds=sd.grad)
        grads_of("comp.", comp, res)
        return grads_of("attn.", attn, res)

    clean = check(build, run)
    if not use_att:
        assert clean["attn.grad.weight"] is None


# ---------------------------------------------------------------------------
# readouts and losses
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [64, 9])
def test_segment_sum(pkg, dev, dim, kind):
    """The graph readout (sum_nodes_graph) and the ego-net readout, whose
    segment count is a device value in capacity mode (ego.seg_dims).  The
    graph readout of a capacity batch has a fixed segment count and no dims:
    its backward must still write the padded rows (segment_broadcast_k left
    them unwritten at float4 widths before this file existed)."""
    s = shape(pkg, dev, kind)
    gen = torch.Generator().manual_seed(71)
    x0, xe0 = randn(gen, s.n, dim, dev=dev), randn(gen, s.ego_rows, dim, dev=dev)
    gy, gye = randn(gen, s.B, dim, dev=dev), randn(gen, s.ego_segments, dim, dev=dev)

    def build():
        return x0.clone().requires_grad_(True), xe0.clone().requires_grad_(True)

    def run(state):
        x, xe = state
        ego = pkg.graph.egonet_batch(s.g, 1)
        y = pkg.ops.sum_nodes_graph(s.g, x)
        ye = pkg.ops.segment_sum(xe, ego.graph_ptr, ego.batch_size, ego.seg_dims)
        y.backward(gy)
        ye.backward(gye)
        return {"y": y, "ye": ye, "dx": x.grad, "dxe": xe.grad}

    check(build, run)


@pytest.mark.parametrize("pair", [False, True], ids=["set2set", "set2set_pair"])
def test_set2set(pkg, dev, pair):
    s = shape(pkg, dev, "exact")
    torch.manual_seed(72)
    s2s0 = pkg.models.Set2Set(64, 2, 1)
    gen = torch.Generator().manual_seed(73)
    xa0, xb0 = randn(gen, s.n, 64, dev=dev), randn(gen, s.n, 64, dev=dev)
    ga, gb = randn(gen, s.B, 128, dev=dev), randn(gen, s.B, 128, dev=dev)

    def build():
        return (copy.deepcopy(s2s0).to(dev), xa0.clone().requires_grad_(True),
                xb0.clone().requires_grad_(True))

    def run(state):
        s2s, xa, xb = state
        assert s2s.n_iters == 2
        if pair:
            ya, yb = pkg.ops.set2set_pair(xa, xb, s.g, s2s.lstm, s2s.n_iters)
            ((ya * ga).sum() + (yb * gb).sum()).backward()
            res = {"ya": ya, "yb": yb, "dxa": xa.grad, "dxb": xb.grad}
        else:
            ya = pkg.ops.set2set(xa, s.g, s2s.lstm, s2s.n_iters)
            ya.backward(ga)
            res = {"ya": ya, "dxa": xa.grad}
        return grads_of("s2s.", s2s, res)

    check(build, run)


@pytest.mark.parametrize("width", [64, 128])
def test_contrastive(pkg, dev, width):
    assert tuple(pkg.ops.CONTRAST_WIDTHS) == (64, 128)
    gen = torch.Generator().manual_seed(74)
    z10, z20 = randn(gen, 100, width, dev=dev), randn(gen, 100, width, dev=dev)

    def build():
        return z10.clone().requires_grad_(True), z20.clone().requires_grad_(True)

    def run(state):
        z1, z2 = state
        loss = pkg.ops.contrastive(z1, z2)
        (3.0 * loss).backward()
        return {"loss": loss, "dz1": z1.grad, "dz2": z2.grad}

    check(build, run)


def _mlp(d_in, seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(d_in, 64), torch.nn.ReLU(),
                               torch.nn.Linear(64, 64))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d_in", [128, 64])
def test_mlp2(pkg, dev, d_in, kind):
    s = shape(pkg, dev, kind)
    mlp0 = _mlp(d_in, 75)
    gen = torch.Generator().manual_seed(76)
    x0, gout = randn(gen, s.n, d_in, dev=dev, scale=0.3), randn(gen, s.n, 64, dev=dev)

    def build():
        return copy.deepcopy(mlp0).to(dev), x0.clone().requires_grad_(True)

    def run(state):
        mlp, x = state
        out = pkg.ops.mlp2(x, mlp, s.g.dims)
        out.backward(gout)
        return grads_of("mlp.", mlp, {"out": out, "dx": x.grad})

    check(build, run)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", ["mlp2_recon", "mlp2_recon_contrastive", "recon_adj"])
def test_recon_adj_heads(pkg, dev, op, kind):
    s = shape(pkg, dev, kind)
    mlp0 = _mlp(128, 77)
    gen = torch.Generator().manual_seed(78)
    d = 64 if op == "recon_adj" else 128
    x0 = randn(gen, s.n, d, dev=dev, scale=0.3)
    z10, z20 = randn(gen, s.B, 64, dev=dev), randn(gen, s.B, 64, dev=dev)

    def build():
        return (copy.deepcopy(mlp0).to(dev), x0.clone().requires_grad_(True),
                z10.clone().requires_grad_(True), z20.clone().requires_grad_(True))

    def run(state):
        mlp, x, z1, z2 = state
        res = {}
        if op == "recon_adj":
            rec = pkg.ops.recon_adj(x, s.g)
            (2.0 * rec).backward()
        elif op == "mlp2_recon":
            rec = pkg.ops.mlp2_recon(x, mlp, s.g)
            (2.0 * rec).backward()
        else:
            rec, con = pkg.ops.mlp2_recon_contrastive(x, mlp, s.g, z1, z2)
            (2.0 * rec + 3.0 * con).backward()
            res.update(con=con, dz1=z1.grad, dz2=z2.grad)
        res.update(rec=rec, dx=x.grad)
        return grads_of("mlp.", mlp, res)

    check(build, run)


def test_mlp2_recon_contrastive_past_the_fold(pkg, dev):
    """More head tiles than recon_fin.h's kFinBlocks (= the co-resident grid
    of the head launch): the loss finish is recon_fin_k's own launch and the
    contrastive loss its own kernels.  The smallest such batch, in steps of 20
    molecules."""
    n_mols = 880
    while True:
        g, _ = rand_graph(pkg, n_mols, "qm9", 9, dev)
        if int(pkg._lib.query("scgib_gin_tiles", g.num_nodes())) > K_FIN_BLOCKS:
            break
        n_mols += 20
    assert n_mols < 1400
    n, B = g.num_nodes(), g.batch_size
    mlp0 = _mlp(128, 79)
    gen = torch.Generator().manual_seed(80)
    x0 = randn(gen, n, 128, dev=dev, scale=0.3)
    z10, z20 = randn(gen, B, 64, dev=dev), randn(gen, B, 64, dev=dev)

    def build():
        return (copy.deepcopy(mlp0).to(dev), x0.clone().requires_grad_(True),
                z10.clone().requires_grad_(True), z20.clone().requires_grad_(True))

    def run(state):
        mlp, x, z1, z2 = state
        rec, con = pkg.ops.mlp2_recon_contrastive(x, mlp, g, z1, z2)
        (2.0 * rec + 3.0 * con).backward()
        return grads_of("mlp.", mlp, {"rec": rec, "con": con, "dx": x.grad, "dz1": z1.grad,
                                      "dz2": z2.grad})

    check(build, run)


@pytest.mark.parametrize("k", [1, 2])
def test_recon_logm_dense(pkg, dev, k):
    s = shape(pkg, dev, "exact")
    mols = list(pkg.cache._split(s.gh, s.gh.batch_size))
    logms = [pkg.graph.trans_logM(gi, k) for gi in mols]
    x0 = randn(torch.Generator().manual_seed(81), s.n, 64, dev=dev, scale=0.3)

    def build():
        return x0.clone().requires_grad_(True)

    def run(x):
        loss = pkg.ops.recon_logm(x, s.g, pkg.graph.LogMBatch(logms, dev))
        loss.backward()
        return {"loss": loss, "dx": x.grad}

    check(build, run)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [1, 2])
def test_recon_logm_sparse(pkg, dev, k, kind):
    """graph.LogMSparse: the targets (s_in, s_sym, C: torch.empty in
    graph.logm_targets) are built inside the poisoned region too."""
    s = shape(pkg, dev, kind, k=k)
    x0 = randn(torch.Generator().manual_seed(82), s.n, 64, dev=dev, scale=0.3)

    def build():
        return x0.clone().requires_grad_(True)

    def run(x):
        lm = pkg.graph.logm_targets(s.g, k)
        loss = pkg.ops.recon_logm(x, s.g, lm)
        loss.backward()
        return {"loss": loss, "dx": x.grad, "C": lm.C}

    check(build, run)


# ---------------------------------------------------------------------------
# heads
# ---------------------------------------------------------------------------
HEAD_ROWS = 37


@pytest.mark.parametrize("sigmoid", [True, False], ids=["sigmoid", "logits"])
@pytest.mark.parametrize("c", [1, 16, 128, 617])
def test_predict_head(pkg, dev, c, sigmoid):
    assert (c <= pkg.ops.HEAD_C_NARROW) == (c in (1, 16))
    torch.manual_seed(91)
    seq0 = torch.nn.Sequential(torch.nn.Linear(128, 64), torch.nn.ReLU(), torch.nn.Linear(64, c))
    gen = torch.Generator().manual_seed(92)
    x0, gout = randn(gen, HEAD_ROWS, 128, dev=dev), randn(gen, HEAD_ROWS, c, dev=dev)

    def build():
        return copy.deepcopy(seq0).to(dev), x0.clone().requires_grad_(True)

    def run(state):
        seq, x = state
        assert pkg.ops.predict_head_ok(x, seq)
        out = pkg.ops.predict_head(x, seq, sigmoid)
        out.backward(gout)
        return grads_of("seq.", seq, {"out": out, "dx": x.grad})

    check(build, run)


def _masked_targets(gen, shape_, kind):
    t = torch.randint(0, 2, shape_, generator=gen).float() if kind in ("bce", "bce_logits") \
        else torch.randn(shape_, generator=gen)
    t[torch.rand(shape_, generator=gen) < 0.3] = float("nan")
    return t


def test_bce_mean(pkg, dev):
    gen = torch.Generator().manual_seed(93)
    s0 = torch.rand(HEAD_ROWS, 12, generator=gen).to(dev)
    t = torch.randint(0, 2, (HEAD_ROWS, 12), generator=gen).float().to(dev)

    def build():
        return s0.clone().requires_grad_(True)

    def run(sc):
        loss = pkg.ops.bce_mean(sc, t)
        (2.0 * loss).backward()
        return {"loss": loss, "ds": sc.grad}

    check(build, run)


@pytest.mark.parametrize("kind_", sorted(["bce", "bce_logits", "mae", "rmse"]))
def test_task_loss(pkg, dev, kind_):
    assert set(pkg.ops.TASK_LOSS_KINDS) == {"bce", "bce_logits", "mae", "rmse"}
    gen = torch.Generator().manual_seed(94)
    shape_ = (70, 128)
    s0 = (torch.rand(shape_, generator=gen) if kind_ == "bce"
          else torch.randn(shape_, generator=gen)).to(dev)
    t = _masked_targets(gen, shape_, kind_)
    frac = float(torch.isnan(t).float().mean())
    assert 0.25 < frac < 0.35
    t = t.to(dev)

    def build():
        return s0.clone().requires_grad_(True)

    def run(sc):
        loss, count = pkg.ops.task_loss(sc, t, kind_, return_count=True)
        (2.0 * loss).backward()
        return {"loss": loss, "count": count, "ds": sc.grad}

    clean = check(build, run)
    assert int(clean["count"]) == int((~torch.isnan(t)).sum())


@pytest.mark.parametrize("c", [2, 7])
@pytest.mark.parametrize("labels", ["float32", "int64"])
def test_class_loss(pkg, dev, labels, c):
    gen = torch.Generator().manual_seed(95)
    s0 = randn(gen, HEAD_ROWS, c, dev=dev)
    y = torch.randint(0, c, (HEAD_ROWS,), generator=gen)
    masked = torch.rand(HEAD_ROWS, generator=gen) < 0.3
    if labels == "float32":
        y = y.float()
        y[masked] = float("nan")
    else:
        y[masked] = -100
    y = y.to(dev)

    def build():
        return s0.clone().requires_grad_(True)

    def run(sc):
        epoch = pkg.metrics.ClassEpoch(dev)
        loss, count, hits, invalid = pkg.ops.class_loss(sc, y, epoch=epoch, return_stats=True)
        (2.0 * loss).backward()
        return {"loss": loss, "count": count, "hits": hits, "invalid": invalid, "ds": sc.grad,
                "epoch": epoch.state}

    clean = check(build, run)
    assert int(clean["count"]) == int((~masked).sum()) and int(clean["invalid"]) == 0


# ---------------------------------------------------------------------------
# metrics and optimizer
# ---------------------------------------------------------------------------
def test_eval_buffer_part_full(pkg, dev):
    """Three appends of 20 rows into a buffer of 100: the 40 rows behind the
    cursor keep whatever the allocation held (here: the poison) and must not
    reach any metric."""
    gen = torch.Generator().manual_seed(101)
    batches = []
    for _ in range(3):
        sc = torch.rand(20, 3, generator=gen)
        tg = torch.randint(0, 2, (20, 3), generator=gen).float()
        tg[torch.rand(20, 3, generator=gen) < 0.3] = float("nan")
        batches.append((sc.to(dev), tg.to(dev)))

    def run(_):
        buf = pkg.metrics.EvalBuffer(100, 3, dev)
        for sc, tg in batches:
            buf.append(sc, tg)
        res = dict(buf.per_task())
        res["cursor"] = buf.state[0:1]
        res["stored_scores"], res["stored_labels"] = buf.scores[:60], buf.labels[:60]
        torch.cuda.synchronize()
        res["rocauc"] = torch.tensor(buf.rocauc()["rocauc"], dtype=torch.float64)
        res["ap"] = torch.tensor(buf.ap(), dtype=torch.float64)
        res["rmse_mean"] = torch.tensor(buf.rmse()["rmse"], dtype=torch.float64)
        res["acc_mean"] = torch.tensor(buf.acc()["acc"], dtype=torch.float64)
        return res

    clean = check(lambda: None, run)
    assert int(clean["cursor"]) == 60 and int(clean["err"]) == 0
    assert torch.isfinite(clean["auc"]).all() and torch.isfinite(clean["rmse"]).all()


def test_class_epoch(pkg, dev):
    gen = torch.Generator().manual_seed(102)
    batches = [(randn(gen, 16, 2, dev=dev), torch.randint(0, 2, (16,), generator=gen).float().to(dev))
               for _ in range(3)]

    def run(_):
        epoch = pkg.metrics.ClassEpoch(dev)
        losses = [pkg.ops.class_loss(sc, y, epoch=epoch) for sc, y in batches]
        torch.cuda.synchronize()
        r = epoch.result()
        return {"losses": torch.stack(losses), "state": epoch.state,
                "loss": torch.tensor(r["loss"], dtype=torch.float64),
                "acc": torch.tensor(r["acc"], dtype=torch.float64)}

    clean = check(lambda: None, run)
    assert int(clean["state"][1]) == 3 and int(clean["state"][3]) == 48


def _adam_state(opt, params, res, prefix=""):
    for i, p in enumerate(params):
        res[f"{prefix}param.{i}"] = p
        st = opt.state.get(p, {})
        for key in ("step", "exp_avg", "exp_avg_sq"):
            res[f"{prefix}{key}.{i}"] = st.get(key)
    return res


def test_adam_step(pkg, dev):
    gen = torch.Generator().manual_seed(103)
    init = [torch.randn(*sh, generator=gen) for sh in OPT.SHAPES]
    grads = [[torch.randn(*sh, generator=gen).to(dev) for sh in OPT.SHAPES] for _ in range(2)]
    assert len(init) > int(pkg._lib.query("scgib_adam_max_tensors"))  # more than one launch

    def build():
        return [t.clone().to(dev).requires_grad_(True) for t in init]

    def run(params):
        opt = pkg.optim.Adam(params, lr=1e-3, weight_decay=5e-5)
        for gs in grads:
            for p, g in zip(params, gs):
                p.grad = g.clone()
            opt.step()
        return _adam_state(opt, params, {})

    check(build, run)


def _pretrain_batch(pkg, dev, s, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(s.n, generator=gen).to(dev), torch.rand(s.n, 64, generator=gen).to(dev))


def _model_state(model, opt, res):
    params = list(model.named_parameters())
    for k, p in params:
        res["param." + k] = p
        res["grad." + k] = p.grad
        if opt is not None:
            st = opt.state.get(p, {})
            for key in ("step", "exp_avg", "exp_avg_sq"):
                res[f"{key}.{k}"] = st.get(key)
    for k, b in model.named_buffers():
        res["buf." + k] = b
    return res


def test_adam_step_reduce_fused_final(pkg, dev, monkeypatch):
    """scgib_adam_step_reduce: the ego chain's final weight-gradient reduce
    left to the optimizer launch (ops.fuse_final_into_step)."""
    monkeypatch.setattr(pkg.ops, "FUSE_FINAL_MIN_SLABS", 0)
    s = shape(pkg, dev, "exact")
    noise = _pretrain_batch(pkg, dev, s, 104)
    base = _pretrain_model(pkg, s.x.shape[1], 1, s.B, torch.device("cpu"))
    seen = []

    def build():
        model = copy.deepcopy(base).to(dev).train()
        return model, pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)

    def run(state):
        model, opt = state
        with pkg.ops.fuse_final_into_step():
            _, kl, con, rec = model(s.g, s.x, None, None, None, 1, None, 1, dev, s.B, noise=noise)
            (kl + con + rec).backward()
            seen.append(bool(pkg.ops._FINAL_PENDING))
            opt.step()
        assert not pkg.ops._FINAL_PENDING
        return _model_state(model, opt, {"losses": torch.stack([kl, con, rec]).detach()})

    check(build, run)
    assert seen == [True, True, True]  # the path under test: the reduce was left to the step


def test_grad_allreducer_pack_unpack(pkg, dev):
    gen = torch.Generator().manual_seed(105)
    shapes = [(64, 64), (64,), (3, 7), (1,), (2049,)]
    init = [torch.randn(*sh, generator=gen).to(dev) for sh in shapes]
    buf0 = torch.randn(64, generator=gen).to(dev)

    def build():
        params = [torch.zeros_like(t).requires_grad_(True) for t in init]
        for p, g in zip(params, init):
            p.grad = g.clone()
        return params, buf0.clone()

    def run(state):
        params, buf = state
        red = pkg.dist.GradAllReducer(params, buffers=[buf])
        red.pack()
        flat = red._flat.clone()
        for p in params:
            p.grad.zero_()
        buf.zero_()
        red.reduce()
        red.unpack()
        res = {"flat": flat, "buf": buf}
        res.update({f"grad.{i}": p.grad for i, p in enumerate(params)})
        return res

    clean = check(build, run)
    assert torch.equal(clean["grad.4"], init[4].cpu()) and torch.equal(clean["buf"], buf0.cpu())


# ---------------------------------------------------------------------------
# the whole step: forward + backward + optim.Adam.step at B = 8, k = 1
# ---------------------------------------------------------------------------
B_STEP = 8


def _args(recons_type="adj", readout_f="sum", use_att=1, dataset="pre-train"):
    return SimpleNamespace(recons_type=recons_type, useAtt=use_att, readout_f=readout_f,
                           d_transfer=32, batch_size=B_STEP, gin_layers=5,
                           task="graph_classification", dataset=dataset)


def _pretrain(pkg, args, f_in, encoder="GIN"):
    torch.manual_seed(111)
    inner = pkg.models.Mainmodel(args, f_in, 64, 4, 4, 1, encoder)
    model = pkg.models.Mainmodel_continue(args, f_in, 64, 4, 4, 1, 1, inner, encoder)
    perturb_bn(model, torch.Generator().manual_seed(112))
    return model


def _step_shape(pkg, dev, kind):
    return shape(pkg, dev, kind, n_mols=B_STEP, seed=17)


def _seed_streams(pkg, dev):
    pkg.ops.seed_noise(dev, 1234)
    pkg.ops.seed_dropout(dev, 555, lane=0)
    pkg.ops.seed_dropout(dev, 556, lane=1)


def _pretrain_step_case(pkg, dev, base, s):
    noise = _pretrain_batch(pkg, dev, s, 113)

    def build():
        _seed_streams(pkg, dev)
        model = copy.deepcopy(base).to(dev).train()
        return model, pkg.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-5)

    def run(state):
        model, opt = state
        _, kl, con, rec = model(s.g, s.x, None, None, None, 1, None, 1, dev, B_STEP, noise=noise)
        (kl + con + rec).backward()
        res = {"losses": torch.stack([kl, con, rec]).detach()}
        for k, p in model.named_parameters():
            res["grad_before_step." + k] = None if p.grad is None else p.grad.clone()
        opt.step()
        return _model_state(model, opt, res)

    clean = check(build, run)
    assert torch.isfinite(clean["losses"]).all()
    assert sum(v is not None for k, v in clean.items() if k.startswith("grad.")) > 20


@pytest.mark.parametrize("use_att", [1, 0], ids=["att", "noatt"])
@pytest.mark.parametrize("readout_f", ["sum", "set2set"])
@pytest.mark.parametrize("recons_type", ["adj", "logM"])
def test_pretrain_step_gin(pkg, dev, recons_type, readout_f, use_att):
    """Mainmodel_continue, GIN; 'logM' with batch_logMs=None (the targets are
    built on the device from the step's own ego batch)."""
    s = _step_shape(pkg, dev, "exact")
    base = _pretrain(pkg, _args(recons_type, readout_f, use_att), s.x.shape[1])
    _pretrain_step_case(pkg, dev, base, s)


@pytest.mark.parametrize("encoder", ["GCN", "GraphSAGE", "Transformer"])
def test_pretrain_step_other_encoders(pkg, dev, encoder, monkeypatch):
    monkeypatch.setattr(pkg.models, "ALL_ENCODER_STRINGS", True)
    s = _step_shape(pkg, dev, "exact")
    base = _pretrain(pkg, _args(), s.x.shape[1], encoder)
    _pretrain_step_case(pkg, dev, base, s)


def test_pretrain_step_gin_capacity(pkg, dev):
    s = _step_shape(pkg, dev, "cap")
    base = _pretrain(pkg, _args(), s.x.shape[1])
    _pretrain_step_case(pkg, dev, base, s)


def _finetune(pkg, f_in, c, dataset):
    args = _args(dataset=dataset)
    pre = _pretrain(pkg, args, f_in)
    torch.manual_seed(114)
    return pkg.models.Mainmodel_finetuning(args, f_in, 64, 4, 4, 1, c, pre, "GIN")


def _finetune_step_case(pkg, dev, s, loss_kind):
    gen = torch.Generator().manual_seed(115)
    if loss_kind == "bce":
        c, dataset = 1, "ogbg-molhiv"
        targets = torch.randint(0, 2, (B_STEP, 1), generator=gen).float()
    elif loss_kind == "wide_masked":
        c, dataset = 128, "ogbg-molpcba"
        targets = torch.randint(0, 2, (B_STEP, c), generator=gen).float()
        targets[torch.rand(B_STEP, c, generator=gen) < 0.3] = float("nan")
    else:
        c, dataset = 2, "Mutagenicity"
        targets = torch.randint(0, 2, (B_STEP, 1), generator=gen).float()
    targets = targets.to(dev)
    base = _finetune(pkg, s.x.shape[1], c, dataset)
    noise = _pretrain_batch(pkg, dev, s, 116)

    def build():
        _seed_streams(pkg, dev)
        ft = copy.deepcopy(base).to(dev).train()
        return ft, pkg.optim.Adam([p for p in ft.parameters() if p.requires_grad], lr=1e-3,
                                  weight_decay=1e-5)

    def run(state):
        ft, opt = state
        scores, *_ = ft(s.g, s.x, None, None, 1, None, 1, dev, B_STEP, noise=noise)
        if loss_kind == "bce":
            loss = ft.loss(scores, targets)
        elif loss_kind == "wide_masked":
            loss = pkg.MetricWrapper(metric=ft.loss, target_nan_mask="ignore-flatten")(scores,
                                                                                       targets)
        else:
            loss = ft.loss_CrossEntropy(scores, targets)
        loss.backward()
        opt.step()
        return _model_state(ft, opt, {"scores": scores, "loss": loss})

    clean = check(build, run)
    assert torch.isfinite(clean["loss"]) and clean["scores"].shape == (B_STEP, c)
    assert clean["grad.predict.2.weight"] is not None


@pytest.mark.parametrize("loss_kind", ["bce", "wide_masked", "ce"])
def test_finetune_step(pkg, dev, loss_kind):
    _finetune_step_case(pkg, dev, _step_shape(pkg, dev, "exact"), loss_kind)


def test_finetune_step_bce_capacity(pkg, dev):
    _finetune_step_case(pkg, dev, _step_shape(pkg, dev, "cap"), "bce")


def test_domainadapt_step(pkg, dev):
    s = _step_shape(pkg, dev, "exact")
    args = _args(dataset="ogbg-molhiv")
    pre = _pretrain(pkg, args, s.x.shape[1])
    torch.manual_seed(117)
    base = pkg.models.Mainmodel_domainadapt(args, s.x.shape[1], 64, 4, 4, 1, 1, pre, "GIN")
    noise = _pretrain_batch(pkg, dev, s, 118)

    def build():
        _seed_streams(pkg, dev)
        model = copy.deepcopy(base).to(dev).train()
        return model, pkg.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-5)

    def run(state):
        model, opt = state
        loss = model(s.g, s.x, None, None, None, 1, None, 1, dev, B_STEP, noise=noise)
        loss.backward()
        opt.step()
        return _model_state(model, opt, {"loss": loss})

    clean = check(build, run)
    assert torch.isfinite(clean["loss"])
