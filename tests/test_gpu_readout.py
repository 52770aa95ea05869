"""The set2set readout and useAtt = 0 on the MI355X (``-m gpu``):
the width-128 contrastive loss, the interaction kernels without the attention,
the two-input Set2Set launch, the pretraining step in the new modes against the
reference's own runs (tools/gen_readout_golden.py), what the modes leave
unchanged, and a captured set2set step."""
import copy
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import CANCELLED, GOLDEN, check_grads, check_grads_model, load_golden, rel_err, rel_l2
from oracle import scgib_ref as R
from test_gpu_parity import (ACT_TOL, CHUNK_COUNTS, GRAD_TOL, LOSS_TOL, _INT_SENTINEL,
                             _interaction_fwd_raw, _untouched, path_batch, rand_graph)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------
# 1. contrastive loss at width 128 vs the oracle in fp64
# ---------------------------------------------------------------------------
# 65: a one-row tail tile; 1100: 18 column tiles over kMaxSplit = 16 splits, so
# the first two splits walk two tiles each
@pytest.mark.parametrize("B", [1, 7, 64, 65, 100, 1100])
def test_contrastive_w128_fwd_bwd(pkg, dev, B):
    gen = torch.Generator().manual_seed(B)
    z1 = torch.randn(B, 128, generator=gen) * 2
    z2 = torch.randn(B, 128, generator=gen) + 0.5 * z1
    if B > 7:
        z2[3] = 0.0  # a zero readout row (F.normalize eps branch)
    z1r = z1.double().requires_grad_(True)
    z2r = z2.double().requires_grad_(True)
    lr = R.semi_loss(z1r, z2r, 16)
    lr.backward()
    z1d = z1.to(dev).requires_grad_(True)
    z2d = z2.to(dev).requires_grad_(True)
    for rep in range(2):  # the arrival counters must be left reusable
        z1d.grad = z2d.grad = None
        ld = pkg.ops.contrastive(z1d, z2d)
        (3.0 * ld).backward()
        print(f"B={B} rep={rep} loss {ld.item():.8g} vs {lr.item():.8g}")
        assert abs(ld.item() - lr.item()) <= 1e-5 * max(1.0, abs(lr.item())), rep
        for mine, ref in ((z1d.grad, z1r.grad), (z2d.grad, z2r.grad)):
            ref = 3.0 * ref
            err = (mine.cpu().double() - ref).norm()
            print(f"  grad err {err.item():.3g} of {ref.norm().item():.3g}")
            assert err <= 1e-5 * max(ref.norm().item(), 1e-2), rep


# ---------------------------------------------------------------------------
# 2. interaction without the attention vs the oracle's compression + cat, fp64
# ---------------------------------------------------------------------------
def _check_noatt(pkg, dev, training, g, gh):
    torch.manual_seed(0)
    n, B = g.num_nodes(), g.batch_size
    counts = torch.from_numpy(gh.batch_num_nodes_host())
    comp = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.BatchNorm1d(64),
                               torch.nn.ReLU(), torch.nn.Linear(64, 1))
    attn = torch.nn.Linear(128, 1)
    with torch.no_grad():
        comp[1].weight.add_(0.2 * torch.randn(64))
        comp[1].bias.add_(0.2 * torch.randn(64))
        comp[1].running_mean.normal_()
        comp[1].running_var.uniform_(0.5, 2.0)
    f, s = torch.randn(n, 64), torch.randn(n, 64)
    u_gate, u_feat = torch.rand(n), torch.rand(n, 64)
    # A two-row graph's KL divides (f - mean) by the std of two values.  Where
    # the rows nearly agree in a channel, the reference's own fp32 evaluation
    # of f - mean loses |f| 2^-24 / |f_1 - f_0| (3e-4 of the KL at the seed's
    # draw, on the CPU oracle in fp32 as on the kernel, which follows the same
    # formula), so against an fp64 oracle the case would measure the formula's
    # conditioning.  The rows are kept >= 0.5 apart in every channel.
    off = 0
    for c in counts.tolist():
        if c == 2:
            d = torch.randn(64)
            f[off + 1] = f[off] + torch.sign(d) * (0.5 + d.abs())
        off += c
    n_last = int(counts[-1])
    # oracle (CPU, fp64): compression, then cat(noisy, sub_readout) (models.py:726)
    p = {"compressor.0.weight": comp[0].weight, "compressor.0.bias": comp[0].bias,
         "compressor.1.weight": comp[1].weight, "compressor.1.bias": comp[1].bias,
         "compressor.3.weight": comp[3].weight, "compressor.3.bias": comp[3].bias}
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in p.items()}
    bn_state = {"compressor.1.running_mean": comp[1].running_mean.double().clone(),
                "compressor.1.running_var": comp[1].running_var.double().clone(),
                "compressor.1.num_batches_tracked": comp[1].num_batches_tracked.clone()}
    fo, so = f.double().requires_grad_(True), s.double().requires_grad_(True)
    if not training:
        orig = R._batchnorm_train
        R._batchnorm_train = lambda x, pp, name, buf, *_: F.batch_norm(
            x, bn_state[name + ".running_mean"], bn_state[name + ".running_var"],
            pp[name + ".weight"], pp[name + ".bias"], False, 0.1, 1e-5)
    try:
        noisy_r, _, kl_r = R.compression(p, fo, counts, u_gate.double(), u_feat.double(),
                                         bn_state if training else None)
    finally:
        if not training:
            R._batchnorm_train = orig
    im_r = torch.cat((noisy_r, so), -1)
    z1_r, z2_r = R.sum_nodes(noisy_r, counts), R.sum_nodes(fo, counts)
    # HIP
    comp_d, attn_d = comp.to(dev), attn.to(dev)
    comp_d.train(training)
    fd = f.to(dev).requires_grad_(True)
    sd = s.to(dev).requires_grad_(True)
    t = comp_d[0](fd)
    im, z1, z2, kl, kl_mean = pkg.ops.interaction(fd, t, sd, u_gate.to(dev), u_feat.to(dev),
                                                  comp_d[1], comp_d[3], attn_d, g, training,
                                                  use_att=False)
    assert torch.equal(im[:, 64:], sd.detach())  # the raw s rows, bitwise
    for a, b, nm in ((im, im_r, "im"), (z1, z1_r, "z1"), (z2, z2_r, "z2"), (kl, kl_r, "kl"),
                     (kl_mean, kl_r.mean(), "kl_mean")):
        assert rel_err(a.detach().cpu(), b.detach()) < ACT_TOL, nm
    assert kl.shape == (2 * n_last, 64)
    if training:
        for k in ("running_mean", "running_var"):
            assert rel_err(getattr(comp_d[1], k).cpu(), bn_state["compressor.1." + k]) < 1e-5
        assert int(comp_d[1].num_batches_tracked) == B
    ws = [torch.randn(x.shape).double() for x in (im_r, z1_r, z2_r, kl_r, kl_r.mean())]
    lr = sum((w * x).sum() for w, x in zip(ws, (im_r, z1_r, z2_r, kl_r, kl_r.mean())))
    lr.backward()
    ld = sum((w.float().to(dev) * x).sum() for w, x in zip(ws, (im, z1, z2, kl, kl_mean)))
    ld.backward()
    assert rel_l2(fd.grad.cpu(), fo.grad) < GRAD_TOL
    assert rel_l2(sd.grad.cpu(), so.grad) < GRAD_TOL
    assert attn_d.weight.grad is None and attn_d.bias.grad is None
    mods = {"compressor.0": comp_d[0], "compressor.1": comp_d[1], "compressor.3": comp_d[3]}
    grads = {k: v.grad.numpy() for k, v in p.items()}
    cancelled = CANCELLED if training else ("attn_layer.bias",)
    check_grads(grads, lambda k: getattr(mods[k.rsplit(".", 1)[0]], k.rsplit(".", 1)[1]).grad,
                tol=GRAD_TOL, cancelled=cancelled, metric="l2")


@pytest.mark.parametrize("training", [True, False])
def test_interaction_noatt_fwd_bwd(pkg, dev, training):
    g, gh = rand_graph(pkg, 48, "qm9", 6, dev)
    _check_noatt(pkg, dev, training, g, gh)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("counts", CHUNK_COUNTS, ids=lambda c: "-".join(map(str, c)))
def test_interaction_noatt_fwd_bwd_multi_chunk(pkg, dev, training, counts):
    g, gh = path_batch(pkg, counts, dev)
    _check_noatt(pkg, dev, training, g, gh)


@pytest.fixture
def raw_noatt(pkg, monkeypatch):
    """test_gpu_parity's raw C-ABI forward, sent to scgib_interaction_fwd_v2
    with use_att = 0 (the same inputs and sentinel-filled outputs)."""
    orig = pkg._lib.call

    def call(name, *args):
        if name == "scgib_interaction_fwd":
            return orig("scgib_interaction_fwd_v2", *args[:-1], 0, args[-1])
        return orig(name, *args)

    monkeypatch.setattr(pkg._lib, "call", call)
    return _interaction_fwd_raw


_STATS_KEPT = 256  # mean / ssq of t, mu, sigma; the three softmax slots are zero


def _noatt_rows_ok(out, n):
    """Live rows: im[:, 64:] written, lam written, logit left alone."""
    assert not (out["im"][:n] == _INT_SENTINEL).any() and not (out["lam"][:n] == _INT_SENTINEL).any()
    assert _untouched(out["logit"][:n])


@pytest.mark.parametrize("training", [True, False])
def test_interaction_noatt_fwd_capacity_padding(pkg, dev, training, raw_noatt):
    gptr = [0, 16, 33, 130]
    N, B, cap = gptr[-1], len(gptr) - 1, gptr[-1] + 70
    exact = raw_noatt(pkg, dev, gptr, N, N, training, pad=0)
    padded = raw_noatt(pkg, dev, gptr, N, cap, training, pad=1)
    _noatt_rows_ok(exact, N)
    for k in ("im", "lam"):
        assert torch.equal(padded[k][:N], exact[k][:N]), k
        assert torch.count_nonzero(padded[k][N:cap]) == 0, k
        assert _untouched(padded[k][cap:]) and _untouched(exact[k][N:]), k
    assert torch.count_nonzero(padded["logit"][N:cap]) == 0 and _untouched(padded["logit"][cap:])
    for k, rows in (("z1", B), ("z2", B), ("kl", 2 * (gptr[-1] - gptr[-2])), ("kl_mean", 1)):
        assert torch.equal(padded[k], exact[k]), k
        assert _untouched(exact[k][rows:]) and not (exact[k][:rows] == _INT_SENTINEL).any(), k
    assert torch.equal(padded["stats"][:B, :_STATS_KEPT], exact["stats"][:B, :_STATS_KEPT])
    assert torch.count_nonzero(exact["stats"][:B, _STATS_KEPT:_STATS_KEPT + 3]) == 0
    assert _untouched(padded["stats"][B:])


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("where", ["middle", "last"])
def test_interaction_noatt_fwd_empty_graph(pkg, dev, training, where, raw_noatt):
    base_ptr = [0, 7, 47, 80]
    N = base_ptr[-1]
    base = raw_noatt(pkg, dev, base_ptr, N, N, training, pad=0)
    if where == "middle":
        gptr, live, empty = [0, 7, 7, 47, 80], [0, 2, 3], 1
    else:
        gptr, live, empty = [0, 7, 47, 80, 80], [0, 1, 2], 3
    got = raw_noatt(pkg, dev, gptr, N, N, training, pad=0)
    _noatt_rows_ok(got, N)
    for k in ("im", "lam", "logit"):
        assert torch.equal(got[k], base[k]), k
    for k in ("z1", "z2"):
        assert torch.equal(got[k][live], base[k][:3]), k
        assert torch.count_nonzero(got[k][empty]) == 0, k
        assert _untouched(got[k][4:]), k
    assert torch.equal(got["stats"][live, :_STATS_KEPT], base["stats"][:3, :_STATS_KEPT])
    if where == "middle":
        assert torch.equal(got["kl"], base["kl"]) and torch.equal(got["kl_mean"], base["kl_mean"])
        assert not (got["kl"][:66] == _INT_SENTINEL).any()
    else:
        assert float(got["kl_mean"][0]) == 0.0 and _untouched(got["kl_mean"][1:])
        assert _untouched(got["kl"])


# ---------------------------------------------------------------------------
# 3. both Set2Set readouts in one launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_mols,mu", [(32, None), (1, None), (6, 150.0)])
def test_set2set_pair(pkg, dev, n_mols, mu):
    """ops.set2set_pair: outputs and dx bitwise those of two ops.set2set
    calls (rows past the batch: zero gradient), the LSTM gradients against the
    fp64 oracle applied twice; mu = 150: graphs past the 64 staged rows."""
    dim = 64
    torch.manual_seed(dim + n_mols)
    if mu is None:
        g, gh = rand_graph(pkg, n_mols, "molhiv", 5, dev)
    else:
        gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(n_mols, "molhiv", seed=5, mu=mu,
                                                          sigma=20.0))
        assert gh.batch_num_nodes_host().max() > 64
        g = gh.to(dev)
    n = g.num_nodes()
    s2s = pkg.models.Set2Set(dim, 2, 1).to(dev)
    full = [torch.randn(n + 37, dim, device=dev) for _ in range(2)]
    xa, xb = (t.clone().requires_grad_(True) for t in full)
    oa, ob = pkg.ops.set2set_pair(xa, xb, g, s2s.lstm, 2)
    wa, wb = torch.randn_like(oa), torch.randn_like(ob)
    ((oa * wa).sum() + (ob * wb).sum()).backward()
    pair_grads = {k: v.grad.clone() for k, v in s2s.named_parameters()}
    # two separate calls
    s2s.zero_grad(set_to_none=True)
    ya, yb = (t.clone().requires_grad_(True) for t in full)
    sa, sb = s2s(g, ya), s2s(g, yb)
    ((sa * wa).sum() + (sb * wb).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(oa, sa) and torch.equal(ob, sb)
    assert torch.equal(xa.grad, ya.grad) and torch.equal(xb.grad, yb.grad)
    assert float(xa.grad[n:].abs().max()) == 0.0 and float(xb.grad[n:].abs().max()) == 0.0
    # the oracle, twice over one parameter set
    p = {"s2s." + k: v.detach().cpu().double().clone().requires_grad_(True)
         for k, v in s2s.state_dict().items()}
    counts = torch.from_numpy(gh.batch_num_nodes_host().astype(np.int64))
    ra = R.set2set(p, "s2s", full[0][:n].cpu().double(), counts)
    rb = R.set2set(p, "s2s", full[1][:n].cpu().double(), counts)
    ((ra * wa.cpu().double()).sum() + (rb * wb.cpu().double()).sum()).backward()
    assert rel_err(oa.detach().cpu(), ra.detach()) < 1e-5
    assert rel_err(ob.detach().cpu(), rb.detach()) < 1e-5
    for k in pair_grads:
        err = rel_err(pair_grads[k].cpu(), p["s2s." + k].grad)
        print(f"{k}: rel_err {err:.3g}")
        assert err < 1e-4, k


def test_set2set_pair_one_output_unused(pkg, dev):
    """A loss over one of the two outputs only: the other's gradient is zero."""
    g, gh = rand_graph(pkg, 9, "molhiv", 5, dev)
    n = g.num_nodes()
    s2s = pkg.models.Set2Set(64, 2, 1).to(dev)
    xa = torch.randn(n, 64, device=dev, requires_grad=True)
    xb = torch.randn(n, 64, device=dev, requires_grad=True)
    _, ob = pkg.ops.set2set_pair(xa, xb, g, s2s.lstm, 2)
    ob.sum().backward()
    want = {k: v.grad.clone() for k, v in s2s.named_parameters()}
    s2s.zero_grad(set_to_none=True)
    yb = xb.detach().clone().requires_grad_(True)
    s2s(g, yb).sum().backward()
    assert torch.count_nonzero(xa.grad) == 0 and torch.equal(xb.grad, yb.grad)
    for k, v in s2s.named_parameters():
        assert rel_err(v.grad.cpu(), want[k].cpu()) < 1e-5, k


# ---------------------------------------------------------------------------
# 4. the pretraining step in the new modes vs the reference's own runs
# ---------------------------------------------------------------------------
READOUT_GOLDENS = ["pretrain_L4_k1_qm9_s2s", "pretrain_L4_k1_qm9_noatt",
                   "pretrain_L5_k1_qm9_continue_s2s_noatt"]
_GOLDEN_CACHE = {}


def _golden(name):
    """The fixture, with the grad_ keys of <name>_grads.npz when it has one
    (loaded once, left unchanged)."""
    if name not in _GOLDEN_CACHE:
        g = load_golden(name)
        if os.path.exists(os.path.join(GOLDEN, name + "_grads.npz")):
            g.update(load_golden(name + "_grads"))
        _GOLDEN_CACHE[name] = g
    return _GOLDEN_CACHE[name]


def _model_from_golden(pkg, g, dev):
    args = SimpleNamespace(recons_type="adj", useAtt=int(g["useAtt"]),
                           readout_f=str(g["readout_f"]), d_transfer=32, device="cuda",
                           batch_size=int(g["chunk"]), task="graph_classification",
                           dataset="pre-train", gin_layers=int(g["L"]))
    F_, k = int(g["F"]), int(g["k"])
    model = pkg.models.Mainmodel(args, F_, 64, 4, 4, k, "GIN")
    wrapped = bool(g["continue_wrapper"])
    if wrapped:
        model = pkg.models.Mainmodel_continue(args, F_, 64, 4, 4, k, 1, model, "GIN")
    sd = {kk[6:]: torch.tensor(v) for kk, v in g.items() if kk.startswith("param_")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected
    pfx = "model." if wrapped else ""
    hot = ("transfer_d.", "MLP.", "s2s.") + tuple(
        pfx + m for m in ("Encoder1.", "Encoder2.", "compressor.", "attn_layer.", "s2s."))
    for m in missing:
        assert not m.startswith(hot) or m.endswith("num_batches_tracked"), m
    return model.to(dev).train()


@pytest.mark.parametrize("name", READOUT_GOLDENS)
@pytest.mark.parametrize("device_ego", [True, False])
def test_readout_step_matches_reference(pkg, dev, name, device_ego):
    g = _golden(name)
    model = _model_from_golden(pkg, g, dev)
    bg = pkg.graph.GraphBatch.from_edges(g["src"], g["dst"], len(g["x_raw"]), True,
                                         g["batch_num_nodes"]).to(dev)
    x = F.normalize(torch.tensor(g["x_raw"]).float()).to(dev)
    if device_ego:
        ego, x_subs = None, None
    else:
        ego = pkg.graph.GraphBatch.from_edges(g["ego_src"], g["ego_dst"],
                                              int(g["ego_batch_num_nodes"].sum()), True,
                                              g["ego_batch_num_nodes"]).to(dev)
        x_subs = x[torch.tensor(g["ego_nodes_global"], device=dev)]
    noise = (torch.tensor(g["u_gate"], device=dev), torch.tensor(g["u_feat"], device=dev))
    _, kl, con, rec = model.forward(bg, x, ego, None, x_subs, 1, None, 2, dev, int(g["chunk"]),
                                    noise=noise)
    for mine, key in ((kl, "loss_kl"), (con, "loss_contrastive"), (rec, "loss_recon")):
        print(f"{key}: {mine.item():.8g} vs {float(g[key]):.8g}")
    assert rel_err(kl.item(), g["loss_kl"]) < LOSS_TOL
    assert rel_err(con.item(), g["loss_contrastive"]) < LOSS_TOL
    assert rel_err(rec.item(), g["loss_recon"]) < LOSS_TOL
    loss = kl + rec + con
    assert rel_err(loss.item(), g["loss_total"]) < LOSS_TOL
    loss.backward()
    params = dict(model.named_parameters())
    golden = {k[5:]: v for k, v in g.items() if k.startswith("grad_")}
    is_rd = lambda k: k.rsplit(".", 1)[0].endswith("reduce_d")  # noqa: E731
    check_grads_model({k: v for k, v in golden.items() if not is_rd(k)},
                      lambda n: params[n].grad, tol=GRAD_TOL)
    # the Set2Set LSTM's gradients (1e-2 beside weight gradients of 1e2..1e4:
    # the concatenated L2 above cannot see them), at the Set2Set test's bound
    lstm = [k for k in golden if ".lstm." in k]
    assert bool(lstm) == (str(g["readout_f"]) != "sum")
    for k in lstm:
        err = rel_err(params[k].grad.cpu(), golden[k])
        print(f"{k}: rel_err {err:.3g}")
        assert err < 1e-4, (k, err)
    # reduce_d: the attention's query is constant within a graph and cancels in
    # the softmax; here it stays out of the graph, the reference's gradient is
    # rounding noise
    for k, v in golden.items():
        if is_rd(k):
            att = golden[k[: k.index("reduce_d")] + "attn_layer.weight"]
            assert np.abs(v).max() <= 1e-3 * np.abs(att[:, 64:]).max(), k
    for k, p in params.items():
        if is_rd(k):
            assert p.grad is None or not p.grad.any(), k
    # parameters without a gradient in the reference have none here
    if not int(g["useAtt"]):
        assert all(p.grad is None for k, p in params.items() if "attn_layer" in k)
    buffers = dict(model.named_buffers())
    for k, v in g.items():
        if k.startswith("after_") and "running" in k:
            assert rel_err(buffers[k[6:]].cpu(), v) < 1e-4, k
        if k.startswith("after_") and "num_batches" in k:
            assert int(buffers[k[6:]]) == int(v), k


# ---------------------------------------------------------------------------
# 5. what the modes leave unchanged
# ---------------------------------------------------------------------------
def _args(readout_f="sum", useAtt=1, B=16):
    return SimpleNamespace(recons_type="adj", useAtt=useAtt, readout_f=readout_f, d_transfer=32,
                           batch_size=B, gin_layers=4, task="graph_classification",
                           dataset="ogbg-molhiv")


def _batch(pkg, dev, n_mols=16, workload="qm9", seed=3):
    g, _ = rand_graph(pkg, n_mols, workload, seed, dev)
    x = F.normalize(g.ndata["x"].float())
    n = g.num_nodes()
    gen = torch.Generator().manual_seed(seed)
    noise = (torch.rand(n, generator=gen).to(dev), torch.rand(n, 64, generator=gen).to(dev))
    return g, x, noise


@pytest.mark.parametrize("encoder", ["GIN", "GCN", "GraphSAGE", "Transformer"])
def test_set2set_step_keeps_kl_and_recon(pkg, dev, encoder, monkeypatch):
    """Same noise, same parameters: the set2set step's KL and recon are the
    sum step's (the attention's query cancels whatever the readout); its
    contrastive loss is finite and the Set2Set LSTM receives a gradient."""
    monkeypatch.setattr(pkg.models, "ALL_ENCODER_STRINGS", True)
    g, x, noise = _batch(pkg, dev)
    torch.manual_seed(5)
    m_sum = pkg.models.Mainmodel(_args("sum"), x.shape[1], 64, 4, 4, 1, encoder).to(dev).train()
    m_s2s = pkg.models.Mainmodel(_args("set2set"), x.shape[1], 64, 4, 4, 1, encoder)
    m_s2s.load_state_dict(m_sum.state_dict())
    m_s2s = m_s2s.to(dev).train()
    out = []
    for m in (m_sum, m_s2s):
        for lane in (0, 1):  # (the Transformer's dropout draws)
            pkg.ops.seed_dropout(dev, 99, 0, lane=lane)
        _, kl, con, rec = m(g, x, None, None, None, 1, None, 1, dev, 16, noise=noise)
        (kl + con + rec).backward()
        out.append((kl.item(), con.item(), rec.item()))
    (kl_a, con_a, rec_a), (kl_b, con_b, rec_b) = out
    print(f"{encoder}: kl {kl_a:.8g} / {kl_b:.8g}  recon {rec_a:.8g} / {rec_b:.8g}  "
          f"contrastive {con_a:.8g} / {con_b:.8g}")
    assert rel_err(kl_b, kl_a) < LOSS_TOL and rel_err(rec_b, rec_a) < LOSS_TOL
    assert np.isfinite(con_b)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.any()
               for p in m_s2s.s2s.lstm.parameters())
    assert all(p.grad is None for p in m_sum.s2s.lstm.parameters())
    assert all(p.grad is None for p in m_s2s.reduce_d.parameters())


def _da(pkg, dev, readout_f, useAtt, state=None):
    args = _args(readout_f, useAtt)
    torch.manual_seed(7)
    inner = pkg.models.Mainmodel(args, 9, 64, 4, 4, 1, "GIN")
    pre = pkg.models.Mainmodel_continue(args, 9, 64, 4, 4, 1, 1, inner, "GIN")
    da = pkg.models.Mainmodel_domainadapt(args, 9, 64, 4, 4, 1, 1, pre, "GIN")
    if state is not None:
        da.load_state_dict(state)
    return da.to(dev).train()


def test_domainadapt_follows_the_switches(pkg, dev):
    g, x, noise = _batch(pkg, dev, 16, "molhiv", 4)
    da_sum = _da(pkg, dev, "sum", 1)
    state = copy.deepcopy(da_sum.state_dict())
    da_s2s = _da(pkg, dev, "set2set", 1, state)
    da_noatt = _da(pkg, dev, "sum", 0, state)
    losses = [m(g, x, None, None, None, 1, None, 1, dev, 16, noise=noise).item()
              for m in (da_sum, da_s2s, da_noatt)]
    print("domainadapt losses sum / set2set / no-att:", losses)
    # it reads extract_features(...)[0] only: the readout changes nothing
    assert rel_err(losses[1], losses[0]) < LOSS_TOL
    # ... and without the attention the interaction map, hence the loss, differs
    assert np.isfinite(losses[2]) and rel_err(losses[2], losses[0]) > 10 * LOSS_TOL
    m = da_noatt
    ego = pkg.graph.egonet_batch(g, 1)
    x_subs = x.index_select(0, ego.ndata["_ID"])
    with torch.no_grad():
        im = m.model.extract_features(None, g, m.transfer_d(x), ego, m.transfer_d(x_subs), dev,
                                      noise)[0]
        assert torch.equal(im[:, 64:], pkg.ops.segment_sum(m.model.subgraphs_features,
                                                           ego.graph_ptr, ego.batch_size))
        want = m.loss_X(m.s2s_rev(g, x), m.r_transfer_d(m.s2s(g, pkg.ops.mlp2(im, m.MLP))))
    assert rel_err(losses[2], want.item()) < LOSS_TOL


# ---------------------------------------------------------------------------
# 6. a captured set2set step
# ---------------------------------------------------------------------------
def test_set2set_step_captures(pkg, dev):
    """B = 32, device ego-nets and device noise, readout_f = set2set, in
    capacity mode (padded StaticBatch rows, as every replayed step): captured
    with torch.cuda.graph and replayed twice; the first replay is the eager
    exact-size step from the same seed (the draws are keyed by row)."""
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(32, "qm9", seed=21))
    dict.__setitem__(gh.ndata, "x", F.normalize(gh.ndata["x"].float()))
    n_cap, e_cap, mgn, caps = pkg.graph.StaticBatch.capacities([gh], 1, slack=1.05)
    static = pkg.graph.StaticBatch(32, n_cap, e_cap, gh.ndata["x"].shape[1], mgn, caps, dev)
    assert n_cap > gh.num_nodes()
    padded = static.pad(gh)
    torch.manual_seed(9)
    model = pkg.models.Mainmodel(_args("set2set", 1, 32), gh.ndata["x"].shape[1], 64, 4, 4, 1,
                                 "GIN").to(dev).train()
    eager = copy.deepcopy(model)
    g = gh.to(dev)
    pkg.ops.seed_noise(dev, 4321)
    _, kl, con, rec = eager(g, g.ndata["x"], None, None, None, 1, None, 1, dev, 32)
    (kl + con + rec).backward()
    want = torch.stack([kl, con, rec]).detach().cpu()
    want_lstm = eager.s2s.lstm.weight_ih_l0.grad.clone()
    torch.cuda.synchronize()

    def step():
        _, kl, con, rec = model(static.graph, static.x, None, None, None, 1, None, 1, dev, 32)
        (kl + con + rec).backward()
        return torch.stack([kl, con, rec]).detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the capture
        static.load(padded)
        step()
    torch.cuda.current_stream().wait_stream(side)
    model.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        losses = step()
    pkg.ops.seed_noise(dev, 4321)
    for rep in range(2):
        static.load(padded)
        graph.replay()
        torch.cuda.synchronize()
        got = losses.cpu()
        print(f"replay {rep}: {got.tolist()} (eager {want.tolist()})")
        assert torch.isfinite(got).all()
        if rep == 0:
            for a, b in zip(got.tolist(), want.tolist()):
                assert rel_err(a, b) < LOSS_TOL
            assert rel_err(model.s2s.lstm.weight_ih_l0.grad.cpu(), want_lstm.cpu()) < 1e-4
        else:  # fresh noise: another step
            assert not torch.equal(got, want)
    assert static.ego_error() == 0
