"""Device-built logM targets and the sparse logM loss on the MI355X (``-m gpu``;
DESIGN.md §11): targets against graph.trans_logM (the restated util.getM_logM)
entry by entry, the loss op against an fp64 restatement of loss_recon, the model
step with ``batch_logMs=None`` against the reference's own run, determinism,
capacity mode / graph replay, dispatch and refusals."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import check_grads_model, golden_logms, load_golden, rel_err
from test_gpu_capacity import _compare, _noise
from test_gpu_parity import GRAD_TOL, LOSS_TOL, build_model_from_golden

pytestmark = pytest.mark.gpu

GOLDEN = "pretrain_L4_k2_logm"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _mol(edges, n=None):
    ei = np.array(edges, np.int64).T
    return ei, np.zeros((int(ei.max()) + 1 if n is None else n, 1), np.float32)


def _hand_molecules():
    """2 nodes; 7-star; 6-ring; an interior node without edges (node 3); paths of
    65 and 130 nodes (one past the ball builder's 64- / 128-node words); a
    self-loop (node 1)."""
    path = lambda n: [(i, i + 1) for i in range(n - 1)]  # noqa: E731
    return [_mol([(0, 1)]), _mol([(0, i) for i in range(1, 7)]),
            _mol([(i, (i + 1) % 6) for i in range(6)]), _mol([(0, 1), (1, 2), (2, 4)]),
            _mol(path(65)), _mol(path(130)), _mol([(0, 1), (1, 2), (1, 1)])]


def _golden_batch(pkg):
    g = load_golden(GOLDEN)
    return g, pkg.graph.GraphBatch.from_edges(g["src"], g["dst"], len(g["x_raw"]), True,
                                              g["batch_num_nodes"])


_HOSTS = {}


def _host(pkg, name):
    """Host batch `name` and its per-molecule graphs (built once, shared)."""
    if name not in _HOSTS:
        if name == "hand":
            gh = pkg.graph.batch([pkg.graph.from_pyg(ei, x) for ei, x in _hand_molecules()])
        elif name == "golden":
            gh = _golden_batch(pkg)[1]
        else:
            gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(32, name, seed=5))
        _HOSTS[name] = (gh, list(pkg.cache._split(gh, gh.batch_size)))
    return _HOSTS[name]


_REFS = {}


def _ref(pkg, name, k):
    """Per molecule (S fp32 [n, n], C float) as graph.LogMBatch packs the dense
    reference targets: the k fp32 terms summed in fp64, S rounded to fp32."""
    if (name, k) not in _REFS:
        out = []
        for gi in _host(pkg, name)[1]:
            m64 = pkg.graph.trans_logM(gi, k).double()
            out.append((m64.sum(0).float().numpy(), float((m64 * m64).sum())))
        _REFS[(name, k)] = out
    return _REFS[(name, k)]


def _check_targets(lm, ref, k):
    dense = lm.to_dense()
    C = lm.C.cpu().numpy()
    assert len(dense) == len(ref)
    worst = worst_c = 0.0
    for i, (S, (want, c_want)) in enumerate(zip(dense, ref)):
        assert S.shape == want.shape, i
        # k terms below 8, each within one ulp (2^-21) of a differently rounded
        # log, plus the final rounding of the sum
        tol = k * 2.0 ** -21 + np.spacing(np.abs(want))
        diff = np.abs(S.astype(np.float64) - want.astype(np.float64))
        worst = max(worst, float(diff.max()))
        assert (diff <= tol).all(), (i, float(diff.max()))
        rc = abs(C[i] - c_want) / max(abs(c_want), 1e-300) if c_want else abs(C[i])
        worst_c = max(worst_c, rc)
        assert rc <= 2.0 ** -20, (i, C[i], c_want)
    print(f"targets: worst |dS| {worst:.3e}, worst rel dC {worst_c:.3e}")


# ---------------------------------------------------------------------------
# 1. targets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", ["hand", "golden", "qm9", "molhiv"])
def test_targets_match_trans_logM(pkg, dev, name, k):
    gh, _ = _host(pkg, name)
    lm = pkg.graph.logm_targets(gh.to(dev), k)
    assert lm.kstep == k and lm.error() == 0
    _check_targets(lm, _ref(pkg, name, k), k)
    # s_sym = S[r, c] + S[c, r] on every slot
    dense = lm.to_dense()
    gp = gh.graph_ptr.numpy().astype(np.int64)
    ep = lm.ego_ptr.cpu().numpy().astype(np.int64)
    rows = lm.ego_nodes.cpu().numpy().astype(np.int64)[: ep[-1]]
    cols = np.repeat(np.arange(gh.num_nodes()), np.diff(ep))
    mol = np.searchsorted(gp, cols, side="right") - 1
    s_sym = lm.s_sym.cpu().numpy()[: ep[-1]]
    want = np.array([np.float32(np.float64(dense[m][r - gp[m], c - gp[m]]) +
                                np.float64(dense[m][c - gp[m], r - gp[m]]))
                     for m, r, c in zip(mol, rows, cols)], np.float32)
    # both halves are fp32-rounded sums on the host side, one rounding on the device
    assert np.abs(s_sym - want).max() <= 2 * np.spacing(np.abs(want)).max()


def test_targets_match_the_golden_flat_targets(pkg, dev):
    """... and the reference's own stored targets (logm_flat) at k = 2."""
    g, gh = _golden_batch(pkg)
    k = int(g["k"])
    assert k == 2
    ref = []
    for m in golden_logms(g):
        m64 = torch.tensor(m).double()
        ref.append((m64.sum(0).float().numpy(), float((m64 * m64).sum())))
    _check_targets(pkg.graph.logm_targets(gh.to(dev), k), ref, k)


# ---------------------------------------------------------------------------
# 2. loss op
# ---------------------------------------------------------------------------
def _loss_ref(im, sizes, logms, k):
    """loss_recon (models.py:770-782) in fp64 on dense targets [k, n, n]."""
    x = im.detach().double().cpu().requires_grad_(True)
    loss = 0
    for xs, t in zip(torch.split(x, tuple(sizes)), logms):
        h = xs @ xs.t()
        for i in range(k):
            loss = loss + ((h - t[i].double()) ** 2).sum() / (h.shape[0] * h.shape[1])
    loss = loss / k
    loss.backward()
    return float(loss.detach()), x.grad


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", ["hand", "qm9", "molhiv"])
def test_recon_logm_sparse_fwd_bwd(pkg, dev, name, k):
    gh, mols = _host(pkg, name)
    g = gh.to(dev)
    sizes = [int(v) for v in gh.batch_num_nodes_host()]
    logms = [pkg.graph.trans_logM(gi, k) for gi in mols]
    lm = pkg.graph.logm_targets(g, k)
    torch.manual_seed(7 + k)
    base = torch.randn(g.num_nodes(), 64)
    # second input: rows of norm ~1.3, X X^T of the targets' size (the three
    # terms of the expanded loss cancel)
    for tag, x0 in (("0.3 randn", 0.3 * base), ("norm 1.3", 1.3 * F.normalize(base))):
        want, gwant = _loss_ref(x0, sizes, logms, k)
        im = x0.to(dev).requires_grad_(True)
        loss = pkg.ops.recon_logm(im, g, lm)
        loss.backward()
        imd = x0.to(dev).requires_grad_(True)
        dense = pkg.ops.recon_logm(imd, g, logms)
        dense.backward()
        e_loss = rel_err(loss.item(), want)
        e_grad = rel_err(im.grad.cpu(), gwant)
        print(f"{name} k={k} {tag}: loss {loss.item():.7g} (fp64 {want:.7g}) rel {e_loss:.2e}; "
              f"grad rel {e_grad:.2e}; vs dense kernels: loss rel "
              f"{rel_err(loss.item(), dense.item()):.2e}, grad rel "
              f"{rel_err(im.grad.cpu(), imd.grad.cpu()):.2e}")
        assert e_loss < LOSS_TOL
        assert e_grad < 1e-5


# ---------------------------------------------------------------------------
# 3. the model step against the reference's own run
# ---------------------------------------------------------------------------
def test_model_step_device_targets_match_reference(pkg, dev):
    g = load_golden(GOLDEN)
    model = build_model_from_golden(pkg, g, dev)
    bg = _golden_batch(pkg)[1].to(dev)
    x = F.normalize(torch.tensor(g["x_raw"]).float()).to(dev)
    noise = (torch.tensor(g["u_gate"], device=dev), torch.tensor(g["u_feat"], device=dev))
    _, kl, con, rec = model.forward(bg, x, None, None, None, 1, None, 2, dev, int(g["chunk"]),
                                    noise=noise)
    assert rel_err(kl.item(), g["loss_kl"]) < LOSS_TOL
    assert rel_err(con.item(), g["loss_contrastive"]) < LOSS_TOL
    assert rel_err(rec.item(), g["loss_recon"]) < LOSS_TOL
    loss = kl + rec + con
    assert rel_err(loss.item(), g["loss_total"]) < LOSS_TOL
    loss.backward()
    params = dict(model.named_parameters())
    check_grads_model({k[5:]: v for k, v in g.items() if k.startswith("grad_")},
                      lambda n: params[n].grad, tol=GRAD_TOL)
    buffers = dict(model.named_buffers())
    for k, v in g.items():
        if k.startswith("after_") and "running" in k:
            assert rel_err(buffers[k[6:]].cpu(), v) < 1e-4, k
        if k.startswith("after_") and "num_batches" in k:
            assert int(buffers[k[6:]]) == int(v), k


# ---------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal(pkg, dev):
    g = _host(pkg, "molhiv")[0].to(dev)
    torch.manual_seed(3)
    x0 = (0.3 * torch.randn(g.num_nodes(), 64)).to(dev)
    runs = []
    for _ in range(2):
        lm = pkg.graph.logm_targets(g, 3)
        im = x0.clone().requires_grad_(True)
        loss = pkg.ops.recon_logm(im, g, lm)
        loss.backward()
        runs.append((lm.s_in, lm.s_sym, lm.C, loss.detach(), im.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# 5. capacity mode and capture
# ---------------------------------------------------------------------------
B = 8
F_IN = 11


def _logm_model(pkg, dev, k):
    args = SimpleNamespace(recons_type="logM", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=B, gin_layers=4)
    torch.manual_seed(11)
    return pkg.models.Mainmodel(args, F_IN, 64, 4, 4, k, "GIN").to(dev).train()


def _batches(pkg, seeds):
    out = []
    for s in seeds:
        gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=s))
        dict.__setitem__(gh.ndata, "x", F.normalize(gh.ndata["x"].float()))
        out.append(gh)
    return out


def _step(model, g, x, noise, dev, k):
    model.zero_grad(set_to_none=True)
    _, kl, con, rec = model(g, x, None, None, None, 1, None, k, dev, B, noise=noise)
    loss = kl + rec + con
    loss.backward()
    return torch.stack([kl, con, rec, loss]).detach()


@pytest.mark.parametrize("k", [1, 2])
def test_capacity_eager_and_replay_match_exact(pkg, dev, k):
    hosts = _batches(pkg, (31, 32, 33))
    n_cap, e_cap, mgn, caps = pkg.graph.StaticBatch.capacities(hosts, k, slack=1.05)
    static = pkg.graph.StaticBatch(B, n_cap, e_cap, F_IN, mgn, caps, dev, k=k)
    padded = [static.pad(gh) for gh in hosts]
    exact_m = _logm_model(pkg, dev, k)
    eager_m = copy.deepcopy(exact_m)
    cap_m = copy.deepcopy(exact_m)
    noises = [_noise(n_cap, dev, 500 + i) for i in range(3)]
    exact = []
    # eager padded step == exact-size step; targets of the padded batch bitwise
    # equal to the unpadded ones; gradient rows past the live N are zero
    for i, gh in enumerate(hosts):
        n = gh.num_nodes()
        ug, uf = noises[i]
        g = gh.to(dev)
        le = _step(exact_m, g, g.ndata["x"], (ug[:n], uf[:n]), dev, k)
        exact.append((le, {kk: p.grad.clone() for kk, p in exact_m.named_parameters()
                           if p.grad is not None},
                      {kk: b.clone() for kk, b in exact_m.named_buffers()}))
        static.load(padded[i])
        lc = _step(eager_m, static.graph, static.x, (ug, uf), dev, k)
        torch.cuda.synchronize()
        _compare(exact_m, eager_m, le, lc)
        lt_e = pkg.graph.logm_targets(g, k)
        lt_c = pkg.graph.logm_targets(static.graph, k)
        n_s = lt_e.s_in.shape[0]
        assert lt_c.s_in.shape[0] >= n_s and lt_c.dims is not None
        assert torch.equal(lt_c.s_in[:n_s], lt_e.s_in)
        assert torch.equal(lt_c.s_sym[:n_s], lt_e.s_sym)
        assert torch.equal(lt_c.C, lt_e.C)
        x0 = 0.3 * torch.randn(n_cap, 64, device=dev)
        im_e = x0[:n].clone().requires_grad_(True)
        im_c = x0.clone().requires_grad_(True)
        l_e = pkg.ops.recon_logm(im_e, g, lt_e)
        l_c = pkg.ops.recon_logm(im_c, static.graph, lt_c)
        l_e.backward()
        l_c.backward()
        assert torch.equal(l_e, l_c)
        assert torch.equal(im_c.grad[:n], im_e.grad)
        assert n_cap > n and not im_c.grad[n:].any()
        assert static.ego_error() == 0

    # one captured step replayed over the three batches == the eager exact steps
    s_ug = torch.zeros(n_cap, device=dev)
    s_uf = torch.zeros(n_cap, 64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    snap = copy.deepcopy(cap_m.state_dict())
    with torch.cuda.stream(side):
        static.load(padded[0])
        _step(cap_m, static.graph, static.x, (s_ug, s_uf), dev, k)
    torch.cuda.current_stream().wait_stream(side)
    cap_m.load_state_dict(snap)
    cap_m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, kl, con, rec = cap_m(static.graph, static.x, None, None, None, 1, None, k, dev, B,
                                noise=(s_ug, s_uf))
        loss = kl + rec + con
        loss.backward()
        static_losses = torch.stack([kl, con, rec, loss]).detach()
    ref_m = copy.deepcopy(exact_m)
    for i in range(3):
        le, grads, bufs = exact[i]
        # the exact model's state after step i, as _compare reads it
        ref_m.zero_grad(set_to_none=True)
        for kk, p in ref_m.named_parameters():
            if kk in grads:
                p.grad = grads[kk].clone()
        ref_m.load_state_dict({**ref_m.state_dict(), **bufs})
        s_ug.copy_(noises[i][0])
        s_uf.copy_(noises[i][1])
        static.load(padded[i])
        graph.replay()
        torch.cuda.synchronize()
        _compare(ref_m, cap_m, le, static_losses.clone())
    assert static.ego_error() == 0


# ---------------------------------------------------------------------------
# 6. dispatch and refusals
# ---------------------------------------------------------------------------
def test_dispatch_by_target_type(pkg, dev, monkeypatch):
    gh, mols = _host(pkg, "golden")
    g = gh.to(dev)
    lm = pkg.graph.logm_targets(g, 2)
    dense = [pkg.graph.trans_logM(gi, 2) for gi in mols]
    im = torch.randn(g.num_nodes(), 64, device=dev)
    called = []
    orig = pkg._lib.call

    def recording(name, *a):
        called.append(name)
        return orig(name, *a)

    monkeypatch.setattr(pkg._lib, "call", recording)
    pkg.ops.recon_logm(im, g, lm)
    assert "scgib_recon_logm_sparse_fwd" in called and "scgib_recon_logm_fwd" not in called
    called.clear()
    pkg.ops.recon_logm(im, g, dense)
    assert "scgib_recon_logm_fwd" in called and "scgib_recon_logm_sparse_fwd" not in called
    called.clear()
    pkg.ops.recon_logm(im, g, pkg.graph.LogMBatch(dense, dev))
    assert called == ["scgib_recon_logm_fwd"]


def test_refusals(pkg, dev):
    E = pkg._lib.ScgibError
    directed = pkg.graph.GraphBatch.from_edges([0, 1], [1, 2], 3, symmetric_hint=False).to(dev)
    with pytest.raises(E, match="symmetric"):
        pkg.graph.logm_targets(directed, 1)
    g = _host(pkg, "golden")[0].to(dev)
    other = _host(pkg, "qm9")[0].to(dev)
    with pytest.raises(E, match="another batch"):
        pkg.ops.recon_logm(torch.zeros(g.num_nodes(), 64, device=dev), g,
                           pkg.graph.logm_targets(other, 1))
    # the stated domain ends at k = scgib_logm_max_k(): refused by the argument
    # check, on the host (no launch)
    kmax = int(pkg._lib.query("scgib_logm_max_k"))
    with pytest.raises(E, match="outside"):
        pkg.graph.logm_targets(g, kmax + 1)
    with pytest.raises(E):
        pkg.graph.logm_targets(g, 0)
