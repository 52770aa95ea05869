"""The molecule-resident eval forward and the scoring API on the MI355X
(csrc/infer.hip, s-cgib_amd/infer.py): every output against the
fp64 oracle at the kernel's edge shapes (all taken from the exported limits),
bitwise independence of a molecule from its batch, capacity mode, poisoned
workspaces, the state a call must not move, the launches of a score step and
the captured dataset pass against eager batches."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import infer_cases as C
import poison
from conftest import rel_err
from eval_loader_cases import batches_of, eval_static
from infer_cases import same_bits
from oracle import scgib_ref as R

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4  # tests/test_gpu_trajectory.py: the layer path's bar against this oracle

CONFIGS = {
    "L5-k1": dict(k=1, layers=5),
    "L4-k2": dict(k=2, layers=4),
    "noatt": dict(k=1, layers=5, useAtt=0),
    "regression": dict(k=1, layers=5, dataset="ZINC", task="graph_regression"),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _trained(pkg, dev, name):
    """The config's fine-tune model after two training steps of the layer path
    (the running statistics are no longer their initial values), in eval mode."""
    cfg = dict(CONFIGS[name])
    k = cfg.pop("k")
    ft = C.finetune_model(pkg, k=k, **cfg).to(dev).train()
    opt = pkg.optim.Adam(ft.parameters(), lr=1e-3)
    before = ft.model.Encoder1.batch_norms[0].running_mean.clone()
    for step in range(2):
        g = C.batch_of(pkg, C.random_mols(pkg, 12, "molhiv", 40 + step)).to(dev)
        scores = ft(g, g.ndata["x"].float(), None, None)[0]
        y = torch.rand(scores.shape, device=dev).round()
        loss = ft.lossMAE(scores, y) if name == "regression" else ft.loss(scores, y)
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, ft.model.Encoder1.batch_norms[0].running_mean)
    return ft.eval(), k


@pytest.fixture(scope="module", autouse=True)
def _release_trained_models():
    """The trained models (and their optimizers) live for this module only:
    nothing of it stays on the device for the test files that follow."""
    yield
    _trained.cache_clear()
    _ds_case.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _noise(n, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=gen).to(dev), torch.rand(n, 64, generator=gen).to(dev)


def _resident(pkg, ft, g, noise):
    """Every output of the resident path for batch ``g`` (on the device)."""
    sc = pkg.infer.Scorer(ft, "resident")
    x = g.ndata["x"].float()
    e = sc.embed(g, x, noise)
    lam, logit, im = sc.rows(g, x, noise)
    out = {"scores": sc.score(g, x, noise), "pooled": e.pooled, "z1": e.z1, "z2": e.z2,
           "lam": lam, "logit": logit, "im": im}
    torch.cuda.synchronize()
    return out


def _oracle(ft, gh, k, noise):
    """finetune_forward(training=False) restated piecewise so that every
    intermediate the kernel can write is at hand; the final scores are checked
    against R.finetune_forward itself."""
    p, buffers = C.oracle_state(ft)
    batch, ego, x, xs = C.oracle_inputs(gh, k)
    ug, uf = noise[0].cpu().double(), noise[1].cpu().double()
    counts = batch["counts"]
    with torch.no_grad():
        pre = {kk[6:]: v for kk, v in p.items() if kk.startswith("model.")}
        bufs = {kk[6:]: v for kk, v in buffers.items() if kk.startswith("model.")}
        h0, hs0 = R._linear(x, p, "transfer_d", bias=False), R._linear(xs, p, "transfer_d", bias=False)
        L = R.num_gin_layers(pre)
        gf = R.gin_encoder(pre, "Encoder1", batch["src"], batch["dst"], h0, bufs, L, training=False)
        sf = R.gin_encoder(pre, "Encoder2", ego["src"], ego["dst"], hs0, bufs, L, training=False)
        noisy, pv, _ = R.compression(pre, gf, counts, ug, uf, bufs, False)
        eps = (0.0001 - (1 - 0.0001)) * ug.reshape(-1, 1) + (1 - 0.0001)
        lam = torch.sigmoid(torch.log(eps) - torch.log(1 - eps) + pv).reshape(-1)
        s = R.sum_nodes(sf, ego["counts"])
        if int(ft.model.useAtt):
            im = R.attention(pre, noisy, s, counts)
            logit = s @ pre["attn_layer.weight"][0, 64:]
        else:
            im, logit = torch.cat((noisy, s), -1), None
        m = R._linear(F.relu(R._linear(im, p, "MLP.0")), p, "MLP.2")
        pooled = R.set2set(p, "s2s", m, counts)
        scores = R._linear(F.relu(R._linear(pooled, p, "predict.0")), p, "predict.2")
        if ft.dataset not in R.FINETUNE_TASKS:
            scores = torch.sigmoid(scores)
        whole = R.finetune_forward(p, batch, ego, x, xs, ug, uf, ft.dataset, buffers, training=False)
    if int(ft.model.useAtt):  # (the oracle's own forward always attends: models.py:726 is not in it)
        ok = torch.isfinite(whole)
        assert torch.equal(ok, torch.isfinite(scores))
        assert torch.allclose(whole[ok], scores[ok], 1e-12, 0)
    return {"scores": scores, "pooled": pooled, "z1": R.sum_nodes(noisy, counts),
            "z2": R.sum_nodes(gf, counts), "lam": lam, "logit": logit, "im": im}


def _compare(tag, mine, ref):
    errs = {}
    for name, r in ref.items():
        if r is None:
            assert mine[name] is None, name
            continue
        errs[name] = rel_err(mine[name].cpu().double().numpy(), r.numpy())
    print(f"{tag}: rel_err vs fp64 oracle", {n: f"{e:.2e}" for n, e in errs.items()})
    for name, e in errs.items():
        assert e < SCORE_TOL, (tag, name, e)
    return errs


# ---------------------------------------------------------------------------
# 1. against the fp64 oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_output_against_the_oracle(pkg, dev, name):
    ft, k = _trained(pkg, dev, name)
    rng = np.random.default_rng(3)
    mols = C.random_mols(pkg, 9, "molhiv", 77) + [C.path(rng, 2), C.star(rng, 5)]
    gh = C.batch_of(pkg, mols)
    assert gh.batch_num_nodes_host().min() >= 2  # the parity inputs hold no one-atom molecule
    g = gh.to(dev)
    noise = _noise(g.num_nodes(), 8, dev)
    ref = _oracle(ft, gh, k, noise)
    _compare(f"resident {name}", _resident(pkg, ft, g, noise), ref)
    # the layer path on the same inputs: what Scorer(model) runs by default
    layers = pkg.infer.Scorer(ft, "layers")
    x = g.ndata["x"].float()
    e = layers.embed(g, x, noise)
    lay = {"scores": layers.score(g, x, noise), "pooled": e.pooled, "z1": e.z1, "z2": e.z2}
    _compare(f"layers {name}", lay, {n: ref[n] for n in lay})


def _edge_molecules_k1(pkg, rng):
    lim = pkg.ops.infer_limits()
    tile, top = lim["ego_tile_rows"], lim["max_nodes"]
    mols = [C.path(rng, 2)]
    mols += [C.path(rng, n) for n in (31, 32, 33, 63, 64, 65) if n <= top]
    mols += [C.path(rng, top)]
    # ego rows of the molecule: exactly one ego tile, one row more, two tiles
    for total in (tile, tile + 1, 2 * tile):
        m = C.path_with_k1_ego_rows(rng, total)
        assert C.k1_ego_rows(m[0], m[1]) == total and m[0] <= top
        mols.append(m)
    mols.append(C.star(rng, 12))  # 13-row ego-nets do not divide a tile
    assert tile % 13 != 0
    mols.append(C.with_loose_atom(rng, 6))  # a one-row ego-net inside a molecule
    return mols


def test_edge_shapes_against_the_oracle_k1(pkg, dev):
    ft, k = _trained(pkg, dev, "L5-k1")
    gh = C.batch_of(pkg, _edge_molecules_k1(pkg, np.random.default_rng(11)))
    assert gh.max_graph_nodes == pkg.ops.infer_limits()["max_nodes"]
    g = gh.to(dev)
    noise = _noise(g.num_nodes(), 9, dev)
    _compare("edges k1", _resident(pkg, ft, g, noise), _oracle(ft, gh, k, noise))
    assert int(pkg.ops.infer_error_word(dev).item()) == 0


def test_an_ego_net_of_exactly_max_ego_rows_at_k2(pkg, dev):
    ft, k = _trained(pkg, dev, "L4-k2")
    assert k == 2
    rng = np.random.default_rng(12)
    rows = pkg.ops.infer_limits()["max_ego_rows"]
    assert rows <= pkg.ops.infer_limits()["max_nodes"]
    # a star: every k = 2 ego-net is the whole molecule, one ego-net per tile
    gh = C.batch_of(pkg, [C.star(rng, rows - 1), C.path(rng, 5)])
    g = gh.to(dev)
    noise = _noise(g.num_nodes(), 10, dev)
    ego = pkg.graph.egonet_batch(g, 2)
    assert int(torch.diff(ego.graph_ptr).max().item()) == rows
    _compare("ego-net of max_ego_rows, k2", _resident(pkg, ft, g, noise), _oracle(ft, gh, k, noise))
    assert int(pkg.ops.infer_error_word(dev).item()) == 0


def test_one_atom_molecule_gives_nan_where_the_oracle_does(pkg, dev):
    ft, k = _trained(pkg, dev, "L5-k1")
    rng = np.random.default_rng(13)
    gh = C.batch_of(pkg, [C.path(rng, 4), C.single_atom(rng), C.path(rng, 3)])
    g = gh.to(dev)
    noise = _noise(g.num_nodes(), 11, dev)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # torch.std_mean over one row
        ref = _oracle(ft, gh, k, noise)
    mine = _resident(pkg, ft, g, noise)
    assert torch.isnan(ref["scores"][1]).all() and torch.isfinite(ref["scores"][[0, 2]]).all()
    for name, r in ref.items():
        m = mine[name].cpu().double()
        nan = torch.isnan(r)
        if name == "scores":
            # the kernel's pooled row is NaN (checked below); what the existing
            # predict head (csrc/head.hip, not this kernel) makes of a NaN row
            # is its own: its ReLU is an fmaxf, which returns 0 for NaN, so the
            # score of the one-atom molecule is sigmoid(predict[2].bias), which
            # is asserted.  The other molecules' scores are compared like every
            # other output.
            assert torch.isnan(mine["pooled"][1]).all()
            with torch.no_grad():
                bias_term = torch.sigmoid(ft.predict[2].bias).cpu().double()
            assert rel_err(m[1].numpy(), bias_term.numpy()) < SCORE_TOL, (m[1], bias_term)
            m = m.clone()
            m[1] = float("nan")  # (asserted above; the oracle's row is NaN)
        assert torch.equal(torch.isnan(m), nan), name  # NaN in the same positions
        assert torch.isfinite(m[~nan]).all(), name  # finite everywhere else
        assert rel_err(m[~nan].numpy(), r[~nan].numpy()) < SCORE_TOL, name  # no row left out


def test_above_max_nodes_auto_is_the_layer_path_and_resident_raises(pkg, dev, monkeypatch):
    monkeypatch.setattr(pkg.infer, "AUTO_RESIDENT", True)
    ft, k = _trained(pkg, dev, "L5-k1")
    rng = np.random.default_rng(14)
    top = pkg.ops.infer_limits()["max_nodes"]
    g = C.batch_of(pkg, [C.path(rng, 5), C.path(rng, top + 1)]).to(dev)
    x, noise = g.ndata["x"].float(), _noise(g.num_nodes(), 12, dev)
    auto = pkg.infer.Scorer(ft, "auto")
    assert auto.route(g) == "layers"
    with torch.no_grad():
        want = ft(g, x, None, None, noise=noise)[0]
    assert same_bits(auto.score(g, x, noise), want)
    with pytest.raises(pkg._lib.ScgibError, match="atoms"):
        pkg.infer.Scorer(ft, "resident").score(g, x, noise)
    # the op itself refuses the batch without a launch
    sc = pkg.infer.Scorer(ft, "resident")
    with pytest.raises(pkg._lib.ScgibError):
        pkg.ops.infer_forward(x, g, pkg.graph.egonet_batch(g, k), sc._tab(), *noise)
    assert int(pkg.ops.infer_error_word(dev).item()) == 0


def _oracle_readouts(owner, transfer, gh, k, noise):
    """(z1, z2) of the fp64 oracle for encoder owner ``owner`` fed by
    ``transfer`` (what models._explain_route hands the Scorer), eval mode."""
    pre, bufs = C.oracle_state(owner)
    batch, ego, x, xs = C.oracle_inputs(gh, k)
    ug, uf = noise[0].cpu().double(), noise[1].cpu().double()
    tw = {"transfer_d.weight": transfer.weight.detach().cpu().double()}
    with torch.no_grad():
        h0, hs0 = R._linear(x, tw, "transfer_d", bias=False), R._linear(xs, tw, "transfer_d", bias=False)
        L = R.num_gin_layers(pre)
        gf = R.gin_encoder(pre, "Encoder1", batch["src"], batch["dst"], h0, bufs, L, training=False)
        noisy, _, _ = R.compression(pre, gf, batch["counts"], ug, uf, bufs, False)
        if int(owner.useAtt):  # the whole oracle forward gives the same readouts
            acts = R.extract_features(pre, batch, ego, h0, hs0, ug, uf, bufs, training=False)
            assert torch.equal(acts["noisy"], noisy) and torch.equal(acts["graph_features"], gf)
    return {"z1": R.sum_nodes(noisy, batch["counts"]), "z2": R.sum_nodes(gf, batch["counts"])}


@pytest.mark.parametrize("use_att", [1, 0], ids=["att", "noatt"])
@pytest.mark.parametrize("kind", ["Mainmodel", "Mainmodel_continue", "Mainmodel_domainadapt"])
def test_embed_of_the_pretraining_classes_against_the_oracle(pkg, dev, kind, use_att):
    """The HEAD = 0 kernel instances and the routing of the three classes
    without a predict head, on both paths."""
    if kind == "Mainmodel":
        model = C.pretrain_model(pkg, wrapped=False, seed=21, useAtt=use_att)
    elif kind == "Mainmodel_continue":
        model = C.pretrain_model(pkg, seed=22, useAtt=use_att)
    else:
        a = C.args_of(useAtt=use_att)
        inner = C.pretrain_model(pkg, wrapped=False, seed=23, useAtt=use_att)
        torch.manual_seed(24)
        model = pkg.models.Mainmodel_domainadapt(a, C.F_IN, 64, 4, 4, 1, 1, inner, "GIN")
        C.shake_norms(model, 24)
    model = model.to(dev).eval()
    owner, transfer, k = pkg.models._explain_route(model)
    assert (owner is model) == (kind == "Mainmodel") and transfer is model.transfer_d
    rng = np.random.default_rng(4)
    gh = C.batch_of(pkg, C.random_mols(pkg, 7, "molhiv", 78) + [C.path(rng, 33), C.star(rng, 4)])
    g = gh.to(dev)
    x, noise = g.ndata["x"].float(), _noise(g.num_nodes(), 19, dev)
    ref = _oracle_readouts(owner, transfer, gh, k, noise)
    for path in ("resident", "layers"):
        sc = pkg.infer.Scorer(model, path)
        e = sc.embed(g, x, noise)
        assert e.pooled is None
        _compare(f"{path} embed {kind} useAtt={use_att}", {"z1": e.z1, "z2": e.z2}, ref)
        with pytest.raises(TypeError, match="predict head"):
            sc.score(g, x, noise)
    lam, logit, im = pkg.infer.Scorer(model, "resident").rows(g, x, noise)
    assert (logit is None) == (not use_att) and tuple(im.shape) == (g.num_nodes(), 128)
    assert torch.isfinite(im).all() and not pkg.ops.infer_error(dev)


def test_a_graph_ptr_range_outside_the_rows_is_an_error_not_a_zero_row(pkg, dev):
    ft, k = _trained(pkg, dev, "L5-k1")
    g = C.batch_of(pkg, C.random_mols(pkg, 5, "molhiv", 79)).to(dev)
    x, noise = g.ndata["x"].float(), _noise(g.num_nodes(), 20, dev)
    want = _resident(pkg, ft, g, noise)
    tab, ego = pkg.infer.Scorer(ft, "resident")._tab(), pkg.graph.egonet_batch(g, k)
    gp = g.graph_ptr.clone()
    gp[-1] += 5  # the last molecule claims rows past the batch's
    bad = pkg.graph.GraphBatch(g.rowptr, g.col, gp, None, max_graph_nodes=g.max_graph_nodes)
    assert not pkg.ops.infer_error(dev, reset=True)
    pooled, z1, z2, lam, logit, im = pkg.ops.infer_forward(x, bad, ego, tab, *noise, rows=True)
    torch.cuda.synchronize()
    assert pkg.ops.infer_error(dev) and pkg.ops.infer_error(dev, reset=True)  # sticky until reset
    assert not pkg.ops.infer_error(dev)
    r0 = int(g.graph_ptr[-2])
    for name, t, cut in (("pooled", pooled, 4), ("z1", z1, 4), ("z2", z2, 4), ("lam", lam, r0),
                         ("logit", logit, r0), ("im", im, r0)):
        assert same_bits(t[:cut], want[name][:cut]), name  # the other molecules: untouched
        assert torch.isnan(t[cut:]).all(), name  # its rows that exist: NaN, all written
    # a flag from before a dataset pass is neither blamed on the pass nor lost
    pkg.ops.infer_error_word(dev).fill_(1)
    mols, idx, ds, static, nz = _ds_case(pkg, dev)
    evl = pkg.graph.DeviceEvalLoader(ds, static, indices=idx)
    pkg.infer.score_dataset(ft, evl, noise=nz, path="resident")
    assert pkg.ops.infer_error(dev, reset=True)


# ---------------------------------------------------------------------------
# 2. a molecule's outputs do not depend on its batch: bitwise
# ---------------------------------------------------------------------------
def _rows_of(out, g, j):
    gp = g.graph_ptr.cpu().numpy()
    a, b = int(gp[j]), int(gp[j + 1])
    res = {n: out[n][j] for n in ("scores", "pooled", "z1", "z2")}
    res.update({n: out[n][a:b] for n in ("lam", "logit", "im")})
    return res


def test_batch_composition_independence_is_bitwise(pkg, dev):
    ft, k = _trained(pkg, dev, "L5-k1")
    rng = np.random.default_rng(15)
    mol = C.path_with_k1_ego_rows(rng, 101)  # 33 atoms and two rings: two row blocks
    n = mol[0]
    ug, uf = _noise(n, 13, dev)
    others = C.random_mols(pkg, 299, "qm9", 21)
    others = [(m[0], m[1], C.feats(rng, m[0])) for m in others]  # F_IN feature columns
    wg = pkg.ops.infer_limits()["max_workgroups"]
    settings = [([mol], 0), ([mol] + others[:2], 0), ([others[0], mol, others[1]], 1),
                (others[:2] + [mol], 2), (others[:150] + [mol] + others[150:], 150),
                # one molecule more than the launch has workgroups: workgroup 0 wraps to it
                ([C.path(rng, 2) for _ in range(wg)] + [mol], wg)]
    assert len(settings[4][0]) == 300
    got = []
    for mols, j in settings:
        g = C.batch_of(pkg, mols).to(dev)
        gp = g.graph_ptr.cpu().numpy()
        bg, bf = _noise(g.num_nodes(), 100 + j, dev)
        bg[gp[j]:gp[j + 1]] = ug
        bf[gp[j]:gp[j + 1]] = uf
        out = _resident(pkg, ft, g, (bg, bf))
        again = _resident(pkg, ft, g, (bg, bf))
        for name in out:  # two runs of the same launch
            assert same_bits(out[name], again[name]), (len(mols), name)
        got.append(_rows_of(out, g, j))
    for other in got[1:]:
        for name, t in got[0].items():
            assert same_bits(t, other[name]), name
    assert torch.isfinite(got[0]["pooled"]).all()


# ---------------------------------------------------------------------------
# 3. capacity mode
# ---------------------------------------------------------------------------
def _capacity_case(pkg, dev, gh, k, extra_b, fill):
    """A StaticBatch whose capacities exceed host batch ``gh`` (rows, edges,
    ego sizes and ``extra_b`` molecules), loaded by hand with every padding
    region holding ``fill``."""
    n, e, B = gh.num_nodes(), gh.num_edges(), gh.batch_size
    en, ee, dmax = pkg.graph.ego_bounds(gh, k)
    st = pkg.graph.StaticBatch(B + extra_b, n + 37, e + 50, C.F_IN, gh.max_graph_nodes,
                               (en + 60, ee + 90, dmax), dev, k)
    st.rowptr.fill_(e)
    st.rowptr[:n + 1] = gh.rowptr.to(dev)
    st.col[:e] = gh.col[:e].to(dev)
    st.graph_ptr.fill_(n)
    st.graph_ptr[:B + 1] = gh.graph_ptr.to(dev)
    st.dims.copy_(torch.tensor([n, e], dtype=torch.int32))
    st.x.fill_(fill)
    st.x[:n] = gh.ndata["x"].to(dev)
    return st


@pytest.mark.parametrize("fill", [float("nan"), poison.SENTINEL], ids=["nan", "sentinel"])
def test_capacity_mode_equals_eager_and_pads_with_zeros(pkg, dev, fill):
    ft, k = _trained(pkg, dev, "L5-k1")
    rng = np.random.default_rng(16)
    gh = C.batch_of(pkg, C.random_mols(pkg, 7, "molhiv", 31) + [C.star(rng, 12)])
    g = gh.to(dev)
    n, B = gh.num_nodes(), gh.batch_size
    noise = _noise(n, 14, dev)
    want = _resident(pkg, ft, g, noise)
    st = _capacity_case(pkg, dev, gh, k, 3, fill)
    cg = torch.full((st.n_cap,), fill, device=dev)
    cf = torch.full((st.n_cap, 64), fill, device=dev)
    cg[:n], cf[:n] = noise
    with poison.poisoned(fill):
        sc = pkg.infer.Scorer(ft, "resident")
        e = sc.embed(st.graph, st.x, (cg, cf))
        lam, logit, im = sc.rows(st.graph, st.x, (cg, cf))
        scores = sc.score(st.graph, st.x, (cg, cf))
        torch.cuda.synchronize()
    for name, t, rows in (("scores", scores, B), ("pooled", e.pooled, B), ("z1", e.z1, B),
                          ("z2", e.z2, B), ("lam", lam, n), ("logit", logit, n), ("im", im, n)):
        assert same_bits(t[:rows], want[name]), name
        if name != "scores":  # (the predict head of a zero row is its bias)
            assert t.shape[0] > rows and not t[rows:].any(), name  # rows past the count: zeros
    assert st.ego_error() == 0 and int(pkg.ops.infer_error_word(dev).item()) == 0


# ---------------------------------------------------------------------------
# 4. fresh workspaces, state, launches
# ---------------------------------------------------------------------------
def test_poisoned_workspaces_change_no_bit(pkg, dev):
    ft, k = _trained(pkg, dev, "L5-k1")
    gh = C.batch_of(pkg, C.random_mols(pkg, 10, "molhiv", 32))

    def build():
        g = gh.to(dev)
        return g, _noise(g.num_nodes(), 15, dev)

    def run(state):
        g, noise = state
        return _resident(pkg, ft, g, noise)

    poison.assert_same(poison.run_thrice(build, run))


def test_calls_move_no_state_but_the_noise_stream(pkg, dev):
    ft, k = _trained(pkg, dev, "L5-k1")
    g = C.batch_of(pkg, C.random_mols(pkg, 10, "molhiv", 33)).to(dev)
    x = g.ndata["x"].float()
    sd = {kk: v.clone() for kk, v in ft.state_dict().items()}
    sc = pkg.infer.Scorer(ft, "resident")
    # the layer path's eval forward: how far a call advances the noise state
    pkg.ops.seed_noise(dev, 7, 5)
    with torch.no_grad():
        lay = ft(g, x, None, None)[0]
    after_layers = pkg.ops.noise_state(dev).clone()
    pkg.ops.seed_noise(dev, 7, 5)
    res = sc.score(g, x)
    assert torch.equal(pkg.ops.noise_state(dev), after_layers)
    assert after_layers.tolist() == [7, 6]
    # equal seeds: both paths saw the same draws
    assert rel_err(res.cpu().numpy(), lay.cpu().numpy()) < SCORE_TOL
    sc.embed(g, x)
    assert pkg.ops.noise_state(dev).tolist() == [7, 7]
    noise = _noise(g.num_nodes(), 16, dev)
    sc.score(g, x, noise)
    sc.embed(g, x, noise)
    sc.rows(g, x, noise)
    assert pkg.ops.noise_state(dev).tolist() == [7, 7]  # explicit noise: no draw
    torch.cuda.synchronize()
    for kk, v in ft.state_dict().items():
        assert same_bits(v, sd[kk]), kk


@pytest.mark.parametrize("explicit", [False, True], ids=["drawn", "noise-given"])
def test_launches_of_a_resident_score_step(pkg, dev, monkeypatch, explicit):
    ft, k = _trained(pkg, dev, "L5-k1")
    g = C.batch_of(pkg, C.random_mols(pkg, 10, "molhiv", 34)).to(dev)
    x = g.ndata["x"].float()
    sc = pkg.infer.Scorer(ft, "resident")
    noise = _noise(g.num_nodes(), 17, dev) if explicit else None
    sc.score(g, x, noise)  # (lazy state: noise stream, error word, parameter table)
    real_call, calls = pkg._lib.call, []

    def counting_call(name, *args):
        calls.append(name)
        return real_call(name, *args)

    monkeypatch.setattr(pkg._lib, "call", counting_call)
    sc.score(g, x, noise)
    monkeypatch.setattr(pkg._lib, "call", real_call)
    torch.cuda.synchronize()
    ego = [c for c in calls if c.startswith("scgib_egonet")]
    rest = [c for c in calls if not c.startswith("scgib_egonet")]
    assert 1 <= len(ego) <= 2, calls
    assert rest == ([] if explicit else ["scgib_noise_uniform"]) + ["scgib_infer_fwd",
                                                                    "scgib_head_fwd"], calls
    for c in calls:
        assert not c.startswith(("scgib_gin_", "scgib_interaction_", "scgib_mlp2_",
                                 "scgib_set2set")), c


# ---------------------------------------------------------------------------
# 5. the captured dataset pass
# ---------------------------------------------------------------------------
B_DS, SENT = 32, -7.0


@pytest.fixture(scope="module")
def ds_case(pkg, dev):
    return _ds_case(pkg, dev)


@functools.lru_cache(maxsize=None)
def _ds_case(pkg, dev):
    mols = pkg.synth.molecules(80, "molhiv", seed=12)
    mols = [(ei, F.normalize(torch.from_numpy(np.asarray(x, np.float32))).numpy())
            for ei, x in mols]
    idx = np.random.default_rng(2).permutation(80)[:70]  # three batches, the last: 6 + 26 fill
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, 1)
    static = eval_static(pkg, ds, B_DS, dev, idx)
    noise = _noise(static.n_cap, 18, dev)
    return mols, idx, ds, static, noise


@pytest.mark.parametrize("path", ["resident", "layers"])
def test_dataset_pass_equals_eager_batches(pkg, dev, ds_case, path):
    mols, idx, ds, static, noise = ds_case
    ft, k = _trained(pkg, dev, "L5-k1")
    assert len(idx) % B_DS != 0
    evl = pkg.graph.DeviceEvalLoader(ds, static, indices=idx)
    assert evl.steps == 3
    out = torch.full((len(ds), 1), SENT, device=dev)
    got = pkg.infer.score_dataset(ft, evl, out=out, noise=noise, path=path)
    assert got is out
    emb = pkg.infer.DatasetEmbedding(ds)
    for t in (emb.z1, emb.z2, emb.pooled):
        t.fill_(SENT)
    pkg.infer.embed_dataset(ft, evl, out=emb, noise=noise, path=path)
    sc = pkg.infer.Scorer(ft, path)
    want = {n: torch.full_like(t, SENT) for n, t in
            (("scores", out), ("z1", emb.z1), ("z2", emb.z2), ("pooled", emb.pooled))}
    batches = batches_of(mols, idx, B_DS)
    assert (batches[-1][1] < 0).sum() > 0
    for rows, marked in batches:
        g = pkg.graph.collate_pyg([mols[int(i)] for i in rows])[0].to(dev)
        x, n = g.ndata["x"].float(), g.num_nodes()
        nz = (noise[0][:n], noise[1][:n])
        s, e = sc.score(g, x, nz), sc.embed(g, x, nz)
        for j, i in enumerate(marked):
            if i >= 0:
                for name, t in (("scores", s), ("z1", e.z1), ("z2", e.z2), ("pooled", e.pooled)):
                    want[name][int(i)] = t[j]
    in_subset = torch.zeros(len(ds), dtype=torch.bool, device=dev)
    in_subset[torch.from_numpy(idx).to(dev)] = True
    for name, t in (("scores", out), ("z1", emb.z1), ("z2", emb.z2), ("pooled", emb.pooled)):
        assert same_bits(t, want[name]), name  # every molecule's row: its eager row, bitwise
        assert not (t[in_subset] == SENT).any(), name
        assert (t[~in_subset] == SENT).all(), name  # fill rows and other molecules: untouched
    # two more passes of the same captured step change nothing
    again = pkg.infer.score_dataset(ft, evl, out=out.clone(), noise=noise, path=path, passes=2)
    assert same_bits(again, out)
    assert evl.error() == 0
