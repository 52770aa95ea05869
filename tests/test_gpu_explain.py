"""Graph cores and significant subgraphs on the MI355X (csrc/explain.hip,
DESIGN.md §26): the gate / logit tensors against what the training forward
saves, lam and alpha against the reference (train-mode goldens through two
derivations, the eval-mode golden directly) and against the fp64 restatement,
ranks / centres / cores against the numpy reference bit for bit, the captured
dataset pass against eager per-batch results, poisoned workspaces, and
``explain`` on the four model classes."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import explain_ref as E
import poison
from big_graphs import directed
from conftest import MODEL_GOLDENS, load_golden, rel_err
from eval_loader_cases import batches_of, eval_static
from oracle import scgib_ref as R
from test_explain_cpu import golden_case

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-4  # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _args(**over):
    base = dict(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32, batch_size=8,
                gin_layers=5, task="graph_classification", dataset="ogbg-molhiv")
    base.update(over)
    return SimpleNamespace(**base)


def _heads(params, dev):
    """(compressor, attn_layer) modules holding a golden's parameters."""
    comp = nn.Sequential(nn.Linear(64, 64), nn.BatchNorm1d(64), nn.ReLU(), nn.Linear(64, 1))
    attn = nn.Linear(128, 1)
    for mod, pfx in ((comp, "compressor."), (attn, "attn_layer.")):
        mod.load_state_dict({k[len(pfx):]: torch.as_tensor(v) for k, v in params.items()
                             if k.startswith(pfx)})
    return comp.to(dev), attn.to(dev)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------
# 1. gates: the tensors the training forward saves, and no state moved
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("use_att", [True, False])
def test_gates_are_the_saved_tensors_and_move_no_state(pkg, dev, training, use_att):
    torch.manual_seed(3)
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(37, "qm9", seed=3))
    g = gh.to(dev)
    n = g.num_nodes()
    comp = nn.Sequential(nn.Linear(64, 64), nn.BatchNorm1d(64), nn.ReLU(), nn.Linear(64, 1))
    with torch.no_grad():
        comp[1].running_mean.normal_()
        comp[1].running_var.uniform_(0.5, 2.0)
        comp[1].weight.add_(0.2 * torch.randn(64))
    comp, attn = comp.to(dev).train(training), nn.Linear(128, 1).to(dev)
    f, s = torch.randn(n, 64, device=dev), torch.randn(n, 64, device=dev)
    u_gate, u_feat = torch.rand(n, device=dev), torch.rand(n, 64, device=dev)
    pkg.ops.seed_noise(dev, 11)
    before = {k: v.clone() for k, v in comp.state_dict().items()}
    noise0 = pkg.ops.noise_state(dev).clone()
    lam, logit = pkg.ops.interaction_gates(f, s, u_gate, comp, attn, g, training, use_att)
    torch.cuda.synchronize()
    for k, v in comp.state_dict().items():
        assert same_bits(v, before[k]), k
    assert torch.equal(pkg.ops.noise_state(dev), noise0)
    out = pkg.ops.interaction_lin(f.clone().requires_grad_(True), s, u_gate, u_feat, comp, attn, g,
                                  training, use_att)
    saved = out[0].grad_fn.saved_tensors
    assert same_bits(lam, saved[9])
    if use_att:
        assert same_bits(logit, saved[10])
    else:
        assert logit is None
    if training:  # (the training forward did move them: the check above has teeth)
        assert int(comp[1].num_batches_tracked) > int(before["1.num_batches_tracked"])
        assert not same_bits(comp[1].running_mean, before["1.running_mean"])
    # u_gate=None is the median gate
    lam_h, _ = pkg.ops.interaction_gates(f, s, None, comp, attn, g, training, use_att)
    lam_5, _ = pkg.ops.interaction_gates(f, s, torch.full((n,), 0.5, device=dev), comp, attn, g,
                                         training, use_att)
    assert same_bits(lam_h, lam_5)


# ---------------------------------------------------------------------------
# 2. against the reference through the train-mode goldens
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODEL_GOLDENS)
def test_lam_and_alpha_match_reference_goldens(pkg, dev, name):
    c = golden_case(name)
    g = c.g
    bg = pkg.graph.GraphBatch.from_edges(g["src"], g["dst"], len(g["x_raw"]), True,
                                         g["batch_num_nodes"]).to(dev)
    comp, attn = _heads(c.params, dev)
    f = torch.tensor(g["act_graph_features"], device=dev)
    ego_ptr = torch.tensor(E.gptr_of(g["ego_batch_num_nodes"]), dtype=torch.int32, device=dev)
    s = pkg.ops.segment_sum(torch.tensor(g["act_subgraph_features"], device=dev), ego_ptr,
                            len(g["ego_batch_num_nodes"]))
    lam, logit = pkg.ops.interaction_gates(f, s, torch.tensor(g["u_gate"], device=dev),
                                           comp.train(), attn, bg, True)
    alpha = pkg.ops.explain_rank(lam, logit, bg, 0)[0]
    lam, alpha = lam.cpu().numpy(), alpha.cpu().numpy()
    u = c.usable
    figures = {"alpha vs reference": rel_err(alpha, c.alpha_d),
               "lam vs reference": rel_err(lam[u], c.lam_d[u]),
               "alpha vs fp64": rel_err(alpha, c.alpha64), "lam vs fp64": rel_err(lam, c.lam64)}
    print(name, {k: f"{v:.2e}" for k, v in figures.items()}, "rows left out for lam:",
          int((~u).sum()), "of", len(u))
    assert (~u).sum() <= 0.05 * len(u)
    for k, v in figures.items():
        assert v < ACT_TOL, (k, v)


# ---------------------------------------------------------------------------
# 3. against the reference in eval mode
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eval_golden(pkg, dev):
    g = load_golden("explain_eval_L5_k1")
    model = pkg.models.Mainmodel(_args(gin_layers=int(g["L"])), int(g["F"]), 64, 4, 4,
                                 int(g["k"]), "GIN")
    sd = {k[6:]: torch.tensor(v) for k, v in g.items() if k.startswith("param_")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected
    assert not [m for m in missing if m.startswith(("transfer_d.", "Encoder", "compressor.",
                                                    "attn_layer."))]
    bg = pkg.graph.GraphBatch.from_edges(g["src"], g["dst"], len(g["x_raw"]), True,
                                         g["batch_num_nodes"]).to(dev)
    x = F.normalize(torch.tensor(g["x_raw"]).float()).to(dev)
    return SimpleNamespace(g=g, model=model.to(dev).eval(), bg=bg, x=x)


def test_eval_mode_matches_reference(pkg, dev, eval_golden):
    c, g = eval_golden, eval_golden.g
    assert 2 in g["batch_num_nodes"]
    ex = c.model.explain(c.bg, c.x, u_gate=torch.tensor(g["u_gate"], device=dev))
    e_lam = rel_err(ex.lam.cpu().numpy(), g["lam_ref"])
    e_alpha = rel_err(ex.alpha.cpu().numpy(), g["alpha_ref"])
    med = c.model.explain(c.bg, c.x, u_gate=None)
    sig = 1.0 / (1.0 + np.exp(-g["p_ref"].astype(np.float64)))
    e_med = rel_err(med.lam.cpu().numpy(), sig)
    print(f"eval golden: lam {e_lam:.2e} alpha {e_alpha:.2e} median gate {e_med:.2e}")
    assert e_lam < ACT_TOL and e_alpha < ACT_TOL and e_med < ACT_TOL
    # host-built ego-nets (the reference's own) give the same explanation
    ego = pkg.graph.GraphBatch.from_edges(g["ego_src"], g["ego_dst"],
                                          int(g["ego_batch_num_nodes"].sum()), True,
                                          g["ego_batch_num_nodes"]).to(dev)
    x_subs = c.x[torch.tensor(g["ego_nodes_global"], device=dev)]
    ex2 = c.model.explain(c.bg, c.x, ego, x_subs, u_gate=torch.tensor(g["u_gate"], device=dev))
    assert rel_err(ex2.lam.cpu().numpy(), g["lam_ref"]) < ACT_TOL
    assert rel_err(ex2.alpha.cpu().numpy(), g["alpha_ref"]) < ACT_TOL


# ---------------------------------------------------------------------------
# 4. ranks and centres: exactly the numpy reference, on the device's own keys
# ---------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 600]


def _edgeless(pkg, counts, dev):
    e = np.zeros(0, np.int64)
    return pkg.graph.GraphBatch.from_edges(e, e, int(np.sum(counts)), True,
                                           np.asarray(counts, np.int64)).to(dev)


def _keys(kind, n, rng):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    k = rng.standard_normal(n).astype(np.float32)
    if kind == "equal":
        k[:] = 0.25
    elif kind == "two":
        k = rng.choice(np.array([0.5, -1.5], np.float32), n)
    elif kind == "nan":
        k[rng.random(n) < 0.3] = nan
        k[:3] = nan  # the 1- and 2-atom molecules: all NaN
    elif kind == "inf":
        k[rng.random(n) < 0.2] = inf
        k[rng.random(n) < 0.2] = -inf
    elif kind == "zero":
        k = rng.choice(np.array([0.0, -0.0, 1e-38, -1e-38], np.float32), n)
    return k


def _check_ranks(pkg, dev, counts, lam, logit, top_m):
    g = _edgeless(pkg, counts, dev)
    gptr = E.gptr_of(counts)
    out = pkg.ops.explain_rank(torch.tensor(lam, device=dev), torch.tensor(logit, device=dev), g,
                               top_m)
    alpha, lam_rank, alpha_rank, cen, wts = [t.cpu().numpy() for t in out]
    assert lam_rank.dtype == alpha_rank.dtype == cen.dtype == np.int32
    assert np.array_equal(lam_rank, E.ranks(lam, gptr))
    want = E.ranks(alpha, gptr)  # on the device's own float keys: no molecule left out
    assert np.array_equal(alpha_rank, want)
    c_ref, w_ref = E.centres(alpha, want, gptr, top_m)
    assert np.array_equal(cen, c_ref)
    assert np.array_equal(wts.view(np.int32), w_ref.view(np.int32))
    return alpha


@pytest.mark.parametrize("top_m", [1, 3, 5])
@pytest.mark.parametrize("kind", ["random", "equal", "two", "nan", "inf", "zero"])
def test_ranks_and_centres_exact(pkg, dev, kind, top_m):
    rng = np.random.default_rng(len(kind) + top_m)
    n = sum(SIZES)
    lam = _keys(kind, n, rng)
    # the attention keys are alpha = softmax(logit): ties, NaN and +-0 reach
    # alpha_rank through logits that are equal, NaN, or far below the maximum
    logit = _keys(kind, n, rng)
    if kind == "zero":
        logit = np.where(rng.random(n) < 0.5, np.float32(-200.0), np.float32(0.0))
        logit[-600] = 0.0  # (a maximum of 0 in the large molecule: exp(-200) underflows to +0)
    alpha = _check_ranks(pkg, dev, SIZES, lam, logit, top_m)
    if kind == "zero":
        assert (alpha[-600:] == 0).sum() > 100


@pytest.mark.parametrize("B", [1, 300])
def test_ranks_batch_sizes(pkg, dev, B):
    rng = np.random.default_rng(B)
    counts = rng.integers(1, 41, size=B)
    n = int(counts.sum())
    _check_ranks(pkg, dev, counts, rng.standard_normal(n).astype(np.float32),
                 rng.standard_normal(n).astype(np.float32), 3)


def test_softmax_cases(pkg, dev):
    gptr = E.gptr_of(SIZES)
    n = int(gptr[-1])
    g = _edgeless(pkg, SIZES, dev)
    lam = torch.zeros(n, device=dev)
    # logits spanning 200 inside every molecule: no overflow, no NaN
    span = np.concatenate([np.linspace(-100.0, 100.0, c) if c > 1 else np.zeros(1)
                           for c in SIZES]).astype(np.float32)
    alpha = pkg.ops.explain_rank(lam, torch.tensor(span, device=dev), g, 0)[0].cpu().numpy()
    assert np.isfinite(alpha).all()
    # expf within 2 ulp, one division, a fixed-order sum of at most 600 terms
    # of which about e / (e - 1) carry weight: a few fp32 roundings of the maximum
    assert rel_err(alpha, E.softmax_ref(span, gptr)) < 2e-6
    assert np.abs(np.add.reduceat(alpha.astype(np.float64), gptr[:-1]) - 1).max() < 2e-6
    # all-equal logits: exactly 1 / n_i; a single atom: exactly 1
    alpha = pkg.ops.explain_rank(lam, torch.full((n,), 3.5, device=dev), g, 0)[0].cpu().numpy()
    want = np.repeat(np.float32(1) / np.asarray(SIZES, np.float32), SIZES)
    assert np.array_equal(alpha.view(np.int32), want.view(np.int32))
    assert alpha[0] == 1.0
    # bitwise reproducible
    again = pkg.ops.explain_rank(lam, torch.tensor(span, device=dev), g, 0)[0]
    first = pkg.ops.explain_rank(lam, torch.tensor(span, device=dev), g, 0)[0]
    assert same_bits(again, first)


def test_no_attention_ranks_only_lam(pkg, dev):
    counts = [3, 70, 1]
    rng = np.random.default_rng(0)
    lam = rng.standard_normal(74).astype(np.float32)
    g = _edgeless(pkg, counts, dev)
    alpha, lam_rank, alpha_rank, cen, wts = pkg.ops.explain_rank(torch.tensor(lam, device=dev),
                                                                 None, g, 0)
    assert alpha is None and alpha_rank is None and cen is None and wts is None
    assert np.array_equal(lam_rank.cpu().numpy(), E.ranks(lam, E.gptr_of(counts)))
    with pytest.raises(pkg._lib.ScgibError, match="useAtt"):
        pkg.ops.explain_rank(torch.tensor(lam, device=dev), None, g, 2)


# ---------------------------------------------------------------------------
# 5. the core against dgl.node_subgraph, bit for bit
# ---------------------------------------------------------------------------
def _paths(counts, loops=()):
    """Bidirected paths of the given sizes (+ self-loops at the listed global
    ids): (src, dst, counts)."""
    src, dst, off = [], [], 0
    for c in counts:
        for i in range(c - 1):
            src += [off + i, off + i + 1]
            dst += [off + i + 1, off + i]
        off += c
    for v in loops:
        src.append(v)
        dst.append(v)
    return np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(counts, np.int64)


def _molecule_graph(pkg, B, seed):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=seed))
    s, d = gh.edges()
    return s.numpy(), d.numpy(), gh.batch_num_nodes_host()


RULES = [("ratio", 1e-9), ("ratio", 0.5), ("ratio", 1.0), ("threshold", 9.0), ("threshold", -9.0)]


def _check_core(pkg, dev, src, dst, counts, lam, rule, value, symmetric=True):
    n = int(np.sum(counts))
    g = pkg.graph.GraphBatch.from_edges(src, dst, n, symmetric, counts).to(dev)
    gptr = E.gptr_of(counts)
    lam_d = torch.tensor(lam, device=dev)
    lam_rank = pkg.ops.explain_rank(lam_d, None, g, 0)[1]
    assert np.array_equal(lam_rank.cpu().numpy(), E.ranks(lam, gptr))
    core, mask = pkg.ops.core_subgraph(lam_d, lam_rank, g, **{rule: value})
    keep = E.core_keep(lam, E.ranks(lam, gptr), gptr, **{rule: value})
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), keep)
    # out-CSR (rows = src), what dgl.node_subgraph slices ...
    rowptr, col, gp, ids = E.core_reference(src, dst, gptr, keep)
    assert np.array_equal(core.rowptr_t.cpu().numpy(), rowptr)
    assert np.array_equal(core.col_t.cpu().numpy()[:len(col)], col)
    assert core.num_edges() == len(col) and core.num_nodes() == len(ids)
    assert np.array_equal(core.graph_ptr.cpu().numpy(), gp)
    assert np.array_equal(core.ndata["_ID"].cpu().numpy(), ids)
    assert core.ndata["_ID"].dtype == torch.int32
    # ... and the in-CSR the kernels walk: the same slice of the reversed graph
    rowptr, col, _, _ = E.core_reference(dst, src, gptr, keep)
    assert np.array_equal(core.rowptr.cpu().numpy(), rowptr)
    assert np.array_equal(core.col.cpu().numpy()[:len(col)], col)
    return core, keep


@pytest.mark.parametrize("rule,value", RULES)
def test_core_of_molecules(pkg, dev, rule, value):
    src, dst, counts = _molecule_graph(pkg, 23, 4)
    lam = np.random.default_rng(1).random(int(counts.sum())).astype(np.float32)
    core, keep = _check_core(pkg, dev, src, dst, counts, lam, rule, value)
    if (rule, value) == ("ratio", 1e-9):
        assert keep.sum() == len(counts)  # m_i = 1
    if (rule, value) == ("threshold", 9.0):
        assert core.num_nodes() == 0 and core.num_edges() == 0
        assert core.graph_ptr.cpu().tolist() == [0] * (len(counts) + 1)
    if value in (1.0, -9.0):
        assert keep.all()


@pytest.mark.parametrize("rule,value", [("ratio", 0.5), ("threshold", 0.4)])
def test_core_self_loops_and_isolated_kept_atom(pkg, dev, rule, value):
    # paths of 5, 2 and 6 atoms, self-loops at 1, 2 and 9; lam chosen so that atom 0
    # is kept while its only neighbour (atom 1) is dropped
    src, dst, counts = _paths([5, 2, 6], loops=(1, 2, 9))
    lam = np.array([0.9, 0.1, 0.8, 0.7, 0.2, 0.5, 0.3, 0.1, 0.9, 0.8, 0.2, 0.7, 0.1],
                   np.float32)
    core, keep = _check_core(pkg, dev, src, dst, counts, lam, rule, value)
    assert keep[0] and not keep[1]
    rp = core.rowptr.cpu().numpy()
    assert rp[1] - rp[0] == 0  # the kept atom 0 has no kept neighbour
    assert keep[2] and (core.col.cpu().numpy()[rp[1]:rp[2]] == 1).any()  # its self-loop, relabelled


@pytest.mark.parametrize("rule,value", [("ratio", 0.5), ("threshold", 0.5)])
def test_core_of_a_directed_graph(pkg, dev, rule, value):
    src, dst, n = directed(50)
    lam = np.random.default_rng(5).random(n).astype(np.float32)
    _check_core(pkg, dev, src, dst, np.array([n]), lam, rule, value, symmetric=False)


@pytest.mark.parametrize("rows", [255, 256, 257])
def test_core_at_the_block_edge(pkg, dev, rows):
    counts = [100, 2, rows - 102 - 31, 31]
    src, dst, counts = _paths(counts)
    lam = np.random.default_rng(rows).random(rows).astype(np.float32)
    _check_core(pkg, dev, src, dst, counts, lam, "ratio", 0.5)
    _check_core(pkg, dev, src, dst, counts, lam, "threshold", 0.3)


def test_core_of_a_large_batch(pkg, dev):
    """About 70 k rows: 274 scan blocks, so the fix-up's 256 threads each
    reduce more than one block record."""
    rng = np.random.default_rng(9)
    counts = rng.integers(2, 120, size=1180)
    assert 256 * 257 < counts.sum() < 80000
    src, dst, counts = _paths(counts.tolist())
    lam = rng.random(int(counts.sum())).astype(np.float32)
    _check_core(pkg, dev, src, dst, counts, lam, "ratio", 0.5)


# ---------------------------------------------------------------------------
# 6. capacity mode and capture
# ---------------------------------------------------------------------------
B_DS, SENT_F, SENT_I = 32, -7.0, -77


@pytest.fixture(scope="module")
def ds_case(pkg, dev):
    mols = pkg.synth.molecules(80, "qm9", seed=12)
    mols = [(ei, F.normalize(torch.from_numpy(np.asarray(x, np.float32))).numpy())
            for ei, x in mols]
    idx = np.random.default_rng(2).permutation(80)[:70]  # three batches, the last: 6 + 26 fill
    ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, 1)
    static = eval_static(pkg, ds, B_DS, dev, idx)
    torch.manual_seed(12)
    inner = pkg.models.Mainmodel(_args(), ds.num_features, 64, 4, 4, 1, "GIN")
    model = pkg.models.Mainmodel_continue(_args(), ds.num_features, 64, 4, 4, 1, 1, inner, "GIN")
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.normal_(0.0, 0.3)
                m.running_var.uniform_(0.5, 2.0)
    return SimpleNamespace(mols=mols, idx=idx, ds=ds, static=static, model=model.to(dev).eval())


def _sentinel_out(pkg, ds):
    out = pkg.explain.DatasetExplanation(ds)
    out.lam.fill_(SENT_F)
    out.alpha.fill_(SENT_F)
    out.lam_rank.fill_(SENT_I)
    out.alpha_rank.fill_(SENT_I)
    return out


def test_dataset_pass_equals_eager_batches(pkg, dev, ds_case):
    c = ds_case
    out = pkg.explain.explain_dataset(c.model, c.ds, c.static, c.idx, out=_sentinel_out(pkg, c.ds))
    got = [t.clone() for t in out.arrays()]
    off = c.ds.host["node_off"]
    want = [t.clone() for t in _sentinel_out(pkg, c.ds).arrays()]
    batches = batches_of(c.mols, c.idx, B_DS)
    assert len(batches) == 3 and (batches[-1][1] < 0).sum() > B_DS // 2  # mostly fill
    for rows, marked in batches:
        g = pkg.graph.collate_pyg([c.mols[int(i)] for i in rows])[0].to(dev)
        ex = c.model.explain(g, g.ndata["x"].float(), top_m=0)
        gp = g.graph_ptr.cpu().numpy()
        for j, i in enumerate(marked):
            if i < 0:
                continue
            a, b = int(off[i]), int(off[i + 1])
            assert b - a == gp[j + 1] - gp[j]
            for w, t in zip(want, (ex.lam, ex.alpha, ex.lam_rank, ex.alpha_rank)):
                w[a:b] = t[gp[j]:gp[j + 1]]
    in_subset = np.zeros(int(off[-1]), bool)
    for i in c.idx:
        in_subset[off[i]:off[i + 1]] = True
    sel = torch.from_numpy(in_subset).to(dev)
    for name, gt, wt in zip(("lam", "alpha", "lam_rank", "alpha_rank"), got, want):
        assert same_bits(gt, wt), name
        sentinel = SENT_F if gt.is_floating_point() else SENT_I
        assert not (gt[sel] == sentinel).any(), name  # every subset row written
        assert (gt[~sel] == sentinel).all(), name  # nothing outside the subset
    # a second and third pass of the same captured step change nothing
    pkg.explain.explain_dataset(c.model, c.ds, c.static, c.idx, out=out, passes=2)
    for name, gt, t in zip(("lam", "alpha", "lam_rank", "alpha_rank"), got, out.arrays()):
        assert same_bits(gt, t), name
    # the stored arrays give the core rule without a batch
    m = out.core_mask(ratio=0.5).cpu().numpy()
    assert np.array_equal(m[in_subset], E.core_keep(None, got[2].cpu().numpy(), off,
                                                    ratio=0.5)[in_subset])


def test_store_skips_fill_rows(pkg, dev):
    counts = [3, 4, 3, 2]  # the batch: molecules 2, fill (a copy of 2), 0, and an id out of range
    g = _edgeless(pkg, counts, dev)
    node_off = torch.tensor([0, 3, 8, 11], dtype=torch.int64, device=dev)  # molecules of 3, 5, 3
    ids = torch.tensor([2, -1, 0, 7], dtype=torch.int32, device=dev)
    n = sum(counts)
    lam = torch.arange(n, dtype=torch.float32, device=dev) + 100
    rank = torch.arange(n, dtype=torch.int32, device=dev)
    out = (torch.full((11,), SENT_F, device=dev), torch.full((11,), SENT_F, device=dev),
           torch.full((11,), SENT_I, dtype=torch.int32, device=dev),
           torch.full((11,), SENT_I, dtype=torch.int32, device=dev))
    pkg.ops.explain_store(lam, lam + 0.5, rank, rank + 1, g, ids, node_off, out)
    s = SENT_F
    assert out[0].cpu().tolist() == [107, 108, 109, s, s, s, s, s, 100, 101, 102]
    assert out[1].cpu().tolist() == [107.5, 108.5, 109.5, s, s, s, s, s, 100.5, 101.5, 102.5]
    t = SENT_I
    assert out[2].cpu().tolist() == [7, 8, 9, t, t, t, t, t, 0, 1, 2]
    assert out[3].cpu().tolist() == [8, 9, 10, t, t, t, t, t, 1, 2, 3]


def test_capacity_mode_defines_the_padding(pkg, dev, ds_case):
    """A static batch: rows past dims[0] get alpha 0, ranks -1, mask 0; the
    core is sized by the capacities with its sizes in core.dims; live rows are
    bitwise the eager batch's."""
    c = ds_case
    rows = batches_of(c.mols, c.idx, B_DS)[2][0]
    gh = pkg.graph.collate_pyg([c.mols[int(i)] for i in rows])[0]
    c.static.load(c.static.pad(gh))
    g = c.static.graph
    n, cap = gh.num_nodes(), g.num_nodes()
    assert cap > n + 64
    ex_c = c.model.explain(g, c.static.x, top_m=3)
    ge = gh.to(dev)
    ex_e = c.model.explain(ge, ge.ndata["x"].float(), top_m=3)
    torch.cuda.synchronize()
    for name in ("lam", "alpha", "lam_rank", "alpha_rank", "core_mask"):
        a, b = getattr(ex_c, name), getattr(ex_e, name)
        assert same_bits(a[:n], b), name
    assert same_bits(ex_c.centres, ex_e.centres) and same_bits(ex_c.weights, ex_e.weights)
    assert (ex_c.alpha[n:] == 0).all() and (ex_c.lam_rank[n:] == -1).all()
    assert (ex_c.alpha_rank[n:] == -1).all() and not ex_c.core_mask[n:].any()
    nc, ec = ex_c.core.dims.cpu().tolist()
    assert (nc, ec) == (ex_e.core.num_nodes(), ex_e.core.num_edges())
    assert torch.equal(ex_c.core.rowptr[:nc + 1], ex_e.core.rowptr)
    assert (ex_c.core.rowptr[nc:] == ec).all()  # empty rows past the core
    assert torch.equal(ex_c.core.col[:ec], ex_e.core.col[:ec])
    assert torch.equal(ex_c.core.graph_ptr, ex_e.core.graph_ptr)
    assert torch.equal(ex_c.core.ndata["_ID"][:nc], ex_e.core.ndata["_ID"])


# ---------------------------------------------------------------------------
# 7. poisoned fresh workspaces
# ---------------------------------------------------------------------------
def test_explain_ops_ignore_workspace_contents(pkg, dev):
    def build():
        torch.manual_seed(8)
        gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(40, "qm9", seed=8))
        g = gh.to(dev)
        n = g.num_nodes()
        comp = nn.Sequential(nn.Linear(64, 64), nn.BatchNorm1d(64), nn.ReLU(),
                             nn.Linear(64, 1)).to(dev).eval()
        attn = nn.Linear(128, 1).to(dev)
        f, s = torch.randn(n, 64, device=dev), torch.randn(n, 64, device=dev)
        ids = torch.arange(40, dtype=torch.int32, device=dev)
        ids[5] = -1
        out = (torch.zeros(n, device=dev), torch.zeros(n, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev))
        return SimpleNamespace(g=g, comp=comp, attn=attn, f=f, s=s, ids=ids, out=out,
                               node_off=g.graph_ptr.to(torch.int64))

    def run(c):
        res = {}
        for training in (False, True):
            lam, logit = pkg.ops.interaction_gates(c.f, c.s, None, c.comp.train(training), c.attn,
                                                   c.g, training)
            res[f"lam{training}"], res[f"logit{training}"] = lam, logit
        alpha, lam_rank, alpha_rank, cen, wts = pkg.ops.explain_rank(lam, logit, c.g, 4)
        res.update(alpha=alpha, lam_rank=lam_rank, alpha_rank=alpha_rank, cen=cen, wts=wts)
        for tag, kw in (("r", {"ratio": 0.3}), ("t", {"threshold": 0.5})):
            core, mask = pkg.ops.core_subgraph(lam, lam_rank, c.g, **kw)
            res.update({tag + "_rowptr": core.rowptr, tag + "_col": core.col,
                        tag + "_gptr": core.graph_ptr, tag + "_id": core.ndata["_ID"],
                        tag + "_mask": mask})
        pkg.ops.explain_store(lam, alpha, lam_rank, alpha_rank, c.g, c.ids, c.node_off, c.out)
        res.update(s_lam=c.out[0], s_alpha=c.out[1], s_lr=c.out[2], s_ar=c.out[3])
        return res

    results = poison.run_thrice(build, run)
    assert torch.isfinite(results[0]["alpha"]).all()
    poison.assert_same(results)


# ---------------------------------------------------------------------------
# 8. the four model classes
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(pkg, dev):
    mols = pkg.synth.molecules(9, "qm9", seed=6)
    gh, _ = pkg.graph.collate_pyg(mols)
    g = gh.to(dev)
    return SimpleNamespace(g=g, x=F.normalize(g.ndata["x"].float()), gptr=E.gptr_of(
        gh.batch_num_nodes_host()), F=int(g.ndata["x"].shape[1]))


def _four(pkg, dev, f_in, **over):
    args = _args(**over)
    torch.manual_seed(1)
    inner = pkg.models.Mainmodel(args, f_in, 64, 4, 4, 1, "GIN")
    pre = pkg.models.Mainmodel_continue(args, f_in, 64, 4, 4, 1, 1, inner, "GIN")
    da = pkg.models.Mainmodel_domainadapt(args, f_in, 64, 4, 4, 1, 1, pre, "GIN")
    ft = pkg.models.Mainmodel_finetuning(args, f_in, 64, 4, 4, 1, 1, pre, "GIN")
    return {"Mainmodel": inner, "Mainmodel_continue": pre, "Mainmodel_domainadapt": da,
            "Mainmodel_finetuning": ft}


def _state_bits(model, pkg, dev):
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return sd, pkg.ops.noise_state(dev).clone()


@pytest.mark.parametrize("cls", ["Mainmodel", "Mainmodel_continue", "Mainmodel_domainadapt",
                                 "Mainmodel_finetuning"])
@pytest.mark.parametrize("readout", ["sum", "set2set"])
def test_explain_on_the_four_model_classes(pkg, dev, batch, cls, readout):
    model = _four(pkg, dev, batch.F, readout_f=readout)[cls].to(dev).eval()
    pkg.ops.seed_noise(dev, 5)
    sd, noise = _state_bits(model, pkg, dev)
    ex = model.explain(batch.g, batch.x, ratio=0.4, top_m=2)
    torch.cuda.synchronize()
    assert isinstance(ex, pkg.models.Explanation)
    for k, v in model.state_dict().items():
        assert same_bits(v, sd[k]), k
    assert torch.equal(pkg.ops.noise_state(dev), noise)
    n, gptr = batch.g.num_nodes(), batch.gptr
    lam, alpha = ex.lam.cpu().numpy(), ex.alpha.cpu().numpy()
    assert lam.shape == alpha.shape == (n,) and ((lam > 0) & (lam < 1)).all()
    assert np.array_equal(ex.lam_rank.cpu().numpy(), E.ranks(lam, gptr))
    assert np.array_equal(ex.alpha_rank.cpu().numpy(), E.ranks(alpha, gptr))
    keep = E.core_keep(lam, E.ranks(lam, gptr), gptr, ratio=0.4)
    assert np.array_equal(ex.core_mask.cpu().numpy(), keep)
    assert np.array_equal(ex.core.ndata["_ID"].cpu().numpy(), np.flatnonzero(keep))
    assert np.array_equal(np.diff(ex.core.graph_ptr.cpu().numpy()), E.core_sizes(gptr, 0.4))
    c_ref, w_ref = E.centres(alpha, E.ranks(alpha, gptr), gptr, 2)
    assert np.array_equal(ex.centres.cpu().numpy(), c_ref)
    assert np.array_equal(ex.weights.cpu().numpy(), w_ref)
    # the ego-net of a centre: the centre itself and its neighbours
    subs = ex.subgraph_nodes()
    assert len(subs) == 9 and all(len(s) == 2 and s[0][0] in s[0][2] for s in subs)
    # deterministic (u_gate=None), and a threshold replaces the ratio
    again = model.explain(batch.g, batch.x, ratio=0.4, top_m=2)
    assert same_bits(again.lam, ex.lam) and same_bits(again.alpha, ex.alpha)
    thr = model.explain(batch.g, batch.x, threshold=float(np.median(lam)), top_m=0)
    assert np.array_equal(thr.core_mask.cpu().numpy(), lam >= np.float32(np.median(lam)))
    assert thr.centres is None and thr.weights is None
    with pytest.raises(RuntimeError, match="eval"):
        model.train().explain(batch.g, batch.x)
    model.eval()


def test_explain_without_attention(pkg, dev, batch):
    model = _four(pkg, dev, batch.F, useAtt=0)["Mainmodel_continue"].to(dev).eval()
    with pytest.raises(ValueError, match="useAtt"):
        model.explain(batch.g, batch.x)  # top_m defaults to 3
    ex = model.explain(batch.g, batch.x, top_m=0)
    assert ex.alpha is None and ex.alpha_rank is None and ex.centres is None
    lam = ex.lam.cpu().numpy()
    assert np.array_equal(ex.lam_rank.cpu().numpy(), E.ranks(lam, batch.gptr))
    assert ex.core.num_nodes() == int(E.core_sizes(batch.gptr, 0.5).sum())


def test_explain_accepts_a_dgl_like_graph(pkg, dev, batch):
    model = _four(pkg, dev, batch.F)["Mainmodel"].to(dev).eval()
    ex = model.explain(batch.g, batch.x)
    s, d = batch.g.edges()
    duck = SimpleNamespace(edges=lambda: (s, d), num_nodes=lambda: batch.g.num_nodes(),
                           batch_num_nodes=lambda: batch.g.batch_num_nodes(),
                           ndata={"x": batch.x})
    ex2 = model.explain(duck, batch.x)
    assert same_bits(ex.lam, ex2.lam) and same_bits(ex.alpha, ex2.alpha)
    assert torch.equal(ex.core.col, ex2.core.col) and torch.equal(ex.centres, ex2.centres)
