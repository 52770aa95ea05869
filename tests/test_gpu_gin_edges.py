"""The fused GIN layers (csrc/gin_layer.hip, gin_bwd5.h, gin_bn.h) at the row
counts where they change code path: tile and sub-tile edges, full and one-row
statistics groups, the second finish round of a deferred layer (32769 rows),
the deferral limit == agg-free switch (65536) and one row past it (the
supergroup level), two full supergroups, capacity batches whose host sizing
and device statistics level disagree.  tests/gin_edge_cases.py holds the table
and each row's reason; tests/test_gin_edges_cpu.py pins the table to the
library's host queries.

Every case runs models.GIN (or ops.gin_encoder_x) forward and backward once on
a batch of exactly that many rows and checks it
  a. against oracle.scgib_ref.gin_encoder in fp64 with the kernels' own ReLU
     decisions at ties, as test_fused_gin_encoder does and at its bars;
  b. against the kernels' own saved z2: the BN record and the output, which
     takes GEMM rounding out and tests the statistics tree alone, at the bars
     of tests/test_gpu_enc_tail.py;
  c. dh0 on row blocks at the boundaries (a global L2 over 1e5 rows hides one
     bad row, a 64-row block does not);
  d. (the boundary-weighted passes) with the upstream gradient on the last 33
     rows only, and with the rows of the last tile scaled until they carry a
     share of the statistics that no bar can hide;
  e. in capacity mode: padding rows exact zeros, and a second forward after
     the valid count changed on the device.
Each step runs twice from equal state copies and must give the same bits
(determinism; every arrival counter was left reset).
"""
from __future__ import annotations

import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gin_edge_cases as E
from conftest import check_grads, gin_relu_masks, rel_err, rel_l2
from oracle import scgib_ref as R
from test_gpu_parity import ACT_TOL, GRAD_TOL  # 1e-4 max-norm | 1e-3 relative L2 (test_fused_gin_encoder)

pytestmark = pytest.mark.gpu

BUF_TOL = 1e-5    # running mean / var: test_fused_gin_encoder's bar
STAT_TOL = 1e-5   # BN record against fp64 statistics of the saved z2: tests/test_gpu_enc_tail.py's bar
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------
# one case: the batch, the module, the inputs
# ---------------------------------------------------------------------------
def _case(pkg, dev, n, training, cap=None, layers=None, fold=False, agg_free=None):
    """agg_free: the expected path of layers l >= 1 (None: the default switch,
    decided from the host row count — the capacity in capacity mode)."""
    layers = layers or E.case_layers(n)
    c = SimpleNamespace(n=n, cap=cap, rows=cap or n, training=training, layers=layers, fold=fold)
    if cap is None:
        c.gh = E.exact_graph(pkg, n)
        c.g, c.static = c.gh.to(dev), None
    else:
        c.static, c.gh = E.capacity_graph(pkg, n, cap, dev)
        c.g = c.static.graph
        assert c.g.num_nodes() == cap and c.g.dims is not None
    c.gin = E.make_gin(pkg, layers)
    c.h0, c.w = E.make_inputs(n, c.rows)
    if fold:
        c.x = F.normalize(c.gh.ndata["x"].float())
        torch.manual_seed(E.SEED + 7)
        c.lin = torch.nn.Linear(E.F_RAW, 32, bias=False)
    c.agg_free = (c.rows >= pkg.ops.AGG_FREE_MIN_ROWS) if agg_free is None else agg_free
    return c


def _device_step(pkg, dev, c, h0, w, backward=True):
    """Forward (and backward) on fresh device copies of the case's module."""
    gd = copy.deepcopy(c.gin).to(dev).train(c.training)
    L = c.layers
    if c.fold:
        lin = copy.deepcopy(c.lin).to(dev)
        hin = None
        out = pkg.ops.gin_encoder_x(c.x.to(dev), c.g, gd, lin)
    else:
        hin = h0.to(dev).requires_grad_(True)
        out = gd(c.g, hin)
    saved = list(out.grad_fn.saved_tensors[:4 * L])
    # the path under test was taken: layers l >= 1 store no agg exactly where agg-free
    assert [saved[4 * l] is None for l in range(L)] == [c.agg_free and l >= 1 for l in range(L)]
    r = SimpleNamespace(out=out.detach(), saved=saved, masks=gin_relu_masks(out, L), grads={},
                        dh0=None, module=gd)
    if backward:
        (w.to(dev) * out).sum().backward()
        r.grads = {k: p.grad for k, p in gd.named_parameters()}
        if c.fold:
            r.grads["wt"] = lin.weight.grad
        else:
            r.dh0 = hin.grad
    torch.cuda.synchronize()
    r.bufs = {k: b.detach().clone() for k, b in gd.named_buffers()}
    return r


def _same_bits(a, b):
    assert torch.equal(a.out, b.out)
    for l, (s, t) in enumerate(zip(a.saved, b.saved)):
        assert (s is None and t is None) or torch.equal(s, t), ("saved", l // 4, l % 4)
    assert a.grads.keys() == b.grads.keys()
    for k in a.grads:
        assert torch.equal(a.grads[k], b.grads[k]), k
    assert (a.dh0 is None and b.dh0 is None) or torch.equal(a.dh0, b.dh0)
    for k in a.bufs:
        assert torch.equal(a.bufs[k], b.bufs[k]), k


def _step_twice(pkg, dev, c, h0, w, backward=True):
    a = _device_step(pkg, dev, c, h0, w, backward)
    _same_bits(a, _device_step(pkg, dev, c, h0, w, backward))
    return a


def _oracle(c, h0, w, masks, backward=True):
    """oracle.scgib_ref.gin_encoder in fp64 over the valid rows, following the
    kernels' ReLU decisions at ties."""
    n = c.n
    p, bufs = E.oracle_params(c.gin)
    src, dst = c.gh.edges()
    o = SimpleNamespace(p=p, bufs=bufs, wt=None, h0=None)
    if c.fold:
        o.wt = c.lin.weight.detach().double().clone().requires_grad_(True)
        hin = c.x.double() @ o.wt.t()
    else:
        o.h0 = hin = h0[:n].double().requires_grad_(True)
    masks = [(m1[:n], m2[:n]) for m1, m2 in masks]
    o.out = R.gin_encoder(p, "Encoder1", src, dst, hin, bufs, c.layers, relu_masks=masks,
                          training=c.training)
    if backward:
        (w[:n].double() * o.out).sum().backward()
    return o


# ---------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------
def _check_oracle(c, r, o, backward=True):
    """a. output, gradients and BN buffers against the fp64 oracle."""
    n = c.n
    err = rel_err(r.out[:n].cpu(), o.out.detach())
    print(f"  out rel_err {err:.3g}")
    assert err < ACT_TOL, err
    if backward:
        if not c.fold:
            err = rel_l2(r.dh0[:n].cpu(), o.h0.grad)
            print(f"  dh0 rel_l2 {err:.3g}")
            assert err < GRAD_TOL, err
        else:
            err = rel_l2(r.grads["wt"].cpu(), o.wt.grad)
            print(f"  dWt rel_l2 {err:.3g}")
            assert err < GRAD_TOL, err
        grads = {k[len("Encoder1."):]: v.grad.numpy() for k, v in o.p.items() if v.grad is not None}
        assert len(grads) == 6 * c.layers
        # (a bias feeding a train-mode BatchNorm: zero in real arithmetic, conftest.CANCELLED)
        check_grads(grads, lambda k: r.grads[k], tol=GRAD_TOL,
                    cancelled=("mlp.2.bias",) if c.training else (), metric="l2")
    for k, v in o.bufs.items():  # train: updated once; eval: untouched
        mine = r.bufs[k[len("Encoder1."):]]
        if "num_batches" in k:
            assert int(mine) == int(v), k
        else:
            assert rel_err(mine.cpu(), v) < BUF_TOL, (k, rel_err(mine.cpu(), v))


def _check_saved(c, r, n=None):
    """b. every layer's BN record against fp64 statistics of the kernel's own
    saved z2 (eval: against the running statistics), and the output against
    relu(scale z2 + shift) of the last layer, element by element within the
    fp32 rounding of the fused multiply-add: 2 ulp of |scale z| + |shift|."""
    n = c.n if n is None else n
    for l in range(c.layers):
        z2, stat = r.saved[4 * l + 2][:n].cpu(), r.saved[4 * l + 3].cpu()
        bn = c.gin.batch_norms[l]
        if c.training:
            rec = E.bn_record(z2, bn.weight.detach(), bn.bias.detach())
        else:
            mean = bn.running_mean.double()
            istd = 1.0 / torch.sqrt(bn.running_var.double() + bn.eps)
            scale = bn.weight.detach().double() * istd
            rec = torch.stack([mean, istd, scale, bn.bias.detach().double() - mean * scale])
        for i, what in enumerate(("mean", "istd", "scale", "shift")):
            err = rel_err(stat[i], rec[i])
            assert err < STAT_TOL, (l, what, err)
    scale, shift = stat[2].double(), stat[3].double()
    sz = scale * z2.double()
    bound = 2 * EPS32 * (sz.abs() + shift.abs()) + 1e-30
    bad = ((r.out[:n].cpu().double() - torch.relu(sz + shift)).abs() > bound).nonzero()
    assert bad.numel() == 0, bad[:8].tolist()


def _check_blocks(c, r, o):
    """c. dh0 on the boundary row blocks, each at the global bar."""
    for name, rows in E.grad_blocks(c.n).items():
        err = rel_l2(r.dh0[:c.n].cpu()[rows], o.h0.grad[rows])
        print(f"  dh0[{name}] rel_l2 {err:.3g}")
        assert err < GRAD_TOL, (name, err)


def _check_padding(c, r):
    """e. rows [n, cap) of the output, of every saved agg / r / z2 and of dh0
    are exact zeros."""
    for name, t in [("out", r.out), ("dh0", r.dh0)] + \
            [(f"saved{l // 4}.{l % 4}", s) for l, s in enumerate(r.saved) if l % 4 != 3]:
        if t is not None:
            assert torch.count_nonzero(t[c.n:]) == 0, name


def _full_case(pkg, dev, c):
    r = _step_twice(pkg, dev, c, c.h0, c.w)
    o = _oracle(c, c.h0, c.w, r.masks)
    _check_oracle(c, r, o)
    _check_saved(c, r)
    if not c.fold:
        _check_blocks(c, r, o)
    return r, o


def _mode(training):
    return "train" if training else "eval"


# ---------------------------------------------------------------------------
# exact-mode rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False], ids=_mode)
@pytest.mark.parametrize("n", E.EXACT_ROWS)
def test_exact_rows(pkg, dev, n, training):
    _full_case(pkg, dev, _case(pkg, dev, n, training))


def test_two_full_supergroups(pkg, dev):
    _full_case(pkg, dev, _case(pkg, dev, E.FULL_SUPER_ROWS, True))


@pytest.mark.parametrize("n,free", E.FLIP_CASES)
def test_agg_path_flipped(pkg, dev, n, free, monkeypatch):
    # (as test_gin_agg_free_matches_stored_agg switches it)
    monkeypatch.setattr(pkg.ops, "AGG_FREE_MIN_ROWS", 0 if free else 1 << 40)
    c = _case(pkg, dev, n, True, agg_free=free)
    assert c.agg_free != (n >= E.DEFER_MAX)  # not the default path at this size
    _full_case(pkg, dev, c)


@pytest.mark.parametrize("training", [True, False], ids=_mode)
@pytest.mark.parametrize("n", E.FOLD_ROWS)
def test_transfer_fold(pkg, dev, n, training):
    _full_case(pkg, dev, _case(pkg, dev, n, training, fold=True))


# ---------------------------------------------------------------------------
# capacity mode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", E.CAPACITY_CASES)
def test_capacity_rows(pkg, dev, n, cap):
    c = _case(pkg, dev, n, True, cap=cap)
    r, _ = _full_case(pkg, dev, c)
    _check_padding(c, r)
    # another valid count on the device, the same buffers and host sizes: the
    # statistics follow it (and every counter had been left zero)
    n2 = 64 if cap == 192 else 1024  # (the two smallest cases run their own count again)
    c.static.dims[:1].fill_(n2)
    c2 = copy.copy(c)
    c2.n = n2
    r2 = _device_step(pkg, dev, c2, c.h0, c.w, backward=False)
    _check_saved(c2, r2)
    assert torch.count_nonzero(r2.out[n2:]) == 0
    assert torch.equal(r2.saved[3], r.saved[3]) == (n2 == n)  # layer 0's record


# ---------------------------------------------------------------------------
# boundary-weighted passes
# ---------------------------------------------------------------------------
def _wid(v):
    return "exact" if v is None else str(v)


def _upstream_pass(pkg, dev, n, cap, training, agg_free=None):
    c = _case(pkg, dev, n, training, cap=cap, agg_free=agg_free)
    w = E.upstream_mask(c.w, n)
    r = _step_twice(pkg, dev, c, c.h0, w)
    o = _oracle(c, c.h0, w, r.masks)
    _check_oracle(c, r, o)
    _check_blocks(c, r, o)
    if not training:  # (a train-mode BatchNorm couples every row)
        lo = E.first_coupled_row(c.gh, n)
        assert 0 < lo <= n - min(n, E.UPSTREAM_ROWS)
        assert torch.count_nonzero(r.dh0[:lo]) == 0
        assert torch.count_nonzero(o.h0.grad[:lo]) == 0
    if cap is not None:
        _check_padding(c, r)


@pytest.mark.parametrize("training", [False, True], ids=_mode)
@pytest.mark.parametrize("n,cap", E.WEIGHTED_CASES, ids=_wid)
def test_upstream_on_last_rows(pkg, dev, n, cap, training):
    """Upstream gradient on the last min(n, 33) rows only: what the boundary
    rows contribute is then all there is in every sum.  On the default path of
    the size: the stored-agg backward (gin_bwd5_k's own row mask) below 65536
    rows."""
    _upstream_pass(pkg, dev, n, cap, training)


@pytest.mark.parametrize("training", [False, True], ids=_mode)
@pytest.mark.parametrize("n,cap", [wc for wc in E.WEIGHTED_CASES if wc[0] < E.DEFER_MAX], ids=_wid)
def test_upstream_on_last_rows_agg_free(pkg, dev, n, cap, training, monkeypatch):
    """The same pass with the agg-free backward forced on at the sizes that do
    not take it by default: gin_bwd5z_k masks its rows through stage_dz2, not
    through gin_bwd5_k's own copy of the mask."""
    monkeypatch.setattr(pkg.ops, "AGG_FREE_MIN_ROWS", 0)
    _upstream_pass(pkg, dev, n, cap, training, agg_free=True)


@pytest.mark.parametrize("n,cap", E.WEIGHTED_CASES, ids=_wid)
def test_outlier_rows_in_last_tile(pkg, dev, n, cap):
    """h0 scaled on the rows of the last tile until they hold at least 5 % of
    layer 0's centred sum of squares: a statistics tree that drops or double
    counts them misses the record by far more than 1e-5."""
    c = _case(pkg, dev, n, True, cap=cap)
    h0 = E.with_outliers(c.h0, n)
    # the condition, on the oracle alone
    p, _ = E.oracle_params(c.gin)
    src, dst = c.gh.edges()
    share = E.outlier_share(E.layer0_z2(p, src, dst, h0[:n]), n)
    assert share >= E.OUTLIER_SHARE, share
    r = _step_twice(pkg, dev, c, h0, c.w, backward=False)
    o = _oracle(c, h0, c.w, r.masks, backward=False)
    _check_saved(c, r)
    _check_oracle(c, r, o, backward=False)
    if cap is not None:
        _check_padding(c, r)
