"""The Set2Set kernels (csrc/set2set.hip) at their staging, width, round and
padding edges on the MI355X (``-m gpu``): every case of
tests/s2s_edge_cases.py against the written-out fp64 reference, judged per
graph, and the properties that need no tolerance — a graph's result does not
depend on its batch, float4 and scalar staging agree, the pair launch is two
single launches, padding rows are zeroed and nothing else is written — bit for
bit.  The library refuses misaligned LSTM weights and the ops pass aligned
copies: no test hands a kernel a misaligned weight pointer."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import s2s_edge_cases as S
from poison import poisoned

pytestmark = pytest.mark.gpu

SENT = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _module(pkg, dev, d, T, state):
    s2s = pkg.models.Set2Set(d, T, 1)
    s2s.lstm.load_state_dict(state)
    s2s = s2s.to(dev)
    assert s2s.lstm.weight_ih_l0.data_ptr() % 16 == 0 and s2s.lstm.weight_hh_l0.data_ptr() % 16 == 0
    return s2s


def _grads(s2s):
    return {k: getattr(s2s.lstm, k).grad.detach().cpu() for k in S.LSTM_KEYS}


def _run(s2s, g, x, w):
    """One forward + backward of models.Set2Set on device tensors: (out, dx,
    LSTM gradients) on the host."""
    s2s.zero_grad(set_to_none=True)
    x = x.detach().requires_grad_(True)
    out = s2s(g, x)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), x.grad.cpu(), _grads(s2s)


def _run_pair(pkg, s2s, g, xa, xb, wa, wb):
    s2s.zero_grad(set_to_none=True)
    xa, xb = (t.detach().requires_grad_(True) for t in (xa, xb))
    oa, ob = pkg.ops.set2set_pair(xa, xb, g, s2s.lstm, s2s.n_iters)
    ((oa * wa).sum() + (ob * wb).sum()).backward()
    torch.cuda.synchronize()
    return (oa.detach().cpu(), ob.detach().cpu()), (xa.grad.cpu(), xb.grad.cpu()), _grads(s2s)


def _check(tag, out, dx, grads, ref, counts, which=0, tols=(S.OUT_TOL, S.DX_TOL, S.LSTM_TOL),
           lstm=True):
    """Print, then assert: output and dx per graph, LSTM gradients per tensor."""
    n = int(np.sum(counts))
    assert torch.isfinite(out).all() and torch.isfinite(dx).all(), tag
    eo = S.out_err(out.numpy(), ref["out"][which])
    ed = S.dx_err(dx[:n].numpy(), ref["dx"][which], counts)
    print(f"{tag}: out {eo:.3g} dx {ed:.3g}", end="")
    el = {}
    if lstm:
        el = S.lstm_errs({k: v.numpy() for k, v in grads.items()}, ref["lstm"])
        print(" lstm " + " ".join(f"{v:.3g}" for v in el.values()), end="")
    print()
    assert eo < tols[0], (tag, "out", eo)
    assert ed < tols[1], (tag, "dx", ed)
    for k, v in el.items():
        assert np.isfinite(grads[k].numpy()).all() and v < tols[2], (tag, k, v)


# ---------------------------------------------------------------------------
# tolerance tests against ref_set2set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", S.ROUNDS)
@pytest.mark.parametrize("d", S.WIDTHS)
def test_edge_batch(pkg, dev, d, T):
    state, feat, w, ref = S.edge_reference(d, T)
    n = S.EDGE_ROWS
    full, _ = S.make_inputs(d, S.EDGE_COUNTS, rows=n + S.PAD_ROWS)
    assert torch.equal(full[:n], feat)
    g = S.stand_in(S.EDGE_COUNTS, dev)
    out, dx, grads = _run(_module(pkg, dev, d, T, state), g, full.to(dev), w.to(dev))
    assert dx.shape == full.shape and torch.count_nonzero(dx[n:]) == 0  # (NaN counts)
    _check(f"d={d} T={T}", out, dx, grads, ref, S.EDGE_COUNTS)


@pytest.mark.parametrize("T", [1, 3])
def test_edge_batch_pair(pkg, dev, T):
    g = S.stand_in(S.EDGE_COUNTS, dev)
    n = S.EDGE_ROWS
    for d in (64, 60):
        state = S.lstm_state(d)
        fa, wa = S.make_inputs(d, S.EDGE_COUNTS, rows=n + S.PAD_ROWS)
        fb, wb = S.make_inputs(d, S.EDGE_COUNTS, seed=S.SEED + 1, rows=n + S.PAD_ROWS)
        ref = S.ref_run(state, [fa[:n], fb[:n]], [wa, wb], S.EDGE_COUNTS, T)
        s2s = _module(pkg, dev, d, T, state)
        xa, xb, wad, wbd = (t.to(dev) for t in (fa, fb, wa, wb))
        outs, dxs, grads = _run_pair(pkg, s2s, g, xa, xb, wad, wbd)
        for i, (x, w) in enumerate(((xa, wad), (xb, wbd))):
            o1, dx1, _ = _run(s2s, g, x, w)
            assert torch.equal(outs[i], o1) and torch.equal(dxs[i], dx1), (d, i)
            assert torch.count_nonzero(dxs[i][n:]) == 0
            _check(f"pair d={d} T={T} input {i}", outs[i], dxs[i], grads, ref, S.EDGE_COUNTS,
                   which=i, lstm=i == 0)


@pytest.mark.parametrize("T", S.ODD_ROUNDS)
@pytest.mark.parametrize("d", S.ODD_WIDTHS)
def test_odd_round_counts(pkg, dev, d, T):
    """R = B T in {1, 3, 5, 9, 15, 25} over the test's T: set2set_wgrad_k's four
    r & 3 accumulators at odd and wrapping round counts."""
    state = S.lstm_state(d)
    s2s = _module(pkg, dev, d, T, state)
    batches = [[c] for c in S.SOLO_COUNTS] + list(S.SMALL_BATCHES.values())
    for counts in batches:
        feat, w = S.make_inputs(d, counts)
        ref = S.ref_run(state, [feat], [w], counts, T)
        out, dx, grads = _run(s2s, S.stand_in(counts, dev), feat.to(dev), w.to(dev))
        _check(f"d={d} counts={counts} R={len(counts) * T}", out, dx, grads, ref, counts)


def test_sharp_logits(pkg, dev):
    """Features scaled by 30: the logits pass expf's overflow, the softmax is
    near one-hot.  Float32 itself drifts there, so the bound is the project's
    or 8 x the float32 CPU reference's own error on these inputs, whichever is
    larger — measured here, per quantity."""
    d, T = 64, 2
    state, feat, w, ref = S.edge_reference(d, T, S.SHARP_SCALE)
    f32 = S.ref_run(state, [feat], [w], S.EDGE_COUNTS, T, torch.float32)
    fo = S.out_err(f32["out"][0], ref["out"][0])
    fd = S.dx_err(f32["dx"][0], ref["dx"][0], S.EDGE_COUNTS)
    fl = max(S.lstm_errs(f32["lstm"], ref["lstm"]).values())
    print(f"float32 CPU reference at scale {S.SHARP_SCALE:g}: out {fo:.3g} dx {fd:.3g} lstm {fl:.3g}")
    tols = (max(S.OUT_TOL, S.SHARP_FACTOR * fo), max(S.DX_TOL, S.SHARP_FACTOR * fd),
            max(S.LSTM_TOL, S.SHARP_FACTOR * fl))
    print("bounds: out %.3g dx %.3g lstm %.3g" % tols)
    g = S.stand_in(S.EDGE_COUNTS, dev)
    out, dx, grads = _run(_module(pkg, dev, d, T, state), g, feat.to(dev), w.to(dev))
    _check("sharp", out, dx, grads, ref, S.EDGE_COUNTS, tols=tols)


# ---------------------------------------------------------------------------
# bitwise tests
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 60, 9])
def test_graph_is_independent_of_its_batch(pkg, dev, d):
    """One workgroup owns a graph: alone in a B = 1 batch, rows cloned, it
    gives the bits it gave inside the edge batch."""
    T = 3
    state, feat, w, _ = S.edge_reference(d, T)
    s2s = _module(pkg, dev, d, T, state)
    x, wd = feat.to(dev), w.to(dev)
    out, dx, _ = _run(s2s, S.stand_in(S.EDGE_COUNTS, dev), x, wd)
    ptr = S.graph_ptr(S.EDGE_COUNTS).tolist()
    for k, c in enumerate(S.EDGE_COUNTS):
        if c == 0:
            continue
        o1, dx1, _ = _run(s2s, S.stand_in([c], dev), x[ptr[k]:ptr[k + 1]].clone(),
                          wd[k:k + 1].clone())
        assert torch.equal(o1[0], out[k]), (d, k, c)
        assert torch.equal(dx1, dx[ptr[k]:ptr[k + 1]]), (d, k, c)


@pytest.mark.parametrize("d", [64, 60, 32])
def test_misaligned_feature_view(pkg, dev, d):
    """A feature view at a one-float storage offset takes scalar staging: the
    bits of an aligned copy (REG at 64, non-REG float4 staging at 60 and 32)."""
    T = 3
    state, feat, w, _ = S.edge_reference(d, T)
    s2s = _module(pkg, dev, d, T, state)
    g = S.stand_in(S.EDGE_COUNTS, dev)
    n = S.EDGE_ROWS
    base = torch.cat([torch.zeros(1), feat.reshape(-1)]).to(dev)
    res = []
    for view in (True, False):
        f = base[1:].view(n, d) if view else base[1:].view(n, d).clone()
        assert (f.data_ptr() % 16 != 0) == view and f.is_contiguous()
        res.append(_run(s2s, g, f, w.to(dev)))
    (oa, ga, pa), (ob, gb, pb) = res
    assert torch.equal(oa, ob) and torch.equal(ga, gb)
    for k in S.LSTM_KEYS:
        assert torch.equal(pa[k], pb[k]), k


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("case", range(len(S.PADDING_CASES)))
def test_padding_rows_zeroed(pkg, dev, case, pair):
    """The padding-zero blocks' grid-stride loop past its first iteration and
    under the 256-block cap, on NaN-filled workspaces: dx is exactly 0 on
    every padding row and the un-padded run's bits on the live rows."""
    counts, rows, d = S.PADDING_CASES[case]
    T, n = 2, int(np.sum(counts))
    assert S.padding_strides(n, rows, d) >= 16
    state = S.lstm_state(d)
    s2s = _module(pkg, dev, d, T, state)
    g = S.stand_in(counts, dev)
    fa, wa = S.make_inputs(d, counts, rows=rows)
    fb, wb = S.make_inputs(d, counts, seed=S.SEED + 1, rows=rows)
    xa, xb, wa, wb = (t.to(dev) for t in (fa, fb, wa, wb))
    torch.cuda.synchronize()

    def run(k):
        if pair:
            return _run_pair(pkg, s2s, g, xa[:k].clone(), xb[:k].clone(), wa, wb)
        o, dx, gr = _run(s2s, g, xa[:k].clone(), wa)
        return (o,), (dx,), gr

    with poisoned(float("nan")):
        outs_p, dxs_p, grads_p = run(rows)
        outs_e, dxs_e, grads_e = run(n)
    for op, oe, dp, de in zip(outs_p, outs_e, dxs_p, dxs_e):
        assert dp.shape == (rows, d) and de.shape == (n, d)
        assert torch.count_nonzero(dp[n:]) == 0  # (an unwritten NaN counts as non-zero)
        assert torch.isfinite(dp).all() and torch.equal(dp[:n], de)
        assert torch.equal(op, oe)
    for k in S.LSTM_KEYS:
        assert torch.equal(grads_p[k], grads_e[k]), k


def test_nothing_written_past_an_exact_buffer(pkg, dev):
    """n_rows == ptr[B] with empty graphs last: the padding blocks have no row
    to zero.  Through the op, the feature buffer past the view is untouched;
    through the C-ABI with a caller's dx, the guard past n_rows is too, and
    the rows are the op's bits."""
    d, T = 64, 2
    lib, ops = pkg._lib, pkg.ops
    state, feat, w, _ = S.edge_reference(d, T)
    n, B, guard = S.EDGE_ROWS, len(S.EDGE_COUNTS), 64
    assert S.EDGE_COUNTS[-2:] == [0, 0]
    s2s = _module(pkg, dev, d, T, state)
    g = S.stand_in(S.EDGE_COUNTS, dev)
    feat_full = torch.cat([feat, torch.full((guard, d), SENT)]).to(dev)
    with poisoned(float("nan")):
        out, dx, _ = _run(s2s, g, feat_full[:n], w.to(dev))
    assert dx.shape == (n, d) and torch.isfinite(dx).all()
    assert bool((feat_full[n:] == SENT).all()) and torch.equal(feat_full[:n].cpu(), feat)
    # the raw entry points on sentinel-filled buffers
    p = [getattr(s2s.lstm, k).detach() for k in S.LSTM_KEYS]  # w_ih, w_hh, b_ih, b_hh
    x, wd = feat_full[:n].contiguous(), w.to(dev)
    fill = lambda *shape: torch.full(shape, SENT, device=dev)  # noqa: E731
    n_save = int(lib.query("scgib_set2set_save_floats", B, d, T))
    save, out_raw = fill(n_save + guard), fill(B * 2 * d + guard)
    lib.call("scgib_set2set_fwd", ops._p(x), ops._p(g.graph_ptr), B, d, T, ops._p(p[0]),
             ops._p(p[2]), ops._p(p[1]), ops._p(p[3]), ops._p(save), ops._p(out_raw),
             ops._stream())
    dx_raw, dgates = fill((n + guard) * d), fill(B * T * 4 * d + guard)
    dws = [fill(4 * d * 2 * d + guard), fill(4 * d * d + guard), fill(4 * d + guard),
           fill(4 * d + guard)]
    lib.call("scgib_set2set_bwd", ops._p(x), ops._p(g.graph_ptr), B, d, T, ops._p(p[0]),
             ops._p(p[1]), ops._p(save), ops._p(wd), ops._p(dx_raw), n, ops._p(dgates),
             *(ops._p(t) for t in dws), ops._stream())
    torch.cuda.synchronize()
    for t, used in ((save, n_save), (out_raw, B * 2 * d), (dx_raw, n * d),
                    (dgates, B * T * 4 * d), (dws[0], 8 * d * d), (dws[1], 4 * d * d),
                    (dws[2], 4 * d), (dws[3], 4 * d)):
        assert bool((t[used:] == SENT).all())
    assert torch.equal(out_raw[:B * 2 * d].view(B, 2 * d).cpu(), out)
    assert torch.equal(dx_raw[:n * d].view(n, d).cpu(), dx)


# ---------------------------------------------------------------------------
# weight alignment
# ---------------------------------------------------------------------------
def _offset_view(t):
    """A contiguous view of t's values at a one-float storage offset."""
    buf = torch.cat([t.new_zeros(1), t.detach().reshape(-1)])
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return buf, v


@pytest.mark.parametrize("d,which", [(64, "w_ih"), (64, "w_hh"), (60, "w_ih"), (60, "w_hh"),
                                     (62, "w_ih"), (9, None)])
def test_library_refuses_misaligned_weights(pkg, dev, d, which):
    """Every entry point that takes the LSTM weights returns SCGIB_EINVAL
    before any launch for a weight it would read as float4 from a base that
    is not 16-byte aligned: sentinel-filled outputs stay untouched.  (d = 62:
    w_ih rows of 124 floats are float4, w_hh rows of 62 are not; which = None:
    the aligned call is accepted — the refusal is not a blanket one.)"""
    lib, ops = pkg._lib, pkg.ops
    T, counts = 2, [5, 0, 70]
    B, n = len(counts), sum(counts)
    state = {k: v.to(dev) for k, v in S.lstm_state(d).items()}
    w_ih, w_hh = state["weight_ih_l0"], state["weight_hh_l0"]
    keep = None
    if which == "w_ih":
        keep, w_ih = _offset_view(w_ih)
    elif which == "w_hh":
        keep, w_hh = _offset_view(w_hh)
    b_ih, b_hh = state["bias_ih_l0"], state["bias_hh_l0"]
    ptr = S.graph_ptr(counts).to(dev)
    feat, w = S.make_inputs(d, counts)
    xa, xb, ga, gb = feat.to(dev), (feat + 1).to(dev), w.to(dev), (2 * w).to(dev)
    fill = lambda k: torch.full((k,), SENT, device=dev)  # noqa: E731
    n_save = int(lib.query("scgib_set2set_save_floats", 2 * B, d, T))
    bufs = {"save": fill(n_save), "out": fill(2 * B * 2 * d), "dxa": fill(n * d),
            "dxb": fill(n * d), "dgates": fill(2 * B * T * 4 * d), "dw_ih": fill(8 * d * d),
            "dw_hh": fill(4 * d * d), "db_ih": fill(4 * d), "db_hh": fill(4 * d)}
    P, st = ops._p, ops._stream()
    dws = [P(bufs[k]) for k in ("dw_ih", "dw_hh", "db_ih", "db_hh")]
    calls = [
        ("scgib_set2set_fwd", (P(xa), P(ptr), B, d, T, P(w_ih), P(b_ih), P(w_hh), P(b_hh),
                               P(bufs["save"]), P(bufs["out"]), st)),
        ("scgib_set2set_fwd2", (P(xa), P(xb), P(ptr), B, d, T, P(w_ih), P(b_ih), P(w_hh),
                                P(b_hh), P(bufs["save"]), P(bufs["out"]), st)),
        ("scgib_set2set_bwd", (P(xa), P(ptr), B, d, T, P(w_ih), P(w_hh), P(bufs["save"]), P(ga),
                               P(bufs["dxa"]), n, P(bufs["dgates"]), *dws, st)),
        ("scgib_set2set_bwd2", (P(xa), P(xb), P(ptr), B, d, T, P(w_ih), P(w_hh),
                                P(bufs["save"]), P(ga), P(gb), P(bufs["dxa"]), P(bufs["dxb"]), n,
                                P(bufs["dgates"]), *dws, st)),
    ]
    if which is None:
        for name, args in calls[1::2]:  # fwd2 writes the save that bwd2 reads
            lib.call(name, *args)
        torch.cuda.synchronize()
        for k, t in bufs.items():  # (save holds the empty graph's max, -inf)
            assert not bool((t == SENT).any()) and (k == "save" or torch.isfinite(t).all()), k
        return
    for name, args in calls:
        with pytest.raises(lib.ScgibError, match=name):
            lib.call(name, *args)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t == SENT).all()), k
    del keep


@pytest.mark.parametrize("d", [60, 64])
def test_offset_weight_views_give_the_aligned_bits(pkg, dev, d):
    """models.Set2Set whose LSTM weights are views at a one-float storage
    offset: ops.set2set / set2set_pair pass aligned copies, and everything is
    bitwise the aligned module's."""
    T = 3
    state, feat, w, _ = S.edge_reference(d, T)
    g = S.stand_in(S.EDGE_COUNTS, dev)
    x, wd = feat.to(dev), w.to(dev)
    wd2 = 2 * wd
    s2s = _module(pkg, dev, d, T, state)
    want = _run(s2s, g, x, wd)
    want_pair = _run_pair(pkg, s2s, g, x, x + 1, wd, wd2)
    # the same module with its lstm replaced by offset views of leaf buffers
    leaves, views = {}, {}
    for k in S.LSTM_KEYS:
        t = getattr(s2s.lstm, k).detach()
        if k.startswith("weight"):
            buf, _ = _offset_view(t)
            leaves[k] = buf.requires_grad_(True)
            views[k] = leaves[k][1:].view(t.shape)
            assert views[k].data_ptr() % 16 != 0
        else:
            leaves[k] = views[k] = t.clone().requires_grad_(True)
    off = pkg.models.Set2Set(d, T, 1)
    del off.lstm
    off.lstm = SimpleNamespace(**views)

    def grads():
        out = {k: (leaves[k].grad[1:].view(views[k].shape) if k.startswith("weight")
                   else leaves[k].grad).detach().cpu().clone() for k in S.LSTM_KEYS}
        for v in leaves.values():
            v.grad = None
        return out

    xg = x.detach().requires_grad_(True)
    out = off(g, xg)
    (out * wd).sum().backward()
    torch.cuda.synchronize()
    got = grads()
    assert torch.equal(out.detach().cpu(), want[0]) and torch.equal(xg.grad.cpu(), want[1])
    for k in S.LSTM_KEYS:
        assert torch.equal(got[k], want[2][k]), k
    xa, xb = x.detach().requires_grad_(True), (x + 1).detach().requires_grad_(True)
    oa, ob = pkg.ops.set2set_pair(xa, xb, g, off.lstm, T)
    ((oa * wd).sum() + (ob * wd2).sum()).backward()
    torch.cuda.synchronize()
    got = grads()
    assert torch.equal(oa.detach().cpu(), want_pair[0][0])
    assert torch.equal(ob.detach().cpu(), want_pair[0][1])
    assert torch.equal(xa.grad.cpu(), want_pair[1][0]) and torch.equal(xb.grad.cpu(), want_pair[1][1])
    for k in S.LSTM_KEYS:
        assert torch.equal(got[k], want_pair[2][k]), k
