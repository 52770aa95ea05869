"""Device evaluation metrics on the MI355X (``-m gpu``):
metrics.EvalBuffer / ops.rank_metrics against the reference's recorded numbers
and the exact oracle (tests/rank_oracle.py), special values, task groups,
append / overflow / reset, graph capture, determinism and the host functions.

Bounds: AUC is one fp64 division of an exact integer; AP is at most P rounded
terms, at most (P + 2) * 2^-53 < 5e-13 at these sizes: 1e-12 absolute.  RMSE
and accuracy are fp64 sums of at most 4,097 terms: 1e-12 relative."""
import os

import numpy as np
import pytest
import torch

import rank_oracle as RO
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = ["hiv_like", "pcba_like", "separable"]
# tile edges of the key kernel (64 rows) and chunk edges of the scan (1,024 keys)
SWEEP_N = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097]
ABS = 1e-12
REL = 1e-12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "metrics.npz"))


def col2(a):
    a = np.asarray(a)
    return a[:, None] if a.ndim == 1 else a


def filled(pkg, dev, y, s, **kw):
    """An EvalBuffer holding labels y and fp32 scores s (numpy [n, C])."""
    y, s = col2(y), col2(s)
    buf = pkg.metrics.EvalBuffer(len(y), y.shape[1], dev, **kw)
    buf.append(torch.from_numpy(np.ascontiguousarray(s, np.float32)).to(dev),
               torch.from_numpy(np.ascontiguousarray(y, np.float32)).to(dev))
    return buf


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


def check_against_oracle(pkg, buf, y, s):
    """per_task() and the scalar means of `buf` against the oracle on (y, s)."""
    ref = RO.per_task(y, np.asarray(s, np.float32).astype(np.float64))
    got = {k: v.cpu().numpy() for k, v in buf.per_task().items()}
    assert got["pos"].tolist() == ref["pos"] and got["neg"].tolist() == ref["neg"]
    assert got["labelled"].tolist() == ref["labelled"]
    for name in ("auc", "ap"):
        for c, want in enumerate(ref[name]):
            if want is None:
                assert np.isnan(got[name][c]), (name, c)
            else:
                assert abs(got[name][c] - want) <= ABS, (name, c, got[name][c], want)
    for name in ("rmse", "acc"):
        for c, want in enumerate(ref[name]):
            if np.isnan(want):
                assert np.isnan(got[name][c]), (name, c)
            elif np.isinf(want):  # an infinite score: the RMSE is infinite on both sides
                assert got[name][c] == want, (name, c)
            else:
                assert abs(got[name][c] - want) <= REL * abs(want), (name, c, got[name][c], want)
    want_auc, want_ap = RO._mean(ref["auc"]), RO._mean(ref["ap"])
    if want_auc is None:
        with pytest.raises(RuntimeError, match="No positively labeled"):
            buf.rocauc()
        with pytest.raises(RuntimeError, match="No positively labeled"):
            buf.ap()
    else:
        assert abs(buf.rocauc()["rocauc"] - want_auc) <= ABS
        assert abs(buf.ap() - want_ap) <= ABS


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_golden_cases(pkg, dev, gold, case):
    y = col2(gold[f"{case}__y_true"])
    p32 = col2(gold[f"{case}__y_pred"]).astype(np.float32)
    buf = filled(pkg, dev, y, p32)
    assert abs(buf.rocauc()["rocauc"] - float(gold[f"{case}__rocauc"])) <= ABS
    assert abs(buf.ap() - float(gold[f"{case}__ap"])) <= ABS
    ref = RO.per_task(y, p32.astype(np.float64))
    want = sum(ref["rmse"]) / len(ref["rmse"])
    assert abs(buf.rmse()["rmse"] - want) <= REL * abs(want)
    a32 = col2(gold[f"{case}__acc_pred"]).astype(np.float32)
    ref = RO.per_task(y, a32.astype(np.float64))
    want = sum(ref["acc"]) / len(ref["acc"])
    assert abs(filled(pkg, dev, y, a32).acc()["acc"] - want) <= REL * abs(want)


def sweep_case(seed, n, c, levels, nan_share):
    rng = np.random.default_rng(seed)
    if levels:
        s = (np.floor(rng.random((n, c)) * levels) / levels).astype(np.float32)
    else:
        s = rng.standard_normal((n, c)).astype(np.float32)
    y = (rng.random((n, c)) < 0.4).astype(np.float64)
    y[rng.random((n, c)) < nan_share] = np.nan
    if c >= 3:
        y[:, 0] = np.nan                                  # no labelled row
        y[:, 1] = np.where(np.isnan(y[:, 1]), np.nan, 0)  # a single class
        y[:, 2] = np.where(np.isnan(y[:, 2]), np.nan, 0)  # the only positive ranked last
        r = int(rng.integers(n))
        y[r, 2] = 1
        s[r, 2] = s[:, 2].min() - 1
    return y, s


@pytest.mark.parametrize("n", SWEEP_N)
def test_sweep_against_oracle(pkg, dev, n):
    seed = 0
    for c in (1, 3, 17):
        for levels in (1, 2, 5, 0):
            for nan_share in (0.0, 0.3):
                seed += 1
                y, s = sweep_case(1000 * n + seed, n, c, levels, nan_share)
                check_against_oracle(pkg, filled(pkg, dev, y, s), y, s)


# ---------------------------------------------------------------------------
def test_signed_zeros_tie_and_infinities_order(pkg, dev):
    y = np.array([[1.0], [0.0], [0.0], [1.0]])
    s = np.array([[-0.0], [0.0], [-0.0], [0.0]], np.float32)
    buf = filled(pkg, dev, y, s)
    assert buf.rocauc()["rocauc"] == 0.5 and buf.ap() == 0.5  # one tie group
    check_against_oracle(pkg, buf, y, s)
    y = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0])[:, None]
    s = np.array([np.inf, -np.inf, 1.0, -1.0, np.inf, -np.inf, 3e38], np.float32)[:, None]
    check_against_oracle(pkg, filled(pkg, dev, y, s), y, s)
    # +inf first, -inf last: a perfect and a fully inverted ranking
    assert filled(pkg, dev, [1.0, 0.0, 0.0], [np.inf, 3e38, -np.inf]).rocauc()["rocauc"] == 1.0
    assert filled(pkg, dev, [0.0, 0.0, 1.0], [np.inf, -3e38, -np.inf]).rocauc()["rocauc"] == 0.0


def test_bad_inputs_are_reported(pkg, dev):
    err = pkg._lib.ScgibError
    y = np.array([[1.0], [0.0], [1.0]])
    for method in ("rocauc", "ap", "rmse", "acc"):
        with pytest.raises(err, match="NaN score"):
            getattr(filled(pkg, dev, y, [[0.5], [np.nan], [0.1]]), method)()
    for method in ("rocauc", "ap"):
        with pytest.raises(err, match="neither 0, 1 nor NaN"):
            getattr(filled(pkg, dev, [[1.0], [0.5], [0.0]], [[0.5], [0.2], [0.1]]), method)()
    # the error word is sticky until reset()
    buf = filled(pkg, dev, y, [[0.5], [np.nan], [0.1]])
    with pytest.raises(err):
        buf.rocauc()
    buf.reset()
    buf.append(torch.tensor([[0.9], [0.1]], device=dev), torch.tensor([[1.0], [0.0]], device=dev))
    assert buf.rocauc()["rocauc"] == 1.0


def test_nan_score_under_nan_label_is_ignored(pkg, dev):
    y = np.array([[1.0, 0.0], [np.nan, 1.0], [0.0, 0.0], [1.0, np.nan]])
    s = np.array([[0.3, 0.1], [np.nan, 0.7], [0.4, 0.2], [0.9, np.nan]], np.float32)
    buf = filled(pkg, dev, y, s)
    keep = np.array([[0.3, 0.1], [5.0, 0.7], [0.4, 0.2], [0.9, 5.0]], np.float32)
    check_against_oracle(pkg, buf, y, keep)
    assert not np.isnan(buf.rmse()["rmse"])


def test_no_task_with_both_classes(pkg, dev):
    y = np.array([[1.0, 0.0, np.nan], [1.0, 0.0, np.nan]])
    buf = filled(pkg, dev, y, np.zeros((2, 3), np.float32))
    with pytest.raises(RuntimeError, match="Cannot compute ROC-AUC") as e:
        buf.rocauc()
    assert not isinstance(e.value, pkg._lib.ScgibError)
    with pytest.raises(RuntimeError, match="Cannot compute Average Precision"):
        buf.ap()
    assert np.isnan(buf.rmse()["rmse"])  # the all-NaN column's RMSE is NaN
    with pytest.raises(ZeroDivisionError):
        buf.acc()
    t = buf.per_task()
    assert np.isnan(t["rmse"][2].item()) and t["rmse"][0].item() == 1.0
    assert t["acc"][1].item() == 1.0 and t["labelled"].tolist() == [2, 2, 0]


# ---------------------------------------------------------------------------
def test_task_groups_are_bitwise_invisible(pkg, dev):
    n, c = 257, 17
    y, s = sweep_case(7, n, c, 5, 0.3)
    st, yt = torch.from_numpy(s).to(dev), torch.from_numpy(y).float().to(dev)
    one, marks = pkg.ops.rank_metrics(st, yt), []
    per_row = pkg.ops.EVAL_ELEMENT_BYTES * n
    grouped = pkg.ops.rank_metrics(st, yt, workspace_bytes=4 * per_row + per_row - 1, marks=marks)
    assert [m[0] for m in marks].count("keys") == 5  # four groups of 4 and a remainder of 1
    assert same_bits(one, grouped)
    single = pkg.ops.rank_metrics(st, yt, workspace_bytes=1)  # one task at a time
    assert same_bits(one, single)
    buf = filled(pkg, dev, y, s, workspace_bytes=4 * per_row)
    assert same_bits({k: v for k, v in buf.per_task().items() if k != "err"},
                     {k: v for k, v in one.items() if k != "err"})


def arena(buf, dev, canary=-7.0, tail=64):
    """Re-seat the buffer's storage inside larger tensors filled with a canary."""
    cap, c = buf.capacity, buf.num_tasks
    big = [torch.full(((cap + tail) * c,), canary, device=dev) for _ in range(2)]
    buf.scores, buf.labels = (b[:cap * c].view(cap, c) for b in big)
    return big


def test_append_concatenates(pkg, dev):
    c = 3
    g = torch.Generator().manual_seed(3)
    parts = [(torch.randn(b, c, generator=g), (torch.rand(b, c, generator=g) < 0.5).float())
             for b in (1, 7, 64)]
    buf = pkg.metrics.EvalBuffer(80, c, dev)
    big = arena(buf, dev)
    for s, y in parts:
        buf.append(s.to(dev), y.to(dev))
    assert buf.rows() == 72
    assert torch.equal(buf.scores[:72].cpu(), torch.cat([p[0] for p in parts]))
    assert torch.equal(buf.labels[:72].cpu(), torch.cat([p[1] for p in parts]))
    assert all((b[72 * c:] == -7.0).all() for b in big)
    # other dtypes are converted like every op's inputs
    buf.append(torch.ones(2, c, dtype=torch.float64, device=dev),
               torch.ones(2, c, dtype=torch.int64, device=dev))
    assert buf.rows() == 74 and (buf.labels[72:74] == 1).all()


def test_append_past_capacity(pkg, dev):
    c, cap = 3, 10
    buf = pkg.metrics.EvalBuffer(cap, c, dev)
    big = arena(buf, dev)
    a = torch.arange(7 * c, dtype=torch.float32, device=dev).view(7, c)
    ya = (a % 2 == 0).float()
    buf.append(a, ya)
    assert buf.rows() == 7
    b = 100 + torch.arange(7 * c, dtype=torch.float32, device=dev).view(7, c)
    buf.append(b, 1 - ya)
    assert buf.rows() == cap                     # the cursor stops at the capacity
    assert torch.equal(buf.scores[:7], a) and torch.equal(buf.labels[:7], ya)
    assert torch.equal(buf.scores[7:], b[:3]) and torch.equal(buf.labels[7:], (1 - ya)[:3])
    assert all((t[cap * c:] == -7.0).all() for t in big)   # nothing behind the buffer
    buf.append(b, ya)                            # a full buffer takes nothing
    assert buf.rows() == cap and torch.equal(buf.scores[7:], b[:3])
    assert all((t[cap * c:] == -7.0).all() for t in big)
    for method in ("rocauc", "ap", "rmse", "acc"):
        with pytest.raises(pkg._lib.ScgibError, match="overflow"):
            getattr(buf, method)()
    buf.reset()
    assert buf.rows() == 0 and buf.state.tolist() == [0, 0, 0, 0]
    buf.append(a, ya)
    assert buf.rows() == 7 and 0.0 <= buf.rocauc()["rocauc"] <= 1.0


def test_append_captured(pkg, dev):
    b, c = 33, 5
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(b, c, generator=g).to(dev),
             (torch.rand(b, c, generator=g) < 0.4).float().to(dev)) for _ in range(4)]
    s_in, y_in = torch.zeros(b, c, device=dev), torch.zeros(b, c, device=dev)
    buf = pkg.metrics.EvalBuffer(3 * b, c, dev)
    buf.append(s_in, y_in)  # first launch outside the capture
    buf.reset()
    torch.cuda.synchronize()
    step, clear = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(step):
        buf.append(s_in, y_in)
    with torch.cuda.graph(clear):
        buf.reset()
    assert buf.rows() == 0  # capturing runs nothing
    for s, y in data[:3]:
        s_in.copy_(s)
        y_in.copy_(y)
        step.replay()
    assert buf.rows() == 3 * b
    eager = pkg.metrics.EvalBuffer(3 * b, c, dev)
    eager.append(torch.cat([d[0] for d in data[:3]]), torch.cat([d[1] for d in data[:3]]))
    assert torch.equal(buf.scores, eager.scores) and torch.equal(buf.labels, eager.labels)
    assert same_bits(buf.per_task(), eager.per_task())
    assert buf.rocauc() == eager.rocauc() and buf.ap() == eager.ap()
    clear.replay()
    s_in.copy_(data[3][0])
    y_in.copy_(data[3][1])
    step.replay()
    assert buf.rows() == b  # starts again from row 0
    assert torch.equal(buf.scores[:b], data[3][0]) and torch.equal(buf.labels[:b], data[3][1])
    assert torch.equal(buf.scores[b:], eager.scores[b:])
    step.replay()
    assert buf.rows() == 2 * b and torch.equal(buf.scores[b:2 * b], data[3][0])


def test_two_runs_are_bitwise_equal(pkg, dev):
    y, s = sweep_case(11, 4097, 17, 5, 0.3)
    buf = filled(pkg, dev, y, s)
    assert same_bits(buf.per_task(), buf.per_task())
    again = filled(pkg, dev, y, s)
    assert same_bits(buf.per_task(), again.per_task())


def test_host_functions_agree(pkg, dev):
    pytest.importorskip("sklearn")
    y, s = sweep_case(13, 1025, 17, 5, 0.3)
    buf = filled(pkg, dev, y, s)
    s64 = s.astype(np.float64)
    assert abs(buf.rocauc()["rocauc"] - pkg.metrics.eval_rocauc(y, s64)["rocauc"]) <= ABS
    assert abs(buf.ap() - pkg.metrics.eval_ap(y, s64)) <= ABS
    y, s = sweep_case(14, 257, 1, 0, 0.0)
    buf = filled(pkg, dev, y, s)
    assert abs(buf.rocauc()["rocauc"] - pkg.metrics.eval_rocauc(y, s.astype(np.float64))["rocauc"]) <= ABS
    want = pkg.metrics.eval_rmse(y, s.astype(np.float64))["rmse"]
    assert abs(buf.rmse()["rmse"] - want) <= REL * want
    assert buf.acc() == pkg.metrics.eval_acc(y, s.astype(np.float64))
