"""Device evaluation metrics, the parts that need no GPU: the exact rank
oracle (tests/rank_oracle.py) against the reference's recorded ROC-AUC / AP
(tests/golden/metrics.npz) and against the host functions, and the new names
through the layers (header, ctypes table, ops, metrics, package)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rank_oracle as RO
from conftest import GOLDEN, ROOT

CASES = ["hiv_like", "pcba_like", "separable"]
ENTRY_POINTS = ("scgib_eval_tiles", "scgib_eval_append", "scgib_eval_keys", "scgib_eval_scan")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "metrics.npz"))


def f32_round_trip(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("case", CASES)
def test_fp32_cast_keeps_order_and_ties(gold, case):
    """What lets fp32 device scores be held to numbers recorded from fp64
    predictions: per column, the cast neither merges nor reorders scores."""
    p = gold[f"{case}__y_pred"]
    p = p[:, None] if p.ndim == 1 else p
    q = f32_round_trip(p)
    for c in range(p.shape[1]):
        order = np.argsort(p[:, c], kind="stable")
        d64, d32 = np.diff(p[order, c]), np.diff(q[order, c])
        assert (d32 >= 0).all(), (case, c)
        assert ((d64 > 0) == (d32 > 0)).all(), (case, c)


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_recorded_rank_metrics(gold, case):
    y, p = gold[f"{case}__y_true"], f32_round_trip(gold[f"{case}__y_pred"])
    assert abs(RO.rocauc(y, p) - float(gold[f"{case}__rocauc"])) <= 1e-12
    assert abs(RO.ap(y, p) - float(gold[f"{case}__ap"])) <= 1e-12


def tie_heavy(seed, n, c, levels, nan_share):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((n, c)).astype(np.float32)
    if levels:
        s = np.floor(rng.random((n, c)) * levels).astype(np.float32) / np.float32(levels)
    y = (rng.random((n, c)) < 0.3).astype(np.float64)
    y[rng.random((n, c)) < nan_share] = np.nan
    return y, s.astype(np.float64)


@pytest.mark.parametrize("n,c,levels,nan_share", [(257, 3, 5, 0.3), (1025, 2, 2, 0.25),
                                                  (4097, 1, 0, 0.2), (64, 4, 3, 0.0)])
def test_oracle_equals_host_functions(pkg, n, c, levels, nan_share):
    pytest.importorskip("sklearn")
    y, s = tie_heavy(n + c, n, c, levels, nan_share)
    assert abs(RO.rocauc(y, s) - pkg.metrics.eval_rocauc(y, s)["rocauc"]) <= 1e-12
    assert abs(RO.ap(y, s) - pkg.metrics.eval_ap(y, s)) <= 1e-12


def test_oracle_tie_group_and_exclusion_rules():
    # every score tied: the chance diagonal, AP = prevalence
    auc, ap, P, N = RO.rank_task([1, 0, 0, 1, np.nan], [2.0, 2.0, 2.0, 2.0, 9.0])
    assert (auc, ap, P, N) == (0.5, 0.5, 2, 2)
    # -0.0 and +0.0 are one group; the only positive ranked last
    assert RO.rank_task([1, 0], [-0.0, 0.0])[:2] == (0.5, 0.5)
    assert RO.rank_task([0, 0, 1], [3.0, 2.0, 1.0])[:2] == (0.0, 1.0 / 3.0)
    assert RO.rank_task([1, 1, np.nan], [1.0, 2.0, 3.0]) == (None, None, 2, 0)
    assert RO.rocauc(np.full((4, 2), np.nan), np.zeros((4, 2))) is None
    t = RO.per_task(np.array([[1.0, np.nan], [0.0, np.nan]]), np.array([[1.0, 0.0], [0.5, 0.0]]))
    assert t["rmse"][0] == pytest.approx(np.sqrt(0.125)) and np.isnan(t["rmse"][1])
    assert t["acc"][0] == 0.5 and np.isnan(t["acc"][1]) and t["labelled"] == [2, 0]


def test_new_names_exist_and_are_exported(pkg):
    assert pkg.EvalBuffer is pkg.metrics.EvalBuffer
    for name in ("append", "reset", "rows", "per_task", "rocauc", "ap", "rmse", "acc"):
        assert callable(getattr(pkg.metrics.EvalBuffer, name)), name
    assert callable(pkg.ops.eval_append) and callable(pkg.ops.rank_metrics)
    assert (pkg.ops.EVAL_ERR_OVERFLOW, pkg.ops.EVAL_ERR_NAN_SCORE, pkg.ops.EVAL_ERR_LABEL) == (1, 2, 4)
    # the host functions are still there, untouched in name
    for name in ("eval_rocauc", "eval_ap", "eval_rmse", "eval_acc"):
        assert callable(getattr(pkg.metrics, name))


def header_arguments():
    """entry point -> number of parameters, from include/scgib.h."""
    src = open(os.path.join(ROOT, "include", "scgib.h")).read()
    out = {}
    for m in re.finditer(r"^(?:int|int64_t)\s+(scgib_eval_\w+)\(([^)]*)\);", src, re.M | re.S):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip()])
    return out


def test_header_and_ctypes_table_agree(pkg):
    args = header_arguments()
    assert set(args) == set(ENTRY_POINTS)
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)  # loads without a GPU: nothing is launched
    for name in ENTRY_POINTS:
        res, types = pkg._lib.SIGNATURES[name]
        assert len(types) == args[name], name
        assert res is (ctypes.c_int64 if name == "scgib_eval_tiles" else ctypes.c_int), name
        assert hasattr(lib, name), name
    loaded = pkg._lib.load()
    assert [loaded.scgib_eval_tiles(n) for n in (0, 1, 64, 65)] == [0, 1, 1, 2]
    # argument errors are refused before any launch
    assert loaded.scgib_eval_append(None, None, 4, 2, None, None, 8, None, None) == -1
    assert loaded.scgib_eval_keys(None, None, 0, 1, 0, 1, None, None, None, None, None, None) == -1
    assert loaded.scgib_eval_scan(None, 4, 2, 1, 2, None, None, None, None, None) == -1


def test_cpu_tensors_are_refused(pkg):
    err = pkg._lib.ScgibError
    with pytest.raises(err):
        pkg.metrics.EvalBuffer(16, 2, "cpu")
    with pytest.raises(err):
        pkg.metrics.EvalBuffer(16, 2, torch.device("cpu"))
    with pytest.raises(err):
        pkg.ops.rank_metrics(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(err):
        pkg.ops.eval_append(torch.zeros(4, 2), torch.zeros(4, 2), torch.zeros(8, 2),
                            torch.zeros(8, 2), torch.zeros(4, dtype=torch.int32))
