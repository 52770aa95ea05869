"""The rank metrics of the device evaluation path in exact arithmetic.

Both come from one descending order of a task's labelled scores; elements
with equal scores form one tie group.  With TP, FP the cumulative positives
and negatives at a group's end, TP', FP' the same at the previous group's end
and P, N the task's totals:

    AUC = [ sum_groups (FP - FP') (TP + TP') ] / (2 P N)
    AP  = [ sum_groups (TP - TP') TP / (TP + FP) ] / P

which are sklearn's trapezoid (roc_auc_score) and step (average_precision_score)
sums restated as counts.  Here they are evaluated in Python integers and
``fractions.Fraction`` over a numpy sort and rounded to a double once, so the
values carry no summation error (tests/test_eval_metrics_cpu.py holds them to
the reference's recorded numbers; csrc/eval_metrics.hip is held to them by
tests/test_gpu_eval_metrics.py).  RMSE and accuracy per task are plain fp64.
"""
from fractions import Fraction

import numpy as np


def _col2(a):
    a = np.asarray(a, dtype=np.float64)
    return a[:, None] if a.ndim == 1 else a


def rank_task(y, s):
    """(auc, ap, P, N) of one task: y labels (NaN = unlabelled; only 0 / 1
    count), s scores.  auc / ap are None unless both classes are present."""
    y, s = np.asarray(y, np.float64), np.asarray(s, np.float64)
    keep = (y == 1) | (y == 0)
    y, s = y[keep], s[keep] + 0.0  # -0.0 + 0.0 = +0.0: one tie group
    P, N = int((y == 1).sum()), int((y == 0).sum())
    if P == 0 or N == 0:
        return None, None, P, N
    order = np.argsort(-s, kind="stable")
    y, s = y[order], s[order]
    num, ap = 0, Fraction(0)
    tp = fp = tp0 = fp0 = 0
    for i in range(len(s)):
        if y[i] == 1:
            tp += 1
        else:
            fp += 1
        if i + 1 == len(s) or s[i + 1] != s[i]:
            num += (fp - fp0) * (tp + tp0)
            ap += Fraction((tp - tp0) * tp, tp + fp)
            tp0, fp0 = tp, fp
    return float(Fraction(num, 2 * P * N)), float(ap / P), P, N


def per_task(y_true, y_pred):
    """dict of per-task lists: auc, ap (None where excluded), pos, neg,
    labelled, rmse, acc (NaN without a labelled row)."""
    y_true, y_pred = _col2(y_true), _col2(y_pred)
    out = {k: [] for k in ("auc", "ap", "pos", "neg", "labelled", "rmse", "acc")}
    for c in range(y_true.shape[1]):
        y, s = y_true[:, c], y_pred[:, c]
        auc, ap, P, N = rank_task(y, s)
        lab = y == y
        n = int(lab.sum())
        out["auc"].append(auc)
        out["ap"].append(ap)
        out["pos"].append(P)
        out["neg"].append(N)
        out["labelled"].append(n)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["rmse"].append(float(np.sqrt(((y[lab] - s[lab]) ** 2).mean())) if n else float("nan"))
            out["acc"].append(float(np.sum(y[lab] == s[lab])) / n if n else float("nan"))
    return out


def _mean(vals):
    vals = [v for v in vals if v is not None]
    return sum(vals) / len(vals) if vals else None


def rocauc(y_true, y_pred):
    """Mean AUC over the tasks with both classes (None: no such task)."""
    return _mean(per_task(y_true, y_pred)["auc"])


def ap(y_true, y_pred):
    return _mean(per_task(y_true, y_pred)["ap"])
