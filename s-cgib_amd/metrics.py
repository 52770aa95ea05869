"""Evaluation metrics of the fine-tune configs (metrics.py of the reference).

  eval_rocauc   metrics.py:18-37   (OGB Evaluator semantics: mean per-task
                                    sklearn roc_auc_score over tasks with both
                                    classes present, NaN labels ignored; the
                                    molhiv harness calls ogb's Evaluator,
                                    train_molhiv.py:109,158, whose rule this is)
  eval_ap       metrics.py:40-61   (mean per-task average precision, same task
                                    rule; returns the bare mean as the reference)
  eval_rmse     metrics.py:64-76   (mean per-task RMSE over labelled rows)
  eval_acc      metrics.py:79-87   (mean per-task accuracy over labelled rows)
  rmse          metrics.py:129-137 (sqrt(MSE + 1e-6), train_molsolv.py:180)
  MAE           metrics.py:140-143
  accuracy_TU   metrics.py:146-159 (argmax over classes, count of matches)
Host-side (numpy / sklearn / torch CPU ops), as in the reference; pinned by
tests/golden/metrics.npz (oracle/gen_metrics_golden.py runs the reference's
own functions).  ClassEpoch keeps accuracy_TU's count and the epoch loss of the
TU loops on the device (ops.class_loss).
"""
from __future__ import annotations

import numpy as np
import torch


def _np2(a):
    a = np.asarray(torch.as_tensor(a).detach().cpu(), dtype=np.float64)
    return a[:, None] if a.ndim == 1 else a


def _both_classes(col):
    return np.sum(col == 1) > 0 and np.sum(col == 0) > 0


def eval_rocauc(y_true, y_pred):
    from sklearn.metrics import roc_auc_score
    y_true, y_pred = _np2(y_true), _np2(y_pred)
    scores = []
    for i in range(y_true.shape[1]):
        col = y_true[:, i]
        if _both_classes(col):
            lab = col == col
            scores.append(roc_auc_score(col[lab], y_pred[lab, i]))
    if not scores:
        raise RuntimeError("No positively labeled data available. Cannot compute ROC-AUC.")
    return {"rocauc": sum(scores) / len(scores)}


def eval_ap(y_true, y_pred):
    from sklearn.metrics import average_precision_score
    y_true, y_pred = _np2(y_true), _np2(y_pred)
    aps = []
    for i in range(y_true.shape[1]):
        col = y_true[:, i]
        if _both_classes(col):
            lab = col == col
            aps.append(average_precision_score(col[lab], y_pred[lab, i]))
    if not aps:
        raise RuntimeError(
            "No positively labeled data available. Cannot compute Average Precision.")
    return sum(aps) / len(aps)


def eval_rmse(y_true, y_pred):
    y_true, y_pred = _np2(y_true), _np2(y_pred)
    out = []
    for i in range(y_true.shape[1]):
        lab = y_true[:, i] == y_true[:, i]
        out.append(np.sqrt(((y_true[lab, i] - y_pred[lab, i]) ** 2).mean()))
    return {"rmse": sum(out) / len(out)}


def eval_acc(y_true, y_pred):
    y_true, y_pred = _np2(y_true), _np2(y_pred)
    out = []
    for i in range(y_true.shape[1]):
        lab = y_true[:, i] == y_true[:, i]
        correct = y_true[lab, i] == y_pred[lab, i]
        out.append(float(np.sum(correct)) / len(correct))
    return {"acc": sum(out) / len(out)}


def rmse(scores, targets):
    return torch.sqrt(torch.nn.functional.mse_loss(scores, targets) + 1e-6).detach().item()


def accuracy_TU(scores, targets):
    targets = targets.squeeze(dim=-1)
    pred = scores.argmax(dim=1)
    return (pred.to(float) == targets.to(float)).sum().item()


def MAE(scores, targets):
    return torch.nn.functional.l1_loss(scores, targets).detach().item()


class EvalBuffer:
    """Device-side score buffer and metrics of an evaluation epoch.

    Replaces the loops' ``scores = torch.cat((scores, batch_scores))`` and the
    host evaluator (train_molpcba.py:156-159, :165-207): ``append`` is one HIP
    launch that copies the batch to a device row cursor and advances it — no
    synchronisation, no allocation, so it captures into ``torch.cuda.graph`` /
    the replayed fine-tune step, and every replay appends the batch that is in
    the static inputs at that moment.  The metrics are computed on the device
    (ops.rank_metrics) with the semantics of eval_rocauc / eval_ap / eval_rmse /
    eval_acc; an epoch ends with the single synchronisation of a scalar method.

    ``capacity`` counts stored rows.  Rows whose labels are all NaN are stored
    like any other row and ignored by every metric; capacity mode's padded
    molecules are such rows, so size ``capacity`` in padded rows (steps x
    batch capacity), not in molecules.  Rows that would pass ``capacity`` are
    dropped, the cursor stops there and the next scalar method raises.
    """

    def __init__(self, capacity, num_tasks, device, workspace_bytes=256 << 20):
        from . import _lib
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.ScgibError(f"EvalBuffer: device {device}; the evaluation buffer lives on the "
                                  "HIP device only (no CPU fallback)")
        capacity, num_tasks = int(capacity), int(num_tasks)
        if capacity < 1 or num_tasks < 1 or capacity > 0x7fffffff:
            raise _lib.ScgibError(f"EvalBuffer: capacity {capacity} x {num_tasks} tasks")
        self.capacity, self.num_tasks = capacity, num_tasks
        self.workspace_bytes = int(workspace_bytes)
        self.scores = torch.empty(capacity, num_tasks, dtype=torch.float32, device=device)
        self.labels = torch.empty(capacity, num_tasks, dtype=torch.float32, device=device)
        # cursor, arrival counter of append's launch, error word, spare
        self.state = torch.zeros(4, dtype=torch.int32, device=device)

    def append(self, scores, targets):
        """Store the [B, C] batch (fp32, or anything ops._f32 converts) at the
        cursor; asynchronous and capturable."""
        from . import ops
        ops.eval_append(scores, targets, self.scores, self.labels, self.state)

    def reset(self):
        """Cursor and error word back to zero (a device memset; capturable)."""
        self.state.zero_()

    def rows(self):
        """Rows stored so far.  Synchronises: for use outside the loop."""
        return int(self.state[0].item())

    def per_task(self):
        """Device tensors ``auc, ap, rmse, acc`` (fp64 [C]) and ``pos, neg``
        (int32 [C]) over the stored rows, without synchronising (also
        ``labelled`` and the error word ``err``)."""
        from . import ops
        return ops.rank_metrics(self.scores, self.labels, rows=self.state[0:1],
                                err=self.state[2:3], workspace_bytes=self.workspace_bytes)

    def _read(self, ignore=0):
        """per_task() and its one read: numpy [7, C] (auc, ap, rmse, acc, pos,
        neg, labelled); raises on the error word's bits outside ``ignore``."""
        from . import _lib, ops
        r = self.per_task()
        flat = torch.cat([torch.stack([r["auc"], r["ap"], r["rmse"], r["acc"]]).flatten(),
                          torch.stack([r["pos"], r["neg"], r["labelled"]]).flatten().double(),
                          r["err"].double()]).cpu().numpy()
        bits = int(flat[-1]) & ~ignore
        if bits:
            names = "; ".join(text for bit, text in ops.EVAL_ERR_NAMES if bits & bit)
            raise _lib.ScgibError(f"EvalBuffer: {names} (error word {bits})")
        return flat[:-1].reshape(7, self.num_tasks)

    def _rank_mean(self, row, what):
        t = self._read()
        vals = [float(v) for v, p, n in zip(t[row], t[4], t[5]) if p > 0 and n > 0]
        if not vals:
            raise RuntimeError(f"No positively labeled data available. Cannot compute {what}.")
        return sum(vals) / len(vals)

    def rocauc(self):
        return {"rocauc": self._rank_mean(0, "ROC-AUC")}

    def ap(self):
        return self._rank_mean(1, "Average Precision")

    def rmse(self):
        from . import ops
        t = self._read(ignore=ops.EVAL_ERR_LABEL)
        return {"rmse": sum(float(v) for v in t[2]) / self.num_tasks}

    def acc(self):
        from . import ops
        t = self._read(ignore=ops.EVAL_ERR_LABEL)
        if (t[6] == 0).any():
            raise ZeroDivisionError("float division by zero")
        return {"acc": sum(float(v) for v in t[3]) / self.num_tasks}


class ClassEpoch:
    """Epoch totals of a TU graph-classification loop (train_tudataset.py:
    137-158, :196-221) kept on the device.

    ``ops.class_loss(scores, labels, epoch=self)`` adds each batch in the
    loss's own launch: the batch loss (``epoch_loss += loss.detach().item()``),
    one to the batch count, the accuracy_TU count of the batch and its
    labelled rows (``nb_data += targets.size(0)``).  Nothing synchronises, so
    the step captures and every replay adds the batch that is in the static
    inputs at that moment; ``result`` is the epoch's single read.  Rows
    without a label (NaN / -100: the fill rows of DeviceEvalLoader's last
    batch) count nowhere, so the last batch's mean is the mean over its real
    molecules — the reference's short last batch."""

    def __init__(self, device):
        from . import _lib, ops
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.ScgibError(f"ClassEpoch: device {device}; the accumulator lives on the HIP "
                                  "device only (no CPU fallback)")
        # sum of loss, batches, hits, labelled, invalid
        self.state = torch.zeros(ops.CLASS_EPOCH_DOUBLES, dtype=torch.float64, device=device)

    def reset(self):
        """Totals back to zero (a device memset; capturable)."""
        self.state.zero_()

    def result(self):
        """``{"loss": sum of batch losses / batches, "acc": hits / labelled,
        "hits", "labelled", "batches"}`` — ``epoch_loss /= (iter + 1)`` and
        ``epoch_acc /= nb_data``.  Synchronises (one read).  Raises ScgibError
        when a label was neither masked nor a class index, ZeroDivisionError
        when no row was labelled."""
        from . import _lib
        loss, batches, hits, labelled, invalid = self.state.cpu().tolist()
        if invalid > 0:
            raise _lib.ScgibError(f"ClassEpoch: {int(invalid)} labels that are neither masked nor "
                                  "a class index in [0, C)")
        if labelled == 0:
            raise ZeroDivisionError("float division by zero")
        return {"loss": loss / batches, "acc": hits / labelled, "hits": int(hits),
                "labelled": int(labelled), "batches": int(batches)}
