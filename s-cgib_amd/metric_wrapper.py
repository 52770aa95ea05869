"""``MetricWrapper`` with the interface of the reference's MetricWrapper.py:
a metric (loss) callable plus a policy for NaN targets, used by the
multi-label fine-tune scripts as
``MetricWrapper(metric=model.loss, target_nan_mask="ignore-flatten")``
(train_molpcba.py:108, train_pep_func.py:131, train_molsider.py:109).

``target_nan_mask``:
  * ``None``               targets are passed on as they are;
  * a number               NaN targets are replaced by it (on a copy);
  * ``"ignore-flatten"``   the metric sees the 1-D vectors of the elements
                           whose target is not NaN;
  * ``"ignore-mean-label"`` the metric is computed per column on that column's
                           non-NaN rows (a column whose metric raises is
                           dropped) and the column values are averaged,
                           NaN values left out (``nan_mean``).

Device path: "ignore-flatten" selects elements with a boolean index, whose
result shape depends on the data — torch synchronises the device with the
host there, so such a step cannot be captured into a graph.  When the
tensors are on the HIP device, ``models.FUSE_HEAD`` is on and the metric is
one of ``Mainmodel_finetuning``'s ``loss`` / ``BCEWithLogitsLoss`` /
``lossMAE`` / ``loss_RMSE`` (recognised by the ``task_loss_kind`` attribute
models.py puts on those functions), the same value comes from
``ops.task_loss``: one launch each way, the mask applied inside the
reduction, no synchronise.  Every other case takes the path described above.
"""
from __future__ import annotations

from typing import Callable, Optional, Union

import torch
from torch import Tensor


class MetricWrapper:
    def __init__(self, metric: Union[str, Callable],
                 target_nan_mask: Optional[Union[str, int]] = None, **kwargs):
        self.metric = metric
        self.target_nan_mask = target_nan_mask
        self.kwargs = kwargs

    def _device_kind(self, preds: Tensor, target: Tensor):
        """The ops.task_loss kind that computes this call, or None."""
        kind = getattr(self.metric, "task_loss_kind", None)
        if kind is None or self.kwargs or self.target_nan_mask != "ignore-flatten":
            return None
        if not (preds.is_cuda and target.is_cuda and preds.shape == target.shape
                and preds.numel() > 0 and preds.is_floating_point()
                and target.is_floating_point()):
            return None
        if kind != "bce" and not (preds.dtype == target.dtype == torch.float32):
            return None  # only model.loss casts to fp32 itself (models.py:522-525)
        from . import models
        return kind if models.FUSE_HEAD else None

    def compute(self, preds: Tensor, target: Tensor) -> Tensor:
        if preds.ndim == 1:
            preds = preds.unsqueeze(-1)
        if target.ndim == 1:
            target = target.unsqueeze(-1)
        mask = self.target_nan_mask
        if isinstance(mask, str) and mask not in ("ignore-flatten", "ignore-mean-label"):
            raise ValueError(f"Invalid option `{mask}`")
        if mask is not None and not isinstance(mask, (int, float, str)):
            raise ValueError(f"Invalid option `{mask}`")

        kind = self._device_kind(preds, target)
        if kind is not None:
            from . import ops
            return ops.task_loss(preds.float(), target.float(), kind)

        if mask is None:
            return self.metric(preds, target, **self.kwargs)
        if isinstance(mask, (int, float)):
            target = torch.where(torch.isnan(target), torch.as_tensor(mask, dtype=target.dtype,
                                                                      device=target.device), target)
            return self.metric(preds, target, **self.kwargs)
        keep = ~torch.isnan(target)
        if mask == "ignore-flatten":
            return self.metric(preds[keep], target[keep], **self.kwargs)
        # "ignore-mean-label"
        values = []
        for col in range(target.shape[-1]):
            rows = keep[..., col]
            try:
                values.append(self.metric(preds[..., col][rows], target[..., col][rows],
                                          **self.kwargs))
            except Exception:  # the column contributes nothing
                pass
        return self.nan_mean(torch.stack(values))

    def __call__(self, preds: Tensor, target: Tensor) -> Tensor:
        return self.compute(preds, target)

    def __repr__(self):
        return f"{self.metric.__name__}"

    def nan_mean(self, input: Tensor, **kwargs) -> Tensor:
        """Mean of the non-NaN entries (over ``dim=`` etc. when given)."""
        return torch.nansum(input, **kwargs) / torch.sum(~torch.isnan(input), **kwargs)
