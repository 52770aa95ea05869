"""CPU side of the wide task heads / NaN-masked losses: MetricWrapper's four
NaN policies against a restatement of the reference's wrapper
(MetricWrapper.py:45-111) on CPU tensors, where every case takes the torch
path, and the C-ABI bookkeeping of the new entry points."""
import pytest
import torch
import torch.nn.functional as F


def _ref_wrapper(metric, mode, preds, target):
    """MetricWrapper.compute as the reference defines it."""
    if preds.ndim == 1:
        preds = preds.unsqueeze(-1)
    if target.ndim == 1:
        target = target.unsqueeze(-1)
    nans = torch.isnan(target)
    if mode is None:
        return metric(preds, target)
    if isinstance(mode, (int, float)):
        target = target.clone()
        target[nans] = mode
        return metric(preds, target)
    if mode == "ignore-flatten":
        return metric(preds[~nans], target[~nans])
    assert mode == "ignore-mean-label"
    vals = torch.stack([metric(preds[..., i][~nans[..., i]], target[..., i][~nans[..., i]])
                        for i in range(target.shape[-1])])
    return torch.nansum(vals) / torch.sum(~torch.isnan(vals))


def _inputs(shape, p_nan, seed=0):
    gen = torch.Generator().manual_seed(seed)
    preds = torch.rand(shape, generator=gen).clamp(1e-4, 1 - 1e-4)
    target = torch.randint(0, 2, shape, generator=gen).float()
    target[torch.rand(shape, generator=gen) < p_nan] = float("nan")
    return preds, target


@pytest.mark.parametrize("metric", [F.binary_cross_entropy, F.l1_loss], ids=["bce", "l1"])
@pytest.mark.parametrize("mode", [None, 0, 0.5, "ignore-flatten", "ignore-mean-label"],
                         ids=["none", "zero", "half", "flatten", "mean-label"])
@pytest.mark.parametrize("shape", [(33, 12), (41,)], ids=["33x12", "1d"])
def test_metric_wrapper_matches_reference_semantics(pkg, metric, mode, shape):
    preds, target = _inputs(shape, 0.2)
    assert torch.isnan(target).any() and not torch.isnan(target).all()
    w = pkg.metric_wrapper.MetricWrapper(metric=metric, target_nan_mask=mode)
    if mode is None and metric is F.binary_cross_entropy:
        # NaN targets reach torch's BCE unchanged, which refuses them: both raise
        with pytest.raises(RuntimeError):
            _ref_wrapper(metric, mode, preds, target)
        with pytest.raises(RuntimeError):
            w(preds, target)
        target = torch.nan_to_num(target, nan=1.0)
    got = w(preds, target)
    torch.testing.assert_close(got, w.compute(preds, target), rtol=0, atol=0, equal_nan=True)
    ref = _ref_wrapper(metric, mode, preds, target)
    assert got.shape == ref.shape == ()
    torch.testing.assert_close(got, ref, rtol=0, atol=0, equal_nan=True)
    if mode is not None:
        assert torch.isfinite(got)


def test_metric_wrapper_mean_label_drops_failing_and_empty_columns(pkg):
    """A column with no label gives NaN (a mean over nothing), which nan_mean
    leaves out; a column whose metric raises is dropped."""
    preds, target = _inputs((33, 12), 0.2)
    target[:, 3] = float("nan")
    preds[:, 5] = 2.0

    def metric(p, t):
        if bool((p == 2.0).all()):
            raise RuntimeError("column 5")
        return F.l1_loss(p, t)

    w = pkg.metric_wrapper.MetricWrapper(metric, "ignore-mean-label")
    cols = [i for i in range(12) if i not in (3, 5)]
    ref = torch.stack([F.l1_loss(preds[:, i][~torch.isnan(target[:, i])],
                                 target[:, i][~torch.isnan(target[:, i])]) for i in cols]).mean()
    torch.testing.assert_close(w(preds, target), ref, rtol=1e-6, atol=0)


def test_metric_wrapper_surface(pkg):
    W = pkg.metric_wrapper.MetricWrapper
    assert pkg.MetricWrapper is W
    w = W(F.l1_loss, "ignore-flatten", reduction="sum")
    assert w.metric is F.l1_loss and w.target_nan_mask == "ignore-flatten"
    assert w.kwargs == {"reduction": "sum"} and repr(w) == "l1_loss"
    preds, target = _inputs((33, 12), 0.2)
    keep = ~torch.isnan(target)
    assert torch.equal(w(preds, target), F.l1_loss(preds[keep], target[keep], reduction="sum"))
    x = torch.tensor([[1.0, float("nan")], [3.0, 5.0]])
    assert float(w.nan_mean(x)) == 3.0
    assert torch.equal(w.nan_mean(x, dim=0), torch.tensor([2.0, 5.0]))
    with pytest.raises(ValueError):
        W(F.l1_loss, "ignore")(preds, target)


def test_loss_methods_carry_their_kernel_kind(pkg):
    M = pkg.models.Mainmodel_finetuning
    kinds = {name: getattr(getattr(M, name), "task_loss_kind", None)
             for name in ("loss", "BCEWithLogitsLoss", "lossMAE", "loss_RMSE", "loss_CrossEntropy")}
    assert kinds == {"loss": "bce", "BCEWithLogitsLoss": "bce_logits", "lossMAE": "mae",
                     "loss_RMSE": "rmse", "loss_CrossEntropy": None}
    assert set(kinds.values()) - {None} == set(pkg.ops.TASK_LOSS_KINDS)


def test_abi_lists_the_new_entry_points(pkg):
    lib = pkg._lib
    assert lib.ABI_VERSION == 24
    for name in ("scgib_head_wide_fwd", "scgib_head_wide_bwd", "scgib_head_wide_slab_floats",
                 "scgib_task_loss_fwd", "scgib_task_loss_bwd", "scgib_task_loss_ws_doubles"):
        assert name in lib.SIGNATURES, name
    # the wide head takes scgib_head_fwd / _bwd's arguments (+ the slab)
    assert lib.SIGNATURES["scgib_head_wide_fwd"] == lib.SIGNATURES["scgib_head_fwd"]
    assert len(lib.SIGNATURES["scgib_head_wide_bwd"][1]) == len(lib.SIGNATURES["scgib_head_bwd"][1]) + 1
