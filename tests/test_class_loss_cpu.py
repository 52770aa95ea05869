"""CPU side of the class-index cross-entropy (csrc/class_loss.hip): the C-ABI
bookkeeping of the new entry points, what stays pinned (ABI version, the
task-loss kinds), and the paths that never reach the kernel on CPU tensors."""
import pytest
import torch
import torch.nn.functional as F


def test_abi_lists_the_class_loss_entry_points(pkg):
    lib = pkg._lib
    assert lib.ABI_VERSION == 24
    for name in ("scgib_class_loss_ws_doubles", "scgib_class_loss_fwd", "scgib_class_loss_bwd"):
        assert name in lib.SIGNATURES, name
    # scores, labels, label type, rows, classes, ws, counter, loss, count, hits, invalid,
    # epoch, stream / ..., g_loss, count, d_scores, stream
    assert len(lib.SIGNATURES["scgib_class_loss_fwd"][1]) == 13
    assert len(lib.SIGNATURES["scgib_class_loss_bwd"][1]) == 9
    loaded = lib.load()  # every listed name resolves in the built library
    assert int(loaded.scgib_class_loss_ws_doubles()) == 256


def test_task_loss_kinds_are_unchanged(pkg):
    assert pkg.ops.TASK_LOSS_KINDS == {"bce": 0, "bce_logits": 1, "mae": 2, "rmse": 3}
    M = pkg.models.Mainmodel_finetuning
    assert getattr(M.loss_CrossEntropy, "task_loss_kind", None) is None
    assert pkg.models.DEVICE_CE is False


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64])
def test_class_loss_refuses_cpu_tensors(pkg, dtype):
    scores = torch.rand(5, 3)
    labels = torch.tensor([0, 1, 2, 1, 0]).to(dtype)
    with pytest.raises(pkg._lib.ScgibError, match="no CPU fallback"):
        pkg.ops.class_loss(scores, labels)


def test_class_epoch_refuses_the_cpu(pkg):
    with pytest.raises(pkg._lib.ScgibError, match="no CPU fallback"):
        pkg.metrics.ClassEpoch("cpu")


@pytest.mark.parametrize("switch", [False, True])
def test_loss_cross_entropy_on_cpu_is_torch(pkg, switch, monkeypatch):
    """CPU tensors run torch whatever DEVICE_CE says: the bits of
    F.cross_entropy on the scores and the squeezed class column."""
    monkeypatch.setattr(pkg.models, "DEVICE_CE", switch)
    gen = torch.Generator().manual_seed(3)
    scores = torch.sigmoid(4 * torch.randn(33, 2, generator=gen)).requires_grad_(True)
    targets = torch.randint(0, 2, (33, 1), generator=gen)
    ref_in = scores.detach().clone().requires_grad_(True)
    ref = F.cross_entropy(ref_in, targets.squeeze(-1))
    ref.backward()
    got = pkg.models.Mainmodel_finetuning.loss_CrossEntropy(None, scores, targets)
    got.backward()
    assert torch.equal(got, ref) and torch.equal(scores.grad, ref_in.grad)
    with pytest.raises(pkg._lib.ScgibError, match="epoch"):
        pkg.models.Mainmodel_finetuning.loss_CrossEntropy(None, scores, targets, epoch=object())
