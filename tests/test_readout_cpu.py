"""The readout_f / useAtt switches of the four model classes, host side (no
GPU): construction, state_dict keys, the Mainmodel_continue mismatch, the
checkpoint round trip and the contrastive op's width refusal."""
from types import SimpleNamespace

import pytest
import torch


def _args(readout_f="sum", useAtt=1):
    return SimpleNamespace(recons_type="adj", useAtt=useAtt, readout_f=readout_f, d_transfer=32,
                           batch_size=8, gin_layers=4, task="graph_classification",
                           dataset="ogbg-molhiv")


def _build(pkg, kind, args, inner_args=None):
    M = pkg.models
    inner = M.Mainmodel(args if inner_args is None else inner_args, 9, 64, 4, 4, 1, "GIN")
    if kind == "Mainmodel":
        return inner
    return getattr(M, kind)(args, 9, 64, 4, 4, 1, 1, inner, "GIN")


KINDS = ["Mainmodel", "Mainmodel_continue", "Mainmodel_domainadapt", "Mainmodel_finetuning"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("readout_f,useAtt", [("set2set", 1), ("sum", 0), ("set2set", 0)])
def test_models_construct_in_every_mode(pkg, kind, readout_f, useAtt):
    base = _build(pkg, kind, _args())
    model = _build(pkg, kind, _args(readout_f, useAtt))
    assert model.readout == readout_f and model.useAtt == useAtt
    assert list(model.state_dict()) == list(base.state_dict())
    for (ka, va), (kb, vb) in zip(model.state_dict().items(), base.state_dict().items()):
        assert va.shape == vb.shape, ka


@pytest.mark.parametrize("outer,inner", [("sum", "set2set"), ("set2set", "sum")])
def test_continue_refuses_mismatched_readouts(pkg, outer, inner):
    with pytest.raises(ValueError) as e:
        _build(pkg, "Mainmodel_continue", _args(outer), _args(inner))
    assert repr(outer) in str(e.value) and repr(inner) in str(e.value)
    # (the head classes read the interaction map only: no such constraint)
    _build(pkg, "Mainmodel_domainadapt", _args(outer), _args(inner))
    _build(pkg, "Mainmodel_finetuning", _args(outer), _args(inner))


@pytest.mark.parametrize("kind", ["Mainmodel", "Mainmodel_continue", "Mainmodel_domainadapt"])
@pytest.mark.parametrize("readout_f,useAtt", [("set2set", 1), ("sum", 0), ("set2set", 0)])
def test_checkpoint_round_trip_keeps_the_switches(pkg, tmp_path, kind, readout_f, useAtt):
    args = _args(readout_f, useAtt)
    model = _build(pkg, kind, args)
    path = tmp_path / "m.pt"
    pkg.models.save_checkpoint(model, path, args, in_dim=9)
    back = pkg.models.load_checkpoint(path, _args())  # the file's values win over the caller's
    assert type(back) is type(model)
    m = back
    while m is not None:
        assert m.readout == readout_f and m.useAtt == useAtt
        m = getattr(m, "model", None)
    for (ka, va), (kb, vb) in zip(model.state_dict().items(), back.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


@pytest.mark.parametrize("shape2", [(4, 96), (4, 64)])
def test_contrastive_refuses_other_widths(pkg, shape2):
    """Width 96 (and two different widths) are refused before any device work."""
    with pytest.raises(pkg._lib.ScgibError):
        pkg.ops.contrastive(torch.zeros(4, 96), torch.zeros(*shape2))
    assert pkg.ops.CONTRAST_WIDTHS == (64, 128)
