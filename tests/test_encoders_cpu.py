"""CPU-only tests of the encoder option: GCN / GraphSAGE construction, their
state_dict surface, and checkpoint round trips.  Nothing is launched."""
from types import SimpleNamespace

import pytest
import torch


def make_args(**kw):
    base = dict(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32, batch_size=16,
                gin_layers=5, task="graph_classification")
    base.update(kw)
    return SimpleNamespace(**base)


H, D = 64, 32
GCN_KEYS = {
    "conv1.weight": (D, 2 * H), "conv1.bias": (2 * H,),
    "conv2.weight": (2 * H, 2 * H), "conv2.bias": (2 * H,),
    "conv3.weight": (2 * H, H), "conv3.bias": (H,),
}
SAGE_KEYS = {}
for _i, _din in ((1, D), (2, H), (3, H)):
    SAGE_KEYS[f"conv{_i}.fc_self.weight"] = (H, _din)
    SAGE_KEYS[f"conv{_i}.fc_neigh.weight"] = (H, _din)
    SAGE_KEYS[f"conv{_i}.bias"] = (H,)
EXPECTED = {"GCN": GCN_KEYS, "GraphSAGE": SAGE_KEYS}


def encoder_keys(model, which):
    pre = which + "."
    return {k[len(pre):]: tuple(v.shape) for k, v in model.state_dict().items()
            if k.startswith(pre)}


@pytest.mark.parametrize("encoder", ["GCN", "GraphSAGE"])
def test_mainmodel_builds_with_reference_keys(pkg, encoder):
    m = pkg.models.Mainmodel(make_args(), 9, 64, 4, 4, 1, encoder)
    for which in ("Encoder1", "Encoder2"):
        assert encoder_keys(m, which) == EXPECTED[encoder]
    assert type(m.Encoder1).__name__ == encoder and type(m.Encoder2).__name__ == encoder
    # DGL's initialisation: zero biases, weights inside the xavier-uniform bound
    for name, p in m.Encoder1.named_parameters():
        if name.endswith("bias"):
            assert torch.count_nonzero(p) == 0, name
        else:
            gain = 2.0 ** 0.5 if encoder == "GraphSAGE" else 1.0
            bound = gain * (6.0 / (p.shape[0] + p.shape[1])) ** 0.5
            assert 0 < p.abs().max() <= bound, name


def test_importable_names(pkg):
    for name in ("GCN", "GraphSAGE", "GraphConv", "SAGEConv"):
        assert hasattr(pkg.models, name), name
    assert encoder_keys(torch.nn.ModuleDict({"e": pkg.models.GCN(32, 64)}), "e") == GCN_KEYS
    assert encoder_keys(torch.nn.ModuleDict({"e": pkg.models.GraphSAGE(32, 64)}), "e") == SAGE_KEYS


def test_transformer_still_raises(pkg):
    with pytest.raises(NotImplementedError):
        pkg.models.Mainmodel(make_args(), 9, 64, 4, 4, 1, "Transformer")
    inner = pkg.models.Mainmodel(make_args(), 9, 64, 4, 4, 1, "GIN")
    with pytest.raises(NotImplementedError):
        pkg.models.Mainmodel_continue(make_args(), 9, 64, 4, 4, 1, 1, inner, "Transformer")
    # the heads outside this change keep refusing the new encoders
    for cls in (pkg.models.Mainmodel_finetuning, pkg.models.Mainmodel_domainadapt):
        with pytest.raises(NotImplementedError):
            cls(make_args(), 9, 64, 4, 4, 1, 1, inner, "GCN")


def test_gin_key_set_unchanged(pkg):
    m = pkg.models.Mainmodel(make_args(), 9, 64, 4, 4, 1, "GIN")
    keys = set(encoder_keys(m, "Encoder1"))
    want = set()
    for l in range(5):
        want |= {f"ginlayers.{l}.eps"}
        want |= {f"ginlayers.{l}.apply_func.mlp.{j}.{t}" for j in (0, 2) for t in ("weight", "bias")}
        want |= {f"batch_norms.{l}.{t}" for t in ("weight", "bias", "running_mean", "running_var",
                                                   "num_batches_tracked")}
    assert keys == want
    assert isinstance(m.Encoder1, pkg.models.GIN) and m.Encoder1.fused


def assert_same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("encoder", ["GCN", "GraphSAGE"])
def test_checkpoint_round_trip(pkg, tmp_path, encoder):
    M = pkg.models
    torch.manual_seed(3)
    args = make_args()
    m = M.Mainmodel(args, 9, 64, 4, 4, 1, encoder)
    path = tmp_path / "main.pt"
    M.save_checkpoint(m, path, args, in_dim=9)
    cfg = torch.load(path, map_location="cpu", weights_only=True)["config"]
    assert cfg["encoder"] == encoder
    back = M.load_checkpoint(path, args)
    assert type(back) is M.Mainmodel
    assert type(back.Encoder1).__name__ == encoder and type(back.Encoder2).__name__ == encoder
    assert_same_state(m, back)

    wrapped = M.Mainmodel_continue(args, 9, 64, 4, 4, 1, 1, m, encoder)
    path2 = tmp_path / "cont.pt"
    M.save_checkpoint(wrapped, path2, args, in_dim=9)
    back2 = M.load_checkpoint(path2, args)
    assert type(back2) is M.Mainmodel_continue and type(back2.model) is M.Mainmodel
    for mod in (back2, back2.model):
        assert type(mod.Encoder1).__name__ == encoder and type(mod.Encoder2).__name__ == encoder
    assert_same_state(wrapped, back2)


def test_mixed_levels_round_trip(pkg, tmp_path):
    """Each level keeps its own encoder (a GCN wrapper around a GIN model)."""
    M = pkg.models
    args = make_args()
    inner = M.Mainmodel(args, 9, 64, 4, 4, 1, "GIN")
    wrapped = M.Mainmodel_continue(args, 9, 64, 4, 4, 1, 1, inner, "GCN")
    path = tmp_path / "mixed.pt"
    M.save_checkpoint(wrapped, path, args, in_dim=9)
    back = M.load_checkpoint(path, args)
    assert type(back.Encoder1).__name__ == "GCN" and type(back.model.Encoder1).__name__ == "GIN"
    assert_same_state(wrapped, back)


def test_checkpoint_without_encoder_entry_is_gin(pkg, tmp_path):
    M = pkg.models
    args = make_args()
    m = M.Mainmodel(args, 9, 64, 4, 4, 1, "GIN")
    path = tmp_path / "gin.pt"
    M.save_checkpoint(m, path, args, in_dim=9)
    blob = torch.load(path, map_location="cpu", weights_only=True)
    for k in ("encoder", "encoders"):
        assert k in blob["config"]
        del blob["config"][k]
    old = tmp_path / "old.pt"
    torch.save(blob, old)
    back = M.load_checkpoint(old, args)
    assert isinstance(back.Encoder1, M.GIN) and isinstance(back.Encoder2, M.GIN)
    assert_same_state(m, back)


def test_old_fc_self_bias_loads_as_bias(pkg):
    M = pkg.models
    torch.manual_seed(5)
    enc = M.GraphSAGE(32, 64)
    sd = enc.state_dict()
    old = {}
    for k, v in sd.items():
        v = torch.randn_like(v)
        old[k.replace(".bias", ".fc_self.bias") if k.endswith(".bias") else k] = v
    assert "conv2.fc_self.bias" in old and "conv2.bias" not in old
    fresh = M.GraphSAGE(32, 64)
    fresh.load_state_dict(old)  # strict
    for i in (1, 2, 3):
        conv = getattr(fresh, f"conv{i}")
        assert torch.equal(conv.bias, old[f"conv{i}.fc_self.bias"])
        assert torch.equal(conv.fc_self.weight, old[f"conv{i}.fc_self.weight"])
        assert conv.fc_self.bias is None
    # and inside a whole model
    m = M.Mainmodel(make_args(), 9, 64, 4, 4, 1, "GraphSAGE")
    msd = {(k.replace(".bias", ".fc_self.bias") if ("Encoder" in k and k.endswith(".bias")) else k): v
           for k, v in m.state_dict().items()}
    msd["Encoder2.conv1.fc_self.bias"] = torch.full((64,), 0.25)
    m.load_state_dict(msd)
    assert torch.equal(m.Encoder2.conv1.bias, torch.full((64,), 0.25))
