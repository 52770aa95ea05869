"""CPU-only tests of the last ``encoder=`` value: every model class builds with
"Transformer" (and the wrapper classes with every reference string) under
models.ALL_ENCODER_STRINGS, and refuses as before without it, the
state_dict keys are the reference's, a checkpoint records a Transformer's depth
and head count, and the ops / C-ABI surface of the folded entry exists.
Nothing is launched."""
import inspect

import pytest
import torch

from test_encoders_cpu import assert_same_state, encoder_keys, make_args
from test_transformer_cpu import expected_table

F_IN = 9
ALL = ("GIN", "GCN", "GraphSAGE", "Transformer")


@pytest.fixture(autouse=True)
def all_encoder_strings(pkg, monkeypatch):
    monkeypatch.setattr(pkg.models, "ALL_ENCODER_STRINGS", True)


def build(pkg, cls, encoder, num_layers=4, num_heads=4, inner=None):
    M = pkg.models
    if cls is M.Mainmodel:
        return cls(make_args(), F_IN, 64, num_layers, num_heads, 1, encoder)
    if inner is None:
        inner = M.Mainmodel(make_args(), F_IN, 64, num_layers, num_heads, 1, encoder)
    return cls(make_args(), F_IN, 64, num_layers, num_heads, 1, 1, inner, encoder)


def test_encoder_tuples(pkg):
    assert pkg.models.ALL_ENCODERS == ALL
    assert pkg.models.ENCODERS == ALL[:3]  # the strings taken without the switch


def test_switch_is_off_by_default_and_then_refuses_as_before(pkg, monkeypatch, tmp_path):
    M = pkg.models
    monkeypatch.undo()  # the module's own default
    assert M.ALL_ENCODER_STRINGS is False
    inner = M.Mainmodel(make_args(), F_IN, 64, 4, 4, 1, "GIN")
    with pytest.raises(NotImplementedError, match="ALL_ENCODER_STRINGS"):
        M.Mainmodel(make_args(), F_IN, 64, 4, 4, 1, "Transformer")
    for cls in (M.Mainmodel_finetuning, M.Mainmodel_domainadapt):
        with pytest.raises(NotImplementedError, match="ALL_ENCODER_STRINGS"):
            cls(make_args(), F_IN, 64, 4, 4, 1, 1, inner, "GCN")
    # a file that records its encoders is rebuilt with them either way
    monkeypatch.setattr(M, "ALL_ENCODER_STRINGS", True)
    da = chain(pkg, 2, 8)
    path = tmp_path / "da.pt"
    M.save_checkpoint(da, path, make_args(), in_dim=F_IN)
    monkeypatch.setattr(M, "ALL_ENCODER_STRINGS", False)
    back = M.load_checkpoint(path, make_args())
    assert type(back.Encoder1) is M.Transformer and type(back.model.model.Encoder2) is M.Transformer
    assert_same_state(da, back)


@pytest.mark.parametrize("depth_heads", [(2, 8), (4, 4)])
@pytest.mark.parametrize("cls", ["Mainmodel", "Mainmodel_continue", "Mainmodel_domainadapt",
                                 "Mainmodel_finetuning"])
def test_every_class_builds_a_transformer(pkg, cls, depth_heads):
    L, heads = depth_heads
    m = build(pkg, getattr(pkg.models, cls), "Transformer", L, heads)
    assert (m.encoder_name, m.num_layers, m.num_heads) == ("Transformer", L, heads)
    for enc in (m.Encoder1, m.Encoder2):
        assert type(enc) is pkg.models.Transformer
        assert len(enc.layers) == L + 1  # the reference appends one extra layer
        assert all(layer.num_heads == heads for layer in enc.layers)
        assert enc.embedding_h.in_features == 32 and enc.hidden_dim == 64


@pytest.mark.parametrize("encoder", ["GCN", "GraphSAGE"])
@pytest.mark.parametrize("cls", ["Mainmodel_domainadapt", "Mainmodel_finetuning"])
def test_wrapper_classes_take_the_conv_encoders(pkg, cls, encoder):
    inner = pkg.models.Mainmodel(make_args(), F_IN, 64, 4, 4, 1, "GIN")
    m = build(pkg, getattr(pkg.models, cls), encoder, inner=inner)
    assert m.encoder_name == encoder
    assert type(m.Encoder1).__name__ == encoder and type(m.Encoder2).__name__ == encoder
    assert type(m.model.Encoder1) is pkg.models.GIN  # the wrapped model keeps its own


@pytest.mark.parametrize("cls", ["Mainmodel", "Mainmodel_continue", "Mainmodel_domainadapt",
                                 "Mainmodel_finetuning"])
def test_unknown_encoder_raises_with_all_names(pkg, cls):
    inner = pkg.models.Mainmodel(make_args(), F_IN, 64, 4, 4, 1, "GIN")
    with pytest.raises(NotImplementedError) as err:
        build(pkg, getattr(pkg.models, cls), "GAT", inner=inner)
    for name in ALL:
        assert name in str(err.value), (name, str(err.value))


def test_transformer_model_keys_are_the_gin_models_with_the_key_table(pkg):
    gin = pkg.models.Mainmodel(make_args(), F_IN, 64, 4, 4, 1, "GIN")
    gt = pkg.models.Mainmodel(make_args(), F_IN, 64, 4, 4, 1, "Transformer")
    table = expected_table(4)
    want = {k: tuple(v.shape) for k, v in gin.state_dict().items() if not k.startswith("Encoder")}
    for which in ("Encoder1", "Encoder2"):
        want.update({f"{which}.{k}": shape for k, shape in table.items()})
        assert encoder_keys(gt, which) == table
    assert {k: tuple(v.shape) for k, v in gt.state_dict().items()} == want


def chain(pkg, L, heads):
    M = pkg.models
    torch.manual_seed(11)
    main = build(pkg, M.Mainmodel, "Transformer", L, heads)
    cont = build(pkg, M.Mainmodel_continue, "Transformer", L, heads, inner=main)
    return build(pkg, M.Mainmodel_domainadapt, "Transformer", L, heads, inner=cont)


def levels_of(m):
    out = []
    while m is not None:
        out.append(m)
        m = getattr(m, "model", None)
    return out


def test_three_level_chain_round_trips_with_depth_and_heads(pkg, tmp_path):
    M = pkg.models
    da = chain(pkg, 2, 8)
    path = tmp_path / "da.pt"
    M.save_checkpoint(da, path, make_args(), in_dim=F_IN)
    cfg = torch.load(path, map_location="cpu", weights_only=True)["config"]
    assert cfg["encoders"] == ["Transformer"] * 3
    assert cfg["num_layers"] == [2, 2, 2] and cfg["num_heads"] == [8, 8, 8]
    back = M.load_checkpoint(path, make_args())
    got = levels_of(back)
    assert [type(m) for m in got] == [M.Mainmodel_domainadapt, M.Mainmodel_continue, M.Mainmodel]
    for m in got:
        assert (m.num_layers, m.num_heads) == (2, 8)
        for enc in (m.Encoder1, m.Encoder2):
            assert type(enc) is M.Transformer and len(enc.layers) == 3
            assert all(layer.num_heads == 8 for layer in enc.layers)
    assert_same_state(da, back)  # (load_checkpoint loads with strict=True)
    res = back.load_state_dict(da.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_file_without_depth_and_heads_loads_as_4_4(pkg, tmp_path):
    M = pkg.models
    da = chain(pkg, 4, 4)
    path = tmp_path / "da.pt"
    M.save_checkpoint(da, path, make_args(), in_dim=F_IN)
    blob = torch.load(path, map_location="cpu", weights_only=True)
    for k in ("num_layers", "num_heads"):
        assert k in blob["config"]
        del blob["config"][k]
    old = tmp_path / "old.pt"
    torch.save(blob, old)
    back = M.load_checkpoint(old, make_args())
    for m in levels_of(back):
        assert (m.num_layers, m.num_heads) == (4, 4)
        assert len(m.Encoder1.layers) == 5 and m.Encoder1.layers[0].num_heads == 4
    assert_same_state(da, back)


def test_ops_surface(pkg):
    ops = pkg.ops
    for fn in (ops.dropout_state, ops.seed_dropout):
        lane = inspect.signature(fn).parameters.get("lane")
        assert lane is not None and lane.default == 0, fn.__name__
    assert list(inspect.signature(ops.seed_dropout).parameters) == ["device", "seed", "offset", "lane"]
    assert list(inspect.signature(ops.gt_embed).parameters) == [
        "x", "transfer_weight", "embedding_weight", "node_map", "dims"]
    assert list(inspect.signature(ops.gt_encoder_x).parameters) == [
        "x", "graph", "module", "transfer", "node_map", "readout", "drop_masks", "lane"]
    assert inspect.signature(ops.gt_encoder_x).parameters["lane"].default == 0
    assert pkg.models.GT_FOLD is True or pkg.models.GT_FOLD is False


def test_entry_points(pkg):
    lib = pkg._lib
    for name in ("scgib_gt_embed_fwd", "scgib_gt_embed_bwd", "scgib_gt_embed_slabs",
                 "scgib_gt_embed_slab_width"):
        assert name in lib.SIGNATURES, name
    assert lib.ABI_VERSION == 24 and lib.load().scgib_abi_version() == 24
    # one slab row: dWe [64][32] | dWt [32][F]
    assert [lib.query("scgib_gt_embed_slab_width", f) for f in (1, 11, 16)] == \
        [64 * 32 + 32 * f for f in (1, 11, 16)]
    assert lib.query("scgib_gt_embed_slab_width", 0) == 0
    assert lib.query("scgib_gt_embed_slab_width", 17) == 0
    assert lib.query("scgib_gt_embed_slabs", 0) == 0
    assert lib.query("scgib_gt_embed_slabs", 65) == 2
    assert lib.query("scgib_gt_embed_slabs", 257 * 64 + 5) == 256
    # the entry points refuse F outside 1..16 and null pointers before any launch
    E = pkg._lib.ScgibError
    for f in (0, 17):
        with pytest.raises(E):
            lib.call("scgib_gt_embed_fwd", None, f, 4, None, None, None, 4, None, None, None)
        with pytest.raises(E):
            lib.call("scgib_gt_embed_bwd", None, None, f, 4, None, None, None, 4, None, None, None)
    with pytest.raises(E):
        lib.call("scgib_gt_embed_fwd", None, 11, 4, None, None, None, 4, None, None, None)
    with pytest.raises(E):
        lib.call("scgib_gt_embed_bwd", None, None, 11, 4, None, None, None, 4, None, None, None)


def test_ops_refuse_cpu_tensors(pkg):
    gh = pkg.graph.GraphBatch.from_edges([0, 1], [1, 0], 2, symmetric_hint=False)
    enc = pkg.models.Transformer(32, 64, 1, 4, "cpu")
    td = torch.nn.Linear(F_IN, 32, bias=False)
    x = torch.zeros(2, F_IN)
    with pytest.raises(pkg._lib.ScgibError):
        pkg.ops.gt_embed(x, td.weight, enc.embedding_h.weight)
    with pytest.raises(pkg._lib.ScgibError):
        pkg.ops.gt_encoder_x(x, gh, enc, td)
