"""The Transformer encoder's modules without a launch: names, layer count,
state_dict keys and shapes (the reference's models.py:807-918), default
initialisation, refusals at construction, and the C-ABI bookkeeping."""
import pytest
import torch

H, F2, IN = 64, 128, 32


def expected_table(num_layers):
    table = {"embedding_h.weight": (H, IN)}
    for i in range(num_layers + 1):  # the reference appends one extra layer
        p = f"layers.{i}."
        for name in ("Q", "K", "V", "q_proj", "k_proj", "v_proj"):
            table[p + f"attention.{name}.weight"] = (H, H)
            table[p + f"attention.{name}.bias"] = (H,)
        table[p + "O.weight"] = (H, H)
        table[p + "O.bias"] = (H,)
        for bn in ("batchnorm1", "batchnorm2"):
            for k in ("weight", "bias", "running_mean", "running_var"):
                table[p + f"{bn}.{k}"] = (H,)
            table[p + f"{bn}.num_batches_tracked"] = ()
        for ln in ("layer_norm1", "layer_norm2"):
            table[p + f"{ln}.weight"] = (H,)
            table[p + f"{ln}.bias"] = (H,)
        table[p + "FFN_layer1.weight"] = (F2, H)
        table[p + "FFN_layer1.bias"] = (F2,)
        table[p + "FFN_layer2.weight"] = (H, F2)
        table[p + "FFN_layer2.bias"] = (H,)
    return table


def test_names_import(pkg):
    for name in ("Transformer", "GraphTransformerLayer", "MultiHeadAttentionLayer"):
        assert isinstance(getattr(pkg.models, name), type), name
        assert getattr(pkg, name) is getattr(pkg.models, name)  # exported by the package


def test_layer_count_and_state_dict_table(pkg):
    enc = pkg.models.Transformer(IN, H, 4, 4, "cpu")
    assert len(enc.layers) == 5
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert got == expected_table(4)
    assert enc.fused is False
    for layer in enc.layers:
        assert isinstance(layer, pkg.models.GraphTransformerLayer)
        assert isinstance(layer.attention, pkg.models.MultiHeadAttentionLayer)
        assert layer.num_heads == 4 and layer.attention.out_dim == H // 4
        for ln in (layer.layer_norm1, layer.layer_norm2):
            assert ln.eps == 1e-5
            assert torch.equal(ln.weight, torch.ones(H)) and torch.equal(ln.bias, torch.zeros(H))


def test_default_initialisation_is_torchs(pkg):
    """nn.Linear's default: weights and biases uniform in +-1/sqrt(fan_in)."""
    torch.manual_seed(3)
    enc = pkg.models.Transformer(IN, H, 1, 8, "cpu")
    lay = enc.layers[0]
    for lin in (lay.attention.Q, lay.attention.K, lay.attention.V, lay.O, lay.FFN_layer1,
                lay.FFN_layer2, enc.embedding_h):
        bound = lin.in_features ** -0.5
        wmax = float(lin.weight.detach().abs().max())
        assert 0.8 * bound < wmax <= bound
        if lin.bias is not None:
            assert 0 < float(lin.bias.detach().abs().max()) <= bound
    assert enc.embedding_h.bias is None


def test_constructors_refuse_indivisible_heads(pkg):
    with pytest.raises(ValueError):
        pkg.models.Transformer(IN, H, 4, 3, "cpu")
    with pytest.raises(ValueError):
        pkg.models.GraphTransformerLayer(H, H, 3)
    with pytest.raises(ValueError):
        pkg.models.MultiHeadAttentionLayer(H, H // 3, 3)


def test_strict_state_dict_round_trip(pkg):
    torch.manual_seed(0)
    a = pkg.models.Transformer(IN, H, 4, 4, "cpu")
    torch.manual_seed(1)
    b = pkg.models.Transformer(IN, H, 4, 4, "cpu")
    assert not torch.equal(a.layers[2].O.weight, b.layers[2].O.weight)
    res = b.load_state_dict(a.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


def test_selection_by_string_is_untouched(pkg):
    assert pkg.models.ENCODERS == ("GIN", "GCN", "GraphSAGE")


def test_entry_points(pkg):
    lib = pkg._lib
    for name in ("scgib_gt_slabs", "scgib_gt_slab_width", "scgib_gt_qkv_fwd", "scgib_gt_attn_fwd",
                 "scgib_gt_attn_bwd", "scgib_gt_out_fwd", "scgib_gt_ffn_fwd", "scgib_gt_ffn_bwd",
                 "scgib_gt_out_bwd", "scgib_gt_qkv_bwd"):
        assert name in lib.SIGNATURES, name
    loaded = lib.load()
    assert loaded.scgib_abi_version() == lib.ABI_VERSION
    # slab widths: dW2 | db2 | dgamma | dbeta; dW1 | db1; dWo | dbo | dgamma | dbeta; 3 x (dW | db)
    want = [H * F2 + 3 * H, F2 * H + F2, H * H + 3 * H, 3 * (H * H + H)]
    assert [lib.query("scgib_gt_slab_width", i) for i in range(4)] == want
    assert lib.query("scgib_gt_slab_width", 4) == 0
    assert lib.query("scgib_gt_slabs", 0) == 0
    assert lib.query("scgib_gt_slabs", 65) == 2
    assert lib.query("scgib_gt_slabs", 64 * 1000) == 256


def test_ops_refuse_cpu_tensors(pkg):
    gh = pkg.graph.GraphBatch.from_edges([0, 1], [1, 0], 2, symmetric_hint=False)
    x = torch.zeros(2, H)
    with pytest.raises(pkg._lib.ScgibError):
        pkg.ops.graph_attention(x, x, x, gh, 4)
    with pytest.raises(pkg._lib.ScgibError):
        pkg.ops.gt_layer(x, gh, pkg.models.GraphTransformerLayer(H, H, 4))
    with pytest.raises(pkg._lib.ScgibError):
        pkg.ops.gt_encoder(torch.zeros(2, IN), gh, pkg.models.Transformer(IN, H, 1, 4, "cpu"))
