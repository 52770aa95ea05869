"""``models.py``-compatible S-CGIB pretraining model on the HIP path.

Drop-in for the reference's classes on the north-star path, same
constructor/forward signatures and the same ``state_dict`` keys:

  MLP ................ models.py:38-49
  GIN ................ models.py:52-72   (GINConv sum aggregation -> HIP kernel)
  GCN, GraphSAGE ..... models.py:75-104  (GraphConv / SAGEConv layers -> the
                                          fused HIP layer of conv_layer.hip)
  Transformer ........ models.py:807-918 (per-edge attention + FFN layers ->
                                          the HIP kernels of gt_layer.hip)
  Mainmodel .......... models.py:546-782 (forward :662-700,
                                          extract_features :702-750)
  Mainmodel_continue . models.py:1010-1276 (the wrapper exp_pretraining.py
                                            actually trains, :109-113)

Differences from the reference, all deliberate:
  * the GIN depth is explicit: ``args.gin_layers`` (default 5, the shipped
    checkpoint's and the paper's depth; the shipped code builds 4 —
    models.py:57-58 — use ``gin_layers=4`` for code-as-shipped parity);
  * the compression + attention loops, the readouts and the dense N x N
    reconstruction loss run as fused HIP kernels (ops.py);
  * randomness: the reference draws the gate/feature noise from the CPU
    generator per graph (models.py:599, 650); here it is drawn on the device
    (counter-based Philox4x32-10 keyed by a device seed/offset,
    ops.device_noise / ops.seed_noise; the draws are kept in
    ``_last_noise`` — under ops.NoisePrefetch the static buffers, which the
    step's backward refills with the next step's draw), or passed explicitly with
    ``noise=(u_gate[N], u_feat[N,64])`` for parity with a recorded run;
  * ``args.readout_f`` / ``args.useAtt`` take the reference's values in all
    four classes: anything but "sum" is the Set2Set readout (both contrastive
    readouts through ops.set2set_pair, the loss at width 128), ``useAtt=0``
    the interaction without the attention; ``reduce_d`` never enters the
    graph (the query it would feed cancels in the per-graph softmax) and a
    Mainmodel_continue around a model of the other readout width is refused
    when it is built;
  * ``batch_g`` and ``flatten_batch_subgraphs`` may be any DGL-like graph
    (``edges()``, ``batch_num_nodes()``, ``num_nodes()``, ``ndata``): the four
    model classes pass them through ``graph.as_graph_batch`` once, at the top
    of ``forward`` / ``extract_features``; a ``graph.GraphBatch`` goes through
    untouched;
  * ``flatten_batch_subgraphs`` may be ``None``: the ego-nets are then built
    on the device from ``batch_g`` (scgib_egonet_*), replacing the offline
    khop_in_subgraph pass and the per-step dgl.batch of the reference;
  * encoders: "GIN" (the north-star path, with its fused pair / fold /
    deferred-reduce machinery), "GCN" and "GraphSAGE" (each layer one fused
    HIP launch forward and two backward, run through the plain two-stream
    encoder branch; DGL 1.1.0's GraphConv / SAGEConv semantics restated, not
    linked) and "Transformer" (Transformer / GraphTransformerLayer /
    MultiHeadAttentionLayer, models.py:807-918, on the kernels of
    gt_layer.hip; in the step each encoder is one autograd node behind the
    folded entry of gt_embed.hip, GT_FOLD) in all four model classes, with
    the reference's constructor arguments and state_dict keys.  The strings
    beyond those accepted before — "Transformer" anywhere, anything but "GIN"
    in the fine-tune / domain-adaptation classes — are accepted with
    ``models.ALL_ENCODER_STRINGS = True`` (off by default: see there).
"""
from __future__ import annotations

import contextlib
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import graph as G
from . import ops
from . import refckpt


class MLP(nn.Module):
    """Linear-ReLU-Linear (models.py:38-49)."""

    def __init__(self, num_features, num_classes, dims=16):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(num_features, dims), nn.ReLU(),
                                 nn.Linear(dims, num_classes))

    def forward(self, x):
        return self.mlp(x)


class GINConv(nn.Module):
    """DGL GINConv, sum aggregator, non-learnt eps buffer (models.py:63)."""

    def __init__(self, apply_func=None, aggregator_type="sum", init_eps=0.0, learn_eps=False,
                 activation=None):
        super().__init__()
        if aggregator_type != "sum" or learn_eps:
            raise NotImplementedError("only the reference's GINConv(sum, learn_eps=False)")
        self.apply_func = apply_func
        self.activation = activation
        self.register_buffer("eps", torch.FloatTensor([init_eps]))
        self._one_plus_eps = 1.0 + float(init_eps)  # host mirror: no device sync per call

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        key = prefix + "eps"
        if key in state_dict:
            self._one_plus_eps = 1.0 + float(state_dict[key].reshape(-1)[0])
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, graph, feat, edge_weight=None):
        rst = ops.gin_aggregate(feat, graph, self._one_plus_eps)
        if self.apply_func is not None:
            rst = self.apply_func(rst)
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class GIN(nn.Module):
    """GIN encoder: L x [GINConv(MLP) -> BatchNorm1d -> ReLU] (models.py:52-72)."""

    def __init__(self, input_dim, hidden_dim=64, num_gin_layers=5, fused=True):
        super().__init__()
        # fused: every layer runs as the fused HIP kernels of gin_layer.hip;
        # otherwise GINConv (HIP gather) + torch Linear/BatchNorm per layer.
        # Both paths run on the HIP device only.
        self.fused = fused and hidden_dim == 64 and input_dim in (32, 64)
        self.ginlayers = nn.ModuleList()
        self.batch_norms = nn.ModuleList()
        for layer in range(num_gin_layers):
            d_in = input_dim if layer == 0 else hidden_dim
            self.ginlayers.append(GINConv(MLP(d_in, hidden_dim, hidden_dim), learn_eps=False))
            self.batch_norms.append(nn.BatchNorm1d(hidden_dim))

    def forward(self, g, h):
        if self.fused:
            return ops.gin_encoder(h, g, self)
        for conv, bn in zip(self.ginlayers, self.batch_norms):
            h = F.relu(bn(conv(g, h)))
        return h


class GraphConv(nn.Module):
    """DGL GraphConv(in, out, norm='both', weight=True, bias=True): symmetric
    degree normalisation (degrees clamped to 1), ``weight`` stored [in, out],
    xavier-uniform; zero ``bias``.  A node without in-edges gets its bias
    (allow_zero_in_degree is accepted and never refuses a graph)."""

    def __init__(self, in_feats, out_feats, norm="both", weight=True, bias=True, activation=None,
                 allow_zero_in_degree=False):
        super().__init__()
        if norm != "both" or not weight or not bias:
            raise NotImplementedError("only the reference's GraphConv(norm='both', weight, bias)")
        self._in_feats, self._out_feats = in_feats, out_feats
        self._allow_zero_in_degree = allow_zero_in_degree
        self._activation = activation
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats))
        self.bias = nn.Parameter(torch.empty(out_feats))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight)
        nn.init.zeros_(self.bias)

    def conv_params(self):
        return self.weight, None, self.bias

    def forward(self, graph, feat, weight=None, edge_weight=None):
        if weight is not None or edge_weight is not None:
            raise NotImplementedError("GraphConv: external weight / edge_weight")
        rst = ops.conv_layer(feat, graph, self.weight, None, self.bias, "gcn", False)
        return rst if self._activation is None else self._activation(rst)


class SAGEConv(nn.Module):
    """DGL SAGEConv(in, out, 'mean'): fc_self(x_v) + fc_neigh(mean of the
    in-neighbours, 0 without any) + bias; both linears [out, in] without a
    bias of their own (xavier-uniform, ReLU gain), ``bias`` [out] zero.  An
    older file's ``fc_self.bias`` loads as ``bias``."""

    def __init__(self, in_feats, out_feats, aggregator_type, feat_drop=0.0, bias=True, norm=None,
                 activation=None):
        super().__init__()
        if aggregator_type != "mean" or feat_drop or not bias or norm is not None:
            raise NotImplementedError("only the reference's SAGEConv(in, out, 'mean')")
        self._in_src_feats = self._in_dst_feats = in_feats
        self._out_feats = out_feats
        self._aggre_type = aggregator_type
        self.activation = activation
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=False)
        self.fc_self = nn.Linear(in_feats, out_feats, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_feats))
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)
        nn.init.zeros_(self.bias)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        old = prefix + "fc_self.bias"  # (this module loads before its children see the key)
        if old in state_dict and prefix + "bias" not in state_dict:
            state_dict[prefix + "bias"] = state_dict.pop(old)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def conv_params(self):
        return self.fc_neigh.weight, self.fc_self.weight, self.bias

    def forward(self, graph, feat, edge_weight=None):
        if edge_weight is not None:
            raise NotImplementedError("SAGEConv: edge_weight")
        rst = ops.conv_layer(feat, graph, self.fc_neigh.weight, self.fc_self.weight, self.bias,
                             "mean", False)
        return rst if self.activation is None else self.activation(rst)


class GCN(nn.Module):
    """GCN encoder (models.py:75-88): conv1 (d -> 2H), ReLU, conv2 (2H -> 2H),
    ReLU, conv3 (2H -> H); no BatchNorm, no activation after conv3."""

    conv_mode = "gcn"
    fused = False  # not the fused GIN machinery (the fold gate of _encode_forked)

    def __init__(self, num_features, hidden_dim=64):
        super().__init__()
        self.conv1 = GraphConv(num_features, hidden_dim * 2, allow_zero_in_degree=True)
        self.conv2 = GraphConv(hidden_dim * 2, hidden_dim * 2, allow_zero_in_degree=True)
        self.conv3 = GraphConv(hidden_dim * 2, hidden_dim, allow_zero_in_degree=True)

    def layer_sequence(self):
        return [(self.conv1, True), (self.conv2, True), (self.conv3, False)]

    def forward(self, g, in_feat):
        return ops.conv_encoder(in_feat, g, self)


class GraphSAGE(nn.Module):
    """GraphSAGE encoder (models.py:91-104), with the reference's forward kept
    literally: conv1, ReLU, conv2, ReLU, conv2 AGAIN (models.py:103) — conv3
    is built (its keys are in the state_dict) and never used, so its
    gradients stay None and conv2's are the sum over its two uses."""

    conv_mode = "mean"
    fused = False

    def __init__(self, in_feats, h_feats):
        super().__init__()
        self.conv1 = SAGEConv(in_feats, h_feats, "mean")
        self.conv2 = SAGEConv(h_feats, h_feats, "mean")
        self.conv3 = SAGEConv(h_feats, h_feats, "mean")

    def layer_sequence(self):
        return [(self.conv1, True), (self.conv2, True), (self.conv2, False)]

    def forward(self, g, in_feat):
        return ops.conv_encoder(in_feat, g, self)


class MultiHeadAttentionLayer(nn.Module):
    """Per-edge multi-head attention (models.py:874-918): ``out_dim`` is the
    width of ONE head.  q_proj / k_proj / v_proj are built as in the reference
    (their keys are in the state_dict) and never used."""

    def __init__(self, in_dim, out_dim, num_heads):
        super().__init__()
        if num_heads <= 0 or in_dim % num_heads != 0:
            raise ValueError(f"MultiHeadAttentionLayer: width {in_dim} is not a multiple of "
                             f"num_heads {num_heads}")
        self.out_dim = out_dim
        self.num_heads = num_heads
        self.Q = nn.Linear(in_dim, out_dim * num_heads, bias=True)
        self.K = nn.Linear(in_dim, out_dim * num_heads, bias=True)
        self.V = nn.Linear(in_dim, out_dim * num_heads, bias=True)
        self.hidden_size = in_dim
        self.head_dim = out_dim // num_heads
        self.scaling = self.head_dim ** -0.5 if self.head_dim else 0.0  # (unused, as in the reference)
        self.q_proj = nn.Linear(in_dim, in_dim)
        self.k_proj = nn.Linear(in_dim, in_dim)
        self.v_proj = nn.Linear(in_dim, in_dim)

    def forward(self, h, g):
        """[N, num_heads, out_dim].  Stand-alone use only (the projections are
        torch linears here); GraphTransformerLayer runs the whole layer,
        projections included, through ops.gt_layer."""
        attn = ops.graph_attention(self.Q(h), self.K(h), self.V(h), g, self.num_heads)
        return attn.view(-1, self.num_heads, self.out_dim)


class GraphTransformerLayer(nn.Module):
    """Graph Transformer layer (models.py:832-871): attention, O, residual +
    LayerNorm, FFN (H -> 2H -> H, dropout 0.5), residual + LayerNorm, on the
    HIP kernels of gt_layer.hip.  batchnorm1 / batchnorm2 are built and never
    used: no gradient, running statistics never move."""

    def __init__(self, in_dim, out_dim, num_heads):
        super().__init__()
        if num_heads <= 0 or out_dim % num_heads != 0:
            raise ValueError(f"GraphTransformerLayer: width {out_dim} is not a multiple of "
                             f"num_heads {num_heads}")
        self.in_channels = in_dim
        self.out_channels = out_dim
        self.num_heads = num_heads
        self.attention = MultiHeadAttentionLayer(in_dim, out_dim // num_heads, num_heads)
        self.O = nn.Linear(out_dim, out_dim)
        self.batchnorm1 = nn.BatchNorm1d(out_dim)
        self.batchnorm2 = nn.BatchNorm1d(out_dim)
        self.layer_norm1 = nn.LayerNorm(out_dim)
        self.layer_norm2 = nn.LayerNorm(out_dim)
        self.FFN_layer1 = nn.Linear(out_dim, out_dim * 2)
        self.FFN_layer2 = nn.Linear(out_dim * 2, out_dim)

    def gt_params(self):
        """The 16 tensors the layer uses, in ops._GtLayer's order."""
        a = self.attention
        return (a.Q.weight, a.Q.bias, a.K.weight, a.K.bias, a.V.weight, a.V.bias,
                self.O.weight, self.O.bias, self.layer_norm1.weight, self.layer_norm1.bias,
                self.FFN_layer1.weight, self.FFN_layer1.bias, self.FFN_layer2.weight,
                self.FFN_layer2.bias, self.layer_norm2.weight, self.layer_norm2.bias)

    def forward(self, h, g, drop_mask=None):
        return ops.gt_layer(h, g, self, drop_mask)


class Transformer(nn.Module):
    """Transformer encoder (models.py:807-829): embedding_h (no bias) and
    num_layers + 1 GraphTransformerLayers — the reference appends one extra.
    ``drop_masks``: one explicit dropout mask (bool [N, 2H], True = keep) per
    layer instead of the device draw, for parity with a recorded run."""

    fused = False  # not the fused GIN machinery (the fold gate of _encode_forked)

    def __init__(self, in_dim, hidden_dim, num_layers, num_heads, device):
        super().__init__()
        if num_heads <= 0 or hidden_dim % num_heads != 0:
            raise ValueError(f"Transformer: hidden_dim {hidden_dim} is not a multiple of "
                             f"num_heads {num_heads}")
        self.h = None
        self.embedding_h = nn.Linear(in_dim, hidden_dim, bias=False)
        self.in_dim = in_dim
        self.hidden_dim = hidden_dim
        self.device = device
        self.layers = nn.ModuleList(
            [GraphTransformerLayer(hidden_dim, hidden_dim, num_heads) for _ in range(num_layers)])
        self.layers.append(GraphTransformerLayer(hidden_dim, hidden_dim, num_heads))

    def extract_features(self, g, h, drop_masks=None):
        return ops.gt_encoder(h, g, self, drop_masks)

    def forward(self, g, h, drop_masks=None):
        return self.extract_features(g, h, drop_masks)


ENCODERS = ("GIN", "GCN", "GraphSAGE")  # by string without ALL_ENCODER_STRINGS
ALL_ENCODERS = ENCODERS + ("Transformer",)  # the reference's ``--encoder`` values
# Every model class takes every reference encoder string.  Off (the default):
# the strings accepted are those from before the switch existed — ENCODERS in
# Mainmodel / Mainmodel_continue, "GIN" alone in Mainmodel_finetuning /
# Mainmodel_domainadapt — and anything else raises NotImplementedError, as it
# did.  A checkpoint that records an encoder is rebuilt with it either way.
ALL_ENCODER_STRINGS = False
_LOADING = [0]  # > 0 while load_checkpoint builds a file's own levels


@contextlib.contextmanager
def _loading():
    _LOADING[0] += 1
    try:
        yield
    finally:
        _LOADING[0] -= 1


def _make_encoder(encoder, in_dim, hidden_dim, args, num_layers, num_heads, head=False):
    """One encoder of a model class (models.py:156-167, :405-416, :573-587,
    :1060-1071).  ``head``: a fine-tune / domain-adaptation class, whose own
    encoders exist for state_dict parity only."""
    if encoder not in ALL_ENCODERS:
        raise NotImplementedError(f"encoder {encoder!r}: implemented are "
                                  f"{', '.join(ALL_ENCODERS)}")
    if not (ALL_ENCODER_STRINGS or _LOADING[0]) and \
            encoder not in (("GIN",) if head else ENCODERS):
        raise NotImplementedError(
            f"encoder {encoder!r}: accepted here with models.ALL_ENCODER_STRINGS = True "
            f"(off by default; without it: {'GIN' if head else ', '.join(ENCODERS)})")
    if encoder == "GIN":
        return GIN(in_dim, hidden_dim, _gin_layers(args))
    if encoder == "GCN":
        return GCN(in_dim, hidden_dim)
    if encoder == "GraphSAGE":
        return GraphSAGE(in_dim, hidden_dim)
    return Transformer(in_dim, hidden_dim, num_layers, num_heads, getattr(args, "device", None))


class Set2Set(nn.Module):
    """DGL Set2Set (LSTM(2d -> d), n_iters rounds; reference models.py:565,
    the fine-tune and domain-adaptation readout): the LSTM recurrence (PyTorch
    gate order i, f, g, o — the reference's single-layer nn.LSTM) and the
    per-graph softmax attention readouts of all rounds in ONE device launch
    per direction (ops.set2set, csrc/set2set.hip; one workgroup per graph).
    No host sync and no host->device copy, so a fine-tune step holding it is
    capturable.  ``lstm`` keeps nn.LSTM's parameters (state_dict parity)."""

    def __init__(self, input_dim, n_iters, n_layers):
        super().__init__()
        if n_layers != 1:
            raise NotImplementedError("Set2Set: the reference uses one LSTM layer")
        if not 1 <= input_dim <= 64:
            # (the device kernels hold a graph's features, 64 lanes wide; a
            # domain-adaptation model over raw features wider than 64 is
            # refused when it is built, not at its first step)
            raise NotImplementedError(f"Set2Set: input width {input_dim} (the device readout "
                                      "supports 1..64: the hidden width, or raw features)")
        self.input_dim, self.output_dim = input_dim, 2 * input_dim
        self.n_iters, self.n_layers = n_iters, n_layers
        self.lstm = nn.LSTM(self.output_dim, self.input_dim, n_layers)

    def forward(self, graph, feat):
        return ops.set2set(feat, graph, self.lstm, self.n_iters)


_SIDE_STREAMS = {}
# forward() runs the ego branch on a second stream (see _encode_forked);
# bench.py turns it off for its single-stream event-timed kernel pass
FORK_ENCODERS = True
# Design switches (module attributes, not environment knobs; tests set them):
# both folded encoders as one autograd node (ops.gin_encoder_pair_x)
PAIR_ENCODERS = True
# contrastive loss on the side stream, beside the head MLP + recon chain (off:
# measured 2-4 % slower — each cross-stream edge of a replayed graph costs more
# than the ~34 us of contrastive kernels it hides; a graph-replay test covers it)
FORK_LOSSES = False
# compressor[0] computed at the end of the core encoder chain (ops.gin_encoder_pair_x)
LIN_IN_PAIR = True
# head MLP + adjacency recon loss as one fused op (ops.mlp2_recon)
FUSE_RECON = True
# ... and the contrastive loss run in extra workgroups of the MLP + recon
# launches (ops.mlp2_recon_contrastive)
FUSE_CONTRAST = True
# gate / feature noise drawn by one Philox kernel (ops.device_noise) on the
# core encoder's chain instead of two torch.rand launches on the critical path
DEVICE_NOISE = True
# fine-tune head: predict (+ sigmoid) and the BCE loss on csrc/head.hip (four
# launches per step instead of ~19 torch ones; tests cover both sides); wider
# heads (C > 16), the MAE / RMSE / BCE-with-logits losses and MetricWrapper's
# NaN-masked "ignore-flatten" losses on csrc/task_head.hip
FUSE_HEAD = True
# loss_CrossEntropy on integer HIP targets through ops.class_loss
# (csrc/class_loss.hip) instead of F.cross_entropy.  Off by default: integer
# targets keep torch's bits.  float32 HIP targets — what the
# device loaders carry, which F.cross_entropy refuses — take the kernel always.
DEVICE_CE = False
# readout_f != "sum": the step's two Set2Set readouts (noisy and plain graph
# features, one LSTM) as one autograd node and one launch per direction
# (ops.set2set_pair); off: two ops.set2set calls (tools/readout_bench.py's A/B)
S2S_PAIR = True
# two Transformer encoders of width 64 behind the folded entry, each one
# autograd node with one weight-gradient reduce and a dropout lane of its own
# (ops.gt_encoder_x); off: the generic two-stream branch
GT_FOLD = True


_GRAPH_ATTRS = ("graph_features", "subgraphs_features", "_last_z1", "_last_kl_mean")


def _drop_graph_refs(*owners):
    """End of a training forward: the attributes the reference keeps
    (self.graph_features, ...) are kept detached, so the model does not hold
    this step's autograd graph — and with it the parameters' AccumulateGrad
    nodes — into the next step: a node created on another stream (a warm-up
    on a side stream before a HIP-graph capture) would then make torch warn
    about a cross-stream AccumulateGrad in the captured backward."""
    for o in owners:
        for a in _GRAPH_ATTRS:
            v = getattr(o, a, None)
            if isinstance(v, torch.Tensor) and v.requires_grad:
                setattr(o, a, v.detach())


def _side_stream(device):
    """The second HIP stream of ``device`` used by the forked encoder branch."""
    key = torch.device(device).index
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = ops.register_fork_stream(torch.cuda.Stream(device))
    return _SIDE_STREAMS[key]


def _gin_layers(args):
    return int(getattr(args, "gin_layers", 5))


def semi_loss(z1, z2, chunk):
    """batched_semi_loss, tau = 1 (models.py:606-629), fused on the device
    (scgib_contrastive_*).  The per-row value does not depend on the
    chunking."""
    return ops.contrastive(z1, z2)


class Explanation:
    """What ``explain`` reads off a batch.  Per atom, [N]:
    ``lam`` (the preservation gate), ``alpha`` (the attention weight of the
    atom's ego-net within its molecule; None with useAtt = 0), ``lam_rank`` /
    ``alpha_rank`` (int32 position inside the molecule by descending key, ties
    by ascending id, 0 = largest) and ``core_mask`` (bool).  ``core``: the
    graph core as a GraphBatch (``core.ndata["_ID"]`` = original node ids).
    ``centres`` / ``weights`` [B, top_m]: the atoms whose ego-nets carry the
    largest attention, and their alpha (-1 / 0 past a molecule's size; None
    when ``top_m`` = 0).  ``ego``: the step's ego batch; the atoms of the
    ego-net of centre c are ``ego.ndata["_ID"][ego.graph_ptr[c] :
    ego.graph_ptr[c + 1]]``."""

    __slots__ = ("lam", "alpha", "lam_rank", "alpha_rank", "core", "core_mask", "centres",
                 "weights", "ego")

    def __init__(self, **fields):
        for name in self.__slots__:
            setattr(self, name, fields[name])

    def subgraph_nodes(self):
        """Host convenience (synchronises: three device reads): per molecule the
        list of (centre id, alpha, original node ids of the centre's ego-net)
        of its significant subgraphs, in rank order."""
        if self.centres is None:
            raise ops._lib.ScgibError("subgraph_nodes: no significant subgraphs (top_m = 0)")
        centres, weights = self.centres.cpu().tolist(), self.weights.cpu().tolist()
        ptr, ids = self.ego.graph_ptr.cpu(), self.ego.ndata["_ID"].cpu()
        return [[(c, w, ids[int(ptr[c]):int(ptr[c + 1])].tolist())
                 for c, w in zip(cs, ws) if c >= 0] for cs, ws in zip(centres, weights)]


def _explain(who, enc_owner, transfer, k, batch_g, batch_x, flatten_batch_subgraphs, x_subs,
             ratio, threshold, top_m, u_gate, with_core=True):
    """``explain`` of the four model classes: the eval forward of ``enc_owner``
    (the module their forward hands ``_extract``) up to the interaction, then
    ops.explain_rank and ops.core_subgraph (``with_core`` False, the dataset
    pass: no core, ``core`` / ``core_mask`` None).  Moves no state: no
    BatchNorm buffer (eval mode is required), no noise draw."""
    if who.training or enc_owner.training:
        raise RuntimeError("explain() needs model.eval(): a train-mode forward would move the "
                           "BatchNorm running statistics")
    if not batch_x.is_cuda:
        raise ops._lib.ScgibError(f"explain: features on {batch_x.device}; the S-CGIB ops run on "
                                  "the HIP device only (no CPU fallback)")
    use_att = bool(enc_owner.useAtt)
    top_m = int(top_m or 0)
    if top_m and not use_att:
        raise ValueError("explain: top_m >= 1 asks for significant subgraphs, but the model has "
                         "no attention (useAtt = 0); pass top_m=0")
    with torch.no_grad():
        batch_g = G.as_graph_batch(batch_g)
        if flatten_batch_subgraphs is None:
            ego = G.egonet_batch(batch_g, k)
        else:
            ego = G.as_graph_batch(flatten_batch_subgraphs)
        if x_subs is None:
            x_subs = batch_x.index_select(0, ego.ndata["_ID"])
        graph_features = enc_owner.Encoder1(batch_g, transfer(batch_x))
        sub_readout = ops.segment_sum(enc_owner.Encoder2(ego, transfer(x_subs)), ego.graph_ptr,
                                      ego.batch_size, ego.seg_dims)
        lam, logit = ops.interaction_gates(graph_features, sub_readout, u_gate,
                                           enc_owner.compressor, enc_owner.attn_layer, batch_g,
                                           False, use_att)
        alpha, lam_rank, alpha_rank, centres, weights = ops.explain_rank(lam, logit, batch_g, top_m)
        core = core_mask = None
        if with_core:
            core, core_mask = ops.core_subgraph(lam, lam_rank, batch_g,
                                                None if threshold is not None else ratio,
                                                threshold)
    return Explanation(lam=lam, alpha=alpha, lam_rank=lam_rank, alpha_rank=alpha_rank, core=core,
                       core_mask=core_mask, centres=centres, weights=weights, ego=ego)


def _explain_route(model):
    """(encoder owner, transfer_d, k) that ``model.explain`` runs: the module
    its forward hands ``_extract``, with the model's own transfer_d."""
    if isinstance(model, Mainmodel):
        return model, model.transfer_d, model.k_transition
    if isinstance(model, (Mainmodel_continue, Mainmodel_domainadapt)):
        return model.model, model.transfer_d, model.k_transition
    if isinstance(model, Mainmodel_finetuning):
        return model.model, model.transfer_d, getattr(model.model, "k_transition",
                                                      model.k_transition)
    raise TypeError(f"explain: {type(model).__name__} is none of the four S-CGIB model classes")


class _Explainable:
    """``explain`` of the four model classes."""

    def explain(self, batch_g, batch_x, flatten_batch_subgraphs=None, x_subs=None, *, ratio=0.5,
                threshold=None, top_m=3, u_gate=None):
        """Graph core and significant subgraphs of a batch.

        Runs the eval-mode forward up to the interaction under no_grad and
        returns an ``Explanation``.  ``ratio`` in (0, 1] keeps the
        ``max(1, ceil(n_i * ratio))`` atoms of largest gate per molecule;
        ``threshold`` (replaces ratio) keeps the atoms with lam >= threshold.
        ``top_m``: significant subgraphs per molecule (0: none; with useAtt = 0
        anything else raises).  ``u_gate`` [N]: the gate draw; None is 0.5
        everywhere, the median gate, which makes the result deterministic.
        Needs ``model.eval()``; leaves state_dict() and the device noise state
        bitwise unchanged.  Graph arguments as in ``forward``."""
        return _explain(self, *_explain_route(self), batch_g, batch_x, flatten_batch_subgraphs,
                        x_subs, ratio, threshold, top_m, u_gate)


class _SCGIBCore(_Explainable, nn.Module):
    """Shared hot-path logic of Mainmodel / Mainmodel_continue."""

    def _prepare_ego(self, batch_g, flatten_batch_subgraphs, batch_x, x_subs):
        if flatten_batch_subgraphs is None:
            ego = G.egonet_batch(batch_g, self.k_transition)
            if x_subs is None:
                x_subs = batch_x.index_select(0, ego.ndata["_ID"])
            return ego, x_subs
        return flatten_batch_subgraphs, x_subs

    def _noise(self, n, device, noise):
        if noise is not None:
            u_gate, u_feat = noise
            return u_gate.reshape(-1), u_feat
        if DEVICE_NOISE and self.hidden_dim == 64:
            return ops.device_noise(n, device)  # Philox on the device, one launch
        ops.note_torch_rng()  # (a capture of this draw must be replayed by torch: ops.SplitGraph)
        return (torch.rand(n, device=device, dtype=torch.float32),
                torch.rand(n, self.hidden_dim, device=device, dtype=torch.float32))

    def _extract(self, enc_owner, batch_g, batch_x, ego, x_subs, noise, encoded=None,
                 z1_s2s=None, readouts=True):
        """extract_features of ``enc_owner`` (models.py:702-750); returns the
        reference's 4-tuple plus z1 = sum_nodes(noisy) (computed in-kernel).
        ``enc_owner.useAtt`` = 0 runs the interaction without the attention;
        ``enc_owner.readout`` != "sum" (the reference: anything else is
        Set2Set) replaces both readouts by Set2Set ones [B, 128], z1 through
        ``z1_s2s`` (a wrapper's own Set2Set, models.py:1184) when given.  The
        attention's query, reduce_d(s2s(noisy)) there, is constant within a
        graph and cancels in the softmax as the sum readout does, so the
        interaction launch is the same and reduce_d stays out of the graph.
        ``readouts`` False: the caller reads the interaction map only (the
        fine-tune / domain-adaptation heads), no Set2Set readout is run.
        ``encoded`` = (graph_features, subgraphs_features, sub_readout, t, drawn)
        when the encoders already ran (_encode_forked); t = compressor[0](graph
        features) and drawn = the device noise when the encoder pair's core
        chain computed them (else None)."""
        t = drawn = None
        if encoded is None:
            graph_features = enc_owner.Encoder1(batch_g, batch_x)
            subgraphs_features = enc_owner.Encoder2(ego, x_subs)
            sub_readout = ops.segment_sum(subgraphs_features, ego.graph_ptr, ego.batch_size,
                                          ego.seg_dims)
        else:
            graph_features, subgraphs_features, sub_readout, t, drawn = encoded
        enc_owner.graph_features = graph_features
        enc_owner.subgraphs_features = subgraphs_features
        if noise is None and drawn is not None:  # drawn on the core encoder's chain
            u_gate, u_feat = drawn
        else:
            u_gate, u_feat = self._noise(graph_features.shape[0], graph_features.device, noise)
        # compressor[0] (models.py:1092) runs fused in front of the interaction
        # its aside work (the compressor-BN running update) is enqueued at
        # the model's join_aside(), after the losses (ops.LATE_FORK)
        use_att = bool(enc_owner.useAtt)
        with ops.aside_deferred():
            if t is not None:
                comp = enc_owner.compressor
                im, z1, z2, kl, kl_mean = ops.interaction(graph_features, t, sub_readout, u_gate,
                                                          u_feat, comp[1], comp[3],
                                                          enc_owner.attn_layer, batch_g,
                                                          enc_owner.training, use_att)
            else:
                im, z1, z2, kl, kl_mean = ops.interaction_lin(graph_features, sub_readout,
                                                              u_gate, u_feat,
                                                              enc_owner.compressor,
                                                              enc_owner.attn_layer, batch_g,
                                                              enc_owner.training, use_att)
        ops.stamp("interaction_end")
        enc_owner._last_kl_mean = kl_mean
        # the draws when noise was None (replayable via noise=)
        enc_owner._last_noise = (u_gate, u_feat) if noise is None else None
        noisy = im[:, : self.hidden_dim]
        if enc_owner.readout != "sum" and readouts:
            # the interaction's own sum readouts are unused (their gradients
            # reach its backward as NULL)
            inner, outer = enc_owner.s2s, (z1_s2s if z1_s2s is not None else enc_owner.s2s)
            if S2S_PAIR and outer is inner:
                z1, z2 = ops.set2set_pair(noisy, graph_features, batch_g, inner.lstm,
                                          inner.n_iters)
            else:  # a wrapper's LSTM for z1, the wrapped model's for z2: two launches
                z1 = ops.set2set(noisy, batch_g, outer.lstm, outer.n_iters)
                z2 = ops.set2set(graph_features, batch_g, inner.lstm, inner.n_iters)
        return im, kl, noisy, z2, z1

    def _encode_forked(self, enc_owner, batch_g, batch_x, fork=True, draw_noise=False,
                       transfer=None):
        """Fast path of forward() when the ego-nets are built on the device:
        the ego branch (ego-net build, x_subs gather, transfer_d, Encoder2,
        readout) runs on a second HIP stream, concurrently with Encoder1 on the
        current one (Encoder1's ~N/64 tiles leave most of the 256 CUs idle).
        Captured into a HIP graph this is a fork/join; autograd runs each
        branch's backward on the stream its forward ran on, so the two
        encoders' backward chains overlap as well."""
        main = torch.cuda.current_stream(batch_x.device)
        side = _side_stream(batch_x.device) if fork else main
        # transfer_d folded into both encoders' first layer (raw features are
        # gathered in-kernel, through the ego -> parent map for Encoder2);
        # ``transfer``: another module's transfer_d (the fine-tune head's)
        td = self.transfer_d if transfer is None else transfer
        fold = (enc_owner.Encoder1.fused and enc_owner.Encoder2.fused
                and td.bias is None and td.out_features == 32
                and batch_x.shape[1] <= 16 and not batch_x.requires_grad)
        if fork:
            ops.check_fork(main)  # never a nested fork while capturing (ops.check_fork)
        side.wait_stream(main)
        batch_x.record_stream(side)
        if fold and PAIR_ENCODERS:
            # one autograd node for both encoders (ops._GinEncoderPair): the
            # ego chain is enqueued first on ``side`` in forward AND backward
            # (fork off: side is the current stream, the chains run in turn)
            # graph.EgoPrefetch: this batch's ego-nets were built during the
            # previous step; the next batch's are built on ``side`` after the
            # ego chain (its idle stretch through the loss section)
            pf = getattr(batch_g, "ego_prefetch", None)
            if pf is not None and not (pf.loaded and pf.k == self.k_transition):
                pf = None
            with torch.cuda.stream(side):
                ego = pf.ego if pf is not None else G.egonet_batch(batch_g, self.k_transition)
            lin0 = enc_owner.compressor[0] if LIN_IN_PAIR else None
            drawn = {}
            tail = bwd_tail = None
            if draw_noise and DEVICE_NOISE and self.hidden_dim == 64:
                # ops.NoisePrefetch (a training step with a backward): this
                # step's noise was drawn by the previous step's backward, and
                # this step's backward draws the next one's
                nf = getattr(batch_g, "noise_prefetch", None)
                # (only when the pair will run a backward: a trainable encoder
                # or transfer_d parameter — a fully frozen pair never redraws)
                if (nf is not None and nf.n == batch_g.num_nodes() and enc_owner.training
                        and torch.is_grad_enabled()
                        and any(p.requires_grad for m in (enc_owner.Encoder1, enc_owner.Encoder2, td)
                                for p in m.parameters())):
                    drawn["u"] = (nf.u_gate, nf.u_feat)
                    bwd_tail = nf.draw
                else:
                    def tail():  # the interaction's noise, drawn beside the ego chain
                        drawn["u"] = ops.device_noise(batch_g.num_nodes(), batch_x.device)
            outs = ops.gin_encoder_pair_x(
                batch_x, ego, enc_owner.Encoder2, batch_g, enc_owner.Encoder1, td,
                ego.ndata["_ID"], side, lin0, tail, pf, bwd_tail)
            subgraphs_features, sub_readout, graph_features = outs[0], outs[1], outs[2]
            t = outs[3] if len(outs) > 3 else None
            return ego, (graph_features, subgraphs_features, sub_readout, t, drawn.get("u"))
        e1, e2 = enc_owner.Encoder1, enc_owner.Encoder2
        if (GT_FOLD and isinstance(e1, Transformer) and isinstance(e2, Transformer)
                and all(e.hidden_dim == 64 and e.embedding_h.in_features == 32
                        and e.layers[0].num_heads in ops.GT_HEADS for e in (e1, e2))
                and td.bias is None and td.out_features == 32
                and batch_x.shape[1] <= 16 and not batch_x.requires_grad):
            # each Transformer one autograd node behind the folded entry
            # (ops.gt_encoder_x): the features gathered in-kernel, transfer_d
            # and embedding_h one launch, one weight-gradient reduce per
            # encoder; the ego chain draws its dropout from lane 1, so either
            # state is advanced by one chain in stream order (reproducible
            # whether or not the chains overlap)
            with torch.cuda.stream(side):
                ego = G.egonet_batch(batch_g, self.k_transition)
                subgraphs_features, sub_readout = ops.gt_encoder_x(
                    batch_x, ego, e2, td, ego.ndata["_ID"],
                    readout=(ego.graph_ptr, ego.batch_size, ego.seg_dims), lane=1)
            graph_features = ops.gt_encoder_x(batch_x, batch_g, e1, td, lane=0)
            main.wait_stream(side)
            subgraphs_features.record_stream(main)
            sub_readout.record_stream(main)
            return ego, (graph_features, subgraphs_features, sub_readout, None, None)
        with torch.cuda.stream(side):
            if fold:
                ego = G.egonet_batch(batch_g, self.k_transition)
                subgraphs_features = ops.gin_encoder_x(batch_x, ego, enc_owner.Encoder2,
                                                       td, ego.ndata["_ID"])
            else:
                ego, x_subs = self._prepare_ego(batch_g, None, batch_x, None)
                subgraphs_features = enc_owner.Encoder2(ego, td(x_subs))
            sub_readout = ops.segment_sum(subgraphs_features, ego.graph_ptr, ego.batch_size,
                                          ego.seg_dims)
        if fold:
            graph_features = ops.gin_encoder_x(batch_x, batch_g, enc_owner.Encoder1, td)
        else:
            graph_features = enc_owner.Encoder1(batch_g, td(batch_x))
        main.wait_stream(side)
        subgraphs_features.record_stream(main)
        sub_readout.record_stream(main)
        return ego, (graph_features, subgraphs_features, sub_readout, None, None)

    def _losses(self, batch_g, im, kl_mean, z1, z2, mlp, batch_size, batch_logMs=None,
                ego=None):
        # the contrastive loss needs only the two readouts: on the side stream
        # it (and, through autograd, its backward) overlaps the head MLP and
        # the reconstruction loss, which form the critical path
        side = _side_stream(im.device) if (FORK_LOSSES and im.is_cuda) else None
        if side is not None:
            main = torch.cuda.current_stream(im.device)
            ops.check_fork(main)
            side.wait_stream(main)
            z1.record_stream(side)
            z2.record_stream(side)
            with torch.cuda.stream(side):
                con = semi_loss(z1, z2, batch_size)
        kl_loss = kl_mean  # == torch.mean(KL_tensor) (models.py:679), computed in-kernel
        # (Set2Set readouts, [B, 128]: the width-128 contrastive kernels in
        # launches of their own beside ops.mlp2_recon; the fused launch holds
        # the width-64 body)
        if side is None and self.recons_type == "adj" and FUSE_RECON and FUSE_CONTRAST \
                and im.is_cuda and im.shape[1] == 2 * self.hidden_dim == 128 \
                and z1.shape[1] == self.hidden_dim:
            # models.py:1174 + loss_recon_adj (:1256-1262) + batched_semi_loss
            # (:606-629) in the same launches
            rec, con = ops.mlp2_recon_contrastive(im, mlp, batch_g, z1, z2)
            return kl_loss, con, rec
        if side is None:
            con = semi_loss(z1, z2, batch_size)
        if self.recons_type == "adj" and FUSE_RECON:
            # models.py:1174 + loss_recon_adj (:1256-1262): MLP and recon fused
            rec = ops.mlp2_recon(im, mlp, batch_g)
            return kl_loss, self._join_losses(side, con), rec
        im = ops.mlp2(im, mlp, batch_g.dims)  # models.py:1174, fused
        if self.recons_type == "adj":
            rec = ops.recon_adj(im, batch_g)
        elif self.recons_type == "logM":  # models.py:692-693 / 770-782
            if batch_logMs is None:
                if not im.is_cuda:
                    raise ValueError("recons_type='logM' needs batch_logMs (graph.trans_logM per "
                                     "molecule, or a graph.LogMBatch) on CPU tensors")
                # targets built on the device from the step's own ego batch
                # (``ego``: the one the encoders ran on, when this step built
                # it; k_transition is the ball radius and kstep, as in the
                # reference's exp_tudataset.py)
                batch_logMs = G.logm_targets(batch_g, self.k_transition, ego)
            rec = ops.recon_logm(im, batch_g, batch_logMs)
        else:  # the reference returns -1.0 (models.py:694-695)
            rec = torch.tensor(-1.0, device=im.device)
        return kl_loss, self._join_losses(side, con), rec

    @staticmethod
    def _join_losses(side, con):
        if side is not None:
            main = torch.cuda.current_stream(con.device)
            main.wait_stream(side)
            con.record_stream(main)
        return con


class Mainmodel(_SCGIBCore):
    def __init__(self, args, in_dim, hidden_dim, num_layers, num_heads, k_transition, encoder):
        super().__init__()
        self.tau = 1.0
        self.recons_type = args.recons_type
        self.useAtt = args.useAtt
        self.readout = args.readout_f
        self.hidden_dim = hidden_dim
        self.k_transition = k_transition
        self.fc1 = nn.Linear(hidden_dim, 1)
        self.in_dim = args.d_transfer
        self.transfer_d = nn.Linear(in_dim, self.in_dim, bias=False)
        self.embedding_h = nn.Linear(self.in_dim, hidden_dim, bias=False)
        self.attn_layer = nn.Linear(self.hidden_dim * 2, 1)
        self.reduce_d = nn.Linear(2 * self.hidden_dim, self.hidden_dim)
        self.device = getattr(args, "device", None)
        self.s2s = Set2Set(hidden_dim, 2, 1)
        self.reconstructX = nn.Sequential(nn.Linear(self.hidden_dim, self.in_dim))
        self.MLP = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU(),
                                 nn.Linear(hidden_dim, hidden_dim))
        self.encoder_name, self.num_layers, self.num_heads = encoder, num_layers, num_heads
        self.Encoder1 = _make_encoder(encoder, self.in_dim, hidden_dim, args, num_layers, num_heads)
        self.Encoder2 = _make_encoder(encoder, self.in_dim, hidden_dim, args, num_layers, num_heads)
        self.compressor = nn.Sequential(nn.Linear(hidden_dim, hidden_dim),
                                        nn.BatchNorm1d(hidden_dim), nn.ReLU(),
                                        nn.Linear(hidden_dim, 1))

    @ops.aside_guard
    def extract_features(self, nodes_list, batch_g, batch_x, flatten_batch_subgraphs, x_subs,
                         device=None, noise=None):
        batch_g = G.as_graph_batch(batch_g)
        if flatten_batch_subgraphs is not None:
            flatten_batch_subgraphs = G.as_graph_batch(flatten_batch_subgraphs)
        ego, x_subs = self._prepare_ego(batch_g, flatten_batch_subgraphs, batch_x, x_subs)
        im, kl, noisy, z2, z1 = self._extract(self, batch_g, batch_x, ego, x_subs, noise)
        self._last_z1 = z1
        ops.join_aside()
        return im, kl, noisy, z2

    @ops.aside_guard
    def forward(self, batch_g, batch_x, flatten_batch_subgraphs, batch_logMs, x_subs,
                current_epoch=None, edge_index=None, k_transition=None, device=None,
                batch_size=16, noise=None):
        self.batch_size = batch_size
        batch_g = G.as_graph_batch(batch_g)
        if flatten_batch_subgraphs is not None:
            flatten_batch_subgraphs = G.as_graph_batch(flatten_batch_subgraphs)
        if flatten_batch_subgraphs is None and x_subs is None and batch_x.is_cuda:
            ego, enc = self._encode_forked(self, batch_g, batch_x, FORK_ENCODERS,
                                           noise is None)
            im, _, _, z2, z1 = self._extract(self, batch_g, None, ego, None, noise, enc)
            self._last_z1 = z1
        else:
            ego = None
            if flatten_batch_subgraphs is None:
                flatten_batch_subgraphs, x_subs = self._prepare_ego(batch_g, None, batch_x,
                                                                    x_subs)
                ego = flatten_batch_subgraphs  # built here on the device: reused by logM
            batch_x = self.transfer_d(batch_x)
            x_subs = self.transfer_d(x_subs)
            im, kl, noisy, z2 = self.extract_features(None, batch_g, batch_x,
                                                      flatten_batch_subgraphs, x_subs, device,
                                                      noise)
        kl_loss, con, rec = self._losses(batch_g, im, self._last_kl_mean, self._last_z1, z2,
                                         self.MLP, batch_size, batch_logMs, ego)
        ops.join_aside()
        _drop_graph_refs(self)
        return None, kl_loss, con, rec


class Mainmodel_continue(_SCGIBCore):
    """The pretraining wrapper (models.py:1010-1276): its own transfer_d and
    MLP around the wrapped model's extract_features (models.py:1167)."""

    def __init__(self, args, in_dim, hidden_dim, num_layers, num_heads, k_transition,
                 num_classes, cp_filename, encoder):
        super().__init__()
        self.tau = 1.0
        self.readout = args.readout_f
        self.s2s = Set2Set(hidden_dim, 2, 1)
        self.s2s_rev = Set2Set(in_dim, 2, 1)
        self.in_dim = args.d_transfer
        self.transfer_d = nn.Linear(in_dim, self.in_dim, bias=False)
        self.recons_type = args.recons_type
        self.batch_size = getattr(args, "batch_size", 16)
        self.useAtt = args.useAtt
        self.embedding_h = nn.Linear(self.in_dim, hidden_dim, bias=False)
        self.hidden_dim = hidden_dim
        self.k_transition = k_transition
        self.reduce_d = nn.Linear(2 * hidden_dim, hidden_dim)
        self.attn_layer = nn.Linear(2 * hidden_dim, 1)
        self.num_nodes = -1
        self.device = getattr(args, "device", None)
        self.r_transfer_d = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU(),
                                          nn.Linear(hidden_dim, in_dim * 2))
        out_dim = 1 if getattr(args, "task", "graph_classification") == "graph_regression" \
            else num_classes
        self.predict = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU(),
                                     nn.Linear(hidden_dim, out_dim))
        self.MLP = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU(),
                                 nn.Linear(hidden_dim, hidden_dim))
        self.encoder_name, self.num_layers, self.num_heads = encoder, num_layers, num_heads
        self.Encoder1 = _make_encoder(encoder, self.in_dim, hidden_dim, args, num_layers, num_heads)
        self.Encoder2 = _make_encoder(encoder, self.in_dim, hidden_dim, args, num_layers, num_heads)
        self.model = load_checkpoint(cp_filename, args)
        inner_readout = getattr(self.model, "readout", "sum")
        if (self.readout == "sum") != (inner_readout == "sum"):
            # the reference fails in the contrastive loss's torch.mm here: its
            # z1 comes from this wrapper's readout, its z2 from the wrapped
            # model's (models.py:1184 / :718), 64 against 128 columns
            raise ValueError(f"Mainmodel_continue: readout_f={self.readout!r} around a model "
                             f"built with readout_f={inner_readout!r}: the contrastive loss "
                             "would compare readouts of 64 and 128 columns")
        for p in self.model.parameters():
            p.requires_grad = True
        self.compressor = nn.Sequential(nn.Linear(hidden_dim, hidden_dim),
                                        nn.BatchNorm1d(hidden_dim), nn.ReLU(),
                                        nn.Linear(hidden_dim, 1))
        self.reconstructX = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
                                          nn.Linear(hidden_dim, in_dim))

    @ops.aside_guard
    def extract_features(self, nodes_list, batch_g, batch_x, flatten_batch_subgraphs, x_subs,
                         device=None, noise=None):
        batch_g = G.as_graph_batch(batch_g)
        if flatten_batch_subgraphs is not None:
            flatten_batch_subgraphs = G.as_graph_batch(flatten_batch_subgraphs)
        ego, x_subs = self._prepare_ego(batch_g, flatten_batch_subgraphs, batch_x, x_subs)
        im, kl, noisy, z2, z1 = self._extract(self, batch_g, batch_x, ego, x_subs, noise)
        self._last_z1 = z1
        ops.join_aside()
        return im, kl, noisy, z2

    def _wrapper_s2s(self):
        """This wrapper's Set2Set for the contrastive z1 (models.py:1184), when
        the readout is Set2Set; None for the sum readout."""
        return self.s2s if self.readout != "sum" else None

    @ops.aside_guard
    def forward(self, batch_g, batch_x, flatten_batch_subgraphs, batch_logMs, x_subs,
                current_epoch=None, edge_index=None, k_transition=None, device=None,
                batch_size=16, noise=None):
        self.batch_size = batch_size
        batch_g = G.as_graph_batch(batch_g)
        if flatten_batch_subgraphs is not None:
            flatten_batch_subgraphs = G.as_graph_batch(flatten_batch_subgraphs)
        if flatten_batch_subgraphs is None and x_subs is None and batch_x.is_cuda:
            # the wrapper's transfer_d feeds the wrapped model's encoders
            ego, enc = self._encode_forked(self.model, batch_g, batch_x, FORK_ENCODERS,
                                           noise is None)
            im, _, _, z2, z1 = self.model._extract(self.model, batch_g, None, ego, None, noise,
                                                   enc, self._wrapper_s2s())
            self.model._last_z1 = z1
        else:
            ego = None
            if flatten_batch_subgraphs is None:
                flatten_batch_subgraphs, x_subs = self._prepare_ego(batch_g, None, batch_x,
                                                                    x_subs)
                ego = flatten_batch_subgraphs  # built here on the device: reused by logM
            batch_x = self.transfer_d(batch_x)
            x_subs = self.transfer_d(x_subs)
            im, kl, noisy, z2 = self.model.extract_features(None, batch_g, batch_x,
                                                            flatten_batch_subgraphs, x_subs,
                                                            device, noise)
            if self.readout != "sum":  # z1 through this wrapper's own Set2Set
                self.model._last_z1 = ops.set2set(noisy, batch_g, self.s2s.lstm,
                                                  self.s2s.n_iters)
        kl_loss, con, rec = self._losses(batch_g, im, self.model._last_kl_mean,
                                         self.model._last_z1, z2, self.MLP, batch_size,
                                         batch_logMs, ego)
        ops.stamp("losses_end")
        ops.join_aside()
        _drop_graph_refs(self, self.model)
        return None, kl_loss, con, rec


# ---------------------------------------------------------------------------
# Domain adaptation
# ---------------------------------------------------------------------------
class Mainmodel_domainadapt(_SCGIBCore):
    """models.py:107-355, driven by run_domain_adaptation (exp_molhiv.py:50-68,
    train_molhiv.py:74-105): the pretrained model's extract_features (every
    parameter trainable) -> MLP -> Set2Set -> r_transfer_d, regressed onto
    Set2Set(raw normalised features) — loss_X = sum of squared differences.

    Same constructor / forward signatures and state_dict keys as the
    reference.  Kept quirks: the model's OWN Encoder1 / Encoder2 /
    compressor / attn_layer are built but unused by forward, and its
    extract_features (models.py:283) runs exactly those — so fine-tuning on
    an adapted model (exp_molhiv.py:129, Mainmodel_finetuning loads it) runs
    freshly initialised encoders, as the reference does."""

    def __init__(self, args, in_dim, hidden_dim, num_layers, num_heads, k_transition,
                 num_classes, cp_filename, encoder):
        super().__init__()
        self.tau = 1.0
        self.readout = args.readout_f
        self.s2s = Set2Set(hidden_dim, 2, 1)
        self.s2s_rev = Set2Set(in_dim, 2, 1)
        self.in_dim = args.d_transfer
        self.transfer_d = nn.Linear(in_dim, self.in_dim, bias=False)
        self.batch_size = getattr(args, "batch_size", 16)
        self.useAtt = args.useAtt
        self.embedding_h = nn.Linear(self.in_dim, hidden_dim, bias=False)
        self.hidden_dim = hidden_dim
        self.k_transition = k_transition
        self.reduce_d = nn.Linear(2 * hidden_dim, hidden_dim)
        self.attn_layer = nn.Linear(2 * hidden_dim, 1)
        self.num_nodes = -1
        self.device = getattr(args, "device", None)
        self.r_transfer_d = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU(),
                                          nn.Linear(hidden_dim, in_dim * 2))
        task = getattr(args, "task", "graph_classification")
        if task in ("graph_regression", "graph_classification"):  # else: no head (:141)
            out_dim = 1 if task == "graph_regression" else num_classes
            self.predict = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU(),
                                         nn.Linear(hidden_dim, out_dim))
        self.MLP = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU(),
                                 nn.Linear(hidden_dim, hidden_dim))
        self.encoder_name, self.num_layers, self.num_heads = encoder, num_layers, num_heads
        self.Encoder1 = _make_encoder(encoder, self.in_dim, hidden_dim, args, num_layers, num_heads,
                                      True)
        self.Encoder2 = _make_encoder(encoder, self.in_dim, hidden_dim, args, num_layers, num_heads,
                                      True)
        self.model = load_checkpoint(cp_filename, args)
        for p in self.model.parameters():
            p.requires_grad = True
        self.compressor = nn.Sequential(nn.Linear(hidden_dim, hidden_dim),
                                        nn.BatchNorm1d(hidden_dim), nn.ReLU(),
                                        nn.Linear(hidden_dim, 1))
        self.reconstructX = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
                                          nn.Linear(hidden_dim, in_dim))

    @ops.aside_guard
    def extract_features(self, nodes_list, batch_g, batch_x, flatten_batch_subgraphs, x_subs,
                         device=None, noise=None):
        """models.py:283-335: the DA model's own encoders / compressor /
        attention (what fine-tuning on an adapted checkpoint runs)."""
        batch_g = G.as_graph_batch(batch_g)
        if flatten_batch_subgraphs is not None:
            flatten_batch_subgraphs = G.as_graph_batch(flatten_batch_subgraphs)
        ego, x_subs = self._prepare_ego(batch_g, flatten_batch_subgraphs, batch_x, x_subs)
        im, kl, noisy, z2, z1 = self._extract(self, batch_g, batch_x, ego, x_subs, noise)
        self._last_z1 = z1
        ops.join_aside()
        return im, kl, noisy, z2

    @ops.aside_guard
    def forward(self, batch_g, batch_x, flatten_batch_subgraphs, batch_logMs, x_subs,
                current_epoch=None, edge_index=None, k_transition=None, device=None,
                batch_size=16, noise=None):
        self.batch_size = batch_size
        self.device = device
        batch_x_org = batch_x
        batch_g = G.as_graph_batch(batch_g)
        if flatten_batch_subgraphs is not None:
            flatten_batch_subgraphs = G.as_graph_batch(flatten_batch_subgraphs)
        inner = self.model
        if flatten_batch_subgraphs is None and x_subs is None and batch_x.is_cuda:
            # this model's transfer_d feeds the pretrained model's encoders
            # (folded into their first layers), ego branch forked
            ego, enc = self._encode_forked(inner, batch_g, batch_x, FORK_ENCODERS,
                                           noise is None)
            im = inner._extract(inner, batch_g, None, ego, None, noise, enc, readouts=False)[0]
        else:
            if flatten_batch_subgraphs is None:
                flatten_batch_subgraphs, x_subs = self._prepare_ego(batch_g, None, batch_x,
                                                                    x_subs)
            im = inner.extract_features(None, batch_g, self.transfer_d(batch_x),
                                        flatten_batch_subgraphs, self.transfer_d(x_subs),
                                        device, noise)[0]
        im = ops.mlp2(im, self.MLP, batch_g.dims)  # 2d -> d
        im = self.r_transfer_d(self.s2s(batch_g, im))  # [B, 2 in_dim]
        org_x = self.s2s_rev(batch_g, batch_x_org)  # [B, 2 in_dim]
        loss = self.loss_X(org_x, im)
        ops.join_aside()
        return loss

    def loss_X(self, batch_x_org, interaction_map):
        """models.py:277-282: sum of squared differences (no mean)."""
        return torch.sum((interaction_map - batch_x_org) ** 2)


# ---------------------------------------------------------------------------
# Fine-tuning head (boundary §8(b))
# ---------------------------------------------------------------------------
class Mainmodel_finetuning(_Explainable, nn.Module):
    """models.py:358-543: a pretrained model's extract_features (frozen except
    the reference's freezing quirk) -> MLP -> Set2Set -> predict [-> sigmoid].

    Same constructor/forward signatures and state_dict keys as the reference.
    ``cp_filename`` is an in-memory pretrained module or a ``save_checkpoint``
    file (the reference unpickles a whole module, models.py:425; such files
    are not loaded here — INTEGRATION.md).  Kept quirks:
      * freezing (models.py:427-436): every parameter of the pretrained model
        is frozen, then the loop over ["layers.4", "layers.3", "layers.2"]
        re-assigns requires_grad for each entry, so only the LAST entry wins —
        exactly the names containing "layers.2" stay trainable;
      * the pretrained Mainmodel_continue's own (wrapper-level) encoders run
        in extract_features (models.py:1204-1252), and the compression noise
        is applied in eval mode too;
      * scores are sigmoid(predict(.)) unless the dataset is one of
        ZINC / Peptides-struct / FreeSolv / ESOL (models.py:517-520).
    Own Encoder1/Encoder2/compressor/embedding_h/reduce_d/attn_layer are
    created for state_dict parity only (unused by forward, as in the reference).
    """

    TASKS = ["ZINC", "Peptides-struct", "FreeSolv", "ESOL"]

    def __init__(self, args, in_dim, hidden_dim, num_layers, num_heads, k_transition,
                 num_classes, cp_filename, encoder):
        super().__init__()
        self.tau = 1.0
        self.dataset = getattr(args, "dataset", None)
        self.readout = args.readout_f
        self.s2s = Set2Set(hidden_dim, 2, 1)
        self.in_dim = args.d_transfer
        self.transfer_d = nn.Linear(in_dim, self.in_dim, bias=False)
        self.batch_size = getattr(args, "batch_size", 16)
        self.useAtt = args.useAtt
        self.embedding_h = nn.Linear(self.in_dim, hidden_dim, bias=False)
        self.hidden_dim = hidden_dim
        self.k_transition = k_transition
        self.reduce_d = nn.Linear(2 * hidden_dim, hidden_dim)
        self.attn_layer = nn.Linear(2 * hidden_dim, 1)
        self.num_nodes = -1
        self.device = getattr(args, "device", None)
        self.tasks = list(self.TASKS)
        task = getattr(args, "task", "graph_classification")
        if task not in ("graph_regression", "graph_classification"):
            raise ValueError(f"task {task!r}: the reference builds no predict head for it")
        out_dim = 1 if task == "graph_regression" else num_classes
        self.predict = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU(),
                                     nn.Linear(hidden_dim, out_dim))
        self.MLP = nn.Sequential(nn.Linear(2 * hidden_dim, hidden_dim), nn.ReLU(),
                                 nn.Linear(hidden_dim, hidden_dim))
        self.encoder_name, self.num_layers, self.num_heads = encoder, num_layers, num_heads
        self.Encoder1 = _make_encoder(encoder, self.in_dim, hidden_dim, args, num_layers, num_heads,
                                      True)
        self.Encoder2 = _make_encoder(encoder, self.in_dim, hidden_dim, args, num_layers, num_heads,
                                      True)
        self.model = load_checkpoint(cp_filename, args)
        freeze_like_reference(self.model)
        self.compressor = nn.Sequential(nn.Linear(hidden_dim, hidden_dim),
                                        nn.BatchNorm1d(hidden_dim), nn.ReLU(),
                                        nn.Linear(hidden_dim, 1))

    @ops.aside_guard
    def forward(self, batch_g, batch_x, flatten_batch_subgraphs, x_subs, current_epoch=None,
                edge_index=None, k_transition=None, device=None, batch_size=2, noise=None):
        self.batch_size = batch_size
        self.device = device
        batch_g = G.as_graph_batch(batch_g)
        if flatten_batch_subgraphs is not None:
            flatten_batch_subgraphs = G.as_graph_batch(flatten_batch_subgraphs)
        inner = self.model
        if flatten_batch_subgraphs is None and x_subs is None and batch_x.is_cuda and \
                isinstance(inner, _SCGIBCore):
            # ego-nets built on the device: this head's transfer_d folded into the
            # pretrained model's encoders, the ego branch forked (as the
            # pretraining step and Mainmodel_domainadapt run them) — the same
            # maths as transfer_d then extract_features (models.py:510-513)
            ego, enc = inner._encode_forked(inner, batch_g, batch_x, FORK_ENCODERS,
                                            noise is None, transfer=self.transfer_d)
            im = inner._extract(inner, batch_g, None, ego, None, noise, enc, readouts=False)[0]
            _drop_graph_refs(inner)
        else:
            if flatten_batch_subgraphs is None:  # ego-nets built on the device
                flatten_batch_subgraphs, x_subs = self._prepare_ego(batch_g, batch_x, x_subs)
            batch_x = self.transfer_d(batch_x)
            x_subs = self.transfer_d(x_subs)
            im = inner.extract_features(None, batch_g, batch_x, flatten_batch_subgraphs, x_subs,
                                        device, noise)[0]
        im = ops.mlp2(im, self.MLP, batch_g.dims)
        im = self.s2s(batch_g, im)
        sig = self.dataset not in self.tasks  # models.py:517-520
        if FUSE_HEAD and ops.predict_head_ok(im, self.predict):
            scores = ops.predict_head(im, self.predict, sig)  # predict (+ sigmoid), one launch
        else:
            scores = self.predict(im)
            scores = torch.sigmoid(scores) if sig else scores
        ops.join_aside()
        return scores, 0, 0, 0

    def _prepare_ego(self, batch_g, batch_x, x_subs):
        k = getattr(self.model, "k_transition", self.k_transition)
        ego = G.egonet_batch(batch_g, k)
        if x_subs is None:
            x_subs = batch_x.index_select(0, ego.ndata["_ID"])
        return ego, x_subs

    # losses (models.py:522-543)
    def loss(self, scores, targets):
        if FUSE_HEAD and scores.is_cuda and scores.shape == targets.shape:
            return ops.bce_mean(scores.float(), targets.float())  # one launch each way
        return F.binary_cross_entropy(scores.float(), targets.float())

    def loss_CrossEntropy(self, scores, targets, epoch=None):
        """models.py:527-530.  ``epoch``: a metrics.ClassEpoch that the device
        loss adds this batch to (the torch path has no such accumulator)."""
        if scores.is_cuda and targets.is_cuda and (
                targets.dtype == torch.float32 or
                (DEVICE_CE and targets.dtype in (torch.int32, torch.int64))):
            return ops.class_loss(scores, targets, epoch=epoch)  # one launch each way
        if epoch is not None:
            raise ops._lib.ScgibError("loss_CrossEntropy: epoch= needs the device loss (float32 HIP "
                                  "targets, or integer ones with models.DEVICE_CE)")
        return F.cross_entropy(scores.to(torch.float32), targets.squeeze(dim=-1))

    def loss_RMSE(self, scores, targets):
        if _task_loss_ok(scores, targets):
            return ops.task_loss(scores, targets, "rmse", ignore_nan=False)
        return torch.sqrt(F.mse_loss(scores, targets))

    def BCEWithLogitsLoss(self, scores, targets):
        if _task_loss_ok(scores, targets):
            return ops.task_loss(scores, targets, "bce_logits", ignore_nan=False)
        return F.binary_cross_entropy_with_logits(scores, targets)

    def lossMAE(self, scores, targets):
        if _task_loss_ok(scores, targets):
            return ops.task_loss(scores, targets, "mae", ignore_nan=False)
        return F.l1_loss(scores, targets)


def _task_loss_ok(scores, targets):
    """The device losses of csrc/task_head.hip take the place of the plain
    F.* call: FUSE_HEAD on, fp32 HIP tensors of one shape, not empty."""
    return (FUSE_HEAD and scores.is_cuda and targets.is_cuda and scores.shape == targets.shape
            and scores.dtype == targets.dtype == torch.float32 and scores.numel() > 0)


# The loss methods whose NaN-masked mean ("ignore-flatten") MetricWrapper runs
# as one ops.task_loss launch: the method's function carries the kernel's kind
# (a bound method forwards attribute reads to its function).
Mainmodel_finetuning.loss.task_loss_kind = "bce"
Mainmodel_finetuning.BCEWithLogitsLoss.task_loss_kind = "bce_logits"
Mainmodel_finetuning.lossMAE.task_loss_kind = "mae"
Mainmodel_finetuning.loss_RMSE.task_loss_kind = "rmse"


def freeze_like_reference(model, num_layers=4):
    """The reference's freezing loop (models.py:427-436), literally: for every
    parameter, requires_grad is re-assigned once per entry of
    unfrezz_layers, so the last entry ("layers.2") decides."""
    for p in model.parameters():
        p.requires_grad = False
    unfrezz_layers = ["layers." + str(num_layers), "layers." + str(num_layers - 1),
                      "layers." + str(num_layers - 2)]
    for name, para in model.named_parameters():
        for layer in unfrezz_layers:
            para.requires_grad = layer in name


# ---------------------------------------------------------------------------
# checkpoints: state_dict based.  The reference pickles whole modules
# (exp_pretraining.py:107); those files are read weights-only through inert
# stand-in classes (refckpt.py) and rebuilt from this package's classes.
# ---------------------------------------------------------------------------
_CKPT_ARGS = ("recons_type", "useAtt", "readout_f", "d_transfer", "gin_layers", "task",
              "batch_size")


def save_checkpoint(model, path, args=None, in_dim=None, num_classes=1):
    """state_dict checkpoint of a Mainmodel, Mainmodel_continue or
    Mainmodel_domainadapt (the nested wrapped models included), loadable with
    weights_only=True."""
    cfg = {}
    if args is not None:
        cfg = {k: getattr(args, k) for k in _CKPT_ARGS if hasattr(args, k)}
    cfg.update(kind=type(model).__name__, in_dim=in_dim, hidden_dim=model.hidden_dim,
               k_transition=model.k_transition, num_classes=num_classes)
    levels, encoders, m = [], [], model  # the wrapper chain (continue / DA around a Mainmodel)
    depths, heads = [], []
    while m is not None:
        levels.append([type(m).__name__, int(m.transfer_d.weight.shape[1])])
        encoders.append(str(getattr(m, "encoder_name", "GIN")))
        depths.append(int(getattr(m, "num_layers", 4)))
        heads.append(int(getattr(m, "num_heads", 4)))
        m = getattr(m, "model", None)
    cfg["levels"] = levels
    # the encoder of each level (files without the entry: GIN at every level)
    cfg["encoder"], cfg["encoders"] = encoders[0], encoders
    # ... and its constructor's num_layers / num_heads (a Transformer's depth
    # and head count; files without the entries: 4 and 4)
    cfg["num_layers"], cfg["num_heads"] = depths, heads
    torch.save({"config": cfg, "state_dict": model.state_dict()}, path)


def load_checkpoint(cp, args):
    """A Mainmodel / Mainmodel_continue / Mainmodel_domainadapt from an
    in-memory module, a save_checkpoint() file, or one of the reference's
    whole-module checkpoints (models.py:421, :1076; e.g. the shipped
    pre_training_v1_GIN_64_5_1.pt) — all weights only: nothing in a file is
    executed (refckpt.py)."""
    if isinstance(cp, nn.Module):
        return cp
    if isinstance(cp, (str, os.PathLike)) and refckpt.is_reference_module_checkpoint(cp):
        levels, cfg, sd = refckpt.read(cp)
        cfg = dict(cfg, task=getattr(args, "task", None))
    else:
        blob = torch.load(cp, map_location="cpu", weights_only=True)
        cfg, sd = blob["config"], blob["state_dict"]
        levels = cfg.get("levels")
        if levels is None:  # round-2 files: up to two wrapped levels, one F
            kinds = [cfg.get("kind"), cfg.get("inner_kind"), cfg.get("inner_inner_kind")]
            kinds = [k for k in kinds if k] + ([] if "Mainmodel" in kinds else ["Mainmodel"])
            levels = [[k, cfg["in_dim"]] for k in kinds]
    return model_from_state(levels, cfg, sd, args)


def model_from_state(levels, cfg, sd, args=None):
    """The wrapper chain ``levels`` = [(kind, F), ...] (outermost first) built
    from this package's classes with ``cfg``'s sizes, ``sd`` loaded strictly."""
    ns = type("Args", (), {})()
    for k in _CKPT_ARGS:
        setattr(ns, k, cfg.get(k, getattr(args, k, None)))
    if ns.task is None:
        ns.task = "graph_classification"
    with _loading():  # the file's own encoders, whatever ALL_ENCODER_STRINGS says
        m = _build_levels([(str(k), int(f)) for k, f in levels], ns, cfg)
    m.load_state_dict(sd)
    return m


def _build_levels(levels, ns, cfg, depth=0):
    """An untrained module for load_state_dict: levels = [(kind, F), ...] from
    the outermost wrapper down to the Mainmodel it wraps; each level's encoder
    from cfg["encoders"] (cfg["encoder"] for all, "GIN" in files without) and
    its num_layers / num_heads from cfg's lists (4 and 4 in files without)."""
    (kind, f_in), rest = levels[0], levels[1:]
    nl, nh = cfg.get("num_layers") or [], cfg.get("num_heads") or []
    dims = (f_in, cfg["hidden_dim"], int(nl[depth]) if depth < len(nl) else 4,
            int(nh[depth]) if depth < len(nh) else 4, cfg["k_transition"])
    encs = cfg.get("encoders") or []
    enc = str(encs[depth]) if depth < len(encs) else str(cfg.get("encoder", "GIN"))
    if kind == "Mainmodel":
        return Mainmodel(ns, *dims, enc)
    inner = _build_levels(rest or [("Mainmodel", f_in)], ns, cfg, depth + 1)
    if kind == "Mainmodel_continue":
        return Mainmodel_continue(ns, *dims, cfg.get("num_classes", 1), inner, enc)
    if kind == "Mainmodel_domainadapt":
        return Mainmodel_domainadapt(ns, *dims, cfg.get("num_classes", 1), inner, enc)
    raise NotImplementedError(f"checkpoint kind {kind!r}")
