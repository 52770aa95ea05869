"""Scoring and embedding with a trained model (csrc/infer.hip).

``Scorer(model)`` answers "what does the model say about these molecules":
``score`` (fine-tune models: the task scores) and ``embed`` (all four model
classes: the sum readouts ``z1`` / ``z2`` and, for a fine-tune model, the
pooled Set2Set vector).  In eval mode the whole model is a pure function of one
molecule, so the ``"resident"`` path runs it as ONE launch that keeps a
molecule in LDS from its raw features to its pooled vector
(``ops.infer_forward``); ``"layers"`` is the existing per-layer forward.
``score_dataset`` / ``embed_dataset`` walk a ``graph.DeviceEvalLoader`` with
one captured step per batch and no host read during the pass.
"""
from __future__ import annotations

import torch

from . import _lib
from . import graph as G
from . import models
from . import ops

PATHS = ("auto", "resident", "layers")
# What "auto" does with a batch the resident kernel supports (model and every
# molecule inside ops.infer_limits()): the path tools/infer_bench.py measured
# faster for the captured score step.  See DESIGN.md §29 for the figures.
AUTO_RESIDENT = False


class Embedding:
    """``z1`` / ``z2`` [B, 64]: the sum readouts of the noisy and of the plain
    graph features; ``pooled`` [B, 128]: the Set2Set vector the predict head
    reads (None for the pretraining classes)."""

    __slots__ = ("z1", "z2", "pooled")

    def __init__(self, z1, z2, pooled):
        self.z1, self.z2, self.pooled = z1, z2, pooled


class Scorer:
    """Eval-mode scoring / embedding of ``model`` (any of the four S-CGIB model
    classes), routed as ``model.explain`` is (models._explain_route): the
    encoder owner and the transfer_d that ``forward`` runs.

    ``path``: ``"resident"`` forces the one-launch kernel and raises where it
    is unsupported (model: two GIN encoders of hidden 64 over d_transfer 32,
    F <= 16, depth 1..8; batch: every molecule within
    ``ops.infer_limits()['max_nodes']`` atoms); ``"layers"`` is the existing
    forward; ``"auto"`` takes the kernel when model and batch are inside the
    limits — decided from host-known sizes only — and ``AUTO_RESIDENT`` says
    the kernel measured faster.  A resident call reads nothing back: a
    molecule that exceeds a limit on the device (capacity mode) gets NaN rows
    and sets a sticky word that eager callers check with ``ops.infer_error``.
    The parameter table is built once: call
    ``refresh()`` after replacing a parameter tensor (in-place updates, e.g.
    an optimizer's, need nothing)."""

    def __init__(self, model, path="auto"):
        if path not in PATHS:
            raise ValueError(f"Scorer: path {path!r}; one of {', '.join(PATHS)}")
        self.model, self.path = model, path
        self.owner, self.transfer, self.k = models._explain_route(model)
        self.finetune = isinstance(model, models.Mainmodel_finetuning)
        if not isinstance(self.owner, models._SCGIBCore):
            raise TypeError(f"Scorer: the wrapped model is a {type(self.owner).__name__}")
        self.unsupported = ops.infer_unsupported(self.owner.Encoder1, self.owner.Encoder2,
                                                 self.transfer, self.owner.compressor)
        if path == "resident" and self.unsupported is not None:
            raise _lib.ScgibError(f"Scorer(path='resident'): {self.unsupported}")
        self._table = None

    def refresh(self):
        self._table = None

    # ----- routing (host logic only) ---------------------------------------
    def _check(self, batch_x):
        if self.model.training or self.owner.training:
            raise RuntimeError("Scorer needs model.eval(): a train-mode forward would move the "
                               "BatchNorm running statistics")
        if not batch_x.is_cuda:
            raise _lib.ScgibError(f"Scorer: features on {batch_x.device}; the S-CGIB ops run on "
                                  "the HIP device only (no CPU fallback)")

    def route(self, batch_g, batch_x=None):
        """The path ("resident" / "layers") a call with this batch takes; a
        forced ``"resident"`` raises where the batch is above a limit."""
        if self.path == "layers":
            return "layers"
        g = G.as_graph_batch(batch_g)
        lim = ops.infer_limits()
        why = self.unsupported
        if why is None and g.max_graph_nodes > lim["max_nodes"]:
            why = (f"a molecule of up to {g.max_graph_nodes} atoms (the resident kernel holds "
                   f"{lim['max_nodes']})")
        if why is None and batch_x is not None and batch_x.shape[1] != self.transfer.in_features:
            why = f"{batch_x.shape[1]} feature columns for a transfer_d of {self.transfer.in_features}"
        if self.path == "resident":
            if why is not None:
                raise _lib.ScgibError(f"Scorer(path='resident'): {why}")
            return "resident"
        return "resident" if why is None and AUTO_RESIDENT else "layers"

    def _tab(self):
        t = self._table
        if t is None or t.params.transfer != self.transfer.weight.data_ptr():
            m = self.model
            t = self._table = ops.InferTable(
                self.owner.Encoder1, self.owner.Encoder2, self.transfer, self.owner.compressor,
                self.owner.attn_layer, bool(self.owner.useAtt),
                m.MLP if self.finetune else None, m.s2s if self.finetune else None)
        return t

    @staticmethod
    def _join_fork(device):
        """A layer-path forward without a backward leaves the ego chain's
        stream unjoined (the backward would join it): a capture has to close
        it."""
        if models.FORK_ENCODERS:
            torch.cuda.current_stream(device).wait_stream(models._side_stream(device))

    # ----- the two forwards --------------------------------------------------
    def _resident(self, g, x, noise, rows=False):
        ego = G.egonet_batch(g, self.k)
        if noise is None:
            u_gate, u_feat = ops.device_noise(g.num_nodes(), x.device)
        else:
            u_gate, u_feat = noise
        return ops.infer_forward(x, g, ego, self._tab(), u_gate, u_feat, rows=rows)

    def rows(self, batch_g, batch_x, noise=None):
        """(lam [N], logit [N] or None, im [N, 128]) of the resident kernel: the
        per-atom gate, attention logit and interaction-map rows it computes on
        the way (tests, explain-style readers)."""
        self._check(batch_x)
        g = G.as_graph_batch(batch_g)
        if self.unsupported is not None:
            raise _lib.ScgibError(f"Scorer.rows: {self.unsupported}")
        return self._resident(g, batch_x, noise, rows=True)[3:]

    def score(self, batch_g, batch_x, noise=None):
        """scores [B, T] of a fine-tune model: ego build, noise draw, one
        scgib_infer_fwd, the predict head (with the sigmoid unless the dataset
        is a regression one, as ``Mainmodel_finetuning.forward``).  ``noise`` =
        (u_gate [N], u_feat [N, 64]) as in ``forward``; None draws through
        ops.device_noise — the same launch and the same amount of Philox state
        as the existing eval forward, so equal seeds give both paths the same
        draws."""
        if not self.finetune:
            raise TypeError(f"Scorer.score: {type(self.model).__name__} has no predict head "
                            "(scores come from a Mainmodel_finetuning; use embed)")
        self._check(batch_x)
        g = G.as_graph_batch(batch_g)
        m = self.model
        with torch.no_grad():
            if self.route(g, batch_x) == "layers":
                scores = m(g, batch_x, None, None, noise=noise)[0]
                self._join_fork(batch_x.device)
                return scores
            pooled = self._resident(g, batch_x, noise)[0]
            sig = m.dataset not in m.tasks  # models.py:517-520
            if models.FUSE_HEAD and ops.predict_head_ok(pooled, m.predict):
                return ops.predict_head(pooled, m.predict, sig)
            scores = m.predict(pooled)
            return torch.sigmoid(scores) if sig else scores

    def embed(self, batch_g, batch_x, noise=None):
        """An ``Embedding`` of the batch (``pooled`` None for the pretraining
        classes)."""
        self._check(batch_x)
        g = G.as_graph_batch(batch_g)
        with torch.no_grad():
            if self.route(g, batch_x) == "resident":
                pooled, z1, z2 = self._resident(g, batch_x, noise)[:3]
                return Embedding(z1, z2, pooled)
            return self._embed_layers(g, batch_x, noise)

    @ops.aside_guard
    def _embed_layers(self, g, x, noise):
        """The layer path of ``embed``: the steps of
        ``Mainmodel_finetuning.forward`` up to the Set2Set vector (the same
        calls in the same order, under the same guards), with the sum readouts
        the interaction launch already returns kept instead of dropped."""
        owner, m = self.owner, self.model
        ego, enc = owner._encode_forked(owner, g, x, models.FORK_ENCODERS, noise is None,
                                        transfer=self.transfer)
        im, _, _, z2, z1 = owner._extract(owner, g, None, ego, None, noise, enc, readouts=False)
        models._drop_graph_refs(owner)
        pooled = None
        if self.finetune:
            pooled = m.s2s(g, ops.mlp2(im, m.MLP, g.dims))
        ops.join_aside()
        self._join_fork(x.device)
        return Embedding(z1, z2, pooled)


class DatasetEmbedding:
    """Per-molecule arrays over a whole DeviceDataset, row = molecule id:
    ``z1`` / ``z2`` [M, 64], ``pooled`` [M, 128] or None; NaN where no pass
    wrote."""

    def __init__(self, dataset, pooled=True):
        def f32(w):
            return torch.full((len(dataset), w), float("nan"), dtype=torch.float32,
                              device=dataset.device)

        self.z1, self.z2 = f32(64), f32(64)
        self.pooled = f32(128) if pooled else None


def _dataset_pass(model, evl, body_of, path, passes):
    """One captured step — load_next, collate_ahead, the score / embed step,
    the row write by ``ids`` — replayed ``steps`` times per pass over ``evl``
    (built like explain.explain_dataset); nothing is read back during it."""
    if model.training:
        raise RuntimeError("score_dataset / embed_dataset need model.eval()")
    static = evl.static
    dev = static.blob.device
    if dev.type != "cuda":
        raise _lib.ScgibError("score_dataset / embed_dataset need a HIP device (no CPU fallback)")
    scorer = Scorer(model, path)
    step = body_of(scorer)
    # the kernel's error word is sticky and process-wide: this pass answers for
    # its own molecules only (an earlier flag is put back afterwards)
    earlier = ops.infer_error(dev, reset=True)

    def body():
        static.load_next(evl.pool)
        evl.collate_ahead()
        step()

    evl.prime()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # warm-up (allocator, lazy workspaces): batch 0, stored once
        body()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    evl.prime()
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for _ in range(int(passes) * evl.steps):
        graph.replay()
    torch.cuda.synchronize(dev)
    if evl.error():
        raise _lib.ScgibError("score_dataset / embed_dataset: a batch did not fit the static "
                              "batch's capacities")
    mine = ops.infer_error(dev)
    if earlier:
        ops.infer_error_word(dev).fill_(1)
    if mine:
        raise _lib.ScgibError("score_dataset / embed_dataset: a molecule exceeded a limit of the "
                              "resident kernel on the device (its rows are NaN)")


def score_dataset(model, eval_loader, out=None, *, noise=None, path="auto", passes=1):
    """scores [M, T] (row = molecule id of ``eval_loader.dataset``; NaN where
    the loader's subset holds no molecule) of a fine-tune model in eval mode.
    ``noise`` = (u_gate [n_cap], u_feat [n_cap, 64]): the draw of every batch
    (None: a fresh device draw per batch).  The loader's fill rows (``ids``
    -1) write nothing.  Returns ``out`` (a new tensor unless one is given)."""
    ds = eval_loader.dataset
    if out is None:
        t = int(model.predict[2].out_features)
        out = torch.full((len(ds), t), float("nan"), dtype=torch.float32, device=ds.device)
    static = eval_loader.static

    def body_of(scorer):
        return lambda: ops.infer_store(scorer.score(static.graph, static.x, noise),
                                       eval_loader.ids, out)

    _dataset_pass(model, eval_loader, body_of, path, passes)
    return out


def embed_dataset(model, eval_loader, out=None, *, noise=None, path="auto", passes=1):
    """A ``DatasetEmbedding`` of the loader's subset (see ``score_dataset``)."""
    if out is None:
        out = DatasetEmbedding(eval_loader.dataset, isinstance(model, models.Mainmodel_finetuning))
    static = eval_loader.static

    def body_of(scorer):
        def step():
            e = scorer.embed(static.graph, static.x, noise)
            ops.infer_store(e.z1, eval_loader.ids, out.z1)
            ops.infer_store(e.z2, eval_loader.ids, out.z2)
            if e.pooled is not None:
                ops.infer_store(e.pooled, eval_loader.ids, out.pooled)
        return step

    _dataset_pass(model, eval_loader, body_of, path, passes)
    return out
