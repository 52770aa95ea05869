"""References for the graph-core / significant-subgraph tests.

Host side only; reads nothing but the arrays it is given.  Two parts:

* numpy: ranks (``np.lexsort``), centres / weights, the core rule
  (``max(1, ceil(n_i * ratio))`` in float64) and the induced core through
  ``oracle.dgl_semantics.node_subgraph``;
* fp64: ``lam`` and ``alpha`` restated from ``oracle.scgib_ref``'s building
  blocks (``compression`` for p, ``_linear`` for the attention logit), and the
  two derivations that read them back out of a recorded reference forward
  (``act_noisy`` / ``act_interaction_map`` of the train-mode goldens).
"""
import numpy as np
import torch

from oracle import dgl_semantics as D
from oracle import scgib_ref as R


# ---------------------------------------------------------------------------
# order, ranks, centres, core rule
# ---------------------------------------------------------------------------
def gptr_of(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])


def ranks(keys, gptr):
    """rank_v inside each molecule: descending key, ties by ascending id; keys
    compare as floats (-0.0 == +0.0); NaN after every number, NaNs by id."""
    keys = np.asarray(keys, np.float32)
    out = np.full(len(keys), -1, np.int32)
    for a, b in zip(gptr[:-1], gptr[1:]):
        k = keys[a:b]
        nan = np.isnan(k)
        neg = np.where(nan, np.float32(0), -k)  # ascending -k == descending k; NaNs tie
        order = np.lexsort((np.arange(b - a), neg, nan))  # last key is the primary one
        out[a:b][order] = np.arange(b - a, dtype=np.int32)
    return out


def centres(alpha, alpha_rank, gptr, top_m):
    B = len(gptr) - 1
    c = np.full((B, top_m), -1, np.int32)
    w = np.zeros((B, top_m), np.float32)
    for g, (a, b) in enumerate(zip(gptr[:-1], gptr[1:])):
        for v in range(a, b):
            r = alpha_rank[v]
            if r < top_m:
                c[g, r] = v
                w[g, r] = alpha[v]
    return c, w


def core_sizes(gptr, ratio):
    n = np.diff(gptr).astype(np.float64)
    return np.maximum(1.0, np.ceil(n * np.float64(ratio)))


def core_keep(lam, lam_rank, gptr, ratio=None, threshold=None):
    assert (ratio is None) != (threshold is None)
    if threshold is not None:
        return np.asarray(lam, np.float32) >= np.float32(threshold)  # NaN: False
    m = np.repeat(core_sizes(gptr, ratio), np.diff(gptr))
    return np.asarray(lam_rank, np.float64) < m


def core_reference(src, dst, gptr, keep):
    """(rowptr, col, graph_ptr, ids) of the core: dgl.node_subgraph of every
    molecule on its kept atoms (ascending ids), re-batched.  Rows are ``src``,
    columns ``dst`` in the oracle's out-CSR order."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    rowptr, col, gp, ids = [0], [], [0], []
    for a, b in zip(gptr[:-1], gptr[1:]):
        m = (src >= a) & (src < b)
        g = D.graph((src[m] - a, dst[m] - a), num_nodes=int(b - a))
        nodes = np.flatnonzero(keep[a:b])
        sg = D.node_subgraph(g, nodes)
        s, d = sg.src.numpy(), sg.dst.numpy()
        base = gp[-1]
        deg = np.bincount(s, minlength=len(nodes))
        for dg in deg:
            rowptr.append(rowptr[-1] + int(dg))
        col += (d + base).tolist()  # (s is row-major: node_subgraph visits rows in order)
        ids += (sg.ndata["_ID"].numpy() + a).tolist()
        gp.append(base + len(nodes))
    return (np.asarray(rowptr, np.int32), np.asarray(col, np.int32), np.asarray(gp, np.int32),
            np.asarray(ids, np.int32))


def softmax_ref(logit, gptr):
    """fp64 softmax per molecule."""
    logit = np.asarray(logit, np.float64)
    out = np.zeros_like(logit)
    for a, b in zip(gptr[:-1], gptr[1:]):
        if b > a:
            e = np.exp(logit[a:b] - logit[a:b].max())
            out[a:b] = e / e.sum()
    return out


# ---------------------------------------------------------------------------
# fp64 restatement of lam and alpha
# ---------------------------------------------------------------------------
def _double(params):
    return {k: (torch.as_tensor(v).double() if torch.as_tensor(v).is_floating_point()
                else torch.as_tensor(v).clone()) for k, v in params.items()}


def gate_eps(u_gate):
    """eps = 0.9999 - 0.9998 u as the reference forms it: in fp32
    (models.py:598-599).  1 - eps reaches 1e-4, where the fp32 rounding of eps
    itself is a 6e-4 relative change of 1 - eps, so the fp32 eps — not u — is
    the input the gate is defined on; everything after it is fp64 here."""
    u = torch.as_tensor(u_gate, dtype=torch.float32).reshape(-1)
    bias = 0.0 + 0.0001
    return ((bias - (1 - bias)) * u + (1 - bias)).double()


def lam_alpha_fp64(params, graph_features, sub_readout, counts, u_gate, training, use_att=True):
    """(lam, alpha, p) in fp64 from Mainmodel-keyed ``params`` (floats of any
    precision; buffers included): p by scgib_ref.compression (per-molecule
    BatchNorm in train mode, running statistics in eval mode), lam =
    sigmoid(log eps - log(1 - eps) + p), alpha = per-molecule softmax of
    attn_layer(cat(z-bar, s)) (z-bar constant per molecule: it cancels)."""
    p = _double(params)
    counts = torch.as_tensor(np.asarray(counts, np.int64))
    gf = torch.as_tensor(graph_features).double()
    n = gf.shape[0]
    bufs = {k: v.clone() for k, v in p.items() if "running" in k or "num_batches" in k}
    if training and "compressor.1.running_mean" not in bufs:
        bufs = None
    with torch.no_grad():
        noisy, pv, _ = R.compression(p, gf, counts, torch.zeros(n, dtype=torch.float64),
                                     torch.zeros(n, 64, dtype=torch.float64), bufs, training)
        eps = gate_eps(u_gate)
        lam = torch.sigmoid(torch.log(eps) - torch.log(1 - eps) + pv.reshape(-1))
        alpha = None
        if use_att:
            s = torch.as_tensor(sub_readout).double()
            zbar = R.sum_nodes(noisy, counts)
            seg = torch.repeat_interleave(torch.arange(len(counts)), counts)
            logit = R._linear(torch.cat((zbar[seg], s), -1), p, "attn_layer").reshape(-1)
            alpha = torch.as_tensor(softmax_ref(logit.numpy(), gptr_of(counts.numpy())))
    return lam.numpy(), None if alpha is None else alpha.numpy(), pv.reshape(-1).numpy()


def ego_sums(sub_features, ego_counts):
    """Per-ego sums of the ego batch's features (the sub-graph readout), fp64."""
    return R.sum_nodes(torch.as_tensor(sub_features).double(),
                       torch.as_tensor(np.asarray(ego_counts, np.int64))).numpy()


# ---------------------------------------------------------------------------
# lam and alpha read back out of a recorded reference forward
# ---------------------------------------------------------------------------
def alpha_from_map(interaction_map, sub_features, ego_counts):
    """alpha_v = interaction_map[v, 64 + c] / S[v, c] at the channel c of
    largest |S[v, c]|, S = the per-ego sums (models.py:747: a = s * alpha)."""
    S = ego_sums(sub_features, ego_counts)
    att = np.asarray(interaction_map, np.float64)[:, 64:]
    c = np.abs(S).argmax(axis=1)
    r = np.arange(len(S))
    return att[r, c] / S[r, c]


def lam_from_noisy(noisy, graph_features, u_feat, counts):
    """(lam, usable): solves noisy = lam f + (1 - lam)(mu + u sigma) at each
    row's channel of largest |f - mu - u sigma| (models.py:647-651; mu / sigma
    the molecule's mean and unbiased std).  Rows of 2-atom molecules are not
    usable: their two feature rows coincide after the GIN's BatchNorm, so
    sigma = 0 and f = mu."""
    f = np.asarray(graph_features, np.float64)
    z = np.asarray(noisy, np.float64)
    u = np.asarray(u_feat, np.float64)
    gptr = gptr_of(counts)
    lam = np.zeros(len(f))
    usable = np.repeat(np.diff(gptr) > 2, np.diff(gptr))
    for a, b in zip(gptr[:-1], gptr[1:]):
        mu = f[a:b].mean(axis=0)
        sig = f[a:b].std(axis=0, ddof=1) if b - a > 1 else np.zeros(f.shape[1])
        base = mu + u[a:b] * sig
        den = f[a:b] - base
        c = np.abs(den).argmax(axis=1)
        r = np.arange(b - a)
        with np.errstate(divide="ignore", invalid="ignore"):
            lam[a:b] = (z[a:b][r, c] - base[r, c]) / den[r, c]
    return lam, usable
