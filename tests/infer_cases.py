"""Shared by test_infer_cpu.py and test_gpu_infer.py (csrc/infer.hip,
DESIGN.md §29): hand-built molecules at the resident kernel's edges, model
builders for the four classes, and the fp64 oracle's inputs of a batch."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

F_IN = 9


def args_of(**over):
    base = dict(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32, batch_size=8,
                gin_layers=5, task="graph_classification", dataset="ogbg-molhiv")
    base.update(over)
    return SimpleNamespace(**base)


# ----- molecules: (n, bonds [(a, b)], x [n, F]) ------------------------------
def feats(rng, n, f=F_IN):
    x = rng.random((n, f), dtype=np.float32) + 0.05
    return F.normalize(torch.from_numpy(x)).numpy()


def path(rng, n, f=F_IN):
    return n, [(i, i + 1) for i in range(n - 1)], feats(rng, n, f)


def star(rng, leaves, f=F_IN):
    """Atom 0 bonded to ``leaves`` others: k = 1 ego-nets of leaves + 1 rows
    (the centre) and 2 rows; every k = 2 ego-net is the whole molecule."""
    return leaves + 1, [(0, i) for i in range(1, leaves + 1)], feats(rng, leaves + 1, f)


def with_loose_atom(rng, n, f=F_IN):
    """A path over atoms 0 .. n - 2 except atom 1, which has no bond: a
    one-row ego-net inside a molecule."""
    keep = [i for i in range(n) if i != 1]
    return n, list(zip(keep[:-1], keep[1:])), feats(rng, n, f)


def single_atom(rng, f=F_IN):
    return 1, [], feats(rng, 1, f)


def path_with_k1_ego_rows(rng, total, f=F_IN):
    """A molecule whose k = 1 ego rows total exactly ``total`` (>= 14): the
    total is sum(deg + 1) = m + 2 E, so a path of m atoms has 3 m - 2, one
    ring closure 3 m, two closures 3 m + 2."""
    extra = {1: 0, 0: 1, 2: 2}[total % 3]
    m = (total + 2 - 2 * extra) // 3
    bonds = [(i, i + 1) for i in range(m - 1)] + [(0, 2), (1, 3)][:extra]
    assert k1_ego_rows(m, bonds) == total, (total, m)
    return m, bonds, feats(rng, m, f)


def k1_ego_rows(n, bonds):
    deg = np.zeros(n, np.int64)
    for a, b in bonds:
        deg[a] += 1
        deg[b] += 1
    return int((deg + 1).sum())


def random_mols(pkg, num, workload, seed):
    """synth.molecules as (n, bonds, normalised x)."""
    out = []
    for ei, x in pkg.synth.molecules(num, workload, seed=seed):
        bonds = sorted({(int(min(a, b)), int(max(a, b))) for a, b in ei.T})
        out.append((len(x), bonds, F.normalize(torch.from_numpy(np.asarray(x, np.float32))).numpy()))
    return out


def batch_of(pkg, mols):
    """Host GraphBatch of hand-built molecules (one-atom molecules and atoms
    without a bond included, which collate_pyg's inferred node count cannot
    express); ``ndata['x']`` = the given rows."""
    src, dst, xs, counts, off = [], [], [], [], 0
    for n, bonds, x in mols:
        assert x.shape[0] == n
        for a, b in bonds:
            assert 0 <= a < n and 0 <= b < n and a != b
            src.append(a + off)
            dst.append(b + off)
        xs.append(x)
        counts.append(n)
        off += n
    counts = np.asarray(counts, np.int64)
    s, d = pkg.graph.bidirected_simple(np.asarray(src, np.int64), np.asarray(dst, np.int64),
                                       max(off, 1))
    gptr = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=gptr[1:])
    e_counts = np.diff(np.searchsorted(s, gptr))
    g = pkg.graph.GraphBatch.from_edges(s, d, off, symmetric_hint=True, batch_num_nodes=counts,
                                        batch_num_edges=e_counts)
    g.ndata["x"] = torch.from_numpy(np.concatenate(xs).astype(np.float32))
    return g


def oracle_inputs(gh, k):
    """(batch, ego, x, x_subs) dicts / fp64 tensors of host batch ``gh`` for
    oracle.scgib_ref (ego-nets from oracle/egonet_ref.c)."""
    from oracle import egonet
    sizes, ecount, nodes, esrc, edst = egonet.egonets(gh.rowptr.numpy(), gh.col.numpy(), k)
    off = np.repeat(np.concatenate([[0], np.cumsum(sizes)[:-1]]), ecount)
    src, dst = gh.edges()
    batch = {"src": src, "dst": dst, "counts": torch.from_numpy(gh.batch_num_nodes_host())}
    ego = {"src": torch.from_numpy(esrc + off), "dst": torch.from_numpy(edst + off),
           "counts": torch.from_numpy(sizes)}
    x = gh.ndata["x"].double()
    return batch, ego, x, x[torch.from_numpy(nodes)]


# ----- models ---------------------------------------------------------------
def shake_norms(model, seed):
    """Non-trivial BatchNorm affines and running statistics."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.weight.add_(0.2 * torch.randn(m.weight.shape, generator=gen))
                m.bias.add_(0.1 * torch.randn(m.bias.shape, generator=gen))
                m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(m.running_var.shape, generator=gen))


def pretrain_model(pkg, k=1, layers=5, seed=5, encoder="GIN", hidden=64, wrapped=True, **over):
    a = args_of(gin_layers=layers, **over)
    torch.manual_seed(seed)
    inner = pkg.models.Mainmodel(a, F_IN, hidden, 4, 4, k, encoder)
    if not wrapped:
        shake_norms(inner, seed)
        return inner
    model = pkg.models.Mainmodel_continue(a, F_IN, hidden, 4, 4, k, 1, inner, encoder)
    shake_norms(model, seed)
    return model


def finetune_model(pkg, k=1, layers=5, seed=5, num_classes=1, **over):
    """Mainmodel_finetuning around a Mainmodel_continue around a Mainmodel."""
    a = args_of(gin_layers=layers, **over)
    pre = pretrain_model(pkg, k, layers, seed, **over)
    torch.manual_seed(seed + 1)
    return pkg.models.Mainmodel_finetuning(a, F_IN, 64, 4, 4, k, num_classes, pre, "GIN")


def oracle_state(model):
    """(params, buffers) in fp64 of ``model``'s state_dict for oracle.scgib_ref."""
    p = {}
    for kk, v in model.state_dict().items():
        t = v.detach().cpu().clone()
        p[kk] = t.double() if t.is_floating_point() else t
    return p, {kk: v for kk, v in p.items() if "running" in kk or "num_batches" in kk}


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))
