"""Cost of the explain launches beside the eval forward they follow
(profiles/explain_baseline/).

QM9-like batch of 512 molecules in capacity mode on one GPU.  Every figure is
the median over ``--windows`` windows of ``--replays`` replays of a captured
HIP graph, timed by device events after a warm-up window:

  forward ........ eval-mode ``extract_features`` (ego-nets built on the
                   device, both encoders, readout, interaction); ``--root``
                   points at the tree whose package is measured, so the same
                   script times the parent commit
  explain ........ rank + core (mask, count / fix-up, fill) + store, and each
                   of the three alone
  rank by size ... the rank launch on 512 molecules of n atoms each

Usage:  python tools/explain_bench.py [--root DIR] [--mode forward|explain|all]
                                      [--out FILE]
Prints one JSON line per figure (and appends them to --out).
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(body, replays, windows, rewind=None):
    """Median microseconds per replay of ``body`` captured into a HIP graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    per = []
    for w in range(windows + 1):  # window 0: warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        if w:
            per.append(a.elapsed_time(b) * 1e3 / replays)
    return float(np.median(per)), float(min(per)), float(max(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--mode", default="all", choices=("forward", "explain", "all"))
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="head")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    pkg = importlib.import_module("s-cgib_amd")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(**rec):
        rec = dict(tag=a.tag, B=512, replays=a.replays, windows=a.windows, **rec)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    mols = pkg.synth.molecules(512, "qm9", seed=0)
    mols = [(ei, F.normalize(torch.from_numpy(np.asarray(x, np.float32))).numpy())
            for ei, x in mols]
    gh, _ = pkg.graph.collate_pyg(mols)
    caps = pkg.graph.StaticBatch.capacities([gh], 1, slack=1.1)
    static = pkg.graph.StaticBatch(512, caps[0], caps[1], gh.ndata["x"].shape[1], caps[2], caps[3],
                                   dev, 1)
    static.load(static.pad(gh))
    g, x = static.graph, static.x
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=512, gin_layers=5, task="graph_classification", device=dev)
    torch.manual_seed(0)
    inner = pkg.models.Mainmodel(args, x.shape[1], 64, 4, 4, 1, "GIN")
    model = pkg.models.Mainmodel_continue(args, x.shape[1], 64, 4, 4, 1, 1, inner, "GIN")
    model = model.to(dev).eval()
    pkg.ops.seed_noise(dev, 1)
    shape = dict(rows=gh.num_nodes(), edges=gh.num_edges(), row_cap=g.num_nodes())

    if a.mode in ("forward", "all"):
        def forward():
            with torch.no_grad():
                model.model.extract_features(None, g, model.transfer_d(x), None, None, dev)
        med, lo, hi = timed(forward, a.replays, a.windows)
        emit(what="eval extract_features forward", us=med, us_min=lo, us_max=hi, **shape)

    if a.mode in ("explain", "all"):
        ex = model.explain(g, x, top_m=3)
        lam, logit = ex.lam, torch.log(ex.alpha.clamp_min(1e-30))
        ids = torch.arange(512, dtype=torch.int32, device=dev)
        node_off = g.graph_ptr.to(torch.int64)
        n_cap = g.num_nodes()
        out = (torch.zeros(n_cap, device=dev), torch.zeros(n_cap, device=dev),
               torch.zeros(n_cap, dtype=torch.int32, device=dev),
               torch.zeros(n_cap, dtype=torch.int32, device=dev))
        ranked = pkg.ops.explain_rank(lam, logit, g, 3)

        def rank():
            return pkg.ops.explain_rank(lam, logit, g, 3)

        def core():
            pkg.ops.core_subgraph(lam, ranked[1], g, ratio=0.5)

        def store():
            pkg.ops.explain_store(lam, ranked[0], ranked[1], ranked[2], g, ids, node_off, out)

        def everything():
            al, lr, ar, _, _ = rank()
            pkg.ops.core_subgraph(lam, lr, g, ratio=0.5)
            pkg.ops.explain_store(lam, al, lr, ar, g, ids, node_off, out)

        for what, body in (("explain: rank + core + store", everything), ("explain: rank", rank),
                           ("explain: core (mask, count, fix-up, fill)", core),
                           ("explain: store", store)):
            med, lo, hi = timed(body, a.replays, a.windows)
            emit(what=what, us=med, us_min=lo, us_max=hi, **shape)
        e = np.zeros(0, np.int64)
        for n in (16, 64, 128, 256, 512, 600):
            gg = pkg.graph.GraphBatch.from_edges(e, e, 512 * n, True,
                                                 np.full(512, n, np.int64)).to(dev)
            kl = torch.randn(512 * n, device=dev)
            kg = torch.randn(512 * n, device=dev)
            med, lo, hi = timed(lambda: pkg.ops.explain_rank(kl, kg, gg, 3), a.replays, a.windows)
            emit(what="explain: rank, 512 molecules of n atoms", n=n, us=med, us_min=lo, us_max=hi)

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
