"""Wall time of one evaluation pass over a subset of a resident dataset: the
captured fine-tune eval step (load_next, forward under no_grad,
EvalBuffer.append) replayed ceil(M / B) times plus the metric's one read, fed by

  loader  graph.DeviceEvalLoader (collate_ahead inside the captured step);
  pool    a fixed StaticBatch.pool of the same batches, padded on the host
          outside the timed region (the control; each step's labels are copied
          device to device into the tensor the captured append reads);
  host    what there was before the loader for a subset: per batch collate_pyg +
          StaticBatch.pad + load and a label upload, then the replay (the
          ego-nets are built inside the step: there is no pool to prefetch from).

molhiv-like molecules from synth, a tenth of the dataset as the subset, binary
labels with NaNs, GIN-64x5 in eval().  The variants live in one process and
alternate; a pass is timed with a host clock from the first replay to the
metric's read (which synchronises).  No bar: nothing here was measured before.

  python tools/eval_loader_bench.py --out profiles/evalloader_baseline/eval_loader_bench.jsonl
"""
import argparse
import importlib
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("s-cgib_amd")
G, ops = pkg.graph, pkg.ops


def stats(v, unit="ms"):
    a = np.sort(np.asarray(v, np.float64))
    return {f"median_{unit}": float(np.median(a)), f"min_{unit}": float(a[0]),
            f"max_{unit}": float(a[-1]), "samples": int(len(a))}


def make_model(f_in, k, B, dev):
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=B, gin_layers=5, task="graph_classification",
                           dataset="ogbg-molhiv", device=dev)
    torch.manual_seed(0)
    inner = pkg.models.Mainmodel(args, f_in, 64, 4, 4, k, "GIN")
    pre = pkg.models.Mainmodel_continue(args, f_in, 64, 4, 4, k, 1, inner, "GIN")
    return pkg.models.Mainmodel_finetuning(args, f_in, 64, 4, 4, k, 1, pre, "GIN").to(dev).eval()


def build(feed, ds, caps, mols, y, idx, model, B, k, dev):
    """One variant: its own static batch, pool, buffer and captured step;
    ``one_pass()`` enqueues a whole pass and reads the metric."""
    static = G.StaticBatch(B, caps[0], caps[1], ds.num_features, caps[2], caps[3], dev, k)
    rows, marked = G.sequential_ids(ds, idx, B)
    steps = len(rows)
    buf = pkg.metrics.EvalBuffer(steps * B, 1, dev)
    evl = pool = pf = labs = None
    keep = []
    if feed == "loader":
        evl = G.DeviceEvalLoader(ds, static, indices=idx)
        evl.prime()
        pool, lab = evl.pool, evl.labels
    else:
        lab = torch.zeros(B, 1, device=dev)
        host_labels = np.stack([np.where((m >= 0)[:, None], y[np.maximum(m, 0)], np.nan)
                                for m in marked]).astype(np.float32)
        if feed == "pool":
            keep = [static.pad(G.collate_pyg([mols[i] for i in r])[0]) for r in rows]
            pool = static.pool(keep)
            labs = torch.from_numpy(host_labels).to(dev)
    if pool is not None:
        pf = G.EgoPrefetch(static, pool)
        pf.prime()

    def body():
        if pool is not None:
            static.load_next(pool, pf)
        if evl is not None:
            evl.collate_ahead()
        with torch.no_grad():
            scores, *_ = model(static.graph, static.x, None, None, 1, None, k, dev, B)
        buf.append(scores, lab)
        if pf is not None:
            pf.join()
        else:
            # a forward without backward and without a prefetch leaves the ego
            # chain's stream unjoined (the backward would join it): a capture
            # has to close it
            torch.cuda.current_stream().wait_stream(pkg.models._side_stream(dev))

    def host_batch(t):  # the path without the loader, inside the timed region
        static.load(static.pad(G.collate_pyg([mols[i] for i in rows[t]])[0]))
        lab.copy_(torch.from_numpy(host_labels[t]), non_blocking=True)

    if feed == "host":
        host_batch(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if evl is not None:
        evl.prime()
    if pool is not None:
        pool["cursor"].zero_()
        pf.prime()
    buf.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()

    def one_pass():
        for t in range(steps):
            if feed == "pool":
                lab.copy_(labs[t], non_blocking=True)
            elif feed == "host":
                host_batch(t)
            graph.replay()
        auc = buf.rocauc()["rocauc"]  # the pass's one read
        rows_seen = buf.rows()
        buf.reset()
        return auc, rows_seen

    return SimpleNamespace(one_pass=one_pass, steps=steps, static=static, evl=evl, pf=pf,
                           keep=(keep, labs, graph, buf, pool))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="32,512")
    ap.add_argument("--molecules", type=int, default=41127)
    ap.add_argument("--subset", type=int, default=4113)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warm-passes", type=int, default=2)
    ap.add_argument("--only", default="loader,pool,host")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_loader_bench: needs the HIP device (nothing is measured on a CPU)")
    dev = torch.device("cuda", 0)
    fh = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fh = open(a.out, "w")

    def out(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    t0 = time.perf_counter()
    mols = [(ei, F.normalize(torch.from_numpy(x)).numpy())
            for ei, x in pkg.synth.molecules(a.molecules, "molhiv", seed=0)]
    rng = np.random.default_rng(0)
    y = (rng.random((len(mols), 1)) < 0.3).astype(np.float32)
    y[rng.random((len(mols), 1)) < 0.1] = np.nan
    ds = G.DeviceDataset.from_molecules(mols, dev, a.k, labels=y, drop_single_atom=True)
    if ds.dropped:  # (ids below index ds, not mols)
        raise SystemExit("eval_loader_bench: the synthetic set holds a one-atom molecule")
    idx = np.sort(rng.permutation(len(ds))[:a.subset])
    out(dict(what="dataset", molecules=len(ds), subset=len(idx),
             nodes=int(ds.host["node_off"][-1]), edges=int(ds.host["edge_off"][-1]),
             features=ds.num_features, build_s=time.perf_counter() - t0))
    feeds = a.only.split(",")
    for B in (int(b) for b in a.batches.split(",")):
        caps = ds.capacities(B, "sequential", indices=idx)
        model = make_model(ds.num_features, a.k, B, dev)
        runs = {feed: build(feed, ds, caps, mols, y, idx, model, B, a.k, dev) for feed in feeds}
        for r in runs.values():
            for _ in range(a.warm_passes):
                r.one_pass()
        per = {feed: [] for feed in runs}
        aucs, rows = {}, {}
        for _ in range(a.rounds):
            for feed, r in runs.items():  # alternating in one process
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                aucs[feed], rows[feed] = r.one_pass()
                per[feed].append((time.perf_counter() - t0) * 1e3)
        for feed, r in runs.items():
            rec = dict(what="pass", feed=feed, batch=B, steps=r.steps, rows=rows[feed],
                       capacities=[caps[0], caps[1], list(caps[3])], rocauc=aucs[feed],
                       passes_ms=per[feed], per_step_us=float(np.median(per[feed])) / r.steps * 1e3,
                       ego_error=r.static.ego_error(), **stats(per[feed]))
            if r.evl is not None:
                rec["loader_error"] = r.evl.error()
            out(rec)
        if "pool" in runs:
            base = float(np.median(per["pool"]))
            for feed in runs:
                if feed != "pool":
                    out(dict(what="pass_delta", feed=feed, batch=B,
                             minus_pool_ms=float(np.median(per[feed])) - base,
                             minus_pool_per_step_us=(float(np.median(per[feed])) - base)
                             / runs[feed].steps * 1e3,
                             pool_spread_ms=max(per["pool"]) - min(per["pool"])))
        del runs


if __name__ == "__main__":
    main()
