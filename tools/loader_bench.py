"""Step time of the replayed pretrain step fed by graph.DeviceLoader against
the same step fed by a fixed StaticBatch.pool of the same batches, and what the
loader replaces: collating, padding and uploading every batch on the host.

A step body like bench.py's (QM9-like molecules from synth, B = 512, k = 1,
GIN-64x5, device noise one step ahead, the final reduce fused into Adam),
captured once per variant (the fixed pool; the loader with collate_ahead
behind load_next on the main queue; the loader with it on the ego chain's
queue behind the ego prefetch, DeviceLoader.ride) and replayed — as ops.SplitGraph's two lanes where
the hand-offs are on, unless --no-split.  The variants live in one process
and alternate in rounds of --round-steps steps after --warmup steps each; a
round is timed with a host clock around a synchronise.  The loader shuffles
and its two permutation buffers repeat (begin_epoch is timed on its own), so
the fixed pool holds exactly the 2 S batches the loader walks.  No bar: neither
side has been measured before.

Also recorded:
  * the two collate launches alone: device events around each, and around
    --pairs back-to-back plan + fill pairs;
  * the host path per batch: collate (collate_pyg of the molecule tuples, and
    CSRCache.collate of a cache written to a temporary directory) +
    StaticBatch.pad + the upload, host clock around a synchronise;
  * one begin_epoch call (host time, and until its copy has landed).

  python tools/loader_bench.py --out profiles/loader_baseline/loader_bench.jsonl
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
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


def make_model(F_in, k, B, dev):
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=B, gin_layers=5, task="graph_classification")
    torch.manual_seed(0)
    inner = pkg.models.Mainmodel(args, F_in, 64, 4, 4, k, "GIN")
    return pkg.models.Mainmodel_continue(args, F_in, 64, 4, 4, k, 1, inner, "GIN").to(dev).train()


def build_step(ds, caps, B, k, dev, feed, mols, split, warm=3):
    """One captured step over its own model, static batch and pool."""
    static = G.StaticBatch(B, caps[0], caps[1], ds.num_features, caps[2], caps[3], dev, k)
    loader = G.DeviceLoader(ds, static, seed=0)
    keep = None
    if feed != "pool":
        loader.prime()
        pool = loader.pool
    else:  # the 2 S batches the loader's two repeating buffers hold, padded on the host
        S = loader.steps_per_epoch
        keep = []
        for j in range(2 * S):
            ids = loader.epoch_permutation(j // S)[(j % S) * B:(j % S) * B + B]
            keep.append(static.pad(G.collate_pyg([mols[i] for i in ids])[0]))
        pool = static.pool(keep)
        loader = None
    model = make_model(ds.num_features, k, B, dev)
    opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
    pf = G.EgoPrefetch(static, pool)
    pf.prime()
    if feed == "loader_ego":  # collate_ahead on the ego chain's queue, behind the ego prefetch
        loader.ride(pf)
    nf = ops.NoisePrefetch(static.graph, dev)
    nf.prime()
    one = torch.ones((), dtype=torch.float32, device=dev)

    def body():
        static.load_next(pool, pf)
        if feed == "loader_main":  # behind load_next on the main queue
            loader.collate_ahead()
        _, kl, con, rec = model(static.graph, static.x, None, None, None, 1, None, k, dev, B)
        torch.autograd.backward((kl, rec, con), (one, one, one))
        pf.join()
        return kl.detach(), rec.detach(), con.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            opt.zero_grad(set_to_none=True)
            with ops.fuse_final_into_step():
                body()
                opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph), ops.fuse_final_into_step():
        losses = body()
        opt.step()
    lanes = None
    if split and ops.xq_enabled():
        try:
            lanes = ops.SplitGraph(graph, dev)
        except ops.SplitUnsupported as exc:
            print(f"loader_bench: {feed}: graph replayed whole: {exc}", file=sys.stderr)
    if lanes is None:
        graph.instantiate()
    step = lanes.replay if lanes is not None else graph.replay
    return SimpleNamespace(step=step, losses=losses, static=static, loader=loader, pool=pool,
                           keep=(keep, one, model, opt, pf, nf, graph), lanes=lanes,
                           replay="two lanes" if lanes is not None else "whole graph")


def bench_steps(a, ds, caps, mols, dev, out):
    runs = {feed: build_step(ds, caps, a.batch, a.k, dev, feed, mols, not a.no_split)
            for feed in ("pool", "loader_main", "loader_ego")}
    for r in runs.values():
        for _ in range(a.warmup):
            r.step()
    torch.cuda.synchronize()
    per_round = {feed: [] for feed in runs}
    for _ in range(a.rounds):
        for feed, r in runs.items():  # alternating in one process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.round_steps):
                r.step()
            torch.cuda.synchronize()
            per_round[feed].append((time.perf_counter() - t0) * 1e3 / a.round_steps)
    for feed, r in runs.items():
        finite = bool(torch.isfinite(torch.stack(r.losses)).all())
        rec = dict(what="step", feed=feed, replay=r.replay, batch=a.batch,
                   steps=a.rounds * a.round_steps, warmup=a.warmup, rounds_ms=per_round[feed],
                   losses_finite=finite, ego_error=r.static.ego_error(),
                   **stats(per_round[feed]))
        if r.loader is not None:
            rec["loader_error"] = r.loader.error()
        out(rec)
    pool_ms = float(np.median(per_round["pool"]))
    for feed in ("loader_main", "loader_ego"):
        load_ms = float(np.median(per_round[feed]))
        out(dict(what="step_delta", feed=feed, loader_minus_pool_us=(load_ms - pool_ms) * 1e3,
                 pool_spread_us=(max(per_round["pool"]) - min(per_round["pool"])) * 1e3,
                 graphs_per_s_loader=a.batch / load_ms * 1e3,
                 graphs_per_s_pool=a.batch / pool_ms * 1e3))
    for r in runs.values():
        if r.lanes is not None:
            r.lanes.close()
    return runs["loader_main"]


def bench_launches(a, run, dev, out):
    loader = run.loader
    d, lib = loader._desc, pkg._lib
    import ctypes
    ref = ctypes.byref(d)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    plan, fill = [], []
    for i in range(a.warmup + a.reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        lib.call("scgib_collate_plan", ref, 2, -1, 1, st())
        e[1].record()
        lib.call("scgib_collate_fill", ref, 1, st())
        e[2].record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            plan.append(e[0].elapsed_time(e[1]) * 1e3)
            fill.append(e[1].elapsed_time(e[2]) * 1e3)
    out(dict(what="collate_launch", kernel="collate_plan_k", **stats(plan, "us")))
    out(dict(what="collate_launch", kernel="collate_fill_k", **stats(fill, "us")))
    pairs = []
    for i in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.pairs):
            loader.collate_ahead()
        e1.record()
        torch.cuda.synchronize()
        pairs.append(e0.elapsed_time(e1) * 1e3 / a.pairs)
    out(dict(what="collate_ahead", note="plan + fill back to back, per pair", pairs=a.pairs,
             blob_bytes=int(run.static.blob.numel()), **stats(pairs, "us")))
    host, landed = [], []
    for e in range(1, 6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loader.begin_epoch(e)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        host.append((t1 - t0) * 1e3)
        landed.append((time.perf_counter() - t0) * 1e3)
    out(dict(what="begin_epoch", molecules=loader.M, host=stats(host), landed=stats(landed)))
    if loader.error():
        raise SystemExit(f"loader_bench: {loader.error()} batches overflowed the sampled capacities")


def bench_host_path(a, ds, caps, mols, labels, dev, out):
    """The figure the loader replaces: per batch, collate + pad + upload on the host."""
    static = G.StaticBatch(a.batch, caps[0], caps[1], ds.num_features, caps[2], caps[3], dev, a.k)
    rng = np.random.default_rng(1)
    batches = [rng.choice(len(mols), a.batch, replace=False) for _ in range(a.host_reps + 3)]

    def timed(collate):
        ms = []
        for i, ids in enumerate(batches):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = static.pad(collate(ids))
            torch.cuda.synchronize()
            if i >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
            del p
        return stats(ms)

    out(dict(what="host_path", collate="graph.collate_pyg", batch=a.batch,
             note="collate + StaticBatch.pad + upload, per batch (the figure the loader replaces)",
             **timed(lambda ids: G.collate_pyg([mols[i] for i in ids])[0])))
    with tempfile.TemporaryDirectory() as tmp:
        cache = pkg.cache.write([(ei, x, y) for (ei, x), y in zip(mols, labels)], tmp, "bench",
                                cap=None)
        out(dict(what="host_path", collate="cache.CSRCache.collate", batch=a.batch,
                 note="collate + StaticBatch.pad + upload, per batch (the figure the loader replaces)",
                 **timed(lambda ids: cache.collate(ids)[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--molecules", type=int, default=16384)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--round-steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--only", default="steps,launches,host")
    a = ap.parse_args()
    if a.rounds * a.round_steps < 300:
        raise SystemExit("loader_bench: time at least 300 steps per variant")
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench: needs the HIP device (nothing is measured on a CPU)")
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

    mols = [(ei, F.normalize(torch.from_numpy(x)).numpy())
            for ei, x in pkg.synth.molecules(a.molecules, "qm9", seed=0)]
    labels = np.random.default_rng(0).standard_normal((len(mols), 1)).astype(np.float32)
    t0 = time.perf_counter()
    ds = G.DeviceDataset.from_molecules(mols, dev, a.k, labels=labels)
    caps = ds.capacities(a.batch, "sampled", slack=1.05)
    out(dict(what="dataset", molecules=len(ds), nodes=int(ds.host["node_off"][-1]),
             edges=int(ds.host["edge_off"][-1]), features=ds.num_features,
             build_s=time.perf_counter() - t0, capacities=[caps[0], caps[1], caps[2], list(caps[3])],
             worst=list(ds.capacities(a.batch, "worst")[:2])))
    only = a.only.split(",")
    run = None
    if "steps" in only:
        run = bench_steps(a, ds, caps, mols, dev, out)
    if "launches" in only:
        if run is None:
            static = G.StaticBatch(a.batch, caps[0], caps[1], ds.num_features, caps[2], caps[3],
                                   dev, a.k)
            run = SimpleNamespace(static=static, loader=G.DeviceLoader(ds, static, seed=0))
            run.loader.prime()
        bench_launches(a, run, dev, out)
    if "host" in only:
        bench_host_path(a, ds, caps, mols, labels, dev, out)


if __name__ == "__main__":
    main()
