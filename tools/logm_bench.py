"""Baseline timings of the two logM reconstruction paths (no bar: nobody has
measured either before; both sides are recorded).

Per batch:
  (a) the host path: the target build (graph.trans_logM per molecule +
      graph.LogMBatch, wall clock, once) and the dense kernels
      (scgib_recon_logm_fwd / _bwd);
  (b) the device path: the ego-net build (for reference), the target build on
      its slots (scgib_logm_targets) and the sparse kernels
      (scgib_recon_logm_sparse_fwd / _bwd).
Device times: device events around single calls, --warmup calls, then --reps
timed repeats; median, min, p10, p90.  Every record carries the launch's
algorithmic bytes (inputs and outputs once, scratch written and read once) and
their share of 8 TB/s at the median.

  python tools/logm_bench.py --out profiles/logm_baseline/logm_bench.jsonl
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("s-cgib_amd")
ops, _lib, G = pkg.ops, pkg._lib, pkg.graph

HBM = 8e12  # bytes / s

BATCHES = [  # (tag, workload, B, synth overrides, k values)
    ("mutagenicity_B32", "mutagenicity", 32, {}, (1, 2, 3)),
    ("qm9_B512", "qm9", 512, {}, (2,)),
    ("long_B32", "molhiv", 32, {"mu": 150, "sigma": 40}, (1, 2)),
]


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_us": float(np.median(a)) * 1e3, "min_us": float(a[0]) * 1e3,
            "p10_us": float(a[len(a) // 10]) * 1e3, "p90_us": float(a[(9 * len(a)) // 10]) * 1e3}


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


def bench_batch(tag, gh, k, warm, reps, out):
    dev = torch.device("cuda", 0)
    g = gh.to(dev)
    B, n, e = g.batch_size, g.num_nodes(), g.num_edges()
    sizes = gh.batch_num_nodes_host()
    n2 = int((sizes.astype(np.int64) ** 2).sum())
    p, st = ops._p, ops._stream
    base = {"batch": tag, "k": k, "B": B, "nodes": n, "edges": e, "sum_n2": n2,
            "max_graph_nodes": int(sizes.max())}

    def rec(path, launch, t, nbytes):
        r = dict(base, path=path, launch=launch, bytes=int(nbytes), **t)
        r["share_of_8TBs"] = nbytes / (t["median_us"] * 1e-6) / HBM
        out(r)
        return t["median_us"]

    torch.manual_seed(0)
    im = (0.3 * torch.randn(n, 64, device=dev)).contiguous()
    gl = torch.ones(1, device=dev)
    grad = torch.empty_like(im)
    lossg = torch.empty(B, device=dev)
    loss = torch.empty((), device=dev)

    # (a) host targets + dense kernels
    t0 = time.perf_counter()
    mols = list(pkg.cache._split(gh, B))
    lb = G.LogMBatch([G.trans_logM(gi, k) for gi in mols], dev)
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    out(dict(base, path="dense", launch="host targets (trans_logM + LogMBatch, wall clock)",
             wall_ms=host_ms, bytes=4 * n2))
    d_f = rec("dense", "recon_logm_fwd (2 launches)", timed(lambda: _lib.call(
        "scgib_recon_logm_fwd", p(im), p(g.graph_ptr), B, p(lb.S), p(lb.offsets), p(lb.C), k,
        p(lossg), p(loss), st()), warm, reps), 256 * n + 4 * n2 + 12 * B)
    d_b = rec("dense", "recon_logm_bwd", timed(lambda: _lib.call(
        "scgib_recon_logm_bwd", p(im), p(g.graph_ptr), B, p(lb.S), p(lb.offsets), k, p(gl),
        p(grad), st()), warm, reps), 512 * n + 4 * n2)
    dense_loss = float(loss)
    del lb

    # (b) device targets + sparse kernels
    ego = G.egonet_batch(g, k)
    rec("sparse", "egonet_batch (the step builds it anyway)",
        timed(lambda: G.egonet_batch(g, k), warm, reps), 0)
    nodes = ego.ndata["_ID"]
    n_s = int(nodes.shape[0])
    base["ego_nodes"] = n_s
    base["slot_share_of_n2"] = n_s / n2
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.empty(k * n_s, dtype=torch.int32, device=dev)
    s_in, s_sym = torch.empty(n_s, device=dev), torch.empty(n_s, device=dev)
    C = torch.empty(B, dtype=torch.float64, device=dev)
    s_t = rec("sparse", "logm_targets", timed(lambda: _lib.call(
        "scgib_logm_targets", p(g.rowptr), p(g.col), p(g.graph_ptr), B, n, e, p(ego.graph_ptr),
        p(nodes), n_s, k, p(counts), p(s_in), p(s_sym), p(C), p(err), None, st()), warm, reps),
        4 * (2 * n + 2 + e) + 4 * n_s + 8 * k * n_s + 8 * n_s + 8 * B)
    assert int(err.item()) == 0
    mgn = max(g.max_graph_nodes, 1)
    parts = torch.empty(B * int(_lib.query("scgib_recon_logm_sparse_parts", mgn)),
                        dtype=torch.float64, device=dev)
    gram = torch.empty(B, 4096, device=dev)
    s_f = rec("sparse", "recon_logm_sparse_fwd (3 launches)", timed(lambda: _lib.call(
        "scgib_recon_logm_sparse_fwd", p(im), p(g.graph_ptr), B, n, p(ego.graph_ptr), p(nodes),
        n_s, p(s_in), p(C), k, mgn, p(gram), p(parts), p(lossg), p(loss), None, st()),
        warm, reps), 512 * n + 264 * n_s + 4 * n + 16384 * B + 8 * parts.numel())
    sparse_loss = float(loss)
    s_b = rec("sparse", "recon_logm_sparse_bwd", timed(lambda: _lib.call(
        "scgib_recon_logm_sparse_bwd", p(im), p(g.graph_ptr), B, n, p(ego.graph_ptr), p(nodes),
        n_s, p(s_sym), p(gram), k, mgn, p(gl), p(grad), None, st()), warm, reps),
        512 * n + 264 * n_s + 4 * n + 16384 * B)
    out(dict(base, path="summary", host_targets_ms=host_ms, dense_fwd_bwd_us=d_f + d_b,
             device_targets_us=s_t, sparse_fwd_bwd_us=s_f + s_b,
             dense_over_sparse_kernels=(d_f + d_b) / (s_f + s_b),
             loss_dense=dense_loss, loss_sparse=sparse_loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logm_bench: needs the HIP device (nothing is measured on a CPU)")
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

    for tag, workload, B, kw, ks in BATCHES:
        gh, _ = G.collate_pyg(pkg.synth.molecules(B, workload, seed=0, **kw))
        for k in ks:
            bench_batch(tag, gh, k, a.warmup, a.reps, out)


if __name__ == "__main__":
    main()
