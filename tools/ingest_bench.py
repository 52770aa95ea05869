"""What the device-side edge-list ingest (csrc/ingest.hip)
costs per batch, against the host route it replaces, on the same inputs.

At the QM9-like B = 512 and the molpcba-like B = 1024 synthetic batches
(synth, seed 0), per batch:

  (a) the host route: graph.collate_pyg + StaticBatch.pad + the upload, host
      clock around a synchronise (as tools/loader_bench.py times it);
  (b) eager graph.from_coo of the flat device edge list, its one device ->
      host read included, host clock around a synchronise;
  (c) the three launches of StaticBatch.ingest: device events around --reps
      back-to-back repetitions.

--only c --reps N runs (c) alone, for a kernel trace of it.  No bar: nothing
here had been measured before.

  python tools/ingest_bench.py --out profiles/ingest_baseline/ingest_bench.jsonl
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
G = pkg.graph


def stats(v, unit="ms"):
    a = np.sort(np.asarray(v, np.float64))
    return {f"median_{unit}": float(np.median(a)), f"min_{unit}": float(a[0]),
            f"max_{unit}": float(a[-1]), "samples": int(len(a))}


def flat(mols, dev):
    counts = np.array([x.shape[0] for _, x in mols], np.int64)
    gptr = np.concatenate([[0], np.cumsum(counts)])
    src = np.concatenate([ei[0] + o for (ei, _), o in zip(mols, gptr)])
    dst = np.concatenate([ei[1] + o for (ei, _), o in zip(mols, gptr)])
    x = np.concatenate([x for _, x in mols]).astype(np.float32)
    return (torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev),
            torch.from_numpy(gptr.astype(np.int32)).to(dev), torch.from_numpy(x).to(dev))


def timed(fn, reps, warm=3):
    ms = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = fn(i)
        torch.cuda.synchronize()
        if i >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
        del keep
    return stats(ms)


def bench(a, workload, B, dev, out):
    nb = a.batches
    sets = [pkg.synth.molecules(B, workload, seed=s) for s in range(nb)]
    hosts = [G.collate_pyg(m)[0] for m in sets]
    caps = G.StaticBatch.capacities(hosts, 1, slack=1.02)
    feat = sets[0][0][1].shape[1]
    static = G.StaticBatch(B, caps[0], caps[1], feat, caps[2], caps[3], dev, 1)
    flats = [flat(m, dev) for m in sets]
    base = dict(workload=workload, batch=B, nodes=hosts[0].num_nodes(), edges=hosts[0].num_edges(),
                raw_edges=int(flats[0][0].numel()), blob_bytes=int(static.blob.numel()))
    only = a.only.split(",")
    if "a" in only:
        out(dict(what="host_route", note="collate_pyg + StaticBatch.pad + upload, per batch", **base,
                 **timed(lambda i: static.pad(G.collate_pyg(sets[i % nb])[0]), a.host_reps)))
    if "b" in only:
        def eager(i):
            src, dst, gptr, x = flats[i % nb]
            return G.from_coo(src, dst, gptr, x.shape[0], x=x)
        out(dict(what="from_coo", note="eager: three launches and the one status read, per batch",
                 **base, **timed(eager, a.host_reps)))
    if "c" in only:
        src, dst, gptr, x = flats[0]
        static.ingest(src, dst, gptr, x)
        torch.cuda.synchronize()
        same = bool(torch.equal(static.blob, static.pad(hosts[0])["blob"]))
        per_call = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                static.ingest(src, dst, gptr, x)
            e1.record()
            torch.cuda.synchronize()
            per_call.append(e0.elapsed_time(e1) * 1e3 / a.reps)
        out(dict(what="static_ingest", note="mark + count + fill back to back, per call (device events)",
                 reps=a.reps, blob_equals_pad=same, ingest_error=static.ingest_error(), **base,
                 **stats(per_call, "us")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", default="a,b,c")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench: needs the HIP device (nothing is measured on a CPU)")
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

    for workload, B in (("qm9", 512), ("molpcba", 1024)):
        bench(a, workload, B, dev, out)


if __name__ == "__main__":
    main()
