"""Timings of the evaluation metrics: the host path (metrics.eval_ap /
eval_rocauc: device-to-host copy, then sklearn per task column) against the
device path (metrics.EvalBuffer) on the same device tensors.  No bar: neither
side has been measured before; both times and their ratio are recorded.

Synthetic data in the shapes of the OGB splits (the datasets themselves are
not available to the benchmark): sigmoid-like fp32 scores, 0/1 labels with
--positive-share ones, and a share of NaN labels that is a stand-in for
molpcba's real sparsity.

  * host: wall clock after a synchronise, median of --host-reps (it runs for
    seconds);
  * device: device events around per_task() plus the final read (EvalBuffer.ap()),
    warm-up then --reps timed repeats, medians; the split into key build,
    torch.sort and scan from events between the phases (summed over the task
    groups);
  * one append of 1,024 x 128 rows, eager and as a replayed graph.

  python tools/eval_bench.py --out profiles/eval_baseline/eval_bench.jsonl
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
ops, metrics = pkg.ops, pkg.metrics

SHAPES = {  # name: (rows, tasks, NaN label share)
    "molhiv_valid": (4113, 1, 0.0),
    "molhiv_train": (32901, 1, 0.0),
    "molpcba_valid": (43793, 128, 0.3),
    "molpcba_train": (350343, 128, 0.3),
}


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1])}


def synth(n, c, nan_share, positive, dev):
    g = torch.Generator(device=dev).manual_seed(n + c)
    scores = torch.sigmoid(torch.randn(n, c, device=dev, generator=g))
    labels = (torch.rand(n, c, device=dev, generator=g) < positive).float()
    if nan_share:
        labels[torch.rand(n, c, device=dev, generator=g) < nan_share] = float("nan")
    return scores, labels


def bench_shape(name, a, dev, out):
    n, c, nan_share = SHAPES[name]
    scores, labels = synth(n, c, nan_share, a.positive_share, dev)
    base = {"shape": name, "rows": n, "tasks": c, "nan_share": nan_share}

    buf = metrics.EvalBuffer(n, c, dev, workspace_bytes=a.workspace_bytes)
    buf.append(scores, labels)
    totals = []
    for i in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ap = buf.ap()  # per_task() and the one read
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            totals.append(e0.elapsed_time(e1))
    vals = (ap, buf.rocauc()["rocauc"])
    phases = {"keys": [], "sort": [], "scan": []}
    groups = 0
    for i in range(a.warmup + a.reps):
        marks = []
        ops.rank_metrics(buf.scores, buf.labels, rows=buf.state[0:1], err=buf.state[2:3],
                         workspace_bytes=a.workspace_bytes, marks=marks)
        torch.cuda.synchronize()
        if i < a.warmup:
            continue
        acc = dict.fromkeys(phases, 0.0)
        for (_, prev), (phase, ev) in zip(marks, marks[1:]):
            acc[phase] += prev.elapsed_time(ev)
        groups = sum(1 for m in marks if m[0] == "keys")
        for k in phases:
            phases[k].append(acc[k])
    rec = dict(base, what="device", task_groups=groups, ap=vals[0], rocauc=vals[1], **stats(totals))
    rec.update({f"{k}_median_ms": float(np.median(v)) for k, v in phases.items()})
    out(rec)

    host = []
    if a.host_reps:
        hv = None
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv = (metrics.eval_ap(labels, scores), metrics.eval_rocauc(labels, scores)["rocauc"])
            host.append((time.perf_counter() - t0) * 1e3)
        # both host metrics: the device path's one per_task() yields both as well
        out(dict(base, what="host", metrics="eval_ap + eval_rocauc", ap=hv[0], rocauc=hv[1],
                 ap_diff=abs(hv[0] - vals[0]), rocauc_diff=abs(hv[1] - vals[1]), **stats(host)))
        out(dict(base, what="ratio",
                 host_over_device=float(np.median(host)) / float(np.median(totals))))


def bench_append(a, dev, out):
    b, c = 1024, 128
    scores, labels = synth(b, c, 0.3, a.positive_share, dev)
    buf = metrics.EvalBuffer(b * (a.warmup + a.reps + 8), c, dev)

    def timed(fn):
        buf.reset()
        ms = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return {k.replace("_ms", "_us"): v * 1e3 for k, v in stats(ms).items()}

    out(dict(what="append", mode="eager", rows=b, tasks=c, **timed(lambda: buf.append(scores, labels))))
    buf.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.append(scores, labels)
    out(dict(what="append", mode="graph", rows=b, tasks=c, **timed(graph.replay)))
    if buf.rows() != b * (a.warmup + a.reps):
        raise SystemExit(f"eval_bench: the replayed appends left {buf.rows()} rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--positive-share", type=float, default=0.1)
    ap.add_argument("--workspace-bytes", type=int, default=256 << 20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--append-mode", default="w", choices=["w", "a"],
                    help="open --out for writing or appending (shapes run in several calls)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs the HIP device (nothing is measured on a CPU)")
    dev = torch.device("cuda", 0)
    fh = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        fh = open(a.out, a.append_mode)

    def out(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    for name in [s for s in a.shapes.split(",") if s]:
        bench_shape(name, a, dev, out)
    bench_append(a, dev, out)


if __name__ == "__main__":
    main()
