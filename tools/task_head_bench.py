"""The multi-label fine-tune tail, torch against csrc/task_head.hip, on one
MI355X: predict head (K = 128 -> 64 -> C, sigmoid), the BCE loss through
MetricWrapper(model.loss, "ignore-flatten") on ~60 % NaN labels, and the
backward to the head's input and weights.

  (a) torch tail   models.FUSE_HEAD = False: torch's head, the wrapper's
                   boolean-index path (it synchronises on its own, so it is
                   timed with a host clock around a device synchronise);
  (b) device tail  models.FUSE_HEAD = True, the same Python: scgib_head_wide_fwd,
                   scgib_task_loss_fwd / _bwd, scgib_head_wide_bwd (+ the slab
                   reduce), timed with device events (and the same host clock),
                   eager and as a captured graph's replay; then each launch alone
                   through the C-ABI.

(a) and (b) alternate repeat by repeat in one process.  Per figure: median
(min; p10-p90) in microseconds over --repeats timed repeats after --warmup.
One JSON line per figure on stdout and in <out>/raw.jsonl.

    python tools/task_head_bench.py --out profiles/task_head_baseline
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("s-cgib_amd")
ops, _lib, models = pkg.ops, pkg._lib, pkg.models

SHAPES = [(32, 128), (1024, 128), (256, 617)]
K, NAN_SHARE = 128, 0.6


class _Tail:
    """Carrier of the model's BCE loss method (the wrapper recognises it)."""
    loss = models.Mainmodel_finetuning.loss


def stats(us):
    us = np.asarray(us, np.float64)
    return {"median_us": float(np.median(us)), "min_us": float(us.min()),
            "p10_us": float(np.percentile(us, 10)), "p90_us": float(np.percentile(us, 90)),
            "n": int(us.size)}


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def bench_shape(B, C, warmup, repeats, dev, emit):
    torch.manual_seed(B * 1000 + C)
    seq = nn.Sequential(nn.Linear(K, 64), nn.ReLU(), nn.Linear(64, C)).to(dev)
    x = torch.randn(B, K, device=dev, requires_grad=True)
    tg = torch.randint(0, 2, (B, C), device=dev).float()
    tg[torch.rand(B, C, device=dev) < NAN_SHARE] = float("nan")
    wrapped = pkg.MetricWrapper(metric=_Tail().loss, target_nan_mask="ignore-flatten")

    def tail(fuse):
        models.FUSE_HEAD = fuse
        x.grad = None
        seq.zero_grad(set_to_none=True)
        if fuse:
            scores = ops.predict_head(x, seq, True)
        else:
            scores = torch.sigmoid(seq(x))
        loss = wrapped(scores, tg)
        loss.backward()
        return loss

    # the two tails compute the same loss
    la, lb = float(tail(False)), float(tail(True))
    assert abs(la - lb) <= 1e-5 * abs(la), (la, lb)
    host = {False: [], True: []}
    dev_us = []
    for it in range(warmup + repeats):
        for fuse in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if fuse:
                d = event_time(lambda: tail(True))
            else:
                tail(False)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if it >= warmup:
                host[fuse].append((t1 - t0) * 1e6)
                if fuse:
                    dev_us.append(d)
    base = {"B": B, "C": C, "K": K, "nan_share": NAN_SHARE, "kept": int((~torch.isnan(tg)).sum())}
    emit({**base, "what": "torch_tail", "clock": "host+sync", **stats(host[False])})
    emit({**base, "what": "device_tail_eager", "clock": "host+sync", **stats(host[True])})
    emit({**base, "what": "device_tail_eager", "clock": "events", **stats(dev_us)})

    # the device tail as a captured graph
    models.FUSE_HEAD = True
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tail(True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    x.grad = None
    seq.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scores = ops.predict_head(x, seq, True)
        wrapped(scores, tg).backward()
    rep = [event_time(graph.replay) for _ in range(warmup + repeats)][warmup:]
    emit({**base, "what": "device_tail_graph_replay", "clock": "events", **stats(rep)})

    # each launch alone, through the C-ABI
    p, st = ops._p, ops._stream
    f = dict(device=dev, dtype=torch.float32)
    w1, b1, w2, b2 = (t.detach() for t in (seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias))
    xd = x.detach()
    hid, out = torch.empty(B, 64, **f), torch.empty(B, C, **f)
    d_out, dx = torch.empty(B, C, **f), torch.empty(B, K, **f)
    dw1, db1, dw2, db2 = torch.empty(64, K, **f), torch.empty(64, **f), torch.empty(C, 64, **f), torch.empty(C, **f)
    nslab = int(_lib.query("scgib_head_wide_slab_floats", B, K))
    slab = torch.empty(max(nslab, 1), **f)
    loss, g = torch.empty((), **f), torch.ones(1, **f)
    count = torch.empty((), dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.query("scgib_task_loss_ws_doubles")), dtype=torch.float64, device=dev)
    cnt = ops.counters(dev, "task_loss", 1)
    n = B * C
    launches = {
        "scgib_head_wide_fwd": lambda: _lib.call(
            "scgib_head_wide_fwd", p(xd), B, K, p(w1), p(b1), p(w2), p(b2), C, 1, p(hid), p(out),
            None, st()),
        "scgib_task_loss_fwd": lambda: _lib.call(
            "scgib_task_loss_fwd", p(out), p(tg), n, 0, 1, p(ws), p(cnt), p(loss), p(count), st()),
        "scgib_task_loss_bwd": lambda: _lib.call(
            "scgib_task_loss_bwd", p(out), p(tg), n, 0, 1, p(g), p(loss), p(count), p(d_out), st()),
        "scgib_head_wide_bwd": lambda: _lib.call(
            "scgib_head_wide_bwd", p(xd), p(hid), p(out), p(d_out), B, K, p(w1), p(w2), C, 1, p(dx),
            p(dw1), p(db1), p(dw2), p(db2), p(slab) if nslab else None, st()),
    }
    for name, fn in launches.items():  # in dependency order: each one's inputs exist
        us = [event_time(fn) for _ in range(warmup + repeats)][warmup:]
        emit({**base, "what": name, "clock": "events", **stats(us)})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--out", default=None, help="directory for raw.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("task_head_bench: no HIP device (a timing needs the GPU)")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for B, C in SHAPES:
        bench_shape(B, C, a.warmup, a.repeats, dev, emit)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "raw.jsonl"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
