"""Baseline timings of the GCN / GraphSAGE encoders (no bar: the first numbers
for later work to beat).

Per layer shape and mode, on the QM9-like B = 512 molecule graph and on its
k = 1 ego graph: the forward launch, the weight-gradient launch and the whole
backward (weight gradients + dx), each timed alone with device events around
single launches (warm-up, then --reps timed repeats; median, min, p10, p90),
with the algorithmic bytes of the launch and their share of 8 TB/s.  Then the
eager (uncaptured) pretrain step, forward + backward + Adam, per encoder.

  python tools/conv_bench.py --out profiles/conv_baseline/conv_bench.jsonl
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
ops, _lib = pkg.ops, pkg._lib

SHAPES = [(32, 128), (128, 128), (128, 64), (32, 64), (64, 64)]
PEAK = 8.0e12  # HBM bytes/s


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


def layer_bytes(n, e, d_in, d_out, self_term, relu):
    w = 4 * d_in * d_out * (2 if self_term else 1) + 4 * d_out
    idx = 4 * e + 4 * (n + 1) + 8 * n  # col, rowptr, the two coefficient vectors
    fwd = 4 * n * d_in + idx + w + 4 * n * d_in + 4 * n * d_out  # x, ..., agg and out written
    wgrad = 4 * n * d_out * (3 if relu else 1) + 4 * n * d_in * (2 if self_term else 1)
    dx = 4 * n * d_out + idx + w + 4 * n * d_in
    return fwd, wgrad, wgrad + dx


def bench_layers(g, tag, dev, warm, reps, out):
    n, e = g.num_nodes(), g.num_edges()
    p, st = ops._p, ops._stream
    for mode in ("gcn", "mean"):
        gcn = mode == "gcn"
        c_src, c_dst = ops.conv_norm(g, mode)
        for d_in, d_out in SHAPES:
            x = torch.randn(n, d_in, device=dev)
            shape = (d_in, d_out) if gcn else (d_out, d_in)
            wn = torch.randn(shape, device=dev) / d_in ** 0.5
            ws = None if gcn else torch.randn(shape, device=dev) / d_in ** 0.5
            b = torch.randn(d_out, device=dev)
            agg, o = torch.empty(n, d_in, device=dev), torch.empty(n, d_out, device=dev)
            go, dz = torch.randn(n, d_out, device=dev), torch.empty(n, d_out, device=dev)
            dx = torch.empty(n, d_in, device=dev)
            width = int(_lib.query("scgib_conv_slab_width", d_in, d_out, int(not gcn)))
            slab = torch.empty(int(_lib.query("scgib_conv_slabs", n)) * width, device=dev)

            def fwd():
                _lib.call("scgib_conv_layer_fwd", p(x), p(g.rowptr), p(g.col), p(c_src), p(c_dst),
                          n, d_in, d_out, p(wn), p(ws), int(gcn), p(b), 1, p(agg), p(o),
                          p(g.dims), st())

            def bwd(with_dx):
                _lib.call("scgib_conv_layer_bwd", p(go), p(o), p(agg), p(x), p(g.rowptr_t),
                          p(g.col_t), p(c_src), p(c_dst), n, d_in, d_out, p(wn), p(ws), int(gcn),
                          0, p(dz), p(dx) if with_dx else None, p(slab), p(g.dims), st())

            bf, bw, bb = layer_bytes(n, e, d_in, d_out, not gcn, True)
            for name, fn, nbytes in (("fwd", fwd, bf), ("wgrad", lambda: bwd(False), bw),
                                     ("bwd", lambda: bwd(True), bb)):
                r = timed(fn, warm, reps)
                r.update(graph=tag, mode=mode, d_in=d_in, d_out=d_out, launch=name, nodes=n,
                         edges=e, alg_bytes=nbytes,
                         frac_of_8TBs=nbytes / (r["median_us"] * 1e-6) / PEAK)
                out(r)


def bench_step(encoder, gh, dev, warm, reps, out):
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=512, gin_layers=5, task="graph_classification")
    torch.manual_seed(0)
    inner = pkg.models.Mainmodel(args, 11, 64, 4, 4, 1, encoder)
    model = pkg.models.Mainmodel_continue(args, 11, 64, 4, 4, 1, 1, inner, encoder).to(dev).train()
    opt = pkg.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-5)
    g = gh.to(dev)
    x = F.normalize(g.ndata["x"].float())

    def step():
        opt.zero_grad(set_to_none=True)
        _, kl, con, rec = model(g, x, None, None, None, 1, None, 1, dev, 512)
        (kl + con + rec).backward()
        opt.step()

    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    r = stats(ms)
    r.update(launch="eager_pretrain_step", encoder=encoder, B=512, nodes=g.num_nodes())
    out(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--molecules", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_bench: needs the HIP device (nothing is measured on a CPU)")
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

    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(a.molecules, "qm9", seed=0))
    g = gh.to(dev)
    ego = pkg.graph.egonet_batch(g, 1)
    ego.num_edges()
    bench_layers(g, "molecules", dev, a.warmup, a.reps, out)
    bench_layers(ego, "ego_k1", dev, a.warmup, a.reps, out)
    for enc in ("GCN", "GraphSAGE", "GIN"):
        bench_step(enc, gh, dev, a.warmup, max(a.reps // 2, 100), out)


if __name__ == "__main__":
    main()
