"""Baseline timings of the Transformer encoder (no bar: nobody has measured
either side before; both times and their ratio are recorded).

On the QM9-like B = 512 molecule graph and on its k = 1 ego graph, heads = 4,
training mode (dropout drawn on the device):
  * every C entry point of one layer timed alone (device events around single
    calls: warm-up, then --reps timed repeats; median, min, p10, p90);
  * one GraphTransformerLayer and the whole 5-layer Transformer, forward +
    backward, eager and as a replayed graph, on the HIP kernels and as a torch
    composition of the same math on the same device (F.linear, index_add over
    the edge list, F.layer_norm, F.dropout) with the same parameters.

  python tools/gt_bench.py --out profiles/gt_baseline/gt_bench.jsonl
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("s-cgib_amd")
ops, _lib = pkg.ops, pkg._lib

H, F2, HEADS = 64, 128, 4


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


# ---------------------------------------------------------------------------
# the torch composition
# ---------------------------------------------------------------------------
def torch_layer(h, src, dst, layer):
    n, heads = h.shape[0], layer.num_heads
    dh = H // heads
    a = layer.attention
    q, k, v = (F.linear(h, m.weight, m.bias).view(n, heads, dh) for m in (a.Q, a.K, a.V))
    e = (k[src] * q[dst]).sum(-1) / dh ** 0.5
    s = torch.exp(e.clamp(-5, 5))
    wv = torch.zeros_like(q).index_add(0, dst, s.unsqueeze(-1) * v[src])
    z = torch.zeros(n, heads, device=h.device).index_add(0, dst, s)
    attn = (wv / (z.unsqueeze(-1) + 1e-6)).reshape(n, H)
    h1 = layer.layer_norm1(h + layer.O(attn))
    r = F.dropout(F.relu(layer.FFN_layer1(h1)), 0.5, training=layer.training)
    return layer.layer_norm2(h1 + layer.FFN_layer2(r))


def torch_encoder(x, src, dst, enc):
    h = enc.embedding_h(x)
    for layer in enc.layers:
        h = torch_layer(h, src, dst, layer)
    return h


# ---------------------------------------------------------------------------
# forward + backward, eager and replayed
# ---------------------------------------------------------------------------
def make_step(fwd, module, x, gout):
    def step():
        for p in module.parameters():
            p.grad = None
        x.grad = None
        fwd().backward(gout)
    return step


def capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up (allocator, counters) off the capture
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)  # (for ops.graph_node_counts)
    with torch.cuda.graph(graph):
        step()
    nodes = ops.graph_node_counts(graph)["total"]
    graph.instantiate()
    return graph, nodes


def bench_pair(what, tag, g, module, x, gout, hip_fwd, torch_fwd, warm, reps, out):
    res = {}
    for impl, fwd in (("hip", hip_fwd), ("torch", torch_fwd)):
        step = make_step(fwd, module, x, gout)
        res[impl, "eager"] = timed(step, warm, reps)
        graph, res[impl, "nodes"] = capture(step)
        res[impl, "graph"] = timed(graph.replay, warm, reps)
        del graph
    for mode in ("eager", "graph"):
        for impl in ("hip", "torch"):
            r = dict(res[impl, mode])
            r.update(what=what, graph=tag, impl=impl, mode=mode, nodes=g.num_nodes(),
                     edges=g.num_edges(), heads=HEADS, graph_nodes=res[impl, "nodes"])
            out(r)
        out({"what": what, "graph": tag, "mode": mode,
             "torch_over_hip": res["torch", mode]["median_us"] / res["hip", mode]["median_us"]})


def bench_kernels(tag, g, layer, warm, reps, out):
    """Each C entry point of one layer alone (buffers as ops._GtLayer makes them)."""
    n, dev = g.num_nodes(), g.rowptr.device
    p, st = ops._p, ops._stream
    new = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=dev)
    wq, bq, wk, bk, wv, bv, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2 = \
        [t.detach().contiguous() for t in layer.gt_params()]
    h, gout = torch.randn(n, H, device=dev), torch.randn(n, H, device=dev)
    q, k, v, attn, z = new(n, H), new(n, H), new(n, H), new(n, H), new(n, HEADS)
    pre1, st1, h1 = new(n, H), new(n, 2), new(n, H)
    r, bits = new(n, F2), new(n, 4, dtype=torch.int32)
    pre2, st2, o = new(n, H), new(n, 2), new(n, H)
    rng, cnt = ops.dropout_state(dev), ops.counters(dev, "gt_dropout", 1)
    dp2, dr, dh1, dp1, dattn = new(n, H), new(n, F2), new(n, H), new(n, H), new(n, H)
    gg, dzs, dq, dk, dv, dh = new(n, H), new(n, HEADS), new(n, H), new(n, H), new(n, H), new(n, H)
    widths = [int(_lib.query("scgib_gt_slab_width", i)) for i in range(4)]
    ns = int(_lib.query("scgib_gt_slabs", n))
    slabs = [new(ns * w) for w in widths]
    wg = [new(w) for w in widths]
    d = g.dims
    calls = [
        ("qkv_fwd", lambda: _lib.call("scgib_gt_qkv_fwd", p(h), p(wq), p(bq), p(wk), p(bk), p(wv),
                                      p(bv), n, p(q), p(k), p(v), p(d), st())),
        ("attn_fwd", lambda: _lib.call("scgib_gt_attn_fwd", p(q), p(k), p(v), p(g.rowptr), p(g.col),
                                       n, HEADS, p(attn), p(z), None, p(d), st())),
        ("out_fwd", lambda: _lib.call("scgib_gt_out_fwd", p(attn), p(h), p(wo), p(bo), p(g1),
                                      p(be1), n, p(pre1), p(st1), p(h1), p(d), st())),
        ("ffn_fwd (2 launches)", lambda: _lib.call(
            "scgib_gt_ffn_fwd", p(h1), p(w1), p(b1), p(w2), p(b2), p(g2), p(be2), n, 1, p(rng),
            p(cnt), None, p(r), p(bits), None, None, p(pre2), p(st2), p(o), p(d), st())),
        ("ffn_bwd (2 launches)", lambda: _lib.call(
            "scgib_gt_ffn_bwd", p(gout), p(pre2), p(st2), p(g2), p(r), p(bits), 1, p(h1), p(w1),
            p(w2), n, p(dp2), p(dr), p(dh1), p(slabs[0]), p(slabs[1]), p(d), st())),
        ("out_bwd", lambda: _lib.call("scgib_gt_out_bwd", p(dh1), p(pre1), p(st1), p(g1), p(attn),
                                      p(wo), n, p(dp1), p(dattn), p(slabs[2]), p(d), st())),
        ("attn_bwd (2 launches)", lambda: _lib.call(
            "scgib_gt_attn_bwd", p(dattn), p(attn), p(z), p(q), p(k), p(v), p(g.rowptr), p(g.col),
            p(g.rowptr_t), p(g.col_t), n, HEADS, p(gg), p(dzs), p(dq), p(dk), p(dv), p(d), st())),
        ("qkv_bwd", lambda: _lib.call("scgib_gt_qkv_bwd", p(dq), p(dk), p(dv), p(h), p(wq), p(wk),
                                      p(wv), p(dp1), n, p(dh), p(slabs[3]), p(d), st())),
        ("slab_reduce", lambda: ops._reduce_jobs(
            [_lib.SlabJob(slabs[i].data_ptr(), wg[i].data_ptr(), widths[i], ns, 0)
             for i in range(4)], st())),
    ]
    for name, fn in calls:  # in layer order: every call reads what the earlier ones wrote
        rec = timed(fn, warm, reps)
        rec.update(what="kernel", launch=name, graph=tag, nodes=n, edges=g.num_edges(), heads=HEADS)
        out(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--molecules", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gt_bench: needs the HIP device (nothing is measured on a CPU)")
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
    torch.manual_seed(0)
    ops.seed_dropout(dev, 1)
    enc = pkg.models.Transformer(32, H, 4, HEADS, dev).to(dev).train()
    layer = enc.layers[0]
    for tag, gr in (("molecules", g), ("ego_k1", ego)):
        n = gr.num_nodes()
        src, dst = gr.edges()
        bench_kernels(tag, gr, layer, a.warmup, a.reps, out)
        x = torch.randn(n, H, device=dev, requires_grad=True)
        gout = torch.randn(n, H, device=dev)
        bench_pair("layer", tag, gr, layer, x, gout, lambda: ops.gt_layer(x, gr, layer),
                   lambda: torch_layer(x, src, dst, layer), a.warmup, a.reps, out)
        x0 = torch.randn(n, 32, device=dev, requires_grad=True)
        bench_pair("encoder", tag, gr, enc, x0, gout, lambda: enc(gr, x0),
                   lambda: torch_encoder(x0, src, dst, enc), a.warmup, a.reps, out)


if __name__ == "__main__":
    main()
