"""A/B of the replayed Transformer pretrain step: models.GT_FOLD on against off.

The step is Mainmodel_continue around Mainmodel, encoder="Transformer", 4 + 1
layers, 4 heads, k = 1, on synthetic QM9-like molecules at B = 512 and B = 128,
training mode (dropout and compression noise drawn on the device): forward +
backward + optim.Adam captured in one torch.cuda.graph.  Both variants are
captured in one process, each in its own graph over its own model (the same
initial weights), and replayed in alternation: after --warmup replays each,
--rounds rounds of --replays replays per variant, timed with a host clock
around a synchronise.  One JSON line per (B, variant) with the median and
[min, max] of the per-round means and the graph's node counts, one line with
the comparison, and after the timing one line per variant on whether
ops.SplitGraph accepts the captured step (its message when it does not; the
split is built, never replayed: nothing is required of it here).  No bar:
nobody has timed this step.

  python tools/gt_step_bench.py --out profiles/gt_fold/gt_step_bench.jsonl
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
ops, models = pkg.ops, pkg.models
models.ALL_ENCODER_STRINGS = True  # encoder="Transformer" by string

LAYERS, HEADS, K = 4, 4, 1


def make_model(f_in, b, dev):
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=b, gin_layers=5, task="graph_classification", device=dev)
    torch.manual_seed(0)
    inner = models.Mainmodel(args, f_in, 64, LAYERS, HEADS, K, "Transformer")
    model = models.Mainmodel_continue(args, f_in, 64, LAYERS, HEADS, K, 1, inner, "Transformer")
    return model.to(dev).train()


def capture(fold, g, x, b, dev):
    """The step of one variant as a captured graph: (graph, losses, node counts, keep-alive).
    (models.GT_FOLD is read when the step is enqueued, so at capture only.)"""
    models.GT_FOLD = fold
    model = make_model(x.shape[1], b, dev)
    opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
    one = torch.ones((), device=dev)

    def body():
        _, kl, con, rec = model(g, x, None, None, None, 1, None, K, dev, b)
        torch.autograd.backward((kl, rec, con), (one, one, one))
        opt.step()
        return torch.stack([kl.detach(), con.detach(), rec.detach()])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up (allocator, counters, Adam state) off the capture
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)  # (for ops.graph_node_counts / SplitGraph)
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        losses = body()
    nodes = ops.graph_node_counts(graph)
    graph.instantiate()
    return graph, losses, nodes, (model, opt, one)


def try_split(graph, dev):
    """Whether ops.SplitGraph takes the captured step (built, never replayed)."""
    if not ops.xq_enabled():
        return None, f"not tried: hand-offs off here ({ops.XQ_REASON})"
    try:
        lanes = ops.SplitGraph(graph, dev)
    except ops.SplitUnsupported as e:
        return False, str(e)
    info = dict(lanes.info)
    lanes.close()
    return True, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=[512, 128])
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--replays", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gt_step_bench: needs the HIP device (nothing is measured on a CPU)")
    if a.rounds < 6 or a.replays < 100 or a.warmup < 50:
        raise SystemExit("gt_step_bench: at least 6 rounds of 100 replays after 50 warm-up replays")
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

    default_fold = bool(models.GT_FOLD)
    for b in a.batches:
        gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(b, "qm9", seed=0))
        g = gh.to(dev)
        x = F.normalize(g.ndata["x"].float())
        ops.seed_noise(dev, 1)
        ops.seed_dropout(dev, 2, lane=0)
        ops.seed_dropout(dev, 3, lane=1)
        runs = {}
        for fold in (True, False):
            runs[fold] = capture(fold, g, x, b, dev)
        for fold in (True, False):
            for _ in range(a.warmup):
                runs[fold][0].replay()
        torch.cuda.synchronize()
        us = {True: [], False: []}
        for _ in range(a.rounds):
            for fold in (True, False):  # the variants alternate
                graph = runs[fold][0]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.replays):
                    graph.replay()
                torch.cuda.synchronize()
                us[fold].append((time.perf_counter() - t0) / a.replays * 1e6)
        for fold in (True, False):
            graph, losses, nodes, _keep = runs[fold]
            t = np.asarray(us[fold])
            out({"what": "transformer_pretrain_step", "B": b, "gt_fold": fold,
                 "nodes": g.num_nodes(), "layers": LAYERS + 1, "heads": HEADS, "k": K,
                 "rounds": a.rounds, "replays": a.replays, "warmup": a.warmup,
                 "median_us": float(np.median(t)), "min_us": float(t.min()),
                 "max_us": float(t.max()), "round_us": [float(v) for v in t],
                 "graph_kernel_nodes": nodes.get("kernel", 0), "graph_nodes": nodes,
                 "losses_finite": bool(torch.isfinite(losses).all())})
        on, off = np.median(us[True]), np.median(us[False])
        spread = float(np.max(us[False]) - np.min(us[False]))
        out({"what": "transformer_pretrain_step_ab", "B": b, "on_over_off": float(on / off),
             "on_minus_off_us": float(on - off), "off_spread_us": spread,
             "fold_stays_on": bool(on - off <= spread)})
        for fold in (True, False):  # after the timing: the split is built, never replayed
            accepted, message = try_split(runs[fold][0], dev)
            out({"what": "transformer_pretrain_step_split", "B": b, "gt_fold": fold,
                 "split_accepted": accepted, "split_message": message})
        del runs
    models.GT_FOLD = default_fold


if __name__ == "__main__":
    main()
