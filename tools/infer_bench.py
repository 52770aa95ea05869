"""The captured score step on both paths of infer.Scorer (DESIGN.md §29,
profiles/infer_baseline/): ``"layers"`` — the existing eval forward of
Mainmodel_finetuning — and ``"resident"`` — ego build, noise draw, ONE
scgib_infer_fwd, predict head.

Every figure is the median over ``--windows`` windows of ``--replays`` replays
of a captured HIP graph, timed by device events after a warm-up window; the
paths of one case are captured in one process and measured in turn.

  step ... one batch in capacity mode (GIN-64x5 fine-tune model, k = 1, the
           noise drawn on the device): QM9-like B = 1 / 32 / 512, molhiv-like
           B = 32
  pass ... the evaluation pass of DESIGN.md §19: 4,113 of 41,127 molhiv-like
           molecules at B = 512 over a graph.DeviceEvalLoader — load_next,
           collate_ahead, the score step, the row write by ids (where the
           measured tree has it) — per step and per pass (ceil(M / B) steps)

``--root`` points at the tree whose package is measured, so the same script
times the ``"layers"`` step on the parent commit (which has no resident path).

Usage:  python tools/infer_bench.py [--root DIR] [--cases step,pass] [--out FILE]
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


def capture(body):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    return graph


def timed(graph, replays, windows):
    """(median, min, max) microseconds per replay over ``windows`` windows."""
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


def normalised(mols):
    return [(ei, F.normalize(torch.from_numpy(np.asarray(x, np.float32))).numpy())
            for ei, x in mols]


def make_model(pkg, f_in, B, dev):
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=B, gin_layers=5, task="graph_classification",
                           dataset="ogbg-molhiv", device=dev)
    torch.manual_seed(0)
    inner = pkg.models.Mainmodel(args, f_in, 64, 4, 4, 1, "GIN")
    pre = pkg.models.Mainmodel_continue(args, f_in, 64, 4, 4, 1, 1, inner, "GIN")
    return pkg.models.Mainmodel_finetuning(args, f_in, 64, 4, 4, 1, 1, pre, "GIN").to(dev).eval()


def score_bodies(pkg, model, static, dev, paths):
    """path -> the score step over ``static`` (scores of the batch)."""
    bodies = {}
    if "layers" in paths:
        def layers():
            with torch.no_grad():
                scores = model(static.graph, static.x, None, None)[0]
            # (a forward without a backward leaves the ego chain's stream unjoined)
            torch.cuda.current_stream().wait_stream(pkg.models._side_stream(dev))
            return scores
        bodies["layers"] = layers
    if "resident" in paths:
        scorer = pkg.infer.Scorer(model, "resident")
        bodies["resident"] = lambda: scorer.score(static.graph, static.x)
    return bodies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--cases", default="step,pass")
    ap.add_argument("--paths", default="layers,resident")
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--molecules", type=int, default=41127)
    ap.add_argument("--subset", type=int, default=4113)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="head")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infer_bench: needs the HIP device (nothing is measured on a CPU)")
    sys.path.insert(0, os.path.abspath(a.root))
    pkg = importlib.import_module("s-cgib_amd")
    dev = torch.device("cuda", 0)
    has_resident = os.path.exists(os.path.join(a.root, "s-cgib_amd", "infer.py"))
    paths = [p for p in a.paths.split(",") if p == "layers" or (p == "resident" and has_resident)]
    lines = []

    def emit(**rec):
        rec = dict(tag=a.tag, replays=a.replays, windows=a.windows, **rec)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    pkg.ops.seed_noise(dev, 1)
    if "step" in a.cases.split(","):
        for workload, B in (("qm9", 1), ("qm9", 32), ("qm9", 512), ("molhiv", 32)):
            gh, _ = pkg.graph.collate_pyg(normalised(pkg.synth.molecules(B, workload, seed=0)))
            caps = pkg.graph.StaticBatch.capacities([gh], 1, slack=1.1)
            static = pkg.graph.StaticBatch(B, caps[0], caps[1], gh.ndata["x"].shape[1], caps[2],
                                           caps[3], dev, 1)
            static.load(static.pad(gh))
            model = make_model(pkg, gh.ndata["x"].shape[1], B, dev)
            graphs = {p: capture(b) for p, b in score_bodies(pkg, model, static, dev, paths).items()}
            for p, graph in graphs.items():
                med, lo, hi = timed(graph, a.replays, a.windows)
                emit(what="score step", workload=workload, B=B, path=p, us=med, us_min=lo,
                     us_max=hi, rows=gh.num_nodes(), edges=gh.num_edges())
            del graphs
    if "pass" in a.cases.split(","):
        B = 512
        mols = normalised(pkg.synth.molecules(a.molecules, "molhiv", seed=0))
        ds = pkg.graph.DeviceDataset.from_molecules(mols, dev, 1, drop_single_atom=True)
        idx = np.sort(np.random.default_rng(0).permutation(len(ds))[:a.subset])
        caps = ds.capacities(B, "sequential", indices=idx)
        model = make_model(pkg, ds.num_features, B, dev)
        store = hasattr(pkg.ops, "infer_store")
        for p in paths:
            static = pkg.graph.StaticBatch(B, caps[0], caps[1], ds.num_features, caps[2], caps[3],
                                           dev, 1)
            evl = pkg.graph.DeviceEvalLoader(ds, static, indices=idx)
            evl.prime()
            out = torch.full((len(ds), 1), float("nan"), device=dev)
            score = score_bodies(pkg, model, static, dev, [p])[p]

            def body():
                static.load_next(evl.pool)
                evl.collate_ahead()
                scores = score()
                if store:
                    pkg.ops.infer_store(scores, evl.ids, out)

            graph = capture(body)
            med, lo, hi = timed(graph, a.replays, a.windows)
            emit(what="eval pass", workload="molhiv", B=B, path=p, molecules=len(ds),
                 subset=len(idx), steps=evl.steps, row_write=store, us_per_step=med,
                 us_per_step_min=lo, us_per_step_max=hi, ms_per_pass=med * evl.steps / 1e3,
                 loader_error=evl.error(), ego_error=static.ego_error())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
