"""The optimizer stage alone, by value against the device-hyper modes
(DESIGN.md §24): optim.Adam.step() on the pretraining model's real tensor
table (Mainmodel_continue, GIN-64x5, QM9 feature width: the parameters one real
pretrain backward on 64 synthetic molecules gives a gradient, with those
gradients resident), captured as a HIP graph of that stage and replayed.

  by_value   optim.Adam(lr, weight_decay=5e-5): scgib_adam_step, the launch
             the parent commit has (same instructions: profiles/optim_dyn/
             resources.txt)
  schedule   + Schedule("cosine", warm-up): scgib_adam_step_dyn, one launch
  sched_clip + max_grad_norm: scgib_grad_norm, then scgib_adam_step_dyn

--runs runs per arm, the arms alternating in one process; a run is --replays
replays between two device synchronises on a host clock (the replays are
enqueued back to back, so a run measures the stage's device time plus what
the graph launch does not hide).  One line per run and one summary line per
arm (median, min, max of the per-replay time).

  python tools/optim_dyn_ab.py --out profiles/optim_dyn/ab.jsonl
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("s-cgib_amd")


def build_model(dev):
    F_in = pkg.synth.WORKLOADS["qm9"][2]
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=64, gin_layers=5, task="graph_classification")
    torch.manual_seed(0)
    inner = pkg.models.Mainmodel(args, F_in, 64, 4, 4, 1, "GIN")
    return pkg.models.Mainmodel_continue(args, F_in, 64, 4, 4, 1, 1, inner, "GIN").to(dev).train()


def real_gradients(model, dev):
    """One pretrain forward + backward (exp_pretraining.py:290-323) on 64
    synthetic QM9 molecules; returns the parameters that received a gradient,
    each with a private copy of it."""
    g = pkg.graph.collate_pyg(pkg.synth.molecules(64, "qm9", seed=0))[0].to(dev)
    x = F.normalize(g.ndata["x"].float())
    n = g.num_nodes()
    gen = torch.Generator().manual_seed(1)
    noise = (torch.rand(n, generator=gen).to(dev), torch.rand(n, 64, generator=gen).to(dev))
    _, kl, con, rec = model(g, x, None, None, None, 1, None, 1, dev, 64, noise=noise)
    (kl + con + rec).backward()
    params = [p for p in model.parameters() if p.grad is not None]
    for p in params:
        p.grad = p.grad.detach().clone()
    return params


def build_arm(name, dev):
    model = build_model(dev)
    params = real_gradients(model, dev)
    kw = {}
    if name != "by_value":
        kw["schedule"] = pkg.optim.Schedule("cosine", warmup=100, total=1_000_000, min_ratio=0.1)
    if name == "sched_clip":
        kw["max_grad_norm"] = 1.0
    opt = pkg.optim.Adam(params, lr=1e-4, weight_decay=5e-5, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # state and blocks outside the capture
        for _ in range(3):
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    return SimpleNamespace(name=name, model=model, opt=opt, graph=graph,
                           tensors=len(params), elements=sum(p.numel() for p in params))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--replays", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_dyn_ab: needs the GPU (no CPU fallback)")
    dev = torch.device("cuda", 0)
    arms = [build_arm(n, dev) for n in ("by_value", "schedule", "sched_clip")]
    lines, per = [], {arm.name: [] for arm in arms}
    for arm in arms:
        for _ in range(a.warmup):
            arm.graph.replay()
    torch.cuda.synchronize()
    for run in range(a.runs):
        for arm in arms:  # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.replays):
                arm.graph.replay()
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / a.replays * 1e6
            per[arm.name].append(us)
            lines.append({"kind": "run", "arm": arm.name, "run": run, "replays": a.replays,
                          "us_per_replay": round(us, 4)})
    for arm in arms:
        v = per[arm.name]
        finite = all(bool(torch.isfinite(p).all()) for p in arm.model.parameters())
        lines.append({"kind": "summary", "arm": arm.name, "tensors": arm.tensors,
                      "elements": arm.elements, "runs": a.runs, "replays": a.replays,
                      "median_us": round(statistics.median(v), 4), "min_us": round(min(v), 4),
                      "max_us": round(max(v), 4), "params_finite": finite,
                      "device": torch.cuda.get_device_name(dev)})
    text = "\n".join(json.dumps(line) for line in lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    sys.stdout.write("".join(json.dumps(line) + "\n" for line in lines if line["kind"] == "summary"))


if __name__ == "__main__":
    main()
