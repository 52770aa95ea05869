"""Class-index cross-entropy on the device (ops.class_loss):
the two measurements its section records.

  step  the captured Mutagenicity fine-tune step (batch load, forward,
        loss_CrossEntropy on int64 targets, backward, Adam) at each --batches
        size, replayed --replays times per run, --runs runs per arm, the arms
        alternating in one process:
          torch   models.DEVICE_CE off: F.cross_entropy, the step as it was
          device  models.DEVICE_CE on: ops.class_loss
  pass  one evaluation pass over --subset molecules of a resident dataset at
        --eval-batch, the forward captured and fed by graph.DeviceEvalLoader:
          host    per batch F.cross_entropy + metrics.accuracy_TU with their
                  .item() reads (train_tudataset.py:196-221)
          device  loss_CrossEntropy(..., epoch=ClassEpoch) inside the captured
                  step and the epoch's single read

Times are a host clock around work that ends in a device synchronise.

  python tools/ce_bench.py --out profiles/ce_baseline/ce_bench.jsonl
"""
import argparse
import copy
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("s-cgib_amd")
import finetune_bench  # noqa: E402

G = pkg.graph
WORKLOAD, DATASET, CLASSES = "mutagenicity", "Mutagenicity", 2


def build_step(ft, host, targets, k, B, dev, device_ce):
    """The captured train step over a resident pool of ``host`` batches;
    returns replay() and the static loss."""
    opt = pkg.optim.Adam(ft.parameters(), lr=1e-3, weight_decay=1e-5)
    n_cap, e_cap, mgn, caps = G.StaticBatch.capacities(host, k, slack=1.02)
    static = G.StaticBatch(B, n_cap, e_cap, host[0].ndata["x"].shape[1], mgn, caps, dev, k=k)
    padded = []
    for gh in host:
        gx = G.GraphBatch.from_edges(*[t.numpy() for t in gh.edges()], gh.num_nodes(), True,
                                     gh.batch_num_nodes_host())
        dict.__setitem__(gx.ndata, "x", F.normalize(gh.ndata["x"].float()))
        padded.append(static.pad(gx))
    pool = static.pool(padded)
    pf = G.EgoPrefetch(static, pool)
    pf.prime()
    tg = targets.to(dev)
    one = torch.ones((), dtype=torch.float32, device=dev)

    def body():
        pkg.models.DEVICE_CE = device_ce
        try:
            static.load_next(pool, pf)
            scores, *_ = ft(static.graph, static.x, None, None, 1, None, 2, dev, B)
            loss = ft.loss_CrossEntropy(scores, tg)
            torch.autograd.backward(loss, one)
            pf.join()
        finally:
            pkg.models.DEVICE_CE = False
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            body()
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    opt.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = body()
        opt.step()
    return graph.replay, loss, (static, pool, pf, padded, tg, one, opt, graph)


def bench_step(a, dev, out):
    F_in = pkg.synth.WORKLOADS[WORKLOAD][2]
    for B in (int(b) for b in a.batches.split(",")):
        base, k = finetune_bench.make_finetune_model(pkg, F_in, B, dev, seed=5, dataset=DATASET,
                                                     num_classes=CLASSES)
        host = [G.collate_pyg(pkg.synth.molecules(B, WORKLOAD, seed=500 + i))[0]
                for i in range(a.pool)]
        targets = torch.randint(0, CLASSES, (B, 1), generator=torch.Generator().manual_seed(7))
        arms, early = {}, {}
        for name in ("torch", "device", "control"):
            # the same noise stream from the first warm-up step on, so the arms
            # train the same model until rounding separates them; "control" is
            # the torch arm built a second time (what a rebuild alone changes)
            pkg.ops.seed_noise(dev, 11)
            arms[name] = build_step(copy.deepcopy(base), host, targets, k, B, dev, name == "device")
            early[name] = []
            for _ in range(a.agree_steps):
                arms[name][0]()
                early[name].append(float(arms[name][1]))
        del arms["control"]
        out(dict(what="step_agreement", batch=B, loss_torch=early["torch"],
                 loss_device=early["device"], loss_torch_again=early["control"]))
        for replay, _, _ in arms.values():
            for _ in range(a.warmup):
                replay()
        torch.cuda.synchronize()
        per = {name: [] for name in arms}
        for _ in range(a.runs):
            for name, (replay, _, _) in arms.items():  # alternating in one process
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.replays):
                    replay()
                torch.cuda.synchronize()
                per[name].append((time.perf_counter() - t0) / a.replays * 1e6)
        for name, (_, loss, _) in arms.items():
            out(dict(what="step", arm=name, batch=B, replays=a.replays, runs_us_per_step=per[name],
                     median_us=float(np.median(per[name])),
                     spread_us=max(per[name]) - min(per[name]), final_loss=float(loss)))
        out(dict(what="step_delta", batch=B,
                 device_minus_torch_us=float(np.median(per["device"]) - np.median(per["torch"])),
                 torch_spread_us=max(per["torch"]) - min(per["torch"])))
        del arms


def build_pass(feed, ds, caps, idx, model, B, k, dev):
    static = G.StaticBatch(B, caps[0], caps[1], ds.num_features, caps[2], caps[3], dev, k)
    evl = G.DeviceEvalLoader(ds, static, indices=idx)
    evl.prime()
    pf = G.EgoPrefetch(static, evl.pool)
    pf.prime()
    ep = pkg.metrics.ClassEpoch(dev)
    box = {}

    def body():
        static.load_next(evl.pool, pf)
        evl.collate_ahead()
        with torch.no_grad():
            scores, *_ = model(static.graph, static.x, None, None, 1, None, k, dev, B)
            if feed == "device":
                model.loss_CrossEntropy(scores, evl.labels, epoch=ep)
        pf.join()
        box["scores"] = scores

    def rewind():
        evl.prime()
        pf.prime()
        ep.reset()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    rewind()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    scores = box["scores"]

    def one_pass():
        if feed == "device":
            for _ in range(evl.steps):
                graph.replay()
            r = ep.result()  # the pass's one read
            ep.reset()
            return r["loss"], r["acc"]
        loss, acc, rows = 0.0, 0, 0
        for _ in range(evl.steps):  # train_tudataset.py:196-221
            graph.replay()
            targets = evl.labels.long()
            loss += F.cross_entropy(scores, targets.squeeze(-1)).detach().item()
            acc += pkg.metrics.accuracy_TU(scores, targets)
            rows += targets.size(0)
        return loss / evl.steps, acc / rows

    return one_pass, evl.steps, (static, evl, pf, graph)


def bench_pass(a, dev, out):
    B, k = a.eval_batch, 1
    if a.subset % B:
        raise SystemExit("ce_bench: --subset must be a multiple of --eval-batch (the host arm "
                         "casts every label to long: it cannot take fill rows)")
    mols = pkg.synth.molecules(a.molecules, WORKLOAD, seed=0)
    rng = np.random.default_rng(0)
    y = rng.integers(0, CLASSES, size=(len(mols), 1)).astype(np.float32)
    ds = G.DeviceDataset.from_molecules(mols, dev, k, labels=y)
    idx = np.sort(rng.permutation(len(ds))[:a.subset])
    caps = ds.capacities(B, "sequential", indices=idx)
    model, _ = finetune_bench.make_finetune_model(pkg, ds.num_features, B, dev, seed=5,
                                                  dataset=DATASET, num_classes=CLASSES)
    model.eval()
    arms = {feed: build_pass(feed, ds, caps, idx, model, B, k, dev) for feed in ("host", "device")}
    for one_pass, _, _ in arms.values():
        for _ in range(2):
            one_pass()
    per, res = {feed: [] for feed in arms}, {}
    for _ in range(a.rounds):
        for feed, (one_pass, _, _) in arms.items():  # alternating in one process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[feed] = one_pass()
            per[feed].append((time.perf_counter() - t0) * 1e3)
    for feed, (_, steps, _) in arms.items():
        out(dict(what="pass", arm=feed, batch=B, molecules=len(idx), steps=steps,
                 passes_ms=per[feed], median_ms=float(np.median(per[feed])),
                 per_step_us=float(np.median(per[feed])) / steps * 1e3,
                 loss=res[feed][0], acc=res[feed][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="32,64")
    ap.add_argument("--pool", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--agree-steps", type=int, default=20)
    ap.add_argument("--molecules", type=int, default=4337)  # Mutagenicity's size
    ap.add_argument("--subset", type=int, default=4032)
    ap.add_argument("--eval-batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="step,pass")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ce_bench: needs the HIP device (nothing is measured on a CPU)")
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

    if "step" in a.only.split(","):
        bench_step(a, dev, out)
    if "pass" in a.only.split(","):
        bench_pass(a, dev, out)


if __name__ == "__main__":
    main()
