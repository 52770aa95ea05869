"""What the readout_f / useAtt modes cost: the replayed pretrain step at QM9
B = 512, GIN-64 x 5, k = 1, in four modes.

  sum/att ........... readout_f="sum", useAtt=1 (the baseline)
  set2set/att ....... readout_f="set2set": both Set2Set readouts in one launch
                      per direction (ops.set2set_pair), contrastive loss at
                      width 128 in launches of its own
  sum/no-att ........ useAtt=0: the interaction kernels without the attention
  set2set/two-calls . set2set with models.S2S_PAIR off: two ops.set2set calls

The model is a plain Mainmodel (Mainmodel_continue takes z1 through its own
Set2Set and z2 through the wrapped model's: two LSTMs, always two calls).  The
step is bench.py's own (build_replay_step: capacity mode, a pool of 8 resident
batches, ego-net and noise prefetch, forward + backward + Adam in one captured
graph, the split replay where the hand-off rule allows).  Every mode runs in a
fresh child process, one at a time: 5 warm-up steps, then 300 timed steps with
a host clock around a synchronise, as README's long runs.  ``--mode contrast``
times the stand-alone contrastive op (forward + backward) at widths 64 and 128,
B = 512, with device events over back-to-back launches; under a kernel trace
of that child the two widths' kernels are the template instances
contrast_fwd_k<64> / <128> and contrast_bwd_k<64> / <128>.  No bar: nobody has
measured these modes.

  python tools/readout_bench.py --out profiles/readout_baseline/readout_bench.jsonl
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"sum/att": ("sum", 1, True), "set2set/att": ("set2set", 1, True),
         "sum/no-att": ("sum", 0, True), "set2set/two-calls": ("set2set", 1, False)}
B, K, LAYERS, POOL = 512, 1, 5, 8


def run_mode(mode, warmup, steps):
    import bench  # bench.py's own replayed step
    pkg = bench.pkg
    readout_f, use_att, pair = MODES[mode]
    pkg.models.S2S_PAIR = pair
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ok, why = pkg.ops.handoff_rule(torch.cuda.device_count(), dict(os.environ, LOCAL_WORLD_SIZE="1"))
    pkg.ops.XQ_FLAGS, pkg.ops.XQ_REASON = ok, why
    torch.manual_seed(1234)
    pool_host = [pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=i))[0]
                 for i in range(POOL)]
    f_in = pkg.synth.WORKLOADS["qm9"][2]
    args = SimpleNamespace(recons_type="adj", useAtt=use_att, readout_f=readout_f, d_transfer=32,
                           batch_size=B, gin_layers=LAYERS, task="graph_classification")
    model = pkg.models.Mainmodel(args, f_in, 64, 4, 4, K, "GIN").to(dev).train()
    opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
    rs = bench.build_replay_step(model, opt, pool_host, K, B, dev)
    for i in range(warmup):
        rs.step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss = rs.step(warmup + i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    kl, rec, con = (float(v) for v in loss)
    nodes = rs.graph_nodes or {}
    return {"what": "readout_pretrain_step", "mode": mode, "readout_f": readout_f,
            "useAtt": use_att, "s2s_pair": pair, "B": B, "layers": LAYERS, "k": K,
            "warmup": warmup, "steps": steps, "ms_per_step": ms,
            "graph_kernel_nodes": nodes.get("kernel"), "split_replay": rs.split is not None,
            "losses": {"kl": kl, "recon": rec, "contrastive": con},
            "losses_finite": all(map(lambda v: v == v and abs(v) != float("inf"), (kl, rec, con)))}


def run_contrast(reps=200):
    pkg = importlib.import_module("s-cgib_amd")
    dev = torch.device("cuda", 0)
    out = []
    for width in (64, 128):
        gen = torch.Generator().manual_seed(width)
        z1 = torch.randn(B, width, generator=gen).to(dev).requires_grad_(True)
        z2 = torch.randn(B, width, generator=gen).to(dev).requires_grad_(True)
        cnt = pkg.ops.counters(dev, "contrastive",
                               int(pkg._lib.query("scgib_contrastive_counters", B)))
        ws = torch.empty(int(pkg._lib.query("scgib_contrastive_workspace_floats_w", B, width)),
                         device=dev)
        loss, g = torch.empty((), device=dev), torch.ones(1, device=dev)
        dz1, dz2 = torch.empty_like(z1), torch.empty_like(z2)
        p, st = pkg.ops._p, pkg.ops._stream

        def fwd():
            pkg._lib.call("scgib_contrastive_fwd_w", p(z1), p(z2), B, width, p(ws), p(loss),
                          p(cnt), st())

        def bwd():
            pkg._lib.call("scgib_contrastive_bwd_w", p(z1), p(z2), B, width, p(ws), p(g), p(dz1),
                          p(dz2), p(cnt), st())

        us = {}
        for name, fn in (("fwd", fwd), ("bwd", bwd)):
            for _ in range(20):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            us[name] = a.elapsed_time(b) / reps * 1e3
        out.append({"what": "contrastive_op", "width": width, "B": B, "reps": reps,
                    "timing": "device events over back-to-back launches (launch gaps included)",
                    "fwd_us": us["fwd"], "bwd_us": us["bwd"], "loss": float(loss)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", default=None, help="child: one of the modes, or 'contrast'")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("readout_bench: needs the HIP device (nothing is measured on a CPU)")
    if a.mode == "contrast":
        for rec in run_contrast():
            print(json.dumps(rec), flush=True)
        return
    if a.mode is not None:
        print(json.dumps(run_mode(a.mode, a.warmup, a.steps)), flush=True)
        return
    lines = []
    for mode in list(MODES) + ["contrast"]:  # one fresh process per mode, one at a time
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--warmup",
                            str(a.warmup), "--steps", str(a.steps)], capture_output=True,
                           text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"readout_bench: mode {mode!r} ended with status {r.returncode}")
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        for ln in got:
            print(ln, flush=True)
        lines += got
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
