"""The host's launch sequence as data: every ``_lib.call`` of a step, in order.

``Recorder`` notes, per call, the entry name, every scalar argument (ints
exact, floats by ``repr``), for every pointer / by-reference argument only
whether it is NULL, for a slab-job table (``_reduce_jobs``, the fused Adam
entries, the GIN fold arguments) each job's ``(width, n_slabs, stride)``, the
``meta`` dict of a call routed through ``ops._launch`` and the label of a
stamp.  No addresses.  ``CASES`` are the steps whose sequence
tests/golden/launch_trace.json pins (test_gpu_launch_trace.py);

    python tests/launch_trace.py --write

regenerates the fixture on a HIP device.
"""
import contextlib
import ctypes
import importlib
import json
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_trace.json")
B, F_IN = 48, 11

# entry -> [(index of the job pointer, index of the job count or None = one
# job by reference)]; negative indices count from the end (the stream is last)
JOB_ARGS = {
    "scgib_slab_reduce_multi": [(0, 1)],
    "scgib_slab_reduce_multi_ex": [(0, 1)],
    "scgib_adam_step_reduce": [(2, 3)],
    "scgib_adamw_step_reduce": [(2, 3)],
    "scgib_adam_step_reduce_dyn": [(2, 3)],
    "scgib_gin_bwd_stats_bn_fold": [(-2, None)],
    "scgib_gin_bwd_stats_z": [(-3, -2)],
    "scgib_gin_layer_bwd_z": [(-3, None), (-2, None)],
}


def _address(arg):
    if arg is None:
        return 0
    if isinstance(arg, int):
        return arg
    if not isinstance(arg, ctypes.c_void_p):
        arg = ctypes.cast(arg, ctypes.c_void_p)
    return arg.value or 0


class Recorder:
    """Context manager: ``calls`` holds one JSON-able record per _lib.call."""

    def __init__(self, pkg):
        self.pkg, self.calls, self._meta = pkg, [], None

    def _describe(self, name, args):
        lib = self.pkg._lib
        kinds = lib.SIGNATURES[name][1]
        assert len(kinds) == len(args), name
        tables = {i % len(args): c for i, c in JOB_ARGS.get(name, ())}
        out = []
        for i, (kind, arg) in enumerate(zip(kinds, args)):
            if kind is not ctypes.c_void_p:
                out.append(repr(float(arg)) if kind in (ctypes.c_float, ctypes.c_double)
                           else int(arg))
            elif not _address(arg):
                out.append("NULL")
            elif i in tables:
                count = 1 if tables[i] is None else int(args[tables[i]])
                jobs = ctypes.cast(ctypes.c_void_p(_address(arg)), ctypes.POINTER(lib.SlabJob))
                out.append({"jobs": [[int(jobs[j].width), int(jobs[j].n_slabs),
                                      int(jobs[j].stride)] for j in range(count)]})
            else:
                out.append("ptr")
        rec = {"entry": name, "args": out}
        if self._meta is not None:
            rec["meta"] = {k: (v if isinstance(v, (bool, int)) else repr(v))
                           for k, v in self._meta.items()}
        if name == "scgib_stamp":
            rec["label"] = self.pkg.ops._STAMPS["labels"][int(args[1])]
        return rec

    def __enter__(self):
        lib, ops = self.pkg._lib, self.pkg.ops
        self._call, self._observer = lib.call, ops.OBSERVER

        def call(name, *args):
            self.calls.append(self._describe(name, args))
            return self._call(name, *args)

        def observer(name, meta, launch):
            self._meta = meta
            try:
                return launch()
            finally:
                self._meta = None

        lib.call, ops.OBSERVER = call, observer
        return self

    def __exit__(self, *exc):
        self.pkg._lib.call, self.pkg.ops.OBSERVER = self._call, self._observer
        return False


@contextlib.contextmanager
def switches(ops, **values):
    old = {k: getattr(ops, k) for k in values}
    for k, v in values.items():
        setattr(ops, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


# ---------------------------------------------------------------------------
# the recorded steps
# ---------------------------------------------------------------------------
def _args(layers):
    return SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=B, gin_layers=layers, task="graph_classification")


def _pretrain(pkg, dev, layers=4, wrapped=False):
    torch.manual_seed(11)
    m = pkg.models.Mainmodel(_args(layers), F_IN, 64, 4, 4, 1, "GIN")
    if wrapped:
        m = pkg.models.Mainmodel_continue(_args(layers), F_IN, 64, 4, 4, 1, 1, m, "GIN")
    return m.to(dev).train()


def _batch(pkg, seed=9):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=seed))
    dict.__setitem__(gh.ndata, "x", F.normalize(gh.ndata["x"].float()))
    return gh


def _noise(n, dev, seed=100):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(n, device=dev, generator=gen), torch.rand(n, 64, device=dev, generator=gen))


def _fwd_bwd(model, g, x, noise, dev):
    _, kl, con, rec = model(g, x, None, None, None, 1, None, 1, dev, B, noise=noise)
    (kl + con + rec).backward()


def _pretrain_case(layers=4, wrapped=False, freeze=False, **sw):
    """One eager exact-mode pretraining step (after an unrecorded one)."""
    def run(pkg, dev, rec):
        model = _pretrain(pkg, dev, layers, wrapped)
        g = _batch(pkg).to(dev)
        noise = _noise(g.num_nodes(), dev)
        with switches(pkg.ops, **sw):
            _fwd_bwd(model, g, g.ndata["x"], noise, dev)
            model.zero_grad(set_to_none=True)
            with rec:
                _fwd_bwd(model, g, g.ndata["x"], noise, dev)
    return run


def _stamped(pkg, dev, rec):
    ops = pkg.ops
    model = _pretrain(pkg, dev)
    g = _batch(pkg).to(dev)
    noise = _noise(g.num_nodes(), dev)
    _fwd_bwd(model, g, g.ndata["x"], noise, dev)
    model.zero_grad(set_to_none=True)
    old = dict(ops._STAMPS)
    ops.stamps_enable(dev, level=2)
    try:
        with rec:
            _fwd_bwd(model, g, g.ndata["x"], noise, dev)
    finally:
        ops._STAMPS.update(old)


def _capacity_fused_adam(pkg, dev, rec):
    """Capacity mode, the final reduce left to optim.Adam.step."""
    model = _pretrain(pkg, dev)
    gh = _batch(pkg)
    n_cap, e_cap, mgn, caps = pkg.graph.StaticBatch.capacities([gh], 1, slack=1.05)
    static = pkg.graph.StaticBatch(B, n_cap, e_cap, F_IN, mgn, caps, dev)
    static.load(static.pad(gh))
    noise = _noise(n_cap, dev)
    opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
    for recorder in (contextlib.nullcontext(), rec):
        opt.zero_grad(set_to_none=True)
        with recorder, pkg.ops.fuse_final_into_step():
            _fwd_bwd(model, static.graph, static.x, noise, dev)
            opt.step()


def _accumulate(pkg, dev, rec):
    """Two backward passes into one step inside fuse_final_into_step: the
    second finds .grad set, so no final reduce is left to the step."""
    model = _pretrain(pkg, dev)
    g = _batch(pkg).to(dev)
    noise = _noise(g.num_nodes(), dev)
    opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
    for recorder in (contextlib.nullcontext(), rec):
        opt.zero_grad(set_to_none=True)
        with recorder, pkg.ops.fuse_final_into_step():
            _fwd_bwd(model, g, g.ndata["x"], noise, dev)
            _fwd_bwd(model, g, g.ndata["x"], noise, dev)
            opt.step()


def _gin_alone(training):
    def run(pkg, dev, rec):
        torch.manual_seed(12)
        gin = pkg.models.GIN(32, 64, 3).to(dev).train(training)
        g = _batch(pkg).to(dev)
        h0 = torch.randn(g.num_nodes(), 32, device=dev, requires_grad=True)
        w = torch.randn(g.num_nodes(), 64, device=dev)
        for recorder in (contextlib.nullcontext(), rec):
            gin.zero_grad(set_to_none=True)
            with recorder:
                (pkg.ops.gin_encoder(h0, g, gin) * w).sum().backward()
    return run


def _gin_x_mapped(pkg, dev, rec):
    """gin_encoder_x over the ego-nets through the node map, with a gradient
    from the rows and one from their per-ego-net sums."""
    torch.manual_seed(13)
    gin = pkg.models.GIN(32, 64, 3).to(dev).train()
    lin = torch.nn.Linear(F_IN, 32, bias=False).to(dev)
    g = _batch(pkg).to(dev)
    ego = pkg.graph.egonet_batch(g, 1)
    w = torch.randn(ego.num_nodes(), 64, device=dev)
    wr = torch.randn(ego.batch_size, 64, device=dev)
    for recorder in (contextlib.nullcontext(), rec):
        gin.zero_grad(set_to_none=True)
        lin.zero_grad(set_to_none=True)
        with recorder:
            out = pkg.ops.gin_encoder_x(g.ndata["x"], ego, gin, lin, ego.ndata["_ID"])
            ro = pkg.ops.segment_sum(out, ego.graph_ptr, ego.batch_size)
            ((out * w).sum() + (ro * wr).sum()).backward()


def _finetune(**sw):
    """Mainmodel_finetuning on the molhiv head (the reference's freezing)."""
    def run(pkg, dev, rec):
        import finetune_bench
        b = 8
        ft, _ = finetune_bench.make_finetune_model(pkg, 9, b, dev, seed=5)
        gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(b, "molhiv", seed=3))
        g = gh.to(dev)
        x = F.normalize(g.ndata["x"].float())
        noise = _noise(g.num_nodes(), dev)
        tgt = torch.randint(0, 2, (b, 1), generator=torch.Generator().manual_seed(4)).float().to(dev)
        with switches(pkg.ops, **sw):
            for recorder in (contextlib.nullcontext(), rec):
                ft.zero_grad(set_to_none=True)
                with recorder:
                    scores, *_ = ft(g, x, None, None, 1, None, 2, dev, b, noise=noise)
                    ft.loss(scores, tgt).backward()
    return run


def _gt_frozen_lower(pkg, dev, rec):
    torch.manual_seed(14)
    enc = pkg.models.Transformer(32, 64, 3, 4, dev).to(dev).train()
    td = torch.nn.Linear(F_IN, 32, bias=False).to(dev)
    for p in enc.layers[0].parameters():
        p.requires_grad = False
    g = _batch(pkg).to(dev)
    w = torch.randn(g.num_nodes(), 64, device=dev)
    for recorder in (contextlib.nullcontext(), rec):
        enc.zero_grad(set_to_none=True)
        td.zero_grad(set_to_none=True)
        pkg.ops.seed_dropout(dev, 99, 0, lane=0)
        with recorder:
            (pkg.ops.gt_encoder_x(g.ndata["x"], g, enc, td) * w).sum().backward()


CASES = {
    "pretrain_L4_exact": _pretrain_case(),
    "pretrain_L4_exact_stamps2": _stamped,
    "pretrain_L4_capacity_fused_adam": _capacity_fused_adam,
    "continue_L5": _pretrain_case(5, True),
    "no_defer_bn": _pretrain_case(DEFER_BN=False),
    "no_fold_slabs": _pretrain_case(FOLD_SLABS=False),
    "no_store_r": _pretrain_case(STORE_R=False),
    "no_defer_loss_reduce": _pretrain_case(DEFER_LOSS_REDUCE=False),
    "no_fuse_enc_tail": _pretrain_case(FUSE_ENC_TAIL=False),
    "agg_free_trainable": _pretrain_case(AGG_FREE_MIN_ROWS=0),
    "agg_free_reference_freezing": _finetune(AGG_FREE_MIN_ROWS=0),
    "accumulate_second_backward": _accumulate,
    "gin_encoder_h0_train": _gin_alone(True),
    "gin_encoder_h0_eval": _gin_alone(False),
    "gin_encoder_x_node_map_readout": _gin_x_mapped,
    "finetune_molhiv": _finetune(),
    "gt_encoder_x_frozen_lower_layer": _gt_frozen_lower,
}


def record(pkg, dev, name):
    rec = Recorder(pkg)
    CASES[name](pkg, dev, rec)
    torch.cuda.synchronize()
    return rec.calls


def dump(traces, path):
    """One call per line: a changed launch shows as one changed line."""
    with open(path, "w") as f:
        f.write("{\n")
        for i, (name, calls) in enumerate(traces.items()):
            f.write(f" {json.dumps(name)}: [\n")
            f.write(",\n".join("  " + json.dumps(c, sort_keys=True) for c in calls))
            f.write("\n ]" + ("," if i + 1 < len(traces) else "") + "\n")
        f.write("}\n")


def load():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("s-cgib_amd")
    if sys.argv[1:2] != ["--write"]:
        sys.exit("usage: python tests/launch_trace.py --write [fixture path]")
    dev = torch.device("cuda", 0)
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    dump({name: record(pkg, dev, name) for name in CASES}, out)
    print(f"wrote {out}")
