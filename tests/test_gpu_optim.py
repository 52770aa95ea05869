"""scgib Adam (optim.Adam, scgib_adam_step) against torch.optim.Adam — the
optimizer of every reference script (exp_molhiv.py:53: lr, weight_decay=5e-5).

Same random parameters and gradient sequence through both; parameters and
the three state tensors agree with torch's fused Adam (the same formula at
the same precisions: measured bit-identical; the bar is relative 1e-6).  Covers tensor counts above one
launch's table (80), sizes that are not multiples of the 1024-element chunk,
empty tensors, parameters without gradients, several param groups, and
replay from a captured HIP graph."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (64,), (64, 32), (1,), (0,), (3, 7), (2049,), (64, 128), (5, 1031)] * 10


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _params(dev, seed, shapes=SHAPES):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(s, generator=g).to(dev).requires_grad_() for s in shapes]


def _grads(params, step, skip=()):
    g = torch.Generator(device="cpu").manual_seed(1000 + step)
    for i, p in enumerate(params):
        p.grad = None if i in skip else torch.randn(p.shape, generator=g).to(p.device)


def _close(a, b, tol=1e-6):
    scale = b.abs().max().item() if b.numel() else 0.0
    return (a - b).abs().max().item() <= tol * max(scale, 1e-30) if a.numel() else True


@pytest.mark.parametrize("wd,lr", [(5e-5, 1e-4), (0.0, 1e-3), (1e-5, 5e-3)])
def test_adam_matches_torch(pkg, dev, wd, lr):
    mine, ref = _params(dev, 1), _params(dev, 1)
    opt_m = pkg.optim.Adam(mine, lr=lr, weight_decay=wd)
    opt_r = torch.optim.Adam(ref, lr=lr, weight_decay=wd, fused=True)
    skip = {3, 17}  # parameters without a gradient are left alone (torch too)
    for step in range(6):
        _grads(mine, step, skip)
        _grads(ref, step, skip)
        opt_m.step()
        opt_r.step()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(mine, ref)):
        assert _close(a.detach(), b.detach()), i
        if i in skip:
            assert i not in opt_m.state or not opt_m.state[a]
            continue
        sm, sr = opt_m.state[a], opt_r.state[b]
        assert float(sm["step"]) == float(sr["step"]) == 6.0
        assert _close(sm["exp_avg"], sr["exp_avg"]), i
        assert _close(sm["exp_avg_sq"], sr["exp_avg_sq"]), i


def test_adam_param_groups_and_state_dict(pkg, dev):
    mine, ref = _params(dev, 2, [(64, 64), (64,), (10,)]), _params(dev, 2, [(64, 64), (64,), (10,)])
    groups = lambda ps: [{"params": ps[:2], "lr": 1e-3}, {"params": ps[2:], "lr": 1e-2,  # noqa: E731
                                                            "weight_decay": 1e-4}]
    opt_m = pkg.optim.Adam(groups(mine), lr=1e-4)
    opt_r = torch.optim.Adam(groups(ref), lr=1e-4, fused=True)
    for step in range(3):
        _grads(mine, step)
        _grads(ref, step)
        opt_m.step()
        opt_r.step()
    for a, b in zip(mine, ref):
        assert _close(a.detach(), b.detach())
    # torch's state_dict loads into ours and training continues identically
    opt_m2 = pkg.optim.Adam(groups(mine), lr=1e-4)
    opt_m2.load_state_dict(copy.deepcopy(opt_r.state_dict()))  # (load aliases tensors)
    for a, b in zip(mine, ref):
        with torch.no_grad():
            a.copy_(b)
    _grads(mine, 9)
    _grads(ref, 9)
    opt_m2.step()
    opt_r.step()
    for a, b in zip(mine, ref):
        assert _close(a.detach(), b.detach())


def test_adam_graph_replay(pkg, dev):
    mine, ref = _params(dev, 3), _params(dev, 3)
    opt_m = pkg.optim.Adam(mine, lr=1e-3, weight_decay=5e-5)
    opt_r = torch.optim.Adam(ref, lr=1e-3, weight_decay=5e-5, fused=True)
    grads = [torch.zeros_like(p) for p in mine]
    for p, g in zip(mine, grads):
        p.grad = g
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # state allocated outside the capture
        for g in grads:
            g.normal_()
        opt_m.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_m.step()
    # reference: the same gradients, eagerly
    for p, g in zip(ref, grads):
        p.grad = g.clone()
    opt_r.step()
    for step in range(4):
        gen = torch.Generator(device="cpu").manual_seed(50 + step)
        for g, p in zip(grads, ref):
            g.copy_(torch.randn(g.shape, generator=gen).to(dev))
            p.grad = g.clone()
        graph.replay()
        opt_r.step()
    torch.cuda.synchronize()
    for a, b in zip(mine, ref):
        assert _close(a.detach(), b.detach())
        assert float(opt_m.state[a]["step"]) == 5.0


def test_grad_pack_unpack_roundtrip(pkg):
    """scgib_grad_pack / _unpack: one launch each over >96 tensors of mixed
    sizes (two table chunks), exact copy and 1/world scaling."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(n, device=dev))
              for n in [1, 64, 4096, 3000, 2049] * 21]
    for p in params:
        p.grad = torch.randn_like(p)
    red = pkg.dist.GradAllReducer(params)
    ref = torch.cat([p.grad.reshape(-1) for p in params])
    red.pack()
    torch.cuda.synchronize()
    assert torch.equal(red._flat, ref)
    red._flat.mul_(4.0)
    red.unpack()  # world 1: scale 1
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in params]), 4.0 * ref)


@pytest.mark.parametrize("strong", [False, True])
def test_bench_two_ranks_gloo_on_one_gpu(tmp_path, strong):
    """The N > 1 bench path (captured backward + bucket pack, all-reduce
    between replays, captured unpack + Adam) end to end with two ranks on one
    GPU over gloo (the driver's 8-GPU runs use RCCL), weak (64/rank) and
    strong (--global-batch 128 split over the ranks) scaling."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SCGIB_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", "--master-port=29533", os.path.join(root, "bench.py"),
           "--gpus", "2", "--steps", "4", "--warmup", "2", "--pool", "2",
           "--no-cpu-baseline", "--no-superbatch", "--no-kernel-timer"]
    cmd += ["--global-batch", "128"] if strong else ["--batch", "64"]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["value"] > 0
    assert line["config"]["parallelism"] == "dp2" and line["config"]["global_batch"] == 128
    assert line["scaling"] == ("strong" if strong else "weak")
    assert line["config"]["allreduce"] == "between two graph replays"
    assert line["config"]["final_loss"] == line["config"]["final_loss"]  # finite (not NaN)
    # replica mode: after the timed steps both ranks hold bitwise the same
    # parameters and BatchNorm statistics (the one averaged bucket applied by
    # both); the step itself is parity-tested in tests/test_gpu_dp.py
    assert line["config"]["replica_max_abs_diff"] == 0.0


def test_bench_allreduce_captured_one_rank_rccl():
    """The RCCL all-reduce of the gradient + BN-statistics bucket captured
    inside the replayed step graph (the N > 1 default), exercised on one GPU
    through a 1-rank nccl (RCCL) group: the capture succeeds and the step runs."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--force-allreduce", "--steps", "6",
           "--warmup", "2", "--batch", "64", "--pool", "2", "--no-cpu-baseline",
           "--no-superbatch", "--no-kernel-timer"]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["config"]["allreduce"] == "captured in the step graph", out.stderr[-2000:]
    assert line["value"] > 0 and line["config"]["final_loss"] == line["config"]["final_loss"]


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain bench run times --steps steps and carries none of the --full
    measurements in its line; --dump-outputs writes the last timed step's loss
    parts and the updated model as float32 arrays, the same from run to run."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for tag in ("a", "b"):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3",
               "--warmup", "1", "--batch", "64", "--pool", "2", "--dump-outputs",
               str(tmp_path / tag)]
        out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=240)
        assert out.returncode == 0, out.stderr[-3000:]
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["unit"] == "graphs/s" and line["higher_is_better"] and line["dtype"] == "fp32"
        assert abs(line["value"] - 64 / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
        for key in ("roofline", "roofline_kernels", "roofline_superbatch", "cpu_baseline",
                    "finetune"):
            assert line[key] is None, key
        dumps.append({f[:-4]: np.load(tmp_path / tag / f) for f in os.listdir(tmp_path / tag)})
    a, b = dumps
    assert sorted(a) == ["bn_buffers", "loss_con", "loss_kl", "loss_rec", "params"]
    for name, arr in a.items():
        assert arr.dtype == np.float32 and np.isfinite(arr).all(), name
        assert np.array_equal(arr, b[name]), name
    assert a["loss_kl"].shape == (1,) and a["params"].size > 100_000
    loss = float(a["loss_kl"][0] + a["loss_rec"][0] + a["loss_con"][0])
    assert abs(loss - line["config"]["final_loss"]) <= 1e-3 + 1e-5 * abs(loss)


def test_adam_step_reduce_matches_reduce_then_step(pkg, dev):
    """scgib_adam_step_reduce: the slab reduce of two jobs (one with a column
    stride) and the Adam step in one launch, bitwise the reduce launch
    followed by scgib_adam_step — for tensors inside a job's output (several
    per job, one not at its start), tensors outside, a reduced output no
    tensor covers, and a tensor larger than one fused chunk; a gradient
    straddling an output's edge is refused."""
    import ctypes
    L, ops = pkg._lib, pkg.ops
    gen = torch.Generator().manual_seed(5)
    nslab, w0, w1, stride1 = 37, 64 * 64 + 64 + 96, 1000, 1200
    slab0 = torch.randn(nslab, w0, generator=gen).to(dev)
    slab1 = torch.randn(nslab + 2, stride1, generator=gen).to(dev)
    shapes = [(64, 64), (64,), (96,), (3, 7), (9000,), (700,)]

    def run(fused):
        out0 = torch.zeros(w0, device=dev)
        out1 = torch.zeros(w1, device=dev)
        ps = [torch.randn(s, generator=torch.Generator().manual_seed(i)).to(dev)
              for i, s in enumerate(shapes)]
        grads = [out0[:4096].view(64, 64), out0[4096:4160], out1[200:296],
                 torch.randn(3, 7, generator=torch.Generator().manual_seed(9)).to(dev),
                 torch.randn(9000, generator=torch.Generator().manual_seed(10)).to(dev),
                 out1[300:1000]]  # (out0's last 96 columns, out1[:200] and [296:300]: no tensor)
        mg = torch.Generator().manual_seed(21)
        steps = [torch.full((), 3.0, device=dev) for _ in shapes]
        ms = [(torch.rand(s, generator=mg).to(dev), torch.rand(s, generator=mg).to(dev))
              for s in shapes]
        ent = [L.AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), s.data_ptr(),
                            p.numel()) for p, g, s, (m, v) in zip(ps, grads, steps, ms)]
        jobs = [L.SlabJob(slab0.data_ptr(), out0.data_ptr(), w0, nslab, 0),
                L.SlabJob(slab1.data_ptr(), out1.data_ptr(), w1, nslab + 2, stride1)]
        tab = (L.AdamTensor * len(ent))(*ent)
        jt = (L.SlabJob * 2)(*jobs)
        cnt = ops.counters(dev, "adam", 1)
        args = (1e-3, 0.9, 0.999, 1e-8, 5e-5, ops._p(cnt), ops._stream())
        if fused:
            L.call("scgib_adam_step_reduce", ctypes.cast(tab, ctypes.c_void_p), len(ent),
                   ctypes.cast(jt, ctypes.c_void_p), 2, *args)
        else:
            L.call("scgib_slab_reduce_multi", ctypes.cast(jt, ctypes.c_void_p), 2, ops._stream())
            L.call("scgib_adam_step", ctypes.cast(tab, ctypes.c_void_p), len(ent), *args)
        torch.cuda.synchronize()
        return [out0, out1] + ps + steps + [t for mv in ms for t in mv]

    a, b = run(False), run(True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert float(b[2 + len(shapes)]) == 4.0  # steps advanced once
    # a gradient straddling the end of a job's output
    out0 = torch.zeros(w0, device=dev)
    p = torch.zeros(128, device=dev)
    m, v, s = torch.zeros(128, device=dev), torch.zeros(128, device=dev), torch.zeros((), device=dev)
    bad = (L.AdamTensor * 1)(L.AdamTensor(p.data_ptr(), out0.data_ptr() + 4 * (w0 - 64),
                                          m.data_ptr(), v.data_ptr(), s.data_ptr(), 128))
    jt = (L.SlabJob * 1)(L.SlabJob(slab0.data_ptr(), out0.data_ptr(), w0, nslab, 0))
    with pytest.raises(L.ScgibError):
        L.call("scgib_adam_step_reduce", ctypes.cast(bad, ctypes.c_void_p), 1,
               ctypes.cast(jt, ctypes.c_void_p), 1, 1e-3, 0.9, 0.999, 1e-8, 0.0,
               ops._p(ops.counters(dev, "adam", 1)), ops._stream())
    # two tensors' gradients overlapping inside one output
    q = torch.zeros(128, device=dev)
    two = (L.AdamTensor * 2)(L.AdamTensor(p.data_ptr(), out0.data_ptr(), m.data_ptr(), v.data_ptr(),
                                          s.data_ptr(), 128),
                             L.AdamTensor(q.data_ptr(), out0.data_ptr() + 4 * 64, m.data_ptr(),
                                          v.data_ptr(), s.data_ptr(), 128))
    with pytest.raises(L.ScgibError):
        L.call("scgib_adam_step_reduce", ctypes.cast(two, ctypes.c_void_p), 2,
               ctypes.cast(jt, ctypes.c_void_p), 1, 1e-3, 0.9, 0.999, 1e-8, 0.0,
               ops._p(ops.counters(dev, "adam", 1)), ops._stream())
