"""optim.Adam with its hyper-parameters on the device:
scgib_grad_norm, scgib_adam_step_dyn and scgib_adam_step_reduce_dyn — a
learning-rate schedule, global-norm clipping and the skipping of a non-finite
step inside a replayed step — and AdamW (decoupled=True) on both paths.

The by-value path (scgib_adam_step, the parent's code) is the reference of
the bitwise claims: a twin optimizer without new arguments, stepped at the
read-back ``last_lr`` on gradients pre-multiplied by the read-back
``clip_coef`` in fp32, feeds the same doubles to the same adam_elem.  torch
(clip_grad_norm_ + fused Adam / AdamW + LambdaLR) is held to the relative
1e-6 of tests/test_gpu_optim.py.

90 tensors (two 80-tensor tables); sizes around the wavefront (63, 65) and
the 1024-element chunk (1023, 1024, 1025), 0- and 1-element tensors, and one
of 300 000 elements: more than 256 chunk partials in its table, so the
last-arriver sum takes two rounds of the 256-thread workgroup.
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

from poison import assert_same, run_thrice
from test_gpu_optim import _close

pytestmark = pytest.mark.gpu

BASE = [(64, 64), (64,), (64, 32), (1,), (0,), (3, 7), (2049,), (64, 128), (5, 1031)]
SHAPES = BASE * 9 + [(63,), (65,), (1023,), (1024,), (1025,), (300_000,), (0,), (1,), (3, 7)]
assert len(SHAPES) == 90
SKIP = (3, 17)  # parameters without a gradient
K = 6
LR = 1e-3
# randn gradients over ~5e5 elements have norm ~700 x scale: the clip bites
# (coef < 1) on the even steps and does not (coef = 1) on the odd ones
MAX_NORM = 1.0
SCALES = [1e-2, 1e-4, 3e-3, 1e-5, 1e-2, 2e-4, 1e-2, 1e-4]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _sched(pkg):
    return pkg.optim.Schedule("cosine", warmup=2, total=5, warmup_start=0.1, min_ratio=0.05)


_CPU = {}


def _cpu_params(seed):
    if ("p", seed) not in _CPU:
        g = torch.Generator().manual_seed(seed)
        _CPU["p", seed] = [torch.randn(s, generator=g) for s in SHAPES]
    return _CPU["p", seed]


def _cpu_grads(step):
    """Step ``step``'s gradients (CPU, fp32), computed once and shared."""
    if ("g", step) not in _CPU:
        g = torch.Generator().manual_seed(1000 + step)
        _CPU["g", step] = [SCALES[step] * torch.randn(s, generator=g) for s in SHAPES]
    return _CPU["g", step]


def _params(dev, seed=1):
    return [p.to(dev).requires_grad_() for p in _cpu_params(seed)]


def _set_grads(params, grads, skip=SKIP, mul=None):
    for i, (p, g) in enumerate(zip(params, grads)):
        if i in skip:
            p.grad = None
        else:
            g = g.to(p.device)
            p.grad = g if mul is None else g * mul  # (an fp32 multiply by a device scalar)


def _np_norm(grads, skip=SKIP):
    s = sum(float((g.double().numpy() ** 2).sum()) for i, g in enumerate(grads) if i not in skip)
    return np.float32(np.sqrt(np.float64(s)))


def _snapshot(params, opt):
    out = {}
    for i, p in enumerate(params):
        out[f"p{i}"] = p.detach().clone()
        for k, v in opt.state.get(p, {}).items():
            out[f"{k}{i}"] = v.detach().clone()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _assert_equal(a, b):
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]
    assert not bad, bad[:8]


def _assert_close(a, b):
    assert a.keys() == b.keys()
    bad = [k for k in a if not _close(a[k].float(), b[k].float())]
    assert not bad, bad[:8]


def _twin_step(twin, tparams, grads, opt, skip=SKIP):
    """The by-value twin's step at the rate and clip coefficient ``opt``'s
    last step read out."""
    twin.param_groups[0]["lr"] = float(opt.last_lr[0])
    _set_grads(tparams, grads, skip, mul=opt.clip_coef)
    twin.step()


# ---------------------------------------------------------------------------
# 1. the norm
# ---------------------------------------------------------------------------
def _norm_run(pkg, dev, grads, skip=SKIP, **kw):
    params = _params(dev)
    opt = pkg.optim.Adam(params, lr=LR, max_grad_norm=MAX_NORM, **kw)
    _set_grads(params, grads, skip)
    opt.step()
    return {"norm": opt.grad_norm.clone(), "coef": opt.clip_coef.clone(),
            "p5": params[5].detach().clone(), "big": params[86].detach().clone()}


def test_norm_one_ulp_of_numpy_and_reproducible(pkg, dev):
    grads = _cpu_grads(0)
    ref = _np_norm(grads)
    a = _norm_run(pkg, dev, grads)
    b = _norm_run(pkg, dev, grads)
    got = np.float32(a["norm"].item())
    # each square is exact in double, the double sum is far inside 2^-24
    # relative, one rounding to fp32 remains: one ulp
    print("norm", got, "numpy", ref, "ulp", np.spacing(ref))
    assert abs(np.float64(got) - np.float64(ref)) <= np.spacing(ref)
    assert torch.equal(_bits(a["norm"]), _bits(b["norm"]))
    coef = np.float32(MAX_NORM) / (got + np.float32(1e-6))
    assert a["coef"].item() == min(np.float32(1.0), coef) and coef < 1
    # fresh workspaces filled with NaN and with the sentinel: the same bits
    res = run_thrice(lambda: grads, lambda g: _norm_run(pkg, dev, g))
    assert_same(res)
    assert torch.equal(_bits(res[0]["norm"].to(dev)), _bits(a["norm"]))


def test_norm_skips_empty_and_gradless(pkg, dev):
    """0- and 1-element tensors in the table and parameters without .grad:
    the norm of the rest; and a step on nothing but such tensors."""
    grads = _cpu_grads(2)
    skip = (0, 3, 17, 85, 86)  # incl. the first tensor and the largest
    a = _norm_run(pkg, dev, grads, skip=skip)
    ref = _np_norm(grads, skip)
    assert abs(np.float64(a["norm"].item()) - np.float64(ref)) <= np.spacing(ref)
    only = tuple(i for i, s in enumerate(SHAPES) if s != (0,))
    z = _norm_run(pkg, dev, grads, skip=only)  # only the empty tensors have gradients
    assert z["norm"].item() == 0.0 and z["coef"].item() == 1.0
    params = _params(dev)
    opt = pkg.optim.Adam(params, lr=LR, max_grad_norm=MAX_NORM, schedule=_sched(pkg))
    opt.step()  # no gradient at all: the call still counts
    assert int(opt.calls) == 1 and opt.grad_norm.item() == 0.0
    assert opt.last_lr.item() == LR * _sched(pkg).factor(0)


# ---------------------------------------------------------------------------
# 2. device-hyper path == by-value path, bitwise;  3. against torch
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dyn_runs(pkg, dev):
    """K eager device-hyper steps per weight decay (schedule + clipping), with
    the per-step read-outs and the final state: shared by the tests below."""
    out = {}
    for wd in (0.0, 5e-5):
        params = _params(dev)
        opt = pkg.optim.Adam(params, lr=LR, weight_decay=wd, schedule=_sched(pkg),
                             max_grad_norm=MAX_NORM)
        tparams = _params(dev)
        twin = pkg.optim.Adam(tparams, lr=LR, weight_decay=wd)
        lrs, coefs, norms, equal = [], [], [], []
        for k in range(K):
            _set_grads(params, _cpu_grads(k))
            opt.step()
            lrs.append(opt.last_lr.clone())
            coefs.append(opt.clip_coef.clone())
            norms.append(opt.grad_norm.clone())
            _twin_step(twin, tparams, _cpu_grads(k), opt)
            a, b = _snapshot(params, opt), _snapshot(tparams, twin)
            equal.append([k_ for k_ in a if not torch.equal(_bits(a[k_]), _bits(b[k_]))])
        torch.cuda.synchronize()
        out[wd] = dict(lrs=[float(v) for v in lrs], coefs=[float(v) for v in coefs],
                       norms=[float(v) for v in norms], mismatch=equal, calls=int(opt.calls),
                       skipped=int(opt.skipped), final=_snapshot(params, opt),
                       twin_final=_snapshot(tparams, twin))
    return out


@pytest.mark.parametrize("wd", [0.0, 5e-5])
def test_dyn_equals_by_value_twin_bitwise(pkg, dev, dyn_runs, wd):
    r = dyn_runs[wd]
    assert any(c < 1.0 for c in r["coefs"]) and any(c == 1.0 for c in r["coefs"]), r["coefs"]
    assert r["calls"] == K and r["skipped"] == 0
    for k, bad in enumerate(r["mismatch"]):
        assert not bad, (k, bad[:8])
    assert set(r["final"]) == set(r["twin_final"])
    step = [v for k_, v in r["final"].items() if k_.startswith("step")]
    assert step and all(float(s) == K for s in step)
    s = _sched(pkg)
    for c, lr in enumerate(r["lrs"]):
        # device double cos is within a few ulp; 1e-12 leaves three orders of
        # margin and still catches a wrong c or u
        want = LR * s.factor(c)
        print("step", c, "last_lr", lr, "host", want, "coef", r["coefs"][c], "norm", r["norms"][c])
        assert abs(lr - want) <= 1e-12 * want
    for c, n in enumerate(r["norms"]):
        ref = _np_norm(_cpu_grads(c))
        assert abs(np.float64(np.float32(n)) - np.float64(ref)) <= np.spacing(ref)


def _torch_run(pkg, dev, cls, wd, clip, sched, **kw):
    params = _params(dev)
    used = [p for i, p in enumerate(params) if i not in SKIP]
    opt = cls(params, lr=LR, weight_decay=wd, fused=True, **kw)
    lam = torch.optim.lr_scheduler.LambdaLR(opt, sched.factor) if sched is not None else None
    for k in range(K):
        _set_grads(params, _cpu_grads(k))
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(used, clip)
        opt.step()
        if lam is not None:
            lam.step()
    return _snapshot(params, opt)


@pytest.mark.parametrize("wd", [0.0, 5e-5])
def test_dyn_against_torch_clip_adam_lambdalr(pkg, dev, dyn_runs, wd):
    ref = _torch_run(pkg, dev, torch.optim.Adam, wd, MAX_NORM, _sched(pkg))
    _assert_close(dyn_runs[wd]["final"], ref)


@pytest.mark.parametrize("path", ["by_value", "device_hyper"])
def test_decoupled_against_torch_adamw(pkg, dev, path):
    wd = 1e-2
    params = _params(dev)
    if path == "by_value":
        opt = pkg.optim.Adam(params, lr=LR, weight_decay=wd, decoupled=True)
        assert not opt.device_hyper
        ref = _torch_run(pkg, dev, torch.optim.AdamW, wd, None, None)
    else:
        opt = pkg.optim.Adam(params, lr=LR, weight_decay=wd, decoupled=True,
                             schedule=_sched(pkg), max_grad_norm=MAX_NORM)
        ref = _torch_run(pkg, dev, torch.optim.AdamW, wd, MAX_NORM, _sched(pkg))
    for k in range(K):
        _set_grads(params, _cpu_grads(k))
        opt.step()
    mine = _snapshot(params, opt)
    _assert_close(mine, ref)
    # and it is not Adam's L2 decay: the two differ far beyond the bar
    l2 = _torch_run(pkg, dev, torch.optim.Adam, wd, None if path == "by_value" else MAX_NORM,
                    None if path == "by_value" else _sched(pkg))
    assert not _close(mine["p0"], l2["p0"], tol=1e-5)


def test_two_param_groups_one_global_norm(pkg, dev):
    """Two groups with their own lr, weight decay and (the second) schedule:
    each launch reads its group's block, the norm and the call counter are the
    optimizer's (one advance per step), bitwise the two-group by-value twin."""
    params, tparams = _params(dev), _params(dev)
    own = pkg.optim.Schedule("linear", warmup=1, total=4, min_ratio=0.2)
    groups = lambda ps: [{"params": ps[:50]},  # noqa: E731
                         {"params": ps[50:], "lr": 5e-3, "weight_decay": 1e-4}]
    g = groups(params)
    g[1]["schedule"] = own
    opt = pkg.optim.Adam(g, lr=LR, schedule=_sched(pkg), max_grad_norm=MAX_NORM)
    twin = pkg.optim.Adam(groups(tparams), lr=LR)
    for k in range(4):
        _set_grads(params, _cpu_grads(k))
        opt.step()
        want = [LR * _sched(pkg).factor(k), 5e-3 * own.factor(k)]
        got = opt.last_lr.tolist()
        assert all(abs(a - b) <= 1e-12 * b for a, b in zip(got, want)), (k, got, want)
        ref = _np_norm(_cpu_grads(k))  # one norm over both groups
        assert abs(np.float64(opt.grad_norm.item()) - np.float64(ref)) <= np.spacing(ref)
        for tg, lr in zip(twin.param_groups, got):
            tg["lr"] = lr
        _set_grads(tparams, _cpu_grads(k), mul=opt.clip_coef)
        twin.step()
    assert int(opt.calls) == 4
    _assert_equal(_snapshot(params, opt), _snapshot(tparams, twin))


# ---------------------------------------------------------------------------
# 4. capture
# ---------------------------------------------------------------------------
def test_capture_replays_schedule_and_synced_edits(pkg, dev):
    """One captured step() replayed: the rate follows the schedule from the
    device call counter, the parameters equal the eager device-hyper run
    bitwise; a host edit of group['lr'] reaches the replays through
    sync_hyper() (the parent bakes lr into the node: the edit would be
    ignored, and it cannot build this optimizer at all); a capture with
    unsynced edits raises."""
    wd = 5e-5
    mk = lambda ps: pkg.optim.Adam(ps, lr=LR, weight_decay=wd, schedule=_sched(pkg),  # noqa: E731
                                   max_grad_norm=MAX_NORM)
    params, eparams, tparams = _params(dev), _params(dev), _params(dev)
    opt, eager = mk(params), mk(eparams)
    twin = pkg.optim.Adam(tparams, lr=LR, weight_decay=wd)
    static = [torch.zeros(s, device=dev) for s in SHAPES]
    _set_grads(params, static, skip=())

    def feed(k):
        for s, g in zip(static, _cpu_grads(k)):
            s.copy_(g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # state and blocks allocated outside the capture
        feed(0)
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    _twin_step(twin, tparams, _cpu_grads(0), opt, skip=())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    _set_grads(eparams, _cpu_grads(0), skip=())
    eager.step()
    s = _sched(pkg)
    for k in range(1, 5):
        feed(k)
        graph.replay()
        want = LR * s.factor(k)
        assert abs(float(opt.last_lr) - want) <= 1e-12 * want, k
        _twin_step(twin, tparams, _cpu_grads(k), opt, skip=())
        _set_grads(eparams, _cpu_grads(k), skip=())
        eager.step()
    assert int(opt.calls) == 5
    _assert_equal(_snapshot(params, opt), _snapshot(eparams, eager))
    assert torch.equal(_bits(opt.grad_norm), _bits(eager.grad_norm))  # eager == replay
    # a host edit between replays
    opt.param_groups[0]["lr"] *= 0.1
    opt.sync_hyper()
    for k in range(5, 7):
        feed(k)
        graph.replay()
        want = 0.1 * LR * s.factor(k)
        assert abs(float(opt.last_lr) - want) <= 1e-12 * want, k
        _twin_step(twin, tparams, _cpu_grads(k), opt, skip=())
    torch.cuda.synchronize()
    _assert_equal(_snapshot(params, opt), _snapshot(tparams, twin))
    # unsynced host values under capture: refused, nothing baked or launched
    before = _snapshot(params, opt)
    opt.param_groups[0]["lr"] *= 0.5
    scratch = torch.zeros(4, device=dev)
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(pkg._lib.ScgibError, match="sync_hyper"):
        with torch.cuda.graph(g2):
            scratch.add_(1.0)
            opt.step()
    torch.cuda.synchronize()
    assert int(opt.calls) == 7
    _assert_equal(before, _snapshot(params, opt))


# ---------------------------------------------------------------------------
# 5. skip
# ---------------------------------------------------------------------------
def _poisoned_grads(kind):
    grads = [g.clone() for g in _cpu_grads(1)]
    if kind == "nan_last":
        grads[-1].view(-1)[-1] = float("nan")
    else:
        grads[0].view(-1)[0] = float("inf")
    return grads


@pytest.mark.parametrize("kind", ["nan_last", "inf_first"])
def test_skip_nonfinite_changes_nothing(pkg, dev, kind):
    params, tparams = _params(dev), _params(dev)
    opt = pkg.optim.Adam(params, lr=LR, weight_decay=5e-5, schedule=_sched(pkg),
                         max_grad_norm=MAX_NORM, skip_nonfinite=True)
    twin = pkg.optim.Adam(tparams, lr=LR, weight_decay=5e-5)
    _set_grads(params, _cpu_grads(0), skip=())
    opt.step()
    _twin_step(twin, tparams, _cpu_grads(0), opt, skip=())
    before = _snapshot(params, opt)
    _set_grads(params, _poisoned_grads(kind), skip=())
    opt.step()
    assert int(opt.skipped) == 1 and int(opt.calls) == 2
    assert not np.isfinite(opt.grad_norm.item())
    _assert_equal(before, _snapshot(params, opt))  # parameters, moments and steps
    _set_grads(params, _cpu_grads(2), skip=())
    opt.step()
    assert int(opt.skipped) == 1 and int(opt.calls) == 3
    want = LR * _sched(pkg).factor(2)  # the skipped call advanced the schedule
    assert abs(float(opt.last_lr) - want) <= 1e-12 * want
    _twin_step(twin, tparams, _cpu_grads(2), opt, skip=())
    _assert_equal(_snapshot(params, opt), _snapshot(tparams, twin))


@pytest.mark.parametrize("kind", ["nan_last", "inf_first"])
def test_without_skip_nonfinite_is_torchs_nan(pkg, dev, kind):
    params, rparams = _params(dev), _params(dev)
    opt = pkg.optim.Adam(params, lr=LR, max_grad_norm=MAX_NORM)
    ref = torch.optim.Adam(rparams, lr=LR, fused=True)
    grads = _poisoned_grads(kind)
    _set_grads(params, grads, skip=())
    _set_grads(rparams, grads, skip=())
    opt.step()
    torch.nn.utils.clip_grad_norm_(rparams, MAX_NORM)
    ref.step()
    assert int(opt.skipped) == 0 and int(opt.calls) == 1
    for i, (a, b) in enumerate(zip(params, rparams)):
        assert torch.equal(torch.isnan(a), torch.isnan(b)), i
        if kind == "nan_last":  # a NaN norm: a NaN coefficient: everything
            assert bool(torch.isnan(a).all()), i
    assert bool(torch.isnan(params[0].view(-1)[0]))


# ---------------------------------------------------------------------------
# 6. the fused final reduce
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True])
def test_fused_final_reduce_on_the_device_hyper_path(pkg, dev, monkeypatch, clip):
    """Inside ops.fuse_final_into_step a schedule-only step is ONE launch of
    scgib_adam_step_reduce_dyn (today's launch count); with clipping the
    reduces run first (the norm needs every reduced gradient), then the norm,
    then scgib_adam_step_dyn.  Either way the gradients, parameters and Adam
    state equal the unfused device-hyper run bitwise."""
    from test_gpu_graph_split import _assert_bitwise, _eager_batches, _fwd_bwd, _grads, _state
    from test_gpu_trajectory import _pretrain_model
    monkeypatch.setattr(pkg.ops, "FUSE_FINAL_MIN_SLABS", 0)
    batches = _eager_batches(pkg, dev, 3)
    real_call, calls, order = pkg._lib.call, {}, []

    def counting_call(name, *args):
        calls[name] = calls.get(name, 0) + 1
        order.append(name)
        return real_call(name, *args)

    monkeypatch.setattr(pkg._lib, "call", counting_call)
    runs = []
    for armed in (False, True):
        model = _pretrain_model(pkg, pkg.synth.WORKLOADS["qm9"][2], 1, 32, dev)
        opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5,
                             schedule=_sched(pkg), max_grad_norm=0.5 if clip else None)
        calls.clear()
        grads = []
        for item in batches:
            opt.zero_grad(set_to_none=True)
            del order[:]
            with (pkg.ops.fuse_final_into_step() if armed else contextlib.nullcontext()):
                _fwd_bwd(model, item, dev)
                opt.step()
            grads.append(_grads(model))
            if armed and clip:
                tail = [n for n in order if n in ("scgib_slab_reduce_multi_ex", "scgib_grad_norm",
                                                  "scgib_adam_step_dyn")][-3:]
                assert tail == ["scgib_slab_reduce_multi_ex", "scgib_grad_norm",
                                "scgib_adam_step_dyn"], order[-6:]
        torch.cuda.synchronize()
        n_red, n_dyn = calls.get("scgib_adam_step_reduce_dyn", 0), calls.get("scgib_adam_step_dyn", 0)
        assert calls.get("scgib_adam_step", 0) == calls.get("scgib_adam_step_reduce", 0) == 0
        if armed and not clip:
            assert (n_red, n_dyn) == (len(batches), 0), (n_red, n_dyn)
        else:
            assert (n_red, n_dyn) == (0, len(batches)), (n_red, n_dyn)
        assert calls.get("scgib_grad_norm", 0) == (len(batches) if clip else 0)
        assert not pkg.ops._FINAL_PENDING and not pkg.ops._FINAL_ARMED[0]
        assert int(opt.calls) == len(batches)
        runs.append((grads, _state(model, opt), opt.last_lr.clone()))
    for ga, gb in zip(runs[0][0], runs[1][0]):
        _assert_bitwise(ga, gb)
    _assert_bitwise(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])


# ---------------------------------------------------------------------------
# 7. in the model's replayed step
# ---------------------------------------------------------------------------
B_MODEL, WARM, REPLAYS = 8, 3, 4


def _model_run(pkg, dev, split, replays, warm, **opt_kw):
    """The bench's pretrain step on 8 synthetic molecules: ``warm`` eager
    steps, the capture, ``replays`` replays.  Returns the state, the read-outs
    per replay, and the optimizer."""
    import bench
    from test_gpu_graph_split import _state
    from test_gpu_trajectory import _pretrain_model
    F_in = pkg.synth.WORKLOADS["qm9"][2]
    hosts = [pkg.graph.collate_pyg(pkg.synth.molecules(B_MODEL, "qm9", seed=40 + i))[0]
             for i in range(2)]
    model = _pretrain_model(pkg, F_in, 1, B_MODEL, dev)
    opt = pkg.optim.Adam(model.parameters(), lr=1e-3, weight_decay=5e-5, **opt_kw)
    pkg.ops.seed_noise(dev, 4242)
    rs = bench.build_replay_step(model, opt, hosts, 1, B_MODEL, dev, prefetch=True, warm=warm,
                                 split=split)
    assert (rs.split is not None) == (split and pkg.ops.xq_enabled())
    lrs, norms = [], []
    for j in range(replays):
        rs.step(j)
        if opt.device_hyper:
            lrs.append(opt.last_lr.clone())
            norms.append(opt.grad_norm.clone())
    torch.cuda.synchronize()
    assert pkg.ops.xq_timeouts(dev) == 0
    state = _state(model, opt)
    if rs.split is not None:
        rs.split.close()
    return state, [float(v) for v in lrs], [float(v) for v in norms], opt


def test_model_step_schedule_and_clip_split_whole_eager(pkg, dev):
    from test_gpu_graph_split import _assert_bitwise
    sched = pkg.optim.Schedule("cosine", warmup=4, total=WARM + REPLAYS, warmup_start=0.2,
                               min_ratio=0.1)
    kw = dict(schedule=sched, max_grad_norm=0.05)
    runs = [_model_run(pkg, dev, split, REPLAYS, WARM, **kw) for split in (False, True)]
    for state, lrs, norms, opt in runs:
        assert int(opt.calls) == WARM + REPLAYS and int(opt.skipped) == 0
        for j, lr in enumerate(lrs):  # the warm-up steps counted as calls 0 .. WARM - 1
            want = 1e-3 * sched.factor(WARM + j)
            assert abs(lr - want) <= 1e-12 * want, (j, lr, want)
        assert all(np.isfinite(n) and n > 0 for n in norms), norms
    assert runs[0][2] == runs[1][2]
    _assert_bitwise(runs[0][0], runs[1][0])
    # the same optimizer stepped eagerly with the same seeds: every step of the
    # replayed run as one of build_replay_step's eager warm-up steps
    eager = _model_run(pkg, dev, False, 0, WARM + REPLAYS, **kw)
    assert int(eager[3].calls) == WARM + REPLAYS
    _assert_bitwise(runs[0][0], eager[0])


def test_model_step_constant_schedule_equals_no_new_arguments(pkg, dev):
    from test_gpu_graph_split import _assert_bitwise
    plain = _model_run(pkg, dev, True, REPLAYS, WARM)
    const = _model_run(pkg, dev, True, REPLAYS, WARM, schedule=pkg.optim.Schedule("constant"))
    assert not plain[3].device_hyper and const[3].device_hyper
    assert const[1] == [1e-3] * REPLAYS
    _assert_bitwise(plain[0], const[0])
