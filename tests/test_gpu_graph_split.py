"""Two-lane replay of a captured step graph (ops.SplitGraph,
csrc/graph_split.hip; DESIGN.md §3 "Host enqueue").

The split must be invisible in the results: the same kernels with the same
launch parameters, one lane per captured chain, the cross-chain edges as
signal / wait kernels.  Checked three ways:
  * a toy two-stream graph of torch elementwise ops with two fork / join
    sections and a read of the main chain's data on the side chain, replayed
    50 times back to back (no host sync: cross-replay ordering included)
    against the closed-form values;
  * the bench's pretrain step (bench.build_replay_step) and the fine-tune
    step (finetune_bench.build_finetune_step), split and whole, from the same
    initial state and the same explicit noise: losses, every parameter, the
    Adam moments and the BatchNorm buffers bitwise equal after K replays
    (every reduction of the step is in a fixed order, so a whole replay and a
    split one are bit-for-bit the same computation);
  * the same two behind a BUSY stream: >= 0.3 s of queued work (1.5 times the
    0.2 s after which a lane's wait gives up) ahead of a replay must not let
    the side lane run ahead of it.
The ego chain's final reduce folded into the Adam launch
(ops.fuse_final_into_step) is checked where gradients already exist, where
.grad is re-bound, and where the step raises; a capture that drew with
torch's generator must not be split.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def test_split_toy_two_stream_graph(pkg, dev):
    if not pkg.ops.xq_enabled():
        pytest.skip(f"hand-offs off here: {pkg.ops.XQ_REASON}")
    n = 1 << 16
    a, b, c, d, e, f = (torch.zeros(n, device=dev) for _ in range(6))
    main = torch.cuda.Stream(dev)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.stream(main):
        with torch.cuda.graph(g, stream=main):
            a.add_(1.0)                         # main
            side.wait_stream(main)              # fork 1
            with torch.cuda.stream(side):
                b.mul_(2.0).add_(a)             # side reads main's a
            torch.mul(a, 3.0, out=d)            # main, beside it
            main.wait_stream(side)              # join 1
            torch.add(b, d, out=c)
            side.wait_stream(main)              # fork 2
            with torch.cuda.stream(side):
                e.add_(c)
            f.add_(1.0)
            main.wait_stream(side)              # join 2
            c.add_(e)
    lanes = pkg.ops.SplitGraph(g, dev)
    info = lanes.info
    assert info["serialised"] == 0 and info["lane0_kernels"] and info["lane1_kernels"], info
    assert info["lane0_kernels"] + info["lane1_kernels"] == info["captured"], info
    assert info["handoffs"] >= 4, info  # two forks, two joins
    K = 50
    for _ in range(K):  # back to back: the next replay's lanes queue behind this one's
        lanes.replay()
    torch.cuda.synchronize()
    ea = eb = ec = ed = ee = ef = 0.0
    for _ in range(K):
        ea += 1.0
        eb = 2.0 * eb + ea
        ed = 3.0 * ea
        ec = eb + ed
        ee += ec
        ef += 1.0
        ec += ee
    # b doubles each replay: compare in relative terms (fp32 of exact integers
    # up to 2^24, then rounded the same way on both sides within 1 ulp chains)
    for t, v in ((a, ea), (d, ed), (f, ef)):
        assert torch.all(t == v), (t[0].item(), v)
    for t, v in ((b, eb), (c, ec), (e, ee)):
        assert torch.allclose(t, torch.full_like(t, v), rtol=1e-5), (t[0].item(), v)
    assert lanes.timeouts() == 0
    lanes.close()


BUSY_S, BUSY_CAP_S = 0.3, 0.6  # 1.5 x the waits' 0.2 s give-up; the filler's cap


class _Filler:
    """Queued work on the current stream: a chain of in-place adds over one
    preallocated 1 GiB buffer, timed with HIP events first and sized for the
    middle of [BUSY_S, BUSY_CAP_S] (the clock may rise after the timing run)."""

    def __init__(self, dev):
        self.buf = torch.zeros(1 << 28, device=dev)
        for _ in range(5):
            self.buf.add_(1.0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(20):
            self.buf.add_(1.0)
        t1.record()
        t1.synchronize()
        unit = t0.elapsed_time(t1) / 20 * 1e-3
        self.units = max(1, min(int(0.5 * (BUSY_S + BUSY_CAP_S) / unit) + 1,
                                int(BUSY_CAP_S / unit)))
        self.marks = []

    def enqueue(self):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(self.units):
            self.buf.add_(1.0)
        t1.record()
        self.marks.append((t0, t1))

    def seconds(self):
        """How long each enqueued filler ran (after a synchronize)."""
        return [t0.elapsed_time(t1) * 1e-3 for t0, t1 in self.marks]


def test_split_toy_graph_behind_busy_stream(pkg, dev):
    """The toy graph replayed three times, each behind >= 0.3 s of queued
    work and then a write the graph reads (a.fill_): the side lane must wait
    for it.  Without a host-side order of the side stream after the caller's,
    the side lane's first wait gives up after 0.2 s and it reads `a` (and
    writes `b`, `e`) ahead of the main lane."""
    if not pkg.ops.xq_enabled():
        pytest.skip(f"hand-offs off here: {pkg.ops.XQ_REASON}")
    n = 1 << 16
    a, b, c, d, e, f = (torch.zeros(n, device=dev) for _ in range(6))
    main = torch.cuda.Stream(dev)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.stream(main):
        with torch.cuda.graph(g, stream=main):
            a.add_(1.0)                         # main
            side.wait_stream(main)              # fork 1
            with torch.cuda.stream(side):
                b.mul_(2.0).add_(a)             # side reads main's a
            torch.mul(a, 3.0, out=d)            # main, beside it
            main.wait_stream(side)              # join 1
            torch.add(b, d, out=c)
            side.wait_stream(main)              # fork 2
            with torch.cuda.stream(side):
                e.add_(c)
            f.add_(1.0)
            main.wait_stream(side)              # join 2
            c.add_(e)
    lanes = pkg.ops.SplitGraph(g, dev)
    try:
        assert lanes.info["lane0_kernels"] and lanes.info["lane1_kernels"], lanes.info
        filler = _Filler(dev)
        values = (5.0, -2.0, 9.0)
        for v in values:
            filler.enqueue()
            a.fill_(v)  # what the replay reads, queued behind the filler
            lanes.replay()
        torch.cuda.synchronize()
        busy = filler.seconds()
        print(f"filler: {filler.units} units, {[f'{t:.3f}' for t in busy]} s; "
              f"timeouts {lanes.timeouts()}, fault {pkg.ops.handoff_fault(dev)}")
        assert min(busy) >= BUSY_S, busy  # else the test shows nothing
        ea = eb = ec = ed = ee = ef = 0.0
        for v in values:
            ea = v + 1.0
            eb = 2.0 * eb + ea
            ed = 3.0 * ea
            ec = eb + ed
            ee += ec
            ef += 1.0
            ec += ee
        # small integers throughout: every buffer exact in fp32
        got = [t[0].item() for t in (a, b, c, d, e, f)]
        for t, v in ((a, ea), (b, eb), (c, ec), (d, ed), (e, ee), (f, ef)):
            assert torch.all(t == v), (got, (ea, eb, ec, ed, ee, ef))
        assert lanes.timeouts() == 0
        assert not pkg.ops.handoff_fault(dev)
    finally:
        torch.cuda.synchronize()
        lanes.close()
        pkg.ops.clear_handoff_fault(dev)


def _state(model, opt):
    out = {n: p.detach().clone() for n, p in model.named_parameters()}
    out.update({"buf." + n: b.detach().clone() for n, b in model.named_buffers()})
    for n, p in model.named_parameters():
        st = opt.state.get(p)
        if st:
            for k, v in st.items():
                if torch.is_tensor(v):
                    out[f"opt.{n}.{k}"] = v.detach().clone()
    return out


def _assert_bitwise(sa, sb):
    assert sa.keys() == sb.keys()
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad[:10]


def test_split_pretrain_step_matches_whole_replay(pkg, dev):
    import bench
    from test_gpu_trajectory import _pretrain_model
    if not pkg.ops.xq_enabled():
        pytest.skip(f"hand-offs off here: {pkg.ops.XQ_REASON}")
    k, B, K, POOL = 1, 128, 6, 3
    F_in = pkg.synth.WORKLOADS["qm9"][2]
    hosts = [pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=30 + i))[0]
             for i in range(POOL)]
    n_cap = pkg.graph.StaticBatch.capacities(hosts, k, slack=1.02)[0]
    gen = torch.Generator().manual_seed(77)
    noise = [(torch.rand(n_cap, generator=gen), torch.rand(n_cap, 64, generator=gen))
             for _ in range(K)]
    runs = []
    for split in (False, True):
        model = _pretrain_model(pkg, F_in, k, B, dev)
        opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
        s_ug = torch.zeros(n_cap, device=dev)
        s_uf = torch.zeros(n_cap, 64, device=dev)
        rs = bench.build_replay_step(model, opt, hosts, k, B, dev, prefetch=True,
                                     noise=(s_ug, s_uf), split=split)
        assert (rs.split is not None) == split
        if split:
            assert rs.split.info["serialised"] == 0, rs.split.info
        losses = []
        for j in range(K):
            s_ug.copy_(noise[j][0])
            s_uf.copy_(noise[j][1])
            kl, rec, con = rs.step(j)
            losses.append(torch.stack([kl, rec, con]).clone())
        torch.cuda.synchronize()
        assert pkg.ops.xq_timeouts(dev) == 0
        runs.append((torch.stack(losses), _state(model, opt)))
        if rs.split is not None:
            rs.split.close()
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    _assert_bitwise(runs[0][1], runs[1][1])


def test_split_pretrain_step_behind_busy_stream(pkg, dev):
    """The pretrain step, split and whole, with >= 0.3 s of queued work ahead
    of replays 1 and 3 (then that replay's noise, written on the device): the
    split replay must still compute bitwise what the whole one does, with no
    wait giving up."""
    import bench
    from test_gpu_trajectory import _pretrain_model
    if not pkg.ops.xq_enabled():
        pytest.skip(f"hand-offs off here: {pkg.ops.XQ_REASON}")
    k, B, K, POOL = 1, 128, 4, 3
    F_in = pkg.synth.WORKLOADS["qm9"][2]
    hosts = [pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=30 + i))[0]
             for i in range(POOL)]
    n_cap = pkg.graph.StaticBatch.capacities(hosts, k, slack=1.02)[0]
    gen = torch.Generator().manual_seed(78)
    # resident on the device: a copy from pageable host memory would drain the stream
    noise = [(torch.rand(n_cap, generator=gen).to(dev), torch.rand(n_cap, 64, generator=gen).to(dev))
             for _ in range(K)]
    filler = _Filler(dev)
    runs = []
    try:
        for split in (False, True):
            model = _pretrain_model(pkg, F_in, k, B, dev)
            opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
            s_ug = torch.zeros(n_cap, device=dev)
            s_uf = torch.zeros(n_cap, 64, device=dev)
            rs = bench.build_replay_step(model, opt, hosts, k, B, dev, prefetch=True,
                                         noise=(s_ug, s_uf), split=split)
            try:
                assert (rs.split is not None) == split
                torch.cuda.synchronize()
                losses = []
                for j in range(K):
                    if j in (1, 3):
                        filler.enqueue()
                    s_ug.copy_(noise[j][0])
                    s_uf.copy_(noise[j][1])
                    kl, rec, con = rs.step(j)
                    losses.append(torch.stack([kl, rec, con]).clone())
                torch.cuda.synchronize()
                assert pkg.ops.xq_timeouts(dev) == 0
                assert not pkg.ops.handoff_fault(dev)
                runs.append((torch.stack(losses), _state(model, opt)))
            finally:
                torch.cuda.synchronize()
                if rs.split is not None:
                    rs.split.close()
        busy = filler.seconds()
        print(f"filler: {filler.units} units, {[f'{t:.3f}' for t in busy]} s")
        assert len(busy) == 4 and min(busy) >= BUSY_S, busy
        assert torch.isfinite(runs[0][0]).all()
        assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
        _assert_bitwise(runs[0][1], runs[1][1])
    finally:
        pkg.ops.clear_handoff_fault(dev)


def test_noise_prefetch_matches_inline_draw(pkg, dev):
    """ops.NoisePrefetch: the bench's replayed step with its compression
    noise drawn one step ahead (by the step before's backward, at the end of
    the core chain) computes bitwise what the step drawing it at the head of
    its forward computes — the same Philox draws in the same order."""
    import bench
    from test_gpu_trajectory import _pretrain_model
    k, B, K, POOL = 1, 128, 6, 3
    F_in = pkg.synth.WORKLOADS["qm9"][2]
    hosts = [pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=40 + i))[0]
             for i in range(POOL)]
    runs = []
    for ahead in (False, True):
        model = _pretrain_model(pkg, F_in, k, B, dev)
        opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
        pkg.ops.seed_noise(dev, 2024)
        rs = bench.build_replay_step(model, opt, hosts, k, B, dev, prefetch=True,
                                     noise_prefetch=ahead)
        assert (rs.noise_prefetch is not None) == ahead
        losses = []
        for j in range(K):
            kl, rec, con = rs.step(j)
            losses.append(torch.stack([kl, rec, con]).clone())
        torch.cuda.synchronize()
        assert pkg.ops.xq_timeouts(dev) == 0
        runs.append((torch.stack(losses), _state(model, opt)))
        if rs.split is not None:
            rs.split.close()
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    _assert_bitwise(runs[0][1], runs[1][1])


def test_split_finetune_step_matches_whole_replay(pkg, dev):
    import finetune_bench
    if not pkg.ops.xq_enabled():
        pytest.skip(f"hand-offs off here: {pkg.ops.XQ_REASON}")
    B, K, POOL = 32, 6, 3
    F_in = pkg.synth.WORKLOADS["molhiv"][2]
    hosts = [pkg.graph.collate_pyg(pkg.synth.molecules(B, "molhiv", seed=60 + i))[0]
             for i in range(POOL)]
    gen = torch.Generator().manual_seed(5)
    targets = [torch.randint(0, 2, (B, 1), generator=gen).float() for _ in range(POOL)]
    runs = []
    for split in (False, True):
        ft, k = finetune_bench.make_finetune_model(pkg, F_in, B, dev, seed=11)
        n_cap = pkg.graph.StaticBatch.capacities(hosts, k, slack=1.02)[0]
        if not runs:
            ng = torch.Generator().manual_seed(8)
            noise = [(torch.rand(n_cap, generator=ng), torch.rand(n_cap, 64, generator=ng))
                     for _ in range(K)]
        opt = pkg.optim.Adam(ft.parameters(), lr=1e-3, weight_decay=1e-5)
        s_ug = torch.zeros(n_cap, device=dev)
        s_uf = torch.zeros(n_cap, 64, device=dev)
        fs = finetune_bench.build_finetune_step(pkg, ft, opt, hosts, targets, k, B, dev,
                                                prefetch=True, noise=(s_ug, s_uf), split=split)
        assert (fs.split is not None) == split
        losses = []
        for j in range(K):
            s_ug.copy_(noise[j][0])
            s_uf.copy_(noise[j][1])
            fs.replay()
            losses.append(torch.cat([fs.loss.reshape(1), fs.scores.reshape(-1)]).clone())
        torch.cuda.synchronize()
        assert pkg.ops.xq_timeouts(dev) == 0
        runs.append((torch.stack(losses), _state(ft, opt)))
        if fs.split is not None:
            fs.split.close()
    assert torch.equal(runs[0][0], runs[1][0])
    _assert_bitwise(runs[0][1], runs[1][1])


def test_finetune_noise_prefetch_matches_inline_draw(pkg, dev):
    """The fine-tune step (frozen lower GIN layers, as finetune_bench builds
    it) with ops.NoisePrefetch computes bitwise what the inline draw gives."""
    import finetune_bench
    B, K, POOL = 32, 6, 3
    F_in = pkg.synth.WORKLOADS["molhiv"][2]
    hosts = [pkg.graph.collate_pyg(pkg.synth.molecules(B, "molhiv", seed=70 + i))[0]
             for i in range(POOL)]
    gen = torch.Generator().manual_seed(6)
    targets = [torch.randint(0, 2, (B, 1), generator=gen).float() for _ in range(POOL)]
    runs = []
    for ahead in (False, True):
        ft, k = finetune_bench.make_finetune_model(pkg, F_in, B, dev, seed=12)
        opt = pkg.optim.Adam(ft.parameters(), lr=1e-3, weight_decay=1e-5)
        pkg.ops.seed_noise(dev, 77)
        fs = finetune_bench.build_finetune_step(pkg, ft, opt, hosts, targets, k, B, dev,
                                                prefetch=True, noise_prefetch=ahead)
        assert (fs.noise_prefetch is not None) == ahead
        losses = []
        for _ in range(K):
            fs.replay()
            losses.append(torch.cat([fs.loss.reshape(1), fs.scores.reshape(-1)]).clone())
        torch.cuda.synchronize()
        assert pkg.ops.xq_timeouts(dev) == 0
        runs.append((torch.stack(losses), _state(ft, opt)))
        if fs.split is not None:
            fs.split.close()
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    _assert_bitwise(runs[0][1], runs[1][1])


def test_fused_final_reduce_adam_matches_separate(pkg, dev, monkeypatch):
    """scgib_adam_step_reduce (ops.fuse_final_into_step): the bench's replayed
    step with the ego chain's final weight-gradient reduce and Adam in one
    launch computes bitwise what the two launches compute — losses, every
    parameter, Adam's moments and steps — over 6 replays."""
    import bench
    from test_gpu_trajectory import _pretrain_model
    k, B, K, POOL = 1, 128, 6, 3
    monkeypatch.setattr(pkg.ops, "FUSE_FINAL_MIN_SLABS", 0)  # (whatever the default gate)
    F_in = pkg.synth.WORKLOADS["qm9"][2]
    hosts = [pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=80 + i))[0]
             for i in range(POOL)]
    runs = []
    real_call, calls = pkg._lib.call, {}

    def counting_call(name, *args):
        calls[name] = calls.get(name, 0) + 1
        return real_call(name, *args)

    monkeypatch.setattr(pkg._lib, "call", counting_call)
    for fuse in (False, True):
        model = _pretrain_model(pkg, F_in, k, B, dev)
        opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
        pkg.ops.seed_noise(dev, 99)
        calls.clear()
        rs = bench.build_replay_step(model, opt, hosts, k, B, dev, prefetch=True, fuse_adam=fuse)
        # the warm-ups and the capture took the path under test: the fused
        # launch when asked for and only then, the plain Adam launch otherwise
        n_fused, n_plain = calls.get("scgib_adam_step_reduce", 0), calls.get("scgib_adam_step", 0)
        assert (n_fused >= 1 and n_plain == 0) if fuse else (n_fused == 0 and n_plain >= 1), \
            (fuse, n_fused, n_plain)
        assert not pkg.ops._FINAL_PENDING and not pkg.ops._FINAL_ARMED[0]
        losses = []
        for j in range(K):
            kl, rec, con = rs.step(j)
            losses.append(torch.stack([kl, rec, con]).clone())
        torch.cuda.synchronize()
        assert pkg.ops.xq_timeouts(dev) == 0
        runs.append((torch.stack(losses), _state(model, opt)))
        if rs.split is not None:
            rs.split.close()
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    _assert_bitwise(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------
# the final reduce left to the Adam launch (ops.fuse_final_into_step) where
# its conditions do not hold: eager steps on a small batch
# ---------------------------------------------------------------------------
B_EAGER = 32


def _eager_batches(pkg, dev, count, seed=300):
    """``count`` QM9 batches on the device with explicit compression noise."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i in range(count):
        gh = pkg.graph.collate_pyg(pkg.synth.molecules(B_EAGER, "qm9", seed=seed + i))[0]
        g = gh.to(dev)
        n = g.num_nodes()
        out.append((g, F.normalize(g.ndata["x"].float()),
                    (torch.rand(n, generator=gen).to(dev), torch.rand(n, 64, generator=gen).to(dev))))
    return out


def _eager_model(pkg, dev):
    from test_gpu_trajectory import _pretrain_model
    model = _pretrain_model(pkg, pkg.synth.WORKLOADS["qm9"][2], 1, B_EAGER, dev)
    return model, pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)


def _fwd_bwd(model, item, dev):
    g, x, noise = item
    _, kl, con, rec = model(g, x, None, None, None, 1, None, 1, dev, B_EAGER, noise=noise)
    (kl + con + rec).backward()


def _grads(model):
    return {"grad." + n: p.grad.detach().clone() for n, p in model.named_parameters()
            if p.grad is not None}


@pytest.mark.parametrize("start", ["zeros", "none"])
def test_fused_final_with_gradient_accumulation(pkg, dev, monkeypatch, start):
    """Two backward passes into one optimizer step, inside and outside
    fuse_final_into_step(): the same arithmetic in the same order, so every
    .grad, parameter and Adam state tensor is bitwise equal.  ``zeros``: the
    gradients exist before the first backward (zero_grad(set_to_none=False)),
    so autograd adds the encoder pair's weight-gradient views at once — a
    reduce left to the step would not have written them yet.  ``none``: the
    first backward may defer, the second must reduce both before autograd
    accumulates."""
    import contextlib
    monkeypatch.setattr(pkg.ops, "FUSE_FINAL_MIN_SLABS", 0)
    batches = _eager_batches(pkg, dev, 2)
    runs = []
    for armed in (False, True):
        model, opt = _eager_model(pkg, dev)
        if start == "zeros":
            _fwd_bwd(model, batches[0], dev)  # (gradients to zero in place)
            opt.zero_grad(set_to_none=False)
            have = [p for p in model.parameters() if p.grad is not None]
            assert have and not any(p.grad.any() for p in have)
        else:
            opt.zero_grad(set_to_none=True)
        # (same BatchNorm running statistics on both sides: the priming pass ran on both)
        with (pkg.ops.fuse_final_into_step() if armed else contextlib.nullcontext()):
            _fwd_bwd(model, batches[0], dev)
            _fwd_bwd(model, batches[1], dev)
            opt.step()
        torch.cuda.synchronize()
        assert not pkg.ops._FINAL_PENDING
        st = _state(model, opt)
        st.update(_grads(model))
        runs.append(st)
    assert any(k.startswith("grad.") and "Encoder2" in k for k in runs[0])
    assert all(torch.isfinite(v).all() for v in runs[0].values())
    _assert_bitwise(runs[0], runs[1])


def test_fused_final_refuses_rebound_gradient(pkg, dev, monkeypatch):
    """A .grad re-bound between the backward and the step is no longer what
    the pending reduce writes: the step must raise (after launching the
    reduces, so nothing is lost) and leave the parameters alone."""
    monkeypatch.setattr(pkg.ops, "FUSE_FINAL_MIN_SLABS", 0)
    (item,) = _eager_batches(pkg, dev, 1)
    model, opt = _eager_model(pkg, dev)
    opt.zero_grad(set_to_none=True)
    with pkg.ops.fuse_final_into_step():
        _fwd_bwd(model, item, dev)
        assert pkg.ops._FINAL_PENDING  # the path under test: the reduce is pending
        w = pkg.ops._gin_layer_params(model.model.Encoder2)[0]
        w.grad = w.grad.clone()
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        with pytest.raises(pkg._lib.ScgibError, match=r"un-aliased gradient: .*\(64, 32\)"):
            opt.step()
        assert not pkg.ops._FINAL_PENDING
        torch.cuda.synchronize()
        for n, p in model.named_parameters():
            assert torch.equal(p, before[n]), n
    assert not pkg.ops._FINAL_PENDING


def test_fused_final_survives_a_failed_step(pkg, dev, monkeypatch):
    """An exception while the step builds its tensor table must not lose the
    pending reduces: the next step() then gives bitwise the unfused result."""
    monkeypatch.setattr(pkg.ops, "FUSE_FINAL_MIN_SLABS", 0)
    (item,) = _eager_batches(pkg, dev, 1)
    model, opt = _eager_model(pkg, dev)
    opt.zero_grad(set_to_none=True)
    _fwd_bwd(model, item, dev)
    opt.step()
    torch.cuda.synchronize()
    want = _state(model, opt)
    want.update(_grads(model))

    model, opt = _eager_model(pkg, dev)
    opt.zero_grad(set_to_none=True)
    real, n_calls = pkg.optim.Adam._entries, [0]

    def entries(self, group):
        n_calls[0] += 1
        if n_calls[0] == 1:
            raise RuntimeError("entries failed once")
        return real(self, group)

    monkeypatch.setattr(pkg.optim.Adam, "_entries", entries)
    with pkg.ops.fuse_final_into_step():
        _fwd_bwd(model, item, dev)
        assert pkg.ops._FINAL_PENDING
        with pytest.raises(RuntimeError, match="entries failed once"):
            opt.step()
        assert pkg.ops._FINAL_PENDING and sum(len(v) for v in pkg.ops._FINAL_PENDING.values()) == 1
        opt.step()
        assert not pkg.ops._FINAL_PENDING
    torch.cuda.synchronize()
    got = _state(model, opt)
    got.update(_grads(model))
    _assert_bitwise(want, got)


def test_split_refused_when_capture_used_torch_rng(pkg, dev, monkeypatch):
    """SplitGraph.replay() launches the lanes itself, so torch's per-replay
    Philox offset update never runs: a capture that drew with torch.rand must
    be replayed whole (fresh noise every step), and the refusal must not
    stick to the next split."""
    import bench
    if not pkg.ops.xq_enabled():
        pytest.skip(f"hand-offs off here: {pkg.ops.XQ_REASON}")
    k, B, POOL = 1, 32, 1
    F_in = pkg.synth.WORKLOADS["qm9"][2]
    hosts = [pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=90))[0]]
    from test_gpu_trajectory import _pretrain_model

    def build():
        model = _pretrain_model(pkg, F_in, k, B, dev)
        # lr = 0: the parameters stay put, so two replays of the one batch
        # differ in nothing but their noise
        opt = pkg.optim.Adam(model.parameters(), lr=0.0, weight_decay=5e-5)
        return bench.build_replay_step(model, opt, hosts, k, B, dev, prefetch=True, split=True,
                                       noise=None)

    with monkeypatch.context() as m:
        m.setattr(pkg.models, "DEVICE_NOISE", False)
        torch.manual_seed(123)
        rs = build()
        assert rs.split is None
        assert pkg.ops._TORCH_RNG_CAPTURE[0] is None  # read and cleared
        kls = []
        for j in range(2):
            kl, rec, con = rs.step(j)
            kls.append(kl.clone())
        torch.cuda.synchronize()
        assert torch.isfinite(kls[0]) and torch.isfinite(kls[1])
        assert kls[0].item() != kls[1].item(), kls
    rs = build()
    try:
        assert rs.split is not None
    finally:
        torch.cuda.synchronize()
        if rs.split is not None:
            rs.split.close()
