"""scgib_enc_out_linear_fwd (csrc/dense.hip): the encoder output's BatchNorm +
ReLU and compressor[0] in one launch.

Through the C ABI against the two entries it replaces in the same library
(scgib_bn_relu_apply then scgib_linear_fwd): every output bit for bit, the BN
record and the running statistics after one call each from equal starts.
Against a float64 torch restatement:
  * the BN record and the running statistics at rel_err < 1e-5 (the BN
    buffers' tolerance of tests/test_gpu_parity.py);
  * f element by element within the fp32 rounding of scale * z + shift, that
    is 2 ulp of |scale z| + |shift| — a relative bound on f itself does not
    exist where the two terms cancel (one row: z equals the mean);
  * t = f W0^T + b0 from the device's own f at rel_l2 < 1e-6 (the forward
    tolerance of test_mlp2_fwd_bwd there).
Row counts: the tile edge (1, 63, 64, 65), one 16-tile statistics group and
the first row of a second (1024, 1025), a partial third group (2049), 257
tiles (16385) and 33 groups (32769: the second load round of bn_fwd_final).
Every output buffer is NaN before the call, has guard rows behind it that
must stay NaN, and holds no NaN in its n rows afterwards.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from conftest import rel_err, rel_l2

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 1024, 1025, 2049, 16385, 32769]
# (capacity, dims[0]): a partial tile and a whole padding tile | a tile edge |
# one full tile and two padding tiles
CAPACITY = [(192, 65), (192, 128), (192, 64)]
GUARD = 3          # rows behind every output that no launch may touch
EPS, MOMENTUM = 1e-5, 0.1
GROUP_ROWS = 16 * 64  # rows of a statistics group (kGroup tiles)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _case(n_valid, cap, seed):
    """Inputs (host, fp32): z2 [cap][64] whose rows past n_valid hold
    live-looking values, W0, b0, gamma, beta, running statistics."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)  # noqa: E731
    z = 1.5 * rnd(n_valid, 64) + 0.5 * rnd(64)
    z = torch.cat([z, 3 + torch.rand(cap - n_valid, 64, generator=gen)])
    return {"z": z, "w": 0.2 * rnd(64, 64), "b": 0.1 * rnd(64), "gamma": 1 + 0.2 * rnd(64),
            "beta": 0.2 * rnd(64), "rm": rnd(64), "rv": 0.5 + torch.rand(64, generator=gen)}


def _reference(c, n_valid):
    """float64 restatement: BN record over the valid rows, running update."""
    z = c["z"][:n_valid].double()
    mean = z.mean(0)
    m2 = ((z - mean) ** 2).sum(0)
    istd = 1.0 / torch.sqrt(m2 / n_valid + EPS)
    scale = c["gamma"].double() * istd
    shift = c["beta"].double() - mean * scale
    unbiased = m2 / (n_valid - 1) if n_valid > 1 else m2
    return {"stat": torch.stack([mean, istd, scale, shift]),
            "rm": (1 - MOMENTUM) * c["rm"].double() + MOMENTUM * mean,
            "rv": (1 - MOMENTUM) * c["rv"].double() + MOMENTUM * unbiased}


def _group_partials(c, n_valid):
    """What a deferred layer leaves (scgib_bn_pending.gpart): per 1024-row
    group the channel sums and the M2 centred on the group's mean, fp64."""
    z = c["z"][:n_valid].double()
    rows = []
    for r0 in range(0, n_valid, GROUP_ROWS):
        zg = z[r0:r0 + GROUP_ROWS]
        s = zg.sum(0)
        rows.append(torch.cat([s, ((zg - s / zg.shape[0]) ** 2).sum(0)]))
    return torch.stack(rows).contiguous()


def _run(pkg, dev, c, n_valid, cap, mode, fused, capacity):
    """One forward of the tail through the C ABI: the new entry (fused) or
    the two it replaces.  Returns the outputs and the BN state, on the host."""
    ops, lib = pkg.ops, pkg._lib
    p, st = ops._p, ops._stream()
    d = {k: v.to(dev).contiguous() for k, v in c.items()}
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)  # noqa: E731
    f, t = nan(cap + GUARD, 64), nan(cap + GUARD, 64)
    dims = torch.tensor([n_valid, 0], dtype=torch.int32, device=dev) if capacity else None
    nbt = torch.tensor([7], dtype=torch.int64, device=dev)
    if mode == "pending":
        gpart = _group_partials(c, n_valid).to(dev)
        stat = nan(4, 64)
        pend = lib.BnPending(gpart.data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(),
                             d["rm"].data_ptr(), d["rv"].data_ptr(), nbt.data_ptr(),
                             stat.data_ptr(), EPS, MOMENTUM)
        pref = ops._byref(pend)
    else:
        stat = _reference(c, n_valid)["stat"].float().to(dev).contiguous()
        pref = None
    if fused:
        lib.call("scgib_enc_out_linear_fwd", p(d["z"]), p(stat), cap, p(d["w"]), p(d["b"]), p(f),
                 p(t), p(dims), pref, st)
    else:
        lib.call("scgib_bn_relu_apply", p(d["z"]), p(stat), cap, p(f), p(dims), pref, st)
        lib.call("scgib_linear_fwd", p(f), cap, p(d["w"]), p(d["b"]), p(t), p(dims), st)
    torch.cuda.synchronize()
    return {"f": f.cpu().numpy(), "t": t.cpu().numpy(), "stat": stat.cpu().numpy(),
            "rm": d["rm"].cpu().numpy(), "rv": d["rv"].cpu().numpy(), "nbt": nbt.cpu().numpy()}


def _check(pkg, dev, n_valid, cap, mode, capacity):
    c = _case(n_valid, cap, seed=1000 + n_valid + cap)
    new = _run(pkg, dev, c, n_valid, cap, mode, True, capacity)
    old = _run(pkg, dev, c, n_valid, cap, mode, False, capacity)
    # the two entries it replaces, bit for bit (NaN guard rows included)
    for k in new:
        assert np.array_equal(new[k], old[k], equal_nan=True), k
    # fresh outputs: every row up to the capacity written, nothing behind it
    for k in ("f", "t"):
        assert not np.isnan(new[k][:cap]).any(), k
        assert np.isnan(new[k][cap:]).all(), k
        assert not new[k][n_valid:cap].any(), k  # padding rows: exact zeros
    ref = _reference(c, n_valid)
    if mode == "pending":
        # the record and the running update, written exactly once: the sums
        # count the valid rows only
        assert rel_err(new["stat"], ref["stat"].numpy()) < 1e-5
        assert rel_err(new["rm"], ref["rm"].numpy()) < 1e-5
        assert rel_err(new["rv"], ref["rv"].numpy()) < 1e-5
        assert int(new["nbt"][0]) == 8
    else:
        assert np.array_equal(new["rm"], c["rm"].numpy()) and int(new["nbt"][0]) == 7
    scale, shift = (new["stat"][i].astype(np.float64) for i in (2, 3))
    z = c["z"][:n_valid].double().numpy()
    f_ref = np.maximum(scale * z + shift, 0.0)
    bound = 2 * np.finfo(np.float32).eps * (np.abs(scale * z) + np.abs(shift)) + 1e-30
    assert (np.abs(new["f"][:n_valid] - f_ref) <= bound).all()
    t_ref = new["f"][:n_valid].astype(np.float64) @ c["w"].double().numpy().T + c["b"].double().numpy()
    assert rel_l2(new["t"][:n_valid], t_ref) < 1e-6


@pytest.mark.parametrize("mode", ["pending", "stat"])
@pytest.mark.parametrize("n", ROWS)
def test_enc_out_linear_fwd_matches_apply_then_linear(pkg, dev, n, mode):
    _check(pkg, dev, n, n, mode, capacity=False)


@pytest.mark.parametrize("mode", ["pending", "stat"])
@pytest.mark.parametrize("cap,n_valid", CAPACITY)
def test_enc_out_linear_fwd_capacity_padding(pkg, dev, cap, n_valid, mode):
    _check(pkg, dev, n_valid, cap, mode, capacity=True)


def test_enc_out_linear_fwd_rejects_bad_arguments(pkg, dev):
    ops, lib = pkg.ops, pkg._lib
    p = ops._p
    x = torch.zeros(64, 64, device=dev)
    fn = lib.load().scgib_enc_out_linear_fwd
    # neither a record nor pending statistics; a missing output
    assert fn(p(x), None, 64, p(x), None, p(x), p(x), None, None, ops._stream()) < 0
    assert fn(p(x), p(x), 64, p(x), None, None, p(x), None, None, ops._stream()) < 0
    # no rows: nothing to do
    assert fn(p(x), p(x), 0, p(x), None, p(x), p(x), None, None, ops._stream()) == 0


def _state(model, opt):
    out = {n: q.detach().clone() for n, q in model.named_parameters()}
    out.update({"buf." + n: b.detach().clone() for n, b in model.named_buffers()})
    for n, q in model.named_parameters():
        for k, v in (opt.state.get(q) or {}).items():
            if torch.is_tensor(v):
                out[f"opt.{n}.{k}"] = v.detach().clone()
    return out


def test_replayed_step_same_bits_with_and_without_fused_tail(pkg, dev, monkeypatch):
    """ops.FUSE_ENC_TAIL on and off: the bench's replayed pretrain step
    (B = 32 QM9-like pool) gives equal losses, parameters, Adam moments and BN
    buffers over 4 replays, and each side took its own launches — a silently
    taken old path fails the count."""
    import bench
    from test_gpu_trajectory import _pretrain_model
    k, B, K, POOL = 1, 32, 4, 3
    F_in = pkg.synth.WORKLOADS["qm9"][2]
    hosts = [pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=90 + i))[0]
             for i in range(POOL)]
    real_call, calls = pkg._lib.call, {}

    def counting_call(name, *args):
        calls[name] = calls.get(name, 0) + 1
        return real_call(name, *args)

    monkeypatch.setattr(pkg._lib, "call", counting_call)
    runs = []
    for fuse in (True, False):
        monkeypatch.setattr(pkg.ops, "FUSE_ENC_TAIL", fuse)
        model = _pretrain_model(pkg, F_in, k, B, dev)
        opt = pkg.optim.Adam(model.parameters(), lr=1e-4, weight_decay=5e-5)
        pkg.ops.seed_noise(dev, 99)
        calls.clear()
        rs = bench.build_replay_step(model, opt, hosts, k, B, dev, prefetch=True)
        n_new = calls.get("scgib_enc_out_linear_fwd", 0)
        n_apply, n_lin = calls.get("scgib_bn_relu_apply", 0), calls.get("scgib_linear_fwd", 0)
        assert (n_new >= 1 and n_apply == 0 and n_lin == 0) if fuse else \
            (n_new == 0 and n_apply >= 1 and n_lin >= 1), (fuse, n_new, n_apply, n_lin)
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
    assert runs[0][1].keys() == runs[1][1].keys()
    bad = [n for n in runs[0][1] if not torch.equal(runs[0][1][n], runs[1][1][n])]
    assert not bad, bad[:10]
