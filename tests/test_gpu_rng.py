"""The device random streams, bit for bit against tests/philox_ref.py (itself
held to the Random123 known-answer vectors by tests/test_philox_cpu.py):

  * the compression noise of scgib_noise_uniform (csrc/interaction.hip), at
    row counts around its 16-row workgroups and past one grid-stride pass
    (256 workgroups x 16 rows), seeds and offsets with high words, the state
    and arrival counter after each launch, and guard rows past n;
  * the FFN dropout keep bits of scgib_gt_ffn_fwd (csrc/gt_layer.hip), on the
    Transformer suite's small cases and in capacity mode.

Every comparison is exact equality: no tolerance, no statistics."""
import numpy as np
import pytest
import torch

import philox_ref as P
from test_gpu_transformer import Case, H, F2, make_layer

pytestmark = pytest.mark.gpu

GUARD = 40         # sentinel rows past n
SENTINEL = -7.0    # no uniform is negative
SEED_B31 = 0x80000001                    # bit 31 of the low key word
SEED_HI = (0x1234ABCD << 32) | 0x9E3779B9  # a non-zero high key word (and bit 31 below it)
OFF_HI = 2 ** 32 + 5                     # a non-zero high offset word


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _noise_ref(seed, off, n):
    rows = np.arange(n)
    return P.noise_gate(seed, off, rows), P.noise_feat(seed, off, rows)


def _draw_guarded(pkg, dev, n):
    """One scgib_noise_uniform launch of n rows into buffers with GUARD
    sentinel rows behind them; returns the whole buffers."""
    ops = pkg.ops
    ug = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    uf = torch.full((n + GUARD, 64), SENTINEL, dtype=torch.float32, device=dev)
    pkg._lib.call("scgib_noise_uniform", ops._p(ug), ops._p(uf), n, ops._p(ops.noise_state(dev)),
                  ops._p(ops.counters(dev, "noise", 1)), ops._stream())
    torch.cuda.synchronize()
    return ug.cpu().numpy(), uf.cpu().numpy()


# 1 / 15 / 16 / 17: below, at and past one 16-row workgroup; 4096 = exactly one
# pass of the 256-workgroup grid; 4097 / 4113: a second grid-stride pass of one
# row / of one workgroup and a ragged row
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096, 4097, 4113])
@pytest.mark.parametrize("seed,off", [(1234, 0), (SEED_B31, OFF_HI), (SEED_HI, 0), (SEED_HI, OFF_HI)])
def test_noise_stream_bit_exact(pkg, dev, n, seed, off):
    ops = pkg.ops
    st = ops.seed_noise(dev, seed, off)
    cnt = ops.counters(dev, "noise", 1)
    # first launch: the op
    ug, uf = ops.device_noise(n, dev)
    torch.cuda.synchronize()
    rg, rf = _noise_ref(seed, off, n)
    assert ug.shape == (n,) and uf.shape == (n, 64)
    assert np.array_equal(ug.cpu().numpy(), rg)
    assert np.array_equal(uf.cpu().numpy(), rf)
    assert st.tolist() == [seed, off + 1]  # advanced once, whatever the grid
    assert int(cnt.item()) == 0
    # second launch: through the C ABI into guarded buffers, at off + 1
    ug2, uf2 = _draw_guarded(pkg, dev, n)
    rg2, rf2 = _noise_ref(seed, off + 1, n)
    assert np.array_equal(ug2[:n], rg2)
    assert np.array_equal(uf2[:n], rf2)
    assert (ug2[n:] == SENTINEL).all() and (uf2[n:] == SENTINEL).all()  # nothing past row n
    assert st.tolist() == [seed, off + 2]
    assert int(cnt.item()) == 0
    assert not np.array_equal(rf, rf2)


def test_noise_zero_rows_leaves_state(pkg, dev):
    ops = pkg.ops
    st = ops.seed_noise(dev, SEED_HI, OFF_HI)
    ug, uf = _draw_guarded(pkg, dev, 0)
    assert (ug == SENTINEL).all() and (uf == SENTINEL).all()
    assert st.tolist() == [SEED_HI, OFF_HI]
    assert int(ops.counters(dev, "noise", 1).item()) == 0
    ug, uf = ops.device_noise(0, dev)
    torch.cuda.synchronize()
    assert ug.shape == (0,) and uf.shape == (0, 64) and st.tolist() == [SEED_HI, OFF_HI]


def test_noise_prefetch_draws_consecutive_offsets(pkg, dev):
    """NoisePrefetch.prime() then draw(): the reference at off, then off + 1,
    one offset per step as the inline draw."""
    ops = pkg.ops
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(5, "qm9", seed=2))
    g = gh.to(dev)
    n = g.num_nodes()
    assert n % 16 != 0
    st = ops.seed_noise(dev, SEED_B31, OFF_HI)
    pre = ops.NoisePrefetch(g, dev)
    assert g.noise_prefetch is pre and pre.n == n
    for step, fn in enumerate((pre.prime, pre.draw, pre.draw)):
        fn()
        torch.cuda.synchronize()
        rg, rf = _noise_ref(SEED_B31, OFF_HI + step, n)
        assert np.array_equal(pre.u_gate.cpu().numpy(), rg), step
        assert np.array_equal(pre.u_feat.cpu().numpy(), rf), step
        assert st.tolist() == [SEED_B31, OFF_HI + step + 1]


# ---------------------------------------------------------------------------
# FFN dropout keep bits
# ---------------------------------------------------------------------------
_CASES = {}


def _case(pkg, dev, name):
    if name not in _CASES:
        _CASES[name] = Case(pkg, dev, name)
    return _CASES[name]


def _keep(pkg, layer, g, h, drop_mask=None):
    with torch.no_grad():
        aux = pkg.ops.gt_layer(h, g, layer, drop_mask, return_aux=True)[1]
    torch.cuda.synchronize()
    return aux["keep"].cpu().numpy()


# isolated_first: 5 rows (one partly live tile); path65: two tiles, one row in
# the second; mols: > 3 tiles, rows no multiple of 64
@pytest.mark.parametrize("name", ["isolated_first", "path65", "mols"])
@pytest.mark.parametrize("seed,off", [(99, 0), (SEED_HI, OFF_HI)])
def test_dropout_keep_bit_exact(pkg, dev, name, seed, off):
    c = _case(pkg, dev, name)
    assert c.n % 64 != 0
    layer = make_layer(pkg, dev, 4, 8, True)
    h = torch.randn(c.n, H, generator=torch.Generator().manual_seed(3)).to(dev)
    st = pkg.ops.seed_dropout(dev, seed, off)
    cnt = pkg.ops.counters(dev, "gt_dropout", 1)
    rows = np.arange(c.n)
    for launch in range(2):  # the offset advances by exactly one per layer launch
        k = _keep(pkg, layer, c.g, h)
        assert k.shape == (c.n, F2) and k.dtype == bool
        assert np.array_equal(k, P.dropout_keep(seed, off + launch, rows)), launch
        assert st.tolist() == [seed, off + launch + 1]
        assert int(cnt.item()) == 0
    # a given mask is the mask used, and the state does not move
    mask = torch.from_numpy(P.dropout_keep(seed ^ 5, 17, rows)).to(dev)
    assert np.array_equal(_keep(pkg, layer, c.g, h, mask), mask.cpu().numpy())
    assert st.tolist() == [seed, off + 2]
    # eval draws nothing and keeps everything
    layer.eval()
    assert _keep(pkg, layer, c.g, h).all() and st.tolist() == [seed, off + 2]


def test_dropout_keep_capacity_mode(pkg, dev):
    """A StaticBatch with spare rows (whole spare tiles and a partly live one):
    live rows draw what the exact-size call draws, rows >= dims[0] read
    all-false, and the launch advances the offset once."""
    B = 47  # 876 rows: 44 live rows in the last live tile
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=21))
    n = gh.num_nodes()
    n_cap, e_cap, mgn, caps = pkg.graph.StaticBatch.capacities([gh], 1, slack=1.3)
    assert (n_cap + 63) // 64 > (n + 63) // 64 and n % 64 != 0
    static = pkg.graph.StaticBatch(B, n_cap, e_cap, gh.ndata["x"].shape[1], mgn, caps, dev)
    static.load(static.pad(gh))
    layer = make_layer(pkg, dev, 4, 8, True)
    h = torch.randn(n_cap, H, generator=torch.Generator().manual_seed(5)).to(dev)
    st = pkg.ops.seed_dropout(dev, SEED_B31, 7)
    k = _keep(pkg, layer, static.graph, h)
    assert k.shape == (n_cap, F2)
    assert np.array_equal(k[:n], P.dropout_keep(SEED_B31, 7, np.arange(n)))
    assert not k[n:].any()
    assert st.tolist() == [SEED_B31, 8]
    assert int(pkg.ops.counters(dev, "gt_dropout", 1).item()) == 0
