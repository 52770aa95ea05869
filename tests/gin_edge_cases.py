"""Row counts at which the fused GIN layers change code path, batches of
exactly that many rows, and the fp64 side of the checks that
tests/test_gpu_gin_edges.py (device) and tests/test_gin_edges_cpu.py (host)
share.  Plain module: no fixtures, no device work at import."""
from __future__ import annotations

import numpy as np
import torch

from oracle import scgib_ref as R

TILE = 64                   # rows of a forward tile (csrc TM)
SUB = 32                    # rows of a d = 64 backward sub-tile (csrc SM)
GROUP = 16 * TILE           # rows of a statistics group (kGroup tiles)
ROUND = 32 * GROUP          # rows one finish round covers (kFinG = 2 * kBFinR = 32 groups)
DEFER_MAX = 64 * GROUP      # scgib_gin_defer_max_nodes() == kSuper groups == ops.AGG_FREE_MIN_ROWS
F_RAW = 11                  # raw QM9 features (synth.WORKLOADS["qm9"])
LAYERS = 3                  # layer 0 (d_in = 32), a consumer of a deferred layer, the finishing layer
SEED = 41

# ---------------------------------------------------------------------------
# the case table (row counts of exact-mode batches, GIN(32, 64, 3), train and
# eval unless noted)
# ---------------------------------------------------------------------------
EXACT_ROWS = [
    # tile and sub-tile edges: one sub-tile | one row into the second | one row
    # short of a tile | a full tile (n % 64 == 0) | one row into a second tile |
    # a full tile and a full sub-tile
    32, 33, 63, 64, 65, 96,
    # statistics group edges: one tile short a row | a full (only) group, the
    # reciprocal-multiply branch of bn_fwd_final | one row into a second group
    # (gsize = 1, rows_in = 1, the divide branch)
    1023, 1024, 1025,
    # the d = 64 backward's sub-tile walk: 256 sub-tiles on 256 workgroups
    # (per = 1) | 257 (per = 2, the last workgroup walks one) | 513 (per = 3,
    # the last workgroup walks two)
    8192, 8193, 16385,
    # 32 groups: one finish round, and bwd_grid's cap of 512 tiles for the
    # d_in = 32 layer | 33 groups: the consumers reload and run a second round
    32768, 32769,
    # one row short of 64 full groups | the deferral limit, the agg-free
    # switch and a full last group at once | one row more: nothing deferred,
    # the supergroup level, a one-row second supergroup
    65535, 65536, 65537,
]
# two full supergroups (bn_fwd_final<true, kSupRows> without a partial entry):
# train only, two layers (the oracle's time)
FULL_SUPER_ROWS, FULL_SUPER_LAYERS = 2 * DEFER_MAX, 2
# path flips through ops.AGG_FREE_MIN_ROWS (train): (rows, agg-free layers l >= 1)
FLIP_CASES = [
    (1025, True), (32769, True),     # agg-free forced on: two groups | two finish rounds
    (65536, False), (65537, False),  # stored agg forced at the deferral limit and past it
]
# transfer_d folded into layer 0 (ops.gin_encoder_x, the layer-0 kernel with
# its own statistics calls): a full tile | a full group | a one-row group |
# two finish rounds | past the deferral limit
FOLD_ROWS = [64, 1024, 1025, 32769, 65537]
# capacity mode (valid rows, capacity), train: a full tile and two padding
# tiles | a full group inside a partial second | a one-row second group inside
# a one-row third | 32 full groups and one padding tile | then three where the
# host sizes the workspaces and decides deferral (none) and agg-free (on) from
# the capacity while the kernels take their statistics level from the valid
# count: valid at the limit | below it | one row past it
CAPACITY_CASES = [(64, 192), (1024, 1100), (1025, 2049), (32768, 32832), (65536, 65600),
                  (60000, 66000), (65537, 66000)]
# the boundary-weighted passes: (valid rows, capacity or None)
WEIGHTED_CASES = [(65, None), (1025, None), (8193, None), (32769, None), (65537, None),
                  (1025, 2049)]
UPSTREAM_ROWS = 33          # upstream gradient on the last min(n, 33) rows
OUTLIER_SHARE = 0.05        # of layer 0's centred sum of squares of z2


def case_layers(n_rows):
    return FULL_SUPER_LAYERS if n_rows == FULL_SUPER_ROWS else LAYERS


def all_row_counts():
    rows = set(EXACT_ROWS) | {FULL_SUPER_ROWS} | set(FOLD_ROWS)
    rows |= {n for n, _ in FLIP_CASES} | {n for n, _ in CAPACITY_CASES}
    return sorted(rows | {n for n, _ in WEIGHTED_CASES})


# ---------------------------------------------------------------------------
# batches of an exact row count
# ---------------------------------------------------------------------------
def _path(m, rng):
    a = np.arange(m - 1, dtype=np.int64)
    ei = np.stack([np.concatenate([a, a + 1]), np.concatenate([a + 1, a])])
    return ei, rng.random((m, F_RAW), dtype=np.float32)


_GRAPHS = {}


def exact_graph(pkg, n_rows, seed=SEED):
    """Host batch of exactly n_rows rows: synth.molecules(..., "qm9") molecules
    while they fit, then one path molecule of the remaining size (at least 2
    atoms: where 0 or 1 would remain, the previous molecule is given back), so
    the last rows of the batch are a path."""
    key = (n_rows, seed)
    if key in _GRAPHS:
        return _GRAPHS[key]
    assert n_rows >= 2
    # (QM9-like molecules have ~18 atoms; were the pool ever to run out, the
    # closing path takes what is left and the count is still exact)
    pool = pkg.synth.molecules(n_rows // 8 + 8, "qm9", seed=seed)
    mols, total = [], 0
    for ei, x in pool:
        if total + x.shape[0] > n_rows:
            break
        mols.append((ei, x))
        total += x.shape[0]
    if n_rows - total < 2 and mols:
        total -= mols.pop()[1].shape[0]
    mols.append(_path(n_rows - total, np.random.default_rng([seed, n_rows])))
    gh, kept = pkg.graph.collate_pyg(mols)
    assert len(kept) == len(mols) and gh.num_nodes() == n_rows
    _GRAPHS[key] = gh
    return gh


def capacity_graph(pkg, n_rows, cap, dev, seed=SEED):
    """exact_graph(n_rows) inside a StaticBatch of cap rows (the way
    tests/test_gpu_workspace_poison.py builds its "cap" shape, with the row
    capacity given): (static batch, host batch).  static.graph.dims holds the
    valid counts on the device."""
    gh = exact_graph(pkg, n_rows, seed)
    _, e_cap, mgn, caps = pkg.graph.StaticBatch.capacities([gh], 1, slack=1.0)
    static = pkg.graph.StaticBatch(gh.batch_size, cap, e_cap, F_RAW, mgn, caps, dev, k=1)
    static.load(static.pad(gh))
    return static, gh


# ---------------------------------------------------------------------------
# module, inputs, oracle
# ---------------------------------------------------------------------------
def make_gin(pkg, layers=LAYERS, seed=SEED):
    """GIN(32, 64, layers) on the host with test_fused_gin_encoder's BN
    parameter and running-statistic perturbation."""
    torch.manual_seed(seed + layers)
    gin = pkg.models.GIN(32, 64, layers)
    with torch.no_grad():
        for bn in gin.batch_norms:
            bn.weight.add_(0.3 * torch.randn(64))
            bn.bias.add_(0.3 * torch.randn(64))
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
    assert gin.fused
    return gin


def make_inputs(n_rows, rows=None, seed=SEED):
    """(h0 [rows, 32], upstream w [rows, 64]) fp32, the first n_rows rows a
    function of (n_rows, seed) alone; rows past them (capacity padding) hold
    live-looking values that nothing may read."""
    gen = torch.Generator().manual_seed(1000 * seed + n_rows)
    h0, w = torch.randn(n_rows, 32, generator=gen), torch.randn(n_rows, 64, generator=gen)
    pad = (rows or n_rows) - n_rows
    if pad:
        h0 = torch.cat([h0, 3 + torch.rand(pad, 32, generator=gen)])
        w = torch.cat([w, 3 + torch.rand(pad, 64, generator=gen)])
    return h0, w


def last_tile_rows(n_rows):
    return slice((n_rows - 1) // TILE * TILE, n_rows)


def with_outliers(h0, n_rows):
    """h0 with the rows of the last tile scaled by 2 sqrt(n / rows in it)."""
    s = last_tile_rows(n_rows)
    out = h0.clone()
    out[s] *= 2.0 * (n_rows / (s.stop - s.start)) ** 0.5
    return out


def upstream_mask(w, n_rows):
    """w supported on the last min(n, 33) valid rows only (capacity padding
    rows keep their live-looking values)."""
    out = w.clone()
    out[:max(n_rows - UPSTREAM_ROWS, 0)] = 0.0
    return out


def first_coupled_row(gh, n_rows):
    """First row of the molecule that holds row n - min(n, 33): no row before
    it shares a molecule with a row that has an upstream gradient."""
    ptr = np.concatenate([[0], np.cumsum(gh.batch_num_nodes_host())])
    lo = max(n_rows - UPSTREAM_ROWS, 0)
    return int(ptr[np.searchsorted(ptr, lo, side="right") - 1])


def oracle_params(gin, prefix="Encoder1"):
    """(fp64 parameter dict keyed like the oracle's, its BN buffers)."""
    p = {(prefix + "." + k): (v.detach().double() if v.is_floating_point() else v.detach()).clone()
         .requires_grad_(v.is_floating_point() and "running" not in k and not k.endswith(".eps"))
         for k, v in gin.state_dict().items()}
    bufs = {k: v for k, v in p.items() if "running" in k or "num_batches" in k}
    return p, bufs


def layer0_z2(p, src, dst, h0, prefix="Encoder1"):
    """The oracle's layer-0 pre-BatchNorm output z2 (fp64, no grad)."""
    with torch.no_grad():
        h = h0.double()
        lp = prefix + ".ginlayers.0"
        rst = h + torch.zeros_like(h).index_add(0, dst, h[src])
        z = torch.relu(R._linear(rst, p, lp + ".apply_func.mlp.0"))
        return R._linear(z, p, lp + ".apply_func.mlp.2")


def outlier_share(z2, n_rows):
    """Share of the centred sum of squares of z2 that the rows of the last
    tile hold: the median over channels."""
    d2 = (z2 - z2.mean(0)) ** 2
    return float((d2[last_tile_rows(n_rows)].sum(0) / d2.sum(0)).median())


def bn_record(z2, gamma, beta, eps=R.BN_EPS):
    """fp64 [4][64] BatchNorm record (mean, istd, scale, shift) of z2's rows."""
    z = z2.double()
    mean = z.mean(0)
    istd = 1.0 / torch.sqrt(((z - mean) ** 2).sum(0) / z.shape[0] + eps)
    scale = gamma.double() * istd
    return torch.stack([mean, istd, scale, beta.double() - mean * scale])


def grad_blocks(n_rows):
    """Row blocks for the row-local dh0 check: the last 64 rows | the 64 rows
    around every statistics-group edge 1024 k | the 64 rows around 65536."""
    blocks = {"last": np.arange(max(n_rows - TILE, 0), n_rows)}
    # rows [1024 k - 32, 1024 k + 32), clipped to n, of every edge inside the batch
    edges = [np.arange(e - SUB, min(e + SUB, n_rows)) for e in range(GROUP, n_rows, GROUP)]
    if edges:
        blocks["group_edges"] = np.concatenate(edges)
    if n_rows > DEFER_MAX:
        blocks["defer_edge"] = np.arange(DEFER_MAX - SUB, min(DEFER_MAX + SUB, n_rows))
    return blocks
