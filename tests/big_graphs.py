"""Test graphs just past 256 tiles of 64 rows, where the weight-gradient
kernels of csrc/conv_layer.hip and csrc/gt_layer.hip stop running one tile per
workgroup (their grid is capped at 256) and walk further tiles in a loop.

Host side only, shared by tests/test_gpu_encoders.py and
tests/test_gpu_transformer.py; tests/test_big_graphs_cpu.py checks without a
GPU that each graph has the property its test relies on.
"""
import numpy as np

TILE = 64
GRID_CAP = 256  # conv_grid / gt_grid: at most this many workgroups

# one full tile per workgroup (the boundary), and workgroup 0 walking a second
# tile that holds 6 live rows.  Both even: for odd n the doubling map below is
# a bijection and in-degree = out-degree almost everywhere.
BIG_SIZES = {"big256": GRID_CAP * TILE, "big257": (GRID_CAP + 1) * TILE + 6}


def tiles(n):
    return (n + TILE - 1) // TILE


def directed(n):
    """(src, dst, n): v -> v+1, v -> v+3, v -> 2v+5 (mod n), no reverse edge
    kept.  Non-symmetric, and the 2v+5 edges reach tiles far from the row's
    own."""
    edges = set()
    for v in range(n):
        for u in ((v + 1) % n, (v + 3) % n, (2 * v + 5) % n):
            if u != v and (u, v) not in edges:
                edges.add((v, u))
    e = np.array(sorted(edges), np.int64)
    return e[:, 0], e[:, 1], n


def degree_asymmetry(src, dst, n):
    """Share of nodes whose in-degree differs from their out-degree: above 0.5
    a backward over the wrong CSR cannot pass."""
    return float((np.bincount(dst, minlength=n) != np.bincount(src, minlength=n)).mean())


def far_edge_share(src, dst):
    """Share of edges whose endpoints lie more than one tile apart."""
    return float((np.abs(src // TILE - dst // TILE) > 1).mean())


_BIG = {}


def big_directed(name):
    """The directed recipe at BIG_SIZES[name] (built once), guards asserted."""
    if name not in _BIG:
        src, dst, n = directed(BIG_SIZES[name])
        assert n % 2 == 0 and degree_asymmetry(src, dst, n) > 0.5
        assert far_edge_share(src, dst) > 0.25  # the dx gather crosses workgroups
        _BIG[name] = (src, dst, n)
    return _BIG[name]


# synth.molecules(N, "qm9", seed): 16,478 rows = 257 full tiles and one of 30
# rows, so workgroups 0 and 1 walk a second tile and the last tile is ragged
BIG_MOLS = (910, 9)


def big_molecules(pkg):
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(BIG_MOLS[0], "qm9", seed=BIG_MOLS[1]))
    n = gh.num_nodes()
    assert n > GRID_CAP * TILE and n % TILE != 0 and tiles(n) < 2 * GRID_CAP
    return gh


# capacity mode across the 256-tile line: name -> (molecules, slack)
CAPACITY_SPLITS = {
    # 260 live tiles of 268: the second tile of workgroups 0..2 is live, that
    # of workgroup 3 partly (37 rows), that of workgroups 4..11 padding
    "live_past_256": (920, 1.03),
    # 198 live tiles of 296: workgroups 198..255 see padding only and must
    # write a zero slab; workgroups 0..39 meet a live tile, then a padded one
    "live_below_256_below_capacity": (700, 1.5),
}


def capacity_case(pkg, name, seed=21):
    """(host batch, StaticBatch.capacities(...)) of a split, its shape asserted."""
    B, slack = CAPACITY_SPLITS[name]
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(B, "qm9", seed=seed))
    caps = pkg.graph.StaticBatch.capacities([gh], 1, slack=slack)
    live, cap = tiles(gh.num_nodes()), tiles(caps[0])
    assert gh.num_nodes() % TILE != 0  # a partly live tile
    if name == "live_past_256":
        assert GRID_CAP + 2 <= live and live + 4 <= cap < 2 * GRID_CAP
    else:
        assert live + 32 <= GRID_CAP and GRID_CAP + 32 <= cap < live + GRID_CAP
    return gh, caps
