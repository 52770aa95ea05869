"""Host side of tests/test_gpu_gin_edges.py: the batches have exactly the row
counts of the case table, every edge in the table sits where the library's
own host queries put it, and the outlier passes meet their condition on the
oracle alone.  A retune of kGroup, a grid cap or the deferral limit fails here
first: then move the table in tests/gin_edge_cases.py to the new edges."""
from __future__ import annotations

import numpy as np
import pytest

import gin_edge_cases as E

MOVE = "the library's edges moved: move the case table of tests/gin_edge_cases.py with them"


def _q(pkg, name, *args):
    return int(pkg._lib.query(name, *args))


def _groups(n):
    return -(-(-(-n // E.TILE)) // 16)


@pytest.mark.parametrize("n", E.all_row_counts())
def test_exact_graph_has_exact_rows_and_a_closing_path(pkg, n):
    gh = E.exact_graph(pkg, n)
    counts = gh.batch_num_nodes_host()
    assert gh.num_nodes() == n and int(counts.sum()) == n
    assert counts.min() >= 2  # (a one-atom molecule cannot train a BatchNorm; the reference skips those)
    m = int(counts[-1])
    deg = gh.host_info["deg"][n - m:]
    # the last molecule is a path: two ends of degree 1, the rest of degree 2
    assert sorted(deg.tolist()) == sorted([1, 1] + [2] * (m - 2))
    col = gh.col.numpy()[int(gh.rowptr[n - m]):]
    assert col.min() >= n - m and np.abs(np.repeat(np.arange(n - m, n), deg) - col).max() == 1
    assert gh.host_info["validated"]
    assert E.exact_graph(pkg, n) is gh  # built once, shared


@pytest.mark.parametrize("n", E.all_row_counts())
def test_library_sizes_follow_the_table_constants(pkg, n):
    tiles, groups = -(-n // E.TILE), _groups(n)
    sup = -(-groups // 64) if groups > 64 else 0
    assert _q(pkg, "scgib_gin_tiles", n) == tiles, MOVE
    assert _q(pkg, "scgib_gin_counters", n) == groups + 1 + sup, MOVE
    assert _q(pkg, "scgib_gin_bn_ws_floats", n) == \
        ((tiles * 128 + 1) & ~1) + 2 * 128 * (groups + sup), MOVE


def test_edges_sit_where_the_library_says(pkg):
    q = lambda name, *a: _q(pkg, name, *a)  # noqa: E731
    # tile: 64 rows are one tile, 65 two
    assert (q("scgib_gin_tiles", 64), q("scgib_gin_tiles", 65)) == (1, 2), MOVE
    # statistics group: counters = groups + 1 (+ supergroups)
    assert [q("scgib_gin_counters", n) for n in (1023, 1024, 1025)] == [2, 2, 3], MOVE
    # 32 groups | 33 groups (the finish rounds take 32: kFinG, 2 * kBFinR)
    assert [q("scgib_gin_counters", n) for n in (32768, 32769)] == [33, 34], MOVE
    assert E.ROUND == 32768
    # deferral limit == agg-free switch == one full supergroup
    assert q("scgib_gin_defer_max_nodes") == E.DEFER_MAX == pkg.ops.AGG_FREE_MIN_ROWS, MOVE
    # ... up to which there are no supergroup counters: 64 + 1, then 65 + 1 + 2
    assert [q("scgib_gin_counters", n) for n in (65535, 65536, 65537)] == [65, 65, 68], MOVE
    assert q("scgib_gin_bn_ws_floats", 65537) - q("scgib_gin_bn_ws_floats", 65536) == \
        128 + 256 * (1 + 2), MOVE  # one tile, one group, two supergroups
    # two full supergroups
    assert q("scgib_gin_counters", E.FULL_SUPER_ROWS) == 128 + 1 + 2, MOVE
    # d = 64 backward: 256 sub-tiles on 256 workgroups, then two and three per workgroup
    slabs = [q("scgib_gin_layer_bwd_slabs", n, 64) for n in (8192, 8193, 16385)]
    assert slabs == [256, 129, 171], MOVE
    assert [-(-(-(-n // E.SUB)) // s) for n, s in zip((8192, 8193, 16385), slabs)] == [1, 2, 3]
    # ... the last workgroup's share: a short walk of one at 8193, a whole one at 16385
    assert [-(-n // E.SUB) - (s - 1) * per for n, s, per in
            zip((8193, 16385), slabs[1:], (2, 3))] == [1, 3], MOVE
    # d_in = 32 backward: one workgroup per tile up to 512 tiles, 513 tiles on 512
    assert [q("scgib_gin_layer_bwd_slabs", n, 32) for n in (32768, 32769)] == [512, 512], MOVE
    assert q("scgib_gin_tiles", 32769) == 513
    # ... the folded layer 0: past 512 the fewest workgroups of two tiles each
    assert [q("scgib_gin_bwd_slabs", n) for n in (32768, 32769)] == [512, 257], MOVE


def test_capacity_cases_straddle_the_host_decisions(pkg):
    lim = _q(pkg, "scgib_gin_defer_max_nodes")
    for n, cap in E.CAPACITY_CASES:
        assert 2 <= n < cap
        assert -(-cap // E.TILE) > -(-n // E.TILE), (n, cap)  # at least one padding-only tile
    # the last three: the host decides from the capacity (no deferral, agg-free,
    # supergroup-sized workspaces), the kernels from the valid count
    assert [(n <= lim, cap <= lim) for n, cap in E.CAPACITY_CASES] == \
        [(True, True)] * 4 + [(True, False), (True, False), (False, False)], MOVE
    for n, cap in E.WEIGHTED_CASES:
        assert cap is None or (n, cap) in E.CAPACITY_CASES


@pytest.mark.parametrize("n,cap", E.WEIGHTED_CASES)
def test_outlier_rows_carry_their_share_in_the_oracle(pkg, n, cap):
    """The rows of the last tile, scaled, hold at least OUTLIER_SHARE of layer
    0's centred sum of squares (median over channels): dropping or double
    counting them moves the statistics far past the 1e-5 bar."""
    gh = E.exact_graph(pkg, n)
    p, _ = E.oracle_params(E.make_gin(pkg))
    h0, _ = E.make_inputs(n)
    src, dst = gh.edges()
    plain = E.outlier_share(E.layer0_z2(p, src, dst, h0), n)
    share = E.outlier_share(E.layer0_z2(p, src, dst, E.with_outliers(h0, n)), n)
    assert share >= E.OUTLIER_SHARE, (n, share)
    assert plain < share


def test_grad_blocks_cover_the_edges():
    b = E.grad_blocks(1024)
    assert set(b) == {"last"} and b["last"].tolist() == list(range(960, 1024))
    b = E.grad_blocks(1025)
    assert b["group_edges"].tolist() == list(range(992, 1025))
    b = E.grad_blocks(65537)
    assert len(b["group_edges"]) == 63 * 64 + 33
    assert b["defer_edge"].tolist() == list(range(65504, 65537))
    assert "defer_edge" not in E.grad_blocks(65536)


def test_first_coupled_row_is_a_molecule_start(pkg):
    for n in (65, 1025):
        gh = E.exact_graph(pkg, n)
        lo = E.first_coupled_row(gh, n)
        ptr = np.concatenate([[0], np.cumsum(gh.batch_num_nodes_host())])
        assert lo in ptr and lo <= n - E.UPSTREAM_ROWS < ptr[np.searchsorted(ptr, lo) + 1]
