"""Host side of tests/test_gpu_ego_edges.py: every batch of the case tables
has the property its case relies on (start lanes, longest edge, max in-degree,
ball sizes, exact node counts, bitmap widths, padded blocks), the thresholds
sit where the library's host queries put them, and on the small cases the
oracle equals a plain BFS restatement, so the reference itself is right at the
window and word edges before the kernels are held to it.  A retune of the
block sizes, the degree bounds or the resident-grid limit fails here first:
then move the tables in tests/ego_edge_cases.py to the new edges."""
from __future__ import annotations

import numpy as np
import pytest

import ego_edge_cases as E

MOVE = "the library's edges moved: move the case tables of tests/ego_edge_cases.py with them"


def _q(pkg, name, *args):
    return int(pkg._lib.query(name, *args))


def test_thresholds_equal_the_host_queries(pkg):
    assert _q(pkg, "scgib_egonet_k1_max_degree") == E.K1_DEGREES[-1], MOVE
    assert _q(pkg, "scgib_egonet_k1_max_graph_nodes") == E.WINDOW_REACH + 1 == E.K1_BLOCK, MOVE
    resident = _q(pkg, "scgib_egonet_k1_resident_blocks")
    # the one-pass builder's scan words: 2 per 64-parent block + 4
    for n in E.BLOCKS:
        assert _q(pkg, "scgib_egonet_k1_scan_words", n) == 2 * E.onepass_blocks(n) + 4, MOVE
        # the bitmap builder's workspace is sized for the k = 1 builders' blocks
        assert _q(pkg, "scgib_egonet_workspace_bytes", n) == 8 * E.onepass_blocks(n), MOVE
        assert 2 * E.bitmap_blocks(n) <= 2 * E.onepass_blocks(n)
    # 65,536 is the last size without the ticket, 65,537 the first with it
    assert [E.onepass_blocks(n) > resident for n in E.BLOCKS] == \
        [False, False, False, False, True, True], MOVE
    assert (E.onepass_blocks(65536), E.onepass_blocks(65537)) == (resident, resident + 1), MOVE
    assert E.TICKET_BLOCKS == tuple(n for n in E.BLOCKS if E.onepass_blocks(n) > resident), MOVE
    # the fix-up's predecessor loop strides by its 256 threads: a block sums
    # ceil(block / 256) rounds, two from block 257 on
    assert [E.bitmap_blocks(n) for n in E.BLOCKS] == [1, 1, 17, 256, 257, 259]
    rounds = lambda n: -(-(E.bitmap_blocks(n) - 1) // E.BM_BLOCK)  # noqa: E731 (the last block's)
    assert [rounds(n) for n in E.BLOCKS] == [0, 0, 1, 1, 1, 2]
    assert E.bitmap_blocks(66049) - 1 - E.BM_BLOCK == 2  # blocks 257 and 258


def test_motifs():
    n, p = E.ring64()
    assert n == 64 and int((p[:, 1] - p[:, 0]).max()) == 63
    for r in (6, 7, 8, 9, 12, 13):
        n, p = E.wheel(r)
        deg = np.bincount(p.reshape(-1), minlength=n)
        assert n == r + 1 and deg[r // 2] == r and sorted(set(deg.tolist())) == [3, r]
        assert 0 < r // 2 < r  # members on either side of the hub: both window words
    for m in E.WORDS + (E.REJECTED_ATOMS,):
        n, p = E.long(m)
        assert n == m and int((p[:, 1] - p[:, 0]).max()) == m - 1
        if m > 65:
            assert {63, 65} <= set((p[:, 1] - p[:, 0]).tolist())


@pytest.mark.parametrize("name", list(E.WINDOW))
def test_window_cases(pkg, name):
    g = E.case_graph(pkg, "window", name)
    _, d, first = E.WINDOW[name]
    counts = g.batch_num_nodes_host()
    big = np.flatnonzero(counts == 64)
    assert len(big) == 3 and big[0] == first
    assert tuple(int(s) % E.K1_BLOCK for s in E.starts(g)[big]) == E.WINDOW_LANES
    assert g.max_graph_nodes == 64 == _q(pkg, "scgib_egonet_k1_max_graph_nodes"), MOVE
    assert E.longest_edge(g) == E.WINDOW_REACH
    dmax = E.max_in_degree(g)
    assert E.k1_degree_bound(dmax) == d and (dmax == d or (d == 6 and dmax <= 6))
    n = g.num_nodes()
    if name.endswith("tail") or name == "d6":
        assert E.starts(g)[big[0]] == 0          # the LDS window's first row
    if name.endswith("head") or name == "d6":
        assert E.starts(g)[big[-1]] + 64 == n    # ... and its last
    # window bits 1 and 127: atoms 63 below and 63 above a ball's centre
    rp, col = g.rowptr.numpy(), g.col.numpy()
    s = int(E.starts(g)[big[-1]])
    assert s in col[rp[s + 63]:rp[s + 64]] and s + 63 in col[rp[s]:rp[s + 1]]


@pytest.mark.parametrize("r", list(E.DEGREE))
def test_degree_cases(pkg, r):
    g = E.case_graph(pkg, "degree", r)
    assert int(g.host_info["deg"].max()) == r
    assert set(E.oracle(g, 1).sizes.tolist()) == E.DEGREE_BALLS[r]
    kmax = _q(pkg, "scgib_egonet_k1_max_degree")
    assert E.k1_degree_bound(r) == {6: 6, 7: 8, 8: 8, 9: 12, 12: 12, 13: None}[r]
    assert (pkg.graph.ego_bounds(g, 1)[2] > kmax) == (r == 13), MOVE
    assert g.max_graph_nodes <= 64 and 0 in g.batch_num_nodes_host()
    if r == 12:  # one full load group | a second with one live member | with six
        assert E.K1_GROUP_D12 in E.DEGREE_BALLS[r] and E.K1_GROUP_D12 + 1 in E.DEGREE_BALLS[r]
        assert max(E.DEGREE_BALLS[r]) == 2 * E.K1_GROUP_D12 - 1


@pytest.mark.parametrize("n", E.BLOCKS)
def test_block_cases(pkg, n):
    g = E.case_graph(pkg, "blocks", n)
    counts = g.batch_num_nodes_host()
    assert g.num_nodes() == n == int(counts.sum())
    assert counts[-1] == 0 and 0 in counts[:-1]  # a 0-atom molecule at the end and inside
    assert g.max_graph_nodes == 64
    if n > 64:
        assert int(g.host_info["deg"].max()) <= 12 and 1 in counts
    if n >= 4097:  # the fast builders under D = 12, the window at its reach
        assert int(g.host_info["deg"].max()) == 12 and E.longest_edge(g) == E.WINDOW_REACH
        # 64-atom molecules across block edges at many lanes
        lanes = set((E.starts(g)[counts == 64] % E.K1_BLOCK).tolist())
        assert {0, 1, 63} <= lanes and len(lanes) > 8
    assert E.case_graph(pkg, "blocks", n) is g  # built once, shared


@pytest.mark.parametrize("m", E.WORDS + (E.REJECTED_ATOMS,))
def test_words_cases(pkg, m):
    table = "rejected" if m == E.REJECTED_ATOMS else "words"
    g = E.case_graph(pkg, table, m)
    assert g.max_graph_nodes == m and E.starts(g)[1] > 0
    need = (m + 63) // 64
    want = {64: 1, 65: 2, 128: 2, 129: 4, 256: 4, 257: 8, 512: 8, 513: None}[m]
    assert E.bitmap_words(m) == want
    if want is not None:
        assert want >= need and (want == 1 or want // 2 < need)
    # only the 64-atom case stays inside the k = 1 fast builders
    fits = m <= _q(pkg, "scgib_egonet_k1_max_graph_nodes")
    assert fits == (m == 64) and E.max_in_degree(g) <= _q(pkg, "scgib_egonet_k1_max_degree")
    if m > 64:  # balls with members in more than one 64-bit word of the molecule's bitmap
        o, s = E.oracle(g, 1), int(E.starts(g)[1])
        owner = np.repeat(np.arange(g.num_nodes()), o.sizes)
        word = (o.nodes - s) >> 6
        inside = (owner >= s) & (owner < s + m)
        lo = np.full(g.num_nodes(), 1 << 30)
        hi = np.full(g.num_nodes(), -1)
        np.minimum.at(lo, owner[inside], word[inside])
        np.maximum.at(hi, owner[inside], word[inside])
        assert int((hi > lo).sum()) >= 2 and int(hi.max()) == (m - 1) >> 6


@pytest.mark.parametrize("name", list(E.CAPACITY))
@pytest.mark.parametrize("k", [1, 2])
def test_capacity_cases(pkg, name, k):
    c = E.capacity_case(pkg, name, k)
    n, n_cap = E.CAPACITY[name]
    resident = _q(pkg, "scgib_egonet_k1_resident_blocks")
    assert c.first.num_nodes() == n and c.n_cap == n_cap
    assert c.second.num_nodes() == n - 62 and c.second.batch_size == c.first.batch_size == c.B
    for g in (c.first, c.second):
        assert g.batch_num_nodes_host().min() >= 2 and g.num_edges() <= c.e_cap
        ns, es, dmax = pkg.graph.ego_bounds(g, k)
        assert ns + E.EGO_PAD[0] <= c.caps[0] and es + E.EGO_PAD[1] <= c.caps[1]
        assert g.max_graph_nodes == c.mgn == 64 and dmax == 12
        # at least one wholly padded 64-row block behind the live part
        assert E.onepass_blocks(n_cap) > E.onepass_blocks(g.num_nodes())
    assert (c.caps[2] == 12) == (k == 1)  # k = 1 runs the one-pass builder, D = 12
    assert (n % E.K1_BLOCK == 0) == (name == "full")
    if name == "ticket":
        assert n == resident * E.K1_BLOCK + 1 and n_cap >= n + 128, MOVE
        assert E.onepass_blocks(n_cap) == E.onepass_blocks(n) + 2 > resident
    else:
        assert E.onepass_blocks(n_cap) <= resident


# ---------------------------------------------------------------------------
# the oracle against a plain restatement, on the small cases
# ---------------------------------------------------------------------------
def _bfs_egonets(rp, col, k):
    """ball = nodes within k hops, sorted; edges = induced, row-major in ball order."""
    sizes, ecount, nodes, row, colv = [], [], [], [], []
    for v in range(len(rp) - 1):
        ball = frontier = {v}
        for _ in range(k):
            frontier = {int(w) for u in frontier for w in col[rp[u]:rp[u + 1]]}
            ball = ball | frontier
        pos = {u: len(nodes) + i for i, u in enumerate(sorted(ball))}
        edges = [(pos[u], pos[int(w)]) for u in sorted(ball) for w in col[rp[u]:rp[u + 1]]
                 if int(w) in pos]
        sizes.append(len(ball))
        ecount.append(len(edges))
        nodes += sorted(ball)
        row += [e[0] for e in edges]
        colv += [e[1] for e in edges]
    return sizes, ecount, nodes, row, colv


_SMALL_CASES = [("window", name) for name in E.WINDOW] + [("degree", r) for r in E.DEGREE] + \
    [("words", m) for m in E.WORDS if m <= 129]


@pytest.mark.parametrize("table,key", _SMALL_CASES)
@pytest.mark.parametrize("k", [1, 2, 3])
def test_oracle_equals_the_bfs_restatement(pkg, table, key, k):
    g = E.case_graph(pkg, table, key)
    o = E.oracle(g, k)
    want = _bfs_egonets(g.rowptr.numpy().astype(np.int64), g.col.numpy().astype(np.int64), k)
    for got, ref in zip((o.sizes, o.ecount, o.nodes, o.row, o.col), want):
        np.testing.assert_array_equal(got, np.asarray(ref, np.int64))
    assert (o.n_s, o.e_s) == (len(want[2]), len(want[3]))
    if k == 1:  # the closed form the dispatcher sizes its buffers by
        info = g.host_info
        np.testing.assert_array_equal(o.sizes, 1 + info["deg"] - info["selfloops"])
