"""The ego-net builders (csrc/egonet.hip) at the edges of their code paths,
each held to oracle.egonet.egonets bit for bit: ball sizes, _ID, edge counts,
CSR rows and columns in DGL order (the comparison of test_gpu_parity's
_check_ego).  tests/ego_edge_cases.py holds the case tables and each case's
reason; tests/test_ego_edges_cpu.py pins the tables to the library's host
queries and the oracle to a plain BFS.

  a. k = 1: the one-pass, the two-launch and the bitmap builder, each against
     the oracle, on 64-atom molecules at lanes 0, 1 and 63 with edges 63
     apart, at max in-degrees 6 | 7, 8 | 9, 12 | 13 and at exact block counts;
     after every one-pass launch the scan state is read and must be zero;
  b. the one-pass builder's ticket path (more than
     scgib_egonet_k1_resident_blocks() blocks), three launches in a row and
     then a one-block launch on the same state;
  c. k = 1, 2, 3 through the bitmap builder at W = 1 | 2 | 4 | 8, and past 256
     blocks, where egonet_scan_fixup_k sums its predecessors in two rounds;
  d. 513 atoms are refused and nothing is written;
  e. capacity mode (StaticBatch, and the pool-indirect EgoPrefetch) against
     the oracle of the unpadded batch, with the tail contract and a second
     batch loaded into the same buffers.
Each test reads back the entry point and the bound (max in-degree, bitmap
width) its launch was given, so a change of the dispatcher shows here."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import ego_edge_cases as E

pytestmark = pytest.mark.gpu

# (EGO_K1_FAST, EGO_K1_ONEPASS) and the entry point that builder goes through
BUILDERS = {"onepass": (True, True, "scgib_egonet_k1_build_onepass"),
            "two_launch": (True, False, "scgib_egonet_k1_build_deg"),
            "bitmap": (False, False, "scgib_egonet_count")}
SCAN_KEY = "egonet_k1_scan"  # graph._egonet_k1's scan-state call site


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture
def calls(pkg, monkeypatch):
    """(name, args) of every library call the test makes."""
    log, real = [], pkg._lib.call

    def spy(name, *args):
        log.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(pkg._lib, "call", spy)
    return log


def _use(pkg, monkeypatch, builder):
    fast, onepass, _ = BUILDERS[builder]
    monkeypatch.setattr(pkg.graph, "EGO_K1_FAST", fast)
    monkeypatch.setattr(pkg.graph, "EGO_K1_ONEPASS", onepass)


def _host(ego):
    torch.cuda.synchronize()
    return (ego.graph_ptr.cpu().numpy().astype(np.int64), ego.ndata["_ID"].cpu().numpy(),
            ego.rowptr.cpu().numpy().astype(np.int64), ego.col.cpu().numpy())


def _assert_live(o, arrays):
    """The ego batch's live part == the oracle's, as _check_ego compares."""
    gp, ids, rp, col = arrays
    n = len(o.sizes)
    assert gp[0] == 0
    np.testing.assert_array_equal(np.diff(gp[: n + 1]), o.sizes)
    np.testing.assert_array_equal(ids[: o.n_s], o.nodes)
    assert rp[0] == 0 and rp[o.n_s] == o.e_s
    np.testing.assert_array_equal(np.diff(rp[gp[: n + 1]]), o.ecount)
    row = np.repeat(np.arange(o.n_s), np.diff(rp[: o.n_s + 1]))
    np.testing.assert_array_equal(row, o.row)
    np.testing.assert_array_equal(col[: o.e_s], o.col)


def _assert_exact(o, arrays):
    gp, ids, rp, _ = arrays
    assert (len(gp), len(ids), len(rp)) == (len(o.sizes) + 1, o.n_s, o.n_s + 1)
    _assert_live(o, arrays)


def _assert_scan_state_zero(pkg, dev, n, key=SCAN_KEY):
    words = int(pkg._lib.query("scgib_egonet_k1_scan_words", n))
    state = pkg.ops.scan_state(dev, key, words)
    torch.cuda.synchronize()
    assert state.numel() == words and not bool(state.any())  # done, ticket, every state word
    return state


def _ran(calls, pkg, gh, builder):
    """The entry point and bound of the last ego build: ("k1", D) or ("bitmap", W)."""
    names = [c[0] for c in calls]
    dmax = E.max_in_degree(gh)
    fits = gh.max_graph_nodes <= 64 and E.k1_degree_bound(dmax) is not None
    want = BUILDERS[builder][2] if fits else BUILDERS["bitmap"][2]
    assert want in names and sum(n in names for *_, n in BUILDERS.values()) == 1, names
    args = next(a for n, a in reversed(calls) if n == want)
    if want == BUILDERS["bitmap"][2]:
        assert "scgib_egonet_fill" in names
        assert args[6] == max(gh.max_graph_nodes, 1)  # max_graph_nodes: selects W
        return "bitmap", E.bitmap_words(args[6])
    assert args[3] == dmax  # max_in_degree: selects D
    return "k1", E.k1_degree_bound(args[3])


def _build_and_check(pkg, dev, calls, gh, k, builder="onepass"):
    del calls[:]
    ego = pkg.graph.egonet_batch(gh.to(dev), k)
    _assert_exact(E.oracle(gh, k), _host(ego))
    ran = _ran(calls, pkg, gh, builder if k == 1 else "bitmap")
    if ran[0] == "k1" and builder == "onepass":
        _assert_scan_state_zero(pkg, dev, gh.num_nodes())
    return ran


def _ticket(pkg, n):
    return E.onepass_blocks(n) > int(pkg._lib.query("scgib_egonet_k1_resident_blocks"))


# ---------------------------------------------------------------------------
# a. k = 1, every builder against the oracle
# ---------------------------------------------------------------------------
# (the one-pass builder on E.TICKET_BLOCKS has a test function of its own, below)
_K1_CASES = [(table, key, builder)
             for table, key in [("window", name) for name in E.WINDOW] +
             [("degree", r) for r in E.DEGREE] + [("blocks", n) for n in E.BLOCKS]
             for builder in BUILDERS
             if not (table == "blocks" and key in E.TICKET_BLOCKS and builder == "onepass")]


@pytest.mark.parametrize("table,key,builder", _K1_CASES)
def test_k1_builders_equal_the_oracle(pkg, dev, calls, monkeypatch, table, key, builder):
    gh = E.case_graph(pkg, table, key)
    assert not (builder == "onepass" and _ticket(pkg, gh.num_nodes()))
    _use(pkg, monkeypatch, builder)
    kind, bound = _build_and_check(pkg, dev, calls, gh, 1, builder)
    # D: the window cases' own | the degree cases' by the dispatch rule | the
    # block cases' 12 once the DEGREE-12 motifs fit, else ring64's 6
    d = {"window": lambda: E.WINDOW[key][1], "degree": lambda: E.k1_degree_bound(key),
         "blocks": lambda: 12 if key >= 4097 else 6}[table]()
    assert (kind, bound) == (("bitmap", 1) if builder == "bitmap" or d is None else ("k1", d))
    print(f"\n[ego-edges] {table} {key} {builder}: {gh.num_nodes()} atoms, one-pass blocks "
          f"{E.onepass_blocks(gh.num_nodes())}, bitmap blocks {E.bitmap_blocks(gh.num_nodes())}, "
          f"ran {kind} bound {bound}")


# ---------------------------------------------------------------------------
# b. the one-pass builder's ticket path
# ---------------------------------------------------------------------------
def test_k1_onepass_ticket_path(pkg, dev, calls, monkeypatch):
    """More blocks than the resident limit: every block takes its logical
    index from the ticket and the last one resets it.  65,537 atoms three
    times in a row (each exact, the state read back as zeros each time), then
    the one-block 64-atom case on the very same state words, then 66,049."""
    _use(pkg, monkeypatch, "onepass")
    resident = int(pkg._lib.query("scgib_egonet_k1_resident_blocks"))
    gh = E.case_graph(pkg, "blocks", 65537)
    assert E.onepass_blocks(65537) == resident + 1
    for _ in range(3):
        assert _build_and_check(pkg, dev, calls, gh, 1) == ("k1", 12)
    big = _assert_scan_state_zero(pkg, dev, 65537)
    small = E.case_graph(pkg, "blocks", 64)
    assert _build_and_check(pkg, dev, calls, small, 1) == ("k1", 6)
    assert _assert_scan_state_zero(pkg, dev, 64).data_ptr() == big.data_ptr()  # the same words
    assert _build_and_check(pkg, dev, calls, E.case_graph(pkg, "blocks", 66049), 1) == ("k1", 12)
    for n in E.BLOCKS:
        print(f"\n[ego-edges] one-pass n={n}: blocks {E.onepass_blocks(n)}, "
              f"ticket {E.onepass_blocks(n) > resident}")


# ---------------------------------------------------------------------------
# c. bitmap widths and the scan fix-up's second round
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("m", E.WORDS)
def test_bitmap_widths_equal_the_oracle(pkg, dev, calls, m, k):
    gh = E.case_graph(pkg, "words", m)
    kind, bound = _build_and_check(pkg, dev, calls, gh, k)
    # molecules over 64 atoms leave the k = 1 fast builders
    # (the 64-atom batch's max in-degree is wheel(6)'s 6: D = 6)
    assert (kind, bound) == (("k1", 6) if (k == 1 and m == 64) else ("bitmap", E.bitmap_words(m)))
    assert bound == (6 if kind == "k1" else {64: 1, 65: 2, 128: 2, 129: 4, 256: 4, 257: 8, 512: 8}[m])
    print(f"\n[ego-edges] words m={m} k={k}: ran {kind} bound {bound}")


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("n", [65537, 66049])
def test_bitmap_builder_past_256_blocks(pkg, dev, calls, n, k):
    assert E.bitmap_blocks(n) > E.BM_BLOCK
    assert _build_and_check(pkg, dev, calls, E.case_graph(pkg, "blocks", n), k) == ("bitmap", 1)


# ---------------------------------------------------------------------------
# d. rejection
# ---------------------------------------------------------------------------
def test_oversized_molecule_is_refused_and_nothing_written(pkg, dev, calls):
    lib, ops = pkg._lib, pkg.ops
    assert _build_and_check(pkg, dev, calls, E.case_graph(pkg, "words", E.MAX_ATOMS), 2) == \
        ("bitmap", 8)
    gh = E.case_graph(pkg, "rejected", E.REJECTED_ATOMS)
    g = gh.to(dev)
    for k in (1, 2):
        with pytest.raises(lib.ScgibError):
            pkg.graph.egonet_batch(g, k)
    # the entry points themselves: refused before any launch
    n, i32 = g.num_nodes(), torch.int32
    o = E.oracle(gh, 1)
    fresh = lambda size: torch.full((size,), -7, dtype=i32, device=dev)  # noqa: E731
    ego_ptr, ego_eptr = fresh(n + 1), fresh(n + 1)
    nodes, rp, col = fresh(o.n_s), fresh(o.n_s + 1), fresh(o.e_s)
    ws = torch.full((int(lib.query("scgib_egonet_workspace_bytes", n)),), 0x5A, dtype=torch.uint8,
                    device=dev)
    err = torch.zeros(1, dtype=i32, device=dev)
    head = (ops._p(g.rowptr), ops._p(g.col), ops._p(g.graph_ptr), g.batch_size, n, 1)
    with pytest.raises(lib.ScgibError):
        lib.call("scgib_egonet_count", *head, E.REJECTED_ATOMS, ops._p(ego_ptr), ops._p(ego_eptr),
                 ops._p(ws), ops._p(err), None, ops._stream())
    with pytest.raises(lib.ScgibError):
        lib.call("scgib_egonet_fill", *head, E.REJECTED_ATOMS, ops._p(ego_ptr), ops._p(ego_eptr),
                 ops._p(nodes), ops._p(rp), ops._p(col), ops._p(err), o.n_s, None, None,
                 ops._stream())
    torch.cuda.synchronize()
    for t in (ego_ptr, ego_eptr, nodes, rp, col):
        assert bool((t == -7).all())
    assert bool((ws == 0x5A).all()) and int(err.item()) == 0
    # told the largest width it has, the count pass flags the molecule (bit 2)
    lib.call("scgib_egonet_count", *head, E.MAX_ATOMS, ops._p(ego_ptr), ops._p(ego_eptr),
             ops._p(ws), ops._p(err), None, ops._stream())
    torch.cuda.synchronize()
    assert int(err.item()) == 2


# ---------------------------------------------------------------------------
# e. capacity mode against the oracle
# ---------------------------------------------------------------------------
def _assert_capacity(o, ego, n_cap, ego_cap):
    """Live part == the oracle of the unpadded batch; the tail contract:
    dims = [N_s, E_s], graph_ptr past the live parents = N_s,
    rowptr[N_s .. cap] = E_s, _ID[N_s .. cap) = 0."""
    arrays = gp, ids, rp, _ = _host(ego)
    assert ego.dims.cpu().tolist() == [o.n_s, o.e_s]
    assert (len(gp), len(ids), len(rp)) == (n_cap + 1, ego_cap, ego_cap + 1)
    _assert_live(o, arrays)
    n = len(o.sizes)
    assert n < n_cap and o.n_s < ego_cap
    assert (gp[n:] == o.n_s).all()
    assert (rp[o.n_s:] == o.e_s).all()
    assert (ids[o.n_s:] == 0).all()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", list(E.CAPACITY))
def test_capacity_mode_equals_the_oracle(pkg, dev, calls, name, k):
    c = E.capacity_case(pkg, name, k)
    static = pkg.graph.StaticBatch(c.B, c.n_cap, c.e_cap, 1, c.mgn, c.caps, dev, k=k)
    # the second batch is smaller: the first's tail must not survive in its padding
    for gh in (c.first, c.second, c.first):
        static.load(static.pad(gh))
        del calls[:]
        ego = pkg.graph.egonet_batch(static.graph, k)
        _assert_capacity(E.oracle(gh, k), ego, c.n_cap, c.caps[0])
        names = [n for n, _ in calls]
        if k == 1:
            args = next(a for n, a in calls if n == BUILDERS["onepass"][2])
            assert args[2] == c.n_cap and args[3] == 12  # launched over the capacity, D = 12
            assert _ticket(pkg, c.n_cap) == (name == "ticket")
            _assert_scan_state_zero(pkg, dev, c.n_cap)
        else:
            assert "scgib_egonet_count" in names and "scgib_egonet_fill" in names
        assert static.ego_error() == 0


def test_pool_indirect_prefetch_equals_the_oracle(pkg, dev):
    """EgoPrefetch (the replayed step's form): the ego-nets of the batch at the
    pool's cursor are built from its blob into staging and moved in by the
    next load_next -- the same persistent buffers for every batch, held to the
    oracle, not to egonet_batch."""
    c = E.capacity_case(pkg, E.CAPACITY_POOLED, 1)
    assert c.first.num_nodes() % E.K1_BLOCK == 0
    static = pkg.graph.StaticBatch(c.B, c.n_cap, c.e_cap, 1, c.mgn, c.caps, dev, k=1)
    hosts = [c.first, c.second]
    pool = static.pool([static.pad(gh) for gh in hosts])
    pf = pkg.graph.EgoPrefetch(static, pool)
    assert pf.onepass
    pf.prime()
    for step in range(3):  # first, second, first again
        gh = hosts[step % 2]
        static.load_next(pool, pf)
        pf.prefetch()  # the next batch's ego-nets, as the step would
        torch.cuda.synchronize()
        assert static.dims.cpu().tolist() == [gh.num_nodes(), gh.num_edges()]
        _assert_capacity(E.oracle(gh, 1), pf.ego, c.n_cap, c.caps[0])
        _assert_scan_state_zero(pkg, dev, c.n_cap, "egonet_k1_scan_prefetch")
    assert pf.error() == 0 and static.ego_error() == 0
