"""Hand-made molecule batches that put the ego-net builders (csrc/egonet.hip) at
the edges of their code paths: the 128-bit window of the k = 1 builders and
the LDS window of the one-pass form, the in-degree bounds D = 6 | 8 | 12 and
the bitmap fallback, the bitmap widths W = 1 | 2 | 4 | 8, the block counts
where the one-pass builder takes its ticket and the scan fix-up a second
round, and capacity batches with dead blocks.  tests/test_ego_edges_cpu.py
(host) pins every property a case relies on to the library's host queries;
tests/test_gpu_ego_edges.py (device) holds each builder to the oracle on
them.  Plain module: no fixtures, no device work."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from oracle import egonet

K1_BLOCK = 64        # parents per block of the k = 1 builders (csrc kK1Block, kK1One)
BM_BLOCK = 256       # parents per block of the bitmap builder and of egonet_scan_fixup_k
WINDOW_REACH = 63    # |u - v| the 128-bit window (bit 64 + u - v) must hold
K1_DEGREES = (6, 8, 12)   # the in-degree bounds D the k = 1 kernels are built for
K1_GROUP_D12 = 7     # members per load group under D = 12 (csrc K1G<12>)
BITMAP_WORDS = (1, 2, 4, 8)  # 64-bit words of a bitmap-builder ball (csrc words_for)
MAX_ATOMS = 64 * BITMAP_WORDS[-1]


# ---------------------------------------------------------------------------
# motifs: (atoms, undirected pairs [m, 2] with u <= v, unique, local ids)
# ---------------------------------------------------------------------------
def _motif(n, pairs):
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    if len(p):
        p = np.unique(np.sort(p, axis=1), axis=0)
        assert p.min() >= 0 and p.max() < n
    return n, p


def path(n):
    a = np.arange(max(n - 1, 0), dtype=np.int64)
    return _motif(n, np.stack([a, a + 1], 1))


def ring64():
    """64 atoms, the longest edge 63 apart: path 0..63, closing edge (0, 63),
    chords (0, 32) and (31, 63) -- window bits 1 and 127 (atoms 63 and 0), and
    balls on either side of the word split at bit 64."""
    return _motif(64, np.concatenate([path(64)[1], [[0, 63], [0, 32], [31, 63]]]))


def wheel(r):
    """Hub at local index r // 2 with an r-atom rim cycle: hub in-degree r,
    its ball of r + 1 members fills both window words; rim in-degree 3."""
    assert r >= 4
    hub = r // 2
    rim = [i for i in range(r + 1) if i != hub]
    return _motif(r + 1, [(rim[i], rim[(i + 1) % r]) for i in range(r)] + [(hub, u) for u in rim])


def long(n):
    """Path of n atoms, closing edge (0, n - 1), chords (i, i + 65) at every
    7th i and (i, i + 63) at every 11th: balls cross the 64-bit words of the
    bitmap and the relabelling rank sums whole words."""
    pairs = [path(n)[1], [[0, n - 1]]]
    pairs.append([[i, i + 65] for i in range(0, n - 65, 7)])
    pairs.append([[i, i + 63] for i in range(0, n - 63, 11)])
    return _motif(n, np.concatenate([np.asarray(p, np.int64).reshape(-1, 2) for p in pairs]))


ISO = _motif(1, [])                     # an isolated atom: a ball of one, no edge
LOOP = _motif(3, [[0, 1], [1, 2], [1, 1]])  # a self-loop on the middle atom of a path
EMPTY = _motif(0, [])                   # a molecule of no atoms (graph_of: "graphs may be empty")
PAIR = path(2)


def batch(pkg, motifs):
    """Host GraphBatch of the motifs in order, symmetric edges."""
    src, dst, counts, base = [], [], [], 0
    for n, p in motifs:
        u, v = p[:, 0] + base, p[:, 1] + base
        off = u != v  # a self-loop is one directed edge
        src += [u, v[off]]
        dst += [v, u[off]]
        counts.append(n)
        base += n
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.int64)  # noqa: E731
    g = pkg.graph.GraphBatch.from_edges(cat(src), cat(dst), base, True, np.asarray(counts, np.int64))
    assert g.num_nodes() == base and g.host_info["validated"] and g.symmetric
    return g


def longest_edge(g):
    rp, col = g.rowptr.numpy().astype(np.int64), g.col.numpy().astype(np.int64)
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return int(np.abs(row - col).max()) if len(col) else 0


def max_in_degree(g):
    deg = g.host_info["deg"]
    return int(deg.max()) if len(deg) else 0


def starts(g):
    """First node of every molecule."""
    return np.concatenate([[0], np.cumsum(g.batch_num_nodes_host())])[:-1]


# ---------------------------------------------------------------------------
# what the dispatcher runs (graph.egonet_batch, scgib_egonet_k1_build_*,
# words_for): restated here, pinned by the host test and read back from the
# launches by the device test
# ---------------------------------------------------------------------------
def k1_degree_bound(dmax):
    """D of the k = 1 kernels for a batch of max in-degree dmax (None: the
    batch leaves them for the bitmap builder)."""
    return next((d for d in K1_DEGREES if dmax <= d), None)


def bitmap_words(max_graph_nodes):
    """W of the bitmap builder: (m + 63) // 64 rounded up to 1, 2, 4 or 8
    (None: rejected)."""
    need = (max(max_graph_nodes, 1) + 63) // 64
    return next((w for w in BITMAP_WORDS if need <= w), None)


def onepass_blocks(n):
    return -(-n // K1_BLOCK)


def bitmap_blocks(n):
    return -(-n // BM_BLOCK)


# ---------------------------------------------------------------------------
# WINDOW: 64-atom molecules whose first atom sits on lanes 0, 1 and 63 of a
# 64-parent block.  In "d6" the first starts at node 0 (row lo = -64 of the
# one-pass builder's LDS window clamps to row 0) and the last ends at node n
# (its last row clamps to n).  "*_tail" append a wheel so the same lanes and
# the first row run under D = 8 and 12; "*_head" put the wheel and a filler
# path in a 64-atom block of their own in front, which keeps the lanes and the
# last row under D = 8 and 12.
# ---------------------------------------------------------------------------
_WINDOW_BASE = [ring64(), ISO, ring64(), path(62), ring64()]
WINDOW_LANES = (0, 1, 63)
WINDOW = {
    "d6": (_WINDOW_BASE, 6, 0),
    "d8_tail": (_WINDOW_BASE + [wheel(8)], 8, 0),
    "d12_tail": (_WINDOW_BASE + [wheel(12)], 12, 0),
    "d8_head": ([wheel(8), path(55)] + _WINDOW_BASE, 8, 2),
    "d12_head": ([wheel(12), path(51)] + _WINDOW_BASE, 12, 2),
}  # name -> (motifs, D, index of the first 64-atom molecule)

# ---------------------------------------------------------------------------
# DEGREE: max in-degree exactly 6 | 7 (D = 6 | 8), 8 | 9 (D = 8 | 12), 12 | 13
# (the fast builders | the bitmap fallback), from wheel(r) and the small
# motifs.  The 12 batch also holds wheel(6) and wheel(7): balls of exactly 7
# members (one load group under D = 12) and 8 (a second group with one live
# member); its own hub's 13 fill the second group but for one slot.
# ---------------------------------------------------------------------------
_SMALL = [ISO, LOOP, EMPTY]
DEGREE = {r: [wheel(r)] + ([wheel(6), wheel(7)] if r == 12 else []) + _SMALL
          for r in (6, 7, 8, 9, 12, 13)}
# ball sizes (k = 1): the hub r + 1, a rim atom 4, ISO 1, LOOP 2 and 3
DEGREE_BALLS = {r: {1, 2, 3, 4, r + 1} | ({7, 8} if r == 12 else set()) for r in DEGREE}

# ---------------------------------------------------------------------------
# BLOCKS: exact node counts.  64: one full block | 65: one atom into a second
# | 4,097: a block of one live lane after 64 full ones, 17 bitmap blocks |
# 65,536: 1,024 one-pass blocks, the last size without the ticket, and 256
# bitmap blocks (the fix-up's one round, full) | 65,537: 1,025 one-pass blocks,
# the first with the ticket, 257 bitmap blocks | 66,049 = 258 * 256 + 1: 259
# bitmap blocks, so blocks 257 and 258 run the fix-up's second round.
# ---------------------------------------------------------------------------
BLOCKS = (64, 65, 4097, 65536, 65537, 66049)
# ... those past scgib_egonet_k1_resident_blocks() one-pass blocks (the host
# test derives them from the query): the one-pass builder runs them in a test
# function of its own
TICKET_BLOCKS = (65537, 66049)
_BLOCK_UNIT = _WINDOW_BASE + [m for m in DEGREE[12] if m[0]]


def _tiled(n, unit):
    """(motifs, atoms left of n): whole units while they fit, then the unit's
    motifs one by one, in order, where they still fit."""
    size = sum(m[0] for m in unit)
    out = unit * (n // size)
    left = n - size * (n // size)
    for m in unit:
        if m[0] <= left:
            out = out + [m]
            left -= m[0]
    return out, left


def block_motifs(n):
    """The WINDOW + DEGREE-12 motifs tiled to exactly n atoms, filled up with
    one-atom molecules; a 0-atom molecule in the middle and one at the end."""
    out, left = _tiled(n, _BLOCK_UNIT)
    out = out + [ISO] * left
    mid = (len(out) + 1) // 2
    return out[:mid] + [EMPTY] + out[mid:] + [EMPTY]


# ---------------------------------------------------------------------------
# WORDS: the largest molecule is long(m) at either side of every bitmap width:
# 64 | 65 (W = 1 | 2; 64 is also the last size of the k = 1 fast builders),
# 128 | 129 (2 | 4), 256 | 257 (4 | 8), 512 (the largest accepted); 513 is
# rejected.  A small motif in front keeps the long molecule off node 0.
# ---------------------------------------------------------------------------
WORDS = (64, 65, 128, 129, 256, 257, 512)
REJECTED_ATOMS = MAX_ATOMS + 1


def words_motifs(m):
    return [LOOP, long(m), ISO, wheel(6), EMPTY]


# ---------------------------------------------------------------------------
# CAPACITY: (live atoms of the first batch, node capacity).  Every molecule
# has at least two atoms (StaticBatch.pad refuses less).  "full": the live
# count is a multiple of 64 and one 64-row block is wholly padding | "mid":
# the live part ends mid-block, two blocks wholly padding | "ticket": 65,537
# live atoms under a capacity of 1,027 one-pass blocks: the ticket path with
# two dead blocks behind a block of one live lane.  The second batch loaded
# into the same buffers has the same molecule count, another order and 62
# atoms fewer, so the first batch's tail lies inside the second's padding.
# ---------------------------------------------------------------------------
CAPACITY = {"full": (320, 421), "mid": (300, 448), "ticket": (65537, 65537 + 128 + 63)}
CAPACITY_POOLED = "full"   # the case that also runs through EgoPrefetch
EGO_PAD = (131, 257)       # ego rows / columns of capacity past the larger batch's need
_CAP_UNIT = [ring64(), PAIR, ring64(), path(62), ring64(), wheel(12), wheel(6), wheel(7), LOOP]


def capacity_motifs(n):
    """(first, second) motif lists: the first of exactly n atoms."""
    out, left = _tiled(n, _CAP_UNIT)
    if left == 1:  # no one-atom molecule: give the last motif back
        left += out.pop()[0]
    first = out + ([LOOP] if left % 2 else []) + [PAIR] * ((left - (3 if left % 2 else 0)) // 2)
    assert sum(m[0] for m in first) == n
    second = first[::-1]
    i = next(j for j, m in enumerate(second) if m[0] == 64)
    second[i] = PAIR
    return first, second


# ---------------------------------------------------------------------------
# batches and oracle results, built once and shared
# ---------------------------------------------------------------------------
_BATCHES = {}


def case_graph(pkg, table, key):
    """Host batch of case `key` of table "window" | "degree" | "blocks" |
    "words" | "rejected"."""
    if (table, key) not in _BATCHES:
        motifs = {"window": lambda: WINDOW[key][0], "degree": lambda: DEGREE[key],
                  "blocks": lambda: block_motifs(key), "words": lambda: words_motifs(key),
                  "rejected": lambda: words_motifs(key)}[table]()
        _BATCHES[table, key] = batch(pkg, motifs)
    return _BATCHES[table, key]


def capacity_case(pkg, name, k):
    """The two host batches of capacity case `name` (with a one-column x, which
    StaticBatch.pad copies) and the capacities of a StaticBatch that holds
    either: SimpleNamespace(first, second, B, n_cap, e_cap, mgn, caps)."""
    if ("capacity", name, k) not in _BATCHES:
        n, n_cap = CAPACITY[name]
        graphs = [batch(pkg, m) for m in capacity_motifs(n)]
        for g in graphs:
            g.ndata["x"] = torch.zeros(g.num_nodes(), 1)
        _, e_cap, mgn, caps = pkg.graph.StaticBatch.capacities(graphs, k, slack=1.0)
        caps = (caps[0] + EGO_PAD[0], caps[1] + EGO_PAD[1], caps[2])
        _BATCHES["capacity", name, k] = SimpleNamespace(
            first=graphs[0], second=graphs[1], B=graphs[0].batch_size, n_cap=n_cap, e_cap=e_cap,
            mgn=mgn, caps=caps)
    return _BATCHES["capacity", name, k]


_ORACLE = {}


def oracle(g, k):
    """oracle.egonet.egonets of host batch g in the ego batch's ids:
    SimpleNamespace(sizes, ecount, nodes, row, col, n_s, e_s) -- row / col are
    the ego batch's CSR entries in DGL order.  Computed once per (batch, k);
    callers leave the arrays unchanged."""
    key = (id(g), k)
    if key not in _ORACLE:
        sizes, ecount, nodes, esrc, edst = egonet.egonets(g.rowptr.numpy(), g.col.numpy(), k)
        ptr = np.concatenate([[0], np.cumsum(sizes)])
        eoff = np.repeat(ptr[:-1], ecount)  # ego-local -> ego-batch ids
        _ORACLE[key] = (g, SimpleNamespace(sizes=sizes, ecount=ecount, nodes=nodes,
                                           row=esrc + eoff, col=edst + eoff,
                                           n_s=int(sizes.sum()), e_s=int(ecount.sum())))
    return _ORACLE[key][1]
