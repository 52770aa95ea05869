"""Row counts, widths and round counts at which the Set2Set kernels
(csrc/set2set.hip) change code path, the batches that hold them, and the fp64
side of the checks that tests/test_gpu_s2s_edges.py (device) and
tests/test_s2s_edges_cpu.py (host) share.  Plain module: no fixtures, no
device work at import."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from conftest import rel_err

S2S_ROWS = 64               # rows of a graph staged in LDS (csrc kS2SRows)
S2S_MAX_D = 64              # widest input (csrc kS2SMaxD)
ROW_GROUPS = 16             # row groups of 16 lanes: group G takes rows G, G + 16, ...
PAD_TILE = 256 * 16         # floats of dx one padding-zero block covers per launch sizing
PAD_BLOCKS_MAX = 256        # cap of the padding-zero blocks
PAD_ROWS = 37               # the padding rows of the existing Set2Set tests
# The inputs' seed.  At d = 1, T = 1 every LSTM gradient is one scalar sum over
# the graphs (one channel, and round 0's h is the same for every graph); under
# seed 53 that sum cancelled to 1e-3 of its terms and the float32 reference
# itself was 4e-4 off.  tests/test_s2s_edges_cpu.py's conditioning guard holds
# whatever seed stands here to a tenth of the device bounds.
SEED = 54

# ---------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------
# One batch, B = 16, 725 rows: an empty graph first, one in the middle, two at
# the end (ptr[B] is still the live row count) | kS2SRows and its neighbours |
# 64 + 15 / + 16 / + 17 rows: the 16 row groups take 0 or 1, exactly 1, and 1
# or 2 global rows | one and two rows | one row per group, and one group with
# two | two and two-plus-one full staging loads
EDGE_COUNTS = [0, 64, 63, 0, 65, 1, 79, 80, 81, 2, 16, 17, 128, 129, 0, 0]
EDGE_ROWS = 725
# B = 1 with each non-zero count (R = T: odd for T = 1, 3, 5), and small
# batches of B = 3 and B = 5 (R = 3 T, 5 T: R = 5 wraps set2set_wgrad_k's four
# r & 3 accumulators with one round in the first)
SOLO_COUNTS = [c for c in EDGE_COUNTS if c > 0]
SMALL_BATCHES = {3: [5, 1, 9], 5: [3, 7, 1, 4, 2]}
ODD_ROUNDS = [1, 3, 5]
ODD_WIDTHS = [64, 9]

WIDTHS = [
    1,   # scalar staging, scalar w_ih (n = 2) and w_hh dots; one lane of 16 holds a channel
    2,   # scalar staging, w_ih dot float4 (n = 4), w_hh scalar: the mixed path at its smallest
    3,   # scalar staging, both dots scalar (n = 6, 3); 3 d = 9 transposed outputs
    4,   # float4 staging and both dots float4 at their smallest (one float4 per w_hh row)
    6,   # mixed: d even, d % 4 != 0 (w_ih rows of 12 floats as float4, w_hh rows of 6 scalar)
    9,   # odd: all scalar (the raw OGB width the suite already runs)
    14,  # mixed, Mutagenicity's F = 14; the last width below one full j + 16 k pass
    16,  # non-REG float4; channels j only (k = 0 full, k >= 1 empty); the kB = 16 batch exact
    17,  # odd; channel 16 alone in the k = 1 pass; kB tail of one row (clamped 15 times)
    32,  # non-REG float4; two full j + 16 k passes; two full kB batches; 3 d = 96 > 64 outputs
    48,  # non-REG float4; three channel passes; 4 d = 192 gate threads, three kB batches
    60,  # non-REG float4 just under REG; kB tail of 12 rows; 3 d = 180 outputs
    62,  # mixed at the top: kB tail of 14 rows in the clamped load
    63,  # odd at the top: all scalar, kB tail of 15 rows; 4 d = 252 gate threads
    64,  # REG: weights in registers, every thread a gate
]
ROUNDS = [
    1,   # no transposed product, REG preload skipped, dx written without accumulation
    2,   # the only count the suite ran before
    3,   # the global-row dx accumulates twice; sDC / sDH carry across rounds
    5,   # four accumulations; R = B T odd for odd B
]
SHARP_SCALE = 30.0          # test_sharp_logits: fp64 logits past 88 (expf's overflow)
SHARP_FACTOR = 8.0          # the kernel's other (fixed) summation order over <= 129 rows
# the project's Set2Set bounds (tests/test_gpu_parity.py, tests/test_gpu_readout.py)
OUT_TOL, DX_TOL, LSTM_TOL = 1e-5, 1e-4, 1e-4
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

# test_padding_rows_zeroed: (live counts, buffer rows, width)
PADDING_CASES = [
    ([60, 40], 4000, 64),        # 100 live rows: 63 blocks, every thread strides 16 times
    ([60, 40], 4000, 9),         # the same, odd width (9 blocks)
    (EDGE_COUNTS, 20000, 64),    # n_rows d > 2^20: 313 blocks capped at 256, 19 strides
]


def padding_blocks(n_rows, d):
    """The padding-zero blocks set2set_bwd launches past the graphs'."""
    tail = -(-n_rows * d // PAD_TILE)
    return min(max(tail, 1), PAD_BLOCKS_MAX)


def padding_strides(live_rows, n_rows, d):
    """Iterations of the longest padding-zero thread's grid-stride loop."""
    return -(-(n_rows - live_rows) * d // (padding_blocks(n_rows, d) * 256))


def global_rows_per_group(count):
    """(fewest, most) rows past the staged ones that a row group takes."""
    extra = max(count - S2S_ROWS, 0)
    return extra // ROW_GROUPS, -(-extra // ROW_GROUPS)


# ---------------------------------------------------------------------------
# batches and inputs
# ---------------------------------------------------------------------------
def graph_ptr(counts):
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)


def stand_in(counts, dev=None):
    """What ops.set2set reads of a batch: graph_ptr and batch_size."""
    ptr = graph_ptr(counts)
    return SimpleNamespace(graph_ptr=ptr if dev is None else ptr.to(dev), batch_size=len(counts))


def lstm_state(d, seed=SEED):
    """nn.LSTM(2 d, d)'s own initialisation, from a seeded CPU generator
    (the global one, forked: nothing outside sees the draw)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1000 * seed + d)
        lstm = torch.nn.LSTM(2 * d, d, 1)
    return {k: v.detach().clone() for k, v in lstm.state_dict().items()}


def make_inputs(d, counts, seed=SEED, scale=1.0, rows=None):
    """(feat [rows, d], upstream w [B, 2 d]) fp32; the live rows are a
    function of (d, counts, seed) alone, rows past them (capacity padding)
    hold live-looking values that nothing may read."""
    n = int(np.sum(counts))
    gen = torch.Generator().manual_seed(1000 * seed + 7 * d + n)
    feat = scale * torch.randn(n, d, generator=gen)
    w = torch.randn(len(counts), 2 * d, generator=gen)
    pad = (rows or n) - n
    if pad:
        feat = torch.cat([feat, 3 + torch.rand(pad, d, generator=gen)])
    return feat, w


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def ref_set2set(p, feat, counts, n_iters):
    """DGL Set2Set(d, n_iters, 1), written out: p holds nn.LSTM's four
    parameters under "s2s.lstm." (the oracle's keys), in feat's dtype.  The
    operations and their order are oracle.scgib_ref.set2set's, so on a batch
    without empty graphs the two agree exactly; an empty graph reads out zeros
    (its softmax has no terms) and its q* is [h, 0]."""
    counts = torch.as_tensor(np.asarray(counts), dtype=torch.int64)
    B, d = len(counts), feat.shape[1]
    seg = torch.repeat_interleave(torch.arange(B), counts)
    w_ih, w_hh = p["s2s.lstm.weight_ih_l0"], p["s2s.lstm.weight_hh_l0"]
    b = p["s2s.lstm.bias_ih_l0"] + p["s2s.lstm.bias_hh_l0"]
    hx = feat.new_zeros(B, d)
    cx = feat.new_zeros(B, d)
    q_star = feat.new_zeros(B, 2 * d)
    for _ in range(n_iters):
        # gates (i, f, g, o) and the cell
        gates = q_star @ w_ih.t() + hx @ w_hh.t() + b
        i, f, g, o = gates.chunk(4, dim=1)
        cx = torch.sigmoid(f) * cx + torch.sigmoid(i) * torch.tanh(g)
        hx = torch.sigmoid(o) * torch.tanh(cx)
        # per-row logit, per-graph max (0 for a graph without rows: unused)
        e = (feat * hx[seg]).sum(dim=-1)
        emax = torch.stack([e[seg == k].max() if int(counts[k]) else e.new_zeros(())
                            for k in range(B)])
        a = torch.exp(e - emax[seg])
        den = torch.zeros(B, dtype=feat.dtype).index_add(0, seg, a)
        alpha = (a / den[seg]).unsqueeze(-1)
        readout = torch.zeros(B, d, dtype=feat.dtype).index_add(0, seg, feat * alpha)
        q_star = torch.cat([hx, readout], dim=-1)
    return q_star


def ref_run(state, feats, ws, counts, n_iters, dtype=torch.float64):
    """ref_set2set forward and backward in ``dtype`` over one parameter set:
    ``feats`` / ``ws`` are lists (one input, or the pair's two), the loss is
    sum_i (out_i * w_i).sum().  Returns numpy: outs, dxs, LSTM gradients."""
    p = {"s2s.lstm." + k: v.detach().to(dtype).clone().requires_grad_(True)
         for k, v in state.items()}
    fs = [f.detach().to(dtype).clone().requires_grad_(True) for f in feats]
    outs = [ref_set2set(p, f, counts, n_iters) for f in fs]
    sum((o * w.to(dtype)).sum() for o, w in zip(outs, ws)).backward()
    return {"out": [o.detach().numpy() for o in outs],
            "dx": [f.grad.numpy() for f in fs],
            "lstm": {k: p["s2s.lstm." + k].grad.numpy() for k in LSTM_KEYS}}


_REF = {}


def edge_reference(d, n_iters, scale=1.0):
    """(state, feat, w, fp64 ref_run) of the edge batch at width d: computed
    once per (d, n_iters, scale), shared, never changed."""
    key = (d, n_iters, scale)
    if key not in _REF:
        state = lstm_state(d)
        feat, w = make_inputs(d, EDGE_COUNTS, scale=scale)
        _REF[key] = (state, feat, w, ref_run(state, [feat], [w], EDGE_COUNTS, n_iters))
    return _REF[key]


# ---------------------------------------------------------------------------
# the judges
# ---------------------------------------------------------------------------
def out_err(mine, ref):
    """Worst graph's rel_err of the output: each row against its own
    reference maximum, so one edge graph cannot hide under another's scale."""
    mine, ref = np.asarray(mine), np.asarray(ref)
    return max(rel_err(mine[g], ref[g]) for g in range(ref.shape[0]))


def dx_err(mine, ref, counts):
    """Worst non-empty graph's rel_err of dx over that graph's rows."""
    mine, ref = np.asarray(mine), np.asarray(ref)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    return max(rel_err(mine[a:b], ref[a:b]) for a, b in zip(ptr[:-1], ptr[1:]) if b > a)


def lstm_errs(mine, ref):
    """{parameter: rel_err} of the four LSTM gradients, per tensor."""
    return {k: rel_err(np.asarray(mine[k]), ref[k]) for k in LSTM_KEYS}
