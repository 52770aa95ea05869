"""Host side of tests/test_gpu_s2s_edges.py: the case tables of
tests/s2s_edge_cases.py name every edge of csrc/set2set.hip they claim to
(against the mirrored constants), the written-out fp64 reference equals the
oracle where the oracle is defined and does the right thing on empty graphs
where it is not, and the same reference in float32 stays a factor of ten
inside the bounds the device tests use — so those bounds measure the kernels,
not the conditioning of the inputs.  A retune of kS2SRows, the row groups or
the padding tile fails here first: then move the tables with it."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import s2s_edge_cases as S
from oracle import scgib_ref as R


def test_tables_name_every_edge():
    c = S.EDGE_COUNTS
    assert len(c) == 16 and sum(c) == S.EDGE_ROWS == 725
    assert int(S.graph_ptr(c)[-1]) == S.EDGE_ROWS  # ptr[B] is the live row count
    # empty graphs: first, in the middle, two at the end
    assert [i for i, n in enumerate(c) if n == 0] == [0, 3, 14, 15]
    # the staging limit and its neighbours
    assert {S.S2S_ROWS - 1, S.S2S_ROWS, S.S2S_ROWS + 1} <= set(c)
    # + 15 / + 16 / + 17: the 16 row groups take 0 or 1, exactly 1, 1 or 2 global rows
    near = [S.S2S_ROWS + S.ROW_GROUPS + k for k in (-1, 0, 1)]
    assert set(near) <= set(c)
    assert [S.global_rows_per_group(n) for n in near] == [(0, 1), (1, 1), (1, 2)]
    assert S.global_rows_per_group(S.S2S_ROWS + 1) == (0, 1)
    assert S.global_rows_per_group(2 * S.S2S_ROWS) == (4, 4)
    assert S.global_rows_per_group(2 * S.S2S_ROWS + 1) == (4, 5)
    assert {1, 2, S.ROW_GROUPS, S.ROW_GROUPS + 1, 2 * S.S2S_ROWS, 2 * S.S2S_ROWS + 1} <= set(c)
    assert S.SOLO_COUNTS == [64, 63, 65, 1, 79, 80, 81, 2, 16, 17, 128, 129]
    # widths: every staging / dot combination, REG, and the kB = 16 tails
    w = S.WIDTHS
    assert w == sorted(set(w)) and w[0] == 1 and w[-1] == S.S2S_MAX_D
    assert any(d % 4 == 0 and d < S.S2S_MAX_D for d in w)          # non-REG float4
    assert any(d % 2 == 0 and d % 4 != 0 for d in w) and 14 in w   # mixed
    assert any(d % 2 == 1 for d in w) and {62, 63} <= set(w)
    assert {d % 16 for d in w} >= {0, 1, 12, 14, 15}               # exact and clamped batches
    assert {-(-d // 16) for d in w} == {1, 2, 3, 4}                # channel passes j + 16 k
    # rounds and round counts
    assert S.ROUNDS == [1, 2, 3, 5]
    R_counts = {B * T for B in (1, 3, 5) for T in S.ODD_ROUNDS}
    assert R_counts == {1, 3, 5, 9, 15, 25} and all(r % 2 for r in R_counts)
    assert {r % 4 for r in R_counts} == {1, 3}
    assert sorted(S.SMALL_BATCHES) == [3, 5]
    assert all(len(v) == B and min(v) > 0 for B, v in S.SMALL_BATCHES.items())
    # padding: one iteration before, 16 / 16 / 19 now, the last under the block cap
    assert S.padding_strides(S.EDGE_ROWS, S.EDGE_ROWS + S.PAD_ROWS, 64) == 1
    strides = [S.padding_strides(int(np.sum(cnt)), rows, d) for cnt, rows, d in S.PADDING_CASES]
    blocks = [S.padding_blocks(rows, d) for _, rows, d in S.PADDING_CASES]
    assert strides == [16, 16, 19] and blocks == [63, 9, S.PAD_BLOCKS_MAX]
    cnt, rows, d = S.PADDING_CASES[2]
    assert rows * d > 2 ** 20 and -(-rows * d // S.PAD_TILE) > S.PAD_BLOCKS_MAX


@pytest.mark.parametrize("T", S.ROUNDS)
def test_reference_equals_the_oracle_without_empty_graphs(T):
    """Exactly: the same fp64 operations in the same order."""
    counts = [n for n in S.EDGE_COUNTS if n > 0]
    for d in (64, 9):
        state = S.lstm_state(d)
        feat, w = S.make_inputs(d, counts)
        mine = S.ref_run(state, [feat], [w], counts, T)
        p = {"s2s.lstm." + k: v.double().clone().requires_grad_(True) for k, v in state.items()}
        fc = feat.double().requires_grad_(True)
        ref = R.set2set(p, "s2s", fc, torch.tensor(counts), n_iters=T)
        (ref * w.double()).sum().backward()
        assert float(np.abs(mine["out"][0] - ref.detach().numpy()).max()) == 0.0
        assert float(np.abs(mine["dx"][0] - fc.grad.numpy()).max()) == 0.0
        for k in S.LSTM_KEYS:
            assert float(np.abs(mine["lstm"][k] - p["s2s.lstm." + k].grad.numpy()).max()) == 0.0


@pytest.mark.parametrize("T", S.ROUNDS)
def test_empty_graphs_in_the_reference(T):
    d = 6
    state, feat, w, ref = S.edge_reference(d, T)
    empty = [g for g, n in enumerate(S.EDGE_COUNTS) if n == 0]
    live = [g for g, n in enumerate(S.EDGE_COUNTS) if n > 0]
    out = ref["out"][0]
    assert np.isfinite(out).all()
    # q* = [h, 0], h that of an LSTM whose readout input was zero every round
    p = {k: v.double() for k, v in state.items()}
    h = c = torch.zeros(d, dtype=torch.float64)
    for _ in range(T):
        q = torch.cat([h, torch.zeros(d, dtype=torch.float64)])
        gates = p["weight_ih_l0"] @ q + p["weight_hh_l0"] @ h + (p["bias_ih_l0"] + p["bias_hh_l0"])
        i, f, g, o = gates.chunk(4)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
    for g in empty:
        assert np.abs(out[g, d:]).max() == 0.0
        assert np.abs(out[g, :d] - h.numpy()).max() < 1e-15
    # the live graphs are those of the batch without the empty ones, exactly
    counts = [S.EDGE_COUNTS[g] for g in live]
    alone = S.ref_run(state, [feat], [w[live]], counts, T)
    assert np.array_equal(alone["out"][0], out[live])
    assert np.array_equal(alone["dx"][0], ref["dx"][0])
    # an upstream gradient on the empty graphs only: no feature gradient, and
    # the LSTM's flows through h alone (the readout half of W_ih sees zeros)
    w0 = torch.zeros_like(w)
    w0[empty] = w[empty]
    only = S.ref_run(state, [feat], [w0], S.EDGE_COUNTS, T)
    assert np.abs(only["dx"][0]).max() == 0.0
    assert np.abs(only["lstm"]["weight_ih_l0"][:, d:]).max() == 0.0
    assert np.abs(only["lstm"]["bias_ih_l0"]).max() > 0.0
    if T > 1:
        assert np.abs(only["lstm"]["weight_ih_l0"][:, :d]).max() > 0.0
        assert np.abs(only["lstm"]["weight_hh_l0"]).max() > 0.0


@pytest.mark.parametrize("T", S.ROUNDS)
def test_float32_reference_is_ten_times_inside_the_bounds(T):
    """The conditioning guard: ref_set2set in float32 on the CPU, judged as
    the device tests judge the kernels (per graph, per tensor), for every
    width.  At unit feature scale the softmax is soft and float32 loses a few
    ulp; the device bounds then hold with a factor of ten to spare for the
    kernels' summation order."""
    worst = {"out": 0.0, "dx": 0.0, "lstm": 0.0}
    for d in S.WIDTHS:
        state, feat, w, ref = S.edge_reference(d, T)
        f32 = S.ref_run(state, [feat], [w], S.EDGE_COUNTS, T, torch.float32)
        worst["out"] = max(worst["out"], S.out_err(f32["out"][0], ref["out"][0]))
        worst["dx"] = max(worst["dx"], S.dx_err(f32["dx"][0], ref["dx"][0], S.EDGE_COUNTS))
        worst["lstm"] = max(worst["lstm"], *S.lstm_errs(f32["lstm"], ref["lstm"]).values())
    print(f"T={T}: float32 reference rel_err out {worst['out']:.3g} dx {worst['dx']:.3g} "
          f"lstm {worst['lstm']:.3g}")
    assert worst["out"] <= S.OUT_TOL / 10
    assert worst["dx"] <= S.DX_TOL / 10
    assert worst["lstm"] <= S.LSTM_TOL / 10


def test_sharp_inputs_overflow_without_the_max():
    """test_sharp_logits' premise: at feature scale 30 the fp64 logits pass
    expf's overflow (88.7), so a softmax without the max-subtraction is inf."""
    state, feat, w, ref = S.edge_reference(64, 2, S.SHARP_SCALE)
    # the last round's query is the first half of the output
    seg = np.repeat(np.arange(len(S.EDGE_COUNTS)), S.EDGE_COUNTS)
    e = (feat.double().numpy() * ref["out"][0][seg, :64]).sum(-1)
    print(f"largest last-round logit {float(e.max()):.4g}")
    assert float(e.max()) > 88.73
    assert np.isfinite(ref["out"][0]).all() and np.isfinite(ref["dx"][0]).all()
