"""The graphs of tests/big_graphs.py have the properties that keep the GPU
tests built on them from being vacuous (checked here without a GPU)."""
import numpy as np
import pytest

import big_graphs as BG


@pytest.mark.parametrize("name", list(BG.BIG_SIZES))
def test_directed_graph_is_asymmetric_and_far_reaching(name):
    src, dst, n = BG.big_directed(name)
    assert n == BG.BIG_SIZES[name] and n % 2 == 0
    assert BG.tiles(n) == (256 if name == "big256" else 258)
    assert n % BG.TILE == (0 if name == "big256" else 6)
    assert BG.degree_asymmetry(src, dst, n) > 0.5
    assert BG.far_edge_share(src, dst) > 0.25
    assert len(set(zip(src.tolist(), dst.tolist()))) == src.size  # a simple graph
    assert not set(zip(src.tolist(), dst.tolist())) & set(zip(dst.tolist(), src.tolist()))
    # the reason n is even: at n + 1 the doubling map is a bijection
    s1, d1, n1 = BG.directed(n + 1)
    assert BG.degree_asymmetry(s1, d1, n1) < 0.5


def test_small_directed_graph_is_the_hand_graph():
    src, dst, n = BG.directed(70)
    assert n == 70 and BG.degree_asymmetry(src, dst, n) > 0.5


def test_big_molecule_batch_is_past_256_tiles_and_ragged(pkg):
    gh = BG.big_molecules(pkg)
    n = gh.num_nodes()
    assert n > 256 * 64 and n % 64 != 0
    assert BG.tiles(n) - 256 in (1, 2, 3)  # just past the line: seconds, not the workload


def test_capacity_splits_straddle_256_tiles(pkg):
    gh, caps = BG.capacity_case(pkg, "live_past_256")
    live, cap = BG.tiles(gh.num_nodes()), BG.tiles(caps[0])
    assert live >= 258 and cap >= live + 4  # a whole live second tile, a partly live one, padding
    gh, caps = BG.capacity_case(pkg, "live_below_256_below_capacity")
    live, cap = BG.tiles(gh.num_nodes()), BG.tiles(caps[0])
    assert live < 256 < cap
    only_padding = np.arange(live, 256)       # workgroups that never see a live row
    live_then_padded = np.arange(0, cap - 256)  # second tile = tile 256 + w, padded
    assert only_padding.size >= 32 and live_then_padded.size >= 32
    assert live_then_padded.max() < live
