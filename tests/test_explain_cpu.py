"""CPU side of the graph-core / significant-subgraph feature (csrc/explain.hip,
DESIGN.md §26): the C-ABI entries, the numpy reference on hand-made cases, the
no-device error, and the two derivations that read lam / alpha back out of a
recorded reference forward, pinned against the fp64 restatement on the five
train-mode goldens (so the GPU test's references are themselves checked)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import explain_ref as E
from conftest import MODEL_GOLDENS, load_golden, rel_err
from oracle import scgib_ref as R

ACT_TOL = 1e-4  # tests/test_gpu_parity.py

ENTRIES = {"scgib_explain_stage_rows": 0, "scgib_explain_rank": 13, "scgib_explain_core_mask": 11,
           "scgib_explain_core_ws_words": 1, "scgib_explain_core_count": 9,
           "scgib_explain_core_fill": 16, "scgib_explain_store": 15}


def test_entries_are_added_without_an_abi_bump(pkg):
    L = pkg._lib
    assert L.ABI_VERSION == 24 and L.load().scgib_abi_version() == 24
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "include", "scgib.h")).read()
    for name, nargs in ENTRIES.items():
        assert name in L.SIGNATURES and name + "(" in header, name
        assert len(L.SIGNATURES[name][1]) == nargs, name
        assert getattr(L.load(), name) is not None
    assert L.SIGNATURES["scgib_explain_core_mask"][1][6] is L._D  # ratio crosses as a double
    assert L.query("scgib_explain_stage_rows") == 512
    assert L.query("scgib_explain_core_ws_words", 0) == 4
    assert L.query("scgib_explain_core_ws_words", 257) == 2 * 258 + 2 * 2


def test_bad_arguments_do_not_launch(pkg):
    L = pkg._lib.load()
    assert L.scgib_explain_rank(None, None, None, -1, 0, 0, None, None, None, None, None, 0,
                                None) == -1
    assert L.scgib_explain_rank(None, None, None, 0, 0, 1, None, None, None, None, None, 0,
                                None) == -1  # (no graph_ptr)
    for ratio in (0.0, 1.5, float("nan")):
        assert L.scgib_explain_core_mask(None, None, None, 0, 0, 0, ratio, 0.0, None, 0,
                                         None) == -1
    assert L.scgib_explain_store(None, None, None, None, None, 3, None, None, 1, 1, None, None,
                                 None, None, None) == -1


# ---------------------------------------------------------------------------
# the numpy reference on hand-made cases
# ---------------------------------------------------------------------------
def test_ranks_ties_nan_inf_zero():
    nan, inf = np.nan, np.inf
    gptr = np.array([0, 4, 9, 10, 14])
    keys = np.array([0.5, 0.7, 0.5, 0.1,            # a tie: the lower id first
                     nan, 1.0, nan, -inf, inf,      # NaN after -inf, NaNs by id
                     nan,                            # a single atom
                     0.0, -0.0, 1e-30, -0.0], np.float32)  # -0.0 ties with +0.0
    want = [1, 0, 2, 3,
            3, 1, 4, 2, 0,
            0,
            1, 2, 0, 3]
    assert E.ranks(keys, gptr).tolist() == want
    assert E.ranks(np.full(5, 2.0, np.float32), np.array([0, 5])).tolist() == [0, 1, 2, 3, 4]


def test_centres_pad_with_minus_one():
    gptr = np.array([0, 2, 7])
    alpha = np.array([0.25, 0.75, 0.1, 0.3, 0.2, 0.3, 0.1], np.float32)
    rk = E.ranks(alpha, gptr)
    c, w = E.centres(alpha, rk, gptr, 3)
    assert c.tolist() == [[1, 0, -1], [3, 5, 4]]
    assert w.tolist() == [[0.75, 0.25, 0.0], [np.float32(0.3), np.float32(0.3), np.float32(0.2)]]


@pytest.mark.parametrize("n", [1, 2, 3, 7, 10, 64, 600])
def test_core_size_rule(n):
    gptr = np.array([0, n])
    assert E.core_sizes(gptr, 1.0 / n)[0] == 1
    assert E.core_sizes(gptr, 0.5)[0] == max(1, -(-n // 2))
    assert E.core_sizes(gptr, 1.0)[0] == n
    assert E.core_sizes(gptr, 1e-9)[0] == 1
    lam = np.linspace(0.0, 1.0, n).astype(np.float32)
    keep = E.core_keep(lam, E.ranks(lam, gptr), gptr, ratio=0.5)
    assert keep.sum() == max(1, -(-n // 2)) and keep[-1]  # the largest gates


def test_threshold_rule_never_keeps_nan():
    lam = np.array([0.2, np.nan, 0.9, 0.5], np.float32)
    gptr = np.array([0, 4])
    assert E.core_keep(lam, None, gptr, threshold=0.5).tolist() == [False, False, True, True]
    assert not E.core_keep(lam, None, gptr, threshold=2.0).any()


def test_core_reference_on_a_path_with_a_self_loop():
    # molecule 0: path 0-1-2-3 with a self-loop at 2; molecule 1: a 2-atom bond
    src = np.array([0, 1, 1, 2, 2, 2, 3, 4, 5])
    dst = np.array([1, 0, 2, 1, 2, 3, 2, 5, 4])
    gptr = np.array([0, 4, 6])
    keep = np.array([True, False, True, True, False, False])
    rowptr, col, gp, ids = E.core_reference(src, dst, gptr, keep)
    assert ids.tolist() == [0, 2, 3] and gp.tolist() == [0, 3, 3]
    assert rowptr.tolist() == [0, 0, 2, 3]  # atom 0 kept, its only neighbour dropped
    assert col.tolist() == [1, 2, 1]


# ---------------------------------------------------------------------------
def test_explain_on_cpu_tensors_raises(pkg):
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=4, gin_layers=2, task="graph_classification")
    model = pkg.models.Mainmodel(args, 11, 64, 4, 4, 1, "GIN").eval()
    gh, _ = pkg.graph.collate_pyg(pkg.synth.molecules(3, "qm9", seed=0))
    x = gh.ndata["x"].float()
    with pytest.raises(pkg._lib.ScgibError, match="HIP device"):
        model.explain(gh, x)
    with pytest.raises(RuntimeError, match="eval"):
        model.train().explain(gh, x)
    lam = torch.zeros(gh.num_nodes())
    with pytest.raises(pkg._lib.ScgibError, match="HIP device"):
        pkg.ops.explain_rank(lam, lam, gh, 1)
    with pytest.raises(pkg._lib.ScgibError, match="HIP device"):
        pkg.ops.core_subgraph(lam, lam.int(), gh, ratio=0.5)
    with pytest.raises(ValueError):
        pkg.ops.core_subgraph(lam, lam.int(), gh, ratio=0.5, threshold=0.1)


# ---------------------------------------------------------------------------
# the derivations against the fp64 restatement, on the train-mode goldens
# ---------------------------------------------------------------------------
def golden_case(name):
    """Everything both the CPU and the GPU test need of a train-mode golden,
    computed once: the fp64 lam / alpha, and the two read back from the
    reference's recorded activations."""
    if name not in _CASES:
        g = load_golden(name)
        params = R.strip_continue({k[6:]: v for k, v in g.items() if k.startswith("param_")})
        counts = g["batch_num_nodes"]
        s64 = E.ego_sums(g["act_subgraph_features"], g["ego_batch_num_nodes"])
        lam64, alpha64, _ = E.lam_alpha_fp64(params, g["act_graph_features"], s64, counts,
                                             g["u_gate"], True)
        lam_d, usable = E.lam_from_noisy(g["act_noisy"], g["act_graph_features"], g["u_feat"],
                                         counts)
        alpha_d = E.alpha_from_map(g["act_interaction_map"], g["act_subgraph_features"],
                                   g["ego_batch_num_nodes"])
        _CASES[name] = SimpleNamespace(g=g, params=params, counts=counts, lam64=lam64,
                                       alpha64=alpha64, lam_d=lam_d, usable=usable,
                                       alpha_d=alpha_d, gptr=E.gptr_of(counts))
    return _CASES[name]


_CASES = {}


@pytest.mark.parametrize("name", MODEL_GOLDENS)
def test_derived_lam_and_alpha_match_the_restatement(name):
    c = golden_case(name)
    n = len(c.lam64)
    left_out = int((~c.usable).sum())
    print(f"{name}: rows {n}, left out for lam {left_out}")
    # only the rows of 2-atom molecules, and at most 5 % of the rows
    assert (~c.usable).tolist() == np.repeat(np.diff(c.gptr) == 2, np.diff(c.gptr)).tolist()
    assert 0 < left_out <= 0.05 * n
    e_lam = rel_err(c.lam_d[c.usable], c.lam64[c.usable])
    e_alpha = rel_err(c.alpha_d, c.alpha64)
    sums = np.add.reduceat(c.alpha_d, c.gptr[:-1])
    print(f"  lam rel {e_lam:.2e}  alpha rel {e_alpha:.2e}  |sum alpha - 1| "
          f"{np.abs(sums - 1).max():.2e}")
    assert e_lam < ACT_TOL and e_alpha < ACT_TOL
    assert np.abs(sums - 1).max() < 2e-7  # fp32 activations behind the quotient
