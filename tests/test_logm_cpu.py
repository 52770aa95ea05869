"""CPU-only checks of the device logM path's host surface:
exports, the ctypes table against the header, LogMSparse.to_dense, and the
refusals of CPU tensors.  Nothing is launched."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_host_cpu import _header_prototypes

NEW = ("scgib_logm_max_k", "scgib_logm_max_graph_nodes", "scgib_logm_targets",
       "scgib_recon_logm_sparse_parts", "scgib_recon_logm_sparse_fwd",
       "scgib_recon_logm_sparse_bwd")


def test_names_exist_and_are_exported(pkg):
    assert callable(pkg.graph.logm_targets)
    assert isinstance(pkg.graph.LogMSparse, type)
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in pkg._lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the stated domain: k <= 4 included, molecules up to the ego builder's 512
    assert pkg._lib.query("scgib_logm_max_k") >= 4
    assert pkg._lib.query("scgib_logm_max_graph_nodes") == 512
    # one Gram part plus one per 64-row chunk of the largest molecule, at most 8
    assert [pkg._lib.query("scgib_recon_logm_sparse_parts", n) for n in (1, 64, 65, 512, 4000)] \
        == [2, 2, 3, 9, 9]


def test_signatures_match_header(pkg):
    L = pkg._lib
    kind = {L._P: "P", L._I64: "I64", L._I32: "I32", L._F: "F", L._D: "D"}
    protos = _header_prototypes()
    for name in NEW:
        assert [kind[t] for t in L.SIGNATURES[name][1]] == protos[name], name


def test_argument_errors_do_not_launch(pkg):
    lib = pkg._lib.load()
    null = [None] * 7
    assert lib.scgib_logm_targets(None, None, None, 1, 4, 0, None, None, 4, 1, *null) == -1
    assert lib.scgib_recon_logm_sparse_fwd(None, None, 0, 4, None, None, 4, None, None, 1, 4,
                                           *[None] * 6) == -1
    assert lib.scgib_recon_logm_sparse_bwd(None, None, 1, 4, None, None, 4, None, None, 0, 4,
                                           *[None] * 4) == -1
    # k beyond the stated domain: refused before any launch (pointers are not read)
    buf = (ctypes.c_int32 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    kmax = int(pkg._lib.query("scgib_logm_max_k"))
    assert lib.scgib_logm_targets(p, p, p, 1, 4, 1, p, p, 4, kmax + 1, p, p, p, p, p, None,
                                  None) == -2


def test_to_dense_on_a_hand_built_instance(pkg):
    # molecules {0, 1, 2} and {3, 4}; balls (sorted, own node included):
    # 0: {0, 1}  1: {0, 1, 2}  2: {1, 2}  3: {3, 4}  4: {3, 4}
    ego_ptr = torch.tensor([0, 2, 5, 7, 9, 11], dtype=torch.int32)
    ego_nodes = torch.tensor([0, 1, 0, 1, 2, 1, 2, 3, 4, 3, 4], dtype=torch.int32)
    s_in = torch.arange(1, 12, dtype=torch.float32)
    lm = pkg.graph.LogMSparse(s_in, 2 * s_in, torch.zeros(2, dtype=torch.float64), 2, ego_ptr,
                              ego_nodes, torch.tensor([0, 3, 5], dtype=torch.int32))
    a, b = lm.to_dense()
    # slot j of ball(c) holds S[ego_nodes[j], c]
    np.testing.assert_array_equal(a, np.array([[1, 3, 0], [2, 4, 6], [0, 5, 7]], np.float32))
    np.testing.assert_array_equal(b, np.array([[8, 10], [9, 11]], np.float32))
    assert a.dtype == np.float32 and lm.kstep == 2 and lm.error() == 0


def test_cpu_tensors_are_refused(pkg):
    gh = pkg.graph.from_pyg(np.array([[0, 1], [1, 2]]), np.zeros((3, 1)))
    with pytest.raises(pkg._lib.ScgibError):
        pkg.graph.logm_targets(gh, 2)
    lm = pkg.graph.LogMSparse(torch.zeros(7), torch.zeros(7), torch.zeros(1, dtype=torch.float64),
                              1, torch.tensor([0, 2, 5, 7], dtype=torch.int32),
                              torch.tensor([0, 1, 0, 1, 2, 1, 2], dtype=torch.int32), gh.graph_ptr)
    with pytest.raises(pkg._lib.ScgibError):
        pkg.ops.recon_logm(torch.zeros(3, 64), gh, lm)


def test_model_on_cpu_still_needs_explicit_targets(pkg, monkeypatch):
    """recons_type='logM' with batch_logMs=None on CPU tensors: the ValueError
    stays (there is no CPU target builder).  The two device ops in front of
    the logM branch are stubbed so that the branch is reached without a GPU."""
    monkeypatch.setattr(pkg.models, "semi_loss", lambda z1, z2, chunk: torch.zeros(()))
    monkeypatch.setattr(pkg.ops, "mlp2", lambda im, mlp, dims: im[:, :64])
    args = SimpleNamespace(recons_type="logM", useAtt=1, readout_f="sum", d_transfer=32,
                           batch_size=2, gin_layers=2)
    m = pkg.models.Mainmodel(args, 11, 64, 4, 4, 1, "GIN")
    gh = pkg.graph.from_pyg(np.array([[0, 1], [1, 2]]), np.zeros((3, 1)))
    with pytest.raises(ValueError, match="batch_logMs"):
        m._losses(gh, torch.zeros(3, 128), torch.zeros(()), torch.zeros(1, 64),
                  torch.zeros(1, 64), m.MLP, 2, None)
