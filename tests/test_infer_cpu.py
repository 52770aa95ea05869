"""Host side of the molecule-resident eval forward and the scoring API
(csrc/infer.hip, s-cgib_amd/infer.py): the exports and their
ctypes table, refusals that must not launch, and the routing of ``"auto"``
(host logic only)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import infer_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("scgib_infer_max_nodes", "scgib_infer_max_ego_rows", "scgib_infer_ego_tile_rows",
           "scgib_infer_max_workgroups", "scgib_infer_fwd", "scgib_infer_store")


def _header_args(header, name):
    m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    args = [a.strip() for a in m.group(2).replace("\n", " ").split(",")]
    return m.group(1), ([] if args == ["void"] else args)


def _ctype_of(arg):
    if "*" in arg or arg.startswith("scgib_stream_t"):
        return ctypes.c_void_p
    return {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float,
            "double": ctypes.c_double}[arg.split()[0]]


def test_exports_match_the_header_without_an_abi_bump(pkg):
    L = pkg._lib
    assert L.ABI_VERSION == 24 and L.load().scgib_abi_version() == 24
    header = open(os.path.join(ROOT, "include", "scgib.h")).read()
    for name in ENTRIES:
        res, args = _header_args(header, name)
        want_res, want_args = L.SIGNATURES[name]
        assert want_res is (ctypes.c_int64 if res == "int64_t" else ctypes.c_int), name
        assert [_ctype_of(a) for a in args] == list(want_args), name
        assert getattr(L.load(), name) is not None
    # the parameter table: the header's struct field for field
    body = re.search(r"typedef struct \{([^}]*)\} scgib_infer_params;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*", "", f.strip().lstrip("*").strip())
                       for f in re.sub(r"^(const\s+)?\w+\s+", "", decl).split(",")]
    assert fields == [f[0] for f in L.InferParams._fields_]
    assert L.INFER_MAX_LAYERS == int(re.search(r"#define SCGIB_INFER_MAX_LAYERS (\d+)",
                                               header).group(1))
    n_ptr = 1 + 8 * 2 * L.INFER_MAX_LAYERS + 17
    assert ctypes.sizeof(L.InferParams) == 8 * n_ptr + 4 * 2 * L.INFER_MAX_LAYERS + 4 * 6 <= 4096


def test_limits_are_exported_and_inside_the_lds_budget(pkg):
    lim = pkg.ops.infer_limits()
    assert set(lim) == {"max_nodes", "max_ego_rows", "ego_tile_rows", "max_workgroups"}
    assert lim["max_nodes"] >= 64 and lim["max_ego_rows"] >= lim["max_nodes"]
    assert lim["max_ego_rows"] <= lim["ego_tile_rows"]  # an ego-net always fits a tile
    # three activation buffers and two weight tiles, row stride 65, in 160 KiB
    assert (3 * max(lim["max_nodes"], lim["ego_tile_rows"]) + 2 * 64) * 65 * 4 < 160 * 1024
    # the synthetic QM9 / molhiv / molpcba batches are inside them
    for wl in ("qm9", "molhiv", "molpcba"):
        mu = pkg.synth.WORKLOADS[wl][0]
        assert int(4 * mu) <= lim["max_nodes"], wl


def test_bad_arguments_do_not_launch(pkg):
    L = pkg._lib
    lib = L.load()
    assert lib.scgib_infer_fwd(None, None, 0, None, None, 0, None, 0, None, 0, None, None, None,
                               None, 0, 0, *([None] * 10)) == -1  # no table
    P = L.InferParams()
    P.n_layers, P.n_feat = 5, 9
    one = ctypes.c_int32(0)

    def call(n_layers=5, n_feat=9, mgn=10, err=ctypes.byref(one)):
        P.n_layers, P.n_feat = n_layers, n_feat
        return lib.scgib_infer_fwd(ctypes.byref(P), None, 0, None, None, 0, None, 1, None, mgn,
                                   None, None, None, None, 0, 0, None, None, None, None, None,
                                   None, None, None, err, None)

    assert call(n_layers=0) == -2 and call(n_layers=9) == -2
    assert call(n_feat=0) == -2 and call(n_feat=17) == -2
    assert call(mgn=pkg.ops.infer_limits()["max_nodes"] + 1) == -2
    assert call(err=None) == -1
    assert call() == -1  # supported sizes, NULL tensors
    assert one.value == 0
    assert lib.scgib_infer_store(None, 3, 1, None, 4, None, None) == -1
    assert lib.scgib_infer_store(None, 3, 0, None, 4, None, None) == -1


def _batch(pkg, sizes, seed=0):
    rng = np.random.default_rng(seed)
    return C.batch_of(pkg, [C.path(rng, n) for n in sizes])


def test_train_mode_and_cpu_tensors_are_refused(pkg):
    ft = C.finetune_model(pkg)
    g = _batch(pkg, [5, 7])
    x = g.ndata["x"]
    sc = pkg.infer.Scorer(ft.train(), "resident")
    for fn in (sc.score, sc.embed, sc.rows):
        with pytest.raises(RuntimeError, match="eval"):
            fn(g, x)
    ft.eval()
    for path in ("auto", "resident", "layers"):
        sc = pkg.infer.Scorer(ft, path)
        for fn in (sc.score, sc.embed):
            with pytest.raises(pkg._lib.ScgibError, match="no CPU fallback"):
                fn(g, x)
    with pytest.raises(pkg._lib.ScgibError, match="no CPU fallback"):
        pkg.ops.InferTable(ft.model.Encoder1, ft.model.Encoder2, ft.transfer_d,
                           ft.model.compressor, ft.model.attn_layer, True, ft.MLP, ft.s2s)
    with pytest.raises(pkg._lib.ScgibError, match="no CPU fallback"):
        pkg.ops.infer_forward(x, g, g, None, torch.rand(12), torch.rand(12, 64))
    with pytest.raises(ValueError):
        pkg.infer.Scorer(ft, "fast")
    with pytest.raises(TypeError):
        pkg.infer.Scorer(torch.nn.Linear(2, 2))


def test_score_needs_a_finetune_model(pkg):
    for model in (C.pretrain_model(pkg), C.pretrain_model(pkg, wrapped=False)):
        sc = pkg.infer.Scorer(model.eval(), "resident")
        g = _batch(pkg, [4])
        with pytest.raises(TypeError, match="predict head"):
            sc.score(g, g.ndata["x"])


def test_unsupported_models_refuse_resident_and_route_auto_to_layers(pkg, monkeypatch):
    monkeypatch.setattr(pkg.infer, "AUTO_RESIDENT", True)  # whatever the measured default is
    monkeypatch.setattr(pkg.models, "ALL_ENCODER_STRINGS", True)
    g = _batch(pkg, [6, 3])
    cases = [C.pretrain_model(pkg, encoder="GCN"), C.pretrain_model(pkg, encoder="Transformer"),
             C.pretrain_model(pkg, hidden=32), C.pretrain_model(pkg, hidden=32, wrapped=False)]
    for model in cases:
        model.eval()
        with pytest.raises(pkg._lib.ScgibError, match="resident"):
            pkg.infer.Scorer(model, "resident")
        assert pkg.infer.Scorer(model, "auto").route(g) == "layers"
        assert pkg.infer.Scorer(model, "layers").route(g) == "layers"
    assert pkg.infer.Scorer(C.pretrain_model(pkg).eval(), "auto").route(g) == "resident"


def test_a_molecule_above_the_limit(pkg, monkeypatch):
    monkeypatch.setattr(pkg.infer, "AUTO_RESIDENT", True)
    lim = pkg.ops.infer_limits()["max_nodes"]
    ft = C.finetune_model(pkg).eval()
    at, above = _batch(pkg, [3, lim]), _batch(pkg, [3, lim + 1, 2])
    assert at.max_graph_nodes == lim and above.max_graph_nodes == lim + 1
    res, auto = pkg.infer.Scorer(ft, "resident"), pkg.infer.Scorer(ft, "auto")
    assert res.route(at) == "resident" and auto.route(at) == "resident"
    assert auto.route(above) == "layers"
    with pytest.raises(pkg._lib.ScgibError, match="atoms"):
        res.route(above)
    # "auto" follows the measured switch
    monkeypatch.setattr(pkg.infer, "AUTO_RESIDENT", False)
    assert auto.route(at) == "layers" and res.route(at) == "resident"
