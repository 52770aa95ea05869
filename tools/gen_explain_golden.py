"""Golden fixture for the eval-mode preservation gate and attention weights,
from the REFERENCE's own model code.

TEST INFRASTRUCTURE ONLY, build container only (it imports the reference
behind ``oracle/refshim.py``, as ``oracle/gen_golden.py`` does).  Writes

  tests/golden/explain_eval_L5_k1.npz

for the B = 8, L = 5, k = 1 QM9-like batch with the 2-atom molecule: a
Mainmodel after one train-mode forward (so the BatchNorm running statistics
are off their initial values), switched to eval(), and from one eval-mode
forward of the reference's own code

  u_gate / u_feat ....... the recorded draws (models.py:599, 650)
  lam_ref / p_ref ....... lambda_pos and p of ``compress`` per molecule
                          (models.py:595-604), by wrapping the method
  attn_logit_ref ........ the ``attn_layer`` outputs per molecule (forward
                          hook, models.py:745)
  alpha_ref ............. their softmax(dim=0) per molecule (models.py:746)

plus the inputs and the ``param_`` keys (parameters and buffers after the
train-mode forward).  Plain ``.npz`` data; no GPU test reads the reference or
this tool.

Usage:  python tools/gen_explain_golden.py        (from the repo root)
"""
from __future__ import annotations

import importlib
import os
import sys
from itertools import chain
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import refshim  # noqa: E402
from oracle import dgl_semantics as D  # noqa: E402
from oracle import gen_golden as GG  # noqa: E402

synth = importlib.import_module("s-cgib_amd.synth")
OUT = os.path.join(ROOT, "tests", "golden")
NAME = "explain_eval_L5_k1"


def main(seed=21, workload="qm9", F=11, B=8, L=5, k=1, chunk=4):
    models = refshim.import_reference_models()
    import util as util_mod  # the reference's util.py (behind the same shim)
    torch.manual_seed(seed)
    mols = synth.molecules(B - 1, workload, seed=seed, mu=12.0, sigma=4.0, F=F)
    x2 = np.random.default_rng(seed).random((2, F), dtype=np.float32)
    mols.insert(B // 2, (np.array([[0, 1], [1, 0]], dtype=np.int64), x2))
    graphs, subgraphs = [], []
    for ei, x in mols:
        g = util_mod.load_dgl_fromPyG(SimpleNamespace(edge_index=torch.from_numpy(ei),
                                                      x=torch.from_numpy(x)))
        graphs.append(g)
        subgraphs.append([D.khop_in_subgraph(g, v, k=k)[0] for v in g.nodes()])
    batch_g = D.batch(graphs)
    ego_g = D.batch(list(chain.from_iterable(subgraphs)))
    batch_x = GG.F_normalize(batch_g.ndata["x"].float())
    x_subs = GG.F_normalize(ego_g.ndata["x"].float())
    args = SimpleNamespace(recons_type="adj", useAtt=1, readout_f="sum", d_transfer=32,
                           device="cpu", batch_size=chunk, task="graph_classification",
                           dataset="pre-train")
    model = models.Mainmodel(args, F, hidden_dim=64, num_layers=4, num_heads=4, k_transition=k,
                             encoder="GIN")
    GG._grow_gin(models, model.Encoder1, L)
    GG._grow_gin(models, model.Encoder2, L)
    model.train()
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if "batch_norms" in n_ or "compressor.1" in n_:
                p_.add_(0.1 * torch.randn_like(p_))

    def forward():
        return model.forward(batch_g, batch_x, ego_g, None, x_subs, 1, batch_g.edges(), 2, "cpu",
                             chunk)

    torch.manual_seed(seed + 1000)
    forward()  # train mode: moves every BatchNorm's running statistics
    model.eval()
    state = {kk: v.detach().clone() for kk, v in model.state_dict().items()}

    lam_ref, p_ref, logits = [], [], []
    real_compress = model.compress

    def compress(features, device):
        lam, p = real_compress(features, device)
        lam_ref.append(lam.detach().reshape(-1).clone())
        p_ref.append(p.detach().reshape(-1).clone())
        return lam, p

    model.compress = compress
    hook = model.attn_layer.register_forward_hook(
        lambda m, i, o: logits.append(o.detach().reshape(-1).clone()))
    torch.manual_seed(seed + 2000)
    with torch.no_grad(), GG._NoiseRecorder() as rec:
        forward()
    hook.remove()
    draws = rec.draws
    assert len(draws) == 2 * B and len(lam_ref) == len(logits) == B
    after = model.state_dict()
    assert all(torch.equal(state[kk], after[kk]) for kk in state)  # eval moved nothing

    out = {
        "B": np.array(B), "L": np.array(L), "k": np.array(k), "F": np.array(F),
        "chunk": np.array(chunk), "continue_wrapper": np.array(False),
        "batch_num_nodes": batch_g.batch_num_nodes().numpy(),
        "src": batch_g.src.numpy(), "dst": batch_g.dst.numpy(),
        "x_raw": batch_g.ndata["x"].numpy(),
        "ego_batch_num_nodes": ego_g.batch_num_nodes().numpy(),
        "ego_src": ego_g.src.numpy(), "ego_dst": ego_g.dst.numpy(),
        "u_gate": torch.cat([draws[2 * i].reshape(-1) for i in range(B)]).numpy(),
        "u_feat": torch.cat([draws[2 * i + 1] for i in range(B)]).numpy(),
        "lam_ref": torch.cat(lam_ref).numpy(), "p_ref": torch.cat(p_ref).numpy(),
        "attn_logit_ref": torch.cat(logits).numpy(),
        "alpha_ref": torch.cat([torch.softmax(l, dim=0) for l in logits]).numpy(),
    }
    gptr = np.concatenate([[0], np.cumsum(out["batch_num_nodes"])])
    node_graph = np.repeat(np.arange(B), out["batch_num_nodes"])
    ego_owner = np.repeat(np.arange(len(out["ego_batch_num_nodes"])), out["ego_batch_num_nodes"])
    out["ego_nodes_global"] = ego_g.ndata["_ID"].numpy() + gptr[node_graph[ego_owner]]
    used = ("transfer_d.", "Encoder1.", "Encoder2.", "compressor.", "attn_layer.")
    for kk, v in state.items():
        if kk.startswith(used):
            out["param_" + kk] = v.numpy()
    path = os.path.join(OUT, NAME + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {NAME}.npz  N={len(out['x_raw'])} bytes={os.path.getsize(path)} "
          f"lam in [{out['lam_ref'].min():.4f}, {out['lam_ref'].max():.4f}]")


if __name__ == "__main__":
    main()
