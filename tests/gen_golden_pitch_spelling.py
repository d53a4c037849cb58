#!/usr/bin/env python3
"""Golden vectors of the pitch-spelling models, produced by RUNNING THE REFERENCE'S OWN SOURCE on the CPU in float64, train mode,
dropout 0.  TEST INFRASTRUCTURE ONLY: runs where the reference tree is available, never on the GPU machine; only the arrays it
writes (tests/golden/pitch_spelling_*.npz) are committed — no reference program text travels.

Executed from the reference: the classes `PKSpell`, `HierarchicalHeteroGraphSage`, `PitchSpellingGNN` and
`PitchSpellingNeighborGNN`, cut out of models/pitch_spelling.py with `ast`.  `PKSpell` needs torch alone: its fixtures are the
reference pure.  The graph classes name torch_geometric and graphmuse, which are absent here; in their place stand the small modules
of tests/pitch_spelling_ref.py (`gnn.HeteroConv`, `gnn.SAGEConv`, `gnn.GraphNorm`, `trim_to_layer` over oracle/pyg_ref.py;
`MetricalGNN` delegating to oracle/encoders_ref.metrical_gnn), so those fixtures are the reference MODULO PyG / graphmuse semantics.

A fixture holds the inputs (float32 values, so the fp32 path reads exactly what the float64 run read), the `state_dict`, the two
outputs, the input and output of the normalisation between encoder and heads (GraphNorm / BatchNorm1d), the recorded cotangents
and the gradients of <out_pc, cot_pc> + <out_ks, cot_ks> with respect to the note inputs and every parameter that receives one
(float64).  Indices are int32 on disk; the weights are drawn as bf16 values.

The seed of a case is advanced (at most 80 times) until
  (a) no ReLU input lies within 3e-6 of the kink relative to its call's largest magnitude (F.relu and Tensor.relu are tapped),
  (b) every column of every BatchNorm input, and of every graph's share of the GraphNorm input, has a standard deviation of at least
      0.05 x that call's largest,
  (c) the reference itself, re-run in fp32 on the same weights, agrees with its float64 run within a quarter of the tests' gate
      (1e-4 x max-abs) on every compared tensor.
The margins are recorded under meta.*.   Usage: python tests/gen_golden_pitch_spelling.py"""
from __future__ import annotations

import ast
import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.gen_golden_r3 import REF_CHORD  # noqa: E402
from oracle.testing import GOLDEN_DIR, ReluTap  # noqa: E402
from analysisgnn_amd.synth import make_score_graph, merge_sampled, sample_hops  # noqa: E402
import pitch_spelling_ref as PR  # noqa: E402

REF_PS = os.path.join(os.path.dirname(REF_CHORD), "pitch_spelling.py")
CLASSES = ["PKSpell", "HierarchicalHeteroGraphSage", "PitchSpellingGNN", "PitchSpellingNeighborGNN"]
GATE = 1e-4
IN_FEATS = 8


def reference_namespace() -> dict:
    gnn = types.SimpleNamespace(HeteroConv=PR.HeteroConv, SAGEConv=PR.SAGEConv, GraphNorm=PR.GraphNormModule)
    ns = {"torch": torch, "nn": nn, "np": np, "gnn": gnn, "trim_to_layer": PR.trim_to_layer, "MetricalGNN": PR.MetricalGNNModule}
    tree = ast.parse(open(REF_PS).read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
    assert sorted(n.name for n in nodes) == sorted(CLASSES), [n.name for n in nodes]
    exec(compile(ast.Module(body=nodes, type_ignores=[]), REF_PS, "exec"), ns)
    return ns


class TensorReluTap:
    """oracle.testing.ReluTap sees F.relu (nn.ReLU ends there); the reference's SAGE stack calls `x.relu()`: the same record."""

    def __init__(self, tap: ReluTap):
        self.tap = tap

    def __enter__(self):
        self._orig = torch.Tensor.relu
        tap, orig = self.tap, self._orig

        def relu(x):
            tap.inputs.append(x.detach())
            return orig(x)
        torch.Tensor.relu = relu
        return self

    def __exit__(self, *exc):
        torch.Tensor.relu = self._orig
        return False


def draw_weights(model, seed):
    """Every vector (biases, norm scales and shifts, GraphNorm's mean_scale) moves by 0.1 * randn, away from the initial values at
    which whole terms vanish; then bf16 values held in fp32."""
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=gen) * 0.1)
            p.copy_(p.bfloat16().float())


def graph_inputs(cfg, seed):
    samples = [sample_hops(make_score_graph(seed=cfg["graph_seed"] + i, n_notes=n), t, [3], seed=seed + i)
               for i, (n, t) in enumerate(zip(cfg["n_notes"], cfg["n_targets"]))]
    g = merge_sampled(samples)
    ets = list(g.edge_index.keys())
    gen = torch.Generator().manual_seed(seed + 2)
    I = dict(x_dict={"note": torch.randn(g.num_nodes["note"], IN_FEATS, generator=gen, dtype=torch.float32)},
             ei_dict={et: torch.from_numpy(np.ascontiguousarray(g.edge_index[et])) for et in ets},
             nodes_per_hop={"note": list(g.num_sampled_nodes["note"])}, edges_per_hop={et: list(g.num_sampled_edges[et]) for et in ets},
             batch=torch.from_numpy(g.batch["note"][:g.batch_size].copy()))
    hop = lambda counts: torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))                  # noqa: E731
    I["mask_node"] = {"note": hop(I["nodes_per_hop"]["note"])}
    I["mask_edge"] = {et: hop(I["edges_per_hop"][et]) for et in ets}
    return I, (["note"], ets)


class NormTap:
    """Input and output of the model's `normalize`, and the smallest column standard deviation of its input relative to the
    largest: over all rows for BatchNorm1d, within every graph for GraphNorm."""

    def __init__(self, model, batch):
        self.rec, self.ratio, self.batch = {}, 1.0, batch
        self.handle = model.normalize.register_forward_hook(self._hook)

    def _hook(self, mod, args, out):
        h = args[0].detach()
        self.rec = {"mid.norm_in": h, "mid.norm_out": out.detach()}
        groups = [h] if isinstance(mod, nn.BatchNorm1d) else [h[self.batch == g] for g in range(int(self.batch.max()) + 1)]
        sd = torch.stack([g.std(dim=0, unbiased=False) for g in groups])
        self.ratio = float(sd.min() / sd.max())

    def close(self):
        self.handle.remove()


def call(model, cfg, I, x):
    if cfg["kind"] == "pkspell":
        return model(x, I["lens"])
    xd = {"note": x}
    if cfg["kind"] == "psgnn":
        return model(xd, I["ei_dict"], I["mask_node"], I["mask_edge"], I["batch"])
    return model(xd, I["ei_dict"], I["edges_per_hop"], I["nodes_per_hop"])


def run_model(model, cfg, I, dtype, cot=None):
    tap = NormTap(model, I.get("batch")) if cfg["kind"] != "pkspell" else None
    x = (I["x"] if cfg["kind"] == "pkspell" else I["x_dict"]["note"]).to(dtype).clone().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        out_pc, out_ks = call(model, cfg, I, x)
    finally:
        torch.set_default_dtype(old)
    if cot is None:
        gen = torch.Generator().manual_seed(12345)
        cot = [torch.randn(v.shape, generator=gen, dtype=torch.float32).double() for v in (out_pc, out_ks)]
    ((out_pc * cot[0].to(dtype)).sum() + (out_ks * cot[1].to(dtype)).sum()).backward()
    rec = {"out.pc": out_pc.detach(), "out.ks": out_ks.detach(), "grad.x": x.grad.detach()}
    ratio = 1.0
    if tap is not None:
        tap.close()
        rec.update(tap.rec)
        ratio = tap.ratio
    for k, p in model.named_parameters():
        if p.grad is not None:
            rec["gw." + k] = p.grad.detach()
    return rec, cot, ratio


def run_case(ns, cfg, seed):
    torch.manual_seed(seed)
    if cfg["kind"] == "pkspell":
        gen = torch.Generator().manual_seed(seed + 2)
        I = dict(x=torch.randn(sum(cfg["lens"]), IN_FEATS, generator=gen, dtype=torch.float32), lens=list(cfg["lens"]))
        model = ns["PKSpell"](IN_FEATS, cfg["h1"], cfg["h2"], PR.OUT_PC, rnn_depth=1, dropout=0.0, cell_type=cfg["cell"])
        metadata = None
    else:
        I, metadata = graph_inputs(cfg, seed)
        if cfg["kind"] == "psgnn":
            model = ns["PitchSpellingGNN"](IN_FEATS, cfg["H"], PR.ENC, PR.OUT_PC, PR.OUT_KS, cfg["L"], metadata, dropout=0.0, add_seq=cfg["add_seq"])
        else:
            model = ns["PitchSpellingNeighborGNN"](IN_FEATS, cfg["H"], PR.ENC, PR.OUT_PC, PR.OUT_KS, cfg["L"], metadata, dropout=0.0)
    draw_weights(model, seed)
    model.train()
    m32 = copy.deepcopy(model)
    model.double()
    with ReluTap() as tap, TensorReluTap(tap):
        rec, cot, ratio = run_model(model, cfg, I, torch.float64)
    rec32, _, _ = run_model(m32, cfg, I, torch.float32, cot)
    # A gradient that is zero in exact arithmetic (lin_l of a layer that keeps no edge) has max-abs 0 or rounding noise: such tensors
    # (below 1e-9 of the largest weight gradient) are listed in meta.zero_grads and held against 1e-4 x the LARGEST weight gradient's
    # max-abs, as in tests/gen_golden_chord.py.
    gmax = max(float(v.abs().max()) for k, v in rec.items() if k.startswith("gw.") and v.numel())
    zero_grads = sorted(k for k, v in rec.items() if k.startswith("gw.") and v.numel() and float(v.abs().max()) < 1e-9 * gmax)
    worst = max(float((v.double() - rec32[k].double()).abs().max()) / (GATE * (gmax if k in zero_grads else float(v.abs().max())))
                for k, v in rec.items() if v.numel())
    no_grad = sorted(k for k, p in model.named_parameters() if p.grad is None)
    out = {"meta.kind": np.array(cfg["kind"]), "meta.seed": np.array(seed), "meta.keys": np.array(list(model.state_dict().keys())),
           "meta.no_grad": np.array(no_grad, dtype="U96"), "meta.zero_grads": np.array(zero_grads, dtype="U96"),
           "meta.grad_max": np.array(gmax), "meta.relu_margin": np.array(tap.margin() if tap.inputs else 1.0),
           "meta.norm_min_ratio": np.array(ratio), "meta.fp32_over_gate": np.array(worst),
           "cot.pc": cot[0].numpy().astype(np.float32), "cot.ks": cot[1].numpy().astype(np.float32)}
    if cfg["kind"] == "pkspell":
        out.update({"meta.cfg": np.array([IN_FEATS, cfg["h1"], cfg["h2"], 1], dtype=np.int64), "meta.cell": np.array(cfg["cell"]),
                    "in.x": I["x"].numpy(), "in.lens": np.array(I["lens"], dtype=np.int32)})
    else:
        ets = metadata[1]
        out.update({"meta.cfg": np.array([IN_FEATS, cfg["H"], cfg["L"], int(cfg.get("add_seq", False))], dtype=np.int64),
                    "meta.node_types": np.array(metadata[0]), "meta.edge_types": np.array([list(et) for et in ets]),
                    "in.x.note": I["x_dict"]["note"].numpy()})
        for et in ets:
            key = "__".join(et)
            out["in.ei." + key] = I["ei_dict"][et].numpy().astype(np.int32)
            if cfg["kind"] == "psgnn":
                out["in.mask_edge." + key] = I["mask_edge"][et].numpy().astype(np.int32)
            else:
                out["in.edges_per_hop." + key] = np.array(I["edges_per_hop"][et], dtype=np.int32)
        if cfg["kind"] == "psgnn":
            out["in.mask_node.note"] = I["mask_node"]["note"].numpy().astype(np.int32)
            out["in.batch"] = I["batch"].numpy().astype(np.int32)
        else:
            out["in.nodes_per_hop.note"] = np.array(I["nodes_per_hop"]["note"], dtype=np.int32)
    for k, v in model.state_dict().items():
        a = v.detach().numpy()
        if a.dtype == np.float64 and "running_" not in k:
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a), k       # the weights are fp32 values
            a = a.astype(np.float32)
        out["w." + k] = a
    out.update({k: v.numpy() for k, v in rec.items()})
    return out, (tap.at_risk(3e-6) if tap.inputs else 0), ratio, worst


GNN = dict(n_notes=(40, 25), n_targets=(24, 15), H=32, L=2, graph_seed=91)
CASES = {
    "pkspell_h16": dict(kind="pkspell", h1=16, h2=8, lens=(11, 7, 1), cell="GRU"),
    "pkspell_lstm": dict(kind="pkspell", h1=16, h2=8, lens=(11, 7, 1), cell="LSTM"),
    "psgnn_h32": dict(GNN, kind="psgnn", add_seq=False),
    "psgnn_seq_h32": dict(GNN, kind="psgnn", add_seq=True),
    "psneighbor_h32": dict(GNN, kind="psneighbor"),
}


def make_case(ns, name, cfg, seed):
    for attempt in range(80):
        s = seed + 1000 * attempt
        rec, risk, ratio, worst = run_case(ns, cfg, s)
        ok = risk == 0 and ratio >= 0.05 and worst <= 0.25
        print(f"  {name}: seed {s}: {risk} ReLU inputs at the kink, normalisation column ratio {ratio:.3f}, fp32 / gate {worst:.3f}"
              + ("" if ok else ": re-drawing"))
        if ok:
            break
    assert ok, f"{name}: no seed met the conditions"
    path = os.path.join(GOLDEN_DIR, "pitch_spelling_" + name + ".npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 2 ** 20
    print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path) / 1024:.1f} KiB), {len(rec['meta.keys'])} state_dict keys, "
          f"{len(rec['meta.no_grad'])} parameters without a gradient: {list(rec['meta.no_grad'])}")


def main():
    torch.set_num_threads(4)
    ns = reference_namespace()
    for i, (name, cfg) in enumerate(CASES.items()):
        make_case(ns, name, cfg, 501 + i)


if __name__ == "__main__":
    main()
