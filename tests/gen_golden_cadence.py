#!/usr/bin/env python3
"""Golden vectors of the cadence models, produced by RUNNING THE REFERENCE'S OWN SOURCE on the CPU in float64, dropout 0.  TEST
INFRASTRUCTURE ONLY: runs where the reference tree is available, never on the GPU machine; only the arrays it writes
(tests/golden/cadence_*.npz) are committed — no reference program text travels.

Executed from the reference: the classes `GNN`, `HierarchicalHeteroGraphSage`, `CadenceGNNNeighbor` and `CadenceGNNPytorch`, cut out
of models/cadence.py with `ast`.  They name torch_geometric, torch_scatter and graphmuse, which are absent here; in their place stand
the modules of tests/pitch_spelling_ref.py (`HeteroConv`, `SAGEConv` — given PyG's forward here, the homogeneous `GNN` calls it —,
`trim_to_layer`, `MetricalGNN` delegating to oracle/encoders_ref.metrical_gnn) and oracle/scatter_ref.py for `torch_scatter`, so the
fixtures are the reference MODULO PyG / graphmuse / torch_scatter semantics.

The reference's `CadenceGNNPytorch.encode` reads `self.use_pitch_spelling`, which its constructor sets only when the argument is
True: for the cases with `use_pitch_spelling=False` the attribute is set on the instance here (recorded in meta.set_attr).

A fixture holds the inputs (float32 values), the `state_dict`, `encode`'s output, the logits of `clf` on it, the tensors on both
sides of the join (mid.join_in: what scatter_mean receives as `out`; mid.pooled: its result; mid.join_out: after `norm`), the
recorded cotangents and the gradients of <enc, cot_enc> + <logits, cot_logits> with respect to the note inputs and every parameter
that receives one (float64).  Indices are int32 on disk; the weights are drawn as bf16 values.  Five cases run in train mode; one
runs in eval mode on drawn running statistics.

The seed of a case is advanced (at most 80 times) until
  (a) no ReLU input lies within 3e-6 of the kink relative to its call's largest magnitude (F.relu and Tensor.relu are tapped),
  (b) every column of the BatchNorm input has a standard deviation of at least 0.05 x the largest (train mode),
  (c) the reference itself, re-run in fp32 on the same weights, agrees with its float64 run within a quarter of the tests' gate
      (1e-4 x max-abs) on every compared tensor.
The margins are recorded under meta.*.   Usage: python tests/gen_golden_cadence.py"""
from __future__ import annotations

import ast
import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import pyg_ref, scatter_ref  # noqa: E402
from oracle.gen_golden_r3 import REF_CHORD  # noqa: E402
from oracle.testing import GOLDEN_DIR, ReluTap  # noqa: E402
import pitch_spelling_ref as PR  # noqa: E402
import cadence_ref as CR  # noqa: E402
from gen_golden_pitch_spelling import TensorReluTap, draw_weights, graph_inputs  # noqa: E402

REF_CAD = os.path.join(os.path.dirname(REF_CHORD), "cadence.py")
CLASSES = ["GNN", "HierarchicalHeteroGraphSage", "CadenceGNNNeighbor", "CadenceGNNPytorch"]
GATE = 1e-4
IN_FEATS = 8


class SAGEConvFwd(PR.SAGEConv):
    """PyG's SAGEConv forward on one node set: lin_l(mean of the in-neighbours) + lin_r(x)."""

    def forward(self, x, edge_index):
        return pyg_ref.sage_conv(dict(self.named_parameters()), "", x, x, edge_index)


def metrical_gnn(*args, fast=False, **kw):
    return PR.MetricalGNNModule(*args, **kw)


class ScatterTap:
    """torch_scatter for the reference: scatter_mean of oracle/scatter_ref.py, which also keeps what it was given as `out`."""

    def __init__(self):
        self.rec = {}

    def scatter_mean(self, src, index, dim=0, out=None, dim_size=None):
        self.rec["mid.join_in"] = out.detach().clone()
        res = scatter_ref.scatter_mean(src, index, dim=dim, out=out, dim_size=dim_size)
        self.rec["mid.pooled"] = res.detach().clone()
        return res


def reference_namespace(tap: ScatterTap) -> dict:
    ns = {"torch": torch, "nn": nn, "F": F, "np": np, "torch_scatter": tap, "SAGEConv": SAGEConvFwd, "HeteroConv": PR.HeteroConv,
          "trim_to_layer": PR.trim_to_layer, "MetricalGNN": metrical_gnn}
    tree = ast.parse(open(REF_CAD).read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
    assert sorted(n.name for n in nodes) == sorted(CLASSES), [n.name for n in nodes]
    exec(compile(ast.Module(body=nodes, type_ignores=[]), REF_CAD, "exec"), ns)
    return ns


def call(model, cfg, I, x):
    """(encode's output, the logits)."""
    if cfg["kind"] == "gnn":
        return model(x, I["ei"]), None
    xd = {"note": x}
    if cfg["kind"] == "pytorch":
        enc = model.encode(xd, I["ei_dict"], I["batch_size"], I["mask_node"], I["mask_edge"], {"note": I["batch"]}, I["ps"])
    else:
        enc = model.encode(xd, I["ei_dict"], I["edges_per_hop"], I["nodes_per_hop"])
    return enc, model.clf(enc)


def run_model(model, cfg, I, dtype, tap: ScatterTap, cot=None):
    rec_mid, ratio = {}, [1.0]
    hooks = []
    if cfg["kind"] != "gnn":
        hooks.append(model.norm.register_forward_hook(lambda m, a, o: rec_mid.__setitem__("mid.join_out", o.detach())))

        def bn_hook(mod, args, out):
            sd = args[0].detach().std(dim=0, unbiased=False)
            ratio[0] = float(sd.min() / sd.max())
        hooks.append(model.cad_clf[2].register_forward_hook(bn_hook))
    x = (I["x"] if cfg["kind"] == "gnn" else I["x_dict"]["note"]).to(dtype).clone().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    tap.rec = {}
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        enc, logits = call(model, cfg, I, x)
    finally:
        torch.set_default_dtype(old)
    for h in hooks:
        h.remove()
    if cot is None:
        gen = torch.Generator().manual_seed(12345)
        cot = [torch.randn(v.shape, generator=gen, dtype=torch.float32).double() if v is not None else None for v in (enc, logits)]
    loss = (enc * cot[0].to(dtype)).sum()
    if logits is not None:
        loss = loss + (logits * cot[1].to(dtype)).sum()
    loss.backward()
    rec = {"out.enc": enc.detach(), "grad.x": x.grad.detach()}
    if logits is not None:
        rec["out.logits"] = logits.detach()
    rec.update(tap.rec)
    rec.update(rec_mid)
    for k, p in model.named_parameters():
        if p.grad is not None:
            rec["gw." + k] = p.grad.detach()
    return rec, cot, ratio[0]


def run_case(ns, tap, cfg, seed):
    torch.manual_seed(seed)
    I, metadata = graph_inputs(cfg, seed)
    gen = torch.Generator().manual_seed(seed + 3)
    n_note = I["x_dict"]["note"].shape[0]
    set_attr = []
    if cfg["kind"] == "gnn":
        I = dict(x=I["x_dict"]["note"], ei=torch.cat([I["ei_dict"][et] for et in metadata[1]], dim=1))
        model = ns["GNN"](IN_FEATS, cfg["H"], cfg["L"], dropout=0.0)
    elif cfg["kind"] == "neighbor":
        model = ns["CadenceGNNNeighbor"](metadata, IN_FEATS, cfg["H"], CR.OUT, cfg["L"], dropout=0.0)
    else:
        from analysisgnn_amd.synth import make_score_graph, merge_sampled, sample_hops
        g = merge_sampled([sample_hops(make_score_graph(seed=cfg["graph_seed"] + i, n_notes=n), t, [3], seed=seed + i)
                           for i, (n, t) in enumerate(zip(cfg["n_notes"], cfg["n_targets"]))])
        I["batch"] = torch.from_numpy(g.batch["note"].copy())            # every note's graph id: encode indexes it by node
        I["batch_size"] = int(g.batch_size)
        I["ps"] = torch.randint(0, 38, (n_note,), generator=gen)
        model = ns["CadenceGNNPytorch"](metadata, IN_FEATS, cfg["H"], CR.OUT, cfg["L"], dropout=0.0, hybrid=cfg["hybrid"],
                                        use_pitch_spelling=cfg["use_ps"])
        if not cfg["use_ps"]:
            model.use_pitch_spelling = False
            set_attr.append("use_pitch_spelling")
    draw_weights(model, seed)
    training = cfg.get("training", True)
    if training:
        model.train()
    else:
        model.eval()
        with torch.no_grad():
            bn = model.cad_clf[2]
            bn.running_mean.copy_((torch.randn(bn.running_mean.shape, generator=gen) * 0.2).bfloat16().float())
            bn.running_var.copy_((0.5 + torch.rand(bn.running_var.shape, generator=gen)).bfloat16().float())
    m32 = copy.deepcopy(model)
    model.double()
    with ReluTap() as rtap, TensorReluTap(rtap):
        rec, cot, ratio = run_model(model, cfg, I, torch.float64, tap)
    rec32, _, _ = run_model(m32, cfg, I, torch.float32, tap, cot)
    gws = [float(v.abs().max()) for k, v in rec.items() if k.startswith("gw.") and v.numel()]
    gmax = max(gws)
    zero_grads = sorted(k for k, v in rec.items() if k.startswith("gw.") and v.numel() and float(v.abs().max()) < 1e-9 * gmax)
    worst = max(float((v.double() - rec32[k].double()).abs().max()) / (GATE * (gmax if k in zero_grads else float(v.abs().max())))
                for k, v in rec.items() if v.numel())
    no_grad = sorted(k for k, p in model.named_parameters() if p.grad is None)
    out = {"meta.kind": np.array(cfg["kind"]), "meta.seed": np.array(seed), "meta.keys": np.array(list(model.state_dict().keys())),
           "meta.no_grad": np.array(no_grad, dtype="U96"), "meta.zero_grads": np.array(zero_grads, dtype="U96"),
           "meta.set_attr": np.array(set_attr, dtype="U32"), "meta.grad_max": np.array(gmax),
           "meta.relu_margin": np.array(rtap.margin() if rtap.inputs else 1.0), "meta.norm_min_ratio": np.array(ratio),
           "meta.fp32_over_gate": np.array(worst),
           "meta.cfg": np.array([IN_FEATS, cfg["H"], cfg["L"], int(cfg.get("hybrid", False)), int(cfg.get("use_ps", False)), int(training)],
                                dtype=np.int64),
           "cot.enc": cot[0].numpy().astype(np.float32)}
    if cot[1] is not None:
        out["cot.logits"] = cot[1].numpy().astype(np.float32)
    if cfg["kind"] == "gnn":
        out.update({"in.x.note": I["x"].numpy(), "in.ei": I["ei"].numpy().astype(np.int32)})
    else:
        ets = metadata[1]
        out.update({"meta.node_types": np.array(metadata[0]), "meta.edge_types": np.array([list(et) for et in ets]),
                    "in.x.note": I["x_dict"]["note"].numpy()})
        for et in ets:
            key = "__".join(et)
            out["in.ei." + key] = I["ei_dict"][et].numpy().astype(np.int32)
            if cfg["kind"] == "pytorch":
                out["in.mask_edge." + key] = I["mask_edge"][et].numpy().astype(np.int32)
            else:
                out["in.edges_per_hop." + key] = np.array(I["edges_per_hop"][et], dtype=np.int32)
        if cfg["kind"] == "pytorch":
            out["in.mask_node.note"] = I["mask_node"]["note"].numpy().astype(np.int32)
            out["in.batch"] = I["batch"].numpy().astype(np.int32)
            out["in.batch_size"] = np.array(I["batch_size"], dtype=np.int64)
            out["in.ps"] = I["ps"].numpy().astype(np.int32)
        else:
            out["in.nodes_per_hop.note"] = np.array(I["nodes_per_hop"]["note"], dtype=np.int32)
    for k, v in model.state_dict().items():
        a = v.detach().numpy()
        if a.dtype == np.float64:
            exact = np.array_equal(a.astype(np.float32).astype(np.float64), a)
            assert exact or (training and "running_" in k), k       # the weights (and the drawn running statistics) are fp32 values
            a = a.astype(np.float32) if exact else a
        out["w." + k] = a
    out.update({k: v.numpy() for k, v in rec.items()})
    return out, (rtap.at_risk(3e-6) if rtap.inputs else 0), (ratio if training else 1.0), worst


G = dict(n_notes=(40, 25), n_targets=(24, 15), H=32, L=2, graph_seed=91)
CASES = {
    "gnn_h16": dict(G, kind="gnn", H=16, L=3),
    "neighbor_h32": dict(G, kind="neighbor"),
    "pytorch_h32": dict(G, kind="pytorch", hybrid=False, use_ps=False),
    "pytorch_ps_h32": dict(G, kind="pytorch", hybrid=False, use_ps=True),
    "pytorch_hybrid_h32": dict(G, kind="pytorch", hybrid=True, use_ps=False),
    "pytorch_eval_h32": dict(G, kind="pytorch", hybrid=False, use_ps=True, training=False),
}
assert list(CASES) == CR.CASES


def make_case(ns, tap, name, cfg, seed):
    for attempt in range(80):
        s = seed + 1000 * attempt
        rec, risk, ratio, worst = run_case(ns, tap, cfg, s)
        ok = risk == 0 and ratio >= 0.05 and worst <= 0.25
        print(f"  {name}: seed {s}: {risk} ReLU inputs at the kink, BatchNorm column ratio {ratio:.3f}, fp32 / gate {worst:.3f}"
              + ("" if ok else ": re-drawing"))
        if ok:
            break
    assert ok, f"{name}: no seed met the conditions"
    path = os.path.join(GOLDEN_DIR, "cadence_" + name + ".npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 2 ** 20
    print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path) / 1024:.1f} KiB), {len(rec['meta.keys'])} state_dict keys, "
          f"{len(rec['meta.no_grad'])} parameters without a gradient: {list(rec['meta.no_grad'])}")


def main():
    torch.set_num_threads(4)
    tap = ScatterTap()
    ns = reference_namespace(tap)
    for i, (name, cfg) in enumerate(CASES.items()):
        make_case(ns, tap, name, cfg, 701 + i)


if __name__ == "__main__":
    main()
