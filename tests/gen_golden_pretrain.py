#!/usr/bin/env python3
"""Golden vectors of the pretraining stage, produced by RUNNING THE REFERENCE'S OWN SOURCE on the CPU in float64.
TEST INFRASTRUCTURE ONLY: runs where the reference tree is available, never on the GPU machine; only the arrays it writes
(tests/golden/pretrain_*.npz, a few KB each) are committed — no reference program text travels.

Executed from the reference file, cut out with `ast` as oracle/gen_golden_r3.load_reference_classes does for classes: the class
`PreEncoder` (models/analysis.py:360-406: the four heads, the link logits, `forward`) and the function `isin_pairwise` (:23-41).
The name `HybridHGT` is bound to a small seeded stand-in encoder (graphmuse exists nowhere offline; the encoder itself is pinned
elsewhere): Linear + tanh on the first `batch_size` note rows.  `PreEncoderPL._common_step` sits in a LightningModule that
cannot be imported; its lines :704-731 are followed here statement by statement around those two pieces, with torch's
`BCEWithLogitsLoss` and `CrossEntropyLoss(label_smoothing=0.1)` as :684-687 builds them.

The seed of a case is advanced until (a) no ReLU input lies within 3e-6 of the kink relative to its call's largest magnitude and
(b) no link logit lies within 1e-4 of zero (the confusion counts of the fp32 path are compared exactly).
Usage: python tests/gen_golden_pretrain.py"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.gen_golden_r3 import REF_ANALYSIS, load_reference_classes  # noqa: E402
from oracle.testing import GOLDEN_DIR, ReluTap  # noqa: E402
from analysisgnn_amd.synth import add_staff_voice, make_score_graph  # noqa: E402

ONSET, CONSECUTIVE = ("note", "onset", "note"), ("note", "consecutive", "note")
STAFF, VOICE = ("note", "staff", "note"), ("note", "voice", "note")


def load_reference_functions(path: str, names, namespace: dict) -> dict:
    """Execute the top-level FunctionDef nodes `names` of the file at `path` inside `namespace`."""
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(nodes) == len(names), f"{path}: {set(names) - {n.name for n in nodes}} not found"
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), namespace)
    return namespace


class StandInEncoder(nn.Module):
    """In the slot of graphmuse's HybridHGT: the reference's constructor keywords, its forward arguments."""

    def __init__(self, metadata, in_channels, out_channels, num_layers, heads=4, dropout=0.5, jk=True):
        super().__init__()
        self.lin = nn.Linear(in_channels, out_channels)

    def forward(self, x_dict, edge_index_dict, batch_dict, batch_size, neighbor_mask_node, neighbor_mask_edge):
        return torch.tanh(self.lin(x_dict["note"][:batch_size]))


def reference_namespace() -> dict:
    ns = {"torch": torch, "nn": nn, "HybridHGT": StandInEncoder}
    load_reference_classes(REF_ANALYSIS, ["PreEncoder"], ns)
    load_reference_functions(REF_ANALYSIS, ["isin_pairwise"], ns)
    return ns


def run_case(ns, n_notes, batch_size, H, in_ch, graph_seed, seed):
    g = add_staff_voice(make_score_graph(seed=graph_seed, n_notes=n_notes), seed=graph_seed + 1)
    torch.manual_seed(seed)
    model = ns["PreEncoder"](g.metadata(), in_ch, H, 2, heads=2, dropout=0.0)
    with torch.no_grad():                                 # biases / LayerNorm shifts away from their initialisation
        gen = torch.Generator().manual_seed(seed + 1)
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=gen) * 0.1)
    model.double().train()
    gen = torch.Generator().manual_seed(seed + 2)
    x_dict = {"note": torch.randn(n_notes, in_ch, generator=gen, dtype=torch.float64)}
    key_signature = torch.randint(0, 15, (n_notes,), generator=gen)
    pitch_spelling = torch.randint(0, 35, (n_notes,), generator=gen)
    edge_index_dict = {et: torch.from_numpy(e.copy()) for et, e in g.edge_index.items()}
    kept = {et: e.clone() for et, e in edge_index_dict.items()}
    isin_pairwise = ns["isin_pairwise"]
    # ---- :704-731
    staff_candidate_edges = torch.cat((edge_index_dict[ONSET], edge_index_dict[CONSECUTIVE]), dim=1)
    staff_candidate_edges = staff_candidate_edges[:, staff_candidate_edges[0].argsort()]
    voice_candidate_edges = edge_index_dict[CONSECUTIVE]
    staff_true_edges = edge_index_dict.pop(STAFF)
    voice_true_edges = edge_index_dict.pop(VOICE)
    staff_candidate_edges = staff_candidate_edges[:, torch.logical_and(staff_candidate_edges[0] < batch_size, staff_candidate_edges[1] < batch_size)]
    voice_candidate_edges = voice_candidate_edges[:, torch.logical_and(voice_candidate_edges[0] < batch_size, voice_candidate_edges[1] < batch_size)]
    staff_true_edges = staff_true_edges[:, torch.logical_and(staff_true_edges[0] < batch_size, staff_true_edges[1] < batch_size)]
    voice_true_edges = voice_true_edges[:, torch.logical_and(voice_true_edges[0] < batch_size, voice_true_edges[1] < batch_size)]
    staff_labels = isin_pairwise(staff_candidate_edges, staff_true_edges, assume_unique=True)
    voice_labels = isin_pairwise(voice_candidate_edges, voice_true_edges, assume_unique=True)
    fifths_labels = key_signature[:batch_size]
    spelling_labels = pitch_spelling[:batch_size]
    with ReluTap() as tap:
        staff_logits, voice_logits, fifths_logits, spelling_logits, x = model(
            x_dict, edge_index_dict, None, batch_size, None, None, staff_candidate_edges, voice_candidate_edges, return_embedding=True)
    x.retain_grad()
    staff_loss = nn.BCEWithLogitsLoss()(staff_logits.squeeze(), staff_labels.squeeze().float().double())
    voice_loss = nn.BCEWithLogitsLoss()(voice_logits.squeeze(), voice_labels.squeeze().float().double())
    fifths_loss = nn.CrossEntropyLoss(label_smoothing=0.1)(fifths_logits, fifths_labels)
    spelling_loss = nn.CrossEntropyLoss(label_smoothing=0.1)(spelling_logits, spelling_labels)
    total_loss = staff_loss + voice_loss + fifths_loss + spelling_loss
    # ----
    total_loss.backward()
    zero_margin = min(float(staff_logits.detach().abs().min()), float(voice_logits.detach().abs().min()))
    rec = {"meta.cfg": np.array([n_notes, batch_size, H, in_ch, graph_seed, seed], dtype=np.int64),
           "meta.keys": np.array(sorted(model.state_dict().keys())),
           "meta.relu_margin": np.array(tap.margin()), "meta.zero_margin": np.array(zero_margin),
           "in.x": x.detach().numpy(), "in.key_signature": key_signature.numpy().astype(np.int32),
           "in.pitch_spelling": pitch_spelling.numpy().astype(np.int32),
           "out.staff_candidates": staff_candidate_edges.numpy().astype(np.int32),
           "out.voice_candidates": voice_candidate_edges.numpy().astype(np.int32),
           "out.staff_logits": staff_logits.detach().numpy(), "out.voice_logits": voice_logits.detach().numpy(),
           "out.staff_labels": staff_labels.numpy(), "out.voice_labels": voice_labels.numpy(),
           "out.fifths_logits": fifths_logits.detach().numpy(), "out.spelling_logits": spelling_logits.detach().numpy(),
           "loss.parts": np.array([staff_loss.item(), voice_loss.item(), fifths_loss.item(), spelling_loss.item()]),
           "loss.total": np.array(total_loss.item()), "grad.x": x.grad.numpy()}
    for et in (ONSET, CONSECUTIVE, STAFF, VOICE):         # what the step reads (int32 on disk: the fixtures stay small)
        rec["edges." + et[1]] = kept[et].numpy().astype(np.int32)
    for k, v in model.state_dict().items():
        if not k.startswith("encoder."):
            rec["w." + k] = v.detach().numpy()
    for k, p in model.named_parameters():
        if not k.startswith("encoder."):
            rec["gw." + k] = p.grad.numpy()
    assert len(staff_labels) and len(voice_labels) and bool(staff_labels.any()) and bool(voice_labels.any()) and not bool(staff_labels.all())
    return rec, tap.at_risk(3e-6), zero_margin


def make_case(ns, name, n_notes, batch_size, H, in_ch, graph_seed, seed):
    for attempt in range(80):
        rec, risk, zero_margin = run_case(ns, n_notes, batch_size, H, in_ch, graph_seed, seed + 1000 * attempt)
        if risk == 0 and zero_margin > 1e-4:
            break
        print(f"  {name}: seed {seed + 1000 * attempt}: {risk} ReLU inputs at the kink, smallest |logit| {zero_margin:.1e}: re-drawing")
    assert risk == 0 and zero_margin > 1e-4, "no alive candidate may lie within 1e-4 of zero"
    path = os.path.join(GOLDEN_DIR, name + ".npz")
    np.savez_compressed(path, **rec)
    print(f"  wrote {name}.npz ({os.path.getsize(path) / 1024:.1f} KiB)  seed {int(rec['meta.cfg'][5])}  total {float(rec['loss.total']):.6f}  "
          f"ReLU margin {float(rec['meta.relu_margin']):.1e}  smallest |logit| {zero_margin:.1e}")


def main():
    torch.set_num_threads(4)
    ns = reference_namespace()
    make_case(ns, "pretrain_h8_whole", 48, 48, 8, 12, 71, 201)          # every note a target
    make_case(ns, "pretrain_h16_targets", 64, 40, 16, 12, 72, 202)      # candidates and true edges that leave the batch


if __name__ == "__main__":
    main()
