#!/usr/bin/env python3
"""Golden vectors of the chord family's post-processing model, produced by RUNNING THE REFERENCE'S OWN SOURCE on the CPU in
float64, train mode, dropout 0.  TEST INFRASTRUCTURE ONLY: runs where the reference tree is available, never on the GPU machine;
only the arrays it writes (tests/golden/postprocess_*.npz) are committed — no reference program text travels.

Executed from the reference: the class `PostProcessingMLTModel`, cut out of models/chord.py with `ast` (as
tests/gen_golden_chord.py cuts its classes), in a namespace of torch, nn and F.

A fixture holds the per-task input logits (float32 values, so the fp32 path reads exactly what the float64 run read), the
`state_dict` (weights drawn by the module's own initialisation, rounded to bf16 values), the output logits per task, the
cotangents, and the gradients of sum_t <out_t, cot_t> with respect to every input and every parameter (float64).

The seed of a case is advanced (at most 40 times) until no ReLU input lies within 3e-6 of the kink relative to its call's largest
magnitude (oracle.testing.ReluTap) and the reference itself, re-run in fp32 on the same weights, agrees with its float64 run
within a quarter of the tests' gate (1e-4 x max(1, max-abs)) on every compared tensor.  Usage: python tests/gen_golden_postprocess.py"""
from __future__ import annotations

import ast
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.gen_golden_r3 import REF_CHORD  # noqa: E402
from oracle.testing import GOLDEN_DIR, ReluTap  # noqa: E402

GATE = 1e-4
TASKS = {"localkey": 38, "degree1": 22, "quality": 11, "inversion": 4}
# shape: of every task's logits without the class axis
CASES = {
    "postprocess_h16_batch": dict(n_hidden=16, n_layers=1, shape=(3, 7)),
    "postprocess_h16_2d": dict(n_hidden=16, n_layers=1, shape=(11,)),          # the unsqueeze / squeeze route
    "postprocess_h16_one": dict(n_hidden=16, n_layers=1, shape=(1, 9)),        # a batch of one: squeeze() drops it
}


def reference_class():
    ns = {"torch": torch, "nn": nn, "F": F}
    tree = ast.parse(open(REF_CHORD).read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PostProcessingMLTModel"]
    assert len(nodes) == 1
    exec(compile(ast.Module(body=nodes, type_ignores=[]), REF_CHORD, "exec"), ns)
    return ns["PostProcessingMLTModel"]


def run_model(model, x, cot, dtype):
    xs = {t: v.to(dtype).clone().requires_grad_(True) for t, v in x.items()}
    model.zero_grad(set_to_none=True)
    pred = model(xs)
    sum((pred[t] * cot[t].to(dtype)).sum() for t in pred).backward()
    rec = {"out." + t: v.detach() for t, v in pred.items()}
    rec.update({"grad.in." + t: v.grad.detach() for t, v in xs.items()})
    rec.update({"gw." + k: p.grad.detach() for k, p in model.named_parameters()})
    return rec


def run_case(cls, cfg, seed):
    torch.manual_seed(seed)
    model = cls(TASKS, cfg["n_hidden"], cfg["n_layers"], dropout=0.0)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.bfloat16().float())
    model.train()
    gen = torch.Generator().manual_seed(seed + 1)
    x = {t: 2.0 * torch.randn(cfg["shape"] + (c,), generator=gen, dtype=torch.float32) for t, c in TASKS.items()}
    out_shape = tuple(d for d in cfg["shape"] if d != 1)                     # the reference's squeeze()
    cot = {t: torch.randn(out_shape + (c,), generator=gen, dtype=torch.float32) for t, c in TASKS.items()}
    m64 = copy.deepcopy(model).double()
    with ReluTap() as tap:
        m64.activation = F.relu                  # the tapped function: the class bound its default before the tap existed
        rec = run_model(m64, x, cot, torch.float64)
    rec32 = run_model(model, x, cot, torch.float32)
    worst = max(float((v.double() - rec32[k].double()).abs().max()) / (GATE * max(1.0, float(v.abs().max()))) for k, v in rec.items())
    for t in TASKS:
        assert rec["out." + t].shape == cot[t].shape
    out = {"meta.cfg": np.array([cfg["n_hidden"], cfg["n_layers"], seed], dtype=np.int64), "meta.tasks": np.array(list(TASKS.keys())),
           "meta.classes": np.array(list(TASKS.values()), dtype=np.int64), "meta.keys": np.array(list(model.state_dict().keys())),
           "meta.relu_margin": np.array(tap.margin()), "meta.fp32_over_gate": np.array(worst)}
    for t in TASKS:
        out["in." + t] = x[t].numpy()
        out["cot." + t] = cot[t].numpy()
    for k, v in model.state_dict().items():
        out["w." + k] = v.detach().numpy()
    for k, v in rec.items():
        out[k] = v.numpy()
    return out, tap.at_risk(3e-6), worst


def main():
    torch.set_num_threads(4)
    cls = reference_class()
    for i, (name, cfg) in enumerate(CASES.items()):
        for attempt in range(40):
            s = 701 + i + 1000 * attempt
            rec, risk, worst = run_case(cls, cfg, s)
            ok = risk == 0 and worst <= 0.25
            print(f"  {name}: seed {s}: {risk} ReLU inputs at the kink, fp32 / gate {worst:.3f}" + ("" if ok else ": re-drawing"))
            if ok:
                break
        assert ok, f"{name}: no seed met the conditions"
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < 2 ** 20
        print(f"  wrote {name}.npz ({os.path.getsize(path) / 1024:.1f} KiB), {len(rec['meta.keys'])} state_dict keys")


if __name__ == "__main__":
    main()
