#!/usr/bin/env python3
"""Generate tests/golden/f64_*.npz: the reference's own in-tree MetricalGNN / HGCN run in FLOAT64 on the inputs and
weights of the committed float32 fixtures (metrical_{eq,ragged}_{train,eval}, hgcn3_jk), with their gradients.

TEST INFRASTRUCTURE ONLY.  Needs the reference tree (loaded as oracle/gen_golden.py loads it); the fixtures it
writes are committed, so tests/test_oracle_vs_reference_live.py compares oracle/intree_ref.py against the
reference's float64 results without the reference.  In float64, rounding noise (fp32 BatchNorm backward) cannot
mask a semantic difference.

Usage:  python oracle/gen_golden_f64.py        (idempotent; no randomness: everything comes from the fixtures)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.gen_golden import load_reference_core  # noqa: E402
from oracle.testing import GOLDEN_DIR  # noqa: E402


def _load(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)


def _save(name, out, x, m):
    rec = {"out": out.detach().numpy(), "gx": x.grad.numpy()}
    for n, p in m.named_parameters():
        rec["g." + n] = p.grad.numpy()
    path = os.path.join(GOLDEN_DIR, f"f64_{name}.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path)


def metrical(hgnn, tag, mode):
    z = _load(f"metrical_{tag}_{mode}")
    rels = [str(r) for r in z["meta.rels"]]
    m = hgnn.MetricalGNN(8, 8, 8, etypes={r: i for i, r in enumerate(rels)}, num_layers=3, dropout=0.0, metrical=True)
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")})
    m.double().train(mode == "train")
    I = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
    x = I["x"].double().requires_grad_(True)
    out = m(x, I["edge_index"], I["edge_type"], I["beat_nodes"], I["measure_nodes"], I["beat_edges"],
            I["measure_edges"], beat_lengths=I.get("beat_lengths"), measure_lengths=I.get("measure_lengths"))
    (out * torch.from_numpy(z["gout"]).double()).sum().backward()
    _save(f"metrical_{tag}_{mode}", out, x, m)


def hgcn(hgnn):
    z = _load("hgcn3_jk")
    rels = [str(r) for r in z["meta.rels"]]
    m = hgnn.HGCN(8, 16, 8, n_layers=2, etypes={r: i for i, r in enumerate(rels)}, dropout=0.0, jk=True)
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")})
    m.double()
    I = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
    x = I["x"].double().requires_grad_(True)
    out = m(x, I["edge_index"], I["edge_type"])
    out.sum().backward()
    _save("hgcn3_jk", out, x, m)


def main():
    _, hgnn = load_reference_core()
    torch.set_default_dtype(torch.float64)      # the reference allocates `torch.zeros(...)` without dtype
    for tag in ("eq", "ragged"):
        for mode in ("train", "eval"):
            metrical(hgnn, tag, mode)
    hgcn(hgnn)


if __name__ == "__main__":
    main()
