#!/usr/bin/env python
"""Record tests/golden/jk_fused_l2.npz and jk_fused_l4.npz: the REFERENCE'S OWN `JumpingKnowledge`, run in float64 on the CPU,
forward and backward.  TEST INFRASTRUCTURE ONLY: it needs the reference tree (its path in AGNN_REFERENCE); the
class is read out of models/core/gnn.py at run time (`ast`, as scripts/gen_golden_sched.py does) and executed, never copied —
only the numbers it gives are committed.

Inputs and parameters are seeded and fp32-representable (drawn in fp32, then widened), so the fp32 kernels under test start from
exactly the values the float64 run saw.  Each file holds
    x0 .. x{T-1} [N, H]            the layer outputs
    p.<name>                       the ten parameters (nn.LSTM's eight, att.weight, att.bias)
    gout [N, H]                    the output gradient fed to backward
    out [N, H], dx0 .. dx{T-1}, g.<name>     the results
(att.bias's gradient is what autograd leaves: a rounding-level residue — the bias cancels in the softmax.)

    python scripts/gen_golden_jk.py            # writes both fixtures
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("AGNN_REFERENCE", "")
REF_GNN = os.path.join(REFERENCE, "analysisgnn", "models", "core", "gnn.py")
NAME = "JumpingKnowledge"
CASES = {"jk_fused_l2": dict(N=130, H=32, L=2, seed=20), "jk_fused_l4": dict(N=70, H=32, L=4, seed=40)}


def reference_class():
    """The class, executed from the reference file's ClassDef node."""
    assert os.path.isfile(REF_GNN), "set AGNN_REFERENCE to the reference tree"
    tree = ast.parse(open(REF_GNN).read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == NAME]
    assert len(nodes) == 1, f"{REF_GNN}: {NAME} not found"
    ns = {"torch": torch, "nn": torch.nn}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), REF_GNN, "exec"), ns)
    return ns[NAME]


def run(cls, N: int, H: int, L: int, seed: int) -> dict:
    torch.manual_seed(seed)
    m = cls(H, L)                                      # fp32 initialisation: every parameter is fp32-representable
    m = m.double()
    g = torch.Generator().manual_seed(seed + 1)
    xs = [torch.randn(N, H, generator=g, dtype=torch.float32).double().requires_grad_(True) for _ in range(L)]
    gout = torch.randn(N, H, generator=g, dtype=torch.float32).double()
    with torch.no_grad():
        m.att.bias.copy_(torch.randn(1, generator=g, dtype=torch.float32).double())
    out = m(xs)
    out.backward(gout)
    rec = {"gout": gout.numpy(), "out": out.detach().numpy()}
    for t, x in enumerate(xs):
        rec[f"x{t}"] = x.detach().numpy()
        rec[f"dx{t}"] = x.grad.numpy()
    for n, p in m.named_parameters():
        rec[f"p.{n}"] = p.detach().numpy()
        rec[f"g.{n}"] = p.grad.numpy()
    assert sum(k.startswith("g.") for k in rec) == 10
    return rec


def main() -> None:
    sys.dont_write_bytecode = True
    cls = reference_class()
    for name, case in CASES.items():
        rec = run(cls, **case)
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"wrote {path}: {os.path.getsize(path)} bytes, |out|max {np.abs(rec['out']).max():.4f}, "
              f"|g.att.bias| {np.abs(rec['g.att.bias']).max():.2e}")


if __name__ == "__main__":
    main()
