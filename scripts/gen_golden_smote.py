#!/usr/bin/env python
"""Record tests/golden/smote_*.npz from the reference itself (needs a checkout of it; runs on the CPU, nothing of it is copied).

The reference's `models/cadence.py` and `models/analysis.py` import packages this project does not need, so the `SMOTE` class and
the `update_feature_loss` method are cut out of their files with `ast` at run time and executed with torch alone.  During the
calls `torch.randint`, `torch.rand` and `torch.randperm` are wrapped, so that every draw is recorded in the order it was made.
Arrays only (`allow_pickle=False` reads them back):
    x [N, D] f32, y [N] i64, k, choice [S] i64, gap [S, D] f32, x_over [N + S, D] f32, y_over [N + S] i64,
    perms (the permutations of the penalty, concatenated) i64, perm_lens i64, batch_size, value f32 (the penalty from 0)

    python scripts/gen_golden_smote.py --reference /path/to/reference
"""
from __future__ import annotations

import argparse
import ast
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [  # name, N, class shares, D, the smallest class must fall below k
    ("a", 300, (0.7, 0.12, 0.1, 0.08), 32, False),
    ("b", 300, (0.6, 0.2, 0.19, 0.01), 8, True),
]
K = 3


def cut(path: str, name: str, inside: str = "") -> str:
    """Source text of class / function `name` (inside class `inside`) of the file."""
    src = open(path).read()
    body = ast.parse(src).body
    if inside:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == inside).body
    node = next(n for n in body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name == name)
    lines = src.splitlines()[node.lineno - 1:node.end_lineno]
    pad = len(lines[0]) - len(lines[0].lstrip())
    return "\n".join(l[pad:] for l in lines)


class Recorder:
    def __init__(self):
        self.log = {"randint": [], "rand": [], "randperm": []}

    def __enter__(self):
        self.saved = {k: getattr(torch, k) for k in self.log}
        for k in self.log:
            setattr(torch, k, self._wrap(k))
        return self

    def _wrap(self, k):
        def fn(*a, **kw):
            out = self.saved[k](*a, **kw)
            self.log[k].append(out.clone())
            return out
        return fn

    def __exit__(self, *exc):
        for k, f in self.saved.items():
            setattr(torch, k, f)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds analysisgnn/models/cadence.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    models = os.path.join(args.reference, "analysisgnn", "models")
    ns = {"torch": torch, "F": F, "nn": nn, "np": np}
    exec(compile(cut(os.path.join(models, "cadence.py"), "SMOTE"), "reference SMOTE", "exec"), ns)
    exec(compile(cut(os.path.join(models, "analysis.py"), "update_feature_loss", "ContinualAnalysisGNN"), "reference update_feature_loss", "exec"), ns)
    for name, N, shares, D, want_small in CASES:
        for seed in range(1000):
            rs = np.random.RandomState(seed)
            y = rs.choice(len(shares), size=N, p=shares).astype(np.int64)
            cnt = np.bincount(y, minlength=len(shares))
            if (cnt[-1] < K) == want_small and (not want_small or cnt[-1] > 0):
                break
        x = np.round(rs.randn(N, D) * 0.6 * 256) / 256           # few mantissa bits: the file compresses
        xt, yt = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y)
        torch.manual_seed(seed)
        with Recorder() as rec:
            x_over, y_over = ns["SMOTE"](dims=D, distance="euclidean", k=K).fit_generate(xt, yt)
        choice = torch.cat(rec.log["randint"])
        gap = torch.cat(rec.log["rand"])
        with Recorder() as rec:
            value = ns["update_feature_loss"](None, torch.zeros(()), x_over, y_over, xt, yt, batch_size=100)
        perms = rec.log["randperm"]
        path = os.path.join(args.out, f"smote_{name}.npz")
        np.savez_compressed(path, x=xt.numpy(), y=y, k=np.int64(K), choice=choice.numpy(), gap=gap.numpy(), x_over=x_over.numpy(),
                            y_over=y_over.numpy(), perms=torch.cat(perms).numpy() if perms else np.zeros(0, np.int64),
                            perm_lens=np.asarray([p.numel() for p in perms], np.int64), batch_size=np.int64(100),
                            value=np.float32(value.item()))
        print(f"{path}: seed {seed}, counts {cnt.tolist()}, S = {x_over.shape[0] - N}, {len(perms)} permutations, penalty {value.item():.6f}, "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
