#!/usr/bin/env python
"""Record tests/golden/lr_schedules.npz: learning rates, in double, as the REFERENCE'S OWN scheduler classes and torch's
`SWALR` produce them when stepped once per optimizer step.  TEST INFRASTRUCTURE ONLY: it needs the reference tree
(AGNN_REFERENCE, default /root/reference); the two `LRScheduler` subclasses are read out of models/analysis.py at run time
(`ast`, as oracle/gen_golden_r3.py does) and executed, never copied — only the numbers they give are committed.

Driving rule (what `"interval": "step"` does): lr[k] is the rate the optimizer holds while it takes step k; after the
optimizer step the scheduler steps once.  SWA case: the base class below K; at K a `SWALR(anneal_strategy="cos")` is created
on the optimizer as the base class left it (its rate is lr(K)) and stepped once per P optimizer steps from then on.

    python scripts/gen_golden_sched.py            # writes the fixture
"""
from __future__ import annotations

import ast
import math
import os
import sys
import warnings
from typing import List

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("AGNN_REFERENCE", "/root/reference")
REF_ANALYSIS = os.path.join(REFERENCE, "analysisgnn", "models", "analysis.py")
NAMES = ["LinearWarmupCosineAnnealingLR", "LinearWarmupExponentialDecayLR"]

BASE_LR, ETA_MIN = 5e-3, 5e-5
COSINE_CASES = [(5, 4, 20), (3, 7, 20), (500, 50, 520)]               # (warmup_steps, max_epochs, steps)
EXP_CASE = dict(warmup_steps=5, decay_steps=7, gamma=0.9, eta_min=4.99e-3, base_lr=5e-3, steps=20)
SWA_CASE = dict(warmup_steps=5, max_epochs=4, start=6, period=3, anneal=2, swa_lr=5e-5, steps=20)


def reference_classes() -> dict:
    """The two scheduler classes, executed from the reference file's ClassDef nodes."""
    from torch.optim import Optimizer
    from torch.optim.lr_scheduler import LRScheduler
    tree = ast.parse(open(REF_ANALYSIS).read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in NAMES]
    assert sorted(n.name for n in nodes) == sorted(NAMES), f"{REF_ANALYSIS}: scheduler classes not found"
    ns = {"LRScheduler": LRScheduler, "Optimizer": Optimizer, "List": List, "math": math, "warnings": warnings}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), REF_ANALYSIS, "exec"), ns)
    return {n: ns[n] for n in NAMES}


def _optimizer(lr: float):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)


def drive(make_scheduler, base_lr: float, steps: int, swa=None) -> np.ndarray:
    """lr[k], k < steps.  `swa` = (start, period, anneal_epochs, swa_lr) or None."""
    from torch.optim.swa_utils import SWALR
    opt = _optimizer(base_lr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched, swalr, out = make_scheduler(opt), None, []
        for k in range(steps):
            if swa is not None and k == swa[0]:
                swalr = SWALR(opt, swa_lr=swa[3], anneal_epochs=swa[2], anneal_strategy="cos")
            out.append(float(opt.param_groups[0]["lr"]))
            opt.step()
            if swalr is None:
                sched.step()
            elif (k + 1 - swa[0]) % swa[1] == 0:
                swalr.step()
    return np.asarray(out, dtype=np.float64)


def cases(classes: dict) -> dict:
    cos, exp = classes[NAMES[0]], classes[NAMES[1]]
    out = {}
    for w, e, steps in COSINE_CASES:
        out[f"cosine_w{w}_e{e}"] = drive(lambda o: cos(o, warmup_steps=w, max_epochs=e, eta_min=ETA_MIN), BASE_LR, steps)
    c = EXP_CASE
    out["exp_w5_d7"] = drive(lambda o: exp(o, warmup_steps=c["warmup_steps"], decay_steps=c["decay_steps"], eta_min=c["eta_min"],
                                           gamma=c["gamma"]), c["base_lr"], c["steps"])
    s = SWA_CASE
    out["swa_cosine_w5_e4"] = drive(lambda o: cos(o, warmup_steps=s["warmup_steps"], max_epochs=s["max_epochs"], eta_min=ETA_MIN),
                                    BASE_LR, s["steps"], swa=(s["start"], s["period"], s["anneal"], s["swa_lr"]))
    return out


def smallest_working_warmup(cls, upto: int = 8) -> int:
    """The smallest warmup_steps for which the reference's cosine class survives construction and 3 * upto steps."""
    for w in range(upto):
        try:
            drive(lambda o: cls(o, warmup_steps=w, max_epochs=4), BASE_LR, 3 * upto)
            return w
        except (AttributeError, ZeroDivisionError):
            continue
    raise AssertionError("no working warm-up found")


def main() -> None:
    sys.dont_write_bytecode = True
    classes = reference_classes()
    out = cases(classes)
    out["meta.cosine_min_warmup"] = np.asarray(smallest_working_warmup(classes[NAMES[0]]), dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", "lr_schedules.npz")
    np.savez(path, **out)
    for k, v in out.items():
        print(f"{k:28s} {v.shape} first {np.atleast_1d(v)[:3]} last {np.atleast_1d(v)[-1]}")
    print("wrote", path)


if __name__ == "__main__":
    main()
