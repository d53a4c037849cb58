#!/usr/bin/env python
"""Time SMOTE oversampling + feature penalty (csrc/smote.hip through analysisgnn_amd/smote.py) against two torch compositions of
the same rules on one GPU, in one process:

  loop        the reference's formulation: per class a T x T similarity matrix and its full argsort, then one Python iteration
              per minority row (randint, rand, two gathers, a fused multiply-add, an indexed store: about eight launches each)
  vectorised  the same T x T argsort, then the synthetic rows of a class in a handful of batched gathers
Both use `cdist` + `min` per class for the penalty, as the reference does.  The compositions are written from the rules in
analysisgnn_amd/smote.py; they draw with torch's generator (the kernel path with Philox), which costs the same launches.

Shape: N = 16 000 rows, D = 128, class shares (0.90, 0.04, 0.03, 0.03), k = 3: 1 600 minority rows, 41 280 synthetic rows.
Measured: forward (`fit_generate` + `feature_penalty`), and forward + backward (the gradient with respect to X of the penalty
and of a fixed random weighting of x_over, through torch.autograd.grad).  Each figure is the median of SETS windows per side; the
sides ALTERNATE window by window, every window is REPS calls between two device events, sized from a first timed call so that
a window lasts about WINDOW_MS.  The spread (min .. max) is printed with every median; a difference counts only where the two
spreads do not overlap.

    python scripts/time_smote.py [--out profiles/smote.md]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = 5
WINDOW_MS = 400.0
MAX_REPS = 2000
DEV = "cuda:0"
N, D, K = 16000, 128, 3
SHARES = (0.90, 0.04, 0.03, 0.03)


def window(fn, reps: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(sides: dict) -> dict:
    reps = {}
    for k, fn in sides.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        reps[k] = max(1, min(MAX_REPS, int(WINDOW_MS / max(window(fn, 1), 1e-3))))
    times = {k: [] for k in sides}
    for _ in range(SETS):
        for k, fn in sides.items():
            times[k].append(window(fn, reps[k]))
    return {k: (statistics.median(v), min(v), max(v), reps[k]) for k, v in times.items()}


def torch_fit_generate(x, y, k, loop: bool):
    occ = torch.bincount(y)
    dominant = int(torch.argmax(occ))
    n_occ = int(occ[dominant].item())
    counts = occ.tolist()
    xs, ys = [x], [y]
    for c, o in enumerate(counts):
        if c == dominant or o < k or o == n_occ:
            continue
        copies = int((n_occ - o) * 100 / o / 100)
        if copies == 0:
            continue
        xc = x[y == c]
        z = F.normalize(xc, p=2, dim=1)
        nb = torch.argsort(z @ z.t(), dim=1)[:, 1:k + 1]
        if loop:
            out = torch.zeros(copies * o, x.shape[1], device=x.device)
            for i in range(o):
                pick = torch.randint(0, k - 1, (copies,), device=x.device)
                gap = torch.rand((copies, x.shape[1]), device=x.device)
                out[torch.arange(i * copies, (i + 1) * copies, device=x.device)] = xc[i] + gap * (xc[nb[i][pick]] - xc[i])
        else:
            own = torch.arange(o, device=x.device).repeat_interleave(copies)
            pick = torch.randint(0, k - 1, (o * copies,), device=x.device)
            gap = torch.rand((o * copies, x.shape[1]), device=x.device)
            base = xc[own]
            out = base + gap * (xc[nb[own, pick]] - base)
        xs.append(out)
        ys.append(torch.full((out.shape[0],), c, dtype=torch.int64, device=x.device))
    return torch.cat(xs), torch.cat(ys)


def torch_penalty(x_over, y_over, x, y, batch_size=100, threshold=1.0):
    labels = y_over.unique()
    bs = batch_size // len(labels)
    total = x.new_zeros(())
    for c in labels:
        xc, qc = x[y == c], x_over[y_over == c]
        if len(xc) > bs:
            xc = xc[torch.randperm(len(xc), device=x.device)[:bs]]
        if len(qc) > bs:
            qc = qc[torch.randperm(len(qc), device=x.device)[:bs]]
        total = total + torch.clamp(torch.cdist(qc, xc).min(dim=1).values - threshold, min=0).mean()
    return total


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_smote.py measures on a HIP device; none found")
    from analysisgnn_amd import smote
    g = torch.Generator().manual_seed(0)
    counts = [int(round(N * s)) for s in SHARES]
    y = torch.arange(len(SHARES)).repeat_interleave(torch.tensor(counts))[torch.randperm(N, generator=g)].to(DEV)
    x = torch.randn(N, D, generator=g).to(DEV).requires_grad_(True)
    S = smote.plan(counts, K).n_synthetic
    w = torch.randn(N + S, D, generator=g).to(DEV)
    sm = smote.SMOTE(dims=D, distance="euclidean", k=K)
    zero = torch.zeros((), device=DEV)

    def side(kind: str, backward: bool):
        def fn():
            with torch.set_grad_enabled(backward):
                if kind == "kernels":
                    xo, yo = sm.fit_generate(x, y)
                    v = smote.feature_penalty(zero, xo, yo, x, y)
                else:
                    xo, yo = torch_fit_generate(x, y, K, loop=(kind == "loop"))
                    v = torch_penalty(xo, yo, x, y)
                if backward:
                    torch.autograd.grad([v, xo], x, [torch.ones_like(v), w])
        return fn

    # the three paths agree on what does not depend on the draws before anything is timed
    with torch.no_grad():
        a, ya = sm.fit_generate(x, y)
        b, yb = torch_fit_generate(x, y, K, loop=False)
    assert a.shape == b.shape == (N + S, D) and torch.equal(ya, yb) and torch.equal(a[:N], b[:N])

    records, rows = [], []
    for backward, tag in ((False, "forward"), (True, "forward + backward")):
        res = alternate({k: side(k, backward) for k in ("kernels", "vectorised", "loop")})
        for k, (med, lo, hi, reps) in res.items():
            records.append(dict(what=tag, side=k, ms=med, ms_min=lo, ms_max=hi, reps=reps, sets=SETS, N=N, D=D, S=S))
            print(json.dumps(records[-1]), flush=True)
        kn = res["kernels"]
        row = [tag] + [f"{res[k][0]:.3f} ({res[k][1]:.3f} .. {res[k][2]:.3f})" for k in ("kernels", "vectorised", "loop")]
        for other in ("vectorised", "loop"):
            o = res[other]
            row.append(f"{o[0] / kn[0]:.2f}x faster" if kn[2] < o[1] else (f"{kn[0] / o[0]:.2f}x SLOWER" if o[2] < kn[1] else "spreads overlap"))
        rows.append(row)
    cols = ["", "kernels ms", "vectorised torch ms", "per-row loop ms", "kernels vs vectorised", "kernels vs loop"]
    table = ["| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)] + ["| " + " | ".join(r) + " |" for r in rows]
    text = "\n".join(table)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"N = {N}, D = {D}, k = {K}, class counts {counts}, {S} synthetic rows; {torch.cuda.get_device_name(0)}; median (min .. max) of "
                    f"{SETS} alternating windows of about {WINDOW_MS:.0f} ms\n\n{text}\n\n" + "\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    main()
