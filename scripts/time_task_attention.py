#!/usr/bin/env python
"""Time the cross-task attention of the logit-fusion block (csrc/taskattn.hip through analysisgnn_amd/task_attention.py) against
the library body (`task_attention.FUSED = False`: F.scaled_dot_product_attention on [N, h, T, d] views of the same projection)
on one GPU, in one process.

Shapes: T = 21 tokens, E = 64, 4 heads (D = 16), N in {500, 4096, 16000} sequences.  For each N:
  attention alone   `task_attention.attention(qkv, T, heads, p)` / the library body on a fixed [N T, 3E] projection: forward,
                    forward + backward; eval (p = 0) and train (p = 0.3)
and at the last N:
  forward_clf       TorchAnalysisGNN(out_channels = 128, 21 tasks, logit_fusion = True).forward_clf, forward + backward
Each figure is the median of SETS windows per side; the two sides ALTERNATE window by window (other work shares the host), every
window is REPS calls between two device events, sized from a first timed call so that a window lasts about WINDOW_MS.  The spread
(min .. max over the windows) is printed with every median.  A difference counts only where the two spreads do not overlap.

The kernel side's rate is the algorithm's own byte count over the window time: forward 16 N T E bytes (qkv read once, o written
once), backward 32 N T E bytes (qkv, dO and o read once, dqkv written once; lse is 1/16 of o and left out); the backward's time
is (forward + backward) - forward.  Bytes are the bound of this kernel (about 1.8 GFLOP forward at N = 16 000): the rate is set
against 8.0 TB/s (HBM specification) and 6.3 TB/s (achievable).

    python scripts/time_task_attention.py [--sizes 500,4096,16000] [--out time_task_attention.json]
Prints one JSON line per measurement and a markdown table at the end.
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

HBM_SPEC_TBS, HBM_ACHIEVABLE_TBS = 8.0, 6.3
SETS = 5
WINDOW_MS = 300.0
MAX_REPS = 20000
DEV = "cuda:0"
T, E, HEADS = 21, 64, 4
CLASSES = [4, 50, 50, 15, 185, 2, 7, 12, 35, 3, 9, 21, 5, 16, 40, 11, 6, 30, 8, 2, 13]


def window(fn, reps: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(sides: dict) -> dict:
    """{name: fn} -> {name: (median ms, min ms, max ms, reps)}; the sides alternate window by window."""
    reps = {}
    for k, fn in sides.items():
        for _ in range(3):
            fn()                                                    # warm-up: code objects, library algorithm choice
        torch.cuda.synchronize()
        reps[k] = max(1, min(MAX_REPS, int(WINDOW_MS / max(window(fn, 1), 1e-3))))
    times = {k: [] for k in sides}
    for _ in range(SETS):
        for k, fn in sides.items():
            times[k].append(window(fn, reps[k]))
    return {k: (statistics.median(v), min(v), max(v), reps[k]) for k, v in times.items()}


def library_body(qkv: torch.Tensor, N: int, p: float) -> torch.Tensor:
    """What heads.CrossTaskTransformer runs with FUSED = False."""
    v5 = qkv.view(N, T, 3, HEADS, E // HEADS)
    q, k, v = (v5[:, :, i].transpose(1, 2) for i in range(3))
    return F.scaled_dot_product_attention(q, k, v, dropout_p=p).transpose(1, 2).reshape(N * T, E)


def verdict(a, b) -> str:
    """a, b: (median, min, max, reps) of kernel and library."""
    if a[2] < b[1]:
        return f"kernel {b[0] / a[0]:.2f}x faster"
    if b[2] < a[1]:
        return f"kernel {a[0] / b[0]:.2f}x SLOWER"
    return "spreads overlap"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,4096,16000")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_task_attention.py measures on a HIP device; none found")
    from analysisgnn_amd import task_attention as ta
    rows, records = [], []
    sizes = [int(s) for s in args.sizes.split(",")]
    for N in sizes:
        g = torch.Generator().manual_seed(N)
        qkv = torch.randn(N * T, 3 * E, generator=g).to(DEV).requires_grad_(True)
        gout = torch.randn(N * T, E, generator=g).to(DEV)

        def attn(fused: bool, backward: bool, p: float):
            def fn():
                with torch.set_grad_enabled(backward):
                    o = ta.attention(qkv, T, HEADS, p) if fused else library_body(qkv, N, p)
                    if backward:
                        torch.autograd.grad(o, qkv, gout)
            return fn

        # the two paths agree at this size before anything is timed (1e-4 of the largest magnitude)
        with torch.no_grad():
            a, b = ta.attention(qkv, T, HEADS), library_body(qkv, N, 0.0)
            err = float((a - b).abs().max()) / float(b.abs().max())
        assert err < 1e-4, f"N={N}: kernel and library attention differ by {err:.2e} of max|o|"
        for mode, p in (("eval", 0.0), ("train p=0.3", 0.3)):
            res = {}
            for backward in (False, True):
                res[backward] = alternate({"kernel": attn(True, backward, p), "library": attn(False, backward, p)})
                for side, (med, lo, hi, reps) in res[backward].items():
                    records.append(dict(N=N, what="attention", mode=mode, side=side, backward=backward, ms=med, ms_min=lo, ms_max=hi,
                                        reps=reps, sets=SETS))
                    print(json.dumps(records[-1]), flush=True)
            row = {"N": N, "what": f"attention, {mode}"}
            for backward, tag in ((False, "fwd"), (True, "fwd+bwd")):
                for side in ("kernel", "library"):
                    med, lo, hi, _ = res[backward][side]
                    row[f"{tag} {side} ms"] = f"{med:.4f} ({lo:.4f} .. {hi:.4f})"
                row[f"{tag}"] = verdict(res[backward]["kernel"], res[backward]["library"])
            f_ms, fb_ms = res[False]["kernel"][0], res[True]["kernel"][0]
            tb_f = 16.0 * N * T * E / (f_ms * 1e-3) / 1e12
            tb_b = 32.0 * N * T * E / (max(fb_ms - f_ms, 1e-6) * 1e-3) / 1e12
            row["kernel fwd TB/s"] = f"{tb_f:.2f} ({100 * tb_f / HBM_SPEC_TBS:.0f} % of {HBM_SPEC_TBS}, {100 * tb_f / HBM_ACHIEVABLE_TBS:.0f} % of {HBM_ACHIEVABLE_TBS})"
            row["kernel bwd TB/s"] = f"{tb_b:.2f} ({100 * tb_b / HBM_SPEC_TBS:.0f} % of {HBM_SPEC_TBS}, {100 * tb_b / HBM_ACHIEVABLE_TBS:.0f} % of {HBM_ACHIEVABLE_TBS})"
            rows.append(row)

    # the whole head block with logit fusion, forward + backward, at the last size
    from analysisgnn_amd.models import TorchAnalysisGNN
    from analysisgnn_amd.synth import make_batch
    N = sizes[-1]
    tasks = {f"task{i:02d}": c for i, c in enumerate(CLASSES)}
    for mode, p in (("eval", 0.0), ("train p=0.3", 0.3)):
        torch.manual_seed(1)
        m = TorchAnalysisGNN(make_batch(1, 30).metadata(), 25, 32, 128, tasks, 2, dropout=p, use_jk=False, logit_fusion=True).to(DEV).train(p > 0)
        x = torch.randn(N, 128, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
        params = [q for k, q in m.named_parameters() if k.split(".")[0] in ("clf_dict", "clf_proj_layers", "cross_task_transformer", "fusion_layers")]
        gl = torch.randn(N, sum(CLASSES), generator=torch.Generator().manual_seed(3)).to(DEV)

        def clf(fused: bool):
            def fn():
                ta.FUSED = fused
                logits, _, _ = m.forward_clf_fused(x)
                torch.autograd.grad(logits, (x, *params), gl)
                ta.FUSED = True
            return fn

        r = alternate({"kernel": clf(True), "library": clf(False)})
        for side, (med, lo, hi, reps) in r.items():
            records.append(dict(N=N, what="forward_clf", mode=mode, side=side, backward=True, ms=med, ms_min=lo, ms_max=hi, reps=reps, sets=SETS))
            print(json.dumps(records[-1]), flush=True)
        row = {"N": N, "what": f"forward_clf, {mode}", "fwd+bwd": verdict(r["kernel"], r["library"])}
        for side in ("kernel", "library"):
            med, lo, hi, _ = r[side]
            row[f"fwd+bwd {side} ms"] = f"{med:.4f} ({lo:.4f} .. {hi:.4f})"
        rows.append(row)

    cols = ["N", "what", "fwd kernel ms", "fwd library ms", "fwd", "fwd+bwd kernel ms", "fwd+bwd library ms", "fwd+bwd", "kernel fwd TB/s",
            "kernel bwd TB/s"]
    table = ["| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
    table += ["| " + " | ".join(str(r.get(c, "")) for c in cols) + " |" for r in rows]
    print("\n".join(table))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(records=records, table=table, device=torch.cuda.get_device_name(0)), f, indent=1)


if __name__ == "__main__":
    main()
