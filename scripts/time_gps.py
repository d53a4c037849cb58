#!/usr/bin/env python
"""Time the graph-transformer attention (csrc/attn.hip through analysisgnn_amd/attention.py) against the library body
(`attention.FUSED = False`: F.scaled_dot_product_attention on the same projections) on one GPU, in one process.

Shapes: N in {500, 4096, 16000}, H = 256, 4 heads (D = 64).  For each N:
  attention alone   `attention.attention(qkv, heads)` / the library body on a fixed [N, 3H] projection: forward, forward + backward
  one HGPSLayer     core_layers.HGPSLayer(H, H, 4) on a random typed graph of 4 N edges: forward, forward + backward
Each figure is the median of SETS windows per side; the two sides ALTERNATE window by window (other work shares the host), every
window is REPS calls between two device events, sized from a first timed call so that a window lasts about WINDOW_MS.  The spread
(min .. max over the windows) is printed with every median.

The fused attention's rate is the algorithm's own product count over the window time: forward 2 products, 4 heads N^2 D FLOPs;
backward 7 products (S twice, dP twice, dQ, dK, dV), 14 heads N^2 D.  Share of the fp32-matrix peak (157.3 TFLOP/s,
v_mfma_f32_32x32x2_f32): that rate over the peak; the backward's share comes from (forward + backward) - forward.

    python scripts/time_gps.py [--sizes 500,4096,16000] [--out time_gps.json]
Prints one JSON line per measurement and a markdown table at the end.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3
SETS = 5
WINDOW_MS = 300.0
MAX_REPS = 2000
DEV = "cuda:0"


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,4096,16000")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gps.py measures on a HIP device; none found")
    from analysisgnn_amd import attention, core_layers as cl
    H, heads = 256, 4
    D = H // heads
    rows, records = [], []
    for N in (int(s) for s in args.sizes.split(",")):
        g = torch.Generator().manual_seed(N)
        qkv = torch.randn(N, 3 * H, generator=g).to(DEV).requires_grad_(True)
        gout = torch.randn(N, H, generator=g).to(DEV)
        x = torch.randn(N, H, generator=g).to(DEV).requires_grad_(True)
        ei = torch.randint(0, N, (2, 4 * N), generator=g).to(DEV)
        et = torch.randint(0, 7, (4 * N,), generator=g).to(DEV)
        torch.manual_seed(1)
        layer = cl.HGPSLayer(H, H, heads).to(DEV).eval()
        leaves = (x, *layer.parameters())

        def attn(fused: bool, backward: bool):
            def fn():
                with torch.set_grad_enabled(backward):
                    o = attention.attention(qkv, heads) if fused else attention._library_attention(qkv, heads, 0.0)
                    if backward:
                        torch.autograd.grad(o, qkv, gout)
            return fn

        def lay(fused: bool, backward: bool):
            def fn():
                attention.FUSED = fused
                with torch.set_grad_enabled(backward):
                    o = layer(x, ei, et)
                    if backward:
                        torch.autograd.grad(o, leaves, gout)
                attention.FUSED = True
            return fn

        # the two paths agree at this size before anything is timed (1e-4 of the largest magnitude)
        with torch.no_grad():
            a, b = attention.attention(qkv, heads), attention._library_attention(qkv, heads, 0.0)
            err = float((a - b).abs().max()) / float(b.abs().max())
        assert err < 1e-4, f"N={N}: fused and library attention differ by {err:.2e} of max|o|"
        for what, make in (("attention", attn), ("HGPSLayer", lay)):
            res = {}
            for backward in (False, True):
                r = alternate({"fused": make(True, backward), "library": make(False, backward)})
                res[backward] = r
                for side, (med, lo, hi, reps) in r.items():
                    records.append(dict(N=N, what=what, side=side, backward=backward, ms=med, ms_min=lo, ms_max=hi, reps=reps, sets=SETS))
                    print(json.dumps(records[-1]), flush=True)
            row = dict(N=N, what=what)
            for backward, tag in ((False, "fwd"), (True, "fwd+bwd")):
                for side in ("fused", "library"):
                    med, lo, hi, _ = res[backward][side]
                    row[f"{tag} {side}"] = f"{med:.3f} ({lo:.3f} .. {hi:.3f})"
            if what == "attention":
                f_ms, fb_ms = res[False]["fused"][0], res[True]["fused"][0]
                tf_f = 4 * heads * N * N * D / (f_ms * 1e-3) / 1e12
                tf_b = 14 * heads * N * N * D / (max(fb_ms - f_ms, 1e-6) * 1e-3) / 1e12
                row["fwd TFLOP/s (share)"] = f"{tf_f:.1f} ({100 * tf_f / PEAK_TFLOPS:.0f} %)"
                row["bwd TFLOP/s (share)"] = f"{tf_b:.1f} ({100 * tf_b / PEAK_TFLOPS:.0f} %)"
            rows.append(row)
    cols = ["N", "what", "fwd fused", "fwd library", "fwd+bwd fused", "fwd+bwd library", "fwd TFLOP/s (share)", "bwd TFLOP/s (share)"]
    table = ["| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
    table += ["| " + " | ".join(str(r.get(c, "")) for c in cols) + " |" for r in rows]
    print("\n".join(table))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(records=records, table=table, device=torch.cuda.get_device_name(0)), f, indent=1)


if __name__ == "__main__":
    main()
