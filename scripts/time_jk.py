#!/usr/bin/env python
"""Time the JumpingKnowledge block alone (forward + backward) on the HIP kernels (jk.FUSED = True) and on the library body
(False), alternating the two in ONE process: `--sets` sets (>= 3), each set three alternating pairs of windows of >= `--window`
seconds, device events around every window, warm-up of both paths first.  Per shape it prints the per-call time of every window,
per set the median and the spread (max - min) of each path, and whether the fused median is below the library's by more than the
library's own spread in EVERY set (the rule that keeps jk.FUSED on for a shape class).

    python scripts/time_jk.py                          # all shapes, JSON lines on stdout
    python scripts/time_jk.py --shapes c2 --profile    # a few fused calls only: the run to wrap in
                                                       #   rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_jk.py ...
    python scripts/time_jk.py --rates DIR/..._kernel_stats.csv --shapes c2     # k_lstm_step's achieved TFLOP/s from that trace

FLOPs of k_lstm_step by formula (kept here): a direction's first step multiplies [M, H] by [4h, H]^T, every later one
[M, H + h] by [4h, H + h]^T, so one forward pass is  2 directions * 2 M 4h (T H + (T - 1) h)  FLOP of exact fp32 on the matrix
cores (peak 157 TFLOP/s: the kernel is compute bound, the bytes it moves — x_t, h, c once per column-tile row from L2, act
M 4h written — need less time than its MFMAs at every shape here).
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"c2": (16000, 256, 3), "c2_h128": (16000, 128, 3), "c5": (2000, 512, 4)}      # name -> (M, H, L); T = L, h = L H / 2
PEAK_TFLOPS = 157.0
PAIRS = 3                # windows per path and set


def step_flops(M: int, H: int, L: int) -> float:
    h, T = (L * H) // 2, L
    return 2.0 * 2.0 * M * 4 * h * (T * H + (T - 1) * h)


def build(M, H, L, dev):
    from analysisgnn_amd.core_layers import JumpingKnowledge
    torch.manual_seed(0)
    m = JumpingKnowledge(H, L).to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(1)
    xs = [torch.nn.functional.normalize(torch.randn(M, H, generator=g).relu(), dim=-1).to(dev).requires_grad_(True) for _ in range(L)]
    gout = torch.randn(M, H, generator=g).to(dev)
    return m, xs, gout


def call(m, xs, gout):
    out = m(xs)
    out.backward(gout)
    for p in m.parameters():
        p.grad = None
    for x in xs:
        x.grad = None
    return out


def window(m, xs, gout, seconds: float, per_call_guess: float) -> float:
    """Per-call milliseconds over one window of at least `seconds`."""
    n = max(5, int(seconds / max(per_call_guess, 1e-5)) + 1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        call(m, xs, gout)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    if ms < 1000.0 * seconds:                      # the guess was too long: once more, 1.5 x the calls the measured rate asks for
        return window(m, xs, gout, seconds, ms / 1000.0 / n / 1.5)
    return ms / n


def measure(name, sets: int, seconds: float, dev) -> dict:
    from analysisgnn_amd import jk
    M, H, L = SHAPES[name]
    m, xs, gout = build(M, H, L, dev)
    was = jk.FUSED, jk.MIN_ROWS
    jk.MIN_ROWS = 0                                 # the kernels at every shape listed: the row threshold is what is being measured
    try:
        guess = {}
        outs = {}
        for on in (True, False):
            jk.FUSED = on
            assert jk.kernel_applicable(m, xs)
            for _ in range(3):
                outs[on] = call(m, xs, gout).detach().clone()
            torch.cuda.synchronize()
            guess[on] = window(m, xs, gout, 0.05, 5e-3) / 1000.0
        diff = float((outs[True] - outs[False]).abs().max())
        rows = []
        for _ in range(sets):                       # a set: PAIRS alternating pairs of windows
            row = {"fused": [], "library": []}
            for _ in range(PAIRS):
                for on in (True, False):
                    jk.FUSED = on
                    row["fused" if on else "library"].append(window(m, xs, gout, seconds, guess[on]))
            rows.append(row)
    finally:
        jk.FUSED, jk.MIN_ROWS = was
    med, spread = statistics.median, lambda v: max(v) - min(v)          # noqa: E731
    per_set = [dict(fused_median_ms=med(r["fused"]), fused_spread_ms=spread(r["fused"]), library_median_ms=med(r["library"]),
                    library_spread_ms=spread(r["library"])) for r in rows]
    return dict(shape=name, M=M, H=H, L=L, h=(L * H) // 2, windows=rows, sets=per_set, out_max_abs_diff=diff,
                fused_wins_every_set=all(p["fused_median_ms"] < p["library_median_ms"] - p["library_spread_ms"] for p in per_set),
                step_fwd_gflop=step_flops(M, H, L) / 1e9)


def profile(name, dev, calls: int = 10) -> None:
    from analysisgnn_amd import jk
    M, H, L = SHAPES[name]
    m, xs, gout = build(M, H, L, dev)
    jk.FUSED, jk.MIN_ROWS = True, 0
    for _ in range(calls):
        call(m, xs, gout)
    torch.cuda.synchronize()
    print(json.dumps(dict(profiled=name, calls=calls)))


def rates(path: str, name: str) -> None:
    """k_lstm_step's share of the fp32-matrix peak from a rocprofv3 kernel-stats CSV of `--profile` on ONE shape."""
    M, H, L = SHAPES[name]
    with open(path) as f:
        for r in csv.DictReader(f):
            kn = r.get("Name") or r.get("KernelName") or ""
            if "k_lstm_step" in kn:
                ns, n = float(r["TotalDurationNs"]), int(r["Calls"])
                first = "ILb0" in kn or "<false>" in kn    # k_lstm_step<false>: the first step of both directions
                per_fwd = n / (1 if first else L - 1)
                h, T = (L * H) // 2, L
                fl = 2.0 * 2.0 * M * 4 * h * (H if first else (T - 1) * (H + h))
                tf = fl * per_fwd / ns / 1e3
                print(json.dumps(dict(kernel=kn[:60], calls=n, total_ms=ns / 1e6, tflops=tf, share_of_peak=tf / PEAK_TFLOPS)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--rates", default=None)
    a = ap.parse_args()
    names = [s for s in a.shapes.split(",") if s]
    if a.rates:
        rates(a.rates, names[0])
        return
    assert torch.cuda.is_available(), "time_jk.py measures on a HIP device"
    assert a.sets >= 3 and a.window >= 0.5 or a.profile
    dev = torch.device("cuda:0")
    for name in names:
        if a.profile:
            profile(name, dev)
        else:
            print(json.dumps(measure(name, a.sets, a.window, dev)), flush=True)


if __name__ == "__main__":
    main()
