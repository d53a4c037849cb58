#!/usr/bin/env python
"""Time one forward + backward of a bidirectional LSTM layer through the persistent kernels (lstm_seq.lstm_forward) and through
the same `nn.LSTM` on the library path (`rnn(x)[0]`, what ran before the kernels existed), alternating the two in ONE process on
one card: `--sets` sets (>= 3), each set three alternating pairs of windows of >= `--window` seconds, device events around every
window, warm-up of both paths first.  Per shape (B, T, I, hidden) it prints a JSON line with the per-call time of every window,
per set the median and the spread (max - min) of each path, the time per step of the recurrence (per-call time / T), the ratio
library / kernel, whether the kernel median is below the library's by more than the two paths' spreads in EVERY set (the rule
that keeps a hidden size routed to the kernels), and the recurrence kernels alone (agnn_lstm_seq_fwd_f32 /
agnn_lstm_seq_bwd_f32 called directly on resident operands): microseconds per time step, to set beside the GRU's 0.61 us
(csrc/gru.hip).

    python scripts/time_lstm_seq.py                       # both shapes
    python scripts/time_lstm_seq.py --shapes h128 --sets 3 --window 0.5
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"h128": (32, 500, 256, 128), "h64": (32, 500, 128, 64)}      # name -> (B, T, I, hidden per direction)
PAIRS = 3                # windows per path and set
GRU_FWD_US_PER_STEP = 0.61


def build(B, T, I, hidden, dev):
    torch.manual_seed(0)
    m = torch.nn.LSTM(I, hidden, num_layers=1, batch_first=True, bidirectional=True).to(dev).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, T, I, generator=g).to(dev).requires_grad_(True)
    gout = torch.randn(B, T, 2 * hidden, generator=g).to(dev)
    return m, x, gout


def call(m, x, gout, kernels: bool):
    from analysisgnn_amd.lstm_seq import lstm_forward
    out = lstm_forward(m, x, True) if kernels else m(x)[0]
    out.backward(gout)
    grads = [x.grad] + [p.grad for p in m.parameters()]
    x.grad = None
    for p in m.parameters():
        p.grad = None
    return out, grads


def timed(fn, seconds: float, guess: float) -> float:
    """Per-call milliseconds over one window of at least `seconds`."""
    n = max(5, int(seconds / max(guess, 1e-5)) + 1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    if ms < 1000.0 * seconds:                      # the guess was too long: once more, 1.5 x the calls the measured rate asks for
        return timed(fn, seconds, ms / 1000.0 / n / 1.5)
    return ms / n


def kernels_alone(B, T, hidden, dev, seconds: float) -> dict:
    """The two recurrence launches alone, on operands that stay where they are: milliseconds per launch and us per time step."""
    from analysisgnn_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)                                 # noqa: E731
    gi, w, b, dy = r(B, T, 2, 4 * hidden), r(2, 4 * hidden, hidden) * 0.1, r(2, 4 * hidden), r(B, T, 2 * hidden)
    y = torch.empty(B, T, 2 * hidden, device=dev)
    saved = torch.empty(B, T, 2, 5, hidden, device=dev)
    dg = torch.empty(B, T, 2, 4 * hidden, device=dev)
    hp = torch.empty(B, T, 2, hidden, device=dev)
    st = _lib.stream_ptr(dev)

    def fwd():
        _lib.check(lib.agnn_lstm_seq_fwd_f32(gi.data_ptr(), w.data_ptr(), b.data_ptr(), B, T, hidden, y.data_ptr(), saved.data_ptr(), None, None,
                                             st), "fwd")

    def bwd():
        _lib.check(lib.agnn_lstm_seq_bwd_f32(dy.data_ptr(), y.data_ptr(), saved.data_ptr(), w.data_ptr(), B, T, hidden, dg.data_ptr(), None,
                                             hp.data_ptr(), st), "bwd")

    out = {}
    for name, fn in (("fwd", fwd), ("bwd", bwd)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = [timed(fn, seconds, 1e-3) for _ in range(PAIRS)]
        out[name] = dict(launch_ms=ms, us_per_time_step=statistics.median(ms) * 1000.0 / T, spread_us_per_time_step=(max(ms) - min(ms)) * 1000.0 / T)
    return out


def measure(name, sets: int, seconds: float, dev) -> dict:
    B, T, I, hidden = SHAPES[name]
    m, x, gout = build(B, T, I, hidden, dev)
    guess, outs = {}, {}
    for on in (True, False):
        for _ in range(3):
            out, grads = call(m, x, gout, on)
            outs[on] = [out.detach().clone()] + [t.clone() for t in grads]
        torch.cuda.synchronize()
        guess[on] = timed(lambda: call(m, x, gout, on), 0.05, 5e-3) / 1000.0
    # faster and different is not faster: outputs and every gradient of the two paths, relative to the library's max-abs
    diff = max(float((a - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip(outs[True], outs[False]))
    rows = []
    for _ in range(sets):                           # a set: PAIRS alternating pairs of windows
        row = {"kernels": [], "library": []}
        for _ in range(PAIRS):
            for on in (True, False):
                row["kernels" if on else "library"].append(timed(lambda: call(m, x, gout, on), seconds, guess[on]))
        rows.append(row)
    med, spread = statistics.median, lambda v: max(v) - min(v)          # noqa: E731
    per_set = [dict(kernels_median_ms=med(r["kernels"]), kernels_spread_ms=spread(r["kernels"]), library_median_ms=med(r["library"]),
                    library_spread_ms=spread(r["library"])) for r in rows]
    km, lm = med([p["kernels_median_ms"] for p in per_set]), med([p["library_median_ms"] for p in per_set])
    alone = kernels_alone(B, T, hidden, dev, seconds)
    return dict(shape=name, B=B, T=T, I=I, hidden=hidden, windows=rows, sets=per_set, paths_max_rel_diff=diff,
                kernels_us_per_step=km * 1000.0 / T, library_us_per_step=lm * 1000.0 / T, library_over_kernels=lm / km,
                kernels_win_every_set=all(p["kernels_median_ms"] < p["library_median_ms"] - (p["library_spread_ms"] + p["kernels_spread_ms"])
                                          for p in per_set),
                recurrence_kernels_alone=alone, gru_fwd_us_per_time_step=GRU_FWD_US_PER_STEP)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_lstm_seq.py measures on a HIP device"
    assert a.sets >= 3 and a.window >= 0.5
    dev = torch.device("cuda:0")
    for name in [s for s in a.shapes.split(",") if s]:
        print(json.dumps(measure(name, a.sets, a.window, dev)), flush=True)


if __name__ == "__main__":
    main()
