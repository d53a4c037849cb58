#!/usr/bin/env python
"""Time the class-balanced cross entropy (`cadence.balanced_cross_entropy`, csrc/balce.hip) on [16000, 5], value and gradient, against
the torch composition of the reference's validation step: bincount, reciprocal, F.cross_entropy(weight=...); and the cadence models'
join (`cadence.pool_norm`, csrc/pooljoin.hip) on [16000, 128] and [16000, 256] with 0 .. 3 in-neighbours per row, value and gradient
(`torch.autograd.grad` of a fixed cotangent), against the composition of the library's own general kernels, written here only:
`ops.aggregate(AggSpec(mean, shared_slot, skip_self, col_limit), self_t=x)` -> `fused.norm_act`.  One GPU, same inputs, one process.
Protocol: hipEvent pairs around every call, WARMUP untimed iterations, ITERS timed ones, the sides alternating iteration by
iteration; median and p10 / p90 in microseconds.  Every call is eager: nothing here is captured into a graph.  Called eagerly,
the sides are bound by the host's issue time of their launches, not by bytes: the figures compare launch chains.

    python scripts/time_cadence.py [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, ITERS = 20, 200
DEV = "cuda:0"
HBM = 8e12


def timed(sides: dict, iters: int = ITERS) -> dict:
    """{name: (median, p10, p90) in microseconds} of the callables, alternating, one event pair per call."""
    for _ in range(WARMUP):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in sides}
    for i in range(iters):
        for k, fn in sides.items():
            a, b = ev[k][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    out = {}
    for k in sides:
        t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[k])
        out[k] = (t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10])
    return out


def row(what, side, stat, nbytes, note):
    med, lo, hi = stat
    floor = f"{nbytes / HBM * 1e6:.1f}" if nbytes else "-"
    size = f"{nbytes / 1e6:.1f} MB ({note})" if nbytes else note
    return f"| {what} | {side} | {med:.1f} | {lo:.1f} .. {hi:.1f} | {size} | {floor} |"


def loss_rows(n, C, lines):
    from analysisgnn_amd import cadence
    g = torch.Generator().manual_seed(n)
    z = torch.randn(n, C, generator=g).to(DEV).requires_grad_(True)
    y = torch.randint(0, C, (n,), generator=g).to(DEV)

    def ours():
        return torch.autograd.grad(cadence.balanced_cross_entropy(z, y), z)

    def ref():
        num = torch.bincount(y, minlength=C)
        w = 1 / (num.float() + 1e-6)
        return torch.autograd.grad(F.cross_entropy(z, y, weight=w), z)
    assert float((ours()[0] - ref()[0]).abs().max()) < 1e-6
    st = timed({"kernels": ours, "torch": ref})
    for s in ("kernels", "torch"):
        lines.append(row(f"balanced cross entropy [{n}, {C}], value and gradient", s, st[s], n * (8 * C + 8), "logits in, gradient out, labels"))


def join_rows(n, H, lines):
    """The join at `join_graph`-like degree: every row has 0 .. 3 in-neighbours, drawn from all rows."""
    from analysisgnn_amd import cadence, fused, ops
    g = torch.Generator().manual_seed(n + H)
    dst = torch.repeat_interleave(torch.arange(n), torch.randint(0, 4, (n,), generator=g))
    src = torch.randint(0, n, (int(dst.numel()),), generator=g)
    src, dst = src.to(DEV), dst.to(DEV)
    x = torch.randn(n, H, generator=g).to(DEV).requires_grad_(True)
    cot = torch.randn(n, H, generator=g).to(DEV)
    ln = torch.nn.LayerNorm(H).to(DEV)
    ix = cadence.join_index(n, src, dst)
    spec = ops.AggSpec(fwd=[ix.by_dst], bwd=[ix.by_src], src_id=[0], n_rows=n, mean=True, shared_slot=True, skip_self=True, col_limit=n)
    leaves = [x, ln.weight, ln.bias]

    def ours():
        return torch.autograd.grad(cadence.pool_norm(x, src, dst, ln, n, n, True, index=ix), leaves, cot)

    def composition():
        return torch.autograd.grad(fused.norm_act(ops.aggregate(spec, [x], self_t=x), ln), leaves, cot)
    for a, b in zip(ours(), composition()):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), "the two sides disagree"
    st = timed({"kernel": ours, "composition": composition})
    deg = float(dst.numel()) / n
    # forward: x read (1 + deg) times, u and y written; backward: dy and u read, du written, du read (1 + deg) times, dx written
    nbytes = int(n * H * 4 * (2 * (1 + deg) + 6))
    for s in ("kernel", "composition"):
        lines.append(row(f"join [{n}, {H}], {deg:.2f} in-neighbours per row, value and gradient", s, st[s], nbytes,
                         "x and du read 1 + deg times; u, y, du, dx written; dy, u read"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    lines = []
    loss_rows(16000, 5, lines)
    join_rows(16000, 128, lines)
    join_rows(16000, 256, lines)
    head = [f"{torch.cuda.get_device_name(0)}; WARMUP {WARMUP}, ITERS {ITERS}, sides alternating", "",
            "| call | side | median µs | p10 .. p90 µs | bytes | floor at 8 TB/s, µs |", "|---|---|---|---|---|---|"]
    text = "\n".join(head + lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
