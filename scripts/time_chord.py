#!/usr/bin/env python
"""Time the two kernels of the ChordGNN model against their torch compositions, on one GPU, same inputs, one process.

Shape: `n_hidden = 256`, the reference's 14 default tasks (models/chord.py:606-609), 32 `synth` graphs of 500 notes: N = 16 000
notes, K = the distinct onsets per graph (`unique_onsets`), the onset edge list of `synth` (self loops included), dropout 0.5.

  block    `chord.colnorm` (csrc/colnorm.hip: ReLU -> BatchNorm1d, batch statistics, running statistics updated -> dropout) on the
           stacked heads' matrix [K, 14 * 256] and on one projection's [K, 256], against
           `F.dropout(F.batch_norm(F.relu(x), rm, rv, gamma, beta, True, 0.1, 1e-5), 0.5, True)`
  pool     `chord.onset_pool` (csrc/onsetpool.hip) on [N, 256] against the literal composition of models/chord.py:284-287 without
           its Linear: `zeros.index_add_(0, cat(dst, arange), a[cat(src, arange)]) / count`, then `[idx]`.  The index structures
           (ours: one CSR build; torch: the concatenated index vectors and the counts) are built once, outside the timing.
Forward and backward are timed separately; a forward builds its autograd graph, a backward is `torch.autograd.grad` on a retained
graph.  Protocol: hipEvent pairs around every call, WARMUP untimed iterations, ITERS timed ones, the sides alternating iteration
by iteration; median and p10 / p90 in microseconds.  The share of 8 TB/s uses ALGORITHMIC bytes, written out per row.

    python scripts/time_chord.py [--out FILE]
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
H, TASKS, P_DROP = 256, 14, 0.5
HBM = 8e12


def timed(sides: dict) -> dict:
    """{name: (median, p10, p90) in microseconds} of the callables, alternating, one event pair per call."""
    for _ in range(WARMUP):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)] for k in sides}
    for i in range(ITERS):
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
    return f"| {what} | {side} | {med:.1f} | {lo:.1f} .. {hi:.1f} | {nbytes / 1e6:.1f} MB ({note}) | {nbytes / (med * 1e-6) / HBM:.3f} |"


def block_rows(K, C, lines):
    from analysisgnn_amd import chord
    g = torch.Generator().manual_seed(C)
    x = torch.randn(K, C, generator=g).to(DEV).requires_grad_(True)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True)
    dy = torch.randn(K, C, generator=g).to(DEV)
    run = [torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)]
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    ours = lambda: chord.colnorm(x, gamma, beta, tuple(run), 1e-5, 0.1, True, P_DROP, True)                      # noqa: E731
    ref = lambda: F.dropout(F.batch_norm(F.relu(x), rm, rv, gamma, beta, True, 0.1, 1e-5), P_DROP, True)         # noqa: E731
    yo, yr = ours(), ref()
    fwd = timed({"kernels": ours, "torch": ref})
    bwd = timed({"kernels": lambda: torch.autograd.grad(yo, [x, gamma, beta], dy, retain_graph=True),
                 "torch": lambda: torch.autograd.grad(yr, [x, gamma, beta], dy, retain_graph=True)})
    el = K * C
    for side in ("kernels", "torch"):
        lines.append(row(f"block forward [{K}, {C}]", side, fwd[side], 12 * el, "x twice, y once"))
    for side in ("kernels", "torch"):
        lines.append(row(f"block backward [{K}, {C}]", side, bwd[side], 20 * el, "x and dy twice, dx once"))


def pool_rows(lines):
    from analysisgnn_amd import chord
    from analysisgnn_amd.synth import make_batch
    b = make_batch(32, 500)
    n = b.num_nodes["note"]
    ei = torch.from_numpy(b.edge_index[("note", "onset", "note")]).to(DEV)
    key = torch.from_numpy(b.batch["note"] * (int(b.onset_div.max()) + 1) + b.onset_div).to(DEV)
    idx = chord.unique_onsets(key)
    K, E = int(idx.numel()), int(ei.shape[1])
    g = torch.Generator().manual_seed(1)
    a = torch.randn(n, H, generator=g).to(DEV).requires_grad_(True)
    cot = torch.randn(K, H, generator=g).to(DEV)
    loops = torch.arange(n, device=DEV)
    src, dst = torch.cat([ei[0], loops]), torch.cat([ei[1], loops])
    cnt = torch.bincount(dst, minlength=n).float().unsqueeze(1)
    into = int(torch.isin(ei[1], idx).sum())
    ours = lambda: chord.onset_pool(a, ei, idx)                                                                   # noqa: E731
    ref = lambda: (torch.zeros_like(a).index_add_(0, dst, a[src]) / cnt)[idx]                                     # noqa: E731
    yo, yr = ours(), ref()
    assert float((yo - yr).detach().abs().max()) < 1e-5
    fwd = timed({"kernels": ours, "torch": ref})
    bwd = timed({"kernels": lambda: torch.autograd.grad(yo, [a], cot, retain_graph=True),
                 "torch": lambda: torch.autograd.grad(yr, [a], cot, retain_graph=True)})
    fb = 4 * H * (K + into + K)
    bb = 4 * H * (K + into + n)
    shape = f"N = {n}, K = {K}, E = {E}, {into} edges into selected rows"
    for side in ("kernels", "torch"):
        lines.append(row("pool forward, H = 256", side, fwd[side], fb, "K + edges into selected rows read, K rows written"))
    for side in ("kernels", "torch"):
        lines.append(row("pool backward, H = 256", side, bwd[side], bb, "a row of g per member read, N rows written"))
    return shape, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    lines = []
    shape, K = pool_rows(lines)
    block_rows(K, TASKS * H, lines)
    block_rows(K, H, lines)
    head = [f"{torch.cuda.get_device_name(0)}; {shape}; WARMUP {WARMUP}, ITERS {ITERS}, sides alternating", "",
            "| call | side | median µs | p10 .. p90 µs | algorithmic bytes | share of 8 TB/s |", "|---|---|---|---|---|---|"]
    text = "\n".join(head + lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
