#!/usr/bin/env python
"""Time GraphNorm on the HIP kernels against its torch composition, on one GPU, same inputs, one process; and one training step of
`PitchSpellingGNN(add_seq=True)` with its GraphNorm on either.

  operator  `pitch_spelling.graph_norm` (csrc/graphnorm.hip) on [16000, 64] in 32 graphs, [10000, 64] in one graph (the reference's
            test loader: subgraph_size 10000, batch_size 1) and [16000, 256] in 32 graphs, against the composition PyG's GraphNorm
            is: two `index_add_` scatter-means, two gathers, the element-wise passes (`batch_size` given: no `batch.max()` read).
            The index (ours: one CSR build and the slab table; torch: the batch vector and the counts) is built outside the timing.
  step      `PitchSpellingGNN(in 64, n_hidden 256, enc 64, add_seq=True)`, 32 graphs x 500 notes, dropout 0.5: forward,
            `pitch_spelling_loss`, backward; `normalize` on the kernels, then replaced by a module that runs the composition.
Forward and backward are timed separately for the operator; a forward builds its autograd graph, a backward is
`torch.autograd.grad` on a retained graph.  Protocol: hipEvent pairs around every call, WARMUP untimed iterations, ITERS timed
ones, the sides alternating iteration by iteration; median and p10 / p90 in microseconds.  The share of 8 TB/s uses ALGORITHMIC
bytes: forward 12 per element (x twice, y once), backward 20 (x and dy twice, dx once).

KERNEL times come from a run of their own under the profiler, one shape per process (the k_gn_* rows of its kernel statistics):
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python scripts/time_pitch_spelling.py --kernels n,C,G
which runs 20 untimed and 200 counted forward + backward calls of the operator alone; `--report DIR n,C,G` then prints each
kernel's average and the calls' sums against the 12 and 20 bytes per element.

    python scripts/time_pitch_spelling.py [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, ITERS = 20, 200
DEV = "cuda:0"
HBM = 8e12
EPS = 1e-5


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


def composition(x, weight, bias, mean_scale, batch, inv_cnt, G):
    """torch_geometric.nn.GraphNorm.forward, with scatter-mean written as index_add_ times the reciprocal counts."""
    mean = torch.zeros(G, x.shape[1], device=x.device).index_add_(0, batch, x) * inv_cnt
    out = x - mean.index_select(0, batch) * mean_scale
    var = torch.zeros(G, x.shape[1], device=x.device).index_add_(0, batch, out * out) * inv_cnt
    return weight * out / (var + EPS).sqrt().index_select(0, batch) + bias


class CompositionNorm(nn.Module):
    def __init__(self, like, G):
        super().__init__()
        self.weight, self.bias, self.mean_scale, self.G = like.weight, like.bias, like.mean_scale, G

    def forward(self, x, batch=None, batch_size=None):
        inv = 1.0 / torch.bincount(batch, minlength=self.G).clamp(min=1).float().unsqueeze(1)
        return composition(x, self.weight, self.bias, self.mean_scale, batch, inv, self.G)


def row(what, side, stat, nbytes, note):
    med, lo, hi = stat
    share = f"{nbytes / (med * 1e-6) / HBM:.3f}" if nbytes else "-"
    size = f"{nbytes / 1e6:.1f} MB ({note})" if nbytes else note
    return f"| {what} | {side} | {med:.1f} | {lo:.1f} .. {hi:.1f} | {size} | {share} |"


def operator_rows(n, C, G, lines, tag=""):
    from analysisgnn_amd import pitch_spelling as ps
    g = torch.Generator().manual_seed(C + G)
    batch = torch.arange(n, device=DEV) * G // n                                           # G graphs of n / G rows, sorted
    x = torch.randn(n, C, generator=g).to(DEV).requires_grad_(True)
    w, b, ms = [(1 + 0.1 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True) for _ in range(3)]
    dy = torch.randn(n, C, generator=g).to(DEV)
    seg = ps.graph_segments(batch, G)
    inv = 1.0 / torch.bincount(batch, minlength=G).clamp(min=1).float().unsqueeze(1)
    ours = lambda: ps.graph_norm(x, w, b, ms, seg, EPS)                                     # noqa: E731
    ref = lambda: composition(x, w, b, ms, batch, inv, G)                                   # noqa: E731
    yo, yr = ours(), ref()
    assert float((yo - yr).detach().abs().max()) < 1e-4
    fwd = timed({"kernels": ours, "torch": ref})
    bwd = timed({"kernels": lambda: torch.autograd.grad(yo, [x, w, b, ms], dy, retain_graph=True),
                 "torch": lambda: torch.autograd.grad(yr, [x, w, b, ms], dy, retain_graph=True)})
    el = n * C
    for side in ("kernels", "torch"):
        lines.append(row(f"forward [{n}, {C}], {G} graph(s){tag}", side, fwd[side], 12 * el, "x twice, y once"))
    for side in ("kernels", "torch"):
        lines.append(row(f"backward [{n}, {C}], {G} graph(s){tag}", side, bwd[side], 20 * el, "x and dy twice, dx once"))


def step_rows(lines):
    from analysisgnn_amd import pitch_spelling as ps
    from analysisgnn_amd.synth import make_batch
    G, notes, in_feats = 32, 500, 64
    b = make_batch(G, notes)
    ets = list(b.edge_index.keys())
    n = b.num_nodes["note"]
    gen = torch.Generator().manual_seed(3)
    x_dict = {"note": torch.randn(n, in_feats, generator=gen).to(DEV)}
    ei = {et: torch.from_numpy(b.edge_index[et]).to(DEV) for et in ets}
    batch = torch.from_numpy(b.batch["note"]).to(DEV)
    labels = torch.stack([torch.randint(0, 35, (n,), generator=gen), torch.randint(0, 15, (n,), generator=gen)]).to(DEV)
    torch.manual_seed(0)
    model = ps.PitchSpellingGNN(in_feats, 256, 64, 35, 15, 2, (["note"], ets), dropout=0.5, add_seq=True).to(DEV).train()
    kernels, comp = model.normalize, CompositionNorm(model.normalize, G)
    lens = [notes] * G

    def step(norm):
        def run():
            model.normalize = norm
            for p in model.parameters():
                p.grad = None
            logits, offs = model.forward_fused(x_dict, ei, None, None, batch, lengths=lens)
            ps.pitch_spelling_loss(logits, offs, labels).backward()
        return run
    st = timed({"kernels": step(kernels), "torch": step(comp)}, iters=50)
    model.normalize = kernels
    for side in ("kernels", "torch"):
        lines.append(row(f"training step, n_hidden 256, {G} x {notes} notes", side, st[side], 0, "whole step: GraphNorm on this side"))


FWD_KERNELS, BWD_KERNELS = ("k_gn_stats", "k_gn_join", "k_gn_apply"), ("k_gn_bwd_sums", "k_gn_bwd_join", "k_gn_bwd_apply")


def kernels_only(n, C, G):
    """The operator alone, for a profiler: WARMUP + ITERS forward + backward calls."""
    from analysisgnn_amd import pitch_spelling as ps
    g = torch.Generator().manual_seed(C + G)
    batch = torch.arange(n, device=DEV) * G // n
    x = torch.randn(n, C, generator=g).to(DEV).requires_grad_(True)
    w, b, ms = [(1 + 0.1 * torch.randn(C, generator=g)).to(DEV).requires_grad_(True) for _ in range(3)]
    dy = torch.randn(n, C, generator=g).to(DEV)
    seg = ps.graph_segments(batch, G)
    for _ in range(WARMUP + ITERS):
        torch.autograd.grad(ps.graph_norm(x, w, b, ms, seg, EPS), [x, w, b, ms], dy)
    torch.cuda.synchronize()


def report(directory, n, C, G):
    """Average nanoseconds per kernel from the profiler's kernel statistics under `directory`, as markdown rows."""
    import csv
    import glob
    avg = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                for k in FWD_KERNELS + BWD_KERNELS:
                    if k + "(" in r["Name"]:
                        avg[k] = (float(r["AverageNs"]), int(r["Calls"]))
    el = n * C
    for what, names, per in (("forward", FWD_KERNELS, 12), ("backward", BWD_KERNELS, 20)):
        us = [avg[k][0] / 1e3 for k in names]
        total = sum(us)
        print(f"| {what} [{n}, {C}], {G} graph(s) | " + " + ".join(f"{u:.1f}" for u in us) + f" = {total:.1f} | {avg[names[0]][1]} | "
              f"{per * el / 1e6:.1f} MB | {per * el / (total * 1e-6) / HBM:.3f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--kernels", help="n,C,G: run the operator alone (under rocprofv3)")
    ap.add_argument("--report", nargs=2, metavar=("DIR", "n,C,G"), help="print the kernel rows of a profiler run")
    args = ap.parse_args()
    if args.report:
        return report(args.report[0], *[int(v) for v in args.report[1].split(",")])
    assert torch.cuda.is_available()
    if args.kernels:
        return kernels_only(*[int(v) for v in args.kernels.split(",")])
    lines = []
    operator_rows(16000, 64, 32, lines)
    operator_rows(10000, 64, 1, lines)
    operator_rows(16000, 256, 32, lines)
    operator_rows(16000, 64, 32, lines, " (again: the first shape, measured last)")
    step_rows(lines)
    head = [f"{torch.cuda.get_device_name(0)}; WARMUP {WARMUP}, ITERS {ITERS} (step: 50), sides alternating", "",
            "| call | side | median µs | p10 .. p90 µs | algorithmic bytes | share of 8 TB/s |", "|---|---|---|---|---|---|"]
    text = "\n".join(head + lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
