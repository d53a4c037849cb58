#!/usr/bin/env python
"""Device time of the scheduled optimizer step (agnn_adamw_sched_f32) beside the plain one (agnn_adamw_f32), on the flat size
of the model bench.py builds (its default workload).  A measurement, not a test:

    python scripts/time_adamw_sched.py [--windows 7] [--calls 200] [--out FILE.json]

One process, the entries ALTERNATED window by window after a warm-up; a window is `--calls` back-to-back calls between two
device events.  Reported per entry: the median over the windows (us per call) and the spread (max - min) of the windows.
  plain      agnn_adamw_f32
  sched      agnn_adamw_sched_f32, warm-up + cosine schedule, SWA off: the same 7 streams of 4n bytes
  snapshot   agnn_adamw_sched_f32 with SWA from step 0, period 1: every step is a snapshot step, 9 streams
Criterion: median(sched) - median(plain) <= spread(plain).  The snapshot ratio is printed next to 9/7."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_flat_size() -> int:
    """FlatAdamW.flat.numel() of bench.py's model (built on the CPU: only its layout is needed)."""
    import torch
    import bench
    from analysisgnn_amd import dp
    from analysisgnn_amd.heads import MultiTaskLoss
    from analysisgnn_amd.models import TorchAnalysisGNN
    g, enc, hid, layers, tasks = bench.build_workload("c2s", 0, 1)
    torch.manual_seed(0)
    model = TorchAnalysisGNN(g.metadata(), bench.IN_CH, hid, bench.OUT, tasks, layers, dropout=0.3, use_jk=False, logit_fusion=False,
                             encoder_type=enc)
    trainable = torch.nn.ModuleDict({"model": model, "clf_loss": MultiTaskLoss(list(tasks), requires_grad=True)})
    params, tight = dp.plan_parameters(trainable)
    sizes = [p.numel() for p in params]
    return dp._aligned_offsets(sizes, tight=[id(p) in tight for p in params])[-1]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--n", type=int, default=0, help="flat size (default: that of bench.py's model)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from analysisgnn_amd import _lib, dp
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    n = args.n or bench_flat_size()
    lib = _lib.load()
    gen = torch.Generator().manual_seed(0)
    ws_bytes = int(lib.agnn_adamw_sched_workspace_bytes())

    def buffers():
        p, g = torch.randn(n, generator=gen).to(dev), (torch.randn(n, generator=gen) * 1e-2).to(dev)
        return dict(p=p, g=g, m=torch.zeros_like(p), v=torch.zeros_like(p), avg=torch.zeros_like(p), t=torch.zeros(1, device=dev),
                    norm=torch.zeros(1, device=dev), state=torch.zeros(2, device=dev),
                    ws=torch.empty(ws_bytes, dtype=torch.uint8, device=dev))

    sched = dp.LRSchedule.reference_cosine(5e-3, 500, 50, eta_min=5e-5)
    structs = {"sched": sched.struct(), "snapshot": sched.struct(dp.SWA(0, 1, anneal_epochs=10, swa_lr=5e-5))}
    bufs = {k: buffers() for k in ("plain", "sched", "snapshot")}
    stream = _lib.stream_ptr(dev)

    def call(kind):
        b = bufs[kind]
        if kind == "plain":
            rc = lib.agnn_adamw_f32(b["p"].data_ptr(), b["g"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), n, 5e-4, 0.9, 0.999, 1e-8,
                                    5e-3, 1.0, b["t"].data_ptr(), b["norm"].data_ptr(), 0, b["ws"].data_ptr(), ws_bytes, stream)
        else:
            rc = lib.agnn_adamw_sched_f32(b["p"].data_ptr(), b["g"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), n,
                                          ctypes.byref(structs[kind]), 0.9, 0.999, 1e-8, 5e-3, 1.0, b["t"].data_ptr(),
                                          b["avg"].data_ptr() if kind == "snapshot" else None, b["state"].data_ptr(),
                                          b["norm"].data_ptr(), 0, b["ws"].data_ptr(), ws_bytes, stream)
        _lib.check(rc, kind)

    def window(kind) -> float:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            call(kind)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.calls              # us per call

    kinds = ("plain", "sched", "snapshot")
    for kind in kinds:                                             # warm-up: code objects loaded, clocks up
        for _ in range(50):
            call(kind)
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for _ in range(args.windows):
        for kind in kinds:
            times[kind].append(window(kind))
    res = {"n": n, "calls_per_window": args.calls, "windows": args.windows, "device": torch.cuda.get_device_name(0)}
    for kind in kinds:
        res[kind] = {"median_us": statistics.median(times[kind]), "min_us": min(times[kind]), "max_us": max(times[kind]),
                     "spread_us": max(times[kind]) - min(times[kind]), "windows_us": [round(t, 3) for t in times[kind]]}
    res["sched_minus_plain_us"] = res["sched"]["median_us"] - res["plain"]["median_us"]
    res["within_plain_spread"] = res["sched_minus_plain_us"] <= res["plain"]["spread_us"]
    res["snapshot_over_sched"] = res["snapshot"]["median_us"] / res["sched"]["median_us"]
    res["streams_ratio"] = 9 / 7
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
