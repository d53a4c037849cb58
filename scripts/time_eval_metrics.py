"""The evaluation kernel at the C2 shape (N = 16 000 notes, the 21 heads of bench.TASK_DICT, sum C = 634) beside the torch-op
composition of the same counters, in one process:
  * the kernel alone: K = 20 `MultiTaskMetrics.update` launches captured back to back in one hipGraph, device events around
    every replay, time / K (no host launch gap inside the window)
  * one eager `update` call, and one eager torch composition (per task argmax, eq, sum, bincount x 3), each between its own
    pair of device events, the two alternating call by call: what a validation step that is not captured pays
2 s of GPU warm-up, 20 warm-up + 100 timed iterations per side, medians.  Prints the kernel's algorithmic bytes
(N sum C 4 + T N 8, + T N 4 with predictions) and what fraction of 8 TB/s they amount to over the kernel time.
usage: python scripts/time_eval_metrics.py [--out FILE]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from analysisgnn_amd.metrics import MultiTaskMetrics
from bench import HBM_PEAK, TASK_DICT

WARMUP, TIMED, N, K = 20, 100, 16000, 20


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_eval_metrics needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    a = torch.randn(4096, 4096, device=dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    while True:                                              # 2 s of work: clocks up before anything is timed
        for _ in range(20):
            a @ a
        t1.record()
        t1.synchronize()
        if t0.elapsed_time(t1) > 2000:
            break

    tasks, cs = list(TASK_DICT), list(TASK_DICT.values())
    offs = [0]
    for c in cs:
        offs.append(offs[-1] + c)
    T, C = len(cs), offs[-1]
    z = torch.randn(N, C, device=dev) * 2
    labels = torch.stack([torch.randint(0, c, (N,), device=dev) for c in cs])
    labels[torch.rand(T, N, device=dev) < 0.2] = -1
    m = MultiTaskMetrics(tasks, offs, device=dev)
    mp = MultiTaskMetrics(tasks, offs, device=dev)

    def hip():
        m.update(z, labels)

    def hip_pred():
        mp.update(z, labels, return_pred=True)

    def composed():
        out = []
        for t in range(T):
            y = labels[t]
            pred = z[:, offs[t]:offs[t + 1]].argmax(-1)
            valid = y != -1
            hit = pred.eq(y) & valid
            out.append((valid.sum(), hit.sum(), torch.bincount(pred[valid], minlength=cs[t]), torch.bincount(y[valid], minlength=cs[t]),
                        torch.bincount(y[hit], minlength=cs[t])))
        return out

    # the same counters from both sides, before anything is timed
    hip()
    ref = composed()
    cnt = m.counts.cpu()
    for t in range(T):
        v, h, n_pred, n_label, tp = (x.cpu() for x in ref[t])
        sl = slice(4 * T + 4 + offs[t], 4 * T + 4 + offs[t + 1])
        assert int(cnt[t]) == int(v) and int(cnt[T + t]) == int(h)
        assert torch.equal(cnt[sl], tp) and torch.equal(cnt[C:][sl], n_pred) and torch.equal(cnt[2 * C:][sl], n_label)

    graphs = {}
    for name, fn in (("kernel", hip), ("kernel+pred", hip_pred)):
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(K):
                fn()
        graphs[name] = g
    times = {k: [] for k in ("kernel", "kernel+pred", "update (eager)", "torch composition (eager)")}
    for i in range(WARMUP + TIMED):
        for name, fn, div in (("kernel", graphs["kernel"].replay, K), ("kernel+pred", graphs["kernel+pred"].replay, K),
                              ("update (eager)", hip, 1), ("torch composition (eager)", composed, 1)):
            us = timed(fn) / div
            if i >= WARMUP:
                times[name].append(us)
    nbytes = {"kernel": N * C * 4 + T * N * 8, "kernel+pred": N * C * 4 + T * N * 8 + T * N * 4}
    lines = [f"N = {N}, T = {T}, sum C = {C}; {WARMUP} warm-up + {TIMED} timed iterations per side; median (min .. max) in microseconds"]
    for name, v in times.items():
        med = statistics.median(v)
        line = f"{name}: {med:.1f} ({min(v):.1f} .. {max(v):.1f})"
        if name in nbytes:
            line += f"; {nbytes[name] / 1e6:.2f} MB algorithmic -> {nbytes[name] / (med * 1e-6) / 1e12:.2f} TB/s = {nbytes[name] / (med * 1e-6) / HBM_PEAK:.3f} of 8 TB/s"
        lines.append(line)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
