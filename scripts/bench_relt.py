#!/usr/bin/env python3
"""Timing of the HGT relation-transform kernels (agnn_relt_fwd / _bwd / _dw), K and V in one launch, beside the torch.einsum
expressions `hgt._relt` ran at D != 64 before the kernels took every head width.  Defaults: the C3 shape, N = 16 000 source
rows, 6 relations, 4 heads, D = 64 (6.3 GFLOP per call).  HIP events around hipGraph replays of 10 back-to-back launches (as
bench.py times its roofline kernel); the two arms ALTERNATE replay by replay in one process, the median of 12 replays each is
reported, and the spread of an arm is (max - min) / median over its own replays.

Bounds per call (two items), for N rows, R relations, H = heads * D:
    FLOP  = 2 * 2 N R H D                                        against the fp32-MFMA peak (157.3 TFLOP/s)
    bytes = 2 * (4 N H (1 + R) + 4 R heads D^2)  [+ slab: dw]    against the measured HBM copy rate (6.2 TB/s)
usage: bench_relt.py [N] [R] [heads] [D]        (D = "all": every head width)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from analysisgnn_amd import _lib  # noqa: E402
from analysisgnn_amd.hgt import HEAD_WIDTHS  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 6
heads = int(sys.argv[3]) if len(sys.argv) > 3 else 4
widths = [64] if len(sys.argv) <= 4 else list(HEAD_WIDTHS) if sys.argv[4] == "all" else [int(sys.argv[4])]
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 6.2e12
REPLAYS, LAUNCHES = 12, 10
dev = torch.device("cuda:0")
lib = _lib.load()


def items(triples):
    arr = (_lib.ReltItem * len(triples))()
    for it, (x, w, y, ldx, ldy) in zip(arr, triples):
        it.x, it.w, it.y, it.ld_x, it.ld_y = x.data_ptr(), w.data_ptr(), y.data_ptr(), ldx, ldy
    return arr


def graph_of(fn):
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            fn()
    return g


def replay_us(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); g.replay(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / LAUNCHES


def bench(D):
    H = heads * D
    kqv = torch.randn(N, 3 * H, device=dev)
    k, v = kqv[:, :H], kqv[:, 2 * H:]
    Wk, Wv = torch.randn(R * heads, D, D, device=dev) * 0.1, torch.randn(R * heads, D, D, device=dev) * 0.1
    yk, yv = torch.randn(N, R * H, device=dev), torch.randn(N, R * H, device=dev)
    dk, dv = torch.empty(N, H, device=dev), torch.empty(N, H, device=dev)
    dWk, dWv = torch.empty_like(Wk), torch.empty_like(Wv)
    nws = int(lib.agnn_relt_dw_workspace_bytes(2, R, heads, D, N))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    I_f = items([(k, Wk, yk, k.stride(0), yk.stride(0)), (v, Wv, yv, v.stride(0), yv.stride(0))])
    I_b = items([(yk, Wk, dk, yk.stride(0), dk.stride(0)), (yv, Wv, dv, yv.stride(0), dv.stride(0))])
    I_w = items([(k, yk, dWk, k.stride(0), yk.stride(0)), (v, yv, dWv, v.stride(0), yv.stride(0))])
    st = lambda: _lib.stream_ptr(dev)      # noqa: E731
    kernels = {"fwd": lambda: _lib.check(lib.agnn_relt_fwd_f32(2, I_f, R, heads, D, N, st()), "f"),
               "bwd": lambda: _lib.check(lib.agnn_relt_bwd_f32(2, I_b, R, heads, D, N, st()), "b"),
               "dw": lambda: _lib.check(lib.agnn_relt_dw_f32(2, I_w, R, heads, D, N, ws.data_ptr(), nws, st()), "w")}

    def einsum(op, its):                   # the torch path `hgt._relt` had at D != 64, verbatim
        for a, b, y in its:
            if op == "fwd":
                y.view(N, R, heads, D).copy_(torch.einsum("nhi,rhij->nrhj", a.view(N, heads, D), b.view(R, heads, D, D)))
            elif op == "bwd":
                y.view(N, heads, D).copy_(torch.einsum("nrhi,rhij->nhj", a.view(N, R, heads, D), b.view(R, heads, D, D)))
            else:
                y.view(R, heads, D, D).copy_(torch.einsum("nhi,nrhj->rhij", a.view(N, heads, D), b.view(N, R, heads, D)))
    torch_arm = {"fwd": lambda: einsum("fwd", ((k, Wk, yk), (v, Wv, yv))),          # the same tensors: the column views k and v
                 "bwd": lambda: einsum("bwd", ((yk, Wk, dk), (yv, Wv, dv))),
                 "dw": lambda: einsum("dw", ((k, yk, dWk), (v, yv, dWv)))}
    flops = 2.0 * 2 * N * R * H * D
    base_bytes = 2.0 * (4.0 * N * H * (1 + R) + 4.0 * R * heads * D * D)
    for name in ("fwd", "bwd", "dw"):
        nbytes = base_bytes + (2.0 * (nws - 256) if name == "dw" else 0.0)     # the slab is written and read back once
        t_flop, t_byte = flops / PEAK_FLOPS * 1e6, nbytes / PEAK_BYTES * 1e6
        gk, gt = graph_of(kernels[name]), graph_of(torch_arm[name])
        tk, tt = [], []
        for _ in range(REPLAYS + 2):
            tk.append(replay_us(gk))
            tt.append(replay_us(gt))
        tk, tt = tk[2:], tt[2:]
        mk, mt = statistics.median(tk), statistics.median(tt)
        bound, which = max(t_flop, t_byte), "mfma" if t_flop >= t_byte else "hbm"
        print(f"D={D:3d} {name:3s}: kernel {mk:8.1f} us (spread {(max(tk) - min(tk)) / mk * 100:4.1f}%)  einsum {mt:8.1f} us "
              f"(spread {(max(tt) - min(tt)) / mt * 100:4.1f}%)  flop bound {t_flop:7.1f} us  byte bound {t_byte:7.1f} us  "
              f"binds {which}  share {bound / mk:5.2f}  ({flops / mk / 1e6:6.1f} TFLOP/s = {flops / mk / 1e6 / 157.3 * 100:3.0f}% of fp32 MFMA, "
              f"{nbytes / mk / 1e6:5.2f} TB/s = {nbytes / mk / 1e6 / 6.2 * 100:3.0f}% of HBM)  N={N} R={R} heads={heads}", flush=True)


for D in widths:
    bench(D)
