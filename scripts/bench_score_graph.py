"""Call time of the device score graph builder (analysisgnn_amd/score_graph.py) beside the numpy builder of `synth` on the same
box's CPU, at the trainer's batch (32 x 500 notes) and at one 10 000-note score (the reference's test `subgraph_size`), beats and
measures included:
  * `build_score_graph` with capacity=None (exact sizes: one host read of the totals inside the call) and with static capacities
    (no host read): device events around every call, 5 warm-up calls, 30 timed calls, median with p10 / p90;
  * `agnn_score_graph_fill` alone over a counted workspace, same protocol: the bytes it writes (16 per edge) over its time, as a
    fraction of the 8 TB/s HBM peak — the time is that of a call between events, launch included, not a kernel time;
  * `synth.make_score_graph` + `collate`: host clock, one run (N x N masks: seconds at 10 000 notes).
usage: python scripts/bench_score_graph.py [--out FILE.json] [--no-cpu]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from analysisgnn_amd import _lib, synth
from analysisgnn_amd.score_graph import build_score_graph

WARMUP, TIMED, HBM_PEAK = 5, 30, 8.0e12
KW = dict(add_beats=True, add_measures=True)
KEYS = (*synth.NOTE_RELATIONS, "beat", "measure")


def timed(fn):
    us = []
    for i in range(WARMUP + TIMED):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= WARMUP:
            us.append(e0.elapsed_time(e1) * 1e3)
    q = np.percentile(us, [50, 10, 90])
    return {"median_us": round(float(q[0]), 1), "p10_us": round(float(q[1]), 1), "p90_us": round(float(q[2]), 1)}


def fill_only(on, du, starts, totals):
    dev = on.device
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    n, S = int(on.numel()), len(starts) - 1
    start_dev = torch.tensor(starts, dtype=torch.int32, device=dev)
    tot = torch.zeros(4, dtype=torch.int64, device=dev)
    faults = torch.zeros(8, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.agnn_score_graph_workspace_bytes(n, S))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    bufs = [torch.empty((2, c), dtype=torch.int64, device=dev) for c in totals]
    g = _lib.ScoreGraphArgs()
    g.onset_div, g.duration_div, g.score_start, g.n_notes, g.n_scores = on.data_ptr(), du.data_ptr(), start_dev.data_ptr(), n, S
    g.flags, g.totals, g.faults = _lib.CONSTS["AGNN_SG_SELF_LOOPS"], tot.data_ptr(), faults.data_ptr()
    for r in range(4):
        g.edges[r], g.cap[r] = bufs[r].data_ptr(), totals[r]
    _lib.check(lib.agnn_score_graph_count(g, ws.data_ptr(), ws_bytes, st), "agnn_score_graph_count")
    t = timed(lambda: _lib.check(lib.agnn_score_graph_fill(g, ws.data_ptr(), ws_bytes, st), "agnn_score_graph_fill"))
    assert faults.tolist() == [0] * 8
    t["bytes_written"] = 16 * int(sum(totals))
    t["fraction_of_hbm_peak"] = round(t["bytes_written"] / (t["median_us"] * 1e-6) / HBM_PEAK, 5)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for name, n_scores, n_notes in (("32x500", 32, 500), ("1x10000", 1, 10000)):
        times = [synth._note_times(sd, n_notes) for sd in range(n_scores)]
        on = torch.from_numpy(np.concatenate([t[0] for t in times])).to(dev)
        du = torch.from_numpy(np.concatenate([t[1] for t in times])).to(dev)
        starts = [i * n_notes for i in range(n_scores + 1)]
        g = build_score_graph(on, du, starts, **KW)
        caps = dict(zip(KEYS, g.totals.tolist()))
        res = {"edges": {k: caps[k] for k in synth.NOTE_RELATIONS}, "beats": caps["beat"], "measures": caps["measure"]}
        res["exact"] = timed(lambda: build_score_graph(on, du, starts, **KW))
        res["static_capacity"] = timed(lambda: build_score_graph(on, du, starts, capacity=caps, **KW))
        res["fill_call"] = fill_only(on, du, starts, [caps[k] for k in synth.NOTE_RELATIONS])
        if not a.no_cpu:
            t0 = time.perf_counter()
            c = synth.collate([synth.make_score_graph(seed=sd, n_notes=n_notes, **KW) for sd in range(n_scores)])
            res["synth_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            for et, e in c.edge_index.items():
                assert np.array_equal(g.edge_index_dict[et].cpu().numpy(), e), et
        out[name] = res
        print(name, json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
