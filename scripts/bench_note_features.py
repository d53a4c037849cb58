"""Call time of the device note descriptors (analysisgnn_amd/descriptors.py) for both feature sets at one 500-note score, at the
trainer's batch (32 x 500 notes) and at one 10 000-note score (the reference's test `subgraph_size`): device events around every
call, 20 warm-up calls, 200 timed calls, median with p10 / p90.  `check=True` includes the one host read of the fault words,
`check=False` is the stream-ordered call alone.  The results at 500 and 32 x 500 notes are compared with tests/note_features_ref.py before they are timed
(the 10 000-note score is not: the numpy rules build N x N masks; tests/test_gpu_note_features.py compares 4 096 notes).
usage: python scripts/bench_note_features.py [--out FILE.json] [--once]      (--once: one call per shape, for a profiler run)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from analysisgnn_amd import synth
from analysisgnn_amd.descriptors import note_features

WARMUP, TIMED = 20, 200
FIELDS = ("onset_div", "duration_div", "pitch", "voice", "ts_beats", "is_downbeat", "onset_beat", "duration_beat")


def notes(seed, n):
    on, du = synth._note_times(seed, n)
    rng = np.random.default_rng(3000 + seed)
    pitch, voice = rng.integers(24, 100, n), rng.integers(1, 5, n)
    order = np.lexsort((pitch, on))
    on, du, pitch, voice = on[order], du[order], pitch[order], voice[order]
    ob = (on / 4 - 1).astype(np.float32)
    ts = np.full(n, 4, dtype=np.int64)
    return dict(onset_div=on, duration_div=du, pitch=pitch, voice=voice, ts_beats=ts, onset_beat=ob,
                is_downbeat=(np.remainder(ob.astype(np.float64), ts) == 0).astype(np.int64), duration_beat=(du / 4).astype(np.float32))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a HIP device is needed: nothing here is measured on a CPU"
    dev = torch.device("cuda:0")
    out = {}
    for name, n_scores, n_notes in (("1x500", 1, 500), ("32x500", 32, 500), ("1x10000", 1, 10000)):
        scores = [notes(sd, n_notes) for sd in range(n_scores)]
        z = {k: np.concatenate([s[k] for s in scores]) for k in FIELDS}
        f = {k: torch.from_numpy(v).to(dev) for k, v in z.items()}
        starts = torch.tensor([i * n_notes for i in range(n_scores + 1)], dtype=torch.int32, device=dev)
        res = {}
        for fs in ("voice", "cadence"):
            x = note_features(f, fs, starts)
            if a.once:
                torch.cuda.synchronize()
                continue
            if n_notes <= 500:
                import note_features_ref as R
                exp = R.note_features(z, fs, starts.cpu().numpy())
                g = x.cpu().numpy()
                assert np.array_equal(g[:, 2:], exp[:, 2:]) and np.abs(g[:, :2] - exp[:, :2]).max() <= 1e-6, (name, fs)
            out_buf = torch.empty_like(x)
            res[fs] = {"check=True": timed(lambda: note_features(f, fs, starts, out=out_buf)),
                       "check=False": timed(lambda: note_features(f, fs, starts, out=out_buf, check=False))}
        out[name] = res
        print(name, json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
