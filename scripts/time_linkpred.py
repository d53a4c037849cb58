#!/usr/bin/env python
"""Time the link-prediction operator of the pretraining stage (csrc/linkpred.hip through analysisgnn_amd/pretrain.py) against the
reference's operator sequence written with torch ops, on one GPU, same inputs, one process.

Shape: C3 — 32 subgraphs x 500 notes with beats and measures (bench.build_workload("c3")), H = 256, staff candidates =
cat(onset, consecutive) and voice candidates = consecutive, true relations from `synth.add_staff_voice`.  Both link tasks go
out together on either side.

Sides
  kernels   `link_bce(plans, feats)`: one agnn_link_bce_fwd_f32 call (two kernels: candidates, final pass) for both tasks;
            backward one agnn_link_bce_bwd_f32 call plus the [2]-sized scale product
  torch     per task index_select x 2, multiply, row sum, BCEWithLogitsLoss on float labels; backward through autograd
            (index_add_ with float atomics for both endpoint gathers).  Candidates and labels are handed over ready-made: the
            reference's mask compactions, isin over Cantor keys and argsort (each with a host read) are NOT timed.
Protocol: hipEvent pairs around every call, WARMUP untimed iterations, ITERS timed ones, the sides alternating iteration by
iteration; median and p10 / p90 per figure.  On both sides the forward builds its autograd graph (`requires_grad` inputs); the
backward is `torch.autograd.grad` on a retained graph.

The forward's share of the HBM roofline uses ALGORITHMIC bytes per task, two models: gather 8 H E (both rows of every
candidate) and compulsory 4 H n_unique (every distinct row once), each plus 16 E of indices and 9 E of outputs.

Also reported: the eager step time of `pretrain_objective` + backward at the same shape (PreEncoder, L = 3, heads = 4, dropout
0.3, inputs already H wide), to set beside bench.py's C3 figure (a different model and objective: 21 heads, hipGraph replay).

    python scripts/time_linkpred.py [--out profiles/linkpred.md]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, ITERS = 20, 200
DEV = "cuda:0"
H = 256


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
        us = sorted(1e3 * a.elapsed_time(b) for a, b in ev[k])
        out[k] = (statistics.median(us), us[int(0.1 * (ITERS - 1))], us[int(0.9 * (ITERS - 1))])
    return out


def count_launches(fn) -> str:
    """Device kernels of one call, from torch's profiler (a run of its own, not timed); 'not counted' if it is unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type.name in ("CUDA", "PrivateUse1") and not e.name.lower().startswith(("memcpy", "memset")))
        return str(n) if n else "not counted"
    except Exception as exc:        # noqa: BLE001
        return f"not counted ({type(exc).__name__})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--no-step", action="store_true", help="leave out the pretrain_objective step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_linkpred.py measures on a HIP device; none found")
    import bench
    from analysisgnn_amd.pretrain import PreEncoder, STAFF, VOICE, link_bce, link_candidates, link_plans, pretrain_objective
    from analysisgnn_amd.synth import add_staff_voice, torch_inputs
    g, _, hid, layers, _ = bench.build_workload("c3", 0, 1)
    assert hid == H
    g = add_staff_voice(g, seed=1)
    n = g.num_nodes["note"]
    I = torch_inputs(g, H, DEV, seed=0)
    ei = I["edge_index_dict"]
    cands = link_candidates(ei)
    trues = (ei[STAFF], ei[VOICE])
    plans = link_plans(list(zip(cands, trues)), n, n)
    gen = torch.Generator().manual_seed(0)
    feats = [(torch.randn(n, H, generator=gen) * H ** -0.25).to(DEV).requires_grad_(True) for _ in range(2)]
    w = torch.tensor([1.0, 1.0], device=DEV)

    # the torch side's ready-made inputs (and the agreement of the two sides before anything is timed)
    info = {}
    loss_k = link_bce(plans, feats, info)
    labels = [l.float() for l in info["labels"]]
    src = [c[0].contiguous() for c in cands]
    dst = [c[1].contiguous() for c in cands]

    def torch_fwd():
        out = []
        for k in range(2):
            x = (feats[k].index_select(0, src[k]) * feats[k].index_select(0, dst[k])).sum(-1)
            out.append(F.binary_cross_entropy_with_logits(x, labels[k]))
        return torch.stack(out)
    loss_t = torch_fwd()
    assert torch.allclose(loss_k, loss_t, rtol=1e-5, atol=1e-6), (loss_k, loss_t)
    gk = torch.autograd.grad((loss_k * w).sum(), feats, retain_graph=True)
    gt = torch.autograd.grad((loss_t * w).sum(), feats, retain_graph=True)
    for a, b in zip(gk, gt):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), "the two sides disagree"

    E = [int(c.shape[1]) for c in cands]
    uniq = [int(torch.unique(c).numel()) for c in cands]
    b_gather = sum(8 * H * e + 25 * e for e in E)
    b_comp = sum(4 * H * u + 25 * e for e, u in zip(E, uniq))
    records = []

    def rec(**kw):
        records.append(kw)
        print(json.dumps(kw), flush=True)

    fwd = timed({"kernels": lambda: link_bce(plans, feats), "torch": torch_fwd})
    bwd = timed({"kernels": lambda: torch.autograd.grad((loss_k * w).sum(), feats, retain_graph=True),
                 "torch": lambda: torch.autograd.grad((loss_t * w).sum(), feats, retain_graph=True)})
    for what, res in (("forward", fwd), ("backward", bwd)):          # the times first: they do not depend on the profiler pass below
        for side, (med, p10, p90) in res.items():
            rec(what=what, side=side, us=med, us_p10=p10, us_p90=p90, iters=ITERS, warmup=WARMUP, n=n, H=H, E=E)
    launches = {("forward", "kernels"): count_launches(lambda: link_bce(plans, feats)), ("forward", "torch"): count_launches(torch_fwd),
                ("backward", "kernels"): count_launches(lambda: torch.autograd.grad((loss_k * w).sum(), feats, retain_graph=True)),
                ("backward", "torch"): count_launches(lambda: torch.autograd.grad((loss_t * w).sum(), feats, retain_graph=True))}
    rows = []
    for what, res in (("forward", fwd), ("backward", bwd)):
        for side in res:
            rec(what=what + " launches", side=side, launches=launches[(what, side)])
        k, t = res["kernels"], res["torch"]
        verdict = f"{t[0] / k[0]:.2f}x faster" if k[2] < t[1] else (f"{k[0] / t[0]:.2f}x SLOWER" if t[2] < k[1] else "p10 .. p90 overlap")
        rows.append([what, f"{k[0]:.1f} ({k[1]:.1f} .. {k[2]:.1f})", launches[(what, "kernels")], f"{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f})",
                     launches[(what, "torch")], verdict])
    t_f = fwd["kernels"][0] * 1e-6
    roof = dict(what="forward roofline (call time: both kernels, allocations and enqueue included)", bytes_gather=b_gather, bytes_compulsory=b_comp,
                frac_gather=b_gather / t_f / bench.HBM_PEAK, frac_compulsory=b_comp / t_f / bench.HBM_PEAK, n_unique=uniq)
    rec(**roof)
    cols = ["", "kernels us, median (p10 .. p90)", "launches", "torch us, median (p10 .. p90)", "launches", "kernels vs torch"]
    table = ["| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)] + ["| " + " | ".join(str(c) for c in r) + " |" for r in rows]
    text = "\n".join(table)
    text += (f"\n\nForward, algorithmic bytes over the call's median time against {bench.HBM_PEAK / 1e12:.0f} TB/s: gather model "
             f"{b_gather / 1e6:.1f} MB -> {100 * roof['frac_gather']:.1f} %; compulsory model {b_comp / 1e6:.1f} MB -> {100 * roof['frac_compulsory']:.1f} %.")

    if not args.no_step:
        md = (g.node_types, [et for et in g.edge_types if et not in (STAFF, VOICE)])
        torch.manual_seed(0)
        model = PreEncoder(md, H, H, layers, heads=4, dropout=0.3).to(DEV).train()

        def step():
            model.zero_grad(set_to_none=True)
            total, _ = pretrain_objective(model, I["x_dict"], ei, I["batch_dict"], I["batch_size"], None, None, I["key_signature"], I["pitch_spelling"])
            total.backward()
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        ms = []
        for _ in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        rec(what="pretrain_objective + backward, eager (plans and CSR builds inside the step, no optimizer)", ms=statistics.median(ms), ms_p10=ms[3], ms_p90=ms[26],
            iters=30, warmup=5, layers=layers, heads=4, dropout=0.3)
        text += (f"\n\n`pretrain_objective` + backward, eager, L = {layers}, heads = 4, dropout 0.3: {statistics.median(ms):.2f} ms "
                 f"(p10 {ms[3]:.2f}, p90 {ms[26]:.2f}; 30 steps after 5).")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"n = {n} notes, H = {H}, candidates staff / voice = {E[0]} / {E[1]}, distinct rows {uniq[0]} / {uniq[1]}; "
                    f"{torch.cuda.get_device_name(0)}; {ITERS} timed calls per figure after {WARMUP}, sides alternating call by call\n\n{text}\n\n"
                    + "\n".join(json.dumps(r) for r in records) + "\n")


if __name__ == "__main__":
    main()
