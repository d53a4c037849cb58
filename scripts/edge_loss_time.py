"""The edge-consistency term at the trainer's shape (the C2 graph of `synth`: 32 x 500 notes, B = 16 000 targets, H = 128, the
four note-note relations, dropout 0.3), beside the same term composed from torch operators on the same device, in one process,
alternating call by call:
  * HIP path:  `edge_plan` (the random subset, the CSRs) + `edge_consistency_loss` + backward
  * HIP path with the plan built beforehand: `edge_consistency_loss` + backward alone (what a captured step replays)
  * baseline:  the reference's schedule (models/analysis.py:991-1019) from torch operators — boolean-mask compaction, `randperm`
               (on the device: the reference draws it on the CPU), two `index_select`s, the decoder's own `nn` modules on the
               gathered rows, `CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)` — + autograd backward
The baseline is never the code under test.  Device events around every call: 2 s of GPU warm-up, then warm-up and timed calls per
side; medians with p10 / p90.  Launch counts come from one profiled call per side (torch.profiler), after the timing.
usage: python scripts/edge_loss_time.py [--out profiles/edge_loss.md]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

from analysisgnn_amd import EdgeDecoder, edge_consistency_loss, edge_plan
from analysisgnn_amd.synth import make_batch

WARMUP, TIMED, N_GRAPHS, N_NOTES, H, P_DROP = 10, 60, 32, 500, 128, 0.3


def alternate(sides):
    """{name: [us per call]}: the sides take turns, one call each, every call between its own pair of device events."""
    times = {k: [] for k in sides}
    for i in range(WARMUP + TIMED):
        for name, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= WARMUP:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return times


def torch_term(dec, x, edge_index_dict, labels, batch_size, ce, kept=None):
    """:991-1019 from torch operators; `kept` (already selected edges) skips the compaction and the draw."""
    if kept is None:
        kept = {}
        for k, v in edge_index_dict.items():
            v = v[:, (v[0] < batch_size) & (v[1] < batch_size)]
            if v.size(1) > batch_size:
                v = v[:, torch.randperm(v.size(1), device=v.device)[:batch_size]]
            kept[k] = v
    total = 0
    for k, v in kept.items():
        y = (labels[:, v[0]] == labels[:, v[1]]).all(dim=0).long()
        emb = dec.embed[k[1]]
        f = emb(x.index_select(0, v[0])) * emb(x.index_select(0, v[1]))
        total = total + ce(dec.fc(f), y)
    return total / len(kept)


def count_launches(fn):
    """Device kernels of one call, or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as exc:                                  # noqa: BLE001
        print(f"launch count not available: {exc}")
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "edge_loss.md"))
    ap.add_argument("--no-profile", action="store_true", help="skip the launch counts")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "edge_loss_time needs a HIP device"
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

    g = make_batch(N_GRAPHS, N_NOTES)
    B = g.num_nodes["note"]
    ei = {et: torch.from_numpy(e.copy()).to(dev) for et, e in g.edge_index.items() if et[0] == "note" and et[2] == "note"}
    rels = [et[1] for et in ei]
    dec = EdgeDecoder(H, rels, dropout=P_DROP).to(dev).train()
    params = list(dec.parameters())
    x = torch.randn(B, H, device=dev).requires_grad_(True)
    seg = torch.arange(B, device=dev) // 6
    gen = torch.Generator().manual_seed(1)
    labels = torch.stack([torch.randint(0, 3, (B // 6 + 1,), generator=gen).to(dev)[seg // (1 + i % 2)] for i in range(5)]).long()
    ce = nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)

    def clear():
        x.grad = None
        for p in params:
            p.grad = None

    def hip():
        clear()
        plan = edge_plan(ei, B, relations=rels)
        loss, _ = edge_consistency_loss(dec, x, plan, labels)
        loss.backward()
        return loss

    fixed = edge_plan(ei, B, relations=rels)

    def hip_planned():                                       # the part a captured step replays: the plan exists beforehand
        clear()
        loss, _ = edge_consistency_loss(dec, x, fixed, labels)
        loss.backward()
        return loss

    def baseline():
        clear()
        loss = torch_term(dec, x, ei, labels, B, ce)
        loss.backward()
        return loss

    # the same selected edges through both, dropout off: the two compute the same term
    dec.eval()
    plan = edge_plan(ei, B, relations=rels)
    kept = {}
    for i, et in enumerate(plan.edge_types):
        s, d = plan.edges(i)
        ok = (s < B) & (d < B)
        kept[et] = torch.stack([s[ok], d[ok]])
    clear()
    lh, parts = edge_consistency_loss(dec, x, plan, labels)
    lh.backward()
    gh = x.grad.clone()
    clear()
    lt = torch_term(dec, x, None, labels, B, ce, kept=kept)
    lt.backward()
    diff = (float((lh - lt).detach().abs()), float(lt.detach()), float((gh - x.grad).abs().max()), float(x.grad.abs().max()))
    sizes = [(r, int(ei[et].shape[1]), int(n)) for r, et, n in zip(rels, plan.edge_types, parts["alive"].cpu().tolist())]
    dec.train()

    times = alternate({"hip": hip, "planned": hip_planned, "torch": baseline})

    def stat(v):
        q = statistics.quantiles(v, n=10)
        return statistics.median(v), q[0], q[-1]

    def emit(launches):
        h, t, hp = stat(times["hip"]), stat(times["torch"]), stat(times["planned"])
        fmt = lambda n: "not measured" if n is None else str(n)                                       # noqa: E731
        lines = ["# Edge-consistency term: HIP path beside the torch composition of the reference's schedule", "",
                 f"`python scripts/edge_loss_time.py` on one MI355X; device events around every call, 2 s GPU warm-up, {WARMUP} warm-up + {TIMED} "
                 "timed calls per side, the two sides alternating call by call in one process.  Times are per call, host launch overhead",
                 "and (baseline) host read-backs included — what an eager step pays; median (p10 .. p90) in microseconds.", "",
                 f"Shape: `synth.make_batch({N_GRAPHS}, {N_NOTES})`, B = {B} targets, H = {H}, dropout {P_DROP}, training mode, relations (edges, kept): "
                 + ", ".join(f"{r} ({e}, {k})" for r, e, k in sizes) + ".", "",
                 "| side | what is timed | time per call | device kernels per call |", "|---|---|---|---|",
                 f"| HIP path | `edge_plan` + `edge_consistency_loss` + backward | {h[0]:.0f} ({h[1]:.0f} .. {h[2]:.0f}) | {fmt(launches['hip'])} |",
                 f"| HIP path, plan built beforehand | `edge_consistency_loss` + backward | {hp[0]:.0f} ({hp[1]:.0f} .. {hp[2]:.0f}) | {fmt(launches.get('planned'))} |",
                 f"| torch composition | mask compaction, `randperm` (device), `index_select` x 2, `nn` modules on gathered rows, `CrossEntropyLoss`, "
                 f"autograd backward | {t[0]:.0f} ({t[1]:.0f} .. {t[2]:.0f}) | {fmt(launches['torch'])} |", "",
                 f"Ratio of the medians (torch / HIP): {t[0] / h[0]:.2f}x.", "",
                 "Same selected edges through both sides, dropout off (fp32 sums in different orders): "
                 f"|loss difference| {diff[0]:.2e} at loss {diff[1]:.4f}, max |x.grad difference| {diff[2]:.2e} at max |x.grad| {diff[3]:.2e}.", ""]
        text = "\n".join(lines)
        print(text)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)

    emit({"hip": None, "torch": None})                       # the times first: they stand whatever becomes of the profiled calls
    if not args.no_profile:
        emit({"hip": count_launches(hip), "planned": count_launches(hip_planned), "torch": count_launches(baseline)})


if __name__ == "__main__":
    main()
