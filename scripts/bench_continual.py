"""The continual-learning terms at the C2 shape (N = 16 000 notes, the 21 heads of bench.TASK_DICT, tau = 2), each beside the
torch-op composition it replaces, in one process, alternating:
  * agnn_multitask_kd_f32 (forward launches, which finish the gradient)   vs   the per-task F.kl_div loop + its autograd backward
  * EWC.add_penalty_ on the model's flat buffers                          vs   the per-parameter EWC loop + its backward
Device events around every call: 2 s of GPU warm-up, 20 warm-up and 100 timed calls per side.  Also prints the algorithmic
bytes (KD: 4 N (2 sum C read + sum C written); EWC: 4 n 5) and what fraction of 8 TB/s they amount to over the measured time.
usage: python scripts/bench_continual.py [--out profiles/continual_terms.md]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from analysisgnn_amd import dp
from analysisgnn_amd.continual import EWC, distillation_loss
from analysisgnn_amd.models import TorchAnalysisGNN
from analysisgnn_amd.synth import make_batch
from bench import HBM_PEAK, TASK_DICT

WARMUP, TIMED, N, TAU, LAM_KD, LAM_EWC = 20, 100, 16000, 2.0, 0.5, 2.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "continual_terms.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_continual needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    a = torch.randn(4096, 4096, device=dev)
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    while True:                                              # 2 s of work: clocks up before anything is timed
        for _ in range(20):
            a @ a
        t1.record()
        t1.synchronize()
        if t0.elapsed_time(t1) > 2000:
            break

    # ---- distillation --------------------------------------------------------------------------------------------------------
    cs = list(TASK_DICT.values())
    offs = [0]
    for c in cs:
        offs.append(offs[-1] + c)
    T, C = len(cs), offs[-1]
    student = (torch.randn(N, C, device=dev) * 2).requires_grad_(True)
    teacher = student.detach() + torch.randn(N, C, device=dev)

    def kd_hip():
        return distillation_loss(student, teacher, offs, TAU, LAM_KD)[0]

    def kd_torch():
        student.grad = None
        terms = [F.kl_div(F.log_softmax(student[:, offs[i]:offs[i + 1]] / TAU, 1), F.softmax(teacher[:, offs[i]:offs[i + 1]] / TAU, 1),
                          reduction="batchmean") * TAU ** 2 for i in range(T)]
        total = LAM_KD * torch.stack(terms).mean()
        total.backward()
        return total
    th = kd_hip()
    g_hip = torch.autograd.grad(th, student)[0]
    tt = kd_torch()
    kd_diff = (float((th - tt).abs()), float((g_hip - student.grad).abs().max()), float(student.grad.abs().max()))
    kd = alternate({"hip": kd_hip, "torch": kd_torch})

    # ---- EWC -----------------------------------------------------------------------------------------------------------------
    g = make_batch(1, 60)
    model = TorchAnalysisGNN(g.metadata(), 25, 256, 128, TASK_DICT, 3, dropout=0.0, use_jk=False, logit_fusion=False).to(dev)
    params, tight = dp.plan_parameters(model)
    grads = dp.FlatGradBuffer(params, views=True, tight=tight)
    opt = dp.FlatAdamW(params, grads)
    ewc = EWC(opt)
    ewc.fisher.copy_(torch.rand_like(ewc.fisher))
    ewc.mean.copy_(opt.flat + 0.01 * torch.randn_like(opt.flat))
    n = opt.flat.numel()
    fisher, means = ewc.fisher_dict(model), ewc.means_dict(model)
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]

    def ewc_hip():
        return ewc.add_penalty_(LAM_EWC)

    def ewc_torch():                                         # gradients accumulate into the same flat buffer (views=True)
        pen = 0
        for k, p in named:
            pen = pen + (fisher[k] * (p - means[k]).pow(2)).sum()
        (LAM_EWC * pen).backward()
        return pen
    grads.flat.zero_()
    ph = float(ewc_hip())
    gh = grads.flat.clone()
    grads.flat.zero_()
    pt = float(ewc_torch())
    gdiff = max(float((gh[o:o + p.numel()] - p.grad.reshape(-1)).abs().max()) for p, o in zip(grads.params, grads.offsets))
    ewc_diff = (abs(ph - pt) / max(abs(pt), 1e-30), gdiff, float(gh.abs().max()))
    ew = alternate({"hip": ewc_hip, "torch": ewc_torch})

    def stat(v):
        return statistics.median(v), min(v), max(v)
    kd_bytes, ewc_bytes = 4 * N * 3 * C, 4 * n * 5
    lines = ["# Continual-learning terms: HIP kernels beside the torch compositions they replace", "",
             f"`python scripts/bench_continual.py` on one MI355X; device events around every call, 2 s GPU warm-up, {WARMUP} warm-up + {TIMED} "
             "timed calls per side, the two sides alternating call by call in one process.  Times are per call, host launch",
             "overhead included (what a step that is not captured into a graph pays); median (min .. max) in microseconds.", "",
             f"Shape: N = {N} rows, the {T} heads of `bench.TASK_DICT` (sum C = {C}), tau = {TAU}; EWC over the C2 model's flat buffers, n = {n} floats.", "",
             "| term | HIP path | torch composition | ratio (torch / HIP, medians) |", "|---|---|---|---|"]
    for name, tm, what_h, what_t in (("distillation", kd, "`distillation_loss` forward (finishes the gradient)", "per-task `F.kl_div` loop + autograd backward"),
                                     ("EWC", ew, "`EWC.add_penalty_`", "per-parameter loop + autograd backward")):
        h, t = stat(tm["hip"]), stat(tm["torch"])
        lines.append(f"| {name} | {what_h}: {h[0]:.1f} ({h[1]:.1f} .. {h[2]:.1f}) | {what_t}: {t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f}) | {t[0] / h[0]:.1f}x |")
    hk, he = stat(kd["hip"])[0], stat(ew["hip"])[0]
    lines += ["", "Algorithmic bytes over the measured call time (an end-to-end rate of the call, launches included — not a kernel's share of peak):", "",
              f"* distillation: 4 N (2 sum C read + sum C written) = {kd_bytes / 1e6:.1f} MB -> {kd_bytes / (hk * 1e-6) / 1e12:.2f} TB/s, "
              f"{100 * kd_bytes / (hk * 1e-6) / HBM_PEAK:.0f} % of 8 TB/s",
              f"* EWC: 4 n 5 = {ewc_bytes / 1e6:.1f} MB -> {ewc_bytes / (he * 1e-6) / 1e12:.2f} TB/s, {100 * ewc_bytes / (he * 1e-6) / HBM_PEAK:.0f} % of 8 TB/s",
              "", "Same inputs, both sides (fp32 sums in different orders):", "",
              f"* distillation: |total difference| {kd_diff[0]:.2e}, max |gradient difference| {kd_diff[1]:.2e} (max |gradient| {kd_diff[2]:.2e})",
              f"* EWC: relative penalty difference {ewc_diff[0]:.2e}, max |gradient difference| {ewc_diff[1]:.2e} (max |gradient| {ewc_diff[2]:.2e})", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
