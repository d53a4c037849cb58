"""The continual-learning terms (analysisgnn_amd/continual.py, csrc/continual.hip) against float64 torch on the CPU, written
from the formulas of include/agnn.h:
    kd[t] = tau^2 / N sum_n sum_c p (log p - log q),  total = w / T sum_t kd[t]          (p, q = softmax(teacher | student / tau))
    penalty = sum_i fisher_i (p_i - mean_i)^2,        g_i += 2 lambda fisher_i (p_i - mean_i)
Tolerances are the project's (as in test_gpu_heads.py): scalars and per-task losses 1e-4 by `assert_close`,
gradients 1e-4 of the tensor's own max|ref| by `assert_close_rel`; the weights are chosen so that max|ref| >= 1e-3 (asserted),
i.e. the bound is the 1e-4 term and not that helper's 1e-7 floor."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import assert_close, assert_close_rel  # noqa: E402

DEV = "cuda:0"
WIDTHS = [2, 15, 16, 17, 49, 185]        # the narrowest head, widths around one 16-lane pass, the reference's widest head


def _pairs(widths, start=0):
    out, a = [], start
    for c in widths:
        out.append((a, a + c))
        a += c
    return out


def kd_oracle(student, teacher, pairs, tau, w):
    """float64: (total, kd[T], d total / d student [N, C])."""
    s = student.detach().cpu().double().requires_grad_(True)
    t = teacher.detach().cpu().double()
    N = s.shape[0]
    kd = []
    for a, b in pairs:
        lq = F.log_softmax(s[:, a:b] / tau, 1)
        lp = F.log_softmax(t[:, a:b] / tau, 1)
        kd.append((F.softmax(t[:, a:b] / tau, 1) * (lp - lq)).sum() / N * tau ** 2)
    kd = torch.stack(kd)
    total = w * kd.mean()
    total.backward()
    return total.detach(), kd.detach(), s.grad


def _logits(N, C, seed, sliced):
    """(student, teacher) [N, C] on the device: column slices of wider matrices with different row strides (an odd and an even
    one, starting 12 and 8 bytes into the row), or contiguous."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(N, C, generator=g) * 2
    t = s + torch.randn(N, C, generator=g)
    if not sliced:
        return s.to(DEV), t.to(DEV)
    bs = torch.randn(N, C + 7, generator=g).to(DEV)
    bt = torch.randn(N, C + 6, generator=g).to(DEV)
    bs[:, 3:3 + C] = s.to(DEV)
    bt[:, 2:2 + C] = t.to(DEV)
    return bs[:, 3:3 + C], bt[:, 2:2 + C]


def _check_kd(student, teacher, offs, pairs, tau, w):
    from analysisgnn_amd.continual import distillation_loss
    s = student.detach().requires_grad_(True)
    total, kd = distillation_loss(s, teacher, offs, tau, w)
    total.backward()
    rt, rkd, rg = kd_oracle(student, teacher, pairs, tau, w)
    print(f"kd: total {float(total):.6g} ref {float(rt):.6g}; max|dstudent ref| {float(rg.abs().max()):.3g}, "
          f"err {float((s.grad.cpu().double() - rg).abs().max()):.3g}")
    assert float(rg.abs().max()) >= 1e-3
    assert_close(total, rt, 1e-4, "total")
    assert_close(kd, rkd, 1e-4, "per-task")
    assert_close_rel(s.grad, rg, 1e-4, "dstudent")
    assert not kd.requires_grad
    return total.detach(), kd, s.grad


@pytest.mark.parametrize("sliced", [True, False])
@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("N", [1, 3, 67, 300])
def test_kd_matches_float64(N, tau, sliced):
    """N = 1, 3: fewer rows than one wave's four; 67, 300: a ragged last wave and workgroup (8 rows each).  Student and teacher
    as column slices with different row strides (4-byte loads) and contiguous (even geometry: the 8-byte loads and stores)."""
    pairs = _pairs(WIDTHS)
    s, t = _logits(N, pairs[-1][1], 10 * N + int(tau), sliced)
    if sliced:
        assert s.stride(0) != t.stride(0) and (N == 1 or not s.is_contiguous())
    _check_kd(s, t, [0] + [b for _, b in pairs], pairs, tau, w=N * len(pairs) / 4.0)


def test_kd_rows_wider_than_the_lds_image():
    """1200 logit columns: beyond the 1024-column LDS image (k_kd_lds), the global-memory kernel gives the same results."""
    widths = WIDTHS * 4 + [64]
    pairs = _pairs(widths)
    assert pairs[-1][1] == 1200
    s, t = _logits(67, 1200, 5, sliced=True)
    _check_kd(s, t, [0] + [b for _, b in pairs], pairs, 2.0, w=67 * len(pairs) / 4.0)


@pytest.mark.parametrize("n_cols,pairs", [(70, [(4, 19), (40, 62)]), (1100, [(4, 19), (40, 62), (1000, 1090)])])
def test_kd_subset_of_heads_zeroes_uncovered_columns(n_cols, pairs):
    """The segments cover a subset of the columns; the gradient buffer arrives filled with NaN (it comes from torch.empty):
    every column below n_cols outside the segments is exactly 0, the rest matches the oracle, and nothing beyond n_cols is
    touched.  70 columns: the LDS kernel; 1100: the global-memory one."""
    from analysisgnn_amd import _lib
    from analysisgnn_amd.continual import _segment_tensors, _segments, distillation_loss
    N, tau, w = 67, 2.0, 67 * len(pairs) / 4.0
    s, t = _logits(N, n_cols, 3, sliced=False)
    starts, ends = _segments(pairs, n_cols)
    assert ends is not None
    seg_off, seg_end = _segment_tensors(starts, ends, torch.device(DEV))
    T = len(pairs)
    lib = _lib.load()
    ds = torch.full((N, n_cols + 2), float("nan"), device=DEV)
    out = torch.empty(T + 1, device=DEV)
    nws = int(lib.agnn_kd_workspace_bytes(N, T))
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    _lib.check(lib.agnn_multitask_kd_f32(s.data_ptr(), s.stride(0), t.data_ptr(), t.stride(0), seg_off.data_ptr(), seg_end.data_ptr(), T, N,
                                         n_cols, tau, w, ds.data_ptr(), ds.stride(0), out.data_ptr(), out[T:].data_ptr(), ws.data_ptr(), nws,
                                         _lib.stream_ptr(torch.device(DEV))), "agnn_multitask_kd_f32")
    rt, rkd, rg = kd_oracle(s, t, pairs, tau, w)
    covered = torch.zeros(n_cols, dtype=torch.bool)
    for a, b in pairs:
        covered[a:b] = True
    d = ds.cpu()
    assert torch.isnan(d[:, n_cols:]).all()
    assert (d[:, :n_cols][:, ~covered] == 0).all()
    assert float(rg.abs().max()) >= 1e-3
    assert_close_rel(d[:, :n_cols], rg, 1e-4, "dstudent")
    assert_close(out[:T], rkd, 1e-4, "per-task")
    assert_close(out[T], rt, 1e-4, "total")
    # the same through the public function
    sg = s.detach().requires_grad_(True)
    total, kd = distillation_loss(sg, t, pairs, tau, w)
    total.backward()
    assert torch.equal(sg.grad.cpu(), d[:, :n_cols]) and torch.equal(kd, out[:T])


@pytest.mark.parametrize("tau", [1.0, 2.0])
def test_kd_extremes(tau):
    """One teacher row spans 400 logit units inside a 15-wide segment: in fp32 p underflows to 0 for the lowest classes, and
    log p is formed as x / tau - lse, so those classes contribute exactly 0 (never 0 * inf).  Student == teacher: total,
    gradient and every kd[t] vanish to rounding."""
    from analysisgnn_amd.continual import distillation_loss
    N, offs, pairs = 5, [0, 15, 19], [(0, 15), (15, 19)]
    g = torch.Generator().manual_seed(7)
    s = torch.randn(N, 19, generator=g) * 2
    t = s + torch.randn(N, 19, generator=g)
    t[2, :15] = torch.linspace(-200.0, 200.0, 15)
    w = N * 2 / 4.0
    total, kd, grad = _check_kd(s.to(DEV), t.to(DEV), offs, pairs, tau, w)
    assert torch.isfinite(total) and torch.isfinite(kd).all() and torch.isfinite(grad).all()
    assert float(F.softmax(t[2, :15] / tau, 0)[0]) == 0.0          # the underflow this case is about
    same = t.to(DEV).requires_grad_(True)
    total, kd = distillation_loss(same, t.to(DEV), offs, tau, w)
    total.backward()
    print(f"student == teacher: total {float(total):.3g}, max|dstudent| {float(same.grad.abs().max()):.3g}, min kd {float(kd.min()):.3g}")
    assert abs(float(total)) <= 1e-6 * w
    assert float(same.grad.abs().max()) <= 1e-6 * w * tau / (N * 2)
    assert float(kd.min()) >= -1e-6


def test_kd_gradient_paths():
    """`backward(gradient=heads.unit_gradient(dev))` hands the finished gradient on without a launch (torch profiler: no kernel
    in the backward pass); bit for bit the general path with an incoming 1.0, within 1e-6 relative of it with 0.37; two
    identical calls give bit-identical total, kd and dstudent."""
    from analysisgnn_amd.continual import distillation_loss
    from analysisgnn_amd.heads import unit_gradient
    pairs = _pairs(WIDTHS)
    offs = [0] + [b for _, b in pairs]
    s, t = _logits(300, offs[-1], 11, sliced=False)

    def run(gradient):
        sg = s.detach().clone().requires_grad_(True)
        total, kd = distillation_loss(sg, t, offs, 2.0, 0.5)
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            total.backward(gradient=gradient)
            torch.cuda.synchronize()
        kernels = [e.key for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
        return total.detach().clone(), kd.clone(), sg.grad, kernels
    fast = run(unit_gradient(DEV))
    again = run(unit_gradient(DEV))
    one = run(torch.ones((), device=DEV))
    part = run(torch.full((), 0.37, device=DEV))
    assert fast[3] == [], f"kernels in the backward pass: {fast[3]}"
    assert one[3] != [] and part[3] != []
    for a, b, c in zip(fast[:3], again[:3], one[:3]):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert_close_rel(part[2], 0.37 * fast[2].cpu().double(), 1e-6, "0.37 * dstudent", floor=0.0)


def test_kd_host_checks():
    from analysisgnn_amd import _lib
    from analysisgnn_amd.continual import distillation_loss
    s, t = torch.randn(4, 10, device=DEV), torch.randn(4, 10, device=DEV)
    for bad in ([0, 4, 4, 10], [0, 4, 11], [(2, 6), (5, 9)]):
        with pytest.raises(_lib.AgnnError):
            distillation_loss(s, t, bad)
    with pytest.raises(_lib.AgnnError):
        distillation_loss(s, t[:, :9], [0, 4, 9])
    with pytest.raises(_lib.AgnnError):
        distillation_loss(s, t, [0, 4, 10], temperature=0.0)
    with pytest.raises(_lib.AgnnError):
        distillation_loss(s.cpu(), t.cpu(), [0, 4, 10])
    total, kd = distillation_loss(s[:0], t[:0], [0, 4, 10])              # no rows: every term is 0
    assert float(total) == 0.0 and (kd == 0).all()


def _ewc_raw(p, mean, fisher, lam, g):
    from analysisgnn_amd import _lib
    lib = _lib.load()
    pen = torch.full((), float("nan"), device=DEV)
    ws = torch.empty(int(lib.agnn_ewc_workspace_bytes()), dtype=torch.uint8, device=DEV)
    _lib.check(lib.agnn_ewc_f32(p.data_ptr(), mean.data_ptr(), fisher.data_ptr(), p.numel(), lam, _lib.ptr(g), pen.data_ptr(), ws.data_ptr(),
                                ws.numel(), _lib.stream_ptr(torch.device(DEV))), "agnn_ewc_f32")
    return pen


@pytest.mark.parametrize("n", [1, 3, 255, 1025, 262147])
def test_ewc_kernels_match_float64(n):
    """Tails that are not a multiple of 4, of a block's slice, or of the grid.  `g` arrives filled with random values: a kernel
    that overwrote instead of accumulating fails.  g = NULL: the penalty alone, bit-identical to the first call's."""
    from analysisgnn_amd import _lib
    gen = torch.Generator().manual_seed(n)
    p, mean, g0 = (torch.randn(n, generator=gen) for _ in range(3))
    fisher = torch.rand(n, generator=gen)
    lam = 0.7
    pd, md, fd, gd = (x.to(DEV) for x in (p, mean, fisher, g0.clone()))
    pen = _ewc_raw(pd, md, fd, lam, gd)
    d = p.double() - mean.double()
    ref_pen = (fisher.double() * d * d).sum()
    ref_g = g0.double() + 2 * lam * fisher.double() * d
    print(f"ewc n={n}: penalty {float(pen):.7g} ref {float(ref_pen):.7g}")
    assert abs(float(pen) - float(ref_pen)) <= 1e-4 * max(float(ref_pen), 1e-30)
    assert_close(pen, ref_pen, 1e-4, "penalty")
    assert_close_rel(gd, ref_g, 1e-4, "g += 2 lam f (p - mean)")
    assert torch.equal(pd.cpu(), p) and torch.equal(md.cpu(), mean) and torch.equal(fd.cpu(), fisher)
    g_after = gd.clone()
    pen2 = _ewc_raw(pd, md, fd, lam, None)
    assert torch.equal(pen2, pen) and torch.equal(gd, g_after)
    # Fisher accumulation: three batches
    lib = _lib.load()
    acc = torch.zeros(n, device=DEV)
    ref = torch.zeros(n, dtype=torch.float64)
    for k in range(3):
        gk = torch.randn(n, generator=gen)
        _lib.check(lib.agnn_fisher_accum_f32(gk.to(DEV).data_ptr(), n, 1.0 / 3.0, acc.data_ptr(), _lib.stream_ptr(torch.device(DEV))),
                   "agnn_fisher_accum_f32")
        torch.cuda.synchronize()
        ref += gk.double() ** 2 / 3.0
    assert_close_rel(acc, ref, 1e-4, "fisher")
    assert float(ref.abs().max()) >= 1e-3


TASKS = {"cadence": 3, "localkey": 50, "hrythm": 2}      # 55 head biases back to back: the flat layout has a padding slot


def _model_and_batch():
    from analysisgnn_amd.models import TorchAnalysisGNN
    from analysisgnn_amd.synth import make_batch, torch_inputs
    dev = torch.device(DEV)
    g = make_batch(2, 60)
    I = torch_inputs(g, 25, dev, seed=0)
    labels = torch.stack([torch.randint(0, c, (I["batch_size"],), generator=torch.Generator().manual_seed(i)).to(dev)
                          for i, c in enumerate(TASKS.values())])
    torch.manual_seed(0)
    model = TorchAnalysisGNN(g.metadata(), 25, 32, 128, TASKS, 2, dropout=0.0, use_jk=False, logit_fusion=False).to(dev).train()
    return model, I, labels


def _objective(model, I, labels):
    from analysisgnn_amd.heads import training_loss
    x = model.encode(**I)
    logits, offs, _ = model.forward_clf_fused(x)
    return training_loss(logits, offs, labels, x, 0.1, 0.1, -1)[0]


def test_ewc_object_on_a_model():
    """`EWC` over the flat buffers of a real model: the dict surfaces alias the flat buffers under the reference's names,
    consolidate -> penalty 0, then one backward, accumulate(2), one optimizer step and add_penalty_: penalty and gradient delta
    against the float64 per-parameter loop of the reference (models/analysis.py:1440-1495); padding slots of the layout stay 0."""
    from analysisgnn_amd import dp
    from analysisgnn_amd.continual import EWC
    model, I, labels = _model_and_batch()
    params, tight = dp.plan_parameters(model)
    grads = dp.FlatGradBuffer(params, views=False, tight=tight)
    opt = dp.FlatAdamW(params, grads, lr=0.05)
    ewc = EWC(opt)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    fd, md = ewc.fisher_dict(model), ewc.means_dict(model)
    assert list(fd) == names and list(md) == names
    named = dict(model.named_parameters())
    ewc.fisher.fill_(3.0)
    for n in names:
        assert fd[n].shape == named[n].shape and md[n].shape == named[n].shape
        assert fd[n].untyped_storage().data_ptr() == ewc.fisher.untyped_storage().data_ptr()
        assert md[n].untyped_storage().data_ptr() == ewc.mean.untyped_storage().data_ptr()
        assert (fd[n] == 3.0).all() and torch.equal(md[n], named[n].detach())
    ewc.consolidate()
    assert float(ewc.fisher.abs().max()) == 0.0 and float(ewc.penalty()) == 0.0
    grads.zero()
    _objective(model, I, labels).backward()
    grads.pack()
    ewc.accumulate(2)
    fisher_ref = {n: named[n].grad.detach().cpu().double() ** 2 / 2 for n in names}
    for n in names:
        assert_close_rel(fd[n], fisher_ref[n], 1e-4, f"fisher[{n}]")
    pad = torch.ones(ewc.fisher.numel(), dtype=torch.bool)
    for p, o in zip(grads.params, grads.offsets):
        pad[o:o + p.numel()] = False
    assert int(pad.sum()) > 0 and (ewc.fisher.cpu()[pad] == 0).all()
    assert float(ewc.penalty()) == 0.0                     # the parameters have not moved yet
    opt.step()
    # the float64 per-parameter restatement; lambda chosen so that the term's gradient is as large as the gradient in the buffer
    d = {n: named[n].detach().cpu().double() - md[n].cpu().double() for n in names}
    pen_ref = sum(float((fd[n].cpu().double() * d[n] ** 2).sum()) for n in names)
    unit = max(float((2 * fd[n].cpu().double() * d[n]).abs().max()) for n in names)
    lam = float(grads.flat.abs().max()) / unit
    before = grads.flat.clone()
    pen = ewc.add_penalty_(lam).clone()
    delta_ref = torch.zeros(before.numel(), dtype=torch.float64)
    where = {id(p): o for p, o in zip(grads.params, grads.offsets)}
    for n in names:
        o = where[id(named[n])]
        delta_ref[o:o + d[n].numel()] = (2 * lam * fd[n].cpu().double() * d[n]).reshape(-1)
    print(f"ewc object: penalty {float(pen):.6g} ref {pen_ref:.6g}, lambda {lam:.4g}, max|delta ref| {float(delta_ref.abs().max()):.3g}")
    assert pen_ref > 0 and abs(float(pen) - pen_ref) <= 1e-4 * pen_ref
    assert float(delta_ref.abs().max()) >= 1e-3
    assert_close_rel(grads.flat - before, delta_ref, 1e-4, "gradient delta")
    assert_close_rel(grads.flat, before.cpu().double() + delta_ref, 1e-4, "gradient after add_penalty_")
    assert torch.equal(ewc.penalty(), pen)
    # state round trip
    state = ewc.state_dict()
    ewc.consolidate()
    ewc.load_state_dict(state)
    assert torch.equal(ewc.fisher, state["fisher"]) and torch.equal(ewc.mean, state["mean"])


def test_stage_two_recipe():
    """training_loss + distill in one backward == the two terms backpropagated separately; the distillation term reaches the
    student's heads only (the memory model encodes: models/analysis.py:1042-1051), the memory model takes no gradient, and the
    head gradients match float64 autograd through a copy of the heads fed the same encoding."""
    from analysisgnn_amd.continual import MemoryModel, distill
    from analysisgnn_amd.linear import join_wgrad
    model, I, labels = _model_and_batch()
    _objective(model, I, labels).backward()                # the model has been trained when its copy is taken
    memory = MemoryModel(model)
    assert not memory.module.training and all(not p.requires_grad for p in memory.parameters())
    with torch.no_grad():                                  # the student has moved on since the task switch
        gen = torch.Generator().manual_seed(5)
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=gen).to(DEV))
    previous = ["cadence", "hrythm"]
    w = 40.0
    names = [n for n, _ in model.named_parameters()]

    def grads_of(fn):
        for p in model.parameters():
            p.grad = None
        total = fn()
        total.backward()
        join_wgrad()                                       # what FlatGradBuffer.pack() does first: weight gradients issued elsewhere are in
        torch.cuda.synchronize()
        return total.detach(), {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    both, g_both = grads_of(lambda: _objective(model, I, labels) + distill(model, memory, I, previous, weight=w)[0])
    ce, g_ce = grads_of(lambda: _objective(model, I, labels))
    kd, g_kd = grads_of(lambda: distill(model, memory, I, previous, weight=w)[0])
    assert float(kd) > 0
    assert_close(both, ce + kd, 1e-6, "total")
    for n in names:
        parts = [g for g in (g_ce[n], g_kd[n]) if g is not None]
        assert (g_both[n] is not None) == bool(parts), n
        if not parts:                                      # a structurally dead branch of the encoder: no gradient in any run
            continue
        assert_close_rel(g_both[n], sum(p.cpu().double() for p in parts), 1e-5, f"d{n}")
        head = n.startswith("clf_dict.") and n.split(".")[1] in previous
        assert (g_kd[n] is not None) == head, f"{n}: distillation gradient {'missing' if head else 'reached a parameter outside the previous heads'}"
    assert all(p.grad is None for p in memory.parameters())
    # float64 autograd through copies of the heads on the same encoding
    with torch.no_grad():
        x = memory.encode(**I).cpu().double()
    s64 = copy.deepcopy(model.clf_dict).double().cpu()
    t64 = copy.deepcopy(memory.module.clf_dict).double().cpu()
    for p in s64.parameters():
        p.grad = None
    kd64 = []
    for t in previous:
        lq = F.log_softmax(s64[t](x) / 2.0, 1)
        with torch.no_grad():
            zt = t64[t](x) / 2.0
        kd64.append((F.softmax(zt, 1) * (F.log_softmax(zt, 1) - lq)).sum() / x.shape[0] * 4.0)
    ref = w * torch.stack(kd64).mean()
    ref.backward()
    assert_close(kd, ref.detach(), 1e-4, "distillation total")
    biggest = 0.0
    for n, p in s64.named_parameters():
        if n.split(".")[0] in previous:
            biggest = max(biggest, float(p.grad.abs().max()))
            assert_close_rel(g_kd["clf_dict." + n], p.grad, 1e-4, f"distillation d clf_dict.{n}")
    print(f"recipe: ce {float(ce):.5g} kd {float(kd):.5g}; largest float64 head gradient {biggest:.3g}")
    assert biggest >= 1e-3
    # update_from refreshes the teacher in place
    ptrs = [p.data_ptr() for p in memory.parameters()]
    memory.update_from(model)
    assert ptrs == [p.data_ptr() for p in memory.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(memory.parameters(), model.parameters()))
    assert all(not p.requires_grad for p in memory.parameters()) and all(p.requires_grad for p in model.parameters())
    assert abs(float(distill(model, memory, I, previous, weight=w)[0])) <= 1e-6 * w


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.a = torch.nn.Parameter(torch.randn(5, 7, generator=g))      # 35 elements: one padding slot behind it
        self.b = torch.nn.Parameter(torch.randn(13, generator=g))


def test_three_optimizer_steps_match_adamw_with_the_penalty_in_the_loss():
    """FlatAdamW + EWC.add_penalty_(2.0) on the gradient buffer against torch.optim.AdamW in float64 with
    `loss + 2.0 * sum fisher (p - mean)^2` as the objective: parameters after three steps within 1e-5 relative."""
    from analysisgnn_amd import dp
    from analysisgnn_amd.continual import EWC
    lam, lr = 2.0, 1e-2
    gen = torch.Generator().manual_seed(1)
    A, U = torch.randn(5, 7, generator=gen), torch.randn(13, generator=gen)
    mean = {"a": torch.randn(5, 7, generator=gen), "b": torch.randn(13, generator=gen)}
    fisher = {"a": torch.rand(5, 7, generator=gen), "b": torch.rand(13, generator=gen)}

    def loss_of(m, cast):
        return (0.5 * (m.a - cast(A)) ** 2).sum() + (torch.sin(m.b) * cast(U)).sum()
    ref = _Toy().double()
    ropt = torch.optim.AdamW(ref.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for _ in range(3):
        ropt.zero_grad()
        pen = sum((fisher[n].double() * (p - mean[n].double()) ** 2).sum() for n, p in ref.named_parameters())
        (loss_of(ref, lambda x: x.double()) + lam * pen).backward()
        ropt.step()
    toy = _Toy().to(DEV)
    params = list(toy.parameters())
    grads = dp.FlatGradBuffer(params, views=False)
    opt = dp.FlatAdamW(params, grads, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    ewc = EWC(opt)
    for n in ("a", "b"):
        ewc.means_dict(toy)[n].copy_(mean[n].to(DEV))
        ewc.fisher_dict(toy)[n].copy_(fisher[n].to(DEV))
    for _ in range(3):
        grads.zero()
        loss_of(toy, lambda x: x.to(DEV)).backward()
        grads.pack()
        ewc.add_penalty_(lam)
        opt.step()
    for n, p in ref.named_parameters():
        assert_close_rel(dict(toy.named_parameters())[n], p.detach(), 1e-5, f"parameter {n} after three steps")
