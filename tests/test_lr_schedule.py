"""The learning-rate schedule of the scheduled optimizer step, on the host (no GPU): `agnn_lr_schedule_at` is the
`__host__ __device__` function the kernel evaluates, compiled for the host, so these tests pin the source the GPU runs.

tests/golden/lr_schedules.npz holds, in double, what the reference's own `LinearWarmupCosineAnnealingLR` /
`LinearWarmupExponentialDecayLR` and torch's `SWALR` give when stepped once per optimizer step (scripts/gen_golden_sched.py).
Bound: |delta| <= 1e-12 * base_lr.  The closed form repeats the classes' operations in their order; what differs is the
rounding of pi * x inside math.cos(math.pi * x) (about 3e-15 relative at |x| <= 4) and, from the SWA start on, SWALR's chained
form (it recovers the initial rate from the current one, a few roundings of 1e-16 relative)."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lr_schedules.npz")
BASE_LR, ETA_MIN = 5e-3, 5e-5
BOUND = 1e-12 * BASE_LR


def _cases():
    """name -> (schedule, swa): the hyper-parameters the fixture was recorded with."""
    from analysisgnn_amd import dp
    return {
        "cosine_w5_e4": (dp.LRSchedule.reference_cosine(BASE_LR, 5, 4, eta_min=ETA_MIN), None),
        "cosine_w3_e7": (dp.LRSchedule.reference_cosine(BASE_LR, 3, 7, eta_min=ETA_MIN), None),
        "cosine_w500_e50": (dp.LRSchedule.reference_cosine(BASE_LR, 500, 50, eta_min=ETA_MIN), None),
        "exp_w5_d7": (dp.LRSchedule.reference_exponential(5e-3, 5, 7, gamma=0.9, eta_min=4.99e-3), None),
        "swa_cosine_w5_e4": (dp.LRSchedule.reference_cosine(BASE_LR, 5, 4, eta_min=ETA_MIN), dp.SWA(6, 3, anneal_epochs=2, swa_lr=5e-5)),
    }


STEPS = {"cosine_w5_e4": 20, "cosine_w3_e7": 20, "cosine_w500_e50": 520, "exp_w5_d7": 20, "swa_cosine_w5_e4": 20}


@pytest.mark.parametrize("name", sorted(STEPS))
def test_closed_form_matches_the_recorded_classes(name):
    z = np.load(GOLDEN)
    sched, swa = _cases()[name]
    exp = z[name]
    assert exp.dtype == np.float64 and exp.shape == (STEPS[name],)
    got = np.array([sched.lr_at(k, swa) for k in range(len(exp))])
    worst = float(np.abs(got - exp).max())
    print(f"{name}: max |delta| = {worst:.3e} (bound {BOUND:.1e})")
    assert worst <= BOUND
    if name == "exp_w5_d7":
        assert (exp[5:] == 4.99e-3).all() and exp[4] == 5e-3           # the clamp is active from step 5
    if name == "swa_cosine_w5_e4":
        assert exp[-1] == 5e-5 and exp[6] == exp[7] == exp[8] != exp[9]  # one SWA epoch = 3 steps; annealed after 2 epochs


def _generator():
    spec = importlib.util.spec_from_file_location("gen_golden_sched", os.path.join(ROOT, "scripts", "gen_golden_sched.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_closed_form_matches_the_reference_classes_live():
    """The same comparison against the reference's classes executed now, and the fixture against them bit for bit."""
    gen = _generator()
    if not os.path.exists(gen.REF_ANALYSIS):
        pytest.skip("reference tree not present")
    live = gen.cases(gen.reference_classes())
    z = np.load(GOLDEN)
    for name, (sched, swa) in _cases().items():
        assert np.array_equal(live[name], z[name]), name
        got = np.array([sched.lr_at(k, swa) for k in range(len(live[name]))])
        assert float(np.abs(got - live[name]).max()) <= BOUND, name
    assert gen.smallest_working_warmup(gen.reference_classes()[gen.NAMES[0]]) == int(z["meta.cosine_min_warmup"])


def test_constructor_refuses_what_the_reference_class_cannot_do():
    from analysisgnn_amd import _lib, dp
    w_min = int(np.load(GOLDEN)["meta.cosine_min_warmup"])       # recorded from the class: it raises AttributeError below this
    assert w_min == 3
    for w in range(w_min):
        with pytest.raises(ValueError, match="warmup_steps"):
            dp.LRSchedule.reference_cosine(BASE_LR, w, 4)
    dp.LRSchedule.reference_cosine(BASE_LR, w_min, 4)
    with pytest.raises(_lib.AgnnError, match="cosine"):
        dp.LRSchedule.reference_cosine(BASE_LR, 12, 4)              # max_epochs == warmup_steps / 3: a zero-length cosine
    with pytest.raises(_lib.AgnnError):
        dp.LRSchedule.reference_exponential(BASE_LR, 5, 0)
    with pytest.raises(_lib.AgnnError):
        dp.LRSchedule.constant(float("nan"))
    with pytest.raises(ValueError):
        dp.SWA(4, 0)
    with pytest.raises(_lib.AgnnError, match="k=-1"):
        dp.LRSchedule.constant(1e-3).lr_at(-1)


def test_other_constructors():
    from analysisgnn_amd import dp
    s = dp.LRSchedule.warmup_cosine(1e-2, 10, 110, eta_min=1e-4)
    assert s.lr_at(0) == 0.0 and s.lr_at(5) == pytest.approx(5e-3, rel=1e-15) and s.lr_at(10) == 1e-2
    assert s.lr_at(60) == pytest.approx(1e-4 + 0.5 * (1e-2 - 1e-4), rel=1e-12) and s.lr_at(110) == pytest.approx(1e-4, rel=1e-12)
    c = dp.LRSchedule.constant(3e-4)
    assert [c.lr_at(k) for k in (0, 1, 10 ** 6)] == [3e-4] * 3
    assert dp.LRSchedule.from_dict(s.to_dict()).to_dict() == s.to_dict()
    swa0 = dp.SWA(2, 1, anneal_epochs=0, swa_lr=7e-5)               # SWALR with anneal_epochs=0: swa_lr at once
    assert c.lr_at(1, swa0) == 3e-4 and c.lr_at(2, swa0) == 7e-5 and c.lr_at(9, swa0) == 7e-5


def _mlp_pair():
    torch.manual_seed(0)
    a = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.ReLU(), torch.nn.Linear(7, 3))
    return a, copy.deepcopy(a)


def test_flat_adamw_cpu_follows_the_schedule_like_torch_adamw():
    """8 steps under cosine (3, 7) against torch.optim.AdamW whose lr is set from the fixture before each step; the bounds of
    test_flat_adamw_matches_torch_adamw / test_fused_clip_adamw_matches_torch."""
    from analysisgnn_amd import dp
    lrs = np.load(GOLDEN)["cosine_w3_e7"]
    a, b = _mlp_pair()
    ref = torch.optim.AdamW(a.parameters(), lr=5e-3, weight_decay=5e-3)
    flat = dp.FlatGradBuffer(b.parameters(), views=False)
    opt = dp.FlatAdamW(b.parameters(), flat, lr=dp.LRSchedule.reference_cosine(BASE_LR, 3, 7, eta_min=ETA_MIN), weight_decay=5e-3)
    assert float(opt.last_lr) == float(np.float32(lrs[0]))
    x = torch.randn(11, 5)
    for k in range(8):
        assert opt.current_lr() == pytest.approx(lrs[k], abs=BOUND)
        ref.param_groups[0]["lr"] = float(lrs[k])
        ref.zero_grad()
        a(x).pow(2).sum().backward()
        ref.step()
        flat.zero()
        b(x).pow(2).sum().backward()
        flat.pack()
        opt.step()
        assert float(opt.last_lr) == float(np.float32(lrs[k]))
        for p, q in zip(a.parameters(), b.parameters()):
            torch.testing.assert_close(q, p, rtol=1e-4, atol=1e-6)


def _swa_optimizer(model):
    from analysisgnn_amd import dp
    flat = dp.FlatGradBuffer(model.parameters(), views=False)
    opt = dp.FlatAdamW(model.parameters(), flat, lr=dp.LRSchedule.reference_cosine(BASE_LR, 3, 7, eta_min=ETA_MIN), weight_decay=5e-3,
                       swa=dp.SWA(2, 2, anneal_epochs=2, swa_lr=5e-5))
    return flat, opt


def _steps(model, flat, opt, xs):
    for x in xs:
        flat.zero()
        model(x).pow(2).sum().backward()
        flat.pack()
        opt.step(max_norm=0.5)


def test_state_dict_round_trip_cpu():
    """4 steps, save, load into a FRESH optimizer, 4 more steps == 8 uninterrupted steps, bit for bit, with SWA on."""
    a, b = _mlp_pair()
    c = copy.deepcopy(a)
    xs = [torch.randn(11, 5, generator=torch.Generator().manual_seed(k)) for k in range(8)]
    fa, oa = _swa_optimizer(a)
    _steps(a, fa, oa, xs)
    fb, ob = _swa_optimizer(b)
    _steps(b, fb, ob, xs[:4])
    sd = ob.state_dict()
    _steps(b, fb, ob, xs[4:5])                                      # the saved state is a copy: further steps leave it alone
    fc, oc = _swa_optimizer(c)
    ptr = oc.flat.data_ptr()
    oc.load_state_dict(sd)
    assert oc.flat.data_ptr() == ptr and all(p.data_ptr() >= ptr for p in c.parameters())      # loaded in place
    assert int(oc.n_averaged) == 1 and int(oc._t) == 4
    _steps(c, fc, oc, xs[4:])
    for name in ("flat", "m", "v", "swa_flat", "_state", "_t"):
        assert torch.equal(getattr(oc, name), getattr(oa, name)), name
    assert int(oa.n_averaged) == 3                                  # snapshots before steps 2, 4, 6
    for p, q in zip(a.parameters(), c.parameters()):
        assert torch.equal(p, q)
    oc.swap_swa_()
    assert torch.equal(oc.flat, oa.swa_flat) and torch.equal(next(c.parameters()).reshape(-1), oa.swa_flat[:35])
    from analysisgnn_amd import dp
    other = dp.FlatAdamW(b.parameters(), fb, lr=dp.LRSchedule.constant(1e-3))
    with pytest.raises(ValueError, match="schedule"):
        other.load_state_dict(sd)


def test_float_path_is_unchanged_and_saves_too():
    from analysisgnn_amd import dp
    a, b = _mlp_pair()
    flat = dp.FlatGradBuffer(b.parameters(), views=False)
    opt = dp.FlatAdamW(b.parameters(), flat, lr=5e-3)
    assert opt.schedule is None and not hasattr(opt, "_t") and opt.current_lr() == 5e-3
    with pytest.raises(AttributeError):
        opt.last_lr
    with pytest.raises(ValueError):
        dp.FlatAdamW(b.parameters(), flat, lr=5e-3, swa=dp.SWA(1, 1))
    sd = opt.state_dict()
    assert float(sd["step"]) == 0 and sd["lr"] == 5e-3 and sd["schedule"] is None
    opt.load_state_dict(sd)
    assert float(opt._t) == 0
