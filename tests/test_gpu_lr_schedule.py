"""The scheduled optimizer step on the GPU (csrc/adamw.hip: agnn_adamw_sched_f32; dp.FlatAdamW(lr=LRSchedule, swa=SWA)).

The expected rates are the recorded doubles of tests/golden/lr_schedules.npz (the reference's scheduler classes and torch's
SWALR, stepped once per optimizer step).  The kernel evaluates lr(k) in double and rounds it to float once, so `last_lr` may
differ from float32(fixture[k]) by at most one float32 ulp (the double results differ by ~1e-15 relative, which can only move
the rounding across one boundary).  Everything that compares two runs of the same kernels asks for bit equality."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_LR, ETA_MIN = 5e-3, 5e-5


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "lr_schedules.npz")))


def _cosine(w, e):
    from analysisgnn_amd import dp
    return dp.LRSchedule.reference_cosine(BASE_LR, w, e, eta_min=ETA_MIN)


def _mlp(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(37, 64), nn.ReLU(), nn.Linear(64, 5)).to(DEV)


def _optimizer(model, lr, swa=None, **kw):
    from analysisgnn_amd import dp
    grads = dp.FlatGradBuffer(model.parameters())                   # views: the tests write the gradient buffer directly
    return grads, dp.FlatAdamW(model.parameters(), grads, lr=lr, weight_decay=5e-3, swa=swa, **kw)


def _fixed_grads(n, steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(DEV) for _ in range(steps)]


def _assert_lr(last_lr, expected_double, k):
    want = np.float32(expected_double)
    got = np.float32(float(last_lr))
    assert abs(float(got) - float(want)) <= float(np.spacing(want)), f"step {k}: last_lr {got!r}, fixture {expected_double!r}"


# ---- 1. the raw entry point at every size class ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 300003])
def test_constant_schedule_is_the_plain_step_bit_for_bit(n):
    """Tail only, fewer than four elements, one block, many blocks with a tail.  A constant schedule against agnn_adamw_f32 on
    the same inputs, 3 steps: p, m, v, the norm and the written-back clipped gradient.  A third run adds SWA from step 1 on
    (swa_lr = lr, so the rate stays put): same p / m / v, and the average over the tail and the vector body is the float64
    mean of the two snapshots within 4 * 2 * 2^-23 * max|p| (two snapshots, each update a few roundings)."""
    from analysisgnn_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(n)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    lr, runs = 5e-3, {}
    for mode in ("plain", "sched", "swa"):
        # 16-byte aligned bases: every buffer is its own allocation
        p, g = p0.to(DEV), g0.to(DEV)
        m, v, avg = torch.zeros_like(p), torch.zeros_like(p), torch.full_like(p, 77.0)
        t, norm, state = (torch.zeros(k, device=DEV) for k in (1, 1, 2))
        sched = _lib.LrSchedule(kind=_lib.LR_CONSTANT, base_lr=lr, swa_start=1 if mode == "swa" else -1, swa_period=1, swa_anneal=0,
                                swa_lr=lr, cos_b=1.0, gamma=1.0, decay_steps=1.0)
        ws = torch.empty(int(lib.agnn_adamw_sched_workspace_bytes()), dtype=torch.uint8, device=DEV)
        snaps = []
        for k in range(3):
            snaps.append(p.double().cpu())
            if mode == "plain":
                rc = lib.agnn_adamw_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, 0.9, 0.999, 1e-8, 5e-3, 0.5,
                                        t.data_ptr(), norm.data_ptr(), 1, ws.data_ptr(), ws.numel(), _lib.stream_ptr(torch.device(DEV)))
            else:
                rc = lib.agnn_adamw_sched_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, ctypes.byref(sched), 0.9, 0.999,
                                              1e-8, 5e-3, 0.5, t.data_ptr(), avg.data_ptr() if mode == "swa" else None,
                                              state.data_ptr(), norm.data_ptr(), 1, ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr(torch.device(DEV)))
            _lib.check(rc, mode)
            if mode == "swa" and k == 0:
                assert bool((avg == 77.0).all())                     # no snapshot below the start: untouched
        torch.cuda.synchronize()
        runs[mode] = dict(p=p, g=g, m=m, v=v, norm=norm, t=t)
        if mode != "plain":
            assert float(state[0]) == float(np.float32(lr)) and float(state[1]) == (2.0 if mode == "swa" else 0.0)
        if mode == "swa":
            mean = (snaps[1] + snaps[2]) / 2
            bound = 4 * 2 * 2.0 ** -23 * float(max(snaps[1].abs().max(), snaps[2].abs().max()))
            assert float((avg.double().cpu() - mean).abs().max()) <= bound
    for mode in ("sched", "swa"):
        for name, ref in runs["plain"].items():
            assert torch.equal(runs[mode][name], ref), (mode, name)
    assert float(runs["plain"]["t"]) == 3.0 and float(runs["plain"]["m"].abs().max()) > 0


# ---- 2 + 3. the rate the kernel used, and its application against the float path ------------------------------------------------
def test_rate_matches_the_fixture_and_the_float_path_applies_it_identically(golden):
    """14 steps of a 37->64->5 MLP under the reference's cosine (5, 4).  After each step `last_lr` is within one float32 ulp of
    float32(fixture[k]); a twin on the float path (agnn_adamw_f32) given `lr = float(last_lr)` and the same gradients has
    bit-identical parameters after every step: computing the rate and applying it are checked apart, the second without a
    tolerance."""
    lrs = golden["cosine_w5_e4"]
    a, b = _mlp(), _mlp()
    ga, oa = _optimizer(a, _cosine(5, 4))
    gb, ob = _optimizer(b, 1.0)
    assert torch.equal(oa.flat, ob.flat)
    _assert_lr(oa.last_lr, lrs[0], -1)                              # before the first step: lr(0)
    x = torch.randn(64, 37, device=DEV)
    for k in range(14):
        assert abs(oa.current_lr() - lrs[k]) <= 1e-12 * BASE_LR
        ga.zero()
        (a(x).pow(2).sum() * 3.0).backward()
        gb.flat.copy_(ga.flat)
        oa.step(max_norm=0.5)
        _assert_lr(oa.last_lr, lrs[k], k)
        ob.lr = float(oa.last_lr)
        ob.step(max_norm=0.5)
        assert torch.equal(oa.flat, ob.flat), f"step {k}"
        assert torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v) and torch.equal(oa.last_norm, ob.last_norm)
    assert float(oa._t) == 14.0


# ---- 4. against torch ------------------------------------------------------------------------------------------------------------
def test_scheduled_step_matches_torch_adamw_with_the_fixture_rate(golden):
    """6 steps under cosine (3, 7) — across the warm-up edge — with max_norm = 0.5, against clip_grad_norm_ + torch.optim.AdamW
    whose lr is set from the fixture; the bounds of test_fused_clip_adamw_matches_torch at the same step count."""
    from analysisgnn_amd import dp
    lrs = golden["cosine_w3_e7"]
    a = _mlp()
    b = copy.deepcopy(a)
    ref = torch.optim.AdamW(a.parameters(), lr=5e-3, weight_decay=5e-3)
    flat = dp.FlatGradBuffer(b.parameters(), views=False)
    opt = dp.FlatAdamW(b.parameters(), flat, lr=_cosine(3, 7), weight_decay=5e-3)
    x = torch.randn(64, 37, device=DEV)
    for k in range(6):
        ref.param_groups[0]["lr"] = float(lrs[k])
        ref.zero_grad(set_to_none=True)
        (a(x).pow(2).sum() * 3.0).backward()
        total = torch.nn.utils.clip_grad_norm_(a.parameters(), 0.5)
        ref.step()
        flat.zero()
        (b(x).pow(2).sum() * 3.0).backward()
        flat.pack()
        opt.step(max_norm=0.5)
        assert abs(float(opt.last_norm) - float(total)) <= 1e-4 * float(total)
        for pa, pb in zip(a.parameters(), b.parameters()):
            torch.testing.assert_close(pb, pa, rtol=1e-4, atol=1e-6)


# ---- 5. capture as the first step ever -------------------------------------------------------------------------------------------
def test_captured_first_step_follows_the_schedule_on_replay(golden):
    """Construct, then capture `opt.step(max_norm=1.0)` before any eager step; 14 replays on fixed gradients against an eager
    twin: parameters and `last_lr` bit-identical after every replay, the counter reads 14."""
    lrs = golden["cosine_w5_e4"]
    a, b = _mlp(), _mlp()
    ga, oa = _optimizer(a, _cosine(5, 4))
    gb, ob = _optimizer(b, _cosine(5, 4))
    g = _fixed_grads(oa.flat.numel(), 1)[0]
    ga.flat.copy_(g)
    gb.flat.copy_(g)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ob.step(max_norm=1.0)
    torch.cuda.synchronize()
    assert float(ob._t) == 0.0 and torch.equal(oa.flat, ob.flat)    # a capture runs nothing
    for k in range(14):
        oa.step(max_norm=1.0)
        cg.replay()
        assert torch.equal(ob.flat, oa.flat), f"replay {k}"
        assert torch.equal(ob.last_lr, oa.last_lr)
        _assert_lr(ob.last_lr, lrs[k], k)
    assert float(ob._t) == 14.0 and float(oa._t) == 14.0


# ---- 6. SWA ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("replayed", [False, True], ids=["eager", "replayed"])
def test_swa_average_rate_and_swap(golden, replayed):
    """K = 6, P = 3, Na = 2 over 14 steps: snapshots before steps 6, 9, 12.  The average against the float64 mean of the three
    host-side snapshots within 4 * n * 2^-23 * max|p| (n = 3; each update rounds a few times), `last_lr` against the fixture
    (base classes below K, torch's SWALR from K), untouched below K (sentinel), and swap_swa_."""
    from analysisgnn_amd import dp
    lrs = golden["swa_cosine_w5_e4"]
    a = _mlp()
    ga, oa = _optimizer(a, _cosine(5, 4), swa=dp.SWA(6, 3, anneal_epochs=2, swa_lr=5e-5))
    oa.swa_flat.fill_(-123.0)
    grads = _fixed_grads(oa.flat.numel(), 14)
    cg = None
    if replayed:
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            oa.step(max_norm=1.0)
    snaps = []
    for k in range(14):
        if k in (6, 9, 12):
            snaps.append(oa.flat.double().cpu())
        ga.flat.copy_(grads[k])
        cg.replay() if replayed else oa.step(max_norm=1.0)
        _assert_lr(oa.last_lr, lrs[k], k)
        if k < 6:
            assert bool((oa.swa_flat == -123.0).all()) and float(oa.n_averaged) == 0.0
    assert float(oa.n_averaged) == 3.0
    mean = (snaps[0] + snaps[1] + snaps[2]) / 3
    bound = 4 * 3 * 2.0 ** -23 * float(max(s.abs().max() for s in snaps))
    worst = float((oa.swa_flat.double().cpu() - mean).abs().max())
    print(f"swa: max |avg - mean64| = {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound
    assert not torch.equal(oa.flat, oa.swa_flat)
    oa.swap_swa_()
    for p, o in zip(a.parameters(), ga.offsets):
        assert torch.equal(p.detach().reshape(-1), oa.swa_flat[o:o + p.numel()])


# ---- 7. resume into a captured optimizer ----------------------------------------------------------------------------------------
def test_state_dict_resumes_a_captured_graph():
    """state_dict after 4 eager steps, loaded into an optimizer whose graph was captured (and replayed) before: 4 replays equal
    8 uninterrupted steps bit for bit, SWA average and count included."""
    from analysisgnn_amd import dp
    swa = dict(anneal_epochs=2, swa_lr=5e-5)
    a, b, c = _mlp(), _mlp(), _mlp()
    ga, oa = _optimizer(a, _cosine(3, 7), swa=dp.SWA(2, 2, **swa))
    gb, ob = _optimizer(b, _cosine(3, 7), swa=dp.SWA(2, 2, **swa))
    gc, oc = _optimizer(c, _cosine(3, 7), swa=dp.SWA(2, 2, **swa))
    grads = _fixed_grads(oa.flat.numel(), 8)
    for k in range(8):
        ga.flat.copy_(grads[k])
        oa.step(max_norm=1.0)
    for k in range(4):
        gb.flat.copy_(grads[k])
        ob.step(max_norm=1.0)
    sd = ob.state_dict()
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        oc.step(max_norm=1.0)
    gc.flat.copy_(grads[7])
    for _ in range(3):                                              # some other history, which the load must replace
        cg.replay()
    oc.load_state_dict(sd)
    assert float(oc._t) == 4.0 and float(oc.n_averaged) == 1.0
    for k in range(4, 8):
        gc.flat.copy_(grads[k])
        cg.replay()
    for name in ("flat", "m", "v", "swa_flat", "_state", "_t"):
        assert torch.equal(getattr(oc, name), getattr(oa, name)), name
    assert float(oa.n_averaged) == 3.0
    for p, q in zip(a.parameters(), c.parameters()):
        assert torch.equal(p, q)
