"""The scheduled optimizer step (csrc/adamw.hip: agnn_adamw_sched_f32, agnn_lr_schedule_at) rejects bad arguments before any
HIP call: safe on a CPU-only host.  Pointers that pass the null checks are made-up addresses; a call that got as far as
using one would not return a code.  Codes as include/agnn.h defines them: -22 (AGNN_EINVAL), -12 (AGNN_ENOMEM), -14
(AGNN_EALIGN); each with a message."""
import ctypes
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 1 << 20          # a made-up, 16-byte aligned device address


@pytest.fixture(scope="module")
def lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _sched(**kw):
    from analysisgnn_amd import _lib
    f = dict(kind=_lib.LR_WARMUP_COSINE, warmup_steps=5, count_offset=1, swa_period=3, swa_start=-1, swa_anneal=2, base_lr=5e-3,
             warmup_start_lr=0.0, eta_min=5e-5, cos_a=5 / 3, cos_b=4.0, gamma=0.9, decay_steps=7.0, swa_lr=5e-5)
    f.update(kw)
    return _lib.LrSchedule(**f)


def _step(lib, sched="ok", n=100, swa_avg=None, state=P, ws=P, wsb=None, p=P, g=P, b1=0.9):
    if sched == "ok":
        sched = _sched()
    if wsb is None:
        wsb = int(lib.agnn_adamw_sched_workspace_bytes())
    ref = ctypes.byref(sched) if sched is not None else None
    return lib.agnn_adamw_sched_f32(p, g, P, P, n, ref, b1, 0.999, 1e-8, 1e-2, 1.0, P, swa_avg, state, P, 0, ws, wsb, None)


def test_workspace_covers_the_plain_step(lib):
    assert lib.agnn_adamw_sched_workspace_bytes() >= lib.agnn_adamw_workspace_bytes() + 3 * 4      # + lr, snapshot flag, count


BAD_SCHEDULES = [
    (dict(kind=3), b"kind"), (dict(kind=-1), b"kind"),
    (dict(warmup_steps=-1), b"warmup_steps"),
    (dict(cos_a=4.0, cos_b=4.0), b"cosine"),                                     # B == A
    (dict(kind=2, decay_steps=0.0), b"decay_steps"), (dict(kind=2, decay_steps=-7.0), b"decay_steps"),
    (dict(kind=2, gamma=0.0), b"gamma"), (dict(kind=2, gamma=-0.5), b"gamma"),
    (dict(base_lr=math.inf), b"non-finite"), (dict(base_lr=math.nan), b"non-finite"),
    (dict(eta_min=math.nan), b"non-finite"), (dict(warmup_start_lr=-math.inf), b"non-finite"),
    (dict(swa_start=6, swa_lr=math.nan), b"non-finite"),
    (dict(swa_start=6, swa_period=0), b"swa_period"), (dict(swa_start=0, swa_period=-2), b"swa_period"),
    (dict(swa_start=6, swa_anneal=-1), b"swa_anneal"),
]


@pytest.mark.parametrize("fields,word", BAD_SCHEDULES, ids=[str(sorted(f.items())) for f, _ in BAD_SCHEDULES])
def test_bad_schedules_are_einval_everywhere(lib, fields, word):
    s = _sched(**fields)
    assert _step(lib, sched=s, swa_avg=P) == -22
    assert word in lib.agnn_last_error()
    assert math.isnan(lib.agnn_lr_schedule_at(ctypes.byref(s), 0)) and word in lib.agnn_last_error()


def test_swa_fields_are_ignored_without_swa(lib):
    s = _sched(swa_start=-1, swa_period=0, swa_anneal=-1, swa_lr=math.nan)
    assert lib.agnn_lr_schedule_at(ctypes.byref(s), 0) == pytest.approx(1e-3, rel=1e-15)
    assert _step(lib, sched=s, n=0) == 0


def test_step_rejects_bad_arguments(lib):
    assert _step(lib, sched=None) == -22 and b"null schedule" in lib.agnn_last_error()
    assert math.isnan(lib.agnn_lr_schedule_at(None, 0)) and b"null schedule" in lib.agnn_last_error()
    assert math.isnan(lib.agnn_lr_schedule_at(ctypes.byref(_sched()), -1)) and b"k=-1" in lib.agnn_last_error()
    assert _step(lib, state=None) == -22 and b"state" in lib.agnn_last_error()
    assert _step(lib, sched=_sched(swa_start=6), swa_avg=None) == -22 and b"swa_avg" in lib.agnn_last_error()
    assert _step(lib, sched=_sched(swa_start=6), swa_avg=P + 4) == -14 and b"swa_avg" in lib.agnn_last_error()
    assert _step(lib, sched=_sched(swa_start=0), swa_avg=P + 8) == -14
    assert _step(lib, wsb=int(lib.agnn_adamw_workspace_bytes())) == -12 and b"workspace" in lib.agnn_last_error()
    assert _step(lib, wsb=0) == -12
    assert _step(lib, ws=None) == -22
    assert _step(lib, n=-1) == -22
    assert _step(lib, p=None) == -22
    assert _step(lib, g=P + 4) == -14 and b"aligned" in lib.agnn_last_error()
    assert _step(lib, b1=1.0) == -22 and b"betas" in lib.agnn_last_error()
    assert _step(lib, n=0) == 0                                                   # nothing to do: no launch


def test_host_evaluation_needs_no_gpu(lib):
    s = _sched()
    assert lib.agnn_lr_schedule_at(ctypes.byref(s), 0) == pytest.approx(1e-3, rel=1e-15)             # warm-up runs on k + 1
    assert lib.agnn_lr_schedule_at(ctypes.byref(s), 3) == pytest.approx(4e-3, rel=1e-15)
    assert lib.agnn_lr_schedule_at(ctypes.byref(s), 4) == pytest.approx(5e-5, rel=1e-12)      # k == cos_b: the cosine's end
    const = _sched(kind=0, base_lr=2.5e-4)
    assert lib.agnn_lr_schedule_at(ctypes.byref(const), 123456) == 2.5e-4
