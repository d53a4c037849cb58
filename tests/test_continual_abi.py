"""The continual-learning entry points (csrc/continual.hip) reject bad arguments before any HIP call: safe on a CPU-only host.
Pointers that pass the null checks are made-up addresses; a call that got as far as using one would not return a code.
Codes as include/agnn.h defines them: -22 (AGNN_EINVAL) for null pointers and bad sizes, -12 (AGNN_ENOMEM) for a workspace
that is too small, -14 (AGNN_EALIGN) for misaligned flat buffers; each with a message."""
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


def _kd(lib, student=P, teacher=P, seg_off=P, seg_end=None, T=2, N=8, n_cols=10, tau=2.0, w=0.5, ds=P, kd=P, total=P, ws=P, ws_bytes=None,
        ld=10):
    if ws_bytes is None:
        ws_bytes = int(lib.agnn_kd_workspace_bytes(N, T))
    return lib.agnn_multitask_kd_f32(student, ld, teacher, ld, seg_off, seg_end, T, N, n_cols, tau, w, ds, ld, kd, total, ws, ws_bytes, None)


def test_module_and_symbols_exist(lib):
    from analysisgnn_amd import continual
    for name in ("distillation_loss", "distill", "MemoryModel", "EWC"):
        assert hasattr(continual, name)
    assert lib.agnn_kd_workspace_bytes(16000, 21) == 16000 * 21 * 4
    assert lib.agnn_kd_workspace_bytes(0, 3) == 0
    assert lib.agnn_ewc_workspace_bytes() >= 4


def test_kd_rejects_bad_arguments(lib):
    for kw in (dict(student=None), dict(teacher=None), dict(seg_off=None), dict(ds=None), dict(kd=None), dict(total=None)):
        assert _kd(lib, **kw) == -22, kw
        assert b"multitask_kd" in lib.agnn_last_error()
    assert _kd(lib, T=0) == -22 and b"n_tasks=0" in lib.agnn_last_error()
    assert _kd(lib, T=-3) == -22
    assert _kd(lib, tau=0.0) == -22 and b"temperature" in lib.agnn_last_error()
    assert _kd(lib, tau=-1.0) == -22
    assert _kd(lib, tau=float("inf")) == -22
    assert _kd(lib, tau=float("nan")) == -22
    assert _kd(lib, N=-1) == -22
    assert _kd(lib, n_cols=11) == -22                      # wider than the row strides
    assert _kd(lib, ws=None) == -22 and b"workspace" in lib.agnn_last_error()
    assert _kd(lib, ws_bytes=8 * 2 * 4 - 1) == -12 and b"workspace" in lib.agnn_last_error()
    assert _kd(lib, ws=P + 2) == -14


def test_ewc_rejects_bad_arguments(lib):
    wsb = int(lib.agnn_ewc_workspace_bytes())
    ok = dict(p=P, mean=P, fisher=P, n=100, lam=1.0, g=P, penalty=P, ws=P, wsb=wsb)

    def ewc(**kw):
        a = dict(ok, **kw)
        return lib.agnn_ewc_f32(a["p"], a["mean"], a["fisher"], a["n"], a["lam"], a["g"], a["penalty"], a["ws"], a["wsb"], None)
    for kw in (dict(p=None), dict(mean=None), dict(fisher=None), dict(penalty=None), dict(ws=None)):
        assert ewc(**kw) == -22, kw
        assert b"ewc" in lib.agnn_last_error()
    assert ewc(n=-1) == -22
    assert ewc(lam=float("nan")) == -22
    assert ewc(wsb=wsb - 1) == -12 and b"workspace" in lib.agnn_last_error()
    assert ewc(wsb=0) == -12
    assert ewc(g=P + 4) == -14 and b"aligned" in lib.agnn_last_error()
    assert ewc(mean=P + 8) == -14


def test_fisher_accum_rejects_bad_arguments(lib):
    assert lib.agnn_fisher_accum_f32(None, 10, 0.5, P, None) == -22 and b"fisher_accum" in lib.agnn_last_error()
    assert lib.agnn_fisher_accum_f32(P, 10, 0.5, None, None) == -22
    assert lib.agnn_fisher_accum_f32(P, -1, 0.5, P, None) == -22
    assert lib.agnn_fisher_accum_f32(P, 10, float("inf"), P, None) == -22
    assert lib.agnn_fisher_accum_f32(P + 4, 10, 0.5, P, None) == -14
    assert lib.agnn_fisher_accum_f32(None, 0, 0.5, None, None) == 0      # nothing to do: no pointer is looked at


def test_offsets_are_checked_on_the_host():
    from analysisgnn_amd import _lib
    from analysisgnn_amd.continual import _segments
    assert _segments([0, 4, 10], 10) == ((0, 4, 10), None)
    assert _segments([(4, 19), (40, 62)], 70) == ((4, 40, 62), (19, 62))
    assert _segments([(4, 19), (19, 62)], 70) == ((4, 19, 62), None)
    for bad, n in (([0, 4, 4], 10), ([0, 4, 11], 10), ([0], 10), ([], 10), ([(4, 19), (18, 30)], 70), ([(-1, 3)], 10), ([5, 3], 10)):
        with pytest.raises(_lib.AgnnError):
            _segments(bad, n)
