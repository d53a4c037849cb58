"""The SMOTE entry points (csrc/smote.hip) reject bad arguments with a message BEFORE any HIP call (safe on a CPU-only host: the
pointers below are never dereferenced): AGNN_EINVAL (-22) for sizes out of range, NULL pointers and inconsistent plans,
AGNN_EALIGN (-14) for a pointer off 16 bytes or a leading dimension that is no multiple of 4 floats.  Empty work is success and
looks at no pointer.  The Python layer refuses what the kernels do not serve instead of falling back."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # a 16-byte aligned non-null address, never read
EINVAL, EALIGN = -22, -14


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _offs(v):
    return (C.c_int32 * len(v))(*v)


def _rowsel(lib, q=P, ld_q=32, q_rows=None, q_n=100, c=P, ld_c=32, c_rows=None, c_n=100, q_off=(0, 40, 100), c_off=(0, 40, 100), D=32, ksel=4,
            mode=0, idx=P, score=P):
    return lib.agnn_rowsel_f32(q, ld_q, q_rows, q_n, c, ld_c, c_rows, c_n, len(q_off) - 1, _offs(q_off) if q_off else None,
                               _offs(c_off) if c_off else None, D, ksel, mode, idx, score, None)


def _plan(t=(0, 10, 30), copies=(2, 3), s=None):
    from analysisgnn_amd import _lib
    p = _lib.SmotePlan()
    p.n_seg = len(copies)
    acc = 0
    for i, c in enumerate(copies):
        p.t_off[i], p.copies[i], p.label[i] = t[i], c, i + 1
        p.s_off[i] = acc if s is None else s[i]
        acc += (t[i + 1] - t[i]) * c
    p.t_off[len(copies)] = t[-1]
    p.s_off[len(copies)] = acc if s is None else s[-1]
    return p


def _fwd(lib, x=P, ld_x=32, y=P, N=100, D=32, plan=None, rows=P, nbr=P, ld_nbr=4, k=3, choice=P, gap=P, rng=None, xo=P, ld_o=32, yo=P, nb_row=P,
         used=None):
    plan = _plan() if plan is None else plan
    return lib.agnn_smote_synth_fwd_f32(x, ld_x, y, N, D, C.byref(plan), rows, nbr, ld_nbr, k, choice, gap, rng, 1, xo, ld_o, yo, nb_row, used, None)


def _bwd(lib, g=P, ld_g=32, N=100, D=32, plan=None, rows=P, gap=P, used=None, dx=P, ld_dx=32, w=P, ld_w=32):
    plan = _plan() if plan is None else plan
    return lib.agnn_smote_synth_bwd_f32(g, ld_g, N, D, C.byref(plan), rows, gap, used, 1, dx, ld_dx, w, ld_w, None)


def _draws(lib, S=10, D=32, k=3, rng=P, choice=P, gap=P):
    return lib.agnn_smote_draws_f32(S, D, k, rng, 1, choice, gap, None)


def test_row_selection_arguments():
    lib = _lib()
    for D in (0, 2, 6, 516):
        assert _rowsel(lib, D=D) == EINVAL and f"D={D}".encode() in lib.agnn_last_error()
    assert _rowsel(lib, ksel=0) == EINVAL and b"ksel=0" in lib.agnn_last_error()
    assert _rowsel(lib, ksel=9) == EINVAL and b"ksel=9" in lib.agnn_last_error()
    assert _rowsel(lib, mode=2) == EINVAL and b"mode=2" in lib.agnn_last_error()
    assert _rowsel(lib, q_off=tuple(range(35)), c_off=tuple(range(35))) == EINVAL and b"n_seg=34" in lib.agnn_last_error()
    assert _rowsel(lib, q_off=(0, 50, 40)) == EINVAL and b"ascending" in lib.agnn_last_error()
    assert _rowsel(lib, c_off=(0, -1, 40)) == EINVAL and b"ascending" in lib.agnn_last_error()
    assert _rowsel(lib, q_n=50) == EINVAL and b"q_n=50" in lib.agnn_last_error()          # positions are rows without q_rows
    assert _rowsel(lib, c_n=50) == EINVAL and b"c_n=50" in lib.agnn_last_error()
    assert _rowsel(lib, q=None) == EINVAL and b"null" in lib.agnn_last_error()
    assert _rowsel(lib, idx=None) == EINVAL and b"idx" in lib.agnn_last_error()
    assert _rowsel(lib, ld_q=28) == EINVAL and b"ld_q=28" in lib.agnn_last_error()
    assert _rowsel(lib, ld_c=34) == EALIGN and b"ld_c=34" in lib.agnn_last_error()
    assert _rowsel(lib, q=P + 4) == EALIGN and b" q " in lib.agnn_last_error()
    assert _rowsel(lib, c=P + 8) == EALIGN and b" c " in lib.agnn_last_error()


def test_row_selection_without_work_succeeds():
    lib = _lib()
    assert lib.agnn_rowsel_f32(None, 0, None, 0, None, 0, None, 0, 0, None, None, 32, 4, 0, None, None, None) == 0
    assert _rowsel(lib, q=None, c=None, idx=None, score=None, q_off=(0, 0, 0), c_off=(0, 5, 9)) == 0      # no query
    assert _rowsel(lib, D=6, q_off=(0, 0), c_off=(0, 0)) == EINVAL                                          # the shape rule still holds


def test_synthesis_forward_arguments():
    lib = _lib()
    assert _fwd(lib, D=10) == EINVAL and b"D=10" in lib.agnn_last_error()
    assert _fwd(lib, k=1) == EINVAL and b"k=1" in lib.agnn_last_error()
    assert _fwd(lib, k=8) == EINVAL and b"k=8" in lib.agnn_last_error()
    assert _fwd(lib, N=-1) == EINVAL and b"N=-1" in lib.agnn_last_error()
    assert _fwd(lib, N=20) == EINVAL and b"30 rows" in lib.agnn_last_error()                # the plan names more rows than x has
    assert _fwd(lib, plan=_plan(copies=(2, 0))) == EINVAL and b"copies=0" in lib.agnn_last_error()
    assert _fwd(lib, plan=_plan(t=(0, 10, 10))) == EINVAL and b"class 1" in lib.agnn_last_error()
    assert _fwd(lib, plan=_plan(s=(0, 20, 70))) == EINVAL and b"s_off" in lib.agnn_last_error()
    bad = _plan()
    bad.n_seg = 33
    assert _fwd(lib, plan=bad) == EINVAL and b"n_seg=33" in lib.agnn_last_error()
    assert _fwd(lib, x=None) == EINVAL and b"x / x_over" in lib.agnn_last_error()
    assert _fwd(lib, y=None) == EINVAL and b"y_over without y" in lib.agnn_last_error()
    assert _fwd(lib, ld_x=28) == EINVAL and b"ld_x=28" in lib.agnn_last_error()
    assert _fwd(lib, ld_o=38) == EALIGN and b"ld_over=38" in lib.agnn_last_error()
    assert _fwd(lib, x=P + 4) == EALIGN and b" x " in lib.agnn_last_error()
    assert _fwd(lib, rows=None) == EINVAL and b"rows" in lib.agnn_last_error()
    assert _fwd(lib, ld_nbr=2) == EINVAL and b"ld_nbr=2" in lib.agnn_last_error()
    assert _fwd(lib, choice=None) == EINVAL and b"come together" in lib.agnn_last_error()
    assert _fwd(lib, choice=None, gap=None) == EINVAL and b"rng" in lib.agnn_last_error()   # no draws and no generator state
    assert _fwd(lib, choice=None, gap=None, rng=P) == EINVAL and b"rng_used" in lib.agnn_last_error()
    assert _fwd(lib, gap=P + 4) == EALIGN and b"gap" in lib.agnn_last_error()
    assert _fwd(lib, N=0, plan=_plan(t=(0,), copies=()), x=None, xo=None) == 0              # nothing to write


def test_synthesis_backward_arguments():
    lib = _lib()
    assert _bwd(lib, D=3) == EINVAL and b"D=3" in lib.agnn_last_error()
    assert _bwd(lib, N=10) == EINVAL and b"30 rows" in lib.agnn_last_error()
    assert _bwd(lib, plan=_plan(copies=(0, 3))) == EINVAL and b"copies=0" in lib.agnn_last_error()
    assert _bwd(lib, g=None) == EINVAL and b"g / dx / w" in lib.agnn_last_error()
    assert _bwd(lib, rows=None) == EINVAL and b"rows" in lib.agnn_last_error()
    assert _bwd(lib, gap=None) == EINVAL and b"rng_used" in lib.agnn_last_error()
    assert _bwd(lib, ld_w=16) == EINVAL and b"ld_w=16" in lib.agnn_last_error()
    assert _bwd(lib, ld_g=34) == EALIGN and b"ld_g=34" in lib.agnn_last_error()
    assert _bwd(lib, dx=P + 8) == EALIGN and b"aligned" in lib.agnn_last_error()
    assert _bwd(lib, plan=_plan(t=(0,), copies=()), g=None, dx=None, w=None) == 0           # no class is oversampled


def test_draw_export_arguments():
    lib = _lib()
    assert _draws(lib, D=7) == EINVAL and b"D=7" in lib.agnn_last_error()
    assert _draws(lib, k=1) == EINVAL and b"k=1" in lib.agnn_last_error()
    assert _draws(lib, S=-1) == EINVAL and b"S=-1" in lib.agnn_last_error()
    assert _draws(lib, rng=None) == EINVAL and b"rng" in lib.agnn_last_error()
    assert _draws(lib, gap=None) == EINVAL and b"choice / gap" in lib.agnn_last_error()
    assert _draws(lib, gap=P + 4) == EALIGN and b"gap" in lib.agnn_last_error()
    assert _draws(lib, S=0, rng=None, choice=None, gap=None) == 0


def test_python_layer_refuses_what_the_kernels_do_not_serve():
    import torch
    from analysisgnn_amd import smote
    from analysisgnn_amd._lib import AgnnError
    x, y = torch.zeros(12, 8), torch.zeros(12, dtype=torch.int64)
    with pytest.raises(AgnnError):
        smote.SMOTE(dims=8, k=3).fit_generate(x, y)                                          # CPU tensors: no fall-back
    with pytest.raises(AgnnError):
        smote.feature_penalty(torch.zeros(()), x, y, x, y)
    with pytest.raises(AgnnError):
        smote.SMOTE(dims=8, k=3).generate(x, 200, 3)
    meta = torch.zeros(12, 6, device="meta")
    with pytest.raises(AgnnError):
        smote._check_x(meta, "t")                                                            # not a HIP device
