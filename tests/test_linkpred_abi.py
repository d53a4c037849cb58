"""The link-prediction entry points (csrc/linkpred.hip) reject bad arguments with a message BEFORE any HIP call (safe on a CPU-only
host: the pointers below are never dereferenced): AGNN_EINVAL (-22) for sizes out of range, NULL pointers and too many tasks,
AGNN_EALIGN (-14) for a pointer off 16 bytes or a leading dimension that is no multiple of 4 floats, AGNN_ENOMEM (-12) for a
workspace that is too small.  Empty work is success and looks at no pointer."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # a 16-byte aligned non-null address, never read
EINVAL, EALIGN, ENOMEM = -22, -14, -12


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _task(**kw):
    from analysisgnn_amd import _lib
    d = dict(z=P, ld_z=32, n=100, src=P, dst=P, E=130, limit=80, t_rowptr=P, t_col=P, logit=P, label=P, g=P, loss=P, inv_cnt=P, counts=P)
    d.update(kw)
    t = _lib.LinkTask()
    for k, v in d.items():
        setattr(t, k, v)
    return t


def _bwd_item(**kw):
    from analysisgnn_amd import _lib
    d = dict(z=P, ld_z=32, n=100, g=P, E=130, s_rowptr=P, s_col=P, s_perm=P, d_rowptr=P, d_col=P, d_perm=P, dz=P, ld_dz=32)
    d.update(kw)
    t = _lib.LinkBwd()
    for k, v in d.items():
        setattr(t, k, v)
    return t


def _table(cls, items):
    arr = (cls * len(items))()
    for i, it in enumerate(items):
        arr[i] = it
    return arr


def _fwd(lib, tasks=None, H=32, ws=P, ws_bytes=1 << 20, **kw):
    from analysisgnn_amd import _lib
    tasks = [_task(**kw)] if tasks is None else tasks
    return lib.agnn_link_bce_fwd_f32(len(tasks), _table(_lib.LinkTask, tasks) if tasks else None, H, ws, ws_bytes, None)


def _bwd(lib, tasks=None, H=32, scale=P, **kw):
    from analysisgnn_amd import _lib
    tasks = [_bwd_item(**kw)] if tasks is None else tasks
    return lib.agnn_link_bce_bwd_f32(len(tasks), _table(_lib.LinkBwd, tasks) if tasks else None, H, scale, None)


def test_forward_arguments():
    lib = _lib()
    for H in (0, 2, 6, 30, -4):
        assert _fwd(lib, H=H) == EINVAL and f"H={H}".encode() in lib.agnn_last_error()
    assert _fwd(lib, tasks=[_task()] * 33) == EINVAL and b"n_tasks=33" in lib.agnn_last_error()
    assert lib.agnn_link_bce_fwd_f32(-1, None, 32, P, 64, None) == EINVAL and b"n_tasks=-1" in lib.agnn_last_error()
    assert lib.agnn_link_bce_fwd_f32(1, None, 32, P, 64, None) == EINVAL and b"tasks is null" in lib.agnn_last_error()
    assert _fwd(lib, E=-1) == EINVAL and b"E=-1" in lib.agnn_last_error()
    assert _fwd(lib, E=2 ** 31) == EINVAL and b"E=2147483648" in lib.agnn_last_error()
    assert _fwd(lib, n=-3) == EINVAL and b"n=-3" in lib.agnn_last_error()
    assert _fwd(lib, limit=101) == EINVAL and b"limit=101" in lib.agnn_last_error()
    assert _fwd(lib, limit=-1) == EINVAL and b"limit=-1" in lib.agnn_last_error()
    for name in ("z", "src", "dst", "t_rowptr", "t_col", "logit", "label", "g", "loss", "inv_cnt", "counts"):
        assert _fwd(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error() and name.encode() in lib.agnn_last_error(), name
    assert _fwd(lib, ld_z=28) == EINVAL and b"ld_z=28" in lib.agnn_last_error()
    assert _fwd(lib, ld_z=34) == EALIGN and b"ld_z=34" in lib.agnn_last_error()
    assert _fwd(lib, z=P + 4) == EALIGN and b" z " in lib.agnn_last_error()
    assert _fwd(lib, z=P + 8) == EALIGN
    assert _fwd(lib, ws=None) == EINVAL and b"workspace" in lib.agnn_last_error()
    assert _fwd(lib, ws_bytes=71) == ENOMEM and b"72 needed" in lib.agnn_last_error()        # 3 tiles of 64 candidates, 24 bytes each
    assert _fwd(lib, ws=P + 2) == EALIGN and b"workspace" in lib.agnn_last_error()
    assert _fwd(lib, tasks=[_task(), _task(E=-5)]) == EINVAL and b"task 1" in lib.agnn_last_error()   # every task of the table is checked


def test_workspace_size():
    from analysisgnn_amd import _lib as L
    lib = _lib()
    assert lib.agnn_link_bce_workspace_bytes(1, _table(L.LinkTask, [_task(E=130)])) == 72
    assert lib.agnn_link_bce_workspace_bytes(2, _table(L.LinkTask, [_task(E=64), _task(E=0)])) == 24
    assert lib.agnn_link_bce_workspace_bytes(0, None) == 0


def test_backward_arguments():
    lib = _lib()
    for H in (0, 3, 10):
        assert _bwd(lib, H=H) == EINVAL and f"H={H}".encode() in lib.agnn_last_error()
    assert _bwd(lib, tasks=[_bwd_item()] * 33) == EINVAL and b"n_tasks=33" in lib.agnn_last_error()
    assert lib.agnn_link_bce_bwd_f32(2, None, 32, P, None) == EINVAL and b"tasks is null" in lib.agnn_last_error()
    assert _bwd(lib, n=-1) == EINVAL and b"n=-1" in lib.agnn_last_error()
    assert _bwd(lib, E=-1) == EINVAL and b"E=-1" in lib.agnn_last_error()
    for name in ("z", "g", "s_rowptr", "s_col", "s_perm", "d_rowptr", "d_col", "d_perm", "dz"):
        assert _bwd(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error(), name
    assert _bwd(lib, scale=None) == EINVAL and b"scale" in lib.agnn_last_error()
    assert _bwd(lib, ld_dz=16) == EINVAL and b"ld_dz=16" in lib.agnn_last_error()
    assert _bwd(lib, ld_dz=38) == EALIGN and b"ld_dz=38" in lib.agnn_last_error()
    assert _bwd(lib, ld_z=28) == EINVAL and b"ld_z=28" in lib.agnn_last_error()
    assert _bwd(lib, ld_z=36 + 2) == EALIGN
    assert _bwd(lib, dz=P + 4) == EALIGN and b"dz" in lib.agnn_last_error()
    assert _bwd(lib, z=P + 8) == EALIGN and b" z " in lib.agnn_last_error()


def test_empty_work_succeeds_without_a_pointer():
    lib = _lib()
    assert lib.agnn_link_bce_fwd_f32(0, None, 32, None, 0, None) == 0
    assert lib.agnn_link_bce_bwd_f32(0, None, 32, None, None) == 0
    assert lib.agnn_link_bce_fwd_f32(0, None, 6, None, 0, None) == EINVAL                    # the shape rule still holds
    assert _bwd(lib, n=0, z=None, g=None, dz=None, s_rowptr=None, d_rowptr=None, scale=None) == 0    # no row to write
