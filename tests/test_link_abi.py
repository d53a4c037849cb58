"""The link-prediction entry points (csrc/linkpred.hip) reject bad arguments with a code and a message BEFORE any HIP call (safe on a
CPU-only host: the pointers below are never dereferenced), in the style of test_edge_abi.py.  The texts are exact: they are those
the library gave before its validators moved to csrc/peredge.h, so the test holds on either side of that move.  Empty work is
success and looks at no pointer."""
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


def _item(cls_name, defaults, kw):
    from analysisgnn_amd import _lib
    d = dict(defaults)
    d.update(kw)
    t = getattr(_lib, cls_name)()
    for k, v in d.items():
        setattr(t, k, v)
    return t


def _task(**kw):
    return _item("LinkTask", dict(z=P, ld_z=32, n=100, src=P, dst=P, E=130, limit=80, t_rowptr=P, t_col=P, logit=P, label=P, g=P, loss=P,
                                  inv_cnt=P, counts=P), kw)


def _bwd(**kw):
    return _item("LinkBwd", dict(z=P, ld_z=32, n=100, g=P, E=130, s_rowptr=P, s_col=P, s_perm=P, d_rowptr=P, d_col=P, d_perm=P, dz=P, ld_dz=32), kw)


def _table(items):
    arr = (type(items[0]) * len(items))()
    for i, it in enumerate(items):
        arr[i] = it
    return arr


def _call_fwd(lib, items=None, H=32, ws=P, ws_bytes=1 << 20, **kw):
    items = [_task(**kw)] if items is None else items
    return lib.agnn_link_bce_fwd_f32(len(items), _table(items), H, ws, ws_bytes, None)


def _call_bwd(lib, items=None, H=32, scale=P, **kw):
    items = [_bwd(**kw)] if items is None else items
    return lib.agnn_link_bce_bwd_f32(len(items), _table(items), H, scale, None)


def _refused(lib, rc, code, text):
    assert (rc, lib.agnn_last_error().decode()) == (code, text)


def test_widths_and_table_sizes():
    lib = _lib()
    for call, item, who in ((_call_fwd, _task, "link_bce_fwd"), (_call_bwd, _bwd, "link_bce_bwd")):
        for H in (0, 2, 6, 30, -4):
            _refused(lib, call(lib, H=H), EINVAL, f"{who}: H={H} must be a positive multiple of 4")
        _refused(lib, call(lib, items=[item()] * 33), EINVAL, f"{who}: n_tasks=33 must be in [0, 32]")
    _refused(lib, lib.agnn_link_bce_fwd_f32(-1, None, 32, P, 64, None), EINVAL, "link_bce_fwd: n_tasks=-1 must be in [0, 32]")
    _refused(lib, lib.agnn_link_bce_fwd_f32(1, None, 32, P, 64, None), EINVAL, "link_bce_fwd: tasks is null")
    _refused(lib, lib.agnn_link_bce_bwd_f32(1, None, 32, P, None), EINVAL, "link_bce_bwd: tasks is null")
    # every entry is checked, and named by its position
    _refused(lib, _call_fwd(lib, items=[_task(), _task(E=-5)]), EINVAL, "link_bce_fwd: task 1: E=-5 must be in [0, 2^31 - 64)")
    _refused(lib, _call_fwd(lib, items=[_task(), _task(ld_z=30)]), EINVAL, "link_bce_fwd: task 1: ld_z=30 < H=32")
    _refused(lib, _call_bwd(lib, items=[_bwd(), _bwd(n=-5)]), EINVAL, "link_bce_bwd: task 1: n=-5 must be in [0, 2^31)")


def test_forward_sizes():
    lib = _lib()
    _refused(lib, _call_fwd(lib, E=-1), EINVAL, "link_bce_fwd: task 0: E=-1 must be in [0, 2^31 - 64)")
    _refused(lib, _call_fwd(lib, E=2 ** 31 - 64), EINVAL, "link_bce_fwd: task 0: E=2147483584 must be in [0, 2^31 - 64)")
    _refused(lib, _call_fwd(lib, n=-3), EINVAL, "link_bce_fwd: task 0: n=-3 must be in [0, 2^31)")
    _refused(lib, _call_fwd(lib, n=2 ** 31), EINVAL, "link_bce_fwd: task 0: n=2147483648 must be in [0, 2^31)")
    _refused(lib, _call_fwd(lib, limit=-1), EINVAL, "link_bce_fwd: task 0: limit=-1 must be in [0, n=100]")
    _refused(lib, _call_fwd(lib, limit=101), EINVAL, "link_bce_fwd: task 0: limit=101 must be in [0, n=100]")


def test_forward_pointers_and_layout():
    lib = _lib()
    groups = {"loss / inv_cnt / counts": ("loss", "inv_cnt", "counts"), "src / dst": ("src", "dst"), "logit / label / g": ("logit", "label", "g"),
              "z": ("z",), "t_rowptr / t_col": ("t_rowptr", "t_col")}
    for text, names in groups.items():
        for name in names:
            _refused(lib, _call_fwd(lib, **{name: None}), EINVAL, f"link_bce_fwd: task 0: {text} is null")
    _refused(lib, _call_fwd(lib, ld_z=28), EINVAL, "link_bce_fwd: task 0: ld_z=28 < H=32")
    _refused(lib, _call_fwd(lib, ld_z=34), EALIGN, "link_bce_fwd: task 0: ld_z=34 is not a multiple of 4")
    _refused(lib, _call_fwd(lib, z=P + 4), EALIGN, "link_bce_fwd: task 0: z is not 16-byte aligned")
    # the order of the checks is part of what a caller sees: of two faults the earlier one is named
    _refused(lib, _call_fwd(lib, z=None, t_rowptr=None), EINVAL, "link_bce_fwd: task 0: z is null")
    _refused(lib, _call_fwd(lib, t_rowptr=None, ld_z=28), EINVAL, "link_bce_fwd: task 0: t_rowptr / t_col is null")


def test_forward_workspace():
    lib = _lib()
    _refused(lib, _call_fwd(lib, ws=None), EINVAL, "link_bce_fwd: workspace is null")
    _refused(lib, _call_fwd(lib, ws_bytes=71), ENOMEM, "link_bce_fwd: workspace of 71 bytes, 72 needed")      # 3 tiles of 64 candidates, 24 bytes each
    _refused(lib, _call_fwd(lib, ws=P + 2), EALIGN, "link_bce_fwd: workspace is not 4-byte aligned")
    assert lib.agnn_link_bce_workspace_bytes(1, _table([_task(E=130)])) == 72
    assert lib.agnn_link_bce_workspace_bytes(2, _table([_task(E=64), _task(E=0)])) == 24
    assert lib.agnn_link_bce_workspace_bytes(1, _table([_task(E=256 * 64 + 1)])) == 257 * 24
    assert lib.agnn_link_bce_workspace_bytes(0, None) == 0
    assert lib.agnn_link_bce_workspace_bytes(33, _table([_task()] * 33)) == 0
    assert lib.agnn_link_bce_workspace_bytes(1, None) == 0


def test_backward_arguments():
    lib = _lib()
    _refused(lib, _call_bwd(lib, n=-1), EINVAL, "link_bce_bwd: task 0: n=-1 must be in [0, 2^31)")
    _refused(lib, _call_bwd(lib, n=2 ** 31), EINVAL, "link_bce_bwd: task 0: n=2147483648 must be in [0, 2^31)")
    _refused(lib, _call_bwd(lib, E=-1), EINVAL, "link_bce_bwd: task 0: E=-1 must be in [0, 2^31)")
    _refused(lib, _call_bwd(lib, E=2 ** 31), EINVAL, "link_bce_bwd: task 0: E=2147483648 must be in [0, 2^31)")
    groups = {"dz": ("dz",), "s_rowptr / d_rowptr": ("s_rowptr", "d_rowptr"), "z / g": ("z", "g"),
              "a col / perm array": ("s_col", "s_perm", "d_col", "d_perm")}
    for text, names in groups.items():
        for name in names:
            _refused(lib, _call_bwd(lib, **{name: None}), EINVAL, f"link_bce_bwd: task 0: {text} is null")
    _refused(lib, _call_bwd(lib, scale=None), EINVAL, "link_bce_bwd: scale is null")
    _refused(lib, _call_bwd(lib, ld_dz=28), EINVAL, "link_bce_bwd: task 0: ld_dz=28 < H=32")
    _refused(lib, _call_bwd(lib, ld_dz=34), EALIGN, "link_bce_bwd: task 0: ld_dz=34 is not a multiple of 4")
    _refused(lib, _call_bwd(lib, dz=P + 8), EALIGN, "link_bce_bwd: task 0: dz is not 16-byte aligned")
    _refused(lib, _call_bwd(lib, ld_z=16), EINVAL, "link_bce_bwd: task 0: ld_z=16 < H=32")
    _refused(lib, _call_bwd(lib, ld_z=38), EALIGN, "link_bce_bwd: task 0: ld_z=38 is not a multiple of 4")
    _refused(lib, _call_bwd(lib, z=P + 4), EALIGN, "link_bce_bwd: task 0: z is not 16-byte aligned")
    _refused(lib, _call_bwd(lib, dz=None, s_rowptr=None), EINVAL, "link_bce_bwd: task 0: dz is null")
    _refused(lib, _call_bwd(lib, s_rowptr=None, ld_dz=28), EINVAL, "link_bce_bwd: task 0: s_rowptr / d_rowptr is null")


def test_empty_work_succeeds_without_a_pointer():
    lib = _lib()
    assert lib.agnn_link_bce_fwd_f32(0, None, 32, None, 0, None) == 0
    assert lib.agnn_link_bce_bwd_f32(0, None, 32, None, None) == 0
    assert lib.agnn_link_bce_fwd_f32(0, None, 6, None, 0, None) == EINVAL                               # the shape rule still holds
    assert _call_bwd(lib, n=0, z=None, g=None, dz=None, s_rowptr=None, d_rowptr=None, scale=None) == 0   # no row to write
    # a candidate list whose limit is 0 reads no row; a task without rows to write and without candidates needs no list
    _refused(lib, _call_fwd(lib, limit=0, z=None, t_rowptr=None, t_col=None, ws=None), EINVAL, "link_bce_fwd: workspace is null")
    _refused(lib, _call_bwd(lib, E=0, z=None, g=None, s_col=None, s_perm=None, d_col=None, d_perm=None, scale=None), EINVAL,
             "link_bce_bwd: scale is null")
