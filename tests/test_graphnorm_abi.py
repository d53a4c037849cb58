"""The entry points of GraphNorm (csrc/graphnorm.hip) are declared in include/agnn.h, bound from there, and reject bad arguments
with a message BEFORE any HIP call (safe on a CPU-only host: the pointers below are never dereferenced): AGNN_EINVAL (-22) for
sizes out of range and NULL pointers, AGNN_EALIGN (-14) for a pointer off its alignment or a leading dimension that is no multiple
of 4 floats, AGNN_ENOMEM (-12) for a workspace or a slab table that is too small, with the needed size named.  Empty work is
success and looks at no pointer."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # a 16-byte aligned non-null address, never read
EINVAL, EALIGN, ENOMEM = -22, -14, -12
NEW = ["agnn_graphnorm_table_bytes", "agnn_graphnorm_workspace_bytes", "agnn_graphnorm_slabs", "agnn_graphnorm_fwd_f32",
       "agnn_graphnorm_bwd_f32"]
N, G, C = 300, 3, 64
BOUND = (N + 127) // 128 + G                       # 6 slabs at the most
TABLE = (4 + 4 * BOUND) * 4                        # slab_off [G + 1 = 4], then 4 int32 per slab
WS = (3 * BOUND + 5 * G) * C * 4                   # slab sums [bound, 3, C], per-graph constants [G, 2, C] and terms [G, 3, C]


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _fwd(lib, **kw):
    a = dict(x=P, ld_x=C, n=N, G=G, C=C, seg_ptr=P, rows=P, table=P, table_bytes=1 << 20, weight=P, bias=P, mean_scale=P, eps=1e-5, y=P,
             ld_y=C, stats=P, workspace=P, ws_bytes=1 << 20)
    a.update(kw)
    return lib.agnn_graphnorm_fwd_f32(a["x"], a["ld_x"], a["n"], a["G"], a["C"], a["seg_ptr"], a["rows"], a["table"], a["table_bytes"],
                                      a["weight"], a["bias"], a["mean_scale"], a["eps"], a["y"], a["ld_y"], a["stats"], a["workspace"],
                                      a["ws_bytes"], None)


def _bwd(lib, **kw):
    a = dict(x=P, ld_x=C, n=N, G=G, C=C, seg_ptr=P, rows=P, table=P, table_bytes=1 << 20, weight=P, mean_scale=P, stats=P, dy=P, ld_dy=C,
             dx=P, ld_dx=C, dweight=P, dbias=P, dmean_scale=P, workspace=P, ws_bytes=1 << 20)
    a.update(kw)
    return lib.agnn_graphnorm_bwd_f32(a["x"], a["ld_x"], a["n"], a["G"], a["C"], a["seg_ptr"], a["rows"], a["table"], a["table_bytes"],
                                      a["weight"], a["mean_scale"], a["stats"], a["dy"], a["ld_dy"], a["dx"], a["ld_dx"], a["dweight"],
                                      a["dbias"], a["dmean_scale"], a["workspace"], a["ws_bytes"], None)


def _slabs(lib, **kw):
    a = dict(seg_ptr=P, n=N, G=G, table=P, table_bytes=1 << 20)
    a.update(kw)
    return lib.agnn_graphnorm_slabs(a["seg_ptr"], a["n"], a["G"], a["table"], a["table_bytes"], None)


def test_declared_and_bound():
    from analysisgnn_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.CONSTS["AGNN_GN_SLAB"] == 128 and _lib.CONSTS["AGNN_GN_JOIN_LANES"] == 16


def test_shapes():
    lib = _lib()
    for call in (_fwd, _bwd):
        for c in (0, 2, 6, -4, 63):
            assert call(lib, C=c) == EINVAL and f"C={c}".encode() in lib.agnn_last_error(), (call.__name__, c)
        assert call(lib, n=-1) == EINVAL and b"n=-1" in lib.agnn_last_error()
        assert call(lib, G=-1) == EINVAL and b"G=-1" in lib.agnn_last_error()
        assert call(lib, G=0) == EINVAL and b"G=0" in lib.agnn_last_error()                  # rows that belong to no graph
        assert call(lib, n=2 ** 31) == EINVAL and b"n=2147483648" in lib.agnn_last_error()   # row indices are int32
        assert call(lib, ld_x=60) == EINVAL and b"ld_x=60" in lib.agnn_last_error()
        assert call(lib, ld_x=66) == EALIGN and b"ld_x=66" in lib.agnn_last_error()
        assert call(lib, workspace=None) == EINVAL and b"workspace is null" in lib.agnn_last_error()
        assert call(lib, ws_bytes=WS - 1) == ENOMEM and f"{WS} needed".encode() in lib.agnn_last_error()
        assert call(lib, workspace=P + 8) == EALIGN and b"workspace" in lib.agnn_last_error()
        assert call(lib, table_bytes=TABLE - 1) == ENOMEM and f"{TABLE} needed".encode() in lib.agnn_last_error()
    assert _fwd(lib, eps=-1.0) == EINVAL and b"eps" in lib.agnn_last_error()
    assert _fwd(lib, eps=float("nan")) == EINVAL and b"eps" in lib.agnn_last_error()
    assert _slabs(lib, n=-1) == EINVAL and b"n=-1" in lib.agnn_last_error()
    assert _slabs(lib, G=-2) == EINVAL and b"G=-2" in lib.agnn_last_error()
    assert _slabs(lib, table_bytes=TABLE - 1) == ENOMEM and f"{TABLE} needed".encode() in lib.agnn_last_error()
    assert _slabs(lib, seg_ptr=None) == EINVAL and b"seg_ptr is null" in lib.agnn_last_error()
    assert _slabs(lib, table=None) == EINVAL and b"table is null" in lib.agnn_last_error()
    assert _slabs(lib, table=P + 4) == EALIGN and b"table" in lib.agnn_last_error()


def test_forward_operands():
    lib = _lib()
    for name in ("x", "weight", "bias", "mean_scale", "y", "stats", "table"):
        assert _fwd(lib, **{name: None}) == EINVAL and f"{name} is null".encode() in lib.agnn_last_error(), name
        assert _fwd(lib, **{name: P + 4}) == EALIGN and name.encode() in lib.agnn_last_error(), name
    for name in ("seg_ptr", "rows"):                                                         # int32 arrays: 4-byte alignment
        assert _fwd(lib, **{name: None}) == EINVAL and f"{name} is null".encode() in lib.agnn_last_error(), name
        assert _fwd(lib, **{name: P + 2}) == EALIGN and name.encode() in lib.agnn_last_error(), name
    assert _fwd(lib, ld_y=62) == EINVAL and b"ld_y=62" in lib.agnn_last_error()
    assert _fwd(lib, ld_y=70) == EALIGN and b"ld_y=70" in lib.agnn_last_error()


def test_backward_operands():
    lib = _lib()
    for name in ("x", "weight", "mean_scale", "stats", "dy", "dx", "dweight", "dbias", "dmean_scale", "table"):
        assert _bwd(lib, **{name: None}) == EINVAL and f"{name} is null".encode() in lib.agnn_last_error(), name
        assert _bwd(lib, **{name: P + 8}) == EALIGN and name.encode() in lib.agnn_last_error(), name
    for name in ("seg_ptr", "rows"):
        assert _bwd(lib, **{name: None}) == EINVAL and f"{name} is null".encode() in lib.agnn_last_error(), name
        assert _bwd(lib, **{name: P + 1}) == EALIGN and name.encode() in lib.agnn_last_error(), name
    assert _bwd(lib, ld_dy=32) == EINVAL and b"ld_dy=32" in lib.agnn_last_error()
    assert _bwd(lib, ld_dy=70) == EALIGN and b"ld_dy=70" in lib.agnn_last_error()
    assert _bwd(lib, ld_dx=60) == EINVAL and b"ld_dx=60" in lib.agnn_last_error()
    assert _bwd(lib, ld_dx=66) == EALIGN and b"ld_dx=66" in lib.agnn_last_error()


def test_sizes_are_monotone():
    lib = _lib()
    f, t = lib.agnn_graphnorm_workspace_bytes, lib.agnn_graphnorm_table_bytes
    assert f(0, 3, 64) == 0 and f(-5, 3, 64) == 0 and f(100, 0, 64) == 0 and f(100, 3, 0) == 0 and t(0, 3) == 0 and t(100, 0) == 0
    assert f(N, G, C) == WS and t(N, G) == TABLE
    assert f(1, 1, 4) == (3 * 2 + 5) * 4 * 4 and f(128, 1, 64) == (3 * 2 + 5) * 64 * 4 and f(129, 1, 64) == (3 * 3 + 5) * 64 * 4
    ns, gs, cs = [1, 2, 127, 128, 129, 1000, 10 ** 4, 10 ** 6], [1, 2, 3, 32, 300, 10 ** 5], [4, 8, 36, 64, 260, 3584]
    for g in gs:
        for c in cs:
            vals = [f(n, g, c) for n in ns]
            assert vals == sorted(vals) and vals[0] > 0
        vals = [t(n, g) for n in ns]
        assert vals == sorted(vals) and vals[0] > 0 and all(v % 16 == 0 for v in vals)
    for n in ns:
        for c in cs:
            vals = [f(n, g, c) for g in gs]
            assert vals == sorted(vals)
        for g in gs:
            vals = [f(n, g, c) for c in cs]
            assert vals == sorted(vals)
        vals = [t(n, g) for g in gs]
        assert vals == sorted(vals)


def test_empty_work_succeeds_without_a_pointer():
    lib = _lib()
    assert lib.agnn_graphnorm_fwd_f32(None, 0, 0, 3, 64, None, None, None, 0, None, None, None, 1e-5, None, 0, None, None, 0, None) == 0
    assert lib.agnn_graphnorm_fwd_f32(None, 0, 0, 0, 64, None, None, None, 0, None, None, None, 1e-5, None, 0, None, None, 0, None) == 0
    assert lib.agnn_graphnorm_bwd_f32(None, 0, 0, 3, 64, None, None, None, 0, None, None, None, None, 0, None, 0, None, None, None, None, 0,
                                      None) == 0
    assert lib.agnn_graphnorm_slabs(None, 0, 3, None, 0, None) == 0
    assert lib.agnn_graphnorm_fwd_f32(None, 0, 0, 3, 6, None, None, None, 0, None, None, None, 1e-5, None, 0, None, None, 0,
                                      None) == EINVAL                                      # the shape rule still holds
