"""The entry points of the column-statistics block (csrc/colnorm.hip) and of onset pooling with selection (csrc/onsetpool.hip) are
declared in include/agnn.h, bound from there, and reject bad arguments with a message BEFORE any HIP call (safe on a CPU-only
host: the pointers below are never dereferenced): AGNN_EINVAL (-22) for sizes out of range and NULL pointers, AGNN_EALIGN (-14)
for a pointer off 16 bytes or a leading dimension that is no multiple of 4 floats, AGNN_ENOMEM (-12) for a workspace that is too
small.  Empty work is success and looks at no pointer."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # a 16-byte aligned non-null address, never read
EINVAL, EALIGN, ENOMEM = -22, -14, -12
RELU, TRAIN = 1, 2
NEW = ["agnn_colnorm_workspace_bytes", "agnn_colnorm_fwd_f32", "agnn_colnorm_bwd_f32", "agnn_onset_pool_fwd_f32", "agnn_onset_pool_bwd_f32"]


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _fwd(lib, **kw):
    a = dict(x=P, ld_x=64, n=300, C=64, gamma=P, beta=P, rm=P, rv=P, nbt=P, eps=1e-5, mom=0.1, p=0.0, flags=RELU | TRAIN, rng=None,
             call=7, y=P, ld_y=64, stats=P, used=None, ws=P, ws_bytes=1 << 20)
    a.update(kw)
    return lib.agnn_colnorm_fwd_f32(a["x"], a["ld_x"], a["n"], a["C"], a["gamma"], a["beta"], a["rm"], a["rv"], a["nbt"], a["eps"], a["mom"],
                                    a["p"], a["flags"], a["rng"], a["call"], a["y"], a["ld_y"], a["stats"], a["used"], a["ws"], a["ws_bytes"], None)


def _bwd(lib, **kw):
    a = dict(x=P, ld_x=64, n=300, C=64, gamma=P, stats=P, p=0.0, flags=RELU | TRAIN, rng=None, call=7, dy=P, ld_dy=64, dx=P, ld_dx=64,
             dgamma=P, dbeta=P, ws=P, ws_bytes=1 << 20)
    a.update(kw)
    return lib.agnn_colnorm_bwd_f32(a["x"], a["ld_x"], a["n"], a["C"], a["gamma"], a["stats"], a["p"], a["flags"], a["rng"], a["call"],
                                    a["dy"], a["ld_dy"], a["dx"], a["ld_dx"], a["dgamma"], a["dbeta"], a["ws"], a["ws_bytes"], None)


def _pool(lib, **kw):
    a = dict(a=P, ld_a=32, n=100, H=32, rowptr=P, col=P, idx=P, K=40, out=P, ld_out=32, status=None)
    a.update(kw)
    return lib.agnn_onset_pool_fwd_f32(a["a"], a["ld_a"], a["n"], a["H"], a["rowptr"], a["col"], a["idx"], a["K"], a["out"], a["ld_out"],
                                       a["status"], None)


def _pool_bwd(lib, **kw):
    a = dict(g=P, ld_g=32, K=40, H=32, n=100, d_rowptr=P, s_rowptr=P, s_col=P, sel_rowptr=P, sel_k=P, da=P, ld_da=32)
    a.update(kw)
    return lib.agnn_onset_pool_bwd_f32(a["g"], a["ld_g"], a["K"], a["H"], a["n"], a["d_rowptr"], a["s_rowptr"], a["s_col"], a["sel_rowptr"],
                                       a["sel_k"], a["da"], a["ld_da"], None)


def test_declared_and_bound():
    from analysisgnn_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.CONSTS["AGNN_CN_RELU"] == RELU and _lib.CONSTS["AGNN_CN_TRAIN"] == TRAIN
    assert _lib.CONSTS["AGNN_CN_SLAB"] == 128 and _lib.CONSTS["AGNN_CN_FINAL_LANES"] == 16


def test_colnorm_shapes():
    lib = _lib()
    for call in (_fwd, _bwd):
        for C in (0, 2, 6, 30, -4, 63):
            assert call(lib, C=C) == EINVAL and f"C={C}".encode() in lib.agnn_last_error(), (call.__name__, C)
        assert call(lib, n=-1) == EINVAL and b"n=-1" in lib.agnn_last_error()
        assert call(lib, n=1) == EINVAL and b"n=1" in lib.agnn_last_error()                 # batch statistics of one row
        assert call(lib, ld_x=60) == EINVAL and b"ld_x=60" in lib.agnn_last_error()
        assert call(lib, ld_x=66) == EALIGN and b"ld_x=66" in lib.agnn_last_error()
        assert call(lib, x=P + 4) == EALIGN and b"x is not 16-byte aligned" in lib.agnn_last_error()       # a misaligned row
        assert call(lib, x=None) == EINVAL and b"x is null" in lib.agnn_last_error()
        assert call(lib, flags=8) == EINVAL and b"flags" in lib.agnn_last_error()
        for p in (-0.1, 1.0, float("nan")):
            assert call(lib, p=p, rng=P) == EINVAL and b"p=" in lib.agnn_last_error()
        assert call(lib, p=0.5, rng=None) == EINVAL and b"rng_state" in lib.agnn_last_error()
        assert call(lib, ws=None) == EINVAL and b"workspace is null" in lib.agnn_last_error()
        need = 3 * 2 * 64 * 4                                                               # 300 rows: 3 slabs of (2, C) floats
        assert call(lib, ws_bytes=need - 1) == ENOMEM and f"{need} needed".encode() in lib.agnn_last_error()
        assert call(lib, ws=P + 8) == EALIGN and b"workspace" in lib.agnn_last_error()


def test_colnorm_forward_arguments():
    lib = _lib()
    for name in ("gamma", "beta", "y", "stats"):
        assert _fwd(lib, **{name: None}) == EINVAL and f"{name} is null".encode() in lib.agnn_last_error(), name
        assert _fwd(lib, **{name: P + 4}) == EALIGN and name.encode() in lib.agnn_last_error(), name
    assert _fwd(lib, ld_y=62) == EINVAL and b"ld_y=62" in lib.agnn_last_error()
    assert _fwd(lib, ld_y=70) == EALIGN and b"ld_y=70" in lib.agnn_last_error()
    assert _fwd(lib, rm=None) == EINVAL and b"go together" in lib.agnn_last_error()
    assert _fwd(lib, rm=None, rv=None, nbt=None, flags=RELU) == EINVAL and b"running statistics" in lib.agnn_last_error()
    assert _fwd(lib, rv=P + 4) == EALIGN and b"running_var" in lib.agnn_last_error()
    assert _fwd(lib, mom=1.5) == EINVAL and b"momentum" in lib.agnn_last_error()
    assert _fwd(lib, eps=-1.0) == EINVAL and b"eps" in lib.agnn_last_error()


def test_colnorm_backward_arguments():
    lib = _lib()
    for name in ("gamma", "stats", "dy", "dx", "dgamma", "dbeta"):
        assert _bwd(lib, **{name: None}) == EINVAL and f"{name} is null".encode() in lib.agnn_last_error(), name
        assert _bwd(lib, **{name: P + 8}) == EALIGN and name.encode() in lib.agnn_last_error(), name
    assert _bwd(lib, ld_dy=32) == EINVAL and b"ld_dy=32" in lib.agnn_last_error()
    assert _bwd(lib, ld_dx=66) == EALIGN and b"ld_dx=66" in lib.agnn_last_error()


def test_onset_pool_arguments():
    lib = _lib()
    for call in (_pool, _pool_bwd):
        for H in (0, 2, 6, 30, -4):
            assert call(lib, H=H) == EINVAL and f"H={H}".encode() in lib.agnn_last_error(), (call.__name__, H)
        assert call(lib, n=-1) == EINVAL and b"n=-1" in lib.agnn_last_error()
        assert call(lib, n=2 ** 31) == EINVAL and b"n=2147483648" in lib.agnn_last_error()   # int32 edge ends could not name every row
        assert call(lib, K=-2) == EINVAL and b"n_sel=-2" in lib.agnn_last_error()
        assert call(lib, K=2 ** 31 + 1) == EINVAL and b"n_sel" in lib.agnn_last_error()       # int32 positions in the selection index
    assert _pool(lib, n=0) == EINVAL and b"out of n=0" in lib.agnn_last_error()               # any idx would be out of range
    for name in ("a", "out"):
        assert _pool(lib, **{name: None}) == EINVAL and f"{name} is null".encode() in lib.agnn_last_error(), name
        assert _pool(lib, **{name: P + 4}) == EALIGN and name.encode() in lib.agnn_last_error(), name
    for name in ("rowptr", "col", "idx"):
        assert _pool(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error(), name
    assert _pool(lib, ld_a=28) == EINVAL and b"ld_a=28" in lib.agnn_last_error()
    assert _pool(lib, ld_a=34) == EALIGN and b"ld_a=34" in lib.agnn_last_error()
    assert _pool(lib, ld_out=30) == EINVAL and b"ld_out=30" in lib.agnn_last_error()
    for name in ("g", "da"):
        assert _pool_bwd(lib, **{name: None}) == EINVAL and f"{name} is null".encode() in lib.agnn_last_error(), name
        assert _pool_bwd(lib, **{name: P + 4}) == EALIGN and name.encode() in lib.agnn_last_error(), name
    for name in ("d_rowptr", "s_rowptr", "s_col", "sel_rowptr", "sel_k"):
        assert _pool_bwd(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error(), name
    assert _pool_bwd(lib, ld_da=38) == EALIGN and b"ld_da=38" in lib.agnn_last_error()
    assert _pool_bwd(lib, ld_g=16) == EINVAL and b"ld_g=16" in lib.agnn_last_error()


def test_workspace_sizes_are_monotone():
    lib = _lib()
    f = lib.agnn_colnorm_workspace_bytes
    assert f(0, 64) == 0 and f(-5, 64) == 0 and f(100, 0) == 0
    assert f(1, 4) == 2 * 4 * 4 and f(128, 64) == 2 * 64 * 4 and f(129, 64) == 2 * 2 * 64 * 4
    ns, cs = [1, 2, 127, 128, 129, 1000, 2176, 2177, 10 ** 6], [4, 8, 36, 224, 260, 3584]
    for C in cs:
        vals = [f(n, C) for n in ns]
        assert vals == sorted(vals) and vals[0] > 0
    for n in ns:
        vals = [f(n, C) for C in cs]
        assert vals == sorted(vals)


def test_empty_work_succeeds_without_a_pointer():
    lib = _lib()
    assert lib.agnn_colnorm_fwd_f32(None, 0, 0, 64, None, None, None, None, None, 1e-5, 0.1, 0.0, RELU | TRAIN, None, 1, None, 0, None, None,
                                    None, 0, None) == 0
    assert lib.agnn_colnorm_bwd_f32(None, 0, 0, 64, None, None, 0.0, TRAIN, None, 1, None, 0, None, 0, None, None, None, 0, None) == 0
    assert lib.agnn_onset_pool_fwd_f32(None, 0, 100, 32, None, None, None, 0, None, 0, None, None) == 0
    assert lib.agnn_onset_pool_fwd_f32(None, 0, 0, 32, None, None, None, 0, None, 0, None, None) == 0
    assert lib.agnn_onset_pool_bwd_f32(None, 0, 0, 32, 0, None, None, None, None, None, None, 0, None) == 0
    assert lib.agnn_colnorm_fwd_f32(None, 0, 0, 6, None, None, None, None, None, 1e-5, 0.1, 0.0, 0, None, 1, None, 0, None, None, None, 0,
                                    None) == EINVAL                                       # the shape rule still holds
