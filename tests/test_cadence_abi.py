"""The entry points of the class-balanced cross entropy (csrc/balce.hip) are declared in include/agnn.h, bound from there, and reject
bad arguments with a message BEFORE any HIP call (safe on a CPU-only host: the pointers below are never dereferenced): AGNN_EINVAL
(-22) for class counts outside [1, AGNN_BCE_MAX_CLASSES], a negative row count, a non-positive eps_w, NULL operands and leading
dimensions below the class count; AGNN_EALIGN (-14) for a workspace off 4 bytes; AGNN_ENOMEM (-12) for a workspace that is too
small.  No call here passes its checks: nothing is launched."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # an aligned non-null address, never read
EINVAL, EALIGN, ENOMEM = -22, -14, -12
NEW = ["agnn_balanced_ce_workspace_bytes", "agnn_balanced_ce_f32"]
N = 300


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _bce(lib, **kw):
    a = dict(logits=P, ld=5, n=N, C=5, labels=P, ignore=-100, eps_w=1e-6, count=P, weight=P, loss=P, d=P, ld_d=5, status=None, ws=P,
             ws_bytes=1 << 20)
    a.update(kw)
    return lib.agnn_balanced_ce_f32(a["logits"], a["ld"], a["n"], a["C"], a["labels"], a["ignore"], a["eps_w"], a["count"], a["weight"],
                                    a["loss"], a["d"], a["ld_d"], a["status"], a["ws"], a["ws_bytes"], None)


def test_declared_and_bound():
    from analysisgnn_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.CONSTS["AGNN_BCE_MAX_CLASSES"] >= 64
    assert _lib.SIGNATURES["agnn_balanced_ce_workspace_bytes"] == (C.c_size_t, [C.c_int64])
    res, args = _lib.SIGNATURES["agnn_balanced_ce_f32"]
    assert res is C.c_int and len(args) == 16 and args[2] is C.c_int64 and args[3] is C.c_int32 and args[6] is C.c_float


def test_balanced_ce_refusals():
    lib = _lib()
    from analysisgnn_amd import _lib as L
    cap = L.CONSTS["AGNN_BCE_MAX_CLASSES"]
    for c in (0, -1, cap + 1):
        assert _bce(lib, C=c, ld=max(c, 1), ld_d=max(c, 1)) == EINVAL and f"n_classes={c}".encode() in lib.agnn_last_error(), c
    assert _bce(lib, n=-1) == EINVAL and b"n_rows=-1" in lib.agnn_last_error()
    assert _bce(lib, n=2 ** 31) == EINVAL
    assert _bce(lib, eps_w=0.0) == EINVAL and b"eps_w" in lib.agnn_last_error()
    assert _bce(lib, eps_w=float("nan")) == EINVAL and b"eps_w" in lib.agnn_last_error()
    for name in ("loss", "ws"):
        assert _bce(lib, **{name: None}) == EINVAL and b"loss or workspace is null" in lib.agnn_last_error(), name
    for name in ("logits", "labels"):
        assert _bce(lib, **{name: None}) == EINVAL and b"logits or labels is null" in lib.agnn_last_error(), name
    assert _bce(lib, ld=4) == EINVAL and b"ld=4" in lib.agnn_last_error()
    assert _bce(lib, ld_d=3) == EINVAL and b"ld_d=3" in lib.agnn_last_error()
    assert _bce(lib, ws=P + 2) == EALIGN and b"workspace" in lib.agnn_last_error()
    need = lib.agnn_balanced_ce_workspace_bytes(N)
    assert _bce(lib, ws_bytes=need - 1) == ENOMEM and f"{need} needed".encode() in lib.agnn_last_error()
    assert _bce(lib, C=cap, ld=cap, ld_d=cap, ws_bytes=need - 1) == ENOMEM                                 # the widest head is a size, not a refusal


def test_workspace_size_is_monotone():
    lib = _lib()
    vals = [lib.agnn_balanced_ce_workspace_bytes(n) for n in (-1, 0, 1, 256, 257, 1000, 10 ** 6)]
    assert vals == sorted(vals) and vals[0] > 0 and vals[3] < vals[4] and all(v % 4 == 0 for v in vals)
