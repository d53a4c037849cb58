"""The join's two entry points (csrc/pooljoin.hip) are declared in include/agnn.h, exported by the built library, bound from the
header, and reject bad arguments with a message BEFORE any HIP call (safe on a CPU-only host: the pointers below are never
dereferenced; no call here passes its checks, so nothing is launched).  The two cadence models construct on the CPU under the
reference's `state_dict` keys; `pool_norm` itself has no CPU path."""
import ctypes as C
import os
import re

import pytest
import torch

import cadence_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # an aligned non-null address, never read
EINVAL, EALIGN = -22, -14
NEW = ["agnn_pool_norm_f32", "agnn_pool_bwd_f32"]
MODELS = ["neighbor_h32", "pytorch_h32", "pytorch_ps_h32", "pytorch_hybrid_h32", "pytorch_eval_h32"]
N, H = 300, 64


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _rel(**kw):
    from analysisgnn_amd import _lib
    a = dict(src=None, rowptr=P, col=P, ld_src=0)
    a.update(kw)
    return _lib.make_rels([a])


def _fwd(lib, **kw):
    a = dict(rel=_rel(), x=P, ld_x=H, n=N, pool_rows=N, H=H, col_limit=N, flags=0, gamma=P, beta=P, eps=1e-5, u=2 * P, ld_u=H, y=3 * P, ld_y=H,
             mean=P, rstd=P, inv_cnt=P)
    a.update(kw)
    return lib.agnn_pool_norm_f32(a["rel"], a["x"], a["ld_x"], a["n"], a["pool_rows"], a["H"], a["col_limit"], a["flags"], a["gamma"], a["beta"],
                                  a["eps"], a["u"], a["ld_u"], a["y"], a["ld_y"], a["mean"], a["rstd"], a["inv_cnt"], None)


def _bwd(lib, **kw):
    a = dict(rel=_rel(), du=P, ld_du=H, inv_cnt=P, n=N, pool_rows=N, H=H, col_limit=N, flags=0, dx=2 * P, ld_dx=H)
    a.update(kw)
    return lib.agnn_pool_bwd_f32(a["rel"], a["du"], a["ld_du"], a["inv_cnt"], a["n"], a["pool_rows"], a["H"], a["col_limit"], a["flags"], a["dx"],
                                 a["ld_dx"], None)


def test_declared_exported_and_bound():
    from analysisgnn_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "agnn.h")).read()
    lib = _lib()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    res, args = L.SIGNATURES["agnn_pool_norm_f32"]
    assert res is C.c_int and len(args) == 19 and args[3] is C.c_int64 and args[5] is C.c_int32 and args[7] is C.c_uint32 and args[10] is C.c_float
    res, args = L.SIGNATURES["agnn_pool_bwd_f32"]
    assert res is C.c_int and len(args) == 12 and args[4] is C.c_int64 and args[6] is C.c_int32 and args[8] is C.c_uint32


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["pool_norm", "pool_bwd"])
def test_sizes_and_index_refused(call):
    lib = _lib()
    for h in (0, 6, 1028, -4):
        assert call(lib, H=h) == EINVAL and f"H={h}".encode() in lib.agnn_last_error(), h
    for pr in (0, N + 1, -1):
        assert call(lib, pool_rows=pr) == EINVAL and f"pool_rows={pr}".encode() in lib.agnn_last_error(), pr
    assert call(lib, n=-1) == EINVAL and call(lib, n=2 ** 31) == EINVAL
    assert call(lib, col_limit=-1) == EINVAL and b"col_limit=-1" in lib.agnn_last_error()
    assert call(lib, flags=1) == EINVAL and b"flags" in lib.agnn_last_error()            # AGNN_SPMM_MEAN is not this call's
    assert call(lib, flags=2 | 1024) == EINVAL
    assert call(lib, rel=None) == EINVAL and b"null index" in lib.agnn_last_error()
    assert call(lib, rel=_rel(rowptr=None)) == EINVAL and b"null index" in lib.agnn_last_error()
    assert call(lib, rel=_rel(col=None)) == EINVAL and b"null index" in lib.agnn_last_error()
    assert call(lib, rel=_rel(ew=P)) == EINVAL and b"per-edge weights" in lib.agnn_last_error()
    # no row: nothing to do, whatever the operands are; the width is still checked
    assert call(lib, n=0, pool_rows=0) == 0
    assert call(lib, n=0, pool_rows=0, H=6) == EINVAL


def test_pool_norm_operands_refused():
    lib = _lib()
    for name in ("x", "u", "y"):
        assert _fwd(lib, **{name: None}) == EINVAL and f"{name} is null".encode() in lib.agnn_last_error(), name
        assert _fwd(lib, **{"ld_" + name: H - 4}) == EINVAL and f"ld_{name}={H - 4}".encode() in lib.agnn_last_error(), name
        assert _fwd(lib, **{"ld_" + name: H + 2}) == EALIGN and f"ld_{name}={H + 2}".encode() in lib.agnn_last_error(), name
        assert _fwd(lib, **{name: 5 * P + 4}) == EALIGN and f"{name} is not 16-byte aligned".encode() in lib.agnn_last_error(), name
    for name in ("gamma", "beta", "mean", "rstd", "inv_cnt"):
        assert _fwd(lib, **{name: None}) == EINVAL and b"is null" in lib.agnn_last_error(), name
    for name in ("gamma", "beta"):
        assert _fwd(lib, **{name: P + 8}) == EALIGN and b"gamma and beta" in lib.agnn_last_error(), name
    assert _fwd(lib, u=P) == EINVAL and b"must not be x" in lib.agnn_last_error()
    assert _fwd(lib, y=P) == EINVAL and b"must not be x" in lib.agnn_last_error()
    for h in (4, 252, 1024):                                                          # the widths at the ends are sizes, not refusals
        assert _fwd(lib, H=h, ld_x=h, ld_u=h, ld_y=h, x=None) == EINVAL and b"x is null" in lib.agnn_last_error(), h


def test_pool_bwd_operands_refused():
    lib = _lib()
    for name in ("du", "dx"):
        assert _bwd(lib, **{name: None}) == EINVAL and f"{name} is null".encode() in lib.agnn_last_error(), name
        assert _bwd(lib, **{"ld_" + name: H - 4}) == EINVAL and f"ld_{name}={H - 4}".encode() in lib.agnn_last_error(), name
        assert _bwd(lib, **{"ld_" + name: H + 2}) == EALIGN and f"ld_{name}={H + 2}".encode() in lib.agnn_last_error(), name
        assert _bwd(lib, **{name: 5 * P + 4}) == EALIGN and f"{name} is not 16-byte aligned".encode() in lib.agnn_last_error(), name
    assert _bwd(lib, inv_cnt=None) == EINVAL and b"inv_cnt is null" in lib.agnn_last_error()
    assert _bwd(lib, dx=P) == EINVAL and b"must not be du" in lib.agnn_last_error()


def test_pool_norm_has_no_cpu_path():
    from analysisgnn_amd import cadence
    from analysisgnn_amd._abi import AgnnError
    ln = torch.nn.LayerNorm(8)
    e = torch.zeros(2, dtype=torch.long)
    with pytest.raises(AgnnError, match="HIP device"):
        cadence.pool_norm(torch.zeros(3, 8), e, e, ln)
    with pytest.raises(AgnnError, match="HIP device"):
        cadence.JoinNorm(8)(torch.zeros(3, 8), e, e)


@pytest.mark.parametrize("case", MODELS)
def test_models_construct_under_the_reference_keys(case):
    import analysisgnn_amd
    from analysisgnn_amd import cadence
    z = CR.load_case(case)
    cfg = CR.config(z)
    if cfg["kind"] == "neighbor":
        model = cadence.CadenceGNNNeighbor(cfg["metadata"], cfg["in_feats"], cfg["H"], CR.OUT, cfg["L"], dropout=0.0)
    else:
        model = cadence.CadenceGNNPytorch(cfg["metadata"], cfg["in_feats"], cfg["H"], CR.OUT, cfg["L"], dropout=0.0, hybrid=cfg["hybrid"],
                                          use_pitch_spelling=cfg["use_ps"])
        assert model.use_pitch_spelling == cfg["use_ps"] and model.hybrid == cfg["hybrid"]
    assert list(model.state_dict().keys()) == [str(k) for k in z["meta.keys"]]
    model.load_state_dict(CR.state(z), strict=True)
    assert isinstance(model.norm, torch.nn.LayerNorm)
    assert analysisgnn_amd.CadenceGNNNeighbor is cadence.CadenceGNNNeighbor and analysisgnn_amd.pool_norm is cadence.pool_norm
