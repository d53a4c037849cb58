"""The edge-term entry points (csrc/edgedec.hip) reject bad arguments with a message BEFORE any HIP call (safe on a CPU-only host:
the pointers below are never dereferenced): AGNN_EINVAL (-22) for sizes out of range, NULL pointers and too many relations,
AGNN_EALIGN (-14) for a pointer off 16 bytes or a leading dimension that is no multiple of 4 floats, AGNN_ENOMEM (-12) for a
workspace that is too small.  Empty work is success and looks at no pointer."""
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


def _keys(**kw):
    return _item("EdgeKeys", dict(src=P, dst=P, E=130, limit=80, pos0=7, key=P), kw)


def _pair(**kw):
    return _item("EdgePair", dict(a=P, ld_a=128, n=100, src=P, dst=P, E=130, limit=80, pos0=0, f=P, ld_f=32, label=P), kw)


def _pair_bwd(**kw):
    return _item("EdgePairBwd", dict(a=P, ld_a=128, n=100, df=P, ld_df=32, E=130, limit=80, pos0=0, s_rowptr=P, s_col=P, s_perm=P, d_rowptr=P,
                                     d_col=P, d_perm=P, da=P, ld_da=128), kw)


def _ce(**kw):
    return _item("EdgeCe", dict(y=P, ld_y=32, src=P, dst=P, label=P, E=130, limit=80, logit=P, dlogit=P, loss=P, inv_cnt=P, counts=P), kw)


def _ce_bwd(**kw):
    return _item("EdgeCeBwd", dict(y=P, ld_y=32, dlogit=P, E=130, dy=P, ld_dy=32), kw)


def _table(items):
    arr = (type(items[0]) * len(items))()
    for i, it in enumerate(items):
        arr[i] = it
    return arr


def _call_keys(lib, items=None, rng=P, **kw):
    items = [_keys(**kw)] if items is None else items
    return lib.agnn_edge_select_keys(len(items), _table(items), rng, 5, None)


def _call_pair(lib, items=None, H=32, labels=P, K=5, ldl=100, p=0.0, rng=None, **kw):
    items = [_pair(**kw)] if items is None else items
    return lib.agnn_edge_pair_fwd_f32(len(items), _table(items), H, labels, K, ldl, p, rng, 9, None, None)


def _call_pair_bwd(lib, items=None, H=32, p=0.0, rng=None, **kw):
    items = [_pair_bwd(**kw)] if items is None else items
    return lib.agnn_edge_pair_bwd_f32(len(items), _table(items), H, p, rng, 9, None)


def _call_ce(lib, items=None, H=32, w4=P, b4=P, smoothing=0.1, total=P, ws=P, ws_bytes=1 << 20, **kw):
    items = [_ce(**kw)] if items is None else items
    return lib.agnn_edge_ce_fwd_f32(len(items), _table(items), H, w4, b4, smoothing, total, ws, ws_bytes, None)


def _call_ce_bwd(lib, items=None, H=32, w4=P, scale=P, dw4=P, db4=P, ws=P, ws_bytes=1 << 24, **kw):
    items = [_ce_bwd(**kw)] if items is None else items
    return lib.agnn_edge_ce_bwd_f32(len(items), _table(items), H, w4, scale, dw4, db4, ws, ws_bytes, None)


CALLS = [(_call_pair, _pair), (_call_pair_bwd, _pair_bwd), (_call_ce, _ce), (_call_ce_bwd, _ce_bwd)]


def test_widths_and_table_sizes():
    lib = _lib()
    for call, item in CALLS:
        for H in (0, 2, 6, 30, -4, 516, 1024):
            assert call(lib, H=H) == EINVAL and f"H={H}".encode() in lib.agnn_last_error(), (call.__name__, H)
        assert call(lib, items=[item()] * 33) == EINVAL and b"n_rel=33" in lib.agnn_last_error()
        assert call(lib, items=[item(), item(E=-5)]) == EINVAL and b"relation 1" in lib.agnn_last_error()    # every entry is checked
        assert call(lib, E=2 ** 31) == EINVAL and b"E=2147483648" in lib.agnn_last_error()
    assert _call_keys(lib, items=[_keys()] * 33) == EINVAL and b"n_rel=33" in lib.agnn_last_error()
    assert lib.agnn_edge_pair_fwd_f32(1, None, 32, P, 5, 100, 0.0, None, 9, None, None) == EINVAL and b"rels is null" in lib.agnn_last_error()
    assert lib.agnn_edge_pair_bwd_f32(1, None, 32, 0.0, None, 9, None) == EINVAL and b"rels is null" in lib.agnn_last_error()
    assert lib.agnn_edge_ce_fwd_f32(1, None, 32, P, P, 0.1, P, P, 64, None) == EINVAL and b"rels is null" in lib.agnn_last_error()
    assert lib.agnn_edge_ce_bwd_f32(1, None, 32, P, P, P, P, P, 64, None) == EINVAL and b"rels is null" in lib.agnn_last_error()
    assert lib.agnn_edge_select_keys(-1, None, P, 5, None) == EINVAL and b"n_rel=-1" in lib.agnn_last_error()


def test_select_keys_arguments():
    lib = _lib()
    assert _call_keys(lib, E=-1) == EINVAL and b"E=-1" in lib.agnn_last_error()
    assert _call_keys(lib, limit=-1) == EINVAL and b"limit=-1" in lib.agnn_last_error()
    assert _call_keys(lib, pos0=-2) == EINVAL and b"pos0=-2" in lib.agnn_last_error()
    for name in ("src", "dst", "key"):
        assert _call_keys(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error(), name
    assert _call_keys(lib, rng=None) == EINVAL and b"rng_state" in lib.agnn_last_error()


def test_pair_forward_arguments():
    lib = _lib()
    assert _call_pair(lib, n=-3) == EINVAL and b"n=-3" in lib.agnn_last_error()
    assert _call_pair(lib, limit=101) == EINVAL and b"limit=101" in lib.agnn_last_error()
    assert _call_pair(lib, pos0=-1) == EINVAL and b"pos0=-1" in lib.agnn_last_error()
    for name in ("a", "src", "dst", "f", "label"):
        assert _call_pair(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error() and name.encode() in lib.agnn_last_error(), name
    assert _call_pair(lib, ld_a=28) == EINVAL and b"ld_a=28" in lib.agnn_last_error()
    assert _call_pair(lib, ld_a=130) == EALIGN and b"ld_a=130" in lib.agnn_last_error()
    assert _call_pair(lib, ld_f=34) == EALIGN and b"ld_f=34" in lib.agnn_last_error()
    assert _call_pair(lib, a=P + 4) == EALIGN and b" a " in lib.agnn_last_error()
    assert _call_pair(lib, f=P + 8) == EALIGN and b" f " in lib.agnn_last_error()
    assert _call_pair(lib, ldl=79) == EINVAL and b"ld_labels=79" in lib.agnn_last_error()
    assert _call_pair(lib, K=-1) == EINVAL and b"K=-1" in lib.agnn_last_error()
    for p in (-0.1, 1.0, float("nan")):
        assert _call_pair(lib, p=p, rng=P) == EINVAL and b"p=" in lib.agnn_last_error()
    assert _call_pair(lib, p=0.3, rng=None) == EINVAL and b"rng_state" in lib.agnn_last_error()      # dropout needs the counter


def test_pair_backward_arguments():
    lib = _lib()
    assert _call_pair_bwd(lib, n=-1) == EINVAL and b"n=-1" in lib.agnn_last_error()
    assert _call_pair_bwd(lib, limit=101) == EINVAL and b"limit=101" in lib.agnn_last_error()
    for name in ("a", "df", "s_rowptr", "s_col", "s_perm", "d_rowptr", "d_col", "d_perm", "da"):
        assert _call_pair_bwd(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error(), name
    assert _call_pair_bwd(lib, ld_da=16) == EINVAL and b"ld_da=16" in lib.agnn_last_error()
    assert _call_pair_bwd(lib, ld_da=38) == EALIGN and b"ld_da=38" in lib.agnn_last_error()
    assert _call_pair_bwd(lib, ld_df=28) == EINVAL and b"ld_df=28" in lib.agnn_last_error()
    assert _call_pair_bwd(lib, ld_a=130) == EALIGN
    assert _call_pair_bwd(lib, da=P + 4) == EALIGN and b"da" in lib.agnn_last_error()
    assert _call_pair_bwd(lib, df=P + 8) == EALIGN and b"df" in lib.agnn_last_error()
    assert _call_pair_bwd(lib, p=0.5, rng=None) == EINVAL and b"rng_state" in lib.agnn_last_error()


def test_cross_entropy_arguments():
    lib = _lib()
    assert _call_ce(lib, E=-1) == EINVAL and b"E=-1" in lib.agnn_last_error()
    assert _call_ce(lib, limit=-1) == EINVAL and b"limit=-1" in lib.agnn_last_error()
    for name in ("y", "src", "dst", "label", "logit", "dlogit", "loss", "inv_cnt", "counts"):
        assert _call_ce(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error() and name.encode() in lib.agnn_last_error(), name
    for name in ("w4", "b4", "total"):
        assert _call_ce(lib, **{name: None}) == EINVAL and name.encode() in lib.agnn_last_error(), name
    assert _call_ce(lib, ld_y=28) == EINVAL and b"ld_y=28" in lib.agnn_last_error()
    assert _call_ce(lib, ld_y=34) == EALIGN and b"ld_y=34" in lib.agnn_last_error()
    assert _call_ce(lib, y=P + 4) == EALIGN and b" y " in lib.agnn_last_error()
    assert _call_ce(lib, w4=P + 4) == EALIGN and b"w4" in lib.agnn_last_error()
    assert _call_ce(lib, logit=P + 4) == EALIGN and b"logit" in lib.agnn_last_error()
    assert _call_ce(lib, smoothing=1.5) == EINVAL and b"smoothing" in lib.agnn_last_error()
    assert _call_ce(lib, ws=None) == EINVAL and b"workspace" in lib.agnn_last_error()
    assert _call_ce(lib, ws_bytes=71) == ENOMEM and b"72 needed" in lib.agnn_last_error()           # 3 tiles of 64 edges, 24 bytes each
    assert _call_ce(lib, ws=P + 2) == EALIGN and b"workspace" in lib.agnn_last_error()


def test_cross_entropy_backward_arguments():
    lib = _lib()
    assert _call_ce_bwd(lib, E=-1) == EINVAL and b"E=-1" in lib.agnn_last_error()
    for name in ("y", "dlogit", "dy"):
        assert _call_ce_bwd(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error(), name
    for name in ("w4", "scale", "dw4", "db4"):
        assert _call_ce_bwd(lib, **{name: None}) == EINVAL and name.encode() in lib.agnn_last_error(), name
    assert _call_ce_bwd(lib, ld_dy=16) == EINVAL and b"ld_dy=16" in lib.agnn_last_error()
    assert _call_ce_bwd(lib, ld_y=38) == EALIGN and b"ld_y=38" in lib.agnn_last_error()
    assert _call_ce_bwd(lib, dy=P + 4) == EALIGN and b"dy" in lib.agnn_last_error()
    assert _call_ce_bwd(lib, dw4=P + 4) == EALIGN and b"dw4" in lib.agnn_last_error()
    assert _call_ce_bwd(lib, ws=None) == EINVAL and b"workspace" in lib.agnn_last_error()
    # 130 edges: one tile of 256; H = 32 -> groups of 8 lanes, 32 groups per workgroup, a slot of 2 * 32 + 4 floats each
    assert _call_ce_bwd(lib, ws_bytes=32 * 68 * 4 - 1) == ENOMEM and f"{32 * 68 * 4} needed".encode() in lib.agnn_last_error()
    assert _call_ce_bwd(lib, ws=P + 4) == EALIGN and b"workspace" in lib.agnn_last_error()


def test_workspace_sizes():
    lib = _lib()
    assert lib.agnn_edge_ce_workspace_bytes(1, _table([_ce(E=130)])) == 72
    assert lib.agnn_edge_ce_workspace_bytes(2, _table([_ce(E=64), _ce(E=0)])) == 24
    assert lib.agnn_edge_ce_workspace_bytes(0, None) == 0
    # backward: tiles of 256 edges x (256 / G) groups x (2 H + 4) floats, G = the power of two in [4, 64] covering H / 4
    assert lib.agnn_edge_ce_bwd_workspace_bytes(1, _table([_ce_bwd(E=130)]), 32) == 1 * 32 * 68 * 4
    assert lib.agnn_edge_ce_bwd_workspace_bytes(2, _table([_ce_bwd(E=257), _ce_bwd(E=1)]), 128) == 3 * 8 * 260 * 4
    assert lib.agnn_edge_ce_bwd_workspace_bytes(1, _table([_ce_bwd(E=256)]), 512) == 1 * 4 * 1028 * 4
    assert lib.agnn_edge_ce_bwd_workspace_bytes(1, _table([_ce_bwd(E=256)]), 4) == 1 * 64 * 12 * 4
    assert lib.agnn_edge_ce_bwd_workspace_bytes(1, _table([_ce_bwd(E=0)]), 32) == 0
    assert lib.agnn_edge_ce_bwd_workspace_bytes(1, _table([_ce_bwd(E=10)]), 6) == 0


def test_empty_work_succeeds_without_a_pointer():
    lib = _lib()
    assert lib.agnn_edge_select_keys(0, None, None, 5, None) == 0
    assert lib.agnn_edge_pair_fwd_f32(0, None, 32, None, 0, 0, 0.0, None, 9, None, None) == 0
    assert lib.agnn_edge_pair_bwd_f32(0, None, 32, 0.0, None, 9, None) == 0
    assert lib.agnn_edge_ce_fwd_f32(0, None, 32, None, None, 0.1, None, None, 0, None) == 0
    assert lib.agnn_edge_ce_bwd_f32(0, None, 32, None, None, None, None, None, 0, None) == 0
    assert lib.agnn_edge_pair_fwd_f32(0, None, 6, None, 0, 0, 0.0, None, 9, None, None) == EINVAL       # the shape rule still holds
    assert _call_keys(lib, E=0, src=None, dst=None, key=None, rng=None) == 0                           # a relation without edges
    assert _call_pair(lib, E=0, a=None, src=None, dst=None, f=None, label=None, labels=None) == 0
    assert _call_pair_bwd(lib, n=0, limit=0, a=None, df=None, da=None, s_rowptr=None, d_rowptr=None) == 0   # no row to write
