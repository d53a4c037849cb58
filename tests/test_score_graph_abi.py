"""The score graph entry points (csrc/scoregraph.hip) are bound from include/agnn.h and reject bad arguments with a message BEFORE
any kernel is launched (safe on a CPU-only host: the pointers below are never dereferenced): AGNN_EINVAL (-22) for NULL pointers,
n_scores < 1, n_notes < 1 and negative capacities, AGNN_ENOMEM (-12) for a workspace that is too small."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # an aligned non-null address, never read
EINVAL, ENOMEM = -22, -12
CALLS = ("agnn_score_graph_count", "agnn_score_graph_fill", "agnn_score_graph_build")


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _graph(**kw):
    from analysisgnn_amd import _lib
    d = dict(onset_div=P, duration_div=P, score_start=P, n_notes=100, n_scores=2, flags=1, rev_mask=0, totals=P, note_score=P, faults=P)
    d.update({k: v for k, v in kw.items() if k not in ("edges", "cap")})
    g = _lib.ScoreGraphArgs()
    for k, v in d.items():
        setattr(g, k, v)
    for r in range(4):
        g.edges[r] = kw.get("edges", [P] * 4)[r]
        g.cap[r] = kw.get("cap", [64] * 4)[r]
    return g


def _groups(**kw):
    from analysisgnn_amd import _lib
    d = dict(key=P, div=4, score_start=P, n_notes=100, n_scores=2, rev=0, parent_of=None, note_edge=P, cap=10, group_score=P,
             group_first=P, parent_edge=None, per_score=P, total=P, faults=P)
    d.update(kw)
    g = _lib.ScoreGroupsArgs()
    for k, v in d.items():
        setattr(g, k, v)
    return g


def test_names_are_bound_from_the_header():
    from analysisgnn_amd import _lib
    for name in (*CALLS, "agnn_score_graph_workspace_bytes", "agnn_score_groups", "agnn_score_groups_workspace_bytes"):
        assert name in _lib.SIGNATURES, name
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    assert [f[0] for f in _lib.ScoreGraphArgs._fields_] == ["onset_div", "duration_div", "score_start", "n_notes", "n_scores", "flags",
                                                            "rev_mask", "edges", "cap", "totals", "note_score", "faults"]
    assert _lib.CONSTS["AGNN_SG_FAULT_WORDS"] == 8 and _lib.CONSTS["AGNN_SG_FAULT_OVERFLOW"] + 3 < _lib.CONSTS["AGNN_SG_FAULT_GROUPS"]
    from analysisgnn_amd import score_graph
    assert sorted(score_graph.FAULT_NAMES) == list(range(8))


def test_graph_arguments():
    lib = _lib()
    big = 1 << 30
    for name in CALLS:
        f = getattr(lib, name)
        assert f(None, P, big, None) == EINVAL and b"g is null" in lib.agnn_last_error()
        for s in (0, -1):
            assert f(_graph(n_scores=s), P, big, None) == EINVAL and f"n_scores={s}".encode() in lib.agnn_last_error()
        for n in (0, -5, 1 << 29):
            assert f(_graph(n_notes=n), P, big, None) == EINVAL and f"n_notes={n}".encode() in lib.agnn_last_error()
        for field in ("onset_div", "duration_div", "score_start", "totals", "faults"):
            assert f(_graph(**{field: None}), P, big, None) == EINVAL and b"null" in lib.agnn_last_error(), field
        assert f(_graph(), None, big, None) == EINVAL and b"workspace is null" in lib.agnn_last_error()
        assert f(_graph(), P, 16, None) == ENOMEM and b"needed" in lib.agnn_last_error()
    for name in CALLS[1:]:                                  # the calls that write edges
        f = getattr(lib, name)
        assert f(_graph(cap=[64, -1, 64, 64]), P, big, None) == EINVAL and b"cap[1]=-1" in lib.agnn_last_error()
        assert f(_graph(edges=[P, P, None, P]), P, big, None) == EINVAL and b"edges[2] is null" in lib.agnn_last_error()


def test_groups_arguments():
    lib = _lib()
    big = 1 << 30
    f = lib.agnn_score_groups
    assert f(None, P, big, None) == EINVAL and b"g is null" in lib.agnn_last_error()
    assert f(_groups(n_scores=0), P, big, None) == EINVAL and b"n_scores=0" in lib.agnn_last_error()
    assert f(_groups(n_notes=0), P, big, None) == EINVAL and b"n_notes=0" in lib.agnn_last_error()
    assert f(_groups(div=0), P, big, None) == EINVAL and b"div=0" in lib.agnn_last_error()
    assert f(_groups(cap=-2), P, big, None) == EINVAL and b"cap=-2" in lib.agnn_last_error()
    for field in ("key", "score_start", "note_edge", "faults"):
        assert f(_groups(**{field: None}), P, big, None) == EINVAL and b"null" in lib.agnn_last_error(), field
    assert f(_groups(parent_edge=P), P, big, None) == EINVAL and b"parent_of" in lib.agnn_last_error()
    assert f(_groups(), None, big, None) == EINVAL and b"workspace is null" in lib.agnn_last_error()
    assert f(_groups(), P, 16, None) == ENOMEM and b"needed" in lib.agnn_last_error()


def test_workspace_sizes():
    lib = _lib()
    assert lib.agnn_score_graph_workspace_bytes(0, 1) == 0 and lib.agnn_score_graph_workspace_bytes(10, 0) == 0
    assert lib.agnn_score_groups_workspace_bytes(0) == 0
    a, b = lib.agnn_score_graph_workspace_bytes(500, 1), lib.agnn_score_graph_workspace_bytes(16000, 32)
    assert 0 < a < b
    assert 0 < lib.agnn_score_groups_workspace_bytes(500) < lib.agnn_score_groups_workspace_bytes(16000)
