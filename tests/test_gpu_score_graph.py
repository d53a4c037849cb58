"""Score graph construction on the device (csrc/scoregraph.hip, analysisgnn_amd/score_graph.py): relation by relation, values and
edge order equal to the reference's own builder (tests/golden/score_graph_*.npz), to synth.make_score_graph / synth.collate and,
where neither has a case, to tests/score_graph_ref.py.  Every comparison is exact integer equality."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import score_graph_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_graph_*.npz")))
RELS = R.NOTE_RELATIONS
GUARD, MARK = 64, 0x5A5A5A5A5A5A


def _dev(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(DEV)


def _same_graph(g, edge_index, num_nodes, batch):
    """DeviceScoreGraph == (numpy edge dict, num_nodes, batch), key order included."""
    assert list(g.edge_index_dict) == list(edge_index)
    for et, e in edge_index.items():
        assert np.array_equal(g.edge_index_dict[et].cpu().numpy(), e), et
    assert g.num_nodes == num_nodes and list(g.num_nodes) == list(num_nodes)
    assert list(g.batch_dict) == list(batch)
    for t, b in batch.items():
        assert np.array_equal(g.batch_dict[t].cpu().numpy(), b), t
    assert g.metadata() == (list(num_nodes), list(edge_index))


def test_fixtures_present():
    assert len(GOLDEN) == 7


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[12:-4] for p in GOLDEN])
def test_equals_the_reference_builder(path):
    from analysisgnn_amd.score_graph import build_score_graph
    z = np.load(path)
    g = build_score_graph(_dev(z["onset_div"]), _dev(z["duration_div"]), self_loops=False)
    for r, rel in enumerate(RELS):
        assert np.array_equal(g.edge_index_dict[("note", rel, "note")].cpu().numpy(), z[rel].astype(np.int64)), rel
    assert g.totals[:4].tolist() == z["counts"].tolist()
    assert g.faults.tolist() == [0] * 8


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 500])
def test_equals_synth(n):
    from analysisgnn_amd import synth
    from analysisgnn_amd.score_graph import build_score_graph
    s = synth.make_score_graph(seed=n, n_notes=n, add_beats=True, add_measures=True, reverse_note_edges=True, reverse_metrical_edges=True)
    g = build_score_graph(_dev(s.onset_div), _dev(s.duration_div), add_beats=True, add_measures=True, reverse_note_edges=True,
                          reverse_metrical_edges=True)
    _same_graph(g, s.edge_index, s.num_nodes, s.batch)
    assert torch.equal(g.onset_div.cpu(), torch.from_numpy(s.onset_div)) and torch.equal(g.duration_div.cpu(), torch.from_numpy(s.duration_div))


def test_three_scores_in_one_call_equal_collate():
    """Onsets restart at 0 in every score: a search that leaves its slice, or a metrical id that is not offset, shows here."""
    from analysisgnn_amd import synth
    from analysisgnn_amd.score_graph import build_score_graph
    sizes = (1, 65, 130)
    kw = dict(add_beats=True, add_measures=True, reverse_note_edges=True, reverse_metrical_edges=True)
    c = synth.collate([synth.make_score_graph(seed=30 + i, n_notes=n, **kw) for i, n in enumerate(sizes)])
    starts = np.concatenate([[0], np.cumsum(sizes)])
    g = build_score_graph(_dev(c.onset_div), _dev(c.duration_div), starts, **kw)
    _same_graph(g, c.edge_index, c.num_nodes, c.batch)
    assert g.batch_dict["note"].agnn_target_lengths == list(sizes)
    for t in ("beat", "measure"):
        per = np.bincount(c.batch[t], minlength=3)
        assert np.array_equal(g.groups_per_score[t].cpu().numpy(), per)
        first = np.nonzero(np.diff(c.edge_index[("note", "connects", t)][1], prepend=-1))[0]
        assert np.array_equal(g.group_first[t].cpu().numpy(), first)


def _long_runs():
    """A 300-note chord; 300 single notes under one note that sustains over all of them (an onset run and a during run longer than
    256); then several distinct end times inside one silence: several `rest` source groups, one destination group."""
    on = [0] * 300 + [2] + list(range(2, 302)) + [410, 410, 410] + [420, 420]
    du = [2] * 300 + [400] + [1] * 300 + [1, 2, 3] + [4, 4]
    return np.asarray(on, dtype=np.int64), np.asarray(du, dtype=np.int64)


@pytest.mark.parametrize("self_loops", [True, False])
def test_long_runs_equal_the_numpy_rules(self_loops):
    from analysisgnn_amd.score_graph import build_score_graph
    on, du = _long_runs()
    ref = R.score_graph(on, du, self_loops=self_loops, add_beats=True, add_measures=True)
    e = ref["edge_index"]
    assert np.bincount(e[("note", "onset", "note")][0]).max() >= 299 and np.bincount(e[("note", "during", "note")][0]).max() == 299
    rest = e[("note", "rest", "note")]
    assert len(set(rest[0][np.isin(rest[1], (604, 605))].tolist())) == 3       # ends 411, 412, 413 -> the two notes at 420
    g = build_score_graph(_dev(on), _dev(du), self_loops=self_loops, add_beats=True, add_measures=True)
    _same_graph(g, e, ref["num_nodes"], ref["batch"])


def _exact_and_caps(on, du, starts, extra):
    from analysisgnn_amd.score_graph import build_score_graph
    kw = dict(add_beats=True, add_measures=True, reverse_note_edges=True, reverse_metrical_edges=True)
    exact = build_score_graph(_dev(on), _dev(du), starts, **kw)
    totals = dict(zip((*RELS, "beat", "measure"), exact.totals.tolist()))
    return exact, totals, {k: v + extra for k, v in totals.items()}, kw


def test_capacity_mode_pads_and_builds_the_same_csr():
    from analysisgnn_amd import synth
    from analysisgnn_amd.graph import SegSpec, build_csr
    from analysisgnn_amd.score_graph import build_score_graph
    c = synth.collate([synth.make_score_graph(seed=40 + i, n_notes=n) for i, n in enumerate((65, 130))])
    starts = [0, 65, 195]
    exact, totals, caps, kw = _exact_and_caps(c.onset_div, c.duration_div, starts, 7)
    g = build_score_graph(_dev(c.onset_div), _dev(c.duration_div), torch.tensor(starts, dtype=torch.int32, device=DEV), capacity=caps, **kw)
    assert not hasattr(g.batch_dict["note"], "agnn_target_lengths")      # score_start on the device is not read back in this mode
    assert list(g.edge_index_dict) == list(exact.edge_index_dict)
    assert g.totals.tolist() == exact.totals.tolist() and g.faults.tolist() == [0] * 8
    g.check()
    for et, e in exact.edge_index_dict.items():
        k = e.shape[1]
        p = g.edge_index_dict[et]
        pad = 0 if "note" in (et[0], et[2]) and et[0] != et[2] else 7       # one membership edge per note: nothing to pad
        assert p.shape[1] == k + pad and torch.equal(p[:, :k], e) and bool((p[:, k:] == -1).all()), et
    for t in ("beat", "measure"):
        k = totals[t]
        assert g.num_nodes[t] == k + 7 and torch.equal(g.batch_dict[t][:k], exact.batch_dict[t]) and bool((g.batch_dict[t][k:] == -1).all())
    n = g.num_nodes["note"]
    for rel in RELS:
        et = ("note", rel, "note")
        a, b = build_csr([SegSpec(row=g.edge_index_dict[et][1], col=g.edge_index_dict[et][0], n_rows=n),
                          SegSpec(row=exact.edge_index_dict[et][1], col=exact.edge_index_dict[et][0], n_rows=n)])
        k = totals[rel]
        assert torch.equal(a.rowptr - a.rowptr[0], b.rowptr - b.rowptr[0])
        assert torch.equal(a.col[int(a.rowptr[0]):int(a.rowptr[0]) + k], b.col[int(b.rowptr[0]):int(b.rowptr[0]) + k])


def _raw_build(on, du, starts, caps, flags=1):
    """agnn_score_graph_build into buffers with a guard region right behind every edge buffer."""
    from analysisgnn_amd import _lib
    lib = _lib.load()
    n, S = len(on), len(starts) - 1
    on_d, du_d = _dev(on), _dev(du)
    st = torch.tensor(starts, dtype=torch.int32, device=DEV)
    bufs = [torch.full((2 * c + GUARD,), MARK, dtype=torch.int64, device=DEV) for c in caps]
    totals = torch.zeros(4, dtype=torch.int64, device=DEV)
    faults = torch.zeros(8, dtype=torch.int32, device=DEV)
    ws_bytes = int(lib.agnn_score_graph_workspace_bytes(n, S))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    g = _lib.ScoreGraphArgs()
    g.onset_div, g.duration_div, g.score_start, g.n_notes, g.n_scores = on_d.data_ptr(), du_d.data_ptr(), st.data_ptr(), n, S
    g.flags, g.rev_mask, g.totals, g.note_score, g.faults = flags, 0, totals.data_ptr(), None, faults.data_ptr()
    for r in range(4):
        g.edges[r], g.cap[r] = bufs[r].data_ptr(), caps[r]
    _lib.check(lib.agnn_score_graph_build(g, ws.data_ptr(), ws_bytes, _lib.stream_ptr(DEV)), "agnn_score_graph_build")
    torch.cuda.synchronize()
    return bufs, totals.tolist(), faults.tolist()


def test_capacity_overflow_is_counted_and_writes_nothing_out_of_range():
    from analysisgnn_amd import _lib, synth
    from analysisgnn_amd.score_graph import build_score_graph
    s = synth.make_score_graph(seed=50, n_notes=130)
    ref = R.score_graph(s.onset_div, s.duration_div)["edge_index"]
    true = [ref[("note", rel, "note")].shape[1] for rel in RELS]
    word = _lib.status_word(DEV)
    before = int(word.item())
    for r, rel in enumerate(RELS):
        caps = list(true)
        caps[r] -= 1
        bufs, totals, faults = _raw_build(s.onset_div, s.duration_div, [0, 130], caps)
        assert totals == true                                          # the true totals, not the cut ones
        assert faults == [0, 0, 0] + [int(q == r) for q in range(4)] + [0], rel
        for q, rel_q in enumerate(RELS):
            c = caps[q]
            assert bool((bufs[q][2 * c:] == MARK).all()), (rel, rel_q)  # the guard behind the buffer is untouched
            e = bufs[q][:2 * c].view(2, c).cpu().numpy()
            assert np.array_equal(e, ref[("note", rel_q, "note")][:, :c]), (rel, rel_q)   # the prefix that fits is the real one
    caps = dict(zip(RELS, true))
    caps["during"] -= 1
    g = build_score_graph(_dev(s.onset_div), _dev(s.duration_div), capacity=caps)
    assert int(g.faults[3 + 2]) > 0
    with pytest.raises(_lib.AgnnError, match="during"):
        g.check()
    assert int(word.item()) == before                                  # the device status word is not involved
    _lib.check_device_status(DEV)


def test_bad_input_is_counted_not_written():
    from analysisgnn_amd import _lib, synth
    from analysisgnn_amd.score_graph import build_score_graph
    sizes = (65, 130, 33)
    graphs = [synth.make_score_graph(seed=60 + i, n_notes=n) for i, n in enumerate(sizes)]
    c = synth.collate(graphs)
    starts = [0, 65, 195, 228]
    on, du = c.onset_div.copy(), c.duration_div.copy()
    k = 65 + int(np.nonzero(np.diff(on[65:195]) > 0)[0][5])
    on[k], on[k + 1] = on[k + 1], on[k]                                # one swapped pair inside score 1
    du[200] = -3                                                       # one negative duration in score 2
    word = _lib.status_word(DEV)
    before = int(word.item())
    good = R.score_graph(c.onset_div[:65], c.duration_div[:65])["edge_index"]
    caps = [c.edge_index[("note", rel, "note")].shape[1] for rel in RELS]
    bufs, totals, faults = _raw_build(on, du, starts, caps)
    assert faults == [1, 1, 0, 0, 0, 0, 0, 0]
    for r, rel in enumerate(RELS):
        e0 = good[("note", rel, "note")]
        assert totals[r] == e0.shape[1]                                # the faulty scores get no edge, the clean one all of its own
        cap = caps[r]
        e = bufs[r][:2 * cap].view(2, cap).cpu().numpy()
        assert np.array_equal(e[:, :totals[r]], e0) and bool((e[:, totals[r]:] == -1).all()), rel
        assert bool((bufs[r][2 * cap:] == MARK).all()), rel
    g = build_score_graph(_dev(on), _dev(du), starts, capacity=dict(zip(RELS, caps)))
    assert g.faults[:2].tolist() == [1, 1]
    with pytest.raises(_lib.AgnnError, match="decrease.*negative"):
        g.check()
    with pytest.raises(_lib.AgnnError, match="decrease"):
        build_score_graph(_dev(on), _dev(du), starts)                  # exact mode checks by itself
    _, _, faults = _raw_build(c.onset_div, c.duration_div, [0, 65, 300, 228], caps)       # score_start that does not tile
    assert faults[2] == 1
    assert int(word.item()) == before
    _lib.check_device_status(DEV)


def test_sort_notes_restores_the_builders_order():
    from analysisgnn_amd import synth
    from analysisgnn_amd.score_graph import build_score_graph, sort_notes
    sizes = (65, 130)
    c = synth.collate([synth.make_score_graph(seed=70 + i, n_notes=n) for i, n in enumerate(sizes)])
    starts = [0, 65, 195]
    rng = np.random.default_rng(0)
    shuffle = np.concatenate([a + rng.permutation(b - a) for a, b in zip(starts[:-1], starts[1:])])
    pitch = np.arange(195)[shuffle]                                   # the original rank inside an onset group
    perm = sort_notes(_dev(c.onset_div[shuffle]), _dev(pitch), starts).cpu().numpy()
    assert np.array_equal(shuffle[perm], np.arange(195))
    g = build_score_graph(_dev(c.onset_div[shuffle][perm]), _dev(c.duration_div[shuffle][perm]), starts)
    _same_graph(g, c.edge_index, c.num_nodes, c.batch)


def test_predict_from_notes_equals_predict_on_synths_graph():
    from analysisgnn_amd import synth
    from analysisgnn_amd.models import TorchAnalysisGNN
    from analysisgnn_amd.postprocess import predict, predict_from_notes
    tasks = {"quality": 15, "inversion": 4, "degree1": 22, "degree2": 22, "localkey": 50, "cadence": 4}
    g = synth.make_batch(2, 60, first_seed=7, add_beats=True, add_measures=True, reverse_metrical_edges=True)
    torch.manual_seed(0)
    m = TorchAnalysisGNN(g.metadata(), 25, 256, 128, tasks, 2, dropout=0.3, use_jk=False, logit_fusion=True, encoder_type="hgt").to(DEV)
    I = synth.torch_inputs(g, 25, DEV, 0)
    exp = predict(m, I["pitch_spelling"], I["key_signature"], I["x_dict"], I["edge_index_dict"], I["batch_dict"],
                  onset_div=torch.from_numpy(g.onset_div).to(DEV))
    got = predict_from_notes(m, I["pitch_spelling"], I["key_signature"], I["x_dict"]["note"], _dev(g.onset_div), _dev(g.duration_div),
                             x_beat=I["x_dict"]["beat"], x_measure=I["x_dict"]["measure"], score_start=[0, 60, 120])
    assert list(got) == list(exp)
    for k in exp:
        assert torch.equal(got[k], exp[k]), k                          # same edges in the same order: the same kernels see the same bits


def test_score_store_from_notes_equals_the_store_of_numpy_graphs():
    from analysisgnn_amd import synth
    from analysisgnn_amd.batching import DeviceSampler, ScoreStore
    graphs = [synth.make_score_graph(seed=80 + i, n_notes=200, add_beats=True, add_measures=True) for i in range(3)]
    for g in graphs:
        g.edge_index = {et: e for et, e in g.edge_index.items() if et[0] == "note"}
    tasks = {"cadence": 4, "localkey": 50}
    a = ScoreStore(graphs, 25, DEV, tasks=tasks, seed=3)
    on, du = np.concatenate([g.onset_div for g in graphs]), np.concatenate([g.duration_div for g in graphs])
    b = ScoreStore.from_notes(on, du, [0, 200, 400, 600], 25, DEV, tasks=tasks, seed=3, add_beats=True, add_measures=True)
    assert a.edge_types == b.edge_types and a.group_types == b.group_types and a.num_notes == b.num_notes
    assert torch.equal(a.x, b.x) and torch.equal(a.attrs, b.attrs) and torch.equal(a.onset_div, b.onset_div)
    for ca, cb in zip(a.csr, b.csr):
        assert torch.equal(ca.rowptr, cb.rowptr)
    assert torch.equal(a.csr[0].col[:int(a.csr[-1].rowptr[-1])], b.csr[0].col[:int(b.csr[-1].rowptr[-1])])
    for t in a.group_types:
        assert torch.equal(a.group_of[t], b.group_of[t]) and torch.equal(a.group_x[t], b.group_x[t])
    wins = np.array([10, 430], dtype=np.int32)
    out = []
    for store in (a, b):
        smp = DeviceSampler(store, 2, 64, (3, 2), (32, 32), seed=5, group_capacity={"beat": 40, "measure": 12})
        smp.set_windows(wins)
        batch = smp.sample()
        torch.cuda.synchronize()
        out.append((smp.node_gid.clone(), {et: e.clone() for et, e in batch["edge_index_dict"].items()}))
    assert torch.equal(out[0][0], out[1][0]) and list(out[0][1]) == list(out[1][1])
    for et in out[0][1]:
        assert torch.equal(out[0][1][et], out[1][1][et]), et
