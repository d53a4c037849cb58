"""tests/score_graph_ref.py (the numpy restatement of the sorted-search rules of csrc/scoregraph.hip) pinned from both sides, no
GPU: against the reference's own builder (tests/golden/score_graph_*.npz, written by tests/gen_golden_score_graph.py) without
self loops, arrays compared in order; and against synth.make_score_graph with self loops, every flag combination.  synth keeps
its open tails (end times with no later onset), so the second comparison pins the skip rule."""
import glob
import itertools
import os

import numpy as np
import pytest

import score_graph_ref as R
from analysisgnn_amd import synth

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_graph_*.npz")))


def test_all_fixtures_present():
    assert [os.path.basename(p) for p in GOLDEN] == [f"score_graph_s{s}_n{n}.npz" for s, n in
                                                    ((0, 500), (1, 97), (2, 64), (3, 1), (4, 2), (5, 33), (6, 130))]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[12:-4] for p in GOLDEN])
def test_ref_equals_the_reference_builder(path):
    z = np.load(path)
    got = R.score_graph(z["onset_div"], z["duration_div"], self_loops=False)["edge_index"]
    for r, rel in enumerate(R.NOTE_RELATIONS):
        assert np.array_equal(got[("note", rel, "note")], z[rel].astype(np.int64)), rel
        assert got[("note", rel, "note")].shape[1] == int(z["counts"][r])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 500])
def test_ref_equals_synth_with_every_flag(n):
    on, du = synth._note_times(n, n)
    for beats, measures, rev in itertools.product((False, True), repeat=3):
        g = synth.make_score_graph(seed=n, n_notes=n, add_beats=beats, add_measures=measures, reverse_note_edges=rev,
                                   reverse_metrical_edges=rev)
        got = R.score_graph(on, du, add_beats=beats, add_measures=measures, reverse_note_edges=rev, reverse_metrical_edges=rev)
        assert list(got["edge_index"]) == list(g.edge_index)
        for et, e in g.edge_index.items():
            assert np.array_equal(got["edge_index"][et], e), (et, beats, measures, rev)
        assert got["num_nodes"] == g.num_nodes
        for t, b in g.batch.items():
            assert np.array_equal(got["batch"][t], b)


def test_ref_many_scores_equals_collate():
    sizes = (1, 65, 130)
    graphs = [synth.make_score_graph(seed=20 + i, n_notes=n, add_beats=True, add_measures=True, reverse_note_edges=True,
                                     reverse_metrical_edges=True) for i, n in enumerate(sizes)]
    c = synth.collate(graphs)
    got = R.score_graph(c.onset_div, c.duration_div, np.concatenate([[0], np.cumsum(sizes)]), add_beats=True, add_measures=True,
                        reverse_note_edges=True, reverse_metrical_edges=True)
    assert list(got["edge_index"]) == list(c.edge_index)
    for et, e in c.edge_index.items():
        assert np.array_equal(got["edge_index"][et], e), et
    assert got["num_nodes"] == c.num_nodes
    for t, b in c.batch.items():
        assert np.array_equal(got["batch"][t], b)
