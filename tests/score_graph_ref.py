"""Numpy restatement of the score graph rules of csrc/scoregraph.hip (no torch, no GPU): sorted searches inside every score's
slice, the stable order by end for `rest`, metrical groups, many scores in one call.  Checked in test_score_graph_ref.py against
the reference's own builder (tests/golden/score_graph_*.npz) and against synth.make_score_graph; the GPU tests compare the
kernels with it where neither of those two has a case (long runs)."""
import numpy as np

NOTE_RELATIONS = ("onset", "consecutive", "during", "rest")


def _runs(src, lo, hi):
    """(i, j) for j in [lo_i, hi_i), sources in the given order, destinations ascending."""
    n = np.maximum(hi - lo, 0)
    s = np.repeat(src, n)
    first = np.repeat(np.cumsum(n) - n, n)
    d = np.repeat(lo, n) + (np.arange(int(n.sum())) - first)
    return np.stack([s, d]).astype(np.int64).reshape(2, -1)


def note_relations(on, du, a=0, self_loops=True):
    """The four relations of ONE score whose notes have the global ids a .. a + n - 1."""
    on, du = np.asarray(on, dtype=np.int64), np.asarray(du, dtype=np.int64)
    n = on.size
    end = on + du
    ids = np.arange(n)
    lb_on, ub_on = np.searchsorted(on, on, "left"), np.searchsorted(on, on, "right")
    lb_end, ub_end = np.searchsorted(on, end, "left"), np.searchsorted(on, end, "right")
    onset = _runs(ids, lb_on, ub_on)
    if not self_loops:
        onset = onset[:, onset[0] != onset[1]]
    cons = _runs(ids, lb_end, ub_end)
    during = _runs(ids, ub_on, np.maximum(ub_on, lb_end))
    order = np.argsort(end, kind="stable")
    lbe = lb_end[order]
    ok = (lbe < n) & (on[np.minimum(lbe, n - 1)] != end[order])
    src, lo = order[ok], lbe[ok]
    rest = _runs(src, lo, np.searchsorted(on, on[lo], "right"))
    return [e + a for e in (onset, cons, during, rest)]


def groups(key, starts):
    """Compact group id per note (global over the scores), group count per score, group's score, group's first note."""
    key = np.asarray(key, dtype=np.int64)
    n = key.size
    flag = np.ones(n, dtype=bool)
    flag[1:] = key[1:] != key[:-1]
    flag[np.asarray(starts[:-1])[np.asarray(starts[:-1]) < n]] = True
    gid = np.cumsum(flag) - 1
    first = np.nonzero(flag)[0]
    score = np.searchsorted(starts, first, "right") - 1
    per_score = np.bincount(score, minlength=len(starts) - 1)
    return gid.astype(np.int64), per_score.astype(np.int64), score.astype(np.int64), first.astype(np.int64)


def score_graph(on, du, score_start=None, self_loops=True, add_beats=False, add_measures=False, reverse_note_edges=False,
                reverse_metrical_edges=False, divs_per_beat=4, beats_per_measure=4):
    """dict(edge_index={edge type: int64 [2, E]} in synth.make_score_graph's key order, num_nodes, batch)."""
    on, du = np.asarray(on, dtype=np.int64), np.asarray(du, dtype=np.int64)
    n = on.size
    starts = np.asarray([0, n] if score_start is None else score_start, dtype=np.int64)
    parts = [note_relations(on[a:b], du[a:b], a, self_loops) for a, b in zip(starts[:-1], starts[1:])]
    ei = {("note", rel, "note"): np.concatenate([p[r] for p in parts], axis=1) for r, rel in enumerate(NOTE_RELATIONS)}
    if reverse_note_edges:
        for rel in NOTE_RELATIONS[1:]:
            ei[("note", rel + "_rev", "note")] = ei[("note", rel, "note")][::-1].copy()
    num_nodes = {"note": n}
    batch = {"note": np.repeat(np.arange(starts.size - 1), np.diff(starts)).astype(np.int64)}
    ids = np.arange(n, dtype=np.int64)
    g = {}
    for t, on_flag, div in (("beat", add_beats, divs_per_beat), ("measure", add_measures, divs_per_beat * beats_per_measure)):
        if not on_flag:
            continue
        g[t] = groups(on // div, starts)
        num_nodes[t] = int(g[t][3].size)
        batch[t] = g[t][2]
        ei[("note", "connects", t)] = np.stack([ids, g[t][0]])
        if reverse_metrical_edges:
            ei[(t, "rev_connects", "note")] = np.stack([g[t][0], ids])
        if t == "measure" and "beat" in g:
            b2m = g["measure"][0][g["beat"][3]]                     # the measure of the beat's first note
            ei[("beat", "connects", "measure")] = np.stack([np.arange(b2m.size, dtype=np.int64), b2m])
            if reverse_metrical_edges:
                ei[("measure", "rev_connects", "beat")] = ei[("beat", "connects", "measure")][::-1].copy()
    return dict(edge_index=ei, num_nodes=num_nodes, batch=batch)
