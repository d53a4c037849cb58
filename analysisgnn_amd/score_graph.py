"""Score graphs built on the device (csrc/scoregraph.hip): from a note array — onsets and durations in divs, which any score
parser yields — to the `edge_index_dict` the models, `postprocess.predict` and `ScoreStore` consume, without leaving the device.
Replaces the reference's in-tree builder `hetero_graph_from_note_array` (analysisgnn/utils/hgraph.py:214-300, an O(N^2) Python
loop) and graphmuse's `create_score_graph` in `predict` (models/analysis.py:1527-1543); the edge rules, the edge order and the
names are those of `synth.make_score_graph` ("Score graph construction").  No CPU path."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .synth import NOTE_RELATIONS

EdgeType = Tuple[str, str, str]
FAULT_WORDS = _lib.CONSTS["AGNN_SG_FAULT_WORDS"]
FAULT_NAMES = {
    _lib.CONSTS["AGNN_SG_FAULT_ORDER"]: "onsets (or metrical keys) that decrease inside a score",
    _lib.CONSTS["AGNN_SG_FAULT_RANGE"]: "negative values or onset + duration >= 2^31",
    _lib.CONSTS["AGNN_SG_FAULT_SCORES"]: "score_start does not tile the notes",
    **{_lib.CONSTS["AGNN_SG_FAULT_OVERFLOW"] + r: f"more `{rel}` edges than capacity" for r, rel in enumerate(NOTE_RELATIONS)},
    _lib.CONSTS["AGNN_SG_FAULT_GROUPS"]: "more beats or measures than capacity",
}
GROUP_TYPES = ("beat", "measure")


class DeviceScoreGraph:
    """What `build_score_graph` returns; the attributes are device tensors (or dicts of them) except `num_nodes`."""

    def __init__(self, edge_index_dict, num_nodes, batch_dict, onset_div, duration_div, totals, faults, group_first, per_score):
        self.edge_index_dict: Dict[EdgeType, torch.Tensor] = edge_index_dict
        self.num_nodes: Dict[str, int] = num_nodes
        self.batch_dict: Dict[str, torch.Tensor] = batch_dict
        self.onset_div, self.duration_div = onset_div, duration_div
        self.totals = totals            # int64 [6]: onset, consecutive, during, rest edges; beats; measures (real counts)
        self.faults = faults            # int32 [AGNN_SG_FAULT_WORDS]: bad input, counted per kind
        self.group_first: Dict[str, torch.Tensor] = group_first      # per beat / measure its first note
        self.groups_per_score: Dict[str, torch.Tensor] = per_score   # per score its number of beats / measures

    def metadata(self) -> Tuple[List[str], List[EdgeType]]:
        return list(self.num_nodes), list(self.edge_index_dict)

    def check(self) -> None:
        """Reads `faults` once (synchronises) and raises AgnnError naming every kind that was counted."""
        words = self.faults.tolist()
        bad = [f"{FAULT_NAMES[k]} ({n})" for k, n in enumerate(words) if n]
        if bad:
            raise _lib.AgnnError("score graph input faults: " + "; ".join(bad))


def _i64(t: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
        raise _lib.AgnnError(f"{what}: 1-D int64 device tensor expected")
    return t if t.is_contiguous() else t.contiguous()


def _starts(score_start, n: int, dev, read_device: bool):
    """(host offsets or None, device int32 offsets).  score_start is host knowledge (as ScoreStore.score_start), [0, n] when absent;
    a device tensor is used where it lies and copied to the host only where the caller reads the device anyway."""
    if isinstance(score_start, torch.Tensor) and score_start.is_cuda:
        if score_start.dim() != 1 or score_start.numel() < 2:
            raise _lib.AgnnError("score_start needs at least two entries (one score)")
        start_dev = score_start.to(torch.int32).contiguous()
        return (start_dev.cpu().numpy().astype(np.int64) if read_device else None), start_dev
    if isinstance(score_start, torch.Tensor):
        score_start = score_start.numpy()
    s = np.asarray([0, n] if score_start is None else score_start, dtype=np.int64).reshape(-1)
    if s.size < 2:
        raise _lib.AgnnError("score_start needs at least two entries (one score)")
    return s, torch.from_numpy(np.clip(s, -1, 2 ** 31 - 1).astype(np.int32)).to(dev)


def build_score_graph(onset_div: torch.Tensor, duration_div: torch.Tensor, score_start=None, *, self_loops: bool = True,
                      add_beats: bool = False, add_measures: bool = False, beat_key: Optional[torch.Tensor] = None,
                      measure_key: Optional[torch.Tensor] = None, divs_per_beat: int = 4, beats_per_measure: int = 4,
                      reverse_note_edges: bool = False, reverse_metrical_edges: bool = False,
                      capacity: Optional[Dict[str, int]] = None) -> DeviceScoreGraph:
    """The score graph of one or many scores whose notes are concatenated: int64 device tensors `onset_div`, `duration_div`,
    and `score_start` (S + 1 offsets, host — or an int32 device tensor, which static-capacity mode never reads back; None = one
    score).  Inside a score the notes are in (onset, pitch) order (`sort_notes`); the builder never reorders them.  `beat_key` / `measure_key`: a per-note int64 key, non-decreasing inside a score, whose changes
    delimit the beats / measures (default onset // divs_per_beat and onset // (divs_per_beat * beats_per_measure)).

    capacity=None: tensors of exact size; costs one host read of the totals (eager only, never under capture) and runs check().
    capacity={"onset": int, "consecutive": .., "during": .., "rest": .., "beat": .., "measure": ..}: static shapes and no host read;
    slots past the real counts hold (-1, -1), `num_nodes` of beats / measures is the capacity, and check() is the caller's to call.
    Both modes allocate their outputs: call them outside a hipGraph capture (as `edge_plan`)."""
    onset_div, duration_div = _i64(onset_div, "onset_div"), _i64(duration_div, "duration_div")
    dev = _lib.require_gpu(onset_div, duration_div)
    n = int(onset_div.numel())
    if n < 1 or duration_div.numel() != n:
        raise _lib.AgnnError(f"onset_div and duration_div need the same length >= 1, got {n} and {duration_div.numel()}")
    exact = capacity is None
    starts, start_dev = _starts(score_start, n, dev, read_device=exact)
    n_scores = int(start_dev.numel() - 1)
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    types = [t for t, on in zip(GROUP_TYPES, (add_beats, add_measures)) if on]
    if not exact:
        missing = [k for k in (*NOTE_RELATIONS, *types) if k not in capacity]
        if missing:
            raise _lib.AgnnError(f"capacity lacks {missing}")
    totals = torch.zeros(6, dtype=torch.int64, device=dev)
    faults = torch.zeros(FAULT_WORDS, dtype=torch.int32, device=dev)
    note_score = torch.empty(n, dtype=torch.int64, device=dev)
    ws_bytes = max(int(lib.agnn_score_graph_workspace_bytes(n, n_scores)), int(lib.agnn_score_groups_workspace_bytes(n)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    g = _lib.ScoreGraphArgs()
    g.onset_div, g.duration_div, g.score_start = onset_div.data_ptr(), duration_div.data_ptr(), start_dev.data_ptr()
    g.n_notes, g.n_scores = n, n_scores
    g.flags = _lib.CONSTS["AGNN_SG_SELF_LOOPS"] if self_loops else 0
    g.rev_mask = 0b1110 if reverse_note_edges else 0
    g.totals, g.note_score, g.faults = totals.data_ptr(), note_score.data_ptr(), faults.data_ptr()

    # ---- metrical groups: measures first (the beats' parents); in exact mode a sizing pass whose faults are thrown away
    keys = {"beat": (beat_key, divs_per_beat), "measure": (measure_key, divs_per_beat * beats_per_measure)}
    rows = 3 if reverse_metrical_edges else 2
    note_edge = {t: torch.empty((rows, n), dtype=torch.int64, device=dev) for t in types}
    per_score = {t: torch.empty(n_scores, dtype=torch.int64, device=dev) for t in types}

    def groups(t, cap, out_faults, sized):
        key, div = keys[t]
        key, div = (onset_div, int(div)) if key is None else (_i64(key, f"{t}_key"), 1)
        if key.numel() != n:
            raise _lib.AgnnError(f"{t}_key needs one entry per note")
        a = _lib.ScoreGroupsArgs()
        a.key, a.div, a.score_start, a.n_notes, a.n_scores = key.data_ptr(), div, start_dev.data_ptr(), n, n_scores
        a.rev, a.cap = int(reverse_metrical_edges), cap
        a.note_edge, a.per_score = note_edge[t].data_ptr(), per_score[t].data_ptr()
        a.total = totals.data_ptr() + 8 * (4 + GROUP_TYPES.index(t))
        a.faults = out_faults.data_ptr()
        out = {}
        if sized:
            out["score"] = torch.empty(cap, dtype=torch.int64, device=dev)
            out["first"] = torch.empty(cap, dtype=torch.int64, device=dev)
            a.group_score, a.group_first = _lib.ptr(out["score"]) or None, _lib.ptr(out["first"]) or None
            if t == "beat" and "measure" in types:
                out["parent"] = torch.empty((rows, cap), dtype=torch.int64, device=dev)
                a.parent_of = note_edge["measure"][1].data_ptr()
                a.parent_edge = _lib.ptr(out["parent"]) or None
        _lib.check(lib.agnn_score_groups(a, ws.data_ptr(), ws_bytes, st), "agnn_score_groups")
        return out

    if exact:
        scratch = torch.zeros(FAULT_WORDS, dtype=torch.int32, device=dev)
        for t in types:
            groups(t, 0, scratch, sized=False)
        _lib.check(lib.agnn_score_graph_count(g, ws.data_ptr(), ws_bytes, st), "agnn_score_graph_count")
        counts = totals.tolist()                                     # the one host read of this mode
        caps = dict(zip((*NOTE_RELATIONS, *GROUP_TYPES), counts))
    else:
        caps = {k: int(capacity[k]) for k in (*NOTE_RELATIONS, *types)}
    bufs = []
    for r, rel in enumerate(NOTE_RELATIONS):
        buf = torch.empty((3 if (g.rev_mask >> r) & 1 else 2, caps[rel]), dtype=torch.int64, device=dev)
        bufs.append(buf)
        g.edges[r], g.cap[r] = (buf.data_ptr() if caps[rel] else None), caps[rel]
    call = lib.agnn_score_graph_fill if exact else lib.agnn_score_graph_build
    _lib.check(call(g, ws.data_ptr(), ws_bytes, st), call.__name__)
    grp = {t: groups(t, caps[t], faults, sized=True) for t in reversed(types)}       # measures before beats

    ei: Dict[EdgeType, torch.Tensor] = {("note", rel, "note"): buf[0:2] for rel, buf in zip(NOTE_RELATIONS, bufs)}
    if reverse_note_edges:
        for rel, buf in zip(NOTE_RELATIONS[1:], bufs[1:]):
            ei[("note", rel + "_rev", "note")] = buf[1:3]
    num_nodes = {"note": n}
    if starts is not None:              # per-score note counts, host knowledge the sequence branch would otherwise read back
        note_score.agnn_target_lengths = np.diff(starts).tolist()
    batch = {"note": note_score}
    for t in types:
        num_nodes[t] = caps[t]
        batch[t] = grp[t]["score"]
        ei[("note", "connects", t)] = note_edge[t][0:2]
        if reverse_metrical_edges:
            ei[(t, "rev_connects", "note")] = note_edge[t][1:3]
        if t == "measure" and "beat" in types:
            ei[("beat", "connects", "measure")] = grp["beat"]["parent"][0:2]
            if reverse_metrical_edges:
                ei[("measure", "rev_connects", "beat")] = grp["beat"]["parent"][1:3]
    out = DeviceScoreGraph(ei, num_nodes, batch, onset_div, duration_div, totals, faults,
                           {t: grp[t]["first"] for t in types}, per_score)
    if exact:
        out.check()
    return out


def sort_notes(onset_div: torch.Tensor, pitch: Optional[torch.Tensor] = None, score_start=None) -> torch.Tensor:
    """The permutation (int64) that puts the notes of every score in (onset, pitch) order, stable otherwise — the order the
    reference establishes before building (models/analysis.py:1534) and `build_score_graph` expects: `onset_div[perm]`."""
    onset_div = _i64(onset_div, "onset_div")
    n = int(onset_div.numel())
    perm = torch.arange(n, dtype=torch.int64, device=onset_div.device)
    if pitch is not None:
        perm = perm[torch.sort(pitch[perm], stable=True).indices]
    perm = perm[torch.sort(onset_div[perm], stable=True).indices]
    starts, _ = _starts(score_start, n, onset_div.device, read_device=True)
    if starts.size > 2:
        score = torch.from_numpy(np.repeat(np.arange(starts.size - 1), np.diff(starts))).to(onset_div.device)
        perm = perm[torch.sort(score[perm], stable=True).indices]
    return perm
