#!/usr/bin/env python3
"""Golden score graphs, produced by RUNNING THE REFERENCE'S OWN BUILDER on the CPU.  TEST INFRASTRUCTURE ONLY: runs where the
reference tree is available, never on the GPU machine; only the arrays it writes (tests/golden/score_graph_*.npz, int32, a few KB
each) are committed — no reference program text travels.

Executed from the reference file, cut out with `ast` (oracle.gen_golden_r2.load_reference_function): the function
`hetero_graph_from_note_array` (utils/hgraph.py:214-300) in the namespace {"np": np}, on a structured note array with the fields
`onset_div` and `duration_div`, with `rest_array=None, pot_edge_dist=0`.

Note times come from synth._note_times.  Every note that ends after the last onset is given the one common final end: when a
non-largest end time has no later onset, the reference's `tmp.min()` is inf and it links the source to EVERY note (hgraph.py:279-280),
which neither synth.make_score_graph nor the device builder reproduces.  The generator asserts that no such end time is left, so
the reference alone is the expected output and nothing is filtered.
Usage: python tests/gen_golden_score_graph.py"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.gen_golden_r2 import load_reference_function  # noqa: E402
from oracle.testing import GOLDEN_DIR  # noqa: E402
from analysisgnn_amd.synth import NOTE_RELATIONS, _note_times  # noqa: E402

REF_HGRAPH = "/root/reference/analysisgnn/utils/hgraph.py"
# (seed, n_notes, grace notes: duration[::7] = 0)
CASES = [(3, 1, False), (4, 2, False), (2, 64, True), (5, 33, True), (1, 97, False), (6, 130, False), (0, 500, False)]
# (onset without self loops, consecutive, during, rest) edge counts, asserted
COUNTS = {(0, 500): (880, 604, 793, 528), (1, 97): (130, 67, 95, 111), (2, 64): (98, 84, 47, 45), (6, 130): (242, 160, 264, 130)}


def note_times(seed: int, n: int, grace: bool):
    on, du = _note_times(seed, n)
    end = on + du
    tail = end > on.max()
    du = np.where(tail, end.max() - on, du)
    if grace:
        du[::7] = 0
    end = on + du
    open_ends = [int(e) for e in np.unique(end)[:-1] if e not in on and not (on > e).any()]
    assert not open_ends, f"seed {seed}, {n} notes: non-largest end times {open_ends} have no later onset"
    return on, du


def main():
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    build = load_reference_function(REF_HGRAPH, "hetero_graph_from_note_array", {"np": np})
    for seed, n, grace in CASES:
        on, du = note_times(seed, n, grace)
        notes = np.zeros(n, dtype=[("onset_div", "<i8"), ("duration_div", "<i8")])
        notes["onset_div"], notes["duration_div"] = on, du
        _, edges = build(notes, rest_array=None, pot_edge_dist=0)
        edges = np.asarray(edges, dtype=np.int64).reshape(3, -1)
        out = {"onset_div": on.astype(np.int32), "duration_div": du.astype(np.int32)}
        for r, rel in enumerate(NOTE_RELATIONS):
            out[rel] = edges[:2, edges[2] == r].astype(np.int32)
        counts = tuple(int(out[rel].shape[1]) for rel in NOTE_RELATIONS)
        if (seed, n) in COUNTS:
            assert counts == COUNTS[(seed, n)], f"seed {seed}, {n} notes: {counts} edges, {COUNTS[(seed, n)]} expected"
        out["counts"] = np.asarray(counts, dtype=np.int32)
        path = os.path.join(GOLDEN_DIR, f"score_graph_s{seed}_n{n}.npz")
        np.savez_compressed(path, **out)
        print(f"{os.path.basename(path)}: {counts} edges, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
