#!/usr/bin/env python3
"""Golden note descriptors, produced by RUNNING THE REFERENCE'S OWN FUNCTIONS on the CPU.  TEST INFRASTRUCTURE ONLY: runs where the
reference tree is available, never on the GPU machine; only the arrays it writes (tests/golden/note_features_*.npz, a few KB each)
are committed — no reference program text travels.

Executed from the reference files, cut out with `ast` (oracle.gen_golden_r2.load_reference_function):
  get_voice_separation_features, get_pc_one_hot, get_octave_one_hot   descriptors/utils/note_features.py (the ndarray branch)
  get_cad_features(None, note_array, include_pitch_spelling=False)    descriptors/utils/cadence_features.py
  chord_to_intervalVector                                             utils/chord_representations.py
in the namespace {"np": np, "Tuple": tuple, "List": list, "pt": a stub whose .performance.PerformedPart is an empty class}, plus
itertools.combinations for the last one.  The reference's bass / high voice test indexes with `"voice" == ...` (always False): its
means are NaN and numpy warns about empty slices; the warnings are silenced here, the behaviour is what the fixtures pin.

Every fixture holds the input fields, `score_start`, `x_voice` (float64 [N, 25], as the reference returns it) and `x_cadence`
(int8 [N, 31]; `voice` is the input field).  Notes are in (onset, pitch) order.  `is_note_onset` is stored only where a case sets it.
Usage: python tests/gen_golden_note_features.py"""
from __future__ import annotations

import os
import sys
import time
import types
import warnings
from itertools import combinations

import numpy as np
import numpy.lib.recfunctions  # noqa: F401  (the reference reaches it as np.lib.recfunctions)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.gen_golden_r2 import load_reference_function  # noqa: E402
from oracle.testing import GOLDEN_DIR  # noqa: E402
from analysisgnn_amd.synth import _note_times  # noqa: E402

REF = "/root/reference/analysisgnn"
REF_NOTE = REF + "/descriptors/utils/note_features.py"
REF_CAD = REF + "/descriptors/utils/cadence_features.py"
REF_CHORD = REF + "/utils/chord_representations.py"
DTYPE = [("onset_div", "<i8"), ("duration_div", "<i8"), ("pitch", "<i8"), ("voice", "<i8"), ("ts_beats", "<i8"),
         ("is_downbeat", "<i8"), ("onset_beat", "<f4"), ("duration_beat", "<f4"), ("is_note_onset", "?")]
INT_FIELDS = ("onset_div", "duration_div", "pitch", "voice", "ts_beats", "is_downbeat")


def reference_functions():
    pt = types.SimpleNamespace(performance=types.SimpleNamespace(PerformedPart=type("PerformedPart", (), {})))
    ns = {"np": np, "Tuple": tuple, "List": list, "pt": pt, "combinations": combinations}
    for path, name in ((REF_NOTE, "get_pc_one_hot"), (REF_NOTE, "get_octave_one_hot"), (REF_NOTE, "get_voice_separation_features"),
                       (REF_CHORD, "chord_to_intervalVector"), (REF_CAD, "get_cad_features")):
        load_reference_function(path, name, ns)
    return ns["get_voice_separation_features"], ns["get_cad_features"]


def note_array(on, du, pitch, voice, *, beat=lambda on: on / 4 - 1, per_beat=4.0, ts=4, note_onset=None):
    """A structured note array in (onset, pitch) order; onset_beat / duration_beat are float32 functions of the divs."""
    order = np.lexsort((pitch, on))
    on, du, pitch, voice = (np.asarray(a, dtype=np.int64)[order] for a in (on, du, pitch, voice))
    a = np.zeros(len(on), dtype=DTYPE)
    a["onset_div"], a["duration_div"], a["pitch"], a["voice"], a["ts_beats"] = on, du, pitch, voice, ts
    a["onset_beat"] = np.asarray(beat(on.astype(np.float64)), dtype=np.float32)
    a["duration_beat"] = (du / per_beat).astype(np.float32)
    a["is_downbeat"] = np.remainder(a["onset_beat"].astype(np.float64), ts) == 0
    a["is_note_onset"] = True if note_onset is None else np.asarray(note_onset)[order]
    return a


def seeded(seed, n, voices=(1, 5), grace=False, **kw):
    on, du = _note_times(seed, n)
    if grace:
        du[::7] = 0
    rng = np.random.default_rng(1000 + seed)
    return note_array(on, du, rng.integers(36, 85, n), rng.integers(voices[0], voices[1], n), **kw)


def crafted():
    """Case (g): 70 notes on one onset with pitches 0..8 and 112..119 among them, a voice (9) on the first and the last note only,
    triads, a dominant seventh, a sus4, a bare fourth, and a bass line (voice 1) that moves by +-1, +-2, +-5, +-7, +-12."""
    notes = []                                                    # (onset, duration, pitch, voice)
    chord = list(range(0, 9)) + list(range(112, 120)) + [9 + 2 * k for k in range(53)]
    for k, p in enumerate(chord):
        notes.append((0, 1 + k % 4, p, 9 if p == 0 else 1 + k % 4))
    bass = [48, 49, 48, 50, 48, 53, 48, 55, 48, 60, 48]
    for k, p in enumerate(bass):
        notes.append((4 + 4 * k, 4, p, 1))
    upper = {4: (64, 67), 12: (55,), 20: (65, 67), 32: (59, 62, 65), 36: (52, 55)}
    for on, ps in upper.items():
        for v, p in enumerate(ps):
            notes.append((on, 4, p, 2 + v))
    notes += [(48, 8, 60, 2), (50, 2, 72, 3), (52, 2, 47, 1), (52, 2, 71, 4), (56, 4, 84, 9)]
    on, du, pitch, voice = (np.asarray(c) for c in zip(*notes))
    a = note_array(on, du, pitch, voice)
    assert len(a) == 96 and int((a["onset_div"] == 0).sum()) == 70
    assert a["voice"][0] == 9 and a["voice"][-1] == 9 and int((a["voice"] == 9).sum()) == 2
    return a


def cases():
    out = {}
    out["a_n1"] = [seeded(3, 1)]
    out["b_n2"] = [seeded(4, 2)]
    c = seeded(5, 33, grace=True, ts=3, note_onset=np.arange(33) % 5 != 0)
    out["c_n33"] = [c]
    out["d_n97"] = [seeded(1, 97, beat=lambda on: on / 3, per_beat=3.0)]
    e = seeded(6, 130, beat=lambda on: on / 16, per_beat=16.0)
    ob = e["onset_beat"]
    assert max(int(((ob < x) & (ob > x - np.float32(8))).sum()) for x in ob) > 64, "case (e): no 8-beat window with more than 64 notes"
    out["e_n130"] = [e]
    out["f_n64_n66"] = [seeded(2, 64, voices=(1, 4)), seeded(7, 66, voices=(2, 7))]
    out["g_n96"] = [crafted()]
    out["h_n500"] = [seeded(0, 500)]
    return out


def main():
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    voice_fn, cad_fn = reference_functions()
    columns = []
    for name, scores in cases().items():
        voice, cadence, seconds = [], [], 0.0
        for a in scores:                                          # every score through the reference on its own
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t0 = time.perf_counter()
                v, v_names = voice_fn(a)
                c, c_names = cad_fn(None, a, include_pitch_spelling=False)
                seconds += time.perf_counter() - t0
            assert v.shape == (len(a), 25) and c.shape == (len(a), 31), (v.shape, c.shape)
            voice.append(np.asarray(v, dtype=np.float64))
            cadence.append(np.asarray(c).astype(np.int8))
        notes = np.concatenate(scores)
        fix = {f: notes[f] for f in (*INT_FIELDS, "onset_beat", "duration_beat")}
        if not notes["is_note_onset"].all():
            fix["is_note_onset"] = notes["is_note_onset"]
        fix["score_start"] = np.concatenate([[0], np.cumsum([len(a) for a in scores])]).astype(np.int32)
        fix["x_voice"], fix["x_cadence"] = np.concatenate(voice), np.concatenate(cadence)
        assert set(np.unique(fix["x_cadence"])) <= {0, 1} and set(np.unique(fix["x_voice"][:, 2:])) <= {0.0, 1.0}
        columns.append(np.concatenate([fix["x_voice"], fix["x_cadence"]], axis=1))
        path = os.path.join(GOLDEN_DIR, f"note_features_{name}.npz")
        np.savez_compressed(path, **fix)
        print(f"{os.path.basename(path)}: {len(notes)} notes, {os.path.getsize(path)} bytes, "
              f"the reference's two functions took {seconds * 1e3:.1f} ms on this CPU")
    names = v_names + c_names
    allc = np.concatenate(columns)
    flat = [names[k] for k in range(56) if np.unique(allc[:, k]).size < 2]
    assert not flat, f"columns that take one value over the whole set: {flat}"
    print("columns:", ", ".join(names))


if __name__ == "__main__":
    main()
