"""tests/note_features_ref.py (the numpy restatement of the two note feature sets) pinned against the reference's own functions
(tests/golden/note_features_*.npz, written by tests/gen_golden_note_features.py), no GPU: the 54 boolean / one-hot columns exactly,
the two float columns of the voice set within 1e-12 as float64, and the many-score call equal to the per-score results stacked."""
import glob
import os

import numpy as np
import pytest

import note_features_ref as R

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "note_features_*.npz")))
NAMES = ["a_n1", "b_n2", "c_n33", "d_n97", "e_n130", "f_n64_n66", "g_n96", "h_n500"]


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def test_all_fixtures_present():
    assert [os.path.basename(p) for p in GOLDEN] == [f"note_features_{n}.npz" for n in NAMES]


def test_column_names():
    assert len(R.VOICE_FEATURES) == 25 and len(R.CADENCE_FEATURES) == 56 and R.CADENCE_FEATURES[:25] == R.VOICE_FEATURES
    assert len(set(R.CADENCE_FEATURES)) == 56


@pytest.mark.parametrize("path", GOLDEN, ids=NAMES[:len(GOLDEN)])
def test_ref_equals_the_reference(path):
    z = load(path)
    assert z["x_voice"].dtype == np.float64 and z["x_cadence"].dtype == np.int8
    v = R.note_features(z, "voice")
    assert v.shape == z["x_voice"].shape and np.array_equal(v[:, 2:], z["x_voice"][:, 2:])
    assert np.abs(v[:, :2] - z["x_voice"][:, :2]).max() <= 1e-12
    c = R.note_features(z, "cadence", z["score_start"])
    assert c.shape == (v.shape[0], 56) and np.array_equal(c[:, :25], v)
    bad = np.nonzero(c[:, 25:] != z["x_cadence"])
    assert bad[0].size == 0, [(int(i), R.CADENCE_FEATURES[25 + k]) for i, k in zip(*bad)][:10]


def test_every_column_takes_two_values_over_the_fixtures():
    rows = []
    for p in GOLDEN:
        z = load(p)
        rows.append(np.concatenate([z["x_voice"], z["x_cadence"]], axis=1))
    rows = np.concatenate(rows)
    assert [R.CADENCE_FEATURES[k] for k in range(56) if np.unique(rows[:, k]).size < 2] == []


def test_many_scores_equal_the_scores_stacked():
    z = load([p for p in GOLDEN if "f_n64_n66" in p][0])
    s = z["score_start"]
    assert s.tolist() == [0, 64, 130]
    whole = R.note_features(z, "cadence", s)
    fields = [k for k in R.FIELDS if k in z]
    parts = [R.note_features({k: z[k][a:b] for k in fields}, "cadence") for a, b in zip(s[:-1], s[1:])]
    assert np.array_equal(whole, np.concatenate(parts))
    alone = R.note_features({k: z[k] for k in fields}, "cadence")           # one score of 130 notes: the boundary matters
    assert not np.array_equal(alone, whole)


def test_unknown_sets_and_bad_pitch_raise():
    z = load(GOLDEN[0])
    with pytest.raises(ValueError, match="voice.*cadence"):
        R.note_features(z, "chord")
    z["pitch"] = z["pitch"] + 120
    with pytest.raises(IndexError):
        R.note_features(z, "voice")
