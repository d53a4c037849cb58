"""Note descriptors on the device (csrc/notefeat.hip, analysisgnn_amd/descriptors.py) against the reference's own output
(tests/golden/note_features_*.npz) and, where no fixture exists, against tests/note_features_ref.py.  The 54 boolean / one-hot
columns are exactly 0.0 or 1.0 and equal; the two float columns are within 1e-6 absolute of the float64 values: they lie in [0, 1],
the inputs are exact float32, and a division, a tanh and one rounding to fp32 stay below 5e-7."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import note_features_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "note_features_*.npz")))
IDS = [os.path.basename(p)[14:-4] for p in GOLDEN]
SETS = ("voice", "cadence")
WIDTH = {"voice": 25, "cadence": 56}
FLOAT_TOL = 1e-6
PITCH, TS, VOICE, ORDER, SCORES = range(5)


def load(path_or_name):
    path = path_or_name if os.path.sep in path_or_name else [p for p in GOLDEN if path_or_name in p][0]
    z = np.load(path)
    return {k: z[k] for k in z.files}


def to_device(z):
    return {k: torch.from_numpy(np.ascontiguousarray(z[k])).to(DEV) for k in R.FIELDS if z.get(k) is not None}


def expected(z, feature_type):
    if feature_type == "voice":
        return z["x_voice"]
    return np.concatenate([z["x_voice"], z["x_cadence"].astype(np.float64)], axis=1)


def same(got, exp, what=""):
    """The exactness rules of this file; `got` a device tensor, `exp` float64."""
    g = got.detach().cpu().numpy()
    assert g.dtype == np.float32 and g.shape == exp.shape, (what, g.dtype, g.shape, exp.shape)
    bad = np.nonzero(g[:, 2:] != exp[:, 2:])
    assert bad[0].size == 0, (what, [(int(i), R.CADENCE_FEATURES[2 + k]) for i, k in zip(*bad)][:10])
    assert np.isin(g[:, 2:], (0.0, 1.0)).all(), what
    err = np.abs(g[:, :2].astype(np.float64) - exp[:, :2]).max()
    print(f"{what}: float columns max |err| = {err:.3e}")
    assert err <= FLOAT_TOL, (what, err)


def synth_notes(seed, n):
    """A note array on synth's note times with an anacrusis, in (onset, pitch) order."""
    from analysisgnn_amd.synth import _note_times
    on, du = _note_times(seed, n)
    rng = np.random.default_rng(2000 + seed)
    pitch, voice = rng.integers(24, 100, n), rng.integers(1, 6, n)
    order = np.lexsort((pitch, on))
    on, du, pitch, voice = on[order], du[order], pitch[order], voice[order]
    ob = (on / 4 - 1).astype(np.float32)
    ts = np.full(n, 3 if seed % 2 else 4, dtype=np.int64)
    return dict(onset_div=on, duration_div=du, pitch=pitch, voice=voice, ts_beats=ts,
                is_downbeat=(np.remainder(ob.astype(np.float64), ts) == 0).astype(np.int64), onset_beat=ob,
                duration_beat=(du / 4).astype(np.float32), is_note_onset=rng.integers(0, 4, n) != 0)


@functools.lru_cache(maxsize=None)
def big_case(name):
    if name == "one score of 4096":
        z, starts = synth_notes(11, 4096), np.asarray([0, 4096])
    else:
        scores = [synth_notes(20 + s, 500) for s in range(32)]
        z, starts = {k: np.concatenate([s[k] for s in scores]) for k in scores[0]}, np.arange(33) * 500
    return z, starts, R.note_features(z, "cadence", starts)


def test_fixtures_present():
    assert len(GOLDEN) == 8


@pytest.mark.parametrize("feature_type", SETS)
@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_equals_the_reference(path, feature_type):
    from analysisgnn_amd.descriptors import note_features
    z = load(path)
    x = note_features(to_device(z), feature_type, z["score_start"])
    assert tuple(x.shape) == (len(z["pitch"]), WIDTH[feature_type])
    same(x, expected(z, feature_type), f"{os.path.basename(path)} {feature_type}")


@pytest.mark.parametrize("feature_type", SETS)
def test_out_as_a_column_block_leaves_the_rest_untouched(feature_type):
    from analysisgnn_amd.descriptors import note_features
    z = load("h_n500")
    w, n = WIDTH[feature_type], 500
    for offset in (4, 3):                                   # 16-byte aligned rows, and rows no vector store may touch
        big = torch.full((n, 64), -7.5, dtype=torch.float32, device=DEV)
        out = big[:, offset:offset + w]
        assert out.stride(0) == 64 and (out.data_ptr() % 16 == 0) == (offset == 4)
        x = note_features(to_device(z), feature_type, out=out)
        assert x.data_ptr() == out.data_ptr()
        same(big[:, offset:offset + w], expected(z, feature_type), f"block at {offset} {feature_type}")
        assert bool((big[:, :offset] == -7.5).all()) and bool((big[:, offset + w:] == -7.5).all())


def test_four_scores_repeat_the_two_and_runs_are_bitwise_equal():
    from analysisgnn_amd.descriptors import note_features
    z = load("f_n64_n66")
    two = note_features(to_device(z), "cadence", z["score_start"])
    f4 = {k: torch.cat([v, v]) for k, v in to_device(z).items()}
    starts = [0, 64, 130, 194, 260]
    a = note_features(f4, "cadence", starts)
    b = note_features(f4, "cadence", torch.tensor(starts, dtype=torch.int32, device=DEV))
    assert torch.equal(a, torch.cat([two, two]))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    same(a, np.concatenate([expected(z, "cadence")] * 2), "four scores")


@pytest.mark.parametrize("name", ["one score of 4096", "32 scores of 500"])
def test_equals_the_numpy_rules_at_sizes_without_a_fixture(name):
    from analysisgnn_amd.descriptors import note_features
    z, starts, exp = big_case(name)
    f = to_device(z)
    same(note_features(f, "cadence", starts), exp, f"{name} cadence")
    same(note_features(f, "voice", starts), exp[:, :25], f"{name} voice")
    del f["is_note_onset"]                                  # absent: all ones, nothing else moves
    exp1 = exp.copy()
    exp1[:, 25 + 15] = 1
    same(note_features(f, "cadence", starts), exp1, f"{name} cadence without is_note_onset")


def _without(z, drop, starts):
    keep = np.setdiff1d(np.arange(len(z["pitch"])), drop)
    kept = {k: np.asarray(z[k])[keep] for k in R.FIELDS if z.get(k) is not None}
    new = np.asarray([int((keep < s).sum()) for s in starts])
    return keep, kept, new


BAD = {
    "pitch": (PITCH, "pitch", {5: 120, 100: -1, 129: 1 << 40}, "pitch outside"),
    "ts_beats": (TS, "ts_beats", {0: 0, 64: -3}, "ts_beats <= 0"),
    "voice": (VOICE, "voice", {63: 1 << 15, 70: -1, 71: -(1 << 40)}, "voice outside"),
}


# the voice set does not read the voice field: that pair is no case
@pytest.mark.parametrize("kind,feature_type", [(k, s) for k in BAD for s in SETS if (k, s) != ("voice", "voice")])
def test_bad_values_are_counted_zeroed_and_left_out(kind, feature_type):
    from analysisgnn_amd import _lib
    from analysisgnn_amd.descriptors import note_features
    word, field, values, message = BAD[kind]
    z = load("f_n64_n66")
    starts = z["score_start"]
    z[field] = z[field].copy()
    for i, v in values.items():
        z[field][i] = v
    drop = np.asarray(sorted(values))
    f = to_device(z)
    with pytest.raises(_lib.AgnnError, match=message):
        note_features(f, feature_type, starts)
    x = note_features(f, feature_type, starts, check=False)
    faults = x.agnn_faults.tolist()
    assert faults == [len(drop) if k == word else 0 for k in range(5)]
    assert bool((x[torch.from_numpy(drop).to(DEV)] == 0).all())
    keep, kept, new_starts = _without(z, drop, starts)
    same(x[torch.from_numpy(keep).to(DEV)], R.note_features(kept, feature_type, new_starts), f"{kind} {feature_type}")
    clean = load("f_n64_n66")
    same(note_features(to_device(clean), feature_type, starts), expected(clean, feature_type), "the call after a raise")
    _lib.check_device_status(DEV)


@pytest.mark.parametrize("feature_type", SETS)
def test_a_decreasing_onset_is_counted_zeroed_and_left_out(feature_type):
    from analysisgnn_amd import _lib
    from analysisgnn_amd.descriptors import note_features
    z = load("f_n64_n66")
    starts = z["score_start"]
    on = z["onset_div"]
    k = 64 + int(np.nonzero(np.diff(on[64:]) > 0)[0][10]) + 1          # first note of an onset run inside the second score
    assert on[k] > on[k - 1] and k + 1 < 130
    for name in ("onset_div", "onset_beat"):
        z[name] = z[name].copy()
        z[name][k] = z[name][k - 1] - 2
    f = to_device(z)
    with pytest.raises(_lib.AgnnError, match="decreases"):
        note_features(f, feature_type, starts)
    x = note_features(f, feature_type, starts, check=False)
    assert x.agnn_faults.tolist() == [int(k == ORDER) for k in range(5)]
    assert bool((x[k] == 0).all())
    keep, kept, new_starts = _without(z, np.asarray([k]), starts)
    same(x[torch.from_numpy(keep).to(DEV)], R.note_features(kept, feature_type, new_starts), f"order {feature_type}")
    _lib.check_device_status(DEV)


@pytest.mark.parametrize("feature_type", SETS)
def test_a_score_start_that_does_not_tile_zeroes_everything(feature_type):
    from analysisgnn_amd import _lib
    from analysisgnn_amd.descriptors import note_features
    z = load("f_n64_n66")
    f = to_device(z)
    for starts in ([0, 64, 129], [0, 70, 64, 130], [1, 64, 130], [0, 64, 500]):
        with pytest.raises(_lib.AgnnError, match="tile"):
            note_features(f, feature_type, starts)
        big = torch.full((130 + 8, 56), -7.5, dtype=torch.float32, device=DEV)
        x = note_features(f, feature_type, starts, out=big[4:134, :WIDTH[feature_type]], check=False)
        assert x.agnn_faults.tolist() == [int(k == SCORES) for k in range(5)]
        assert bool((x == 0).all()) and bool((big[:4] == -7.5).all()) and bool((big[134:] == -7.5).all())
    _lib.check_device_status(DEV)


@pytest.mark.parametrize("feature_type", SETS)
def test_capture_and_replay_on_fresh_values(feature_type):
    from analysisgnn_amd import _lib
    from analysisgnn_amd.descriptors import note_features
    first, second = load("e_n130"), synth_notes(9, 130)
    names = [k for k in R.FIELDS if first.get(k) is not None]
    f = to_device(first)
    starts = torch.tensor([0, 130], dtype=torch.int32, device=DEV)
    out = torch.empty((130, 56), dtype=torch.float32, device=DEV)[:, :WIDTH[feature_type]]
    eager = note_features(f, feature_type, starts, out=out, check=False).clone()
    same(eager, expected(first, feature_type), "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x = note_features(f, feature_type, starts, out=out, check=False)
        with pytest.raises(_lib.AgnnError, match="capture"):
            note_features(f, feature_type, starts, out=out, check=True)
    faults = x.agnn_faults
    out.fill_(-1)
    graph.replay()
    assert torch.equal(out, eager) and faults.tolist() == [0] * 5
    for k in names:                                          # fresh values in the same tensors
        f[k].copy_(torch.from_numpy(np.ascontiguousarray(second[k])).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, note_features(f, feature_type, starts, check=False))
    same(out, R.note_features({k: second[k] for k in names}, feature_type), "replay")


@pytest.mark.parametrize("feature_type", SETS)
def test_predict_from_notes_computes_the_note_rows(feature_type):
    from analysisgnn_amd import synth
    from analysisgnn_amd.descriptors import note_features
    from analysisgnn_amd.models import TorchAnalysisGNN
    from analysisgnn_amd.postprocess import predict_from_notes
    tasks = {"quality": 15, "inversion": 4, "cadence": 4}
    g = synth.make_batch(2, 60, first_seed=7)
    starts = [0, 60, 120]
    z = {k: np.concatenate([synth_notes(40 + s, 60)[k] for s in range(2)]) for k in R.FIELDS}
    z["onset_div"], z["duration_div"] = g.onset_div, g.duration_div
    z["onset_beat"], z["duration_beat"] = (g.onset_div / 4).astype(np.float32), (g.duration_div / 4).astype(np.float32)
    f = to_device(z)
    torch.manual_seed(0)
    m = TorchAnalysisGNN(g.metadata(), WIDTH[feature_type], 32, 32, tasks, 2, dropout=0.3, use_jk=False, logit_fusion=True).to(DEV)
    I = synth.torch_inputs(g, 25, DEV, 0)
    on, du = f["onset_div"], f["duration_div"]
    x = note_features(f, feature_type, starts)
    exp = predict_from_notes(m, I["pitch_spelling"], I["key_signature"], x, on, du, score_start=starts)
    got = predict_from_notes(m, I["pitch_spelling"], I["key_signature"], None, on, du, score_start=starts, note_fields=f,
                             feature_type=feature_type)
    assert list(got) == list(exp) == list(tasks)
    for k in exp:
        assert torch.equal(got[k], exp[k]) and bool(torch.isfinite(got[k]).all()), k
    with pytest.raises(ValueError, match="'voice'.*'cadence'"):
        predict_from_notes(m, I["pitch_spelling"], I["key_signature"], None, on, du, note_fields=f, feature_type="chord")
