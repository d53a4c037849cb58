"""Vectorised numpy restatement of the two note feature sets ("Note descriptors"; the reference's
get_voice_separation_features and get_cad_features(include_pitch_spelling=False)), score by score with dense N x N masks.  Pinned
against the reference's own output by tests/test_note_features_ref.py; the GPU tests use it for shapes that have no fixture.
numpy only: it travels with the tests."""
from __future__ import annotations

import numpy as np

VOICE_FEATURES = ["bar_exp_duration", "onset_bar_norm", "is_down_beat"] + [f"pc_{i:02d}" for i in range(12)] + \
                 [f"octave_{i:02d}" for i in range(10)]
CADENCE_ONLY = ["perfect_triad", "perfect_major_triad", "is_sus4", "in_perfect_triad_or_sus4", "highest_is_3", "highest_is_1",
                "bass_compatible_with_I", "bass_compatible_with_I_scale", "one_comes_from_7", "one_comes_from_1", "one_comes_from_2",
                "three_comes_from_4", "five_comes_from_5", "strong_beat", "sustained_note", "is_note_onset", "rest_highest",
                "rest_lowest", "rest_middle", "voice_ends", "is_downbeat", "v7", "v7-3", "has_7", "has_9", "bass_voice",
                "bass_moves_chromatic", "bass_moves_octave", "bass_compatible_v-i", "bass_compatible_i-v", "bass_moves_2M"]
CADENCE_FEATURES = VOICE_FEATURES + CADENCE_ONLY
FIELDS = ("onset_div", "duration_div", "pitch", "voice", "ts_beats", "is_downbeat", "onset_beat", "duration_beat", "is_note_onset")


def _bits(*pcs):
    return sum(1 << p for p in pcs)


def _iv(*counts):                      # an interval vector as six 4-bit counts
    return sum(c << (4 * k) for k, c in enumerate(counts))


def _masks(member, pc):
    """member [n, m] bool, pc [m] in 0..11 -> per row the 12-bit mask of the members' pitch classes."""
    onehot = np.zeros((pc.size, 12), dtype=np.float32)
    onehot[np.arange(pc.size), pc] = 1
    present = (member.astype(np.float32) @ onehot) > 0
    return (present * (1 << np.arange(12))).sum(1).astype(np.int64)


def _rot12(m, k):                      # bit b -> bit (b + k) % 12, k an array in 0..11
    return ((m << k) | (m >> (12 - k))) & 0xFFF


def _bit(m, b):
    return ((m >> b) & 1).astype(bool)


def voice_features(f) -> np.ndarray:
    ts = np.asarray(f["ts_beats"], dtype=np.int64)
    ob, db = np.asarray(f["onset_beat"], dtype=np.float32), np.asarray(f["duration_beat"], dtype=np.float32)
    pitch = np.asarray(f["pitch"], dtype=np.int64)
    n = pitch.size
    out = np.zeros((n, 25), dtype=np.float64)
    out[:, 0] = 1 - np.tanh(db / ts)
    out[:, 1] = np.remainder(ob, ts) / ts
    out[:, 2] = np.remainder(ob, 1) == 0
    out[np.arange(n), 3 + pitch % 12] = 1
    out[np.arange(n), 15 + pitch // 12] = 1
    return out


def _cadence_one_score(f) -> np.ndarray:
    on, du = np.asarray(f["onset_div"], dtype=np.int64), np.asarray(f["duration_div"], dtype=np.int64)
    pitch, voice = np.asarray(f["pitch"], dtype=np.int64), np.asarray(f["voice"], dtype=np.int64)
    ts, ob = np.asarray(f["ts_beats"], dtype=np.int64), np.asarray(f["onset_beat"], dtype=np.float32)
    n = on.size
    pc = pitch % 12
    same = on[None, :] == on[:, None]
    thru = (on[None, :] < on[:, None]) & ((on + du)[None, :] > on[:, None])
    member = same | thru
    mask = _masks(member, pc)
    lo = np.where(member, pitch[None, :], 1 << 20).min(1)
    hi = np.where(member, pitch[None, :], -1).max(1)
    cnt = member.sum(1)
    code = np.zeros(n, dtype=np.int64)
    for k in range(1, 7):
        both = mask & _rot12(mask, k)
        c = sum((both >> b) & 1 for b in range(12)) >> (1 if k == 6 else 0)
        code |= c << (4 * (k - 1))
    ctz = np.argmax(np.stack([(mask >> b) & 1 for b in range(12)], axis=1), axis=1)
    rec = mask >> ctz
    triad = np.isin(code, [_iv(0, 0, 1, 1, 1, 0), _iv(0, 0, 1), _iv(0, 0, 0, 1), _iv(0, 0, 0, 0, 1)])
    major = np.isin(rec, [_bits(0, 4, 7), _bits(0, 5, 9), _bits(0, 3, 8), _bits(0, 4), _bits(0, 8), _bits(0, 7), _bits(0, 5)])
    sus4 = (code == _iv(0, 1, 0, 0, 2, 0)) | (rec == _bits(0, 5))
    v7 = np.isin(code, [_iv(0, 1, 2, 1, 1, 1), _iv(0, 1, 0, 1, 0, 1), _iv(0, 1)])
    span, own = (hi - lo) % 12, (pitch - lo) % 12
    before = ob[None, :] < ob[:, None]
    prev4 = _masks(before & (ob[None, :] > (ob - np.float32(4))[:, None]), pc)
    prev8 = _masks(before & (ob[None, :] > (ob - np.float32(8))[:, None]), pc)
    minor = (pitch + 3 < 12) & _bit(mask, np.minimum(pitch + 3, 11))
    scale = np.where(minor, _bits(2, 3, 5, 7, 8, 11), _bits(2, 4, 5, 7, 9, 11))
    compat = _bit(prev4, (pc + 5) % 12) & _bit(prev4, (pc + 11) % 12)
    compat_scale = (prev8 != 0) & ((_rot12(scale, pc) & ~prev8) == 0)
    same_voice = voice[None, :] == voice[:, None]
    earlier = same_voice & (on[None, :] < on[:, None])
    has_pv = earlier.any(1)
    last = np.where(earlier, on[None, :], np.iinfo(np.int64).min).max(1)
    pv = earlier & (on[None, :] == last[:, None])
    pvr = _rot12(_masks(pv, pc), (12 - lo % 12) % 12)
    diff = pitch[None, :] - pitch[:, None]
    moves = {d: (pv & (diff == d)).any(1) for d in (-12, -7, -5, -2, -1, 1, 2, 5, 7, 12)}
    later = same_voice & (on[None, :] > on[:, None])
    has_nv = later.any(1)
    nv = np.where(later, on[None, :], np.iinfo(np.int64).max).min(1)
    rest = has_nv & (nv > on + du)
    bass, high = voice == voice.min(), voice == voice.max()
    come = has_pv & (cnt > 1) & (own == 0)
    ob64 = ob.astype(np.float64)
    strong = ((ts == 4) & (np.fmod(ob64, 2) == 0)) | (np.fmod(ob64, ts) == 0)
    note_onset = np.ones(n, dtype=bool) if f.get("is_note_onset") is None else np.asarray(f["is_note_onset"]).astype(bool)
    cols = [triad, triad & major, sus4, triad | sus4, (span == 3) | (span == 4), (span == 0) & (hi != lo), compat, compat_scale,
            come & _bit(pvr, 11), come & _bit(pvr, 0), come & _bit(pvr, 2), has_pv & _bit(pvr, 5) & ((own == 3) | (own == 4)),
            has_pv & _bit(pvr, 7) & (own == 7), strong, thru.any(1), note_onset, rest & high, rest & bass, rest & ~high & ~bass,
            ~has_nv, np.asarray(f["is_downbeat"]) != 0, v7, v7 & _bit(rec, 4), _bit(rec, 10), _bit(rec, 1) | _bit(rec, 2), bass,
            bass & (moves[1] | moves[-1]), bass & (moves[12] | moves[-12]), bass & (moves[7] | moves[-5]),
            bass & (moves[-7] | moves[5]), bass & (moves[2] | moves[-2])]
    return np.stack(cols, axis=1).astype(np.float64)


def note_features(fields, feature_type: str = "voice", score_start=None) -> np.ndarray:
    """float64 [N, 25 | 56] of a mapping of numpy arrays by the reference's field names; `score_start`: S + 1 offsets."""
    f = {k: np.asarray(fields[k]) for k in FIELDS if fields.get(k) is not None}
    n = f["pitch"].size
    if np.any((f["pitch"] < 0) | (f["pitch"] >= 120)):
        raise IndexError("pitch outside [0, 120)")            # as the reference's octave one-hot
    v = voice_features(f)
    if feature_type == "voice":
        return v
    if feature_type != "cadence":
        raise ValueError(f"feature_type {feature_type!r}: 'voice' and 'cadence' are supported")
    starts = np.asarray([0, n] if score_start is None else score_start, dtype=np.int64)
    parts = [_cadence_one_score({k: a[lo:hi] for k, a in f.items()}) for lo, hi in zip(starts[:-1], starts[1:])]
    return np.concatenate([v, np.concatenate(parts)], axis=1)
