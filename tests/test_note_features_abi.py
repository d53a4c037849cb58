"""The note descriptor entry points (csrc/notefeat.hip) are bound from include/agnn.h and reject bad arguments with a message BEFORE
any kernel is launched (safe on a CPU-only host: the pointers below are never dereferenced): AGNN_EINVAL (-22) for NULL pointers,
n_notes < 1, n_scores < 1, an ld_x below the set's width and an unknown feature_set, AGNN_ENOMEM (-12) for a workspace that is too
small."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # an aligned non-null address, never read
EINVAL, ENOMEM = -22, -12
VOICE, CADENCE = 0, 1
INPUTS = ("onset_div", "duration_div", "pitch", "ts_beats", "onset_beat", "duration_beat", "score_start")


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _args(**kw):
    from analysisgnn_amd import _lib
    d = dict(onset_div=P, duration_div=P, pitch=P, voice=P, ts_beats=P, is_downbeat=P, onset_beat=P, duration_beat=P,
             is_note_onset=None, score_start=P, n_notes=100, n_scores=2, feature_set=CADENCE, x=P, ld_x=56, faults=P)
    d.update(kw)
    a = _lib.NoteFeaturesArgs()
    for k, v in d.items():
        setattr(a, k, v)
    return a


def test_names_are_bound_from_the_header():
    from analysisgnn_amd import _lib, descriptors
    for name in ("agnn_note_features_f32", "agnn_note_features_workspace_bytes"):
        assert name in _lib.SIGNATURES, name
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    assert [f[0] for f in _lib.NoteFeaturesArgs._fields_] == [
        "onset_div", "duration_div", "pitch", "voice", "ts_beats", "is_downbeat", "onset_beat", "duration_beat", "is_note_onset",
        "score_start", "n_notes", "n_scores", "feature_set", "x", "ld_x", "faults"]
    c = _lib.CONSTS
    assert (c["AGNN_NF_VOICE"], c["AGNN_NF_CADENCE"], c["AGNN_NF_VOICE_WIDTH"], c["AGNN_NF_CADENCE_WIDTH"]) == (0, 1, 25, 56)
    assert sorted(descriptors.FAULT_NAMES) == list(range(c["AGNN_NF_FAULT_WORDS"])) == list(range(5))
    assert len(descriptors.VOICE_FEATURES) == 25 and len(descriptors.CADENCE_FEATURES) == 56


def test_public_names_and_unknown_sets():
    import analysisgnn_amd
    from analysisgnn_amd import descriptors
    assert analysisgnn_amd.note_features is descriptors.note_features
    assert analysisgnn_amd.VOICE_FEATURES is descriptors.VOICE_FEATURES and analysisgnn_amd.CADENCE_FEATURES is descriptors.CADENCE_FEATURES
    for name in ("chord", "panalysis", "Voice", ""):
        with pytest.raises(ValueError, match="'voice'.*'cadence'"):
            descriptors.note_features({}, name)


def test_cpu_tensors_raise():
    import torch
    from analysisgnn_amd import _lib, descriptors
    i, f = torch.zeros(4, dtype=torch.int64), torch.zeros(4)
    fields = dict(onset_div=i, duration_div=i, pitch=i, ts_beats=i + 4, onset_beat=f, duration_beat=f)
    with pytest.raises(_lib.AgnnError, match="no CPU fallback"):
        descriptors.note_features(fields)
    with pytest.raises(_lib.AgnnError, match="voice.*is_downbeat"):
        descriptors.note_features(fields, "cadence")
    with pytest.raises(_lib.AgnnError, match="pitch"):
        descriptors.note_features(dict(fields, pitch=i.to(torch.int32)))


def test_arguments():
    lib = _lib()
    big = 1 << 30
    f = lib.agnn_note_features_f32
    assert f(None, P, big, None) == EINVAL and b"f is null" in lib.agnn_last_error()
    for s in (0, -1):
        assert f(_args(n_scores=s), P, big, None) == EINVAL and f"n_scores={s}".encode() in lib.agnn_last_error()
    for n in (0, -5, 1 << 29):
        assert f(_args(n_notes=n), P, big, None) == EINVAL and f"n_notes={n}".encode() in lib.agnn_last_error()
    for field in (*INPUTS, "voice", "is_downbeat", "x", "faults"):
        assert f(_args(**{field: None}), P, big, None) == EINVAL and b"null" in lib.agnn_last_error(), field
    for field in INPUTS:
        assert f(_args(feature_set=VOICE, ld_x=25, **{field: None}), P, big, None) == EINVAL, field
    for fs in (2, -1):
        assert f(_args(feature_set=fs), P, big, None) == EINVAL and f"feature_set={fs}".encode() in lib.agnn_last_error()
    assert f(_args(ld_x=55), P, big, None) == EINVAL and b"ld_x=55" in lib.agnn_last_error()
    assert f(_args(feature_set=VOICE, ld_x=24), P, big, None) == EINVAL and b"ld_x=24" in lib.agnn_last_error()
    assert f(_args(), None, big, None) == EINVAL and b"workspace is null" in lib.agnn_last_error()
    assert f(_args(), P, 16, None) == ENOMEM and b"needed" in lib.agnn_last_error()
    need = lib.agnn_note_features_workspace_bytes(100, 2, CADENCE)
    assert f(_args(), P, need - 1, None) == ENOMEM
    assert f(_args(feature_set=VOICE, ld_x=25), P, 16, None) == ENOMEM


def test_workspace_sizes():
    lib = _lib()
    w = lib.agnn_note_features_workspace_bytes
    assert w(0, 1, CADENCE) == 0 and w(10, 0, CADENCE) == 0 and w(10, 1, 2) == 0 and w(1 << 29, 1, VOICE) == 0
    for fs in (VOICE, CADENCE):
        sizes = [w(n, 1, fs) for n in (1, 2, 63, 64, 500, 501, 4096, 16000, 1 << 20)]
        assert sizes[0] > 0 and sizes == sorted(sizes), (fs, sizes)                 # monotone in n_notes
    assert w(500, 1, CADENCE) < w(16000, 32, CADENCE) and w(500, 1, VOICE) < w(500, 1, CADENCE)
    assert w(500, 1, CADENCE) <= w(500, 4096, CADENCE)
