"""Note descriptors computed on the device (csrc/notefeat.hip): from the note array a score parser yields to `x_note`, the per-note
rows that `in_channels` counts.  Replaces the reference's `select_features(note_array, "voice" | "cadence")`
(descriptors/general.py:110-139): `get_voice_separation_features` (descriptors/utils/note_features.py:176-226, 25 columns) and
`get_cad_features(include_pitch_spelling=False)` (descriptors/utils/cadence_features.py:6-119, 31 more; an O(N^2) Python loop).
Columns, order and quirks are the reference's ("Note descriptors").  No CPU path."""
from __future__ import annotations

from typing import Mapping, Optional

import torch

from . import _lib, resident
from .score_graph import _i64, _starts

VOICE_FEATURES = ["bar_exp_duration", "onset_bar_norm", "is_down_beat"] + [f"pc_{i:02d}" for i in range(12)] + \
                 [f"octave_{i:02d}" for i in range(10)]
CADENCE_FEATURES = VOICE_FEATURES + [
    "perfect_triad", "perfect_major_triad", "is_sus4", "in_perfect_triad_or_sus4", "highest_is_3", "highest_is_1",
    "bass_compatible_with_I", "bass_compatible_with_I_scale", "one_comes_from_7", "one_comes_from_1", "one_comes_from_2",
    "three_comes_from_4", "five_comes_from_5", "strong_beat", "sustained_note", "is_note_onset", "rest_highest", "rest_lowest",
    "rest_middle", "voice_ends", "is_downbeat", "v7", "v7-3", "has_7", "has_9", "bass_voice", "bass_moves_chromatic",
    "bass_moves_octave", "bass_compatible_v-i", "bass_compatible_i-v", "bass_moves_2M"]
FEATURE_SETS = {"voice": (_lib.CONSTS["AGNN_NF_VOICE"], _lib.CONSTS["AGNN_NF_VOICE_WIDTH"]),
                "cadence": (_lib.CONSTS["AGNN_NF_CADENCE"], _lib.CONSTS["AGNN_NF_CADENCE_WIDTH"])}
FAULT_WORDS = _lib.CONSTS["AGNN_NF_FAULT_WORDS"]
FAULT_NAMES = {
    _lib.CONSTS["AGNN_NF_FAULT_PITCH"]: "pitch outside [0, 120)",
    _lib.CONSTS["AGNN_NF_FAULT_TS"]: "ts_beats <= 0",
    _lib.CONSTS["AGNN_NF_FAULT_VOICE"]: "voice outside [0, 2^15)",
    _lib.CONSTS["AGNN_NF_FAULT_ORDER"]: "onset_div that decreases inside a score",
    _lib.CONSTS["AGNN_NF_FAULT_SCORES"]: "score_start does not tile the notes",
}
INT_FIELDS = ("onset_div", "duration_div", "pitch", "ts_beats")
CADENCE_INT_FIELDS = ("voice", "is_downbeat")
FLOAT_FIELDS = ("onset_beat", "duration_beat")


def _f32(t, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1:
        raise _lib.AgnnError(f"{what}: 1-D float32 device tensor expected")
    return t if t.is_contiguous() else t.contiguous()


def _feature_set(feature_type: str):
    if feature_type not in FEATURE_SETS:
        raise ValueError(f"feature_type {feature_type!r}: the supported sets are 'voice' (25 columns) and 'cadence' (56 columns)")
    return FEATURE_SETS[feature_type]


def note_features(fields: Mapping[str, torch.Tensor], feature_type: str = "voice", score_start=None,
                  out: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
    """float32 [N, 25] ("voice", `VOICE_FEATURES`) or [N, 56] ("cadence", `CADENCE_FEATURES`) of the notes in `fields`, a mapping of
    device tensors by the reference's field names: int64 `onset_div`, `duration_div`, `pitch`, `ts_beats`, float32 `onset_beat`,
    `duration_beat`; for "cadence" also int64 `voice`, `is_downbeat`; optional `is_note_onset` (bool / uint8, absent = all ones).
    The notes of a score are in (onset, pitch) order (`score_graph.sort_notes`); `score_start` delimits several scores as for
    `build_score_graph`.  `out`: a float32 matrix (or column block of a wider one, unit column stride) to write into; without it
    the rows are padded to a multiple of four floats, the layout the input projection reads in place.

    check=True reads the fault words once (synchronises; eager only, AgnnError under stream capture) and raises AgnnError naming
    every kind of bad input.  check=False never reads the device and is capturable: the result carries the words as
    `.agnn_faults` (int32 [5], indexed by AGNN_NF_FAULT_*), an offending note's row is zeros."""
    set_id, width = _feature_set(feature_type)
    cadence = feature_type == "cadence"
    needed = (*INT_FIELDS, *FLOAT_FIELDS, *(CADENCE_INT_FIELDS if cadence else ()))
    missing = [k for k in needed if fields.get(k) is None]
    if missing:
        raise _lib.AgnnError(f"note_features({feature_type!r}) needs the fields {missing}")
    t = {k: _i64(fields[k], k) for k in needed if k not in FLOAT_FIELDS}
    t.update({k: _f32(fields[k], k) for k in FLOAT_FIELDS})
    note_onset = fields.get("is_note_onset")
    if note_onset is not None:
        if not isinstance(note_onset, torch.Tensor) or note_onset.dtype not in (torch.bool, torch.uint8) or note_onset.dim() != 1:
            raise _lib.AgnnError("is_note_onset: 1-D bool or uint8 device tensor expected")
        note_onset = note_onset.contiguous().view(torch.uint8)
    dev = _lib.require_gpu(*t.values(), note_onset, out)
    n = int(t["pitch"].numel())
    if n < 1 or any(int(v.numel()) != n for v in (*t.values(), *(() if note_onset is None else (note_onset,)))):
        raise _lib.AgnnError(f"every field needs the same length >= 1, got {({k: int(v.numel()) for k, v in t.items()})}")
    capturing = torch.cuda.is_current_stream_capturing()
    if check and capturing:
        raise _lib.AgnnError("note_features(check=True) reads the fault words on the host: eager only; under stream capture "
                             "pass check=False and read `.agnn_faults` after the replay")
    if score_start is None:                  # [0, n], filled on the device: nothing crosses from the host under capture
        start_dev = torch.zeros(2, dtype=torch.int32, device=dev)
        start_dev[1] = n
    elif capturing and not (isinstance(score_start, torch.Tensor) and score_start.is_cuda):
        raise _lib.AgnnError("note_features under stream capture: pass score_start as an int32 device tensor")
    else:
        _, start_dev = _starts(score_start, n, dev, read_device=False)
    n_scores = int(start_dev.numel() - 1)
    if out is None:
        out = torch.empty((n, (width + 3) & ~3), dtype=torch.float32, device=dev)[:, :width]
    elif (out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (n, width) or out.stride(1) != 1
          or (n > 1 and out.stride(0) < width)):
        raise _lib.AgnnError(f"out: float32 [{n}, {width}] with unit column stride expected, got {out.dtype} {tuple(out.shape)} "
                             f"strides {tuple(out.stride())}")
    ld = int(out.stride(0)) if n > 1 else max(int(out.stride(0)), width)
    lib = _lib.load()
    if check:       # a ticket: zero when it is handed out, zero again when the call is over
        faults = resident.scratch(dev, "note_features faults", 4 * FAULT_WORDS, zeroed=True).view(torch.int32)
    else:
        faults = torch.zeros(FAULT_WORDS, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.agnn_note_features_workspace_bytes(n, n_scores, set_id))
    ws = resident.scratch(dev, "note_features", ws_bytes, zeroed=False)

    a = _lib.NoteFeaturesArgs()
    a.onset_div, a.duration_div, a.pitch, a.ts_beats = (t[k].data_ptr() for k in INT_FIELDS)
    a.voice, a.is_downbeat = (_lib.ptr(t.get(k)) for k in CADENCE_INT_FIELDS)
    a.onset_beat, a.duration_beat = (t[k].data_ptr() for k in FLOAT_FIELDS)
    a.is_note_onset = _lib.ptr(note_onset)
    a.score_start, a.n_notes, a.n_scores, a.feature_set = start_dev.data_ptr(), n, n_scores, set_id
    a.x, a.ld_x, a.faults = out.data_ptr(), ld, faults.data_ptr()
    _lib.check(lib.agnn_note_features_f32(a, ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev)), "agnn_note_features_f32")
    if check:
        words = faults.tolist()                                      # the one host read
        bad = [f"{FAULT_NAMES[k]} ({c})" for k, c in enumerate(words) if c]
        if bad:
            faults.zero_()
            raise _lib.AgnnError("note array faults: " + "; ".join(bad))
    else:
        out.agnn_faults = faults
    return out
