"""Pure-torch restatement of the pretraining stage, for float64 on the CPU.  TEST INFRASTRUCTURE ONLY.

Restated from the reference: `PreEncoder`'s four heads and link logits (models/analysis.py:367-403), `isin_pairwise` (:23-41) and
`PreEncoderPL._common_step` :704-731, with torch's own `BCEWithLogitsLoss` / `CrossEntropyLoss(label_smoothing=0.1)`.
tests/test_pretrain_ref.py holds it against fixtures produced by the reference's own source (tests/gen_golden_pretrain.py).
`link_task` is the per-task operator in the layout of `agnn_link_bce_fwd_f32` (one entry per candidate, alive or not)."""
from typing import Dict, Mapping, Tuple

import torch
import torch.nn.functional as F

ONSET = ("note", "onset", "note")
CONSECUTIVE = ("note", "consecutive", "note")
STAFF = ("note", "staff", "note")
VOICE = ("note", "voice", "note")
HEADS = ("staff_clf", "voice_clf", "fifths_clf", "spelling_clf")


def head(P: Mapping[str, torch.Tensor], name: str, x: torch.Tensor) -> torch.Tensor:
    """nn.Sequential(Linear, ReLU, LayerNorm, Linear): state_dict keys <name>.{0,2,3}.*"""
    y = F.relu(x @ P[f"{name}.0.weight"].t() + P[f"{name}.0.bias"])
    y = F.layer_norm(y, (y.shape[-1],), P[f"{name}.2.weight"], P[f"{name}.2.bias"], 1e-5)
    return y @ P[f"{name}.3.weight"].t() + P[f"{name}.3.bias"]


def isin_pairwise(element: torch.Tensor, test_elements: torch.Tensor) -> torch.Tensor:
    """:23-41: membership of the pairs element[:, i] among the pairs test_elements[:, j], through Cantor's pairing."""
    def cantor(a, b):
        return (a + b) * (a + b + 1) // 2 + b
    return torch.isin(cantor(element[0], element[1]), cantor(test_elements[0], test_elements[1]))


def decode(P, x, staff_candidates, voice_candidates):
    """:397-403 behind the encoder: (staff_logits, voice_logits, fifths_logits, spelling_logits) from the embedding x."""
    staff_x, voice_x = head(P, "staff_clf", x), head(P, "voice_clf", x)
    staff_logits = (staff_x[staff_candidates[0]] * staff_x[staff_candidates[1]]).sum(-1)
    voice_logits = (voice_x[voice_candidates[0]] * voice_x[voice_candidates[1]]).sum(-1)
    return staff_logits, voice_logits, head(P, "fifths_clf", x), head(P, "spelling_clf", x)


def _to_batch(e: torch.Tensor, batch_size: int) -> torch.Tensor:
    return e[:, torch.logical_and(e[0] < batch_size, e[1] < batch_size)]                       # :712-717


def common_step(P, x, edge_index_dict: Dict[tuple, torch.Tensor], batch_size: int, key_signature, pitch_spelling, sort: bool = True):
    """:704-731 from the embedding x [batch_size, H] on.  Returns a dict: the filtered candidate lists, logits, labels, the four
    losses and their sum.  `sort=False` leaves out the source argsort of :707 (the losses do not depend on it)."""
    staff_c = torch.cat((edge_index_dict[ONSET], edge_index_dict[CONSECUTIVE]), dim=1)         # :704-705
    if sort:
        staff_c = staff_c[:, staff_c[0].argsort()]                                             # :707
    voice_c = edge_index_dict[CONSECUTIVE]                                                     # :708
    staff_c, voice_c = _to_batch(staff_c, batch_size), _to_batch(voice_c, batch_size)
    staff_t, voice_t = _to_batch(edge_index_dict[STAFF], batch_size), _to_batch(edge_index_dict[VOICE], batch_size)
    staff_y, voice_y = isin_pairwise(staff_c, staff_t), isin_pairwise(voice_c, voice_t)        # :718-719
    staff_l, voice_l, fifths_l, spelling_l = decode(P, x, staff_c, voice_c)
    bce = torch.nn.BCEWithLogitsLoss()
    ce = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    out = {"staff_candidates": staff_c, "voice_candidates": voice_c, "staff_logits": staff_l, "voice_logits": voice_l,
           "fifths_logits": fifths_l, "spelling_logits": spelling_l, "staff_labels": staff_y, "voice_labels": voice_y,
           "staff": bce(staff_l.squeeze(), staff_y.squeeze().to(staff_l.dtype)),
           "voice": bce(voice_l.squeeze(), voice_y.squeeze().to(voice_l.dtype)),
           "fifths": ce(fifths_l, key_signature[:batch_size]), "spelling": ce(spelling_l, pitch_spelling[:batch_size])}
    out["total"] = out["staff"] + out["voice"] + out["fifths"] + out["spelling"]
    return out


def link_task(z: torch.Tensor, cand: torch.Tensor, true: torch.Tensor, limit: int) -> Tuple[torch.Tensor, ...]:
    """One link task over ALL candidates cand [2, E] on the rows of z: (logits [E] with 0 where not alive, labels bool [E],
    alive bool [E], mean loss over the alive candidates — 0 when there is none, where torch gives NaN).  Differentiable in z."""
    alive = (cand[0] >= 0) & (cand[1] >= 0) & (cand[0] < limit) & (cand[1] < limit)
    c = cand[:, alive]
    t = true[:, (true[0] < limit) & (true[1] < limit)]
    y = isin_pairwise(c, t)
    x = (z[c[0]] * z[c[1]]).sum(-1)
    logits = torch.zeros(cand.shape[1], dtype=z.dtype).index_put((alive.nonzero().reshape(-1),), x)
    labels = torch.zeros(cand.shape[1], dtype=torch.bool)
    labels[alive] = y
    loss = torch.nn.BCEWithLogitsLoss()(x, y.to(z.dtype)) if c.shape[1] else (z.sum() * 0)
    return logits, labels, alive, loss


def confusion(logits: torch.Tensor, labels: torch.Tensor, alive: torch.Tensor):
    """[alive, tp, fp, fn, tn] with "predicted positive" = logit > 0 (sigmoid > 0.5)."""
    pos = logits > 0
    return [int(alive.sum()), int((alive & pos & labels).sum()), int((alive & pos & ~labels).sum()), int((alive & ~pos & labels).sum()),
            int((alive & ~pos & ~labels).sum())]


def binary_f1(tp: int, fp: int, fn: int) -> float:
    return 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn > 0 else 0.0
