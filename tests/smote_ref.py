"""Float64 restatement of the reference's SMOTE oversampling and feature penalty (models/cadence.py:13-118,
models/analysis.py:1412-1438), written from its rules and independent of the package: the oracle of tests/test_smote_ref.py
(against fixtures recorded from the reference itself) and of tests/test_gpu_smote.py.  Draws and permutations are arguments,
never generated here; everything is torch float64 on the CPU, so `torch.autograd` gives the reference gradients.

Rules (see analysisgnn_amd/smote.py for the longer statement):
  plan        dominant = first arg-max of the counts; ascending labels; skip the dominant class, occ < k, occ == n_occ;
              copies = int(((n_occ - occ) * 100 / occ) / 100) in float32, 0 adds nothing
  neighbours  'euclidian': ranks 1..k of ascending Euclidean distance; anything else: ranks 1..k of ASCENDING cosine similarity of
              rows normalised with eps 1e-12 (the least similar rows); stable sort; min(k, T - 1) columns
  synthesis   row (i, n) -> x_i + gap * (x_nb[choice] - x_i), choice in [0, k - 2], gap per feature; output = originals, then
              class by class, row i * copies + n
  penalty     bs = batch_size // n_unique(y_over); per class (ascending) the rows of x, then those of x_over, are cut to bs rows by
              a permutation when longer; mean(clamp(min_j |q - c_j| - threshold, min=0)) summed over the classes"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch


def plan(counts: Sequence[int], k: int) -> List[Tuple[int, int, int]]:
    """[(label, occ, copies)] of the classes that add rows, in output order."""
    counts = [int(c) for c in counts]
    if not counts:
        return []
    dominant = max(range(len(counts)), key=lambda c: (counts[c], -c))
    n_occ = counts[dominant]
    out = []
    for c, occ in enumerate(counts):
        if c == dominant or occ < k:
            continue
        n = (np.float32(n_occ) - np.float32(occ)) * np.float32(100) / np.float32(occ)
        if n == 0:
            continue
        copies = int(n / np.float32(100))
        if copies > 0:
            out.append((c, occ, copies))
    return out


def scores(xc: torch.Tensor, distance: str) -> torch.Tensor:
    """[T, T] float64: what the reference argsorts (cosine similarity, or Euclidean distance SQUARED — the same order)."""
    xc = xc.detach().double()
    if distance == "euclidian":
        return ((xc[:, None, :] - xc[None, :, :]) ** 2).sum(-1)
    z = xc / xc.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return z @ z.t()


def neighbours(xc: torch.Tensor, k: int, distance: str) -> torch.Tensor:
    """int64 [T, min(k, T - 1)]: columns 1..k of the stable ascending argsort."""
    return torch.sort(scores(xc, distance), dim=1, stable=True).indices[:, 1:k + 1]


def fit_generate(x: torch.Tensor, y: torch.Tensor, choice: torch.Tensor, gap: torch.Tensor, k: int = 3, distance: str = "euclidean",
                 tables: Optional[dict] = None):
    """x [N, D] (float64, may require grad), y int64 [N], choice int [S], gap [S, D] -> (x_over [N + S, D], y_over, info).
    `tables` {label: int64 [T, >= k - 1] neighbour table in class-local indices}: used instead of the float64 one where given.
    info: `tables` (those used), `rows` {label: rows of x}, `nb_row` int64 [S] (the neighbour's row of x per synthetic row)."""
    counts = torch.bincount(y).tolist() if y.numel() else []
    parts, labels, nb_rows = [x], [y.long()], []
    used, rows_of = {}, {}
    s = 0
    for c, occ, copies in plan(counts, k):
        rows = torch.nonzero(y == c)[:, 0]
        xc = x[rows]
        tab = tables[c] if tables is not None and c in tables else neighbours(xc, k, distance)
        used[c], rows_of[c] = tab, rows
        n = occ * copies
        ch = choice[s:s + n].long()
        gp = gap[s:s + n].to(x.dtype)
        own = torch.arange(occ).repeat_interleave(copies)
        nb = tab[own, ch]
        parts.append(xc[own] + gp * (xc[nb] - xc[own]))
        labels.append(torch.full((n,), c, dtype=torch.int64))
        nb_rows.append(rows[nb])
        s += n
    info = dict(tables=used, rows=rows_of, nb_row=torch.cat(nb_rows) if nb_rows else torch.zeros(0, dtype=torch.int64), S=s)
    return torch.cat(parts), torch.cat(labels), info


def n_synthetic(y: torch.Tensor, k: int) -> int:
    return sum(occ * copies for _, occ, copies in plan(torch.bincount(y).tolist() if y.numel() else [], k))


def feature_penalty(x_over: torch.Tensor, y_over: torch.Tensor, x: torch.Tensor, y: torch.Tensor, perms: Sequence[torch.Tensor],
                    batch_size: int = 100, threshold: float = 1.0) -> torch.Tensor:
    """The sum over the classes (a float64 scalar, differentiable).  `perms`: the permutations in the order the reference draws
    them.  A minimum distance of exactly 0 has gradient 0."""
    perms = list(perms)
    classes = torch.unique(y_over).tolist()
    bs = batch_size // len(classes)
    total = x_over.new_zeros(())
    for c in classes:
        xc = x[y == c]
        qc = x_over[y_over == c]
        if len(xc) > bs:
            xc = xc[perms.pop(0).long()[:bs]]
        if len(qc) > bs:
            qc = qc[perms.pop(0).long()[:bs]]
        d2 = ((qc[:, None, :] - xc[None, :, :]) ** 2).sum(-1)
        m2 = d2.min(dim=1).values
        pos = m2 > 0
        d = torch.where(pos, torch.where(pos, m2, torch.ones_like(m2)).sqrt(), torch.zeros_like(m2))
        total = total + torch.clamp(d - threshold, min=0).mean()
    assert not perms, "more permutations than the classes need"
    return total


def n_perms(y_over: torch.Tensor, y: torch.Tensor, batch_size: int = 100) -> List[int]:
    """Lengths of the permutations the penalty needs, in drawing order."""
    classes = torch.unique(y_over).tolist()
    bs = batch_size // len(classes)
    out = []
    for c in classes:
        for n in (int((y == c).sum()), int((y_over == c).sum())):
            if n > bs:
                out.append(n)
    return out
