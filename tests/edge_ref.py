"""Pure-torch restatement of the edge-consistency term, for float64 on the CPU.  TEST INFRASTRUCTURE ONLY.

Restated from the reference: `EdgeDecoder` (models/analysis.py:805-836) and the edge term of `ContinualAnalysisGNN.common_step`
(:987-1019) from the selected edges on, with torch's own `CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)`.  Parameters are
a dict under the reference's state_dict keys (`embed.<rel>.{0,2}.*`, `fc.{0,2,4}.*`).  tests/test_edge_ref.py holds it against
fixtures produced by the reference's own source (tests/gen_golden_edge.py).  `pair_features`, `pair_backward` and `confusion` are
the operators in the layout of csrc/edgedec.hip (one entry per edge, alive or not)."""
from typing import Dict, Mapping, Optional, Tuple

import torch
import torch.nn.functional as F

RNA_KEYS = ("quality", "inversion", "degree1", "degree2", "localkey")


def embed(P: Mapping[str, torch.Tensor], rel: str, x: torch.Tensor) -> torch.Tensor:
    """embed[rel] = Sequential(Linear, ReLU, LayerNorm, Dropout) with the dropout off: row-wise."""
    y = F.relu(x @ P[f"embed.{rel}.0.weight"].t() + P[f"embed.{rel}.0.bias"])
    return F.layer_norm(y, (y.shape[-1],), P[f"embed.{rel}.2.weight"], P[f"embed.{rel}.2.bias"], 1e-5)


def fc(P: Mapping[str, torch.Tensor], f: torch.Tensor) -> torch.Tensor:
    """fc = Sequential(Linear, ReLU, LayerNorm, Dropout, Linear(channels, 2)) with the dropout off."""
    y = F.relu(f @ P["fc.0.weight"].t() + P["fc.0.bias"])
    y = F.layer_norm(y, (y.shape[-1],), P["fc.2.weight"], P["fc.2.bias"], 1e-5)
    return y @ P["fc.4.weight"].t() + P["fc.4.bias"]


def decode(P, x: torch.Tensor, edge_dict: Dict[str, Tuple[torch.Tensor, torch.Tensor]]) -> Dict[str, torch.Tensor]:
    """`EdgeDecoder.forward` (:826-836), keyed by relation name: the gathers come first there, the result is the same."""
    return {r: fc(P, embed(P, r, x[s]) * embed(P, r, x[d])) for r, (s, d) in edge_dict.items()}


def edge_labels(labels: torch.Tensor, s: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """:1007-1010: 1 where all rows of labels [K, N] agree at s and d (equal -1s are equal)."""
    return (labels[:, s] == labels[:, d]).all(dim=0).long()


def edge_term(P, x, kept: Dict[str, Tuple[torch.Tensor, torch.Tensor]], labels: torch.Tensor, smoothing: float = 0.1):
    """:1001-1019 on the selected edges `kept` (relation name -> (src, dst), every edge alive): {"logits", "labels", "losses"} per
    relation and "total" = mean of the relations' losses.  A relation without an edge has loss 0 (the build's departure; torch
    gives NaN) and still counts in the division."""
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=smoothing)
    logits = decode(P, x, kept)
    y = {r: edge_labels(labels, s, d) for r, (s, d) in kept.items()}
    losses = {r: ce(logits[r], y[r]) if logits[r].shape[0] else x.sum() * 0 for r in kept}
    total = sum(losses.values()) / len(kept)
    return {"logits": logits, "labels": y, "losses": losses, "total": total}


def alive_mask(s: torch.Tensor, d: torch.Tensor, limit: int) -> torch.Tensor:
    return (s >= 0) & (d >= 0) & (s < limit) & (d < limit)


def pair_features(a: torch.Tensor, s: torch.Tensor, d: torch.Tensor, limit: int, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F [E, H] = mask * a[s] * a[d] for alive edges, zero rows otherwise (`mask`: the product of the two ends' keep factors)."""
    ok = alive_mask(s, d, limit)
    f = torch.zeros((s.numel(), a.shape[1]), dtype=a.dtype)
    prod = a[s[ok]] * a[d[ok]]
    if mask is not None:
        prod = prod * mask[ok]
    return f.index_put((ok.nonzero().reshape(-1),), prod)


def pair_backward(a: torch.Tensor, s, d, limit: int, df: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dA of `pair_features` by autograd."""
    a = a.detach().clone().requires_grad_(True)
    (pair_features(a, s, d, limit, mask) * df).sum().backward()
    return a.grad


def confusion(logits: torch.Tensor, labels: torch.Tensor, alive: torch.Tensor):
    """[alive, tp, fp, fn, tn] with "predicted positive" = logit 1 > logit 0."""
    pos, labels = logits[:, 1] > logits[:, 0], labels.bool()
    return [int(alive.sum()), int((alive & pos & labels).sum()), int((alive & pos & ~labels).sum()), int((alive & ~pos & labels).sum()),
            int((alive & ~pos & ~labels).sum())]
