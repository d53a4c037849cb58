"""Plain torch statement of the two in-tree aggregations the HIP kernels csrc/gated.hip and csrc/reledge.hip compute, on COO
edge lists, in any floating dtype.  TEST INFRASTRUCTURE ONLY.

    gated    S_i = sum_{e: dst[e] = i} sigmoid(a_i + b_{src[e]} [+ c_e]) * h_{src[e]}           (core/gnn.py:246-257)
    absdiff  S_i = sum_{e: dst[e] = i} h_{src[e]} ,   D_i = sum_{e: dst[e] = i} |h_i - h_{src[e]}|   (core/gnn.py:99-105)

Only the forward is written down; every gradient is torch.autograd's (the subgradient of |.| at 0 is therefore torch's own:
sign(0) = 0).  PARITY: composed with the layers' Linear maps these reproduce the fixtures `resgated*` / `r2_reledge*`
(tests/test_oracle_intree_agg.py)."""
from __future__ import annotations

from typing import Optional

import torch


def _leaf(t: Optional[torch.Tensor], dtype) -> Optional[torch.Tensor]:
    return None if t is None else t.detach().to(dtype).clone().requires_grad_(True)


def _index_sum(msg: torch.Tensor, dst: torch.Tensor, n: int) -> torch.Tensor:
    out = msg.new_zeros((n, msg.shape[1]))
    return out.index_add(0, dst, msg) if dst.numel() else out


def gated_forward(a, b, h, c, dst, src):
    """a [n_dst, H]; b, h [n_src, H]; c [E, H] or None; dst, src int64 [E]  ->  S [n_dst, H] (differentiable)."""
    z = a[dst] + b[src]
    if c is not None:
        z = z + c
    return _index_sum(torch.sigmoid(z) * h[src], dst, a.shape[0])


def gated(a, b, h, c, dst, src, ds, dtype=torch.float64):
    """-> S, da, db, dh, dc (dc None without c): the forward and the gradients of <S, ds> in `dtype`."""
    a, b, h, c = _leaf(a, dtype), _leaf(b, dtype), _leaf(h, dtype), _leaf(c, dtype)
    S = gated_forward(a, b, h, c, dst, src)
    leaves = [a, b, h] + ([c] if c is not None else [])
    grads = torch.autograd.grad((S * ds.to(dtype)).sum(), leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
    return (S.detach(), *grads[:3], grads[3] if c is not None else None)


def absdiff_forward(h, dst, src):
    """h [n, H]; dst, src int64 [E]  ->  S, D [n, H] (differentiable)."""
    n = h.shape[0]
    return _index_sum(h[src], dst, n), _index_sum((h[dst] - h[src]).abs(), dst, n)


def absdiff_ends(h, dst, src, gs=None, gd=None, dtype=torch.float64):
    """-> S, D, dh_row, dh_col: as `absdiff`, with the gradient of <S, gs> + <D, gd> split by the END of the edge it arrives
    through — dh_row what h receives as the aggregating row i (h[dst]), dh_col as the gathered row j (h[src]); their sum is
    `absdiff`'s dh.  Two leaves holding the same values and autograd; no formula of its own."""
    hi, hj = _leaf(h, dtype), _leaf(h, dtype)
    n = hi.shape[0]
    S, D = _index_sum(hj[src], dst, n), _index_sum((hi[dst] - hj[src]).abs(), dst, n)
    loss = (hi * 0).sum() + (hj * 0).sum()
    if gs is not None:
        loss = loss + (S * gs.to(dtype)).sum()
    if gd is not None:
        loss = loss + (D * gd.to(dtype)).sum()
    gi, gj = torch.autograd.grad(loss, [hi, hj])
    return S.detach(), D.detach(), gi, gj


def absdiff(h, dst, src, gs=None, gd=None, dtype=torch.float64):
    """-> S, D, dh: the forward and the gradient of <S, gs> + <D, gd> (an absent term counts as zero) in `dtype`."""
    h = _leaf(h, dtype)
    S, D = absdiff_forward(h, dst, src)
    loss = (h * 0).sum()
    if gs is not None:
        loss = loss + (S * gs.to(dtype)).sum()
    if gd is not None:
        loss = loss + (D * gd.to(dtype)).sum()
    (dh,) = torch.autograd.grad(loss, [h])
    return S.detach(), D.detach(), dh
