"""Plain reference of the HGT edge-softmax attention, forward and backward.  TEST INFRASTRUCTURE ONLY.

Written from the formulas in include/agnn.h (`agnn_hgt_attn_*`) / SURVEY.md App. A.4 with dense index ops on the COO lists:
no CSR, no tiling, no online softmax.  For destination row i, head h (D = H / heads floats per head), over ALL kept
edges e of all relations that end in the row:

    forward   s_e = <q_dst,h , k_src,h> * pscale[h]        m = rowwise max of s        l = sum exp(s - m)
              linv = 1 / (l + 1e-16)                       alpha_e = exp(s_e - m) * linv
              out_i,h = sum_e alpha_e v_src,h              (rows without edges: out = 0, m = -inf, linv = 1 / 1e-16)
    backward  dsum_i,h = <dm_i,h , out_i,h>                ds_e = alpha_e (<dm_dst,h , v_src,h> - dsum_dst,h)
              gs_e = ds_e * pscale[h]                      tdot_e = ds_e * <q_dst,h , k_src,h>
              dq_i,h = sum_e gs_e k_src,h                  dk_j,h = sum_e gs_e q_dst,h         dv_j,h = sum_e alpha_e dm_dst,h

Trimming (PyG `trim_to_layer`: COO prefix, row prefix) is applied by MASKING THE COO LIST: a relation's `e_limit` keeps
the COO positions < e_limit, `n_keep` keeps the edges with dst < n_keep and computes the rows < n_keep only.

A relation is a dict with `k`, `v` [n_src, H], `src`, `dst` [E] (int64), `pscale` [heads] and optionally `e_limit`.
`dtype` picks the arithmetic: float64 for the reference, float32 to measure what rounding the same formulas suffer in
plain single precision (the yardstick of the kernels' tolerance)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch


def kept_edges(rel: dict, n_rows: int) -> torch.Tensor:
    """bool [E]: the COO positions of `rel` that take part when `n_rows` destination rows are computed."""
    E = int(rel["src"].numel())
    keep = rel["dst"] < n_rows
    lim = rel.get("e_limit")
    if lim is not None:
        keep = keep & (torch.arange(E) < int(lim))
    return keep


def forward(q: torch.Tensor, heads: int, rels: Sequence[dict], n_keep: Optional[int] = None, dtype=torch.float64) -> dict:
    """The forward formulas in torch ops of `dtype` (differentiable w.r.t. q and every relation's k, v, pscale).
    Returns out [n, H], m, linv [n, heads] and, per relation, the kept mask and the kept edges' src, dst, dot, alpha."""
    n = int(q.shape[0]) if n_keep is None else int(n_keep)
    H = int(q.shape[1])
    D = H // heads
    qh = q.to(dtype)[:n].reshape(n, heads, D)
    per: List[dict] = []
    for rel in rels:
        keep = kept_edges(rel, n)
        src, dst = rel["src"][keep], rel["dst"][keep]
        kh = rel["k"].to(dtype).reshape(-1, heads, D)
        vh = rel["v"].to(dtype).reshape(-1, heads, D)
        dot = (qh[dst] * kh[src]).sum(-1)                                        # [e, heads]
        per.append(dict(keep=keep, src=src, dst=dst, dot=dot, s=dot * rel["pscale"].to(dtype).view(1, heads), val=vh[src]))
    if per:
        dst_all = torch.cat([p["dst"] for p in per])
        s_all = torch.cat([p["s"] for p in per])
        val_all = torch.cat([p["val"] for p in per])
    else:
        dst_all = torch.zeros(0, dtype=torch.int64)
        s_all, val_all = torch.zeros(0, heads, dtype=dtype), torch.zeros(0, heads, D, dtype=dtype)
    m = torch.full((n, heads), -float("inf"), dtype=dtype).scatter_reduce(
        0, dst_all.unsqueeze(-1).expand(-1, heads), s_all.detach(), reduce="amax", include_self=True)
    ex = torch.exp(s_all - m[dst_all])
    l = torch.zeros(n, heads, dtype=dtype).index_add(0, dst_all, ex)
    linv = 1.0 / (l + 1e-16)
    alpha = ex * linv[dst_all]
    out = torch.zeros(n, heads, D, dtype=dtype).index_add(0, dst_all, alpha.unsqueeze(-1) * val_all).reshape(n, H)
    pos = 0
    for p in per:
        e = int(p["dst"].numel())
        p["alpha"] = alpha[pos:pos + e]
        pos += e
    return dict(out=out, m=m, linv=linv, per=per)


def attention(q: torch.Tensor, dm: torch.Tensor, heads: int, rels: Sequence[dict], n_keep: Optional[int] = None,
              dtype=torch.float64) -> dict:
    """Forward and the closed-form backward for the upstream gradient `dm` of `out`.
    Returns out, dq [n, H], m, linv [n, heads] and `rels`: per relation alpha, gs, tdot [E, heads] (NaN at the COO
    positions that are not kept), dk, dv [n_src, H] and the kept mask."""
    with torch.no_grad():
        f = forward(q, heads, rels, n_keep, dtype)
        out = f["out"]
        n, H = out.shape
        D = H // heads
        qh = q.to(dtype)[:n].reshape(n, heads, D)
        dmh = dm.to(dtype)[:n].reshape(n, heads, D)
        dsum = (dmh * out.view(n, heads, D)).sum(-1)                             # [n, heads]
        dq = torch.zeros(n, heads, D, dtype=dtype)
        res: List[Dict[str, torch.Tensor]] = []
        for rel, p in zip(rels, f["per"]):
            src, dst, alpha, dot = p["src"], p["dst"], p["alpha"], p["dot"]
            E, n_src = int(rel["src"].numel()), int(rel["k"].shape[0])
            ps = rel["pscale"].to(dtype).view(1, heads)
            kh = rel["k"].to(dtype).reshape(-1, heads, D)
            ds = alpha * ((dmh[dst] * p["val"]).sum(-1) - dsum[dst])
            gs = ds * ps
            tdot = ds * dot
            dq = dq.index_add(0, dst, gs.unsqueeze(-1) * kh[src])
            dk = torch.zeros(n_src, heads, D, dtype=dtype).index_add(0, src, gs.unsqueeze(-1) * qh[dst])
            dv = torch.zeros(n_src, heads, D, dtype=dtype).index_add(0, src, alpha.unsqueeze(-1) * dmh[dst])
            full = {}
            for name, t in (("alpha", alpha), ("gs", gs), ("tdot", tdot)):
                a = torch.full((E, heads), float("nan"), dtype=dtype)
                a[p["keep"]] = t
                full[name] = a
            full.update(dk=dk.reshape(n_src, H), dv=dv.reshape(n_src, H), keep=p["keep"])
            res.append(full)
        return dict(out=out, m=f["m"], linv=f["linv"], dq=dq.reshape(n, H), rels=res)
