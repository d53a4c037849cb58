"""Host side of the per-edge objectives (`pretrain.link_bce`, `edge_loss`), the counterpart of csrc/peredge.h: the edge-list
argument, the alive mask, the two CSRs of an edge list, and what the launch tables' entries share."""
import itertools

import torch

from . import _lib
from .graph import SegSpec


def edge_index(e, what: str, dev=None):
    """Contiguous (src, dst), int64 [E] each: a PyG edge_index [2, E] (returned whole: it unpacks into its rows), a pair, or None (empty)."""
    if e is None:
        return torch.zeros((2, 0), dtype=torch.int64, device=dev)
    if isinstance(e, torch.Tensor):
        if e.dim() != 2 or e.shape[0] != 2 or e.dtype != torch.int64:
            raise _lib.AgnnError(f"{what}: int64 [2, E] expected (a PyG edge_index), got {e.dtype} {tuple(e.shape)}")
        return e.contiguous()
    s, d = e
    if s.dtype != torch.int64 or d.dtype != torch.int64 or s.dim() != 1 or s.shape != d.shape:
        raise _lib.AgnnError(f"{what}: two int64 [E] index vectors expected")
    return s.contiguous(), d.contiguous()


def alive_mask(src, dst, limit: int):
    """The kernels' "alive": both ends in [0, limit)."""
    return (src >= 0) & (dst >= 0) & (src < limit) & (dst < limit)


def end_specs(src, dst, n_rows: int):
    """The `build_csr` segments of an edge list by source (col = destination) and by destination (col = source)."""
    return [SegSpec(row=src, col=dst, n_rows=n_rows), SegSpec(row=dst, col=src, n_rows=n_rows)]


def fill_csr(t, by_src, by_dst) -> None:
    """The two CSR triples of a backward table's entry."""
    t.s_rowptr, t.s_col, t.s_perm = by_src.rowptr.data_ptr(), by_src.col.data_ptr(), by_src.perm.data_ptr()
    t.d_rowptr, t.d_col, t.d_perm = by_dst.rowptr.data_ptr(), by_dst.col.data_ptr(), by_dst.perm.data_ptr()


def loss_outputs(tab, dev):
    """(stats [2, K] = mean loss | 1 / alive count, counts int32 [K, 5] = alive, tp, fp, fn, tn), wired into a forward table's entries."""
    stats = torch.empty((2, len(tab)), dtype=torch.float32, device=dev)
    counts = torch.empty((len(tab), 5), dtype=torch.int32, device=dev)
    for i in range(len(tab)):
        tab[i].loss, tab[i].inv_cnt, tab[i].counts = stats[0, i:].data_ptr(), stats[1, i:].data_ptr(), counts[i].data_ptr()
    return stats, counts


def offsets(sizes):
    """[0, n_0, n_0 + n_1, ...]: where each segment starts in the arrays that hold all segments one after the other."""
    return [0, *itertools.accumulate(int(n) for n in sizes)]


def fold_logit_grad(coef, scale, e_off, g_logits, ends):
    """A gradient arriving through the logits, folded into the per-edge coefficient: segment k of `coef` ([sum E] or [sum E, C]) times
    scale[k], plus g_logits[k] (or None) where ends[k] = (src, dst, limit) is alive (elsewhere the logits are constants); the scale -> 1."""
    parts = []
    for k, g in enumerate(g_logits):
        c = coef[e_off[k]:e_off[k + 1]] * scale[k]
        if g is not None:
            c = c + g.to(torch.float32) * alive_mask(*ends[k]).reshape((-1,) + (1,) * (c.dim() - 1))
        parts.append(c)
    return torch.cat(parts).contiguous(), torch.ones_like(scale)
