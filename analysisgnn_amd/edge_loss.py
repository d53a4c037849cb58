"""Edge-consistency term of the continual trainer (reference: models/analysis.py:805-836 `EdgeDecoder`, :857-867, :986-1019 in
`ContinualAnalysisGNN.common_step`): for every note-note relation the batch's edges — at most `batch_size` of them, drawn at
random — are classified "all five RNA labels agree at the two ends" from `embed_r(x[src]) * embed_r(x[dst])` through `fc` and a
label-smoothed two-class cross entropy; the term is the mean of the relations' losses, weighted by `lambda_edge` by the caller.

What the reference composes per relation from two `index_select`s, the `embed` chain on the gathered rows (twice), a multiply, the
`fc` chain and a cross entropy (about 20 launches per relation, backward through two `index_add_` with float atomics), around
boolean-mask compactions and a CPU `randperm` that read a size back per relation, is here, for ALL relations of the step:

* `edge_plan`: once per batch and outside any capture, everything with a host-side size — the random subset (keys from the
  library's random stream, `agnn_edge_select_keys`, and `torch.topk`: no read-back), the selected edge list and its CSRs by source
  and by destination (one `graph.build_csr` call).
* `embed_r` is row-wise up to its dropout: A_r = LN(ReLU(x W_r^T + b_r)) is computed once per NODE, one stacked `linear` and one
  `grouped_norm_act` for all relations; `agnn_edge_pair_fwd_f32` multiplies the two ends' rows, applies the two independent dropout
  masks per (edge, end, column) from the counter-based stream (backward regenerates them) and writes the edge labels.
* `linear` (`fc.0`), `norm_act` (`fc.1-3`), `agnn_edge_ce_fwd_f32` (`fc.4` and the objective, gradient coefficient included).
* backward: `agnn_edge_ce_bwd_f32`, the library's own backward of the two middle steps, `agnn_edge_pair_bwd_f32` (gather-reduce
  over the two CSRs: every row of dA written once, no atomics).

Departure from the reference, deliberate (the same as `pretrain.link_bce`): a relation WITHOUT an alive edge has loss 0 and zero
gradient — torch's cross entropy over nothing is NaN, which would poison the flat gradient buffer.  It still counts in the
division by the number of relations, and its alive count of 0 is returned (`parts["alive"]`).  What this objective shares with
`pretrain.link_bce` is `analysisgnn_amd/peredge.py` on the host (edge-list check, alive mask, CSRs by either end, loss outputs,
a gradient through the logits) and csrc/peredge.h on the device."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from . import _lib, fused, peredge
from .fused import grouped_norm_act, norm_act
from .graph import Csr, EdgeType, build_csr
from .heads import _cat_params, deepcopy_without_last
from .linear import linear

__all__ = ["EdgeDecoder", "EdgePlan", "edge_plan", "edge_consistency_loss", "RNA_KEYS", "SELECT_CALL_ID"]

RNA_KEYS = ("quality", "inversion", "degree1", "degree2", "localkey")          # models/analysis.py:988
SELECT_CALL_ID = 0xED6E5E1E      # call id of the subset draw: far from the dropout sites' running ids (fused._CALL_IDS counts from 1)
INT64_MAX = 2 ** 63 - 1


@dataclass
class EdgePlan:
    """The selected edges of a batch (device tensors; sizes are host integers).  Edges that are not alive — an end outside
    [0, limit), or left out by the draw — carry the ids (n_rows, n_rows): the CSR build leaves them out, the kernels skip them."""
    relations: List[str]          # relation names, in the order of the launch tables
    edge_types: List[EdgeType]    # the dict keys they came under
    src: torch.Tensor             # int64 [sum E_r]: the relations' lists one after the other
    dst: torch.Tensor
    e_off: List[int]              # [R + 1] offsets into src / dst
    n_rows: int                   # rows of the embedding the edges index
    limit: int                    # batch_size (<= n_rows)
    by_src: List[Csr] = field(default_factory=list)     # col = destination, perm = position in the relation's list
    by_dst: List[Csr] = field(default_factory=list)     # col = source

    @property
    def n_edges(self) -> int:
        return self.e_off[-1]

    def edges(self, r: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.src[self.e_off[r]:self.e_off[r + 1]], self.dst[self.e_off[r]:self.e_off[r + 1]]


def edge_plan(edge_index_dict: Dict[EdgeType, Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]], batch_size: int,
              n_rows: Optional[int] = None, select: bool = True, rng: Optional[torch.Tensor] = None, call_id: Optional[int] = None,
              relations: Optional[Sequence[str]] = None) -> EdgePlan:
    """The plan of a batch's edge term (models/analysis.py:991-997).  Of `edge_index_dict` every ("note", r, "note") relation is
    taken — with `relations` given (a decoder's `relations`), those of them it names, in ITS order.  An edge is alive when both
    ends are below `batch_size` (:991).  `select=True`: where a relation has more than `batch_size` alive edges a uniformly random
    `batch_size`-subset is kept (:993-997) — every alive edge gets a key whose high bits are its word of the library's random stream
    and whose low bits are its position, and `torch.topk` takes the `batch_size` smallest: no host read.  The subset is a pure
    function of `rng` (device int64[2] = (seed, step), default `fused.rng_state`), `call_id` and the relation's position; it does
    not depend on anything else.  `select=False` keeps every alive edge: for an already-selected dict (`EdgeDecoder.forward`).
    `n_rows`: rows of the embedding (default `batch_size`).  Eager: build it once per batch, before a capture."""
    bs = int(batch_size)
    n_rows = bs if n_rows is None else int(n_rows)
    if bs < 0 or n_rows < 0:
        raise _lib.AgnnError(f"edge_plan: batch_size={bs}, n_rows={n_rows} must not be negative")
    limit = min(bs, n_rows)
    found = {et[1]: et for et in edge_index_dict if isinstance(et, tuple) and len(et) == 3 and et[0] == "note" and et[2] == "note"}
    names = [r for r in relations if r in found] if relations is not None else list(found)
    if not names:
        raise _lib.AgnnError("edge_plan: no note-note relation to plan")
    if len(names) > _lib.MAX_SEG:
        raise _lib.AgnnError(f"edge_plan: {len(names)} relations, at most {_lib.MAX_SEG} per call")
    lists = [peredge.edge_index(edge_index_dict[found[r]], f"edge_plan: {r}") for r in names]
    dev = _lib.require_gpu(*[t for p in lists for t in p])
    drawn = [i for i, (s, _) in enumerate(lists) if select and s.numel() > bs]
    picks = {}
    if drawn:
        rng = fused.rng_state(dev) if rng is None else rng
        if rng.dtype != torch.int64 or rng.numel() != 2 or rng.device != dev:
            raise _lib.AgnnError("edge_plan: rng is a device int64[2] = (seed, step)")
        pos0 = peredge.offsets(s.numel() for s, _ in lists)
        k_off = peredge.offsets(lists[i][0].numel() for i in drawn)
        keys = torch.empty((k_off[-1],), dtype=torch.int64, device=dev)
        tab = (_lib.EdgeKeys * len(drawn))()
        for j, i in enumerate(drawn):
            s, d = lists[i]
            t = tab[j]
            t.src, t.dst, t.E, t.limit, t.pos0, t.key = s.data_ptr(), d.data_ptr(), int(s.numel()), limit, pos0[i], keys[k_off[j]:].data_ptr()
        _lib.check(_lib.load().agnn_edge_select_keys(len(drawn), tab, rng.data_ptr(), (SELECT_CALL_ID if call_id is None else int(call_id)) & 0xFFFFFFFF,
                                                     _lib.stream_ptr(dev)), "agnn_edge_select_keys")
        for j, i in enumerate(drawn):
            val, idx = torch.topk(keys[k_off[j]:k_off[j + 1]], bs, largest=False, sorted=True)
            picks[i] = (val, idx)
    srcs, dsts, oks = [], [], []
    for i, (s, d) in enumerate(lists):
        if i in picks:
            val, idx = picks[i]
            s, d = s[idx], d[idx]
            ok = val != INT64_MAX          # fewer than batch_size alive edges: the tail of the cut is not alive
        else:
            ok = peredge.alive_mask(s, d, limit)
        srcs.append(s)
        dsts.append(d)
        oks.append(ok)
    ok, e_off = torch.cat(oks), peredge.offsets(s.numel() for s in srcs)
    out = torch.full((1,), n_rows, dtype=torch.int64, device=dev)
    # "dropped" folded into the ids the CSR build sees (as postprocess does with row = n): out of range, so left out of every row
    src = torch.where(ok, torch.cat(srcs), out).contiguous()
    dst = torch.where(ok, torch.cat(dsts), out).contiguous()
    specs = []
    for r in range(len(names)):
        specs += peredge.end_specs(src[e_off[r]:e_off[r + 1]], dst[e_off[r]:e_off[r + 1]], n_rows)
    csrs = build_csr(specs)
    return EdgePlan(relations=names, edge_types=[found[r] for r in names], src=src, dst=dst, e_off=e_off, n_rows=n_rows, limit=limit,
                    by_src=csrs[0::2], by_dst=csrs[1::2])


class _EdgePair(torch.autograd.Function):
    """F [sum E, H] = dropout(A_r[src]) * dropout(A_r[dst]) of every relation of the plan, from the stacked A [n_rows, R H]; the
    edge labels (uint8 [sum E]) go to `info`."""

    @staticmethod
    def forward(ctx, plan: EdgePlan, info: dict, a, labels, p: float, call_id: int):
        dev = _lib.require_gpu(a)
        lib = _lib.load()
        a = _lib.rows16(a)
        R = len(plan.relations)
        H = int(a.shape[1]) // R
        E = plan.n_edges
        f = torch.empty((E, H), dtype=torch.float32, device=dev)
        label = torch.empty((E,), dtype=torch.uint8, device=dev)
        rng = fused.rng_state(dev) if p > 0 else None
        used = torch.empty(2, dtype=torch.int64, device=dev) if p > 0 else None
        tab = (_lib.EdgePair * R)()
        for r in range(R):
            t, lo, n = tab[r], plan.e_off[r], plan.e_off[r + 1] - plan.e_off[r]
            t.a, t.ld_a, t.n = (a.data_ptr() + 4 * r * H if a.numel() else None), max(a.stride(0), R * H), plan.n_rows
            t.src, t.dst = (plan.src[lo:].data_ptr(), plan.dst[lo:].data_ptr()) if n else (None, None)
            t.E, t.limit, t.pos0 = n, plan.limit, lo
            t.f, t.ld_f, t.label = (f[lo:].data_ptr(), H, label[lo:].data_ptr()) if n else (None, H, None)
        K = int(labels.shape[0]) if labels is not None else 0
        _lib.check(lib.agnn_edge_pair_fwd_f32(R, tab, H, _lib.ptr(labels), K, labels.stride(0) if K else 0, float(p), _lib.ptr(rng),
                                              int(call_id), _lib.ptr(used), _lib.stream_ptr(dev)), "agnn_edge_pair_fwd_f32")
        ctx.plan, ctx.cfg = plan, (H, float(p), int(call_id))
        ctx.save_for_backward(a, *([used] if used is not None else []))
        info["edge_labels"] = label
        return f

    @staticmethod
    def backward(ctx, df):
        a, *used = ctx.saved_tensors
        plan = ctx.plan
        H, p, call_id = ctx.cfg
        dev = a.device
        R = len(plan.relations)
        df = _lib.rows16(df)
        da = torch.empty((plan.n_rows, R * H), dtype=torch.float32, device=dev)
        tab = (_lib.EdgePairBwd * R)()
        for r in range(R):
            t, lo, n = tab[r], plan.e_off[r], plan.e_off[r + 1] - plan.e_off[r]
            t.a, t.ld_a, t.n = (a.data_ptr() + 4 * r * H if a.numel() else None), max(a.stride(0), R * H), plan.n_rows
            t.df, t.ld_df = (df[lo:].data_ptr() if n else None), max(df.stride(0), H)
            t.E, t.limit, t.pos0 = n, plan.limit, lo
            peredge.fill_csr(t, plan.by_src[r], plan.by_dst[r])
            t.da, t.ld_da = (da.data_ptr() + 4 * r * H if da.numel() else None), R * H
        _lib.check(_lib.load().agnn_edge_pair_bwd_f32(R, tab, H, p, _lib.ptr(used[0]) if used else None, call_id, _lib.stream_ptr(dev)),
                   "agnn_edge_pair_bwd_f32")
        return None, None, da, None, None, None


class _EdgeCE(torch.autograd.Function):
    """(total, logits [sum E, 2]) of `fc.4` and the label-smoothed cross entropy over the plan's relations; differentiable in y,
    w4 and b4 through the total and through the logits."""

    @staticmethod
    def forward(ctx, plan: EdgePlan, info: dict, smoothing: float, y, w4, b4):
        dev = _lib.require_gpu(y, w4, b4)
        lib = _lib.load()
        y, w4, b4 = _lib.rows16(y), _lib.vec16(w4), _lib.vec16(b4)
        R, E, H = len(plan.relations), plan.n_edges, int(y.shape[1])
        label = info["edge_labels"]
        logit = torch.empty((E, 2), dtype=torch.float32, device=dev)
        dlogit = torch.empty((E, 2), dtype=torch.float32, device=dev)
        total = torch.empty((), dtype=torch.float32, device=dev)
        tab = (_lib.EdgeCe * R)()
        stats, counts = peredge.loss_outputs(tab, dev)
        for r in range(R):
            t, lo, n = tab[r], plan.e_off[r], plan.e_off[r + 1] - plan.e_off[r]
            t.y, t.ld_y = (y[lo:].data_ptr() if n else None), max(y.stride(0), H)
            t.src, t.dst, t.label = (plan.src[lo:].data_ptr(), plan.dst[lo:].data_ptr(), label[lo:].data_ptr()) if n else (None, None, None)
            t.E, t.limit = n, plan.limit
            t.logit, t.dlogit = (logit[lo:].data_ptr(), dlogit[lo:].data_ptr()) if n else (None, None)
        nws = int(lib.agnn_edge_ce_workspace_bytes(R, tab))
        ws = torch.empty((max(nws, 4),), dtype=torch.uint8, device=dev)
        _lib.check(lib.agnn_edge_ce_fwd_f32(R, tab, H, w4.data_ptr(), b4.data_ptr(), float(smoothing), total.data_ptr(), ws.data_ptr(), nws,
                                            _lib.stream_ptr(dev)), "agnn_edge_ce_fwd_f32")
        ctx.plan, ctx.H = plan, H
        ctx.save_for_backward(y, w4, dlogit, stats)
        ctx.set_materialize_grads(False)
        info.update(losses=stats[0], inv_cnt=stats[1], counts=counts, dlogit=dlogit)
        return total, logit

    @staticmethod
    def backward(ctx, g_total, g_logit):
        y, w4, dlogit, stats = ctx.saved_tensors
        plan, H = ctx.plan, ctx.H
        if g_total is None and g_logit is None:
            return (None,) * 6
        dev = y.device
        lib = _lib.load()
        R, E = len(plan.relations), plan.n_edges
        scale = (g_total.to(torch.float32) * stats[1] / R).contiguous() if g_total is not None else torch.zeros(R, dtype=torch.float32, device=dev)
        if g_logit is not None:
            ends = [plan.edges(r) + (plan.limit,) for r in range(R)]
            dlogit, scale = peredge.fold_logit_grad(dlogit, scale, plan.e_off, g_logit.split([s.numel() for s, _, _ in ends]), ends)
        dy = torch.empty((E, H), dtype=torch.float32, device=dev)
        dw4 = torch.empty((2, H), dtype=torch.float32, device=dev)
        db4 = torch.empty((2,), dtype=torch.float32, device=dev)
        tab = (_lib.EdgeCeBwd * R)()
        for r in range(R):
            t, lo, n = tab[r], plan.e_off[r], plan.e_off[r + 1] - plan.e_off[r]
            t.y, t.ld_y = (y[lo:].data_ptr() if n else None), max(y.stride(0), H)
            t.dlogit, t.E = (dlogit[lo:].data_ptr() if n else None), n
            t.dy, t.ld_dy = (dy[lo:].data_ptr() if n else None), H
        nws = int(lib.agnn_edge_ce_bwd_workspace_bytes(R, tab, H))
        ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=dev)
        _lib.check(lib.agnn_edge_ce_bwd_f32(R, tab, H, w4.data_ptr(), scale.data_ptr(), dw4.data_ptr(), db4.data_ptr(), ws.data_ptr(), nws,
                                            _lib.stream_ptr(dev)), "agnn_edge_ce_bwd_f32")
        return None, None, None, dy, dw4, db4


class EdgeDecoder(nn.Module):
    """The reference's `EdgeDecoder` (models/analysis.py:805-836): same constructor, same `state_dict` keys
    (`embed.<rel>.{0,2}.{weight,bias}`, `fc.{0,2,4}.{weight,bias}`), same `forward(edge_dict, x) -> {edge_type: logits [E, 2]}`.
    Schedule (module docstring): one stacked `linear` for the relations' `embed.*.0`, one `grouped_norm_act` over the [B, R, H]
    view, the pair kernel (dropout inside), `linear` for `fc.0`, `norm_act` for `fc.1-3`, the cross-entropy kernel for `fc.4`.
    `last` keeps the call's losses, edge labels, counts and logits."""

    def __init__(self, channels, edge_types, dropout=0.5):
        super().__init__()
        self.embed = nn.ModuleDict()
        for edge_type in edge_types:
            self.embed[edge_type] = nn.Sequential(nn.Linear(channels, channels), nn.ReLU(), nn.LayerNorm(channels), nn.Dropout(dropout))
        self.fc = nn.Sequential(nn.Linear(channels, channels), nn.ReLU(), nn.LayerNorm(channels), nn.Dropout(dropout), nn.Linear(channels, 2))
        self.last: dict = {}

    __deepcopy__ = deepcopy_without_last

    @property
    def relations(self) -> List[str]:
        return list(self.embed.keys())

    def node_features(self, x: torch.Tensor, relations: Sequence[str]) -> torch.Tensor:
        """A [B, R H]: LN(ReLU(x W_r^T + b_r)) of the named relations side by side — `embed_r` without its dropout, per node."""
        mods = [self.embed[r] for r in relations]
        R, H = len(mods), mods[0][0].out_features
        W1 = _cat_params([m[0].weight for m in mods])                          # [R H, H]
        b1 = _cat_params([m[0].bias for m in mods])
        a = linear(x, W1, b1)                                                  # [B, R H]
        gl = H // 4
        if 256 % H == 0 and (gl & (gl - 1)) == 0 and R * H <= 2048 and fused.ENABLED:
            gamma = _cat_params([m[2].weight for m in mods], stack=True)       # [R, H]
            beta = _cat_params([m[2].bias for m in mods], stack=True)
            return grouped_norm_act(a.view(-1, R, H), gamma, beta, mods[0][2].eps, pre_relu=True).reshape(-1, R * H)
        # a width the segmented LayerNorm does not take: one launch per relation
        return torch.cat([norm_act(a[:, r * H:(r + 1) * H], m[2], pre_relu=True) for r, m in enumerate(mods)], dim=1)

    def decode(self, x: torch.Tensor, plan: EdgePlan, labels: Optional[torch.Tensor] = None, label_smoothing: float = 0.1):
        """(total, logits [sum E, 2]) over the plan's relations from an embedding x [n_rows, H]; fills `last`.  Without `labels`
        every edge label is 0 (logits only: `last["loss"]` then stands for all-zero labels)."""
        dev = _lib.require_gpu(x)
        for r, et in zip(plan.relations, plan.edge_types):
            if r not in self.embed:
                raise ValueError(f"Edge type {et} not found in embed dictionary.")
        H = self.fc[0].in_features
        if x.dim() != 2 or x.shape[1] != H or x.shape[0] != plan.n_rows or x.dtype != torch.float32:
            raise _lib.AgnnError(f"EdgeDecoder: x {tuple(x.shape)} {x.dtype} for a plan over {plan.n_rows} rows, fp32 H={H}")
        if H % 4 != 0 or not 4 <= H <= 512:
            raise _lib.AgnnError(f"EdgeDecoder: channels={H} must be a multiple of 4 in [4, 512] (csrc/edgedec.hip)")
        if labels is not None:
            if labels.dim() != 2 or labels.dtype != torch.int64 or labels.shape[1] < plan.limit or labels.stride(1) != 1:
                raise _lib.AgnnError(f"EdgeDecoder: labels are int64 [K, >= {plan.limit}], got {labels.dtype} {tuple(labels.shape)}")
            _lib.require_gpu(x, labels)
        info: dict = {}
        R = len(plan.relations)
        if plan.n_edges == 0:
            # nothing to score: the term and every gradient are zero (no launch takes an empty matrix)
            total = x[:0].sum()
            logit = torch.zeros((0, 2), dtype=torch.float32, device=dev)
            info.update(edge_labels=torch.zeros((0,), dtype=torch.uint8, device=dev), losses=torch.zeros(R, device=dev),
                        inv_cnt=torch.zeros(R, device=dev), counts=torch.zeros((R, 5), dtype=torch.int32, device=dev))
        else:
            p0 = float(self.embed[plan.relations[0]][3].p) if self.training else 0.0
            a = self.node_features(x, plan.relations)
            f = _EdgePair.apply(plan, info, a, labels, p0, next(fused._CALL_IDS) & 0xFFFFFFFF)
            h = linear(f, self.fc[0].weight, self.fc[0].bias)
            y = norm_act(h, self.fc[2], pre_relu=True, p=float(self.fc[3].p), training=self.training)
            total, logit = _EdgeCE.apply(plan, info, float(label_smoothing), y, self.fc[4].weight, self.fc[4].bias)
        off = plan.e_off
        self.last = dict(info, loss=total, logits=[logit[off[r]:off[r + 1]] for r in range(R)],
                         labels=[info["edge_labels"][off[r]:off[r + 1]] for r in range(R)], plan=plan)
        return total, logit

    def forward(self, edge_dict, x):
        for edge_type in edge_dict:
            if edge_type[1] not in self.embed:
                raise ValueError(f"Edge type {edge_type} not found in embed dictionary.")
        if not edge_dict:
            return {}
        n = int(x.shape[0])
        plan = edge_plan(dict(edge_dict), n, n, select=False)
        _, logit = self.decode(x, plan)
        return {et: logit[plan.e_off[r]:plan.e_off[r + 1]] for r, et in enumerate(plan.edge_types)}


def edge_consistency_loss(decoder: EdgeDecoder, x: torch.Tensor, plan: EdgePlan,
                          labels: Union[torch.Tensor, Dict[str, torch.Tensor]], label_smoothing: float = 0.1):
    """The edge term of `common_step` (:986-1019) -> (loss, parts): `loss` is the 0-dim mean over the plan's relations of the
    label-smoothed cross entropy between `decoder`'s edge logits and "all label rows agree at the two ends" (equal -1s count as
    equal, as the reference's `==`), to be multiplied by `lambda_edge` by the caller; `parts` = {"relations": names, "losses": [R]
    per-relation means, "alive": int32 [R] alive edge counts}.  `labels`: int64 [K, >= batch_size], or the trainer's label dict
    (its five `RNA_KEYS` are stacked).  A relation without an alive edge has loss 0 and zero gradient (torch: NaN) and still
    counts in the division by R — see the module docstring.  With the plan built beforehand nothing is read back: the call
    can be captured (the rule of `resident.py`: what it needs on the device must exist before the capture)."""
    if isinstance(labels, dict):
        missing = [k for k in RNA_KEYS if k not in labels]
        if missing:
            raise _lib.AgnnError(f"edge_consistency_loss: labels {missing} missing (the reference skips the term then, :989)")
        labels = torch.stack([labels[k].long() for k in RNA_KEYS])
    total, _ = decoder.decode(x, plan, labels, label_smoothing)
    last = decoder.last
    return total, {"relations": list(plan.relations), "losses": last["losses"], "alive": last["counts"][:, 0]}
