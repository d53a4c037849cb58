"""Self-supervised pretraining stage (reference: models/analysis.py:360-406 `PreEncoder`, :697-744 `PreEncoderPL._common_step`):
a `HybridHGT` encoder, four `Linear -> ReLU -> LayerNorm -> Linear` heads, two link-prediction tasks (staff, voice) scored as
the dot product of the endpoint rows of every candidate edge and trained with `BCEWithLogitsLoss` against membership in the true
staff / voice relations, and two label-smoothed cross entropies (key signature, pitch spelling), on the kernels of
csrc/linkpred.hip and the library's head / cross-entropy kernels.

What the reference composes per link task from `index_select` x 2, multiply, sum, BCE and — backward — two `index_add_` with
float atomics, around boolean-mask compactions, `torch.isin` over Cantor-paired keys and an `argsort` that each read a size back
to the host, is here one forward call and one backward call for BOTH tasks:

* `link_plan` builds, once per batch and outside any capture, everything with a host-side size: the candidate list's CSR by source
  and by destination and the true relation's CSR by source (`graph.build_csr`).
* `link_bce(plans, feats)` = `agnn_link_bce_fwd_f32` / `agnn_link_bce_bwd_f32`: no host read, capturable (the rule of
  `resident.py`).  Pair membership replaces the Cantor keys (the pairing is one-to-one on non-negative integers, so the two agree);
  `alive = (s < limit) & (d < limit)` replaces the compactions (a true edge can only match a surviving candidate when both its
  ends are below the limit too, so the true relation needs no filter of its own).

Departures from the reference, both deliberate:

* A task WITHOUT an alive candidate has loss 0, `inv_cnt` 0 and zero gradient.  The reference's `BCEWithLogitsLoss` over nothing is
  NaN, and its step is skipped (`if torch.isnan(total_loss): return`, :732); a NaN here would poison the flat gradient buffer, so
  the alive counts are returned (`info["counts"][:, 0]`) and skipping is the caller's decision.
* The `argsort` of the staff candidates by source (:707) is not reproduced: the objective is a mean over the candidates and does
  not depend on their order.  Logits and labels come back in the order of `cat(onset, consecutive)`.

Out of scope: `FAMO` (the reference's own call `FAMO(n_tasks=4, ...)` does not match its constructor, SURVEY A.7: the effective
objective is the plain sum built here), the Lightning optimizer plumbing.  (`EdgeDecoder` is `analysisgnn_amd/edge_loss.py`; what
the two per-edge objectives share lives in `analysisgnn_amd/peredge.py` on the host and csrc/peredge.h on the device.)"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib, heads, peredge
from .fused import grouped_norm_act
from .graph import Csr, EdgeType, SegSpec, build_csr
from .heads import _cat_params, deepcopy_without_last, grouped_projection, multitask_cross_entropy
from .hgt import HybridHGT
from .linear import linear
from .metrics import MultiTaskMetrics

__all__ = ["LinkPlan", "link_plan", "link_plans", "link_bce", "link_candidates", "PreEncoder", "pretrain_objective", "PretrainMetrics",
           "STAFF", "VOICE", "ONSET", "CONSECUTIVE", "FIFTHS_CLASSES", "SPELLING_CLASSES"]

ONSET: EdgeType = ("note", "onset", "note")
CONSECUTIVE: EdgeType = ("note", "consecutive", "note")
STAFF: EdgeType = ("note", "staff", "note")
VOICE: EdgeType = ("note", "voice", "note")
FIFTHS_CLASSES, SPELLING_CLASSES = 15, 35
CLS_OFFS = (0, FIFTHS_CLASSES, FIFTHS_CLASSES + SPELLING_CLASSES)


@dataclass
class LinkPlan:
    """One link task's index structures (device tensors; sizes are host integers known at collation time)."""
    cand: torch.Tensor            # int64 [2, E], contiguous: the candidates as they arrived
    n_rows: int                   # rows of the feature matrix the task scores
    limit: int                    # candidates with an end >= limit are not alive (<= n_rows)
    by_src: Csr                   # candidates by source: col = destination, perm = candidate position
    by_dst: Csr                   # candidates by destination: col = source
    true: Csr                     # the true relation by source
    keep: list = field(default_factory=list, repr=False)

    @property
    def n_edges(self) -> int:
        return int(self.cand.shape[1])


def link_plans(tasks: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]], n_rows: int, limit: Optional[int] = None) -> List[LinkPlan]:
    """Plans of several link tasks over feature matrices of `n_rows` rows, their 3 CSRs each in ONE `agnn_csr_build` call.
    `tasks`: (candidates int64 [2, E], true edges int64 [2, E_true] or None) per task.  Candidate ends outside [0, n_rows) never
    reach a row (the CSR build leaves such rows out, the kernels skip such columns).  Eager: call it before a capture."""
    n_rows = int(n_rows)
    limit = n_rows if limit is None else int(limit)
    if n_rows < 0 or not 0 <= limit <= n_rows:
        raise _lib.AgnnError(f"link_plan: limit={limit} must lie in [0, n_rows={n_rows}]")
    if not tasks:
        return []
    dev = _lib.require_gpu(*[t[0] for t in tasks])
    specs, cands = [], []
    for cand, true in tasks:
        cand = peredge.edge_index(cand, "link_plan: candidates", dev)
        true = peredge.edge_index(true, "link_plan: true edges", dev)
        _lib.require_gpu(cand, true)
        cands.append((cand, true))
        specs += peredge.end_specs(cand[0], cand[1], n_rows) + [SegSpec(row=true[0], col=true[1], n_rows=n_rows)]
    csrs = build_csr(specs)
    return [LinkPlan(cand=c, n_rows=n_rows, limit=limit, by_src=csrs[3 * i], by_dst=csrs[3 * i + 1], true=csrs[3 * i + 2], keep=[t])
            for i, (c, t) in enumerate(cands)]


def link_plan(candidates: torch.Tensor, true_edges: Optional[torch.Tensor], n_rows: int, limit: Optional[int] = None) -> LinkPlan:
    """`link_plans` for one task."""
    return link_plans([(candidates, true_edges)], n_rows, limit)[0]


class _LinkBCE(torch.autograd.Function):
    """(loss [K], logits of task 0, ..., logits of task K - 1) of K link tasks; differentiable in the feature matrices through
    the losses and through the logits."""

    @staticmethod
    def forward(ctx, plans, info, *feats):
        K = len(plans)
        dev = _lib.require_gpu(*feats)
        lib = _lib.load()
        feats = [_lib.rows16(z) for z in feats]
        H = int(feats[0].shape[1])
        for p, z in zip(plans, feats):
            if z.shape[1] != H or z.shape[0] != p.n_rows:
                raise _lib.AgnnError(f"link_bce: features {tuple(z.shape)} for a plan over {p.n_rows} rows (one width H={H} per call)")
        e_off = peredge.offsets(p.n_edges for p in plans)
        logit = torch.empty((e_off[-1],), dtype=torch.float32, device=dev)
        label = torch.empty((e_off[-1],), dtype=torch.uint8, device=dev)
        g = torch.empty((e_off[-1],), dtype=torch.float32, device=dev)
        tab = (_lib.LinkTask * K)()
        stats, counts = peredge.loss_outputs(tab, dev)
        for i, (p, z) in enumerate(zip(plans, feats)):
            t, E, lo = tab[i], p.n_edges, e_off[i]
            t.z, t.ld_z, t.n = (z.data_ptr() if z.numel() else None), z.stride(0) if z.shape[0] > 1 else max(z.stride(0), H), p.n_rows
            t.src, t.dst = (p.cand[0].data_ptr(), p.cand[1].data_ptr()) if E else (None, None)
            t.E, t.limit = E, p.limit
            t.t_rowptr, t.t_col = p.true.rowptr.data_ptr(), p.true.col.data_ptr()
            t.logit, t.label, t.g = (logit[lo:].data_ptr(), label[lo:].data_ptr(), g[lo:].data_ptr()) if E else (None, None, None)
        nws = int(lib.agnn_link_bce_workspace_bytes(K, tab))
        ws = torch.empty((max(nws, 4),), dtype=torch.uint8, device=dev)
        _lib.check(lib.agnn_link_bce_fwd_f32(K, tab, H, ws.data_ptr(), nws, _lib.stream_ptr(dev)), "agnn_link_bce_fwd_f32")
        ctx.plans, ctx.e_off, ctx.H = plans, e_off, H
        ctx.save_for_backward(g, stats, *feats)
        ctx.set_materialize_grads(False)
        logits = tuple(logit[e_off[i]:e_off[i + 1]] for i in range(K))
        if info is not None:
            info.update(logits=list(logits), labels=[label[e_off[i]:e_off[i + 1]] for i in range(K)],
                        g=[g[e_off[i]:e_off[i + 1]] for i in range(K)], counts=counts, inv_cnt=stats[1], loss=stats[0])
        return (stats[0],) + logits

    @staticmethod
    def backward(ctx, g_loss, *g_logits):
        g, stats, *feats = ctx.saved_tensors
        plans, e_off, H = ctx.plans, ctx.e_off, ctx.H
        K = len(plans)
        dev = g.device
        if g_loss is None and all(t is None for t in g_logits):
            return (None, None) + (None,) * K
        scale = (g_loss.to(torch.float32) * stats[1]).contiguous() if g_loss is not None else torch.zeros(K, dtype=torch.float32, device=dev)
        if any(t is not None for t in g_logits):
            g, scale = peredge.fold_logit_grad(g, scale, e_off, g_logits, [(p.cand[0], p.cand[1], p.limit) for p in plans])
        dzs = [torch.empty((p.n_rows, H), dtype=torch.float32, device=dev) for p in plans]
        tab = (_lib.LinkBwd * K)()
        for i, (p, z, dz) in enumerate(zip(plans, feats, dzs)):
            t, E = tab[i], p.n_edges
            t.z, t.ld_z, t.n = (z.data_ptr() if z.numel() else None), z.stride(0) if z.shape[0] > 1 else max(z.stride(0), H), p.n_rows
            t.g, t.E = (g[e_off[i]:].data_ptr() if E else None), E
            peredge.fill_csr(t, p.by_src, p.by_dst)
            t.dz, t.ld_dz = (dz.data_ptr() if dz.numel() else None), H
        _lib.check(_lib.load().agnn_link_bce_bwd_f32(K, tab, H, scale.data_ptr(), _lib.stream_ptr(dev)), "agnn_link_bce_bwd_f32")
        return (None, None) + tuple(dzs)


def link_bce(plans: Sequence[LinkPlan], feats: Sequence[torch.Tensor], info: Optional[dict] = None) -> torch.Tensor:
    """Mean `BCEWithLogitsLoss` [K] of K link tasks in one launch pair: task k scores the candidates of `plans[k]` on the rows of
    `feats[k]` ([n_rows, H] fp32, one H for all).  Differentiable in `feats`.  `info` (a dict, filled when given) keeps what the
    forward wrote: `logits` (list of [E_k] fp32 views, differentiable as well; 0 where not alive), `labels` (uint8 [E_k]), `g`
    (sigmoid(logit) - label, 0 where not alive), `counts` int32 [K, 5] = alive, tp, fp, fn, tn with "positive" = logit > 0,
    `inv_cnt` [K].  A task without an alive candidate has loss 0 and zero gradient (torch: NaN) — see the module docstring.
    With the plans built beforehand neither direction reads anything back: the call can be captured."""
    plans, feats = list(plans), list(feats)
    if len(plans) != len(feats) or not plans:
        raise _lib.AgnnError(f"link_bce: {len(plans)} plans for {len(feats)} feature matrices (at least one task)")
    if len(plans) > _lib.MAX_SEG:
        raise _lib.AgnnError(f"link_bce: {len(plans)} tasks, at most {_lib.MAX_SEG} per call")
    for z in feats:
        if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.dtype != torch.float32 or z.shape[1] % 4 != 0 or z.shape[1] < 4:
            raise _lib.AgnnError("link_bce: feature matrices are fp32 [n, H] with H a positive multiple of 4")
    own = {} if info is None else info
    out = _LinkBCE.apply(plans, own, *feats)
    own["logits"] = list(out[1:])                                 # the differentiable ones
    return out[0]


def link_candidates(edge_index_dict: Dict[EdgeType, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(staff candidates, voice candidates) of a batch (models/analysis.py:704-708): staff = cat(onset, consecutive), voice =
    consecutive.  The reference then sorts the staff candidates by source (:707); the objective does not depend on candidate
    order, so the sort (and its launch) is left out."""
    cons = edge_index_dict[CONSECUTIVE]
    return torch.cat((edge_index_dict[ONSET], cons), dim=1), cons


def _head(h: int, out: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.LayerNorm(h), nn.Linear(h, out))


class PreEncoder(nn.Module):
    """The reference's `PreEncoder`: same constructor (`jk` is our `HybridHGT(use_jk=)`), same forward signature and return
    tuple (`return_embedding` included), same `state_dict` keys (`encoder.*`, `staff_clf.{0,2,3}.*`, `voice_clf.*`,
    `fifths_clf.*`, `spelling_clf.*`).  Schedule: the four heads' first layers are ONE stacked GEMM, ReLU + LayerNorm one
    `grouped_norm_act` launch over the [B, 4, H] view; the two H-wide second layers are plain `linear`s, the 15- and 35-wide ones
    one `grouped_projection` where H is one of its widths (two `linear`s otherwise) — not a block-diagonal GEMM over all four,
    which would do about 4x the useful work.  The link logits come from `link_bce` (candidates with an end outside the encoder's
    `batch_size` rows score 0); `last` keeps the call's link losses, labels, counts and the side-by-side class logits."""

    def __init__(self, metadata, in_channels, out_channels, num_layers, heads, dropout=0.5, jk=True):
        super().__init__()
        self.encoder = HybridHGT(metadata, in_channels, out_channels, num_layers, heads=heads, dropout=dropout, use_jk=jk)
        self.pitch_spelling_classes = SPELLING_CLASSES
        self.fifths_classes = FIFTHS_CLASSES
        self.staff_clf = _head(out_channels, out_channels)
        self.voice_clf = _head(out_channels, out_channels)
        self.fifths_clf = _head(out_channels, self.fifths_classes)
        self.spelling_clf = _head(out_channels, self.pitch_spelling_classes)
        self.last: dict = {}

    __deepcopy__ = deepcopy_without_last

    def head_features(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(staff_x [B, H], voice_x [B, H], class logits [B, 15 + 35] side by side) of an embedding x [B, H]."""
        mods = [self.staff_clf, self.voice_clf, self.fifths_clf, self.spelling_clf]
        H = mods[0][0].out_features
        W1 = _cat_params([m[0].weight for m in mods])                          # [4H, H]
        b1 = _cat_params([m[0].bias for m in mods])
        gamma = _cat_params([m[2].weight for m in mods], stack=True)           # [4, H]
        beta = _cat_params([m[2].bias for m in mods], stack=True)
        a = linear(x, W1, b1)                                                  # [B, 4H]
        a = grouped_norm_act(a.view(-1, 4, H), gamma, beta, mods[0][2].eps, pre_relu=True).reshape(-1, 4 * H)
        staff_x = linear(a[:, :H], mods[0][3].weight, mods[0][3].bias)
        voice_x = linear(a[:, H:2 * H], mods[1][3].weight, mods[1][3].bias)
        if a.is_cuda and H in heads.GPROJ_K and heads.GPROJ_ENABLED:
            W2 = _cat_params([mods[2][3].weight, mods[3][3].weight])           # [50, H]
            b2 = _cat_params([mods[2][3].bias, mods[3][3].bias])
            cls = grouped_projection(a[:, 2 * H:], W2, b2, CLS_OFFS, H)
        else:
            cls = torch.cat([linear(a[:, 2 * H:3 * H], mods[2][3].weight, mods[2][3].bias),
                             linear(a[:, 3 * H:], mods[3][3].weight, mods[3][3].bias)], dim=1)
        return staff_x, voice_x, cls

    def decode(self, x: torch.Tensor, staff_candidate_edges=None, voice_candidate_edges=None, plans: Optional[Sequence[LinkPlan]] = None):
        """Everything behind the encoder, from an embedding x [B, H]: (staff_logits, voice_logits, fifths_logits,
        spelling_logits).  `plans` = (staff plan, voice plan) built with the true relations (`link_plans`); without them the
        candidates are scored against an empty true relation (logits only: `last["link_loss"]` then stands for all-zero labels)."""
        _lib.require_gpu(x)
        staff_x, voice_x, cls = self.head_features(x)
        if plans is None:
            plans = link_plans([(staff_candidate_edges, None), (voice_candidate_edges, None)], int(x.shape[0]))
        info: dict = {}
        loss = link_bce(plans, [staff_x, voice_x], info)
        self.last = dict(info, link_loss=loss, cls_logits=cls, plans=list(plans))
        return info["logits"][0], info["logits"][1], cls[:, :CLS_OFFS[1]], cls[:, CLS_OFFS[1]:CLS_OFFS[2]]

    def forward(self, x_dict, edge_index_dict, batch_dict, batch_size, neighbor_mask_node, neighbor_mask_edge, staff_candidate_edges,
                voice_candidate_edges, return_embedding=False, plans: Optional[Sequence[LinkPlan]] = None):
        x = self.encoder(x_dict, edge_index_dict, batch_dict, batch_size, neighbor_mask_node, neighbor_mask_edge)
        out = self.decode(x, staff_candidate_edges, voice_candidate_edges, plans)
        return out + (x,) if return_embedding else out


def pretrain_objective(model: PreEncoder, x_dict, edge_index_dict, batch_dict, batch_size: int, neighbor_mask_node, neighbor_mask_edge,
                       key_signature: torch.Tensor, pitch_spelling: torch.Tensor, label_smoothing: float = 0.1):
    """`PreEncoderPL._common_step` (:697-731) -> (total, parts): total = staff + voice + fifths + spelling, parts = {"staff",
    "voice", "fifths", "spelling"} (0-dim tensors of the same graph) plus "alive" (int32 [2]: the link tasks' alive candidate
    counts — 0 means the reference would have skipped the step, see the module docstring).  The caller's `edge_index_dict` is
    not mutated (the reference pops from it): the encoder gets a copy without the `staff` and `voice` relations.  Both link
    plans are built here with limit = batch_size; the cross entropies run through `multitask_cross_entropy` on the side-by-side
    [B, 15 + 35] logits (label smoothing 0.1, ignore index -1: no label hits it).  `model.last` keeps logits, labels and
    counts for `PretrainMetrics`."""
    bs = int(batch_size)
    seen = {et: ei for et, ei in edge_index_dict.items() if et not in (STAFF, VOICE)}
    staff_c, voice_c = link_candidates(edge_index_dict)
    plans = link_plans([(staff_c, edge_index_dict[STAFF]), (voice_c, edge_index_dict[VOICE])], bs, bs)
    model(x_dict, seen, batch_dict, bs, neighbor_mask_node, neighbor_mask_edge, staff_c, voice_c, plans=plans)
    last = model.last
    labels = torch.stack([key_signature[:bs].long(), pitch_spelling[:bs].long()])
    ce = multitask_cross_entropy(last["cls_logits"], CLS_OFFS, labels, label_smoothing, -1)
    link = last["link_loss"]
    last["cls_labels"] = labels
    parts = {"staff": link[0], "voice": link[1], "fifths": ce[0], "spelling": ce[1]}
    total = link[0] + link[1] + ce[0] + ce[1]
    parts["alive"] = last["counts"][:, 0]
    return total, parts


class PretrainMetrics:
    """Validation metrics of `_common_step` (:739-743): binary F1 of the staff and voice link tasks, 2 tp / (2 tp + fp + fn) (0
    when that is empty), from the confusion counts `agnn_link_bce_fwd_f32` wrote — "positive" = logit > 0, i.e. sigmoid > 0.5 —
    and the accuracies of key signature and pitch spelling from `MultiTaskMetrics`.  Counters accumulate on the device over the
    epoch; `compute()` is the only device -> host copy.  One torchmetrics quirk is NOT reproduced: given inputs that all happen to
    lie in [0, 1], torchmetrics' binary F1 takes them for probabilities and thresholds at 0.5 instead of applying the sigmoid;
    here a logit is always a logit."""

    def __init__(self, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.AgnnError(f"PretrainMetrics needs a HIP device (no CPU fallback), got {self.device}")
        self.link = torch.zeros((2, 5), dtype=torch.int64, device=self.device)          # alive, tp, fp, fn, tn per link task
        self.cls = MultiTaskMetrics(["fifths", "spelling"], list(CLS_OFFS), gate_task=None, joint=None, device=self.device)

    @torch.no_grad()
    def update(self, last: dict) -> None:
        """Add one batch: `model.last` after `pretrain_objective` (its `counts`, `cls_logits`, `cls_labels`)."""
        self.link += last["counts"]
        self.cls.update(last["cls_logits"].detach(), last["cls_labels"])

    @torch.no_grad()
    def reset(self) -> None:
        self.link.zero_()
        self.cls.reset()

    def compute(self) -> Dict[str, float]:
        c = self.link.cpu().tolist()
        out = {}
        for name, (_, tp, fp, fn, _tn) in zip(("staff_f1", "voice_f1"), c):
            den = 2 * tp + fp + fn
            out[name] = 2 * tp / den if den > 0 else 0.0
        acc = self.cls.compute()["acc"]
        out["fifths_acc"], out["spelling_acc"] = acc["fifths"], acc["spelling"]
        return out
