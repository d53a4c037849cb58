"""Validation and test metrics of the task heads (`ContinualAnalysisGNN.validation_step` / `test_step`,
analysisgnn/models/analysis.py:1097-1164, :1184-1282): per task `Accuracy(task="multiclass")` and `F1Score(average="macro")`
(:890-891), the same accuracies on the notes predicted as chord tones (`NCT_*`), and the joint Roman-numeral accuracies
`total_rna_acc`, `RN(NCT)` and `RN(Onset)`.

Composed from torch ops that is, per validation batch, about 21 x (argmax, eq, sum, three bincounts, boolean indexing with a
host sync).  Here the logits already lie side by side in one [N, sum C] matrix (`forward_clf_fused`) and the labels as int64
[T, N] with -1 for ignored rows (what `heads.multitask_cross_entropy` reads), so everything above is ONE launch of
`agnn_multitask_eval_f32` per batch: a segmented argmax per row and integer counters that accumulate on the device over the
epoch.  Integer sums do not depend on order: the figures are bitwise reproducible.  `compute()` is the only device -> host copy.
INTEGRATION.md has the validation / test step recipe."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

from . import _lib, ops
from .continual import _segment_tensors, _segments
from .graph import SegSpec, build_csr
from .heads import _check_labels
from .postprocess import RNA_KEYS

__all__ = ["multitask_argmax", "MultiTaskMetrics", "metrics_from_counts", "onset_rna_accuracy"]

JOINT_KEYS = ("quality", "inversion", "degree1", "degree2", "localkey")      # models/analysis.py:1154, :1273


def _logits_arg(logits: torch.Tensor, n_cols: int):
    """(tensor kept alive, leading dimension) of fp32 logits with unit column stride; column-slice views pass as they are."""
    if logits.dim() != 2:
        raise _lib.AgnnError(f"metrics: logits must be a matrix [N, C], got shape {tuple(logits.shape)}")
    if logits.shape[1] < n_cols:
        raise _lib.AgnnError(f"metrics: logits have {logits.shape[1]} columns, the task segments need {n_cols}")
    if logits.dtype != torch.float32 or logits.stride(1) != 1 or (logits.shape[0] > 1 and logits.stride(0) < n_cols):
        logits = logits.float().contiguous()
    # a one-row view may carry any stride(0): the kernel only needs it to reach the columns
    ld = logits.stride(0) if logits.shape[0] > 1 else max(logits.stride(0), n_cols)
    return logits, ld


def _launch(logits, ld, seg_off, seg_end, T, n_cols, labels, ignore_index, row_mask, gate, group, pred, counts, dev):
    N = logits.shape[0]
    if N == 0:                                                # empty tensors have no address to hand over
        return
    _lib.check(_lib.load().agnn_multitask_eval_f32(logits.data_ptr(), ld, seg_off.data_ptr(), _lib.ptr(seg_end), T, n_cols, _lib.ptr(labels),
                                                   N, int(ignore_index), _lib.ptr(row_mask), int(gate), int(group), _lib.ptr(pred),
                                                   _lib.ptr(counts), _lib.stream_ptr(dev)), "agnn_multitask_eval_f32")


def _row_mask_arg(row_mask: Optional[torch.Tensor], N: int) -> Optional[torch.Tensor]:
    if row_mask is None:
        return None
    if tuple(row_mask.shape) != (N,):
        raise _lib.AgnnError(f"metrics: row_mask must have shape [N={N}], got {tuple(row_mask.shape)}")
    row_mask = row_mask.contiguous()
    if row_mask.dtype == torch.bool:
        return row_mask.view(torch.uint8)
    if row_mask.dtype != torch.uint8:
        raise _lib.AgnnError(f"metrics: row_mask must be bool or uint8, got {row_mask.dtype}")
    return row_mask


@torch.no_grad()
def multitask_argmax(logits: torch.Tensor, offs) -> torch.Tensor:
    """int32 [T, N]: the argmax of every task segment of side-by-side logits [N, sum C], in one launch — what `predict_step`
    needs (models/analysis.py:1302-1303; softmax does not move the argmax).  `offs`: T+1 ascending offsets or T `(start, end)`
    pairs, as `continual.distillation_loss` takes them.  `torch.argmax`'s rule: the lowest index among equal maxima, a NaN
    counts as the maximum."""
    dev = _lib.require_gpu(logits)
    starts, ends = _segments(offs, logits.shape[1] if logits.dim() == 2 else 0)
    T, n_cols = len(starts) - 1, (ends[-1] if ends is not None else starts[-1])
    logits, ld = _logits_arg(logits, n_cols)
    seg_off, seg_end = _segment_tensors(starts, ends, dev)
    pred = torch.empty((T, logits.shape[0]), dtype=torch.int32, device=dev)
    _launch(logits, ld, seg_off, seg_end, T, n_cols, None, -1, None, -1, 0, pred, None, dev)
    return pred


def metrics_from_counts(counts, starts: Sequence[int], ends: Sequence[int], tasks: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """The figures behind `MultiTaskMetrics.compute()`, from the integer counters alone: pure Python on the host, no device.
    `counts` (any sequence of 4T + 4 + 3W integers, W = the number of logit columns) in the layout of `agnn_multitask_eval_f32`:
    valid[T] | correct[T] | valid_g[T] | correct_g[T] | joint_valid, joint_correct, joint_valid_g, joint_correct_g | tp[W] |
    n_pred[W] | n_label[W]; task t owns the class bins [starts[t], ends[t]).  Keys of the per-task dicts: `tasks[t]`, or t.

        acc[t]     = correct / valid                                                   (multiclass micro accuracy)
        f1[t]      = mean over the classes c with n_pred_c + n_label_c > 0 of 2 tp_c / (n_pred_c + n_label_c)
        nct_acc[t] = correct_g / valid_g                                               (rows the gate task predicts != 0)
        rna_acc, total_rna_acc = joint_correct / joint_valid, ungated and gated
        support[t] = valid                                                             (int)

    An empty denominator gives nan, as the reference's mean over nothing does.  The macro rule is that of torchmetrics >= 1.0
    and of sklearn's default `f1_score(average="macro")`: classes that occur neither in the labels nor in the predictions are
    left out of the mean.  Parity with torchmetrics itself is UNPINNED — the package is not available where this is tested —
    and is pinned against sklearn instead (tests/test_metrics_counts.py)."""
    c = [int(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    T = len(starts)
    if len(ends) != T or (tasks is not None and len(tasks) != T):
        raise ValueError(f"metrics_from_counts: {T} starts, {len(ends)} ends, {None if tasks is None else len(tasks)} task names")
    rest = len(c) - 4 * T - 4
    if rest < 0 or rest % 3:
        raise ValueError(f"metrics_from_counts: {len(c)} counters do not hold 4 T + 4 + 3 W with T = {T}")
    W = rest // 3
    names = list(tasks) if tasks is not None else list(range(T))
    tp, n_pred, n_label = (c[4 * T + 4 + k * W:4 * T + 4 + (k + 1) * W] for k in range(3))

    def ratio(a: int, b: int) -> float:
        return a / b if b > 0 else math.nan
    out = {"acc": {}, "f1": {}, "nct_acc": {}, "support": {}}
    for t, name in enumerate(names):
        a, b = int(starts[t]), int(ends[t])
        if not 0 <= a <= b <= W:
            raise ValueError(f"metrics_from_counts: segment [{a}, {b}) leaves the {W} class bins")
        valid = c[t]
        out["support"][name] = valid
        out["acc"][name] = ratio(c[T + t], valid)
        out["nct_acc"][name] = ratio(c[3 * T + t], c[2 * T + t])
        f = [2.0 * tp[k] / (n_pred[k] + n_label[k]) for k in range(a, b) if n_pred[k] + n_label[k] > 0]
        out["f1"][name] = math.fsum(f) / len(f) if (f and valid > 0) else math.nan
    j = c[4 * T:4 * T + 4]
    out["rna_acc"] = ratio(j[1], j[0])
    out["total_rna_acc"] = ratio(j[3], j[2])
    return out


class MultiTaskMetrics:
    """The epoch state of the reference's `accuracy_dict` / `f1_dict` and of its gated and joint accuracies: ONE int64 counter
    buffer on the device, zeroed at construction, which every `update` adds to (one launch, no sync, no allocation of its own:
    capturable in a hipGraph from the first call on) and `compute()` reads back once.

    `tasks`: the task names in the order of the logit segments; `offs`: T+1 ascending offsets (`forward_clf_fused`) or T
    `(start, end)` pairs (a `current_val_tasks` subset of a wider matrix).  `gate_task` names the task whose non-zero
    prediction selects the `NCT_*` rows, `joint` the tasks that must all be right for the joint accuracy; a `gate_task` that is
    not among `tasks`, or a `joint` with a member that is not, switches that part off — the reference's `if "tpc_in_label" in
    logits_dict` and `if all(k in labels_dict ...)` (:1153, :1157)."""

    def __init__(self, tasks: Sequence[str], offs, gate_task: Optional[str] = "tpc_in_label", joint: Optional[Sequence[str]] = JOINT_KEYS,
                 device=None, ignore_index: int = -1):
        self.tasks = list(tasks)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.AgnnError(f"MultiTaskMetrics needs a HIP device (no CPU fallback), got {self.device}")
        flat = list(offs)
        n_cols = max(int(o[1]) if isinstance(o, (tuple, list)) else int(o) for o in flat) if flat else 0
        self.starts, self.ends = _segments(flat, n_cols)
        self.T = len(self.starts) - 1
        if self.T != len(self.tasks):
            raise _lib.AgnnError(f"MultiTaskMetrics: {len(self.tasks)} task names for {self.T} segments")
        if self.T > _lib.MAX_SEG:
            raise _lib.AgnnError(f"MultiTaskMetrics: {self.T} tasks, at most {_lib.MAX_SEG}")
        self.n_cols = n_cols
        self.ignore_index = int(ignore_index)
        self.gate = self.tasks.index(gate_task) if gate_task in self.tasks else -1
        joint = list(joint or ())
        self.group = sum(1 << self.tasks.index(k) for k in set(joint)) if joint and all(k in self.tasks for k in joint) else 0
        self._seg_off, self._seg_end = _segment_tensors(self.starts, self.ends, self.device)
        self.counts = torch.zeros(int(_lib.load().agnn_eval_counts_len(self.T, n_cols)), dtype=torch.int64, device=self.device)

    def _ends(self):
        return self.ends if self.ends is not None else self.starts[1:]

    @torch.no_grad()
    def update(self, logits: torch.Tensor, labels: torch.Tensor, row_mask: Optional[torch.Tensor] = None,
               return_pred: bool = False) -> Optional[torch.Tensor]:
        """Add one batch: logits [N, >= n_cols] fp32 (column-slice views as they are), labels int64 [T, N] with `ignore_index`
        for rows a task does not judge (clamping labels beyond a head's width stays the caller's job, :1110-1112: left as they
        are they count as valid and wrong), `row_mask` bool / uint8 [N] to leave rows out altogether (`valid_label_mask`).
        `return_pred`: the same launch also writes the predictions of EVERY row, int32 [T, N] (as `multitask_argmax`)."""
        dev = _lib.require_gpu(logits, labels, row_mask, self.counts)
        logits, ld = _logits_arg(logits, self.n_cols)
        labels = _check_labels(labels, self.T, logits.shape[0])
        pred = torch.empty((self.T, logits.shape[0]), dtype=torch.int32, device=dev) if return_pred else None
        _launch(logits, ld, self._seg_off, self._seg_end, self.T, self.n_cols, labels, self.ignore_index,
                _row_mask_arg(row_mask, logits.shape[0]), self.gate, self.group, pred, self.counts, dev)
        return pred

    @torch.no_grad()
    def reset(self) -> None:
        self.counts.zero_()

    def all_reduce_(self, group=None) -> None:
        """ONE `all_reduce(SUM)` of the counter buffer over the process group: the reference's `dist_reduce_fx="sum"`."""
        import torch.distributed as dist
        dist.all_reduce(self.counts, op=dist.ReduceOp.SUM, group=group)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"counts": self.counts.detach().clone()}

    @torch.no_grad()
    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        if state["counts"].numel() != self.counts.numel():
            raise _lib.AgnnError(f"MultiTaskMetrics.load_state_dict: {state['counts'].numel()} counters, this layout has {self.counts.numel()}")
        self.counts.copy_(state["counts"].reshape(-1))

    def compute(self) -> Dict[str, object]:
        """One device -> host copy; plain Python floats: {"acc": {task: .}, "f1": {task: .}, "nct_acc": {task: .}, "support":
        {task: int}, "rna_acc": ., "total_rna_acc": .} (`metrics_from_counts`)."""
        return metrics_from_counts(self.counts.cpu(), self.starts[:-1], self._ends(), self.tasks)


@torch.no_grad()
def onset_rna_accuracy(probs_or_logits: torch.Tensor, offs, labels: torch.Tensor, edge_index_dict, batch: torch.Tensor,
                       onset_div: torch.Tensor, batch_size: int, valid_label_mask: Optional[torch.Tensor] = None,
                       rna_keys: Sequence[str] = RNA_KEYS, return_counts: bool = False):
    """`test_step`'s `RN(Onset)` accuracy (models/analysis.py:1226-1264) as a device scalar: the share of onsets at which all of
    `rna_keys` are predicted right after the predictions were averaged over the notes of the onset.

    `probs_or_logits` [n, >= sum C] holds the heads' outputs of the `rna_keys`, in that order, in the segments `offs` (T+1
    offsets or T pairs); each segment is softmaxed first, as the reference does with the model's logits (:1217) — hand over
    what the model returns.  `labels` int64 [T, batch_size].  Steps: softmax per segment; mean over the onset neighbours on the
    gather-reduce kernel exactly as `postprocess.onsetwise_logit_aggregation` builds it (the note itself in the numerator, the
    neighbour count in the denominator, edges with both ends < batch_size, no self loops; :1229-1239); softmax again; one row
    per `(batch id, onset)` pair — the first valid note of the pair — through `agnn_multitask_eval_f32` with all keys as the
    joint group, on a counter buffer of its own.  Returns joint_correct / joint_valid (nan when no row is judged); with
    `return_counts` also the int64 device tensor [joint_valid, joint_correct].

    The first-occurrence mask is built with torch ops (`unique` + `scatter_reduce_`, as :1246-1255 does): ONE host sync per test
    batch.  Unlike the reference this keys on the pair itself: its Cantor pairing `(o + b)(o + b + 1) / 2 + b` is not
    one-to-one on (onset, batch id) — e.g. (2, 0) and (0, 1) both give 3 — and merges such onsets; here they stay apart."""
    dev = _lib.require_gpu(probs_or_logits, labels, batch, onset_div, valid_label_mask)
    x = probs_or_logits
    if x.dim() != 2:
        raise _lib.AgnnError(f"onset_rna_accuracy: a matrix [n, C] expected, got shape {tuple(x.shape)}")
    starts, ends = _segments(offs, x.shape[1])
    ends = ends if ends is not None else starts[1:]
    T = len(starts) - 1
    if T != len(list(rna_keys)):
        raise _lib.AgnnError(f"onset_rna_accuracy: {T} segments for the {len(list(rna_keys))} keys {tuple(rna_keys)}")
    n = int(x.shape[0])
    lim = min(int(batch_size), n)
    labels = _check_labels(labels, T, lim)
    widths = [ends[t] - starts[t] for t in range(T)]
    W = sum(widths)
    Wp = (W + 3) & ~3
    seg = [0]
    for w in widths:
        seg.append(seg[-1] + w)
    v = torch.zeros((n, Wp), dtype=torch.float32, device=dev)
    for t in range(T):
        v[:, seg[t]:seg[t + 1]] = torch.softmax(x[:, starts[t]:ends[t]].float(), dim=-1)                 # :1217
    onset_edges = edge_index_dict["note", "onset", "note"]
    e0, e1 = onset_edges[0], onset_edges[1]
    fwd, bwd = build_csr([SegSpec(e1, e0, n), SegSpec(e0, e1, n)])                                       # rows = edge row 1 (the scatter index)
    spec = ops.AggSpec(fwd=[fwd], bwd=[bwd], src_id=[0], n_rows=lim, mean=True, shared_slot=True, skip_self=True, col_limit=lim)
    s = ops.aggregate(spec, [v], self_t=v)                                                               # :1229-1239, [lim, Wp]
    for t in range(T):
        s[:, seg[t]:seg[t + 1]] = torch.softmax(s[:, seg[t]:seg[t + 1]], dim=-1)                         # :1239 `.softmax(-1)`
    # ---- :1242-1255  the first valid note of every (batch id, onset) pair
    valid = torch.ones(lim, dtype=torch.bool, device=dev) if valid_label_mask is None else valid_label_mask[:lim].bool()
    on = onset_div[:lim].to(torch.int64)
    bid = batch[:lim].to(torch.int64)
    row_mask = torch.zeros(lim + 1, dtype=torch.uint8, device=dev)
    if lim > 0:
        key = bid * (on.max() - on.min() + 1) + (on - on.min())                                          # one-to-one on the pairs
        uniq, inverse = torch.unique(key, return_inverse=True)                                           # the host sync
        idx = torch.arange(lim, dtype=torch.int64, device=dev)
        first = torch.full((uniq.numel(),), lim, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, inverse, torch.where(valid, idx, torch.full_like(idx, lim)), reduce="amin")
        row_mask[first] = 1                                                                              # slot `lim`: pairs with no valid note
    counts = torch.zeros(int(_lib.load().agnn_eval_counts_len(T, W)), dtype=torch.int64, device=dev)
    seg_off, _ = _segment_tensors(tuple(seg), None, dev)
    _launch(s, s.stride(0), seg_off, None, T, W, labels, -1, row_mask[:lim], -1, (1 << T) - 1, None, counts, dev)
    joint = counts[4 * T:4 * T + 2]
    acc = (joint[1].double() / joint[0].double()).float()
    return (acc, joint) if return_counts else acc
