"""Parts of the reference's cadence family (models/cadence.py) on the HIP kernels: the homogeneous `GNN`, the cadence
`HierarchicalHeteroGraphSage` (which also returns the trimmed `edge_index_dict`), the classifier head both cadence models share,
the class-balanced cross entropy of the validation steps (csrc/balce.hip) and the Lightning steps restated as functions:
`cadence_training_loss`, `cadence_validation_loss`, `cadence_metrics`.  Same class names, constructor arguments and parameter names
as the reference, so its `state_dict`s load by name.  `SMOTE` is smote.SMOTE, re-exported.  Inputs live on a HIP device; there is
no CPU path.

Not here: `CadenceGNNNeighbor` and `CadenceGNNPytorch` and the join `LayerNorm(scatter_mean(x[src], dst,
out=x.clone()))` between their encoder and `pool_mlp`; the three Lightning modules, their optimizers and schedulers;
`CadenceAssistedPLModel`'s unpadding of a foreign encoder's output.  tests/cadence_ref.py states the two models and the join in
float64, and tests/golden/cadence_*.npz hold what the reference's own classes compute, for whoever builds them."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, fused, ops
from . import pitch_spelling as _ps
from . import smote as _smote
from ._abi import AgnnError
from .chord import act_norm_drop
from .encoders import SAGEConv
from .fused import norm_act
from .graph import hetero_index
from .heads import multitask_cross_entropy
from .linear import Linear, linear
from .metrics import MultiTaskMetrics
from .smote import SMOTE

__all__ = ["SMOTE", "GNN", "HierarchicalHeteroGraphSage", "cad_clf", "run_cad_clf", "balanced_cross_entropy", "cadence_training_loss",
           "cadence_validation_loss", "cadence_metrics"]

BCE_MAX_CLASSES = _lib.CONSTS["AGNN_BCE_MAX_CLASSES"]
_EDGE = ("n", "e", "n")


# ---- class-balanced cross entropy -----------------------------------------------------------------------------------------------
class _BalancedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index, eps_w, out):
        dev = _lib.require_gpu(logits, labels)
        lib = _lib.load()
        n, C = logits.shape
        z = logits if (logits.dtype == torch.float32 and logits.stride(1) == 1) else logits.float().contiguous()
        want = ctx.needs_input_grad[0]
        count = torch.empty((C,), dtype=torch.int64, device=dev)
        weight = torch.empty((C,), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        d = torch.empty((n, C), dtype=torch.float32, device=dev) if want else None
        nws = int(lib.agnn_balanced_ce_workspace_bytes(n))
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        _lib.check(lib.agnn_balanced_ce_f32(_lib.ptr(z) if n else None, z.stride(0) if n else C, n, C, _lib.ptr(labels) if n else None,
                                            int(ignore_index), float(eps_w), count.data_ptr(), weight.data_ptr(), loss.data_ptr(), _lib.ptr(d),
                                            C, _lib.status_word(dev).data_ptr(), ws.data_ptr(), nws, _lib.stream_ptr(dev)),
                   "agnn_balanced_ce_f32")
        if out is not None:
            out.update(class_count=count, weight=weight)
        ctx.save_for_backward(*([d] if want else []))
        ctx.dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        d, = ctx.saved_tensors
        return (d * g).to(ctx.dtype), None, None, None, None


def balanced_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100, eps_w: float = 1e-6,
                           out: Optional[dict] = None) -> torch.Tensor:
    """F.cross_entropy(logits, labels, weight=1 / (bincount(labels) + eps_w)) on agnn_balanced_ce_f32: logits [n, C] fp32,
    1 <= C <= AGNN_BCE_MAX_CLASSES (a thread owns a row: meant for the few classes of a cadence head), labels int64 [n].  No
    valid row: 0 (torch: NaN).  A label outside [0, C) that is not `ignore_index` contributes nothing and raises the device
    status word (`_lib.check_device_status`).  `out`: a dict that receives `class_count` int64 [C] and `weight` fp32 [C].
    Differentiable in the logits."""
    _lib.require_gpu(logits, labels)
    if logits.dim() != 2 or not 1 <= logits.shape[1] <= BCE_MAX_CLASSES:
        raise AgnnError(f"balanced_cross_entropy: logits [n, C] with 1 <= C <= {BCE_MAX_CLASSES} expected, got {tuple(logits.shape)}")
    if labels.dtype != torch.int64 or tuple(labels.shape) != (logits.shape[0],):
        raise AgnnError(f"balanced_cross_entropy: labels must be int64 [{logits.shape[0]}], got {tuple(labels.shape)} {labels.dtype}")
    return _BalancedCE.apply(logits, labels.contiguous(), int(ignore_index), float(eps_w), out)


# ---- the classifier head ----------------------------------------------------------------------------------------------------------
def cad_clf(hidden_dim: int, output_dim: int, dropout: float = 0.5) -> nn.Sequential:
    """`cad_clf` of both cadence models (models/cadence.py:194-200, :268-274): the same modules at the same indices."""
    return nn.Sequential(Linear(hidden_dim, hidden_dim // 2), nn.ReLU(), nn.BatchNorm1d(hidden_dim // 2), nn.Dropout(dropout),
                         Linear(hidden_dim // 2, output_dim))


def run_cad_clf(seq: nn.Sequential, x: torch.Tensor, training: bool) -> torch.Tensor:
    """Linear -> ReLU -> BatchNorm1d -> Dropout -> Linear with the middle three in one block (chord.act_norm_drop).  One row in
    training mode is refused, as torch refuses it for BatchNorm1d."""
    first, act, bn, drop, last = list(seq)
    if training and x.shape[0] == 1:
        raise AgnnError("cad_clf: one row in training mode (BatchNorm1d needs more than one value per channel)")
    h = linear(x, first.weight, first.bias)
    h = act_norm_drop(h, bn, act, drop.p, training)
    return linear(h, last.weight, last.bias)


# ---- the stacks -------------------------------------------------------------------------------------------------------------------
class GNN(nn.Module):
    """models/cadence.py:121-139: a homogeneous SAGEConv stack, `ReLU -> LayerNorm -> Dropout` between the layers (one
    `normalize` for all of them, as in the reference)."""

    def __init__(self, input_dim, output_dim, num_layers, dropout=0.5):
        super().__init__()
        self.convs = nn.ModuleList()
        self.convs.append(SAGEConv(input_dim, output_dim))
        for _ in range(num_layers - 1):
            self.convs.append(SAGEConv(output_dim, output_dim))
        self.dropout = nn.Dropout(dropout)
        self.activation = nn.ReLU()
        self.normalize = nn.LayerNorm(output_dim)

    @staticmethod
    def _conv(conv: SAGEConv, x, index):
        """lin_l(mean of the in-neighbours) + lin_r(x): one aggregation, the second GEMM accumulates onto the first."""
        xp, H = ops.pad4(x)
        spec = ops.AggSpec(fwd=[index.fwd[_EDGE]], bwd=[index.bwd[_EDGE]], src_id=[0], n_rows=int(x.shape[0]), mean=True, shared_slot=True)
        a = ops.aggregate(spec, [xp])
        a = a if a.shape[1] == H else a[:, :H]
        return linear(x, conv.lin_r.weight, None, acc=linear(a, conv.lin_l.weight, conv.lin_l.bias))

    def forward(self, x, edge_index):
        _lib.require_gpu(x, edge_index)
        if self.training and self.dropout.p > 0:
            fused.advance_rng(x.device)
        index = hetero_index({_EDGE: edge_index}, {"n": int(x.shape[0])})        # by destination and by source, cached per batch
        for conv in self.convs[:-1]:
            x = self._conv(conv, x, index)
            x = norm_act(x, self.normalize, pre_relu=True, p=self.dropout.p, training=self.training)
        return self._conv(self.convs[-1], x, index)


class HierarchicalHeteroGraphSage(_ps.HierarchicalHeteroGraphSage):
    """models/cadence.py:142-176: the pitch-spelling stack (HeteroConv{SAGEConv}(aggr='sum') with trim_to_layer, ReLU after every
    layer, no LayerNorm, `lin` on the note rows), which here returns (x, the trimmed edge_index_dict) as the reference's does."""

    def forward(self, x_dict, edge_index_dict, num_sampled_edges_dict=None, num_sampled_nodes_dict=None):
        x, last = self._run(x_dict, edge_index_dict, num_sampled_edges_dict, num_sampled_nodes_dict)
        trimmed = {et: (ei if last.get(et) is None else ei[:, :max(int(last[et]), 0)]) for et, ei in edge_index_dict.items()}
        return x, trimmed


# ---- the Lightning steps, as functions ------------------------------------------------------------------------------------------
def cadence_training_loss(module, x: torch.Tensor, y: torch.Tensor, smote: SMOTE, reg_loss_weight: float, epoch: Optional[int] = None,
                          perms=None, draws=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(total, logits, y_over) of the training steps on the encoded target rows x [n, D] and their labels y; `module` is anything
    with the cadence models' `clf(x)`:
        feature = mean(x^2) + smote.feature_penalty (each class cut to 100 rows, models/cadence.py:401-417 and :511-533)
        ce      = cross entropy, label smoothing 0.1, of module.clf on SMOTE.fit_generate's oversampled rows
        total   = ce + reg_loss_weight * feature                      epoch None (CadenceNeighborPLModel, :493-509)
                = ce + reg_loss_weight * feature * epoch * 0.01       otherwise  (CadencePLModel, :420)
    `perms` as smote.feature_penalty takes them, `draws` as SMOTE.fit_generate does (None: the library's generators)."""
    _lib.require_gpu(x, y)
    feature = x.pow(2).mean()
    x_over, y_over = smote.fit_generate(x, y, draws=draws)
    n_cls = int(torch.unique(y_over).numel())                       # the penalty cuts every class to 100 rows: 100 * classes in all
    feature = _smote.feature_penalty(feature, x_over, y_over, x, y, batch_size=100 * max(n_cls, 1), perms=perms)
    logits = module.clf(x_over)
    ce = multitask_cross_entropy(logits, [0, int(logits.shape[1])], y_over.long()[None], label_smoothing=0.1, ignore_index=-1)[0]
    reg = float(reg_loss_weight) * (1.0 if epoch is None else float(epoch) * 0.01)
    return ce + reg * feature, logits, y_over


def cadence_validation_loss(logits: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The validation steps' loss (models/cadence.py:425-434, :535-544): cross entropy weighted by 1 / (class count + 1e-6)."""
    return balanced_cross_entropy(logits, y.long(), eps_w=1e-6)


def cadence_metrics(logits: torch.Tensor, y: torch.Tensor) -> Dict[str, float]:
    """{"acc", "f1"}: multiclass accuracy and macro F1 over the logits' columns, from metrics.MultiTaskMetrics' counters."""
    dev = _lib.require_gpu(logits, y)
    m = MultiTaskMetrics(["cadence"], [0, int(logits.shape[1])], gate_task=None, joint=None, device=dev)
    m.update(logits, y.long()[None])
    out = m.compute()
    return {"acc": out["acc"]["cadence"], "f1": out["f1"]["cadence"]}
