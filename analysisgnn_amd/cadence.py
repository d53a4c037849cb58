"""The reference's cadence family (models/cadence.py) on the HIP kernels: `CadenceGNNNeighbor` and `CadenceGNNPytorch`, the join
`LayerNorm(scatter_mean(x[src], dst, out=x.clone()))` between their encoder and `pool_mlp` in one launch each way (`pool_norm`,
csrc/pooljoin.hip), the homogeneous `GNN`, the cadence `HierarchicalHeteroGraphSage` (which also returns the trimmed
`edge_index_dict`), the classifier head both models share, the class-balanced cross entropy of the validation steps
(csrc/balce.hip) and the Lightning steps restated as functions: `cadence_training_loss`, `cadence_validation_loss`,
`cadence_metrics`.  Same class names, constructor arguments and parameter names as the reference, so its `state_dict`s load by name
with `strict=True`.  `SMOTE` is smote.SMOTE, re-exported.  Inputs live on a HIP device; there is no CPU path, and a shape the join
kernel does not take raises `AgnnError`.

Not here: the three Lightning modules, their optimizers and schedulers; `CadenceAssistedPLModel`'s unpadding of a
foreign encoder's output."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, fused, ops
from . import pitch_spelling as _ps
from . import smote as _smote
from ._abi import AgnnError
from .chord import act_norm_drop
from .embedding import embedding
from .encoders import MetricalGNN, SAGEConv, _HybridMixin, _head
from .fused import FusedSequential, norm_act
from .graph import SegSpec, build_csr, hetero_index
from .heads import multitask_cross_entropy
from .linear import Linear, linear, linear2
from .metrics import MultiTaskMetrics
from .smote import SMOTE

__all__ = ["SMOTE", "GNN", "HierarchicalHeteroGraphSage", "CadenceGNNNeighbor", "CadenceGNNPytorch", "JoinNorm", "JoinIndex", "join_index",
           "pool_norm", "cad_clf", "run_cad_clf", "balanced_cross_entropy", "cadence_training_loss", "cadence_validation_loss",
           "cadence_metrics"]

BCE_MAX_CLASSES = _lib.CONSTS["AGNN_BCE_MAX_CLASSES"]
_EDGE = ("n", "e", "n")
_ONSET = ("note", "onset", "note")


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


# ---- the join: onset mean-pool + LayerNorm in one launch --------------------------------------------------------------------------
class JoinIndex:
    """The two index structures of one edge list over n rows, from ONE agnn_csr_build: the edges by destination (rows =
    `dst`, what the forward walks) and by source (the backward).  Messages flow src -> dst, PyG's direction."""

    def __init__(self, n: int, src: torch.Tensor, dst: torch.Tensor):
        if src.dim() != 1 or dst.dim() != 1 or src.shape != dst.shape or src.dtype != torch.int64 or dst.dtype != torch.int64:
            raise AgnnError(f"pool_norm: src and dst must be int64 [E], got {tuple(src.shape)} {src.dtype} and {tuple(dst.shape)} {dst.dtype}")
        _lib.require_gpu(src, dst)
        self.n = int(n)
        self.by_dst, self.by_src = build_csr([SegSpec(dst, src, self.n), SegSpec(src, dst, self.n)])


_JOIN_CACHE: "Dict[tuple, JoinIndex]" = {}
_JOIN_CACHE_MAX = 8


def join_index(n: int, src: torch.Tensor, dst: torch.Tensor) -> JoinIndex:
    """Build (or fetch) the index of a batch: keyed on identity and version of the two tensors, as chord.pool_index is."""
    key = (int(n), src.data_ptr(), tuple(src.shape), src._version, dst.data_ptr(), tuple(dst.shape), dst._version)
    hit = _JOIN_CACHE.get(key)
    if hit is None:
        hit = JoinIndex(n, src, dst)
        if len(_JOIN_CACHE) >= _JOIN_CACHE_MAX:
            _JOIN_CACHE.pop(next(iter(_JOIN_CACHE)))
        _JOIN_CACHE[key] = hit
        hit._keepalive = (src, dst)
    return hit


def clear_join_cache() -> None:
    _JOIN_CACHE.clear()


def _rel(csr):
    return _lib.make_rels([dict(src=None, rowptr=csr.rowptr.data_ptr(), col=csr.col.data_ptr(), ld_src=0)])


class _PoolJoin(torch.autograd.Function):
    """u = the pooled rows, written by agnn_pool_norm_f32, which also leaves LayerNorm(u) and its statistics in `box` for the
    consumer (`fused.norm_act(u, ln, pre=box)`: that node carries the LayerNorm's backward).  Backward: agnn_pool_bwd_f32 on du."""

    @staticmethod
    def forward(ctx, x, ix, pool_rows, col_limit, flags, gamma, beta, eps, box):
        dev = x.device
        n, H = x.shape
        u = torch.empty((n, H), dtype=torch.float32, device=dev)
        y = torch.empty((n, H), dtype=torch.float32, device=dev)
        mean = torch.empty((max(n, 1),), dtype=torch.float32, device=dev)
        rstd = torch.empty((max(n, 1),), dtype=torch.float32, device=dev)
        inv_cnt = torch.empty((max(n, 1),), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().agnn_pool_norm_f32(_rel(ix.by_dst), x.data_ptr(), x.stride(0) if n else H, n, pool_rows, H, col_limit, flags,
                                                  gamma.data_ptr(), beta.data_ptr(), float(eps), u.data_ptr(), H, y.data_ptr(), H,
                                                  mean.data_ptr(), rstd.data_ptr(), inv_cnt.data_ptr(), _lib.stream_ptr(dev)),
                   "agnn_pool_norm_f32")
        box.extend([y, mean, rstd])
        ctx.ix, ctx.cfg = ix, (pool_rows, col_limit, flags)
        ctx.save_for_backward(inv_cnt)
        return u

    @staticmethod
    def backward(ctx, du):
        inv_cnt, = ctx.saved_tensors
        pool_rows, col_limit, flags = ctx.cfg
        du = _lib.rows16(du)
        n, H = du.shape
        dx = torch.empty((n, H), dtype=torch.float32, device=du.device)
        _lib.check(_lib.load().agnn_pool_bwd_f32(_rel(ctx.ix.by_src), du.data_ptr(), du.stride(0) if n else H, inv_cnt.data_ptr(), n, pool_rows,
                                                 H, col_limit, flags, dx.data_ptr(), H, _lib.stream_ptr(du.device)), "agnn_pool_bwd_f32")
        return dx, None, None, None, None, None, None, None, None


def pool_norm(x: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, ln: nn.LayerNorm, pool_rows: Optional[int] = None,
              col_limit: Optional[int] = None, skip_self: bool = False, index: Optional[JoinIndex] = None) -> torch.Tensor:
    """ln(scatter_mean(x[src], dst, dim=0, out=x.clone())) of both cadence models (models/cadence.py:204-205, :324-330) from one
    launch (csrc/pooljoin.hip): x [n, H] fp32 on a HIP device, H a multiple of 4 in [4, 1024]; messages flow src -> dst.  Only
    rows below `pool_rows` pool (default n), only sources below `col_limit` count (default n), `skip_self` drops self loops:
    the reference's two mask compactions as kernel-side predicates.  `index`: a `join_index(n, src, dst)` built earlier.
    There is one path: any other shape raises AgnnError."""
    if x.dim() != 2 or not x.is_cuda or x.dtype != torch.float32:
        raise AgnnError(f"pool_norm: x must be an fp32 [n, H] matrix on a HIP device, got {tuple(x.shape)} {x.dtype} on {x.device}")
    n, H = int(x.shape[0]), int(x.shape[1])
    if H < 4 or H % 4 != 0 or H > 1024:
        raise AgnnError(f"pool_norm: H={H} must be a multiple of 4 in [4, 1024]")
    if not ln.elementwise_affine or tuple(ln.normalized_shape) != (H,) or ln.weight.dtype != torch.float32 or ln.bias is None:
        raise AgnnError(f"pool_norm: an affine fp32 LayerNorm over ({H},) expected, got {ln}")
    _lib.require_gpu(x, src, dst, ln.weight)
    pool_rows = n if pool_rows is None else min(int(pool_rows), n)
    col_limit = n if col_limit is None else max(min(int(col_limit), n), 0)
    if n > 0 and pool_rows < 1:
        raise AgnnError(f"pool_norm: pool_rows={pool_rows} (at least one pooled row)")
    if index is None:
        index = join_index(n, src, dst)
    elif index.n != n:
        raise AgnnError(f"pool_norm: the index was built for {index.n} rows, x has {n}")
    x = _lib.rows16(x)
    gamma, beta = _lib.vec16(ln.weight.detach()), _lib.vec16(ln.bias.detach())
    box: list = []
    u = _PoolJoin.apply(x, index, pool_rows, col_limit, _lib.SPMM_SKIP_SELF if skip_self else 0, gamma, beta, ln.eps, box)
    return norm_act(u, ln, pre=box)


class JoinNorm(nn.LayerNorm):
    """The models' `norm`: an `nn.LayerNorm` (same parameters, same `state_dict` keys) whose forward takes the onset edges and
    runs the pooling in the same launch (a forward hook on it sees the join's output)."""

    def forward(self, x, src, dst, pool_rows=None, col_limit=None, skip_self=False, index=None):
        return pool_norm(x, src, dst, self, pool_rows, col_limit, skip_self, index)


def _pool_mlp(hidden: int, dropout: float) -> FusedSequential:
    return FusedSequential(Linear(hidden, hidden), nn.ReLU(), nn.LayerNorm(hidden), nn.Dropout(dropout), Linear(hidden, hidden))


# ---- the two models ---------------------------------------------------------------------------------------------------------------
class CadenceGNNNeighbor(nn.Module):
    """models/cadence.py:179-226.  The join runs on the trimmed onset edges the stack returns, over all rows, self loops kept."""

    def __init__(self, metadata, input_dim, hidden_dim, output_dim, num_layers, dropout=0.5):
        super().__init__()
        self.gnn = HierarchicalHeteroGraphSage(edge_types=[tuple(e) for e in metadata[1]], input_channels=input_dim, hidden_channels=hidden_dim,
                                               out_channels=hidden_dim // 2, num_layers=num_layers)
        hidden_dim = hidden_dim // 2
        self.norm = JoinNorm(hidden_dim)
        self.pool_mlp = _pool_mlp(hidden_dim, dropout)
        self.cad_clf = cad_clf(hidden_dim, output_dim, dropout)

    def onset_pool(self, x, edge_index_dict):
        onset_index = edge_index_dict[_ONSET]
        return self.pool_mlp(self.norm(x, onset_index[0], onset_index[1]))

    def encode(self, x_dict, edge_index_dict, num_sampled_edges_dict=None, num_sampled_nodes_dict=None):
        dev = _lib.require_gpu(*x_dict.values())
        if self.training:
            fused.advance_rng(dev)
        x, edge_index_dict = self.gnn(x_dict, edge_index_dict, num_sampled_edges_dict=num_sampled_edges_dict,
                                      num_sampled_nodes_dict=num_sampled_nodes_dict)
        return self.onset_pool(x, edge_index_dict)

    def forward(self, x_dict, edge_index_dict, num_sampled_edges_dict=None, num_sampled_nodes_dict=None):
        x = self.encode(x_dict, edge_index_dict, num_sampled_edges_dict, num_sampled_nodes_dict)
        return torch.softmax(self.clf(x), dim=-1)

    def clf(self, x):
        return run_cad_clf(self.cad_clf, x, self.training)


class CadenceGNNPytorch(nn.Module, _HybridMixin):
    """models/cadence.py:229-344 on encoders.MetricalGNN.  The targets are the first `batch_size` rows; the join pools over the
    onset edges with both ends among them, self loops removed.  `use_pitch_spelling` is always set (the reference leaves it unset
    when False) and `pitch_spelling` (int64 [n_notes], values in [0, 38)) is the last keyword of `encode` AND of `forward` (the
    reference's `forward` never passes it and so cannot run); it is refused when needed and absent."""

    def __init__(self, metadata, input_dim, hidden_dim, output_dim, num_layers, dropout=0.5, hybrid=False, use_pitch_spelling=True):
        super().__init__()
        self.gnn = MetricalGNN(input_channels=input_dim, hidden_channels=hidden_dim, output_channels=hidden_dim // 2, num_layers=num_layers,
                               metadata=metadata, dropout=dropout, fast=True)
        self.use_pitch_spelling = bool(use_pitch_spelling)
        if self.use_pitch_spelling:
            self.pitch_spelling_emb = nn.Sequential(nn.Embedding(38, input_dim), nn.LayerNorm(input_dim))
            self.input_projection = FusedSequential(Linear(2 * input_dim, input_dim), nn.ReLU(), nn.LayerNorm(input_dim))
        hidden_dim = hidden_dim // 2
        self.norm = JoinNorm(hidden_dim)
        self.hybrid = bool(hybrid)
        if self.hybrid:
            self._init_hybrid(input_dim, hidden_dim, num_layers, dropout, use_jk=False)
        self.pool_mlp = _pool_mlp(hidden_dim, dropout)
        self.cad_clf = cad_clf(hidden_dim, output_dim, dropout)

    def encode(self, x_dict, edge_index_dict, batch_size, neighbor_mask_node, neighbor_mask_edge, batch_dict=None, pitch_spelling=None):
        note = x_dict["note"]
        dev = _lib.require_gpu(note)
        batch_size = min(int(batch_size), int(note.shape[0]))
        if self.training:
            fused.advance_rng(dev)
        if self.use_pitch_spelling:
            if pitch_spelling is None:
                raise AgnnError("CadenceGNNPytorch: use_pitch_spelling=True needs `pitch_spelling` (int64 [n_notes])")
            emb, ln = self.pitch_spelling_emb
            table = norm_act(emb.weight, ln)                          # the 38 rows normalised once, then gathered
            note = self.input_projection(torch.cat((note, embedding(pitch_spelling, table)), dim=-1))
            x_dict = {**x_dict, "note": note}
        x = self.gnn(x_dict, edge_index_dict, neighbor_mask_node=neighbor_mask_node, neighbor_mask_edge=neighbor_mask_edge,
                     batch_size=batch_size)
        if self.hybrid:
            batch_note = (torch.zeros(batch_size, dtype=torch.long, device=dev) if batch_dict is None else batch_dict["note"][:batch_size])
            z = self.hybrid_forward(_head(note, batch_size), batch_note)          # on the current stream
            w, E = self.cat_proj.weight, x.shape[1]
            y = linear2(x, z, w, self.cat_proj.bias)
            x = y if y is not None else linear(x, w[:, :E], self.cat_proj.bias, acc=linear(z, w[:, E:]))
        onset_index = edge_index_dict[_ONSET]
        x = self.norm(x, onset_index[0], onset_index[1], pool_rows=batch_size, col_limit=batch_size, skip_self=True)
        return self.pool_mlp(x)

    def forward(self, x_dict, edge_index_dict, batch_size, neighbor_mask_node=None, neighbor_mask_edge=None, batch_dict=None,
                pitch_spelling=None):
        """softmax of the logits.  Masks left at None mean zeros, as in the reference: nothing is trimmed."""
        x = self.encode(x_dict, edge_index_dict, batch_size, neighbor_mask_node, neighbor_mask_edge, batch_dict, pitch_spelling)
        return torch.softmax(self.clf(x), dim=-1)

    def clf(self, x):
        return run_cad_clf(self.cad_clf, x, self.training)


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
