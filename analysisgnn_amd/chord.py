"""The reference's ChordGNN family (models/chord.py) on the HIP kernels: `MetricalChordPredictionModel` -> `MetricalChordEncoder`
-> in-tree `MetricalGNN` -> `OnsetEdgePoolingVersion2` -> BatchNorm projections -> bi-GRU -> `MultiTaskMLP` / `NadeClassifierLayer`.
Same class names, constructor arguments, parameter and buffer names and forward signatures, so a reference `state_dict` loads by
name and a caller switches imports; `nn.BatchNorm1d`, `nn.Linear`, `nn.Embedding`, `nn.GRU`, `nn.LayerNorm` stay as parameter
holders.  Inputs live on a HIP device; there is no CPU path.

Two schedules differ from the reference's:
  * `activation -> BatchNorm1d -> dropout` over the row axis is one block of launches (`colnorm`, csrc/colnorm.hip); the T task
    heads' first layers are ONE stacked GEMM [N, T * hidden] and ONE such block, since batch statistics are per column;
  * onset pooling computes only the selected rows and pools BEFORE `trans` (`onset_pool`, csrc/onsetpool.hip): the weights of a
    mean sum to one, so trans(mean) == mean(trans), and the Linear runs on K rows instead of N.
Also here: `PostProcessingMLTModel` (models/chord.py:751-783), whose LSTM runs the persistent kernels of lstm_seq.py.
Not here: `idx=None` pooling (`__merge_edges__` returns a mask where chord.py:568 needs an index), unequal `lengths` (the
reference then returns padded rows), and the classes DESIGN.md §19 lists as out of scope."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, fused
from ._abi import AgnnError
from .core_layers import GATConvLayer, MetricalGNN, RelEdgeConv, ResGatedGraphConv, SageConvScatter, _is_relu
from .embedding import embed_cat
from .graph import Csr, SegSpec, build_csr
from .gru import gru_forward
from .heads import GPROJ_K, _cat_params, grouped_projection
from .linear import linear

CN_RELU, CN_TRAIN = _lib.CONSTS["AGNN_CN_RELU"], _lib.CONSTS["AGNN_CN_TRAIN"]


# ---- y = dropout(BatchNorm1d(act(x))) over the rows -----------------------------------------------------------------------------
class _ColNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running, eps, momentum, p, flags, call_id):
        """x [n, C]; gamma / beta [C]; running = (running_mean, running_var, num_batches_tracked or None) or None: updated in
        place by the kernel with AGNN_CN_TRAIN, read without it."""
        dev = _lib.require_gpu(x, gamma, beta)
        lib = _lib.load()
        x = _lib.rows16(x)
        gamma, beta = _lib.vec16(gamma), _lib.vec16(beta)
        n, C = x.shape
        train = bool(flags & CN_TRAIN)
        need_bwd = any(ctx.needs_input_grad[:3])
        y = torch.empty((n, C), dtype=torch.float32, device=dev)
        stats = torch.empty((3, C), dtype=torch.float32, device=dev) if (train or need_bwd) else None
        rng = fused.rng_state(dev) if p > 0 else None
        used = torch.empty(2, dtype=torch.int64, device=dev) if p > 0 else None
        nws = int(lib.agnn_colnorm_workspace_bytes(n, C)) if train else 0
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev) if train else None
        rm, rv, nbt = running if running is not None else (None, None, None)
        _lib.check(lib.agnn_colnorm_fwd_f32(x.data_ptr(), x.stride(0), n, C, gamma.data_ptr(), beta.data_ptr(), _lib.ptr(rm), _lib.ptr(rv),
                                            _lib.ptr(nbt), float(eps), float(momentum), float(p), int(flags), _lib.ptr(rng), int(call_id),
                                            y.data_ptr(), y.stride(0), _lib.ptr(stats), _lib.ptr(used), _lib.ptr(ws), nws,
                                            _lib.stream_ptr(dev)), "agnn_colnorm_fwd_f32")
        if need_bwd:
            ctx.save_for_backward(x, gamma, stats, *([used] if used is not None else []))
        ctx.cfg = (float(p), int(flags), int(call_id))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, stats, *used = ctx.saved_tensors
        p, flags, call_id = ctx.cfg
        dev = dy.device
        lib = _lib.load()
        dy = _lib.rows16(dy)
        n, C = x.shape
        dx = torch.empty_like(x)
        dgamma = torch.empty((C,), dtype=torch.float32, device=dev)
        dbeta = torch.empty((C,), dtype=torch.float32, device=dev)
        if n > 0:
            nws = int(lib.agnn_colnorm_workspace_bytes(n, C))
            ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
            _lib.check(lib.agnn_colnorm_bwd_f32(x.data_ptr(), x.stride(0), n, C, gamma.data_ptr(), stats.data_ptr(), p, flags,
                                                _lib.ptr(used[0] if used else None), call_id, dy.data_ptr(), dy.stride(0), dx.data_ptr(),
                                                dx.stride(0), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), nws, _lib.stream_ptr(dev)),
                       "agnn_colnorm_bwd_f32")
        else:
            dgamma.zero_()
            dbeta.zero_()
        return dx, dgamma, dbeta, None, None, None, None, None, None


def colnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running, eps: float, momentum: float, relu: bool, p: float,
            training: bool) -> torch.Tensor:
    """dropout_p(batch_norm(relu?(x))) over the rows of x [n, C] (fp32, C % 4 == 0) on `agnn_colnorm_*`.  `training`: batch
    statistics, `running` = (running_mean [C], running_var [C], num_batches_tracked or None) updated in place as nn.BatchNorm1d
    does, and dropout; otherwise the running statistics and no dropout.  `running` None: batch statistics always."""
    _lib.require_gpu(x)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] % 4 != 0 or x.shape[1] < 4:
        raise AgnnError(f"colnorm: a [n, C] fp32 matrix with C % 4 == 0 expected, got {tuple(x.shape)} {x.dtype}")
    batch_stats = training or running is None
    if batch_stats and x.shape[0] == 1:
        raise AgnnError(f"colnorm: expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    flags = (CN_RELU if relu else 0) | (CN_TRAIN if batch_stats else 0)
    return _ColNorm.apply(x, gamma, beta, running if (training or not batch_stats) else None, eps, momentum, float(p) if training else 0.0,
                          flags, next(fused._CALL_IDS) & 0xFFFFFFFF)


def _running(bn: nn.BatchNorm1d):
    if not bn.track_running_stats or bn.running_mean is None:
        return None
    return (bn.running_mean, bn.running_var, bn.num_batches_tracked)


def _check_bn(bn: nn.BatchNorm1d) -> None:
    if not bn.affine:
        raise AgnnError("act_norm_drop: BatchNorm1d without affine parameters is not built")
    if bn.track_running_stats and bn.momentum is None:
        raise AgnnError("act_norm_drop: momentum=None (cumulative average) is not built")


def act_norm_drop(x: torch.Tensor, bn: nn.BatchNorm1d, activation, p: float, training: bool) -> torch.Tensor:
    """dropout_p(bn(activation(x))): ReLU and identity are fused into the block; any other activation runs as its torch call in
    front of an identity block."""
    _check_bn(bn)
    if activation is None or isinstance(activation, nn.Identity):
        relu = False
    elif _is_relu(activation):
        relu = True
    else:
        x, relu = activation(x), False
    return colnorm(x, bn.weight, bn.bias, _running(bn), bn.eps, bn.momentum if bn.momentum is not None else 0.0, relu, p, training)


# ---- onset pooling with selection -------------------------------------------------------------------------------------------------
class PoolIndex:
    """The three index structures of one (onset edge list, selected rows) pair, from ONE agnn_csr_build: the edges by destination
    (forward), by source (backward) and the selected positions by node (backward: a node selected twice takes both gradients)."""

    def __init__(self, n: int, edge_index: torch.Tensor, idx: torch.Tensor):
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise AgnnError(f"onset_pool: edge_index must be int64 [2, E], got {tuple(edge_index.shape)} {edge_index.dtype}")
        if idx.dim() != 1 or idx.dtype != torch.int64:
            raise AgnnError(f"onset_pool: idx must be int64 [K], got {tuple(idx.shape)} {idx.dtype}")
        _lib.require_gpu(edge_index, idx)
        self.n, self.K = int(n), int(idx.shape[0])
        self.idx = idx if idx.is_contiguous() else idx.contiguous()
        ks = torch.arange(self.K, dtype=torch.int64, device=idx.device)
        self.by_dst, self.by_src, self.sel = build_csr([SegSpec(edge_index[1], edge_index[0], self.n),
                                                        SegSpec(edge_index[0], edge_index[1], self.n), SegSpec(self.idx, ks, self.n)])


_POOL_CACHE: "Dict[tuple, PoolIndex]" = {}
_POOL_CACHE_MAX = 8


def pool_index(n: int, edge_index: torch.Tensor, idx: torch.Tensor) -> PoolIndex:
    """Build (or fetch) the index of a batch: keyed on identity and version of the two tensors, as graph.hetero_index is."""
    key = (int(n), edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, idx.data_ptr(), tuple(idx.shape), idx._version)
    hit = _POOL_CACHE.get(key)
    if hit is None:
        hit = PoolIndex(n, edge_index, idx)
        if len(_POOL_CACHE) >= _POOL_CACHE_MAX:
            _POOL_CACHE.pop(next(iter(_POOL_CACHE)))
        _POOL_CACHE[key] = hit
        hit._keepalive = (edge_index, idx)
    return hit


def clear_pool_cache() -> None:
    _POOL_CACHE.clear()


class _OnsetPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, ix: PoolIndex):
        dev = _lib.require_gpu(a)
        lib = _lib.load()
        a = _lib.rows16(a)
        n, H = a.shape
        out = torch.empty((ix.K, H), dtype=torch.float32, device=dev)
        _lib.check(lib.agnn_onset_pool_fwd_f32(a.data_ptr(), a.stride(0), n, H, ix.by_dst.rowptr.data_ptr(), ix.by_dst.col.data_ptr(),
                                               ix.idx.data_ptr(), ix.K, out.data_ptr(), out.stride(0) if ix.K else H,
                                               _lib.status_word(dev).data_ptr(), _lib.stream_ptr(dev)), "agnn_onset_pool_fwd_f32")
        ctx.ix, ctx.shape = ix, (n, H)
        return out

    @staticmethod
    def backward(ctx, g):
        ix: PoolIndex = ctx.ix
        n, H = ctx.shape
        dev = g.device
        lib = _lib.load()
        g = _lib.rows16(g)
        da = torch.empty((n, H), dtype=torch.float32, device=dev)
        _lib.check(lib.agnn_onset_pool_bwd_f32(g.data_ptr(), g.stride(0) if ix.K else H, ix.K, H, n, ix.by_dst.rowptr.data_ptr(),
                                               ix.by_src.rowptr.data_ptr(), ix.by_src.col.data_ptr(), ix.sel.rowptr.data_ptr(),
                                               ix.sel.col.data_ptr(), da.data_ptr(), da.stride(0), _lib.stream_ptr(dev)),
                   "agnn_onset_pool_bwd_f32")
        return da, None


def onset_pool(a: torch.Tensor, edge_index: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """pooled[k] = (a[idx[k]] + sum_{e : edge_index[1][e] == idx[k]} a[edge_index[0][e]]) / (1 + indeg(idx[k])) for a [n, H] fp32,
    H % 4 == 0: the mean over each selected note's onset neighbours and itself (csrc/onsetpool.hip)."""
    _lib.require_gpu(a, edge_index, idx)
    if a.dim() != 2 or a.dtype != torch.float32 or a.shape[1] % 4 != 0 or a.shape[1] < 4:
        raise AgnnError(f"onset_pool: a [n, H] fp32 matrix with H % 4 == 0 expected, got {tuple(a.shape)} {a.dtype}")
    return _OnsetPool.apply(a, pool_index(a.shape[0], edge_index, idx))


def unique_onsets(onsets: torch.Tensor) -> torch.Tensor:
    """The first note index of each distinct onset, in ascending order of the onsets (models/chord.py:1692-1702).  Device ops only;
    the one host read is the number of distinct onsets (`torch.unique`).  The smallest index wins by a min-reduction: the
    reference's `scatter_` of a flipped range leaves the winner among equal targets to the scatter's write order."""
    unique, inverse = torch.unique(onsets, sorted=True, return_inverse=True)
    perm = torch.arange(inverse.size(0), dtype=inverse.dtype, device=inverse.device)
    return inverse.new_empty(unique.numel()).scatter_reduce_(0, inverse, perm, reduce="amin", include_self=False)


class OnsetEdgePoolingVersion2(nn.Module):
    """models/chord.py:255-290.  `forward(x, edge_index, idx)` -> (trans(pooled rows), idx)."""

    def __init__(self, in_channels, dropout=0):
        super().__init__()
        self.in_channels = in_channels
        self.trans = nn.Linear(in_channels, in_channels)
        self.reset_parameters()

    def reset_parameters(self):
        self.trans.reset_parameters()

    def forward(self, x, edge_index, idx=None):
        if idx is None:
            raise AgnnError("OnsetEdgePoolingVersion2: idx=None is not built: the reference's __merge_edges__ returns a 0/1 mask where "
                            "models/chord.py:568 indexes with it (a size mismatch there); pass unique_onsets(onsets)")
        pooled = onset_pool(x, edge_index, idx)
        return linear(pooled, self.trans.weight, self.trans.bias), idx


# ---- core/mlp.py and the classifier layers ------------------------------------------------------------------------------------------
class MLP(nn.Module):
    """core/mlp.py: (Linear -> activation -> BatchNorm1d -> Dropout) per hidden layer, all through the ONE `normalize`, then Linear."""

    def __init__(self, in_feats, n_hidden, out_feats=None, n_layers=1, activation=F.relu, dropout=0.5, bias=False):
        super().__init__()
        if out_feats is None:
            out_feats = n_hidden
        self.n_hidden = n_hidden
        self.layers = nn.ModuleList()
        self.normalize = nn.BatchNorm1d(n_hidden)
        self.activation = activation
        self.dropout = nn.Dropout(dropout)
        self.layers.append(nn.Linear(in_feats, n_hidden, bias=bias))
        for _ in range(n_layers - 1):
            self.layers.append(nn.Linear(n_hidden, n_hidden, bias=bias))
        self.layers.append(nn.Linear(n_hidden, out_feats, bias=bias))
        self.reset_parameters()

    def reset_parameters(self):
        for layer in self.layers:
            nn.init.xavier_uniform_(layer.weight, gain=nn.init.calculate_gain('relu'))
            if layer.bias is not None:
                nn.init.constant_(layer.bias, 0.)

    def forward(self, x):
        _lib.require_gpu(x)
        h = x
        for layer in list(self.layers)[:-1]:
            h = linear(h, layer.weight, layer.bias)
            h = act_norm_drop(h, self.normalize, self.activation, self.dropout.p, self.training)
        return linear(h, self.layers[-1].weight, self.layers[-1].bias)


class NadeClf(nn.Module):
    def __init__(self, input_size, n_hidden, out_dim, n_layers, activation=F.relu, dropout=0.5):
        super().__init__()
        self.VtoH = nn.Linear(out_dim, input_size, bias=False)
        self.HtoV = MLP(input_size, n_hidden, out_dim, n_layers=n_layers, bias=True, activation=activation, dropout=dropout)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.VtoH.weight, gain=nn.init.calculate_gain('relu'))

    def forward(self, h):
        out = self.HtoV(h)
        return out, linear(torch.sigmoid(out), self.VtoH.weight, None, acc=h)


class NadeClassifierLayer(nn.Module):
    """models/chord.py:344-354: the chain over the tasks is serial (each step reads the state the previous one updated)."""

    def __init__(self, input_size, n_hidden, tasks, n_layers, activation=F.relu, dropout=0.5):
        super().__init__()
        self.tasks = tasks
        self.classifier = nn.ModuleDict({task: NadeClf(input_size, n_hidden, tdim, n_layers, activation, dropout) for task, tdim in tasks.items()})

    def forward(self, h):
        prediction = {}
        for task in self.tasks.keys():
            prediction[task], h = self.classifier[task](h)
        return prediction


def _adjacent_flat(ts: Sequence[torch.Tensor]) -> Optional[torch.Tensor]:
    """The one tensor whose equal slices `ts` are, when they lie side by side in one storage; else None."""
    t0 = ts[0]
    k = t0.numel()
    st = t0.untyped_storage().data_ptr()
    for i, t in enumerate(ts):
        if (not t.is_contiguous() or t.numel() != k or t.untyped_storage().data_ptr() != st
                or t.storage_offset() != t0.storage_offset() + i * k):
            return None
    return t0.as_strided((len(ts) * k,), (1,), t0.storage_offset())


class MultiTaskMLP(nn.Module):
    """models/chord.py:357-375.  With one hidden layer per task (what the prediction model builds) the T first layers are one
    stacked GEMM, the T `activation -> BatchNorm1d -> dropout` blocks one `colnorm` over [N, T * hidden], and the T last layers
    one grouped projection (hidden widths 32, 64, 128; otherwise T products on column windows); the running statistics of the T BatchNorms are kept side by side in one buffer for that (each
    module's `running_mean` / `running_var` / `num_batches_tracked` is a slice of it: `state_dict` is unchanged)."""

    def __init__(self, in_feats, n_hidden, tasks: dict, n_layers, activation=F.relu, dropout=0.5):
        super().__init__()
        self.dropout = dropout
        self.n_layers = n_layers
        self.tasks = tasks
        self.classifier = nn.ModuleDict({task: MLP(in_feats, n_hidden, tdim, n_layers, activation, dropout) for task, tdim in tasks.items()})

    def reset_parameters(self):
        for task in self.tasks.keys():
            self.classifier[task].reset_parameters()

    def _stacked_running(self, mods: List[MLP]):
        """(running_mean [T * h], running_var [T * h], num_batches_tracked [T]) whose slices ARE the modules' buffers; buffers that
        do not lie side by side (a fresh module, one moved by `.to()`) are laid out anew, once, outside any capture."""
        out = []
        for name in ("running_mean", "running_var", "num_batches_tracked"):
            ts = [getattr(m.normalize, name).reshape(-1) for m in mods]
            flat = _adjacent_flat(ts)
            if flat is None:
                flat = torch.cat(ts)
                k = ts[0].numel()
                for i, m in enumerate(mods):
                    setattr(m.normalize, name, flat[i * k:(i + 1) * k].view(getattr(m.normalize, name).shape))
            out.append(flat)
        return tuple(out)

    def _stackable(self) -> bool:
        mods = [self.classifier[t] for t in self.tasks.keys()]
        m0 = mods[0]
        return (len(m0.layers) == 2 and all(len(m.layers) == 2 and m.n_hidden == m0.n_hidden and m.activation is m0.activation
                                            and m.dropout.p == m0.dropout.p and m.normalize.eps == m0.normalize.eps
                                            and m.normalize.momentum == m0.normalize.momentum and m.normalize.track_running_stats
                                            and m.normalize.affine and (m.layers[0].bias is None) == (m0.layers[0].bias is None)
                                            and (m.layers[1].bias is None) == (m0.layers[1].bias is None) for m in mods)
                and m0.n_hidden % 4 == 0)

    def forward_fused(self, x) -> Tuple[torch.Tensor, List[int], List[str]]:
        """(logits [N, sum of classes] side by side, their offsets, the task names), as TorchAnalysisGNN.forward_clf_fused."""
        _lib.require_gpu(x)
        tasks = list(self.tasks.keys())
        mods = [self.classifier[t] for t in tasks]
        offs = [0]
        for m in mods:
            offs.append(offs[-1] + m.layers[-1].out_features)
        if not self._stackable():
            return torch.cat([m(x) for m in mods], dim=1), offs, tasks
        m0, T, h = mods[0], len(mods), mods[0].n_hidden
        _check_bn(m0.normalize)
        W1 = _cat_params([m.layers[0].weight for m in mods])                                   # [T * h, in]
        b1 = _cat_params([m.layers[0].bias for m in mods]) if m0.layers[0].bias is not None else None
        a = linear(x, W1, b1)                                                                  # [N, T * h]
        gamma = _cat_params([m.normalize.weight for m in mods])
        beta = _cat_params([m.normalize.bias for m in mods])
        rm, rv, nbt = self._stacked_running(mods)
        act = m0.activation
        if act is None or isinstance(act, nn.Identity):
            relu = False
        elif _is_relu(act):
            relu = True
        else:
            a, relu = act(a), False
        a = colnorm(a, gamma, beta, (rm, rv, None), m0.normalize.eps, m0.normalize.momentum, relu, m0.dropout.p, self.training)
        if self.training:
            nbt.add_(1)                                                                        # the T counters, one launch
        if h in GPROJ_K and T <= _lib.MAX_SEG:
            W2 = _cat_params([m.layers[1].weight for m in mods])                               # [sum C, h]
            b2 = _cat_params([m.layers[1].bias for m in mods]) if m0.layers[1].bias is not None else None
            logits = grouped_projection(a, W2, b2, offs, h)
        else:                  # widths the grouped kernel is not built for: T products, each on its column window of `a`, read in place
            logits = torch.cat([linear(a[:, i * h:(i + 1) * h], m.layers[1].weight, m.layers[1].bias) for i, m in enumerate(mods)], dim=1)
        return logits, offs, tasks

    def forward(self, x):
        logits, offs, tasks = self.forward_fused(x)
        return {t: logits[:, offs[i]:offs[i + 1]] for i, t in enumerate(tasks)}


# ---- the encoder and the model ----------------------------------------------------------------------------------------------------
_CONV_BLOCKS = {"ResConv": ResGatedGraphConv, "SageConv": SageConvScatter, "Sage": SageConvScatter, None: SageConvScatter,
                "GAT": GATConvLayer, "GATConv": GATConvLayer, "RelEdgeConv": RelEdgeConv}
_METRICAL_ARGS = ("beat_nodes", "measure_nodes", "beat_edges", "measure_edges")


class MetricalChordEncoder(nn.Module):
    """models/chord.py:506-583 (`layernorm1/2` are BatchNorm1d there, despite the names)."""

    def __init__(self, in_feats, n_hidden, n_layers, activation=F.relu, dropout=0.5, use_jk=False, metrical=False, use_reledge=False,
                 **kwargs):
        super().__init__()
        self.activation = activation
        self.spelling_embedding = nn.Embedding(49, 16)
        self.pitch_embedding = nn.Embedding(128, 16)
        self.embedding = nn.Linear(in_feats - 3, 32)
        self.etypes = {"onset": 0, "consecutive": 1, "during": 2, "rests": 3, "consecutive_rev": 4, "during_rev": 5, "rests_rev": 6}
        pitch_embedding = kwargs.get("pitch_embedding", 0)
        pitch_embedding = 0 if pitch_embedding is None else pitch_embedding
        block = kwargs.get("conv_block", "SageConv")
        if block not in _CONV_BLOCKS:
            raise ValueError("Block type not supported")
        self.encoder = MetricalGNN(64, n_hidden, n_hidden, self.etypes, n_layers, dropout=dropout, jk=use_jk,
                                   in_edge_features=3 + pitch_embedding, metrical=metrical, use_reledge=use_reledge,
                                   conv_block=_CONV_BLOCKS[block])
        self.pool = OnsetEdgePoolingVersion2(n_hidden, dropout=dropout)
        self.proj1 = nn.Linear(n_hidden + 1, n_hidden)
        self.layernorm1 = nn.BatchNorm1d(n_hidden)
        self.proj2 = nn.Linear(n_hidden, n_hidden // 2)
        self.layernorm2 = nn.BatchNorm1d(n_hidden // 2)
        self.gru = nn.GRU(input_size=n_hidden // 2, hidden_size=int(n_hidden / 2), num_layers=2, bidirectional=True, batch_first=True,
                          dropout=dropout)
        self.layernormgru = nn.LayerNorm(n_hidden)
        self.reset_parameters()

    def reset_parameters(self):
        relu_gain = nn.init.calculate_gain('relu')
        for lin in (self.embedding, self.proj1, self.proj2):
            nn.init.xavier_uniform_(lin.weight, gain=relu_gain)
            nn.init.constant_(lin.bias, 0)
        self.layernormgru.reset_parameters()
        self.layernorm1.reset_parameters()
        self.layernorm2.reset_parameters()
        self.pool.reset_parameters()

    def forward(self, x, edge_index, edge_type, onset_index, onset_idx, lengths, **kwargs):
        _lib.require_gpu(x)
        B = 1
        if lengths is not None:
            # a device tensor costs a host read here on every forward (and cannot be captured): hand over host integers (a list,
            # a tuple or a CPU tensor), once per batch
            ls = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
            if len(set(ls)) > 1:
                raise AgnnError(f"MetricalChordEncoder: unequal lengths {ls} are not built: the reference reshapes the PADDED GRU "
                                "output (models/chord.py:579) and returns more rows than there are labels; only equal lengths "
                                "(and None: one sequence) are meaningful")
            B = len(ls)
        h = linear(x[:, 2:-1], self.embedding.weight, self.embedding.bias)
        h = embed_cat(h, [x[:, 0].long(), x[:, 1].long()], [self.pitch_embedding.weight, self.spelling_embedding.weight])
        for k in _METRICAL_ARGS:
            kwargs.setdefault(k, None)
        h = self.encoder(h, edge_index, edge_type, **kwargs)
        h = F.normalize(self.activation(h))
        h, idx = self.pool(h, onset_index, onset_idx)
        # proj1(cat([h, s])) with s = x[:, -1][idx], without the [K, H + 1] cat: h W[:, :H]^T + b + s W[:, H]^T
        Hn = h.shape[1]
        w1 = self.proj1.weight
        h = linear(h, w1[:, :Hn], self.proj1.bias, acc=x[:, -1][idx].unsqueeze(1) * w1[:, Hn].unsqueeze(0))
        h = act_norm_drop(h, self.layernorm1, self.activation, 0.0, self.training)
        h = act_norm_drop(linear(h, self.proj2.weight, self.proj2.bias), self.layernorm2, self.activation, 0.0, self.training)
        K, C = h.shape
        if lengths is not None and B * ls[0] != K:
            raise AgnnError(f"MetricalChordEncoder: lengths {ls} do not add up to the {K} selected rows")
        h = gru_forward(self.gru, h.view(B, K // B, C), self.training)                          # equal lengths: packed == padded
        h = fused.norm_act(h, self.layernormgru, training=self.training)
        return h.reshape(K, h.shape[-1])


class MetricalChordPredictionModel(nn.Module):
    """models/chord.py:605-653, with its unused `pitch_embedding` and the `in_feats + 128` of its encoder."""

    def __init__(self, in_feats, n_hidden=256, pitch_dims=35, tasks: dict = {
            "localkey": 38, "tonkey": 38, "degree1": 22, "degree2": 22, "quality": 11, "inversion": 4,
            "root": 35, "romanNumeral": 31, "hrhythm": 7, "pcset": 121, "bass": 35, "tenor": 35,
            "alto": 35, "soprano": 35}, n_layers=1, activation=F.relu, dropout=0.5, use_nade=False, use_jk=False,
                 metrical=False, use_reledge=False, **kwargs):
        super().__init__()
        self.dropout = dropout
        self.n_layers = n_layers
        self.tasks = tasks
        self.pitch_embedding = nn.Embedding(35, 128)
        self.encoder = MetricalChordEncoder(in_feats + 128, n_hidden, n_layers, activation=activation, dropout=dropout, use_jk=use_jk,
                                            metrical=metrical, use_reledge=use_reledge, **kwargs)
        if use_nade:
            self.classifier = NadeClassifierLayer(n_hidden, n_hidden, tasks=tasks, n_layers=1, activation=activation, dropout=dropout)
        else:
            self.classifier = MultiTaskMLP(n_hidden, n_hidden, tasks=tasks, n_layers=1, activation=activation, dropout=dropout)

    def encode(self, x, edge_index, edge_type, onset_edges, onset_idx, lengths, **kwargs):
        if self.training:
            fused.advance_rng(x.device)            # a fresh set of dropout masks per training forward (graph-safe: in-stream)
        return self.encoder(x, edge_index, edge_type, onset_edges, onset_idx, lengths=lengths, **kwargs)

    def forward(self, x, edge_index, edge_type, onset_edges, onset_idx, lengths, **kwargs):
        return self.classifier(self.encode(x, edge_index, edge_type, onset_edges, onset_idx, lengths, **kwargs))

    def forward_fused(self, x, edge_index, edge_type, onset_edges, onset_idx, lengths, **kwargs):
        """(logits, offs, tasks) for heads.training_loss / heads.multitask_cross_entropy; MultiTaskMLP heads only."""
        if not isinstance(self.classifier, MultiTaskMLP):
            raise AgnnError("forward_fused: the NADE chain has no side-by-side logits; use forward")
        return self.classifier.forward_fused(self.encode(x, edge_index, edge_type, onset_edges, onset_idx, lengths, **kwargs))


class PostProcessingMLTModel(nn.Module):
    """models/chord.py:751-783: a bidirectional LSTM over the per-task soft-maxes of a prediction model's outputs, `fc`, and one
    Linear head per task.  `forward(x: {task: logits [T, C_t] or [B, T, C_t]})` -> {task: logits}.  The LSTM runs the persistent
    kernels (lstm_seq.py) at n_hidden 64 or 128, the library RNN on the GPU otherwise.  The stages, and what each runs on:
      1. the per-task soft-maxes side by side: T `F.softmax` calls and ONE `torch.cat` (the library has no kernel that writes a
         soft-max into a column block of a wider matrix);
      2. a 2-D input becomes one sequence [1, T, sum C];
      3. `lstm_forward`;
      4. activation(fc(h.squeeze())) — the reference's `squeeze()`, which also drops a batch of one;
      5. `F.normalize`, then dropout on the library's random stream (pitch_spelling._drop);
      6. the heads as ONE product on their stacked weights [sum C, n_hidden], at every width: they all read the same rows, and
         `heads.grouped_projection` gives each group its own column window of the input, so it would need h repeated per task.
    Not here: the Lightning module `PostChordPrediction`."""

    def __init__(self, tasks, n_hidden, n_layers, activation=F.relu, dropout=0.0):
        super().__init__()
        self.tasks = tasks
        self.n_hidden = n_hidden
        self.n_layers = n_layers
        logits_dim = sum(self.tasks.values())
        self.lstm = nn.LSTM(logits_dim, n_hidden, n_layers, batch_first=True, bidirectional=True, dropout=dropout)
        self.fc = nn.Linear(n_hidden * 2, n_hidden)
        self.clf = nn.ModuleDict({task: nn.Linear(n_hidden, n_classes) for task, n_classes in self.tasks.items()})
        self.dropout = nn.Dropout(dropout)
        self.activation = activation

    def forward(self, x):
        from .lstm_seq import lstm_forward
        from .pitch_spelling import _drop
        tasks = list(self.tasks.keys())
        _lib.require_gpu(*[x[t] for t in tasks])
        if self.training and self.dropout.p > 0:
            fused.advance_rng(x[tasks[0]].device)
        h = torch.cat([F.softmax(x[t], dim=-1) for t in tasks], dim=-1)
        if h.dim() == 2:
            h = h.unsqueeze(0)
        h = lstm_forward(self.lstm, h, self.training).squeeze()
        lead = tuple(h.shape[:-1])
        h = self.activation(linear(h.reshape(-1, h.shape[-1]), self.fc.weight, self.fc.bias))
        h = _drop(F.normalize(h, p=2, dim=-1), self.dropout.p, self.training)
        offs = [0]
        for t in tasks:
            offs.append(offs[-1] + self.clf[t].out_features)
        logits = linear(h, _cat_params([self.clf[t].weight for t in tasks]), _cat_params([self.clf[t].bias for t in tasks]))
        logits = logits.view(lead + (offs[-1],))
        return {t: logits[..., offs[i]:offs[i + 1]] for i, t in enumerate(tasks)}

    def predict(self, x):
        out = self.forward({k: v for k, v in x.items() if k in self.tasks.keys()})
        out["onset"] = x["onset"]
        out["s_measure"] = x["s_measure"]
        return out
