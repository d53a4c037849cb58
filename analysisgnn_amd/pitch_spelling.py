"""The reference's pitch-spelling family (models/pitch_spelling.py) on the HIP kernels: `PKSpell`, `HierarchicalHeteroGraphSage`,
`PitchSpellingGNN`, `PitchSpellingNeighborGNN`, and PyG's `GraphNorm`, the one operator of the three that nothing else in the
library expresses (csrc/graphnorm.hip).  Same class names, constructor arguments, parameter names and forward signatures, so a
reference `state_dict` of `module.*` loads by name (`gnn_enc.*` of `PitchSpellingGNN` follows encoders.MetricalGNN, whose build
spec is this library's); `nn.Linear`, `nn.GRU`, `nn.LSTM`, `nn.LayerNorm`, `nn.BatchNorm1d` stay as parameter holders.  Inputs
live on a HIP device; there is no CPU path.

Schedules that differ from the reference's:
  * `GraphNorm` is three launches each way on a per-batch index (`graph_segments`) instead of two scatter-means, two gathers
    and five element-wise passes with a host read of `batch.max()`;
  * the key-signature head reads `[x | out_pc]` without the concatenation: linear(x, W[:, :E], b, acc=linear(out_pc, W[:, E:]));
  * both heads' last layers write their column block of one [N, 35 + 15] matrix, which `forward_fused` returns for
    `pitch_spelling_loss` and `metrics.MultiTaskMetrics`.
Not here: the Lightning modules, their optimizers and schedulers."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib, fused, resident
from ._abi import AgnnError
from .chord import act_norm_drop
from .encoders import HeteroConv, MetricalGNN, TrimPlan, _head, _hop_counts
from .fused import FusedSequential, norm_act
from .graph import SegSpec, build_csr, hetero_index
from .gru import gru_forward
from .heads import multitask_cross_entropy
from .linear import Linear, linear, linear2
from .lstm_seq import lstm_forward


# ---- the per-batch index of GraphNorm ------------------------------------------------------------------------------------------
class GraphSegments:
    """The rows of every graph of a batch, as the kernels read them: `seg_ptr` int32 [G + 1] and `rows` int32 [n] (the rows of
    graph g are rows[seg_ptr[g] : seg_ptr[g + 1]]; one `agnn_csr_build`, so `batch` need not be sorted) and the slab table
    (`agnn_graphnorm_slabs`, one launch pair, here and not per call)."""

    def __init__(self, batch: Optional[torch.Tensor], n: int, G: int, device=None):
        self.n, self.G = int(n), int(G)
        if batch is None:
            dev = torch.device(device)
            self.seg_ptr = torch.tensor([0, self.n], dtype=torch.int32, device=dev)
            self.rows = torch.arange(max(self.n, 1), dtype=torch.int32, device=dev)
        else:
            if batch.dim() != 1 or batch.dtype != torch.int64:
                raise AgnnError(f"graph_segments: batch must be int64 [n], got {tuple(batch.shape)} {batch.dtype}")
            dev = _lib.require_gpu(batch)
            csr = build_csr([SegSpec(batch, torch.arange(self.n, dtype=torch.int64, device=dev), self.G)])[0]
            self.seg_ptr, self.rows = csr.rowptr, csr.col
        lib = _lib.load()
        self.table_bytes = int(lib.agnn_graphnorm_table_bytes(self.n, self.G))
        self.table = torch.empty(max(self.table_bytes // 4, 4), dtype=torch.int32, device=dev)
        if self.n > 0:
            _lib.check(lib.agnn_graphnorm_slabs(self.seg_ptr.data_ptr(), self.n, self.G, self.table.data_ptr(), self.table_bytes,
                                                _lib.stream_ptr(dev)), "agnn_graphnorm_slabs")


_SEG_CACHE: "Dict[tuple, GraphSegments]" = {}
_SEG_CACHE_MAX = 8


def graph_segments(batch: Optional[torch.Tensor], batch_size: Optional[int] = None, n: Optional[int] = None,
                   device=None) -> GraphSegments:
    """Build (or fetch) the index of a batch vector: keyed on the tensor's identity and version, as chord.pool_index is.
    `batch_size` None costs the one host read PyG's GraphNorm makes too (`batch.max()`); an int costs none.  `batch` None: one
    graph of `n` rows on `device`."""
    if batch is None:
        if n is None or device is None:
            raise AgnnError("graph_segments: batch=None needs the row count n and the device")
        key = ("one", int(n), resident.device_index(device))
    else:
        key = (batch.data_ptr(), tuple(batch.shape), batch._version, batch_size, resident.device_index(batch.device))
    hit = _SEG_CACHE.get(key)
    if hit is None:
        if batch is None:
            hit = GraphSegments(None, int(n), 1, device)
        else:
            G = int(batch_size) if batch_size is not None else (int(batch.max()) + 1 if batch.numel() else 0)
            hit = GraphSegments(batch, int(batch.shape[0]), G)
            hit._keepalive = batch
        if len(_SEG_CACHE) >= _SEG_CACHE_MAX:
            _SEG_CACHE.pop(next(iter(_SEG_CACHE)))
        _SEG_CACHE[key] = hit
    return hit


def clear_segment_cache() -> None:
    _SEG_CACHE.clear()


class _GraphNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mean_scale, seg: GraphSegments, eps):
        dev = _lib.require_gpu(x, weight, bias, mean_scale)
        lib = _lib.load()
        x = _lib.rows16(x)
        weight, bias, mean_scale = _lib.vec16(weight), _lib.vec16(bias), _lib.vec16(mean_scale)
        n, C = x.shape
        y = torch.empty((n, C), dtype=torch.float32, device=dev)
        stats = torch.empty((max(seg.G, 1), 3, C), dtype=torch.float32, device=dev)
        if n > 0:
            nws = int(lib.agnn_graphnorm_workspace_bytes(n, seg.G, C))
            ws = resident.scratch(dev, "graphnorm", nws, zeroed=False)
            _lib.check(lib.agnn_graphnorm_fwd_f32(x.data_ptr(), x.stride(0), n, seg.G, C, seg.seg_ptr.data_ptr(), seg.rows.data_ptr(),
                                                  seg.table.data_ptr(), seg.table_bytes, weight.data_ptr(), bias.data_ptr(),
                                                  mean_scale.data_ptr(), float(eps), y.data_ptr(), y.stride(0), stats.data_ptr(),
                                                  ws.data_ptr(), nws, _lib.stream_ptr(dev)), "agnn_graphnorm_fwd_f32")
        ctx.save_for_backward(x, weight, mean_scale, stats)
        ctx.seg = seg
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean_scale, stats = ctx.saved_tensors
        seg: GraphSegments = ctx.seg
        dev = dy.device
        lib = _lib.load()
        dy = _lib.rows16(dy)
        n, C = x.shape
        dx = torch.empty_like(x)
        dw = torch.empty((C,), dtype=torch.float32, device=dev)
        db = torch.empty((C,), dtype=torch.float32, device=dev)
        dms = torch.empty((C,), dtype=torch.float32, device=dev)
        if n > 0:
            nws = int(lib.agnn_graphnorm_workspace_bytes(n, seg.G, C))
            ws = resident.scratch(dev, "graphnorm", nws, zeroed=False)
            _lib.check(lib.agnn_graphnorm_bwd_f32(x.data_ptr(), x.stride(0), n, seg.G, C, seg.seg_ptr.data_ptr(), seg.rows.data_ptr(),
                                                  seg.table.data_ptr(), seg.table_bytes, weight.data_ptr(), mean_scale.data_ptr(),
                                                  stats.data_ptr(), dy.data_ptr(), dy.stride(0), dx.data_ptr(), dx.stride(0), dw.data_ptr(),
                                                  db.data_ptr(), dms.data_ptr(), ws.data_ptr(), nws, _lib.stream_ptr(dev)),
                       "agnn_graphnorm_bwd_f32")
        else:
            dw.zero_()
            db.zero_()
            dms.zero_()
        return dx, dw, db, dms, None, None


def graph_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, mean_scale: torch.Tensor, segments: GraphSegments,
               eps: float = 1e-5) -> torch.Tensor:
    """PyG GraphNorm of x [n, C] (fp32, C % 4 == 0) on `agnn_graphnorm_*`: per graph and column, o = x - mean_scale * mean(x),
    y = weight * o / sqrt(mean(o^2) + eps) + bias.  Differentiable in x and the three parameters."""
    _lib.require_gpu(x)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] % 4 != 0 or x.shape[1] < 4:
        raise AgnnError(f"graph_norm: a [n, C] fp32 matrix with C % 4 == 0 expected, got {tuple(x.shape)} {x.dtype}")
    if segments.n != x.shape[0]:
        raise AgnnError(f"graph_norm: the segments index {segments.n} rows, x has {x.shape[0]}")
    return _GraphNorm.apply(x, weight, bias, mean_scale, segments, float(eps))


class GraphNorm(nn.Module):
    """torch_geometric.nn.GraphNorm(in_channels, eps): the same parameter names and initial values.  `batch` may be a batch
    vector (int64 [n]), a `GraphSegments`, or None (one graph).  Training and evaluation are the same function."""

    def __init__(self, in_channels: int, eps: float = 1e-5):
        super().__init__()
        self.in_channels = in_channels
        self.eps = eps
        self.weight = nn.Parameter(torch.empty(in_channels))
        self.bias = nn.Parameter(torch.empty(in_channels))
        self.mean_scale = nn.Parameter(torch.empty(in_channels))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.ones_(self.weight)
        nn.init.zeros_(self.bias)
        nn.init.ones_(self.mean_scale)

    def forward(self, x, batch=None, batch_size: Optional[int] = None):
        seg = batch if isinstance(batch, GraphSegments) else graph_segments(batch, batch_size, n=x.shape[0], device=x.device)
        return graph_norm(x, self.weight, self.bias, self.mean_scale, seg, self.eps)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels})"


# ---- padded sequences -------------------------------------------------------------------------------------------------------------
def _pad(x: torch.Tensor, lens: Sequence[int]) -> torch.Tensor:
    """[sum lens, F] -> [B, max len, F] with zeros behind every sequence (the reference pads, it does not pack)."""
    if len(set(lens)) == 1:
        return x.view(len(lens), lens[0], x.shape[1])
    return nn.utils.rnn.pad_sequence(x.split(list(lens)), batch_first=True)


def _unpad(y: torch.Tensor, lens: Sequence[int]) -> torch.Tensor:
    if len(set(lens)) == 1:
        return y.reshape(-1, y.shape[-1])
    return torch.cat([y[i, :l] for i, l in enumerate(lens)], dim=0)


def _rnn(rnn: nn.Module, x: torch.Tensor, training: bool) -> torch.Tensor:
    """The persistent GRU / LSTM kernels where they are built (bidirectional, 64 or 128 per direction), the library RNN on the GPU
    otherwise (unidirectional cells, other widths)."""
    if isinstance(rnn, nn.GRU):
        return gru_forward(rnn, x, training)
    return lstm_forward(rnn, x, training) if isinstance(rnn, nn.LSTM) else rnn(x)[0]


def _drop(x: torch.Tensor, p: float, training: bool) -> torch.Tensor:
    """Dropout on the library's random stream (agnn_skip_act_*: no skip, no activation)."""
    if not training or p <= 0:
        return x
    return fused.skip_act(x.reshape(-1, x.shape[-1]), None, None, False, p, True).view(x.shape)


class PKSpell(nn.Module):
    """models/pitch_spelling.py:50-151: two stacked bidirectional RNNs on padded sentences, dropout, two top layers.
    `forward(sentences [sum len, in_feats], sentences_len)` -> padded ([B, T, out_feats], [B, T, 15]).  Either `cell_type` with
    n_hidden // 2 of 64 or 128 runs its persistent kernels (gru.py, lstm_seq.py); `bidirectional=False` and every other width
    run the library RNN on the GPU.  Two defects of the reference have working equivalents here: `predict`
    returns the first l entries of row i (the reference indexes `[:l, i]` on a batch-first tensor), and `loss_computation` uses
    `out_feats`, 15 and the constructor's `ignore_index` values (the reference reads attributes that do not exist)."""

    def __init__(self, in_feats, n_hidden1, n_hidden2, out_feats, rnn_depth=1, dropout=0.5, cell_type="GRU", bidirectional=True,
                 mode="both"):
        super().__init__()
        if n_hidden1 % 2 != 0:
            raise ValueError("Hidden_dim must be an even integer")
        if n_hidden2 % 2 != 0:
            raise ValueError("Hidden_dim2 must be an even integer")
        self.n_hidden1 = n_hidden1
        self.n_hidden2 = n_hidden2
        self.out_feats = out_feats
        if cell_type == "GRU":
            rnn_cell = nn.GRU
        elif cell_type == "LSTM":
            rnn_cell = nn.LSTM
        else:
            raise ValueError(f"Unknown RNN cell type: {cell_type}")
        self.rnn = rnn_cell(input_size=in_feats, hidden_size=n_hidden1 // 2 if bidirectional else n_hidden1,
                            bidirectional=bidirectional, num_layers=rnn_depth, batch_first=True)
        self.rnn2 = rnn_cell(input_size=n_hidden1, hidden_size=n_hidden2 // 2 if bidirectional else n_hidden2,
                             bidirectional=bidirectional, num_layers=rnn_depth, batch_first=True)
        self.dropout = nn.Dropout(dropout)
        self.top_layer_pitch = Linear(n_hidden1, out_feats)
        self.top_layer_ks = Linear(n_hidden2, 15)
        self.loss_pitch = nn.CrossEntropyLoss(reduction="mean", ignore_index=out_feats)
        self.loss_ks = nn.CrossEntropyLoss(reduction="mean", ignore_index=15)
        self.mode = mode

    def forward(self, sentences, sentences_len):
        _lib.require_gpu(sentences)
        lens = [int(v) for v in (sentences_len.tolist() if torch.is_tensor(sentences_len) else sentences_len)]
        if self.training and self.dropout.p > 0:
            fused.advance_rng(sentences.device)
        x = _pad(sentences, lens)
        h = _drop(_rnn(self.rnn, x, self.training), self.dropout.p, self.training)
        out_pitch = self.top_layer_pitch(h)
        h = _drop(_rnn(self.rnn2, h, self.training), self.dropout.p, self.training)
        out_ks = self.top_layer_ks(h)
        return out_pitch, out_ks

    def predict(self, sentences, sentences_len):
        scores_pitch, scores_ks = self.forward(sentences, sentences_len)
        predicted_pitch = scores_pitch.argmax(dim=2)
        predicted_ks = scores_ks.argmax(dim=2)
        return ([predicted_pitch[i, :int(l)].cpu().numpy() for i, l in enumerate(sentences_len)],
                [predicted_ks[i, :int(l)].cpu().numpy() for i, l in enumerate(sentences_len)])

    def loss_computation(self, pred_pitch, pred_ks, true_pitch, true_ks):
        scores_pitch = pred_pitch.reshape(-1, self.out_feats)
        scores_ks = pred_ks.reshape(-1, 15)
        pitches = true_pitch.reshape(-1)
        keysignatures = true_ks.reshape(-1)
        if self.mode == "both":
            return self.loss_pitch(scores_pitch, pitches) + self.loss_ks(scores_ks, keysignatures)
        if self.mode == "ks":
            return self.loss_ks(scores_ks, keysignatures)
        return self.loss_pitch(scores_pitch, pitches)


# ---- the graph models -------------------------------------------------------------------------------------------------------------
class HierarchicalHeteroGraphSage(nn.Module):
    """models/pitch_spelling.py:13-47: HeteroConv{SAGEConv}(aggr='sum') layers with trim_to_layer, ReLU after EVERY layer, no
    LayerNorm (unlike encoders.HeteroSAGEStack), then `lin` on the note rows."""

    def __init__(self, edge_types, input_channels, hidden_channels, out_channels, num_layers):
        super().__init__()
        self.num_layers = num_layers
        self.convs = nn.ModuleList()
        for i in range(num_layers):
            self.convs.append(HeteroConv(edge_types, input_channels if i == 0 else hidden_channels, hidden_channels, "sum"))
        self.lin = nn.Linear(hidden_channels, out_channels)

    def _run(self, x_dict, edge_index_dict, num_sampled_edges_dict, num_sampled_nodes_dict):
        """(lin(x_note), the COO prefixes the last layer keeps: what its trim_to_layer leaves of every edge list)."""
        _lib.require_gpu(*x_dict.values())
        plan = TrimPlan(self.num_layers, x_dict, edge_index_dict, num_sampled_nodes_dict, num_sampled_edges_dict)
        index = hetero_index(edge_index_dict, {k: int(v.shape[0]) for k, v in x_dict.items()})
        index.prepare_trim(plan.e_keep)
        for i, conv in enumerate(self.convs):
            x_dict = conv(dict(x_dict), edge_index_dict, index, plan.n_keep[i], plan.e_keep[i])
            x_dict = {k: v.relu() for k, v in x_dict.items()}
        return linear(x_dict["note"], self.lin.weight, self.lin.bias), plan.e_keep[-1]

    def forward(self, x_dict, edge_index_dict, num_sampled_edges_dict=None, num_sampled_nodes_dict=None):
        return self._run(x_dict, edge_index_dict, num_sampled_edges_dict, num_sampled_nodes_dict)[0]


def _heads(enc: int, pc: int, ks: int, dropout: float):
    def body(n_in, n_out):
        return FusedSequential(Linear(n_in, enc // 2), nn.ReLU(), nn.LayerNorm(enc // 2), nn.Dropout(dropout), Linear(enc // 2, n_out))
    return body(enc, pc), body(enc + pc, ks)


class _SideBySide(torch.autograd.Function):
    """The [N, pc + ks] matrix that the two heads' last layers wrote their column blocks of (`_TwoHeads._tail`): nothing is
    launched, backward hands each head its columns of the gradient as views."""

    @staticmethod
    def forward(ctx, out_pc, out_ks, buf):
        ctx.split = out_pc.shape[1]
        return buf

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.split], g[:, ctx.split:], None


class _TwoHeads:
    """`mlp_clf_pc(x)` and `mlp_clf_ks(.)` of both graph models.  Each head's last layer writes its column block of ONE
    [N, pc + ks] matrix (rows padded to a multiple of 4 floats): `out_pc` is the first block, read there by whatever follows
    it, `forward_fused` returns the matrix itself and `forward` the two blocks; nothing is concatenated."""

    def _logit_buffer(self, x):
        width = self.mlp_clf_pc[-1].out_features + self.mlp_clf_ks[-1].out_features
        return torch.empty((x.shape[0], (width + 3) & ~3), dtype=torch.float32, device=x.device)

    @staticmethod
    def _columns(buf, c0, c1):
        """Columns [c0, c1) of `buf` as a tensor of its own on the same memory (not a view in autograd's books: the blocks are
        written one after the other, and a view would count the later write as a change of the earlier block)."""
        return torch.empty(0, dtype=buf.dtype, device=buf.device).set_(buf.untyped_storage(), buf.storage_offset() + c0,
                                                                         (buf.shape[0], c1 - c0), (buf.stride(0), 1))

    def _tail(self, seq, a, block):
        """ReLU -> LayerNorm -> Dropout -> Linear of a head on its first layer's product `a`, the result written into `block`."""
        _, _, ln, drop, last = list(seq)
        h = norm_act(a, ln, pre_relu=True, p=drop.p, training=self.training)
        with torch.no_grad():
            torch.addmm(last.bias, h, last.weight.t(), out=block)
        return linear(h, last.weight, last.bias, pre=[block])

    def _pc_head(self, x, buf):
        first = self.mlp_clf_pc[0]
        return self._tail(self.mlp_clf_pc, linear(x, first.weight, first.bias), self._columns(buf, 0, self.mlp_clf_pc[-1].out_features))

    def _ks_head(self, a, buf):
        pc = self.mlp_clf_pc[-1].out_features
        return self._tail(self.mlp_clf_ks, a, self._columns(buf, pc, pc + self.mlp_clf_ks[-1].out_features))

    def _both(self, x):
        """(out_pc, out_ks, their matrix) with mlp_clf_ks(cat[x, out_pc]) computed without the concatenation: the first layer's
        product split at the seam, the second half handed to the first as its accumulator."""
        buf = self._logit_buffer(x)
        out_pc = self._pc_head(x, buf)
        first, E = self.mlp_clf_ks[0], x.shape[1]
        a = linear(x, first.weight[:, :E], first.bias, acc=linear(out_pc, first.weight[:, E:]))
        return out_pc, self._ks_head(a, buf), buf

    @classmethod
    def _fused(cls, out_pc, out_ks, buf) -> Tuple[torch.Tensor, List[int]]:
        offs = [0, out_pc.shape[1], out_pc.shape[1] + out_ks.shape[1]]
        buf = cls._columns(buf, 0, offs[-1])
        if torch.is_grad_enabled() and (out_pc.requires_grad or out_ks.requires_grad):
            return _SideBySide.apply(out_pc, out_ks, buf), offs
        return buf, offs


class PitchSpellingNeighborGNN(nn.Module, _TwoHeads):
    """models/pitch_spelling.py:239-266: the SAGE stack, BatchNorm1d (through chord.act_norm_drop: identity activation, no
    dropout), the two heads.  Per-hop count lists (or hop-index tensors) trim the layers as PyG's trim_to_layer does."""

    def __init__(self, in_feats, n_hidden, out_feats_enc, out_feats_pc, out_feats_ks, n_layers, metadata, dropout=0.5):
        super().__init__()
        self.gnn_enc = HierarchicalHeteroGraphSage(metadata[1], in_feats, n_hidden, out_feats_enc, n_layers)
        self.normalize = nn.BatchNorm1d(out_feats_enc)
        self.mlp_clf_pc, self.mlp_clf_ks = _heads(out_feats_enc, out_feats_pc, out_feats_ks, dropout)

    def _encode(self, x_dict, edge_index_dict, num_sampled_edges_dict, num_sampled_nodes_dict):
        if self.training:
            fused.advance_rng(x_dict["note"].device)
        x = self.gnn_enc(x_dict, edge_index_dict, num_sampled_edges_dict, num_sampled_nodes_dict)
        return act_norm_drop(x, self.normalize, None, 0.0, self.training)

    def forward(self, x_dict, edge_index_dict, num_sampled_edges_dict=None, num_sampled_nodes_dict=None):
        return self._both(self._encode(x_dict, edge_index_dict, num_sampled_edges_dict, num_sampled_nodes_dict))[:2]

    def forward_fused(self, x_dict, edge_index_dict, num_sampled_edges_dict=None, num_sampled_nodes_dict=None):
        """([N, out_feats_pc + out_feats_ks] logits side by side, their offsets): the matrix `forward`'s two outputs are blocks of."""
        return self._fused(*self._both(self._encode(x_dict, edge_index_dict, num_sampled_edges_dict, num_sampled_nodes_dict)))


class PitchSpellingGNN(nn.Module, _TwoHeads):
    """models/pitch_spelling.py:154-236: encoders.MetricalGNN (this library's build spec), GraphNorm over the target notes'
    graphs, the two heads; with `add_seq=True` two padded bi-GRU branches (`rnn` on the raw target-note inputs, `rnn_ks` on
    `[x | out_pc]`).  The targets are the first rows: `bincount(neighbor_mask_node["note"])[0]` of them for hop-index tensors,
    the first entry of a per-hop count list, every note without masks.  `batch` is the TARGET notes' batch vector (or a
    `GraphSegments`).  `lengths=` (host ints, the targets per graph) spares the one `bincount(batch).tolist()` host read per
    forward that the sequence branches otherwise make, as the reference does; without it the forward cannot be captured."""

    def __init__(self, in_feats, n_hidden, out_feats_enc, out_feats_pc, out_feats_ks, n_layers, metadata, dropout=0.5, add_seq=False):
        super().__init__()
        self.gnn_enc = MetricalGNN(in_feats, n_hidden, out_feats_enc, n_layers, metadata, dropout=dropout)
        self.normalize = GraphNorm(out_feats_enc)
        self.add_seq = add_seq
        if add_seq:
            self.rnn = nn.GRU(input_size=in_feats, hidden_size=n_hidden // 2, bidirectional=True, num_layers=1, batch_first=True)
            self.rnn_norm = nn.LayerNorm(n_hidden)
            self.rnn_project = nn.Linear(n_hidden, out_feats_enc)
            self.cat_lin = nn.Linear(out_feats_enc * 2, out_feats_enc)
            self.rnn_ks = nn.GRU(input_size=out_feats_enc + out_feats_pc, hidden_size=n_hidden // 2, bidirectional=True, num_layers=1,
                                 batch_first=True)
            self.rnn_norm_ks = nn.LayerNorm(n_hidden)
            self.rnn_project_ks = nn.Linear(n_hidden, out_feats_enc + out_feats_pc)
        self.mlp_clf_pc, self.mlp_clf_ks = _heads(out_feats_enc, out_feats_pc, out_feats_ks, dropout)

    def _sequence(self, rnn, norm, project, z, lens):
        y = gru_forward(rnn, _pad(z, lens), self.training)
        y = norm_act(y, norm, training=self.training)
        return _unpad(linear(y, project.weight, project.bias), lens)

    def sequential_forward(self, note, lens):
        return self._sequence(self.rnn, self.rnn_norm, self.rnn_project, note, lens)

    def sequential_ks_forward(self, x, lens):
        return self._sequence(self.rnn_ks, self.rnn_norm_ks, self.rnn_project_ks, x, lens)

    def _run(self, x_dict, edge_index_dict, neighbor_mask_node, neighbor_mask_edge, batch, lengths):
        note = x_dict["note"]
        _lib.require_gpu(note)
        if self.training:
            fused.advance_rng(note.device)
        n_t = int(note.shape[0])
        if neighbor_mask_node is not None and "note" in neighbor_mask_node:
            n_t = _hop_counts(neighbor_mask_node, ["note"], self.gnn_enc.num_layers)["note"][0]
        x = self.gnn_enc(x_dict, edge_index_dict, neighbor_mask_node, neighbor_mask_edge, batch_size=n_t)
        x = self.normalize(x, batch=batch)
        if not self.add_seq:
            return self._both(x)
        if lengths is not None:
            lens = [int(v) for v in lengths]
        elif isinstance(batch, GraphSegments) or batch is None:
            lens = [n_t] if batch is None else (batch.seg_ptr[1:] - batch.seg_ptr[:-1]).tolist()
        else:
            lens = torch.bincount(batch).tolist()                  # the reference's host read (models/pitch_spelling.py:199-200)
        if sum(lens) != n_t:
            raise AgnnError(f"PitchSpellingGNN: lengths {lens} do not add up to the {n_t} target notes")
        z = self.sequential_forward(_head(note, n_t), lens)
        w = self.cat_lin.weight
        E = x.shape[1]
        y = linear2(x, z, w, self.cat_lin.bias)
        x = y if y is not None else linear(x, w[:, :E], self.cat_lin.bias, acc=linear(z, w[:, E:]))
        buf = self._logit_buffer(x)
        out_pc = self._pc_head(x, buf)
        xk = self.sequential_ks_forward(torch.cat((x, out_pc), dim=-1), lens)          # the GRU's input: this concatenation is made
        first = self.mlp_clf_ks[0]
        return out_pc, self._ks_head(linear(xk, first.weight, first.bias), buf), buf

    def forward(self, x_dict, edge_index_dict, neighbor_mask_node=None, neighbor_mask_edge=None, batch=None, lengths=None):
        return self._run(x_dict, edge_index_dict, neighbor_mask_node, neighbor_mask_edge, batch, lengths)[:2]

    def forward_fused(self, x_dict, edge_index_dict, neighbor_mask_node=None, neighbor_mask_edge=None, batch=None, lengths=None):
        """([N, out_feats_pc + out_feats_ks] logits side by side, their offsets): the matrix `forward`'s two outputs are blocks of."""
        return self._fused(*self._run(x_dict, edge_index_dict, neighbor_mask_node, neighbor_mask_edge, batch, lengths))


def pitch_spelling_loss(logits: torch.Tensor, offs: Sequence[int], labels: torch.Tensor) -> torch.Tensor:
    """loss_ps + loss_ks of the reference's Lightning modules (models/pitch_spelling.py:399-403): two mean cross entropies
    without label smoothing, on the side-by-side logits of `forward_fused`; labels int64 [2, N], -1 for a row to ignore."""
    return multitask_cross_entropy(logits, list(offs), labels, label_smoothing=0.0, ignore_index=-1).sum()
