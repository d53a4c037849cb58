"""HGT path: `HGTConv` with PyG (>= 2.3) parameter names and semantics, the
layer stack, and the `HybridHGT` encoder the reference constructs at
analysisgnn/models/analysis.py:445-453 (`heads=4`).  The per-edge work (scores, edge softmax over all
incoming relations, weighted sum, and their gradients) runs on the C-ABI kernels
`agnn_hgt_attn_*`, the per-(relation, head) D x D transforms on `agnn_relt_*` (every head width in
`HEAD_WIDTHS`), the per-type K/Q/V and output projections on `linear`.  Build-spec notes
(parity unpinned vs graphmuse): encoders.py header."""
from __future__ import annotations

import contextlib
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, resident
from .encoders import TrimPlan, _HybridMixin
from .graph import HeteroIndex, hetero_index
from .fused import skip_act
from .linear import all_steal, defer, deferring, leaf_refs, linear
from .params import cat_rows, pack

EdgeType = Tuple[str, str, str]


class _DictLinear(nn.Module):
    """`HeteroDictLinear`: one Linear per node type, parameters under `lins.<type>`."""

    def __init__(self, in_channels, out_channels, types: Sequence[str]):
        super().__init__()
        self.lins = nn.ModuleDict({t: nn.Linear(in_channels, out_channels) for t in types})

    def forward(self, x_dict):
        return {k: self.lins[k](v) for k, v in x_dict.items() if k in self.lins}


class _RelWeight(nn.Module):
    """`HeteroLinear(D, D, num_types=heads*edge_types, bias=False)`: weight [T, D, D], y = x @ W[type]."""

    def __init__(self, num_types, dim):
        super().__init__()
        bound = 1.0 / math.sqrt(dim)
        self.weight = nn.Parameter(torch.empty(num_types, dim, dim).uniform_(-bound, bound))


def _index_tensor(ids: tuple, device) -> torch.Tensor:
    return resident.value(device, ("index table", ids), lambda: torch.tensor(list(ids), device=device))


HEAD_WIDTHS = (4, 8, 16, 32, 64, 128, 256)    # the head widths D the attention (csrc/hgt.hip) and relation-transform (csrc/relt.hip) kernels take
ATTN_ONE_LAUNCH = True  # A/B switch (bench.py --set hgt.ATTN_ONE_LAUNCH=False): the destination types' forward attention in one launch
TYPE_STREAMS = True   # A/B switch (bench.py --set hgt.TYPE_STREAMS=False): the small node types' projections on a second stream


def _relt(op: str, items, R: int, heads: int, D: int, dev) -> None:
    """The per-(relation, head) D x D relation transforms of one source type, written in place for both (a, b, y) of `items`
    (K and V); block (r, h) is columns (r*heads + h)*D .. +D of an [N, R*H] operand, columns h*D .. +D of an [N, H] one:
      fwd  y_rh = a_h @ b[r*heads + h]                  a = x [N, H], b = weight blocks [R*heads, D, D], y = x' [N, R*H]
      bwd  y_h = sum_r a_rh @ b[r*heads + h]            a = dx' [N, R*H], b = TRANSPOSED weight blocks, y = dx [N, H]
      dw   y[r*heads + h] = a_h^T @ b_rh                a = x [N, H], b = dx' [N, R*H], y = weight-block gradients [R*heads, D, D]
    One `agnn_relt_<op>_f32` launch at every head width in HEAD_WIDTHS (csrc/relt.hip: VALU kernels at D = 4, 8, one MFMA tile per
    block at D = 16, 32, the 32x32x2 fp32 MFMA pipeline at D = 64 and, tiled over D, at 128 and 256); any other D is an error."""
    N = items[0][0].shape[0]
    lib = _lib.load()
    arr = (_lib.ReltItem * 2)()
    for it, (a, b, y) in zip(arr, items):
        it.x, it.w, it.y, it.ld_x, it.ld_y = a.data_ptr(), b.data_ptr(), y.data_ptr(), a.stride(0), (b if op == "dw" else y).stride(0)
    if op == "dw":
        nws = int(lib.agnn_relt_dw_workspace_bytes(2, R, heads, D, N))
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
        _lib.check(lib.agnn_relt_dw_f32(2, arr, R, heads, D, N, ws.data_ptr(), nws, _lib.stream_ptr(dev)), "agnn_relt_dw_f32")
    else:
        fn = lib.agnn_relt_fwd_f32 if op == "fwd" else lib.agnn_relt_bwd_f32
        _lib.check(fn(2, arr, R, heads, D, N, _lib.stream_ptr(dev)), f"agnn_relt_{op}_f32")


def attention_forward(rels, q: torch.Tensor, out: torch.Tensor, m: torch.Tensor, linv: torch.Tensor, heads: int) -> None:
    """One `k_hgt_fwd` launch (`agnn_hgt_attn_fwd_f32`): the edge-softmax attention of the out.shape[0] rows of one destination
    type over the relations of the `_lib.HgtRel` table `rels`.  q [n, H] (a column view is fine), out [n, H]; m / linv [n, heads]
    receive the softmax statistics the backward pass reads."""
    n, H = out.shape
    _lib.check(_lib.load().agnn_hgt_attn_fwd_f32(len(rels), rels, q.data_ptr(), q.stride(0), n, H, heads, out.data_ptr(), out.stride(0),
                                                 m.data_ptr(), linv.data_ptr(), _lib.stream_ptr(out.device)), "agnn_hgt_attn_fwd_f32")


class _CorePlan:
    """Static layout of one HGTConv layer on one batch (nothing that carries a gradient)."""

    def __init__(self, types, n_of, heads, D, src_rels, dst_rels, block_of, index, e_keep, n_edge_types):
        self.types, self.n_of, self.heads, self.D = types, n_of, heads, D
        self.src_rels, self.dst_rels, self.block_of = src_rels, dst_rels, block_of
        self.index, self.e_keep, self.n_edge_types = index, e_keep, n_edge_types

    def limit(self, et):
        return None if self.e_keep is None else self.e_keep[et]


class _HGTCore(torch.autograd.Function):
    """Everything of an HGTConv layer between the K|Q|V projections and the output projections, for ALL node types at
    once:  kqv[t] [n_t, 3H]  ->  m[t] [n_t, H]  (relation transforms, scores, edge softmax over all incoming relations,
    weighted sum).  One autograd node instead of ~15 per layer, so that every gradient is WRITTEN IN PLACE by a kernel:
      * the attention's source-side pass writes dK' / dV' of a relation straight into its column block of the source type's
        [N_s, R_s*H] gradient (no per-relation tensors, no packing launch, no zero-filled placeholders);
      * the input-gradient relation transform writes dk / dv, and the destination-side pass writes dq, straight into the
        three column blocks of d kqv[t] (no [N, 3H] re-assembly);
      * the 1/sqrt(D) scale of p_rel, the per-relation stacking and the gradient fan-out are one small launch each way."""

    @staticmethod
    def forward(ctx, plan: _CorePlan, wk, wv, p_all, *kqv):
        dev = _lib.require_gpu(wk, wv, p_all, *kqv)
        lib = _lib.load()
        heads, D = plan.heads, plan.D
        H = heads * D
        X = {t: _lib.rows16(x) for t, x in zip(plan.types, kqv)}
        for t, x in X.items():
            if x.shape[1] != 3 * H:
                raise _lib.AgnnError("HGT core: kqv must be [n, 3H]")
        # relation transforms, K and V of one source type in one launch
        kp, vp, Wk, Wv = {}, {}, {}, {}
        for s_t, e_ids in plan.src_rels.items():
            x = X[s_t]
            N, R = x.shape[0], len(e_ids)
            ids = tuple(e * heads + h for e in e_ids for h in range(heads))
            if ids == tuple(range(wk.shape[0])):
                Wk[s_t], Wv[s_t] = _lib.vec16(wk.detach()), _lib.vec16(wv.detach())      # every relation leaves this type, in order: no gather
            else:
                sel = _index_tensor(ids, dev)
                Wk[s_t], Wv[s_t] = wk.detach().index_select(0, sel), wv.detach().index_select(0, sel)
            kp[s_t] = torch.empty((N, R * H), dtype=torch.float32, device=dev)
            vp[s_t] = torch.empty((N, R * H), dtype=torch.float32, device=dev)
            if N > 0:
                _relt("fwd", ((x[:, :H], Wk[s_t], kp[s_t]), (x[:, 2 * H:], Wv[s_t], vp[s_t])), R, heads, D, dev)
        ps = (p_all.detach() * (1.0 / math.sqrt(D))).contiguous()                   # [n_edge_types, heads]
        outs, stats = [], {}
        live = [t for t in plan.types if plan.dst_rels.get(t) and plan.n_of[t] > 0]
        one_launch = (ATTN_ONE_LAUNCH and 1 < len(live) <= _lib.HGT_MAX_DST
                      and sum(len(plan.dst_rels[t]) for t in live) <= _lib.MAX_SEG)
        items = (_lib.HgtDstItem * max(len(live), 1))()
        hold = []                                            # relation tables and row-end vectors: alive until the launch is issued
        for t in plan.types:
            n = plan.n_of[t]
            rels = plan.dst_rels.get(t, [])
            if not rels or n == 0:
                outs.append(torch.zeros((n, H), dtype=torch.float32, device=dev))
                continue
            out = torch.empty((n, H), dtype=torch.float32, device=dev)
            m = torch.empty((n, heads), dtype=torch.float32, device=dev)
            linv = torch.empty((n, heads), dtype=torch.float32, device=dev)
            arr, keep = _HGTCore._rel_table(plan, rels, kp, vp, ps, H)
            q = X[t]
            if one_launch:                               # every destination type's attention in ONE launch (agnn_hgt_attn_fwd_multi_f32)
                it = items[len(hold)]
                it.rels, it.n_rel = _lib.C.cast(arr, _lib.C.c_void_p), len(rels)
                it.q, it.ld_q, it.n_rows = q.data_ptr() + 4 * H, q.stride(0), n
                it.out, it.ld_out, it.m_out, it.linv_out = out.data_ptr(), out.stride(0), m.data_ptr(), linv.data_ptr()
                hold.append((arr, keep))
            else:
                attention_forward(arr, q[:, H:2 * H], out, m, linv, heads)
            stats[t] = (m, linv)
            outs.append(out)
        if one_launch:
            _lib.check(lib.agnn_hgt_attn_fwd_multi_f32(len(hold), items, H, heads, _lib.stream_ptr(dev)), "agnn_hgt_attn_fwd_multi_f32")
        ctx.plan = plan
        ctx.steal_refs = leaf_refs(wk, wv)             # (their gradients may be produced late: see backward)
        ctx.wg_defer = all(t.is_leaf or getattr(t, "_agnn_wgrad_deferrable", False) for t in (wk, wv))
        ctx.srcs = list(plan.src_rels.keys())
        ctx.dsts = list(stats.keys())
        saved = list(X.values()) + [ps]
        for s_t in ctx.srcs:
            saved += [Wk[s_t], Wv[s_t], kp[s_t], vp[s_t]]
        for t in ctx.dsts:
            saved += [stats[t][0], stats[t][1], outs[plan.types.index(t)]]
        ctx.save_for_backward(*saved)
        ctx.shapes = (tuple(wk.shape), tuple(wv.shape), tuple(p_all.shape))
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def _rel_table(plan, rels, kp, vp, ps, H, extra=None):
        arr = (_lib.HgtRel * max(len(rels), 1))()
        keep = []
        for r, (e_idx, et) in enumerate(rels):
            s_t, blk = plan.block_of[e_idx]
            c = plan.index.fwd[et]
            re = c.rowend(plan.limit(et))
            keep.append(re)
            arr[r].k, arr[r].v = kp[s_t].data_ptr() + 4 * blk * H, vp[s_t].data_ptr() + 4 * blk * H
            arr[r].ld = kp[s_t].stride(0)
            arr[r].rowptr, arr[r].rowend = c.rowptr.data_ptr(), _lib.ptr(re)
            arr[r].col, arr[r].perm = c.col.data_ptr(), c.perm.data_ptr()
            arr[r].pscale = ps[e_idx].data_ptr()
            if extra is not None:
                arr[r].alpha, arr[r].gs, arr[r].tdot = (x.data_ptr() for x in extra[r])
        return arr, keep

    @staticmethod
    def backward(ctx, *dms):
        plan: _CorePlan = ctx.plan
        lib = _lib.load()
        heads, D = plan.heads, plan.D
        H = heads * D
        saved = list(ctx.saved_tensors)
        nt = len(plan.types)
        X = dict(zip(plan.types, saved[:nt]))
        ps = saved[nt]
        pos = nt + 1
        Wk, Wv, kp, vp = {}, {}, {}, {}
        for s_t in ctx.srcs:
            Wk[s_t], Wv[s_t], kp[s_t], vp[s_t] = saved[pos:pos + 4]
            pos += 4
        stats = {}
        for t in ctx.dsts:
            stats[t] = tuple(saved[pos:pos + 3])
            pos += 3
        dev = ps.device
        st = _lib.stream_ptr(dev)
        dkqv = {t: torch.empty_like(X[t]) for t in plan.types}
        dkp = {s_t: torch.empty_like(kp[s_t]) for s_t in ctx.srcs}
        dvp = {s_t: torch.empty_like(vp[s_t]) for s_t in ctx.srcs}
        written = set()                                              # relations whose dK' / dV' block a kernel has written
        zero_q = set()                                               # types whose dq is structurally zero
        dps_rows, dps_ids = [], []
        keep_alive = []                      # row-end tensors referenced by a launch table until the launch is issued
        for ti, t in enumerate(plan.types):
            dm = dms[ti]
            n = plan.n_of[t]
            rels = plan.dst_rels.get(t, [])
            if t not in stats or dm is None:                         # no incoming relation / output not used downstream: dq = 0
                zero_q.add(t)
                continue
            dm = _lib.rows16(dm)
            m, linv, out = stats[t]
            q = X[t]
            R = len(rels)
            ne = [max(plan.index.num_edges[et], 1) for _, et in rels]
            offs = [0]
            for k_ in ne:
                offs.append(offs[-1] + k_)
            a_all = torch.empty((offs[-1], heads), dtype=torch.float32, device=dev)
            g_all = torch.empty((offs[-1], heads), dtype=torch.float32, device=dev)
            # tdot head-major as [R, heads, max E_r] (zero padded): the sums over the edges are ONE contiguous reduction
            t3 = torch.zeros((R, heads, max(ne)), dtype=torch.float32, device=dev)
            extra = [(a_all[offs[r]:offs[r + 1]], g_all[offs[r]:offs[r + 1]], t3[r]) for r in range(R)]
            arr, keep = _HGTCore._rel_table(plan, rels, kp, vp, ps, H, extra)
            for r in range(R):
                arr[r].ld_tdot = max(ne)
            dq_ptr = dkqv[t].data_ptr() + 4 * H
            _lib.check(lib.agnn_hgt_attn_bwd_dst_f32(R, arr, q.data_ptr() + 4 * H, q.stride(0), dm.data_ptr(), dm.stride(0), out.data_ptr(),
                                                     out.stride(0), m.data_ptr(), linv.data_ptr(), n, H, heads, dq_ptr, dkqv[t].stride(0), st),
                       "agnn_hgt_attn_bwd_dst_f32")
            dps_rows.append(t3.sum(dim=2))
            dps_ids += [e_idx for e_idx, _ in rels]
            src_items = (_lib.HgtSrcItem * len(rels))()
            n_items = 0
            for r, (e_idx, et) in enumerate(rels):
                s_t, blk = plan.block_of[e_idx]
                c = plan.index.bwd[et]
                n_src = X[s_t].shape[0]
                re = c.rowend(plan.limit(et))
                lim = n if plan.index.fwd[et].n_rows > n else _lib.INT32_MAX
                if n_src > 0:
                    it = src_items[n_items]
                    n_items += 1
                    it.rowptr, it.rowend, it.col, it.perm = c.rowptr.data_ptr(), _lib.ptr(re), c.col.data_ptr(), c.perm.data_ptr()
                    it.alpha, it.gs = extra[r][0].data_ptr(), extra[r][1].data_ptr()
                    it.dk, it.dv = dkp[s_t].data_ptr() + 4 * blk * H, dvp[s_t].data_ptr() + 4 * blk * H
                    it.ld_o, it.n_src_rows, it.col_limit = dkp[s_t].stride(0), n_src, lim
                    keep_alive.append(re)
                written.add(e_idx)
            if n_items:                                   # every relation that ends in this type: one launch
                _lib.check(lib.agnn_hgt_attn_bwd_src_batch_f32(n_items, src_items, q.data_ptr() + 4 * H, q.stride(0), dm.data_ptr(), dm.stride(0),
                                                               H, heads, st), "agnn_hgt_attn_bwd_src_batch_f32")
        gwk = gwv = None
        wk_shape, wv_shape, p_shape = ctx.shapes
        later = ctx.wg_defer and dev.type == "cuda" and deferring(next(iter(X.values()))) and all_steal(ctx.steal_refs)
        # column blocks that no kernel writes (a type without live outgoing relations, a relation trimmed to nothing, a type whose
        # own output is unused) are cleared in ONE launch (pack with no sources); as `.zero_()` calls they were six ~6 us launches
        # per layer on the stack's backward chain
        clears = []
        for s_t in plan.types:
            live_src = s_t in kp and any(e_idx in written for e_idx in plan.src_rels[s_t])
            if not live_src:
                if s_t not in zero_q:
                    clears += [dkqv[s_t][:, :H], dkqv[s_t][:, 2 * H:]]          # no (live) outgoing relation: dk = dv = 0
                continue
            if s_t in zero_q:
                clears.append(dkqv[s_t][:, H:2 * H])
            for blk, e_idx in enumerate(plan.src_rels[s_t]):
                if e_idx not in written:
                    clears += [dkp[s_t][:, blk * H:(blk + 1) * H], dvp[s_t][:, blk * H:(blk + 1) * H]]
        clears = [c for c in clears if c.numel() > 0]
        if clears:
            pack([(c, []) for c in clears], dev)
        dead = set()                                                 # types whose whole d kqv is structurally zero: hand back None,
        for s_t in plan.types:                                       # so that autograd prunes everything upstream of it
            x = X[s_t]
            N = x.shape[0]
            live_src = s_t in kp and any(e_idx in written for e_idx in plan.src_rels[s_t])
            if not live_src:
                if s_t in zero_q:
                    dead.add(s_t)
                continue
            e_ids = plan.src_rels[s_t]
            R = len(e_ids)
            dx = dkqv[s_t]
            if N > 0:
                Wkt, Wvt = Wk[s_t].transpose(1, 2).contiguous(), Wv[s_t].transpose(1, 2).contiguous()
                _relt("bwd", ((dkp[s_t], Wkt, dx[:, :H]), (dvp[s_t], Wvt, dx[:, 2 * H:])), R, heads, D, dev)
            # The relation weights' gradients only feed the optimizer: with dp.defer_weight_grads they leave the stack's backward
            # chain (95 us per layer at C3, between the input-gradient transform and the next layer's backward) and run at the
            # stream's flush.  The closure works on aliases (a second reference to the returned gradient would make
            # AccumulateGrad clone it before it is computed: see linear._LinearFn.backward).
            dWk, dWv = torch.empty_like(Wk[s_t]), torch.empty_like(Wv[s_t])
            ids = tuple(e * heads + h for e in e_ids for h in range(heads))
            whole = gwk is None and ids == tuple(range(wk_shape[0])) and len(ctx.srcs) == 1
            if whole:
                gwk, gwv = dWk, dWv                                  # the one source type covers the whole parameter
            elif gwk is None:
                gwk = torch.zeros(wk_shape, dtype=torch.float32, device=dev)
                gwv = torch.zeros(wv_shape, dtype=torch.float32, device=dev)

            def weight_grads(x=x, dk_=dkp[s_t], dv_=dvp[s_t], dWk=dWk.detach(), dWv=dWv.detach(), R=R, ids=ids, whole=whole,
                             gk=gwk.detach(), gv=gwv.detach()):
                _relt("dw", ((x[:, :H], dk_, dWk), (x[:, 2 * H:], dv_, dWv)), R, heads, D, dev)
                if not whole:
                    sel = _index_tensor(ids, dev)
                    gk.index_copy_(0, sel, dWk)
                    gv.index_copy_(0, sel, dWv)

            if later:
                defer(weight_grads, dev)
            else:
                weight_grads()
        if dps_rows and tuple(dps_ids) == tuple(range(p_shape[0])):
            dp_all = (torch.cat(dps_rows, dim=0) * (1.0 / math.sqrt(D))).view(p_shape)
        else:
            dp_all = torch.zeros(p_shape, dtype=torch.float32, device=dev)
            if dps_rows:
                dp_all.index_copy_(0, _index_tensor(tuple(dps_ids), dev), torch.cat(dps_rows, dim=0) * (1.0 / math.sqrt(D)))
        if gwk is None:      # no live source type this step: still parameters of the step — zero gradients, as the SAGE path hands out
            gwk = torch.zeros(wk_shape, dtype=torch.float32, device=dev)
            gwv = torch.zeros(wv_shape, dtype=torch.float32, device=dev)
        # A structurally dead node type (no live outgoing relation, its own output unused) gets None: autograd prunes its
        # whole upstream.  PyG's HGTConv routes those parameters through empty index ops and they receive ZERO gradients;
        # dp.FlatGradBuffer.pack substitutes zeros, a stock torch optimizer needs dp.fill_missing_grads(model) first.
        return (None, gwk, gwv, dp_all, *[None if t in dead else dkqv[t] for t in plan.types])


class HGTConv(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, metadata, heads: int = 1):
        super().__init__()
        if out_channels % heads:
            raise ValueError("out_channels must be divisible by heads")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.node_types = list(metadata[0])
        self.edge_types = [tuple(e) for e in metadata[1]]
        D = out_channels // heads
        self.kqv_lin = _DictLinear(in_channels, out_channels * 3, self.node_types)
        self.out_lin = _DictLinear(out_channels, out_channels, self.node_types)
        self.k_rel = _RelWeight(heads * len(self.edge_types), D)
        self.v_rel = _RelWeight(heads * len(self.edge_types), D)
        self.skip = nn.ParameterDict({t: nn.Parameter(torch.ones(1)) for t in self.node_types})
        self.p_rel = nn.ParameterDict({"__".join(e): nn.Parameter(torch.ones(1, heads)) for e in self.edge_types})

    def forward(self, x_dict, edge_index_dict, index: Optional[HeteroIndex] = None,
                n_keep: Optional[Dict[str, int]] = None, e_keep: Optional[Dict[EdgeType, Optional[int]]] = None, post=None):
        """`post` = (relu, dropout p, training) or None: the activation the caller would apply to every output right after this
        layer (HeteroHGTStack between layers) — folded into the layer's epilogue launch; None: the plain HGTConv output."""
        _lib.require_gpu(*x_dict.values())
        D = self.out_channels // self.heads
        if D not in HEAD_WIDTHS or any(x.shape[1] != self.in_channels for x in x_dict.values()):
            raise _lib.AgnnError(f"HGTConv: head width out_channels / heads = {D} must be one of {HEAD_WIDTHS}, and every input "
                                 f"{self.in_channels} features wide (got {[tuple(x.shape) for x in x_dict.values()]})")
        if index is None:
            index = hetero_index(edge_index_dict, {k: int(v.shape[0]) for k, v in x_dict.items()})
        n_of = {t: (n_keep[t] if n_keep is not None else int(x.shape[0])) for t, x in x_dict.items()}
        return self._forward_core(x_dict, index, n_of, e_keep, post)

    def adjacent_parameter_groups(self):
        """The per-relation priors are consumed stacked (one [n_edge_types, heads] operand): adjacent in the flat buffer
        (dp.plan_parameters) the stack is a view."""
        return [[self.p_rel["__".join(e)] for e in self.edge_types]]

    def _forward_core(self, x_dict, index: HeteroIndex, n_of, e_keep, post=None):
        """One K|Q|V GEMM per node type -> `_HGTCore` (one autograd node for the whole message passing) -> one output GEMM
        per node type (+ skip)."""
        heads, H = self.heads, self.out_channels
        D = H // heads
        types = list(x_dict.keys())
        dev = x_dict[types[0]].device
        # The node types' projections are independent of each other, and every type but the largest is small (C3: 16 000 notes,
        # ~2 600 beats, ~700 measures): their kernels are launch-latency bound and, in one stream, sat between the note type's
        # — 130 us per layer of the stack's serial chain.  They run on a second stream beside the note type's kernels.
        big = max(types, key=lambda t: n_of[t])
        two = TYPE_STREAMS and dev.type == "cuda" and len(types) > 1
        main = torch.cuda.current_stream(dev) if two else None
        side = resident.stream(dev, "types") if two else None

        def where(t):
            return torch.cuda.stream(side) if (two and t != big) else contextlib.nullcontext()
        if two:
            side.wait_stream(main)
        kqv = []
        for t in types:
            lin = self.kqv_lin.lins[t]
            x = x_dict[t]
            with where(t):
                if two and t != big:
                    x.record_stream(side)
                kqv.append(linear(x if n_of[t] >= x.shape[0] else x[:n_of[t]], lin.weight, lin.bias))
        if two:
            main.wait_stream(side)
            for t, y in zip(types, kqv):
                if t != big:
                    y.record_stream(main)
        src_rels: Dict[str, List[int]] = {}
        dst_rels: Dict[str, List[Tuple[int, EdgeType]]] = {}
        for e_idx, et in enumerate(self.edge_types):
            s_t, _, d_t = et
            if et in index.fwd and s_t in x_dict and d_t in x_dict:
                src_rels.setdefault(s_t, []).append(e_idx)
                dst_rels.setdefault(d_t, []).append((e_idx, et))
        block_of = {e_idx: (s_t, blk) for s_t, ids in src_rels.items() for blk, e_idx in enumerate(ids)}
        plan = _CorePlan(types, n_of, heads, D, src_rels, dst_rels, block_of, index, e_keep, len(self.edge_types))
        p_all = cat_rows([self.p_rel["__".join(e)] for e in self.edge_types])       # [n_edge_types, heads]
        ms = _HGTCore.apply(plan, self.k_rel.weight, self.v_rel.weight, p_all, *kqv)
        out = {}
        if two:
            side.wait_stream(main)
        for t, m in zip(types, ms):
            x, n = x_dict[t], n_of[t]
            lo = self.out_lin.lins[t]
            with where(t):
                if two and t != big:
                    m.record_stream(side)
                o = linear(F.gelu(m), lo.weight, lo.bias)
                # skip connection (+ the ReLU / dropout the stack puts between layers, when it hands them in): one launch each way
                relu, p, training = post if post is not None else (False, 0.0, False)
                xs = (x if n >= x.shape[0] else x[:n]) if o.shape[-1] == x.shape[-1] else None
                out[t] = skip_act(o, xs, self.skip[t] if xs is not None else None, relu, p, training)
        if two:
            main.wait_stream(side)
            for t in types:
                if t != big:
                    out[t].record_stream(main)
        return out


class HeteroHGTStack(nn.Module):
    def __init__(self, metadata, input_channels, hidden_channels, num_layers, heads=4, dropout=0.5):
        super().__init__()
        self.num_layers, self.dropout = num_layers, dropout
        self.convs = nn.ModuleList([HGTConv(input_channels if i == 0 else hidden_channels, hidden_channels, metadata, heads)
                                    for i in range(num_layers)])

    def forward(self, x_dict, edge_index_dict, plan: TrimPlan, collect: Optional[list] = None):
        index = hetero_index(edge_index_dict, {k: int(v.shape[0]) for k, v in x_dict.items()})
        index.prepare_trim(plan.e_keep)
        self.last_index = index
        for i, conv in enumerate(self.convs):
            post = (True, self.dropout, self.training) if i < self.num_layers - 1 else None
            x_dict = conv(x_dict, edge_index_dict, index, plan.n_keep[i], plan.e_keep[i], post)
            if collect is not None:
                collect.append(x_dict["note"])
        return x_dict


class HybridHGT(nn.Module, _HybridMixin):
    """analysis.py:445-453 constructor (`heads=4`); forward keywords analysis.py:576-579."""

    def __init__(self, metadata, input_channels, hidden_channels, num_layers, heads=4, dropout=0.5, use_jk=False, **kwargs):
        super().__init__()
        self.metadata = (list(metadata[0]), [tuple(e) for e in metadata[1]])
        self.num_layers = num_layers
        self.gnn = HeteroHGTStack(self.metadata, input_channels, hidden_channels, num_layers, heads, dropout)
        self._init_hybrid(input_channels, hidden_channels, num_layers, dropout, use_jk)

    def forward(self, x_dict, edge_index_dict, batch_dict=None, batch_size=None, neighbor_mask_node=None,
                neighbor_mask_edge=None, return_edge_index=False, edge_attr_dict=None):
        _lib.require_gpu(*x_dict.values())
        if batch_size is None:
            batch_size = int(x_dict["note"].shape[0])
        plan = TrimPlan(self.num_layers, x_dict, edge_index_dict, neighbor_mask_node, neighbor_mask_edge)
        outs: list = []
        z, side, gnn_note = self._start_branch(x_dict["note"], batch_dict, batch_size)
        h = self.gnn(self._gnn_input(x_dict, gnn_note), edge_index_dict, plan, outs)
        out = self._finish(h["note"], outs, z, side, batch_size)
        return (out, edge_index_dict) if return_edge_index else out


def attention_roofline_case(g, I, hid: int, dev, timed, hbm_peak: float, heads: int = 4) -> dict:
    """bench.py's `roofline` object for the HGT workload (C3): the forward edge-softmax attention launch of the note
    destination type (the relations that end in `note`), same CSR and shapes as in the step, timed by `timed`.
    ALGORITHMIC bytes per launch: per relation the CSR (4 (N_dst + 1) + 4 E_r) and every distinct K', V' row once
    (2 * 4 H * N_src_unique_r: K' and V' are relation-specific), plus q and the output once (2 * 4 H * N_dst) and the
    softmax statistics kept for backward (2 * 4 * heads * N_dst)."""
    import numpy as np
    n_nodes = {k: int(v.shape[0]) for k, v in I["x_dict"].items()}
    hix = HeteroIndex(I["edge_index_dict"], n_nodes)
    ets = [et for et in hix.edge_types if et[2] == "note"]
    n = n_nodes["note"]
    gen = torch.Generator(device="cpu").manual_seed(0)
    q = torch.randn(n, hid, generator=gen).to(dev)
    kv = []
    for et in ets:
        kv += [torch.randn(n_nodes[et[0]], hid, generator=gen).to(dev), torch.randn(n_nodes[et[0]], hid, generator=gen).to(dev)]
    ps = torch.full((len(ets), heads), 1.0 / math.sqrt(hid // heads), device=dev)
    rels = (_lib.HgtRel * len(ets))()
    for r, et in enumerate(ets):
        c, k, v = hix.fwd[et], kv[2 * r], kv[2 * r + 1]
        rels[r].k, rels[r].v, rels[r].ld, rels[r].pscale = k.data_ptr(), v.data_ptr(), k.stride(0), ps[r].data_ptr()
        rels[r].rowptr, rels[r].col, rels[r].perm = c.rowptr.data_ptr(), c.col.data_ptr(), c.perm.data_ptr()
    out = torch.empty((n, hid), device=dev)
    m, linv = torch.empty((n, heads), device=dev), torch.empty((n, heads), device=dev)
    t_k, launches = timed(lambda: attention_forward(rels, q, out, m, linv, heads))
    b_alg, e_tot = 0, 0
    for et in ets:
        ei = g.edge_index[et]
        ei = ei[:, ei[0] >= 0]                                   # (-1, -1): padding slots of a device-sampled batch
        e_tot += int(ei.shape[1])
        b_alg += 4 * (n + 1) + 4 * int(ei.shape[1]) + 2 * 4 * hid * int(np.unique(ei[0]).size)
    b_alg += 2 * 4 * hid * n + 2 * 4 * heads * n
    return {"bound": "hbm",
            "kernel": f"k_hgt_fwd forward edge-softmax attention of the note type (R={len(ets)}, N_dst={n}, E={e_tot}, H={hid}, heads={heads})",
            "achieved": b_alg / t_k / 1e9, "peak": hbm_peak / 1e9, "unit": "GB/s", "frac": (b_alg / t_k) / hbm_peak,
            "traffic": None, "traffic_source": "profiles/r02_hgt_pmc.md (rocprofv3 --pmc passes of this launch)",
            "alg_bytes_per_launch": b_alg, "avg_us": t_k * 1e6, "launches": launches,
            "timing": "HIP events around hipGraph replays of 10 back-to-back launches"}
