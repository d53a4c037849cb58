"""SMOTE oversampling of the minority classes and the feature penalty that goes with it (reference: models/cadence.py:13-118
`SMOTE`, models/analysis.py:1023-1029 and :1412-1438 `update_feature_loss`), on the kernels of csrc/smote.hip.

What the reference computes, and this module reproduces as it is:

* `fit_generate(X, y)`: class counts `occ`, the dominant class is the FIRST arg-max.  Classes are visited in ascending label
  order; a class is skipped when it is the dominant one, when `occ < k`, or when `occ == n_occ`.  Every other class makes
  `copies = int(((n_occ - occ) * 100 / occ) / 100)` synthetic rows per original row (float32 arithmetic; 0 is possible and adds
  nothing).  `X_over` = the originals, then class by class, row `i * copies + n` of a class coming from its i-th original.
* Neighbours.  The trainer builds `SMOTE(dims=out_channels, distance="euclidean", k=3)`; the class tests for the spelling
  `'euclidian'`, so the trained path is the cosine similarity of L2-normalised rows sorted ASCENDING, columns 1..k: ranks
  1..k of the LEAST similar rows of the class, not the nearest ones.  `'euclidian'` gives ranks 1..k of ascending Euclidean
  distance (rank 0 is the row itself); `'cosine'` and every other string give the similarity rule.
* Synthesis.  Per synthetic row `choice = randint(0, k - 1)` lies in [0, k - 2] (the k-th neighbour is never used),
  `gap = rand(dims)` is drawn per feature, `row = x_i + gap * (x_nb[choice] - x_i)`.  The result is differentiable with respect
  to X through x_i and x_nb; indices and draws carry no gradient.
* Penalty.  `bs = batch_size // n_unique(y_over)`; per class the rows of `x_over` and of `x` are cut to `bs` rows by a random
  permutation when there are more, and `mean(clamp(min_j |q - c_j| - threshold, min=0))` is added to `feature_loss`.

The class counts are read back once per call (the output shapes depend on them, as in the reference's `.item()`), so both calls
are eager-only: under stream capture they raise before any launch."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, fused, ops
from .graph import SegSpec, build_csr

MAX_D = 512


@dataclass
class PlanClass:
    label: int
    occ: int
    copies: int          # >= 1


@dataclass
class Plan:
    """What `fit_generate` does for given class counts: a pure function of them (no device)."""
    dominant: int
    n_occ: int
    classes: List[PlanClass]          # the classes that add rows, in output order
    skipped: List[Tuple[int, str]]    # (label, "dominant" | "below k" | "equal to dominant" | "zero copies")

    @property
    def n_synthetic(self) -> int:
        return sum(c.occ * c.copies for c in self.classes)

    def offsets(self) -> Tuple[List[int], List[int]]:
        """(t_off, s_off): class-sorted row offsets and synthetic-row offsets of `classes`."""
        t, s = [0], [0]
        for c in self.classes:
            t.append(t[-1] + c.occ)
            s.append(s[-1] + c.occ * c.copies)
        return t, s


def plan(counts: Sequence[int], k: int) -> Plan:
    """counts[c] = rows of label c (length max label + 1)."""
    occ = [int(c) for c in counts]
    if not occ:
        return Plan(-1, 0, [], [])
    dominant = int(np.argmax(np.asarray(occ)))            # first arg-max, as torch.argmax
    n_occ = occ[dominant]
    classes, skipped = [], []
    for c, o in enumerate(occ):
        if c == dominant:
            skipped.append((c, "dominant"))
        elif o < k:
            skipped.append((c, "below k"))
        else:
            n = (np.float32(n_occ) - np.float32(o)) * np.float32(100) / np.float32(o)      # the reference's float32 tensor arithmetic
            if n == 0:
                skipped.append((c, "equal to dominant"))
                continue
            copies = int(n / np.float32(100))
            if copies == 0:
                skipped.append((c, "zero copies"))
            else:
                classes.append(PlanClass(c, o, copies))
    return Plan(dominant, n_occ, classes, skipped)


def _no_capture(what: str) -> None:
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise _lib.AgnnError(f"{what} reads the class counts back to the host (its output shapes depend on them): it cannot be captured")


def _check_x(x: torch.Tensor, what: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise _lib.AgnnError(f"{what}: a 2-D feature matrix is expected")
    _lib.require_gpu(x)
    if x.dtype != torch.float32:
        raise _lib.AgnnError(f"{what}: fp32 expected, got {x.dtype}")
    D = x.shape[1]
    if D % 4 != 0 or D < 4 or D > MAX_D:
        raise _lib.AgnnError(f"{what}: D={D} must be a multiple of 4 in [4, {MAX_D}]")


def _i32(vals: Sequence[int]):
    return (_lib.C.c_int32 * len(vals))(*vals)


def row_select(q: torch.Tensor, c: torch.Tensor, q_off: Sequence[int], c_off: Sequence[int], ksel: int, mode: int,
               q_rows: Optional[torch.Tensor] = None, c_rows: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """agnn_rowsel_f32: per query the `ksel` smallest scores among the candidates of its segment (ascending, ties to the lower
    index) as (idx int32 [Q, ksel] of candidate positions or -1, score fp32 [Q, ksel] or +inf).  `q_rows` / `c_rows`: int32 row
    numbers of q / c per position (None: the position itself)."""
    dev = _lib.require_gpu(q, c, q_rows, c_rows)
    q, c = _lib.rows16(q), _lib.rows16(c)
    n_seg = len(q_off) - 1
    if len(c_off) != len(q_off) or n_seg < 0 or n_seg > _lib.MAX_SEG:
        raise _lib.AgnnError(f"row_select: {n_seg} segments (at most {_lib.MAX_SEG}; q_off and c_off of one length)")
    for r, off in ((q_rows, q_off), (c_rows, c_off)):
        if r is not None and (r.dtype != torch.int32 or not r.is_contiguous() or r.numel() < off[-1]):
            raise _lib.AgnnError("row_select: row numbers are contiguous int32, one per position")
    Q = int(q_off[-1]) if n_seg >= 0 and len(q_off) else 0
    idx = torch.empty((Q, ksel), dtype=torch.int32, device=dev)
    score = torch.empty((Q, ksel), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().agnn_rowsel_f32(q.data_ptr(), q.stride(0), _lib.ptr(q_rows), q.shape[0], c.data_ptr(), c.stride(0), _lib.ptr(c_rows),
                                           c.shape[0], n_seg, _i32([int(v) for v in q_off]), _i32([int(v) for v in c_off]), q.shape[1], int(ksel),
                                           int(mode), idx.data_ptr(), score.data_ptr(), _lib.stream_ptr(dev)), "agnn_rowsel_f32")
    return idx, score


def draws(S: int, D: int, k: int, call_id: int, rng: Optional[torch.Tensor] = None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(choice int32 [S], gap fp32 [S, D]) that a call with this call id draws from `rng` (device int64[2] = (seed, step);
    None: the live state, `fused.rng_state`) — by the device functions the kernels use.  `SMOTE.last_call` holds what a call used."""
    if rng is None:
        rng = fused.rng_state(torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
    dev = _lib.require_gpu(rng)
    choice = torch.empty((S,), dtype=torch.int32, device=dev)
    gap = torch.empty((S, D), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().agnn_smote_draws_f32(int(S), int(D), int(k), rng.data_ptr(), int(call_id) & 0xFFFFFFFF, choice.data_ptr(), gap.data_ptr(),
                                                _lib.stream_ptr(dev)), "agnn_smote_draws_f32")
    return choice, gap


def _c_plan(classes: Sequence[PlanClass]) -> _lib.SmotePlan:
    if len(classes) > _lib.MAX_SEG:
        raise _lib.AgnnError(f"SMOTE: {len(classes)} classes to oversample, at most {_lib.MAX_SEG} per call")
    p = _lib.SmotePlan()
    p.n_seg = len(classes)
    t = s = 0
    for i, c in enumerate(classes):
        p.t_off[i], p.s_off[i], p.copies[i], p.label[i] = t, s, c.copies, c.label
        t += c.occ
        s += c.occ * c.copies
        if s > _lib.INT32_MAX:
            raise _lib.AgnnError("SMOTE: more than 2^31 - 1 synthetic rows")
    p.t_off[len(classes)], p.s_off[len(classes)] = t, s
    return p


def _sum_by_row(row: torch.Tensor, src: torch.Tensor, n_rows: int, onto: Optional[torch.Tensor]) -> torch.Tensor:
    """out[r] = onto[r] + sum of src[e] over row[e] == r: a CSR by `row` and the library's sum aggregation (no float atomics)."""
    E = row.numel()
    csr = build_csr([SegSpec(row=row.long(), col=torch.arange(E, dtype=torch.int64, device=row.device), n_rows=n_rows)])[0]
    spec = ops.AggSpec(fwd=[csr], bwd=[csr], src_id=[0], n_rows=n_rows, mean=False, shared_slot=True)
    with torch.no_grad():
        return ops.aggregate(spec, [src], self_t=onto)


class _Synthesize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, cplan, rows, nbr, k, choice, gap, call_id, info):
        dev = x.device
        lib = _lib.load()
        x = _lib.rows16(x)
        N, D = x.shape
        S = int(cplan.s_off[cplan.n_seg])
        xo = torch.empty((N + S, D), dtype=torch.float32, device=dev)
        yo = torch.empty((N + S,), dtype=torch.int64, device=dev) if y is not None else None
        nb_row = torch.empty((max(S, 1),), dtype=torch.int32, device=dev)
        rng = used = None
        if gap is None:
            rng = fused.rng_state(dev)
            used = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.agnn_smote_synth_fwd_f32(x.data_ptr(), x.stride(0), _lib.ptr(y), N, D, _lib.C.byref(cplan), rows.data_ptr(), nbr.data_ptr(),
                                                nbr.stride(0), k, _lib.ptr(choice), _lib.ptr(gap), _lib.ptr(rng), call_id, xo.data_ptr(),
                                                xo.stride(0), _lib.ptr(yo), nb_row.data_ptr(), _lib.ptr(used), _lib.stream_ptr(dev)),
                   "agnn_smote_synth_fwd_f32")
        ctx.cfg = (cplan, k, call_id, N, D, S)
        ctx.save_for_backward(rows, nb_row, *([gap] if gap is not None else [used]))
        ctx.explicit = gap is not None
        info.update(call_id=call_id, rng_used=used, nb_row=nb_row[:S], rows=rows, nbr=nbr, S=S, D=D, k=k,
                    t_off=[int(cplan.t_off[i]) for i in range(cplan.n_seg + 1)], labels=[int(cplan.label[i]) for i in range(cplan.n_seg)])
        if yo is None:
            return xo
        ctx.mark_non_differentiable(yo)
        return xo, yo

    @staticmethod
    def backward(ctx, g, *_):
        cplan, k, call_id, N, D, S = ctx.cfg
        rows, nb_row, last = ctx.saved_tensors
        dev = g.device
        g = _lib.rows16(g)
        dx = g[:N].clone()
        w = torch.empty((S, D), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().agnn_smote_synth_bwd_f32(g.data_ptr(), g.stride(0), N, D, _lib.C.byref(cplan), rows.data_ptr(),
                                                        last.data_ptr() if ctx.explicit else None, None if ctx.explicit else last.data_ptr(),
                                                        call_id, dx.data_ptr(), dx.stride(0), w.data_ptr(), w.stride(0), _lib.stream_ptr(dev)),
                   "agnn_smote_synth_bwd_f32")
        dx = _sum_by_row(nb_row[:S], w, N, dx)          # the neighbour term: dx[nb_row[s]] += gap o g[N + s]
        return (dx,) + (None,) * 9


class SMOTE(object):
    """The reference's `SMOTE` (same constructor, `fit_generate(X, y)` and `generate(min_samples, N, k)`, same result layout).
    NOTE the neighbour rule documented at the top of this module: with any `distance` but 'euclidian' — the trainer's
    "euclidean" included — the neighbours are ranks 1..k of the LEAST cosine-similar rows of the class.

    Keyword extras: `draws=(choice int32 [S], gap fp32 [S, dims])` replaces the generator; `call_id` names the call's Philox
    stream (None: the next of `fused._CALL_IDS`).  `last_call` holds call id, rng state, the neighbour table (`nbr`: class-sorted
    positions, rank 0 included; `rows`: position -> row of X; `t_off`, `labels`: the classes' position ranges) and sizes of the latest call: `smote.draws(S, D, k, call_id, rng_used)` rebuilds its draws."""

    def __init__(self, distance='custom', dims=512, k=2):
        super(SMOTE, self).__init__()
        self.newindex = 0
        self.k = k
        self.dims = dims
        self.distance_measure = distance
        self.last_call: dict = {}
        self.last_plan: Optional[Plan] = None

    def _mode(self) -> int:
        return _lib.ROWSEL_SQDIST if self.distance_measure == 'euclidian' else _lib.ROWSEL_COSINE

    def _check(self, x, k: int, what: str) -> None:
        _check_x(x, what)
        if k < 2:
            raise _lib.AgnnError(f"{what}: k={k}: the neighbour choice randint(0, k - 1) needs k >= 2")
        if k > _lib.ROWSEL_MAX_K - 1:
            raise _lib.AgnnError(f"{what}: k={k} exceeds {_lib.ROWSEL_MAX_K - 1}")
        if x.shape[1] != self.dims:
            raise _lib.AgnnError(f"{what}: rows of width {x.shape[1]}, dims={self.dims}")

    def _run(self, x, y, classes: Sequence[PlanClass], rows: torch.Tensor, k: int, draws_, call_id):
        D = x.shape[1]
        cplan = _c_plan(classes)
        S = int(cplan.s_off[cplan.n_seg])
        choice = gap = None
        if draws_ is not None:
            choice, gap = draws_
            _lib.require_gpu(choice, gap)
            if choice.dtype != torch.int32 or tuple(choice.shape) != (S,) or gap.dtype != torch.float32 or tuple(gap.shape) != (S, D):
                raise _lib.AgnnError(f"SMOTE: draws are (int32 [{S}], fp32 [{S}, {D}])")
            choice, gap = choice.contiguous(), gap.contiguous()
            if S and (int(choice.min()) < 0 or int(choice.max()) > k - 2):
                raise _lib.AgnnError(f"SMOTE: neighbour choices must lie in [0, {k - 2}]")
        call_id = (next(fused._CALL_IDS) if call_id is None else int(call_id)) & 0xFFFFFFFF
        t_off = [int(cplan.t_off[i]) for i in range(cplan.n_seg + 1)]
        xd = _lib.rows16(x.detach())
        nbr, _ = row_select(xd, xd, t_off, t_off, k + 1, self._mode(), rows, rows)
        self.last_call = {}
        return _Synthesize.apply(x, y, cplan, rows, nbr, k, choice, gap, call_id, self.last_call)

    def generate(self, min_samples, N, k, device=None, draws=None, call_id=None):
        """`int(N / 100)` synthetic rows per row of `min_samples`, row-major (`i * copies + n`): [int(N / 100) * T, dims]."""
        self._check(min_samples, int(k), "SMOTE.generate")
        _no_capture("SMOTE.generate")
        T = min_samples.shape[0]
        copies = int(N / 100)
        if T == 0 or copies < 1:
            return torch.zeros((max(copies, 0) * T, self.dims), dtype=torch.float32, device=min_samples.device)
        rows = torch.arange(T, dtype=torch.int32, device=min_samples.device)
        xo = self._run(min_samples, None, [PlanClass(0, T, copies)], rows, int(k), draws, call_id)
        return xo[T:]

    def fit_generate(self, X, y, draws=None, call_id=None):
        """(X_over fp32 [N + S, D], y_over int64 [N + S]): the originals, then the synthetic rows class by class."""
        self._check(X, int(self.k), "SMOTE.fit_generate")
        _lib.require_gpu(X, y)
        if y.dim() != 1 or y.shape[0] != X.shape[0] or y.dtype not in (torch.int64, torch.int32):
            raise _lib.AgnnError("SMOTE.fit_generate: y is an integer label per row of X")
        if X.shape[0] == 0:
            return X, y
        _no_capture("SMOTE.fit_generate")
        y = y.long().contiguous()
        counts = torch.bincount(y).tolist()                     # the call's one device-to-host read
        p = plan(counts, self.k)
        self.last_plan = p
        if not p.classes:
            self.last_call = {}
            return X, y
        # class-sorted once, stable (a class keeps its row order), the oversampled classes first
        rank = torch.full((len(counts),), len(p.classes), dtype=torch.int64)
        for i, c in enumerate(p.classes):
            rank[c.label] = i
        order = torch.sort(rank.to(y.device)[y], stable=True).indices
        rows = order[:sum(c.occ for c in p.classes)].int()
        return self._run(X, y, p.classes, rows, int(self.k), draws, call_id)


class _Penalty(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_over, x, q_rows, c_rows, offs, weight, threshold):
        q_off, c_off = offs
        idx, d2 = row_select(x_over.detach(), x.detach(), q_off, c_off, 1, _lib.ROWSEL_SQDIST, q_rows, c_rows)
        d = d2[:, 0].sqrt()
        c_sel = c_rows.index_select(0, idx[:, 0].long().clamp_min(0))   # the nearest original's row of x (-1, nothing selectable among NaN rows: the value is inf)
        ctx.save_for_backward(x_over, x, q_rows, c_sel, d, weight)
        ctx.threshold = threshold
        return (torch.clamp(d - threshold, min=0) * weight).sum()

    @staticmethod
    def backward(ctx, gout):
        x_over, x, q_rows, c_sel, d, weight = ctx.saved_tensors
        ql, cl = q_rows.long(), c_sel.long()
        live = (d > ctx.threshold) & (d > 0)                         # d = 0 (an original meeting itself): zero gradient, not 0 / 0
        coef = torch.where(live, gout * weight / torch.where(live, d, torch.ones_like(d)), torch.zeros_like(d))
        gq = coef[:, None] * (x_over.detach().index_select(0, ql) - x.detach().index_select(0, cl))
        dxo = dx = None
        if ctx.needs_input_grad[0]:
            dxo = torch.zeros_like(x_over)
            dxo.index_copy_(0, ql, gq)                               # the queries of a call are distinct rows
        if ctx.needs_input_grad[1]:
            dx = _sum_by_row(c_sel, -gq, x.shape[0], None).to(x.dtype)
        return dxo, dx, None, None, None, None, None


def feature_penalty(feature_loss, x_over, y_over, x, y, batch_size=100, threshold=1.0, perms=None):
    """The reference's `update_feature_loss`: feature_loss + sum over the classes of y_over of
    mean(clamp(min_j |q - c_j| - threshold, min=0)), q the class's rows of x_over and c_j its rows of x, each cut to
    `bs = batch_size // n_classes` rows by a random permutation when there are more.

    `perms`: the permutations in the order the reference draws them — per class in ascending order, one over the class's rows of
    x if they are more than bs, then one over its rows of x_over if they are more than bs — as 1-D integer tensors; None draws
    them with `torch.randperm` on the device.  Differentiable with respect to x_over and x; the nearest original is searched by
    agnn_rowsel_f32 (squared distances summed from the differences), the gradient reaches the rows of x through a CSR and the
    library's sum aggregation.  Eager-only (one device-to-host read of the class counts)."""
    _check_x(x_over, "feature_penalty")
    _check_x(x, "feature_penalty")
    dev = _lib.require_gpu(x_over, y_over, x, y)
    if x_over.shape[1] != x.shape[1] or y_over.shape[0] != x_over.shape[0] or y.shape[0] != x.shape[0]:
        raise _lib.AgnnError("feature_penalty: x_over / y_over and x / y are rows with one label each, of one width")
    if x_over.shape[0] == 0:
        return feature_loss
    _no_capture("feature_penalty")
    y_over, y = y_over.long(), y.long()
    co = torch.bincount(y_over)
    cy = torch.bincount(y, minlength=co.numel())
    n_lab = max(co.numel(), cy.numel())
    both = torch.cat([torch.nn.functional.pad(co, (0, n_lab - co.numel())), cy]).tolist()      # the call's one device-to-host read
    co_h, cy_h = both[:n_lab], both[n_lab:]
    classes = [c for c in range(n_lab) if co_h[c] > 0]
    bs = int(batch_size) // len(classes)
    if bs < 1:
        raise _lib.AgnnError(f"feature_penalty: batch_size={batch_size} leaves no row for each of {len(classes)} classes")
    order_o = torch.sort(y_over, stable=True).indices
    order_y = torch.sort(y, stable=True).indices
    off_o = np.concatenate([[0], np.cumsum(co_h)])
    off_y = np.concatenate([[0], np.cumsum(cy_h)])
    perms = list(perms) if perms is not None else None

    def cut(order, lo, n):
        rows = order[lo:lo + n]
        if n > bs:
            if perms is None:
                pm = torch.randperm(n, device=dev)
            else:
                if not perms:
                    raise _lib.AgnnError("feature_penalty: fewer permutations than the classes need")
                pm = perms.pop(0).to(dev).long()
                if pm.numel() != n:
                    raise _lib.AgnnError(f"feature_penalty: a permutation of {pm.numel()} where the class has {n} rows")
            rows = rows[pm[:bs]]
        return rows

    q_parts, c_parts, q_off, c_off, wts = [], [], [0], [0], []
    for c in classes:
        if cy_h[c] == 0:
            raise _lib.AgnnError(f"feature_penalty: class {c} has rows in x_over and none in x")
        cr = cut(order_y, int(off_y[c]), cy_h[c])               # the reference cuts x's rows first, then x_over's
        qr = cut(order_o, int(off_o[c]), co_h[c])
        q_parts.append(qr)
        c_parts.append(cr)
        q_off.append(q_off[-1] + qr.numel())
        c_off.append(c_off[-1] + cr.numel())
        wts += [1.0 / qr.numel()] * qr.numel()
    if perms:
        raise _lib.AgnnError("feature_penalty: more permutations than the classes need")
    q_rows = torch.cat(q_parts).int()
    c_rows = torch.cat(c_parts).int()
    weight = torch.tensor(wts, dtype=torch.float32).to(dev)
    pen = _Penalty.apply(x_over, x, q_rows, c_rows, (q_off, c_off), weight, float(threshold))
    return feature_loss + pen
