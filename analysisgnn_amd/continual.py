"""The continual-learning terms of the reference's training step (`ContinualAnalysisGNN`, analysisgnn/models/analysis.py:1039-1072):
from the second task stage on the objective gains

  * a distillation term: a frozen copy of the model (`memory_model`, :918-932, :1370-1378) encodes the batch, the student's
    and the memory model's heads are both applied to THAT encoding for the previous tasks, and the term is
    `lambda_dctn * mean_t( kl_div(log_softmax(student_t / 2), softmax(teacher_t / 2), 'batchmean') * 4 )` (:1041-1062);
  * the EWC penalty `lambda_ewc * sum_n (fisher[n] * (p_n - mean_n)^2).sum()` (:1479-1495), `fisher` accumulated as
    `grad^2 / n_batches` after replay batches (:1440-1455), the means snapshotted at a task switch (:1460-1476).

Composed from torch ops the first is ~10 launches per task forward and as many backward, the second five whole-model
passes plus a per-parameter Python loop.  Here the distillation term and its FINISHED gradient come out of the three launches
of `agnn_multitask_kd_f32` (side-by-side logits, as `heads.training_loss`), and the EWC term is one pass over the flat
buffers of `dp.FlatAdamW` / `dp.FlatGradBuffer` (`agnn_ewc_f32`): the penalty's gradient is added straight into the packed
gradient buffer, before the optimizer's clipping sees it.  INTEGRATION.md has the stage-two step recipe."""
from __future__ import annotations

import copy
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib, resident
from .heads import unit_gradient


def _segments(offs, n_cols: int) -> Tuple[Tuple[int, ...], Optional[Tuple[int, ...]]]:
    """(starts + [last end], ends or None) from `offs`: either T+1 ascending offsets (segments side by side, what
    `forward_clf_fused` returns) or T `(start, end)` pairs (ascending, may leave columns between them uncovered)."""
    offs = list(offs)
    if offs and isinstance(offs[0], (tuple, list)):
        pairs = [(int(a), int(b)) for a, b in offs]
    else:
        flat = [int(o) for o in offs]
        pairs = [(flat[i], flat[i + 1]) for i in range(len(flat) - 1)]
    if not pairs:
        raise _lib.AgnnError("distillation_loss: no task segment given")
    prev = 0
    for a, b in pairs:
        if b - a < 1:
            raise _lib.AgnnError(f"distillation_loss: segment [{a}, {b}) is narrower than one class")
        if a < prev or b > n_cols:
            raise _lib.AgnnError(f"distillation_loss: segment [{a}, {b}) overlaps its predecessor or leaves the {n_cols} logit columns")
        prev = b
    starts = tuple(a for a, _ in pairs) + (pairs[-1][1],)
    gaps = any(pairs[i][1] != pairs[i + 1][0] for i in range(len(pairs) - 1))
    return starts, (tuple(b for _, b in pairs) if gaps else None)


def _segment_tensors(starts, ends, device):
    """(starts, ends or None) as int32 device tensors: host -> device once per layout, before any capture (a resident value)."""
    return resident.value(device, ("segment table", starts, ends), lambda: (
        torch.tensor(starts, dtype=torch.int32, device=device), torch.tensor(ends, dtype=torch.int32, device=device) if ends is not None else None))


class _Distill(torch.autograd.Function):
    """(total, kd[T]) of agnn_multitask_kd_f32 and the gradient w.r.t. the student logits, finished by the forward's launches
    for an incoming gradient of one; the backward hands it on (`heads.unit_gradient`) or multiplies by the incoming scalar."""

    @staticmethod
    def forward(ctx, student, teacher, seg_off, seg_end, T: int, tau: float, weight: float):
        dev = _lib.require_gpu(student, teacher, seg_off)
        if student.dtype != torch.float32 or student.stride(1) != 1:
            student = student.float().contiguous()
        if teacher.dtype != torch.float32 or teacher.stride(1) != 1:
            teacher = teacher.float().contiguous()
        N, n_cols = student.shape
        lib = _lib.load()
        dstudent = torch.empty((N, n_cols), dtype=torch.float32, device=dev)
        if N == 0:                                            # no row: every term is 0 (empty tensors have no address to hand over)
            out = torch.zeros((T + 1,), dtype=torch.float32, device=dev)
            ctx.save_for_backward(dstudent)
            ctx.mark_non_differentiable(out)
            ctx.set_materialize_grads(False)
            return out[T], out
        out = torch.empty((T + 1,), dtype=torch.float32, device=dev)          # kd[T] | total
        nws = int(lib.agnn_kd_workspace_bytes(N, T))
        ws = resident.scratch(dev, "distillation", nws, zeroed=False)
        # a one-row view may carry any stride(0): the kernel only needs it to reach the columns
        ld_s = student.stride(0) if N > 1 else max(student.stride(0), n_cols)
        ld_t = teacher.stride(0) if N > 1 else max(teacher.stride(0), n_cols)
        _lib.check(lib.agnn_multitask_kd_f32(student.data_ptr(), ld_s, teacher.data_ptr(), ld_t, seg_off.data_ptr(), _lib.ptr(seg_end), T, N,
                                             n_cols, float(tau), float(weight), dstudent.data_ptr(), dstudent.stride(0), out.data_ptr(),
                                             out[T:].data_ptr(), ws.data_ptr(), nws, _lib.stream_ptr(dev)), "agnn_multitask_kd_f32")
        ctx.save_for_backward(dstudent)
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)                      # no zero-filled gradient for the logging output
        return out[T], out

    @staticmethod
    def backward(ctx, g, _g_parts):
        (dstudent,) = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None, None
        if g.data_ptr() == unit_gradient(dstudent.device).data_ptr():      # one, known by identity: the gradient is finished
            return dstudent, None, None, None, None, None, None
        return dstudent * g.to(torch.float32), None, None, None, None, None, None


def distillation_loss(student_logits: torch.Tensor, teacher_logits: torch.Tensor, offs, temperature: float = 2.0,
                      weight: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(total, per_task): the distillation term of the reference's step (models/analysis.py:1052-1062),
        per_task[t] = tau^2 * kl_div(log_softmax(student_t / tau), softmax(teacher_t / tau), 'batchmean')
        total       = weight * per_task.mean()                       weight = the caller's lambda_dctn
    for logits that hold the tasks side by side in the same columns of both matrices [N, C] (fp32; column-slice views of wider
    matrices are taken as they are: `stride(1) == 1`, any row stride).  `offs`: the host list of T+1 segment offsets that
    `forward_clf_fused` returns, or T `(start, end)` pairs when the tasks are a subset of the columns — the gradient is 0 in
    columns no segment covers.  The gradient goes to the student only; it is finished in the forward's three launches, so
    `total.backward(gradient=heads.unit_gradient(dev))` launches nothing here,
    any other incoming gradient costs one multiply.  per_task [T] is for logging (not differentiable)."""
    if student_logits.dim() != 2 or student_logits.shape != teacher_logits.shape:
        raise _lib.AgnnError(f"distillation_loss: student {tuple(student_logits.shape)} and teacher {tuple(teacher_logits.shape)} "
                             "must be matrices of one shape")
    if not (temperature > 0 and temperature < float("inf")):
        raise _lib.AgnnError(f"distillation_loss: temperature={temperature}")
    starts, ends = _segments(offs, student_logits.shape[1])
    T = len(starts) - 1
    seg_off, seg_end = _segment_tensors(starts, ends, student_logits.device)
    total, out = _Distill.apply(student_logits, teacher_logits.detach(), seg_off, seg_end, T, float(temperature), float(weight))
    return total, out[:T]


class MemoryModel:
    """The frozen teacher (the reference's `memory_model`, models/analysis.py:918-932, `update_memory_model` :1370-1378): a
    deep copy of the model holding its `state_dict`, `requires_grad_(False)`, `eval()`.  Deliberately not an `nn.Module`: kept
    as an attribute of a training module it stays out of that module's parameters, optimizer and checkpoints of the student.
    `update_from(model)` refreshes the copy IN PLACE (at a task switch), so the teacher's storage is stable across steps and a
    captured step graph keeps reading the right memory."""

    _TRANSIENT = ("last_index", "_cut")      # per-step state some modules keep (the batch's CSR index, a cut autograd graph)

    def __init__(self, model: nn.Module):
        memo = {id(m.__dict__[k]): None for m in model.modules() for k in self._TRANSIENT if m.__dict__.get(k) is not None}
        self.module = copy.deepcopy(model, memo)             # those attributes are None in the copy
        for p in self.module.parameters():
            p.grad = None
        self.update_from(model)

    @torch.no_grad()
    def update_from(self, model: nn.Module) -> "MemoryModel":
        self.module.load_state_dict(model.state_dict())      # copies into the existing tensors
        self.module.requires_grad_(False)
        self.module.eval()
        return self

    def encode(self, *args, **kwargs):
        return self.module.encode(*args, **kwargs)

    def forward_clf_fused(self, x, tasks=None):
        return self.module.forward_clf_fused(x, tasks)

    def forward_clf(self, x, tasks=None):
        return self.module.forward_clf(x, tasks)

    def parameters(self):
        return self.module.parameters()

    def state_dict(self):
        return self.module.state_dict()


def distill(model: nn.Module, memory: MemoryModel, encode_kwargs: dict, previous_tasks: Sequence[str], temperature: float = 2.0,
            weight: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's distillation wiring in one call (models/analysis.py:1041-1062): the MEMORY model encodes the batch
    (no gradient), both models' heads — and logit fusion, when it is on — are applied to that encoding for `previous_tasks`,
    and `distillation_loss` compares them.  Gradients therefore reach the student's head (and logit-fusion) parameters only,
    never its encoder — exactly as in the reference.  `weight` = lambda_dctn (default 0.5, :909).  Returns (total, per_task)."""
    previous_tasks = list(previous_tasks)
    if not previous_tasks:
        raise _lib.AgnnError("distill: no previous task given (the reference adds the term only when there are previous tasks)")
    with torch.no_grad():
        x = memory.encode(**encode_kwargs)
        teacher, offs, _ = memory.forward_clf_fused(x, previous_tasks)
    student, offs_s, _ = model.forward_clf_fused(x, previous_tasks)
    if list(offs_s) != list(offs):
        raise _lib.AgnnError("distill: model and memory model lay the previous tasks out differently")
    return distillation_loss(student, teacher, offs, temperature, weight)


class EWC:
    """Elastic weight consolidation on the flat buffers of a `dp.FlatAdamW` (the reference's `_means` / `fisher` dicts and
    `get_ewc_loss`, models/analysis.py:1440-1495): `mean` and `fisher` are two flat fp32 buffers with the optimizer's layout,
    so the penalty and its gradient are ONE pass over four buffers (`agnn_ewc_f32`), whatever the number of parameters.

        task switch:   ewc.consolidate()                      mean <- parameters, fisher <- 0        (get_optimal_params)
                       per replay batch: backward, grads.pack(), ewc.accumulate(n_batches)            (compute_fisher)
        every step:    ... backward, grads.pack() / all-reduce, ewc.add_penalty_(lambda_ewc), opt.step(max_norm)

    `add_penalty_` adds d(lam * penalty)/dp into the packed gradient buffer, so the optimizer's clipping sees the term as it
    does when the term is part of the loss.  Graph-capturable after construction: every buffer exists from `__init__` on."""

    def __init__(self, optimizer):
        self.opt = optimizer
        self.grads = optimizer.grads
        flat = optimizer.flat
        self.dev = _lib.require_gpu(flat, self.grads.flat)
        self.mean = flat.detach().clone()
        self.fisher = torch.zeros_like(flat)
        lib = _lib.load()
        self._ws = torch.empty(int(lib.agnn_ewc_workspace_bytes()), dtype=torch.uint8, device=self.dev)
        self._penalty = torch.zeros((), dtype=torch.float32, device=self.dev)

    @torch.no_grad()
    def consolidate(self) -> None:
        """mean <- the current parameters, fisher <- 0 (the reference's `get_optimal_params` + `_init_fisher`)."""
        self.mean.copy_(self.opt.flat)
        self.fisher.zero_()

    @torch.no_grad()
    def accumulate(self, n_batches: int) -> None:
        """fisher += grads.flat^2 / n_batches, after a backward pass and `grads.pack()` (`compute_fisher`; a parameter that took
        no gradient packs as zeros and adds nothing, as the reference skips `p.grad is None`)."""
        if n_batches < 1:
            raise _lib.AgnnError(f"EWC.accumulate: n_batches={n_batches}")
        g = self.grads.flat
        _lib.check(_lib.load().agnn_fisher_accum_f32(g.data_ptr(), g.numel(), 1.0 / float(n_batches), self.fisher.data_ptr(),
                                                     _lib.stream_ptr(self.dev)), "agnn_fisher_accum_f32")

    def _run(self, lam: float, g: Optional[torch.Tensor]) -> torch.Tensor:
        p = self.opt.flat
        _lib.check(_lib.load().agnn_ewc_f32(p.data_ptr(), self.mean.data_ptr(), self.fisher.data_ptr(), p.numel(), float(lam), _lib.ptr(g),
                                            self._penalty.data_ptr(), self._ws.data_ptr(), self._ws.numel(), _lib.stream_ptr(self.dev)),
                   "agnn_ewc_f32")
        return self._penalty

    @torch.no_grad()
    def add_penalty_(self, lam: float) -> torch.Tensor:
        """grads.flat += lam * d penalty / d p  (= 2 lam fisher (p - mean)) and the UNWEIGHTED penalty `sum fisher (p - mean)^2`
        as a device scalar (the object's own: the next call overwrites it; log `lam * penalty` from it).  Call it on the
        packed — or all-reduced — gradient buffer, before `FlatAdamW.step`."""
        return self._run(lam, self.grads.flat)

    @torch.no_grad()
    def penalty(self) -> torch.Tensor:
        """The unweighted penalty alone (gradients untouched)."""
        return self._run(0.0, None)

    def _views(self, flat: torch.Tensor, model: nn.Module) -> Dict[str, torch.Tensor]:
        where = {id(p): (o, p.numel()) for p, o in zip(self.grads.params, self.grads.offsets)}
        out = {}
        for n, p in model.named_parameters():
            if not p.requires_grad:
                continue
            if id(p) not in where:
                raise _lib.AgnnError(f"EWC: parameter {n} is not in the optimizer's flat buffer")
            o, k = where[id(p)]
            out[n] = flat[o:o + k].view(p.shape)
        return out

    def fisher_dict(self, model: nn.Module) -> Dict[str, torch.Tensor]:
        """{name: view of `fisher`} over the `named_parameters()` that require a gradient (the reference's `self.fisher[n]`)."""
        return self._views(self.fisher, model)

    def means_dict(self, model: nn.Module) -> Dict[str, torch.Tensor]:
        """{name: view of `mean`} (the reference's `self._means[n]`)."""
        return self._views(self.mean, model)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"mean": self.mean.detach().clone(), "fisher": self.fisher.detach().clone()}

    @torch.no_grad()
    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        for k in ("mean", "fisher"):
            if state[k].numel() != getattr(self, k).numel():
                raise _lib.AgnnError(f"EWC.load_state_dict: {k} has {state[k].numel()} elements, the flat layout {getattr(self, k).numel()}")
        self.mean.copy_(state["mean"].reshape(-1))
        self.fisher.copy_(state["fisher"].reshape(-1))
