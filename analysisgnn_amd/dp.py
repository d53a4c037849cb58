"""Single-node data parallelism: one process per GPU, gradients all-reduced over RCCL/xGMI.

Replaces what Lightning's implicit DDP does for the reference
(analysisgnn/train/train_analysisgnn.py:138-146, :246-255): sampled subgraphs are independent
units (block-diagonal batches, no cross edges), so ranks take disjoint subgraphs, run the hot
path locally and exchange only gradients — ONE collective per step on a flat fp32 buffer.
MI355X notes: ~5 M parameters = ~20 MB; a node's 8 GPUs are fully connected by xGMI links, so
one large all-reduce (all links busy) beats per-parameter messages; parameters' `.grad` are views
into the flat buffer, so backward writes straight into the message (no pack/unpack copies).
Works on the `gloo` backend with CPU tensors too (that is how the N>1 path is tested without GPUs).
"""
from __future__ import annotations

import os
from typing import Iterable, List, Optional, Sequence

import torch
import torch.distributed as dist


def init_distributed(backend: Optional[str] = None) -> tuple:
    """Read RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* (torch.distributed.run contract)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            # AGNN_DIST_BACKEND=gloo lets several ranks share ONE GPU (rehearsing the N>1 flow on a 1-GPU box)
            backend = os.environ.get("AGNN_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if backend == "nccl":
            torch.cuda.set_device(local)
            dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, local, world


def shard_units(n_units: int, rank: int, world: int) -> List[int]:
    """Subgraph ids of this rank: {i : i mod world == rank} (DistributedSampler semantics)."""
    return list(range(rank, n_units, world))


def _aligned_offsets(sizes: Sequence[int], align: int = 4, tight: Optional[Sequence[bool]] = None) -> List[int]:
    """Start offset of every slot (+ the end): slots start on `align`-float boundaries, except that a slot marked `tight`
    starts right where the previous one ends (members of a group that is consumed as one concatenated operand)."""
    offs, end = [], 0
    for i, k in enumerate(sizes):
        start = end if (tight is not None and tight[i] and i > 0) else (end + align - 1) // align * align
        offs.append(start)
        end = start + k
    offs.append((end + align - 1) // align * align)
    return offs


def plan_parameters(model: torch.nn.Module, late: Iterable[torch.nn.Parameter] = ()):
    """(params, tight): the trainable parameters in the order the flat buffers should hold them, and the ids of those that
    must sit right behind their predecessor.  `late`: parameters whose gradients the backward pass produces LAST (the input
    layers) — placed at the END of the buffer so that everything before them is one contiguous message that can be all-reduced
    while they are still being computed (FlatGradBuffer(late=...), all_reduce_early_async).  Modules may expose `adjacent_parameter_groups()` -> lists of parameters
    that the hot path consumes concatenated (task-head layers, GRU direction pairs): laid out back to back, the cat /
    stack is a view of the flat parameter buffer instead of a launch per step (params.cat_rows / stack_rows).  All other
    parameters follow in `model.parameters()` order."""
    groups = []
    for m in model.modules():
        fn = getattr(m, "adjacent_parameter_groups", None)
        if fn is not None:
            groups.extend([[p for p in g] for g in fn()])
    late_ids = {id(p) for p in late}
    seen, params, tight = set(), [], set()
    for g in groups:
        if any(id(p) in late_ids for p in g):
            raise ValueError("plan_parameters: an adjacency group cannot hold late parameters")
        g = [p for p in g if p.requires_grad and id(p) not in seen]
        for i, p in enumerate(g):
            seen.add(id(p))
            params.append(p)
            if i > 0:
                tight.add(id(p))
    for want_late in (False, True):
        for p in model.parameters():
            if p.requires_grad and id(p) not in seen and (id(p) in late_ids) == want_late:
                seen.add(id(p))
                params.append(p)
    return params, tight


def _grad_in_place() -> bool:
    from . import linear
    return bool(linear.GRAD_IN_PLACE)


class FlatGradBuffer:
    """All gradients of `params` in one contiguous fp32 buffer (the all-reduce message).

    Two modes:
      * `views=True`  — `.grad` of each parameter is a view into the buffer, backward accumulates straight into
        the message (no pack step; costs one tiny accumulate launch per parameter, fine when GPU-bound);
      * `views=False` — autograd hands over fresh gradient tensors (no per-parameter accumulate launches, which
        dominate when a step is launch-bound: ~130 parameters here) and `pack()` gathers them;
        `.grad` then become views of the buffer so the optimizer sees the reduced / clipped values.  On a GPU the
        parameters' slots are registered (linear.register_grad_slots): the native kernels that produce a gradient write
        it into its slot themselves (linear.GRAD_IN_PLACE), and `pack()` only copies or zero-fills the rest.
    """

    def __init__(self, params: Iterable[torch.nn.Parameter], views: bool = True, tight: Optional[set] = None,
                 late: Iterable[torch.nn.Parameter] = ()):
        """`late`: the parameters of the second bucket (must be the LAST ones of `params`, dp.plan_parameters(model, late=...)
        puts them there): `pack("early")` / `pack("late")` gather the two buckets separately, `all_reduce_early_async` ships
        the first while the backward pass still works on the second."""
        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        dev = self.params[0].device
        self.sizes = [p.numel() for p in self.params]
        # every slot starts on a 16-byte boundary (the HIP kernels read parameters / gradients as float4), except the
        # members of an adjacency group (plan_parameters), which are consumed through one view of the whole group
        self.offsets = _aligned_offsets(self.sizes, tight=[tight is not None and id(p) in tight for p in self.params])
        n = self.offsets[-1]
        self.views = views
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("FlatGradBuffer: fp32 parameters on one device expected")
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self._pad = torch.zeros(4, dtype=torch.float32, device=dev)
        # a parameter that took no gradient this step (a layer that keeps no edge: encoders.HeteroConv) packs from here
        self._none = torch.zeros(max(self.sizes) if self.sizes else 1, dtype=torch.float32, device=dev)
        late_ids = {id(p) for p in late}
        self.n_early = len(self.params)
        if late_ids:
            flags = [id(p) in late_ids for p in self.params]
            self.n_early = flags.index(True) if True in flags else len(flags)
            if not all(flags[self.n_early:]) or sum(flags) != len(late_ids):
                raise ValueError("FlatGradBuffer: the late parameters must be the last ones of the buffer (dp.plan_parameters(model, late=...))")
        self.cut = self.offsets[self.n_early]                # flat[:cut] = early bucket, flat[cut:] = late bucket
        if views:
            self._assign_views()
        elif dev.type == "cuda":
            import weakref
            from . import linear
            linear.register_grad_slots(self, self.params, self.flat, self.offsets)
            weakref.finalize(self, linear.unregister_grad_slots, id(self))       # removing the buffer removes its entries

    def close(self) -> None:
        """Withdraw the parameters' slots from the registry (also done when the buffer is collected)."""
        from . import linear
        linear.unregister_grad_slots(id(self))

    def _assign_views(self) -> None:
        for p, k, o in zip(self.params, self.sizes, self.offsets):
            p.grad = self.flat[o:o + k].view_as(p)

    def zero(self) -> None:
        if self.views:
            self.flat.zero_()
        else:
            for p in self.params:
                p.grad = None
            self._packed = set()
            if self.flat.is_cuda:
                from .linear import reset_grad_slots
                reset_grad_slots(self.params)

    def pack(self, part: Optional[str] = None) -> None:
        """views=False: gather the fresh gradients into the flat buffer (one launch; `part` = "early" / "late": one bucket, one
        launch each).  Also the join point of the weight-gradient stream (linear.enable_wgrad_overlap)."""
        from .linear import join_wgrad
        join_wgrad()
        if self.views:
            return
        done = getattr(self, "_packed", set())
        if not isinstance(done, set):
            done = {"early", "late"} if done else set()
        for name, lo, hi in (("early", 0, self.n_early), ("late", self.n_early, len(self.params))):
            if (part is not None and part != name) or name in done or lo == hi:
                done.add(name) if lo == hi else None
                continue
            if self.flat.is_cuda and _grad_in_place():
                self._pack_native(lo, hi)
            else:                                    # CPU buffers, and linear.GRAD_IN_PLACE off: the one-cat gather as it was
                parts = []
                for i in range(lo, hi):
                    p, k, o, o_next = self.params[i], self.sizes[i], self.offsets[i], self.offsets[i + 1]
                    parts.append(p.grad.reshape(-1) if p.grad is not None else self._none[:k])
                    if o_next - o > k:
                        parts.append(self._pad[: o_next - o - k])
                torch.cat(parts, out=self.flat[self.offsets[lo]:self.offsets[hi]])
            for i in range(lo, hi):
                p, k, o = self.params[i], self.sizes[i], self.offsets[i]
                p.grad = self.flat[o:o + k].view_as(p)
            done.add(name)
        self._packed = done

    def _pack_native(self, lo: int, hi: int) -> None:
        """The gradients of parameters lo .. hi - 1 that are not in their slots yet — made by torch ops or by kernels that do not
        take a destination — copied there, and the slots of parameters that took no gradient zero-filled (they hold the last
        step's values), by one `agnn_pack_f32` launch (up to 24 pieces) or `agnn_gather_f32` (128 pieces per launch).  The few floats of padding behind a slot whose size is no
        multiple of four are zero-filled as well: after `pack()` every element of the buffer has been written this step."""
        from . import _lib
        from .linear import reset_grad_slots
        from .params import pack
        items = []
        for i in range(lo, hi):
            p, k, o, o_next = self.params[i], self.sizes[i], self.offsets[i], self.offsets[i + 1]
            g = p.grad
            if o_next - o > k:
                items.append((self.flat[o + k:o_next].view(1, -1), []))
            if k == 0:
                continue
            slot = self.flat[o:o + k]
            if g is None:
                items.append((slot.view(1, -1), []))
                continue
            if g.data_ptr() == slot.data_ptr() and g.shape == p.shape and g.is_contiguous():
                continue                                       # written in place by its producer
            if g.dtype != torch.float32 or g.device != self.flat.device:
                raise ValueError("FlatGradBuffer.pack: fp32 gradients on the buffer's device expected")
            items.append((slot.view(1, -1), [g.contiguous().view(1, -1)]))
        if len(items) <= _lib.PACK_MAX_ITEMS:
            if items:
                pack(items, self.flat.device)
        else:
            # more pieces than one agnn_pack_f32 launch takes (HGT's relation parameters, a GRU on the library path): the plain
            # gather, 128 pieces per launch — a launch per 24 cost more than the two torch.cat launches it replaced
            arr = (_lib.GatherItem * len(items))()
            keep = []
            for a, (dst, srcs) in zip(arr, items):
                a.dst, a.n = dst.data_ptr(), dst.numel()
                a.src = srcs[0].data_ptr() if srcs else None
                keep.extend(srcs)
            _lib.check(_lib.load().agnn_gather_f32(len(items), arr, _lib.stream_ptr(self.flat.device)), "agnn_gather_f32")
        reset_grad_slots(self.params[lo:hi])

    def all_reduce_mean(self, world: Optional[int] = None) -> None:
        """SUM over ranks then divide: the same mean DDP applies."""
        self.pack()
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)
            self.flat.div_(dist.get_world_size())

    def all_reduce_early_async(self):
        """Bucket 1 of 2 (what Lightning DDP's reverse-order buckets do, train/train_analysisgnn.py:246-255): gather and ship
        everything but the late parameters NOW — the collective runs on the communicator's stream beside whatever the caller
        queues next (the input layers' backward).  Returns the work handle for `all_reduce_late_and_finish` (None: one rank)."""
        self.pack("early")
        if dist.is_initialized() and dist.get_world_size() > 1 and self.cut > 0:
            return dist.all_reduce(self.flat[:self.cut], op=dist.ReduceOp.SUM, async_op=True)
        return None

    def all_reduce_late_and_finish(self, work) -> None:
        """Bucket 2 of 2 (small: the input layers), then wait for bucket 1 and divide: the buffer holds the mean, bit-identical
        to `all_reduce_mean` (SUM over ranks is element-wise: where a message is cut does not change a sum)."""
        self.pack("late")
        if dist.is_initialized() and dist.get_world_size() > 1:
            if self.cut < self.flat.numel():
                dist.all_reduce(self.flat[self.cut:], op=dist.ReduceOp.SUM)
            if work is not None:
                work.wait()
            self.flat.div_(dist.get_world_size())

    def clip_norm_(self, max_norm: float) -> torch.Tensor:
        """clip_grad_norm_ on the flat view (one norm, no per-parameter launches, no host sync)."""
        total = torch.linalg.vector_norm(self.flat)
        self.flat.mul_(torch.clamp(max_norm / (total + 1e-6), max=1.0))
        return total


class LRSchedule:
    """Learning rate as a closed form of the optimizer's DEVICE step counter (`agnn_lr_schedule_t`, include/agnn.h): step k
    (k optimizer steps already taken) uses `lr_at(k)`.  The hyper-parameters are constants of the launch, so a captured
    `FlatAdamW.step` follows the schedule on every replay; changing them afterwards needs a new capture."""
    FIELDS = ("kind", "warmup_steps", "count_offset", "base_lr", "warmup_start_lr", "eta_min", "cos_a", "cos_b", "gamma", "decay_steps")

    def __init__(self, kind: int, base_lr: float, warmup_steps: int = 0, count_offset: int = 0, warmup_start_lr: float = 0.0,
                 eta_min: float = 0.0, cos_a: float = 0.0, cos_b: float = 1.0, gamma: float = 1.0, decay_steps: float = 1.0):
        self.kind, self.warmup_steps, self.count_offset = int(kind), int(warmup_steps), int(count_offset)
        self.base_lr, self.warmup_start_lr, self.eta_min = float(base_lr), float(warmup_start_lr), float(eta_min)
        self.cos_a, self.cos_b, self.gamma, self.decay_steps = float(cos_a), float(cos_b), float(gamma), float(decay_steps)
        self.lr_at(0)                                    # the library's own validation (AgnnError)

    @classmethod
    def constant(cls, lr: float) -> "LRSchedule":
        from . import _lib
        return cls(_lib.LR_CONSTANT, lr)

    @classmethod
    def warmup_cosine(cls, base_lr: float, warmup_steps: int, total_steps: int, eta_min: float = 0.0) -> "LRSchedule":
        """Step-based: linear warm-up from 0 over `warmup_steps` optimizer steps, then a half cosine that reaches `eta_min`
        at step `total_steps`."""
        from . import _lib
        return cls(_lib.LR_WARMUP_COSINE, base_lr, warmup_steps, 0, 0.0, eta_min, cos_a=warmup_steps, cos_b=total_steps)

    @classmethod
    def reference_cosine(cls, base_lr: float, warmup_steps: int, max_epochs: int, eta_min: float = 0.0,
                         warmup_start_lr: float = 0.0) -> "LRSchedule":
        """The reference's `LinearWarmupCosineAnnealingLR` stepped once per optimizer step, taken LITERALLY
        (models/analysis.py:104-188, "interval": "step"): the warm-up runs on k + 1, the cosine on
        (k - warmup_steps / 3) / (max_epochs - warmup_steps / 3) — the class derives its `steps_per_epoch` as
        current_step / last_epoch at its third `step()` call, which is 3.0.  It raises AttributeError when the warm-up ends
        before that call (warmup_steps < 3), and so does this constructor (ValueError)."""
        from . import _lib
        if warmup_steps < 3:
            raise ValueError(f"reference_cosine: warmup_steps={warmup_steps}: the reference's class fails for warm-ups shorter than 3 "
                             "steps (it reads steps_per_epoch before its third step() call has set it)")
        return cls(_lib.LR_WARMUP_COSINE, base_lr, warmup_steps, 1, warmup_start_lr, eta_min, cos_a=warmup_steps / 3.0, cos_b=max_epochs)

    @classmethod
    def reference_exponential(cls, base_lr: float, warmup_steps: int, decay_steps: int, gamma: float = 0.999, eta_min: float = 0.0,
                              warmup_start_lr: float = 0.0) -> "LRSchedule":
        """The reference's `LinearWarmupExponentialDecayLR` stepped once per optimizer step (models/analysis.py:191-275)."""
        from . import _lib
        return cls(_lib.LR_WARMUP_EXP, base_lr, warmup_steps, 1, warmup_start_lr, eta_min, gamma=gamma, decay_steps=decay_steps)

    def to_dict(self) -> dict:
        return {k: getattr(self, k) for k in self.FIELDS}

    @classmethod
    def from_dict(cls, d: dict) -> "LRSchedule":
        return cls(**{k: d[k] for k in cls.FIELDS})

    def struct(self, swa: Optional["SWA"] = None):
        """The `agnn_lr_schedule_t` of this schedule, with `swa`'s fields (none: swa_start = -1)."""
        from . import _lib
        s = _lib.LrSchedule(**self.to_dict())
        s.swa_start, s.swa_period, s.swa_anneal, s.swa_lr = -1, 1, 0, 0.0
        if swa is not None:
            s.swa_start, s.swa_period, s.swa_anneal, s.swa_lr = swa.start_step, swa.period, swa.anneal_epochs, swa.swa_lr
        return s

    def lr_at(self, k: int, swa: Optional["SWA"] = None) -> float:
        """lr(k) in double, from `agnn_lr_schedule_at`: the function the kernel evaluates, compiled for the host (no GPU needed)."""
        import ctypes
        import math
        from . import _lib
        lib = _lib.load()
        lr = float(lib.agnn_lr_schedule_at(ctypes.byref(self.struct(swa)), int(k)))
        if math.isnan(lr):
            raise _lib.AgnnError(f"agnn_lr_schedule_at failed: {(lib.agnn_last_error() or b'').decode()}")
        return lr


class SWA:
    """Stochastic weight averaging on the optimizer's step counter: from optimizer step `start_step` on, every `period`
    steps (one SWA "epoch") the parameters as they are before that step's update enter a running average
    (`torch.optim.swa_utils.AveragedModel`'s default rule), and the rate anneals to `swa_lr` over `anneal_epochs` epochs as
    `torch.optim.swa_utils.SWALR(anneal_strategy="cos")` stepped once per epoch does.  The reference's
    `StochasticWeightAveraging(swa_lrs=5e-5, swa_epoch_start=50)` is start_step = 50 * steps_per_epoch, period =
    steps_per_epoch; parity with Lightning's callback itself is not pinned, and BatchNorm statistics are not refreshed
    (`update_bn`: out of scope — the encoders here normalise with LayerNorm)."""

    def __init__(self, start_step: int, period: int, anneal_epochs: int = 10, swa_lr: float = 5e-5):
        if start_step < 0 or period <= 0 or anneal_epochs < 0:
            raise ValueError(f"SWA: start_step={start_step}, period={period}, anneal_epochs={anneal_epochs}")
        self.start_step, self.period, self.anneal_epochs, self.swa_lr = int(start_step), int(period), int(anneal_epochs), float(swa_lr)

    def to_dict(self) -> dict:
        return dict(start_step=self.start_step, period=self.period, anneal_epochs=self.anneal_epochs, swa_lr=self.swa_lr)


class FlatAdamW:
    """AdamW over ONE flat parameter buffer (decoupled weight decay, bias correction — torch.optim.AdamW's update
    rule, reference optimizer: models/analysis.py:1380-1381).  Parameters are re-pointed at views of the buffer,
    gradients come from a `FlatGradBuffer`, so a step is a handful of whole-model elementwise launches instead of
    per-parameter lists: ~5 M parameters in ~130 tensors make the foreach path launch-bound.

    `lr`: a float (a constant of the launch: `opt.lr = x` between EAGER steps changes it, a captured step keeps the value
    it was captured with) or an `LRSchedule`, optionally with `swa=SWA(...)`: the rate is then evaluated on the device from
    the step counter (`agnn_adamw_sched_f32`), so a captured step follows the schedule, and all device state (counter,
    workspace, `last_lr` / `n_averaged`, `last_norm`, the SWA average) exists from construction on — a capture may be the
    first thing that runs."""

    def __init__(self, params: Iterable[torch.nn.Parameter], grads: FlatGradBuffer, lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, weight_decay=1e-2, swa: Optional[SWA] = None):
        self.params = [p for p in params if p.requires_grad]
        assert [id(p) for p in self.params] == [id(p) for p in grads.params], "same parameter order as the gradient buffer"
        self.grads = grads
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        dev = self.params[0].device
        self.flat = torch.zeros(grads.offsets[-1], dtype=torch.float32, device=dev)       # same 16-byte-aligned layout
        for p, o in zip(self.params, grads.offsets):
            self.flat[o:o + p.numel()] = p.detach().reshape(-1)
            p.data = self.flat[o:o + p.numel()].view_as(p)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.schedule = lr if isinstance(lr, LRSchedule) else None
        self.swa = swa
        if self.schedule is None:
            if swa is not None:
                raise ValueError("FlatAdamW: swa needs lr=LRSchedule (LRSchedule.constant(lr) for a fixed rate)")
            return
        self._sched = self.schedule.struct(swa)
        self._t = torch.zeros((), dtype=torch.float32, device=dev)
        self._state = torch.zeros(2, dtype=torch.float32, device=dev)                     # [lr the last step used, snapshots averaged]
        self._state[0] = self.schedule.lr_at(0, swa)
        self.last_norm = torch.zeros((), dtype=torch.float32, device=dev)
        self.swa_flat = torch.zeros_like(self.flat) if swa is not None else None
        if self.flat.is_cuda:
            from . import _lib
            self._ws = torch.empty(int(_lib.load().agnn_adamw_sched_workspace_bytes()), dtype=torch.uint8, device=dev)

    @property
    def last_lr(self) -> torch.Tensor:
        """The rate the last step used (before the first step: lr(0)), a device scalar: reading it here costs no sync."""
        return self._scheduled("last_lr")._state[0]

    @property
    def n_averaged(self) -> torch.Tensor:
        """Snapshots in `swa_flat` so far, a device scalar (float, as the kernel counts them)."""
        return self._scheduled("n_averaged")._state[1]

    def current_lr(self) -> float:
        """The rate the NEXT step will use, as a host float (float path: `opt.lr`; with a schedule this reads the counter)."""
        if self.schedule is None:
            return float(self.lr)
        return self.schedule.lr_at(int(self._t.item()), self.swa)

    def _scheduled(self, what: str) -> "FlatAdamW":
        if self.schedule is None:
            raise AttributeError(f"FlatAdamW.{what} needs lr=LRSchedule")
        return self

    @torch.no_grad()
    def swap_swa_(self) -> None:
        """Copy the SWA average into the flat parameters (what the callback does at the end of fit).  In place: the model's
        parameters are views of `flat`.  BatchNorm statistics are not refreshed (`update_bn` is out of scope)."""
        if self.swa is None:
            raise AttributeError("FlatAdamW.swap_swa_ needs swa=SWA(...)")
        if int(self._state[1].item()) == 0:                  # end of fit: the one host read is no cost there
            raise RuntimeError("FlatAdamW.swap_swa_: no snapshot has been averaged yet")
        self.flat.copy_(self.swa_flat)

    def state_dict(self) -> dict:
        """Everything a run needs to resume: parameters, moments, step counter, the schedule / SWA hyper-parameters, the average
        and its count (clones; the layout is this optimizer's flat layout).  Not a `torch.optim` / Lightning optimizer
        checkpoint: resuming from one of the reference's is not provided."""
        t = getattr(self, "_t", None)
        d = {"flat": self.flat.clone(), "m": self.m.clone(), "v": self.v.clone(),
             "step": t.clone() if t is not None else torch.zeros((), dtype=torch.float32, device=self.flat.device),
             "lr": None if self.schedule is not None else float(self.lr),
             "schedule": self.schedule.to_dict() if self.schedule is not None else None,
             "swa": self.swa.to_dict() if self.swa is not None else None}
        if self.schedule is not None:
            d["state"] = self._state.clone()
        if self.swa is not None:
            d["swa_flat"] = self.swa_flat.clone()
        return d

    @torch.no_grad()
    def load_state_dict(self, d: dict) -> None:
        """Write a `state_dict()` into the EXISTING buffers, so a captured graph stays valid and resumes at the saved step.
        The schedule and SWA hyper-parameters are constants of the launch: they must equal this optimizer's."""
        if d["flat"].numel() != self.flat.numel():
            raise ValueError(f"load_state_dict: {d['flat'].numel()} parameters saved, {self.flat.numel()} here")
        mine = (self.schedule.to_dict() if self.schedule is not None else None, self.swa.to_dict() if self.swa is not None else None)
        if (d["schedule"], d["swa"]) != mine:
            raise ValueError("load_state_dict: the saved schedule / SWA hyper-parameters differ from this optimizer's (they are constants "
                             f"of the launch; construct FlatAdamW with them): saved {(d['schedule'], d['swa'])}, here {mine}")
        if not hasattr(self, "_t"):
            self._t = torch.zeros((), dtype=torch.float32, device=self.flat.device)
        for dst, key in ((self.flat, "flat"), (self.m, "m"), (self.v, "v"), (self._t, "step")):
            dst.copy_(d[key])
        if self.schedule is None:
            self.lr = d["lr"]
        else:
            self._state.copy_(d["state"])
        if self.swa is not None:
            self.swa_flat.copy_(d["swa_flat"])

    @torch.no_grad()
    def step(self, max_norm: float = 0.0) -> None:
        """One AdamW update; `max_norm > 0` first clips the global gradient norm (clip_grad_norm_ semantics).
        Graph-capturable: the step counter and the bias corrections live on the device, and with an `LRSchedule` so do the
        rate and the SWA bookkeeping.  On a GPU the whole thing is the two launches of `agnn_adamw_f32` /
        `agnn_adamw_sched_f32`; on CPU tensors (gloo tests) the same arithmetic in torch ops."""
        if not hasattr(self, "_t"):
            self._t = torch.zeros((), dtype=torch.float32, device=self.flat.device)
        g = self.grads.flat
        if self.flat.is_cuda:
            import ctypes
            from . import _lib
            lib = _lib.load()
            if self.schedule is not None:
                _lib.check(lib.agnn_adamw_sched_f32(self.flat.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                                    self.flat.numel(), ctypes.byref(self._sched), float(self.betas[0]),
                                                    float(self.betas[1]), float(self.eps), float(self.wd), float(max_norm),
                                                    self._t.data_ptr(), _lib.ptr(self.swa_flat), self._state.data_ptr(),
                                                    self.last_norm.data_ptr(), 0, self._ws.data_ptr(), self._ws.numel(),
                                                    _lib.stream_ptr(self.flat.device)), "agnn_adamw_sched_f32")
                return
            if not hasattr(self, "_ws"):
                self._ws = torch.empty(int(lib.agnn_adamw_workspace_bytes()), dtype=torch.uint8, device=self.flat.device)
                self.last_norm = torch.zeros((), dtype=torch.float32, device=self.flat.device)
            _lib.check(lib.agnn_adamw_f32(self.flat.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.flat.numel(),
                                          float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.wd),
                                          float(max_norm), self._t.data_ptr(), self.last_norm.data_ptr(), 0, self._ws.data_ptr(),
                                          self._ws.numel(), _lib.stream_ptr(self.flat.device)), "agnn_adamw_f32")
            return
        lr = self.lr
        if self.schedule is not None:                        # the kernel's rule: lr(k) in double, rounded to float once
            k = int(self._t)
            lr = float(torch.tensor(self.schedule.lr_at(k, self.swa), dtype=torch.float64).float())
            self._state[0] = lr
            if self.swa is not None and k >= self.swa.start_step and (k - self.swa.start_step) % self.swa.period == 0:
                n = float(self._state[1])
                if n == 0:
                    self.swa_flat.copy_(self.flat)
                else:
                    self.swa_flat.add_((self.flat - self.swa_flat) / (n + 1.0))
                self._state[1] = n + 1.0
        if max_norm > 0:
            total = self.grads.clip_norm_(max_norm)
            if self.schedule is not None:
                self.last_norm.copy_(total)
        b1, b2 = self.betas
        self._t += 1.0
        bc1 = 1.0 - (b1 ** self._t)
        bc2 = 1.0 - (b2 ** self._t)
        self.flat.mul_(1.0 - lr * self.wd)
        self.m.mul_(b1).add_(g, alpha=1.0 - b1)
        self.v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
        denom = (self.v.sqrt() / bc2.sqrt()).add_(self.eps)
        self.flat.addcdiv_(self.m / bc1, denom, value=-lr)


def enable_wgrad_overlap(flag: bool = True, scope="all") -> None:
    """Issue weight-gradient GEMMs on their own HIP stream (joined in FlatGradBuffer.pack).  Requires gradients to be
    None when backward starts — FlatGradBuffer(views=False).zero() — see linear.py."""
    from . import linear
    linear.enable_wgrad_overlap(flag, scope)


def defer_weight_grads(flag: bool = True) -> None:
    """Weight / bias gradients of the projections on the backward pass's own stream are postponed to where that stream
    would otherwise idle (linear.defer_weight_grads); `FlatGradBuffer.pack` runs whatever is still pending."""
    from .linear import defer_weight_grads as _set
    _set(flag)


def fill_missing_grads(module_or_params) -> int:
    """Give every trainable parameter that took no gradient this step a ZERO gradient; returns how many.  The encoders prune
    structurally dead branches (hgt._HGTCore: a node type nothing reads; encoders.HeteroConv: a layer that keeps no edge hands
    zeros itself), where the reference's graph still reaches those parameters through empty index ops and gives zeros.
    `torch.optim.AdamW` SKIPS a parameter whose grad is None (no weight decay, no moment decay), so a stock optimizer
    reproduces the reference's update only after this call; FlatGradBuffer.pack + FlatAdamW substitute zeros themselves."""
    params = module_or_params.parameters() if isinstance(module_or_params, torch.nn.Module) else module_or_params
    n = 0
    for p in params:
        if p.requires_grad and p.grad is None:
            p.grad = torch.zeros_like(p)
            n += 1
    return n


def barrier_and_sync() -> None:
    if dist.is_initialized():
        dist.barrier()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def max_over_ranks(x: float) -> float:
    if not (dist.is_initialized() and dist.get_world_size() > 1):
        return x
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    t = torch.tensor([x], dtype=torch.float64, device=dev)  # tiny scalar exchange, outside the timed region
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())
