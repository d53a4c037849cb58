"""Cross-task attention of the logit-fusion block (heads.CrossTaskTransformer; reference models/analysis.py:408-418) on the HIP
kernels of csrc/taskattn.hip.

The reference calls `nn.MultiheadAttention(batch_first=True)` on [N, T, E]: N independent sequences of the T task tokens of a
note.  Here the packed in-projection [N T, 3E] (one `linear.linear`) is read where it lies, row n T + t = token t of note n,
and o [N T, E] comes out with the heads side by side: the out-projection's input as it stands.  The backward writes dqkv
[N T, 3E], the in-projection's dY.  No [N, h, T, d] copy and nothing of size N x heads x T x T exists in either direction.

Saved for the backward, per call: qkv, o (the out-projection keeps it anyway), lse [N T, heads] and, under dropout, the
(seed, step) pair the forward drew from (`rng_used`); the masks are redrawn from it.  A forward that needs no gradient asks for
no lse.  Everything is allocated with torch inside the call (a first use under capture belongs to that graph).

The kernel is the path at every shape it serves (`kernel_applicable` looks at shapes, dtype and device only).  `FUSED = False`
runs the library body in heads.CrossTaskTransformer (A/B timing, cross-checks; its dropout masks are torch's)."""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib, fused

FUSED = True                 # A/B switch: False runs the library body (F.scaled_dot_product_attention)
HEAD_WIDTHS = (8, 16, 32)    # csrc/taskattn.hip's instantiations
MAX_TOKENS = _lib.MAX_SEG    # tokens per sequence
MAX_WIDTH = 128              # heads * D
MAX_LANES = 256              # heads * T: one lane per (head, token) of a sequence


def kernel_applicable(n_seq: int, T: int, heads: int, E: int, dtype, device) -> bool:
    """Shapes, dtype and device only.  n_seq = 0 is served (nothing is launched)."""
    if n_seq < 0 or heads < 1 or E < 1 or E % heads or not 1 <= T <= MAX_TOKENS:
        return False
    if (E // heads) not in HEAD_WIDTHS or E > MAX_WIDTH or heads * T > MAX_LANES:
        return False
    return torch.device(device).type == "cuda" and dtype == torch.float32


def _check(who: str, qkv: torch.Tensor, T: int, heads: int) -> tuple:
    if qkv.dim() != 2 or qkv.shape[1] % 3 or T < 1 or qkv.shape[0] % T:
        raise _lib.AgnnError(f"{who}: qkv [n_seq * T, 3E] expected, got {tuple(qkv.shape)} with T = {T}")
    n_seq, E = qkv.shape[0] // T, qkv.shape[1] // 3
    if not kernel_applicable(n_seq, T, heads, E, qkv.dtype, qkv.device):
        raise _lib.AgnnError(f"{who}: no kernel for qkv {tuple(qkv.shape)} {qkv.dtype} on {qkv.device} with T = {T}, {heads} heads (fp32, head "
                             f"widths {HEAD_WIDTHS}, T <= {MAX_TOKENS}, E <= {MAX_WIDTH}, heads * T <= {MAX_LANES})")
    return n_seq, E


def forward_raw(qkv: torch.Tensor, T: int, heads: int, p: float = 0.0, call_id: int = 0, out: Optional[torch.Tensor] = None,
                want_lse: bool = True):
    """(o, lse, rng_used) of `agnn_taskattn_fwd_f32`.  qkv: [n_seq T, 3E] (a column block of a wider buffer is fine); `out`: where
    o goes (a [n_seq T, E] view) or None for a fresh tensor.  lse is None unless wanted, rng_used is None at p == 0."""
    dev = _lib.require_gpu(qkv, out)
    n_seq, E = _check("task_attention.forward_raw", qkv, T, heads)
    D = E // heads
    o = torch.empty((n_seq * T, E), dtype=torch.float32, device=dev) if out is None else out
    if tuple(o.shape) != (n_seq * T, E) or o.dtype != torch.float32 or (n_seq and not (_lib.rows_ok(qkv) and _lib.rows_ok(o))):
        raise _lib.AgnnError("task_attention.forward_raw: fp32 rows with unit column stride, 16-byte aligned, o [n_seq * T, E] expected")
    lse = torch.empty((n_seq * T, heads), dtype=torch.float32, device=dev) if want_lse else None
    rng = fused.rng_state(dev) if p > 0 else None
    used = torch.empty(2, dtype=torch.int64, device=dev) if p > 0 else None
    _lib.check(_lib.load().agnn_taskattn_fwd_f32(qkv.data_ptr(), qkv.stride(0), n_seq, T, heads, D, 1.0 / math.sqrt(D), float(p), _lib.ptr(rng),
                                                 int(call_id), o.data_ptr(), o.stride(0), _lib.ptr(lse), _lib.ptr(used), _lib.stream_ptr(dev)),
               "agnn_taskattn_fwd_f32")
    return o, lse, used


def backward_raw(qkv: torch.Tensor, T: int, heads: int, o: torch.Tensor, lse: torch.Tensor, dO: torch.Tensor, dqkv: torch.Tensor,
                 p: float = 0.0, call_id: int = 0, rng_used: Optional[torch.Tensor] = None) -> None:
    """`agnn_taskattn_bwd_f32` into dqkv ([n_seq T, 3E], every element written)."""
    dev = _lib.require_gpu(qkv, o, lse, dO, dqkv, rng_used)
    n_seq, E = _check("task_attention.backward_raw", qkv, T, heads)
    D = E // heads
    for name, t, w in (("o", o, E), ("dO", dO, E), ("dqkv", dqkv, 3 * E), ("qkv", qkv, 3 * E)):
        if tuple(t.shape) != (n_seq * T, w) or t.dtype != torch.float32 or (n_seq and not _lib.rows_ok(t)):
            raise _lib.AgnnError(f"task_attention.backward_raw: {name} must be fp32 [{n_seq * T}, {w}] with unit column stride and 16-byte aligned rows")
    if tuple(lse.shape) != (n_seq * T, heads) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise _lib.AgnnError("task_attention.backward_raw: lse must be the forward's contiguous fp32 [n_seq * T, heads]")
    _lib.check(_lib.load().agnn_taskattn_bwd_f32(qkv.data_ptr(), qkv.stride(0), n_seq, T, heads, D, 1.0 / math.sqrt(D), float(p),
                                                 _lib.ptr(rng_used), int(call_id), dO.data_ptr(), dO.stride(0), o.data_ptr(), o.stride(0),
                                                 lse.data_ptr(), dqkv.data_ptr(), dqkv.stride(0), _lib.stream_ptr(dev)), "agnn_taskattn_bwd_f32")


def dropout_keep(n_seq: int, T: int, heads: int, p: float, rng_used: Optional[torch.Tensor], call_id: int, device) -> torch.Tensor:
    """The keep factors (0 or 1 / (1 - p)) a forward with (rng_used, call_id) applied, dense [n_seq, heads, T, T]."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.AgnnError("task_attention.dropout_keep: a HIP device is needed")
    keep = torch.empty((n_seq, heads, T, T), dtype=torch.float32, device=device)
    _lib.check(_lib.load().agnn_taskattn_dropout_keep_f32(n_seq, T, heads, float(p), _lib.ptr(rng_used), int(call_id), keep.data_ptr(),
                                                          _lib.stream_ptr(device)), "agnn_taskattn_dropout_keep_f32")
    return keep


class _TaskAttnFn(torch.autograd.Function):
    """o [n_seq T, E] from the packed in-projection [n_seq T, 3E]; dqkv back.  The call id and the forward's rng_used are kept with
    the node: together they name the dropout masks that were drawn.  No double backward."""

    @staticmethod
    def forward(ctx, qkv, T: int, heads: int, p: float, call_id: int, need: bool):
        o, lse, used = forward_raw(qkv, T, heads, p, call_id, want_lse=need)
        ctx.cfg = (int(T), int(heads), float(p), int(call_id))
        if need:
            ctx.save_for_backward(qkv, o, lse, *([used] if used is not None else []))
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, dO):
        qkv, o, lse, *used = ctx.saved_tensors
        T, heads, p, call_id = ctx.cfg
        E = o.shape[1]
        dO = _lib.rows16(dO)
        dqkv = torch.empty_like(qkv)
        backward_raw(qkv, T, heads, o, lse, dO, dqkv, p=p, call_id=call_id, rng_used=used[0] if used else None)
        return dqkv, None, None, None, None, None


def attention(qkv: torch.Tensor, T: int, heads: int, p: float = 0.0, call_id: Optional[int] = None) -> torch.Tensor:
    """softmax(q k^T / sqrt(D)) v per (sequence, head) on the kernels: qkv [n_seq T, 3E] fp32 -> o [n_seq T, E]; dropout p on the
    probabilities.  `call_id` names the dropout masks (None: the next id of the library's call-site counter; a caller that
    wants to rebuild the masks with `dropout_keep` passes its own)."""
    _lib.require_gpu(qkv)
    _check("task_attention.attention", qkv, T, heads)
    qkv = _lib.rows16(qkv)
    if call_id is None:
        call_id = next(fused._CALL_IDS)
    need = torch.is_grad_enabled() and qkv.requires_grad          # a forward that needs no gradient writes no lse
    return _TaskAttnFn.apply(qkv, int(T), int(heads), float(p), int(call_id) & 0xFFFFFFFF, need)
