"""Global multi-head self-attention of the graph-transformer layers (core_layers.GPSLayer / HGPSLayer; reference
models/core/gnn.py:471, core/hgnn.py:273) on the HIP kernels of csrc/attn.hip.

The reference calls `nn.MultiheadAttention` on the whole batch as one unbatched sequence of N tokens (no mask: attention crosses
the subgraphs of a batch), which materialises heads x N x N scores.  Here the module only holds the parameters (its forward is
never called, so `attn.in_proj_weight`, `attn.in_proj_bias`, `attn.out_proj.weight`, `attn.out_proj.bias` keep the reference's
names): the in-projection is ONE `linear.linear` to [N, 3E], `agnn_attn_fwd_f32` reads its three column blocks where they lie and
writes the heads side by side, `out_proj` is a second `linear.linear`.  The backward (`agnn_attn_bwd_f32`) writes dq | dk | dv as
the column blocks of one [N, 3E] tensor: the in-projection's dY as it stands.

Saved for the backward, per call: the [N, 3E] projections, o [N, E], lse [heads, N] and, under dropout, the (seed, step) pair the
forward drew from (`rng_used`); the masks are regenerated from it.  Everything is allocated with torch inside the call (a first
use under capture belongs to that graph).

Unlike the hand GEMMs there is no minimum-rows rule: the kernel is the path at every N (`kernel_applicable` looks at shapes,
dtype and device only).  `FUSED = False` runs `F.scaled_dot_product_attention` on the same projections (A/B timing, cross-checks;
its dropout masks are torch's, not this library's)."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib, fused, linear

FUSED = True                     # A/B switch: False runs the library body (F.scaled_dot_product_attention)
HEAD_WIDTHS = (8, 16, 32, 64)    # csrc/attn.hip's instantiations


def kernel_applicable(x: torch.Tensor, heads: int) -> bool:
    """Shapes, dtype and device only (works on meta tensors).  x: the [N, E] input of the attention."""
    if x.dim() != 2 or heads < 1 or x.shape[0] < 1 or x.shape[1] % heads:
        return False
    return x.device.type == "cuda" and x.dtype == torch.float32 and (x.shape[1] // heads) in HEAD_WIDTHS


def _blocks(t: torch.Tensor, E: int):
    """The three [N, E] column blocks of a [N, 3E] tensor."""
    return t[:, :E], t[:, E:2 * E], t[:, 2 * E:3 * E]


def _check_blocks(who: str, shape, heads: int, ld: int, *ts: torch.Tensor) -> None:
    if heads < 1 or shape[1] % heads:
        raise _lib.AgnnError(f"{who}: width {shape[1]} is not a multiple of heads = {heads}")
    for t in ts:
        if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != tuple(shape) or t.stride(1) != 1 or t.stride(0) != ld:
            raise _lib.AgnnError(f"{who}: fp32 {tuple(shape)} blocks with unit column stride and one common row stride expected")


def forward_raw(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, p: float = 0.0, call_id: int = 0,
                out: Optional[torch.Tensor] = None, q_rows: int = 0):
    """(o, lse, rng_used) of `agnn_attn_fwd_f32`.  q, k, v: [N, E] views with one common row stride; `out`: where o goes (a
    [N, E] view) or None for a fresh tensor.  rng_used is None at p == 0."""
    dev = _lib.require_gpu(q, k, v, out)
    lib = _lib.load()
    N, E = q.shape
    _check_blocks("attention.forward_raw", q.shape, heads, q.stride(0), q, k, v)
    D = E // heads
    o = torch.empty((N, E), dtype=torch.float32, device=dev) if out is None else out
    _check_blocks("attention.forward_raw", q.shape, heads, o.stride(0), o)
    lse = torch.empty((heads, N), dtype=torch.float32, device=dev)
    rng = fused.rng_state(dev) if p > 0 else None
    used = torch.empty(2, dtype=torch.int64, device=dev) if p > 0 else None
    _lib.check(lib.agnn_attn_fwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), N, heads, D, 1.0 / math.sqrt(D), float(p),
                                     _lib.ptr(rng), int(call_id), int(q_rows), o.data_ptr(), o.stride(0), lse.data_ptr(), _lib.ptr(used),
                                     _lib.stream_ptr(dev)), "agnn_attn_fwd_f32")
    return o, lse, used


def backward_raw(q, k, v, heads: int, o, lse, dO, dq, dk, dv, p: float = 0.0, call_id: int = 0, rng_used=None, q_rows: int = 0) -> None:
    """`agnn_attn_bwd_f32` into dq, dk, dv ([N, E] views with one common row stride)."""
    dev = _lib.require_gpu(q, k, v, o, lse, dO, dq, dk, dv)
    lib = _lib.load()
    N, E = q.shape
    _check_blocks("attention.backward_raw", q.shape, heads, q.stride(0), q, k, v)
    _check_blocks("attention.backward_raw", q.shape, heads, dq.stride(0), dq, dk, dv)
    _check_blocks("attention.backward_raw", q.shape, heads, o.stride(0), o)
    _check_blocks("attention.backward_raw", q.shape, heads, dO.stride(0), dO)
    if tuple(lse.shape) != (heads, N) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise _lib.AgnnError("attention.backward_raw: lse must be the forward's contiguous fp32 [heads, N]")
    D = E // heads
    nws = int(lib.agnn_attn_bwd_workspace_bytes(N, heads))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _lib.check(lib.agnn_attn_bwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), N, heads, D, 1.0 / math.sqrt(D), float(p),
                                     _lib.ptr(rng_used), int(call_id), int(q_rows), dO.data_ptr(), dO.stride(0), o.data_ptr(), o.stride(0),
                                     lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dq.stride(0), ws.data_ptr(), nws,
                                     _lib.stream_ptr(dev)), "agnn_attn_bwd_f32")


def dropout_keep(N: int, heads: int, p: float, rng_used: Optional[torch.Tensor], call_id: int, device) -> torch.Tensor:
    """The keep factors (0 or 1 / (1 - p)) a forward with (rng_used, call_id) applied, dense [heads, N, N] (small N only)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.AgnnError("attention.dropout_keep: a HIP device is needed")
    keep = torch.empty((heads, N, N), dtype=torch.float32, device=device)
    _lib.check(_lib.load().agnn_attn_dropout_keep_f32(N, heads, float(p), _lib.ptr(rng_used), int(call_id), keep.data_ptr(),
                                                      _lib.stream_ptr(device)), "agnn_attn_dropout_keep_f32")
    return keep


class _AttnFn(torch.autograd.Function):
    """o [N, E] from the [N, 3E] in-projection (q | k | v); dqkv [N, 3E] back.  The call id and the forward's rng_used are kept
    with the node: together they name the dropout masks that were drawn.  No double backward."""

    @staticmethod
    def forward(ctx, qkv, heads: int, p: float, call_id: int, q_rows: int):
        E = qkv.shape[1] // 3
        q, k, v = _blocks(qkv, E)
        o, lse, used = forward_raw(q, k, v, heads, p, call_id, q_rows=q_rows)
        ctx.cfg = (int(heads), float(p), int(call_id), int(q_rows))
        ctx.save_for_backward(qkv, o, lse, *([used] if used is not None else []))
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, dO):
        qkv, o, lse, *used = ctx.saved_tensors
        heads, p, call_id, q_rows = ctx.cfg
        E = o.shape[1]
        dO = _lib.rows16(dO)
        dqkv = torch.empty_like(qkv)
        backward_raw(*_blocks(qkv, E), heads, o, lse, dO, *_blocks(dqkv, E), p=p, call_id=call_id, rng_used=used[0] if used else None,
                     q_rows=q_rows)
        return dqkv, None, None, None, None


def attention(qkv: torch.Tensor, heads: int, p: float = 0.0, call_id: Optional[int] = None, q_rows: int = 0) -> torch.Tensor:
    """softmax(q k^T / sqrt(D)) v per head on the kernels; qkv [N, 3E] fp32, dropout p on the probabilities.  `call_id` names
    the dropout masks (None: the next id of the library's call-site counter; a caller that wants to rebuild the masks with
    `dropout_keep` passes its own); `q_rows`: query rows per workgroup, 0 = the kernel's own rule, 64 or 128 (timing, tests)."""
    _lib.require_gpu(qkv)
    if qkv.dim() != 2 or qkv.shape[1] % 3 or not kernel_applicable(qkv[:, :qkv.shape[1] // 3], heads):
        raise _lib.AgnnError(f"attention: no kernel for qkv {tuple(qkv.shape)} {qkv.dtype} with {heads} heads "
                             f"(fp32, head widths {HEAD_WIDTHS})")
    qkv = _lib.rows16(qkv)
    if call_id is None:
        call_id = next(fused._CALL_IDS)
    return _AttnFn.apply(qkv, heads, float(p), int(call_id) & 0xFFFFFFFF, int(q_rows))


def _library_attention(qkv: torch.Tensor, heads: int, p: float) -> torch.Tensor:
    N, E3 = qkv.shape
    E = E3 // 3
    q, k, v = (t.reshape(N, heads, E // heads).transpose(0, 1) for t in _blocks(qkv, E))
    o = F.scaled_dot_product_attention(q, k, v, dropout_p=p)
    return o.transpose(0, 1).reshape(N, E)


def self_attention(mha: nn.MultiheadAttention, x: torch.Tensor, training: bool) -> torch.Tensor:
    """`mha(x, x, x)[0]` for a 2-D x [N, E] (torch's unbatched sequence: every row attends to every row).  `mha` is the
    parameter holder only; its attention dropout acts when `training`."""
    _lib.require_gpu(x)
    if x.dim() != 2 or x.shape[1] != mha.embed_dim:
        raise _lib.AgnnError(f"self_attention: [N, {mha.embed_dim}] input expected, got {tuple(x.shape)}")
    if not mha._qkv_same_embed_dim or mha.bias_k is not None or mha.bias_v is not None or mha.add_zero_attn:
        raise _lib.AgnnError("self_attention: plain self-attention expected (kdim = vdim = embed_dim, no bias_k / bias_v, no zero row)")
    heads = int(mha.num_heads)
    p = float(mha.dropout) if training else 0.0
    qkv = linear.linear(x, mha.in_proj_weight, mha.in_proj_bias)
    if FUSED and kernel_applicable(x, heads):
        o = attention(qkv, heads, p)
    else:
        o = _library_attention(qkv, heads, p)
    return linear.linear(o, mha.out_proj.weight, mha.out_proj.bias)
