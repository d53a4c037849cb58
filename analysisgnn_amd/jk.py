"""JumpingKnowledge (core_layers.JumpingKnowledge; reference models/core/gnn.py:345-365) on the HIP kernels of csrc/lstm.hip.

The bidirectional LSTM runs over the T layer outputs of every row: one `agnn_lstm_step_f32` launch per time step carries both
directions (the forward one at t = s, the reverse one at t = T - 1 - s), applies the cell in the GEMM's epilogue and leaves the
attention score's partial dot products; `agnn_jk_combine_fwd_f32` sums them, takes the softmax over the steps and forms the
weighted sum of the layer outputs, which are read where they lie (no stack).  The backward pass is `agnn_jk_combine_bwd_f32`,
then per step (last to first) `agnn_lstm_cell_bwd_f32` and the two input-gradient products on `agnn_gemm_nn_f32`, then the
weight gradients through `linear.weight_grad_batch` and one `agnn_pack_f32` launch per group of sums.

`att.bias` adds the same constant to the score of every step, so it cancels in the softmax: the kernels never read it and its
gradient is delivered as exact zeros (autograd on the library path leaves a rounding-level residue there instead).

Saved for the backward, per call: act 2 T M 4h floats, c and h 2 T M h each, alpha M T, and the attention partials
2 T M (h / 32).  All of it is allocated with torch inside the call (a first use under capture belongs to that graph)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, linear

FUSED = True             # A/B switch: False runs core_layers.JumpingKnowledge's library body
MIN_ROWS = 4096          # linear.HAND_GEMM_MIN_ROWS' value: the same 128 x 128 tile (not measured separately for this kernel)
MAX_HIDDEN = 1024


def shapes_applicable(n_hidden: int, h: int, T: int, rows: int) -> bool:
    """The size rule alone: T steps of width n_hidden, h hidden units per direction, `rows` rows."""
    return (2 <= T <= _lib.JK_MAX_T and n_hidden > 0 and n_hidden % 16 == 0 and h > 0 and h % 32 == 0 and h <= MAX_HIDDEN
            and n_hidden + h <= linear.HAND_GEMM_MAX_K and rows >= max(MIN_ROWS, 1))


def kernel_applicable(module, xs) -> bool:
    """Shapes, dtype and device only (no data is looked at: works on meta tensors)."""
    if not isinstance(xs, (list, tuple)) or len(xs) == 0:
        return False
    H, h = int(module.lstm.input_size), int(module.lstm.hidden_size)
    x0 = xs[0]
    if x0.dim() != 2 or x0.shape[1] != H or not shapes_applicable(H, h, len(xs), int(x0.shape[0])):
        return False
    w = module.att.weight
    if w.shape[1] != 2 * h or w.dtype != torch.float32 or w.device.type != "cuda":
        return False
    for x in xs:
        if not (x.device.type == "cuda" and x.dtype == torch.float32 and tuple(x.shape) == tuple(x0.shape) and x.stride(1) == 1):
            return False
    return True


def _params(module):
    l = module.lstm
    ps = [l.weight_ih_l0, l.weight_hh_l0, l.bias_ih_l0, l.bias_hh_l0,
          l.weight_ih_l0_reverse, l.weight_hh_l0_reverse, l.bias_ih_l0_reverse, l.bias_hh_l0_reverse]
    return ps + [module.att.weight, module.att.bias]


def _forward(xs, P, save: bool):
    """(out, saved state or None).  P: the eight LSTM parameters (forward direction first), att.weight, att.bias."""
    lib = _lib.load()
    dev = xs[0].device
    st = _lib.stream_ptr(dev)
    T, (M, H) = len(xs), xs[0].shape
    h = P[1].shape[1]
    nt = h // 32
    W = [_lib.vec16(p.detach()) for p in P[:9]]
    att_w = W[8]
    f32 = dict(dtype=torch.float32, device=dev)
    hbuf = torch.empty((2, T, M, h), **f32)          # step order: direction 1's step s is t = T - 1 - s
    cbuf = torch.empty((2, T, M, h), **f32)
    act = torch.empty((2, T, M, 4 * h), **f32) if save else None
    part = torch.empty((2, T, M, nt), **f32)
    for s in range(T):
        items = (_lib.LstmStep * 2)()
        for d, it in enumerate(items):
            t = s if d == 0 else T - 1 - s
            x = xs[t]
            it.x, it.ld_x = x.data_ptr(), x.stride(0)
            if s:
                it.hprev, it.ld_hprev, it.cprev, it.ld_cprev = hbuf[d, s - 1].data_ptr(), h, cbuf[d, s - 1].data_ptr(), h
            it.w_ih, it.w_hh, it.b_ih, it.b_hh = (W[4 * d + k].data_ptr() for k in range(4))
            it.hout, it.ld_hout, it.cout, it.ld_cout = hbuf[d, s].data_ptr(), h, cbuf[d, s].data_ptr(), h
            it.act = act[d, s].data_ptr() if save else None
            it.att_w = att_w.data_ptr() + 4 * d * h
            it.part = part[d, t].data_ptr()
            it.M, it.K0, it.h = M, H, h
        _lib.check(lib.agnn_lstm_step_f32(2, items, st), "agnn_lstm_step_f32")
    out = torch.empty((M, H), **f32)
    alpha = torch.empty((M, T), **f32)
    px = (C.c_void_p * T)(*[x.data_ptr() for x in xs])
    lx = (C.c_int64 * T)(*[x.stride(0) for x in xs])
    _lib.check(lib.agnn_jk_combine_fwd_f32(T, px, lx, M, H, part.data_ptr(), 2, nt, alpha.data_ptr(), out.data_ptr(), H, st),
               "agnn_jk_combine_fwd_f32")
    return out, ((hbuf, cbuf, act, alpha) if save else None)


def _gemm_nn(lib, a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, st) -> None:
    """out = a w with w [K, N] as it lies: the hand-written kernel where N % 64 == 0 (K = 4h always fits), else the library."""
    if w.shape[1] % 64 == 0 and w.shape[0] % 16 == 0:
        _lib.check(lib.agnn_gemm_nn_f32(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), None, a.shape[0], w.shape[1], w.shape[0],
                                        out.data_ptr(), out.stride(0), st), "agnn_gemm_nn_f32")
    else:
        torch.mm(a, w, out=out)


class _JKFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, T, *args):
        xs, P = args[:T], args[T:]
        out, state = _forward(xs, P, True)
        ctx.T = T
        ctx.save_for_backward(*xs, *P[:9], *state)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .params import pack
        T = ctx.T
        sv = ctx.saved_tensors
        xs, P, (hbuf, cbuf, act, alpha) = sv[:T], sv[T:T + 9], sv[T + 9:]
        lib = _lib.load()
        dev = dout.device
        st = _lib.stream_ptr(dev)
        M, H = xs[0].shape
        h = P[1].shape[1]
        W = [_lib.vec16(p.detach()) for p in P]
        att_w = W[8]
        f32 = dict(dtype=torch.float32, device=dev)
        dout = _lib.rows16(dout)
        need_dx = any(ctx.needs_input_grad[1:1 + T])
        need_dp = any(ctx.needs_input_grad[1 + T:1 + T + 9])

        # attention: dscore and the direct term alpha_t dout (tmp[0]); tmp[1 + d] takes direction d's dgates W_ih
        tmp = torch.empty((3, T, M, H), **f32)
        dscore = torch.empty((M, T), **f32)
        px = (C.c_void_p * T)(*[x.data_ptr() for x in xs])
        lx = (C.c_int64 * T)(*[x.stride(0) for x in xs])
        pd = (C.c_void_p * T)(*[tmp[0, t].data_ptr() for t in range(T)])
        ld = (C.c_int64 * T)(*([H] * T))
        _lib.check(lib.agnn_jk_combine_bwd_f32(T, px, lx, M, H, alpha.data_ptr(), dout.data_ptr(), dout.stride(0), dscore.data_ptr(),
                                               pd, ld, st), "agnn_jk_combine_bwd_f32")

        nrb = int(lib.agnn_lstm_cell_bwd_row_blocks(M))
        dgates = torch.empty((2, T, M, 4 * h), **f32)
        wpart = torch.empty((2, T, nrb, h), **f32)
        dh = [None, None]
        dc = [None, None]
        for s in range(T - 1, -1, -1):
            items = (_lib.LstmCellBwd * 2)()
            dc_prev = [torch.empty((M, h), **f32) if s else None for _ in range(2)]
            for d, it in enumerate(items):
                t = s if d == 0 else T - 1 - s
                it.act, it.c, it.ld_c = act[d, s].data_ptr(), cbuf[d, s].data_ptr(), h
                if s:
                    it.cprev, it.ld_cprev = cbuf[d, s - 1].data_ptr(), h
                    it.dc_prev, it.ld_dc_prev = dc_prev[d].data_ptr(), h
                if dh[d] is not None:
                    it.dh, it.ld_dh, it.dc_next, it.ld_dc_next = dh[d].data_ptr(), h, dc[d].data_ptr(), h
                it.dscore, it.ld_dscore = dscore.data_ptr() + 4 * t, T
                it.att_w = att_w.data_ptr() + 4 * d * h
                it.dgates, it.wpart = dgates[d, s].data_ptr(), wpart[d, s].data_ptr()
                it.M, it.h = M, h
            _lib.check(lib.agnn_lstm_cell_bwd_f32(2, items, st), "agnn_lstm_cell_bwd_f32")
            for d in range(2):
                t = s if d == 0 else T - 1 - s
                if s:                                # dh_{s-1} = dgates_s W_hh (skipped at each direction's first step)
                    nxt = torch.empty((M, h), **f32)
                    _gemm_nn(lib, dgates[d, s], W[4 * d + 1], nxt, st)
                    dh[d], dc[d] = nxt, dc_prev[d]
                if need_dx:
                    _gemm_nn(lib, dgates[d, s], W[4 * d], tmp[1 + d, t], st)

        grads = [None] * (T + 10)
        if need_dx:                                  # dx_t = alpha_t dout + dgates_fwd W_ih_fwd + dgates_rev W_ih_rev: one launch
            dx = torch.empty((T, M, H), **f32)
            pack([(dx[t], [tmp[0, t], tmp[1, t], tmp[2, t]]) for t in range(T)], dev)
            for t in range(T):
                grads[t] = dx[t] if ctx.needs_input_grad[1 + t] else None
        if need_dp:
            dw_ih_s = torch.empty((2, T, 4 * h, H), **f32)
            db_s = torch.empty((2, T, 4 * h), **f32)
            dw_ih = torch.empty((2, 4 * h, H), **f32)
            dw_hh = torch.empty((2, 4 * h, h), **f32)
            db = torch.empty((2, 2, 4 * h), **f32)
            datt = torch.empty((1, 2 * h), **f32)
            wg = []
            for d in range(2):
                for s in range(T):
                    wg.append(linear.WgItem(dgates[d, s], xs[s if d == 0 else T - 1 - s], True, dw_ih_s[d, s], db_s[d, s]))
                # each direction's h and dgates are contiguous in step order: dW_hh is ONE product over (T - 1) M rows
                wg.append(linear.WgItem(dgates[d, 1:].reshape((T - 1) * M, 4 * h), hbuf[d, :T - 1].reshape((T - 1) * M, h), False,
                                        dw_hh[d], None))
            linear.weight_grad_batch(wg)
            items = []
            for d in range(2):
                items.append((dw_ih[d], [dw_ih_s[d, s] for s in range(T)]))
                for k in range(2):                   # b_ih and b_hh: the same column sums, one tensor each
                    items.append((db[d, k].view(1, -1), [db_s[d, s].view(1, -1) for s in range(T)]))
            pack(items, dev)
            for d in range(2):
                _lib.check(lib.agnn_colsum_parts_f32(wpart[d].data_ptr(), T * nrb, h, datt.data_ptr() + 4 * d * h, st), "agnn_colsum_parts_f32")
            for d in range(2):
                grads[T + 4 * d:T + 4 * d + 4] = [dw_ih[d], dw_hh[d], db[d, 0], db[d, 1]]
            grads[T + 8] = datt
            for k in range(9):
                if not ctx.needs_input_grad[1 + T + k]:
                    grads[T + k] = None
        if ctx.needs_input_grad[1 + T + 9]:          # att.bias cancels in the softmax: exact zeros
            grads[T + 9] = torch.zeros((1,), **f32)
        return (None, *grads)


def jumping_knowledge(module, xs) -> torch.Tensor:
    """`module(xs)` for a core_layers.JumpingKnowledge on the HIP kernels (`kernel_applicable(module, xs)` must hold).  Works in
    eval() with gradients; under torch.no_grad(), or when nothing requires grad, nothing is saved and the output has the bits of
    the training forward.  att.bias receives an exactly zero gradient (it cancels in the softmax over the steps)."""
    P = _params(module)
    _lib.require_gpu(*xs, *P)
    if any(p.dtype != torch.float32 for p in P):
        raise _lib.AgnnError("jumping_knowledge: fp32 parameters expected")
    xs = [_lib.rows16(x) for x in xs]
    if torch.is_grad_enabled() and any(t.requires_grad for t in (*xs, *P)):
        return _JKFn.apply(len(xs), *xs, *P)
    return _forward(xs, P, False)[0]
