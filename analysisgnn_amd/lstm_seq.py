"""Host side of the persistent LSTM kernels (include/agnn.h: agnn_lstm_seq_fwd_f32 / agnn_lstm_seq_bwd_f32).

Takes the parameters of a plain `torch.nn.LSTM(batch_first=True, bidirectional=True)` — the module the reference's
`PKSpell(cell_type="LSTM")` (models/pitch_spelling.py:50-151) and `PostProcessingMLTModel` (models/chord.py:751-783) build — so
`state_dict`s stay identical; the input projection, dx and all weight gradients are GEMMs, the T-step recurrence (forward and
backward) is one kernel launch per layer.  gru.py without its branch scheduling: these LSTMs are not part of the benchmarked
step, so nothing is forked onto another stream or deferred onto the step's flush."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .gru import _ones, _stack_gru_params
from .linear import WgItem, weight_grad, weight_grad_batch

KERNEL_HIDDEN = (64, 128)      # hidden sizes per direction the kernels are instantiated for


class _LSTMLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, drop_scale=None):
        """x [B, T, I]; w_ih [2, 4H, I]; w_hh [2, 4H, H]; b_ih, b_hh [2, 4H].  `drop_scale` [B, T, 2*H] (0 or 1 / (1 - p) per
        element): the layer's OUTPUT is y * drop_scale — nn.LSTM's inter-layer dropout — written by the recurrence kernel itself;
        the backward kernel applies the same factor to the incoming gradient."""
        dev = _lib.require_gpu(x, w_ih, w_hh, b_ih, b_hh)
        B, T, I = x.shape
        Hh = w_hh.shape[2]
        x2 = x.reshape(B * T, I)
        gi = torch.addmm(b_ih.reshape(-1), x2, w_ih.reshape(8 * Hh, I).t())         # [B*T, 2*4H]: 1-D bias, added in the GEMM epilogue
        w_hh_c = w_hh.contiguous()
        b_hh_c = b_hh.contiguous()
        y = torch.empty((B, T, 2 * Hh), dtype=torch.float32, device=dev)
        saved = torch.empty((B, T, 2, 5, Hh), dtype=torch.float32, device=dev)
        out = y
        if drop_scale is not None:
            if tuple(drop_scale.shape) != (B, T, 2 * Hh) or drop_scale.dtype != torch.float32 or not drop_scale.is_contiguous():
                raise _lib.AgnnError("lstm_seq: drop_scale must be a contiguous fp32 [B, T, 2*hidden] tensor")
            out = torch.empty_like(y)
        if B * T > 0:                            # (the entry points refuse empty work)
            lib = _lib.load()
            _lib.check(lib.agnn_lstm_seq_fwd_f32(gi.data_ptr(), w_hh_c.data_ptr(), b_hh_c.data_ptr(), B, T, Hh, y.data_ptr(), saved.data_ptr(),
                                                 _lib.ptr(drop_scale), out.data_ptr() if drop_scale is not None else None,
                                                 _lib.stream_ptr(dev)), "agnn_lstm_seq_fwd_f32")
        ctx.save_for_backward(x2, w_ih, w_hh_c, y, saved, *([drop_scale] if drop_scale is not None else []))
        ctx.dims = (B, T, I, Hh)
        return out

    @staticmethod
    def backward(ctx, dy):
        x2, w_ih, w_hh, y, saved, *drop = ctx.saved_tensors
        drop_scale = drop[0] if drop else None
        B, T, I, Hh = ctx.dims
        dev = dy.device
        dy = dy.contiguous()
        dg = torch.empty((B, T, 2, 4 * Hh), dtype=torch.float32, device=dev)     # gradient of the pre-activations: input AND hidden side
        hp = torch.empty((B, T, 2, Hh), dtype=torch.float32, device=dev)         # h_{t-1} per direction: left by the walk itself
        if B * T > 0:
            lib = _lib.load()
            _lib.check(lib.agnn_lstm_seq_bwd_f32(dy.data_ptr(), y.data_ptr(), saved.data_ptr(), w_hh.data_ptr(), B, T, Hh, dg.data_ptr(),
                                                 _lib.ptr(drop_scale), hp.data_ptr(), _lib.stream_ptr(dev)), "agnn_lstm_seq_bwd_f32")
        dg2 = dg.view(B * T, 8 * Hh)
        dx = (dg2 @ w_ih.reshape(8 * Hh, I)).view(B, T, I) if ctx.needs_input_grad[0] else None
        dw_ih = torch.empty((8 * Hh, I), dtype=torch.float32, device=dev)
        db = torch.empty((8 * Hh,), dtype=torch.float32, device=dev)             # db_ih; db_hh is a copy of it (below)
        dw_hh = torch.empty((2, 4 * Hh, Hh), dtype=torch.float32, device=dev)    # both directions land in the stacked gradient
        items = []
        if I % 2 == 0:
            items.append(WgItem(dg2, x2, True, dw_ih, db))
        else:                                   # odd input width: the kernel pads a column, results are copied into place
            dw, dbv = weight_grad(dg2, x2, True)
            dw_ih.copy_(dw)
            db.copy_(dbv)
        hp2 = hp.view(B * T, 2 * Hh)
        for d in range(2):
            items.append(WgItem(dg2[:, d * 4 * Hh:(d + 1) * 4 * Hh], hp2[:, d * Hh:(d + 1) * Hh], False, dw_hh[d], None))
        weight_grad_batch(items)                # the layer's three products and the bias sum in one launch pair
        db = db.view(2, 4 * Hh)
        # db_hh: the same values in a buffer of its own.  One tensor for both would leave `bias_ih.grad` and `bias_hh.grad` on one
        # storage (AccumulateGrad takes the views over), and anything in place on `.grad` — clipping, accumulation — would act twice
        return dx, dw_ih.view(2, 4 * Hh, I), dw_hh, db, db.clone(), None


def kernel_applicable(rnn: nn.Module) -> bool:
    return (isinstance(rnn, nn.LSTM) and rnn.hidden_size in KERNEL_HIDDEN and rnn.bidirectional and rnn.batch_first
            and rnn.bias and getattr(rnn, "proj_size", 0) == 0)


def lstm_forward(rnn: nn.LSTM, x: torch.Tensor, training: bool) -> torch.Tensor:
    """y = rnn(x)[0] with zero initial state.  Persistent HIP kernels when `kernel_applicable(rnn)` (bidirectional, batch-first,
    biased, no projection, hidden_size 64 or 128); everything else runs the library RNN (MIOpen) — still on the GPU (hidden
    256: W_hh does not fit one CU's registers + LDS)."""
    _lib.require_gpu(x)
    if not kernel_applicable(rnn):
        return rnn(x)[0]
    y = x
    stacked = _stack_gru_params(rnn)             # the parameter names of nn.GRU and nn.LSTM are the same
    for layer in range(rnn.num_layers):
        w_ih, w_hh, b_ih, b_hh = stacked[4 * layer:4 * layer + 4]
        drop = None
        if layer < rnn.num_layers - 1 and rnn.dropout > 0 and training:
            B, T = y.shape[0], y.shape[1]
            drop = F.dropout(_ones((B, T, 2 * rnn.hidden_size), y.device), rnn.dropout, True)     # 0 or 1 / (1 - p): one launch
        y = _LSTMLayer.apply(y.contiguous(), w_ih, w_hh, b_ih, b_hh, drop)
    return y
