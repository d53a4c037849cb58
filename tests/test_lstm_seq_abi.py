"""The entry points of the persistent LSTM (csrc/lstmseq.hip) are declared in include/agnn.h, bound from there, and reject bad
arguments with AGNN_EINVAL (-22) and a message BEFORE any HIP call (safe on a CPU-only host: the pointers below are never
dereferenced); `lstm_seq.kernel_applicable` accepts exactly the modules the kernels are built for."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # a 16-byte aligned non-null address, never read
EINVAL, EALIGN = -22, -14
NEW = ["agnn_lstm_seq_fwd_f32", "agnn_lstm_seq_bwd_f32"]


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _fwd(lib, **kw):
    a = dict(gi=P, w_hh=P, b_hh=P, B=3, T=17, hidden=128, y=P, saved=P, drop_scale=None, y_drop=None)
    a.update(kw)
    return lib.agnn_lstm_seq_fwd_f32(a["gi"], a["w_hh"], a["b_hh"], a["B"], a["T"], a["hidden"], a["y"], a["saved"], a["drop_scale"],
                                     a["y_drop"], None)


def _bwd(lib, **kw):
    a = dict(dy=P, y=P, saved=P, w_hh=P, B=3, T=17, hidden=128, dg=P, drop_scale=None, hprev=P)
    a.update(kw)
    return lib.agnn_lstm_seq_bwd_f32(a["dy"], a["y"], a["saved"], a["w_hh"], a["B"], a["T"], a["hidden"], a["dg"], a["drop_scale"],
                                     a["hprev"], None)


def test_declared_and_bound():
    from analysisgnn_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    # beside the GRU pair, with its conventions: the stream last, (B, T, hidden) in the middle
    assert len(_lib.SIGNATURES["agnn_lstm_seq_fwd_f32"][1]) == len(_lib.SIGNATURES["agnn_gru_fwd_f32"][1])
    assert len(_lib.SIGNATURES["agnn_lstm_seq_bwd_f32"][1]) == len(_lib.SIGNATURES["agnn_gru_bwd_f32"][1]) - 1      # ONE dg, not dgi + dgh


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_sizes_are_refused_with_a_message(call):
    lib = _lib()
    for h in (48, 32, 256, 0, -128):
        assert call(lib, hidden=h) == EINVAL and f"hidden={h}".encode() in lib.agnn_last_error(), h
    assert call(lib, B=0) == EINVAL and b"B=0" in lib.agnn_last_error()
    assert call(lib, T=0) == EINVAL and b"T=0" in lib.agnn_last_error()
    assert call(lib, B=-1) == EINVAL and b"B=-1" in lib.agnn_last_error()
    assert call(lib, T=2 ** 31) == EINVAL and b"T=2147483648" in lib.agnn_last_error()
    assert call(lib, B=2 ** 30) == EINVAL and b"B=1073741824" in lib.agnn_last_error()       # the grid is 2 * B
    assert call(lib, hidden=64, B=0) == EINVAL


def test_required_pointers():
    lib = _lib()
    for name in ("gi", "w_hh", "b_hh", "y", "saved"):
        assert _fwd(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error(), name
    for name in ("gi", "w_hh", "y", "saved"):
        assert _fwd(lib, **{name: P + 4}) == EALIGN and b"aligned" in lib.agnn_last_error(), name
    for name in ("dy", "saved", "w_hh", "dg"):
        assert _bwd(lib, **{name: None}) == EINVAL and b"null" in lib.agnn_last_error(), name
        assert _bwd(lib, **{name: P + 8}) == EALIGN and b"aligned" in lib.agnn_last_error(), name
    assert _bwd(lib, y=None) == EINVAL and b"hprev needs y" in lib.agnn_last_error()         # y is read for hprev only
    # the two dropout operands go together
    assert _fwd(lib, drop_scale=P) == EINVAL and b"go together" in lib.agnn_last_error()
    assert _fwd(lib, y_drop=P) == EINVAL and b"go together" in lib.agnn_last_error()


def test_kernel_applicable():
    from analysisgnn_amd.lstm_seq import KERNEL_HIDDEN, kernel_applicable
    assert KERNEL_HIDDEN == (64, 128)
    ok = dict(batch_first=True, bidirectional=True)
    assert kernel_applicable(torch.nn.LSTM(8, 128, **ok))
    assert kernel_applicable(torch.nn.LSTM(99, 64, num_layers=2, dropout=0.3, **ok))
    assert not kernel_applicable(torch.nn.GRU(8, 128, **ok))
    assert not kernel_applicable(torch.nn.LSTM(8, 128, batch_first=True, bidirectional=False))
    assert not kernel_applicable(torch.nn.LSTM(8, 128, batch_first=False, bidirectional=True))
    assert not kernel_applicable(torch.nn.LSTM(8, 128, bias=False, **ok))
    assert not kernel_applicable(torch.nn.LSTM(8, 128, proj_size=16, **ok))
    assert not kernel_applicable(torch.nn.LSTM(8, 32, **ok))
    assert not kernel_applicable(torch.nn.LSTM(8, 256, **ok))
