"""The dense-attention entry points (csrc/attn.hip) reject bad arguments with a message BEFORE any HIP call (safe on a CPU-only
host: the pointers below are never dereferenced), and the workspace query answers in 256-byte multiples.  Codes as
include/agnn.h defines them for every entry point: AGNN_EINVAL (-22) for bad sizes and null pointers, AGNN_EALIGN (-14) for a
misaligned pointer or leading dimension (a leading dimension that is not a multiple of 4 floats is -14 here, as in the rest of
the ABI, not -22)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # a 16-byte aligned non-null address (never read: every call below fails its checks first)


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _fwd(lib, N=64, heads=4, D=16, ld=None, ld_o=None, q=P, o=P, p=0.0, rng=None, q_rows=0):
    E = heads * D
    return lib.agnn_attn_fwd_f32(q, P, P, 3 * E if ld is None else ld, N, heads, D, 0.25, p, rng, 1, q_rows, o, E if ld_o is None else ld_o,
                                 P, None, None)


def _bwd(lib, N=64, heads=4, D=16, ld=None, ld_d=None, ld_do=None, dq=P, ws=P, ws_bytes=1 << 20, p=0.0, rng=None):
    E = heads * D
    return lib.agnn_attn_bwd_f32(P, P, P, 3 * E if ld is None else ld, N, heads, D, 0.25, p, rng, 1, 0, P, E if ld_do is None else ld_do,
                                 P, E, P, dq, P, P, 3 * E if ld_d is None else ld_d, ws, ws_bytes, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_head_width_and_head_count(call):
    lib = _lib()
    assert call(lib, D=12) == -22 and b"D=12" in lib.agnn_last_error()
    assert call(lib, D=128) == -22
    assert call(lib, heads=0) == -22 and b"heads=0" in lib.agnn_last_error()
    assert call(lib, N=0) == -22 and b"N=0" in lib.agnn_last_error()


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_leading_dimensions(call):
    lib = _lib()
    assert call(lib, ld=60) == -22 and b"ld_qkv=60" in lib.agnn_last_error()          # smaller than heads * D = 64
    assert call(lib, ld=66) == -14 and b"16-byte" in lib.agnn_last_error()            # rows off 16 bytes
    assert call(lib, p=0.2) == -22 and b"rng" in lib.agnn_last_error()                # dropout without its state
    assert call(lib, p=1.0) == -22


def test_forward_output_arguments():
    lib = _lib()
    assert _fwd(lib, ld_o=60) == -22 and b"o" in lib.agnn_last_error()
    assert _fwd(lib, ld_o=66) == -14
    assert _fwd(lib, o=P + 4) == -14
    assert _fwd(lib, q=P + 8) == -14
    assert _fwd(lib, o=None) == -22
    assert _fwd(lib, q_rows=32) == -22 and b"q_rows=32" in lib.agnn_last_error()


def test_backward_output_arguments():
    lib = _lib()
    assert _bwd(lib, ld_d=60) == -22 and b"dq" in lib.agnn_last_error()
    assert _bwd(lib, ld_d=70) == -14
    assert _bwd(lib, ld_do=60) == -22 and b"dO" in lib.agnn_last_error()
    assert _bwd(lib, dq=P + 4) == -14
    assert _bwd(lib, ws=None) == -22
    assert _bwd(lib, ws_bytes=16) == -12 and b"workspace" in lib.agnn_last_error()


def test_mask_export_arguments():
    lib = _lib()
    keep = lib.agnn_attn_dropout_keep_f32
    assert keep(0, 4, 0.2, P, 1, P, None) == -22 and b"N=0" in lib.agnn_last_error()
    assert keep(1 << 20, 4, 0.2, P, 1, P, None) == -22
    assert keep(16, 0, 0.2, P, 1, P, None) == -22 and b"heads=0" in lib.agnn_last_error()
    assert keep(16, 4, 1.5, P, 1, P, None) == -22
    assert keep(16, 4, 0.2, None, 1, P, None) == -22 and b"rng" in lib.agnn_last_error()
    assert keep(16, 4, 0.2, P, 1, None, None) == -22


def test_workspace_sizes():
    lib = _lib()
    for N, heads in [(1, 1), (63, 4), (300, 4), (4096, 4), (16000, 4)]:
        b = lib.agnn_attn_bwd_workspace_bytes(N, heads)
        assert b > 0 and b % 256 == 0 and b >= 4 * N * heads
    assert lib.agnn_attn_bwd_workspace_bytes(0, 0) > 0


def test_python_dispatch_rule():
    """kernel_applicable looks at shapes, dtype and device only; there is no minimum-rows rule."""
    import torch
    from analysisgnn_amd import attention
    meta = lambda n, e, dt=torch.float32: torch.empty(n, e, dtype=dt, device="meta")      # noqa: E731
    assert not attention.kernel_applicable(meta(300, 256), 4)                             # not a HIP device
    assert not attention.kernel_applicable(torch.empty(300, 256), 4)
    assert attention.FUSED is True and attention.HEAD_WIDTHS == (8, 16, 32, 64)
    with pytest.raises(attention._lib.AgnnError):
        attention.self_attention(torch.nn.MultiheadAttention(32, 4), torch.zeros(5, 32), False)
