"""The cross-task attention entry points (csrc/taskattn.hip) reject bad arguments with a message that names the offending
argument BEFORE any HIP call (safe on a CPU-only host: the pointers below are never dereferenced).  Codes as include/agnn.h
defines them for every entry point: AGNN_EINVAL (-22) for sizes out of range, shapes not served, leading dimensions that are
too small, NULL pointers and dropout without its state; AGNN_EALIGN (-14) for a pointer off 16 bytes or a leading dimension
that is not a multiple of 4 floats.  n_seq = 0 is success and looks at no pointer."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 4096          # a 16-byte aligned non-null address (never read: every call below fails its checks first, or n_seq is 0)
EINVAL, EALIGN = -22, -14


def _lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _fwd(lib, n_seq=64, T=21, heads=4, D=16, ld=None, ld_o=None, qkv=P, o=P, p=0.0, rng=None, used=None):
    E = heads * D
    return lib.agnn_taskattn_fwd_f32(qkv, 3 * E if ld is None else ld, n_seq, T, heads, D, 0.25, p, rng, 1, o, E if ld_o is None else ld_o,
                                     P, used, None)


def _bwd(lib, n_seq=64, T=21, heads=4, D=16, ld=None, ld_d=None, ld_do=None, ld_o=None, qkv=P, dO=P, o=P, lse=P, dqkv=P, p=0.0, rng=None):
    E = heads * D
    return lib.agnn_taskattn_bwd_f32(qkv, 3 * E if ld is None else ld, n_seq, T, heads, D, 0.25, p, rng, 1, dO, E if ld_do is None else ld_do,
                                     o, E if ld_o is None else ld_o, lse, dqkv, 3 * E if ld_d is None else ld_d, None)


def _keep(lib, n_seq=8, T=21, heads=4, p=0.3, rng=P, keep=P):
    return lib.agnn_taskattn_dropout_keep_f32(n_seq, T, heads, p, rng, 1, keep, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_shapes_not_served(call):
    lib = _lib()
    for D in (4, 12, 64):
        assert call(lib, D=D, heads=1) == EINVAL and f"D={D}".encode() in lib.agnn_last_error()
    assert call(lib, T=0) == EINVAL and b"T=0" in lib.agnn_last_error()
    assert call(lib, T=33) == EINVAL and b"T=33" in lib.agnn_last_error()
    assert call(lib, heads=0) == EINVAL and b"heads=0" in lib.agnn_last_error()
    assert call(lib, heads=5, D=32) == EINVAL and b"heads=5" in lib.agnn_last_error()            # heads * D = 160 > 128
    assert call(lib, heads=16, D=8, T=17) == EINVAL and b"heads=16" in lib.agnn_last_error()     # heads * T = 272 > 256
    assert call(lib, n_seq=-1) == EINVAL and b"n_seq=-1" in lib.agnn_last_error()
    assert call(lib, n_seq=1 << 40) == EINVAL and b"n_seq=" in lib.agnn_last_error()


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_dropout_arguments(call):
    lib = _lib()
    assert call(lib, p=1.0) == EINVAL and b"p=" in lib.agnn_last_error()
    assert call(lib, p=-0.1) == EINVAL and b"p=" in lib.agnn_last_error()
    assert call(lib, p=float("nan")) == EINVAL
    assert call(lib, p=0.3, rng=None) == EINVAL and b"rng" in lib.agnn_last_error()              # dropout without its state


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_packed_projection_argument(call):
    lib = _lib()
    assert call(lib, ld=188) == EINVAL and b"ld_qkv=188" in lib.agnn_last_error()                # smaller than 3E = 192
    assert call(lib, ld=194) == EALIGN and b"ld_qkv=194" in lib.agnn_last_error()                # rows off 16 bytes
    assert call(lib, qkv=P + 4) == EALIGN and b"qkv" in lib.agnn_last_error()
    assert call(lib, qkv=None) == EINVAL and b"qkv" in lib.agnn_last_error()


def test_forward_output_arguments():
    lib = _lib()
    assert _fwd(lib, ld_o=60) == EINVAL and b"ld_o=60" in lib.agnn_last_error()                  # smaller than E = 64
    assert _fwd(lib, ld_o=66) == EALIGN and b"ld_o=66" in lib.agnn_last_error()
    assert _fwd(lib, o=P + 8) == EALIGN and b" o " in lib.agnn_last_error()
    assert _fwd(lib, o=None) == EINVAL and b"o is null" in lib.agnn_last_error()
    assert _fwd(lib, p=0.3, rng=P, used=None) == EINVAL and b"rng_used" in lib.agnn_last_error()


def test_backward_arguments():
    lib = _lib()
    assert _bwd(lib, ld_do=60) == EINVAL and b"ld_do=60" in lib.agnn_last_error()
    assert _bwd(lib, ld_do=70) == EALIGN and b"ld_do=70" in lib.agnn_last_error()
    assert _bwd(lib, dO=None) == EINVAL and b"dO" in lib.agnn_last_error()
    assert _bwd(lib, dO=P + 4) == EALIGN and b"dO" in lib.agnn_last_error()
    assert _bwd(lib, ld_o=32) == EINVAL and b"ld_o=32" in lib.agnn_last_error()
    assert _bwd(lib, o=None) == EINVAL and b"o is null" in lib.agnn_last_error()
    assert _bwd(lib, ld_d=100) == EINVAL and b"ld_dqkv=100" in lib.agnn_last_error()             # smaller than 3E = 192
    assert _bwd(lib, ld_d=198) == EALIGN and b"ld_dqkv=198" in lib.agnn_last_error()
    assert _bwd(lib, dqkv=None) == EINVAL and b"dqkv" in lib.agnn_last_error()
    assert _bwd(lib, dqkv=P + 12) == EALIGN and b"dqkv" in lib.agnn_last_error()
    assert _bwd(lib, lse=None) == EINVAL and b"lse" in lib.agnn_last_error()


def test_mask_export_arguments():
    lib = _lib()
    assert _keep(lib, T=0) == EINVAL and b"T=0" in lib.agnn_last_error()
    assert _keep(lib, T=33) == EINVAL and b"T=33" in lib.agnn_last_error()
    assert _keep(lib, heads=0) == EINVAL and b"heads=0" in lib.agnn_last_error()
    assert _keep(lib, heads=16, T=21) == EINVAL and b"heads=16" in lib.agnn_last_error()
    assert _keep(lib, n_seq=-2) == EINVAL and b"n_seq=-2" in lib.agnn_last_error()
    assert _keep(lib, p=1.5) == EINVAL and b"p=" in lib.agnn_last_error()
    assert _keep(lib, rng=None) == EINVAL and b"rng" in lib.agnn_last_error()
    assert _keep(lib, keep=None) == EINVAL and b"keep" in lib.agnn_last_error()


def test_empty_batch_succeeds_and_looks_at_no_pointer():
    """A batch whose valid mask is empty: success, even with NULL or misaligned pointers and dropout without a state."""
    lib = _lib()
    assert _fwd(lib, n_seq=0) == 0
    assert _fwd(lib, n_seq=0, qkv=None, o=None, p=0.3, rng=None) == 0
    assert _fwd(lib, n_seq=0, qkv=P + 4, ld=190) == 0
    assert _bwd(lib, n_seq=0) == 0
    assert _bwd(lib, n_seq=0, qkv=None, dO=None, o=None, lse=None, dqkv=None, p=0.3, rng=None) == 0
    assert _keep(lib, n_seq=0, keep=None, rng=None) == 0
    assert _fwd(lib, n_seq=0, D=4, heads=1) == EINVAL            # the shape rule still holds


def test_python_dispatch_rule():
    """kernel_applicable looks at shapes, dtype and device only (nothing is allocated; the device is a description)."""
    import torch
    from analysisgnn_amd import task_attention as ta
    hip = torch.device("cuda", 0)
    f32 = torch.empty(0, dtype=torch.float32, device="meta").dtype
    assert ta.kernel_applicable(16000, 21, 4, 64, f32, hip) is True
    assert ta.kernel_applicable(16000, 21, 4, 64, f32, "cuda") is True
    assert ta.kernel_applicable(0, 21, 4, 64, f32, hip) is True                   # an empty batch is served
    assert not ta.kernel_applicable(16000, 21, 4, 16, f32, hip)                   # D = 4
    assert not ta.kernel_applicable(16000, 33, 4, 64, f32, hip)                   # T = 33
    assert not ta.kernel_applicable(16000, 21, 4, 64, f32, torch.device("cpu"))
    assert not ta.kernel_applicable(16000, 21, 4, 64, f32, torch.empty(1, device="meta").device)
    assert not ta.kernel_applicable(16000, 21, 4, 64, torch.float64, hip)
    assert not ta.kernel_applicable(16000, 21, 4, 64, torch.bfloat16, hip)
    assert not ta.kernel_applicable(16000, 21, 4, 66, f32, hip)                   # E not a multiple of heads
    assert not ta.kernel_applicable(16000, 21, 8, 256, f32, hip)                  # E = 256 > 128
    assert not ta.kernel_applicable(16000, 32, 16, 128, f32, hip)                 # heads * T = 512 > 256
    assert ta.kernel_applicable(3, 32, 8, 128, f32, hip) and ta.kernel_applicable(19, 6, 2, 16, f32, hip)
    assert ta.FUSED is True and ta.HEAD_WIDTHS == (8, 16, 32)
    with pytest.raises(ta._lib.AgnnError):
        ta.attention(torch.zeros(42, 192), 21, 4)                                 # a CPU tensor: no fall-back
