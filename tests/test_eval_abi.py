"""The evaluation entry point (csrc/eval.hip) rejects bad arguments before any HIP call: safe on a CPU-only host.
Pointers that pass the null checks are made-up addresses; a call that got as far as using one would not return a code.
Codes as include/agnn.h defines them: -22 (AGNN_EINVAL) for null pointers and bad sizes, -14 (AGNN_EALIGN) for a counter
buffer off 8 bytes; each with a message."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "analysisgnn_amd", "libagnn_hip.so")
P = 1 << 20          # a made-up, 16-byte aligned device address


@pytest.fixture(scope="module")
def lib():
    from analysisgnn_amd import _lib
    if not os.path.exists(SO):
        pytest.fail("libagnn_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _ev(lib, logits=P, ld=10, seg_off=P, seg_end=None, T=2, n_cols=10, labels=P, N=8, ignore=-1, row_mask=None, gate=-1, group=0, pred=P,
        counts=P):
    return lib.agnn_multitask_eval_f32(logits, ld, seg_off, seg_end, T, n_cols, labels, N, ignore, row_mask, gate, group, pred, counts, None)


def test_module_and_symbols_exist(lib):
    from analysisgnn_amd import metrics
    for name in ("multitask_argmax", "MultiTaskMetrics", "metrics_from_counts", "onset_rna_accuracy"):
        assert hasattr(metrics, name)
    assert lib.agnn_eval_counts_len(21, 634) == 4 * 21 + 4 + 3 * 634
    assert lib.agnn_eval_counts_len(1, 2) == 4 + 4 + 6


def test_eval_rejects_bad_arguments(lib):
    for kw in (dict(logits=None), dict(seg_off=None)):
        assert _ev(lib, **kw) == -22, kw
        assert b"multitask_eval" in lib.agnn_last_error()
    assert _ev(lib, pred=None, counts=None) == -22 and b"neither pred nor counts" in lib.agnn_last_error()
    assert _ev(lib, labels=None) == -22 and b"counts without labels" in lib.agnn_last_error()
    assert _ev(lib, T=0) == -22 and b"n_tasks=0" in lib.agnn_last_error()
    assert _ev(lib, T=33) == -22 and b"n_tasks=33" in lib.agnn_last_error()
    assert _ev(lib, T=-1) == -22
    assert _ev(lib, N=-1) == -22 and b"n_rows=-1" in lib.agnn_last_error()
    assert _ev(lib, n_cols=0) == -22
    assert _ev(lib, n_cols=11) == -22                      # wider than the row stride
    assert _ev(lib, gate=2) == -22 and b"gate_task=2" in lib.agnn_last_error()
    assert _ev(lib, gate=-2) == -22
    assert _ev(lib, group=0b100) == -22 and b"group_mask" in lib.agnn_last_error()
    assert _ev(lib, group=1 << 31) == -22
    assert _ev(lib, counts=P + 4) == -14 and b"8-byte" in lib.agnn_last_error()


def test_histogram_limit_is_named(lib):
    """The staged rows and the 4 T + 4 + 3 n_cols histogram bins share the LDS: beyond AGNN_EVAL_MAX_COLS columns the call is
    refused with a message that names the limit (include/agnn.h documents it)."""
    assert _ev(lib, n_cols=801, ld=801) == -22
    assert b"AGNN_EVAL_MAX_COLS=800" in lib.agnn_last_error()
    assert "#define AGNN_EVAL_MAX_COLS 800" in open(os.path.join(ROOT, "include", "agnn.h")).read()


def test_no_rows_is_a_no_op_that_looks_at_no_pointer(lib):
    assert _ev(lib, logits=None, seg_off=None, labels=None, pred=None, counts=None, N=0) == 0
    assert _ev(lib, logits=None, seg_off=None, labels=None, pred=None, counts=None, N=0, T=21, n_cols=634, ld=634, gate=15, group=0x1F) == 0
