"""_lib.rows_ok / rows16 / vec16: the one rule for what a kernel may read where it lies ("Operand layout").
CPU tensors only: the rule looks at dtype, shape, strides and the address, never at the device."""
import glob
import os

import pytest
import torch

from analysisgnn_amd import _lib
from analysisgnn_amd._abi import AgnnError


def _flat(n=256):
    return torch.arange(n, dtype=torch.float32)        # (torch's CPU allocations are 64-byte aligned: asserted below)


# name -> (factory, rows_ok at vec=4, rows_ok at vec=2)
CASES = {
    "dense": (lambda: _flat()[:96].view(8, 12), True, True),
    "row slice": (lambda: _flat()[:96].view(8, 12)[1:7], True, True),
    "column block, keeps its ld": (lambda: _flat()[:192].view(8, 24)[:, 4:16], True, True),
    "column block from column 2": (lambda: _flat()[:192].view(8, 24)[:, 2:14], False, True),
    "transpose": (lambda: _flat()[:96].view(12, 8).t(), False, False),
    "one row expanded to 8, strides (0, 1)": (lambda: _flat()[:12].view(1, 12).expand(8, 12), False, False),
    "one row with stride 0": (lambda: _flat()[:12].as_strided((1, 12), (0, 1)), True, True),
    "ld smaller than the row": (lambda: _flat().as_strided((8, 12), (4, 1)), False, False),
    "contiguous at element offset 1": (lambda: _flat()[1:97].view(8, 12), False, False),
    "contiguous at element offset 2": (lambda: _flat()[2:98].view(8, 12), False, True),
    "width 6 contiguous": (lambda: _flat()[:48].view(8, 6), False, True),
    "zero rows": (lambda: torch.empty((0, 12), dtype=torch.float32), True, True),
}


def _shares_storage(a, b):
    return a.numel() > 0 and b.numel() > 0 and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def test_base_allocations_are_aligned():
    assert _flat().data_ptr() % 16 == 0


@pytest.mark.parametrize("name", list(CASES))
def test_rows_ok_table(name):
    make, ok4, ok2 = CASES[name]
    t = make()
    assert _lib.rows_ok(t) is ok4
    assert _lib.rows_ok(t, vec=4) is ok4
    assert _lib.rows_ok(t, vec=2) is ok2


@pytest.mark.parametrize("name", list(CASES))
def test_rows16_returns_the_input_or_a_real_copy(name):
    make, ok4, _ = CASES[name]
    t = make()
    before = t.clone()
    r = _lib.rows16(t)
    assert r.shape == t.shape and r.dtype == torch.float32
    assert torch.equal(r, before)
    assert _lib.rows_ok(r)
    if ok4:
        assert r is t
    else:
        assert r is not t and not _shares_storage(r, t)
        assert r.stride() == ((t.shape[1] + 3) // 4 * 4, 1)       # dense, or rows padded to whole vectors
    assert torch.equal(t, before)                 # the input is never written


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("vec", [1, 2])
def test_rows16_at_a_narrower_vector(name, vec):
    """An operand its kernel reads with shorter vectors (`vec=2`: float2; `vec=1`: float by float) stays in place more often."""
    make, _, ok2 = CASES[name]
    t = make()
    ok = ok2 if vec == 2 else name not in ("transpose", "one row expanded to 8, strides (0, 1)", "ld smaller than the row")
    assert _lib.rows_ok(t, vec=vec) is ok
    r = _lib.rows16(t, vec=vec)
    assert torch.equal(r, t) and _lib.rows_ok(r, vec=vec)
    assert (r is t) if ok else (r is not t and not _shares_storage(r, t) and _lib.rows_ok(r))


@pytest.mark.parametrize("bad", [lambda: torch.zeros((8, 12), dtype=torch.float64), lambda: torch.zeros((8, 12), dtype=torch.float16),
                                 lambda: torch.zeros(12), lambda: torch.zeros((2, 4, 4))])
def test_rows16_raises_on_dtype_and_rank(bad):
    t = bad()
    assert not _lib.rows_ok(t) and not _lib.rows_ok(t, vec=2)
    with pytest.raises(AgnnError):
        _lib.rows16(t)


VEC_CASES = {
    "dense": (lambda: _flat()[:12], True),
    "at element offset 1": (lambda: _flat()[1:13], False),
    "at element offset 2": (lambda: _flat()[2:14], False),
    "at element offset 4": (lambda: _flat()[4:16], True),
    "strided": (lambda: _flat()[:24:2], False),
    "stacked weights, dense": (lambda: _flat()[:96].view(2, 6, 8), True),
    "stacked weights at element offset 1": (lambda: _flat()[1:97].view(2, 6, 8), False),
    "stacked weights, transposed blocks": (lambda: _flat()[:96].view(2, 6, 8).transpose(1, 2), False),
    "empty": (lambda: torch.empty((0,), dtype=torch.float32), True),
}


@pytest.mark.parametrize("name", list(VEC_CASES))
def test_vec16_returns_the_input_or_a_real_copy(name):
    make, ok = VEC_CASES[name]
    t = make()
    before = t.clone()
    assert _lib.vec_ok(t) is ok
    r = _lib.vec16(t)
    assert r.shape == t.shape and torch.equal(r, before)
    assert _lib.vec_ok(r)
    if ok:
        assert r is t
    else:
        assert r is not t and not _shares_storage(r, t)
    assert torch.equal(t, before)


def test_vec_ok_at_vec2():
    assert _lib.vec_ok(_flat()[2:14], vec=2) and not _lib.vec_ok(_flat()[1:13], vec=2)


def test_vec16_raises_on_dtype():
    with pytest.raises(AgnnError):
        _lib.vec16(torch.zeros(12, dtype=torch.float64))


def test_contiguous_is_not_a_copy():
    """The trap rows16 exists for: a contiguous view at an odd offset of a flat buffer is returned unchanged by `.contiguous()`."""
    t = _flat()[1:97].view(8, 12)
    c = t.contiguous()
    assert c.data_ptr() == t.data_ptr() and c.data_ptr() % 16 == 4
    assert _lib.rows16(t).data_ptr() % 16 == 0


def test_a_broadcast_gradient_is_not_readable_in_place():
    """The other trap: autograd hands a custom backward a (0, 1)-strided gradient behind `out.sum(0)`, and 0 % 4 == 0."""
    seen = []

    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2.0

        @staticmethod
        def backward(ctx, g):
            seen.append(g)
            return g * 2.0

    x = _flat()[:96].view(8, 12).clone().requires_grad_(True)
    F.apply(x).sum(0).pow(2).sum().backward()
    g = seen[0]
    assert tuple(g.shape) == (8, 12) and g.stride() == (0, 1)
    assert not _lib.rows_ok(g) and _lib.rows16(g).stride() == (12, 1)


def test_no_private_alignment_spelling_outside_lib():
    pkg = os.path.dirname(os.path.abspath(_lib.__file__))
    for path in sorted(glob.glob(os.path.join(pkg, "*.py"))):
        if os.path.basename(path) == "_lib.py":
            continue
        with open(path) as f:
            src = f.read()
        for needle in ("data_ptr() % 16", "data_ptr() % 8"):
            assert needle not in src, f"{os.path.basename(path)} spells its own alignment test ({needle}): use _lib.rows_ok / vec_ok"
