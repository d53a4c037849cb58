"""The dense-attention kernels alone (csrc/attn.hip through attention.forward_raw / backward_raw) against
softmax(Q K^T / sqrt(D)) V and its gradients, computed here in float64 on the CPU from the same fp32 inputs.
Tolerance: helpers.assert_close_rel at 1e-4 of the reference tensor's largest magnitude."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import assert_close_rel  # noqa: E402

TOL = 1e-4
DEV = "cuda:0"


def reference(q, k, v, dO, heads, keep=None):
    """float64: (o [N, E], lse [heads, N], dq, dk, dv).  keep: [heads, N, N] factors on the normalised probabilities."""
    N, E = q.shape
    D = E // heads
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    split = lambda t: t.view(N, heads, D).transpose(0, 1)      # noqa: E731
    S = split(qd) @ split(kd).transpose(1, 2) / math.sqrt(D)
    P = torch.softmax(S, dim=-1)
    if keep is not None:
        P = P * keep.double()
    o = (P @ split(vd)).transpose(0, 1).reshape(N, E)
    o.backward(dO.double())
    return o.detach(), torch.logsumexp(S.detach(), dim=-1), qd.grad, kd.grad, vd.grad


def inputs(N, D, heads, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(N, heads * D, generator=g) for _ in range(4))      # q, k, v, dO


def run(q, k, v, dO, heads, p=0.0, call_id=0, q_rows=0):
    """The kernels on contiguous device copies -> (o, lse, dq, dk, dv, rng_used) (device tensors)."""
    from analysisgnn_amd import attention
    qd, kd, vd, gd = (t.to(DEV) for t in (q, k, v, dO))
    o, lse, used = attention.forward_raw(qd, kd, vd, heads, p, call_id, q_rows=q_rows)
    dq, dk, dv = (torch.full_like(qd, float("nan")) for _ in range(3))
    attention.backward_raw(qd, kd, vd, heads, o, lse, gd, dq, dk, dv, p=p, call_id=call_id, rng_used=used, q_rows=q_rows)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv, used


def check(got, ref, what):
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), got, ref):
        assert torch.isfinite(a).all(), f"{what}: {name} not finite"
        assert_close_rel(a, b, TOL, f"{what}: {name}")


# N: one row, around one and two 32-key tiles and the 64-row block, several tiles; every head width; 1 and 4 heads;
# q_rows = 128: the four-wave workgroup (the automatic rule takes it only at N heads >= 32 768)
CASES = [(1, 8, 1, 0), (31, 16, 4, 0), (32, 32, 1, 0), (33, 64, 4, 0), (63, 8, 4, 0), (64, 16, 1, 0), (65, 32, 4, 0), (130, 64, 4, 0),
         (300, 64, 4, 0), (300, 8, 1, 0), (130, 16, 4, 0), (65, 64, 1, 0), (300, 64, 4, 128), (130, 16, 1, 128)]


@functools.lru_cache(maxsize=None)
def case(N, D, heads):
    ins = inputs(N, D, heads, 1000 + N + D + heads)
    return ins, reference(*ins, heads)


@pytest.mark.parametrize("N,D,heads,q_rows", CASES)
def test_forward_and_backward(N, D, heads, q_rows):
    ins, ref = case(N, D, heads)
    check(run(*ins, heads, q_rows=q_rows)[:5], ref, f"N={N} D={D} heads={heads} q_rows={q_rows}")


def test_column_blocks_of_wider_buffers():
    """q / k / v as column blocks of one wider buffer (ld_qkv = 3E + 16), o into a column block, dq / dk / dv into a buffer
    that is NaN outside its blocks: nothing outside the blocks changes."""
    from analysisgnn_amd import attention
    N, D, heads = 130, 16, 4
    E = heads * D
    ins, ref = case(N, D, heads)
    buf = torch.full((N, 3 * E + 16), float("nan"), device=DEV)
    for j, t in enumerate(ins[:3]):
        buf[:, 4 + j * E:4 + (j + 1) * E] = t.to(DEV)
    q, k, v = (buf[:, 4 + j * E:4 + (j + 1) * E] for j in range(3))
    obuf = torch.full((N, E + 8), float("nan"), device=DEV)
    o, lse, _ = attention.forward_raw(q, k, v, heads, out=obuf[:, 4:4 + E])
    gbuf = torch.full((N, 3 * E + 16), float("nan"), device=DEV)
    dq, dk, dv = (gbuf[:, 8 + j * E:8 + (j + 1) * E] for j in range(3))
    attention.backward_raw(q, k, v, heads, o, lse, ins[3].to(DEV), dq, dk, dv)
    torch.cuda.synchronize()
    check((o, lse, dq, dk, dv), ref, "column blocks")
    assert o.data_ptr() == obuf[:, 4:].data_ptr()
    assert torch.isnan(obuf[:, :4]).all() and torch.isnan(obuf[:, 4 + E:]).all()
    assert torch.isnan(gbuf[:, :8]).all() and torch.isnan(gbuf[:, 8 + 3 * E:]).all()
    assert torch.isnan(buf[:, :4]).all() and torch.isnan(buf[:, 4 + 3 * E:]).all()


def test_online_rescale_by_a_late_dominant_key():
    """One key row of the LAST 32-key tile is scaled by 125: for the queries it agrees with in sign (a good fifth of the
    (head, query) pairs, asserted) its score is more than 80 above every score of the earlier tiles, so exp() of those
    underflows after the rescale; the other queries keep ordinary rows.  lse, o and the gradients must still match."""
    N, D, heads = 130, 16, 4
    q, k, v, dO = inputs(N, D, heads, 77)
    k[129] *= 125.0
    S = (q.double().view(N, heads, D).transpose(0, 1) @ k.double().view(N, heads, D).transpose(0, 1).transpose(1, 2)) / math.sqrt(D)
    margin = S[:, :, 129] - S[:, :, :128].max(dim=-1).values
    assert float((margin > 80.0).double().mean()) > 0.2 and float((margin < 0.0).double().mean()) > 0.2
    check(run(q, k, v, dO, heads)[:5], reference(q, k, v, dO, heads), "late dominant key")


@pytest.mark.parametrize("N", [65, 130])
def test_dropout(N):
    from analysisgnn_amd import attention, fused
    D, heads, p, call_id = 16, 4, 0.2, 4242
    ins = inputs(N, D, heads, 500 + N)
    o, lse, dq, dk, dv, used = run(*ins, heads, p=p, call_id=call_id)
    keep = attention.dropout_keep(N, heads, p, used, call_id, DEV)
    # the factors are 0 or 1 / (1 - p); the share of zeros is binomial(n, p): within 4 standard deviations of p
    kc = keep.cpu()
    zeros = kc == 0
    assert bool((zeros | (kc == 1.0 / (1.0 - torch.tensor(p, dtype=torch.float32)))).all())
    n = kc.numel()
    share = float(zeros.double().mean())
    print(f"N={N}: zero share {share:.5f} (p = {p}, 4 sigma = {4 * math.sqrt(p * (1 - p) / n):.5f})")
    assert abs(share - p) <= 4 * math.sqrt(p * (1 - p) / n)
    # forward and the three gradients against the float64 formula with the exported factors (lse is of the undropped scores)
    check((o, lse, dq, dk, dv), reference(*ins, heads, keep=kc), f"dropout N={N}")
    # the same (seed, step, call id): the same bits, forward and backward
    o2, _, dq2, dk2, dv2, used2 = run(*ins, heads, p=p, call_id=call_id)
    assert torch.equal(used, used2) and torch.equal(o, o2)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)
    # another call id, or the next training step, draws another mask
    assert not torch.equal(attention.dropout_keep(N, heads, p, used, call_id + 1, DEV), keep)
    fused.advance_rng(torch.device(DEV))
    o3, _, _, _, _, used3 = run(*ins, heads, p=p, call_id=call_id)
    assert int(used3[1]) == int(used[1]) + 1 and int(used3[0]) == int(used[0])
    assert not torch.equal(attention.dropout_keep(N, heads, p, used3, call_id, DEV), keep) and not torch.equal(o3, o)


def test_backward_is_bitwise_reproducible():
    ins, _ = case(300, 64, 4)
    a = run(*ins, 4)
    b = run(*ins, 4)
    for name, x, y in zip(("o", "lse", "dq", "dk", "dv"), a, b):
        assert torch.equal(x, y), name


def test_unsupported_width_is_an_error():
    from analysisgnn_amd import _lib, attention
    with pytest.raises(_lib.AgnnError):
        attention.attention(torch.zeros(8, 3 * 48, device=DEV), 4)           # D = 12
