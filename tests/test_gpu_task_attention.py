"""The cross-task attention kernels (csrc/taskattn.hip through task_attention) and the module that calls them
(heads.CrossTaskTransformer) on the GPU.  The reference is float64 torch on the CPU, written out here from the same fp32
inputs: matmul, softmax, mask, matmul; its autograd gives the gradients.  Tolerance: helpers.assert_close_rel at 1e-4 of the
reference tensor's own largest magnitude (plain fp32 arithmetic of this computation differs from float64 by at most 5.3e-7 at
the ordinary shapes and 4.0e-6 with the queries scaled by 30: more than a tenfold margin)."""
import functools
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import assert_close_rel  # noqa: E402

TOL = 1e-4
DEV = "cuda:0"


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------
def reference(qkv, dO, T, heads, keep=None):
    """float64 (o [n T, E], dqkv [n T, 3E]).  keep: [n, heads, T, T] factors on the normalised probabilities."""
    rows, E3 = qkv.shape
    n, E = rows // T, E3 // 3
    D = E // heads
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = (x[:, j * E:(j + 1) * E].reshape(n, T, heads, D).transpose(1, 2) for j in range(3))       # [n, heads, T, D]
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), dim=-1)
    if keep is not None:
        P = P * keep.double()
    o = (P @ v).transpose(1, 2).reshape(rows, E)
    o.backward(dO.double())
    return o.detach(), x.grad


def inputs(n, T, heads, D, seed, q_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    E = heads * D
    qkv = torch.randn(n * T, 3 * E, generator=g)
    qkv[:, :E] *= q_scale
    return qkv, torch.randn(n * T, E, generator=g)


@functools.lru_cache(maxsize=None)
def case(n, T, heads, D, q_scale=1.0):
    qkv, dO = inputs(n, T, heads, D, 3000 + 7 * n + 5 * T + 3 * heads + D, q_scale)
    return (qkv, dO), reference(qkv, dO, T, heads)


def run(qkv, dO, T, heads, p=0.0, call_id=0):
    """The two kernels on contiguous device copies -> (o, dqkv, rng_used); dqkv starts as NaN: every element is written."""
    from analysisgnn_amd import task_attention as ta
    qd, gd = qkv.to(DEV), dO.to(DEV)
    o, lse, used = ta.forward_raw(qd, T, heads, p, call_id)
    dqkv = torch.full_like(qd, float("nan"))
    ta.backward_raw(qd, T, heads, o, lse, gd, dqkv, p=p, call_id=call_id, rng_used=used)
    torch.cuda.synchronize()
    return o, dqkv, used


def check(got, ref, what, E):
    o, dqkv = got[:2]
    assert torch.isfinite(o).all() and torch.isfinite(dqkv).all(), f"{what}: not finite"
    assert_close_rel(o, ref[0], TOL, f"{what}: o")
    for j, name in enumerate(("dq", "dk", "dv")):
        assert_close_rel(dqkv[:, j * E:(j + 1) * E], ref[1][:, j * E:(j + 1) * E], TOL, f"{what}: {name}")


# ---- 1. raw forward and backward ---------------------------------------------------------------------------------------------------
# (n_seq, T, heads, D): one key; the 3-task subset (a workgroup that is not full); the default shape with a part-full last
# workgroup; largest T and D; other head counts and the smallest width; heads * T = 256, the edge of the rule
CASES = [(1, 1, 4, 16), (5, 3, 4, 16), (7, 21, 4, 16), (257, 21, 4, 16), (33, 32, 4, 32), (19, 6, 2, 8), (64, 21, 1, 32), (3, 32, 8, 16)]


@pytest.mark.parametrize("n,T,heads,D", CASES)
def test_forward_and_backward(n, T, heads, D):
    ins, ref = case(n, T, heads, D)
    got = run(*ins, T, heads)
    check(got, ref, f"n={n} T={T} heads={heads} D={D}", heads * D)
    if T == 1:                                   # a softmax over one key: o = v, and dq = dk = 0 exactly
        E = heads * D
        assert torch.equal(got[0].cpu(), ins[0][:, 2 * E:]) and float(got[1][:, :2 * E].abs().max()) == 0.0


def test_column_blocks_of_wider_buffers():
    """qkv read from, o and dqkv written into, and dO read from column blocks of wider buffers (ld larger than 3E / E); the
    neighbouring columns hold NaN before and after."""
    from analysisgnn_amd import task_attention as ta
    n, T, heads, D = 7, 21, 4, 16
    E = heads * D
    (qkv, dO), ref = case(n, T, heads, D)
    rows = n * T
    nan = lambda w: torch.full((rows, w), float("nan"), device=DEV)      # noqa: E731
    buf, obuf, gbuf, dbuf = nan(3 * E + 16), nan(E + 8), nan(3 * E + 16), nan(E + 12)
    buf[:, 4:4 + 3 * E] = qkv.to(DEV)
    dbuf[:, 8:8 + E] = dO.to(DEV)
    o, lse, _ = ta.forward_raw(buf[:, 4:4 + 3 * E], T, heads, out=obuf[:, 4:4 + E])
    ta.backward_raw(buf[:, 4:4 + 3 * E], T, heads, o, lse, dbuf[:, 8:8 + E], gbuf[:, 8:8 + 3 * E])
    torch.cuda.synchronize()
    assert o.data_ptr() == obuf[:, 4:].data_ptr()
    check((o, gbuf[:, 8:8 + 3 * E]), ref, "column blocks", E)
    assert torch.isnan(obuf[:, :4]).all() and torch.isnan(obuf[:, 4 + E:]).all()
    assert torch.isnan(gbuf[:, :8]).all() and torch.isnan(gbuf[:, 8 + 3 * E:]).all()
    assert torch.isnan(buf[:, :4]).all() and torch.isnan(buf[:, 4 + 3 * E:]).all()
    assert torch.isnan(dbuf[:, :8]).all() and torch.isnan(dbuf[:, 8 + E:]).all()


def test_large_scores():
    """q scaled by 30: scores near +-110, so exp() of a raw score overflows fp32; the maximum subtraction must hold."""
    n, T, heads, D = 9, 21, 4, 16
    ins, ref = case(n, T, heads, D, 30.0)
    E = heads * D
    S = (ins[0][:, :E].double().view(n, T, heads, D).transpose(1, 2) @ ins[0][:, E:2 * E].double().view(n, T, heads, D).transpose(1, 2).transpose(-1, -2)) / 4.0
    assert float(S.max()) > 89.0 and float(S.min()) < -89.0
    check(run(*ins, T, heads), ref, "q x 30", E)


# ---- 2. dropout --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", [(64, 21), (5, 3)])
def test_dropout(n, T):
    from analysisgnn_amd import fused, task_attention as ta
    heads, D, p, call_id = 4, 16, 0.3, 515151
    E = heads * D
    ins = inputs(n, T, heads, D, 900 + n)
    o, dqkv, used = run(*ins, T, heads, p=p, call_id=call_id)
    keep = ta.dropout_keep(n, T, heads, p, used, call_id, DEV)
    kc = keep.cpu()
    assert tuple(kc.shape) == (n, heads, T, T)
    # the factors are 0 or 1 / (1 - p); the kept share is binomial(count, 1 - p): within 5 standard deviations of 1 - p
    kept = kc != 0
    assert bool((~kept | (kc == 1.0 / (1.0 - torch.tensor(p, dtype=torch.float32)))).all())
    cnt = kc.numel()
    share = float(kept.double().mean())
    bound = 5 * math.sqrt(p * (1 - p) / cnt)
    print(f"n={n} T={T}: kept share {share:.5f} (1 - p = {1 - p}, 5 sigma = {bound:.5f}, {cnt} factors)")
    assert abs(share - (1 - p)) <= bound
    # forward and the three gradients against the float64 formula with the exported factors
    check((o, dqkv), reference(*ins, T, heads, keep=kc), f"dropout n={n} T={T}", E)
    # the same (seed, step, call id): the same bits, forward and backward
    o2, dqkv2, used2 = run(*ins, T, heads, p=p, call_id=call_id)
    assert torch.equal(used, used2) and torch.equal(o, o2) and torch.equal(dqkv, dqkv2)
    assert torch.equal(ta.dropout_keep(n, T, heads, p, used2, call_id, DEV), keep)
    # another call id, or the next training step, draws another mask
    assert not torch.equal(ta.dropout_keep(n, T, heads, p, used, call_id + 1, DEV), keep)
    dev = torch.device(DEV)
    assert torch.equal(used, fused.rng_state(dev))
    fused.advance_rng(dev)
    o3, _, used3 = run(*ins, T, heads, p=p, call_id=call_id)
    assert int(used3[1]) == int(used[1]) + 1 and int(used3[0]) == int(used[0])
    assert not torch.equal(ta.dropout_keep(n, T, heads, p, used3, call_id, DEV), keep) and not torch.equal(o3, o)


def test_no_dropout_leaves_the_generator_alone():
    from analysisgnn_amd import fused, task_attention as ta
    dev = torch.device(DEV)
    before = fused.rng_state(dev).clone()
    (qkv, dO), _ = case(7, 21, 4, 16)
    o, lse, used = ta.forward_raw(qkv.to(DEV), 21, 4, p=0.0)
    torch.cuda.synchronize()
    assert used is None and torch.equal(fused.rng_state(dev), before)
    assert bool((ta.dropout_keep(2, 21, 4, 0.0, None, 1, DEV) == 1).all())


# ---- 3. reproducibility and memory -------------------------------------------------------------------------------------------------
def test_bitwise_reproducible():
    ins, _ = case(257, 21, 4, 16)
    a, b = run(*ins, 21, 4), run(*ins, 21, 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_nothing_of_score_size_is_allocated():
    """(4096, 21, 4, 16) under no_grad: the peak across attention() rises by at most the bytes of o plus 1 MiB (the scores
    alone would be 28.9 MB)."""
    from analysisgnn_amd import task_attention as ta
    n, T, heads, D = 4096, 21, 4, 16
    qkv = torch.randn(n * T, 3 * heads * D, device=DEV)
    with torch.no_grad():
        ta.attention(qkv[:T * 8], T, heads)          # the library is loaded, the kernel's code object too
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        o = ta.attention(qkv, T, heads)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(DEV)
    o_bytes = o.numel() * 4
    print(f"peak rise {peak - base} bytes, o {o_bytes} bytes, scores would be {n * heads * T * T * 4} bytes")
    assert tuple(o.shape) == (n * T, heads * D) and peak - base <= o_bytes + (1 << 20)


# ---- 4. the module -----------------------------------------------------------------------------------------------------------------
CLASSES = [4, 50, 50, 15, 185, 2, 7, 12, 35, 3, 9, 21, 5, 16, 40, 11, 6, 30, 8, 2, 13]
TASKS21 = {f"task{i:02d}": c for i, c in enumerate(CLASSES)}


def model(out_channels, seed=5, dropout=0.0):
    from analysisgnn_amd.models import TorchAnalysisGNN
    from analysisgnn_amd.synth import make_batch
    torch.manual_seed(seed)
    return TorchAnalysisGNN(make_batch(1, 30).metadata(), 25, 32, out_channels, TASKS21, 2, dropout=dropout, use_jk=False, logit_fusion=True)


def head_parameters(m):
    return [(k, p) for k, p in m.named_parameters() if k.split(".")[0] in ("clf_dict", "clf_proj_layers", "cross_task_transformer", "fusion_layers")]


def clf_step(m, x, subset=None, seed=11):
    """(logits [N, sum C], dx, {name: gradient or None}) of forward_clf + a fixed cotangent; nothing is left behind."""
    x = x.detach().requires_grad_(True)
    names, params = zip(*head_parameters(m))
    logits, offs, _ = m.forward_clf_fused(x, subset)
    gout = torch.randn(logits.shape, generator=torch.Generator().manual_seed(seed)).to(logits.device)
    grads = torch.autograd.grad(logits, (x, *params), gout, allow_unused=True)
    return logits.detach(), grads[0], dict(zip(names, grads[1:]))


def no_library_attention(monkeypatch):
    def refuse(*a, **k):
        raise RuntimeError("library attention called")
    monkeypatch.setattr(F, "scaled_dot_product_attention", refuse)


@pytest.mark.parametrize("subset", [None, ["task01", "task00", "task04"], ["task04"]], ids=["all", "three", "one"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_module_runs_on_the_kernel(subset, train, monkeypatch):
    """out_channels = 128 (E = 64, head width 16): forward_clf and its backward never reach the library attention."""
    no_library_attention(monkeypatch)
    m = model(128, dropout=0.3 if train else 0.0).to(DEV).train(train)
    x = torch.randn(200, 128, generator=torch.Generator().manual_seed(2)).to(DEV)
    logits, dx, grads = clf_step(m, x, subset)
    torch.cuda.synchronize()
    use = list(TASKS21) if subset is None else subset
    assert tuple(logits.shape) == (200, sum(TASKS21[t] for t in use))
    assert torch.isfinite(logits).all() and torch.isfinite(dx).all() and float(dx.abs().max()) > 0
    for k, g in grads.items():
        if k.startswith("cross_task_transformer."):
            assert g is not None and torch.isfinite(g).all(), k
    if len(use) > 1:                              # (one token: the softmax is 1 and q, k get no gradient)
        assert float(grads["cross_task_transformer.multihead_attn.in_proj_weight"][:128].abs().max()) > 0


def test_unserved_width_stays_on_the_library_body(monkeypatch):
    """out_channels = 16: E = 8, head width 2, which the kernel does not serve: the library body is still the path."""
    no_library_attention(monkeypatch)
    m = model(16).to(DEV).eval()
    with pytest.raises(RuntimeError, match="library attention called"):
        clf_step(m, torch.randn(50, 16).to(DEV))


class RefCrossTaskTransformer(torch.nn.Module):
    """The reference's module (models/analysis.py:408-418): nn.MultiheadAttention + residual + LayerNorm."""

    def __init__(self, proj_dim, num_heads=4, dropout=0.1):
        super().__init__()
        self.multihead_attn = torch.nn.MultiheadAttention(proj_dim, num_heads, dropout=dropout, batch_first=True)
        self.norm = torch.nn.LayerNorm(proj_dim)

    def forward(self, x):
        attended, _ = self.multihead_attn(x, x, x)
        return self.norm(x + attended)


@pytest.mark.parametrize("E,T", [(8, 21), (64, 21), (64, 3)], ids=["width2-library", "width16-kernel", "width16-three-tasks"])
def test_module_matches_float64_multihead_attention(E, T):
    from analysisgnn_amd.heads import CrossTaskTransformer
    torch.manual_seed(40 + E + T)
    m = CrossTaskTransformer(E, 4, 0.1).eval()
    ref = RefCrossTaskTransformer(E, 4, 0.1)
    ref.load_state_dict(m.state_dict(), strict=True)
    ref = ref.double().eval()
    x = torch.randn(50, T, E)
    gout = torch.randn(50, T, E)
    xr = x.double().requires_grad_(True)
    rnames, rparams = zip(*ref.named_parameters())
    rgrads = torch.autograd.grad(ref(xr), (xr, *rparams), gout.double())
    m = m.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    names, params = zip(*m.named_parameters())
    out = m(xg)
    grads = torch.autograd.grad(out, (xg, *params), gout.to(DEV))
    torch.cuda.synchronize()
    assert names == rnames
    assert_close_rel(out, ref(xr).detach(), TOL, "out")
    for k, a, b in zip(("x",) + names, grads, rgrads):
        assert_close_rel(a, b, TOL, f"g.{k}")


def test_the_two_sides_agree(monkeypatch):
    """FUSED = True against FUSED = False (the library body) in eval mode on the same parameters, N = 300: logits and every
    parameter gradient within 1e-4."""
    from analysisgnn_amd import task_attention as ta
    m = model(128, seed=9).to(DEV).eval()
    x = torch.randn(300, 128, generator=torch.Generator().manual_seed(3)).to(DEV)
    monkeypatch.setattr(ta, "FUSED", False)
    ref = clf_step(m, x)
    monkeypatch.setattr(ta, "FUSED", True)
    no_library_attention(monkeypatch)
    got = clf_step(m, x)
    torch.cuda.synchronize()
    assert_close_rel(got[0], ref[0], TOL, "logits")
    assert_close_rel(got[1], ref[1], TOL, "dx")
    assert set(got[2]) == set(ref[2]) and len(ref[2]) > 100
    for k in ref[2]:
        assert ref[2][k] is not None and got[2][k] is not None, k
        assert_close_rel(got[2][k], ref[2][k], TOL, f"g.{k}")


# ---- 5. graph capture --------------------------------------------------------------------------------------------------------------
def train_step(m, x, labels, monkeypatch):
    """forward_clf + the training objective + backward -> [logits, loss, dx, parameter gradients]; the call sites draw under the
    same ids in every pass."""
    from analysisgnn_amd import fused, heads
    monkeypatch.setattr(fused, "_CALL_IDS", itertools.count(7000))
    x = x.detach().requires_grad_(True)
    params = [p for _, p in head_parameters(m)]
    logits, offs, _ = m.forward_clf_fused(x)
    loss, _ = heads.training_loss(logits, offs, labels, x)
    grads = torch.autograd.grad(loss, (x, *params))
    return [logits.detach(), loss.detach(), *grads]


def capture_setup(p):
    m = model(128, seed=13, dropout=p).to(DEV).train()
    g = torch.Generator().manual_seed(17)
    x = torch.randn(300, 128, generator=g).to(DEV)
    labels = torch.stack([torch.randint(0, c, (300,), generator=g) for c in CLASSES]).to(DEV)
    return m, x, labels


def test_step_under_capture_without_dropout(monkeypatch):
    """One eager step, then the same step captured: two replays equal the eager result bitwise."""
    no_library_attention(monkeypatch)
    m, x, labels = capture_setup(0.0)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        eager = [t.clone() for t in train_step(m, x, labels, monkeypatch)]
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in eager)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        captured = train_step(m, x, labels, monkeypatch)
    for i in range(2):
        for t in captured:
            t.fill_(float("nan"))
        cg.replay()
        torch.cuda.synchronize()
        for j, (a, b) in enumerate(zip(eager, captured)):
            assert torch.equal(a, b), f"replay {i}, tensor {j}"


def test_step_under_capture_with_dropout(monkeypatch):
    """Dropout 0.3 on the attention probabilities: two replays separated by fused.advance_rng are finite and differ."""
    from analysisgnn_amd import fused
    no_library_attention(monkeypatch)
    m, x, labels = capture_setup(0.3)
    dev = torch.device(DEV)
    fused.rng_state(dev)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        train_step(m, x, labels, monkeypatch)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        captured = train_step(m, x, labels, monkeypatch)
    replays = []
    for i in range(2):
        cg.replay()
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in captured), f"replay {i}"
        replays.append([t.clone() for t in captured])
        fused.advance_rng(dev)
    assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[0][2], replays[1][2])


# ---- 6. an empty batch -------------------------------------------------------------------------------------------------------------
def test_empty_batch(monkeypatch):
    from analysisgnn_amd import task_attention as ta
    from analysisgnn_amd.heads import CrossTaskTransformer
    no_library_attention(monkeypatch)
    m = CrossTaskTransformer(64, 4, 0.3).to(DEV).train()
    x = torch.zeros(0, 21, 64, device=DEV, requires_grad=True)
    out = m(x)
    assert tuple(out.shape) == (0, 21, 64)
    out.sum().backward()
    assert x.grad is not None and tuple(x.grad.shape) == (0, 21, 64)
    qkv = torch.zeros(0, 192, device=DEV, requires_grad=True)
    o = ta.attention(qkv, 21, 4, p=0.3)
    assert tuple(o.shape) == (0, 64)
    o.sum().backward()
    torch.cuda.synchronize()
    assert tuple(qkv.grad.shape) == (0, 192)
