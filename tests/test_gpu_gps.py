"""The graph-transformer modules (core_layers.GPSLayer / HGPSLayer / HGPS) on the GPU: the reference-run float64 fixtures
(scripts/gen_golden_gps.py), the two attention paths against each other at the production head width, training mode with the
attention dropout against a float64 restatement that applies the exported masks, graph capture, and the memory condition.
Tolerance: helpers.assert_close_rel at 1e-4 of the reference tensor's largest magnitude."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import assert_close_rel, load_golden  # noqa: E402
from test_gps_modules import ETYPES2, ETYPES4, FIXTURES, build, fixture_state  # noqa: E402

TOL = 1e-4
DEV = "cuda:0"


def graph(N, E, R, width, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, width, generator=g), torch.randint(0, N, (2, E), generator=g), torch.randint(0, R, (E,), generator=g))


def forward_backward(m, x, ei, et, gout):
    """(out, dx, {name: gradient}) of one step; no autograd graph or .grad is left behind."""
    x = x.detach().requires_grad_(True)
    names, params = zip(*m.named_parameters())
    out = m(x, ei) if et is None else m(x, ei, et)
    grads = torch.autograd.grad(out, (x, *params), gout)
    return out.detach(), grads[0], dict(zip(names, grads[1:]))


# ---- 1. the reference's own modules, float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixture(name, monkeypatch):
    from analysisgnn_amd import attention, jk
    monkeypatch.setattr(jk, "MIN_ROWS", 0)        # the stack's JumpingKnowledge on its kernels (the library LSTM refuses a backward in eval())
    calls = []
    real = attention.attention
    monkeypatch.setattr(attention, "attention", lambda qkv, heads, p=0.0: (calls.append(tuple(qkv.shape)), real(qkv, heads, p))[1])
    z = load_golden(name)
    m = build(name)
    m.load_state_dict(fixture_state(z), strict=True)
    m = m.to(DEV).eval()
    t = lambda k: torch.from_numpy(np.asarray(z[k])).to(DEV)      # noqa: E731
    out, dx, grads = forward_backward(m, t("x"), t("edge_index"), t("edge_type") if "edge_type" in z.files else None, t("gout"))
    torch.cuda.synchronize()
    assert len(calls) == (3 if name.startswith("gps_stack") else 1) and calls[0][0] == z["x"].shape[0]      # the kernels ran
    assert_close_rel(out, z["out"], TOL, f"{name}: out")
    assert_close_rel(dx, z["dx"], TOL, f"{name}: dx")
    assert len(grads) == sum(k.startswith("g.") for k in z.files)
    for k, g in grads.items():
        if k == "jk.att.bias":        # cancels in the softmax over the layers: exactly zero, recorded (and computed) as a rounding residue
            assert float(g.abs().max()) <= TOL * float(np.abs(z["g.jk.att.weight"]).max())
            continue
        assert_close_rel(g, z["g." + k], TOL, f"{name}: g.{k}")


# ---- 2. the two attention paths at D = 64 ------------------------------------------------------------------------------------------
def test_cross_check_of_the_two_attention_paths(monkeypatch):
    """A cross-check of two implementations, not parity: HGPSLayer(64, 256, 4) (D = 64, the production width, for which no
    fixture is affordable) with the kernels against the same layer on F.scaled_dot_product_attention.  The D = 64 parity itself
    is tests/test_gpu_attention.py."""
    from analysisgnn_amd import attention, core_layers as cl
    torch.manual_seed(5)
    m = cl.HGPSLayer(64, 256, 4, etypes=ETYPES2).to(DEV).eval()
    x, ei, et = graph(300, 1200, 2, 64, 6)
    gout = torch.randn(300, 256, generator=torch.Generator().manual_seed(7)).to(DEV)
    args = (x.to(DEV), ei.to(DEV), et.to(DEV), gout)
    monkeypatch.setattr(attention, "FUSED", False)
    ref = forward_backward(m, *args)
    monkeypatch.setattr(attention, "FUSED", True)
    got = forward_backward(m, *args)
    torch.cuda.synchronize()
    assert_close_rel(got[0], ref[0], TOL, "out")
    assert_close_rel(got[1], ref[1], TOL, "dx")
    for k in ref[2]:
        assert_close_rel(got[2][k], ref[2][k], TOL, f"g.{k}")


# ---- 3. training mode: only the attention dropout acts -----------------------------------------------------------------------------
def layer_f64(P, rels, heads, x, ei, et, keep):
    """HGPSLayer.forward (core/hgnn.py:261-287) in the dtype of its arguments, the attention written out with `keep` on the
    normalised probabilities; the local branch is oracle/intree_ref.py's restatement."""
    from oracle import intree_ref as R
    H = P["embedding.weight"].shape[0]
    D = H // heads
    N = x.shape[0]
    ln = lambda h, name: F.layer_norm(torch.relu(h), (H,), P[name + ".weight"], P[name + ".bias"])      # noqa: E731
    h0 = R._lin(P, "embedding", x)
    local = ln(R.hetero_layer(P, "local.", rels, R.res_gated_conv, h0, ei, et), "normalize_local") + h0
    q, k, v = ((h0 @ P["attn.in_proj_weight"].t() + P["attn.in_proj_bias"])[:, j * H:(j + 1) * H].view(N, heads, D).transpose(0, 1) for j in range(3))
    prob = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(D), dim=-1) * keep
    att = R._lin(P, "attn.out_proj", (prob @ v).transpose(0, 1).reshape(N, H))
    out = local + ln(att, "normalize_attn") + h0
    h = R._lin(P, "ff2", torch.relu(R._lin(P, "ff1", out)))
    return F.normalize(out + h)


def test_training_mode_with_exported_masks(monkeypatch):
    from analysisgnn_amd import attention, core_layers as cl, fused
    call_id, real = 777001, attention.attention           # the layer's attention call draws under an id this test knows
    monkeypatch.setattr(attention, "attention", lambda qkv, heads, p=0.0: real(qkv, heads, p, call_id=call_id))
    torch.manual_seed(21)
    m = cl.HGPSLayer(24, 32, 4, etypes=ETYPES4)
    for d in (m.dropout_ff, m.dropout_attn, m.dropout_local):
        d.p = 0.0
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    N = 130
    x, ei, et = graph(N, 520, 4, 24, 22)
    gout = torch.randn(N, 32, generator=torch.Generator().manual_seed(23))
    used = fused.rng_state(torch.device(DEV)).clone()
    out, dx, grads = forward_backward(m, x.to(DEV), ei.to(DEV), et.to(DEV), gout.to(DEV))
    keep = attention.dropout_keep(N, 4, m.attn.dropout, used, call_id, DEV).cpu()
    assert 0.1 < float((keep == 0).double().mean()) < 0.3          # the attention dropout did act (p = 0.2)
    P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xd = x.double().requires_grad_(True)
    ref = layer_f64(P, list(ETYPES4), 4, xd, ei, et, keep.double())
    ref.backward(gout.double())
    assert_close_rel(out, ref.detach(), TOL, "out")
    assert_close_rel(dx, xd.grad, TOL, "dx")
    for k, g in grads.items():
        assert_close_rel(g, P[k].grad, TOL, f"g.{k}")


# ---- 4. graph capture ------------------------------------------------------------------------------------------------------------
def test_forward_backward_under_capture(monkeypatch):
    """After one eager step, forward + backward of an HGPSLayer in train() mode (all three dropouts and the attention dropout
    active) captured on one stream: each replay gives the bits of the eager run at the same rng step (every mask follows the
    device-side counter), and the two replays differ.  The eager steps run on the stream that is captured afterwards and leave
    no autograd graph behind (tests/test_gpu_jk.py)."""
    from analysisgnn_amd import core_layers as cl, fused
    torch.manual_seed(31)
    m = cl.HGPSLayer(24, 32, 4, etypes=ETYPES4).to(DEV).train()
    N = 130
    x, ei, et = graph(N, 520, 4, 24, 32)
    x, ei, et = x.to(DEV), ei.to(DEV), et.to(DEV)
    gout = torch.randn(N, 32, generator=torch.Generator().manual_seed(33)).to(DEV)
    dev = torch.device(DEV)
    state = fused.rng_state(dev)
    s0 = int(state[1])

    def step():
        monkeypatch.setattr(fused, "_CALL_IDS", itertools.count(9000))      # the same call sites draw under the same ids in every pass
        out, dx, grads = forward_backward(m, x, ei, et, gout)
        return [out, dx, *grads.values()]

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        eager = []
        for s in (s0, s0 + 1):
            state[1:2].fill_(s)
            eager.append([t.clone() for t in step()])
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert not torch.equal(eager[0][0], eager[1][0])
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        captured = step()
    state[1:2].fill_(s0)
    replays = []
    for i in range(2):
        for t in captured:
            t.fill_(float("nan"))
        cg.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager[i], captured):
            assert torch.equal(a, b), f"replay {i}"
        replays.append(captured[0].clone())
        fused.advance_rng(dev)
    assert not torch.equal(replays[0], replays[1])


def test_stack_masks_follow_the_device_counter(monkeypatch):
    """HGPS in train() mode: every dropout of the stack (the layers' and the stack's own) draws from the library's generator, so
    the same (rng step, call ids) give the same bits and the next step gives other masks."""
    from analysisgnn_amd import fused
    torch.manual_seed(51)
    m = build("gps_stack").to(DEV).train()
    x, ei, et = (t.to(DEV) for t in graph(130, 520, 2, 24, 52))
    dev = torch.device(DEV)

    def run():
        monkeypatch.setattr(fused, "_CALL_IDS", itertools.count(5000))
        with torch.no_grad():
            return m(x, ei, et)

    a, b = run(), run()
    fused.advance_rng(dev)
    c = run()
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b) and not torch.equal(a, c)
    assert float((a == 0).double().mean()) > 0.3                  # the stack's own dropout (p = 0.5) acted


# ---- 5. memory: O(N E), not heads N^2 --------------------------------------------------------------------------------------------
def test_attention_memory_condition():
    """N = 4096, H = 256, 4 heads, forward + backward of the attention call (in-projection, kernels, out-projection): the peak
    above the starting level stays below a quarter of the heads x N x N fp32 score matrix (67 MB of 268 MB)."""
    from analysisgnn_amd import attention
    N, H, heads = 4096, 256, 4
    torch.manual_seed(41)
    mha = torch.nn.MultiheadAttention(H, heads, dropout=0.2, batch_first=True).to(DEV)
    x = torch.randn(N, H, device=DEV, requires_grad=True)
    gout = torch.randn(N, H, device=DEV)
    assert attention.FUSED and attention.kernel_applicable(x, heads)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    out = attention.self_attention(mha, x, True)
    grads = torch.autograd.grad(out, (x, *mha.parameters()), gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - base
    print(f"peak above the starting level: {peak / 2 ** 20:.1f} MiB")
    assert all(torch.isfinite(g).all() for g in grads)
    assert peak < heads * N * N * 4 // 4
