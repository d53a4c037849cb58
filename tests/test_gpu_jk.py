"""JumpingKnowledge on the HIP kernels (analysisgnn_amd/jk.py, csrc/lstm.hip) against float64: the step kernel alone, the
reference-run fixtures (scripts/gen_golden_jk.py), the float64 restatement (oracle/intree_ref.py), determinism and modes, the
encoders that use the block, and graph capture.  Tolerance: 1e-4 relative to max(1, |ref|max) (helpers.assert_close, the
north-star bound of tests/test_gpu_core_layers.py).  jk.MIN_ROWS is patched to 0 so that small row counts reach the kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import assert_close, load_golden  # noqa: E402

TOL = 1e-4
DEV = "cuda:0"


@pytest.fixture()
def fused(monkeypatch):
    """The kernels at every row count, and a count of the calls that reached them."""
    from analysisgnn_amd import jk
    monkeypatch.setattr(jk, "MIN_ROWS", 0)
    monkeypatch.setattr(jk, "FUSED", True)
    calls = []
    real = jk.jumping_knowledge
    monkeypatch.setattr(jk, "jumping_knowledge", lambda m, xs: (calls.append(tuple(xs[0].shape)), real(m, xs))[1])
    return calls


# ---- 1. the step kernel ------------------------------------------------------------------------------------------------------
def _step_case(M, K0, h, later, seed, wide=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    c = dict(w_ih=r(4 * h, K0) * 0.2, w_hh=r(4 * h, h) * 0.2, b_ih=r(4 * h) * 0.2, b_hh=r(4 * h) * 0.2, att_w=r(h))
    xw = r(M, K0 + 12)
    c["x"] = xw[:, 8:8 + K0] if wide else xw[:, :K0].contiguous()          # wide: a column slice, ld = K0 + 12 > K0
    if later:
        c["hprev"], c["cprev"] = torch.tanh(r(M, h)), r(M, h)
    return c


def _step_ref(c):
    d = {k: v.double() for k, v in c.items()}
    g = d["x"] @ d["w_ih"].t() + d["b_ih"] + d["b_hh"]
    if "hprev" in d:
        g = g + d["hprev"] @ d["w_hh"].t()
    i, f, gg, o = g.chunk(4, dim=-1)
    i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
    cc = i * gg + (f * d["cprev"] if "cprev" in d else 0)
    hh = o * torch.tanh(cc)
    return dict(hout=hh, cout=cc, act=torch.cat([i, f, gg, o], dim=-1), score=hh @ d["att_w"])


def _launch(cases):
    """One agnn_lstm_step_f32 launch over `cases` (device tensors) -> per case (hout, cout, act, part)."""
    from analysisgnn_amd import _lib
    lib = _lib.load()
    items = (_lib.LstmStep * len(cases))()
    outs = []
    for it, c in zip(items, cases):
        M, K0 = c["x"].shape
        h = c["w_hh"].shape[1]
        o = dict(hout=torch.full((M, h + 4), 7.0, device=DEV), cout=torch.full((M, h), 7.0, device=DEV),
                 act=torch.full((M, 4 * h), 7.0, device=DEV), part=torch.full((M, h // 32), 7.0, device=DEV))
        it.x, it.ld_x = c["x"].data_ptr(), c["x"].stride(0)
        if "hprev" in c:
            it.hprev, it.ld_hprev, it.cprev, it.ld_cprev = c["hprev"].data_ptr(), h, c["cprev"].data_ptr(), h
        it.w_ih, it.w_hh, it.b_ih, it.b_hh = (c[k].data_ptr() for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
        it.hout, it.ld_hout, it.cout, it.ld_cout = o["hout"].data_ptr(), h + 4, o["cout"].data_ptr(), h          # hout with its own ld
        it.act, it.att_w, it.part = o["act"].data_ptr(), c["att_w"].data_ptr(), o["part"].data_ptr()
        it.M, it.K0, it.h = M, K0, h
        outs.append(o)
    _lib.check(lib.agnn_lstm_step_f32(len(cases), items, _lib.stream_ptr(torch.device(DEV))), "agnn_lstm_step_f32")
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("later", [False, True], ids=["first", "later"])
@pytest.mark.parametrize("M,K0,h", [(130, 64, 64), (1, 64, 64), (130, 64, 96), (257, 256, 384)])
def test_step_kernel(M, K0, h, later):
    """hout, cout, act and the summed attention partials against float64; both directions in one launch give the bits of two
    single-item launches.  The second direction's x is a column slice of a wider matrix (ld > K0)."""
    host = [_step_case(M, K0, h, later, 11), _step_case(M, K0, h, later, 12, wide=True)]
    assert host[1]["x"].stride(0) > K0
    dev = []
    for c in host:
        d = {k: v.to(DEV) for k, v in c.items() if k != "x"}
        base = c["x"]._base if c["x"]._base is not None else c["x"]
        d["x"] = base.to(DEV).as_strided(c["x"].shape, c["x"].stride(), c["x"].storage_offset())
        assert d["x"].stride() == c["x"].stride()
        dev.append(d)
    both = _launch(dev)
    for c, d, got in zip(host, dev, both):
        ref = _step_ref(c)
        assert_close(got["hout"][:, :h], ref["hout"], TOL, "hout")
        assert float(got["hout"][:, h:].min()) == 7.0 and float(got["hout"][:, h:].max()) == 7.0, "wrote past its row"
        assert_close(got["cout"], ref["cout"], TOL, "cout")
        assert_close(got["act"], ref["act"], TOL, "act")
        assert_close(got["part"].double().sum(dim=1), ref["score"], TOL, "sum_j part")
        single = _launch([d])[0]
        for k in ("hout", "cout", "act", "part"):
            assert torch.equal(single[k], got[k]), f"{k}: one launch for both directions differs from a launch of its own"


def test_step_kernel_refuses_bad_sizes():
    from analysisgnn_amd import _lib
    lib = _lib.load()
    items = (_lib.LstmStep * 1)()
    items[0].M, items[0].K0, items[0].h = 10, 64, 48
    assert lib.agnn_lstm_step_f32(1, items, None) == -22 and b"h=48" in lib.agnn_last_error()
    items[0].K0, items[0].h = 24, 64
    assert lib.agnn_lstm_step_f32(1, items, None) == -22
    assert lib.agnn_lstm_step_f32(3, items, None) == -22


# ---- 2. fixtures recorded from the reference's own class ---------------------------------------------------------------------
def _module_from(z, H, L):
    from analysisgnn_amd.core_layers import JumpingKnowledge
    m = JumpingKnowledge(H, L)
    m.load_state_dict({k[2:]: torch.from_numpy(np.asarray(z[k])).float() for k in z.files if k.startswith("p.")}, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("name,H,L", [("jk_fused_l2", 32, 2), ("jk_fused_l4", 32, 4)])
def test_reference_fixture(name, H, L, fused):
    z = load_golden(name)
    m = _module_from(z, H, L)
    for k in z.files:                      # the recorded operands are fp32-representable: the kernels see what float64 saw
        if k.startswith(("p.", "x")):
            assert np.array_equal(z[k].astype(np.float32).astype(np.float64), z[k]), k
    xs = [torch.from_numpy(z[f"x{t}"]).float().to(DEV).requires_grad_(True) for t in range(L)]
    out = m(xs)
    assert fused == [tuple(xs[0].shape)]
    assert_close(out, z["out"], TOL, "out")
    out.backward(torch.from_numpy(z["gout"]).float().to(DEV))
    for t in range(L):
        assert_close(xs[t].grad, z[f"dx{t}"], TOL, f"dx{t}")
    n = 0
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        assert_close(p.grad, z[f"g.{k}"], TOL, f"g.{k}")
        n += 1
    assert n == 10
    assert float(m.att.bias.grad.abs().max()) == 0.0 and abs(float(z["g.att.bias"][0])) < 1e-12


# ---- 3. the module against the float64 restatement ---------------------------------------------------------------------------
_REF = {}


def _case(N, H, L):
    """(module on the CPU, inputs, gout, float64 reference (out, input grads, parameter grads)) — computed once per shape."""
    key = (N, H, L)
    if key not in _REF:
        from analysisgnn_amd.core_layers import JumpingKnowledge
        from oracle import intree_ref as R
        torch.manual_seed(100 + N + H + L)
        m = JumpingKnowledge(H, L)
        with torch.no_grad():
            m.att.bias.fill_(0.25)
        g = torch.Generator().manual_seed(N)
        xs = [torch.randn(N, H, generator=g) for _ in range(L)]
        gout = torch.randn(N, H, generator=g)
        P = {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
        x64 = [x.double().requires_grad_(True) for x in xs]
        ref = R.jumping_knowledge(P, "", x64)
        names = [k for k, _ in m.named_parameters()]
        grads = torch.autograd.grad(ref, x64 + [P[k] for k in names], gout.double())
        _REF[key] = (m.state_dict(), xs, gout, ref.detach(), grads[:L], dict(zip(names, grads[L:])))
    return _REF[key]


def _run(N, H, L, train=True):
    from analysisgnn_amd.core_layers import JumpingKnowledge
    sd, xs, gout, ref, gx, gp = _case(N, H, L)
    m = JumpingKnowledge(H, L)
    m.load_state_dict(sd)
    m = m.to(DEV).train(train)
    xd = [x.to(DEV).requires_grad_(True) for x in xs]
    out = m(xd)
    out.backward(gout.to(DEV))
    return m, xd, out


def _check_against_ref(N, H, L, m, xd, out):
    _, _, _, ref, gx, gp = _case(N, H, L)
    assert_close(out, ref, TOL, "out")
    for t in range(L):
        assert_close(xd[t].grad, gx[t], TOL, f"dx{t}")
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        assert_close(p.grad, gp[k], TOL, f"grad {k}")


SHAPES = [(130, 64, 3), (200, 256, 3), (130, 128, 2)]


@pytest.mark.parametrize("N,H,L", SHAPES)
def test_module_against_float64(N, H, L, fused, monkeypatch):
    from analysisgnn_amd import jk
    m, xd, out = _run(N, H, L)
    assert fused == [(N, H)] and jk.kernel_applicable(m, xd)
    _check_against_ref(N, H, L, m, xd, out)
    monkeypatch.setattr(jk, "FUSED", False)
    m0, xd0, out0 = _run(N, H, L)
    assert fused == [(N, H)], "FUSED = False must not reach the kernels"
    assert_close(out, out0, TOL, "fused vs library: out")
    for a, b in zip(xd, xd0):
        assert_close(a.grad, b.grad, TOL, "fused vs library: dx")
    for (k, p), q in zip(m.named_parameters(), m0.parameters()):
        assert_close(p.grad, q.grad, TOL, f"fused vs library: grad {k}")


# ---- 4. determinism and modes -------------------------------------------------------------------------------------------------
def test_two_runs_same_bits_and_no_grad_forward(fused):
    N, H, L = SHAPES[0]
    a = _run(N, H, L)
    b = _run(N, H, L)
    assert len(fused) == 2
    assert torch.equal(a[2], b[2])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x.grad, y.grad)
    for (k, p), q in zip(a[0].named_parameters(), b[0].parameters()):
        assert torch.equal(p.grad, q.grad), k
    with torch.no_grad():
        out = a[0]([x.detach() for x in a[1]])
    assert len(fused) == 3 and not out.requires_grad
    assert torch.equal(out, a[2])


def test_eval_mode_with_gradients(fused):
    """The library LSTM refuses a backward pass in eval mode; the kernels do not care."""
    N, H, L = SHAPES[0]
    m, xd, out = _run(N, H, L, train=False)
    assert fused == [(N, H)] and not m.training
    _check_against_ref(N, H, L, m, xd, out)


# ---- 5. the encoders ----------------------------------------------------------------------------------------------------------
def _encoder_run(kind, defer):
    """(loss, {name: grad}, flat gradient) of one forward + backward on a sampled batch (64 target rows of ~300 notes)."""
    from analysisgnn_amd import dp
    from analysisgnn_amd.encoders import HybridGNN, MetricalGNN
    from analysisgnn_amd.synth import make_score_graph, sample_hops, torch_inputs
    g = sample_hops(make_score_graph(seed=2, n_notes=300), n_targets=64, num_neighbors=[4, 4], seed=1, random_targets=True)
    H, L = 64, 2
    torch.manual_seed(3)
    if kind == "hybrid":
        m = HybridGNN(metadata=g.metadata(), input_channels=H, hidden_channels=H, num_layers=L, dropout=0.0, use_jk=True)
    else:
        m = MetricalGNN(H, H, H, L, g.metadata(), dropout=0.0, use_jk=True)
    m = m.to(DEV).train()
    I = torch_inputs(g, in_channels=H, seed=1)
    assert I["batch_size"] < I["x_dict"]["note"].shape[0]
    xg = {k: v.to(DEV).requires_grad_(True) for k, v in I["x_dict"].items()}
    kw = dict(x_dict=xg, edge_index_dict={k: v.to(DEV) for k, v in I["edge_index_dict"].items()},
              batch_dict={k: v.to(DEV) for k, v in I["batch_dict"].items()}, batch_size=I["batch_size"],
              neighbor_mask_node=I["neighbor_mask_node"], neighbor_mask_edge=I["neighbor_mask_edge"])
    params, tight = dp.plan_parameters(m)
    flat = dp.FlatGradBuffer(params, views=False, tight=tight)
    dp.defer_weight_grads(defer)
    try:
        flat.zero()
        out = m(**kw)
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
        loss = (out * gout).sum()
        loss.backward()
        flat.pack()
        torch.cuda.synchronize()
        return float(loss), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, flat.flat.clone(), xg["note"].grad.clone()
    finally:
        dp.defer_weight_grads(False)
        flat.close()


@pytest.mark.parametrize("kind", ["hybrid", "metrical"])
def test_encoders_reach_the_kernels(kind, fused, monkeypatch):
    from analysisgnn_amd import jk
    on = _encoder_run(kind, False)
    assert fused == [(64, 64)], "the row-sliced layer outputs must reach the kernels"
    deferred = _encoder_run(kind, True)
    assert len(fused) == 2
    monkeypatch.setattr(jk, "FUSED", False)
    off = _encoder_run(kind, False)
    assert len(fused) == 2
    assert abs(on[0] - off[0]) <= TOL * max(1.0, abs(off[0]))
    assert set(on[1]) == set(off[1]) and any(k.startswith("jk.lstm.") for k in on[1])
    for k in off[1]:
        assert_close(on[1][k], off[1][k], TOL, f"fused vs library: grad {k}")
    assert_close(on[3], off[3], TOL, "fused vs library: grad x[note]")
    assert_close(deferred[2], on[2], TOL, "flat gradient with deferral vs without")
    assert float(on[2].abs().max()) > 0


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------------
def test_forward_backward_under_capture(fused):
    """After one eager step, forward + backward captured on one stream and replayed twice give the eager run's bits.
    The eager step runs on the stream that is captured afterwards and leaves no autograd graph behind: a gradient accumulator
    that outlives a step on ANOTHER stream (the default one) would make that stream wait for the capture — a second, never
    joined stream inside it."""
    from analysisgnn_amd.core_layers import JumpingKnowledge
    N, H, L = SHAPES[0]
    sd, xs, gout = _case(N, H, L)[:3]
    m = JumpingKnowledge(H, L)
    m.load_state_dict(sd)
    m = m.to(DEV)
    xd = [x.to(DEV).requires_grad_(True) for x in xs]
    gd = gout.to(DEV)
    leaves = xd + list(m.parameters())

    def step():
        out = m(xd)
        return (out.detach(), *torch.autograd.grad(out, leaves, gd))

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = step()
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)
    assert len(fused) == 2
