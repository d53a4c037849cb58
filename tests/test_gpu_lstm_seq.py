"""Persistent LSTM kernels (csrc/lstmseq.hip, analysisgnn_amd/lstm_seq.py) vs the explicit-recurrence oracle
(oracle/rnn_ref.lstm, itself pinned against torch.nn.LSTM).  fp32; the GRU kernels' tolerance: 1e-4 relative to
max(1, |ref|max) for outputs, input gradients and all weight gradients.

The shapes are the smallest at which the operand ring (4 slots), the loaders' look-ahead (8 register sets forward, 4 or 8
backward), the unrolled loops' tails and both instantiations can go wrong; none is a workload's size."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import pitch_spelling_ref as PR  # noqa: E402
from helpers import assert_close  # noqa: E402

DEV = "cuda:0"
TOL = 1e-4


def _module(I, hidden, layers, seed, dropout=0.0):
    torch.manual_seed(seed)
    m = torch.nn.LSTM(I, hidden, num_layers=layers, batch_first=True, bidirectional=True, dropout=dropout)
    with torch.no_grad():                      # larger recurrent weights: make the chain matter
        for n, p in m.named_parameters():
            if "weight_hh" in n:
                p.mul_(2.0)
    return m


def _run(B, T, I, layers, seed, hidden=128):
    from analysisgnn_amd.lstm_seq import kernel_applicable, lstm_forward
    from oracle import rnn_ref
    m = _module(I, hidden, layers, seed)
    assert kernel_applicable(m)
    x = torch.randn(B, T, I)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xc = x.clone().requires_grad_(True)
    ref = rnn_ref.lstm(P, "", xc, layers, True)
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(seed + 1))
    (ref * gout).sum().backward()
    mg = m.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    out = lstm_forward(mg, xg, training=False)
    assert_close(out, ref, TOL, "y")
    (out * gout.to(DEV)).sum().backward()
    assert_close(xg.grad, xc.grad, TOL, "dx")
    for n, p in mg.named_parameters():
        assert_close(p.grad, P[n].grad, TOL, f"d{n}")
    assert set(dict(mg.named_parameters())) == set(P)


@pytest.mark.parametrize("B,T,I,layers", [(1, 1, 8, 1), (2, 2, 8, 2), (2, 3, 8, 1), (1, 4, 8, 2), (3, 5, 8, 1), (2, 6, 8, 1), (2, 7, 8, 2),
                                           (3, 37, 64, 1), (2, 19, 256, 2), (5, 64, 32, 2)])
def test_lstm_hidden_128(B, T, I, layers):
    _run(B, T, I, layers, seed=B * 100 + T)


@pytest.mark.parametrize("B,T,I,layers", [(1, 1, 8, 1), (3, 37, 64, 1), (4, 50, 128, 2)])
def test_lstm_hidden_64(B, T, I, layers):
    """The hidden-64 instantiation: eight k chunks of eight columns, the gate math on wave 0 only; backward with half the lanes
    carrying units and eight register sets in the loader."""
    _run(B, T, I, layers, seed=B * 10 + T, hidden=64)


def test_lstm_odd_input_width():
    """PitchSpelling's `[x | out_pc]` input has width 99: the weight gradient of W_ih takes the padded / library path."""
    _run(2, 9, 99, 1, seed=99)


def test_other_hidden_sizes_use_library_rnn():
    from analysisgnn_amd.lstm_seq import kernel_applicable, lstm_forward
    m = torch.nn.LSTM(16, 32, num_layers=2, batch_first=True, bidirectional=True).to(DEV)
    assert not kernel_applicable(m)
    x = torch.randn(2, 5, 16, device=DEV)
    assert torch.allclose(lstm_forward(m, x, False), m(x)[0])


@pytest.mark.parametrize("B,T,I,hidden", [(3, 41, 64, 128), (2, 13, 16, 64)])
def test_inter_layer_dropout_rides_with_the_recurrence_kernels(B, T, I, hidden):
    """nn.LSTM(dropout=p) between the two layers as a factor the first layer's kernels apply themselves: with a GIVEN
    0 / (1 / (1 - p)) pattern, outputs and all gradients equal those of two one-layer LSTMs with `y0 * pattern` between them
    (torch.nn.LSTM on the GPU as the yardstick); and in training mode the first layer's outputs really are dropped."""
    from analysisgnn_amd.gru import _stack_gru_params
    from analysisgnn_amd.lstm_seq import _LSTMLayer, lstm_forward
    torch.manual_seed(B + T)
    H2 = 2 * hidden
    m = torch.nn.LSTM(I, hidden, num_layers=2, batch_first=True, bidirectional=True, dropout=0.3).to(DEV)
    x = torch.randn(B, T, I, device=DEV)
    pattern = (torch.rand(B, T, H2, device=DEV) >= 0.3).float() / 0.7
    l0 = torch.nn.LSTM(I, hidden, batch_first=True, bidirectional=True).to(DEV)
    l1 = torch.nn.LSTM(H2, hidden, batch_first=True, bidirectional=True).to(DEV)
    sd = m.state_dict()
    l0.load_state_dict({k: sd[k] for k in l0.state_dict()})
    l1.load_state_dict({k: sd[k.replace("_l0", "_l1")] for k in l1.state_dict()})
    xr = x.clone().requires_grad_(True)
    ref = l1(l0(xr)[0] * pattern)[0]
    gout = torch.randn_like(ref)
    (ref * gout).sum().backward()
    xg = x.clone().requires_grad_(True)
    st = _stack_gru_params(m)
    y0 = _LSTMLayer.apply(xg, st[0], st[1], st[2], st[3], pattern)
    out = _LSTMLayer.apply(y0, st[4], st[5], st[6], st[7], None)
    assert_close(out, ref, TOL, "y")
    (out * gout).sum().backward()
    assert_close(xg.grad, xr.grad, TOL, "dx")
    for n, p in m.named_parameters():
        src = l0 if n.endswith("_l0") or n.endswith("_l0_reverse") else l1
        pr = dict(src.named_parameters())[n.replace("_l1", "_l0")]
        assert_close(p.grad, pr.grad, TOL, f"d{n}")
    with torch.no_grad():
        a = lstm_forward(m.train(), x, training=True)
        b = lstm_forward(m, x, training=True)
        c = lstm_forward(m, x, training=False)
    assert not torch.equal(a, b) and not torch.equal(a, c)


def _direct(B, T, hidden, fill, seed, drop=False):
    """The two entry points called directly into buffers pre-filled with `fill`: (y, saved, y_drop, dg, hprev, drop_scale)."""
    from analysisgnn_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                                 # noqa: E731
    gi, w, b = r(B, T, 2, 4 * hidden), r(2, 4 * hidden, hidden) * 0.1, r(2, 4 * hidden)
    dy = r(B, T, 2 * hidden)
    scale = ((torch.rand(B, T, 2 * hidden, generator=g) >= 0.3).float() / 0.7).to(DEV) if drop else None
    st = _lib.stream_ptr(torch.device(DEV))
    y = torch.full((B, T, 2 * hidden), fill, device=DEV)
    saved = torch.full((B, T, 2, 5, hidden), fill, device=DEV)
    yd = torch.full_like(y, fill) if drop else None
    _lib.check(lib.agnn_lstm_seq_fwd_f32(gi.data_ptr(), w.data_ptr(), b.data_ptr(), B, T, hidden, y.data_ptr(), saved.data_ptr(),
                                         _lib.ptr(scale), _lib.ptr(yd), st), "fwd")
    dg = torch.full((B, T, 2, 4 * hidden), fill, device=DEV)
    hp = torch.full((B, T, 2, hidden), fill, device=DEV)
    _lib.check(lib.agnn_lstm_seq_bwd_f32(dy.data_ptr(), y.data_ptr(), saved.data_ptr(), w.data_ptr(), B, T, hidden, dg.data_ptr(),
                                         _lib.ptr(scale), hp.data_ptr(), st), "bwd")
    dg2 = torch.full_like(dg, fill)
    _lib.check(lib.agnn_lstm_seq_bwd_f32(dy.data_ptr(), None, saved.data_ptr(), w.data_ptr(), B, T, hidden, dg2.data_ptr(),
                                         _lib.ptr(scale), None, st), "bwd without hprev")
    assert torch.equal(dg, dg2)
    return y, saved, yd, dg, hp, scale


@pytest.mark.parametrize("fill", [float("nan"), float("inf"), -1e38])
@pytest.mark.parametrize("B,T,hidden", [(2, 40, 128), (3, 23, 64)])
def test_results_ignore_what_the_buffers_held(B, T, hidden, fill):
    """Without dropout the forward kernel gets its output buffer as a stand-in for the dropout-scale operand and reads it AHEAD
    of the walk: whatever the allocator left there must not reach a result.  Same bits as into zero-filled buffers, forward and
    backward, `hprev` and the gradient buffer included."""
    clean = _direct(B, T, hidden, 0.0, seed=11)
    dirty = _direct(B, T, hidden, fill, seed=11)
    for a, c in zip(clean, dirty):
        if a is not None:
            assert torch.isfinite(c).all()
            assert torch.equal(a, c)


@pytest.mark.parametrize("B,T,hidden,drop", [(1, 1, 128, False), (3, 37, 128, True), (2, 6, 128, False), (4, 50, 64, True), (2, 9, 64, False)])
def test_backward_walk_leaves_previous_states(B, T, hidden, drop):
    """`hprev` = y shifted by one step per direction (zero at each chain's first step), bit for bit: the walk copies y, the
    undropped state, also under dropout; and y_drop = y * drop_scale."""
    y, saved, yd, dg, hp, scale = _direct(B, T, hidden, float("nan"), seed=5, drop=drop)
    want = torch.zeros_like(hp)
    want[:, 1:, 0] = y[:, :-1, :hidden]
    want[:, :-1, 1] = y[:, 1:, hidden:]
    assert torch.equal(hp, want)
    assert torch.isfinite(dg).all() and torch.isfinite(saved).all()
    if drop:
        assert torch.equal(yd, y * scale) and bool((yd == 0).any())


def _step(m, x, gout, training=False):
    from analysisgnn_amd.lstm_seq import lstm_forward
    leaves = [x] + list(m.parameters())
    out = lstm_forward(m, x, training)
    return (out.detach(), *torch.autograd.grad(out, leaves, gout))


@pytest.mark.parametrize("hidden", [128, 64])
def test_two_runs_give_identical_bits_and_eval_mode_has_a_backward(hidden):
    """No atomics, fixed-order sums: the same bits on every run.  And a backward in eval() mode, which the library LSTM refuses
    (tests/test_gpu_jk.py), gives the training-mode gradients (no dropout configured)."""
    m = _module(24, hidden, 2, seed=3).to(DEV)
    x = torch.randn(3, 29, 24, device=DEV, requires_grad=True)
    gout = torch.randn(3, 29, 2 * hidden, device=DEV)
    a = _step(m.train(), x, gout, training=True)
    b = _step(m, x, gout, training=True)
    c = _step(m.eval(), x, gout, training=False)
    assert len(a) == 2 + 16
    for u, v, w in zip(a, b, c):
        assert torch.isfinite(u).all() and float(u.abs().max()) > 0
        assert torch.equal(u, v) and torch.equal(u, w)


@pytest.mark.parametrize("hidden", [128, 64])
def test_parameter_gradients_own_their_memory(hidden):
    """`db_hh` has `db_ih`'s values, not its memory: no two parameters' `.grad` overlap, so gradient accumulation over two
    backwards and an in-place `clip_grad_norm_` give what the library LSTM gives (with one storage behind both biases the
    accumulation adds twice and the clipping scales twice)."""
    import copy
    from analysisgnn_amd.lstm_seq import lstm_forward
    m = _module(12, hidden, 2, seed=21).to(DEV).train()
    lib = copy.deepcopy(m)
    x = torch.randn(2, 11, 12, device=DEV)
    gouts = [torch.randn(2, 11, 2 * hidden, device=DEV) for _ in range(2)]
    for g in gouts:                             # two backwards into the same `.grad`s
        (lstm_forward(m, x, True) * g).sum().backward()
        (lib(x)[0] * g).sum().backward()
    spans = sorted((p.grad.data_ptr(), p.grad.data_ptr() + 4 * p.grad.numel(), n) for n, p in m.named_parameters())
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, f"the gradients of {an} and {bn} overlap"
    for n, p in m.named_parameters():
        assert_close(p.grad, dict(lib.named_parameters())[n].grad, TOL, f"accumulated d{n}")
    na = torch.nn.utils.clip_grad_norm_(m.parameters(), 0.5)
    nb = torch.nn.utils.clip_grad_norm_(lib.parameters(), 0.5)
    assert float(nb) > 0.5 and abs(float(na) - float(nb)) <= TOL * float(nb)
    for n, p in m.named_parameters():
        assert_close(p.grad, dict(lib.named_parameters())[n].grad, TOL, f"clipped d{n}")


def test_forward_backward_under_capture():
    """After one eager step, forward + backward captured on one stream and replayed twice give the eager run's bits
    (tests/test_gpu_jk.py's recipe: the eager step runs on the stream that is captured afterwards)."""
    m = _module(16, 128, 2, seed=8).to(DEV)
    x = torch.randn(2, 21, 16, device=DEV, requires_grad=True)
    gout = torch.randn(2, 21, 256, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        eager = [t.clone() for t in _step(m, x, gout)]
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = _step(m, x, gout)
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)


# ---- PKSpell at kernel size ---------------------------------------------------------------------------------------------------------
def test_pkspell_lstm_on_the_persistent_kernels():
    """PKSpell(8, 128, 128, ..., cell_type="LSTM", dropout=0.0) against tests/pitch_spelling_ref.py's float64 restatement on the
    same state_dict, as the GRU case of tests/test_gpu_pitch_spelling.py: outputs, grad.x and every weight gradient."""
    from analysisgnn_amd import lstm_seq, pitch_spelling
    torch.manual_seed(3)
    cfg = dict(kind="pkspell", in_feats=8, h1=128, h2=128, depth=1, cell="LSTM")
    model = pitch_spelling.PKSpell(8, 128, 128, PR.OUT_PC, dropout=0.0, cell_type="LSTM")
    assert lstm_seq.kernel_applicable(model.rnn) and lstm_seq.kernel_applicable(model.rnn2)
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():                       # bf16-exact weights, as the GRU case draws them
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=gen) * 0.1)
            p.copy_(p.bfloat16().float())
    model = model.to(DEV).train()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    x = torch.randn(19, 8, generator=torch.Generator().manual_seed(5))
    lens = [11, 7, 1]
    calls = []
    orig = lstm_seq._LSTMLayer.apply
    xg = x.to(DEV).requires_grad_(True)
    try:
        lstm_seq._LSTMLayer.apply = lambda *a: (calls.append(1), orig(*a))[1]
        out_pc, out_ks = model(xg, lens)
    finally:
        lstm_seq._LSTMLayer.apply = orig
    assert len(calls) == 2                       # both stacks ran the kernels
    gen = torch.Generator().manual_seed(31)
    cot_pc, cot_ks = torch.randn(out_pc.shape, generator=gen), torch.randn(out_ks.shape, generator=gen)
    ((out_pc * cot_pc.to(DEV)).sum() + (out_ks * cot_ks.to(DEV)).sum()).backward()
    rec = PR.run_params(sd, cfg, dict(x=x, lens=lens), cot_pc, cot_ks)

    def close(got, exp, what):                   # GATE of tests/test_gpu_pitch_spelling.py: 1e-4 x max-abs of the compared tensor
        got, exp = got.detach().double().cpu(), exp.detach().double().cpu()
        assert got.shape == exp.shape, (what, got.shape, exp.shape)
        err, s = float((got - exp).abs().max()), float(exp.abs().max())
        print(f"{what}: err {err:.3e}  bound {TOL * s:.3e}")
        assert err <= TOL * s, (what, err, TOL * s)

    close(out_pc, rec["out.pc"], "out.pc")
    close(out_ks, rec["out.ks"], "out.ks")
    close(xg.grad, rec["grad.x"], "grad.x")
    n = 0
    for k, p in model.named_parameters():
        if p.grad is not None:
            close(p.grad, rec["gw." + k], f"gw.{k}")
            n += 1
        else:
            assert "gw." + k not in rec, k
    assert n >= 20
