"""`chord.PostProcessingMLTModel` (the reference's models/chord.py:751-783) on the GPU.

Small fixtures (tests/golden/postprocess_*.npz, written by tests/gen_golden_postprocess.py from a float64 run of the reference's
own class): n_hidden 16, one layer — the library-RNN path — as a batch, as a 2-D input (the unsqueeze / squeeze route) and as a
batch of one.  At n_hidden 64 and 128 with two layers, where the LSTM runs the persistent kernels, the model is held against the
float64 restatement below, built from oracle/rnn_ref.lstm; the restatement itself is first held against the fixtures on the CPU.

Tolerance: the GRU kernels' — helpers.assert_close at 1e-4 relative to max(1, |ref|max) — for outputs, input gradients and every
weight gradient."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, load_golden

DEV = "cuda:0"
TOL = 1e-4
CASES = ["postprocess_h16_batch", "postprocess_h16_2d", "postprocess_h16_one"]


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------------
def restatement(P, tasks, n_layers, x):
    """{task: logits} of the model on the state_dict `P` (dropout 0, ReLU): its forward written out on the explicit recurrence."""
    from oracle import rnn_ref
    h = torch.cat([F.softmax(x[t], dim=-1) for t in tasks], dim=-1)
    if h.dim() == 2:
        h = h.unsqueeze(0)
    h = rnn_ref.lstm(P, "lstm.", h, n_layers, True).squeeze()
    h = F.normalize(F.relu(h @ P["fc.weight"].t() + P["fc.bias"]), p=2, dim=-1)
    return {t: h @ P[f"clf.{t}.weight"].t() + P[f"clf.{t}.bias"] for t in tasks}


def run_restatement(sd, tasks, n_layers, x, cot, dtype=torch.float64):
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xs = {t: v.detach().to(dtype).clone().requires_grad_(True) for t, v in x.items()}
    out = restatement(P, tasks, n_layers, xs)
    sum((out[t] * cot[t].to(dtype)).sum() for t in tasks).backward()
    rec = {"out." + t: v.detach() for t, v in out.items()}
    rec.update({"grad.in." + t: v.grad for t, v in xs.items()})
    rec.update({"gw." + k: v.grad for k, v in P.items()})
    return rec


def fixture(name):
    z = load_golden(name)
    tasks = {str(t): int(c) for t, c in zip(z["meta.tasks"], z["meta.classes"])}
    n_hidden, n_layers = int(z["meta.cfg"][0]), int(z["meta.cfg"][1])
    sd = {str(k): torch.from_numpy(np.asarray(z["w." + str(k)])) for k in z["meta.keys"]}
    x = {t: torch.from_numpy(np.asarray(z["in." + t])) for t in tasks}
    cot = {t: torch.from_numpy(np.asarray(z["cot." + t])) for t in tasks}
    want = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith(("out.", "grad.in.", "gw."))}
    return tasks, n_hidden, n_layers, sd, x, cot, want


def run_model(model, tasks, x, cot):
    xs = {t: v.to(DEV).requires_grad_(True) for t, v in x.items()}
    out = model(xs)
    assert list(out.keys()) == list(tasks.keys())
    sum((out[t] * cot[t].to(DEV)).sum() for t in tasks).backward()
    rec = {"out." + t: v.detach() for t, v in out.items()}
    rec.update({"grad.in." + t: v.grad for t, v in xs.items()})
    rec.update({"gw." + k: p.grad for k, p in model.named_parameters()})
    return rec


def compare(got, want, what):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k in sorted(want):
        assert got[k] is not None, k
        assert_close(got[k], want[k], TOL, f"{what} {k}")


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    """The float64 restatement on the fixture's weights gives the reference's outputs and gradients (to float64 rounding)."""
    tasks, n_hidden, n_layers, sd, x, cot, want = fixture(name)
    rec = run_restatement(sd, tasks, n_layers, x, cot)
    assert set(rec) == set(want)
    for k in want:
        assert_close(rec[k], want[k], 1e-10, f"{name} {k}")


def test_fixtures_hold_data_only_and_state_dicts_load_strictly():
    from analysisgnn_amd.chord import PostProcessingMLTModel
    for name in CASES:
        z = load_golden(name)
        assert all(k.split(".")[0] in ("meta", "in", "cot", "w", "out", "grad", "gw") for k in z.files)
        tasks, n_hidden, n_layers, sd, x, cot, want = fixture(name)
        model = PostProcessingMLTModel(tasks, n_hidden, n_layers)
        assert list(model.state_dict().keys()) == list(sd.keys())
        model.load_state_dict(sd, strict=True)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_model_on_the_fixture(name):
    from analysisgnn_amd import lstm_seq
    from analysisgnn_amd.chord import PostProcessingMLTModel
    tasks, n_hidden, n_layers, sd, x, cot, want = fixture(name)
    model = PostProcessingMLTModel(tasks, n_hidden, n_layers, dropout=0.0)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).train()
    assert not lstm_seq.kernel_applicable(model.lstm)                       # hidden 16: the library RNN
    got = run_model(model, tasks, x, cot)
    for t in tasks:
        assert got["out." + t].shape == want["out." + t].shape              # the squeeze: [3, 7, C], [11, C], [9, C]
    compare(got, want, name)


@pytest.mark.gpu
@pytest.mark.parametrize("n_hidden,shape", [(64, (3, 23)), (128, (2, 37)), (128, (19,)), (64, (1, 12))])
def test_model_on_the_persistent_kernels(n_hidden, shape):
    """n_layers 2 at the kernel widths, as a batch, a 2-D input and a batch of one, against the float64 restatement on the same
    state_dict; the LSTM really runs the kernels (two layers: two `_LSTMLayer` nodes)."""
    from analysisgnn_amd import lstm_seq
    from analysisgnn_amd.chord import PostProcessingMLTModel
    tasks = {"localkey": 38, "degree1": 22, "quality": 11, "inversion": 4}
    torch.manual_seed(n_hidden + len(shape))
    model = PostProcessingMLTModel(tasks, n_hidden, 2, dropout=0.0)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.bfloat16().float())
    assert lstm_seq.kernel_applicable(model.lstm)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(5)
    x = {t: 2.0 * torch.randn(shape + (c,), generator=gen) for t, c in tasks.items()}
    out_shape = tuple(d for d in shape if d != 1)
    cot = {t: torch.randn(out_shape + (c,), generator=gen) for t, c in tasks.items()}
    want = run_restatement(sd, tasks, 2, x, cot)
    model = model.to(DEV).train()
    calls = []
    orig = lstm_seq._LSTMLayer.apply
    try:
        lstm_seq._LSTMLayer.apply = lambda *a: (calls.append(1), orig(*a))[1]
        got = run_model(model, tasks, x, cot)
    finally:
        lstm_seq._LSTMLayer.apply = orig
    assert len(calls) == 2
    compare(got, want, f"n_hidden={n_hidden} shape={shape}")


@pytest.mark.gpu
def test_dropout_and_predict():
    """Training-mode dropout (between the LSTM layers and behind `normalize`) changes the outputs from call to call, evaluation
    does not; `predict` passes `onset` and `s_measure` through and ignores other keys."""
    from analysisgnn_amd.chord import PostProcessingMLTModel
    tasks = {"quality": 11, "inversion": 4}
    torch.manual_seed(2)
    model = PostProcessingMLTModel(tasks, 64, 2, dropout=0.3).to(DEV)
    x = {t: torch.randn(2, 15, c, device=DEV) for t, c in tasks.items()}
    with torch.no_grad():
        a, b = model.train()(x), model(x)
        c, d = model.eval()(x), model(x)
    assert not torch.equal(a["quality"], b["quality"])
    assert torch.equal(c["quality"], d["quality"]) and torch.equal(c["inversion"], d["inversion"])
    onset, meas = torch.arange(15), torch.zeros(15)
    out = model.predict(dict(x, onset=onset, s_measure=meas, other=torch.ones(3, device=DEV)))
    assert set(out) == {"quality", "inversion", "onset", "s_measure"} and out["onset"] is onset and out["s_measure"] is meas
    assert torch.equal(out["quality"], c["quality"])
