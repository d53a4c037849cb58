"""The plain-torch restatement of the pitch-spelling models (tests/pitch_spelling_ref.py: the schedule the HIP path uses) against the
fixtures the reference's own classes produced in float64 (tests/gen_golden_pitch_spelling.py; the graph models modulo PyG /
graphmuse semantics), and GraphNorm against values computed by hand.  No GPU.

Bound: both sides are float64 evaluations of the same function in different orders (the key-signature head's product split at
the seam, explicit recurrences instead of nn.GRU / nn.LSTM), so they agree to rounding: 1e-10 x the compared tensor's max-abs, a
few thousand float64 ulp.  A gradient that is zero in exact arithmetic (meta.zero_grads) is held against 1e-10 x the largest weight
gradient's max-abs."""
import numpy as np
import pytest
import torch

import pitch_spelling_ref as PR

TOL = 1e-10


def close(got, exp, what, scale=None):
    got, exp = got.detach().double(), torch.as_tensor(exp).double()
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    s = float(exp.abs().max()) if scale is None else scale
    err = float((got - exp).abs().max())
    assert err <= TOL * s, (what, err, TOL * s)


@pytest.mark.parametrize("name", PR.CASES)
def test_restatement_against_the_fixtures(name):
    z = PR.load_case(name)
    rec = PR.run_case(z)
    zero = set(str(k) for k in z["meta.zero_grads"])
    compared = 0
    for k in z:
        if k.startswith(("out.", "mid.", "grad.", "gw.")):
            assert k in rec, f"{k}: the restatement gives no such tensor"
            close(rec[k], z[k], f"{name} {k}", float(z["meta.grad_max"]) if k in zero else None)
            compared += 1
    assert compared >= 3 + len(z["meta.keys"]) - len(z["meta.no_grad"]) - sum(1 for k in z["meta.keys"] if "running_" in str(k) or "num_batches" in str(k))
    with_grad = {k[3:] for k in rec if k.startswith("gw.")}
    floats = {str(k) for k in z["meta.keys"] if "running_" not in str(k) and "num_batches" not in str(k)}
    assert floats - with_grad == set(str(k) for k in z["meta.no_grad"])
    assert float(z["meta.fp32_over_gate"]) <= 0.25 and float(z["meta.norm_min_ratio"]) >= 0.05 and float(z["meta.relu_margin"]) > 3e-6


def test_fixture_files_hold_arrays_only_and_stay_small():
    import os
    for name in PR.CASES:
        path = os.path.join(PR.GOLDEN, "pitch_spelling_" + name + ".npz")
        assert os.path.getsize(path) < 2 ** 20
        with np.load(path, allow_pickle=False) as d:
            assert all(d[k].dtype.kind in "fiuU" for k in d.files)


def test_graphnorm_by_hand():
    """5 rows, 2 graphs, 2 columns, mean_scale 0.5, weight 2, bias 1, eps 0 — every figure worked out on paper.
    graph 0 = rows 0, 1, 3: column 0 holds 1, 3, 5: m = 3, o = x - 1.5 = (-0.5, 1.5, 3.5), v = (0.25 + 2.25 + 12.25) / 3 = 59 / 12;
    graph 1 = rows 2, 4:    column 0 holds 2, 6: m = 4, o = x - 2 = (0, 4), v = 8.
    Column 1 is constant 4 in both graphs: m = 4, o = 2, v = 4, y = 2 * 2 / 2 + 1 = 3."""
    x = torch.tensor([[1.0, 4.0], [3.0, 4.0], [2.0, 4.0], [5.0, 4.0], [6.0, 4.0]], dtype=torch.float64)
    batch = torch.tensor([0, 0, 1, 0, 1])
    w, b, ms = torch.full((2,), 2.0, dtype=torch.float64), torch.ones(2, dtype=torch.float64), torch.full((2,), 0.5, dtype=torch.float64)
    y = PR.graph_norm(x, w, b, ms, batch, 2, eps=0.0)
    r0, r1 = (59.0 / 12.0) ** 0.5, 8.0 ** 0.5
    exp = torch.tensor([[1 + 2 * -0.5 / r0, 3.0], [1 + 2 * 1.5 / r0, 3.0], [1 + 2 * 0.0 / r1, 3.0], [1 + 2 * 3.5 / r0, 3.0], [1 + 2 * 4.0 / r1, 3.0]],
                       dtype=torch.float64)
    assert float((y - exp).abs().max()) < 1e-14
    # v is the mean of o^2, NOT the centred variance: with mean_scale = 1 the two coincide, with 0.5 they do not
    centred = (x[batch == 1][:, 0] - 4.0).pow(2).mean()
    assert float(centred) == 4.0 and abs(float(((x[4, 0] - 2.0) / (y[4, 0] - 1) * 2) ** 2) - 8.0) < 1e-12


def test_graphnorm_one_row_graph_and_empty_graph_id():
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(4, 3, generator=gen, dtype=torch.float64)
    w, b = torch.randn(3, generator=gen, dtype=torch.float64), torch.randn(3, generator=gen, dtype=torch.float64)
    one = torch.ones(3, dtype=torch.float64)
    # graph 1 has one row: with mean_scale = 1 its output is the bias, whatever x holds (BatchNorm refuses n = 1; GraphNorm does not)
    y = PR.graph_norm(x, w, b, one, torch.tensor([0, 1, 0, 0]), 2)
    assert torch.equal(y[1], b)
    # graph id 1 has no row: the same values as without it
    with_gap = PR.graph_norm(x, w, b, 0.7 * one, torch.tensor([0, 2, 0, 2]), 3)
    dense = PR.graph_norm(x, w, b, 0.7 * one, torch.tensor([0, 1, 0, 1]), 2)
    assert torch.equal(with_gap, dense) and bool(torch.isfinite(with_gap).all())
    y2, dx, dw, db, dms = PR.graph_norm_grads(x, w, b, 0.7 * one, torch.tensor([0, 2, 0, 2]), 3, torch.ones(4, 3))
    assert all(bool(torch.isfinite(t).all()) for t in (y2, dx, dw, db, dms))
    assert torch.equal(db, torch.full((3,), 4.0, dtype=torch.float64))
    # batch=None is one graph
    assert torch.equal(PR.graph_norm(x, w, b, one, None), PR.graph_norm(x, w, b, one, torch.zeros(4, dtype=torch.long), 1))


def test_gradients_match_the_formulas_of_the_header():
    """do = w rstd (g - ohat mean_g(g ohat)), dx = do - mean_scale mean_g(do), dweight = sum g ohat, dbias = sum g,
    dmean_scale = -sum_g n_g m_g mean_g(do): the formulas include/agnn.h states, against autograd."""
    gen = torch.Generator().manual_seed(1)
    n, C, G = 9, 3, 3
    x, g = torch.randn(n, C, generator=gen, dtype=torch.float64), torch.randn(n, C, generator=gen, dtype=torch.float64)
    w, b, ms = [torch.randn(C, generator=gen, dtype=torch.float64) for _ in range(3)]
    batch = torch.tensor([0, 0, 0, 0, 2, 2, 2, 1, 1])
    _, dx, dw, db, dms = PR.graph_norm_grads(x, w, b, ms, batch, G, g)
    e_dx, e_dw, e_dms = torch.zeros_like(x), torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for k in range(G):
        rows = batch == k
        m = x[rows].mean(dim=0)
        o = x[rows] - ms * m
        rstd = 1.0 / torch.sqrt((o * o).mean(dim=0) + PR.EPS)
        oh = o * rstd
        do = w * rstd * (g[rows] - oh * (g[rows] * oh).mean(dim=0))
        e_dx[rows] = do - ms * do.mean(dim=0)
        e_dw += (g[rows] * oh).sum(dim=0)
        e_dms -= int(rows.sum()) * m * do.mean(dim=0)
    for got, exp in ((dx, e_dx), (dw, e_dw), (db, g.sum(dim=0)), (dms, e_dms)):
        assert float((got - exp).abs().max()) <= 1e-12 * float(exp.abs().max())
