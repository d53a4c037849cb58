"""tests/cadence_ref.py — the plain-torch statement of the cadence models in the schedule of analysisgnn_amd/cadence.py — held against
the fixtures the reference's own classes produced (tests/gen_golden_cadence.py, float64), before any kernel is involved; and the
formulas of the join and of the loss held against torch: the pooling against oracle/scatter_ref.py and autograd, the balanced cross
entropy against F.cross_entropy(weight=...).  CPU, float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cadence_ref as CR
from oracle import scatter_ref

GATE = 1e-4


def _close(a, b, tol, what, scale=None):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} vs {tuple(b.shape)}"
    s = float(b.abs().max()) if scale is None else scale
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * s, f"{what}: {err:.3e} > {tol:g} * {s:.3g}"


@pytest.mark.parametrize("name", CR.CASES)
def test_restatement_reproduces_the_reference(name):
    z = CR.load_case(name)
    rec = CR.run_case(z)
    gmax = float(z["meta.grad_max"])
    zero = set(str(k) for k in z["meta.zero_grads"])
    seen = 0
    for k in z:
        if k.split(".")[0] not in ("out", "mid", "grad", "gw"):
            continue
        assert k in rec, f"{name}: the restatement has no {k}"
        _close(rec[k], z[k], 1e-9, f"{name} {k}", gmax if k in zero else None)
        seen += 1
    assert seen >= 8 and not [k for k in rec if k not in z], [k for k in rec if k not in z]


@pytest.mark.parametrize("name", CR.CASES)
def test_fixture_margins(name):
    """What the generator promised: no ReLU input at the kink, no near-constant BatchNorm column, fp32 within a quarter of the gate."""
    z = CR.load_case(name)
    assert float(z["meta.relu_margin"]) > 3e-6 and float(z["meta.fp32_over_gate"]) <= 0.25
    if CR.config(z)["training"]:
        assert float(z["meta.norm_min_ratio"]) >= 0.05
    if CR.config(z)["kind"] == "pytorch" and not CR.config(z)["use_ps"]:
        assert list(z["meta.set_attr"]) == ["use_pitch_spelling"]


def test_restatement_in_fp32_passes_the_gate():
    """The gate the kernels are held to is one the reference's arithmetic itself meets in fp32."""
    for name in CR.CASES:
        z = CR.load_case(name)
        rec = CR.run_case(z, torch.float32)
        gmax = float(z["meta.grad_max"])
        zero = set(str(k) for k in z["meta.zero_grads"])
        for k, v in rec.items():
            _close(v, z[k], GATE, f"{name} {k}", gmax if k in zero else None)


@pytest.mark.parametrize("skip_self", [False, True])
@pytest.mark.parametrize("n", [1, 3, 33])
def test_pool_formula_is_scatter_mean(n, skip_self):
    """pool() with pool_rows = col_limit = n is torch_scatter.scatter_mean(x[src], dst, out=x.clone()) on the (filtered) list, and
    pool_bwd() is its gradient."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 8, generator=g, dtype=torch.float64, requires_grad=True)
    src, dst = CR.join_graph(n)
    keep = (src != dst) if skip_self else torch.ones_like(src, dtype=torch.bool)
    want = scatter_ref.scatter_mean(x[src[keep]], dst[keep], dim=0, out=x.clone())
    got, inv = CR.pool(x, src, dst, n, n, skip_self)
    _close(got.detach(), want.detach(), 1e-12, "pooled")
    du = torch.randn(n, 8, generator=g, dtype=torch.float64)
    dx, = torch.autograd.grad((want * du).sum(), x)
    _close(CR.pool_bwd(du, src, dst, inv, n, n, skip_self), dx, 1e-12, "dx")


@pytest.mark.parametrize("skip_self", [False, True])
def test_pool_formula_with_limits(skip_self):
    """pool_rows = col_limit = n - 2: rows behind keep their value, sources behind are dropped; the backward formula is autograd's."""
    n = 33
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, 8, generator=g, dtype=torch.float64, requires_grad=True)
    src, dst = CR.join_graph(n)
    u, inv = CR.pool(x, src, dst, n - 2, n - 2, skip_self)
    assert torch.equal(u[n - 2:].detach(), x[n - 2:].detach()) and torch.equal(u[0].detach(), x[0].detach())     # row 0 is isolated
    du = torch.randn(n, 8, generator=g, dtype=torch.float64)
    dx, = torch.autograd.grad((u * du).sum(), x)
    _close(CR.pool_bwd(du, src, dst, inv.detach(), n - 2, n - 2, skip_self), dx, 1e-12, "dx")


@pytest.mark.parametrize("n,C", [(1, 2), (63, 5), (1000, 37)])
def test_balanced_ce_formula_is_torch(n, C):
    g = torch.Generator().manual_seed(n + C)
    z = torch.randn(n, C, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.randint(0, max(C - 1, 1), (n,), generator=g)                  # the last class never occurs
    if n > 4:
        y[::7] = -100
    num = torch.bincount(y[y >= 0], minlength=C)
    weight = 1.0 / (num.double() + 1e-6)
    want = F.cross_entropy(z, y, weight=weight, ignore_index=-100)
    dz, = torch.autograd.grad(want, z)
    loss, d, count, w, bad = CR.balanced_ce(z.detach(), y)
    _close(loss, want.detach(), 1e-12, "loss")
    _close(d, dz, 1e-12, "dlogits")
    assert torch.equal(count, num) and bad == 0
    _close(w, weight, 1e-15, "weight")


def test_balanced_ce_empty_and_out_of_range():
    z = torch.randn(9, 5, dtype=torch.float64)
    loss, d, count, w, bad = CR.balanced_ce(z, torch.full((9,), -100))
    assert float(loss) == 0.0 and float(d.abs().max()) == 0.0 and int(count.sum()) == 0 and bad == 0
    y = torch.tensor([0, 1, 2, 3, 4, 0, 1, 2, 3])
    base = CR.balanced_ce(z[:8], y[:8])
    y2 = y.clone()
    y2[8] = 7
    with_bad = CR.balanced_ce(z, y2)
    assert with_bad[4] == 1 and float(with_bad[0]) == float(base[0]) and torch.equal(with_bad[1][:8], base[1]) and float(with_bad[1][8].abs().max()) == 0


def test_metrics_against_numpy():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(200, 5, generator=g)
    y = torch.randint(0, 4, (200,), generator=g)
    acc, f1 = CR.metrics(logits, y)
    p = logits.argmax(dim=1)
    assert acc == pytest.approx(float((p == y).double().mean()))
    per = [2.0 * int(((p == c) & (y == c)).sum()) / (int((p == c).sum()) + int((y == c).sum())) for c in range(5)
           if int((p == c).sum()) + int((y == c).sum())]
    assert f1 == pytest.approx(float(np.mean(per)))
