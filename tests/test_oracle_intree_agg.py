"""Pin oracle/intree_agg_ref.py (the plain statement of the edge-gated and the |h_i - h_j| aggregation that the kernel parity
tests compare with) against fixtures produced by the reference's own layers: composed with the layers' Linear maps as
oracle/intree_ref.res_gated_conv / rel_edge_conv compose them, it must give the fixtures' output, input gradient and every
parameter gradient.  fp32, tolerance 1e-5 relative to max(1, max|ref|), as tests/test_oracle_r2.py.  Also: gradcheck in
float64 and the tie behaviour of |.| (sign(0) = 0)."""
import pytest
import torch

from oracle import intree_agg_ref as A
from oracle.intree_ref import _degree, _lin
from helpers import inputs_from_npz, load_golden, params_from_npz
from test_oracle_intree import _check


@pytest.mark.parametrize("name", ["resgated", "resgated_edgefeat"])
def test_gated_reproduces_the_res_gated_fixtures(name):
    z = load_golden(name)
    gk = ["x"] + (["edge_features"] if "in.edge_features" in z.files else [])
    P, I = params_from_npz(z), inputs_from_npz(z, gk)
    x, ei = I["x"], I["edge_index"]
    c = _lin(P, "W5", I["edge_features"]) if "edge_features" in I and "W5.weight" in P else None
    S = A.gated_forward(_lin(P, "W3", x), _lin(P, "W4", x), _lin(P, "W2", x), c, ei[0], ei[1])
    _check(z, 2.0 * _lin(P, "W1", x) + S, P, I, gk)


@pytest.mark.parametrize("name", ["r2_reledge", "r2_reledge_edgefeat"])
def test_absdiff_reproduces_the_rel_edge_fixtures(name):
    """sum_j W_e [h_j || e_ij] + b_e = W_e [S_i || D_i] + deg_i b_e (given edge features: their row sums in place of D)."""
    z = load_golden(name)
    gk = ["x"] + (["edge_features"] if "in.edge_features" in z.files else [])
    P, I = params_from_npz(z), inputs_from_npz(z, gk)
    x, ei = I["x"], I["edge_index"]
    n = x.shape[0]
    h = _lin(P, "neigh_linear", x)
    S, D = A.absdiff_forward(h, ei[0], ei[1])
    if "edge_features" in I:
        D = A._index_sum(I["edge_features"], ei[0], n)
    deg = _degree(ei[0], n, x.dtype).unsqueeze(-1)
    msg = torch.cat([S, D], dim=-1) @ P["edge_linear.weight"].t()
    if "edge_linear.bias" in P:
        msg = msg + deg * P["edge_linear.bias"]
    s = (h + msg) / deg.clamp(min=1)
    _check(z, _lin(P, "linear", torch.cat([x, s], dim=-1)), P, I, gk)


def _five_nodes():
    g = torch.Generator().manual_seed(3)
    dst = torch.tensor([0, 0, 1, 2, 2, 2, 4, 4])
    src = torch.tensor([1, 3, 0, 2, 4, 4, 3, 0])                 # a self loop (2, 2), a duplicated edge (2, 4), row 3 without edges
    return g, dst, src


def test_gradcheck_float64():
    g, dst, src = _five_nodes()
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True)   # noqa: E731
    a, b, h, c = mk(5, 3), mk(5, 3), mk(5, 3), mk(8, 3)
    assert torch.autograd.gradcheck(lambda a, b, h, c: A.gated_forward(a, b, h, c, dst, src), (a, b, h, c))
    assert torch.autograd.gradcheck(lambda a, b, h: A.gated_forward(a, b, h, None, dst, src), (a, b, h))
    # bipartite: 5 destination rows, 4 source rows
    b4, h4 = mk(4, 3), mk(4, 3)
    assert torch.autograd.gradcheck(lambda a, b, h: A.gated_forward(a, b, h, None, dst, src.clamp(max=3)), (a, b4, h4))
    # |.| away from its kink: distinct random rows; the self loop contributes the constant 0
    assert torch.autograd.gradcheck(lambda h: A.absdiff_forward(h, dst, src), (h,))


def test_returned_gradients_are_those_of_the_inner_product():
    g, dst, src = _five_nodes()
    mk = lambda *s: torch.randn(*s, generator=g)                                            # noqa: E731
    a, b, h, c, ds = mk(5, 4), mk(5, 4), mk(5, 4), mk(8, 4), mk(5, 4)
    S, da, db, dh, dc = A.gated(a, b, h, c, dst, src, ds)
    assert S.dtype == torch.float64 and dc.shape == (8, 4)
    eps = 1e-6
    a2 = a.double().clone()
    a2[2, 1] += eps
    S2 = A.gated(a2, b, h, c, dst, src, ds)[0]
    assert abs(float(((S2 - S) * ds.double()).sum()) / eps - float(da[2, 1])) < 1e-5
    assert A.gated(a, b, h, None, dst, src, ds)[4] is None
    S32 = A.gated(a, b, h, c, dst, src, ds, dtype=torch.float32)[0]
    assert S32.dtype == torch.float32 and float((S32.double() - S).abs().max()) < 1e-5
    Sa, Da, dha = A.absdiff(h, dst, src, gs=ds, gd=None)
    assert torch.equal(Sa[3], torch.zeros(4, dtype=torch.float64)) and torch.equal(Da[3], torch.zeros(4, dtype=torch.float64))
    # S only: dh_j = sum of gs over the edges that gather j
    exp = torch.zeros(5, 4, dtype=torch.float64).index_add(0, src, ds.double()[dst])
    assert torch.allclose(dha, exp, atol=1e-12)


def test_ties_give_a_zero_gradient_of_D():
    """A self loop and two identical rows joined in both directions: |h_i - h_j| = 0 there and torch's subgradient is 0,
    so the D term adds nothing to either end — only the S term and the other edges remain."""
    g = torch.Generator().manual_seed(4)
    h = torch.randn(4, 6, generator=g)
    h[1] = h[0]
    dst = torch.tensor([0, 1, 0, 1, 2, 3])
    src = torch.tensor([1, 0, 0, 1, 2, 3])                        # 0 <-> 1 identical, self loops on every node
    gd = torch.randn(4, 6, generator=g)
    _, D, dh = A.absdiff(h, dst, src, gs=None, gd=gd)
    assert torch.equal(D, torch.zeros_like(D)) and torch.equal(dh, torch.zeros_like(dh))
    # one more edge between distinct rows: exactly its own contribution survives
    dst2, src2 = torch.cat([dst, torch.tensor([2])]), torch.cat([src, torch.tensor([0])])
    _, D2, dh2 = A.absdiff(h, dst2, src2, gs=None, gd=gd)
    sg = torch.sign(h[2].double() - h[0].double()) * gd[2].double()
    exp = torch.zeros(4, 6, dtype=torch.float64)
    exp[2], exp[0] = sg, -sg
    assert torch.equal(dh2, exp) and torch.equal(D2[2], (h[2].double() - h[0].double()).abs())
