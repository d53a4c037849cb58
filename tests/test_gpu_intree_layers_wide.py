"""The in-tree convolutions at the widths users pick — not the 8 and 12 of the fixtures — against oracle/intree_ref evaluated
in float64: ResGatedGraphConv at 250 (padded to 252 and sliced back) and 516 outputs, RelEdgeConv at 260 features, GATConvLayer
at 250 outputs, so that the second and third chunk instantiations of the aggregation kernels, a last chunk of one lane and
the weighted SpMM run under the layers that call them; and ops.aggregate with per-edge weights against the dense formula.
The graph is the 90-note chord plus ring of test_gpu_edge_cases.py (every chord note has 90 incoming edges and a self loop)
with four isolated notes behind it.  Forward, input gradients and every parameter gradient, each relative to its own
largest magnitude, at the project's 1e-4."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import assert_close_rel  # noqa: E402
from oracle import intree_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
TOL = 1e-4
N, N_RING = 154, 150


def _graph():
    """edge_index [2, 8250]: all 90 x 90 pairs among the first notes, a ring over the first 150, notes 150 .. 153 isolated."""
    a, b = np.nonzero(np.ones((90, 90), dtype=bool))
    ring = np.stack([np.arange(N_RING), (np.arange(N_RING) + 1) % N_RING])
    ei = torch.from_numpy(np.concatenate([np.stack([a, b]), ring], axis=1).astype(np.int64))
    return ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(0))]


def _check_layer(m, ref_fn, inputs, what):
    """m(*inputs on the device) against ref_fn(P float64, *inputs float64): forward, d inputs, d parameters."""
    P = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    m = m.to(DEV)
    cpu = [t.double().clone().requires_grad_(True) if t is not None and t.is_floating_point() else t for t in inputs]
    gpu = [t.to(DEV).requires_grad_(True) if t is not None and t.is_floating_point() else (t.to(DEV) if t is not None else None) for t in inputs]
    ref = ref_fn(P, *cpu)
    out = m(*gpu)
    assert_close_rel(out, ref, TOL, f"{what} forward")
    go = torch.randn(ref.shape, generator=torch.Generator().manual_seed(2))
    (ref * go.double()).sum().backward()
    (out * go.to(DEV)).sum().backward()
    for i, (c, g) in enumerate(zip(cpu, gpu)):
        if c is not None and c.is_floating_point():
            assert g.grad is not None, f"{what}: input {i} has no gradient"
            assert_close_rel(g.grad, c.grad, TOL, f"{what} d input {i}")
    n_par = 0
    for name, p in m.named_parameters():
        if P[name].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, f"{what} {name}: no gradient on the HIP path"
        assert_close_rel(p.grad, P[name].grad, TOL, f"{what} grad {name}")
        n_par += 1
    return n_par


@pytest.mark.parametrize("fin,fout,fe", [(32, 250, None), (48, 516, 5)])
def test_res_gated_conv_wide(fin, fout, fe):
    from analysisgnn_amd.core_layers import ResGatedGraphConv
    ei = _graph()
    g = torch.Generator().manual_seed(fout)
    torch.manual_seed(fout)
    x = torch.randn(N, fin, generator=g)
    ef = torch.randn(ei.shape[1], fe, generator=g) if fe else None
    m = ResGatedGraphConv(fin, fout, in_edge_features=fe)
    n_par = _check_layer(m, lambda P, x, ei, ef: R.res_gated_conv(P, "", x, ei, ef), [x, ei, ef], f"ResGatedGraphConv({fin}, {fout}, {fe})")
    assert n_par == (10 if fe else 8)


@pytest.mark.parametrize("fe", [None, 5])
def test_rel_edge_conv_wide(fe):
    from analysisgnn_amd.core_layers import RelEdgeConv
    ei = _graph()
    g = torch.Generator().manual_seed(260 + (fe or 0))
    torch.manual_seed(260 + (fe or 0))
    x = torch.randn(N, 260, generator=g)
    assert int(torch.unique(x, dim=0).shape[0]) == N               # no two notes share a feature row: |h_i - h_j| has no tie
    ef = torch.randn(ei.shape[1], fe, generator=g) if fe else None
    m = RelEdgeConv(260, 40, in_edge_features=fe)
    n_par = _check_layer(m, lambda P, x, ei, ef: R.rel_edge_conv(P, "", x, ei, ef), [x, ei, ef], f"RelEdgeConv(260, 40, {fe})")
    assert n_par == 6


def test_gat_conv_wide():
    from analysisgnn_amd.core_layers import GATConvLayer
    ei = _graph()
    g = torch.Generator().manual_seed(250)
    torch.manual_seed(250)
    x = torch.randn(N, 64, generator=g)
    m = GATConvLayer(64, 250, num_heads=3, dropout=0.0)
    n_par = _check_layer(m, lambda P, x, ei: R.gat_conv(P, "", x, ei, num_heads=3), [x, ei], "GATConvLayer(64, 250, 3)")
    assert n_par >= 2                                              # linear.weight / linear.bias carry the whole gradient


@pytest.mark.parametrize("H,mean,shared", [(12, True, True), (12, False, False), (256, True, False), (256, False, True)])
def test_aggregate_with_edge_weights_matches_the_dense_formula(H, mean, shared):
    """ops.aggregate(edge_weight=...) over two relations (the chord plus ring graph, and a sparse random one): forward and the
    source gradient against out_r = A_r x (/ number of edges of the row), A_r[i, j] = sum of the weights of the edges (i, j),
    in float64.  The backward multiplies the weights by the 1 / count column scale of the forward."""
    from analysisgnn_amd import ops
    from analysisgnn_amd.graph import SegSpec, build_csr
    g = torch.Generator().manual_seed(H)
    eis = [_graph(), torch.randint(0, N, (2, 300), generator=g)]
    ws = [torch.randn(e.shape[1], generator=g) for e in eis]
    ws[0][::7] = 0.0
    specs = []
    for e in eis:
        specs += [SegSpec(e[0].to(DEV), e[1].to(DEV), n_rows=N), SegSpec(e[1].to(DEV), e[0].to(DEV), n_rows=N)]
    csrs = build_csr(specs)
    spec = ops.AggSpec(fwd=csrs[0::2], bwd=csrs[1::2], src_id=[0, 0], n_rows=N, mean=mean, shared_slot=shared,
                       edge_weight=[w.to(DEV) for w in ws])
    x0 = torch.randn(N, H, generator=g)
    go = torch.randn(N, H if shared else 2 * H, generator=g)

    def dense(x):
        outs = []
        for e, w in zip(eis, ws):
            a = torch.zeros(N, N, dtype=torch.float64).index_put_((e[0], e[1]), w.double(), accumulate=True)
            cnt = torch.bincount(e[0], minlength=N).clamp(min=1).double().unsqueeze(1)
            outs.append(a @ x / cnt if mean else a @ x)
        return sum(outs) if shared else torch.cat(outs, dim=1)

    xr = x0.double().requires_grad_(True)
    ref = dense(xr)
    ref.backward(go.double())
    xa = x0.to(DEV).requires_grad_(True)
    out = ops.aggregate(spec, [xa])
    assert_close_rel(out, ref, TOL, "forward")
    out.backward(go.to(DEV))
    assert_close_rel(xa.grad, xr.grad, TOL, "d src")
