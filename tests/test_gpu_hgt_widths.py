"""HGTConv at the head widths the layer tests of test_gpu_hgt.py leave out (D = 16, 32, 128: hidden sizes 64, 128 and 512 at
the reference's heads = 4) against the CPU restatement of PyG HGTConv (oracle/pyg_ref.py): forward, input gradients and every
parameter gradient, on the small C3-type graph and on the one with reversed metrical edges.  Tolerance: the one of
`test_hgt_conv_layer` (1e-4 relative to max(1, |ref|max))."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import assert_close  # noqa: E402

TOL = 1e-4
DEV = "cuda:0"


def _graph(kind):
    from analysisgnn_amd.synth import make_batch
    if kind == "c3":      # note + beat + measure, 4 note-note relations + note->beat + note->measure (C3 layout)
        return make_batch(2, 60, first_seed=7, add_beats=True, add_measures=True)
    if kind == "metrical_rev":
        return make_batch(2, 60, first_seed=9, add_beats=True, add_measures=True, reverse_metrical_edges=True)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["c3", "metrical_rev"])
@pytest.mark.parametrize("C,heads", [(64, 4), (128, 4), (512, 4)])
def test_hgt_conv_layer_widths(kind, C, heads):
    from analysisgnn_amd.hgt import HGTConv
    from analysisgnn_amd.synth import torch_inputs
    from oracle import pyg_ref as G
    g = _graph(kind)
    md = g.metadata()
    torch.manual_seed(C + heads)
    m = HGTConv(C, C, md, heads)
    with torch.no_grad():
        for p in m.p_rel.values():
            p.uniform_(0.5, 1.5)
        for p in m.skip.values():
            p.uniform_(-1, 1)
    P = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    m = m.to(DEV)
    I = torch_inputs(g, in_channels=C, seed=5)
    xc = {k: v.clone().requires_grad_(True) for k, v in I["x_dict"].items()}
    ref = G.hgt_conv(P, "", md[0], md[1], heads, xc, I["edge_index_dict"])
    xg = {k: v.to(DEV).requires_grad_(True) for k, v in I["x_dict"].items()}
    out = m(xg, {k: v.to(DEV) for k, v in I["edge_index_dict"].items()})
    assert set(out) == set(ref)
    gen = torch.Generator().manual_seed(3)
    lr = lg = 0
    for t in ref:
        assert_close(out[t], ref[t], TOL, f"out[{t}]")
        go = torch.randn(ref[t].shape, generator=gen)
        lr = lr + (ref[t] * go).sum()
        lg = lg + (out[t] * go.to(DEV)).sum()
    lr.backward()
    lg.backward()
    for t in xc:
        assert_close(xg[t].grad, xc[t].grad, TOL, f"grad x[{t}]")
    n = 0
    for name, p in m.named_parameters():
        if P[name].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, f"{name}: no gradient on the HIP path"
        assert_close(p.grad, P[name].grad, TOL, f"grad {name}")
        n += 1
    assert n > 0
