"""Float64 check of oracle/intree_ref.py against the reference's own in-tree layers.

The reference's MetricalGNN / HGCN were run in float64 on the inputs and weights of the float32 fixtures
(oracle/gen_golden_f64.py, loading core/gnn.py + core/hgnn.py as oracle/gen_golden.py does); their outputs and
gradients are stored in tests/golden/f64_*.npz.  In float64, rounding noise (fp32 BatchNorm backward) cannot mask a
semantic difference.
"""
import numpy as np
import pytest
import torch

from helpers import load_golden


@pytest.fixture()
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)   # as the reference run was made
    yield
    torch.set_default_dtype(old)


def _max_diff(a, ref):
    return float((a.detach() - torch.from_numpy(np.asarray(ref))).abs().max())


@pytest.mark.parametrize("tag", ["eq", "ragged"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_metrical_gnn_f64(f64, tag, mode):
    from oracle import intree_ref as R
    z = load_golden(f"metrical_{tag}_{mode}")
    ref = load_golden(f"f64_metrical_{tag}_{mode}")
    rels = [str(r) for r in z["meta.rels"]]
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}
    I = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
    g = torch.from_numpy(z["gout"]).double()
    P = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    x2 = I["x"].double().requires_grad_(True)
    o2 = R.metrical_gnn(P, rels, 3, x2, I["edge_index"], I["edge_type"], I["beat_nodes"].numel(),
                        I["measure_nodes"].numel(), I["beat_edges"], I["measure_edges"],
                        I.get("beat_lengths"), I.get("measure_lengths"), training=(mode == "train"))
    (o2 * g).sum().backward()
    assert _max_diff(o2, ref["out"]) < 1e-10
    assert _max_diff(x2.grad, ref["gx"]) < 1e-10
    names = [k[2:] for k in ref.files if k.startswith("g.")]
    assert names, "no parameter gradients in the fixture"
    for n in names:
        assert _max_diff(P[n].grad, ref["g." + n]) < 1e-9, n


def test_hgcn_f64(f64):
    from oracle import intree_ref as R
    z = load_golden("hgcn3_jk")
    ref = load_golden("f64_hgcn3_jk")
    rels = [str(r) for r in z["meta.rels"]]
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}
    I = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
    P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x2 = I["x"].double().requires_grad_(True)
    o2 = R.hgcn(P, rels, 3, x2, I["edge_index"], I["edge_type"], jk=True)
    o2.sum().backward()
    assert _max_diff(o2, ref["out"]) < 1e-11
    assert _max_diff(x2.grad, ref["gx"]) < 1e-10
