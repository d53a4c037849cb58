"""The graph-transformer modules (core_layers.GPSLayer / HGPSLayer / HGPS) without a GPU: they construct, carry the reference's
`state_dict` keys in the reference's order (the `p.*` names of the reference-run fixtures, scripts/gen_golden_gps.py), load the
reference's weights strictly, and refuse CPU tensors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import load_golden

ETYPES4 = {"onset": 0, "consecutive": 1, "during": 2, "rests": 3}
ETYPES2 = {"onset": 0, "consecutive": 1}


def build(name):
    from analysisgnn_amd import core_layers as cl
    return {
        "gps_hlayer_h32": lambda: cl.HGPSLayer(24, 32, 4, etypes=ETYPES4),
        "gps_hlayer_h64": lambda: cl.HGPSLayer(64, 64, 4, etypes=ETYPES2),
        "gps_layer_h32": lambda: cl.GPSLayer(32, 32, 4, F.relu),
        "gps_stack": lambda: cl.HGPS(24, 32, 32, 2, etypes=ETYPES2, jk=False),
        "gps_stack_jk": lambda: cl.HGPS(24, 32, 32, 2, etypes=ETYPES2, jk=True),
    }[name]()


FIXTURES = ["gps_hlayer_h32", "gps_hlayer_h64", "gps_layer_h32", "gps_stack", "gps_stack_jk"]


def fixture_state(z):
    return {k[2:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith("p.")}


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_matches_the_reference(name):
    z = load_golden(name)
    m = build(name)
    ref_keys = [k[2:] for k in z.files if k.startswith("p.")]
    assert list(m.state_dict().keys()) == ref_keys
    assert all(z["p." + k].dtype == np.float32 for k in ref_keys)
    m.load_state_dict(fixture_state(z), strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, torch.from_numpy(np.asarray(z["p." + k])))
    # every parameter has a recorded gradient, and the recorded worst fp32-vs-float64 figure of the reference is inside its bound
    assert sorted(k[2:] for k in z.files if k.startswith("g.")) == sorted(n for n, _ in m.named_parameters())
    assert 0.0 < float(z["meta.fp32_vs_f64"]) <= 1e-5


def test_hetero_layer_entries():
    m = build("gps_hlayer_h32")
    keys = list(m.state_dict().keys())
    assert len(keys) == 46                                       # 14 of the block + 4 relations x 4 projections x (weight, bias)
    assert keys[:2] == ["embedding.weight", "embedding.bias"]
    assert keys[10:14] == ["attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias"]
    assert keys[14] == "local.conv.onset.W1.weight"
    assert m.attn.in_proj_weight.shape == (96, 32) and m.attn.num_heads == 4


def test_defaults_follow_the_reference():
    from analysisgnn_amd import core_layers as cl
    s = cl.HGPS(24, 32, 32, 2, dropout=0.5)
    assert len(s.layers) == 3 and s.dropout.p == 0.5             # n_layers + 1 layers, all in the loop
    for layer in s.layers:                                       # the layers keep THEIR default, the attention dropout included
        assert layer.dropout_ff.p == layer.dropout_attn.p == layer.dropout_local.p == 0.2 and layer.attn.dropout == 0.2
        assert layer.num_heads == 4 and len(layer.local.conv) == 7 and layer.activation is F.relu
    assert [l.in_features for l in s.layers] == [24, 32, 32] and not s.use_knowledge
    j = cl.HGPS(24, 32, 32, 2, jk=True)
    assert j.use_knowledge and j.jk.lstm.input_size == 32 and j.jk.lstm.hidden_size == 32
    g = cl.GPSLayer(32, 32, 4, torch.tanh, dropout=0.1, bias=False)
    assert g.ff1.bias is None and g.attn.in_proj_bias is None and g.local.W1.bias is None and g.dropout_attn.p == 0.1
    assert not hasattr(g, "embedding") and isinstance(g.local, cl.ResGatedGraphConv)


def test_cpu_tensors_are_refused():
    from analysisgnn_amd import _lib
    ei = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(_lib.AgnnError):
        build("gps_hlayer_h32")(torch.zeros(5, 24), ei, torch.zeros(3, dtype=torch.long))
    with pytest.raises(_lib.AgnnError):
        build("gps_layer_h32")(torch.zeros(5, 32), ei)
    with pytest.raises(_lib.AgnnError):
        build("gps_stack")(torch.zeros(5, 24), ei, torch.zeros(3, dtype=torch.long))
