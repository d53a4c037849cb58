"""The float64 restatement of the edge-consistency term (tests/edge_ref.py) against fixtures produced by the reference's own
`EdgeDecoder` source (tests/gen_golden_edge.py): logits, edge labels, losses and all gradients to 1e-12; and the module that
carries the reference's parameters (`analysisgnn_amd.EdgeDecoder`): its state_dict keys, deepcopy, load_state_dict."""
import copy

import numpy as np
import pytest
import torch

import edge_ref as R
from helpers import load_golden

CASES = ["edge_h8_whole", "edge_h16_targets"]


def golden_case(name):
    """(npz, relation names, P float64 leaf tensors, x float64 leaf, labels int64 [5, N], kept {relation: (src, dst)}, batch_size)"""
    z = load_golden(name)
    rels = [str(r) for r in z["meta.relations"]]
    P = {k[2:]: torch.from_numpy(np.asarray(z[k])).double().requires_grad_(True) for k in z.files if k.startswith("w.")}
    x = torch.from_numpy(np.asarray(z["in.x"])).double().requires_grad_(True)
    labels = torch.from_numpy(np.asarray(z["in.labels"])).long()
    kept = {r: tuple(torch.from_numpy(np.asarray(z["kept." + r])).long()) for r in rels}
    return z, rels, P, x, labels, kept, int(z["meta.cfg"][1])


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    z, rels, P, x, labels, kept, bs = golden_case(name)
    out = R.edge_term(P, x, kept, labels)
    for r in rels:
        assert np.abs(out["logits"][r].detach().numpy() - z["out.logits." + r]).max() <= 1e-12, r
        assert np.array_equal(out["labels"][r].numpy().astype(np.uint8), z["out.labels." + r]), r
    parts = np.array([out["losses"][r].item() for r in rels])
    assert np.abs(parts - z["loss.parts"]).max() <= 1e-12
    assert abs(out["total"].item() - float(z["loss.total"])) <= 1e-12
    out["total"].backward()
    assert np.abs(x.grad.numpy() - z["grad.x"]).max() <= 1e-12
    assert len(P) == 22 and all("gw." + k in z.files for k in P)
    for k, p in P.items():
        assert np.abs(p.grad.numpy() - z["gw." + k]).max() <= 1e-12, k


@pytest.mark.parametrize("name", CASES)
def test_kernel_layout_agrees_with_the_step(name):
    """`pair_features` over ALL edges of a relation with everything but the kept ones folded out of range (the plan's layout)
    gives the kept edges' features, zero rows elsewhere; the kept edges are alive, distinct, and as many as :994-997 keep."""
    z, rels, P, x, labels, kept, bs = golden_case(name)
    capped = 0
    for i, r in enumerate(rels):
        s, d = kept[r]
        alive = int(z["meta.alive"][i])
        assert s.numel() == min(alive, bs) and bool(R.alive_mask(s, d, bs).all())
        assert len({(int(a), int(b)) for a, b in zip(s, d)}) == s.numel()
        capped += alive > bs
        a = R.embed(P, r, x).detach()
        pad = torch.full((3,), bs, dtype=torch.int64)
        f = R.pair_features(a, torch.cat([s, pad]), torch.cat([d, pad]), bs)
        assert torch.equal(f[:-3], a[s] * a[d]) and float(f[-3:].abs().max()) == 0.0
        y = torch.from_numpy(np.asarray(z["out.labels." + r])).bool()
        assert 0 < int(y.sum()) < y.numel()                                   # both classes in every relation
    assert 0 < capped < len(rels)                                             # both branches of :994


def test_golden_margins_hold():
    """What the generator asserts: no edge's logits within 1e-4 of each other (confusion counts are compared exactly on the GPU),
    no ReLU input at its kink."""
    for name in CASES:
        z = load_golden(name)
        assert float(z["meta.logit_margin"]) > 1e-4 and float(z["meta.relu_margin"]) > 3e-6


def test_edge_labels_treat_equal_minus_ones_as_equal():
    labels = torch.tensor([[0, 0, 1, -1, -1], [2, 2, 2, 2, 2]])
    s, d = torch.tensor([0, 0, 3, 3, 2]), torch.tensor([1, 2, 4, 0, 2])
    assert R.edge_labels(labels, s, d).tolist() == [1, 0, 1, 0, 1]


def test_edge_decoder_state_dict_is_the_reference_s():
    from analysisgnn_amd import EdgeDecoder
    for name in CASES:
        z = load_golden(name)
        H, rels = int(z["meta.cfg"][2]), [str(r) for r in z["meta.relations"]]
        m = EdgeDecoder(H, rels, dropout=0.5)
        sd = m.state_dict()
        assert sorted(sd.keys()) == [str(k) for k in z["meta.keys"]] and len(sd) == 22
        assert m.relations == rels
        for k in sd:
            assert tuple(sd[k].shape) == tuple(z["w." + k].shape), k
        res = m.load_state_dict({k[2:]: torch.from_numpy(np.asarray(z[k])).float() for k in z.files if k.startswith("w.")}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys


def test_edge_decoder_deepcopy_drops_the_last_call():
    from analysisgnn_amd import EdgeDecoder
    torch.manual_seed(0)
    a = EdgeDecoder(16, ["onset", "rest"], dropout=0.3)
    a.last = {"anything": torch.ones(2, requires_grad=True) * 2}              # a call's leftovers are not state
    b = copy.deepcopy(a)
    assert b.last == {} and "last" not in "".join(a.state_dict().keys())
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) and sa[k].data_ptr() != sb[k].data_ptr() for k in sa)
    assert b.embed["onset"][3].p == 0.3 and b.fc[3].p == 0.3


def test_python_layer_refuses_what_the_kernels_do_not_serve():
    from analysisgnn_amd import EdgeDecoder, edge_plan
    from analysisgnn_amd._lib import AgnnError
    e = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(AgnnError):
        edge_plan({("note", "onset", "note"): e}, 4)                          # CPU tensors: no fall-back
    with pytest.raises(AgnnError):
        edge_plan({("note", "onset", "beat"): e}, 4)                          # no note-note relation
    with pytest.raises(AgnnError):
        edge_plan({("note", "onset", "note"): e.int()}, 4)
    m = EdgeDecoder(8, ["onset"])
    with pytest.raises(ValueError, match="not found in embed dictionary"):    # the reference's own error (:829-830)
        m({("note", "rest", "note"): (e[0], e[1])}, torch.zeros(4, 8))
