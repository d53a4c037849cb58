"""The float64 restatement of the pretraining stage (tests/pretrain_ref.py) against fixtures produced by the reference's own
`PreEncoder` / `isin_pairwise` source (tests/gen_golden_pretrain.py): logits, labels and losses to 1e-12; and the module that
carries the reference's parameters (`analysisgnn_amd.pretrain.PreEncoder`): its state_dict keys, deepcopy, load_state_dict."""
import copy

import numpy as np
import pytest
import torch

import pretrain_ref as R
from helpers import load_golden

CASES = ["pretrain_h8_whole", "pretrain_h16_targets"]


def golden_case(name):
    """(npz, P float64 leaf tensors, x float64 leaf, edge_index_dict int64, batch_size, key_signature, pitch_spelling)"""
    z = load_golden(name)
    P = {k[2:]: torch.from_numpy(np.asarray(z[k])).double().requires_grad_(True) for k in z.files if k.startswith("w.")}
    x = torch.from_numpy(np.asarray(z["in.x"])).double().requires_grad_(True)
    ei = {("note", r, "note"): torch.from_numpy(np.asarray(z["edges." + r])).long() for r in ("onset", "consecutive", "staff", "voice")}
    return z, P, x, ei, int(z["meta.cfg"][1]), torch.from_numpy(np.asarray(z["in.key_signature"])).long(), \
        torch.from_numpy(np.asarray(z["in.pitch_spelling"])).long()


def by_pair(cand, values):
    """{(s, d): value}: the candidates of these graphs are distinct pairs, so logits and labels can be matched whatever the order."""
    c = np.asarray(cand)
    out = {(int(s), int(d)): v for s, d, v in zip(c[0], c[1], np.asarray(values))}
    assert len(out) == c.shape[1]
    return out


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    z, P, x, ei, bs, ks, ps = golden_case(name)
    before = {k: v.clone() for k, v in ei.items()}
    out = R.common_step(P, x, ei, bs, ks, ps)
    assert set(ei) == set(before) and all(torch.equal(ei[k], before[k]) for k in ei)
    for task in ("staff", "voice"):
        # the argsort of :707 is not stable: compare per candidate pair
        ref_l, ref_y = by_pair(z[f"out.{task}_candidates"], z[f"out.{task}_logits"]), by_pair(z[f"out.{task}_candidates"], z[f"out.{task}_labels"])
        got_l = by_pair(out[f"{task}_candidates"], out[f"{task}_logits"].detach())
        got_y = by_pair(out[f"{task}_candidates"], out[f"{task}_labels"])
        assert set(got_l) == set(ref_l)
        assert max(abs(got_l[k] - ref_l[k]) for k in ref_l) <= 1e-12
        assert all(bool(got_y[k]) == bool(ref_y[k]) for k in ref_y)
    assert np.abs(out["fifths_logits"].detach().numpy() - z["out.fifths_logits"]).max() <= 1e-12
    assert np.abs(out["spelling_logits"].detach().numpy() - z["out.spelling_logits"]).max() <= 1e-12
    parts = np.array([out[k].item() for k in ("staff", "voice", "fifths", "spelling")])
    assert np.abs(parts - z["loss.parts"]).max() <= 1e-12
    assert abs(out["total"].item() - float(z["loss.total"])) <= 1e-12
    # without the sort the losses are the same sums in another order
    unsorted = R.common_step(P, x, ei, bs, ks, ps, sort=False)
    assert abs(unsorted["total"].item() - float(z["loss.total"])) <= 1e-12
    out["total"].backward()
    assert np.abs(x.grad.numpy() - z["grad.x"]).max() <= 1e-12
    for k, p in P.items():
        if "gw." + k in z.files:
            assert np.abs(p.grad.numpy() - z["gw." + k]).max() <= 1e-12, k


@pytest.mark.parametrize("name", CASES)
def test_link_task_layout_agrees_with_the_step(name):
    """`link_task` (one entry per candidate, alive or not — the kernels' layout) gives the step's link losses and labels."""
    z, P, x, ei, bs, ks, ps = golden_case(name)
    with torch.no_grad():
        for i, (task, cand) in enumerate((("staff", torch.cat((ei[R.ONSET], ei[R.CONSECUTIVE]), dim=1)), ("voice", ei[R.CONSECUTIVE]))):
            feat = R.head(P, f"{task}_clf", x)
            logits, labels, alive, loss = R.link_task(feat, cand, ei[("note", task, "note")], bs)
            assert abs(loss.item() - float(z["loss.parts"][i])) <= 1e-12
            assert int(alive.sum()) == z[f"out.{task}_candidates"].shape[1]
            ref_y = by_pair(z[f"out.{task}_candidates"], z[f"out.{task}_labels"])
            got = by_pair(cand[:, alive], labels[alive])
            assert got.keys() == ref_y.keys() and all(bool(got[k]) == bool(ref_y[k]) for k in got)
            assert float(logits[~alive].abs().sum()) == 0.0 and not bool(labels[~alive].any())
    if name == "pretrain_h16_targets":
        assert int((~alive).sum()) > 0


def test_golden_margins_hold():
    """What the generator asserts: no alive candidate within 1e-4 of zero (confusion counts are compared exactly on the GPU), no
    ReLU input at its kink."""
    for name in CASES:
        z = load_golden(name)
        assert float(z["meta.zero_margin"]) > 1e-4 and float(z["meta.relu_margin"]) > 3e-6


def _metadata():
    return (["note"], [("note", r, "note") for r in ("onset", "consecutive", "during", "rest")])


def test_preencoder_state_dict_is_the_reference_s():
    from analysisgnn_amd import PreEncoder
    from analysisgnn_amd.hgt import HybridHGT
    z = load_golden(CASES[0])
    H = int(z["meta.cfg"][2])
    m = PreEncoder(_metadata(), 12, H, 2, heads=2, dropout=0.0)
    keys = set(m.state_dict().keys())
    ref = {str(k) for k in z["meta.keys"]}
    # the heads' keys are the reference's own; under `encoder.` the fixture holds its stand-in, the module the build's HybridHGT
    assert {k for k in keys if not k.startswith("encoder.")} == {k for k in ref if not k.startswith("encoder.")}
    enc = HybridHGT(_metadata(), 12, H, 2, heads=2, dropout=0.0, use_jk=True)
    assert {k for k in keys if k.startswith("encoder.")} == {"encoder." + k for k in enc.state_dict().keys()}
    for k in ref:
        if not k.startswith("encoder."):
            assert tuple(m.state_dict()[k].shape) == tuple(z["w." + k].shape), k
    assert any(k.startswith("encoder.jk.") for k in keys)                  # jk=True is the reference's default
    assert not any(k.startswith("encoder.jk.") for k in PreEncoder(_metadata(), 12, H, 2, heads=2, jk=False).state_dict())


def test_preencoder_deepcopy_and_load_state_dict_round_trip():
    from analysisgnn_amd import PreEncoder
    torch.manual_seed(0)
    a = PreEncoder(_metadata(), 12, 16, 2, heads=2, dropout=0.0)
    a.last = {"anything": torch.ones(2, requires_grad=True) * 2}              # a call's leftovers are not state
    b = copy.deepcopy(a)
    assert b.last == {}
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) and sa[k].data_ptr() != sb[k].data_ptr() for k in sa)
    torch.manual_seed(1)
    c = PreEncoder(_metadata(), 12, 16, 2, heads=2, dropout=0.0)
    assert any(not torch.equal(c.state_dict()[k], sa[k]) for k in sa)
    missing, unexpected = c.load_state_dict(sa, strict=True)
    assert not missing and not unexpected
    assert all(torch.equal(c.state_dict()[k], sa[k]) for k in sa)
    z = load_golden(CASES[1])                                                 # the reference's head weights load by name
    d = PreEncoder(_metadata(), 12, 16, 2, heads=2, dropout=0.0)
    res = d.load_state_dict({k[2:]: torch.from_numpy(np.asarray(z[k])).float() for k in z.files if k.startswith("w.")}, strict=False)
    assert not res.unexpected_keys and all(k.startswith("encoder.") for k in res.missing_keys)


def test_python_layer_refuses_what_the_kernels_do_not_serve():
    from analysisgnn_amd import link_bce, link_plan
    from analysisgnn_amd._lib import AgnnError
    cand = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(AgnnError):
        link_plan(cand, None, 4)                                              # CPU tensors: no fall-back
    with pytest.raises(AgnnError):
        link_bce([], [])
    with pytest.raises(AgnnError):
        link_plan(cand, None, 4, limit=5)                                     # limit beyond the rows


def test_synthetic_staff_and_voice_relations():
    from analysisgnn_amd.synth import add_staff_voice, make_batch
    g0 = make_batch(2, 60, first_seed=3, add_beats=True)
    g = add_staff_voice(g0, seed=5)
    assert ("note", "staff", "note") not in g0.edge_index and set(g0.edge_index) < set(g.edge_index)
    staff, voice, st = g.edge_index[("note", "staff", "note")], g.edge_index[("note", "voice", "note")], g.extras["staff"]
    assert staff.dtype == np.int64 and voice.dtype == np.int64 and voice.shape[1] > 0 and staff.shape[1] > 0
    cons = {(int(s), int(d)) for s, d in g.edge_index[("note", "consecutive", "note")].T}
    pool = cons | {(int(s), int(d)) for s, d in g.edge_index[("note", "onset", "note")].T}
    sp = [(int(s), int(d)) for s, d in staff.T]
    assert len(set(sp)) == len(sp) and set(sp) == {p for p in pool if st[p[0]] == st[p[1]]}
    vp = [(int(s), int(d)) for s, d in voice.T]
    assert set(vp) <= cons and len(set(voice[0])) == len(vp) and len(set(voice[1])) == len(vp)      # chains
    assert all(st[s] == st[d] for s, d in vp)
    again = add_staff_voice(g0, seed=5)
    assert np.array_equal(again.edge_index[("note", "voice", "note")], voice) and np.array_equal(again.extras["pitch"], g.extras["pitch"])
    assert not np.array_equal(add_staff_voice(g0, seed=6).extras["pitch"], g.extras["pitch"])
