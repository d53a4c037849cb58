"""`PreEncoder`, `pretrain_objective` and `PretrainMetrics` (analysisgnn_amd/pretrain.py) on the HIP path: against the fixtures of the
reference's own `PreEncoder` source (tests/gen_golden_pretrain.py) from the embedding on, and end to end against
oracle.encoders_ref.hybrid_hgt + tests/pretrain_ref.py in float64 on the same parameters.  fp32, tolerance 1e-4 relative."""
import functools

import numpy as np
import pytest
import torch

import pretrain_ref as R
from helpers import assert_close_rel, assert_grads_close_or_relu_flips
from test_pretrain_ref import CASES, by_pair, golden_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4
NOTE_RELS = [("note", r, "note") for r in ("onset", "consecutive", "during", "rest")]


@pytest.mark.parametrize("name", CASES)
def test_heads_and_objective_from_the_golden_embedding(name):
    """The stand-in encoder of the fixture is replaced by its output: the golden embedding x goes to the heads."""
    from analysisgnn_amd.heads import multitask_cross_entropy
    from analysisgnn_amd.pretrain import CLS_OFFS, PreEncoder, link_candidates, link_plans
    z, P, _, ei, bs, ks, ps = golden_case(name)
    H = int(z["meta.cfg"][2])
    m = PreEncoder((["note"], NOTE_RELS), 12, H, 2, heads=2, dropout=0.0)
    res = m.load_state_dict({k: v.detach().float() for k, v in P.items()}, strict=False)
    assert not res.unexpected_keys and all(k.startswith("encoder.") for k in res.missing_keys)
    m = m.to(DEV).train()
    x = torch.from_numpy(np.asarray(z["in.x"])).float().to(DEV).requires_grad_(True)
    eid = {k: v.to(DEV) for k, v in ei.items()}
    staff_c, voice_c = link_candidates(eid)
    plans = link_plans([(staff_c, eid[R.STAFF]), (voice_c, eid[R.VOICE])], bs, bs)
    staff_l, voice_l, fifths_l, spelling_l = m.decode(x, plans=plans)
    for task, cand, got in (("staff", staff_c, staff_l), ("voice", voice_c, voice_l)):
        ref = by_pair(z[f"out.{task}_candidates"], z[f"out.{task}_logits"])
        ref_y = by_pair(z[f"out.{task}_candidates"], z[f"out.{task}_labels"])
        k = ("staff", "voice").index(task)
        c = cand.cpu().numpy()
        alive = (c[0] < bs) & (c[1] < bs)
        assert int(alive.sum()) == len(ref) == int(m.last["counts"][k, 0])
        g = by_pair(c[:, alive], got.detach().cpu().numpy()[alive])
        gy = by_pair(c[:, alive], m.last["labels"][k].cpu().numpy()[alive])
        scale = max(abs(v) for v in ref.values())
        assert max(abs(g[p] - ref[p]) for p in ref) <= TOL * scale, task
        assert all(bool(gy[p]) == bool(ref_y[p]) for p in ref), task
        assert float(got.detach().cpu()[torch.from_numpy(~alive)].abs().sum()) == 0.0
        pos = np.array([ref[p] > 0 for p in ref]), np.array([bool(ref_y[p]) for p in ref])
        conf = [int((pos[0] & pos[1]).sum()), int((pos[0] & ~pos[1]).sum()), int((~pos[0] & pos[1]).sum()), int((~pos[0] & ~pos[1]).sum())]
        assert m.last["counts"][k, 1:].cpu().tolist() == conf, task
    assert_close_rel(fifths_l, z["out.fifths_logits"], TOL, "fifths logits")
    assert_close_rel(spelling_l, z["out.spelling_logits"], TOL, "spelling logits")
    labels = torch.stack([ks[:bs], ps[:bs]]).to(DEV)
    ce = multitask_cross_entropy(m.last["cls_logits"], CLS_OFFS, labels, 0.1, -1)
    parts = torch.stack([m.last["link_loss"][0], m.last["link_loss"][1], ce[0], ce[1]])
    assert_close_rel(parts, z["loss.parts"], TOL, "losses")
    total = parts.sum()
    assert abs(float(total.detach()) - float(z["loss.total"])) <= TOL * abs(float(z["loss.total"]))
    total.backward()
    assert_close_rel(x.grad, z["grad.x"], TOL, "grad x")
    n = 0
    for k, p in m.named_parameters():
        if not k.startswith("encoder."):
            assert p.grad is not None, k
            assert_close_rel(p.grad, z["gw." + k], TOL, f"grad {k}")
            n += 1
    assert n == 24


def hop_layout(g, bs, n_last):
    """A neighbour-sampling layout for a whole graph: the first `bs` notes are the targets, the last `n_last` notes the deepest hop;
    every relation's edges that touch one of those come last (the per-hop counts PyG's trim_to_layer reads)."""
    n = g.num_nodes["note"]
    first_last = n - n_last
    nodes = {t: [k, 0, 0] for t, k in g.num_nodes.items()}
    nodes["note"] = [bs, first_last - bs, n_last]
    edges = {}
    for et, e in list(g.edge_index.items()):
        late = np.zeros(e.shape[1], dtype=bool)
        if et[0] == "note":
            late |= e[0] >= first_last
        if et[2] == "note":
            late |= e[1] >= first_last
        order = np.concatenate([np.nonzero(~late)[0], np.nonzero(late)[0]])
        g.edge_index[et] = np.ascontiguousarray(e[:, order])
        edges[et] = [int((~late).sum()), int(late.sum())]
    g.num_sampled_nodes, g.num_sampled_edges, g.batch_size = nodes, edges, bs
    return g


@functools.lru_cache(maxsize=None)
def end_to_end_case(masks: bool, seed: int = 22):
    """(model on the device, inputs on the CPU, float64 reference dict with its tape) — computed once per setting."""
    from analysisgnn_amd.pretrain import PreEncoder
    from analysisgnn_amd.synth import add_staff_voice, make_score_graph, torch_inputs
    from oracle import encoders_ref as E
    from oracle.testing import ReluTap
    H, L, heads = 64, 2, 4
    g = add_staff_voice(make_score_graph(seed=seed, n_notes=60, add_beats=True, add_measures=True), seed=seed + 1)
    if masks:
        g = hop_layout(g, 40, 8)
    md = (g.node_types, [et for et in g.edge_types if et not in (R.STAFF, R.VOICE)])
    torch.manual_seed(seed)
    m = PreEncoder(md, H, H, L, heads=heads, dropout=0.0, jk=not masks).train()
    with torch.no_grad():
        gen = torch.Generator().manual_seed(seed + 2)
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=gen) * 0.1)
    P = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items() if v.is_floating_point()}
    I = torch_inputs(g, in_channels=H, seed=seed + 3)
    bs = I["batch_size"]
    x64 = {k: v.double().requires_grad_(k == "note") for k, v in I["x_dict"].items()}
    seen = {et: e for et, e in I["edge_index_dict"].items() if et not in (R.STAFF, R.VOICE)}
    with ReluTap(keep_graph=True) as tap:
        x = E.hybrid_hgt(P, "encoder.", md, L, heads, x64, seen, I["batch_dict"], bs, I["neighbor_mask_node"], I["neighbor_mask_edge"],
                         use_jk=not masks)
        ref = R.common_step(P, x, I["edge_index_dict"], bs, I["key_signature"], I["pitch_spelling"])
    for task in ("staff", "voice"):
        assert float(ref[f"{task}_logits"].detach().abs().min()) > 1e-4 and bool(ref[f"{task}_labels"].any())
    return m.to(DEV), I, dict(ref, x_note=x64["note"], P=P, tap=tap, bs=bs)


def to_dev(I):
    return ({k: v.to(DEV) for k, v in I["x_dict"].items()}, {k: v.to(DEV) for k, v in I["edge_index_dict"].items()},
            {k: v.to(DEV) for k, v in I["batch_dict"].items()})


@pytest.mark.parametrize("masks", [False, True])
def test_objective_end_to_end(masks):
    from analysisgnn_amd.pretrain import pretrain_objective
    m, I, ref = end_to_end_case(masks)
    bs = ref["bs"]
    if masks:
        assert bs == 40 and int((ref["staff_candidates"].shape[1])) < I["edge_index_dict"][R.ONSET].shape[1] + I["edge_index_dict"][R.CONSECUTIVE].shape[1]
    xg, eg, bg = to_dev(I)
    xg["note"].requires_grad_(True)
    m.zero_grad(set_to_none=True)
    total, parts = pretrain_objective(m, xg, eg, bg, bs, I["neighbor_mask_node"], I["neighbor_mask_edge"], I["key_signature"].to(DEV),
                                      I["pitch_spelling"].to(DEV))
    for k in ("staff", "voice", "fifths", "spelling"):
        print(f"[masks={masks}] {k}: hip {float(parts[k]):.7f} float64 {float(ref[k]):.7f}")
        assert abs(float(parts[k]) - float(ref[k])) <= TOL * abs(float(ref[k])), k
    assert abs(float(total) - float(ref["total"])) <= TOL * abs(float(ref["total"]))
    assert parts["alive"].cpu().tolist() == [ref["staff_candidates"].shape[1], ref["voice_candidates"].shape[1]]
    total.backward()
    torch.cuda.synchronize()
    names = [k for k, _ in m.named_parameters()]
    plist = [ref["P"][k] for k in names] + [ref["x_note"]]
    hip = [p.grad.detach().cpu().double() if p.grad is not None else None for _, p in m.named_parameters()] + [xg["note"].grad.cpu().double()]
    assert sum(h is not None for h in hip) > 40
    assert_grads_close_or_relu_flips(names + ["x_note"], hip, ref["tap"], ref["total"], plist, tol=TOL, label=f"pretrain masks={masks}")


def test_encoder_never_sees_the_true_relations_and_the_dict_is_left_alone():
    from analysisgnn_amd.pretrain import pretrain_objective
    m, I, ref = end_to_end_case(False)
    xg, eg, bg = to_dev(I)
    before = dict(eg)
    seen = []
    inner = m.encoder.forward

    def spy(x_dict, edge_index_dict, *a, **k):
        seen.append(set(edge_index_dict.keys()))
        return inner(x_dict, edge_index_dict, *a, **k)
    m.encoder.forward = spy
    try:
        with torch.no_grad():
            pretrain_objective(m, xg, eg, bg, ref["bs"], None, None, I["key_signature"].to(DEV), I["pitch_spelling"].to(DEV))
    finally:
        del m.encoder.forward
    assert len(seen) == 1 and R.STAFF not in seen[0] and R.VOICE not in seen[0] and R.ONSET in seen[0]
    assert seen[0] == set(before) - {R.STAFF, R.VOICE}
    assert list(eg.keys()) == list(before.keys()) and all(eg[k] is before[k] for k in before)


def test_metrics_over_two_batches():
    """F1 of the link tasks and accuracy of the class tasks, accumulated on the device over two batches, against the figures of the
    float64 predictions."""
    from analysisgnn_amd.pretrain import PretrainMetrics, pretrain_objective
    met = PretrainMetrics(DEV)
    conf = {"staff": [0] * 5, "voice": [0] * 5}
    hit = {"fifths": [0, 0], "spelling": [0, 0]}
    for masks in (False, True):
        m, I, ref = end_to_end_case(masks)
        xg, eg, bg = to_dev(I)
        with torch.no_grad():
            pretrain_objective(m, xg, eg, bg, ref["bs"], I["neighbor_mask_node"], I["neighbor_mask_edge"], I["key_signature"].to(DEV),
                               I["pitch_spelling"].to(DEV))
        met.update(m.last)
        for task in conf:
            l, y = ref[f"{task}_logits"].detach(), ref[f"{task}_labels"]
            conf[task] = [a + b for a, b in zip(conf[task], R.confusion(l, y, torch.ones_like(y)))]
        for task, lab in (("fifths", I["key_signature"]), ("spelling", I["pitch_spelling"])):
            top = ref[f"{task}_logits"].detach().sort(dim=1, descending=True).values
            assert float((top[:, 0] - top[:, 1]).min()) > 1e-4                      # no argmax of the fp32 path hangs on rounding
            hit[task][0] += int((ref[f"{task}_logits"].argmax(1) == lab[:ref["bs"]]).sum())
            hit[task][1] += ref["bs"]
    out = met.compute()
    assert met.link.cpu().tolist() == [conf["staff"], conf["voice"]]
    assert out["staff_f1"] == R.binary_f1(*conf["staff"][1:4]) and out["voice_f1"] == R.binary_f1(*conf["voice"][1:4])
    assert 0.0 < out["staff_f1"] <= 1.0
    assert out["fifths_acc"] == hit["fifths"][0] / hit["fifths"][1] and out["spelling_acc"] == hit["spelling"][0] / hit["spelling"][1]
    met.reset()
    assert met.compute()["staff_f1"] == 0.0
