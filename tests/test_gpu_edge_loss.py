"""The edge-consistency term on the GPU (csrc/edgedec.hip through `analysisgnn_amd.edge_loss`) against the reference's fixtures
(tests/golden/edge_*.npz) and the float64 restatement tests/edge_ref.py.  Gate: every float tensor within 1e-4 of
the reference tensor's largest magnitude; edge labels, alive counts and confusion counts exact — the float64 logits of every
case keep 1e-4 apart (asserted; the seeds below were chosen on the CPU so that it holds)."""
import numpy as np
import pytest
import torch

import edge_ref as R
from helpers import assert_close_rel, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4
N, LIMIT = 40, 32


def et(r):
    return ("note", r, "note")


def rand_params(H, rels, seed):
    """float64 parameters under the reference's state_dict keys, LayerNorm affines and biases away from their initialisation."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    def lin(name, out, inp):
        P[name + ".weight"] = torch.randn(out, inp, generator=g, dtype=torch.float64) * inp ** -0.5
        P[name + ".bias"] = torch.randn(out, generator=g, dtype=torch.float64) * 0.1
    def ln(name):
        P[name + ".weight"] = 1 + torch.randn(H, generator=g, dtype=torch.float64) * 0.1
        P[name + ".bias"] = torch.randn(H, generator=g, dtype=torch.float64) * 0.1
    for r in rels:
        lin(f"embed.{r}.0", H, H)
        ln(f"embed.{r}.2")
    lin("fc.0", H, H)
    ln("fc.2")
    lin("fc.4", 2, H)
    return P


def seg_labels(n, seed, K=5):
    """Piecewise constant labels [K, n] with a few -1s: both edge classes occur."""
    g = torch.Generator().manual_seed(seed)
    seg = torch.arange(n) // 5
    lab = torch.stack([torch.randint(0, 2, (int(seg.max()) + 1,), generator=g)[seg // (1 + i % 2)] for i in range(K)])
    lab[3, 2:4] = -1
    return lab.long()


def random_edges(E, seed, n=N):
    return tuple(torch.randint(0, n, (2, E), generator=torch.Generator().manual_seed(seed)))


def reference_term(P, x, edges, labels, limit):
    """float64: edge_ref.edge_term on the alive edges of every relation -> (out, P leaves, x leaf, alive masks)."""
    P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    x = x.double().clone().requires_grad_(True)
    alive = {r: R.alive_mask(s, d, limit) for r, (s, d) in edges.items()}
    kept = {r: (s[alive[r]], d[alive[r]]) for r, (s, d) in edges.items()}
    out = R.edge_term(P, x, kept, labels)
    for r in kept:
        if kept[r][0].numel():
            z = out["logits"][r].detach()
            assert float((z[:, 1] - z[:, 0]).abs().min()) > 1e-4, "float64 logits within 1e-4 of each other: choose another seed"
    out["total"].backward()
    return out, P, x, alive


def hip_term(P, x, edges, labels, limit, rels=None, dropout=0.0, train=True):
    """The HIP path on the same operands -> (loss, parts, decoder, x leaf, plan)."""
    from analysisgnn_amd import EdgeDecoder, edge_consistency_loss, edge_plan
    rels = list(edges) if rels is None else rels
    H = P["fc.0.weight"].shape[0]
    dec = EdgeDecoder(H, rels, dropout=dropout)
    dec.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    dec.to(DEV).train(train)
    xd = x.float().to(DEV).requires_grad_(True)
    plan = edge_plan({et(r): (s.to(DEV), d.to(DEV)) for r, (s, d) in edges.items()}, limit, x.shape[0], select=False, relations=rels)
    loss, parts = edge_consistency_loss(dec, xd, plan, labels.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), parts, dec, xd, plan


def check_term(hip, ref, edges):
    loss, parts, dec, xd, plan = hip
    out, P64, x64, alive = ref
    last = dec.last
    assert parts["relations"] == list(edges)
    for i, r in enumerate(edges):
        a = alive[r]
        logits = last["logits"][i].detach().cpu()
        labels = last["labels"][i].cpu()
        assert logits.shape == (a.numel(), 2) and float(logits[~a].abs().sum()) == 0.0 and not bool(labels[~a].any()), r
        assert torch.equal(labels[a].long(), out["labels"][r]), f"{r}: edge labels"
        assert_close_rel(logits[a], out["logits"][r], TOL, f"{r}: logits")
        full = torch.zeros(a.numel(), 2, dtype=torch.float64).index_put((a.nonzero().reshape(-1),), out["logits"][r].detach())
        lab = torch.zeros(a.numel(), dtype=torch.long).index_put((a.nonzero().reshape(-1),), out["labels"][r])
        assert last["counts"][i].cpu().tolist() == R.confusion(full, lab, a), f"{r}: alive / confusion counts"
        assert int(parts["alive"][i]) == int(a.sum())
        assert_close_rel(parts["losses"][i], out["losses"][r], TOL, f"{r}: loss")
    assert_close_rel(loss, out["total"], TOL, "total")
    assert_close_rel(xd.grad, x64.grad, TOL, "x.grad")
    sd = dict(dec.named_parameters())
    assert set(sd) == set(P64)
    for k, p in P64.items():
        got = sd[k].grad
        if p.grad is None:                                 # a relation without an alive edge: its block gets zeros
            assert got is None or float(got.abs().max()) == 0.0, k
        else:
            assert got is not None, k
            assert_close_rel(got, p.grad, TOL, "grad " + k)


# ---- the reference's fixtures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_h8_whole", "edge_h16_targets"])
def test_golden(name):
    from analysisgnn_amd import EdgeDecoder, edge_consistency_loss, edge_plan
    z = load_golden(name)
    rels = [str(r) for r in z["meta.relations"]]
    bs, H = int(z["meta.cfg"][1]), int(z["meta.cfg"][2])
    dec = EdgeDecoder(H, rels, dropout=0.5)
    dec.load_state_dict({k[2:]: torch.from_numpy(np.asarray(z[k])).float() for k in z.files if k.startswith("w.")}, strict=True)
    dec.to(DEV).eval()                                                        # the fixture was made with dropout 0
    x = torch.from_numpy(np.asarray(z["in.x"])).float().to(DEV).requires_grad_(True)
    labels = torch.from_numpy(np.asarray(z["in.labels"])).long().to(DEV)
    kept = {et(r): torch.from_numpy(np.asarray(z["kept." + r])).long().to(DEV) for r in rels}
    plan = edge_plan(kept, bs, select=False, relations=dec.relations)         # the fixture's own draw: already selected
    loss, parts = edge_consistency_loss(dec, x, plan, labels)
    loss.backward()
    torch.cuda.synchronize()
    for i, r in enumerate(rels):
        assert_close_rel(dec.last["logits"][i], z["out.logits." + r], TOL, f"{r}: logits")
        assert np.array_equal(dec.last["labels"][i].cpu().numpy(), z["out.labels." + r]), f"{r}: edge labels"
        ref_logits, y = torch.from_numpy(z["out.logits." + r]), torch.from_numpy(z["out.labels." + r])
        assert dec.last["counts"][i].cpu().tolist() == R.confusion(ref_logits, y, torch.ones(len(y), dtype=torch.bool))
    assert_close_rel(parts["losses"], z["loss.parts"], TOL, "per-relation losses")
    assert parts["alive"].cpu().tolist() == [z["kept." + r].shape[1] for r in rels]
    assert_close_rel(loss, z["loss.total"], TOL, "total")
    assert_close_rel(x.grad, z["grad.x"], TOL, "x.grad")
    grads = {k: p.grad for k, p in dec.named_parameters()}
    assert len(grads) == 22
    for k, g in grads.items():
        assert g is not None, k
        assert_close_rel(g, z["gw." + k], TOL, "grad " + k)
    # the reference's forward signature: {edge_type: logits [E, 2]} from {edge_type: (src, dst)}
    with torch.no_grad():
        logit_dict = dec({k: (v[0], v[1]) for k, v in kept.items()}, x.detach())
    assert list(logit_dict) == [et(r) for r in rels]
    for r in rels:
        assert_close_rel(logit_dict[et(r)], z["out.logits." + r], TOL, f"{r}: forward()")
    with pytest.raises(ValueError, match="not found in embed dictionary"):
        dec({("note", "nonesuch", "note"): (kept[et(rels[0])][0], kept[et(rels[0])][1])}, x.detach())


# ---- the pair kernel alone ----------------------------------------------------------------------------------------------------
PAIR_N, PAIR_LIMIT = 14, 10


def pair_graph():
    """14 rows, limit 10.  Relation 0: a hub (node 0), the self loops (2, 2), (0, 0) and — beyond the limit — (12, 12), the edge
    (3, 4) listed twice and its reverse, ends at or above the limit, a negative id.  Node 9 (below the limit) and node 13 have no
    edge at all.  Relation 1 has no alive edge."""
    r0 = [(0, 1), (1, 0), (2, 2), (3, 4), (0, 5), (5, 0), (0, 6), (7, 8), (8, 10), (11, 3), (12, 12), (3, 4), (6, 7), (-1, 2), (0, 0), (4, 3)]
    r1 = [(10, 1), (2, 11), (12, 12)]
    def t(p):
        return tuple(torch.tensor(p, dtype=torch.int64).t().contiguous())
    return [t(r0), t(r1)]


def hip_pair(a, rel_edges, limit, labels=None, p=0.0, call_id=77, df=None):
    """`_EdgePair` on the stacked a [n, R H] (CPU) -> (F list per relation, edge labels per relation, dA or None)."""
    from analysisgnn_amd.edge_loss import _EdgePair, edge_plan
    plan = edge_plan({et(f"r{i}"): (s.to(DEV), d.to(DEV)) for i, (s, d) in enumerate(rel_edges)}, limit, a.shape[0], select=False)
    ad = a.float().to(DEV).requires_grad_(True)
    info = {}
    f = _EdgePair.apply(plan, info, ad, None if labels is None else labels.to(DEV), p, call_id)
    da = None
    if df is not None:
        f.backward(df.float().to(DEV))
        da = ad.grad.cpu()
    torch.cuda.synchronize()
    off = plan.e_off
    return ([f.detach()[off[i]:off[i + 1]].cpu() for i in range(len(rel_edges))],
            [info["edge_labels"][off[i]:off[i + 1]].cpu() for i in range(len(rel_edges))], da)


@pytest.mark.parametrize("H", [4, 8, 36, 128, 260])
def test_pair_kernel_at_every_lane_grouping(H):
    """4: one float4; 36: 9 column quads in a 16-lane group; 128: the trainer's width; 260: a second column pass."""
    rel = pair_graph()
    g = torch.Generator().manual_seed(100 + H)
    a = torch.randn(PAIR_N, 2 * H, generator=g, dtype=torch.float64)
    labels = seg_labels(PAIR_N, 5)
    E = sum(s.numel() for s, _ in rel)
    df = torch.randn(E, H, generator=g, dtype=torch.float64)
    f, y, da = hip_pair(a, rel, PAIR_LIMIT, labels, df=df)
    lo = 0
    for i, (s, d) in enumerate(rel):
        blk = a[:, i * H:(i + 1) * H]
        alive = R.alive_mask(s, d, PAIR_LIMIT)
        assert_close_rel(f[i], R.pair_features(blk, s, d, PAIR_LIMIT), 1e-6, f"relation {i}: F")
        assert float(f[i][~alive].abs().sum()) == 0.0
        exp_y = torch.zeros(s.numel(), dtype=torch.long)
        exp_y[alive] = R.edge_labels(labels, s[alive], d[alive])
        assert torch.equal(y[i].long(), exp_y), f"relation {i}: edge labels"
        ref = R.pair_backward(blk, s, d, PAIR_LIMIT, df[lo:lo + s.numel()])
        assert_close_rel(da[:, i * H:(i + 1) * H], ref, TOL, f"relation {i}: dA")
        lo += s.numel()
    assert int(y[0].sum()) > 0 and int(R.alive_mask(*rel[0], PAIR_LIMIT).sum()) > int(y[0].sum())
    assert float(da[:, H:].abs().max()) == 0.0                                  # a relation without an alive edge: zeros, written
    assert float(da[9].abs().max()) == 0.0 and float(da[PAIR_LIMIT:].abs().max()) == 0.0    # no edge / beyond the limit
    assert float(da[0, :H].abs().max()) > 0 and float(da[2, :H].abs().max()) > 0


def test_self_loop_counts_twice():
    H = 8
    a = torch.randn(6, H, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    s = torch.tensor([3], dtype=torch.int64)
    df = torch.randn(1, H, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    _, _, da = hip_pair(a, [(s, s.clone())], 6, df=df)
    assert_close_rel(da[3], 2 * df[0] * a[3], 1e-6, "self loop")
    da[3] = 0
    assert float(da.abs().max()) == 0.0


def test_pair_launch_grouping():
    """Two relations in one launch equal each alone, bit for bit; a full table of MAX_SEG relations works."""
    from analysisgnn_amd import _lib
    H = 36
    rel = [pair_graph()[0], random_edges(90, 3, PAIR_N)]
    g = torch.Generator().manual_seed(7)
    a = torch.randn(PAIR_N, 2 * H, generator=g, dtype=torch.float64)
    df = torch.randn(sum(s.numel() for s, _ in rel), H, generator=g, dtype=torch.float64)
    labels = seg_labels(PAIR_N, 6)
    both = hip_pair(a, rel, PAIR_LIMIT, labels, df=df)
    lo = 0
    for i, (s, d) in enumerate(rel):
        alone = hip_pair(a[:, i * H:(i + 1) * H].contiguous(), [(s, d)], PAIR_LIMIT, labels, df=df[lo:lo + s.numel()])
        assert torch.equal(alone[0][0], both[0][i]) and torch.equal(alone[1][0], both[1][i])
        assert torch.equal(alone[2], both[2][:, i * H:(i + 1) * H])
        lo += s.numel()
    Rn, H = _lib.MAX_SEG, 8
    rel = [random_edges([0, 3, 70][k % 3], 500 + k, PAIR_N) for k in range(Rn)]
    a = torch.randn(PAIR_N, Rn * H, generator=g, dtype=torch.float64)
    df = torch.randn(sum(s.numel() for s, _ in rel), H, generator=g, dtype=torch.float64)
    f, y, da = hip_pair(a, rel, PAIR_LIMIT, labels, df=df)
    lo = 0
    for i, (s, d) in enumerate(rel):
        blk = a[:, i * H:(i + 1) * H]
        assert_close_rel(f[i], R.pair_features(blk, s, d, PAIR_LIMIT), 1e-6, f"relation {i}: F")
        assert_close_rel(da[:, i * H:(i + 1) * H], R.pair_backward(blk, s, d, PAIR_LIMIT, df[lo:lo + s.numel()]), TOL, f"relation {i}: dA")
        lo += s.numel()


# ---- the whole term at other shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [0, 1, 63, 64, 65])
def test_edge_counts_around_the_tile(E):
    P = rand_params(16, ["onset"], 40)
    x = torch.randn(N, 16, generator=torch.Generator().manual_seed(41))
    edges = {"onset": random_edges(E, 300 + E)}
    labels = seg_labels(N, 42)
    hip = hip_term(P, x, edges, labels, LIMIT)
    check_term(hip, reference_term(P, x, edges, labels, LIMIT), edges)
    if E == 0:
        assert float(hip[0]) == 0.0 and float(hip[3].grad.abs().max()) == 0.0


def test_full_table_of_relations_and_grouping_of_the_cross_entropy():
    """MAX_SEG relations through the cross-entropy kernels (empty ones among them) against torch in float64; two relations in one
    launch equal each alone, bit for bit."""
    from analysisgnn_amd import _lib
    from analysisgnn_amd.edge_loss import _EdgeCE, edge_plan
    H = 36

    def run(rel, y, w4, b4, lab):
        plan = edge_plan({et(f"r{i}"): (s.to(DEV), d.to(DEV)) for i, (s, d) in enumerate(rel)}, LIMIT, N, select=False)
        yd, wd, bd = (t.float().to(DEV).requires_grad_(True) for t in (y, w4, b4))
        info = {"edge_labels": lab.to(DEV)}
        total, logit = _EdgeCE.apply(plan, info, 0.1, yd, wd, bd)
        total.backward()
        torch.cuda.synchronize()
        return total.detach().cpu(), logit.detach().cpu(), info["losses"].cpu(), info["counts"].cpu(), yd.grad.cpu(), wd.grad.cpu(), bd.grad.cpu()

    g = torch.Generator().manual_seed(9)
    for Rn in (2, _lib.MAX_SEG):
        rel = [random_edges([70, 130, 0, 3][k % 4], 700 + k) for k in range(Rn)]
        E = sum(s.numel() for s, _ in rel)
        y = torch.randn(E, H, generator=g, dtype=torch.float64)
        w4 = torch.randn(2, H, generator=g, dtype=torch.float64) * H ** -0.5
        b4 = torch.randn(2, generator=g, dtype=torch.float64) * 0.1
        lab = torch.randint(0, 2, (E,), generator=g).to(torch.uint8)
        total, logit, losses, counts, dy, dw, db = run(rel, y, w4, b4, lab)
        y64, w64, b64 = (t.clone().requires_grad_(True) for t in (y, w4, b4))
        z = y64 @ w64.t() + b64
        ce = torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
        ref_losses, lo = [], 0
        for i, (s, d) in enumerate(rel):
            a = R.alive_mask(s, d, LIMIT)
            zi, li = z[lo:lo + s.numel()], lab[lo:lo + s.numel()].long()
            ref_losses.append(ce(zi[a], li[a]) if bool(a.any()) else z.sum() * 0)
            if bool(a.any()):
                assert float((zi[a][:, 1] - zi[a][:, 0]).detach().abs().min()) > 1e-4, "choose another seed"
            assert_close_rel(logit[lo:lo + s.numel()][a], zi[a].detach(), TOL, f"relation {i}: logits")
            assert float(logit[lo:lo + s.numel()][~a].abs().sum()) == 0.0 and float(dy[lo:lo + s.numel()][~a].abs().sum()) == 0.0
            assert counts[i].tolist() == R.confusion(zi.detach(), li, a), f"relation {i}: counts"
            lo += s.numel()
        ref_total = sum(ref_losses) / Rn
        ref_total.backward()
        assert_close_rel(losses, torch.stack([t.detach() for t in ref_losses]), TOL, "losses")
        assert_close_rel(total, ref_total, TOL, "total")
        assert_close_rel(dy, y64.grad, TOL, "dy")
        assert_close_rel(dw, w64.grad, TOL, "dw4")
        assert_close_rel(db, b64.grad, TOL, "db4")
        if Rn == 2:
            lo = 0
            for i, (s, d) in enumerate(rel):
                n = s.numel()
                alone = run([(s, d)], y[lo:lo + n], w4, b4, lab[lo:lo + n])
                assert torch.equal(alone[1], logit[lo:lo + n]) and torch.equal(alone[2][0], losses[i]) and torch.equal(alone[3][0], counts[i])
                lo += n


def test_more_tiles_than_the_final_pass_has_lanes():
    """256 * 64 + 1 edges in one relation are 257 tiles of the cross entropy: lane 0 of the final pass adds tiles 0 and 256 before
    the tree in LDS (every other case here has at most 5 tiles).  Loss, 1 / alive and the five counts against torch in float64; the
    small relation behind it in the table gives the bits it gives alone."""
    from analysisgnn_amd.edge_loss import _EdgeCE, edge_plan
    H = 4

    def run(rel, y, lab):
        plan = edge_plan({et(f"r{i}"): (s.to(DEV), d.to(DEV)) for i, (s, d) in enumerate(rel)}, LIMIT, N, select=False)
        info = {"edge_labels": lab.to(DEV)}
        total, logit = _EdgeCE.apply(plan, info, 0.1, y.float().to(DEV), w4.float().to(DEV), b4.float().to(DEV))
        torch.cuda.synchronize()
        return total.cpu(), logit.cpu(), info["losses"].cpu(), info["inv_cnt"].cpu(), info["counts"].cpu()

    g = torch.Generator().manual_seed(90)
    rel = [random_edges(256 * 64 + 1, 91), random_edges(70, 92)]
    E = sum(s.numel() for s, _ in rel)
    y = torch.randn(E, H, generator=g, dtype=torch.float64)
    w4 = torch.randn(2, H, generator=g, dtype=torch.float64) * H ** -0.5
    b4 = torch.randn(2, generator=g, dtype=torch.float64) * 0.1
    lab = torch.randint(0, 2, (E,), generator=g).to(torch.uint8)
    total, logit, losses, inv_cnt, counts = run(rel, y, lab)
    z = y @ w4.t() + b4
    ce = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    ref_losses, lo = [], 0
    for i, (s, d) in enumerate(rel):
        a = R.alive_mask(s, d, LIMIT)
        zi, li = z[lo:lo + s.numel()], lab[lo:lo + s.numel()].long()
        assert int(a.sum()) > 0 and float((zi[a][:, 1] - zi[a][:, 0]).abs().min()) > 1e-4, "choose another seed"
        ref_losses.append(ce(zi[a], li[a]))
        assert bool(torch.isfinite(ref_losses[-1]))
        assert bool(a[-1]), "the last edge (alone in tile 256 of relation 0) must be alive: leaving its tile out must move the counts"
        assert counts[i].tolist() == R.confusion(zi, li, a), f"relation {i}: counts"
        assert float(inv_cnt[i]) == pytest.approx(1.0 / int(a.sum()), rel=1e-6, abs=0.0)
        lo += s.numel()
    assert_close_rel(losses, torch.stack(ref_losses), TOL, "losses")
    assert_close_rel(total, sum(ref_losses) / 2, TOL, "total")
    n0 = rel[0][0].numel()
    alone = run([rel[1]], y[n0:], lab[n0:])
    assert torch.equal(alone[1], logit[n0:]) and torch.equal(alone[2][0], losses[1]) and torch.equal(alone[3][0], inv_cnt[1])
    assert torch.equal(alone[4][0], counts[1])


def test_empty_relations():
    """A relation without an alive edge: loss 0, zero gradient blocks, count 0, and the total stays finite — it is still one of
    the R relations the mean is taken over."""
    rels = ["onset", "during", "rest"]
    P = rand_params(16, rels, 50)
    x = torch.randn(N, 16, generator=torch.Generator().manual_seed(51))
    beyond = (torch.tensor([33, 34, 2], dtype=torch.int64), torch.tensor([1, 35, 39], dtype=torch.int64))
    edges = {"onset": random_edges(50, 52), "during": beyond, "rest": (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))}
    labels = seg_labels(N, 53)
    hip = hip_term(P, x, edges, labels, LIMIT)
    loss, parts, dec, xd, _ = hip
    assert parts["alive"].cpu().tolist()[1:] == [0, 0] and parts["losses"].cpu().tolist()[1:] == [0.0, 0.0]
    assert dec.last["counts"][1:].cpu().tolist() == [[0] * 5] * 2
    assert bool(torch.isfinite(loss)) and float(loss) == pytest.approx(float(parts["losses"][0]) / 3, rel=1e-6)
    for r in ("during", "rest"):
        for k, p in dec.named_parameters():
            if k.startswith(f"embed.{r}."):
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    assert bool(torch.isfinite(xd.grad).all())
    check_term(hip, reference_term(P, x, edges, labels, LIMIT), edges)


def test_two_runs_give_the_same_bits():
    rels = ["onset", "rest"]
    P = rand_params(16, rels, 60)
    x = torch.randn(N, 16, generator=torch.Generator().manual_seed(61))
    edges = {"onset": random_edges(257, 62), "rest": random_edges(65, 63)}
    labels = seg_labels(N, 64)
    a, b = hip_term(P, x, edges, labels, LIMIT), hip_term(P, x, edges, labels, LIMIT)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3].grad, b[3].grad) and torch.equal(a[1]["losses"], b[1]["losses"])
    for (k, p), (_, q) in zip(a[2].named_parameters(), b[2].named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    for i in range(2):
        assert torch.equal(a[2].last["logits"][i], b[2].last["logits"][i])
    H = 260                                                                   # the pair kernel's second column pass
    rel = [pair_graph()[0], random_edges(130, 65, PAIR_N)]
    g = torch.Generator().manual_seed(66)
    am = torch.randn(PAIR_N, 2 * H, generator=g, dtype=torch.float64)
    df = torch.randn(sum(s.numel() for s, _ in rel), H, generator=g, dtype=torch.float64)
    u, v = hip_pair(am, rel, PAIR_LIMIT, df=df), hip_pair(am, rel, PAIR_LIMIT, df=df)
    assert all(torch.equal(p, q) for p, q in zip(u[0], v[0])) and torch.equal(u[2], v[2])


# ---- dropout ------------------------------------------------------------------------------------------------------------------
def test_dropout_masks():
    from analysisgnn_amd.fused import advance_rng, rng_state
    H, E, n, p = 128, 200, 64, 0.3
    g = torch.Generator().manual_seed(70)
    a = (0.5 + torch.rand(n, H, generator=g, dtype=torch.float64)) * (1 - 2 * torch.randint(0, 2, (n, H), generator=g))      # no zeros
    a = a.float().double()
    s, d = torch.randint(0, n, (2, E), generator=g)
    df = torch.randn(E, H, generator=g, dtype=torch.float64).float().double()
    rng_state(torch.device(DEV))
    f, _, da = hip_pair(a, [(s, d)], n, p=p, df=df)
    f = f[0].double()
    full = a[s] * a[d] / (1 - p) ** 2
    kept = f != 0
    assert float((f - full)[kept].abs().max()) <= 1e-6 * float(full.abs().max())           # 0 or A[s] A[d] / (1 - p)^2
    share, want = float(kept.double().mean()), (1 - p) ** 2
    sigma = (want * (1 - want) / kept.numel()) ** 0.5                                       # 0.0031 at 200 x 128 elements
    assert abs(share - want) <= 5 * sigma, f"kept share {share:.4f}: the two ends of an edge must draw independent masks ({want:.2f}, not {1 - p:.2f})"
    mask = kept.double() / (1 - p) ** 2
    assert_close_rel(da, R.pair_backward(a, s, d, n, df, mask), TOL, "dA with the masks recovered from F")
    again = hip_pair(a, [(s, d)], n, p=p)[0][0].double()
    assert torch.equal(again != 0, kept)                                                    # the same (seed, step, call id): the same masks
    other_site = hip_pair(a, [(s, d)], n, p=p, call_id=78)[0][0].double()
    assert not torch.equal(other_site != 0, kept)
    advance_rng(torch.device(DEV))
    try:
        moved = hip_pair(a, [(s, d)], n, p=p)[0][0].double()
    finally:
        rng_state(torch.device(DEV))[1:2].sub_(1)                                           # leave the counter as it was found
    assert not torch.equal(moved != 0, kept)
    assert abs(float((moved != 0).double().mean()) - want) <= 5 * sigma
    eval_f = hip_pair(a, [(s, d)], n, p=0.0)[0][0].double()
    assert bool((eval_f != 0).all())                                                        # p = 0: nothing is dropped


def test_training_mode_runs_with_dropout():
    """The decoder in training mode (dropout 0.3 in the pair kernel and in `fc`): finite loss and gradients, and the eval-mode
    forward of the same module gives the dropout-free logits."""
    rels = ["onset", "rest"]
    P = rand_params(16, rels, 80)
    x = torch.randn(N, 16, generator=torch.Generator().manual_seed(81))
    edges = {"onset": random_edges(100, 82), "rest": random_edges(30, 83)}
    labels = seg_labels(N, 84)
    loss, parts, dec, xd, plan = hip_term(P, x, edges, labels, LIMIT, dropout=0.3, train=True)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) > 0
    assert all(bool(torch.isfinite(p.grad).all()) for p in dec.parameters())
    ev = hip_term(P, x, edges, labels, LIMIT, dropout=0.3, train=False)
    check_term(ev, reference_term(P, x, edges, labels, LIMIT), edges)


# ---- selection ----------------------------------------------------------------------------------------------------------------
def _selection_case():
    z = load_golden("edge_h8_whole")
    rels = [str(r) for r in z["meta.relations"]]
    ei = {et(r): torch.from_numpy(np.asarray(z["edges." + r])).long().to(DEV) for r in rels}
    return z, rels, ei, int(z["meta.cfg"][1])


def _kept_pairs(plan, r):
    s, d = (t.cpu() for t in plan.edges(r))
    ok = R.alive_mask(s, d, plan.limit)
    assert bool(((s == plan.n_rows) & (d == plan.n_rows))[~ok].all())           # dropped edges carry the out-of-range id
    return [(int(a), int(b)) for a, b in zip(s[ok], d[ok])]


def test_selection():
    from analysisgnn_amd import edge_plan
    z, rels, ei, bs = _selection_case()
    rng = torch.tensor([1234, 0], dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                  # the plan is built without a device-to-host copy
    try:
        plan = edge_plan(ei, bs, rng=rng, relations=rels)
        same = edge_plan(ei, bs, rng=rng, relations=rels)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    other = edge_plan(ei, bs, rng=torch.tensor([1234, 1], dtype=torch.int64, device=DEV), relations=rels)
    assert plan.relations == rels
    capped = 0
    for i, r in enumerate(rels):
        e = ei[et(r)].cpu()
        pool = {(int(a), int(b)) for a, b in zip(e[0], e[1]) if a < bs and b < bs}
        alive = int(z["meta.alive"][i])
        assert len(pool) == alive
        kept = _kept_pairs(plan, i)
        assert len(kept) == min(alive, bs), r                                 # the count of :994-997
        assert len(set(kept)) == len(kept) and set(kept) <= pool, r           # alive, no duplicates
        assert plan.e_off[i + 1] - plan.e_off[i] == min(e.shape[1], bs)       # never more than batch_size rows per relation
        assert _kept_pairs(same, i) == kept                                   # the same (seed, step): the same subset
        if alive > bs:
            capped += 1
            if alive > bs + 10:                                               # another step: another subset (49 choose 48 could repeat)
                assert set(_kept_pairs(other, i)) != set(kept), r
        else:
            assert set(kept) == pool
    assert capped >= 2


def test_selection_reaches_every_alive_edge():
    """64 steps on the onset relation (128 alive, 48 kept a step): every alive edge is kept at least once; under a uniform draw a
    miss has probability 128 (1 - 48 / 128)^64 < 1e-11."""
    from analysisgnn_amd import edge_plan
    _, _, ei, bs = _selection_case()
    one = {et("onset"): ei[et("onset")]}
    e = one[et("onset")].cpu()
    pool = {(int(a), int(b)) for a, b in zip(e[0], e[1]) if a < bs and b < bs}
    assert len(pool) == 128
    seen, times = set(), {}
    for step in range(64):
        kept = _kept_pairs(edge_plan(one, bs, rng=torch.tensor([99, step], dtype=torch.int64, device=DEV)), 0)
        assert len(kept) == bs
        seen |= set(kept)
        for k in kept:
            times[k] = times.get(k, 0) + 1
    assert seen == pool
    assert max(times.values()) < 64                                           # and none is kept every time ((48 / 128)^64)


# ---- capture ------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_under_capture():
    """With the plan built beforehand the term, forward + backward, is captured once and replayed twice: bitwise the eager result."""
    from analysisgnn_amd import EdgeDecoder, edge_consistency_loss, edge_plan
    rels = ["onset", "rest"]
    P = rand_params(16, rels, 90)
    dec = EdgeDecoder(16, rels, dropout=0.0)
    dec.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    dec.to(DEV).train()
    x = torch.randn(N, 16, generator=torch.Generator().manual_seed(91)).to(DEV).requires_grad_(True)
    labels = seg_labels(N, 92).to(DEV)
    edges = {et("onset"): tuple(t.to(DEV) for t in random_edges(130, 93)), et("rest"): tuple(t.to(DEV) for t in random_edges(20, 94))}
    plan = edge_plan(edges, LIMIT, N, select=False, relations=rels)
    params = list(dec.parameters())
    torch.cuda.synchronize()

    def step():
        loss, parts = edge_consistency_loss(dec, x, plan, labels)
        return (loss, parts["losses"]) + torch.autograd.grad(loss, [x] + params)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        eager = [t.detach().clone() for t in step()]
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in eager) and float(eager[2].abs().max()) > 0
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        captured = step()
    for _ in range(2):
        for t in captured:
            t.detach().fill_(float("nan"))
        cg.replay()
        torch.cuda.synchronize()
        for j, (a, b) in enumerate(zip(eager, captured)):
            assert torch.equal(a, b.detach()), f"tensor {j}"
