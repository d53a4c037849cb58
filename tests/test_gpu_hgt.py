"""HGT edge-softmax attention on the HIP kernels vs the CPU restatement of PyG HGTConv (oracle/pyg_ref.py,
oracle/encoders_ref.py).  fp32, tolerance 1e-4 relative to max(1,|ref|max) (north-star bound) for outputs,
input gradients and every parameter gradient; dropout = 0, train() mode (MIOpen RNN backward needs it)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import assert_close  # noqa: E402

TOL = 1e-4
DEV = "cuda:0"


def _cpu_params(module):
    return {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in module.state_dict().items()}


def _cmp_grads(module, P):
    n = 0
    for name, p in module.named_parameters():
        if P[name].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, f"{name}: no gradient on the HIP path"
        assert_close(p.grad, P[name].grad, TOL, f"grad {name}")
        n += 1
    assert n > 0


def _graph(kind):
    from analysisgnn_amd.synth import make_batch, make_score_graph, sample_hops
    if kind == "notes":
        return make_batch(2, 50, first_seed=4)
    if kind == "c3":      # note + beat + measure, 4 note-note relations + note->beat + note->measure (C3 layout)
        return make_batch(2, 60, first_seed=7, add_beats=True, add_measures=True)
    if kind == "metrical_rev":
        return make_batch(2, 60, first_seed=9, add_beats=True, add_measures=True, reverse_metrical_edges=True)
    if kind == "sampled":
        return sample_hops(make_score_graph(seed=3, n_notes=260), n_targets=48, num_neighbors=[4, 4], seed=2,
                           random_targets=True)
    raise ValueError(kind)


def _c3_edge_types(g):
    """C3 uses 6 relation types: drop beat->measure so only note-sourced relations remain."""
    return [et for et in g.edge_types if et[0] == "note"]


# every graph at D = 8 and 64; the ends of the head-width range (D = 4, 128, 256 — the last at H = 512, two chunks per row) on the
# C3 graph: the relation transforms' torch path and the RELT_D dispatch of `_relt` beside the attention kernels
@pytest.mark.parametrize("C,heads,kind", [(C, heads, kind) for C, heads in [(32, 4), (64, 1), (256, 4)] for kind in ["notes", "c3", "metrical_rev"]]
                         + [(64, 16, "c3"), (128, 1, "c3"), (512, 2, "c3")])
def test_hgt_conv_layer(kind, C, heads):
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
    P = _cpu_params(m)
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
    _cmp_grads(m, P)


def test_attention_forward_weights_sum_to_one():
    """Property at the C3 shape (H=256, heads=4, 32 x 500 notes + beats + measures): with v' = 1 every destination
    row that has an incoming edge aggregates exactly 1 (sum of softmax weights), rows without edges give 0."""
    from analysisgnn_amd import _lib
    from analysisgnn_amd.graph import HeteroIndex
    from analysisgnn_amd.hgt import attention_forward
    from analysisgnn_amd.synth import make_batch
    g = make_batch(32, 500, add_beats=True, add_measures=True)
    ets = [et for et in g.edge_types if et[0] == "note" and et[2] == "beat"] + []
    dev = torch.device(DEV)
    eid = {et: torch.from_numpy(g.edge_index[et]).to(dev) for et in g.edge_types}
    hix = HeteroIndex(eid, g.num_nodes)
    for dst in ("note", "beat", "measure"):
        rels = [et for et in g.edge_types if et[2] == dst]
        n = g.num_nodes[dst]
        gen = torch.Generator().manual_seed(1)
        q = torch.randn(n, 256, generator=gen).to(dev)
        kv = []
        for et in rels:
            kv += [torch.randn(g.num_nodes[et[0]], 256, generator=gen).to(dev), torch.ones(g.num_nodes[et[0]], 256, device=dev)]
        ps = torch.rand(len(rels), 4, generator=gen).to(dev) + 0.5
        table = (_lib.HgtRel * len(rels))()
        for r, et in enumerate(rels):
            c = hix.fwd[et]
            table[r].k, table[r].v, table[r].ld, table[r].pscale = kv[2 * r].data_ptr(), kv[2 * r + 1].data_ptr(), 256, ps[r].data_ptr()
            table[r].rowptr, table[r].col, table[r].perm = c.rowptr.data_ptr(), c.col.data_ptr(), c.perm.data_ptr()
        out = torch.empty(n, 256, device=dev)
        m, linv = torch.empty(n, 4, device=dev), torch.empty(n, 4, device=dev)
        attention_forward(table, q, out, m, linv, 4)
        deg = torch.zeros(n, device=dev)
        for et in rels:
            deg.index_add_(0, eid[et][1], torch.ones(eid[et].shape[1], device=dev))
        has = deg > 0
        assert torch.allclose(out[has], torch.ones_like(out[has]), atol=1e-5)
        assert torch.all(out[~has] == 0)


@pytest.mark.parametrize("kind", ["c3", "sampled"])
def test_hybrid_hgt_encoder(kind):
    from analysisgnn_amd.hgt import HybridHGT
    from analysisgnn_amd.synth import torch_inputs
    from oracle import encoders_ref as E
    g = _graph(kind)
    H, L = 32, 3
    torch.manual_seed(0)
    m = HybridHGT(metadata=g.metadata(), input_channels=H, hidden_channels=H, num_layers=L, heads=4, dropout=0.0,
                  use_jk=False, logit_fusion=False).train()
    P = _cpu_params(m)
    m = m.to(DEV)
    I = torch_inputs(g, in_channels=H, seed=1)
    xc = {k: v.clone().requires_grad_(True) for k, v in I["x_dict"].items()}
    ref = E.hybrid_hgt(P, "", g.metadata(), L, 4, xc, I["edge_index_dict"], I["batch_dict"], I["batch_size"],
                       I["neighbor_mask_node"], I["neighbor_mask_edge"])
    xg = {k: v.to(DEV).requires_grad_(True) for k, v in I["x_dict"].items()}
    out = m(x_dict=xg, edge_index_dict={k: v.to(DEV) for k, v in I["edge_index_dict"].items()},
            batch_dict={k: v.to(DEV) for k, v in I["batch_dict"].items()}, batch_size=I["batch_size"],
            neighbor_mask_node=I["neighbor_mask_node"], neighbor_mask_edge=I["neighbor_mask_edge"])
    assert_close(out, ref, TOL, "out")
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(9))
    (ref * gout).sum().backward()
    (out * gout.to(DEV)).sum().backward()
    for k in xc:
        if xc[k].grad is not None:
            assert_close(xg[k].grad, xc[k].grad, TOL, f"grad x[{k}]")
    _cmp_grads(m, P)


def test_analysis_model_hgt_logits():
    from analysisgnn_amd.models import TorchAnalysisGNN
    from analysisgnn_amd.synth import make_batch, torch_inputs
    from oracle import encoders_ref as E
    g = make_batch(2, 64, first_seed=13, add_beats=True, add_measures=True)
    tasks = {"cadence": 4, "localkey": 50, "romanNumeral": 185}
    torch.manual_seed(3)
    m = TorchAnalysisGNN(g.metadata(), in_channels=25, hidden_channels=32, out_channels=16, task_dict=tasks, num_layers=3,
                         dropout=0.0, use_jk=False, logit_fusion=False, encoder_type="hgt").train()
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    I = torch_inputs(g, in_channels=25, seed=4)
    with torch.no_grad():
        x = E.analysis_encode(P, "hgt", g.metadata(), 3, I["pitch_spelling"], I["key_signature"], I["x_dict"],
                              I["edge_index_dict"], I["batch_dict"], I["batch_size"])
        ref = E.analysis_logits(P, x, list(tasks))
        out = m(I["pitch_spelling"].to(DEV), I["key_signature"].to(DEV), {k: v.to(DEV) for k, v in I["x_dict"].items()},
                {k: v.to(DEV) for k, v in I["edge_index_dict"].items()}, {k: v.to(DEV) for k, v in I["batch_dict"].items()},
                I["batch_size"], None, None)
    for t in tasks:
        assert_close(out[t], ref[t], TOL, f"logits[{t}]")


@pytest.mark.parametrize("N,R,heads,T,D", [(16000, 6, 4, 6, 64), (1003, 2, 4, 7, 64), (130, 1, 1, 3, 64), (5, 3, 2, 3, 64),
                                           (1003, 2, 4, 7, 8), (1003, 2, 4, 7, 16)])
def test_relation_transforms_match_float64(N, R, heads, T, D):
    """The per-head D x D relation transforms of HGTConv as `_HGTCore` issues them (hgt._relt: agnn_relt_fwd / _bwd / _dw at
    D = 64, torch batched matmuls at other head widths) against per-block float64 matmuls: K and V in one call, relations picked
    out of a larger parameter (`rel_ids`), rows not a multiple of the 128-row tile, gradients w.r.t. both operands and both
    parameters."""
    from analysisgnn_amd.hgt import _relt
    H = heads * D
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(N + R)
    rel_ids = tuple(sorted(torch.randperm(T, generator=g)[:R].tolist()))
    kqv = torch.randn(N, 3 * H, generator=g)                       # K | Q | V side by side: the operands are column views
    wk = torch.randn(T * heads, D, D, generator=g) * 0.2
    wv = torch.randn(T * heads, D, D, generator=g) * 0.2
    gk, gv = torch.randn(N, R * H, generator=g), torch.randn(N, R * H, generator=g)
    kqv64, wk64, wv64 = (t.double().requires_grad_(True) for t in (kqv, wk, wv))

    def ref_of(x, w):
        blocks = []
        for r in rel_ids:
            for h in range(heads):
                blocks.append(x[:, h * D:(h + 1) * D] @ w[r * heads + h])
        return torch.cat(blocks, dim=1)
    rk, rv = ref_of(kqv64[:, :H], wk64), ref_of(kqv64[:, 2 * H:], wv64)
    ((rk * gk.double()).sum() + (rv * gv.double()).sum()).backward()
    kd, wkd, wvd, gkd, gvd = (t.to(dev) for t in (kqv, wk, wv, gk, gv))
    sel = torch.tensor([r * heads + h for r in rel_ids for h in range(heads)], device=dev)
    Wk, Wv = wkd.index_select(0, sel), wvd.index_select(0, sel)
    yk, yv = torch.empty(N, R * H, device=dev), torch.empty(N, R * H, device=dev)
    _relt("fwd", ((kd[:, :H], Wk, yk), (kd[:, 2 * H:], Wv, yv)), R, heads, D, dev)
    dkqv = torch.zeros(N, 3 * H, device=dev)                        # the gradients of the K and V column views; Q's stays 0
    _relt("bwd", ((gkd, Wk.transpose(1, 2).contiguous(), dkqv[:, :H]), (gvd, Wv.transpose(1, 2).contiguous(), dkqv[:, 2 * H:])),
          R, heads, D, dev)
    dWk, dWv = torch.empty_like(Wk), torch.empty_like(Wv)
    _relt("dw", ((kd[:, :H], gkd, dWk), (kd[:, 2 * H:], gvd, dWv)), R, heads, D, dev)
    assert_close(yk, rk.float(), 1e-5, "k'")
    assert_close(yv, rv.float(), 1e-5, "v'")
    assert_close(dkqv, kqv64.grad.float(), 1e-5, "d kqv")
    assert_close(torch.zeros_like(wkd).index_copy_(0, sel, dWk), wk64.grad.float(), 1e-5, "d k_rel.weight")
    assert_close(torch.zeros_like(wvd).index_copy_(0, sel, dWv), wv64.grad.float(), 1e-5, "d v_rel.weight")


@pytest.mark.parametrize("n,H,relu,p,with_x", [(16000, 256, True, 0.0, True), (3584, 256, True, 0.3, True), (897, 64, False, 0.0, True),
                                                (50, 256, True, 0.0, False)])
def test_skip_act_epilogue_matches_torch(n, H, relu, p, with_x):
    """agnn_skip_act_*: z = dropout(relu(lerp(x, o, sigmoid(skip)))) in one launch each way against the torch ops it replaces
    (float64): values, d o, d x and the scalar d skip (a deterministic ticket reduction).  With dropout the mask is the library's
    own: checked through its invariants (kept elements = value / (1 - p), dropped = 0, rate ~ p) and by replaying the backward
    through the SAME mask (read off the forward result)."""
    from analysisgnn_amd.fused import skip_act
    from helpers import assert_close_rel
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(n + H)
    o = torch.randn(n, H, generator=g)
    x = torch.randn(n, H, generator=g) if with_x else None
    skip = torch.tensor([0.3]) if with_x else None
    od = o.to(dev).requires_grad_(True)
    xd = x.to(dev).requires_grad_(True) if with_x else None
    sd = skip.to(dev).requires_grad_(True) if with_x else None
    z = skip_act(od, xd, sd, relu, p, True)
    gz = torch.randn(n, H, generator=g)
    z.backward(gz.to(dev))
    o64 = o.double().requires_grad_(True)
    x64 = x.double().requires_grad_(True) if with_x else None
    s64 = skip.double().requires_grad_(True) if with_x else None
    y = o64 if not with_x else torch.lerp(x64, o64, torch.sigmoid(s64))
    y = torch.relu(y) if relu else y
    if p > 0:
        zc = z.detach().cpu().double()
        keep = (zc != 0) | (y.detach() == 0)                       # where the forward kept the element (exact zeros of y: either way)
        rate = 1.0 - float(((zc != 0).sum()) / max(int((y.detach() != 0).sum()), 1))
        assert abs(rate - p) < 0.02, rate
        y = y * keep.double() / (1.0 - p)
    assert_close_rel(z, y.detach(), 1e-6, "z")
    y.backward(gz.double())
    assert_close_rel(od.grad, o64.grad, 1e-6, "d o")
    if with_x:
        assert_close_rel(xd.grad, x64.grad, 1e-6, "d x")
        assert_close_rel(sd.grad, s64.grad, 1e-5, "d skip")


def test_destination_types_in_one_attention_launch_give_the_same_layer():
    """agnn_hgt_attn_fwd_multi_f32 (every destination type's edge softmax in one launch) against one launch per type: the layer's
    outputs and input gradients bit for bit (the same rows by the same code), on the graph with note / beat / measure destinations."""
    from analysisgnn_amd import hgt
    from analysisgnn_amd.hgt import HGTConv
    from analysisgnn_amd.synth import torch_inputs
    g = _graph("metrical_rev")
    torch.manual_seed(3)
    m = HGTConv(256, 256, g.metadata(), 4).to(DEV)
    I = torch_inputs(g, in_channels=256, seed=2)
    ei = {k: v.to(DEV) for k, v in I["edge_index_dict"].items()}
    saved = hgt.ATTN_ONE_LAUNCH
    res = []
    try:
        for one in (True, False):
            hgt.ATTN_ONE_LAUNCH = one
            xg = {k: v.to(DEV).requires_grad_(True) for k, v in I["x_dict"].items()}
            out = m(xg, ei)
            sum(o.square().sum() for o in out.values()).backward()
            res.append(({k: o.detach() for k, o in out.items()}, {k: x.grad for k, x in xg.items()}))
    finally:
        hgt.ATTN_ONE_LAUNCH = saved
    assert len(res[0][0]) >= 3
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_type_streams_leave_every_gradient_unchanged():
    """hgt.TYPE_STREAMS runs the small node types' projections and `skip_act` epilogues on a second stream, and autograd replays
    each backward on its forward's stream: the note type's agnn_skip_act_bwd_f32 (several hundred blocks) and the beat type's then
    run side by side, each counting its blocks on a ticket.  They must not share one (resident.scratch: one workspace per stream
    lane): every gradient, each `skip` parameter's included, equals the one-stream step's to fp32 rounding, and each setting
    reproduces its own gradients bit for bit."""
    from analysisgnn_amd import graph, hgt
    from analysisgnn_amd.heads import training_loss
    from analysisgnn_amd.models import TorchAnalysisGNN
    from analysisgnn_amd.synth import make_batch, torch_inputs
    from test_gpu_step import _same_to_rounding
    dev = torch.device(DEV)
    tasks = {"cadence": 4, "localkey": 50, "hrythm": 2}
    g = make_batch(5, 500, first_seed=21, add_beats=True, add_measures=True)
    assert g.num_nodes["note"] >= 2000 and g.num_nodes["beat"] > 64
    I = torch_inputs(g, 25, dev, seed=0)
    labels = torch.stack([torch.randint(0, c, (I["batch_size"],), generator=torch.Generator().manual_seed(i)).to(dev)
                          for i, c in enumerate(tasks.values())])
    torch.manual_seed(0)
    model = TorchAnalysisGNN(g.metadata(), 25, 64, 32, tasks, 3, dropout=0.0, use_jk=False, logit_fusion=False, encoder_type="hgt").to(dev).train()
    saved = (graph.index_cache_enabled, hgt.TYPE_STREAMS)
    graph.index_cache_enabled = False

    def step(two_streams):
        hgt.TYPE_STREAMS = two_streams
        model.zero_grad(set_to_none=True)
        x = model.encode(I["pitch_spelling"], I["key_signature"], I["x_dict"], I["edge_index_dict"], I["batch_dict"], I["batch_size"],
                         I["neighbor_mask_node"], I["neighbor_mask_edge"])
        logits, offs, _ = model.forward_clf_fused(x)
        loss, _ = training_loss(logits, offs, labels, x, 0.1, 0.1, -1)
        loss.backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    try:
        one, one_again = step(False), step(False)
        two, two_again = step(True), step(True)
    finally:
        graph.index_cache_enabled, hgt.TYPE_STREAMS = saved
    skips = [n for n in one if ".skip." in n]
    assert len(skips) >= 3 and all(float(one[n].abs().max()) > 0 for n in skips), skips
    assert set(one) == set(two)
    for n in one:
        assert torch.isfinite(one[n]).all(), n
        assert torch.equal(one[n], one_again[n]), n
        assert torch.equal(two[n], two_again[n]), n
        _same_to_rounding(two[n], one[n], n)
