"""Pins oracle/hgt_attn_ref.py (the float64 reference the attention kernels are compared with, tests/test_gpu_hgt_attention.py)
before anything is compared with it: its closed-form backward against torch.autograd through its own forward formulas, its
forward against the restatement of PyG's HGTConv every other HGT test rests on (oracle/pyg_ref.hgt_conv), and its trimming
against the same function on narrowed inputs.  CPU only."""
import pytest
import torch

from oracle import hgt_attn_ref as A


def _rel_err(a, b):
    scale = float(b.abs().max())
    return float((a - b).abs().max()) / scale if scale > 0 else float((a - b).abs().max())


def _case(H, heads, seed, n=23, n_src=(17, 9, 30)):
    """Three relations into n destination rows: a dense random one in which row 2 has 500 edges and rows 5..8 none, an EMPTY
    one, and a sparse one with duplicate edges.  Rows 5 and 6 have no edge in any relation."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(n, H, generator=g, dtype=torch.float64)
    dm = torch.randn(n, H, generator=g, dtype=torch.float64)
    rels = []
    for r, ns in enumerate(n_src):
        if r == 0:
            dst = torch.cat([torch.full((500,), 2), torch.randint(0, n, (150,), generator=g)])
            dst = dst[~((dst >= 5) & (dst <= 8))]
            dst = dst[torch.randperm(dst.numel(), generator=g)]
        elif r == 1:
            dst = torch.zeros(0, dtype=torch.int64)
        else:
            dst = torch.tensor([0, 0, 7, 8, 8, 22, 22, 22, 1])
        src = torch.randint(0, ns, (dst.numel(),), generator=g)
        if r == 2:
            src[0] = src[1]                                          # a duplicate edge
        rels.append(dict(k=torch.randn(ns, H, generator=g, dtype=torch.float64), v=torch.randn(ns, H, generator=g, dtype=torch.float64),
                         src=src, dst=dst, pscale=(torch.rand(heads, generator=g, dtype=torch.float64) + 0.5) / (H // heads) ** 0.5))
    return q, dm, rels


@pytest.mark.parametrize("H,heads", [(16, 4), (256, 4), (256, 1)])       # D = 4, 64, 256
def test_closed_form_backward_equals_autograd(H, heads):
    q, dm, rels = _case(H, heads, seed=H + heads)
    ref = A.attention(q, dm, heads, rels)
    assert bool(torch.isinf(ref["m"][5]).all()) and bool((ref["out"][5] == 0).all()) and bool((ref["dq"][6] == 0).all())
    assert int((rels[0]["dst"] == 2).sum()) >= 500
    leaves = [q.clone().requires_grad_(True)]
    arels = []
    for rel in rels:
        a = dict(rel)
        for name in ("k", "v", "pscale"):
            a[name] = rel[name].clone().requires_grad_(True)
            leaves.append(a[name])
        arels.append(a)
    out = A.forward(leaves[0], heads, arels)["out"]
    grads = torch.autograd.grad((out * dm).sum(), leaves, allow_unused=True)
    assert _rel_err(ref["out"], out.detach()) == 0.0
    assert _rel_err(ref["dq"], grads[0]) <= 1e-12
    for r, (rel, rr) in enumerate(zip(rels, ref["rels"])):
        gk, gv, gp = grads[1 + 3 * r:4 + 3 * r]
        if rel["src"].numel() == 0:                                   # the empty relation: zero gradients, nothing per edge
            assert float(rr["dk"].abs().max()) == 0.0 and float(rr["dv"].abs().max()) == 0.0 and rr["alpha"].shape == (0, heads)
            assert gk is None or float(gk.abs().max()) == 0.0
            continue
        assert _rel_err(rr["dk"], gk) <= 1e-12, r
        assert _rel_err(rr["dv"], gv) <= 1e-12, r
        assert _rel_err(rr["tdot"].sum(0), gp) <= 1e-12, r           # sum_e tdot = d / d pscale
        assert not torch.isnan(rr["alpha"]).any() and not torch.isnan(rr["gs"]).any()
    # every row with an edge: its weights sum to 1 per head
    tot = torch.zeros(q.shape[0], heads, dtype=torch.float64)
    for rel, rr in zip(rels, ref["rels"]):
        tot.index_add_(0, rel["dst"], rr["alpha"])
    has = ~torch.isinf(ref["m"][:, 0])
    assert torch.allclose(tot[has], torch.ones_like(tot[has]), atol=1e-12) and float(tot[~has].abs().max()) == 0.0


@pytest.mark.parametrize("C,heads", [(32, 4), (64, 1)])
def test_forward_equals_the_messages_of_pyg_ref_hgt_conv(C, heads):
    """On a note / beat / measure graph the reference's `out`, fed the q / k' / v' that pyg_ref.hgt_conv forms, is the `m`
    hgt_conv aggregates — per destination type, over all relations that end in it."""
    from analysisgnn_amd.hgt import HGTConv
    from analysisgnn_amd.synth import make_batch, torch_inputs
    from oracle import pyg_ref as G
    g = make_batch(2, 60, first_seed=7, add_beats=True, add_measures=True)
    md = g.metadata()
    torch.manual_seed(C)
    layer = HGTConv(C, C, md, heads)
    with torch.no_grad():
        for p in layer.p_rel.values():
            p.uniform_(0.5, 1.5)
    P = {k: v.detach().double() for k, v in layer.state_dict().items()}
    I = torch_inputs(g, in_channels=C, seed=5)
    x = {k: v.double() for k, v in I["x_dict"].items()}
    taps = {}
    res = G.hgt_conv(P, "", md[0], md[1], heads, x, I["edge_index_dict"], taps=taps)
    plain = G.hgt_conv(P, "", md[0], md[1], heads, x, I["edge_index_dict"])
    assert all(torch.equal(res[t], plain[t]) for t in res)            # the taps do not change what the layer returns
    seen = 0
    for t in x:
        rels = [dict(k=k2, v=v2, pscale=ps, src=I["edge_index_dict"][et][0], dst=I["edge_index_dict"][et][1])
                for et, k2, v2, ps in taps.get("rels", {}).get(t, [])]
        out = A.forward(taps["q"][t], heads, rels)["out"]
        assert _rel_err(out, taps["m"][t]) <= 1e-12, t
        seen += len(rels)
    assert seen == len(md[1]) and len(taps["m"]) >= 3


def test_trimmed_equals_narrowed():
    """`e_limit` / `n_keep` (masks on the COO list) against the same function on inputs narrowed the way
    pyg_ref.trim_to_layer narrows them: COO prefix per relation, row prefix of the destination type."""
    H, heads = 64, 4
    q, dm, rels = _case(H, heads, seed=11)
    n_keep = 15
    limits = [rels[0]["src"].numel() // 2, 0, 6]
    trimmed = [dict(rel, e_limit=lim) for rel, lim in zip(rels, limits)]
    a = A.attention(q, dm, heads, trimmed, n_keep=n_keep)
    narrowed = []
    for rel, lim in zip(rels, limits):
        src, dst = rel["src"][:lim], rel["dst"][:lim]
        inside = dst < n_keep                       # edges into dropped rows: none in a real sampled batch, dropped here
        narrowed.append(dict(rel, src=src[inside], dst=dst[inside]))
    b = A.attention(q[:n_keep], dm[:n_keep], heads, narrowed)
    for name in ("out", "m", "linv", "dq"):
        assert a[name].shape[0] == n_keep and torch.equal(a[name], b[name]), name
    for rel, lim, ra, rb in zip(rels, limits, a["rels"], b["rels"]):
        keep = ra["keep"]
        assert torch.equal(keep, (torch.arange(rel["src"].numel()) < lim) & (rel["dst"] < n_keep))
        for name in ("alpha", "gs", "tdot"):
            assert torch.equal(ra[name][keep], rb[name]) and bool(torch.isnan(ra[name][~keep]).all()), name
        assert torch.equal(ra["dk"], rb["dk"]) and torch.equal(ra["dv"], rb["dv"])
    assert int(a["rels"][0]["keep"].sum()) > 0 and int(a["rels"][1]["keep"].sum()) == 0


def test_float32_evaluation_is_close_to_float64():
    """The same code in float32 (the yardstick of the kernels' tolerance) is within a few 1e-7 of float64 on every tensor."""
    q, dm, rels = _case(256, 4, seed=3)
    q, dm = q.float(), dm.float()
    rels = [dict(r, k=r["k"].float(), v=r["v"].float(), pscale=r["pscale"].float()) for r in rels]
    a64 = A.attention(q, dm, 4, rels)                                  # the float32 inputs, evaluated in float64
    a32 = A.attention(q, dm, 4, rels, dtype=torch.float32)
    assert a32["out"].dtype == torch.float32 and a32["rels"][0]["gs"].dtype == torch.float32
    for name in ("out", "dq"):
        assert _rel_err(a32[name].double(), a64[name]) < 5e-6, name
    assert float(a32["linv"][5, 0]) == float(torch.tensor(1.0) / torch.tensor(1e-16))
