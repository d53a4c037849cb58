"""The join block between the encoder and project_enc without copies: the projection GEMM that reads [a0 | a1] where the two
blocks lie (agnn_gemm_nt2_f32), the onset pooling that writes its own concatenation and normalises it
(agnn_pool_cat_norm_f32) and the pooling's backward in one launch (agnn_pool_cat_bwd_f32) — against the launches they replace
(bit for bit where the arithmetic is the same) and against float64."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import assert_close_rel  # noqa: E402

DEV = torch.device("cuda", 0)
N, H = 300, 256
RTOL, ATOL = 1e-5, 1e-6          # tests/test_gpu_fused.py's figures for the LayerNorm kernels


# ---------------------------------------------------------------------------------------------------------------------
# two-operand GEMM
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_out", [64, 256])
@pytest.mark.parametrize("K0,K1", [(16, 16), (256, 256), (48, 272)])
@pytest.mark.parametrize("M", [1, 127, 129, 300])
def test_gemm_nt2_has_the_bits_of_gemm_nt_on_the_cat(M, K0, K1, N_out):
    """a0 a row-offset view, both blocks with leading dimensions of their own that are larger than their widths; rows below,
    at and above the 128-row tile; one k-step per block, a seam on an even and on an odd step (K0 = 48: three steps)."""
    from analysisgnn_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(1000 * M + K0 + N_out)
    a0 = torch.randn(M + 3, K0 + 8, generator=g).to(DEV)[3:, :K0]
    a1 = torch.randn(M, K1 + 20, generator=g).to(DEV)[:, :K1]
    assert a0.stride(0) != a1.stride(0) and a0.stride(0) > K0 and a1.stride(0) > K1
    w = (torch.randn(N_out, K0 + K1, generator=g) * 0.1).to(DEV)
    b = torch.randn(N_out, generator=g).to(DEV)
    s = _lib.stream_ptr(DEV)
    cat = torch.cat((a0, a1), dim=1)
    ref = torch.full((M, N_out + 4), 7.0, device=DEV)
    _lib.check(lib.agnn_gemm_nt_f32(cat.data_ptr(), cat.stride(0), w.data_ptr(), w.stride(0), b.data_ptr(), M, N_out, K0 + K1, ref.data_ptr(),
                                    ref.stride(0), s), "agnn_gemm_nt_f32")
    c = torch.full((M, N_out + 4), float("nan"), device=DEV)
    c[:, N_out:] = 7.0
    _lib.check(lib.agnn_gemm_nt2_f32(a0.data_ptr(), a0.stride(0), K0, a1.data_ptr(), a1.stride(0), K1, w.data_ptr(), w.stride(0), b.data_ptr(),
                                     M, N_out, c.data_ptr(), c.stride(0), s), "agnn_gemm_nt2_f32")
    assert torch.equal(c, ref)                                   # the product bit for bit, nothing written past N
    r64 = cat.double() @ w.double().t() + b.double()
    err = float((c[:, :N_out].double() - r64).abs().max() / r64.abs().max())
    assert err < 5e-6, err                                       # tests/test_gpu_kernels.py's bound for k_gemm_nt
    assert lib.agnn_gemm_nt2_f32(a0.data_ptr(), a0.stride(0), K0 + 8, a1.data_ptr(), a1.stride(0), K1, w.data_ptr(), w.stride(0), None, M, N_out,
                                 c.data_ptr(), c.stride(0), None) < 0          # K0 not a multiple of the k-step


def test_weight_gradient_in_two_column_blocks_equals_the_product_on_the_cat():
    """linear2's deferred weight gradient: two items that write column blocks of one dW (ld_dw), the bias gradient with the first.
    The row slices a product is cut into depend on what else is in the batch, so the two agree to fp32 rounding — 2e-6 of the
    largest magnitude, tests/test_gpu_step.py's figure for regrouped weight-gradient batches — and both with float64."""
    from analysisgnn_amd import linear as L
    g = torch.Generator().manual_seed(5)
    n, out_f, K0, K1 = 2500, 256, 48, 272
    dy = torch.randn(n, out_f, generator=g).to(DEV)
    x0 = torch.randn(n + 3, K0 + 8, generator=g).to(DEV)[3:, :K0]
    x1 = torch.randn(n, K1 + 20, generator=g).to(DEV)[:, :K1]
    cat = torch.cat((x0, x1), dim=1)
    dw1, db1 = torch.full((out_f, K0 + K1), float("nan"), device=DEV), torch.full((out_f,), float("nan"), device=DEV)
    L.weight_grad_batch([L.WgItem(dy, cat, True, dw1, db1)])
    dw2, db2 = torch.full((out_f, K0 + K1), float("nan"), device=DEV), torch.full((out_f,), float("nan"), device=DEV)
    items = [L.WgItem(dy, x0, True, dw2[:, :K0], db2), L.WgItem(dy, x1, False, dw2[:, K0:], None)]
    L.weight_grad_batch(items)
    dw3 = torch.full((out_f, K0 + K1), float("nan"), device=DEV)
    L.weight_grad(dy, x0, False, dw_out=dw3[:, :K0])              # one by one: agnn_wgrad_f32 with a column block as destination
    L.weight_grad(dy, x1, False, dw_out=dw3[:, K0:])
    r64 = dy.double().t() @ cat.double()
    scale = float(r64.abs().max())
    for got, what in ((dw2, "two items"), (dw3, "two single launches")):
        assert float((got.double() - dw1.double()).abs().max()) <= 2e-6 * scale, what
        assert float((got.double() - r64).abs().max()) <= 2e-6 * scale, what
    assert torch.equal(db2, db1)
    assert float((db2.double() - dy.double().sum(0)).abs().max()) <= 2e-6 * float(dy.double().sum(0).abs().max())


def test_weight_gradient_in_two_128_column_multiples_has_the_bits_of_the_product_on_the_cat():
    """The step's case (K0 = K1 = 256): blocks that are multiples of the 128-column tile have the tiles of the concatenation, and
    the pair counts as one product when groups are formed — so beside other pending products every item gets the row slices it had
    with the input concatenated, and every gradient of the group its bits.  16 products, one of them in two blocks: one group."""
    from analysisgnn_amd import linear as L
    g = torch.Generator().manual_seed(7)
    n, out_f, K = 2500, 256, 256
    dy = torch.randn(n, out_f, generator=g).to(DEV)
    x0 = torch.randn(n, K + 8, generator=g).to(DEV)[:, :K]
    x1 = torch.randn(n, K + 20, generator=g).to(DEV)[:, :K]
    cat = torch.cat((x0, x1), dim=1)
    others = [(torch.randn(n, 64, generator=g).to(DEV), torch.randn(n, 128, generator=g).to(DEV)) for _ in range(15)]

    def run(pair):
        outs = [(torch.full((64, 128), float("nan"), device=DEV), torch.full((64,), float("nan"), device=DEV)) for _ in others]
        items = [L.WgItem(d, x, True, o[0], o[1]) for (d, x), o in zip(others, outs)]
        dw, db = torch.full((out_f, 2 * K), float("nan"), device=DEV), torch.full((out_f,), float("nan"), device=DEV)
        mine = ([L.WgItem(dy, x0, True, dw[:, :K], db), L.WgItem(dy, x1, False, dw[:, K:], None, follows=True)] if pair
                else [L.WgItem(dy, cat, True, dw, db)])
        L.weight_grad_batch(items[:7] + mine + items[7:])
        return [dw, db] + [t for o in outs for t in o]
    for a, b in zip(run(True), run(False)):
        assert torch.equal(a, b)


def test_linear2_forward_and_backward_equal_linear_on_the_cat():
    """encoders._finish's call: same output bits as `linear` on the concatenation, input gradients as views of one product,
    weight and bias gradients to fp32 rounding; operands the kernel does not take are declined (the caller concatenates)."""
    from analysisgnn_amd import linear as L
    g = torch.Generator().manual_seed(6)
    M, K0, K1, N_out = 4200, 256, 256, 256
    stack = torch.randn(M + 50, K0, generator=g).to(DEV)
    x0 = stack[:M].detach().requires_grad_(True)                 # a row slice of the stack's output
    x1 = torch.randn(M, K1, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(N_out, K0 + K1, generator=g) * 0.1).to(DEV).requires_grad_(True)
    b = torch.randn(N_out, generator=g).to(DEV).requires_grad_(True)
    dy = torch.randn(M, N_out, generator=g).to(DEV)
    y2 = L.linear2(x0, x1, w, b)
    assert y2 is not None
    y2.backward(dy)
    got = [t.grad.clone() for t in (x0, x1, w, b)]
    for t in (x0, x1, w, b):
        t.grad = None
    y1 = L.linear(torch.cat((x0, x1), dim=-1), w, b)
    y1.backward(dy)
    assert torch.equal(y2, y1)
    assert torch.equal(got[0], x0.grad) and torch.equal(got[1], x1.grad)
    for a, r in ((got[2], w.grad), (got[3], b.grad)):
        assert float((a.double() - r.double()).abs().max()) <= 2e-6 * float(r.double().abs().max())
    assert L.linear2(x0[:100], x1[:100], w, b) is None           # fewer than 4 096 rows
    assert L.linear2(x0[:, :250], x1, w[:, :506], b) is None      # a block that is no multiple of the k-step


# ---------------------------------------------------------------------------------------------------------------------
# pooling + cat + LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def _edges(batch_size):
    """[2, E] onset edges (messages from row 1 to row 0) over N notes: random pairs, self loops, duplicates, sources and
    destinations at or beyond batch_size, rows without a neighbour (250 .. 255 appear nowhere), one destination with 70 incoming
    edges and one source with 70 outgoing ones (more than the 64 ids a wave keeps in registers), (-1, -1) padding."""
    g = torch.Generator().manual_seed(11)
    dst = torch.randint(0, N, (500,), generator=g)
    src = torch.randint(0, N, (500,), generator=g)
    keep = ~(((dst >= 250) & (dst < 256)) | ((src >= 250) & (src < 256)))
    dst, src = dst[keep], src[keep]
    loops = torch.arange(0, N, 7)
    dup = torch.stack([dst[:40], src[:40]])
    many = torch.arange(100, 170)
    far = torch.tensor([[3, 4, 290, 299, 10], [280, 299, 3, 298, 257]])       # ends >= 257
    pad = torch.full((2, 9), -1, dtype=torch.long)
    e = torch.cat([torch.stack([dst, src]), torch.stack([loops, loops]), dup, torch.stack([torch.full_like(many, 5), many]),
                   torch.stack([many, torch.full_like(many, 7)]), far, pad], dim=1)
    return e[:, torch.randperm(e.shape[1], generator=g)].to(DEV)


def _reference64(x, edges, batch_size, gamma, beta, eps):
    """analysis.py:580-587 followed by LayerNorm(2H), float64, differentiable."""
    n = x.shape[0]
    dst, src = edges[0], edges[1]
    ok = (dst >= 0) & (src >= 0) & (dst < batch_size) & (src < batch_size) & (dst != src)
    dst, src = dst[ok], src[ok]
    n_pool = min(n, batch_size)
    acc = torch.zeros(n_pool, x.shape[1], dtype=torch.float64, device=x.device).index_add(0, dst, x[src])
    cnt = torch.zeros(n_pool, dtype=torch.float64, device=x.device).index_add(0, dst, torch.ones_like(dst, dtype=torch.float64))
    pooled = torch.cat([(x[:n_pool] + acc) / cnt.clamp(min=1.0).unsqueeze(1), x[n_pool:]], dim=0)
    u = torch.cat([x, pooled], dim=1)
    return u, F.layer_norm(u, (u.shape[1],), gamma, beta, eps)


class _Case:
    pass


@pytest.fixture(scope="module", params=[300, 257])
def case(request):
    """Everything the tests of one batch size share, computed once: the inputs, the three-launch path's results and gradients,
    the float64 reference's."""
    from analysisgnn_amd import fused, models
    c = _Case()
    c.bs = request.param
    g = torch.Generator().manual_seed(c.bs)
    c.x = torch.randn(N, H, generator=g).to(DEV)
    c.edges = _edges(c.bs)
    c.ln = torch.nn.LayerNorm(2 * H).to(DEV)
    with torch.no_grad():
        c.ln.weight.copy_(1.0 + 0.2 * torch.randn(2 * H, generator=g))
        c.ln.bias.copy_(0.1 * torch.randn(2 * H, generator=g))
    c.dy = torch.randn(N, 2 * H, generator=g).to(DEV)
    c.du = torch.randn(N, 2 * H, generator=g).to(DEV)
    # the old path: aggregate, cat, cat, k_na_fwd — and its backward
    x = c.x.clone().requires_grad_(True)
    u = models.onset_pool(x, c.edges, c.bs)
    y = fused.norm_act(u, c.ln)
    y.backward(c.dy)
    c.u_old, c.y_old = u.detach(), y.detach()
    c.g_old = (x.grad.clone(), c.ln.weight.grad.clone(), c.ln.bias.grad.clone())
    c.ln.weight.grad = c.ln.bias.grad = None
    x2 = c.x.clone().requires_grad_(True)
    models.onset_pool(x2, c.edges, c.bs).backward(c.du)         # the pooling's three backward launches alone, on a given du
    c.dx_old_du = x2.grad.clone()
    # float64
    x64 = c.x.double().requires_grad_(True)
    g64, b64 = c.ln.weight.detach().double().requires_grad_(True), c.ln.bias.detach().double().requires_grad_(True)
    u64, y64 = _reference64(x64, c.edges, c.bs, g64, b64, c.ln.eps)
    c.u64, c.y64 = u64.detach(), y64.detach()
    c.g64 = torch.autograd.grad(y64, (x64, g64, b64), c.dy.double(), retain_graph=True)
    c.du64_max = float(torch.autograd.grad(y64, u64, c.dy.double(), retain_graph=True)[0].abs().max())
    c.dx64_du = torch.autograd.grad(u64, x64, c.du.double())[0]
    torch.cuda.synchronize()
    return c


def _index(c):
    from analysisgnn_amd import models
    return models._onset_index(N, c.edges, c.bs, None)


def _pool_cat_norm(c, poison):
    from analysisgnn_amd import _lib
    lib = _lib.load()
    fwd, _ = _index(c)
    fill = float("nan") if poison else 0.0
    u, y = torch.full((N, 2 * H), fill, device=DEV), torch.full((N, 2 * H), fill, device=DEV)
    mean, rstd, inv = (torch.full((N,), fill, device=DEV) for _ in range(3))
    rel = _lib.make_rels([dict(src=None, rowptr=fwd.rowptr.data_ptr(), col=fwd.col.data_ptr(), ld_src=0)])
    gamma, beta = c.ln.weight.detach(), c.ln.bias.detach()
    _lib.check(lib.agnn_pool_cat_norm_f32(rel, c.x.data_ptr(), c.x.stride(0), N, min(N, c.bs), H, c.bs, gamma.data_ptr(), beta.data_ptr(), c.ln.eps,
                                          u.data_ptr(), u.stride(0), y.data_ptr(), y.stride(0), mean.data_ptr(), rstd.data_ptr(), inv.data_ptr(),
                                          _lib.stream_ptr(DEV)), "agnn_pool_cat_norm_f32")
    return u, y, mean, rstd, inv


def test_pool_cat_norm_forward(case):
    from analysisgnn_amd import _lib
    c = case
    u, y, mean, rstd, inv = _pool_cat_norm(c, poison=True)
    assert torch.equal(u, c.u_old)                               # x copied, pooled with the old kernel's summation order
    # k_na_fwd on that u
    lib = _lib.load()
    y_k = torch.empty_like(y)
    mean_k, rstd_k = torch.empty_like(mean), torch.empty_like(rstd)
    _lib.check(lib.agnn_norm_act_fwd_f32(u.data_ptr(), u.stride(0), c.ln.weight.data_ptr(), c.ln.bias.data_ptr(), 2 * H, N, 2 * H, c.ln.eps, 0.0, 0,
                                         None, 0, y_k.data_ptr(), y_k.stride(0), mean_k.data_ptr(), rstd_k.data_ptr(), None, _lib.stream_ptr(DEV)),
               "agnn_norm_act_fwd_f32")
    for got, ref, what in ((y, y_k, "y"), (mean, mean_k, "mean"), (rstd, rstd_k, "rstd"), (y, c.y_old, "y (old path)")):
        d = float((got - ref).abs().max())
        print(f"bs={c.bs} {what}: max |new - k_na_fwd| = {d:.3e}")
        assert torch.allclose(got, ref, rtol=RTOL, atol=ATOL), what
    # float64: u to one rounding of a mean of up to 71 terms, the LayerNorm to a few roundings of values of magnitude <= ~5
    assert torch.allclose(u.double(), c.u64, rtol=RTOL, atol=ATOL)
    m64 = c.u64.mean(1)
    r64 = 1.0 / torch.sqrt(c.u64.var(1, unbiased=False) + c.ln.eps)
    for got, ref, what in ((y, c.y64, "y"), (mean, m64, "mean"), (rstd, r64, "rstd")):
        print(f"bs={c.bs} {what}: max |new - float64| = {float((got.double() - ref).abs().max()):.3e}")
        assert torch.allclose(got.double(), ref, rtol=RTOL, atol=ATOL), what
    # 1 / count: rows beyond the pooled ones count as one
    assert bool((inv[min(N, c.bs):] == 1.0).all()) and bool(torch.isfinite(inv).all()) and float(inv.min()) < 0.02      # (71 valid neighbours somewhere)
    # a NaN-poisoned output buffer gives the same result as a zeroed one: every element is written, none is read
    for a, b in zip(_pool_cat_norm(c, poison=False), (u, y, mean, rstd, inv)):
        assert torch.equal(a, b)


def test_pool_cat_backward_in_one_launch(case):
    """dx = du[:, :H] + inv_cnt * du[:, H:] + sum over the destinations a row feeds — against the three launches it replaces
    (backward SpMM, accumulating self term, autograd's add) on the same du, and against float64 autograd."""
    from analysisgnn_amd import _lib
    c = case
    lib = _lib.load()
    _, bwd = _index(c)
    inv = _pool_cat_norm(c, poison=False)[4]
    dx = torch.full((N, H), float("nan"), device=DEV)
    rel = _lib.make_rels([dict(src=None, rowptr=bwd.rowptr.data_ptr(), col=bwd.col.data_ptr(), ld_src=0)])
    _lib.check(lib.agnn_pool_cat_bwd_f32(rel, c.du.data_ptr(), c.du.stride(0), inv.data_ptr(), N, min(N, c.bs), H, dx.data_ptr(), dx.stride(0),
                                         _lib.stream_ptr(DEV)), "agnn_pool_cat_bwd_f32")
    print(f"bs={c.bs} dx: max |new - old| = {float((dx - c.dx_old_du).abs().max()):.3e}, max |new - float64| = {float((dx.double() - c.dx64_du).abs().max()):.3e}")
    assert torch.allclose(dx, c.dx_old_du, rtol=RTOL, atol=ATOL)
    assert torch.equal(dx, c.dx_old_du)                          # the three terms are summed in the old launches' order, each step rounded
    assert torch.allclose(dx.double(), c.dx64_du, rtol=RTOL, atol=ATOL)


def test_join_node_gradients(case):
    """models.pool_cat_norm + FusedSequential(pre=...): dx, dgamma, dbeta of the whole block against the old path's nodes at
    rtol 1e-5 / atol 1e-6 and against float64 autograd.  Against float64 the absolute term is the bound of the fp32 sums behind
    each result, terms * 2^-24 * the largest addend, on top of rtol (the addends cancel: a sum can be far smaller than the terms
    that went into it): 300 rows for the column sums dgamma / dbeta; the 2H = 512 columns of the LayerNorm backward's two row
    means for dx, taken relative to the largest du (the pooling's own sums are far shorter)."""
    from analysisgnn_amd import fused, models
    c = case
    x = c.x.clone().requires_grad_(True)
    joined = models.pool_cat_norm(x, c.edges, c.bs, c.ln)
    assert joined is not None
    u, pre = joined
    seq = fused.FusedSequential(c.ln)
    y = seq(u, pre=pre)
    assert torch.equal(u, c.u_old) and y.data_ptr() == pre[0].data_ptr()
    y.backward(c.dy)
    got = (x.grad.clone(), c.ln.weight.grad.clone(), c.ln.bias.grad.clone())
    c.ln.weight.grad = c.ln.bias.grad = None
    xhat = (c.u64 - c.u64.mean(1, keepdim=True)) / torch.sqrt(c.u64.var(1, unbiased=False, keepdim=True) + c.ln.eps)
    colsum_atol = N * 2.0 ** -24 * max(float((c.dy.double() * xhat).abs().max()), float(c.dy.abs().max()))
    dx_atol = 2 * H * 2.0 ** -24 * c.du64_max
    for a, old, r64, what, atol64 in zip(got, c.g_old, c.g64, ("dx", "dgamma", "dbeta"), (dx_atol, colsum_atol, colsum_atol)):
        print(f"bs={c.bs} {what}: max |new - old| = {float((a - old).abs().max()):.3e}, max |new - float64| = {float((a.double() - r64).abs().max()):.3e}")
        assert torch.allclose(a, old, rtol=RTOL, atol=ATOL), what
        assert torch.allclose(a.double(), r64, rtol=RTOL, atol=atol64), what


def test_pool_cat_norm_declines_other_widths():
    from analysisgnn_amd import models
    x = torch.randn(50, 32, device=DEV)
    e = torch.randint(0, 50, (2, 80), device=DEV)
    assert models.pool_cat_norm(x, e, 50, torch.nn.LayerNorm(64).to(DEV)) is None
    assert models.pool_cat_norm(torch.randn(50, 256, device=DEV), e, 0, torch.nn.LayerNorm(512).to(DEV)) is None     # no pooled row


# ---------------------------------------------------------------------------------------------------------------------
# whole model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc,hidden", [("hybridgnn", 256), ("hgt", 32)])
def test_model_with_the_join_block_fused_equals_the_three_launch_model(enc, hidden, monkeypatch):
    """TorchAnalysisGNN on two 60-note neighbour-sampled subgraphs: loss and every gradient with the switches on against off
    at 1e-4 (the wrapper tests' tolerance).  H = 256 takes the fused launches; H = 32 (hgt) must decline them and fall back."""
    from analysisgnn_amd import encoders, graph, models
    from analysisgnn_amd.heads import MultiTaskLoss, training_loss
    from analysisgnn_amd.synth import make_score_graph, merge_sampled, sample_hops, torch_inputs
    tasks = {"cadence": 4, "localkey": 50, "hrythm": 2}
    g = merge_sampled([sample_hops(make_score_graph(seed=sd, n_notes=200), 60, (5, 5), seed=sd, first_target=20) for sd in (1, 2)])
    I = torch_inputs(g, 25, DEV, seed=0)
    labels = torch.stack([torch.randint(0, c, (I["batch_size"],), generator=torch.Generator().manual_seed(i)).to(DEV)
                          for i, c in enumerate(tasks.values())])
    torch.manual_seed(0)
    model = models.TorchAnalysisGNN(g.metadata(), 25, hidden, 128, tasks, 2, dropout=0.0, use_jk=False, logit_fusion=False, encoder_type=enc).to(DEV).train()
    clf = MultiTaskLoss(list(tasks)).to(DEV)
    taken = []
    real = models.pool_cat_norm
    monkeypatch.setattr(models, "pool_cat_norm", lambda *a, **k: (taken.append(real(*a, **k)), taken[-1])[1])
    was = graph.index_cache_enabled
    graph.index_cache_enabled = False

    def run(on):
        monkeypatch.setattr(models, "JOIN_FUSED", on)
        monkeypatch.setattr(encoders, "CAT_PROJ_TWO_OPERANDS", on)
        model.zero_grad(set_to_none=True)
        x = model.encode(I["pitch_spelling"], I["key_signature"], I["x_dict"], I["edge_index_dict"], I["batch_dict"], I["batch_size"],
                         I["neighbor_mask_node"], I["neighbor_mask_edge"])
        logits, offs, _ = model.forward_clf_fused(x)
        loss, _ = training_loss(logits, offs, labels, x, 0.1, 0.1, -1, task_params=clf.weights())
        loss.backward()
        return float(loss), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    try:
        l_on, g_on = run(True)
        assert len(taken) == 1 and (taken[0] is not None) == (hidden == 256)
        l_off, g_off = run(False)
        assert len(taken) == 1
    finally:
        graph.index_cache_enabled = was
    assert abs(l_on - l_off) <= 1e-4 * abs(l_off), (l_on, l_off)
    assert g_on.keys() == g_off.keys() and len(g_on) > 20
    for k in g_off:
        assert_close_rel(g_on[k], g_off[k], 1e-4, f"grad {k}", floor=1e-9)
