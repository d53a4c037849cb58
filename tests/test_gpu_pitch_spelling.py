"""GraphNorm and the pitch-spelling models on the GPU (analysisgnn_amd/pitch_spelling.py; csrc/graphnorm.hip).

Gates are the project's own (tests/test_gpu_chord.py): GATE 1e-4 x max-abs of the compared tensor end to end, TIGHT
1e-5 x max-abs for a kernel alone on float64-exact inputs.  The kernel's y and all five gradients are held against TIGHT x their
own max-abs at n in {127, 128, 129, 300} and on the ill-conditioned column.  At n in {1, 2} every graph has one or two rows and
every entry of dx = do - mean_scale * mean_g(do) and of dmean_scale = -sum_g n_g m_g mean_g(do) is a difference whose terms cancel
down to eps * rstd^2 of their size; an fp32 evaluation, whose rounding error is a few ulp of the terms, cannot be held against the
result of such a difference, so there (and only there) these two are held against TIGHT x the size of their TERMS
(pitch_spelling_ref.grad_term_scales), as tests/test_gpu_chord.py holds the BatchNorm block's dx at two rows.  dweight where it is
exactly zero (every ohat is: one-row graphs with mean_scale = 1) is held against TIGHT x max|dy|.

The kernel against the float64 restatement (tests/pitch_spelling_ref.graph_norm, gradients by autograd) at every size where its
code takes another path: one row, a slab of 128 positions and its neighbours, more slabs than one, graphs of one row, an empty
graph id, an unsorted batch vector, column tiles of 64 with remainders, a strided x."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pitch_spelling_ref as PR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE, TIGHT = 1e-4, 1e-5


def close(got, exp, tol, what, scale=None):
    got, exp = got.detach().double().cpu(), exp.detach().double().cpu()
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if exp.numel() == 0:
        return
    s = float(exp.abs().max()) if scale is None else scale
    err = float((got - exp).abs().max())
    print(f"{what}: err {err:.3e}  bound {tol * s:.3e}")
    assert err <= tol * s, (what, err, tol * s)


def ps():
    from analysisgnn_amd import pitch_spelling
    return pitch_spelling


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
def gn_run(x, w, b, ms, batch, G, dy):
    """(y, dx, dw, db, dms) of the HIP path; x may be a strided view."""
    mod = ps()
    seg = mod.graph_segments(batch.to(DEV), G)
    leaves = [t.detach().requires_grad_(True) for t in (x, w, b, ms)]
    y = mod.graph_norm(*leaves, seg)
    grads = torch.autograd.grad((y * dy).sum(), leaves)
    return (y.detach(), *grads)


def close_each(got, exp, tol, scale, what):
    """Element by element (or column by column) against a scale of the same shape."""
    got, exp = got.detach().double().cpu(), exp.detach().double().cpu()
    assert got.shape == exp.shape == scale.shape, (what, got.shape, exp.shape, scale.shape)
    if exp.numel() == 0:
        return
    err = (got - exp).abs()
    worst = int((err / scale.clamp(min=1e-300)).argmax())
    print(f"{what}: worst element {worst}: err {float(err.flatten()[worst]):.3e}  bound {tol * float(scale.flatten()[worst]):.3e}")
    assert bool((err <= tol * scale).all()), (what, worst, float(err.flatten()[worst]), tol * float(scale.flatten()[worst]))


def gn_check(x, w, b, ms, batch, G, dy, what, cancelled=False):
    """`cancelled`: every graph has at most two rows (n in {1, 2}): dx and dmean_scale against the size of their terms."""
    got = gn_run(x, w, b, ms, batch, G, dy)
    exp = PR.graph_norm_grads(x.cpu(), w.cpu(), b.cpu(), ms.cpu(), batch, G, dy.cpu())
    close(got[0], exp[0], TIGHT, f"{what} y")
    if cancelled:
        dx_scale, dms_scale = PR.grad_term_scales(x, w, ms, batch, G, dy)
        close_each(got[1], exp[1], TIGHT, dx_scale, f"{what} dx")
        close_each(got[4], exp[4], TIGHT, dms_scale, f"{what} dmean_scale")
    else:
        close(got[1], exp[1], TIGHT, f"{what} dx")
        close(got[4], exp[4], TIGHT, f"{what} dmean_scale")
    # dweight = sum g * ohat is exactly zero where every ohat is (one-row graphs with mean_scale = 1): held against the terms there too
    own = float(exp[2].abs().max())
    close(got[2], exp[2], TIGHT, f"{what} dweight", own if own > 0 else float(dy.abs().max()))
    close(got[3], exp[3], TIGHT, f"{what} dbias")


@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 300])
def test_graphnorm_kernel(n):
    gen = torch.Generator().manual_seed(100 + n)
    for sname, (batch, G) in PR.segmentations(n).items():
        for C in (4, 36, 64, 68, 260):
            for unit in (False, True):
                wide = torch.randn(n, C + 8, generator=gen).to(DEV)
                w = (1.0 + 0.3 * torch.randn(C, generator=gen)).to(DEV)
                b = (0.3 * torch.randn(C, generator=gen)).to(DEV)
                ms = torch.ones(C, device=DEV) if unit else (0.5 + torch.rand(C, generator=gen)).to(DEV)
                dy = torch.randn(n, C, generator=gen).to(DEV)
                for strided in (False, True):              # dense, and the same values as a column window of a wider matrix
                    x = wide[:, 4:4 + C] if strided else wide[:, 4:4 + C].contiguous()
                    gn_check(x, w, b, ms, batch, G, dy, f"n={n} {sname} C={C} mean_scale={'1' if unit else 'drawn'} strided={strided}",
                             cancelled=n <= 2)


def test_graphnorm_ill_conditioned_column():
    """mean 1e3, std 1e-2, mean_scale = 1: the plain fp32 composition is 0.9 % of max-abs off its float64 value; the two-float shift
    must meet TIGHT."""
    gen = torch.Generator().manual_seed(5)
    n, C = 300, 8
    x = (1e3 + 1e-2 * torch.randn(n, C, generator=gen)).float().to(DEV)
    w, b, ms = (1.0 + 0.3 * torch.randn(C, generator=gen)).to(DEV), torch.randn(C, generator=gen).to(DEV), torch.ones(C, device=DEV)
    dy = torch.randn(n, C, generator=gen).to(DEV)
    for sname in ("single", "1_170_129", "unsorted"):
        batch, G = PR.segmentations(n)[sname]
        gn_check(x, w, b, ms, batch, G, dy, f"ill-conditioned {sname}")


def test_graphnorm_deterministic_and_capturable():
    gen = torch.Generator().manual_seed(9)
    n, C = 300, 68
    batch, G = PR.segmentations(n)["unsorted"]
    x, dy = torch.randn(n, C, generator=gen).to(DEV), torch.randn(n, C, generator=gen).to(DEV)
    w, b, ms = [(1.0 + 0.2 * torch.randn(C, generator=gen)).to(DEV) for _ in range(3)]
    first = gn_run(x, w, b, ms, batch, G, dy)
    second = gn_run(x, w, b, ms, batch, G, dy)
    for a, c in zip(first, second):
        assert torch.equal(a, c)
    mod = ps()
    seg = mod.graph_segments(batch.to(DEV), G)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b, ms)]

    def step():
        for t in leaves:
            t.grad = None
        y = mod.graph_norm(*leaves, seg)
        (y * dy).sum().backward()
        return y
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                             # the warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        y = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), first[0])
    for t, e in zip(leaves, first[1:]):
        assert torch.equal(t.grad, e)


def test_graphnorm_module():
    mod = ps()
    m = mod.GraphNorm(8).to(DEV)
    assert [k for k, _ in m.named_parameters()] == ["weight", "bias", "mean_scale"]
    assert float(m.weight.detach().min()) == 1 and float(m.bias.detach().abs().max()) == 0 and float(m.mean_scale.detach().min()) == 1
    x = torch.randn(5, 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    batch = torch.tensor([0, 0, 1, 1, 1], device=DEV)
    y_train = m.train()(x, batch)
    y_eval = m.eval()(x, batch)
    assert torch.equal(y_train, y_eval)                    # the same function
    assert torch.equal(m(x, mod.graph_segments(batch, 2)), y_train) and torch.equal(m(x, batch, batch_size=2), y_train)
    close(m(x), PR.graph_norm(x.cpu().double(), *[p.detach().cpu().double() for p in m.parameters()], None), TIGHT, "batch=None")
    one = m(x[:1], torch.zeros(1, dtype=torch.long, device=DEV))
    assert torch.equal(one, m.bias.detach().expand(1, 8))  # a one-row graph with mean_scale = 1
    twin = copy.deepcopy(m)
    assert torch.equal(twin(x, batch), y_train)
    mod.clear_segment_cache()


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
def build(name, dropout=0.0):
    mod = ps()
    z = PR.load_case(name)
    cfg = PR.config(z)
    if cfg["kind"] == "pkspell":
        model = mod.PKSpell(cfg["in_feats"], cfg["h1"], cfg["h2"], PR.OUT_PC, rnn_depth=cfg["depth"], dropout=dropout, cell_type=cfg["cell"])
    elif cfg["kind"] == "psgnn":
        model = mod.PitchSpellingGNN(cfg["in_feats"], cfg["H"], PR.ENC, PR.OUT_PC, PR.OUT_KS, cfg["L"], cfg["metadata"], dropout=dropout,
                                     add_seq=cfg["add_seq"])
    else:
        model = mod.PitchSpellingNeighborGNN(cfg["in_feats"], cfg["H"], PR.ENC, PR.OUT_PC, PR.OUT_KS, cfg["L"], cfg["metadata"], dropout=dropout)
    model.load_state_dict(PR.state(z), strict=True)
    return model.to(DEV).train(), z, cfg, PR.inputs(z, DEV)


def call(model, cfg, I, x, **kw):
    if cfg["kind"] == "pkspell":
        return model(x, I["lens"])
    xd = dict(I["x_dict"], note=x)
    if cfg["kind"] == "psgnn":
        return model(xd, I["ei_dict"], I["mask_node"], I["mask_edge"], I["batch"], **kw)
    return model(xd, I["ei_dict"], I["edges_per_hop"], I["nodes_per_hop"])


def note_input(cfg, I):
    return (I["x"] if cfg["kind"] == "pkspell" else I["x_dict"]["note"]).clone().requires_grad_(True)


@pytest.mark.parametrize("name", PR.CASES)
def test_goldens(name):
    model, z, cfg, I = build(name)
    keep = {}
    hook = None
    if cfg["kind"] != "pkspell":
        hook = model.normalize.register_forward_hook(lambda m, a, o: keep.update({"mid.norm_in": a[0].detach(), "mid.norm_out": o.detach()}))
    x = note_input(cfg, I)
    out_pc, out_ks = call(model, cfg, I, x)
    ((out_pc * torch.from_numpy(z["cot.pc"]).to(DEV)).sum() + (out_ks * torch.from_numpy(z["cot.ks"]).to(DEV)).sum()).backward()
    if hook is not None:
        hook.remove()
    close(out_pc, torch.from_numpy(z["out.pc"]), GATE, f"{name} out.pc")
    close(out_ks, torch.from_numpy(z["out.ks"]), GATE, f"{name} out.ks")
    for k, v in keep.items():
        close(v, torch.from_numpy(z[k]), GATE, f"{name} {k} (inside the model)")
    close(x.grad, torch.from_numpy(z["grad.x"]), GATE, f"{name} grad.x")
    zero = set(str(k) for k in z["meta.zero_grads"])    # zero in exact arithmetic (the bias in front of the BatchNorm, lin_l of a layer
    without = set()                                     # without edges): held against the largest weight gradient's max-abs
    for k, p in model.named_parameters():
        if p.grad is None:
            without.add(k)
            continue
        assert "gw." + k in z, f"{k} has a gradient the reference does not give"
        close(p.grad, torch.from_numpy(z["gw." + k]), GATE, f"{name} gw.{k}", float(z["meta.grad_max"]) if "gw." + k in zero else None)
    assert without == set(str(k) for k in z["meta.no_grad"])


@pytest.mark.parametrize("name", ["psgnn_h32", "psgnn_seq_h32"])
def test_graphnorm_alone_on_the_fixture(name):
    model, z, cfg, I = build(name)
    y = model.normalize(torch.from_numpy(z["mid.norm_in"]).float().to(DEV), I["batch"])
    close(y, torch.from_numpy(z["mid.norm_out"]), TIGHT, f"{name} GraphNorm alone")


# ---- models at kernel sizes ---------------------------------------------------------------------------------------------------------
def _bf16_weights(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=gen) * 0.1)
            p.copy_(p.bfloat16().float())


def _against_restatement(model, cfg, I, tol, what, **kw):
    """Outputs, grad.x and every weight gradient of the HIP model against the float64 restatement on the same state_dict."""
    gen = torch.Generator().manual_seed(31)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    Icpu = {k: (v.cpu() if torch.is_tensor(v) else ({a: (b.cpu() if torch.is_tensor(b) else b) for a, b in v.items()} if isinstance(v, dict) else v))
            for k, v in I.items()}
    x = note_input(cfg, I)
    out_pc, out_ks = call(model, cfg, I, x, **kw)
    cot_pc, cot_ks = torch.randn(out_pc.shape, generator=gen), torch.randn(out_ks.shape, generator=gen)
    ((out_pc * cot_pc.to(DEV)).sum() + (out_ks * cot_ks.to(DEV)).sum()).backward()
    rec = PR.run_params(sd, cfg, Icpu, cot_pc, cot_ks)
    close(out_pc, rec["out.pc"], tol, f"{what} out.pc")
    close(out_ks, rec["out.ks"], tol, f"{what} out.ks")
    close(x.grad, rec["grad.x"], tol, f"{what} grad.x")
    for k, p in model.named_parameters():
        if p.grad is not None:
            close(p.grad, rec["gw." + k], tol, f"{what} gw.{k}")
        else:
            assert "gw." + k not in rec, k
    return out_pc.detach(), out_ks.detach()


def test_pkspell_on_the_persistent_gru_kernels():
    from analysisgnn_amd import gru
    torch.manual_seed(3)
    cfg = dict(kind="pkspell", in_feats=8, h1=128, h2=128, depth=1, cell="GRU")
    model = ps().PKSpell(8, 128, 128, PR.OUT_PC, dropout=0.0)
    assert gru.kernel_applicable(model.rnn) and gru.kernel_applicable(model.rnn2)
    _bf16_weights(model, 4)
    model = model.to(DEV).train()
    I = dict(x=torch.randn(19, 8, generator=torch.Generator().manual_seed(5)).to(DEV), lens=[11, 7, 1])
    _against_restatement(model, cfg, I, GATE, "PKSpell 128/128")


def _wide_gnn(add_seq):
    model, z, cfg, I = build("psgnn_seq_h32" if add_seq else "psgnn_h32")
    cfg = dict(cfg, H=128)
    torch.manual_seed(7)
    model = ps().PitchSpellingGNN(cfg["in_feats"], 128, PR.ENC, PR.OUT_PC, PR.OUT_KS, cfg["L"], cfg["metadata"], dropout=0.0, add_seq=add_seq)
    _bf16_weights(model, 8)
    return model.to(DEV).train(), cfg, I


def test_pitch_spelling_gnn_with_sequences_at_128():
    model, cfg, I = _wide_gnn(True)
    pc, ks = _against_restatement(model, cfg, I, GATE, "PitchSpellingGNN(add_seq) H=128")
    lens = torch.bincount(I["batch"]).tolist()
    x = note_input(cfg, I)
    pc2, ks2 = call(model, cfg, I, x, lengths=lens)        # host ints: the same bits as the tensor path
    assert torch.equal(pc2, pc) and torch.equal(ks2, ks)


# ---- heads and outputs --------------------------------------------------------------------------------------------------------------
def test_heads_fused_logits_loss_and_metrics():
    from analysisgnn_amd.metrics import MultiTaskMetrics
    mod = ps()
    model, cfg, I = _wide_gnn(False)
    xd = I["x_dict"]
    with torch.no_grad():
        out_pc, out_ks = model(xd, I["ei_dict"], I["mask_node"], I["mask_edge"], I["batch"])
        logits, offs = model.forward_fused(xd, I["ei_dict"], I["mask_node"], I["mask_edge"], I["batch"])
    assert offs == [0, PR.OUT_PC, PR.OUT_PC + PR.OUT_KS] and tuple(logits.shape) == (out_pc.shape[0], offs[-1])
    assert torch.equal(logits[:, :PR.OUT_PC], out_pc) and torch.equal(logits[:, PR.OUT_PC:], out_ks)
    # backward through the side-by-side matrix: the same gradients as through the two blocks
    cot = torch.randn(logits.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    grads = []
    for fused_path in (False, True):
        for p in model.parameters():
            p.grad = None
        if fused_path:
            lg, _ = model.forward_fused(xd, I["ei_dict"], I["mask_node"], I["mask_edge"], I["batch"])
            (lg * cot).sum().backward()
        else:
            a, b = model(xd, I["ei_dict"], I["mask_node"], I["mask_edge"], I["batch"])
            ((a * cot[:, :PR.OUT_PC]).sum() + (b * cot[:, PR.OUT_PC:]).sum()).backward()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 10
    for k in grads[0]:
        own = float(grads[0][k].abs().max())
        close(grads[1][k], grads[0][k], TIGHT, f"forward_fused gw.{k}", own if own > 0 else 1.0)
    # the key-signature head without the concatenation against the concatenated product, in float64
    x = torch.randn(out_pc.shape[0], PR.ENC, generator=torch.Generator().manual_seed(2)).to(DEV)
    with torch.no_grad():
        pc, ks, _ = model._both(x)
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    h = F.relu(torch.cat([x.cpu().double(), pc.cpu().double()], dim=1) @ sd["mlp_clf_ks.0.weight"].t() + sd["mlp_clf_ks.0.bias"])
    h = F.layer_norm(h, (h.shape[1],), sd["mlp_clf_ks.2.weight"], sd["mlp_clf_ks.2.bias"], 1e-5)
    close(ks, h @ sd["mlp_clf_ks.4.weight"].t() + sd["mlp_clf_ks.4.bias"], TIGHT, "out_ks without the concatenation")
    # loss and metrics on the side-by-side logits
    gen = torch.Generator().manual_seed(3)
    N = logits.shape[0]
    labels = torch.stack([torch.randint(0, PR.OUT_PC, (N,), generator=gen), torch.randint(0, PR.OUT_KS, (N,), generator=gen)])
    labels[0, 3] = -1
    loss = mod.pitch_spelling_loss(logits, offs, labels.to(DEV))
    ref = (F.cross_entropy(out_pc.cpu().double(), labels[0], ignore_index=-1) + F.cross_entropy(out_ks.cpu().double(), labels[1], ignore_index=-1))
    close(loss, ref, TIGHT, "pitch_spelling_loss")
    mt = MultiTaskMetrics(["ps", "ks"], offs, gate_task=None, joint=None, device=DEV)
    mt.update(logits, labels.to(DEV))
    res = mt.compute()
    for i, (t, o) in enumerate((("ps", out_pc), ("ks", out_ks))):
        pred, lab = o.argmax(dim=1).cpu().numpy(), labels[i].numpy()
        valid = lab >= 0
        assert abs(res["acc"][t] - float((pred[valid] == lab[valid]).mean())) < 1e-12, t
        f1 = []
        for c in range(o.shape[1]):
            tp = int(((pred == c) & (lab == c) & valid).sum())
            fp, fn = int(((pred == c) & (lab != c) & valid).sum()), int(((pred != c) & (lab == c) & valid).sum())
            if tp + fp + fn:
                f1.append(2 * tp / (2 * tp + fp + fn))
        assert abs(res["f1"][t] - float(np.mean(f1))) < 1e-9, (t, res["f1"][t], float(np.mean(f1)))


# ---- module behaviour ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pkspell_h16", "psneighbor_h32"])
def test_state_dict_round_trip_and_deepcopy(name):
    model, z, cfg, I = build(name)
    ref_sd = {str(k): torch.from_numpy(np.asarray(z["w." + str(k)])) for k in z["meta.keys"]}
    model.load_state_dict(ref_sd, strict=True)
    back = model.state_dict()
    assert list(back.keys()) == list(ref_sd.keys())       # the reference's keys, in the reference's order
    for k, v in ref_sd.items():
        assert torch.equal(back[k].cpu(), v.to(back[k].dtype)), k
    twin = copy.deepcopy(model).eval()
    model.eval()
    with torch.no_grad():
        a, b = call(model, cfg, I, note_input(cfg, I).detach()), call(twin, cfg, I, note_input(cfg, I).detach())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_pkspell_dropout_and_predict():
    model, z, cfg, I = build("pkspell_h16", dropout=0.5)
    from analysisgnn_amd import pitch_spelling
    model.train()
    seen = {}
    hooks = [model.top_layer_pitch.register_forward_pre_hook(lambda m, a: seen.__setitem__("pitch", a[0].detach())),
             model.top_layer_ks.register_forward_pre_hook(lambda m, a: seen.__setitem__("ks", a[0].detach()))]
    big = torch.randn(40 * 50, cfg["in_feats"], generator=torch.Generator().manual_seed(6)).to(DEV)      # 40 sentences of 50: 2000 x 16 / x 8 elements
    model(big, [50] * 40)
    for h in hooks:
        h.remove()
    with torch.no_grad():                                                                     # what the model's RNNs give without dropout
        h1 = pitch_spelling._rnn(model.rnn, big.view(40, 50, -1), True)
        h2 = pitch_spelling._rnn(model.rnn2, seen["pitch"], True)
    for name, h in (("pitch", h1), ("ks", h2)):
        d = seen[name]
        kept = d != 0
        assert abs(float(kept.float().mean()) - 0.5) <= 4 * 0.5 / np.sqrt(d.numel()), name    # 4 sigma of a fair coin over the elements
        assert bool((h != 0).all()) and torch.equal(d[kept], (2.0 * h)[kept]), name           # kept values scaled by 1 / (1 - p) = 2
    model.train()
    a, _ = model(I["x"], I["lens"])
    b, _ = model(I["x"], I["lens"])
    assert not torch.equal(a, b)                                                              # a fresh mask per training forward
    model.eval()
    pitch, ks = model.predict(I["x"], I["lens"])
    with torch.no_grad():
        sp, sk = model(I["x"], I["lens"])
    for i, l in enumerate(I["lens"]):                                                         # row i's first l entries
        assert pitch[i].shape == (l,) and np.array_equal(pitch[i], sp[i, :l].argmax(dim=1).cpu().numpy())
        assert ks[i].shape == (l,) and np.array_equal(ks[i], sk[i, :l].argmax(dim=1).cpu().numpy())
    tp = torch.randint(0, PR.OUT_PC + 1, sp.shape[:2], generator=torch.Generator().manual_seed(1)).to(DEV)      # out_feats = ignored
    tk = torch.randint(0, 16, sk.shape[:2], generator=torch.Generator().manual_seed(2)).to(DEV)
    loss = model.loss_computation(sp, sk, tp, tk)
    ref = (F.cross_entropy(sp.reshape(-1, PR.OUT_PC).double(), tp.reshape(-1), ignore_index=PR.OUT_PC)
           + F.cross_entropy(sk.reshape(-1, 15).double(), tk.reshape(-1), ignore_index=15))
    close(loss, ref, TIGHT, "PKSpell.loss_computation")
