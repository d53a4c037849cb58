"""The cadence models' join (csrc/pooljoin.hip: agnn_pool_norm_f32, agnn_pool_bwd_f32; cadence.pool_norm) and the two models on the GPU.

Gates are tests/test_gpu_cadence.py's: TIGHT 1e-5 x max-abs for a kernel alone against float64 on bf16-valued inputs, GATE 1e-4 x
max-abs end to end.  The float64 side is tests/cadence_ref.py (gradients by autograd); a reference is computed once per case and
shared.  The (n, H) pairs sit at the edges the kernels have: 4 rows per workgroup, the grid rounded to 8 workgroups, 256-float
chunks (1, 2 or 4 of them), lanes partly outside the row."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import cadence_ref as CR
import helpers

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE, TIGHT = 1e-4, 1e-5
PAIRS = [(1, 4), (3, 4), (5, 16), (63, 252), (64, 256), (65, 260), (257, 512), (1000, 1024), (6, 1020)]
MODELS = ["neighbor_h32", "pytorch_h32", "pytorch_ps_h32", "pytorch_hybrid_h32", "pytorch_eval_h32"]


def close(got, exp, tol, what, scale=None):
    got, exp = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(exp).detach().double().cpu()
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if exp.numel() == 0:
        return
    s = float(exp.abs().max()) if scale is None else scale
    err = float((got - exp).abs().max())
    print(f"{what}: err {err:.3e}  bound {tol * s:.3e}")
    assert err <= tol * s, (what, err, tol * s)


def cad():
    from analysisgnn_amd import cadence
    return cadence


def bf16(*shape, gen, scale=1.0, shift=0.0):
    return (shift + scale * torch.randn(*shape, generator=gen)).bfloat16().float()


def configs(n):
    m = max(n - 2, 1)
    return [(n, n, False), (n, n, True), (m, m, True)]


# ---- the kernels' float64 side, once per case ---------------------------------------------------------------------------------------
def hub_graph(n=80, hub=5, deg=70):
    src, dst = CR.join_graph(n)
    extra = torch.arange(deg) % n
    return torch.cat([src, extra]), torch.cat([dst, torch.full((deg,), hub)])


@functools.lru_cache(maxsize=None)
def case(n, H, pool_rows, col_limit, skip_self, hub=False):
    """Inputs (bf16-valued, CPU fp32) and everything float64 says about them: the forward's five results, the gradients of
    <y, cot> in x, gamma, beta, and the pooling's backward of `cot` from its own formula."""
    gen = torch.Generator().manual_seed(31 * n + H)
    src, dst = hub_graph(n) if hub else CR.join_graph(n)
    x, gamma, beta, cot = bf16(n, H, gen=gen), bf16(H, gen=gen, scale=0.5, shift=1.0), bf16(H, gen=gen, scale=0.5), bf16(n, H, gen=gen)
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    u, y, mean, rstd, inv = CR.pool_norm(x64, src, dst, pool_rows, col_limit, skip_self, g64, b64)
    grads = torch.autograd.grad((y * cot.double()).sum(), [x64, g64, b64])
    pb = CR.pool_bwd(cot.double(), src, dst, inv.detach(), pool_rows, col_limit, skip_self)
    ref = dict(u=u, y=y, mean=mean, rstd=rstd, inv=inv, dx=grads[0], dgamma=grads[1], dbeta=grads[2], pool_bwd=pb)
    return dict(x=x, gamma=gamma, beta=beta, cot=cot, src=src, dst=dst), {k: v.detach() for k, v in ref.items()}


def raw_fwd(x, ix, pool_rows, col_limit, skip_self, gamma, beta, rowend=None):
    """(u, y, mean, rstd, inv_cnt) straight from agnn_pool_norm_f32; x is read where it lies."""
    from analysisgnn_amd import _lib
    n, H = x.shape
    u, y = torch.full((n, H), float("nan"), device=DEV), torch.full((n, H), float("nan"), device=DEV)
    mean, rstd, inv = (torch.full((n,), float("nan"), device=DEV) for _ in range(3))
    rel = _lib.make_rels([dict(src=None, rowptr=ix.by_dst.rowptr.data_ptr(), col=ix.by_dst.col.data_ptr(), ld_src=0, rowend=_lib.ptr(rowend))])
    _lib.check(_lib.load().agnn_pool_norm_f32(rel, x.data_ptr(), x.stride(0), n, pool_rows, H, col_limit, 2 if skip_self else 0, gamma.data_ptr(),
                                              beta.data_ptr(), 1e-5, u.data_ptr(), H, y.data_ptr(), H, mean.data_ptr(), rstd.data_ptr(),
                                              inv.data_ptr(), _lib.stream_ptr(x.device)), "agnn_pool_norm_f32")
    torch.cuda.synchronize()
    return u, y, mean, rstd, inv


def raw_bwd(du, ix, inv, pool_rows, col_limit, skip_self, rowend=None):
    from analysisgnn_amd import _lib
    n, H = du.shape
    dx = torch.full((n, H), float("nan"), device=DEV)
    rel = _lib.make_rels([dict(src=None, rowptr=ix.by_src.rowptr.data_ptr(), col=ix.by_src.col.data_ptr(), ld_src=0, rowend=_lib.ptr(rowend))])
    _lib.check(_lib.load().agnn_pool_bwd_f32(rel, du.data_ptr(), du.stride(0), inv.data_ptr(), n, pool_rows, H, col_limit, 2 if skip_self else 0,
                                             dx.data_ptr(), H, _lib.stream_ptr(du.device)), "agnn_pool_bwd_f32")
    torch.cuda.synchronize()
    return dx


def check_forward(I, ref, got, what):
    u, y, mean, rstd, inv = got
    H = I["x"].shape[1]
    close(u, ref["u"], TIGHT, what + " u")
    close(y, ref["y"], TIGHT, what + " y")
    assert torch.equal(inv.cpu(), ref["inv"].float()), what + " inv_cnt"
    # a mean's fp32 error is a rounding of the ROW: at one row its own max-abs can be arbitrarily small
    close(mean, ref["mean"], TIGHT, what + " mean", max(float(ref["mean"].abs().max()), float(ref["u"].abs().max()) / H ** 0.5))
    close(rstd, ref["rstd"], TIGHT, what + " rstd")


def layer_norm(gamma, beta):
    ln = nn.LayerNorm(gamma.shape[0]).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(gamma)
        ln.bias.copy_(beta)
    return ln


def run_join(I, pool_rows, col_limit, skip_self, index=None):
    """(y, dx, dgamma, dbeta) of cadence.pool_norm and the backward of <y, cot>."""
    x = I["x"].to(DEV).requires_grad_(True)
    ln = layer_norm(I["gamma"], I["beta"])
    y = cad().pool_norm(x, I["src"].to(DEV), I["dst"].to(DEV), ln, pool_rows, col_limit, skip_self, index=index)
    dx, dg, db = torch.autograd.grad((y * I["cot"].to(DEV)).sum(), [x, ln.weight, ln.bias])
    return y.detach(), dx, dg, db


# ---- (1) forward, (3) backward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H", PAIRS)
def test_join_forward(n, H):
    for pool_rows, col_limit, skip_self in configs(n):
        I, ref = case(n, H, pool_rows, col_limit, skip_self)
        ix = cad().join_index(n, I["src"].to(DEV), I["dst"].to(DEV))
        got = raw_fwd(I["x"].to(DEV), ix, pool_rows, col_limit, skip_self, I["gamma"].to(DEV), I["beta"].to(DEV))
        check_forward(I, ref, got, f"n={n} H={H} pool_rows={pool_rows} skip_self={skip_self}")
        assert float(got[4][pool_rows:].sub(1).abs().sum()) == 0.0                  # rows behind pool_rows: 1
        assert torch.equal(got[0][pool_rows:].cpu(), I["x"][pool_rows:])            # ... and their own values


@pytest.mark.parametrize("n,H", PAIRS)
def test_join_backward(n, H):
    for pool_rows, col_limit, skip_self in configs(n):
        I, ref = case(n, H, pool_rows, col_limit, skip_self)
        what = f"n={n} H={H} pool_rows={pool_rows} skip_self={skip_self}"
        ix = cad().join_index(n, I["src"].to(DEV), I["dst"].to(DEV))
        dx = raw_bwd(I["cot"].to(DEV), ix, ref["inv"].float().to(DEV), pool_rows, col_limit, skip_self)
        close(dx, ref["pool_bwd"], TIGHT, what + " pool_bwd")
        y, dx, dg, db = run_join(I, pool_rows, col_limit, skip_self)
        close(y, ref["y"], TIGHT, what + " y (pool_norm)")
        close(dx, ref["dx"], TIGHT, what + " dx")
        close(dg, ref["dgamma"], TIGHT, what + " dgamma")
        close(db, ref["dbeta"], TIGHT, what + " dbeta")


# ---- (2) a row with more than 64 neighbours -------------------------------------------------------------------------------------------
def test_hub_row():
    n, H = 80, 16
    for pool_rows, col_limit, skip_self in configs(n):
        I, ref = case(n, H, pool_rows, col_limit, skip_self, hub=True)
        assert int((I["dst"] == 5).sum()) >= 70
        what = f"hub pool_rows={pool_rows} skip_self={skip_self}"
        ix = cad().join_index(n, I["src"].to(DEV), I["dst"].to(DEV))
        check_forward(I, ref, raw_fwd(I["x"].to(DEV), ix, pool_rows, col_limit, skip_self, I["gamma"].to(DEV), I["beta"].to(DEV)), what)
        close(raw_bwd(I["cot"].to(DEV), ix, ref["inv"].float().to(DEV), pool_rows, col_limit, skip_self), ref["pool_bwd"], TIGHT, what + " pool_bwd")
        y, dx, dg, db = run_join(I, pool_rows, col_limit, skip_self)
        close(dx, ref["dx"], TIGHT, what + " dx")
        close(dg, ref["dgamma"], TIGHT, what + " dgamma")
        close(db, ref["dbeta"], TIGHT, what + " dbeta")


# ---- (4) two runs, the same bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,hub", [(257, 512, False), (80, 16, True), (1000, 1024, False)])
def test_two_runs_same_bits(n, H, hub):
    I, _ = case(n, H, n, n, True, hub)
    a, b = run_join(I, n, n, True), run_join(I, n, n, True)
    for s, t, name in zip(a, b, ("y", "dx", "dgamma", "dbeta")):
        assert torch.equal(s, t), name


# ---- (5) rows whose level dwarfs their spread -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [4, 128, 1024])
def test_offset_rows(H):
    """Rows 1e3 + 1e-2 * randn, self edges only (dropped by skip_self): u is x bit for bit, and y holds TIGHT against float64
    LayerNorm of the same fp32 rows, which a mean centred once in fp32 misses by a factor of several hundred."""
    n = 8
    gen = torch.Generator().manual_seed(H)
    x = (1e3 + 1e-2 * torch.randn(n, H, generator=gen)).float()
    gamma, beta = bf16(H, gen=gen, scale=0.5, shift=1.0), bf16(H, gen=gen, scale=0.5)
    e = torch.arange(n)
    ix = cad().join_index(n, e.to(DEV), e.to(DEV))
    u, y, mean, rstd, inv = raw_fwd(x.to(DEV), ix, n, n, True, gamma.to(DEV), beta.to(DEV))
    assert torch.equal(u.cpu(), x) and torch.equal(inv.cpu(), torch.ones(n))
    close(y, F.layer_norm(x.double(), (H,), gamma.double(), beta.double(), 1e-5), TIGHT, f"offset rows H={H} y")


# ---- (6) operands read where they lie ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H", [(65, 260), (6, 1020)])
def test_operands_in_place(n, H):
    from analysisgnn_amd import _lib
    I, ref = case(n, H, n, n, True)
    packed = run_join(I, n, n, True)
    wide = torch.zeros(n, H + 12, device=DEV)
    wide[:, 4:4 + H] = I["x"].to(DEV)
    for name, view in (("column slice", wide[:, 4:4 + H]), ("16-byte offset", helpers.at_offset(I["x"].to(DEV), 4))):
        assert _lib.rows_ok(view) and (name != "column slice" or view.stride(0) > H)
        got = run_join({**I, "x": view.detach()}, n, n, True)
        for s, t, what in zip(got, packed, ("y", "dx", "dgamma", "dbeta")):
            assert torch.equal(s, t), (name, what)
    ix = cad().join_index(n, I["src"].to(DEV), I["dst"].to(DEV))
    a = raw_fwd(wide[:, 4:4 + H], ix, n, n, True, I["gamma"].to(DEV), I["beta"].to(DEV))
    b = raw_fwd(I["x"].to(DEV), ix, n, n, True, I["gamma"].to(DEV), I["beta"].to(DEV))
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    du = torch.zeros(n, H + 8, device=DEV)
    du[:, 8:] = I["cot"].to(DEV)
    inv = ref["inv"].float().to(DEV)
    assert torch.equal(raw_bwd(du[:, 8:], ix, inv, n, n, True), raw_bwd(I["cot"].to(DEV), ix, inv, n, n, True))


def test_trimmed_index():
    """`rowend` (the row ends of a COO prefix) gives what an index built from the prefix alone gives, both ways."""
    n, H = 65, 260
    I, ref = case(n, H, n, n, True)
    src, dst = I["src"].to(DEV), I["dst"].to(DEV)
    keep = int(src.shape[0]) * 2 // 3
    full, cut = cad().join_index(n, src, dst), cad().join_index(n, src[:keep].clone(), dst[:keep].clone())
    x, gamma, beta, cot = (I[k].to(DEV) for k in ("x", "gamma", "beta", "cot"))
    a = raw_fwd(x, full, n, n, True, gamma, beta, rowend=full.by_dst.rowend(keep))
    b = raw_fwd(x, cut, n, n, True, gamma, beta)
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and not torch.equal(b[0], raw_fwd(x, full, n, n, True, gamma, beta)[0])
    assert torch.equal(raw_bwd(cot, full, b[4], n, n, True, rowend=full.by_src.rowend(keep)), raw_bwd(cot, cut, b[4], n, n, True))


# ---- (7) the two models on the reference's fixtures ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_ref(name):
    return CR.run_case(CR.load_case(name))


def build_model(name):
    z = CR.load_case(name)
    cfg, I = CR.config(z), CR.inputs(z, DEV)
    if cfg["kind"] == "neighbor":
        model = cad().CadenceGNNNeighbor(cfg["metadata"], cfg["in_feats"], cfg["H"], CR.OUT, cfg["L"], dropout=0.0)
    else:
        model = cad().CadenceGNNPytorch(cfg["metadata"], cfg["in_feats"], cfg["H"], CR.OUT, cfg["L"], dropout=0.0, hybrid=cfg["hybrid"],
                                        use_pitch_spelling=cfg["use_ps"])
    model.load_state_dict(CR.state(z), strict=True)
    return model.to(DEV).train(cfg["training"]), z, cfg, I


def encode(model, cfg, I, x_dict):
    if cfg["kind"] == "neighbor":
        return model.encode(x_dict, I["ei_dict"], I["edges_per_hop"], I["nodes_per_hop"])
    return model.encode(x_dict, I["ei_dict"], I["batch_size"], I["mask_node"], I["mask_edge"], {"note": I["batch"]},
                        pitch_spelling=I["ps"] if cfg["use_ps"] else None)


@pytest.mark.parametrize("name", MODELS)
def test_model_fixture(name):
    model, z, cfg, I = build_model(name)
    ref = fixture_ref(name)
    seen = []
    model.norm.register_forward_hook(lambda mod, args, out: seen.append(out.detach()))
    x_dict = {k: v.clone().requires_grad_(k == "note") for k, v in I["x_dict"].items()}
    enc = encode(model, cfg, I, x_dict)
    logits = model.clf(enc)
    ((enc * torch.from_numpy(z["cot.enc"]).to(DEV)).sum() + (logits * torch.from_numpy(z["cot.logits"]).to(DEV)).sum()).backward()
    assert len(seen) == 1, "the hook on `norm` did not run"
    close(seen[0], ref["mid.join_out"], GATE, f"{name} mid.join_out")
    close(enc, ref["out.enc"], GATE, f"{name} out.enc")
    close(logits, ref["out.logits"], GATE, f"{name} out.logits")
    close(enc, torch.from_numpy(z["out.enc"]), GATE, f"{name} out.enc (fixture)")
    close(logits, torch.from_numpy(z["out.logits"]), GATE, f"{name} out.logits (fixture)")
    close(x_dict["note"].grad, ref["grad.x"], GATE, f"{name} grad.x")
    gmax = float(z["meta.grad_max"])
    zero = set(str(k) for k in z["meta.zero_grads"])                                  # gradients that are zero up to rounding: the case's scale
    params = dict(model.named_parameters())
    checked = 0
    for k, g in ref.items():
        if not k.startswith("gw."):
            continue
        p = params[k[3:]]
        assert p.grad is not None, f"{name}: {k} has a reference gradient and none here"
        close(p.grad, g, GATE, f"{name} {k}", gmax if k in zero else None)
        checked += 1
    assert checked == sum(1 for k in z if k.startswith("gw.")) and checked >= 10
    if not cfg["training"]:
        assert not model.training
        with torch.no_grad():
            if cfg["kind"] == "neighbor":
                prob = model(I["x_dict"], I["ei_dict"], I["edges_per_hop"], I["nodes_per_hop"])
            else:
                prob = model(I["x_dict"], I["ei_dict"], I["batch_size"], I["mask_node"], I["mask_edge"], {"note": I["batch"]},
                             pitch_spelling=I["ps"] if cfg["use_ps"] else None)
        assert float((prob.sum(dim=1) - 1).abs().max()) <= 1e-6
        close(prob, torch.softmax(ref["out.logits"], dim=-1), GATE, f"{name} forward")
        sd = CR.state(z)
        for k in ("cad_clf.2.running_mean", "cad_clf.2.running_var"):                 # read, not updated
            assert torch.equal(model.state_dict()[k].cpu(), sd[k]), k


# ---- (8) the training step with a real model as `module` ----------------------------------------------------------------------------
def test_training_loss_with_the_neighbour_model():
    import smote_ref as R
    from analysisgnn_amd import smote
    model, z, cfg, I = build_model("neighbor_h32")
    n = int(z["out.enc"].shape[0])
    D, k, reg = int(z["out.enc"].shape[1]), 3, 0.1
    gen = torch.Generator().manual_seed(23)
    y = torch.cat([torch.zeros(n - 15), torch.ones(10), torch.full((5,), 2.0)]).long()[torch.randperm(n, generator=gen)]
    S = R.n_synthetic(y, k)
    choice, gap = torch.randint(0, k - 1, (S,), generator=gen).int(), torch.rand(S, D, generator=gen).float()
    sm = smote.SMOTE(dims=D, distance="euclidian", k=k)
    x_dict = {t: v.clone().requires_grad_(t == "note") for t, v in I["x_dict"].items()}
    x = encode(model, cfg, I, x_dict)
    total, logits, y_over = cad().cadence_training_loss(model, x, y.to(DEV), sm, reg, perms=None, draws=(choice.to(DEV), gap.to(DEV)))
    total.backward()
    tables = {lab: t for lab, t in zip(sm.last_call["labels"],
                                       [sm.last_call["nbr"].cpu().long()[a:b, 1:k] - a for a, b in zip(sm.last_call["t_off"][:-1], sm.last_call["t_off"][1:])])}
    I64 = CR.inputs(z)
    x64 = {t: v.double().clone().requires_grad_(t == "note") for t, v in I64["x_dict"].items()}
    P = {key: (v.double().requires_grad_(True) if v.is_floating_point() and "running_" not in key else v) for key, v in CR.state(z).items()}
    enc = CR.neighbor_encode(P, cfg, x64, I64["ei_dict"], I64["nodes_per_hop"], I64["edges_per_hop"])
    xo, yo, _ = R.fit_generate(enc, y, choice, gap.double(), k=k, distance="euclidian", tables=tables)
    assert torch.equal(yo, y_over.cpu())
    ref = CR.training_loss(P, enc, y, xo, yo, reg, None, [])
    gx, = torch.autograd.grad(ref, [x64["note"]])
    close(total, ref, GATE, "cadence_training_loss on CadenceGNNNeighbor")
    close(x_dict["note"].grad, gx, GATE, "cadence_training_loss grad.x")
    assert tuple(logits.shape) == (int(yo.shape[0]), CR.OUT)


# ---- (9) refusals on the device -------------------------------------------------------------------------------------------------------
def test_refusals():
    from analysisgnn_amd._abi import AgnnError
    z = CR.load_case("pytorch_ps_h32")
    cfg, I = CR.config(z), CR.inputs(z, DEV)
    zn = CR.load_case("neighbor_h32")
    cfgn, In = CR.config(zn), CR.inputs(zn, DEV)
    torch.manual_seed(3)
    odd = cad().CadenceGNNNeighbor(cfgn["metadata"], cfgn["in_feats"], 36, CR.OUT, cfgn["L"], dropout=0.0).to(DEV).train()     # 36 // 2 = 18
    with pytest.raises(AgnnError, match="H=18"):
        odd.encode(dict(In["x_dict"]), In["ei_dict"], In["edges_per_hop"], In["nodes_per_hop"])
    odd = cad().CadenceGNNPytorch(cfg["metadata"], cfg["in_feats"], 36, CR.OUT, cfg["L"], dropout=0.0, use_pitch_spelling=False).to(DEV).train()
    with pytest.raises(AgnnError, match="H=18"):
        odd(dict(I["x_dict"]), I["ei_dict"], I["batch_size"])
    model = cad().CadenceGNNPytorch(cfg["metadata"], cfg["in_feats"], cfg["H"], CR.OUT, cfg["L"], dropout=0.0, use_pitch_spelling=True).to(DEV).train()
    with pytest.raises(AgnnError, match="pitch_spelling"):
        model(dict(I["x_dict"]), I["ei_dict"], I["batch_size"], I["mask_node"], I["mask_edge"])
    out = model(dict(I["x_dict"]), I["ei_dict"], I["batch_size"], pitch_spelling=I["ps"])     # masks left at None: nothing is trimmed
    assert tuple(out.shape) == (I["batch_size"], CR.OUT) and bool(torch.isfinite(out).all())
    with pytest.raises(AgnnError, match="one row"):
        model.clf(torch.zeros(1, cfg["H"] // 2, device=DEV))
    ln = nn.LayerNorm(16).to(DEV)
    e = torch.zeros(1, dtype=torch.long, device=DEV)
    with pytest.raises(AgnnError, match="fp32"):
        cad().pool_norm(torch.zeros(4, 16, device=DEV, dtype=torch.float64), e, e, ln)
    with pytest.raises(AgnnError, match="H=1028"):
        cad().pool_norm(torch.zeros(4, 1028, device=DEV), e, e, nn.LayerNorm(1028).to(DEV))
    with pytest.raises(AgnnError, match="affine"):
        cad().pool_norm(torch.zeros(4, 16, device=DEV), e, e, nn.LayerNorm(16, elementwise_affine=False).to(DEV))
    with pytest.raises(AgnnError, match="index was built"):
        cad().pool_norm(torch.zeros(4, 16, device=DEV), e, e, ln, index=cad().join_index(5, e, e))


# ---- (10) one capture -----------------------------------------------------------------------------------------------------------------
def test_one_captured_forward_and_backward():
    n, H = 65, 260
    I, _ = case(n, H, n, n, True)
    x = I["x"].to(DEV).requires_grad_(True)
    ln = layer_norm(I["gamma"], I["beta"])
    src, dst, cot = I["src"].to(DEV), I["dst"].to(DEV), I["cot"].to(DEV)
    ix = cad().join_index(n, src, dst)                                            # built before anything is captured
    leaves = [x, ln.weight, ln.bias]

    def one_step():
        y = cad().pool_norm(x, src, dst, ln, n, n, True, index=ix)
        (y * cot).sum().backward()
        return y

    # The eager steps run on a side stream, as every captured training step of this suite does: autograd pins a leaf's
    # AccumulateGrad node to the stream that was current when the leaf first entered a graph, and a capture must not make the
    # default stream wait for the capturing one.
    eager = []
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            for t in leaves:
                t.grad = None
            y = one_step()
            eager.append((y.detach().clone(), [t.grad.clone() for t in leaves]))
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    del y                                                                       # nothing keeps the eager steps' autograd graph alive
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                                      # the stream the leaves' AccumulateGrad nodes are pinned to
        y = one_step()
    for r in range(2):
        g.replay()
        torch.cuda.synchronize()
        out, grads = eager[r]
        assert torch.equal(y.detach(), out), f"replay {r} y"
        for t, e, name in zip(leaves, grads, ("x", "gamma", "beta")):
            assert torch.equal(t.grad, e), f"replay {r} grad {name}"
