"""The ChordGNN model on the GPU (analysisgnn_amd/chord.py; csrc/colnorm.hip, csrc/onsetpool.hip).

Goldens (tests/golden/chord_*.npz, the reference's own classes in float64, tests/gen_golden_chord.py): logits, encoder output,
running statistics, input and weight gradients within 1e-4 x the compared tensor's max-abs (the project's parity gate, SURVEY
§8d); the pooled rows and the BatchNorm block, each run alone on float64-exact inputs, within 1e-5 x max-abs.  A gradient that is
zero in exact arithmetic (meta.zero_grads: the bias in front of JumpingKnowledge's softmax over layers) has max-abs 0 and is held
against 1e-4 x the largest weight gradient's max-abs instead.

The kernels against torch in float64 on their own inputs, at every size where their code takes another path (a slab of 128 rows,
64 rows of lanes, 16 lanes of the final passes, groups of 4 .. 64 lanes per pooled row).

Dropout.  "dx is zero exactly where y was dropped" does not hold with BATCH statistics, for any implementation: dx_i = gamma * rstd * (g_i - mean(g) - xhat_i * mean(g * xhat)) keeps the two means where g_i = 0.  It holds with
running statistics, where dx = gamma * rstd * g; the C entry point takes dropout and the statistics' source independently, so
the statement is checked there, and with batch statistics dx is held against the float64 formula evaluated with the mask read
off y (which pins that backward regenerates the forward's mask, element by element)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import chord_ref as CR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE, TIGHT = 1e-4, 1e-5
SLAB, FINAL_LANES = 128, 16


def close(got, exp, tol, what, scale=None):
    got, exp = got.detach().double().cpu(), exp.detach().double().cpu()
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if exp.numel() == 0:
        return
    s = float(exp.abs().max()) if scale is None else scale
    err = float((got - exp).abs().max())
    print(f"{what}: err {err:.3e}  bound {tol * s:.3e}")
    assert err <= tol * s, (what, err, tol * s)


# ---- goldens ------------------------------------------------------------------------------------------------------------------------
def build_model(name, dropout=0.0):
    from analysisgnn_amd import chord
    z = CR.load_case(name)
    cfg = CR.config(z)
    model = chord.MetricalChordPredictionModel(cfg["in_feats"], n_hidden=cfg["H"], tasks=cfg["tasks"], n_layers=cfg["L"], dropout=dropout,
                                               use_nade=cfg["nade"], use_jk=cfg["jk"], metrical=cfg["metrical"], conv_block=cfg["block"])
    model.load_state_dict(CR.initial_state(z), strict=True)
    return model.to(DEV).train(), z, cfg, CR.inputs(z, DEV)


def step(model, I, z, tasks):
    x = I["x"].clone().requires_grad_(True)
    for p in model.parameters():
        p.grad = None
    pred = model(x, I["edge_index"], I["edge_type"], I["onset_index"], I["onset_idx"], I["lengths"], **I["extra"])
    sum((pred[t] * torch.from_numpy(z["cot." + t]).to(DEV)).sum() for t in tasks).backward()
    return pred, x.grad


@pytest.mark.parametrize("name", CR.CASES)
def test_goldens(name):
    model, z, cfg, I = build_model(name)
    keep = {}
    hooks = [model.encoder.pool.register_forward_hook(lambda m, a, o: keep.__setitem__("mid.pooled", o[0].detach())),
             model.encoder.register_forward_hook(lambda m, a, o: keep.__setitem__("mid.encoder", o.detach()))]
    pred, gx = step(model, I, z, cfg["tasks"])
    for h in hooks:
        h.remove()
    for t in cfg["tasks"]:
        close(pred[t], torch.from_numpy(z["out." + t]), GATE, f"{name} out.{t}")
    close(keep["mid.encoder"], torch.from_numpy(z["mid.encoder"]), GATE, f"{name} mid.encoder")
    close(keep["mid.pooled"], torch.from_numpy(z["mid.pooled"]), GATE, f"{name} mid.pooled (inside the model)")
    sd = model.state_dict()
    for k in sd:
        if "running_" in k:
            close(sd[k], torch.from_numpy(z["w." + k]), GATE, f"{name} {k}")
        elif k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(z["w." + k]) == 1, k
    close(gx, torch.from_numpy(z["grad.x"]), GATE, f"{name} grad.x")
    zero = set(str(k) for k in z["meta.zero_grads"])
    without = set()
    for k, p in model.named_parameters():
        if p.grad is None:
            without.add(k)
            continue
        assert "gw." + k in z, f"{k} has a gradient the reference does not give"
        close(p.grad, torch.from_numpy(z["gw." + k]), GATE, f"{name} gw.{k}", float(z["meta.grad_max"]) if "gw." + k in zero else None)
    assert without == set(str(k) for k in z["meta.no_grad"])


@pytest.mark.parametrize("name", ["chord_h16_whole", "chord_h32_resgated"])
def test_pool_and_batchnorm_block_alone(name):
    """Each on float64-exact inputs: the pool on the restated schedule's float64 input rows, the block on the fixture's bn1 input."""
    from analysisgnn_amd import chord
    model, z, cfg, I = build_model(name)
    P = {k: v.double() for k, v in CR.initial_state(z).items()}
    Iref = CR.inputs(z)
    Iref["x"] = Iref["x"].double()
    _, mids, _ = CR.forward(P, cfg, Iref)
    a = mids["mid.pool_in"].float().to(DEV)
    pooled, _ = model.encoder.pool(a, I["onset_index"], I["onset_idx"])
    close(pooled, torch.from_numpy(z["mid.pooled"]), TIGHT, f"{name} pooled rows alone")
    bn = model.encoder.layernorm1
    y = chord.act_norm_drop(torch.from_numpy(z["mid.bn1_in"]).float().to(DEV), bn, None, 0.0, True)
    close(y, torch.from_numpy(z["mid.bn1_out"]), TIGHT, f"{name} BatchNorm block alone")


def test_state_dict_round_trip_deepcopy_and_eval():
    model, z, cfg, I = build_model("chord_h16_whole")
    ref_sd = {k: torch.from_numpy(np.asarray(z["w." + k])) for k in (str(s) for s in z["meta.keys"])}
    model.load_state_dict(ref_sd, strict=True)                                  # the reference-format state_dict, running statistics included
    back = model.state_dict()
    assert list(back.keys()) == list(ref_sd.keys())
    for k, v in ref_sd.items():
        assert torch.equal(back[k].cpu(), v.to(back[k].dtype)), k
    step(model, I, z, cfg["tasks"])                                             # lays the heads' running statistics side by side
    twin = copy.deepcopy(model)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), twin.state_dict().values()))
    args = (I["x"], I["edge_index"], I["edge_type"], I["onset_index"], I["onset_idx"], I["lengths"])
    model.eval()
    twin.eval()
    with torch.no_grad():
        first = {t: v.clone() for t, v in model(*args, **I["extra"]).items()}
        other = {t: v.clone() for t, v in twin(*args, **I["extra"]).items()}
        stats = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()                                  # the first call's own outputs are freed: only clones live
        second = model(*args, **I["extra"])
        second = {t: v.clone() for t, v in second.items()}
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated() - before - sum(v.numel() * v.element_size() for v in second.values())
        assert grown <= 512 * len(second), grown                                # no workspace kept: only the clones (allocator rounding apart)
    for t in first:
        assert torch.equal(first[t], second[t]) and torch.equal(first[t], other[t]), t
    for k, v in stats.items():
        assert torch.equal(model.state_dict()[k], v), k                         # eval leaves the running statistics alone


@pytest.mark.parametrize("H,seed", [(128, 640), (256, 626)])
def test_wide_model_against_the_float64_restatement(H, seed):
    """Widths the fixtures do not have: the encoder GRU on the persistent kernels (hidden 64 / 128), the heads' last layers as the
    grouped projection (128) and as per-task products on column windows (256).  Yardstick: tests/chord_ref.py in float64, which
    the fixtures pin; bound: the parity gate.  The seeds were chosen on the CPU so that the restatement's own fp32 evaluation
    stays within 0.11 / 0.17 of the gate on every tensor."""
    model, cfg, I, cots = CR.wide_case(H, seed)
    exp = CR.run_params(model.state_dict(), cfg, I, cots)
    model = model.to(DEV).train()
    Id = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in I.items() if k != "extra"}
    x = Id["x"].clone().requires_grad_(True)
    keep = {}
    hook = model.encoder.register_forward_hook(lambda m, a, o: keep.__setitem__("mid.encoder", o.detach()))
    pred = model(x, Id["edge_index"], Id["edge_type"], Id["onset_index"], Id["onset_idx"], None)
    hook.remove()
    sum((pred[t] * cots[t].to(DEV)).sum() for t in pred).backward()
    for t in pred:
        close(pred[t], exp["out." + t], GATE, f"H={H} out.{t}")
    close(keep["mid.encoder"], exp["mid.encoder"], GATE, f"H={H} mid.encoder")
    close(x.grad, exp["grad.x"], GATE, f"H={H} grad.x")
    gmax = max(float(v.abs().max()) for k, v in exp.items() if k.startswith("gw."))
    for k, p in model.named_parameters():
        if "gw." + k in exp:
            e = exp["gw." + k]
            close(p.grad, e, GATE, f"H={H} gw.{k}", gmax if float(e.abs().max()) < 1e-9 * gmax else None)
        else:
            assert p.grad is None, k
    for k, v in model.state_dict().items():
        if "running_" in k:
            close(v, exp["w." + k], GATE, f"H={H} {k}")


def test_two_runs_give_the_same_bits():
    model, z, cfg, I = build_model("chord_h16_windows")
    sd0 = copy.deepcopy(model.state_dict())
    runs = []
    for _ in range(2):
        model.load_state_dict(sd0)
        pred, gx = step(model, I, z, cfg["tasks"])
        runs.append(([pred[t].clone() for t in cfg["tasks"]], gx.clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                     copy.deepcopy(model.state_dict())))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1], runs[1][1])
    assert runs[0][2].keys() == runs[1][2].keys()
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    for k in runs[0][3]:
        assert torch.equal(runs[0][3][k], runs[1][3][k]), k


def test_graph_replay_matches_eager():
    model, z, cfg, I = build_model("chord_h16_whole")
    tasks = list(cfg["tasks"])
    sd0 = copy.deepcopy(model.state_dict())
    cots = [torch.from_numpy(z["cot." + t]).to(DEV) for t in tasks]
    x = I["x"].clone().requires_grad_(True)
    args = (x, I["edge_index"], I["edge_type"], I["onset_index"], I["onset_idx"], I["lengths"])

    def one_step():
        pred = model(*args, **I["extra"])
        sum((pred[t] * c).sum() for t, c in zip(tasks, cots)).backward()
        return pred

    # The eager steps run on a side stream, as every captured training step of this suite does: autograd pins a leaf's
    # AccumulateGrad node to the stream that was current when the leaf first entered a graph, and a capture must not make the
    # default stream wait for the capturing one.
    eager = []
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):                                                      # two eager steps from the initial state
            x.grad = None
            for p in model.parameters():
                p.grad = None
            pred = one_step()
            eager.append(([pred[t].clone() for t in tasks], x.grad.clone(),
                          {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, copy.deepcopy(model.state_dict())))
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    model.load_state_dict(sd0)
    x.grad = None
    for p in model.parameters():
        p.grad = None
    torch.cuda.synchronize()
    del pred                                                                    # nothing keeps the eager steps' autograd graph alive
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                                      # the stream the leaves' AccumulateGrad nodes are pinned to
        pred = one_step()
    model.load_state_dict(sd0)                                                  # capture runs nothing; start the replays from the initial state
    for r in range(2):
        g.replay()
        torch.cuda.synchronize()
        logits, gx, gw, sd = eager[r]
        for t, e in zip(tasks, logits):
            close(pred[t], e, 1e-6, f"replay {r} out.{t}")
        close(x.grad, gx, 1e-6, f"replay {r} grad.x")
        for k, p in model.named_parameters():
            if k in gw:
                close(p.grad, gw[k], 1e-6, f"replay {r} gw.{k}", max(float(gw[k].abs().max()), 1e-12))
        now = model.state_dict()
        for k in sd:
            if k.endswith("num_batches_tracked"):
                assert int(now[k]) == r + 1, k                                  # the running statistics advance once per replay
            elif "running_" in k:
                close(now[k], sd[k], 1e-6, f"replay {r} {k}")


def test_refusals():
    from analysisgnn_amd import chord
    from analysisgnn_amd._abi import AgnnError
    model, z, cfg, I = build_model("chord_h16_whole")
    with pytest.raises(AgnnError, match="chord.py:568"):
        model.encoder.pool(torch.zeros(8, 16, device=DEV), I["onset_index"], None)
    with pytest.raises(AgnnError, match="unequal lengths"):
        model(I["x"], I["edge_index"], I["edge_type"], I["onset_index"], I["onset_idx"], torch.tensor([12, 10], device=DEV), **I["extra"])
    bn = nn.BatchNorm1d(8).to(DEV).train()
    with pytest.raises(AgnnError, match="more than 1 value per channel"):
        chord.act_norm_drop(torch.zeros(1, 8, device=DEV), bn, F.relu, 0.0, True)
    with pytest.raises(AgnnError):
        chord.onset_pool(torch.zeros(8, 16), I["onset_index"].cpu(), I["onset_idx"].cpu())          # no CPU path


# ---- kernel a: the column-statistics block against torch in float64 -------------------------------------------------------------------
def bn_reference(x, gamma, beta, relu, mask=None, rm=None, rv=None, training=True, dy=None):
    """float64 on the CPU: (y, dx, dgamma, dbeta, running_mean, running_var) of dropout-mask * batch_norm(act(x))."""
    x = x.detach().double().cpu().requires_grad_(True)
    gamma, beta = gamma.detach().double().cpu().requires_grad_(True), beta.detach().double().cpu().requires_grad_(True)
    rm = rm.detach().double().cpu().clone() if rm is not None else None
    rv = rv.detach().double().cpu().clone() if rv is not None else None
    a = F.relu(x) if relu else x
    y = F.batch_norm(a, rm, rv, gamma, beta, training, 0.1, 1e-5)
    if mask is not None:
        y = y * mask.double().cpu()
    out = [y.detach()]
    if dy is not None:
        y.backward(dy.detach().double().cpu())
        out += [x.grad, gamma.grad, beta.grad]
    return out + [rm, rv]


def run_block(x, gamma, beta, relu, training=True, p=0.0, rm=None, rv=None, nbt=None, dy=None):
    from analysisgnn_amd import chord
    xg = x.detach().requires_grad_(True)
    gg, bg = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
    running = (rm, rv, nbt) if rm is not None else None
    y = chord.colnorm(xg, gg, bg, running, 1e-5, 0.1, relu, p, training)
    if dy is None:
        return y.detach()
    y.backward(dy)
    return y.detach(), xg.grad, gg.grad, bg.grad


def block_inputs(N, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, generator=g) * (0.5 + torch.rand(C, generator=g) * 2) + torch.randn(C, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(N, C, generator=g)
    return x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)


def dx_scale(x, gamma, relu, dy, var=None, p=0.0):
    """Per column: |gamma| * rstd * max|dy| / (1 - p), the size of the TERMS of dx = gamma * rstd * (g - mean g - xhat * mean(g xhat)).
    The three terms cancel (for two rows, down to eps / var of their size), so an fp32 evaluation, whose rounding error is a few
    ulp of the terms, is held against 1e-5 of the terms (84 ulp), not of the result."""
    a = x.detach().double().cpu()
    a = a.relu() if relu else a
    var = a.var(dim=0, unbiased=False) if var is None else var.detach().double().cpu()
    return gamma.detach().double().cpu().abs() / torch.sqrt(var + 1e-5) * dy.detach().double().cpu().abs().max(dim=0).values / (1 - p)


def close_cols(got, exp, tol, scale, what):
    got, exp = got.detach().double().cpu(), exp.detach().double().cpu()
    err = (got - exp).abs().max(dim=0).values
    worst = int((err / scale.clamp(min=1e-300)).argmax())
    print(f"{what}: worst column {worst}: err {float(err[worst]):.3e}  bound {tol * float(scale[worst]):.3e}")
    assert bool((err <= tol * scale).all()), (what, worst, float(err[worst]), tol * float(scale[worst]))


def check_block(got, exp, x, gamma, relu, dy, what, p=0.0):
    (y, dx, dg, db), (ey, edx, edg, edb) = got, exp
    close_cols(y, ey, TIGHT, ey.abs().max(dim=0).values, f"{what} y")
    close_cols(dx, edx, TIGHT, dx_scale(x, gamma, relu, dy, p=p), f"{what} dx")
    close(dg, edg, TIGHT, f"{what} dgamma")
    close(db, edb, TIGHT, f"{what} dbeta")


ROWS = [2, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, FINAL_LANES * SLAB + 1]     # the last: 17 slabs, one more than the final pass has lanes
COLS = [4, 8, 36, 224, 260]                                                  # 224 = 14 x 16 stacked heads


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", COLS)
def test_block_against_float64(C, relu):
    for N in ROWS:
        x, gamma, beta, dy = block_inputs(N, C, 1000 * C + N)
        rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
        y, dx, dg, db = run_block(x, gamma, beta, relu, rm=rm, rv=rv, nbt=nbt, dy=dy)
        ey, edx, edg, edb, erm, erv = bn_reference(x, gamma, beta, relu, rm=torch.zeros(C), rv=torch.ones(C), dy=dy)
        check_block((y, dx, dg, db), (ey, edx, edg, edb), x, gamma, relu, dy, f"N={N} C={C} relu={relu}")
        close(rm, erm, TIGHT, f"N={N} C={C} relu={relu} running_mean")
        close(rv, erv, TIGHT, f"N={N} C={C} relu={relu} running_var")
        assert int(nbt) == 1


def test_block_on_a_column_window():
    N, C = 200, 36
    x, gamma, beta, dy = block_inputs(N, 64, 7)
    win = x[:, 8:8 + C]                                                         # rows 256 bytes apart, the window 32 bytes in
    y, dx, dg, db = run_block(win, gamma[:C], beta[:C], True, dy=dy[:, :C].contiguous())
    ey, edx, edg, edb, _, _ = bn_reference(win, gamma[:C], beta[:C], True, dy=dy[:, :C])
    check_block((y, dx, dg, db), (ey, edx, edg, edb), win, gamma[:C], True, dy[:, :C], "window")


def test_block_constant_and_cancellation_columns():
    N, C = 300, 8
    x, gamma, beta, dy = block_inputs(N, C, 11)
    x[:, 2] = 0.75                                                              # exactly constant: y == beta, xhat == 0
    g = torch.Generator().manual_seed(12)
    x[:, 5] = (1e3 + 1e-2 * torch.randn(N, generator=g)).to(DEV)                # mean 1e3, standard deviation 1e-2
    y, dx, dg, db = run_block(x, gamma, beta, False, dy=dy)
    ey, edx, edg, edb, _, _ = bn_reference(x, gamma, beta, False, dy=dy)
    assert torch.equal(y[:, 2], beta[2].expand(N))
    check_block((y, dx, dg, db), (ey, edx, edg, edb), x, gamma, False, dy, "constant / cancellation")     # column by column
    assert float(dg[2]) == 0.0                                                  # xhat == 0 down the constant column


def test_block_eval_after_three_training_calls():
    N, C = 150, 36
    bn = nn.BatchNorm1d(C).to(DEV)
    ref = nn.BatchNorm1d(C).double()
    from analysisgnn_amd import chord
    with torch.no_grad():
        x0, gamma, beta, _ = block_inputs(N, C, 21)
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
        ref.weight.copy_(gamma.double().cpu()); ref.bias.copy_(beta.double().cpu())
    bn.train(); ref.train()
    for i in range(3):
        x = block_inputs(N, C, 22 + i)[0]
        chord.act_norm_drop(x, bn, F.relu, 0.0, True)
        ref(F.relu(x.double().cpu()))
    assert int(bn.num_batches_tracked) == 3 == int(ref.num_batches_tracked)
    close(bn.running_mean, ref.running_mean, TIGHT, "running_mean after three calls")
    close(bn.running_var, ref.running_var, TIGHT, "running_var after three calls")
    bn.eval(); ref.eval()
    xe = x0.clone().requires_grad_(True)
    y = chord.act_norm_drop(xe, bn, F.relu, 0.5, False)                         # eval: no dropout whatever p says
    xr = x0.double().cpu().requires_grad_(True)
    ye = ref(F.relu(xr))
    close(y, ye, TIGHT, "eval y")
    dy = block_inputs(N, C, 30)[3]
    y.backward(dy)
    ye.backward(dy.double().cpu())
    close(xe.grad, xr.grad, TIGHT, "eval dx")
    close(bn.weight.grad, ref.weight.grad, TIGHT, "eval dgamma")
    assert int(bn.num_batches_tracked) == 3


def test_block_dropout():
    N, C, p = 400, 36, 0.5
    x, gamma, beta, dy = block_inputs(N, C, 41)
    y0 = run_block(x, gamma, beta, True)
    y, dx, dg, db = run_block(x, gamma, beta, True, p=p, dy=dy)
    dropped = y == 0                                                            # BatchNorm output is zero with probability zero
    assert not bool((y0 == 0).any())
    kept = ~dropped
    expect = y0 / (1 - p)
    ulp = torch.abs(torch.nextafter(expect, torch.full_like(expect, float("inf"))) - expect)
    assert bool(((y - expect).abs()[kept] <= ulp[kept]).all())                  # kept positions: the p = 0 output / (1 - p), to 1 ulp
    share, sd = float(dropped.float().mean()), (p * (1 - p) / (N * C)) ** 0.5
    assert abs(share - p) <= 5 * sd, (share, p, sd)
    ey, edx, edg, edb, _, _ = bn_reference(x, gamma, beta, True, mask=kept.double() / (1 - p), dy=dy)
    check_block((y, dx, dg, db), (ey, edx, edg, edb), x, gamma, True, dy, "dropout", p=p)   # backward regenerated exactly the forward's mask
    y2 = run_block(x, gamma, beta, True, p=p)                                   # a second block of the same step: another call id
    assert not torch.equal(y2 == 0, dropped)
    assert abs(float(((y2 == 0) & dropped).float().mean()) - p * p) <= 5 * (p * p * (1 - p * p) / (N * C)) ** 0.5


def test_block_dropout_with_running_statistics_zeroes_dx_where_dropped():
    """Dropout and the statistics' source are independent at the C entry point: with running statistics dx = gamma * rstd * g."""
    from analysisgnn_amd import _lib, fused
    N, C, p = 200, 36, 0.5
    x, gamma, beta, dy = block_inputs(N, C, 51)
    lib = _lib.load()
    rm, rv = torch.randn(C, device=DEV) * 0.1, torch.rand(C, device=DEV) + 0.5
    y, dx, stats = torch.empty_like(x), torch.empty_like(x), torch.empty(3, C, device=DEV)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rng, used = fused.rng_state(torch.device(DEV)), torch.empty(2, dtype=torch.int64, device=DEV)
    nws = int(lib.agnn_colnorm_workspace_bytes(N, C))
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))
    _lib.check(lib.agnn_colnorm_fwd_f32(x.data_ptr(), C, N, C, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), None, 1e-5, 0.1, p,
                                        0, rng.data_ptr(), 77, y.data_ptr(), C, stats.data_ptr(), used.data_ptr(), None, 0, st), "fwd")
    _lib.check(lib.agnn_colnorm_bwd_f32(x.data_ptr(), C, N, C, gamma.data_ptr(), stats.data_ptr(), p, 0, used.data_ptr(), 77, dy.data_ptr(), C,
                                        dx.data_ptr(), C, dg.data_ptr(), db.data_ptr(), ws.data_ptr(), nws, st), "bwd")
    dropped = y == 0
    assert 0.4 < float(dropped.float().mean()) < 0.6
    assert bool((dx[dropped] == 0).all()) and bool((dx[~dropped] != 0).all())
    exp = (dy.double() * (~dropped).double() / (1 - p) * gamma.double() / torch.sqrt(rv.double() + 1e-5)).cpu()
    close(dx, exp, TIGHT, "dx with running statistics")


# ---- kernel b: onset pooling with selection against float64 ---------------------------------------------------------------------------
def pool_case(n, H, E, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, H, generator=g)
    ei = torch.randint(0, n, (2, E), generator=g) if E else torch.zeros(2, 0, dtype=torch.long)
    idx = torch.randperm(n, generator=g)[:K] if K <= n else torch.randint(0, n, (K,), generator=g)
    return a, ei, idx


def run_pool(a, ei, idx, cot):
    from analysisgnn_amd import chord
    ag = a.to(DEV).requires_grad_(True)
    out = chord.onset_pool(ag, ei.to(DEV), idx.to(DEV))
    if out.numel():
        out.backward(cot.to(DEV))
    else:
        out.sum().backward()
    ad = a.double().requires_grad_(True)
    ref = CR.pool_then_select(ad, ei, idx)
    ref.backward(cot.double()) if ref.numel() else ref.sum().backward()
    return out.detach(), ag.grad, ref.detach(), ad.grad


@pytest.mark.parametrize("H", [4, 8, 36, 128, 260])
def test_pool_against_float64(H):
    n = 90
    for K in (0, 1, 63, 64, 65):
        a, ei, idx = pool_case(n, H, 300, K, 100 * H + K)
        ei[:, :5] = ei[0, :5]                                                   # self loops in the list: counted once more
        cot = torch.randn(K, H, generator=torch.Generator().manual_seed(K))
        out, da, ref, dref = run_pool(a, ei, idx, cot)                          # idx is a random permutation's head: unsorted
        close(out, ref, TIGHT, f"H={H} K={K} pooled")
        close(da, dref, TIGHT, f"H={H} K={K} da", max(float(dref.abs().max()), 1.0))


def test_pool_edge_cases():
    n, H = 40, 36
    a, ei, _ = pool_case(n, H, 120, 1, 3)
    ei = ei[:, (ei[1] != 7)]                                                    # node 7: in-degree 0
    ei = torch.cat([ei, torch.tensor([[9, 9], [9, 9]])], dim=1)                 # node 9: a self loop twice in the list
    idx = torch.tensor([30, 7, 9, 2, 9, 30, 30])                                # unsorted, repeated entries: their gradients add
    cot = torch.randn(idx.numel(), H, generator=torch.Generator().manual_seed(4))
    out, da, ref, dref = run_pool(a, ei, idx, cot)
    close(out, ref, TIGHT, "pooled")
    close(da, dref, TIGHT, "da")
    assert torch.equal(out[1].cpu(), a[7])                                      # in-degree 0: the row itself
    assert torch.equal(out[2], out[4]) and torch.equal(out[0], out[5])
    selected = set(idx.tolist())
    touched = set(idx.tolist()) | {int(s) for s, d in zip(ei[0], ei[1]) if int(d) in selected}
    for j in range(n):
        if j not in touched:
            assert bool((da[j] == 0).all()), j                                  # nothing reaches a row no selected mean contains
    # edges into unselected rows have no effect, forward or backward
    keep = torch.tensor([int(d) in selected for d in ei[1]])
    out2, da2, _, _ = run_pool(a, ei[:, keep], idx, cot)
    assert torch.equal(out, out2) and torch.equal(da, da2)
    # an empty edge list: every pooled row is its own row
    out3, da3, ref3, dref3 = run_pool(a, torch.zeros(2, 0, dtype=torch.long), idx, cot)
    assert torch.equal(out3.cpu(), a[idx])
    close(da3, dref3, TIGHT, "da, no edges")


def test_pool_then_trans_equals_the_literal_composition():
    from analysisgnn_amd import chord
    n, H = 64, 36
    a, ei, idx = pool_case(n, H, 200, 20, 9)
    pool = chord.OnsetEdgePoolingVersion2(H).to(DEV)
    out, same = pool(a.to(DEV), ei.to(DEV), idx.to(DEV))
    assert same is not None and torch.equal(same.cpu(), idx)
    ref = CR.literal_pool(a.double(), pool.trans.weight.detach().double().cpu(), pool.trans.bias.detach().double().cpu(), ei, idx)
    close(out, ref, TIGHT, "trans(pool) against scatter(trans)[idx]")


def test_unique_onsets_on_the_device():
    from analysisgnn_amd.chord import unique_onsets
    g = torch.Generator().manual_seed(1)
    for n in (1, 7, 500):
        on = torch.randint(0, max(n // 3, 1), (n,), generator=g)
        got = unique_onsets(on.to(DEV))
        assert got.device.type == "cuda" and got.cpu().tolist() == CR.unique_onsets(on).tolist()
