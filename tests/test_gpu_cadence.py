"""The class-balanced cross entropy, the cadence stacks and the step functions on the GPU (analysisgnn_amd/cadence.py; csrc/balce.hip).

Gates are the project's own (tests/test_gpu_chord.py): GATE 1e-4 x max-abs of the compared tensor end to end, TIGHT
1e-5 x max-abs for a kernel alone on bf16-valued inputs against float64 (tests/cadence_ref.py, gradients by autograd)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import cadence_ref as CR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE, TIGHT = 1e-4, 1e-5


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


# ---- the class-balanced cross entropy -------------------------------------------------------------------------------------------------
def bce_raw(z, y, ignore=-100, want_d=True):
    """(loss, dlogits, count, weight, status) straight from agnn_balanced_ce_f32, with a status word of its own."""
    from analysisgnn_amd import _lib
    lib = _lib.load()
    n, C = z.shape
    count, weight = torch.empty(C, dtype=torch.int64, device=DEV), torch.empty(C, device=DEV)
    loss, status = torch.empty((), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    d = torch.full((n, C), float("nan"), device=DEV) if want_d else None
    nws = int(lib.agnn_balanced_ce_workspace_bytes(n))
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    _lib.check(lib.agnn_balanced_ce_f32(z.data_ptr(), z.stride(0), n, C, y.data_ptr(), ignore, 1e-6, count.data_ptr(), weight.data_ptr(),
                                        loss.data_ptr(), _lib.ptr(d), C, status.data_ptr(), ws.data_ptr(), nws, _lib.stream_ptr(z.device)),
               "agnn_balanced_ce_f32")
    torch.cuda.synchronize()
    return loss, d, count, weight, int(status)


@pytest.mark.parametrize("C", [2, 5, 37])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_balanced_ce(n, C):
    gen = torch.Generator().manual_seed(10 * n + C)
    z = bf16(n, C, gen=gen, scale=2.0)
    y = torch.randint(0, C - 1, (n,), generator=gen)                             # the last class never occurs
    if n > 4:
        y[::7] = -100
    ref = CR.balanced_ce(z.double(), y)
    zd, yd = z.to(DEV), y.to(DEV)
    loss, d, count, weight, status = bce_raw(zd, yd)
    what = f"n={n} C={C}"
    close(loss, ref[0], TIGHT, what + " loss")
    close(d, ref[1], TIGHT, what + " dlogits")
    assert torch.equal(count.cpu(), ref[2]) and int(count[C - 1]) == 0 and status == 0
    close(weight, ref[3], TIGHT, what + " weight")
    again = bce_raw(zd, yd)
    assert torch.equal(again[0], loss) and torch.equal(again[1], d)              # two runs, the same bits
    # the module path: value and gradient by autograd, a strided logits matrix read in place
    wide = torch.zeros(n, C + 3, device=DEV)
    wide[:, 1:C + 1] = zd
    zl = wide[:, 1:C + 1].requires_grad_(True)
    out: dict = {}
    val = cad().balanced_cross_entropy(zl, yd, out=out)
    g, = torch.autograd.grad(val * 3.0, zl)
    assert torch.equal(val.detach(), loss) and torch.equal(out["class_count"], count)
    close(g, 3.0 * ref[1], TIGHT, what + " autograd")
    close(cad().cadence_validation_loss(zd, yd), ref[0], TIGHT, what + " cadence_validation_loss")


def test_balanced_ce_empty_and_out_of_range():
    gen = torch.Generator().manual_seed(2)
    z = bf16(300, 5, gen=gen).to(DEV)
    loss, d, count, weight, status = bce_raw(z, torch.full((300,), -100, device=DEV))
    assert float(loss) == 0.0 and float(d.abs().max()) == 0.0 and int(count.sum()) == 0 and status == 0
    y = torch.randint(0, 5, (300,), generator=gen)
    y[17] = -100
    base = bce_raw(z, y.to(DEV))
    y[17] = 5                                                                      # out of range, not the ignore value
    bad = bce_raw(z, y.to(DEV))
    assert bad[4] == 1 and base[4] == 0
    for a, b in zip(bad[:4], base[:4]):
        assert torch.equal(a, b)
    assert float(bad[1][17].abs().max()) == 0.0
    assert float(bce_raw(z[:0], y[:0].to(DEV))[0]) == 0.0                          # no rows at all


# ---- the stacks -------------------------------------------------------------------------------------------------------------------
def test_gnn_golden():
    z = CR.load_case("gnn_h16")
    cfg, I = CR.config(z), CR.inputs(z, DEV)
    model = cad().GNN(cfg["in_feats"], cfg["H"], cfg["L"], dropout=0.0)
    model.load_state_dict(CR.state(z), strict=True)
    model = model.to(DEV).train()
    x = I["x"].clone().requires_grad_(True)
    out = model(x, I["ei"])
    (out * torch.from_numpy(z["cot.enc"]).to(DEV)).sum().backward()
    close(out, torch.from_numpy(z["out.enc"]), GATE, "gnn_h16 out")
    close(x.grad, torch.from_numpy(z["grad.x"]), GATE, "gnn_h16 grad.x")
    for k, p in model.named_parameters():
        close(p.grad, torch.from_numpy(z["gw." + k]), GATE, f"gnn_h16 gw.{k}")
    assert list(model.state_dict().keys()) == [str(k) for k in z["meta.keys"]]


def test_hierarchical_sage_on_the_neighbour_fixture():
    """The cadence stack is the neighbour model's `gnn`: its weights load under `gnn.*`, its output is the fixture's join input and
    the dict it returns is what the last trim_to_layer leaves."""
    z = CR.load_case("neighbor_h32")
    cfg, I = CR.config(z), CR.inputs(z, DEV)
    model = cad().HierarchicalHeteroGraphSage(cfg["edge_types"], cfg["in_feats"], cfg["H"], cfg["H"] // 2, cfg["L"])
    sd = {k[len("gnn."):]: v for k, v in CR.state(z).items() if k.startswith("gnn.")}
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).train()
    x, trimmed = model(dict(I["x_dict"]), I["ei_dict"], I["edges_per_hop"], I["nodes_per_hop"])
    close(x, torch.from_numpy(z["mid.join_in"]), GATE, "neighbor_h32 gnn output")
    for et, ei in trimmed.items():
        keep = I["ei_dict"][et].shape[1] - sum(I["edges_per_hop"][et][-(cfg["L"] - 1):])
        assert ei.shape[1] == keep and (keep == 0 or int(ei.max()) < x.shape[0]), et
        assert torch.equal(ei, I["ei_dict"][et][:, :keep])


class Head(nn.Module):
    """What `cadence_training_loss` needs of a cadence model: `cad_clf` and `clf`."""

    def __init__(self, hidden, out):
        super().__init__()
        self.cad_clf = cad().cad_clf(hidden, out, dropout=0.0)

    def clf(self, x):
        return cad().run_cad_clf(self.cad_clf, x, self.training)


def test_classifier_head():
    from analysisgnn_amd._abi import AgnnError
    z = CR.load_case("pytorch_eval_h32")
    sd = {k: v for k, v in CR.state(z).items() if k.startswith("cad_clf.")}
    head = Head(16, CR.OUT)
    head.load_state_dict(sd, strict=True)                   # the reference's keys
    head = head.to(DEV).eval()
    enc = torch.from_numpy(z["out.enc"]).float().to(DEV)
    close(head.clf(enc), torch.from_numpy(z["out.logits"]), GATE, "cad_clf in eval mode on the fixture's running statistics")
    with pytest.raises(AgnnError, match="one row"):
        head.train().clf(torch.zeros(1, 16, device=DEV))


def _bf16_weights(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=gen) * 0.1)
            p.copy_(p.bfloat16().float())


def test_training_loss_against_the_restatement():
    """cadence_training_loss with fixed SMOTE draws and permutations: value, d/dx and the classifier's gradients against float64."""
    import smote_ref as R
    from analysisgnn_amd import smote
    mod = cad()
    gen = torch.Generator().manual_seed(17)
    D, k = 16, 3
    y = torch.cat([torch.zeros(130), torch.ones(30), torch.full((12,), 2.0)]).long()[torch.randperm(172, generator=gen)]
    x = bf16(172, D, gen=gen)
    S = R.n_synthetic(y, k)
    choice, gap = torch.randint(0, k - 1, (S,), generator=gen).int(), torch.rand(S, D, generator=gen).float()
    perms = [torch.randperm(m, generator=gen) for m in (130, 130, 120, 120)]
    torch.manual_seed(5)
    model = Head(D, CR.OUT)
    _bf16_weights(model, 6)
    model = model.to(DEV).train()
    sd = {key: v.detach().cpu().clone() for key, v in model.state_dict().items()}
    for epoch, reg in ((None, 0.1), (7, 0.5)):
        sm = smote.SMOTE(dims=D, distance="euclidian", k=k)
        xd = x.to(DEV).requires_grad_(True)
        model.zero_grad(set_to_none=True)
        total, logits, y_over = mod.cadence_training_loss(model, xd, y.to(DEV), sm, reg, epoch=epoch, perms=[p.to(DEV) for p in perms],
                                                          draws=(choice.to(DEV), gap.to(DEV)))
        total.backward()
        tables = {lab: t for lab, t in zip(sm.last_call["labels"],
                                           [sm.last_call["nbr"].cpu().long()[a:b, 1:k] - a for a, b in zip(sm.last_call["t_off"][:-1], sm.last_call["t_off"][1:])])}
        x64 = x.double().requires_grad_(True)
        P = {key: (v.double().requires_grad_(True) if v.is_floating_point() and "running_" not in key else v) for key, v in sd.items()}
        xo, yo, _ = R.fit_generate(x64, y, choice, gap.double(), k=k, distance="euclidian", tables=tables)
        assert torch.equal(yo, y_over.cpu()) and [int((yo == c).sum()) for c in range(3)] == [130, 120, 120]
        ref = CR.training_loss(P, x64, y, xo, yo, reg, epoch, perms)
        names = [key for key in P if key.startswith("cad_clf") and torch.is_tensor(P[key]) and P[key].requires_grad]
        grads = torch.autograd.grad(ref, [x64] + [P[key] for key in names])
        what = f"cadence_training_loss epoch={epoch}"
        close(total, ref, GATE, what)
        close(xd.grad, grads[0], GATE, what + " d/dx")
        for key, g in zip(names, grads[1:]):
            close(dict(model.named_parameters())[key].grad, g, GATE, f"{what} gw.{key}")
        assert tuple(logits.shape) == (370, CR.OUT)


def test_metrics_against_numpy():
    gen = torch.Generator().manual_seed(8)
    logits = bf16(500, CR.OUT, gen=gen)
    y = torch.randint(0, CR.OUT - 1, (500,), generator=gen)
    got = cad().cadence_metrics(logits.to(DEV), y.to(DEV))
    acc, f1 = CR.metrics(logits, y)
    assert abs(got["acc"] - acc) < 1e-12 and abs(got["f1"] - f1) < 1e-9, (got, acc, f1)
