"""SMOTE oversampling and its feature penalty on the HIP kernels (csrc/smote.hip through analysisgnn_amd/smote.py) against the
float64 restatement (tests/smote_ref.py) and the fixtures recorded from the reference (tests/golden/smote_*.npz).

Near ties.  Float64 and fp32 may order two almost equal scores differently.  A query row counts as near-tied when two of the
oracle's ranks 0 .. ksel of it (one more than is compared) are closer than 2e-6 for cosine scores, 2e-6 x the row's largest score
for squared distances; such rows are left out of INDEX comparisons, and every case first asserts on the oracle's own scores
that at most 3 % of its rows are left out.  Scores are compared on all rows.

Tolerances: values 1e-5 and gradients 1e-4 of the tensor's largest entry are the project's gates.  The
squared-distance inputs are scaled to scores of order 1, so that 1e-5 is an absolute and a relative bound at once (fp32 carries
6e-8 per operation; the kernel sums a row in four partial sums)."""
import functools
import os

import numpy as np
import pytest
import torch

import smote_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LAYOUTS = {"ragged": (3, 4, 65, 130), "tiles": (63, 64, 257)}
COS, SQD = 0, 1


def load(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"smote_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def offsets(sizes):
    return [0] + np.cumsum(sizes).tolist()


@functools.lru_cache(maxsize=None)
def selection_case(layout, D, mode):
    """(x fp32 [N, D] on the CPU, rows or None, per segment the oracle's sorted scores and indices) — computed once."""
    sizes = LAYOUTS[layout]
    n = sum(sizes)
    g = torch.Generator().manual_seed(1000 * D + 10 * len(sizes) + mode)
    x = (torch.randn(n + 7, D, generator=g) * (0.7 / D ** 0.5)).float()
    rows = torch.randperm(n + 7, generator=g)[:n].int() if layout == "ragged" else None      # positions -> rows of x, or the identity
    xs = x[rows.long()] if rows is not None else x[:n]
    oracle = []
    off = offsets(sizes)
    for s in range(len(sizes)):
        sc = R.scores(xs[off[s]:off[s + 1]], "euclidian" if mode == SQD else "cosine")
        oracle.append(torch.sort(sc, dim=1, stable=True))
    return x, rows, oracle


@pytest.mark.parametrize("ksel", [1, 4, 8])
@pytest.mark.parametrize("mode", [COS, SQD], ids=["cosine", "sqdist"])
@pytest.mark.parametrize("D", [4, 8, 128, 512])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_row_selection_against_float64(layout, D, mode, ksel):
    from analysisgnn_amd import smote
    x, rows, oracle = selection_case(layout, D, mode)
    sizes = LAYOUTS[layout]
    off = offsets(sizes)
    xd = x.to(DEV)
    rd = rows.to(DEV) if rows is not None else None
    idx, score = smote.row_select(xd, xd, off, off, ksel, mode, rd, rd)
    idx, score = idx.cpu().long(), score.cpu().double()
    left_out = total = 0
    for s, T in enumerate(sizes):
        vals, order = oracle[s]
        got_i, got_s = idx[off[s]:off[s + 1]], score[off[s]:off[s + 1]]
        m = min(ksel, T)
        # nothing leaves its segment; what the segment cannot fill is -1 / +inf
        assert bool(((got_i[:, :m] >= off[s]) & (got_i[:, :m] < off[s + 1])).all())
        assert bool((got_i[:, m:] == -1).all()) and bool(torch.isinf(got_s[:, m:]).all())
        err = float((got_s[:, :m] - vals[:, :m]).abs().max())
        assert err <= 1e-5, f"segment {s}: scores differ by {err:.3e}"
        top = vals[:, :min(ksel + 1, T)]
        margin = 2e-6 if mode == COS else 2e-6 * vals.max(dim=1).values
        gaps = top[:, 1:] - top[:, :-1]
        tied = (gaps < (margin if mode == COS else margin[:, None])).any(dim=1) if top.shape[1] > 1 else torch.zeros(T, dtype=torch.bool)
        left_out += int(tied.sum())
        total += T
        ok = ~tied
        assert torch.equal(got_i[ok][:, :m] - off[s], order[ok][:, :m]), f"segment {s}: indices differ outside near ties"
    print(f"{layout} D={D} mode={mode} ksel={ksel}: {left_out} of {total} rows near-tied")
    assert left_out <= 0.03 * total


@pytest.mark.parametrize("mode", [COS, SQD], ids=["cosine", "sqdist"])
def test_exact_ties_go_to_the_lower_index(mode):
    """A class of 20 distinct rows, each present twice at shuffled positions: every ranking is full of exact ties."""
    from analysisgnn_amd import smote
    g = torch.Generator().manual_seed(5)
    base = (torch.randn(20, 32, generator=g) * 0.12).float()
    ids = torch.arange(20).repeat(2)[torch.randperm(40, generator=g)]
    x = torch.cat([torch.randn(9, 32, generator=g).float() * 0.12, base[ids]])  # a first segment, so that positions are not local indices
    off = [0, 9, 49]
    # the float64 scores of the 20 distinct rows, expanded: twins score exactly alike whatever order a matrix product sums in
    sc = R.scores(base, "euclidian" if mode == SQD else "cosine")[ids][:, ids]
    want = torch.sort(sc, dim=1, stable=True).indices[:, :8] + 9
    xd = x.to(DEV)
    a_i, a_s = smote.row_select(xd, xd, off, off, 8, mode)
    b_i, b_s = smote.row_select(xd, xd, off, off, 8, mode)
    assert torch.equal(a_i, b_i) and torch.equal(a_s, b_s)                       # two runs, the same bits
    assert torch.equal(a_i[9:].cpu().long(), want)
    twins = a_s[9:].cpu()
    assert int((twins[:, 1:] == twins[:, :-1]).sum()) >= 40                      # the ties are exact in fp32 as well


def class_tables(info, k):
    """{label: class-local neighbour table [T, k - 1]} of a call, from SMOTE.last_call (rank 0 dropped)."""
    nbr, t_off = info["nbr"].cpu().long(), info["t_off"]
    return {lab: nbr[t_off[i]:t_off[i + 1], 1:k] - t_off[i] for i, lab in enumerate(info["labels"])}


@pytest.mark.parametrize("name", ["a", "b"])
def test_fit_generate_reproduces_the_reference_run(name):
    from analysisgnn_amd import smote
    g = load(name)
    k, D = int(g["k"]), g["x"].shape[1]
    sm = smote.SMOTE(dims=D, distance="euclidean", k=k)
    draws = (torch.from_numpy(g["choice"]).int().to(DEV), torch.from_numpy(g["gap"]).to(DEV))
    xo, yo = sm.fit_generate(torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV), draws=draws)
    assert yo.dtype == torch.int64 and torch.equal(yo.cpu(), torch.from_numpy(g["y_over"]))
    err = float((xo.cpu() - torch.from_numpy(g["x_over"])).abs().max())
    print(f"smote_{name}: max |x_over - reference| = {err:.3e}")
    assert err <= 1e-5


@functools.lru_cache(maxsize=None)
def grad_case():
    g = torch.Generator().manual_seed(11)
    y = torch.cat([torch.zeros(150), torch.ones(31), torch.full((27,), 2.0), torch.full((2,), 3.0)]).long()[torch.randperm(210, generator=g)]
    x = torch.randn(210, 64, generator=g).float()
    S = R.n_synthetic(y, 3)
    choice = torch.randint(0, 2, (S,), generator=g).int()
    gap = torch.rand(S, 64, generator=g).float()
    w = torch.randn(210 + S, 64, generator=g).float()
    return x, y, choice, gap, w


@pytest.mark.parametrize("distance", ["euclidean", "euclidian"])
def test_gradient_against_float64_autograd(distance):
    from analysisgnn_amd import smote
    x, y, choice, gap, w = grad_case()
    sm = smote.SMOTE(dims=64, distance=distance, k=3)
    grads = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_(True)
        xo, yo = sm.fit_generate(xd, y.to(DEV), draws=(choice.to(DEV), gap.to(DEV)))
        (xo * w.to(DEV)).sum().backward()
        grads.append(xd.grad.clone())
    assert torch.equal(grads[0], grads[1])                                       # two runs, the same bits
    x64 = x.double().requires_grad_(True)
    ro, ryo, info = R.fit_generate(x64, y, choice, gap.double(), k=3, distance=distance, tables=class_tables(sm.last_call, 3))
    assert torch.equal(ryo, yo.cpu()) and torch.equal(info["nb_row"], sm.last_call["nb_row"].cpu().long())
    assert float((xo.detach().cpu().double() - ro.detach()).abs().max()) <= 1e-5
    (ro * w.double()).sum().backward()
    err = float((grads[0].cpu().double() - x64.grad).abs().max()) / float(x64.grad.abs().max())
    print(f"{distance}: dX differs by {err:.3e} of its largest entry")
    assert err <= 1e-4


def test_philox_draws():
    from analysisgnn_amd import smote
    g = torch.Generator().manual_seed(3)
    y = torch.cat([torch.zeros(960), torch.ones(120), torch.full((120,), 2.0)]).long()[torch.randperm(1200, generator=g)]
    x = torch.randn(1200, 128, generator=g).float().to(DEV)
    yd = y.to(DEV)
    sm = smote.SMOTE(dims=128, distance="euclidean", k=3)
    xo, yo = sm.fit_generate(x, yd, call_id=77)
    call = dict(sm.last_call)
    S, D = call["S"], call["D"]
    assert S == R.n_synthetic(y, 3) and S * D >= 1e5
    choice, gap = smote.draws(S, D, 3, 77, call["rng_used"])
    assert int(choice.min()) >= 0 and int(choice.max()) <= 1                    # [0, k - 2]
    assert float(gap.min()) >= 0.0 and float(gap.max()) < 1.0
    mean = float(gap.double().mean())
    print(f"mean gap {mean:.5f} over {S * D} draws, choices {torch.bincount(choice.long()).tolist()}")
    assert abs(mean - 0.5) <= 0.01                                               # 11 standard errors at 1e5 draws
    ro, ryo, _ = R.fit_generate(x.cpu().double(), y, choice.cpu(), gap.cpu().double(), k=3, tables=class_tables(call, 3))
    assert torch.equal(ryo, yo.cpu())
    assert float((xo.cpu().double() - ro).abs().max()) <= 1e-5
    xo2, _ = sm.fit_generate(x, yd, call_id=77)                                  # the same (seed, step, call id): the same bits
    assert torch.equal(xo, xo2)
    xo3, _ = sm.fit_generate(x, yd, call_id=78)
    assert torch.equal(xo3[:1200], xo[:1200]) and not torch.equal(xo3[1200:], xo[1200:])
    # the gradient regenerates the draws of its own call
    xg = x.clone().requires_grad_(True)
    xo4, _ = sm.fit_generate(xg, yd, call_id=77)
    w = torch.randn(xo4.shape, generator=g).float()
    (xo4 * w.to(DEV)).sum().backward()
    x64 = x.cpu().double().requires_grad_(True)
    ro, _, _ = R.fit_generate(x64, y, choice.cpu(), gap.cpu().double(), k=3, tables=class_tables(call, 3))
    (ro * w.double()).sum().backward()
    assert float((xg.grad.cpu().double() - x64.grad).abs().max()) / float(x64.grad.abs().max()) <= 1e-4


def penalty_case(scale, seed=21):
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(3).repeat_interleave(30)[torch.randperm(90, generator=g)]
    y_over = torch.cat([y, torch.arange(3).repeat_interleave(torch.tensor([10, 14, 0]))])[torch.randperm(114, generator=g)]
    x = torch.randn(90, 32, generator=g).float() * scale
    x_over = torch.randn(114, 32, generator=g).float() * scale
    perms = [torch.randperm(n, generator=g) for n in R.n_perms(y_over, y, 60)]
    return x, y, x_over, y_over, perms


def run_penalty(x, y, x_over, y_over, perms, batch_size, threshold=1.0):
    from analysisgnn_amd import smote
    xd, xod = x.to(DEV).requires_grad_(True), x_over.to(DEV).requires_grad_(True)
    base = torch.full((), 0.25, device=DEV)
    v = smote.feature_penalty(base, xod, y_over.to(DEV), xd, y.to(DEV), batch_size=batch_size, threshold=threshold,
                              perms=[p.to(DEV) for p in perms])
    v.backward()
    x64, xo64 = x.double().requires_grad_(True), x_over.double().requires_grad_(True)
    r = 0.25 + R.feature_penalty(xo64, y_over, x64, y, perms, batch_size, threshold)
    r.backward()
    return float(v.detach()), xd.grad.cpu().double(), xod.grad.cpu().double(), float(r.detach()), x64.grad, xo64.grad


def test_feature_penalty_every_row_penalised():
    """Unit-scale rows at D = 32 lie about 8 apart; batch_size = 60 gives bs = 20, so every class (30 rows of x, 30 .. 44 of x_over)
    goes through the permutation cut."""
    case = penalty_case(1.0)
    assert len(case[4]) == 6
    v, gx, gxo, r, rx, rxo = run_penalty(*case, batch_size=60)
    print(f"penalty {v:.6f}, float64 {r:.6f}")
    assert r > 3 * 3.0 and abs(v - r) <= 1e-5 * max(1.0, abs(r))
    assert float((gx - rx).abs().max()) <= 1e-4 * float(rx.abs().max())
    assert float((gxo - rxo).abs().max()) <= 1e-4 * float(rxo.abs().max())
    assert int((gxo.abs().sum(dim=1) > 0).sum()) == 60                          # bs rows of x_over per class, all of them penalised


def test_feature_penalty_zero_below_the_threshold():
    case = penalty_case(0.05)
    v, gx, gxo, r, rx, rxo = run_penalty(*case, batch_size=60)
    assert v == 0.25 and r == 0.25
    assert not gx.any() and not gxo.any() and not rx.any() and not rxo.any()


@pytest.mark.parametrize("threshold", [1.0, 0.0])
def test_feature_penalty_where_originals_meet_themselves(threshold):
    """x_over holds x's own rows: minimum distances of exactly 0, whose gradient is 0, not NaN.  No class is cut (bs = 1000)."""
    from analysisgnn_amd import smote
    x, y, choice, gap, _ = grad_case()
    xo, yo = smote.SMOTE(dims=64, k=3).fit_generate(x.to(DEV), y.to(DEV), draws=(choice.to(DEV), gap.to(DEV)))
    v, gx, gxo, r, rx, rxo = run_penalty(x, y, xo.cpu(), yo.cpu(), [], batch_size=4000, threshold=threshold)
    assert np.isfinite(v) and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gxo).all())
    assert abs(v - r) <= 1e-5 * max(1.0, abs(r))
    assert float((gx - rx).abs().max()) <= 1e-4 * max(float(rx.abs().max()), 1e-30)
    assert float((gxo - rxo).abs().max()) <= 1e-4 * max(float(rxo.abs().max()), 1e-30)
    assert not gxo[:210].any()                                                   # the originals are at distance 0 from themselves


def test_plan_edge_cases_on_the_device():
    from analysisgnn_amd import smote
    from analysisgnn_amd._lib import AgnnError
    g = torch.Generator().manual_seed(9)
    # counts (20, 14, 2, 5, 3): class 1 makes 0 copies, class 2 is below k, class 4 has T = k rows
    y = torch.arange(5).repeat_interleave(torch.tensor([20, 14, 2, 5, 3]))[torch.randperm(44, generator=g)]
    x = torch.randn(44, 16, generator=g).float()
    S = R.n_synthetic(y, 3)
    assert S == 5 * 3 + 3 * 5
    choice, gap = torch.randint(0, 2, (S,), generator=g).int(), torch.rand(S, 16, generator=g).float()
    sm = smote.SMOTE(dims=16, distance="euclidean", k=3)
    xo, yo = sm.fit_generate(x.to(DEV), y.to(DEV), draws=(choice.to(DEV), gap.to(DEV)))
    assert sm.last_call["labels"] == [3, 4] and [c for c, _ in sm.last_plan.skipped] == [0, 1, 2]
    nbr = sm.last_call["nbr"].cpu()
    assert bool((nbr[5:, 3] == -1).all()) and bool((nbr[5:, :3] >= 5).all())    # T = k: the table has T - 1 = 2 columns after rank 0
    ro, ryo, _ = R.fit_generate(x.double(), y, choice, gap.double(), k=3, tables=class_tables(sm.last_call, 3))
    assert torch.equal(ryo, yo.cpu()) and float((xo.cpu().double() - ro).abs().max()) <= 1e-5
    # nothing to add: the input comes back
    xe, ye = x.to(DEV), torch.zeros(44, dtype=torch.int64, device=DEV)
    out = sm.fit_generate(xe, ye)
    assert out[0] is xe and torch.equal(out[1], ye)
    e = torch.zeros(0, 16, device=DEV)
    assert sm.fit_generate(e, torch.zeros(0, dtype=torch.int64, device=DEV))[0] is e
    # generate(): the reference's second entry point
    syn = sm.generate(x[:6].to(DEV), 250, 3, draws=(choice[:12].to(DEV), gap[:12].to(DEV)))
    assert tuple(syn.shape) == (12, 16)
    for bad in (dict(k=1), dict(k=8)):
        with pytest.raises(AgnnError):
            smote.SMOTE(dims=16, **bad).fit_generate(x.to(DEV), y.to(DEV))
    with pytest.raises(AgnnError):
        smote.SMOTE(dims=6, k=3).fit_generate(torch.zeros(44, 6, device=DEV), y.to(DEV))
    with pytest.raises(AgnnError):
        sm.fit_generate(x.double().to(DEV), y.to(DEV))


def test_refused_under_stream_capture(monkeypatch):
    """Both calls read the class counts back, so they cannot become graph nodes: AgnnError before anything is launched or read."""
    from analysisgnn_amd import smote
    from analysisgnn_amd._lib import AgnnError
    x, y, choice, gap, _ = grad_case()
    xd, yd = x.to(DEV), y.to(DEV)
    sm = smote.SMOTE(dims=64, k=3)
    xo, yo = sm.fit_generate(xd, yd, draws=(choice.to(DEV), gap.to(DEV)))
    before = dict(sm.last_call)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(AgnnError, match="captured"):
        sm.fit_generate(xd, yd)
    with pytest.raises(AgnnError, match="captured"):
        sm.generate(xd[:8], 200, 3)
    with pytest.raises(AgnnError, match="captured"):
        smote.feature_penalty(torch.zeros((), device=DEV), xo, yo, xd, yd)
    assert sm.last_call["call_id"] == before["call_id"]                          # no call got as far as a launch
