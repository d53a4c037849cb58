"""agnn_link_bce_fwd_f32 / agnn_link_bce_bwd_f32 (csrc/linkpred.hip) alone, through `pretrain.link_plan` / `pretrain.link_bce`,
against the float64 restatement tests/pretrain_ref.py.  Gates: logits and losses within 1e-5 of the tensor's largest
magnitude, dz within 1e-4, labels, alive counts and confusion counts exact — the float64 logits of every case keep 1e-4 away
from zero (asserted; the seeds below were chosen on the CPU so that it holds)."""
import pytest
import torch

import pretrain_ref as R
from helpers import assert_close_rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 40
LIMIT = 32
WIDTHS = [4, 12, 64, 256, 260, 512]          # one float4, an odd number of them, a sub-wave group, one wave pass, a pass + a tail, two passes
COUNTS = [0, 1, 63, 64, 65, 257]             # around the 64-candidate tile, several tiles


def feats(n, H, seed):
    """Rows whose pairwise dot products have unit scale at every width (logits that neither vanish nor saturate the BCE)."""
    return torch.randn(n, H, generator=torch.Generator().manual_seed(seed)) * H ** -0.25


def special_graph():
    """n = 40 rows, limit 32.  Node 39 has no candidate; node 0 is a hub (70 candidates out, 70 in: its rows of both CSRs take
    more than one 64-entry pass and repeat destinations); self loops (0, 0), (3, 3) and (35, 35) — the last beyond the limit; the
    candidate (5, 7) three times; ends at or above the limit (32 .. 38), one end outside the matrix (45) and a padding slot
    (-1, -1).  True relation: row 2 is empty, (5, 7) and (0, 4) are listed twice, true edges that leave the limit, and some
    candidates' reverse pairs (membership is of the ordered pair)."""
    c = [(0, 1 + j % 38) for j in range(70)] + [(1 + (7 * j) % 38, 0) for j in range(70)]
    c += [(0, 0), (3, 3), (35, 35), (5, 7), (5, 7), (5, 7), (7, 5), (2, 9), (2, 10), (31, 32), (32, 31), (33, 34), (38, 1), (4, 45), (-1, -1),
          (10, 11), (11, 12), (12, 13), (30, 31), (31, 30), (6, 6)]
    t = [(5, 7), (5, 7), (0, 4), (0, 4), (0, 0), (3, 3), (0, 1), (0, 33), (33, 34), (35, 35), (9, 2), (10, 11), (12, 11), (31, 30), (1, 0), (8, 0),
         (15, 0), (6, 6), (38, 1)]
    return torch.tensor(c, dtype=torch.int64).t().contiguous(), torch.tensor(t, dtype=torch.int64).t().contiguous()


def random_graph(E, seed, n=N):
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(0, n, (2, E), generator=g)
    k = E // 2
    true = torch.cat([cand[:, torch.randperm(E, generator=g)[:k]], torch.randint(0, n, (2, 5), generator=g)], dim=1) if E else torch.zeros((2, 0), dtype=torch.int64)
    return cand.contiguous(), true.contiguous()


def reference(tasks, weights):
    """float64: per task (logits, labels, alive, loss, dz, confusion) with dz the gradient of sum_k weights[k] loss_k."""
    out = []
    for (z, cand, true, limit), w in zip(tasks, weights):
        z64 = z.double().requires_grad_(True)
        logits, labels, alive, loss = R.link_task(z64, cand, true, limit)
        if bool(alive.any()):
            assert float(logits.detach()[alive].abs().min()) > 1e-4, "a float64 logit within 1e-4 of zero: choose another seed"
        (loss * w).backward()
        out.append((logits.detach(), labels, alive, loss.detach(), z64.grad, R.confusion(logits.detach(), labels, alive)))
    return out


def run_hip(tasks, weights, n_rows=N):
    """The HIP path on the same tasks: (loss [K], info, [dz_k])."""
    from analysisgnn_amd.pretrain import link_bce, link_plan
    plans = [link_plan(cand.to(DEV), true.to(DEV), z.shape[0], limit) for z, cand, true, limit in tasks]
    zs = [z.to(DEV).requires_grad_(True) for z, _, _, _ in tasks]
    info = {}
    loss = link_bce(plans, zs, info)
    (loss * torch.tensor(weights, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return loss.detach(), info, [z.grad for z in zs], plans, zs


def check(tasks, weights, hip, ref):
    loss, info, dzs = hip[:3]
    for k, (r_logits, r_labels, r_alive, r_loss, r_dz, r_conf) in enumerate(ref):
        assert torch.equal(info["labels"][k].cpu().bool(), r_labels), f"task {k}: labels"
        assert info["counts"][k].cpu().tolist() == r_conf, f"task {k}: alive / confusion counts"
        assert_close_rel(info["logits"][k], r_logits, 1e-5, f"task {k}: logits")
        assert bool((info["logits"][k].detach().cpu()[~r_alive] == 0).all()) and bool((info["g"][k].cpu()[~r_alive] == 0).all())
        assert_close_rel(loss[k], r_loss, 1e-5, f"task {k}: loss")
        assert_close_rel(dzs[k], r_dz, 1e-4, f"task {k}: dz")
        alive = r_conf[0]
        assert float(info["inv_cnt"][k]) == pytest.approx(1.0 / alive if alive else 0.0, rel=1e-6, abs=0.0)


@pytest.mark.parametrize("H", WIDTHS)
def test_every_width_on_the_graph_of_edge_cases(H):
    cand, true = special_graph()
    tasks = [(feats(N, H, 200 + H), cand, true, LIMIT)]
    ref = reference(tasks, [1.7])
    alive = ref[0][2]
    assert 0 < int(alive.sum()) < cand.shape[1] and bool(ref[0][1].any())
    hip = run_hip(tasks, [1.7])
    check(tasks, [1.7], hip, ref)
    dz = hip[2][0].cpu()
    assert float(dz[39].abs().max()) == 0.0 and float(dz[LIMIT:].abs().max()) == 0.0      # no candidate / beyond the limit: zeros, written
    assert float(dz[0].abs().max()) > 0


def test_self_loop_counts_twice():
    """One alive self loop (3, 3) and nothing else: dz[3] = scale * 2 g z[3]."""
    H = 64
    z = feats(N, H, 5)
    cand = torch.tensor([[3], [3]], dtype=torch.int64)
    loss, info, dzs, _, _ = run_hip([(z, cand, cand.clone(), LIMIT)], [1.0])
    g = float(info["g"][0][0])
    assert float(info["labels"][0][0]) == 1 and g < 0
    expect = 2.0 * g * z[3].double()
    assert_close_rel(dzs[0][3], expect, 1e-5, "self loop")
    others = dzs[0].clone()
    others[3] = 0
    assert float(others.abs().max()) == 0.0


@pytest.mark.parametrize("E", COUNTS)
def test_edge_counts_around_the_tile(E):
    cand, true = random_graph(E, 300 + E)
    tasks = [(feats(N, 64, 7), cand, true, LIMIT)]
    ref = reference(tasks, [0.6])
    hip = run_hip(tasks, [0.6])
    check(tasks, [0.6], hip, ref)
    if E == 0:
        assert float(hip[0][0]) == 0.0 and float(hip[2][0].abs().max()) == 0.0


def test_two_tasks_in_one_launch_equal_each_alone():
    H = 256
    c0, t0 = special_graph()
    c1, t1 = random_graph(90, 11, n=57)
    tasks = [(feats(N, H, 21), c0, t0, LIMIT), (feats(57, H, 22), c1, t1, 57)]
    w = [1.0, 0.25]
    ref = reference(tasks, w)
    both = run_hip(tasks, w)
    check(tasks, w, both, ref)
    for k in range(2):
        alone = run_hip([tasks[k]], [w[k]])
        assert torch.equal(alone[0][0], both[0][k]) and torch.equal(alone[2][0], both[2][k])
        assert torch.equal(alone[1]["logits"][0], both[1]["logits"][k])


def test_a_full_table_of_tasks():
    """AGNN_MAX_SEG tasks in one call (the tables travel as kernel arguments), empty ones among them."""
    from analysisgnn_amd import _lib
    H = 12
    tasks, w = [], []
    for k in range(_lib.MAX_SEG):
        cand, true = random_graph([0, 3, 70][k % 3], 500 + k)
        tasks.append((feats(N, H, 600 + k), cand, true, LIMIT if k % 2 else N))
        w.append(0.5 + 0.1 * k)
    check(tasks, w, run_hip(tasks, w), reference(tasks, w))


def test_more_tiles_than_the_final_pass_has_lanes():
    """256 * 64 + 1 candidates in one task are 257 tiles: lane 0 of the final pass adds tiles 0 and 256 before the tree in LDS (every
    other case here has at most 5 tiles).  Tile 256 holds one candidate, the last: it is made a true edge below the limit, so a
    pass that left that tile out would lose one alive candidate and one of tp / fn.  Loss, 1 / alive and the five counts against
    float64; the small task behind it in the table gives the bits it gives alone."""
    H = 4
    c0, t0 = random_graph(256 * 64 + 1, 77)
    c0[:, -1] = torch.tensor([5, 7])
    t0 = torch.cat([t0, c0[:, -1:]], dim=1).contiguous()
    c1, t1 = random_graph(70, 78)
    tasks = [(feats(N, H, 79), c0, t0, LIMIT), (feats(N, H, 80), c1, t1, N)]
    w = [1.0, 0.5]
    ref = reference(tasks, w)
    assert all(int(r[2].sum()) > 0 and bool(torch.isfinite(r[3])) for r in ref) and int(ref[0][2].sum()) > 256 * 32
    assert bool(ref[0][2][-1]) and bool(ref[0][1][-1]), "the one candidate of tile 256 must be alive and labelled positive"
    both = run_hip(tasks, w)
    check(tasks, w, both, ref)
    alone = run_hip([tasks[1]], [w[1]])
    assert torch.equal(alone[0][0], both[0][1]) and torch.equal(alone[1]["inv_cnt"][0], both[1]["inv_cnt"][1])
    assert torch.equal(alone[1]["counts"][0], both[1]["counts"][1]) and torch.equal(alone[1]["logits"][0], both[1]["logits"][1])
    assert torch.equal(alone[2][0], both[2][1])


def test_a_task_without_an_alive_candidate_gives_zero():
    H = 64
    cand = torch.tensor([[33, 34, 2], [1, 35, 39]], dtype=torch.int64)        # every candidate has an end at or above the limit
    true = cand.clone()
    c1, t1 = random_graph(20, 3)
    tasks = [(feats(N, H, 1), cand, true, LIMIT), (feats(N, H, 2), torch.zeros((2, 0), dtype=torch.int64), true, LIMIT),
             (feats(N, H, 3), c1, t1, LIMIT)]
    w = [1.0, 1.0, 1.0]
    loss, info, dzs, _, _ = run_hip(tasks, w)
    for k in (0, 1):
        assert float(loss[k]) == 0.0 and float(info["inv_cnt"][k]) == 0.0 and info["counts"][k].cpu().tolist() == [0] * 5
        assert float(dzs[k].abs().max()) == 0.0 and bool(torch.isfinite(dzs[k]).all())
    assert bool((info["labels"][0] == 0).all()) and bool((info["logits"][0] == 0).all())
    check(tasks, w, (loss, info, dzs), reference(tasks, w))


def test_two_runs_give_the_same_bits():
    cand, true = special_graph()
    c1, t1 = random_graph(257, 9)
    tasks = [(feats(N, 260, 31), cand, true, LIMIT), (feats(N, 260, 32), c1, t1, N)]
    a, b = run_hip(tasks, [1.0, 2.0]), run_hip(tasks, [1.0, 2.0])
    assert torch.equal(a[0], b[0])
    for k in range(2):
        assert torch.equal(a[2][k], b[2][k]) and torch.equal(a[1]["logits"][k], b[1]["logits"][k]) and torch.equal(a[1]["counts"], b[1]["counts"])


def test_gradient_through_the_logits():
    """The logits `link_bce` hands out are differentiable too (a caller's own loss on them): d/dz of sum(c * logits)."""
    from analysisgnn_amd.pretrain import link_bce, link_plan
    cand, true = special_graph()
    z = feats(N, 64, 41)
    coef = torch.randn(cand.shape[1], generator=torch.Generator().manual_seed(1))
    z64 = z.double().requires_grad_(True)
    logits, _, alive, loss = R.link_task(z64, cand, true, LIMIT)
    ((logits * coef.double()).sum() + 0.5 * loss).backward()
    zd = z.to(DEV).requires_grad_(True)
    info = {}
    l = link_bce([link_plan(cand.to(DEV), true.to(DEV), N, LIMIT)], [zd], info)
    ((info["logits"][0] * coef.to(DEV)).sum() + 0.5 * l[0]).backward()
    assert_close_rel(zd.grad, z64.grad, 1e-4, "dz through logits and loss")


def test_forward_and_backward_under_capture():
    """With the plans built beforehand `link_bce` forward + backward is captured once and replayed once: bitwise the eager result."""
    from analysisgnn_amd.pretrain import link_bce, link_plan
    cand, true = special_graph()
    c1, t1 = random_graph(130, 13)
    plans = [link_plan(cand.to(DEV), true.to(DEV), N, LIMIT), link_plan(c1.to(DEV), t1.to(DEV), N, N)]
    zs = [feats(N, 256, 51).to(DEV).requires_grad_(True), feats(N, 256, 52).to(DEV).requires_grad_(True)]
    w = torch.tensor([1.0, 0.5], device=DEV)
    torch.cuda.synchronize()

    def step():
        loss = link_bce(plans, zs)
        return (loss,) + torch.autograd.grad((loss * w).sum(), zs)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        eager = [t.detach().clone() for t in step()]
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in eager) and float(eager[1].abs().max()) > 0
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        captured = step()
    for t in captured:
        t.detach().fill_(float("nan"))
    cg.replay()
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(eager, captured)):
        assert torch.equal(a, b.detach()), f"tensor {j}"
