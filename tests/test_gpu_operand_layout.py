"""Every wrapper family reads its float operands through _lib.rows16 / vec16 ("Operand layout"): the same values
dense, behind a row sum (the gradient arrives with strides (0, 1)) and at element offset 1 of a flat buffer give the same bits.
Shapes: the smallest at which the wrapper's own eligibility test still selects its kernel, a row count that is no multiple of 4
where the kernel allows it, more than one workgroup.  helpers.check_operand_layouts runs the three variants."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import check_operand_layouts  # noqa: E402

DEV = "cuda:0"
N, E_ = 203, 900


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(1000 * len(shape) + sum(shape) + seed)
    return (torch.randn(*shape, generator=g) * scale).float().to(DEV)


@functools.lru_cache(maxsize=None)
def edges(seed=0, n=N, e=E_):
    g = torch.Generator().manual_seed(77 + seed)
    return torch.randint(0, n, (2, e), generator=g).to(DEV)


@functools.lru_cache(maxsize=None)
def csr_pair():
    from analysisgnn_amd.graph import SegSpec, build_csr
    ei = edges()
    return build_csr([SegSpec(ei[0], ei[1], N), SegSpec(ei[1], ei[0], N)])


@functools.lru_cache(maxsize=None)
def hetero():
    from analysisgnn_amd.graph import HeteroIndex
    ets = [("note", "a", "note"), ("note", "b", "note")]
    return ets, HeteroIndex({et: edges(i) for i, et in enumerate(ets)}, {"note": N})


@pytest.mark.parametrize("shared", [True, False], ids=["shared slot", "per-relation slots"])
def test_aggregate(shared):
    from analysisgnn_amd import ops
    ets, hix = hetero()
    spec = ops.AggSpec(fwd=[hix.fwd[e] for e in ets], bwd=[hix.bwd[e] for e in ets], src_id=[0, 0], n_rows=N, mean=True, shared_slot=shared)
    if shared:
        check_operand_layouts(lambda x, s: ops.aggregate(spec, [x], self_t=s), [rand(N, 8), rand(N, 8, seed=1)], {0, 1})
    else:
        check_operand_layouts(lambda x: ops.aggregate(spec, [x]), [rand(N, 8)], {0})


def test_norm_act():
    from analysisgnn_amd import fused
    fn = lambda x, g, b: fused._NormAct.apply(x, g, b, 1e-5, 0.0, fused.POST_RELU, 1)                # noqa: E731
    check_operand_layouts(fn, [rand(N, 20), rand(20, seed=1), rand(20, seed=2)], {0, 1})


def test_skip_act():
    from analysisgnn_amd import fused
    fn = lambda o, x, s: fused._SkipAct.apply(o, x, s, True, 0.0, 1)                                 # noqa: E731
    check_operand_layouts(fn, [rand(N, 20), rand(N, 20, seed=1), rand(1, seed=2)], {1, 2})


def test_attention():
    from analysisgnn_amd import attention
    check_operand_layouts(lambda qkv: attention.attention(qkv, 2), [rand(N, 3 * 16, scale=0.5)], {0})


def test_task_attention():
    from analysisgnn_amd import task_attention
    check_operand_layouts(lambda qkv: task_attention.attention(qkv, 3, 2), [rand(67 * 3, 3 * 16, scale=0.5)], {0})


def test_jk_fused_block(monkeypatch):
    from analysisgnn_amd import jk
    from analysisgnn_amd.core_layers import JumpingKnowledge
    torch.manual_seed(3)
    m = JumpingKnowledge(32, 2).to(DEV)
    M = jk.MIN_ROWS + 2
    xs = [rand(M, 32, seed=t, scale=0.5) for t in range(2)]
    assert jk.kernel_applicable(m, xs)
    P = [p.detach() for p in jk._params(m)]

    def fn(*a):                    # the module's parameters are operands like the layer outputs: handed in where the module keeps them
        monkeypatch.setattr(jk, "_params", lambda module: list(a[2:]))
        return jk.jumping_knowledge(m, list(a[:2]))
    check_operand_layouts(fn, xs + P, {0, 2 + 2})                                                    # x_0 and lstm.bias_ih_l0


def test_hgt_attention_function():
    from analysisgnn_amd import hgt
    from analysisgnn_amd.graph import HeteroIndex
    heads, D = 2, 8
    et = ("note", "to", "note")
    index = HeteroIndex({et: edges()}, {"note": N})
    plan = hgt._CorePlan(["note"], {"note": N}, heads, D, {"note": [0]}, {"note": [(0, et)]}, {0: ("note", 0)}, index, None, 1)
    fn = lambda kqv, wk, wv, p: hgt._HGTCore.apply(plan, wk, wv, p, kqv)[0]                          # noqa: E731
    check_operand_layouts(fn, [rand(N, 3 * heads * D, scale=0.5), rand(heads, D, D, scale=0.3), rand(heads, D, D, seed=1, scale=0.3),
                               rand(1, heads, seed=2)], {0, 1})


def test_rel_edge_aggregate():
    from analysisgnn_amd.core_layers import _RelEdgeAggregate
    fwd, bwd = csr_pair()
    check_operand_layouts(lambda h: _RelEdgeAggregate.apply(fwd, bwd, h, True), [rand(N, 8)], {0})


def test_gated_aggregate():
    from analysisgnn_amd.core_layers import _GatedAggregate
    fwd, bwd = csr_pair()
    fn = lambda a, b, h, c: _GatedAggregate.apply(fwd, bwd, a, b, h, c)                              # noqa: E731
    check_operand_layouts(fn, [rand(N, 8), rand(N, 8, seed=1), rand(N, 8, seed=2), rand(E_, 8, seed=3)], {0, 3})


OFFS, K = (0, 3, 38, 44), 32


def test_grouped_projection():
    from analysisgnn_amd.heads import grouped_projection
    fn = lambda a, w, b: grouped_projection(a, w, b, OFFS, K)                                        # noqa: E731
    check_operand_layouts(fn, [rand(N, 3 * K), rand(OFFS[-1], K, scale=0.2), rand(OFFS[-1], seed=1)], {1, 2})


def test_grouped_in_projection():
    from analysisgnn_amd.heads import grouped_in_projection
    fn = lambda x, w: grouped_in_projection(x, w, OFFS, K)                                           # noqa: E731
    check_operand_layouts(fn, [rand(N, OFFS[-1]), rand(OFFS[-1], K, scale=0.2)], {0, 1})


def test_linear_with_the_weight_gradient_kernel():
    from analysisgnn_amd import linear
    n = linear.MIN_ROWS + 2
    x, w, b = rand(n, 8), rand(12, 8, scale=0.3), rand(12, seed=1)
    assert linear.ENABLED and linear._ok(x) and 12 * 8 <= linear.MAX_OUT_IN        # weight_grad's own test: the kernel, not the library
    check_operand_layouts(linear.linear, [x, w, b], {1, 2})


def test_smote_fit_generate():
    import smote_ref as R
    from analysisgnn_amd import smote
    g = torch.Generator().manual_seed(11)
    y = torch.cat([torch.zeros(150), torch.ones(31), torch.full((27,), 2.0), torch.full((2,), 3.0)]).long()[torch.randperm(210, generator=g)]
    S = R.n_synthetic(y, 3)
    choice, gap = torch.randint(0, 2, (S,), generator=g).int().to(DEV), torch.rand(S, 8, generator=g).float().to(DEV)
    sm = smote.SMOTE(dims=8, distance="euclidean", k=3)
    yd = y.to(DEV)
    check_operand_layouts(lambda x: sm.fit_generate(x, yd, draws=(choice, gap))[0], [rand(210, 8)], {0})


def test_smote_row_select_reads_a_misplaced_matrix():
    from analysisgnn_amd import smote
    from helpers import at_offset
    x = rand(N, 8)
    off = [0, 70, N]
    a = smote.row_select(x, x, off, off, 4, 1)
    xm = at_offset(x)
    b = smote.row_select(xm, xm, off, off, 4, 1)
    assert xm.data_ptr() % 16 == 4 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_pretrain_link_bce():
    from analysisgnn_amd import pretrain
    g = torch.Generator().manual_seed(5)
    cand = torch.randint(0, N, (2, 300), generator=g).to(DEV)
    plan = pretrain.link_plan(cand, cand[:, :100].contiguous(), N)
    check_operand_layouts(lambda z: pretrain.link_bce([plan], [z]), [rand(N, 8, scale=0.5)], {0})
