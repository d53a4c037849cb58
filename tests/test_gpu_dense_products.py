"""The dense product kernels of csrc/wgrad.hip and csrc/gemm.hip through the C ABI, so that no Python dispatch threshold stands
between a test and the kernel: agnn_wgrad_f32, agnn_wgrad_batch_f32, agnn_grad_epilogue_f32, agnn_gemm_nt_f32, agnn_gemm_nn_f32,
agnn_gemm_nt2_f32.

Every case asserts two things.

1. Exact on integers.  Operands (and biases) are integers of {-2 .. 2} stored as float32.  Every product and every partial sum,
   in whatever order, is then an integer below 2^24, so float32 arithmetic is exact whatever the slicing, the slab order or the
   MFMA pairing: the result must be `torch.equal` to the float64 product.  A dropped, doubled or wrongly masked row, a wrong seam,
   a missing or repeated slab term changes an integer.  The 2^24 bound is asserted on the sum of the |products|.

2. Nothing read or written outside the windows.  Every operand lies in ONE larger allocation filled with NaN: guard rows in front
   of the matrix and behind it, a leading dimension wider than the row.  The kernels neutralise rows that are out of range by a
   0 / 1 mask and clamp addresses instead of branching, so a read outside the [n, width] window reaches the arithmetic as NaN
   and shows in the result (and, lying inside the allocation, cannot fault).  Results are column blocks of NaN-filled buffers
   (helpers.Guarded): every element inside written, every one outside still NaN.  The workspace has exactly the size the
   *_workspace_bytes call reports, is filled with 0xFF bytes (NaN) and is followed by a sentinel region that must keep its bytes.

A third, small group runs unit-normal operands under the project's parity convention (profiles/dense_product_parity.md):

    ratio = kernel_err / max(float32_reference_err, 2^-21),      both errors max |x - ref64| / max |ref64|

with the same product evaluated in float32 on the CPU as the yardstick; `pytest -s` prints one PARITY line per tensor, and
MARGIN[kind] is twice the worst ratio measured on an MI355X, rounded up to a power of two, at least 4 and at most 16.

Row counts of the weight-gradient sweep: `make_plan` cuts n rows into S <= 64 slices of an even length >= 64 (fewer rows: one
slice), and `wgrad_tile` walks a slice in chunks of 16 rows, three per trip: the loop on running offsets while the chunks it
fetches (two ahead) lie inside the MATRIX, then the loop that clamps row numbers, then up to three chunks under the 0 / 1 row
mask.  ROWS holds the smallest n per combination of those paths (found by running the plan and the loop conditions on the CPU)."""
import functools
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import ROOT, Guarded  # noqa: E402

DEV = torch.device("cuda", 0)
NAN = float("nan")
AGNN_OK, AGNN_EINVAL = 0, -22                           # include/agnn.h
FLOOR = 2.0 ** -21
EXACT = 2 ** 24                                         # integers below it are float32 values, and so are their sums
SENTINEL = 4096                                         # bytes behind the workspace that no kernel may touch
# worst measured ratio (profiles/dense_product_parity.md): wgrad dw 0.43, db 0.26, the same through the batched call; gemm nt, nn and nt2
# 0.49 each — every kernel error lies below the 2^-21 floor, twice the worst ratio below 1, so every kind gets the rule's minimum of 4
MARGIN = {"wgrad.dw": 4.0, "wgrad.db": 4.0, "wgrad_batch.dw": 4.0, "wgrad_batch.db": 4.0, "gemm_nt": 4.0, "gemm_nn": 4.0, "gemm_nt2": 4.0}


# ---------------------------------------------------------------------------------------------------------------------
# operands, workspaces, references
# ---------------------------------------------------------------------------------------------------------------------
class _Window:
    """`vals` [rows, cols] as a kernel operand inside one NaN-filled allocation: `guard` rows of NaN in front of the matrix and
    behind it, `ld - cols` NaN columns after every row.  `align` bytes: what the kernel asks of the pointer (the guard rows keep
    it as long as `ld` is a multiple of align / 4 floats)."""

    def __init__(self, vals, ld, align, guard=3):
        rows, cols = vals.shape
        assert ld >= cols and (ld * 4) % align == 0
        host = torch.full((rows + 2 * guard, ld), NAN, dtype=torch.float32)
        host[guard:guard + rows, :cols] = vals
        self.buf = host.to(DEV)
        self.view = self.buf[guard:guard + rows, :cols]
        self.ptr, self.ld, self.shape = self.view.data_ptr(), ld, (rows, cols)
        assert self.ptr % align == 0


class _Workspace:
    """Exactly `nbytes` of 0xFF for the kernel, `SENTINEL` more bytes of 0xFF behind them that must stay as they are."""

    def __init__(self, nbytes):
        assert nbytes > 0
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + SENTINEL,), 0xFF, dtype=torch.uint8, device=DEV)
        self.ptr = self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.nbytes:] == 0xFF).all()), f"{what}: written behind the workspace"


def _ints(g, *shape, nonzero_col0=False):
    """Integers of {-2 .. 2} as float32.  `nonzero_col0`: no zero in column 0, so that every single ROW of a weight-gradient
    operand pair contributes to dw[0, 0] and db[0] — losing or doubling any one row changes the result for every seed."""
    v = torch.randint(-2, 3, shape, generator=g).float()
    if nonzero_col0:
        v[:, 0][v[:, 0] == 0] = 1.0
    return v


def _exact_wgrad(dy, x):
    """(dw, db) of the float64 product as float32, after asserting that every partial sum in any order is below 2^24."""
    assert float((dy.abs().double().t() @ x.abs().double()).max()) < EXACT and float(dy.abs().double().sum(0).max()) < EXACT
    dw, db = dy.double().t() @ x.double(), dy.double().sum(0)
    assert float(dw.abs().max()) < EXACT and float(db.abs().max()) < EXACT
    return dw.float(), db.float()


def _compare(kind, got, ref64, ref32, what):
    """got (kernel, float32) against ref64 within MARGIN[kind] * max(rel_err(ref32, ref64), 2^-21) of max |ref64|."""
    got, ref32 = got.detach().cpu().double(), ref32.double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} NaN in the result"
    scale = float(ref64.abs().max())
    assert scale > 0, what
    err = float((got - ref64).abs().max()) / scale
    unit = max(float((ref32 - ref64).abs().max()) / scale, FLOOR)
    print(f"PARITY kind={kind} ratio={err / unit:.3f} err={err:.3e} f32_err={unit:.3e} what={what}")
    assert err <= MARGIN[kind] * unit, f"{what}: rel err {err:.3e} > {MARGIN[kind]:g} * {unit:.3e} (float32 evaluation, floor 2^-21)"


def _lib():
    from analysisgnn_amd import _lib as L
    return L, L.load(), L.stream_ptr(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# agnn_wgrad_f32
# ---------------------------------------------------------------------------------------------------------------------
def _wgrad(dy, x, with_db, ld_dy=None, ld_x=None, ld_dw=None):
    """One agnn_wgrad_f32 call on CPU operands dy [n, out], x [n, in]: (dw, db or None) on the device, windows, destinations,
    workspace and sentinel checked."""
    L, lib, stream = _lib()
    (n, o), i = dy.shape, x.shape[1]
    wdy, wx = _Window(dy, ld_dy or o + 2, 8), _Window(x, ld_x or i + 2, 8)
    dw = Guarded(o, i, ld=ld_dw or i + 2)
    db = Guarded(1, o) if with_db else None
    ws = _Workspace(int(lib.agnn_wgrad_workspace_bytes(n, o, i)))
    L.check(lib.agnn_wgrad_f32(wdy.ptr, wdy.ld, wx.ptr, wx.ld, n, o, i, dw.view.data_ptr(), dw.ld, db.view.data_ptr() if with_db else None,
                               ws.ptr, ws.nbytes, stream), "agnn_wgrad_f32")
    torch.cuda.synchronize()
    what = f"wgrad n={n} {o}x{i}"
    ws.check(what)
    dw.check(what + " dw")
    if with_db:
        db.check(what + " db")
    return dw.view, (db.view[0] if with_db else None)


def _wgrad_exact(n, o, i, with_db, **ld):
    g = torch.Generator().manual_seed(100003 * n + 131 * o + i)
    dy, x = _ints(g, n, o, nonzero_col0=True), _ints(g, n, i, nonzero_col0=True)
    ref_w, ref_b = _exact_wgrad(dy, x)
    dw, db = _wgrad(dy, x, with_db, **ld)
    bad = (dw.cpu() != ref_w).nonzero()
    assert torch.equal(dw.cpu(), ref_w), f"dw differs at {len(bad)} of {ref_w.numel()} elements, first {bad[0].tolist()}"
    if with_db:
        assert torch.equal(db.cpu(), ref_b), f"db differs at {(db.cpu() != ref_b).nonzero().flatten().tolist()[:8]}"


ROWS = [1, 2, 3, 15, 16,                  # one slice, one masked chunk, odd and even last row
        17, 31, 32,                       # two masked chunks
        33, 47,                           # three masked chunks
        48, 49, 50, 63, 64,               # the clamped loop once, then no / one masked chunk
        65, 79, 80, 81,                   # two slices, masked chunks only
        93, 95, 96, 97,                   # the first slice takes the running-offset loop once, the last the clamped loop or masked chunks
        129, 130, 131,                    # three slices, the last shorter by 3 / 2 / 1 rows
        513, 577,                         # 9 / 10 slices: the reduction's `k += 8` stride takes a second term
        1000, 1025,                       # 16 / 17 slices, a short last one (40 / 33 rows)
        4033,                             # S = 64 (the cap) with a last slice of ONE row
        4097, 4157,                       # 66-row slices: running offsets once + 2 masked chunks; near the end the clamped loop + 2 masked chunks
        6401, 6449,                       # 102-row slices: running offsets twice; last slice clamped + 2 masked / running + clamped in the one before it
        12801, 12833, 12887]              # 202-row slices: running offsets four times; the last slice mixes running, clamped and 1 - 2 masked chunks


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("n", ROWS)
def test_wgrad_row_counts_exact(n, with_db):
    """out = in = 2: kilobytes of data, one tile, every slicing and every path of the K loop."""
    _wgrad_exact(n, 2, 2, with_db)


WIDTHS = [(2, 2), (2, 130), (130, 2), (126, 128), (128, 126), (128, 128), (130, 258), (256, 256)]


@pytest.mark.parametrize("n", [131, 513])
@pytest.mark.parametrize("out_f,in_f", WIDTHS)
def test_wgrad_widths_exact(out_f, in_f, n):
    """Partial and full 128 x 128 tiles along either side, one to three tiles along `in`, lanes whose columns lie past the matrix."""
    _wgrad_exact(n, out_f, in_f, True)


def test_wgrad_reduction_beyond_its_block_cap_exact():
    """512 x 514 at n = 70: 512 * 257 column pairs are 4112 blocks of 32, above launch_slab_reduce's cap of 4096 — the grid-stride
    loop of the reduction takes a second trip in the first 16 blocks."""
    assert (512 * (514 // 2) + 31) // 32 > 4096
    _wgrad_exact(70, 512, 514, True)


def test_wgrad_wide_leading_dimensions_exact():
    _wgrad_exact(131, 130, 258, True, ld_dy=256, ld_x=512, ld_dw=328)


# ---------------------------------------------------------------------------------------------------------------------
# agnn_wgrad_batch_f32
# ---------------------------------------------------------------------------------------------------------------------
def _batch(items):
    """One agnn_wgrad_batch_f32 call.  items: dicts with `dy`, `x` (_Window), `dw` (device view of a Guarded), `db` (device
    vector or None).  Returns the workspace after its sentinel check."""
    L, lib, stream = _lib()
    arr = (L.WgradItem * len(items))()
    for a, it in zip(arr, items):
        a.dy, a.x, a.dw, a.db = it["dy"].ptr, it["x"].ptr, it["dw"].data_ptr(), L.ptr(it["db"])
        a.ld_dy, a.ld_x, a.ld_dw = it["dy"].ld, it["x"].ld, it["dw"].stride(0)
        a.n, a.out_f, a.in_f = it["dy"].shape[0], it["dy"].shape[1], it["x"].shape[1]
    ws = _Workspace(int(lib.agnn_wgrad_batch_workspace_bytes(len(items), arr)))
    L.check(lib.agnn_wgrad_batch_f32(len(items), arr, ws.ptr, ws.nbytes, stream), "agnn_wgrad_batch_f32")
    torch.cuda.synchronize()
    ws.check("wgrad_batch")
    return ws


def _batch_group(shapes, order=None, seed=0, ints=True):
    """Items (n, out, in, with_db) with fresh operands and destinations, launched in `order`: per item (dw, db or None, dy, x)."""
    g = torch.Generator().manual_seed(seed)
    made = []
    for n, o, i, with_db in shapes:
        dy = _ints(g, n, o, nonzero_col0=True) if ints else torch.randn(n, o, generator=g)
        x = _ints(g, n, i, nonzero_col0=True) if ints else torch.randn(n, i, generator=g)
        made.append(dict(dy_cpu=dy, x_cpu=x, dy=_Window(dy, o + 2, 8), x=_Window(x, i + 4, 8), gw=Guarded(o, i, ld=i + 2),
                         gb=Guarded(1, o) if with_db else None))
    for m in made:
        m["dw"], m["db"] = m["gw"].view, (m["gb"].view[0] if m["gb"] else None)
    _batch([made[k] for k in (order or range(len(made)))])
    for k, m in enumerate(made):
        m["gw"].check(f"item {k} dw")
        if m["gb"]:
            m["gb"].check(f"item {k} db")
    return made


def _assert_group_exact(made):
    for k, m in enumerate(made):
        ref_w, ref_b = _exact_wgrad(m["dy_cpu"], m["x_cpu"])
        assert torch.equal(m["dw"].cpu(), ref_w), f"item {k}: dw differs at {int((m['dw'].cpu() != ref_w).sum())} elements"
        if m["db"] is not None:
            assert torch.equal(m["db"].cpu(), ref_b), f"item {k}: db"


def test_wgrad_batch_one_item_exact():
    _assert_group_exact(_batch_group([(131, 130, 258, True)]))


def test_wgrad_batch_item_limit_exact():
    """AGNN_WGRAD_BATCH_MAX_ITEMS tiny items in one launch; one more is refused."""
    L, lib, stream = _lib()
    n_max = L.WGRAD_BATCH_MAX_ITEMS
    made = _batch_group([(1 + 7 * k, 2, 2 + 2 * (k % 3), k % 2 == 0) for k in range(n_max)], seed=1)
    _assert_group_exact(made)
    arr = (L.WgradItem * (n_max + 1))()
    for k, a in enumerate(arr):
        m = made[k % n_max]
        a.dy, a.x, a.dw, a.db = m["dy"].ptr, m["x"].ptr, m["dw"].data_ptr(), None
        a.ld_dy, a.ld_x, a.ld_dw = m["dy"].ld, m["x"].ld, m["dw"].stride(0)
        a.n, a.out_f, a.in_f = m["dy"].shape[0], m["dy"].shape[1], m["x"].shape[1]
    before = [m["gw"].buf.clone() for m in made]
    ws = _Workspace(1 << 20)
    assert int(lib.agnn_wgrad_batch_workspace_bytes(n_max + 1, arr)) == 0
    assert lib.agnn_wgrad_batch_f32(n_max + 1, arr, ws.ptr, ws.nbytes, stream) == AGNN_EINVAL
    torch.cuda.synchronize()
    assert bool((ws.buf == 0xFF).all())
    for m, b in zip(made, before):
        assert torch.equal(m["gw"].buf.view(torch.int32), b.view(torch.int32))


# rows 1, 17, 64, 65, 200, 513 on 2 x 2, 130 x 258, 128 x 384 and 256 x 258; 256 * 129 column pairs are 1032 blocks of 32, above the
# batched reduction's cap of 1024 blocks per item, and its 513 rows are 9 slices (a second term of the `k += 8` stride)
MIXED = [(1, 2, 2, True), (17, 130, 258, False), (64, 128, 384, True), (65, 2, 2, False), (200, 130, 258, True), (513, 256, 258, True)]


def test_wgrad_batch_mixed_group_exact_in_either_order():
    """Items of different row counts, widths and bias presence in one launch.  The slice count is shared by the batch, the item
    order moves every item's workgroups and slabs: the sums are integers, so each item's result is the same either way."""
    assert (256 * (258 // 2) + 31) // 32 > 1024
    fwd = _batch_group(MIXED, seed=2)
    _assert_group_exact(fwd)
    rev = _batch_group(MIXED, order=list(range(len(MIXED)))[::-1], seed=2)
    _assert_group_exact(rev)
    for k, (a, b) in enumerate(zip(fwd, rev)):
        assert torch.equal(a["dw"], b["dw"]) and (a["db"] is None or torch.equal(a["db"], b["db"])), f"item {k} depends on the item order"


def test_wgrad_batch_two_column_blocks_of_one_matrix_exact():
    """Two items share dy; their dw are the column blocks [0, 128) and [128, 176) of ONE [64, 176] matrix (ld_dw > in_f)."""
    g = torch.Generator().manual_seed(3)
    n, o, i0, i1 = 300, 64, 128, 48
    dy, x0, x1 = _ints(g, n, o, nonzero_col0=True), _ints(g, n, i0, nonzero_col0=True), _ints(g, n, i1, nonzero_col0=True)
    wdy = _Window(dy, o + 2, 8)
    dw, db = Guarded(o, i0 + i1, ld=i0 + i1 + 6), Guarded(1, o)
    _batch([dict(dy=wdy, x=_Window(x0, i0 + 2, 8), dw=dw.view[:, :i0], db=db.view[0]),
            dict(dy=wdy, x=_Window(x1, i1 + 2, 8), dw=dw.view[:, i0:], db=None)])
    dw.check("dw in two blocks")
    db.check("db")
    ref_w, ref_b = _exact_wgrad(dy, torch.cat((x0, x1), dim=1))
    assert torch.equal(dw.view.cpu(), ref_w) and torch.equal(db.view[0].cpu(), ref_b)


# ---------------------------------------------------------------------------------------------------------------------
# agnn_grad_epilogue_f32
# ---------------------------------------------------------------------------------------------------------------------
def test_grad_epilogue_exact():
    """The product set of test_gpu_grad_delivery (a pair of column blocks, the 281-column block on the scalar store path, four
    relation blocks with the root block four times, a wide-ld destination) on integer operands against float64: that file's
    bit-for-bit comparison with agnn_wgrad_batch_f32 thereby reaches a real reference."""
    import test_gpu_grad_delivery as gd
    L, lib, stream = _lib()
    products = gd._products()
    g = torch.Generator().manual_seed(4)
    for p in products:                                   # the same tensors (dy of the column-block pair stays shared), integer values
        for key in ("dy", "x"):
            p[key].copy_(_ints(g, *p[key].shape, nonzero_col0=True))
    dest = gd._destinations(products)
    garr = (L.GradItem * len(products))()
    for a, p, (recs, dbs) in zip(garr, products, dest):
        (n, o), i = p["dy"].shape, p["x"].shape[1]
        a.dy, a.x, a.ld_dy, a.ld_x, a.n, a.out_f, a.in_f = p["dy"].data_ptr(), p["x"].data_ptr(), o, i, n, o, i
        a.n_dw, a.n_db = len(recs), len(dbs)
        for k, (c0, c1, view, _) in enumerate(recs):
            a.dw[k].p, a.dw[k].ld, a.dw[k].c0, a.dw[k].c1 = view.data_ptr(), view.stride(0), c0, c1
        for k, d in enumerate(dbs):
            a.db[k] = d.view.data_ptr()
    ws = _Workspace(int(lib.agnn_grad_epilogue_workspace_bytes(len(products), garr)))
    L.check(lib.agnn_grad_epilogue_f32(len(products), garr, 0, None, ws.ptr, ws.nbytes, stream), "agnn_grad_epilogue_f32")
    torch.cuda.synchronize()
    ws.check("grad_epilogue")
    n_rec = 0
    for k, (p, (recs, dbs)) in enumerate(zip(products, dest)):
        ref_w, ref_b = _exact_wgrad(p["dy"].cpu(), p["x"].cpu())
        for j, (c0, c1, view, guard) in enumerate(recs):
            guard.check(f"product {k}, record {j}")
            assert torch.equal(view.cpu(), ref_w[:, c0:c1]), f"product {k}, record {j}: columns [{c0}, {c1})"
            n_rec += 1
        for j, d in enumerate(dbs):
            d.check(f"product {k}, bias {j}")
            assert torch.equal(d.view[0].cpu(), ref_b), f"product {k}, bias {j}"
    assert n_rec == 15                                   # 3 + 2 column blocks + 1 odd block + (4 + 4) + 1 wide: nothing of the set got lost


# ---------------------------------------------------------------------------------------------------------------------
# agnn_gemm_nt_f32, agnn_gemm_nn_f32, agnn_gemm_nt2_f32
# ---------------------------------------------------------------------------------------------------------------------
def _gemm(kind, a, w, bias, K0=None, rows_c=None):
    """C = a w^T (+ bias) on CPU operands a [M, K], w [N, K] through `kind` = nt / nn / nt2 (nn: the kernel gets w^T as [K, N];
    nt2: a as the two column blocks [:, :K0] and [:, K0:] with leading dimensions of their own).  Returns C on the device, every
    window, the destination's surroundings and (nt2) the seam checked by the NaN that lies behind each block's columns."""
    L, lib, stream = _lib()
    (M, K), N = a.shape, w.shape[0]
    c = Guarded(M, N, ld=N + 4)
    wb = _Window(bias.view(1, N), N, 16, guard=1) if bias is not None else None
    pb = wb.ptr if wb is not None else None
    if kind == "nt2":
        a0, a1, ww = _Window(a[:, :K0], K0 + 4, 16), _Window(a[:, K0:], K - K0 + 12, 16), _Window(w, K + 4, 16)
        assert a0.ld != a1.ld
        rc = lib.agnn_gemm_nt2_f32(a0.ptr, a0.ld, K0, a1.ptr, a1.ld, K - K0, ww.ptr, ww.ld, pb, M, N, c.view.data_ptr(), c.ld, stream)
    else:
        wa = _Window(a, K + 4, 16)
        ww = _Window(w.t().contiguous(), N + 8, 16) if kind == "nn" else _Window(w, K + 4, 16)
        fn = lib.agnn_gemm_nn_f32 if kind == "nn" else lib.agnn_gemm_nt_f32
        rc = fn(wa.ptr, wa.ld, ww.ptr, ww.ld, pb, M, N, K, c.view.data_ptr(), c.ld, stream)
    L.check(rc, f"agnn_gemm_{kind}_f32")
    torch.cuda.synchronize()
    c.check(f"gemm_{kind} M={M} N={N} K={K}")
    return c.view


def _exact_gemm(a, w, bias):
    r = a.double() @ w.double().t()
    bound = a.abs().double() @ w.abs().double().t()
    if bias is not None:
        r, bound = r + bias.double(), bound + bias.abs().double()
    assert float(bound.max()) < EXACT
    return r.float()


def _assert_gemm_exact(kind, a, w, bias, ref, K0=None):
    c = _gemm(kind, a, w, bias, K0)
    ref = ref.to(DEV)
    if not torch.equal(c, ref):
        bad = (c != ref).nonzero()
        raise AssertionError(f"gemm_{kind}: {len(bad)} of {ref.numel()} elements differ, first (row, column) {bad[0].tolist()}")


GEMM_M = [1, 63, 64, 65, 127, 128, 129, 1025]      # around the 64-row wave and the 128-row tile; 1025: nine row tiles — one full group of
GEMM_N = [64, 128, 192]                            # the XCD tile map and a second with seven empty slots, a last tile of one row
GEMM_K = [16, 32, 48, 80]                          # one, two, three (odd) and five K steps: every clamp of the prefetch to `last`


@pytest.mark.parametrize("K", GEMM_K)
@pytest.mark.parametrize("N", GEMM_N)
@pytest.mark.parametrize("M", GEMM_M)
@pytest.mark.parametrize("kind", ["nt", "nn"])
def test_gemm_narrow_tiles_exact(kind, M, N, K):
    """k_gemm_nt<64, NN>: every M x N x K of the lists above, with and without bias."""
    g = torch.Generator().manual_seed(10007 * M + 101 * N + K)
    a, w, bias = _ints(g, M, K), _ints(g, N, K), _ints(g, N)
    _assert_gemm_exact(kind, a, w, bias, _exact_gemm(a, w, bias))
    _assert_gemm_exact(kind, a, w, None, _exact_gemm(a, w, None))


@pytest.mark.parametrize("K0,K1", [(16, 16), (16, 48), (48, 16), (32, 32)])
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("M", [1, 129, 1025])
def test_gemm_nt2_narrow_tiles_exact(M, N, K0, K1):
    """The seam on the first step, on an even and on an odd later step, against float64 (not against gemm_nt): a0's columns end
    where NaN begins, so a step that reads the wrong block at the seam shows."""
    g = torch.Generator().manual_seed(10007 * M + 101 * N + 7 * K0 + K1)
    a, w, bias = _ints(g, M, K0 + K1), _ints(g, N, K0 + K1), _ints(g, N)
    _assert_gemm_exact("nt2", a, w, bias, _exact_gemm(a, w, bias), K0)
    _assert_gemm_exact("nt2", a, w, None, _exact_gemm(a, w, None), K0)


def _wide_shape():
    """(M, N) of the wide-tile cases: at N = 2048, the fewest full row tiles that `launch_gemm` (csrc/gemm.hip) sends to the
    128-wide kernels, plus one row.

    WHY THESE M AND N.  The rule as committed is
        narrow = (N % 128) != 0 || ceil(M / 128) * (N / 128) < 512
    and only `!narrow` launches k_gemm_nt<128, ...>.  The threshold is read from the source line here, so that a changed rule
    fails this function (re-derive the case) instead of letting the cases below fall silently to the 64-wide side.  With 512:
    N = 2048 has 16 column tiles, 31 row tiles stay narrow (496), 32 reach 512, and M = 32 * 128 + 1 = 4097 has 33 row tiles
    (33 * 16 = 528 >= 512): four full groups of eight in the XCD tile map, a fifth with seven empty slots, and a last row tile
    of ONE row."""
    src = open(os.path.join(ROOT, "analysisgnn_amd", "csrc", "gemm.hip")).read()
    m = re.search(r"const bool narrow = \(N % 128\) != 0 \|\| tiles_m \* \(N / 128\) < (\d+);", src)
    assert m, "launch_gemm's dispatch rule is not the one this case was derived from: re-derive the wide-tile shape"
    need, N = int(m.group(1)), 2048
    M = -(-need // (N // 128)) * 128 + 1
    assert N % 128 == 0 and -(-M // 128) * (N // 128) >= need          # takes BN = 128 ...
    assert (-(-M // 128) - 2) * (N // 128) < need                       # ... and with one full row tile fewer it would not
    return M, N


@functools.lru_cache(maxsize=None)
def _wide_case(K, ints):
    """Operands and references of the wide shape, computed once per K: (a, w, bias, float64 product + bias as float32 / float64,
    float32 evaluation or None).  nt, nn and nt2 compute the same product and share it."""
    M, N = _wide_shape()
    g = torch.Generator().manual_seed(K + (0 if ints else 1000))
    if ints:
        a, w, bias = _ints(g, M, K), _ints(g, N, K), _ints(g, N)
        return a, w, bias, _exact_gemm(a, w, bias), None
    a, w, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    return a, w, bias, a.double() @ w.double().t() + bias.double(), a @ w.t() + bias


@pytest.mark.parametrize("kind,K,K0", [("nt", 16, None), ("nt", 48, None), ("nn", 16, None), ("nn", 48, None), ("nt2", 48, 16)])
def test_gemm_wide_tiles_exact(kind, K, K0):
    """k_gemm_nt<128, false>, <128, true> and <128, false, true> at the shape of _wide_shape() (today 4097 x 2048)."""
    a, w, bias, ref, _ = _wide_case(K, True)
    _assert_gemm_exact(kind, a, w, bias, ref, K0)


def test_gemm_refusals_and_no_rows():
    L, lib, stream = _lib()
    g = torch.Generator().manual_seed(5)
    a, w = _Window(_ints(g, 8, 96), 100, 16), _Window(_ints(g, 128, 96), 100, 16)
    c = Guarded(8, 128, ld=132)
    for fn in (lib.agnn_gemm_nt_f32, lib.agnn_gemm_nn_f32):
        assert fn(a.ptr, a.ld, w.ptr, w.ld, None, 8, 96, 32, c.view.data_ptr(), c.ld, stream) == AGNN_EINVAL      # N no multiple of 64
        assert fn(a.ptr, a.ld, w.ptr, w.ld, None, 8, 64, 24, c.view.data_ptr(), c.ld, stream) == AGNN_EINVAL      # K no multiple of 16
        assert fn(a.ptr, a.ld, w.ptr, w.ld, None, 0, 64, 32, c.view.data_ptr(), c.ld, stream) == AGNN_OK          # no rows: nothing to do
    nt2 = lambda K0, K1, M: lib.agnn_gemm_nt2_f32(a.ptr, a.ld, K0, a.ptr + 4 * 48, a.ld, K1, w.ptr, w.ld, None, M, 64, c.view.data_ptr(),      # noqa: E731
                                                  c.ld, stream)
    assert nt2(24, 16, 8) == AGNN_EINVAL and nt2(16, 40, 8) == AGNN_EINVAL and nt2(16, 32, 0) == AGNN_OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(c.buf).all()), "a refused call or one without rows wrote to C"


# ---------------------------------------------------------------------------------------------------------------------
# unit-normal operands: the kernels' rounding against the float32 evaluation's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [131, 513, 4097])
def test_wgrad_float_parity(n):
    """130 x 258 through agnn_wgrad_f32 and as the one item of agnn_wgrad_batch_f32 (which cuts the rows differently)."""
    o, i = 130, 258
    g = torch.Generator().manual_seed(n)
    dy, x = torch.randn(n, o, generator=g), torch.randn(n, i, generator=g)
    w64, b64 = dy.double().t() @ x.double(), dy.double().sum(0)
    w32, b32 = dy.t() @ x, dy.sum(0)
    dw, db = _wgrad(dy, x, True)
    _compare("wgrad.dw", dw, w64, w32, f"n={n}")
    _compare("wgrad.db", db, b64, b32, f"n={n}")
    m = dict(dy=_Window(dy, o + 2, 8), x=_Window(x, i + 2, 8), gw=Guarded(o, i, ld=i + 2), gb=Guarded(1, o))
    m["dw"], m["db"] = m["gw"].view, m["gb"].view[0]
    _batch([m])
    m["gw"].check("dw")
    m["gb"].check("db")
    _compare("wgrad_batch.dw", m["dw"], w64, w32, f"n={n}")
    _compare("wgrad_batch.db", m["db"], b64, b32, f"n={n}")


@pytest.mark.parametrize("kind", ["nt", "nn", "nt2"])
def test_gemm_float_parity_narrow(kind):
    M, N, K = 129, 192, 80
    g = torch.Generator().manual_seed(6)
    a, w, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    c = _gemm(kind, a, w, bias, 48 if kind == "nt2" else None)
    _compare("gemm_" + kind, c, a.double() @ w.double().t() + bias.double(), a @ w.t() + bias, f"{M}x{N}x{K}")


@pytest.mark.parametrize("kind", ["nt", "nn", "nt2"])
def test_gemm_float_parity_wide(kind):
    a, w, bias, r64, r32 = _wide_case(48, False)
    c = _gemm(kind, a, w, bias, 16 if kind == "nt2" else None)
    _compare("gemm_" + kind, c, r64, r32, f"{a.shape[0]}x{w.shape[0]}x48")
