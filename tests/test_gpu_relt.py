"""The relation-transform kernels (csrc/relt.hip), each called directly through its C entry point (agnn_relt_fwd_f32,
agnn_relt_bwd_f32, agnn_relt_dw_f32), against per-block float64 matmuls written here: every head width D the kernels take
(hgt.HEAD_WIDTHS), row counts around the row tiles of every kernel family, relation / head / item counts that hit the loop
structure (relations in passes and in pairs, four heads per workgroup, 1 .. 4 items), the model sizes H = 128 and H = 512 at
16 000 rows, strided operands, run-to-run and launch-shape determinism, the dispatch of `hgt._relt`, and what the host-side
checks refuse.

Every output buffer is filled with NaN before a launch, and every operand and output is a column block of a wider matrix
with three more rows than the call is told of: a slot that should have been written and was not, a write into a neighbouring
column block or a row >= n_rows, and a read outside the operand's block or rows (NaN there) all fail.

Tolerance (per compared tensor, relative to that tensor's own largest magnitude in the float64 reference):

    tol = MARGIN[kind] * max( rel_err(the same formulas in float32 torch on the CPU, float64), 2^-21 )

MARGIN is twice the worst ratio measured on an MI355X over all cases of this file, rounded up to a power of two, at least 4
and at most 32; the measured ratios are in profiles/relt_parity.md.  The input gradient carries ONE accumulator through all
R * D products of an output element (1 792 at D = 256, R = 7) as a sequential fused-multiply-add chain, where the CPU's
float32 matmul sums each block in shorter partial chains: its ratio grows with R * D, that of the others does not.  Each
comparison prints its ratio (`pytest -s`) before it asserts."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# worst measured ratio (profiles/relt_parity.md): y 1.85, dx 4.15, dw 2.13
MARGIN = {"y": 4.0, "dx": 16.0, "dw": 8.0}
FLOOR = 2.0 ** -21
NAN = float("nan")
EINVAL, EALIGN, ENOMEM = -22, -14, -12
PAD_ROWS = 3
WIDTHS = (4, 8, 16, 32, 64, 128, 256)


# ------------------------------------------------------------------------------------------------------------------------
# cases and references (CPU)
# ------------------------------------------------------------------------------------------------------------------------
def make_case(D, N, R, heads, T=None, n_items=2, seed=0):
    """n_items operands of one shape: x [N, heads*D], the blocks of R relations picked out of a T-relation parameter
    (w [R*heads, D, D]), dy [N, R*heads*D]."""
    T = R if T is None else T
    g = torch.Generator().manual_seed(1000 * D + 10 * N + 7 * R + heads + seed)
    rel_ids = sorted(torch.randperm(T, generator=g)[:R].tolist())
    sel = [r * heads + h for r in rel_ids for h in range(heads)]
    H = heads * D
    items = []
    for _ in range(n_items):
        w_full = torch.randn(T * heads, D, D, generator=g) * 0.2
        items.append(dict(x=torch.randn(N, H, generator=g), w=w_full[sel].contiguous(), dy=torch.randn(N, R * H, generator=g)))
    return dict(D=D, N=N, R=R, heads=heads, items=items)


def reference(case, dtype):
    """[(y, dx, dw)] per item: per-block matmuls in `dtype`."""
    D, N, R, heads = case["D"], case["N"], case["R"], case["heads"]
    H = heads * D
    out = []
    for it in case["items"]:
        x, w, dy = it["x"].to(dtype), it["w"].to(dtype), it["dy"].to(dtype)
        y = torch.empty(N, R * H, dtype=dtype)
        dx = torch.zeros(N, H, dtype=dtype)
        dw = torch.empty(R * heads, D, D, dtype=dtype)
        for r in range(R):
            for h in range(heads):
                b = r * heads + h
                xs, ds = x[:, h * D:(h + 1) * D], dy[:, b * D:(b + 1) * D]
                y[:, b * D:(b + 1) * D] = xs @ w[b]
                dx[:, h * D:(h + 1) * D] += ds @ w[b].t()
                dw[b] = xs.t() @ ds
        out.append((y, dx, dw))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# harness (GPU)
# ------------------------------------------------------------------------------------------------------------------------
def _place(t, blk, nblk, dev):
    """t as column block `blk` of a NaN-filled [n + PAD_ROWS, nblk * width] matrix -> (matrix, view of the block's n rows)."""
    n, w = t.shape
    full = torch.full((n + PAD_ROWS, nblk * w), NAN, dtype=torch.float32, device=dev)
    view = full[:n, blk * w:(blk + 1) * w]
    view.copy_(t)
    return full, view


class Relt:
    """One case on the device.  Item i: x is column block X_BLK[i] of a [N + 3, 3H] matrix (as `_HGTCore` hands K and V over),
    dy block i % 2 of a [N + 3, 2 R H] one, y block Y_BLK[i] of [N + 3, 3 R H], dx block X_BLK[i] of [N + 3, 3H], dw the first
    R*heads blocks of a [R*heads + 1, D, D] buffer."""
    X_BLK, Y_BLK = (0, 2, 1, 0), (1, 0, 2, 1)

    def __init__(self, case):
        from analysisgnn_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.dev = dev = torch.device(DEV)
        self.case = case
        self.D, self.N, self.R, self.heads = case["D"], case["N"], case["R"], case["heads"]
        self.H = self.heads * self.D
        self.n = len(case["items"])
        self.x = [_place(it["x"], self.X_BLK[i], 3, dev) for i, it in enumerate(case["items"])]
        self.dy = [_place(it["dy"], i % 2, 2, dev) for i, it in enumerate(case["items"])]
        self.w = [it["w"].to(dev).contiguous() for it in case["items"]]
        self.wt = [w.transpose(1, 2).contiguous() for w in self.w]
        self.fresh()

    def fresh(self):
        """New NaN-filled output buffers."""
        dev, N, H, R, D = self.dev, self.N, self.H, self.R, self.D
        nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device=dev)          # noqa: E731
        self.y_full = [nan(N + PAD_ROWS, 3 * R * H) for _ in range(self.n)]
        self.dx_full = [nan(N + PAD_ROWS, 3 * H) for _ in range(self.n)]
        self.dw = [nan(R * self.heads + 1, D, D) for _ in range(self.n)]
        self.y = [f[:N, self.Y_BLK[i] * R * H:(self.Y_BLK[i] + 1) * R * H] for i, f in enumerate(self.y_full)]
        self.dx = [f[:N, self.X_BLK[i] * H:(self.X_BLK[i] + 1) * H] for i, f in enumerate(self.dx_full)]
        nws = int(self.lib.agnn_relt_dw_workspace_bytes(self.n, R, self.heads, D, N))
        self.nws = nws
        self.ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)

    def _items(self, triples, which=None):
        which = range(self.n) if which is None else which
        arr = (self._lib.ReltItem * len(which))()
        for it, i in zip(arr, which):
            a, b, y, ld_x, ld_y = triples(i)
            it.x, it.w, it.y, it.ld_x, it.ld_y = a, b, y, ld_x, ld_y
        return arr

    def stream(self):
        return self._lib.stream_ptr(self.dev)

    def fwd(self, which=None, D=None, n_rows=None, x_off=0, ld_x_add=0):
        arr = self._items(lambda i: (self.x[i][1].data_ptr() + x_off, self.w[i].data_ptr(), self.y[i].data_ptr(),
                                     self.x[i][0].stride(0) + ld_x_add, self.y_full[i].stride(0)), which)
        return self.lib.agnn_relt_fwd_f32(len(arr), arr, self.R, self.heads, self.D if D is None else D,
                                          self.N if n_rows is None else n_rows, self.stream())

    def bwd(self, which=None, D=None, n_rows=None, x_off=0, ld_x_add=0):
        arr = self._items(lambda i: (self.dy[i][1].data_ptr() + x_off, self.wt[i].data_ptr(), self.dx[i].data_ptr(),
                                     self.dy[i][0].stride(0) + ld_x_add, self.dx_full[i].stride(0)), which)
        return self.lib.agnn_relt_bwd_f32(len(arr), arr, self.R, self.heads, self.D if D is None else D,
                                          self.N if n_rows is None else n_rows, self.stream())

    def dwg(self, which=None, D=None, n_rows=None, x_off=0, ld_x_add=0, ws_bytes=None):
        arr = self._items(lambda i: (self.x[i][1].data_ptr() + x_off, self.dy[i][1].data_ptr(), self.dw[i].data_ptr(),
                                     self.x[i][0].stride(0) + ld_x_add, self.dy[i][0].stride(0)), which)
        return self.lib.agnn_relt_dw_f32(len(arr), arr, self.R, self.heads, self.D if D is None else D,
                                         self.N if n_rows is None else n_rows, self.ws.data_ptr(),
                                         self.nws if ws_bytes is None else ws_bytes, self.stream())

    def run(self):
        for name, fn in (("fwd", self.fwd), ("bwd", self.bwd), ("dw", self.dwg)):
            self._lib.check(fn(), f"agnn_relt_{name}_f32")
        torch.cuda.synchronize()
        return self

    def buffers(self):
        """Every output buffer, whole (neighbouring blocks and padding rows included), on the CPU."""
        torch.cuda.synchronize()
        bufs = {}
        for i in range(self.n):
            bufs.update({f"y{i}": self.y_full[i].cpu(), f"dx{i}": self.dx_full[i].cpu(), f"dw{i}": self.dw[i].cpu()})
        return bufs

    def all_outputs_untouched(self):
        return all(bool(torch.isnan(v).all()) for v in self.buffers().values())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _block(full, n_rows, blk, width, what):
    """Rows < n_rows of column block `blk` of a [n + PAD_ROWS, nblk * width] buffer; everything else must still be NaN."""
    mask = torch.zeros(full.shape[1], dtype=torch.bool)
    mask[blk * width:(blk + 1) * width] = True
    assert bool(torch.isnan(full[:, ~mask]).all()), f"{what}: a neighbouring column block was written"
    assert bool(torch.isnan(full[n_rows:]).all()), f"{what}: rows beyond n_rows were written"
    return full[:n_rows, mask]


def _compare(group, kind, got, ref64, ref32, what):
    """got (kernel, float32) against ref64 within MARGIN[kind] * max(rel_err(ref32, ref64), 2^-21) of max |ref64|."""
    got, ref32 = got.double(), ref32.double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} slots not written"
    scale = float(ref64.abs().max())
    assert scale > 0, f"{what}: the reference is all zero — the case does not test this tensor"
    err = float((got - ref64).abs().max()) / scale
    unit = max(float((ref32 - ref64).abs().max()) / scale, FLOOR)
    print(f"PARITY group={group} kind={kind} ratio={err / unit:.3f} err={err:.3e} f32_err={unit:.3e} what={what}")
    assert err <= MARGIN[kind] * unit, (f"{what}: rel err {err:.3e} > {MARGIN[kind]:g} * {unit:.3e} (float32 evaluation of the "
                                        "reference, floor 2^-21)")


def _check(a: Relt, group, what):
    """All outputs of a finished run against the references: values and untouched slots."""
    r64, r32 = reference(a.case, torch.float64), reference(a.case, torch.float32)
    b = a.buffers()
    R, H, G = a.R, a.H, a.R * a.heads
    for i in range(a.n):
        y = _block(b[f"y{i}"], a.N, a.Y_BLK[i], R * H, f"{what} y[{i}]")
        dx = _block(b[f"dx{i}"], a.N, a.X_BLK[i], H, f"{what} dx[{i}]")
        dw = b[f"dw{i}"]
        assert bool(torch.isnan(dw[G:]).all()), f"{what} dw[{i}]: the block behind the last one was written"
        _compare(group, "y", y, r64[i][0], r32[i][0], f"{what} y[{i}]")
        _compare(group, "dx", dx, r64[i][1], r32[i][1], f"{what} dx[{i}]")
        _compare(group, "dw", dw[:G], r64[i][2], r32[i][2], f"{what} dw[{i}]")
    return b


def _what(c):
    return f"D={c['D']} N={c['N']} R={c['R']} heads={c['heads']} items={len(c['items'])}"


# ------------------------------------------------------------------------------------------------------------------------
# the cases of every group, as data (a rehearsal of the generator and of both references can walk them without a GPU)
# ------------------------------------------------------------------------------------------------------------------------
ROW_WIDTHS = (4, 16, 32, 128, 256)
ROW_COUNTS = (1, 31, 32, 33, 127, 128, 129, 257)
SHAPE_WIDTHS = (4, 16, 32, 128, 256)
# relation counts beyond one staging pass of the D <= 32 kernels (8 relations at D = 16 / 32; 8192 / (heads * D * D) at D = 4 / 8)
PASSES = [(16, 9, 2), (32, 17, 1), (8, 9, 16), (4, 9, 64), (8, 64, 1)]
GROUPS = {
    "widths": [dict(D=D, N=1003, R=2, heads=4, T=7) for D in WIDTHS],
    "rows": [dict(D=D, N=N, R=3, heads=2) for D in ROW_WIDTHS for N in ROW_COUNTS],
    "shapes": ([dict(D=D, N=130, R=R, heads=2) for D in SHAPE_WIDTHS for R in (1, 3, 6, 7)]
               + [dict(D=D, N=130, R=2, heads=h) for D in SHAPE_WIDTHS for h in (1, 2, 3, 5, 8)]
               + [dict(D=D, N=130, R=3, heads=4, n_items=k) for D in SHAPE_WIDTHS for k in (1, 3, 4)]
               + [dict(D=D, N=70, R=R, heads=h) for D, R, h in PASSES]),
    "model": [dict(D=32, N=16000, R=6, heads=4), dict(D=128, N=16000, R=6, heads=4)],
}


def _id(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", GROUPS["widths"], ids=_id)
def test_widths(kw):
    """Every head width, K and V in one call, 1003 rows, 2 relations picked out of a 7-relation parameter, 4 heads, operands
    column views of [N, 3H]."""
    from analysisgnn_amd.hgt import HEAD_WIDTHS
    assert tuple(HEAD_WIDTHS) == WIDTHS
    case = make_case(**kw)
    a = Relt(case)
    assert a.x[0][1].stride(0) == 3 * a.H and a.x[1][1].data_ptr() == a.x[1][0].data_ptr() + 4 * 2 * a.H
    _check(a.run(), "widths", _what(case))


@pytest.mark.parametrize("kw", GROUPS["rows"], ids=_id)
def test_row_edges(kw):
    """Row counts around the 32-, 64- and 128-row tiles of the kernels, and below one MFMA k-step of the weight gradient."""
    case = make_case(**kw)
    _check(Relt(case).run(), "rows", _what(case))


@pytest.mark.parametrize("kw", GROUPS["shapes"], ids=_id)
def test_loop_shapes(kw):
    """Relation counts (the input gradient walks them in pairs, the D <= 32 kernels stage them in passes), head counts (the
    weight gradient packs four waves per workgroup), item counts."""
    case = make_case(**kw)
    _check(Relt(case).run(), "shapes", _what(case))


@pytest.mark.parametrize("kw", GROUPS["model"], ids=_id)
def test_model_sizes(kw):
    """H = 128 and H = 512 at heads = 4, 16 000 rows, 6 relations: the weight gradient sums 16 000 rows in many slices."""
    case = make_case(**kw)
    _check(Relt(case).run(), "model", _what(case))


# ------------------------------------------------------------------------------------------------------------------------
# bitwise properties
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_two_runs_are_bitwise_identical(D):
    a = Relt(make_case(D=D, N=1003, R=3, heads=4, seed=1))
    first = a.run().buffers()
    a.fresh()
    second = a.run().buffers()
    assert not bool(torch.isnan(first["dw0"][:-1]).any())
    for name in first:
        assert _same_bits(first[name], second[name]), name


@pytest.mark.parametrize("D", [8, 32, 128])
def test_four_items_equal_four_single_launches(D):
    case = make_case(D=D, N=700, R=3, heads=4, n_items=4, seed=2)
    a = Relt(case)
    together = a.run().buffers()
    assert not any(bool(torch.isnan(together[f"dw{i}"][:-1]).any()) for i in range(4))
    a.fresh()
    for i in range(4):
        for name, fn in (("fwd", a.fwd), ("bwd", a.bwd), ("dw", a.dwg)):
            a._lib.check(fn(which=[i]), f"agnn_relt_{name}_f32")
    alone = a.buffers()
    for name in together:
        assert _same_bits(together[name], alone[name]), name


@pytest.mark.parametrize("D", [32, 128])
def test_hgt_relt_is_the_entry_point(D):
    """`hgt._relt` on the same tensors gives the bits of the direct call: it runs these kernels and nothing else."""
    from analysisgnn_amd.hgt import _relt
    a = Relt(make_case(D=D, N=1003, R=3, heads=4, seed=3))
    direct = a.run().buffers()
    a.fresh()
    R, heads, dev = a.R, a.heads, a.dev
    _relt("fwd", tuple((a.x[i][1], a.w[i], a.y[i]) for i in range(2)), R, heads, D, dev)
    _relt("bwd", tuple((a.dy[i][1], a.wt[i], a.dx[i]) for i in range(2)), R, heads, D, dev)
    _relt("dw", tuple((a.x[i][1], a.dy[i][1], a.dw[i][:-1]) for i in range(2)), R, heads, D, dev)
    module = a.buffers()
    assert not bool(torch.isnan(module["y0"][:a.N, a.Y_BLK[0] * R * a.H:(a.Y_BLK[0] + 1) * R * a.H]).any())
    for name in direct:
        assert _same_bits(direct[name], module[name]), name


# ------------------------------------------------------------------------------------------------------------------------
# refusals: the host-side checks reject before any launch
# ------------------------------------------------------------------------------------------------------------------------
ENTRY = ["fwd", "bwd", "dw"]


@pytest.fixture(scope="module")
def small():
    return Relt(make_case(D=16, N=40, R=2, heads=2, seed=4))


def _call(a, entry, **kw):
    return {"fwd": a.fwd, "bwd": a.bwd, "dw": a.dwg}[entry](**kw)


@pytest.mark.parametrize("entry", ENTRY)
@pytest.mark.parametrize("D", [0, 12, 24, 512, -64])
def test_refused_widths(small, entry, D):
    a = small
    a.fresh()
    assert _call(a, entry, D=D) == EINVAL, f"{entry} D={D}"
    msg = a.lib.agnn_last_error().decode()
    assert "4, 8, 16, 32, 64, 128, 256" in msg, msg
    assert a.all_outputs_untouched()


@pytest.mark.parametrize("entry", ENTRY)
@pytest.mark.parametrize("how", ["pointer", "ld"])
def test_refused_alignment(small, entry, how):
    a = small
    a.fresh()
    rc = _call(a, entry, x_off=4) if how == "pointer" else _call(a, entry, ld_x_add=1)
    assert rc == EALIGN and a.lib.agnn_last_error()
    assert a.all_outputs_untouched()


@pytest.mark.parametrize("D", [4, 32, 64, 256])
def test_refused_workspace_one_byte_short(D):
    a = Relt(make_case(D=D, N=40, R=2, heads=2, seed=5))
    assert a.nws > 256
    assert a.dwg(ws_bytes=a.nws - 1) == ENOMEM and a.lib.agnn_last_error()
    assert a.all_outputs_untouched()
    a._lib.check(a.dwg(), "agnn_relt_dw_f32")
    assert not bool(torch.isnan(a.buffers()["dw0"][:-1]).any())


@pytest.mark.parametrize("D", [4, 16, 32, 128])
def test_no_rows(D):
    """n_rows = 0: forward and input gradient write nothing, the weight gradient zero-fills its blocks (and only them)."""
    a = Relt(make_case(D=D, N=40, R=2, heads=2, seed=6))
    assert a.fwd(n_rows=0) == 0 and a.bwd(n_rows=0) == 0
    assert a.all_outputs_untouched()
    assert a.dwg(n_rows=0) == 0
    b = a.buffers()
    G = a.R * a.heads
    for i in range(a.n):
        assert bool((b[f"dw{i}"][:G] == 0).all()) and bool(torch.isnan(b[f"dw{i}"][G:]).all())
        assert bool(torch.isnan(b[f"y{i}"]).all()) and bool(torch.isnan(b[f"dx{i}"]).all())
