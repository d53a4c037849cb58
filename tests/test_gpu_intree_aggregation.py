"""The five aggregation kernels of the in-tree convolutions — agnn_gated_fwd_f32 / _bwd_dst_f32 / _bwd_src_f32 (csrc/gated.hip)
and agnn_absdiff_fwd_f32 / _bwd_f32 (csrc/reledge.hip) — each called directly through its C entry point, against the plain
float64 reference oracle/intree_agg_ref.py (pinned by tests/test_oracle_intree_agg.py): all three chunk instantiations
(H <= 256, <= 512, <= 1024) with a full, a one-lane and a nearly full last chunk, row counts over one to four rounds of the
8-XCD row remap, rows of 0 .. 500 edges on either side with self loops, duplicated edges and isolated rows, bipartite
operands, leading dimensions larger than H, the per-edge term with and without its gradient, both directions and both
`accumulate` modes of the |h_i - h_j| backward, exact ties, saturated gates, empty work, run-to-run determinism and what
the host-side checks refuse.

Every output buffer is filled with NaN before a launch: a slot that should have been written and was not, and a guard
column that should have stayed untouched and did not, both fail.  Every row holds its own random values, so a row computed
from or stored to the wrong place fails.

Tolerance (per compared tensor, relative to that tensor's own largest magnitude in the float64 reference):

    tol = MARGIN[kind] * max( rel_err(reference evaluated in float32 on the CPU, reference in float64), 2^-21 )

computed for the very inputs of the case.  MARGIN is the constant factor a tensor kind is allowed over it (expf and an IEEE
divide against torch's sigmoid, fused multiply-adds in CSR order instead of COO order): twice the worst ratio measured on an
MI355X over all cases of this file, rounded up to a power of two, at least 4 and at most 16 — the measured ratios are in
profiles/intree_aggregation_parity.md.  Each comparison prints its ratio (`pytest -s`) before it asserts."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import intree_agg_ref as A  # noqa: E402

DEV = "cuda:0"
# worst measured ratio (profiles/intree_aggregation_parity.md): gated S 1.09, da 1.63, db 1.34, dh 1.00, dc 1.00; absdiff S ("sum") 1.00,
# D ("absdiff") 1.00, dh ("abs_dh") 2.25 — twice 2.25 lies above 4, so that kind alone gets 8
MARGIN = {"S": 4.0, "da": 4.0, "db": 4.0, "dh": 4.0, "dc": 4.0, "sum": 4.0, "absdiff": 4.0, "abs_dh": 8.0}
FLOOR = 2.0 ** -21
NAN = float("nan")
OK, EINVAL, EALIGN = 0, -22, -14
WIDTHS = [4, 12, 252, 256, 260, 508, 512, 516, 1020, 1024]
ROWS = [1, 4, 5, 33, 65, 97]                                  # grids of 8, 8, 8, 16, 24 and 32 workgroups


# ------------------------------------------------------------------------------------------------------------------------
# graphs (CPU, COO)
# ------------------------------------------------------------------------------------------------------------------------
def _degree_edges(deg, others, gen):
    """COO (row, other): row i occurs exactly deg[i] times, `other` drawn from the index list `others`; random order."""
    rows = torch.repeat_interleave(torch.arange(len(deg)), torch.tensor(deg))
    other = torch.as_tensor(others)[torch.randint(0, len(others), (rows.numel(),), generator=gen)]
    p = torch.randperm(rows.numel(), generator=gen)
    return rows[p], other[p]


PATTERN = [500, 0, 1, 2, 7, 65, 3, 0, 0, 4]                   # row 8 is isolated: no edge on either side


def _pattern_graph(seed):
    """10 rows with 500, 0, 1, 2, 7, 65, 3, 0, 0 and 4 edges on the `row` side.  Rows 0, 4 and 5 carry a self loop, the two
    edges of row 3 are the same edge twice, rows 1 and 7 occur only on the other side, row 8 on neither."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.repeat_interleave(torch.arange(10), torch.tensor(PATTERN))
    others = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 9])
    other = others[torch.randint(0, 9, (rows.numel(),), generator=g)]
    first = {r: int((rows == r).nonzero()[0]) for r in (0, 3, 4, 5, 6, 9)}
    for r in (0, 4, 5):
        other[first[r]] = r                                     # self loops
    other[first[3]] = other[first[3] + 1] = 6                   # a duplicated edge
    other[first[6]], other[first[9]] = 1, 7                     # rows without an edge of their own are still gathered
    p = torch.randperm(rows.numel(), generator=g)
    rows, other = rows[p], other[p]
    assert torch.bincount(rows, minlength=10).tolist() == PATTERN and not bool(((rows == 8) | (other == 8)).any())
    return rows, other


def _covering_graph(n_row, n_other, seed):
    """Every one of the n_row rows has 1 .. 4 edges and every one of the n_other indices is gathered at least once."""
    g = torch.Generator().manual_seed(seed)
    rows, other = _degree_edges([1 + (3 * i + seed) % 4 for i in range(n_row)], list(range(n_other)), g)
    cover = torch.arange(n_other)
    return torch.cat([rows, cover % n_row]), torch.cat([other, cover])


def _gated_case(n_dst, n_src, H, dst, src, seed, with_c=True, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                 # noqa: E731
    return dict(H=H, n_dst=n_dst, n_src=n_src, dst=dst.long(), src=src.long(), a=r(n_dst, H) * scale, b=r(n_src, H) * scale,
                h=r(n_src, H), c=r(dst.numel(), H) if with_c else None, ds=r(n_dst, H))


# ------------------------------------------------------------------------------------------------------------------------
# harness (GPU)
# ------------------------------------------------------------------------------------------------------------------------
def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _placed(t, ld, lo):
    """t as columns lo .. lo + H of a NaN-filled [n, ld] matrix on the device -> (matrix, view)."""
    full = _nan(t.shape[0], ld)
    view = full[:, lo:lo + t.shape[1]]
    view.copy_(t)
    return full, view


def _inner(full, lo, H, what):
    """Columns lo .. lo + H of a buffer; every other column must still be NaN."""
    full = full.cpu()
    mask = torch.zeros(full.shape[1], dtype=torch.bool)
    mask[lo:lo + H] = True
    assert bool(torch.isnan(full[:, ~mask]).all()), f"{what}: a guard column was written"
    return full[:, mask]


def _csr_pair(dst, src, n_dst, n_src):
    from analysisgnn_amd import _lib
    from analysisgnn_amd.graph import SegSpec, build_csr
    dev = torch.device(DEV)
    fwd, bwd = build_csr([SegSpec(row=dst.to(dev), col=src.to(dev), n_rows=n_dst), SegSpec(row=src.to(dev), col=dst.to(dev), n_rows=n_src)])
    _lib.check_device_status(dev)
    return fwd, bwd


class GatedRun:
    """One gated case on the device.  layout "plain": contiguous operands, every leading dimension H.  "blocks": a / b / h are
    the column blocks 1 / 2 / 3 of [n, 4H + 4] matrices (one matrix when n_dst = n_src), the way ResGatedGraphConv's single
    projection GEMM lays them out; da / db / dh are written into the same blocks of NaN matrices of that leading dimension;
    out sits at columns 4 .. 4 + H of [n_dst, H + 8], ds at columns 8 .. 8 + H of [n_dst, H + 12], c and dc at columns
    0 .. H of [E, H + 4]."""

    def __init__(self, case, layout="plain"):
        from analysisgnn_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.dev = torch.device(DEV)
        self.case, self.layout = case, layout
        self.H, self.n_dst, self.n_src = case["H"], case["n_dst"], case["n_src"]
        H = self.H
        self.E = int(case["dst"].numel())
        blocks = layout == "blocks"
        self.ld = 4 * H + 4 if blocks else H
        self.off = dict(a=H, b=2 * H, h=3 * H) if blocks else dict(a=0, b=0, h=0)
        self.out_ld, self.out_lo = (H + 8, 4) if blocks else (H, 0)
        self.ds_ld, self.ds_lo = (H + 12, 8) if blocks else (H, 0)
        self.ld_c = H + 4 if blocks else H
        if blocks and self.n_dst == self.n_src:
            m = _nan(self.n_dst, self.ld)
            self.m_dst = self.m_src = m
        else:
            self.m_dst, self.m_src = (_nan(self.n_dst, self.ld), _nan(self.n_src, self.ld)) if blocks else (None, None)
        if blocks:
            self.a = self.m_dst[:, H:2 * H]
            self.b, self.h = self.m_src[:, 2 * H:3 * H], self.m_src[:, 3 * H:4 * H]
            for v, k in ((self.a, "a"), (self.b, "b"), (self.h, "h")):
                v.copy_(case[k])
        else:
            self.a, self.b, self.h = (case[k].to(self.dev).contiguous() for k in ("a", "b", "h"))
        self.ds_full, self.ds = _placed(case["ds"], self.ds_ld, self.ds_lo)
        self.c_full = self.c = None
        if case["c"] is not None:
            self.c_full, self.c = _placed(case["c"], self.ld_c, 0)
        self.fwd, self.bwd = _csr_pair(case["dst"], case["src"], self.n_dst, self.n_src)
        self.fresh()

    def fresh(self):
        H = self.H
        self.out_full = _nan(self.n_dst, self.out_ld)
        self.da_full, self.db_full, self.dh_full = _nan(self.n_dst, self.ld), _nan(self.n_src, self.ld), _nan(self.n_src, self.ld)
        self.dc_full = _nan(max(self.E, 1), self.ld_c)
        self.out = self.out_full[:, self.out_lo:self.out_lo + H]
        self.da = self.da_full[:, self.off["a"]:self.off["a"] + H]
        self.db = self.db_full[:, self.off["b"]:self.off["b"] + H]
        self.dh = self.dh_full[:, self.off["h"]:self.off["h"] + H]
        return self

    def desc(self, csr, n_rows, **over):
        f = dict(rowptr=csr.rowptr.data_ptr(), col=csr.col.data_ptr(), perm=csr.perm.data_ptr(), a=self.a.data_ptr(), b=self.b.data_ptr(),
                 h=self.h.data_ptr(), c=self._lib.ptr(self.c), ld=self.ld, ld_c=self.ld_c if self.c is not None else 0, n_rows=n_rows, H=self.H)
        f.update({k: v for k, v in over.items() if k in f})
        g = self._lib.Gated()
        for k, v in f.items():
            setattr(g, k, v)
        return g

    def stream(self):
        return self._lib.stream_ptr(self.dev)

    def forward(self, **over):
        g = self.desc(self.fwd, self.n_dst, **over)
        return self.lib.agnn_gated_fwd_f32(g, over.get("out", self.out.data_ptr()), over.get("ld_out", self.out_ld), self.stream())

    def backward_dst(self, with_dc=True, **over):
        g = self.desc(self.fwd, self.n_dst, **over)
        dc = self.dc_full.data_ptr() if (with_dc and self.c is not None) else None
        return self.lib.agnn_gated_bwd_dst_f32(g, over.get("ds", self.ds.data_ptr()), over.get("ld_ds", self.ds_ld),
                                               over.get("da", self.da.data_ptr()), over.get("dc", dc), self.stream())

    def backward_src(self, **over):
        g = self.desc(self.bwd, self.n_src, **over)
        return self.lib.agnn_gated_bwd_src_f32(g, over.get("ds", self.ds.data_ptr()), over.get("ld_ds", self.ds_ld),
                                               over.get("db", self.db.data_ptr()), over.get("dh", self.dh.data_ptr()), self.stream())

    def run(self, with_dc=True):
        self._lib.check(self.forward(), "agnn_gated_fwd_f32")
        self._lib.check(self.backward_dst(with_dc=with_dc), "agnn_gated_bwd_dst_f32")
        self._lib.check(self.backward_src(), "agnn_gated_bwd_src_f32")
        torch.cuda.synchronize()
        return self

    def buffers(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k + "_full").cpu() for k in ("out", "da", "db", "dh", "dc")}

    def untouched(self):
        return all(bool(torch.isnan(v).all()) for v in self.buffers().values())

    def outputs(self, with_dc=True):
        """The five results cut out of their buffers (guard columns checked); dc None when it was not asked for."""
        b, H = self.buffers(), self.H
        res = dict(S=_inner(b["out"], self.out_lo, H, "out"), da=_inner(b["da"], self.off["a"], H, "da"),
                   db=_inner(b["db"], self.off["b"], H, "db"), dh=_inner(b["dh"], self.off["h"], H, "dh"), dc=None)
        if with_dc and self.c is not None:
            res["dc"] = _inner(b["dc"], 0, H, "dc")[:self.E]
        else:
            assert bool(torch.isnan(b["dc"]).all()), "dc was written although it was not passed"
        return res


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _compare(group, kind, got, ref64, ref32, what):
    """got (kernel, float32) against ref64 within MARGIN[kind] * max(rel_err(ref32, ref64), 2^-21) of max |ref64|."""
    got, ref32 = got.double(), ref32.double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} slots not written"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    scale = float(ref64.abs().max())
    assert scale > 0, f"{what}: the reference is all zero — the case does not test this tensor"
    err = float((got - ref64).abs().max()) / scale
    unit = max(float((ref32 - ref64).abs().max()) / scale, FLOOR)
    print(f"PARITY group={group} kind={kind} ratio={err / unit:.3f} err={err:.3e} f32_err={unit:.3e} what={what}")
    assert err <= MARGIN[kind] * unit, (f"{what}: rel err {err:.3e} > {MARGIN[kind]:g} * {unit:.3e} (float32 evaluation of the "
                                        "reference, floor 2^-21)")


def _gated_refs(case):
    args = (case["a"], case["b"], case["h"], case["c"], case["dst"], case["src"], case["ds"])
    return A.gated(*args, dtype=torch.float64), A.gated(*args, dtype=torch.float32)


def _check_gated(run: GatedRun, group, what, with_dc=True):
    r64, r32 = _gated_refs(run.case)
    got = run.outputs(with_dc)
    case = run.case
    for i, kind in enumerate(("S", "da", "db", "dh")):
        _compare(group, kind, got[kind], r64[i], r32[i], f"{what} {kind}")
    # rows without an edge on their side are exact zeros
    no_dst = torch.bincount(case["dst"], minlength=run.n_dst) == 0
    no_src = torch.bincount(case["src"], minlength=run.n_src) == 0
    assert bool((got["S"][no_dst] == 0).all()) and bool((got["da"][no_dst] == 0).all()), f"{what}: rows without incoming edges"
    assert bool((got["db"][no_src] == 0).all()) and bool((got["dh"][no_src] == 0).all()), f"{what}: rows without outgoing edges"
    if got["dc"] is not None:
        _compare(group, "dc", got["dc"], r64[4], r32[4], f"{what} dc")
    return got


# ------------------------------------------------------------------------------------------------------------------------
# gated: widths, rows, degrees, bipartite, strides, per-edge term, saturation
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", WIDTHS)
def test_gated_widths(H):
    """All three instantiations, each with a full last chunk (256, 512, 1024), a one-lane one (4, 260, 516) and a nearly full
    one (252, 508, 1020): 9 rows, one of them with 70 edges, strided operands, per-edge term and its gradient."""
    g = torch.Generator().manual_seed(H)
    dst, src = _degree_edges([70, 0, 1, 2, 7, 3, 1, 5, 2], list(range(9)), g)
    _check_gated(GatedRun(_gated_case(9, 9, H, dst, src, seed=H), "blocks").run(), "widths", f"H={H}")


@pytest.mark.parametrize("H", [12, 516])
@pytest.mark.parametrize("n", ROWS)
def test_gated_row_counts(n, H):
    """Grids of 8, 16, 24 and 32 workgroups (G >> 3 = 1 .. 4 in the XCD row remap), the last workgroup partly filled; every
    row has an edge on both sides, so no result is a trivial zero."""
    dst, src = _covering_graph(n, n, seed=n)
    assert int(torch.bincount(dst, minlength=n).min()) > 0 and int(torch.bincount(src, minlength=n).min()) > 0
    _check_gated(GatedRun(_gated_case(n, n, H, dst, src, seed=n + H), "plain" if H == 12 else "blocks").run(), "rows", f"n={n} H={H}")


@pytest.mark.parametrize("H", [12, 260, 1024])
def test_gated_degrees_on_both_sides(H):
    """Rows of 0, 1, 2, 7, 65 and 500 edges, self loops, a duplicated edge and an isolated row, once as DESTINATION rows (the
    forward and the by-destination backward walk them) and once as SOURCE rows (the by-source backward does)."""
    rows, other = _pattern_graph(seed=7)
    for side, (dst, src) in (("dst", (rows, other)), ("src", (other, rows))):
        got = _check_gated(GatedRun(_gated_case(10, 10, H, dst, src, seed=H + len(side))).run(), "degrees", f"H={H} side={side}")
        for k in ("S", "da", "db", "dh"):
            assert bool((got[k][8] == 0).all()), f"{k}: the isolated row"


@pytest.mark.parametrize("H", [12, 260])
@pytest.mark.parametrize("n_dst,n_src", [(13, 7), (7, 13)])
@pytest.mark.parametrize("layout", ["plain", "blocks"])
def test_gated_bipartite(n_dst, n_src, H, layout):
    """a has n_dst rows, b and h have n_src: the by-source pass runs over n_src rows and reads a and ds by column."""
    dst, src = _covering_graph(n_dst, n_src, seed=n_dst)
    run = GatedRun(_gated_case(n_dst, n_src, H, dst, src, seed=n_dst + H), layout).run()
    assert run.m_dst is None or run.m_dst.data_ptr() != run.m_src.data_ptr()
    _check_gated(run, "bipartite", f"{n_dst}x{n_src} H={H} {layout}")


@pytest.mark.parametrize("H", [12, 260, 1020])
def test_gated_strides(H):
    """The same case contiguous and as column blocks of one [n, 4H + 4] matrix (out / ds / c / dc with their own larger
    leading dimensions): bit-identical results, NaN around every operand and every result."""
    dst, src = _covering_graph(33, 33, seed=2)
    case = _gated_case(33, 33, H, dst, src, seed=H)
    plain, blocks = GatedRun(case, "plain").run(), GatedRun(case, "blocks").run()
    assert blocks.a.stride(0) == 4 * H + 4 and blocks.m_dst is blocks.m_src and blocks.out_ld == H + 8 and blocks.ld_c == H + 4
    assert blocks.b.data_ptr() == blocks.m_src.data_ptr() + 4 * 2 * H
    gp, gb = _check_gated(plain, "strides", f"H={H} plain"), _check_gated(blocks, "strides", f"H={H} blocks")
    for k in gp:
        assert _same_bits(gp[k], gb[k]), f"{k}: the strided launch differs from the contiguous one"


@pytest.mark.parametrize("layout", ["plain", "blocks"])
@pytest.mark.parametrize("H", [12, 260])
def test_gated_per_edge_term(H, layout):
    """c absent; c present without dc; c present with dc — every COO row of dc is written (no NaN left) with its own edge's
    summand, and da does not depend on whether dc was asked for."""
    rows, other = _pattern_graph(seed=9)
    with_c = _gated_case(10, 10, H, rows, other, seed=H, with_c=True)
    without = dict(with_c, c=None)
    _check_gated(GatedRun(without, layout).run(), "edge-term", f"H={H} {layout} no c")
    no_dc = _check_gated(GatedRun(with_c, layout).run(with_dc=False), "edge-term", f"H={H} {layout} c, dc NULL", with_dc=False)
    full = _check_gated(GatedRun(with_c, layout).run(), "edge-term", f"H={H} {layout} c and dc")
    assert full["dc"].shape == (rows.numel(), H) and not bool(torch.isnan(full["dc"]).any())
    assert _same_bits(no_dc["da"], full["da"]) and _same_bits(no_dc["S"], full["S"])
    # c matters: the reference without it is far from the result with it
    r_without = A.gated(without["a"], without["b"], without["h"], None, rows, other, without["ds"])
    assert float((full["S"].double() - r_without[0]).abs().max()) > 0.1


@pytest.mark.parametrize("H", [12, 260, 1024])
def test_gated_saturated_gates(H):
    """a and b scaled by 30 (most gates within rounding of 0 or 1) and a few entries at +-200 (expf overflows to inf / underflows
    to 0): forward and every gradient finite and within tolerance."""
    rows, other = _pattern_graph(seed=11)
    case = _gated_case(10, 10, H, rows, other, seed=H + 1, scale=30.0)
    for t in (case["a"], case["b"]):
        t[0, 0], t[0, 1], t[4, 2], t[5, 3] = 200.0, -200.0, 200.0, -200.0
    case["c"][0, 0], case["c"][1, 1] = 200.0, -200.0
    got = _check_gated(GatedRun(case).run(), "saturated", f"H={H}")
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


# ------------------------------------------------------------------------------------------------------------------------
# absdiff
# ------------------------------------------------------------------------------------------------------------------------
class AbsRun:
    """h on the device (layout "blocks": the middle column block of a NaN-filled [n, 3H] matrix) with both CSR directions."""

    def __init__(self, h, dst, src, layout="plain"):
        from analysisgnn_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.dev = torch.device(DEV)
        self.n, self.H = h.shape
        self.h_cpu, self.dst, self.src = h, dst.long(), src.long()
        self.h_full, self.h = _placed(h, 3 * self.H, self.H) if layout == "blocks" else _placed(h, self.H, 0)
        self.fwd, self.bwd = _csr_pair(self.dst, self.src, self.n, self.n)

    def stream(self):
        return self._lib.stream_ptr(self.dev)

    def forward_raw(self, out_s, out_d, ld_out, **over):
        c = self.fwd
        return self.lib.agnn_absdiff_fwd_f32(over.get("rowptr", c.rowptr.data_ptr()), over.get("col", c.col.data_ptr()),
                                             over.get("h", self.h.data_ptr()), over.get("ld", self.h.stride(0)), over.get("n_rows", self.n),
                                             over.get("H", self.H), out_s, out_d, ld_out, self.stream())

    def forward(self, mode):
        """mode "both": S | D side by side in [n, 2H]; "s" / "d": one of them alone at columns 4 .. 4 + H of [n, H + 8].
        -> (S or None, D or None) on the CPU, guard columns checked."""
        H = self.H
        if mode == "both":
            out = _nan(self.n, 2 * H)
            rc = self.forward_raw(out.data_ptr(), out.data_ptr() + 4 * H, 2 * H)
        else:
            out = _nan(self.n, H + 8)
            p = out.data_ptr() + 16
            rc = self.forward_raw(p if mode == "s" else None, p if mode == "d" else None, H + 8)
        self._lib.check(rc, "agnn_absdiff_fwd_f32")
        torch.cuda.synchronize()
        if mode == "both":
            o = out.cpu()
            return o[:, :H], o[:, H:]
        o = _inner(out, 4, H, f"absdiff out ({mode})")
        return (o, None) if mode == "s" else (None, o)

    def backward_raw(self, csr, gd, gs, ld_g, by_col, accumulate, out, ld_out, **over):
        return self.lib.agnn_absdiff_bwd_f32(over.get("rowptr", csr.rowptr.data_ptr()), over.get("col", csr.col.data_ptr()),
                                             over.get("h", self.h.data_ptr()), over.get("ld", self.h.stride(0)), over.get("n_rows", self.n),
                                             over.get("H", self.H), gd, gs, ld_g, by_col, accumulate, out, ld_out, self.stream())

    def grads(self, gs, gd, side_by_side):
        """gs / gd (CPU or None) on the device: column blocks of one [n, 2H] matrix (as autograd hands the gradient of [S | D]
        over) or each at columns 4 .. 4 + H of its own [n, H + 8] matrix.  -> (gd pointer, gs pointer, ld_g, keep-alive)."""
        H = self.H
        if side_by_side:
            g = _nan(self.n, 2 * H)
            if gs is not None:
                g[:, :H].copy_(gs)
            if gd is not None:
                g[:, H:].copy_(gd)
            return (g.data_ptr() + 4 * H if gd is not None else None), (g.data_ptr() if gs is not None else None), 2 * H, g
        keep = [_placed(t, H + 8, 4) if t is not None else None for t in (gd, gs)]
        return (keep[0][1].data_ptr() if gd is not None else None), (keep[1][1].data_ptr() if gs is not None else None), H + 8, keep

    def backward(self, csr, gs, gd, by_col, prefill=None, side_by_side=True):
        """One launch into columns 4 .. 4 + H of a [n, H + 8] buffer (NaN, or `prefill` with accumulate = 1) -> result (CPU)."""
        H = self.H
        pd, ps, ld_g, keep = self.grads(gs, gd, side_by_side)
        out = _nan(self.n, H + 8)
        if prefill is not None:
            out[:, 4:4 + H].copy_(prefill)
        self._lib.check(self.backward_raw(csr, pd, ps, ld_g, by_col, 1 if prefill is not None else 0, out.data_ptr() + 16, H + 8),
                        "agnn_absdiff_bwd_f32")
        torch.cuda.synchronize()
        return _inner(out, 4, H, "absdiff dh")

    def backward_pair(self, gs, gd):
        """The two launches of _RelEdgeAggregate.backward: forward CSR by row, then the transposed CSR by column, accumulating."""
        H = self.H
        pd, ps, ld_g, keep = self.grads(gs, gd, True)
        out = _nan(self.n, H)
        self._lib.check(self.backward_raw(self.fwd, pd, None, ld_g, 0, 0, out.data_ptr(), H), "agnn_absdiff_bwd_f32")
        self._lib.check(self.backward_raw(self.bwd, pd, ps, ld_g, 1, 1, out.data_ptr(), H), "agnn_absdiff_bwd_f32")
        torch.cuda.synchronize()
        return out.cpu()


def _abs_data(n, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, H, generator=g), torch.randn(n, H, generator=g), torch.randn(n, H, generator=g), torch.randn(n, H, generator=g)


def _check_abs(run: AbsRun, gs, gd, group, what, forward_modes=("both",)):
    """Forward (each mode) and the two-launch backward against the reference."""
    h, dst, src = run.h_cpu, run.dst, run.src
    S64, D64, dh64 = A.absdiff(h, dst, src, gs, gd, dtype=torch.float64)
    S32, D32, dh32 = A.absdiff(h, dst, src, gs, gd, dtype=torch.float32)
    no_dst = torch.bincount(dst, minlength=run.n) == 0
    for mode in forward_modes:
        S, D = run.forward(mode)
        if S is not None:
            _compare(group, "sum", S, S64, S32, f"{what} S ({mode})")
            assert bool((S[no_dst] == 0).all())
        if D is not None:
            _compare(group, "absdiff", D, D64, D32, f"{what} D ({mode})")
            assert bool((D[no_dst] == 0).all())
    dh = run.backward_pair(gs, gd)
    _compare(group, "abs_dh", dh, dh64, dh32, f"{what} dh")
    return dh


@pytest.mark.parametrize("H", WIDTHS)
def test_absdiff_widths(H):
    g = torch.Generator().manual_seed(H + 1)
    dst, src = _degree_edges([70, 0, 1, 2, 7, 3, 1, 5, 2], list(range(9)), g)
    h, gs, gd, _ = _abs_data(9, H, H)
    _check_abs(AbsRun(h, dst, src, "blocks"), gs, gd, "widths", f"H={H}", forward_modes=("both", "s", "d"))


@pytest.mark.parametrize("H", [12, 516])
@pytest.mark.parametrize("n", ROWS)
def test_absdiff_row_counts(n, H):
    dst, src = _covering_graph(n, n, seed=n + 1)
    if n == 1:                                                   # a single row only has self loops, whose D is 0: nothing to scale by
        h, gs, gd, _ = _abs_data(1, H, 1)
        run = AbsRun(h, dst, src)
        S, D = run.forward("both")
        assert torch.equal(S, h * float(dst.numel())) and bool((D == 0).all())
        assert torch.equal(run.backward_pair(gs, gd), gs * float(dst.numel()))
        return
    h, gs, gd, _ = _abs_data(n, H, n + H)
    _check_abs(AbsRun(h, dst, src, "plain" if H == 12 else "blocks"), gs, gd, "rows", f"n={n} H={H}")


@pytest.mark.parametrize("H", [12, 260, 1024])
def test_absdiff_degrees_on_both_sides(H):
    rows, other = _pattern_graph(seed=13)
    h, gs, gd, _ = _abs_data(10, H, H + 2)
    for side, (dst, src) in (("dst", (rows, other)), ("src", (other, rows))):
        dh = _check_abs(AbsRun(h, dst, src), gs, gd, "degrees", f"H={H} side={side}", forward_modes=("both", "s", "d"))
        assert bool((dh[8] == 0).all()), "the isolated row"


@pytest.mark.parametrize("H", [12, 260])
@pytest.mark.parametrize("side_by_side", [True, False])
def test_absdiff_backward_modes(H, side_by_side):
    """Each launch on its own: by_col = 0 on the forward CSR (the aggregating end, gd only) and by_col = 1 on the transposed
    CSR (the gathered end; gd only, gs only, both), overwriting NaN and accumulating onto known random contents."""
    rows, other = _pattern_graph(seed=15)
    h, gs, gd, pre = _abs_data(10, H, H + 3)
    run = AbsRun(h, rows, other, "blocks")
    for name, s, d in (("gd", None, gd), ("gs", gs, None), ("both", gs, gd)):
        _, _, row64, col64 = A.absdiff_ends(h, rows, other, s, d, dtype=torch.float64)
        _, _, row32, col32 = A.absdiff_ends(h, rows, other, s, d, dtype=torch.float32)
        for prefill in (None, pre):
            add64 = pre.double() if prefill is not None else 0.0
            add32 = pre if prefill is not None else 0.0
            tag = f"H={H} {name} accumulate={int(prefill is not None)}"
            if d is not None:
                got = run.backward(run.fwd, None, d, 0, prefill, side_by_side)
                _compare("bwd-modes", "abs_dh", got, row64 + add64, row32 + add32, f"{tag} by_col=0")
            got = run.backward(run.bwd, s, d, 1, prefill, side_by_side)
            _compare("bwd-modes", "abs_dh", got, col64 + add64, col32 + add32, f"{tag} by_col=1")


@pytest.mark.parametrize("H", [12, 260, 516])
def test_absdiff_ties_are_exact(H):
    """Rows 0 and 1 identical and joined in both directions, self loops on rows 0 .. 3, and ordinary edges besides.  Kernel
    and reference get the same float32 values, so every sign — sign(0) = 0 included — is exact on both sides."""
    g = torch.Generator().manual_seed(H)
    h, gs, gd, _ = _abs_data(6, H, H + 4)
    h[1] = h[0]
    dst = torch.tensor([0, 1, 0, 1, 0, 1, 2, 3, 2, 4, 5, 5, 3])
    src = torch.tensor([1, 0, 1, 0, 0, 1, 2, 3, 0, 1, 4, 2, 5])
    p = torch.randperm(dst.numel(), generator=g)
    dst, src = dst[p], src[p]
    run = AbsRun(h, dst, src)
    _check_abs(run, gs, gd, "ties", f"H={H}")
    # the tie-only subgraph: D and its gradient are exactly zero; with sign(0) = +-1 they would be +-4 gd or so
    tie = ((dst < 2) & (src < 2)) | (dst == src)
    sub = AbsRun(h, dst[tie], src[tie])
    S, D = sub.forward("both")
    assert bool((D == 0).all())
    assert bool((sub.backward(sub.fwd, None, gd, 0) == 0).all()) and bool((sub.backward(sub.bwd, None, gd, 1) == 0).all())
    _, _, dh64 = A.absdiff(h, dst[tie], src[tie], None, gd)
    assert bool((dh64 == 0).all())


# ------------------------------------------------------------------------------------------------------------------------
# empty work, determinism
# ------------------------------------------------------------------------------------------------------------------------
def test_no_rows_is_a_successful_no_op():
    from analysisgnn_amd import _lib
    lib = _lib.load()
    st = _lib.stream_ptr(torch.device(DEV))
    g = _lib.Gated()
    g.n_rows, g.H = 0, 4
    assert lib.agnn_gated_fwd_f32(g, None, 0, st) == OK
    assert lib.agnn_gated_bwd_dst_f32(g, None, 0, None, None, st) == OK
    assert lib.agnn_gated_bwd_src_f32(g, None, 0, None, None, st) == OK
    assert lib.agnn_absdiff_fwd_f32(None, None, None, 0, 0, 4, None, None, 0, st) == OK
    assert lib.agnn_absdiff_bwd_f32(None, None, None, 0, 0, 4, None, None, 0, 0, 0, None, 0, st) == OK


@pytest.mark.parametrize("H", [12, 516])
def test_graph_without_edges_gives_exact_zeros(H):
    none = torch.zeros(0, dtype=torch.int64)
    case = _gated_case(5, 5, H, none, none, seed=1, with_c=False)
    got = GatedRun(case, "blocks").run().outputs()
    for k in ("S", "da", "db", "dh"):
        assert bool((got[k] == 0).all()), f"{k}: exact zeros expected, not NaN"
    h, gs, gd, _ = _abs_data(5, H, 2)
    run = AbsRun(h, none, none, "blocks")
    S, D = run.forward("both")
    assert bool((S == 0).all()) and bool((D == 0).all()) and bool((run.backward_pair(gs, gd) == 0).all())


@pytest.mark.parametrize("H", [260, 1024])
def test_two_launches_are_bitwise_identical(H):
    rows, other = _pattern_graph(seed=17)
    case = _gated_case(10, 10, H, rows, other, seed=H)
    run = GatedRun(case, "blocks")
    first = run.run().buffers()
    second = run.fresh().run().buffers()
    assert not bool(torch.isnan(first["out"][:, run.out_lo:run.out_lo + H]).any())
    for k in first:
        assert _same_bits(first[k], second[k]), k
    h, gs, gd, _ = _abs_data(10, H, H)
    ab = AbsRun(h, rows, other)
    f1, f2 = ab.forward("both"), ab.forward("both")
    assert _same_bits(f1[0], f2[0]) and _same_bits(f1[1], f2[1])
    assert _same_bits(ab.backward_pair(gs, gd), ab.backward_pair(gs, gd))


# ------------------------------------------------------------------------------------------------------------------------
# refusals: the host-side checks reject before any launch.  Every buffer has its full [n, H] size and every index array is
# valid, so a call that slipped through would still stay inside its buffers.
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_gated():
    dst, src = _covering_graph(6, 6, seed=3)
    return GatedRun(_gated_case(6, 6, 8, dst, src, seed=3), "plain")


GATED_ENTRIES = ["forward", "backward_dst", "backward_src"]
GATED_COMMON = [("H=0", dict(H=0), EINVAL), ("H=6", dict(H=6), EINVAL), ("H=1028", dict(H=1028), EINVAL),
                ("ld odd", dict(ld=10), EALIGN), ("ld<H", dict(ld=4), EALIGN),
                ("null a", dict(a=None), EINVAL), ("null b", dict(b=None), EINVAL), ("null h", dict(h=None), EINVAL),
                ("null rowptr", dict(rowptr=None), EINVAL), ("c without perm", dict(perm=None), EALIGN),
                ("ld_c<H", dict(ld_c=4), EALIGN), ("ld_c odd", dict(ld_c=10), EALIGN)]


@pytest.mark.parametrize("entry", GATED_ENTRIES)
@pytest.mark.parametrize("why,over,code", GATED_COMMON, ids=[w.replace(" ", "_") for w, _, _ in GATED_COMMON])
def test_gated_refusals(small_gated, entry, why, over, code):
    r = small_gated.fresh()
    rc = getattr(r, entry)(**over)
    assert rc == code, f"{entry} {why}: rc = {rc}"
    assert r.lib.agnn_last_error(), "an error text is set"
    assert r.untouched()


@pytest.mark.parametrize("entry", GATED_ENTRIES)
@pytest.mark.parametrize("name", ["a", "b", "h", "c"])
def test_gated_refuses_a_pointer_off_by_four_bytes(small_gated, entry, name):
    r = small_gated.fresh()
    rc = getattr(r, entry)(**{name: getattr(r, name).data_ptr() + 4})
    assert rc == EALIGN and r.lib.agnn_last_error() and r.untouched()


def test_gated_refusals_of_the_results(small_gated):
    """Misaligned or missing result / gradient pointers, a backward call without perm, dc without c."""
    r = small_gated.fresh()
    H = r.H
    calls = [(r.forward, dict(out=r.out.data_ptr() + 4)), (r.forward, dict(out=None)), (r.forward, dict(ld_out=H + 2)),
             (r.backward_dst, dict(ds=r.ds.data_ptr() + 4)), (r.backward_dst, dict(da=r.da.data_ptr() + 4)), (r.backward_dst, dict(ld_ds=H + 2)),
             (r.backward_dst, dict(dc=r.dc_full.data_ptr() + 4)), (r.backward_dst, dict(da=None)),
             (r.backward_src, dict(ds=r.ds.data_ptr() + 4)), (r.backward_src, dict(db=r.db.data_ptr() + 4)),
             (r.backward_src, dict(dh=r.dh.data_ptr() + 4)), (r.backward_src, dict(ld_ds=H + 2)), (r.backward_src, dict(dh=None))]
    for fn, over in calls:
        assert fn(**over) == EALIGN and r.lib.agnn_last_error(), f"{fn.__name__} {over}"
    # without c the forward needs no perm; both backward calls always do (dc rows, and the by-source pass reads c by it)
    assert r.backward_dst(c=None, ld_c=0, perm=None, dc=None) == EALIGN and r.backward_src(c=None, ld_c=0, perm=None) == EALIGN
    assert r.backward_dst(c=None, ld_c=0, dc=r.dc_full.data_ptr()) == EALIGN, "dc without c: it would be written with ld_c = 0"
    assert r.untouched()
    assert r.forward(c=None, ld_c=0, perm=None) == OK
    torch.cuda.synchronize()
    assert not bool(torch.isnan(r.out).any())


@pytest.mark.parametrize("case", ["ld_out<H", "ld_ds<H dst", "ld_ds<H src", "null col"])
def test_gated_refuses_what_would_leave_a_row(case):
    """ld_out < H lets the forward write past a row of `out`, ld_ds < H lets a backward pass read past a row of `ds`, and a
    null `col` is dereferenced for the first edge.  All buffers have their full [n, H] size and the null-col CSR has no
    edge, so the launch these checks prevent would have stayed in bounds."""
    none = torch.zeros(0, dtype=torch.int64)
    if case == "null col":
        r = GatedRun(_gated_case(6, 6, 8, none, none, seed=4, with_c=False), "plain")
        rcs = [r.forward(col=None), r.backward_dst(col=None), r.backward_src(col=None)]
        assert rcs == [EINVAL] * 3
    else:
        dst, src = _covering_graph(6, 6, seed=4)
        r = GatedRun(_gated_case(6, 6, 8, dst, src, seed=4), "plain")
        fn, over = {"ld_out<H": (r.forward, dict(ld_out=4)), "ld_ds<H dst": (r.backward_dst, dict(ld_ds=4)),
                    "ld_ds<H src": (r.backward_src, dict(ld_ds=4))}[case]
        assert fn(**over) == EALIGN
    assert r.lib.agnn_last_error() and r.untouched()


def test_absdiff_refusals():
    dst, src = _covering_graph(6, 6, seed=5)
    h, gs, gd, _ = _abs_data(6, 8, 5)
    r = AbsRun(h, dst, src)
    H = 8
    out = _nan(6, 2 * H)
    o = out.data_ptr()
    g = torch.cat([gs, gd], 1).to(DEV)
    pgs, pgd = g.data_ptr(), g.data_ptr() + 4 * H
    fwd = lambda out_s=o, out_d=o + 4 * H, ld_out=2 * H, **kw: r.forward_raw(out_s, out_d, ld_out, **kw)                      # noqa: E731
    bwd = lambda gd_=pgd, gs_=pgs, ld_g=2 * H, by_col=1, acc=0, out_=o, ld_out=2 * H, **kw: r.backward_raw(                  # noqa: E731
        r.bwd, gd_, gs_, ld_g, by_col, acc, out_, ld_out, **kw)
    cases = [(fwd(H=0), EINVAL), (fwd(H=6), EINVAL), (fwd(H=1028), EINVAL), (bwd(H=0), EINVAL), (bwd(H=6), EINVAL), (bwd(H=1028), EINVAL),
             (fwd(h=r.h.data_ptr() + 4), EALIGN), (bwd(h=r.h.data_ptr() + 4), EALIGN), (fwd(ld=10), EALIGN), (bwd(ld=10), EALIGN),
             (fwd(ld=4), EALIGN), (bwd(ld=4), EALIGN),
             (fwd(h=None), EINVAL), (fwd(rowptr=None), EINVAL), (fwd(col=None), EINVAL),
             (bwd(h=None), EINVAL), (bwd(rowptr=None), EINVAL), (bwd(col=None), EINVAL),
             (fwd(out_s=None, out_d=None), EINVAL), (fwd(out_s=o + 4), EALIGN), (fwd(out_d=o + 4), EALIGN), (fwd(ld_out=H + 2), EALIGN),
             (fwd(ld_out=4), EALIGN),
             (bwd(gd_=None, gs_=None), EINVAL), (bwd(by_col=0), EINVAL), (bwd(out_=None), EALIGN), (bwd(out_=o + 4), EALIGN),
             (bwd(ld_out=4), EALIGN), (bwd(ld_out=H + 2), EALIGN), (bwd(ld_g=4), EALIGN), (bwd(ld_g=H + 2), EALIGN),
             (bwd(gd_=pgd + 4), EALIGN), (bwd(gs_=pgs + 4), EALIGN)]
    for i, (rc, code) in enumerate(cases):
        assert rc == code, f"case {i}: rc = {rc}, expected {code}"
    assert r.lib.agnn_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call launched"
    assert bwd(gs_=None, by_col=0) == OK and fwd() == OK          # the same arguments, valid, are accepted
