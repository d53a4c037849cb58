"""The four HGT attention kernels (csrc/hgt.hip), each called directly through its C entry point, against the plain float64
reference oracle/hgt_attn_ref.py (pinned by tests/test_oracle_hgt_attn.py): every head width D = H / heads the kernels take,
every chunk count (H <= 256, <= 512, <= 1024, with a partly filled last chunk), destination AND source rows of 0 .. 500 edges
(second and later 64-edge batches, odd tails), strided operands, both `tdot` layouts, trimmed rows (`rowend`, `col_limit`),
the multi-item forward launch, large logits, what the host-side checks refuse, and run-to-run determinism.

Every output buffer is filled with NaN before a launch: a slot that should have been written and was not, and a slot that
should have stayed untouched and did not, both fail.

Tolerance (per compared tensor, relative to that tensor's own largest magnitude in the reference):

    tol = MARGIN[kind] * max( rel_err(reference evaluated in float32 on the CPU, reference in float64), 2^-21 )

computed for the very inputs of the case — the rounding the same formulas suffer in plain float32 torch, floored at 4 float32
ulp.  MARGIN is the constant factor a tensor kind is allowed over it (hardware exp on an argument pre-scaled by log2 e, fused
multiply-adds in another order, the online rescaling of the running sum): twice the worst ratio measured on an MI355X over
all cases of this file, rounded up to a power of two, at least 4 and at most 32 — the measured ratios are in
profiles/hgt_attention_parity.md.  Each comparison prints its ratio (`pytest -s`) before it asserts."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import hgt_attn_ref as A  # noqa: E402

DEV = "cuda:0"
# worst measured ratio (profiles/hgt_attention_parity.md): out 1.29, m 0.41, linv 3.75, alpha 7.10, gs 4.76, tdot 5.94, dq 6.34, dk 4.30, dv 5.41
MARGIN = {"out": 4.0, "m": 4.0, "linv": 8.0, "alpha": 16.0, "gs": 16.0, "tdot": 16.0, "dq": 16.0, "dk": 16.0, "dv": 16.0}
FLOOR = 2.0 ** -21
NAN = float("nan")
EINVAL, EALIGN = -22, -14
PATTERN = [0, 1, 2, 63, 64, 65, 127, 128, 129, 500]          # row lengths around the 64-edge batches of the kernels' loops


# ------------------------------------------------------------------------------------------------------------------------
# cases (CPU): dict(H, heads, q [n, H], dm [n, H], rels=[dict(k, v [n_src, H], src, dst [E], pscale [heads], e_limit?)], n_keep?)
# ------------------------------------------------------------------------------------------------------------------------
def _degree_edges(deg, n_other, gen):
    """COO (row, other) in random order in which row i occurs exactly deg[i] times; `other` uniform in [0, n_other)."""
    rows = torch.repeat_interleave(torch.arange(len(deg)), torch.tensor(deg))
    other = torch.randint(0, n_other, (rows.numel(),), generator=gen)
    p = torch.randperm(rows.numel(), generator=gen)
    return rows[p], other[p]


def _fill(H, heads, n_dst, edges, seed):
    """Random float32 data for the COO lists `edges` = [(n_src, src, dst)]."""
    g = torch.Generator().manual_seed(seed)
    D = H // heads
    rels = []
    for n_src, src, dst in edges:
        rels.append(dict(k=torch.randn(n_src, H, generator=g), v=torch.randn(n_src, H, generator=g), src=src.long(), dst=dst.long(),
                         pscale=(torch.rand(heads, generator=g) + 0.5) / math.sqrt(D)))
    return dict(H=H, heads=heads, q=torch.randn(n_dst, H, generator=g), dm=torch.randn(n_dst, H, generator=g), rels=rels)


def _long_rows_case(H, heads, seed=0):
    """13 destination rows; a relation in which DESTINATION rows have 130, 129, 65, 64, 63, ... edges, an empty relation, and a
    relation in which SOURCE rows have 131, 66, 64, ... outgoing edges: every kernel sees second and third 64-edge batches and
    odd tails on its own side."""
    g = torch.Generator().manual_seed(100 + seed)
    n = 13
    dst_a, src_a = _degree_edges([130, 0, 1, 2, 65, 64, 63, 3, 129, 5, 0, 7, 8], 11, g)
    src_b, dst_b = _degree_edges([131, 1, 0, 66, 2, 64, 9], n, g)
    none = torch.zeros(0, dtype=torch.int64)
    return _fill(H, heads, n, [(11, src_a, dst_a), (6, none, none), (7, src_b, dst_b)], seed=H * 7 + heads)


def _for_reference(case, dtype):
    return A.attention(case["q"], case["dm"], case["heads"], case["rels"], case.get("n_keep"), dtype=dtype)


# ------------------------------------------------------------------------------------------------------------------------
# harness (GPU): CSR by the library's own build, relation / item tables, NaN-filled outputs, the four entry points
# ------------------------------------------------------------------------------------------------------------------------
def _place(t, blk, nblk, dev):
    """t as column block `blk` of a NaN-filled [n, nblk * H] matrix on the device -> (matrix, view of the block)."""
    n, H = t.shape
    full = torch.full((n, nblk * H), NAN, dtype=torch.float32, device=dev)
    view = full[:, blk * H:(blk + 1) * H]
    view.copy_(t)
    return full, view


class Attn:
    """One case on the device.  layout "plain": contiguous [n, H] operands; "blocks": q / dm / out / dq are the middle column
    block of [n, 3H] matrices (as `_HGTCore` hands them over), k / v / dk / dv of relation r block r % 3 of [n_src, 3H] ones.
    tdot "edge": [E, heads] per relation (ld_tdot = 0); "head": [heads, max E_r] per relation (ld_tdot = max E_r)."""

    def __init__(self, case, layout="plain", tdot="head"):
        from analysisgnn_amd import _lib
        from analysisgnn_amd.graph import SegSpec, build_csr
        self.lib, self._lib = _lib.load(), _lib
        self.dev = dev = torch.device(DEV)
        self.case = case
        self.H, self.heads = case["H"], case["heads"]
        self.n_full = int(case["q"].shape[0])
        self.n = int(case["n_keep"]) if case.get("n_keep") is not None else self.n_full
        nblk = 3 if layout == "blocks" else 1
        self.nblk, self.qblk = nblk, (1 if layout == "blocks" else 0)
        self.q_full, self.q = _place(case["q"], self.qblk, nblk, dev)
        self.dm_full, self.dm = _place(case["dm"], self.qblk, nblk, dev)
        rels = case["rels"]
        self.R = R = len(rels)
        self.E = [int(r["src"].numel()) for r in rels]
        self.n_src = [int(r["k"].shape[0]) for r in rels]
        self.blk = [(r % 3 if layout == "blocks" else 0) for r in range(R)]
        self.k, self.v = [], []
        for r, rel in enumerate(rels):
            self.k.append(_place(rel["k"], self.blk[r], nblk, dev))
            self.v.append(_place(rel["v"], self.blk[r], nblk, dev))
        self.ps = torch.stack([r["pscale"] for r in rels]).to(dev).contiguous() if R else torch.zeros(1, self.heads, device=dev)
        if self.n_full > 0 and R > 0:
            specs = [SegSpec(row=r["dst"].to(dev), col=r["src"].to(dev), n_rows=self.n_full) for r in rels]
            specs += [SegSpec(row=r["src"].to(dev), col=r["dst"].to(dev), n_rows=ns) for r, ns in zip(rels, self.n_src)]
            csrs = build_csr(specs)
            _lib.check_device_status(dev)
            self.fwd, self.bwd = csrs[:R], csrs[R:]
        else:
            self.fwd = self.bwd = [None] * R
        self.rowend_f = [c.rowend(r.get("e_limit")) if c is not None else None for c, r in zip(self.fwd, rels)]
        self.rowend_b = [c.rowend(r.get("e_limit")) if c is not None else None for c, r in zip(self.bwd, rels)]
        self.ld_tdot = max(self.E + [1]) if tdot == "head" else 0
        self.fresh()

    def fresh(self):
        """New NaN-filled output buffers."""
        dev, H, heads = self.dev, self.H, self.heads
        nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device=dev)          # noqa: E731
        self.out_full, self.dq_full = nan(self.n_full, self.nblk * H), nan(self.n_full, self.nblk * H)
        self.out = self.out_full[:, self.qblk * H:(self.qblk + 1) * H]
        self.dq = self.dq_full[:, self.qblk * H:(self.qblk + 1) * H]
        self.m, self.linv = nan(self.n_full, heads), nan(self.n_full, heads)
        self.alpha = [nan(max(e, 1), heads) for e in self.E]
        self.gs = [nan(max(e, 1), heads) for e in self.E]
        self.tdot = [nan(heads, self.ld_tdot) if self.ld_tdot else nan(max(e, 1), heads) for e in self.E]
        self.dk_full = [nan(ns, self.nblk * H) for ns in self.n_src]
        self.dv_full = [nan(ns, self.nblk * H) for ns in self.n_src]

    def table(self, n_rel=None):
        """The relation table; entries beyond the case's relations repeat them (relation capacity, refused calls)."""
        n_rel = self.R if n_rel is None else n_rel
        arr = (self._lib.HgtRel * max(n_rel, 1))()
        for i in range(n_rel):
            r = i % max(self.R, 1)
            c = self.fwd[r]
            arr[i].k, arr[i].v, arr[i].ld = self.k[r][1].data_ptr(), self.v[r][1].data_ptr(), self.k[r][0].stride(0)
            arr[i].rowptr, arr[i].rowend = c.rowptr.data_ptr(), self._lib.ptr(self.rowend_f[r])
            arr[i].col, arr[i].perm, arr[i].pscale = c.col.data_ptr(), c.perm.data_ptr(), self.ps[r].data_ptr()
            arr[i].alpha, arr[i].gs, arr[i].tdot = self.alpha[r].data_ptr(), self.gs[r].data_ptr(), self.tdot[r].data_ptr()
            arr[i].ld_tdot = self.ld_tdot
        return arr

    def stream(self):
        return self._lib.stream_ptr(self.dev)

    def forward(self, H=None, heads=None, ld_q=None, n_rel=None):
        arr = self.table(n_rel)
        return self.lib.agnn_hgt_attn_fwd_f32(self.R if n_rel is None else n_rel, arr, self.q.data_ptr(),
                                              self.q.stride(0) if ld_q is None else ld_q, self.n, self.H if H is None else H,
                                              self.heads if heads is None else heads, self.out.data_ptr(), self.out.stride(0),
                                              self.m.data_ptr(), self.linv.data_ptr(), self.stream())

    def backward_dst(self, H=None, heads=None, ld_q=None, n_rel=None):
        arr = self.table(n_rel)
        return self.lib.agnn_hgt_attn_bwd_dst_f32(self.R if n_rel is None else n_rel, arr, self.q.data_ptr(),
                                                  self.q.stride(0) if ld_q is None else ld_q, self.dm.data_ptr(), self.dm.stride(0),
                                                  self.out.data_ptr(), self.out.stride(0), self.m.data_ptr(), self.linv.data_ptr(), self.n,
                                                  self.H if H is None else H, self.heads if heads is None else heads, self.dq.data_ptr(),
                                                  self.dq.stride(0), self.stream())

    def src_items(self, n_items=None):
        n_items = self.R if n_items is None else n_items
        items = (self._lib.HgtSrcItem * max(n_items, 1))()
        H = self.H
        for i in range(n_items):
            r = i % max(self.R, 1)
            c, it, b = self.bwd[r], items[i], self.blk[r]
            it.rowptr, it.rowend, it.col, it.perm = c.rowptr.data_ptr(), self._lib.ptr(self.rowend_b[r]), c.col.data_ptr(), c.perm.data_ptr()
            it.alpha, it.gs = self.alpha[r].data_ptr(), self.gs[r].data_ptr()
            it.dk, it.dv = self.dk_full[r].data_ptr() + 4 * b * H, self.dv_full[r].data_ptr() + 4 * b * H
            it.ld_o, it.n_src_rows = self.dk_full[r].stride(0), self.n_src[r]
            it.col_limit = self.n if self.n < self.n_full else self._lib.INT32_MAX
        return items

    def backward_src(self, H=None, heads=None, ld_q=None, n_items=None):
        items = self.src_items(n_items)
        return self.lib.agnn_hgt_attn_bwd_src_batch_f32(self.R if n_items is None else n_items, items, self.q.data_ptr(),
                                                        self.q.stride(0) if ld_q is None else ld_q, self.dm.data_ptr(), self.dm.stride(0),
                                                        self.H if H is None else H, self.heads if heads is None else heads, self.stream())

    def run(self):
        for name, fn in (("fwd", self.forward), ("bwd_dst", self.backward_dst), ("bwd_src_batch", self.backward_src)):
            self._lib.check(fn(), f"agnn_hgt_attn_{name}_f32")
        torch.cuda.synchronize()
        return self

    def buffers(self):
        """Every output buffer, whole (neighbouring blocks and padding included), on the CPU."""
        bufs = dict(out=self.out_full, dq=self.dq_full, m=self.m, linv=self.linv)
        for r in range(self.R):
            bufs.update({f"alpha{r}": self.alpha[r], f"gs{r}": self.gs[r], f"tdot{r}": self.tdot[r], f"dk{r}": self.dk_full[r],
                         f"dv{r}": self.dv_full[r]})
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in bufs.items()}

    def all_outputs_untouched(self):
        return all(bool(torch.isnan(v).all()) for v in self.buffers().values())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _block(full, blk, H, what):
    """Column block `blk` of a [n, nblk * H] buffer; every other column must still be NaN."""
    mask = torch.zeros(full.shape[1], dtype=torch.bool)
    mask[blk * H:(blk + 1) * H] = True
    assert bool(torch.isnan(full[:, ~mask]).all()), f"{what}: a neighbouring column block was written"
    return full[:, mask]


# ------------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------------
def _compare(group, kind, got, ref64, ref32, what):
    """got (kernel, float32) against ref64 within MARGIN[kind] * max(rel_err(ref32, ref64), 2^-21) of max |ref64|."""
    got, ref32 = got.double(), ref32.double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    if not ref64.numel():
        return
    assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} slots not written"
    scale = float(ref64.abs().max())
    assert scale > 0, f"{what}: the reference is all zero — the case does not test this tensor"
    err = float((got - ref64).abs().max()) / scale
    unit = max(float((ref32 - ref64).abs().max()) / scale, FLOOR)
    print(f"PARITY group={group} kind={kind} ratio={err / unit:.3f} err={err:.3e} f32_err={unit:.3e} what={what}")
    assert err <= MARGIN[kind] * unit, (f"{what}: rel err {err:.3e} > {MARGIN[kind]:g} * {unit:.3e} (float32 evaluation of the "
                                        "reference, floor 2^-21)")


def _check(a: Attn, group, what=""):
    """All outputs of a finished run against the reference: values, exact values of rows without edges, untouched slots."""
    case, H, heads, n = a.case, a.H, a.heads, a.n
    r64, r32 = _for_reference(case, torch.float64), _for_reference(case, torch.float32)
    b = a.buffers()
    out, dq = _block(b["out"], a.qblk, H, "out"), _block(b["dq"], a.qblk, H, "dq")
    for name, t in (("out", out), ("dq", dq), ("m", b["m"]), ("linv", b["linv"])):
        assert bool(torch.isnan(t[n:]).all()), f"{what} {name}: rows beyond n_rows were written"
    out, dq, m, linv = out[:n], dq[:n], b["m"][:n], b["linv"][:n]
    empty = torch.isinf(r64["m"])                                             # [n, heads]: (row, head) without a kept edge
    assert bool((m[empty] == -float("inf")).all()) and bool(torch.isfinite(m[~empty]).all()), f"{what} m: -inf exactly on the rows without edges"
    assert bool((linv[empty] == (torch.tensor(1.0) / torch.tensor(1e-16))).all()), f"{what} linv of rows without edges"
    erow = empty[:, 0]
    assert bool((out[erow] == 0).all()) and bool((dq[erow] == 0).all()), f"{what}: out / dq of rows without edges must be 0"
    fin = lambda t: torch.where(empty, torch.zeros_like(t), t)               # noqa: E731
    _compare(group, "out", out, r64["out"], r32["out"], f"{what} out")
    _compare(group, "m", fin(m), fin(r64["m"]), fin(r32["m"]), f"{what} m")
    _compare(group, "linv", fin(linv), fin(r64["linv"]), fin(r32["linv"]), f"{what} linv")
    _compare(group, "dq", dq, r64["dq"], r32["dq"], f"{what} dq")
    for r, (x64, x32) in enumerate(zip(r64["rels"], r32["rels"])):
        keep, E = x64["keep"], a.E[r]
        for kind in ("alpha", "gs", "tdot"):
            t = b[f"{kind}{r}"]
            if kind == "tdot" and a.ld_tdot:
                assert bool(torch.isnan(t[:, E:]).all()), f"{what} tdot[{r}]: padding beyond the relation's edges was written"
                t = t[:, :E].t()
            else:
                assert bool(torch.isnan(t[E:]).all())
                t = t[:E]
            assert bool(torch.isnan(t[~keep]).all()), f"{what} {kind}[{r}]: the slot of an edge outside the kept set was written"
            _compare(group, kind, t[keep], x64[kind][keep], x32[kind][keep], f"{what} {kind}[{r}]")
        for kind in ("dk", "dv"):
            t = _block(b[f"{kind}{r}"], a.blk[r], H, f"{kind}[{r}]")
            if int(keep.sum()) == 0:
                assert bool((t == 0).all()), f"{what} {kind}[{r}]: a relation without kept edges has a zero gradient"
            else:
                _compare(group, kind, t, x64[kind], x32[kind], f"{what} {kind}[{r}]")
    return r64, b


# ------------------------------------------------------------------------------------------------------------------------
# widths: every head width, every chunk count, full forward + both backward passes on a graph with > 128-edge rows
# ------------------------------------------------------------------------------------------------------------------------
WIDTHS = ([(256, h) for h in (64, 32, 16, 8, 4, 2, 1)] + [(512, 2), (512, 4), (512, 8), (512, 128), (1024, 4), (1024, 16),
                                                           (260, 65), (384, 3), (4, 1), (64, 1)])


@pytest.mark.parametrize("H,heads", WIDTHS, ids=[f"H{H}-heads{h}-D{H // h}" for H, h in WIDTHS])
def test_widths(H, heads):
    from analysisgnn_amd.hgt import HEAD_WIDTHS
    assert H // heads in HEAD_WIDTHS
    case = _long_rows_case(H, heads)
    deg_dst = torch.bincount(case["rels"][0]["dst"], minlength=13)
    deg_src = torch.bincount(case["rels"][2]["src"], minlength=7)
    assert int(deg_dst.max()) > 128 and int(deg_src.max()) > 128
    _check(Attn(case, tdot="head" if (H // heads) in (4, 16, 64, 256) else "edge").run(), "widths", f"H={H} heads={heads}")


# ------------------------------------------------------------------------------------------------------------------------
# rows: degree patterns on both sides, partial workgroups
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,heads", [(256, 4), (1024, 16), (32, 8), (64, 4), (256, 8), (512, 4)])       # D = 64, 64, 4, 16, 32, 128
def test_rows_degrees_on_both_sides(H, heads):
    """Rows of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 500 edges as DESTINATION rows of one relation and as SOURCE rows of
    another, an empty relation between them, and a relation whose only edges — one of them twice — land on one row."""
    g = torch.Generator().manual_seed(5)
    deg = PATTERN + [0, 3]
    n = len(deg)
    dst_a, src_a = _degree_edges(deg, n, g)
    src_b, dst_b = _degree_edges(deg, n, g)
    none = torch.zeros(0, dtype=torch.int64)
    one_row = (torch.tensor([3, 3, 1, 0, 7]), torch.full((5,), 4))                   # src 3 -> row 4 twice
    case = _fill(H, heads, n, [(n, src_a, dst_a), (4, none, none), (n, src_b, dst_b), (9, *one_row)], seed=H + heads)
    assert sorted(torch.bincount(dst_a, minlength=n).tolist()) == sorted(deg)
    assert sorted(torch.bincount(src_b, minlength=n).tolist()) == sorted(deg)
    _check(Attn(case).run(), "rows", f"H={H} heads={heads}")


@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 31, 32, 33])
def test_rows_partial_workgroups(n_rows):
    """n_rows destination rows and n_rows source rows (4 rows per workgroup, the grid padded to a multiple of 8 workgroups):
    the last workgroup partly filled, whole workgroups without a row."""
    g = torch.Generator().manual_seed(n_rows)
    deg = [PATTERN[(3 * i + n_rows) % len(PATTERN)] for i in range(n_rows)]
    dst_a, src_a = _degree_edges(deg, n_rows, g)
    src_b, dst_b = _degree_edges(deg[::-1], n_rows, g)
    case = _fill(256, 4, n_rows, [(n_rows, src_a, dst_a), (n_rows, src_b, dst_b)], seed=n_rows)
    _check(Attn(case).run(), "rows", f"n_rows={n_rows}")


# ------------------------------------------------------------------------------------------------------------------------
# layout: strided operands, both tdot layouts
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdot", ["edge", "head"])
@pytest.mark.parametrize("H,heads", [(256, 4), (260, 65), (1024, 4), (64, 1)])
def test_layout_column_blocks_and_tdot(H, heads, tdot):
    """q / dm / out / dq as the middle column block of [n, 3H] matrices, k / v read from and dk / dv written into block r % 3 of
    [n_src, 3H] ones (everything around the blocks is NaN: a read outside poisons the result, a write outside is seen), with
    tdot edge-major and head-major against the same reference."""
    a = Attn(_long_rows_case(H, heads, seed=1), layout="blocks", tdot=tdot)
    assert a.q.stride(0) == 3 * H and a.k[2][1].data_ptr() == a.k[2][0].data_ptr() + 4 * 2 * H
    _check(a.run(), "layout", f"H={H} heads={heads} tdot={tdot}")


# ------------------------------------------------------------------------------------------------------------------------
# trim: rowend on both CSRs, col_limit
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,heads,n_keep,layout", [(256, 4, None, "plain"), (256, 4, 15, "plain"), (512, 128, 15, "blocks"),
                                                    (32, 4, 9, "plain"), (1024, 4, 23, "plain")])
def test_trim_rowend_and_col_limit(H, heads, n_keep, layout):
    """Five relations keeping the COO prefixes 0, 1, E/2, E - 1 and E (`Csr.rowend` on the CSR by destination and on the one
    by source), the destination rows narrowed to n_keep of 24 (`col_limit` in the source pass); the reference trims by
    masking the COO list.  Edges outside the kept set leave their alpha / gs / tdot slots untouched."""
    g = torch.Generator().manual_seed(17)
    n_full, E = 24, 150
    edges = [(18, torch.randint(0, 18, (E,), generator=g), torch.randint(0, n_full, (E,), generator=g)) for _ in range(5)]
    case = _fill(H, heads, n_full, edges, seed=H + heads)
    for rel, lim in zip(case["rels"], (0, 1, E // 2, E - 1, E)):
        rel["e_limit"] = lim
    if n_keep is not None:
        case["n_keep"] = n_keep
        assert any(bool((rel["dst"][:rel["e_limit"]] == n_keep).any()) for rel in case["rels"])   # an edge into the first dropped row
    a = Attn(case, layout=layout)
    assert a.rowend_f[0] is not None and a.rowend_b[3] is not None and a.rowend_f[4] is None
    r64, _ = _check(a.run(), "trim", f"H={H} heads={heads} n_keep={n_keep}")
    assert int(r64["rels"][0]["keep"].sum()) == 0 and int(r64["rels"][1]["keep"].sum()) <= 1 and int(r64["rels"][4]["keep"].sum()) > 0


# ------------------------------------------------------------------------------------------------------------------------
# multi: several destination types in one forward launch
# ------------------------------------------------------------------------------------------------------------------------
def _multi_call(lib, _lib, attns, n_rels, H, heads, n_items=None):
    items = (_lib.HgtDstItem * max(len(attns), 1))()
    hold = []
    for it, a, n_rel in zip(items, attns, n_rels):
        arr = a.table(n_rel) if (a.R and a.n_full) else (_lib.HgtRel * max(n_rel, 1))()     # (an item without rows: never read)
        hold.append(arr)
        it.rels, it.n_rel = C.cast(arr, C.c_void_p), n_rel
        it.q, it.ld_q, it.n_rows = a.q.data_ptr(), a.q.stride(0), a.n
        it.out, it.ld_out, it.m_out, it.linv_out = a.out.data_ptr(), a.out.stride(0), a.m.data_ptr(), a.linv.data_ptr()
    return lib.agnn_hgt_attn_fwd_multi_f32(len(attns) if n_items is None else n_items, items, H, heads, attns[0].stream())


def _multi_cases(H, heads, rel_counts, rows):
    cases = []
    for i, (R, n) in enumerate(zip(rel_counts, rows)):
        g = torch.Generator().manual_seed(40 + i)
        edges = []
        for r in range(R):
            n_src = 6 + r
            dst, src = _degree_edges([PATTERN[(i + r + j) % 6] for j in range(n)], n_src, g) if n else (torch.zeros(0, dtype=torch.int64),) * 2
            edges.append((n_src, src, dst))
        cases.append(_fill(H, heads, n, edges, seed=H + i))
    return cases


def _check_multi(H, heads, rel_counts, rows, what):
    from analysisgnn_amd import _lib
    lib = _lib.load()
    cases = _multi_cases(H, heads, rel_counts, rows)
    layouts = ["blocks", "plain", "plain", "blocks"]
    multi = [Attn(c, layout=l) for c, l in zip(cases, layouts)]
    _lib.check(_multi_call(lib, _lib, multi, rel_counts, H, heads), "agnn_hgt_attn_fwd_multi_f32")
    torch.cuda.synchronize()
    for i, (a, c, l) in enumerate(zip(multi, cases, layouts)):
        if a.n == 0:
            continue
        single = Attn(c, layout=l)
        _lib.check(single.forward(), "agnn_hgt_attn_fwd_f32")
        bm, bs = a.buffers(), single.buffers()
        for name in ("out", "m", "linv"):
            assert _same_bits(bm[name], bs[name]), f"{what} item {i} {name}: the multi launch differs from the single launch"
        r64, r32 = _for_reference(c, torch.float64), _for_reference(c, torch.float32)
        out = _block(bm["out"], a.qblk, H, "out")
        empty = torch.isinf(r64["m"])
        fin = lambda t: torch.where(empty, torch.zeros_like(t), t)           # noqa: E731
        assert bool((bm["m"][empty] == -float("inf")).all()) and bool((out[empty[:, 0]] == 0).all())
        if a.R == 0:
            assert bool(empty.all()) and bool((bm["linv"] == (torch.tensor(1.0) / torch.tensor(1e-16))).all())
            continue
        _compare("multi", "out", out, r64["out"], r32["out"], f"{what} item {i} out")
        _compare("multi", "m", fin(bm["m"]), fin(r64["m"]), fin(r32["m"]), f"{what} item {i} m")
        _compare("multi", "linv", fin(bm["linv"]), fin(r64["linv"]), fin(r32["linv"]), f"{what} item {i} linv")
    return multi


@pytest.mark.parametrize("H,heads", [(256, 4), (512, 8), (1024, 4), (16, 4)])
def test_multi_four_items(H, heads):
    """Four items: three relations; NO ROWS (between live items); rows but no relation (out = 0, m = -inf); one relation over
    33 rows.  Bitwise equal to one agnn_hgt_attn_fwd_f32 per item, and within tolerance of the reference."""
    _check_multi(H, heads, rel_counts=[3, 1, 0, 1], rows=[9, 0, 5, 33], what=f"H={H} heads={heads}")


def test_multi_relation_capacity():
    """32 relations in all (AGNN_MAX_SEG) are accepted and computed; 33 are refused before any launch."""
    from analysisgnn_amd import _lib
    lib = _lib.load()
    assert _lib.MAX_SEG == 32 and _lib.HGT_MAX_DST == 4
    multi = _check_multi(256, 4, rel_counts=[8, 8, 8, 8], rows=[5, 4, 3, 6], what="32 relations")
    for a in multi:
        a.fresh()
    rc = _multi_call(lib, _lib, multi, [8, 8, 8, 9], 256, 4)                  # the ninth entry repeats the item's first relation
    assert rc == EINVAL and lib.agnn_last_error()
    assert all(a.all_outputs_untouched() for a in multi)


# ------------------------------------------------------------------------------------------------------------------------
# range: logit magnitude
# ------------------------------------------------------------------------------------------------------------------------
def _range_case(H, heads, target, winner):
    """17 destination rows, two relations.  Rows 0 .. 12 and 16: ordinary random edges, q scaled so that max |logit| = target.
    Row 13: the FIRST edge of the row is its smallest logit (min(5, target) below every other, all heads); row 14: the first
    edge is its largest (by as much); row 15: seven edges with equal logits (sources with identical k); row 16, if `winner`: one edge whose logit
    exceeds every other of the row by more than 110 (exp(-110) < 2^-150: every other weight is 0 in float32)."""
    g = torch.Generator().manual_seed(int(target) + H)
    D = H // heads
    n, n_ord = 17, 12
    SMALL, LARGE, WIN, EQ0 = 12, 13, 14, 15                                        # special sources of relation 0
    dst0 = torch.cat([torch.randint(0, 15, (150,), generator=g), torch.full((9,), 16)])
    src0 = torch.randint(0, n_ord, (dst0.numel(),), generator=g)
    dst1 = torch.cat([torch.randint(0, 15, (100,), generator=g), torch.full((6,), 16)])
    src1 = torch.randint(0, 10, (dst1.numel(),), generator=g)
    case = _fill(H, heads, n, [(EQ0 + 7, src0, dst0), (10, src1, dst1)], seed=H + heads + int(target))
    f = A.forward(case["q"], heads, case["rels"])
    smax = max(float(p["s"].abs().max()) for p in f["per"])
    case["q"] = (case["q"].double() * (target / smax)).float()
    q, rel0 = case["q"], case["rels"][0]
    ps = rel0["pscale"].double()

    def k_for(row, logit):
        """k row that gives `logit` on every head against q[row]: k_h = q_h * logit / (|q_h|^2 pscale_h)."""
        qh = q[row].double().view(heads, D)
        return (qh * (logit / ((qh * qh).sum(-1) * ps)).unsqueeze(-1)).reshape(H).float()
    gap = min(5.0, target)
    rel0["k"][SMALL] = k_for(13, -(target + gap))
    rel0["k"][LARGE] = k_for(14, target + gap)
    rel0["k"][EQ0:EQ0 + 7] = torch.randn(H, generator=g)                            # seven identical rows
    first_src, first_dst = [SMALL, LARGE], [13, 14]                                 # at the FRONT of the COO list: first in their rows
    extra_src, extra_dst = list(range(EQ0, EQ0 + 7)), [15] * 7
    if winner:
        rel0["k"][WIN] = k_for(16, target + 115.0)
        extra_src, extra_dst = extra_src + [WIN], extra_dst + [16]
    rel0["src"] = torch.cat([torch.tensor(first_src), src0, torch.tensor(extra_src)])   # (row 15 has the equal-logit edges only)
    rel0["dst"] = torch.cat([torch.tensor(first_dst), dst0, torch.tensor(extra_dst)])
    return case


@pytest.mark.parametrize("H,heads,target,winner", [(256, 4, 1.0, False), (256, 4, 30.0, False), (256, 4, 80.0, False),
                                                    (256, 4, 30.0, True), (512, 2, 80.0, True), (32, 8, 30.0, True)])
def test_range_logit_magnitude(H, heads, target, winner):
    case = _range_case(H, heads, target, winner)
    r64 = _for_reference(case, torch.float64)
    s_max = float(torch.where(torch.isinf(r64["m"]), torch.zeros_like(r64["m"]), r64["m"]).abs().max())
    assert s_max >= 0.9 * target
    rel0 = case["rels"][0]
    a0 = r64["rels"][0]["alpha"]
    # the construction holds in float64: first edge smallest / largest, equal weights, a winner that takes all
    for row, smallest in ((13, True), (14, False)):
        mine = torch.cat([x["alpha"][rel["dst"] == row] for x, rel in zip(r64["rels"], case["rels"])])
        first = a0[0 if smallest else 1]
        assert bool((first <= mine.min(0).values).all()) if smallest else bool((first >= mine.max(0).values).all())
    a = Attn(case).run()
    _, b = _check(a, "range", f"H={H} heads={heads} max|s|={target:g} winner={winner}")
    eq = b["alpha0"][:a.E[0]][rel0["dst"] == 15].double()
    assert eq.shape[0] == 7 and float((eq * 7 - 1).abs().max()) <= 8 * FLOOR, "equal logits: alpha = 1 / degree"
    if winner:
        row = b["alpha0"][:a.E[0]][rel0["dst"] == 16]
        assert bool((row[-1] > 0.999).all()) and bool((row[:-1] == 0).all()), "every weight but the winner's underflows to 0"
        assert bool((b["alpha1"][:a.E[1]][case["rels"][1]["dst"] == 16] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------
# refusals: the host-side checks reject before any launch
# ------------------------------------------------------------------------------------------------------------------------
ENTRY = ["fwd", "fwd_multi", "bwd_dst", "bwd_src_batch"]
BAD_SHAPES = [(48, 4, "D=12"), (96, 4, "D=24"), (1024, 2, "D=512"), (256, 3, "heads does not divide H"), (0, 1, "H=0"),
              (1028, 4, "H=1028"), (6, 1, "H=6")]


def _call(a, entry, **kw):
    from analysisgnn_amd import _lib
    if entry == "fwd":
        return a.forward(**kw)
    if entry == "bwd_dst":
        return a.backward_dst(**kw)
    if entry == "bwd_src_batch":
        return a.backward_src(**kw)
    items = (_lib.HgtDstItem * 1)()
    arr = a.table()
    it = items[0]
    it.rels, it.n_rel, it.q, it.ld_q, it.n_rows = C.cast(arr, C.c_void_p), a.R, a.q.data_ptr(), kw.get("ld_q", a.q.stride(0)), a.n
    it.out, it.ld_out, it.m_out, it.linv_out = a.out.data_ptr(), a.out.stride(0), a.m.data_ptr(), a.linv.data_ptr()
    return a.lib.agnn_hgt_attn_fwd_multi_f32(1, items, kw.get("H", a.H), kw.get("heads", a.heads), a.stream())


@pytest.fixture(scope="module")
def small_attn():
    return Attn(_long_rows_case(256, 4, seed=2))


@pytest.mark.parametrize("entry", ENTRY)
@pytest.mark.parametrize("H,heads,why", BAD_SHAPES, ids=[w.replace(" ", "_") for _, _, w in BAD_SHAPES])
def test_refused_shapes(small_attn, entry, H, heads, why):
    a = small_attn
    a.fresh()
    rc = _call(a, entry, H=H, heads=heads)
    assert rc == EINVAL, f"{entry} {why}: rc = {rc}"
    assert a.lib.agnn_last_error(), "an error text is set"
    assert a.all_outputs_untouched()


@pytest.mark.parametrize("entry", ENTRY)
def test_refused_leading_dimension(small_attn, entry):
    a = small_attn
    a.fresh()
    rc = _call(a, entry, ld_q=a.H + 2)
    assert rc == EALIGN and a.lib.agnn_last_error()
    assert a.all_outputs_untouched()


@pytest.mark.parametrize("entry", ["fwd", "bwd_dst", "bwd_src_batch", "fwd_multi"])
def test_refused_counts(small_attn, entry):
    """33 relations (AGNN_MAX_SEG = 32) in the single launches and the source batch, 5 items (AGNN_HGT_MAX_DST = 4) in the
    multi launch."""
    from analysisgnn_amd import _lib
    a = small_attn
    a.fresh()
    if entry == "fwd_multi":
        items = (_lib.HgtDstItem * 5)()
        arr = a.table()
        for it in items:
            it.rels, it.n_rel, it.q, it.ld_q, it.n_rows = C.cast(arr, C.c_void_p), 1, a.q.data_ptr(), a.q.stride(0), a.n
            it.out, it.ld_out, it.m_out, it.linv_out = a.out.data_ptr(), a.out.stride(0), a.m.data_ptr(), a.linv.data_ptr()
        rc = a.lib.agnn_hgt_attn_fwd_multi_f32(5, items, a.H, a.heads, a.stream())
    elif entry == "bwd_src_batch":
        rc = a.backward_src(n_items=33)
    else:
        rc = _call(a, entry, n_rel=33)
    assert rc == EINVAL and a.lib.agnn_last_error()
    assert a.all_outputs_untouched()


# ------------------------------------------------------------------------------------------------------------------------
# determinism
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,heads", [(256, 4), (1024, 16), (260, 65)])
def test_two_runs_are_bitwise_identical(H, heads):
    a = Attn(_long_rows_case(H, heads, seed=3), layout="blocks")
    first = a.run().buffers()
    a.fresh()
    second = a.run().buffers()
    assert not bool(torch.isnan(first["out"][:, H:2 * H]).any())
    for name in first:
        assert _same_bits(first[name], second[name]), name
