"""Gradients delivered straight into the flat gradient buffer.

`agnn_grad_epilogue_f32` against the three launches it replaces (`agnn_wgrad_batch_f32`, the `agnn_pack_f32` fan-out,
`agnn_norm_act_colsum_batch_f32`): every destination bit for bit, nothing written outside.  Then whole training steps with
`linear.GRAD_IN_PLACE` on against off: the flat buffer after `pack()` and the parameters after the optimizer step are
`torch.equal`, the gradients of the kernels that take a destination already ARE their slots before `pack()`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import Guarded as _Guarded  # noqa: E402        (the NaN-guarded destination, shared with test_gpu_dense_products.py)

DEV = torch.device("cuda", 0)
NAN = float("nan")
AGNN_OK, AGNN_EINVAL, AGNN_EALIGN = 0, -22, -14        # include/agnn.h


def _bits(t):
    return t.contiguous().view(torch.int32)


def _products():
    """(dy, x, [(c0, c1, rows x cols, ld)], bias copies, follows) — x given with its leading dimension."""
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)      # noqa: E731
    out = []
    for n, o, i in ((64, 2, 2), (200, 130, 258), (131, 128, 384)):          # partial tiles, few slices
        out.append(dict(dy=rnd(n, o), x=rnd(n, i), dst=[(0, i, None)], nb=1))
    dy = rnd(300, 64)                                                         # one product in two column blocks of ONE [64, 176] matrix
    out.append(dict(dy=dy, x=rnd(300, 128), dst=[(0, 128, "blk0")], nb=1))
    out.append(dict(dy=dy, x=rnd(300, 48), dst=[(0, 48, "blk1")], nb=0))
    xp = torch.zeros(150, 282, device=DEV)                                   # 281 columns, computed on the padded 282
    xp[:, :281] = rnd(150, 281)
    out.append(dict(dy=rnd(150, 32), x=xp, dst=[(0, 281, None)], nb=1))
    R, w = 4, 32                                                              # four relation blocks, the root block four times, four biases
    out.append(dict(dy=rnd(210, 64), x=rnd(210, (R + 1) * w), nb=R,
                    dst=[(r * w, (r + 1) * w, None) for r in range(R)] + [(R * w, (R + 1) * w, None)] * R))
    out.append(dict(dy=rnd(100, 16), x=rnd(100, 24), dst=[(0, 24, "wide")], nb=1))     # ld_dw > in inside a wider matrix
    return out


def _colsums():
    from analysisgnn_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(11)
    out = []
    for H, n in ((64, 5), (256, 4096), (1344, 5000)):                        # 2, 1024 and 1024 partial rows
        nws = int(lib.agnn_norm_act_workspace_bytes(H))
        ws = torch.randn(nws // 4, generator=g).to(DEV).view(torch.uint8)
        out.append((ws, n, H))
    return out


def _destinations(products):
    """Fresh guarded destinations for every record and bias copy of every product."""
    blk = _Guarded(64, 176)
    wide = _Guarded(16, 24, ld=40)
    made = []
    for p in products:
        o = p["dy"].shape[1]
        recs = []
        for c0, c1, where in p["dst"]:
            if where == "blk0":
                recs.append((c0, c1, blk.view[:, :128], blk))
            elif where == "blk1":
                recs.append((c0, c1, blk.view[:, 128:], blk))
            elif where == "wide":
                recs.append((c0, c1, wide.view, wide))
            else:
                d = _Guarded(o, c1 - c0)
                recs.append((c0, c1, d.view, d))
        made.append((recs, [_Guarded(1, o) for _ in range(p["nb"])]))
    return made


def test_epilogue_equals_batched_products_fan_out_and_column_sums():
    from analysisgnn_amd import _lib, params
    lib = _lib.load()
    products, sums = _products(), _colsums()
    stream = _lib.stream_ptr(DEV)
    # ---- what it replaces: products into temporaries, fan-out, column sums
    ref = _destinations(products)
    tmp = []
    arr = (_lib.WgradItem * len(products))()
    for a, p in zip(arr, products):
        n, o = p["dy"].shape
        i = p["x"].shape[1]
        dw = torch.full((o, i), NAN, device=DEV)
        db = torch.full((o,), NAN, device=DEV) if p["nb"] else None
        tmp.append((dw, db))
        a.dy, a.x, a.dw, a.db = p["dy"].data_ptr(), p["x"].data_ptr(), dw.data_ptr(), _lib.ptr(db)
        a.ld_dy, a.ld_x, a.ld_dw, a.n, a.out_f, a.in_f = o, i, i, n, o, i
    nws = int(lib.agnn_wgrad_batch_workspace_bytes(len(products), arr))
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    _lib.check(lib.agnn_wgrad_batch_f32(len(products), arr, ws.data_ptr(), nws, stream), "agnn_wgrad_batch_f32")
    items = []
    for (dw, db), (recs, dbs) in zip(tmp, ref):
        for c0, c1, view, _ in recs:
            items.append((view, [dw[:, c0:c1]]))
        for d in dbs:
            items.append((d.view, [db.view(1, -1)]))
    params.pack(items, DEV)
    ref_sums = [(_Guarded(1, H), _Guarded(1, H)) for _, _, H in sums]
    sarr = (_lib.ColsumItem * len(sums))()
    for a, (wsp, n, H), (dg, db) in zip(sarr, sums, ref_sums):
        a.workspace, a.workspace_bytes, a.n, a.H = wsp.data_ptr(), wsp.numel(), n, H
        a.dgamma, a.dbeta = dg.view.data_ptr(), db.view.data_ptr()
    _lib.check(lib.agnn_norm_act_colsum_batch_f32(len(sums), sarr, stream), "agnn_norm_act_colsum_batch_f32")
    # ---- the one entry point, same items
    new = _destinations(products)
    new_sums = [(_Guarded(1, H), _Guarded(1, H)) for _, _, H in sums]
    garr = (_lib.GradItem * len(products))()
    for a, p, (recs, dbs) in zip(garr, products, new):
        n, o = p["dy"].shape
        i = p["x"].shape[1]
        a.dy, a.x, a.ld_dy, a.ld_x, a.n, a.out_f, a.in_f = p["dy"].data_ptr(), p["x"].data_ptr(), o, i, n, o, i
        a.n_dw, a.n_db = len(recs), len(dbs)
        for k, (c0, c1, view, _) in enumerate(recs):
            a.dw[k].p, a.dw[k].ld, a.dw[k].c0, a.dw[k].c1 = view.data_ptr(), view.stride(0), c0, c1
        for k, d in enumerate(dbs):
            a.db[k] = d.view.data_ptr()
    for a, (wsp, n, H), (dg, db) in zip(sarr, sums, new_sums):
        a.dgamma, a.dbeta = dg.view.data_ptr(), db.view.data_ptr()
    assert int(lib.agnn_grad_epilogue_workspace_bytes(len(products), garr)) == nws
    ws.fill_(0xFF)
    _lib.check(lib.agnn_grad_epilogue_f32(len(products), garr, len(sums), sarr, ws.data_ptr(), nws, stream), "agnn_grad_epilogue_f32")
    torch.cuda.synchronize()
    for k, ((r_recs, r_dbs), (n_recs, n_dbs)) in enumerate(zip(ref, new)):
        for j, (r, m) in enumerate(zip([x[3] for x in r_recs] + r_dbs, [x[3] for x in n_recs] + n_dbs)):
            m.check(f"product {k}, destination {j}")
            assert torch.equal(_bits(r.buf), _bits(m.buf)), f"product {k}, destination {j}"
    for k, (r, m) in enumerate(zip(ref_sums, new_sums)):
        for j in range(2):
            m[j].check(f"column sum {k}.{j}")
            assert torch.equal(_bits(r[j].buf), _bits(m[j].buf)), f"column sum {k}.{j}"


def _one_item(dst_ptrs, in_f=8, out_f=4, n=64, db=None):
    from analysisgnn_amd import _lib
    dy = torch.randn(n, out_f, device=DEV)
    x = torch.randn(n, in_f, device=DEV)
    arr = (_lib.GradItem * 1)()
    a = arr[0]
    a.dy, a.x, a.ld_dy, a.ld_x, a.n, a.out_f, a.in_f = dy.data_ptr(), x.data_ptr(), out_f, in_f, n, out_f, in_f
    a.n_dw = len(dst_ptrs)
    for k, (p, ld, c0, c1) in enumerate(dst_ptrs):
        a.dw[k].p, a.dw[k].ld, a.dw[k].c0, a.dw[k].c1 = p, ld, c0, c1
    if db is not None:
        a.n_db, a.db[0] = 1, db
    return arr, (dy, x)


def test_epilogue_validation():
    from analysisgnn_amd import _lib
    lib = _lib.load()
    stream = _lib.stream_ptr(DEV)
    assert lib.agnn_grad_epilogue_f32(0, None, 0, None, None, 0, stream) == AGNN_OK
    buf = torch.zeros(4 * 8 + 16, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    call = lambda arr: lib.agnn_grad_epilogue_f32(1, arr, 0, None, ws.data_ptr(), ws.numel(), stream)      # noqa: E731
    p = buf.data_ptr()
    arr, keep = _one_item([(p, 8, 0, 4), (p + 8, 8, 2, 6)])                 # columns 2 .. 3 of the first, 0 .. 1 of the second: the same floats
    assert call(arr) == AGNN_EINVAL
    arr, keep = _one_item([(p, 8, 0, 8)], db=p + 16)                         # the bias vector inside the matrix
    assert call(arr) == AGNN_EINVAL
    arr, keep = _one_item([(p + 4, 8, 0, 8)])                                # 4-byte aligned, even column count
    assert call(arr) == AGNN_EALIGN
    arr, keep = _one_item([(p, 8, 0, 8), (p, 8, 0, 8)])                      # declared copies of one range may coincide
    assert call(arr) == AGNN_OK
    arr, keep = _one_item([(p, 8, 0, 4), (p + 16, 8, 4, 8)])                 # column blocks of one matrix
    assert call(arr) == AGNN_OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# whole training steps, switch on against off
# ---------------------------------------------------------------------------------------------------------------------
TASKS = {"cadence": 4, "localkey": 50, "hrythm": 2}


def _batch(seeds, n_targets, neighbors=(5, 5)):
    from analysisgnn_amd.synth import make_sampled_batch, torch_inputs
    g = make_sampled_batch(len(seeds), n_targets, neighbors, score_notes=n_targets + 300, first_target=150, seeds=seeds)
    I = torch_inputs(g, 25, DEV, seed=seeds[0])
    labels = torch.stack([torch.randint(0, c, (I["batch_size"],), generator=torch.Generator().manual_seed(i)).to(DEV)
                          for i, c in enumerate(TASKS.values())])
    return g, I, labels


class _Trainer:
    def __init__(self, enc, hidden, meta):
        from analysisgnn_amd import dp
        from analysisgnn_amd.heads import MultiTaskLoss
        from analysisgnn_amd.models import TorchAnalysisGNN
        torch.manual_seed(0)
        self.model = TorchAnalysisGNN(meta, 25, hidden, 128, TASKS, 2, dropout=0.0, use_jk=False, logit_fusion=False,
                                      encoder_type=enc).to(DEV).train()
        self.clf = MultiTaskLoss(list(TASKS)).to(DEV)
        both = torch.nn.ModuleDict({"model": self.model, "clf_loss": self.clf})
        self.names = {id(p): n for n, p in both.named_parameters()}
        params, tight = dp.plan_parameters(both)
        self.flat = dp.FlatGradBuffer(params, views=False, tight=tight)
        self.opt = dp.FlatAdamW(params, self.flat, lr=5e-4, weight_decay=5e-3)

    def backward(self, batch):
        from analysisgnn_amd.heads import training_loss
        _, I, labels = batch
        x = self.model.encode(I["pitch_spelling"], I["key_signature"], I["x_dict"], I["edge_index_dict"], I["batch_dict"], I["batch_size"],
                              I["neighbor_mask_node"], I["neighbor_mask_edge"])
        logits, offs, _ = self.model.forward_clf_fused(x)
        loss, _ = training_loss(logits, offs, labels, x, 0.1, 0.1, -1, task_params=self.clf.weights())
        loss.backward()

    def in_place(self):
        """Names of the parameters whose gradient is its slot of the flat buffer right now."""
        out = set()
        for p, k, o in zip(self.flat.params, self.flat.sizes, self.flat.offsets):
            if p.grad is not None and p.grad.data_ptr() == self.flat.flat[o:o + k].data_ptr() and p.grad.shape == p.shape:
                out.add(self.names[id(p)])
        return out


@pytest.fixture()
def training_setup():
    from analysisgnn_amd import dp, graph
    was = graph.index_cache_enabled
    graph.index_cache_enabled = False
    dp.enable_wgrad_overlap(True, "sequence")
    dp.defer_weight_grads(True)
    yield
    dp.defer_weight_grads(False)
    dp.enable_wgrad_overlap(False)
    graph.index_cache_enabled = was


def _expected_elsewhere(names, enc):
    """The parameters whose gradients are NOT produced by a kernel that takes a destination, so that `pack()` copies them: the
    embedding tables (k_embed_bwd_rows and its reduction), the objective's task weights (the loss kernel), and with `hgt` the
    relation transforms, priors and skip gates (HGT kernels and torch ops) and the GRU, whose hidden size 16 is not the
    recurrence kernels' (library RNN).  Everything else — projections, LayerNorms, every SAGE relation's lin_l / lin_r, GRU
    layers of the hybrid model, task heads — must already be in its slot."""
    out = {"clf_loss.params", "model.key_embedding.weight", "model.pitch_embedding.weight"}
    if enc == "hgt":
        out |= {n for n in names if n.startswith("model.encoder.rnn.")
                or (n.startswith("model.encoder.gnn.convs.") and any(k in n for k in (".k_rel.", ".v_rel.", ".p_rel.", ".skip.")))}
    return out


@pytest.mark.parametrize("enc,hidden", [("hybridgnn", 128), ("hgt", 32)])
def test_training_step_in_place_equals_gathered(enc, hidden, monkeypatch, training_setup):
    """One step (deferred weight gradients, FlatGradBuffer(views=False), FlatAdamW, clipping) on 3 subgraphs x 700 notes."""
    from analysisgnn_amd import linear
    batch = _batch((1, 2, 3), 700)
    got = {}
    for on in (True, False):
        monkeypatch.setattr(linear, "GRAD_IN_PLACE", on)
        t = _Trainer(enc, hidden, batch[0].metadata())
        t.flat.zero()
        t.backward(batch)
        placed = t.in_place()
        t.flat.pack()
        flat = t.flat.flat.clone()
        assert all(p.grad.data_ptr() == t.flat.flat[o:o + k].data_ptr() for p, k, o in zip(t.flat.params, t.flat.sizes, t.flat.offsets))
        t.opt.step(max_norm=1.0)
        torch.cuda.synchronize()
        got[on] = (flat, t.opt.flat.clone(), placed, set(t.names.values()))
        t.flat.close()
    assert torch.isfinite(got[False][0]).all() and float(got[False][0].abs().max()) > 0
    assert torch.equal(got[True][0], got[False][0]), float((got[True][0] - got[False][0]).abs().max())
    assert torch.equal(got[True][1], got[False][1])
    assert not got[False][2], sorted(got[False][2])
    names, placed = got[True][3], got[True][2]
    print(f"{enc}: {len(placed)} of {len(names)} gradients in place; others: {sorted(names - placed)}")
    assert names - placed == _expected_elsewhere(names, enc), (sorted(names - placed - _expected_elsewhere(names, enc)),
                                                               sorted(_expected_elsewhere(names, enc) - (names - placed)))
    assert len(placed) > 50


def test_slot_of_a_layer_without_edges_is_zero_filled(monkeypatch, training_setup):
    """Step 1 samples two hops, step 2 a single one: the last SAGE layer then keeps no edge, its lin_l weights take no product
    and their slots, which hold step 1's gradient, must read zero after pack()."""
    from analysisgnn_amd import linear
    b1, b2 = _batch((1, 2, 3), 700, (5, 5)), _batch((4, 5, 6), 700, (5,))
    got = {}
    for on in (True, False):
        monkeypatch.setattr(linear, "GRAD_IN_PLACE", on)
        t = _Trainer("hybridgnn", 128, b1[0].metadata())
        flats = []
        for b in (b1, b2):
            t.flat.zero()
            t.backward(b)
            t.flat.pack()
            flats.append(t.flat.flat.clone())
            t.opt.step(max_norm=1.0)
        torch.cuda.synchronize()
        got[on] = (flats, t.opt.flat.clone())
        for p, k, o in zip(t.flat.params, t.flat.sizes, t.flat.offsets):
            n = t.names[id(p)]
            if n.startswith("model.encoder.gnn.convs.1.") and n.endswith("lin_l.weight"):
                assert float(flats[0][o:o + k].abs().max()) > 0, n
                assert float(flats[1][o:o + k].abs().max()) == 0, n
        t.flat.close()
    for a, b in zip(got[True][0], got[False][0]):
        assert torch.equal(a, b)
    assert torch.equal(got[True][1], got[False][1])


def test_accumulation_over_two_backward_passes(monkeypatch, training_setup):
    """Two backward passes without zero(): the second finds `.grad` set, must not write the slots (they hold the first pass's
    gradient, which autograd adds onto) and gives the gradients of the switch-off run."""
    from analysisgnn_amd import linear
    b1, b2 = _batch((1, 2, 3), 700), _batch((7, 8, 9), 700)
    got = {}
    for on in (True, False):
        monkeypatch.setattr(linear, "GRAD_IN_PLACE", on)
        t = _Trainer("hybridgnn", 128, b1[0].metadata())
        t.flat.zero()
        t.backward(b1)
        t.backward(b2)
        t.flat.pack()
        torch.cuda.synchronize()
        got[on] = t.flat.flat.clone()
        t.flat.close()
    assert torch.isfinite(got[False]).all()
    assert torch.equal(got[True], got[False]), float((got[True] - got[False]).abs().max())


def test_registry_follows_the_buffer(training_setup):
    from analysisgnn_amd import dp, linear
    lin = torch.nn.Linear(8, 6).to(DEV)
    a = dp.FlatGradBuffer(lin.parameters(), views=False)
    assert linear.grad_slot_of(lin.weight).data_ptr() == a.flat.data_ptr()
    b = dp.FlatGradBuffer(lin.parameters(), views=False)                      # a second buffer over the same parameters takes over
    assert linear.grad_slot_of(lin.weight).data_ptr() == b.flat.data_ptr()
    a.close()                                                                # ... and the first one's removal leaves its entries alone
    assert linear.grad_slot_of(lin.weight).data_ptr() == b.flat.data_ptr()
    got = linear.grad_slots([lin.weight])
    assert got is not None and linear.grad_slots([lin.weight]) is None       # handed out once per backward pass
    b.zero()
    assert linear.grad_slots([lin.weight]) is not None
    b.close()
    assert linear.grad_slot_of(lin.weight) is None
    c = dp.FlatGradBuffer(lin.parameters(), views=True)                       # views=True registers nothing
    assert linear.grad_slot_of(lin.weight) is None and lin.weight.grad.data_ptr() == c.flat.data_ptr()


def test_gather_copies_and_clears_many_pieces():
    """agnn_gather_f32: 300 pieces (three launches) of odd and even sizes at aligned and unaligned offsets of one buffer, every
    third one a zero-fill, one piece of several blocks; the gaps between the pieces keep their NaN."""
    from analysisgnn_amd import _lib
    g = torch.Generator().manual_seed(3)
    sizes = [1 + (37 * i) % 53 for i in range(299)] + [3 * 4096 + 5]
    buf = torch.full((sum(sizes) + 3 * len(sizes) + 8,), NAN, device=DEV)
    want = buf.clone()
    arr = (_lib.GatherItem * len(sizes))()
    keep, off = [], 2
    for i, n in enumerate(sizes):
        src = None if i % 3 == 0 else torch.randn(n + 1, generator=g).to(DEV)[i % 2:i % 2 + n]
        keep.append(src)
        arr[i].dst, arr[i].src, arr[i].n = buf[off:].data_ptr(), _lib.ptr(src), n
        want[off:off + n] = 0.0 if src is None else src
        off += n + (i % 4)
    lib = _lib.load()
    assert lib.agnn_gather_f32(0, None, _lib.stream_ptr(DEV)) == AGNN_OK
    _lib.check(lib.agnn_gather_f32(len(sizes), arr, _lib.stream_ptr(DEV)), "agnn_gather_f32")
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(want))
    arr[0].n = -1
    assert lib.agnn_gather_f32(1, arr, _lib.stream_ptr(DEV)) == AGNN_EINVAL
