"""`agnn_multitask_eval_f32` through `analysisgnn_amd.metrics` on the GPU.  The oracle is written here from torch CPU ops —
argmax, eq, bincount, as analysisgnn/models/analysis.py:1143-1164 and :1221-1282 use them — and never calls the code under
test.  Every comparison of counters and predictions is exact integer equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TASK_DICT = {"cadence": 4, "localkey": 50, "tonkey": 50, "quality": 15, "inversion": 4, "root": 38, "bass": 38, "degree1": 22,
             "degree2": 22, "hrythm": 2, "pcset": 94, "romanNumeral": 185, "section": 2, "phrase": 2, "organ_point": 2,
             "tpc_in_label": 2, "tpc_is_root": 2, "tpc_is_bass": 2, "downbeat": 45, "note_degree": 49, "staff": 4}
JOINT = ("quality", "inversion", "degree1", "degree2", "localkey")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _offsets(widths):
    offs = [0]
    for w in widths:
        offs.append(offs[-1] + w)
    return offs


def oracle_counts(logits, segs, labels, row_mask=None, gate=-1, group=(), ignore=-1):
    """(pred int64 [T, N], counts int64 [4T + 4 + 3W]) on the CPU; W = logits.shape[1], segs = [(start, end)]."""
    T, (N, W) = len(segs), logits.shape
    pred = torch.stack([logits[:, a:b].argmax(-1) for a, b in segs])
    part = torch.ones(N, dtype=torch.bool) if row_mask is None else row_mask.bool()
    gated = pred[gate].bool() if gate >= 0 else torch.zeros(N, dtype=torch.bool)
    c = torch.zeros(4 * T + 4 + 3 * W, dtype=torch.int64)
    tp, n_pred, n_label = (c[4 * T + 4 + k * W:4 * T + 4 + (k + 1) * W] for k in range(3))
    hits, valids = [], []
    for t, (a, b) in enumerate(segs):
        y = labels[t]
        labelled = y != ignore
        in_range = labelled & (y >= 0) & (y < b - a)
        hit = in_range & pred[t].eq(y)
        valid = part & labelled
        c[t], c[T + t] = valid.sum(), (part & hit).sum()
        if gate >= 0:
            c[2 * T + t], c[3 * T + t] = (valid & gated).sum(), (part & hit & gated).sum()
        n_pred[a:b] += torch.bincount(pred[t][valid], minlength=b - a)
        n_label[a:b] += torch.bincount(y[part & in_range], minlength=b - a)
        tp[a:b] += torch.bincount(y[part & hit], minlength=b - a)
        hits.append(hit)
        valids.append(labelled)
    if len(group):
        jv = part & torch.stack([valids[t] for t in group]).all(0)
        jc = jv & torch.stack([hits[t] for t in group]).all(0)
        c[4 * T:4 * T + 4] = torch.stack([jv.sum(), jc.sum(), (jv & gated).sum(), (jc & gated).sum()])
    return pred, c


def _labels(widths, N, gen, ignored_task=None):
    lab = torch.stack([torch.randint(0, w, (N,), generator=gen) for w in widths])
    lab[torch.rand(lab.shape, generator=gen) < 0.2] = -1
    if ignored_task is not None:
        lab[ignored_task] = -1
    return lab


# ---- 1. widths around one 16-lane pass, row counts that rows per wave and per block do not divide, two memory layouts -------------
@pytest.mark.parametrize("layout", ["contiguous", "slice"])
@pytest.mark.parametrize("N", [1, 3, 257, 1030])
def test_counts_and_pred_match_the_oracle(dev, N, layout):
    from analysisgnn_amd.metrics import MultiTaskMetrics, multitask_argmax
    widths = [2, 15, 16, 17, 49, 185]
    tasks = ["g", "a", "b", "c", "d", "e"]
    offs = _offsets(widths)
    W = offs[-1]
    gen = torch.Generator().manual_seed(100 + N)
    if layout == "contiguous":
        z = torch.randn(N, W, generator=gen)
        zd = z.to(dev)
    else:                                                   # odd row stride, the first column 12 bytes into the row
        big = torch.randn(N, W + 7, generator=gen)
        z = big[:, 3:3 + W]
        zd = big.to(dev)[:, 3:3 + W]
        assert zd.stride(0) % 2 == 1 and zd.data_ptr() % 8 == 4
    lab = _labels(widths, N, gen, ignored_task=3)
    pred_o, cnt_o = oracle_counts(z, list(zip(offs[:-1], offs[1:])), lab, gate=0, group=(1, 4))
    m = MultiTaskMetrics(tasks, offs, gate_task="g", joint=("a", "d"), device=dev)
    pred = m.update(zd, lab.to(dev), return_pred=True)
    assert pred.dtype == torch.int32 and torch.equal(pred.cpu().long(), pred_o)
    assert torch.equal(m.counts.cpu(), cnt_o)
    assert int(cnt_o[3]) == 0 and (N < 3 or int(cnt_o[:6].sum()) > 0)
    assert torch.equal(multitask_argmax(zd, offs).cpu().long(), pred_o)


# ---- 2. (and 8.) the reference's 21 heads: the histogram at its real size, the gate and the five-key joint accuracy ----------------
def test_reference_heads_gate_and_joint(dev):
    from analysisgnn_amd.metrics import MultiTaskMetrics, metrics_from_counts
    tasks, widths = list(TASK_DICT), list(TASK_DICT.values())
    offs = _offsets(widths)
    assert offs[-1] == 634
    N, T = 515, len(tasks)
    gen = torch.Generator().manual_seed(2)
    z = torch.randn(N, 634, generator=gen)
    lab = _labels(widths, N, gen)
    # the five keys agree with the prediction on most rows, so the joint accuracies are neither 0 nor 1
    for k in JOINT:
        t = tasks.index(k)
        keep = torch.rand(N, generator=gen) < 0.8
        lab[t] = torch.where(keep & (lab[t] != -1), z[:, offs[t]:offs[t + 1]].argmax(-1), lab[t])
    gate = tasks.index("tpc_in_label")
    group = tuple(tasks.index(k) for k in JOINT)
    _, cnt_o = oracle_counts(z, list(zip(offs[:-1], offs[1:])), lab, gate=gate, group=group)
    m = MultiTaskMetrics(tasks, offs, device=dev)
    m.update(z.to(dev), lab.to(dev))
    cnt = m.counts.cpu()
    assert torch.equal(cnt, cnt_o)
    # the reference's own lines (:1153-1164, :1272-1282) on rows that carry all five labels
    logits = {k: z[:, offs[i]:offs[i + 1]] for i, k in enumerate(tasks)}
    mask = logits["tpc_in_label"].argmax(-1).bool()
    for k in JOINT:
        t = tasks.index(k)
        sel = mask & (lab[t] != -1)
        assert int(cnt[2 * T + t]) == int(sel.sum()) > 0
        assert int(cnt[3 * T + t]) == int(logits[k][sel].argmax(-1).eq(lab[t][sel]).sum())          # NCT_{k}_acc
    full = torch.stack([lab[tasks.index(k)] != -1 for k in JOINT]).all(0)
    eq = torch.stack([logits[k].argmax(-1) == lab[tasks.index(k)] for k in JOINT]).all(0)
    assert [int(v) for v in cnt[4 * T:4 * T + 4]] == [int(full.sum()), int((full & eq).sum()), int((full & mask).sum()),
                                                      int((full & mask & eq).sum())]
    assert 0 < int(cnt[4 * T + 3]) < int(cnt[4 * T + 2])                                             # total_rna_acc / RN(NCT)
    got = m.compute()
    exp = metrics_from_counts(cnt_o, offs[:-1], offs[1:], tasks)
    assert got == exp
    assert 0.0 < got["total_rna_acc"] < 1.0 and 0.0 < got["rna_acc"] < 1.0
    assert all(0.0 < got["f1"][k] < 1.0 for k in JOINT) and all(got["support"][k] > 0 for k in tasks)


# ---- 3. planted ties and specials --------------------------------------------------------------------------------------------------
def planted_rows():
    """(logits [R, 16 + 32 + 185], expected int64 [3, R]) for heads of 16 (one 16-lane pass), 32 and 185 classes."""
    inf, nan = float("inf"), float("nan")
    widths = [16, 32, 185]
    rows, exp = [], []

    def base(seed):
        g = torch.Generator().manual_seed(seed)
        return [torch.rand(w, generator=g) - 2.0 for w in widths]           # in [-2, -1)

    def add(parts, e):
        rows.append(torch.cat(parts))
        exp.append(e)
    p = base(0)                 # equal maxima inside one pass / across passes (3 and 19) / 0 and 64 + k
    p[0][[5, 9]] = 5.0; p[1][[3, 19]] = 5.0; p[2][[0, 64]] = 5.0
    add(p, [5, 3, 0])
    p = base(1)
    p[0][[9, 12]] = 0.5; p[1][[19, 20]] = 0.5; p[2][[0, 64 + 5]] = 0.5
    add(p, [9, 19, 0])
    p = base(2)
    p[0][[15, 0]] = 2.0; p[1][[31, 3, 19]] = 2.0; p[2][[64 + 15, 130, 184]] = 2.0
    add(p, [0, 3, 79])
    add([torch.full((w,), 1.0) for w in widths], [0, 0, 0])                 # an all-equal row
    p = [torch.full((w,), -inf) for w in widths]                            # -inf everywhere but one entry
    p[0][7] = -3.0; p[1][21] = -3.0; p[2][100] = -3.0
    add(p, [7, 21, 100])
    add([torch.full((w,), -inf) for w in widths], [0, 0, 0])                # all -inf
    p = base(3)                                                             # NaN at one index, larger values elsewhere
    p[0][4] = nan; p[0][10] = 9.0; p[1][17] = nan; p[1][1] = 9.0; p[2][183] = nan; p[2][0] = 9.0
    add(p, [4, 17, 183])
    p = base(4)                                                             # NaN at two indices: the first wins
    p[0][[6, 11]] = nan; p[1][[18, 2]] = nan; p[2][[150, 70]] = nan
    add(p, [6, 2, 70])
    p = base(5)                                                             # NaN beside +inf
    p[0][2] = inf; p[0][3] = nan; p[1][20] = nan; p[1][1] = inf; p[2][0] = inf; p[2][184] = nan
    add(p, [3, 20, 184])
    p = base(6)                                                             # -0 and +0 are equal; +inf twice; -inf beside finite
    p[0][3] = -0.0; p[0][8] = 0.0; p[1][[30, 14]] = inf; p[2][:] = -inf; p[2][[77, 141]] = -1e30
    add(p, [3, 14, 77])
    return torch.stack(rows), torch.tensor(exp).t().contiguous()


def test_planted_ties_and_specials(dev):
    from analysisgnn_amd.metrics import MultiTaskMetrics, multitask_argmax
    z, exp = planted_rows()
    offs = [0, 16, 48, 233]
    cpu = torch.stack([z[:, a:b].argmax(-1) for a, b in zip(offs[:-1], offs[1:])])
    assert torch.equal(cpu, exp), "the test's own expectation disagrees with torch.argmax on the CPU"
    assert torch.equal(multitask_argmax(z.to(dev), offs).cpu().long(), exp)
    # the same through the counting launch: labels = the expected classes, so every row of every task is a hit
    m = MultiTaskMetrics(["a", "b", "c"], offs, gate_task=None, joint=("a", "b", "c"), device=dev)
    pred = m.update(z.to(dev), exp.to(dev), return_pred=True)
    assert torch.equal(pred.cpu().long(), exp)
    R = z.shape[0]
    assert m.counts[:6].tolist() == [R] * 6 and m.counts[12:14].tolist() == [R, R]


# ---- 4. segments with gaps, out-of-range labels, canaries around the counter range ---------------------------------------------------
def test_gapped_segments_out_of_range_labels_and_canaries(dev):
    from analysisgnn_amd.metrics import MultiTaskMetrics
    segs = [(3, 9), (12, 20), (25, 39)]                                 # an odd first column and an odd covered range, even row stride
    N, W, T, nc = 203, 44, 3, 39
    gen = torch.Generator().manual_seed(4)
    z = torch.randn(N, W, generator=gen)
    lab = _labels([b - a for a, b in segs], N, gen)
    odd = [(0, 5, 6), (0, 6, -7), (1, 7, 8), (2, 8, 14)]                # C and -7: neither a class nor the ignore value
    lab_ign = lab.clone()
    for t, r, y in odd:
        lab[t, r], lab_ign[t, r] = y, -1
    _, cnt_o = oracle_counts(z[:, :nc], segs, lab, gate=0, group=(0, 2))
    _, cnt_i = oracle_counts(z[:, :nc], segs, lab_ign, gate=0, group=(0, 2))
    m = MultiTaskMetrics(["a", "b", "c"], segs, gate_task="a", joint=("a", "c"), device=dev)
    assert m.n_cols == nc and m.counts.numel() == 4 * T + 4 + 3 * nc
    canary = -0x0123456789ABCDEF
    buf = torch.full((m.counts.numel() + 2,), canary, dtype=torch.int64, device=dev)
    m.counts = buf[1:-1]
    m.reset()
    m.update(z.to(dev), lab.to(dev))
    cnt = m.counts.cpu()
    assert torch.equal(cnt, cnt_o)
    assert int(buf[0]) == canary and int(buf[-1]) == canary

    def bins(c):
        return [c[4 * T + 4 + k * nc:4 * T + 4 + (k + 1) * nc] for k in range(3)]
    tp, n_pred, n_label = bins(cnt)
    covered = torch.zeros(nc, dtype=torch.bool)
    for a, b in segs:
        covered[a:b] = True
    for v in (tp, n_pred, n_label):
        assert int(v[~covered].abs().sum()) == 0 and int(v[covered].sum()) > 0
    # the four odd labels are valid and wrong: against the run that ignores them, valid grows and no label / hit bin moves
    tp_i, n_pred_i, n_label_i = bins(cnt_i)
    assert (cnt[:T] - cnt_i[:T]).tolist() == [2, 1, 1] and (cnt[T:2 * T] - cnt_i[T:2 * T]).tolist() == [0, 0, 0]
    assert torch.equal(tp, tp_i) and torch.equal(n_label, n_label_i)
    assert int((n_pred - n_pred_i).sum()) == 4 and int((n_pred - n_pred_i).min()) == 0


# ---- 5. row masks; the gate and group counters stay untouched when switched off ----------------------------------------------------
def test_row_mask_and_switched_off_parts(dev):
    from analysisgnn_amd.metrics import MultiTaskMetrics
    widths = [2, 5, 33]
    offs = _offsets(widths)
    N, T = 77, 3
    gen = torch.Generator().manual_seed(5)
    z = torch.randn(N, offs[-1], generator=gen)
    lab = _labels(widths, N, gen)
    segs = list(zip(offs[:-1], offs[1:]))
    pred_o, cnt_all = oracle_counts(z, segs, lab, gate=0, group=(1, 2))
    m = MultiTaskMetrics(["g", "a", "b"], offs, gate_task="g", joint=("a", "b"), device=dev)
    zd, ld = z.to(dev), lab.to(dev)
    for mask in (torch.ones(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool), torch.rand(N, generator=gen) < 0.6):
        _, cnt_o = oracle_counts(z, segs, lab, row_mask=mask, gate=0, group=(1, 2))
        m.reset()
        pred = m.update(zd, ld, row_mask=mask.to(dev), return_pred=True)
        assert torch.equal(m.counts.cpu(), cnt_o)
        assert torch.equal(pred.cpu().long(), pred_o)              # written for masked rows too
    assert int(cnt_o.sum()) not in (0, int(cnt_all.sum()))
    m.reset()
    m.update(zd, ld, row_mask=(torch.rand(N, generator=gen) < 0.6).to(torch.uint8).to(dev))      # uint8 masks pass as they are
    assert 0 < int(m.counts[:T].sum()) < int(cnt_all[:T].sum())
    # no gate, no group: those counters keep whatever they held, everything else is ADDED to what is there
    off = MultiTaskMetrics(["g", "a", "b"], offs, gate_task="absent", joint=("a", "absent"), device=dev)
    assert off.gate == -1 and off.group == 0
    off.counts.fill_(1000)
    off.update(zd, ld)
    _, cnt_plain = oracle_counts(z, segs, lab)
    assert int(cnt_plain[2 * T:4 * T + 4].sum()) == 0
    assert torch.equal(off.counts.cpu(), cnt_plain + 1000)


# ---- 6. accumulation, reset, run-to-run identity, one update inside a captured graph -----------------------------------------------
def test_accumulation_reset_and_graph_replay(dev):
    from analysisgnn_amd.metrics import MultiTaskMetrics
    widths = [2, 15, 4, 22, 22, 50]
    tasks = ["tpc_in_label", "quality", "inversion", "degree1", "degree2", "localkey"]
    offs = _offsets(widths)
    N = 333
    gen = torch.Generator().manual_seed(6)
    z = torch.randn(N, offs[-1], generator=gen)
    lab = _labels(widths, N, gen)
    _, cnt_o = oracle_counts(z, list(zip(offs[:-1], offs[1:])), lab, gate=0, group=(1, 2, 3, 4, 5))
    zd, ld = z.to(dev), lab.to(dev)
    m = MultiTaskMetrics(tasks, offs, device=dev)
    m.update(zd, ld)
    whole = m.counts.clone()
    assert torch.equal(whole.cpu(), cnt_o)
    m.reset()
    assert int(m.counts.abs().sum()) == 0
    m.update(zd[:150], ld[:, :150])
    m.update(zd[150:], ld[:, 150:])
    assert torch.equal(m.counts, whole)
    m.reset()
    m.update(zd, ld)
    assert torch.equal(m.counts, whole)
    state = m.state_dict()
    # one update captured on a single stream after the eager warm-up above; each replay adds the batch once
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        m.update(zd, ld)
    m.reset()
    cg.replay()
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(m.counts, 2 * whole)
    m.load_state_dict(state)
    assert torch.equal(m.counts, whole)


# ---- 7. RN(Onset) ------------------------------------------------------------------------------------------------------------------
def onset_case():
    """Inputs and the float64 CPU oracle of models/analysis.py:1226-1264 on synth.make_batch(2, 120).  The logits are drawn in
    float64 (generator seed 0; per key randn, then randint for the class that gets +4) and rounded to fp32 for both sides: with
    these draws the oracle's smallest top-2 margin over ALL rows is 1.0e-4 (fp32 draws from the same seed: 9.4e-7)."""
    from analysisgnn_amd.synth import make_batch
    b = make_batch(2, 120)
    N = b.num_nodes["note"]
    widths = (15, 4, 22, 22)
    gen = torch.Generator().manual_seed(0)
    parts = []
    for C in widths:
        z = torch.randn(N, C, generator=gen, dtype=torch.float64)
        z[torch.arange(N), torch.randint(0, C, (N,), generator=gen)] += 4
        parts.append(z.float())                                               # what the device gets; the oracle widens it again
    edges = torch.from_numpy(np.ascontiguousarray(b.edge_index["note", "onset", "note"])).long()
    batch = torch.from_numpy(np.ascontiguousarray(b.batch["note"])).long()
    onset_div = torch.from_numpy(np.ascontiguousarray(b.onset_div)).long()
    batch_size = N
    e = edges[:, (edges[0] < batch_size) & (edges[1] < batch_size)]
    e = e[:, e[0] != e[1]]
    cnt = torch.bincount(e[1], minlength=N).clamp(min=1).double()
    agg = []
    for z in parts:
        v = z.double().softmax(-1)                                            # :1217
        out = v.clone().index_add_(0, e[1], v[e[0]])                          # scatter_mean(..., out=v): the note itself in the sum,
        agg.append((out / cnt[:, None]).softmax(-1))                          # divided by the neighbour count;  :1239
    onsets = onset_div[:batch_size] - onset_div[:batch_size].min()
    first = {}
    for i, key in enumerate(zip(batch[:batch_size].tolist(), onsets.tolist())):
        first.setdefault(key, i)                                              # the first note of every (batch id, onset) pair
    sel = torch.tensor(sorted(first.values()))
    g2 = torch.Generator().manual_seed(1)
    own = torch.rand(N, generator=g2) < 0.7
    labels = torch.stack([torch.where(own, a.argmax(-1), torch.randint(0, a.shape[1], (N,), generator=g2)) for a in agg])
    top2 = torch.stack([a.topk(2, dim=-1).values for a in agg])            # every row, so also every row a mask may select
    margin = float((top2[..., 0] - top2[..., 1]).min())
    hit = torch.stack([a[sel].argmax(-1) == labels[t][sel] for t, a in enumerate(agg)]).all(0)
    return dict(N=N, n_edges=int(edges.shape[1]), widths=widths, logits=torch.cat(parts, 1), edges=edges, batch=batch, onset_div=onset_div,
                labels=labels, sel=sel, agg=agg, margin=margin, joint_valid=int(sel.numel()), joint_correct=int(hit.sum()))


def test_onset_rna_accuracy(dev):
    from analysisgnn_amd.metrics import onset_rna_accuracy
    c = onset_case()
    assert c["N"] == 240 and c["n_edges"] == 616
    assert c["margin"] >= 5e-5, c["margin"]                 # every selected row: fp32 cannot turn an argmax of the oracle round
    assert 0 < c["joint_correct"] < c["joint_valid"]
    offs = _offsets(c["widths"])
    eid = {("note", "onset", "note"): c["edges"].to(dev)}
    acc, joint = onset_rna_accuracy(c["logits"].to(dev), offs, c["labels"].to(dev), eid, c["batch"].to(dev), c["onset_div"].to(dev),
                                    c["N"], return_counts=True)
    assert joint.tolist() == [c["joint_valid"], c["joint_correct"]]
    assert acc.is_cuda and acc.dim() == 0
    assert abs(float(acc) - c["joint_correct"] / c["joint_valid"]) <= 1e-6
    # with a valid-label mask the first VALID note of a pair stands for it; pairs without one drop out
    g = torch.Generator().manual_seed(7)
    valid = torch.rand(c["N"], generator=g) < 0.5
    first = {}
    on = (c["onset_div"] - c["onset_div"].min()).tolist()
    for i, key in enumerate(zip(c["batch"].tolist(), on)):
        if valid[i]:
            first.setdefault(key, i)
    _, joint_v = onset_rna_accuracy(c["logits"].to(dev), offs, c["labels"].to(dev), eid, c["batch"].to(dev), c["onset_div"].to(dev),
                                    c["N"], valid_label_mask=valid.to(dev), return_counts=True)
    rows = torch.tensor(sorted(first.values()))
    hit = torch.stack([a[rows].argmax(-1) == c["labels"][t][rows] for t, a in enumerate(c["agg"])]).all(0)
    assert joint_v.tolist() == [len(first), int(hit.sum())] and len(first) < c["joint_valid"]
