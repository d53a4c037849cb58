"""`metrics.metrics_from_counts`: accuracy, macro F1 and the gated / joint ratios from the integer counters alone (no GPU).
The counters are built here with a few lines of numpy from (label, prediction) pairs, in the layout of include/agnn.h:
valid[T] | correct[T] | valid_g[T] | correct_g[T] | joint_valid, joint_correct, joint_valid_g, joint_correct_g | tp[W] |
n_pred[W] | n_label[W]."""
import math

import numpy as np
import pytest

from analysisgnn_amd.metrics import metrics_from_counts


def build_counts(widths, labels, preds, gate=-1, group=(), ignore=-1):
    """labels, preds: int [T, N].  Returns (counts, starts, ends)."""
    labels, preds = np.asarray(labels), np.asarray(preds)
    T, N = labels.shape
    starts = np.concatenate([[0], np.cumsum(widths)[:-1]]).astype(int)
    ends = starts + np.asarray(widths)
    W = int(ends[-1])
    c = np.zeros(4 * T + 4 + 3 * W, dtype=np.int64)
    tp, n_pred, n_label = (c[4 * T + 4 + k * W:4 * T + 4 + (k + 1) * W] for k in range(3))
    gated = preds[gate] != 0 if gate >= 0 else np.zeros(N, bool)
    valid = labels != ignore
    hit = valid & (labels == preds)
    for t in range(T):
        c[t], c[T + t] = valid[t].sum(), hit[t].sum()
        c[2 * T + t], c[3 * T + t] = (valid[t] & gated).sum(), (hit[t] & gated).sum()
        np.add.at(n_pred, starts[t] + preds[t][valid[t]], 1)
        np.add.at(n_label, starts[t] + labels[t][valid[t]], 1)
        np.add.at(tp, starts[t] + labels[t][hit[t]], 1)
    if len(group):
        jv, jc = valid[list(group)].all(0), hit[list(group)].all(0)
        c[4 * T:4 * T + 4] = jv.sum(), (jv & jc).sum(), (jv & gated).sum(), (jv & jc & gated).sum()
    return c, list(starts), list(ends)


def test_hand_computed_six_rows():
    # one task, four classes; class 3 is neither a label nor a prediction: it stays out of the macro mean
    labels = [[0, 0, 1, 1, 2, -1]]
    preds = [[0, 1, 1, 1, 0, 2]]
    c, s, e = build_counts([4], labels, preds)
    assert list(c[:2]) == [5, 3]
    assert list(c[8:12]) == [1, 2, 0, 0] and list(c[12:16]) == [2, 3, 0, 0] and list(c[16:20]) == [2, 2, 1, 0]     # tp, n_pred, n_label
    m = metrics_from_counts(c, s, e, ["task"])
    assert m["support"]["task"] == 5
    assert m["acc"]["task"] == 3 / 5
    # F1 per class: 0: 2*1/(2+2) = 0.5;  1: 2*2/(3+2) = 0.8;  2: 2*0/(0+1) = 0;  3: absent
    assert m["f1"]["task"] == pytest.approx((0.5 + 0.8 + 0.0) / 3, abs=1e-15)
    assert math.isnan(m["nct_acc"]["task"]) and math.isnan(m["rna_acc"]) and math.isnan(m["total_rna_acc"])
    assert all(isinstance(v, float) for v in (m["acc"]["task"], m["f1"]["task"], m["rna_acc"]))


def test_against_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(0)
    widths, N = [2, 7, 50], 400
    # some classes are never a label, some never a prediction, some neither
    lab_sets = [np.array([0, 1]), np.array([0, 1, 2, 5]), np.arange(0, 30)]
    pred_sets = [np.array([0, 1]), np.array([1, 2, 3, 5]), np.arange(10, 45)]
    labels = np.stack([rng.choice(s, N) for s in lab_sets])
    preds = np.stack([rng.choice(s, N) for s in pred_sets])
    agree = rng.random((3, N)) < 0.5
    preds = np.where(agree & np.stack([np.isin(labels[t], pred_sets[t]) for t in range(3)]), labels, preds)
    labels = np.where(rng.random((3, N)) < 0.2, -1, labels)
    c, s, e = build_counts(widths, labels, preds)
    m = metrics_from_counts(c, s, e)
    for t in range(3):
        v = labels[t] != -1
        assert 0 < v.sum() < N
        assert m["support"][t] == v.sum()
        assert abs(m["acc"][t] - skm.accuracy_score(labels[t][v], preds[t][v])) <= 1e-12
        assert abs(m["f1"][t] - skm.f1_score(labels[t][v], preds[t][v], average="macro")) <= 1e-12
        assert 0.0 < m["f1"][t] < 1.0


def test_task_without_valid_rows_gives_nan():
    labels = [[-1, -1, -1], [0, 1, -1]]
    preds = [[0, 1, 0], [0, 0, 1]]
    c, s, e = build_counts([2, 2], labels, preds)
    m = metrics_from_counts(c, s, e, ["empty", "full"])
    assert m["support"] == {"empty": 0, "full": 2}
    assert math.isnan(m["acc"]["empty"]) and math.isnan(m["f1"]["empty"]) and math.isnan(m["nct_acc"]["empty"])
    assert m["acc"]["full"] == 0.5
    assert m["f1"]["full"] == pytest.approx((2 * 1 / 3 + 0.0) / 2, abs=1e-15)     # class 0: tp 1, n_pred 2, n_label 1; class 1: tp 0


def test_gated_and_joint_ratios():
    # task 0 is the gate (rows 0, 1, 3 predict != 0); tasks 1 and 2 form the joint group
    #            row   0   1   2   3   4
    labels = [[1,  1,  0,  0,  1],
              [2,  0,  1, -1,  1],
              [0,  1,  1,  0,  0]]
    preds = [[1,  1,  0,  1,  0],
             [2,  1,  1,  0,  1],
             [0,  1,  0,  0,  0]]
    c, s, e = build_counts([2, 3, 2], labels, preds, gate=0, group=(1, 2))
    m = metrics_from_counts(c, s, e, ["gate", "a", "b"])
    assert m["acc"] == {"gate": 3 / 5, "a": 3 / 4, "b": 4 / 5}
    # gated rows 0, 1, 3: task a judges 0 (right) and 1 (wrong), row 3 is ignored; task b judges all three, all right
    assert m["nct_acc"] == {"gate": 2 / 3, "a": 1 / 2, "b": 3 / 3}
    # joint: rows 0, 1, 2, 4 carry both labels; both right on rows 0 and 4;  gated among them: rows 0, 1 -> row 0 right
    assert m["rna_acc"] == 2 / 4
    assert m["total_rna_acc"] == 1 / 2


def test_layout_is_checked():
    with pytest.raises(ValueError):
        metrics_from_counts([0] * 13, [0], [2])            # 4 + 4 + 3 W has no W with 13 counters
    with pytest.raises(ValueError):
        metrics_from_counts([0] * 14, [0], [3])            # segment wider than the W = 2 class bins
