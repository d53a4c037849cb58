"""The float64 restatement of SMOTE and its feature penalty (tests/smote_ref.py) against fixtures recorded from the reference
itself (scripts/gen_golden_smote.py: `x_over` at 1e-6, `y_over` exactly, the penalty at 1e-6), and the package's plan function
(`analysisgnn_amd.smote.plan`, a pure host function of the class counts) on hand-made counts.  No GPU."""
import os

import numpy as np
import pytest
import torch

import smote_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"smote_{name}.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_reproduces_the_reference_run(name):
    g = load(name)
    x, y = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["y"])
    xo, yo, info = R.fit_generate(x, y, torch.from_numpy(g["choice"]), torch.from_numpy(g["gap"]).double(), k=int(g["k"]))
    assert tuple(xo.shape) == g["x_over"].shape
    assert torch.equal(yo, torch.from_numpy(g["y_over"]))
    err = float((xo - torch.from_numpy(g["x_over"]).double()).abs().max())
    print(f"smote_{name}: max |x_over - reference| = {err:.3e}")
    assert err <= 1e-6
    assert info["S"] == g["choice"].shape[0] == R.n_synthetic(y, int(g["k"]))
    assert int(g["choice"].min()) >= 0 and int(g["choice"].max()) <= int(g["k"]) - 2          # the k-th neighbour is never used
    perms = list(torch.split(torch.from_numpy(g["perms"]), g["perm_lens"].tolist()))
    assert R.n_perms(yo, y, int(g["batch_size"])) == g["perm_lens"].tolist()
    v = float(R.feature_penalty(torch.from_numpy(g["x_over"]).double(), yo, x, y, perms, int(g["batch_size"])))
    print(f"smote_{name}: penalty {v:.9f}, reference {float(g['value']):.9f}")
    assert abs(v - float(g["value"])) <= 1e-6


def test_fixture_b_skips_the_class_below_k():
    g = load("b")
    counts = np.bincount(g["y"])
    assert 0 < counts[3] < int(g["k"])
    assert 3 not in g["y_over"][g["y"].shape[0]:]


def test_restatement_plan_agrees_with_the_package_plan():
    from analysisgnn_amd import smote
    rs = np.random.RandomState(0)
    for _ in range(200):
        counts = rs.randint(0, 40, size=rs.randint(1, 7)).tolist()
        k = int(rs.randint(2, 6))
        assert [(c.label, c.occ, c.copies) for c in smote.plan(counts, k).classes] == R.plan(counts, k)


def test_plan_on_hand_made_counts():
    from analysisgnn_amd.smote import plan
    p = plan([100, 2, 30], 3)                                     # a class below k
    assert p.dominant == 0 and [(c.label, c.copies) for c in p.classes] == [(2, 2)] and (1, "below k") in p.skipped
    p = plan([10, 6, 3], 3)                                       # (10 - 6) / 6 < 1: copies == 0 adds nothing
    assert [(c.label, c.copies) for c in p.classes] == [(2, 2)] and (1, "zero copies") in p.skipped
    p = plan([20, 50, 50, 10], 3)                                 # a tie for dominant: the first arg-max; the other adds nothing
    assert p.dominant == 1 and p.n_occ == 50 and (2, "equal to dominant") in p.skipped
    assert [(c.label, c.occ, c.copies) for c in p.classes] == [(0, 20, 1), (3, 10, 4)]
    p = plan([40, 0, 8], 3)                                       # a label that never occurs
    assert (1, "below k") in p.skipped and [(c.label, c.copies) for c in p.classes] == [(2, 4)]
    p = plan([7, 7, 7], 3)                                        # all classes equal: the output is the input
    assert p.classes == [] and p.n_synthetic == 0
    p = plan([12], 3)                                             # a single class
    assert p.classes == [] and p.skipped == [(0, "dominant")]
    assert plan([], 3).classes == []
    p = plan([210, 36, 30, 24], 3)
    assert [(c.label, c.copies) for c in p.classes] == [(1, 4), (2, 6), (3, 7)] and p.n_synthetic == 144 + 180 + 168
    assert p.offsets() == ([0, 36, 66, 90], [0, 144, 324, 492])
