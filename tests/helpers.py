"""Shared test helpers (CPU side)."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def params_from_npz(z, requires_grad=True, device="cpu"):
    """'w.<name>' arrays -> dict of leaf tensors."""
    P = {}
    for k in z.files:
        if k.startswith("w."):
            t = torch.from_numpy(np.asarray(z[k])).to(device)
            if t.is_floating_point() and requires_grad:
                t.requires_grad_(True)
            P[k[2:]] = t
    return P


def inputs_from_npz(z, grad_keys=(), device="cpu"):
    I = {}
    for k in z.files:
        if k.startswith("in."):
            t = torch.from_numpy(np.asarray(z[k])).to(device)
            if k[3:] in grad_keys:
                t.requires_grad_(True)
            I[k[3:]] = t
    return I


def assert_close(a, b, tol, what=""):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} > {tol:.1e} * {scale:.3g}"


def assert_close_rel(a, b, tol, what="", floor=1e-7):
    """max |a - b| <= tol * max |b| (+ floor): the tolerance is relative to the tensor's OWN largest magnitude,
    not to max(1, .) as `assert_close` — small-valued gradients are held to the same relative bound as O(1) logits."""
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    if not b.numel():
        return
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= tol * scale + floor, f"{what}: max abs err {err:.3e} > {tol:.1e} * max|ref| {scale:.3g}"


class Guarded:
    """A [rows, cols] destination (leading dimension `ld`) inside a NaN-filled buffer: `guard` floats in front of it and behind
    it, and whatever `ld` leaves between the rows."""

    def __init__(self, rows, cols, ld=None, guard=8, device="cuda:0"):
        self.rows, self.cols, self.ld, self.guard = rows, cols, ld or cols, guard
        self.buf = torch.full((2 * guard + rows * self.ld,), float("nan"), dtype=torch.float32, device=device)
        self.view = self.buf[guard:guard + rows * self.ld].view(rows, self.ld)[:, :cols]

    def check(self, what):
        inside = torch.zeros_like(self.buf, dtype=torch.bool)
        inside[self.guard:self.guard + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = True
        assert not torch.isnan(self.buf[inside]).any(), f"{what}: an element inside was left unwritten"
        assert torch.isnan(self.buf[~inside]).all(), f"{what}: written outside the destination"


class _DenseGrad(torch.autograd.Function):
    """Identity whose backward hands on a dense, freshly allocated copy of the gradient."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.clone(memory_format=torch.contiguous_format)


def at_offset(t, offset=1):
    """The values of `t` as a contiguous view `offset` elements into a flat buffer (where parameters and gradient slots live)."""
    flat = torch.zeros(t.numel() + offset, dtype=t.dtype, device=t.device)
    v = flat[offset:].view(t.shape)
    v.copy_(t)
    return v


def check_operand_layouts(fn, operands, misplaced):
    """`fn(*operands) -> out` (float tensors, every one a leaf that takes a gradient) run three ways on the same values, the loss
    `out.sum(0).pow(2).sum()` each time:
      (a) dense, aligned operands, the gradient reaching `fn` as a dense copy;
      (b) the same operands, the gradient reaching `fn` as autograd makes it: rows with strides (0, 1);
      (c) the operands numbered in `misplaced` at element offset 1 of a flat buffer (4 bytes past a 16-byte boundary), the
          gradient dense as in (a).
    The kernels read the same values each time: the output and every gradient are equal bit for bit."""
    def run(place, dense):
        args = [place(i, t.detach()).requires_grad_(True) for i, t in enumerate(operands)]
        out = fn(*args)
        seen = []
        out.register_hook(lambda g: seen.append(g.stride()))
        (_DenseGrad.apply(out) if dense else out).sum(0).pow(2).sum().backward()
        torch.cuda.synchronize()
        return out.detach(), [a.grad for a in args], seen[0], args

    clone = lambda i, t: t.clone()                                                    # noqa: E731
    out_a, g_a, s_a, _ = run(clone, True)
    out_b, g_b, s_b, _ = run(clone, False)
    out_c, g_c, _, args_c = run(lambda i, t: at_offset(t) if i in misplaced else t.clone(), True)
    if out_a.dim() == 2 and out_a.shape[0] > 1:
        assert s_a == (out_a.shape[1], 1) and s_b == (0, 1), (s_a, s_b)
    assert misplaced and all(args_c[i].data_ptr() % 16 == 4 for i in misplaced)
    assert any(g is not None and float(g.abs().max()) > 0 for g in g_a)
    for what, out, grads in (("broadcast gradient", out_b, g_b), ("operands at offset 1", out_c, g_c)):
        assert torch.equal(out, out_a), f"{what}: output differs"
        for i, (g, r) in enumerate(zip(grads, g_a)):
            assert (g is None) == (r is None), f"{what}: gradient of operand {i}"
            assert g is None or torch.equal(g, r), f"{what}: gradient of operand {i} differs by {float((g - r).abs().max()):.3e}"


R3_CASES = ["r3_wrapper_hybrid_fusion", "r3_wrapper_hybrid_plain_sampled", "r3_wrapper_hybrid_jk_sum", "r3_wrapper_hgt_fusion",
            "r3_wrapper_metrical_plain", "r3_wrapper_c2_h256", "r3_wrapper_c2_h256_fusion"]


def r3_case(name):
    """A round-3 wrapper fixture (oracle/gen_golden_r3.py: the reference's own TorchAnalysisGNN / MultiTaskLoss class source run
    in float64) -> (npz, cfg dict, graph, inputs on CPU, labels): everything the generator fed the reference, rebuilt."""
    from analysisgnn_amd.synth import torch_inputs
    from oracle.testing import r3_graphs
    z = load_golden(name)
    H, OUT, L, fusion, use_jk, wloss, in_ch, seed, big = (int(v) for v in z["meta.cfg"])
    cfg = dict(H=H, OUT=OUT, L=L, fusion=bool(fusion), use_jk=bool(use_jk), wloss=bool(wloss), in_ch=in_ch, seed=seed, big=bool(big),
               enc=str(z["meta.encoder"]), tasks={str(t): int(c) for t, c in zip(z["meta.tasks"], z["meta.classes"])})
    g = r3_graphs()[str(z["meta.graph"])]
    I = torch_inputs(g, in_channels=in_ch, seed=seed + 3)
    labels = torch.from_numpy(np.asarray(z["in.labels"]))
    if not big:
        assert np.array_equal(I["x_dict"]["note"].numpy(), z["in.x_note"]) and np.array_equal(I["pitch_spelling"].numpy(), z["in.pitch_spelling"])
    return z, cfg, g, I, labels


def assert_grads_close_or_relu_flips(names, hip_grads, tap64, loss64, plist, tol=1e-4, label="", max_flips=8):
    """Gradients of the fp32 HIP path (`hip_grads`, in the order of `plist`) against the float64 graph that produced `loss64`
    under `oracle.testing.ReluTap(keep_graph=True)`: each tensor within tol * max(1, |ref|max) — directly, or after removing
    the exactly computed effect of ReLU derivatives that the fp32 evaluation flipped (inputs within rounding of the kink;
    oracle.testing.explain_by_relu_flips, profiles/r03_parity_notes.md).  The flips found are printed, never tolerated blindly:
    the deviation over ALL tensors at once must be a 0/1 combination of the flip directions."""
    import torch
    from oracle.testing import explain_by_relu_flips
    g64 = torch.autograd.grad(loss64, plist, retain_graph=True, allow_unused=True)
    bound = lambda ref: tol * max(1.0, float(ref.abs().max()))                        # noqa: E731
    beyond = []
    for k, gh, gr in zip(names, hip_grads, g64):
        if gr is None:
            assert gh is None or float(gh.abs().max()) == 0.0, k
            continue
        err = float((gh.detach().cpu().double() - gr).abs().max())
        if err > bound(gr):
            beyond.append((k, f"{err:.1e}"))
    if not beyond:
        return []
    hip = [gh if gh is not None else torch.zeros_like(p) for gh, p in zip(hip_grads, plist)]
    rep = explain_by_relu_flips(tap64, loss64, plist, hip, bound)
    print(f"[{label}] {len(beyond)} gradient tensors beyond {tol:g} of float64 (e.g. {beyond[:3]}); {rep['n_candidates']} ReLU inputs near "
          f"the kink examined, flipped on the HIP path: {rep['flips']}; worst residual after removing them: {rep['worst']}")
    assert rep["ok"], f"{label}: gradient deviation is not explained by flipped ReLU derivatives: {rep['worst']}, coefficients {rep['coeffs']}"
    assert 0 < len(rep["flips"]) <= max_flips, rep["flips"]
    return rep["flips"]
