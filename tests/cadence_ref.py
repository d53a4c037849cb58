"""Plain-torch restatement of the cadence models (models/cadence.py), of the three step functions, of agnn_balanced_ce_f32's formula
and of the join `LayerNorm(scatter_mean(x[src], dst, out=x.clone()))` with its backward, written as a row-owning kernel would
compute them (the two full models and the join are stated and pinned here, not yet built on the HIP side).  TEST INFRASTRUCTURE ONLY, CPU, any dtype: tests/test_cadence_ref.py holds it against the fixtures the reference's
own classes produced (tests/gen_golden_cadence.py) in float64, before any kernel is involved.

Parameters are a flat mapping name -> tensor under the modules' `state_dict` names.  The SAGE layers and trim_to_layer are
oracle/pyg_ref.py, MetricalGNN is oracle/encoders_ref.metrical_gnn (the library's build spec, parity unpinned), the GRU branch is
oracle/encoders_ref.hybrid_branch."""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import encoders_ref, pyg_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["gnn_h16", "neighbor_h32", "pytorch_h32", "pytorch_ps_h32", "pytorch_hybrid_h32", "pytorch_eval_h32"]
OUT = 5
EPS = 1e-5
ONSET = ("note", "onset", "note")
_CACHE: dict = {}


# ---- the join's and the loss's formulas---------------------------------------------------------------------------------------------------
def pool(x, src, dst, pool_rows: int, col_limit: int, skip_self: bool):
    """(pooled, inv_cnt): pooled_i = (x_i + sum over the valid edges src -> i) / max(cnt_i, 1) for i < pool_rows, x_i behind them.
    An edge is valid when dst < pool_rows, src < min(col_limit, n) and, with skip_self, src != dst."""
    n = x.shape[0]
    ok = (dst < pool_rows) & (src < min(col_limit, n)) & (src >= 0)
    if skip_self:
        ok = ok & (src != dst)
    s, d = src[ok], dst[ok]
    cnt = torch.zeros(n, dtype=x.dtype).index_add(0, d, torch.ones(d.shape[0], dtype=x.dtype))
    inv = 1.0 / cnt.clamp(min=1)
    inv[pool_rows:] = 1.0
    tot = x.index_add(0, d, x[s])
    return tot * inv.unsqueeze(-1), inv


def pool_norm(x, src, dst, pool_rows, col_limit, skip_self, gamma, beta, eps: float = EPS):
    """(u, y, mean, rstd, inv_cnt) of the join: the pooled rows, their LayerNorm and its statistics."""
    u, inv = pool(x, src, dst, pool_rows, col_limit, skip_self)
    mean = u.mean(dim=1)
    rstd = 1.0 / torch.sqrt(u.var(dim=1, unbiased=False) + eps)
    y = (u - mean.unsqueeze(-1)) * rstd.unsqueeze(-1) * gamma + beta
    return u, y, mean, rstd, inv


def pool_bwd(du, src, dst, inv_cnt, pool_rows, col_limit, skip_self):
    """dx of the pooling, written from its own formula (not by autograd)."""
    n = du.shape[0]
    ok = (dst < pool_rows) & (src < min(col_limit, n)) & (src >= 0)
    if skip_self:
        ok = ok & (src != dst)
    s, d = src[ok], dst[ok]
    scale = inv_cnt.clone()
    scale[pool_rows:] = 1.0
    dx = du * scale.unsqueeze(-1)
    return dx.index_add(0, s, du[d] * inv_cnt[d].unsqueeze(-1))


def balanced_ce(z, y, ignore_index: int = -100, eps_w: float = 1e-6):
    """(loss, dlogits, class_count, weight, bad) of agnn_balanced_ce_f32 from its formula; no valid row: 0 and zeros."""
    n, C = z.shape
    valid = (y != ignore_index) & (y >= 0) & (y < C)
    bad = int(((y != ignore_index) & ~((y >= 0) & (y < C))).sum())
    yv = y[valid]
    count = torch.bincount(yv, minlength=C)
    w = 1.0 / (count.to(z.dtype) + eps_w)
    d = torch.zeros_like(z)
    if yv.numel() == 0:
        return z.new_zeros(()), d, count, w, bad
    zv = z[valid]
    lse = torch.logsumexp(zv, dim=1)
    wy = w[yv]
    W = wy.sum()
    loss = (wy * (lse - zv.gather(1, yv[:, None])[:, 0])).sum() / W
    g = torch.softmax(zv, dim=1)
    g[torch.arange(yv.numel()), yv] -= 1.0
    d[valid] = g * (wy / W).unsqueeze(-1)
    return loss, d, count, w, bad


# ---- the models ---------------------------------------------------------------------------------------------------------------------
def _lin(P, name, x):
    y = x @ P[name + ".weight"].t()
    return y + P[name + ".bias"] if (name + ".bias") in P else y


def _ln(P, name, x):
    return F.layer_norm(x, (x.shape[-1],), P[name + ".weight"], P[name + ".bias"], EPS)


def _mlp5(P, pre, x):
    return _lin(P, pre + ".4", _ln(P, pre + ".2", F.relu(_lin(P, pre + ".0", x))))


def cad_clf(P, x, training: bool = True):
    h = F.relu(_lin(P, "cad_clf.0", x))
    if training:
        mean, var = h.mean(dim=0), h.var(dim=0, unbiased=False)
    else:
        mean, var = P["cad_clf.2.running_mean"].to(h.dtype), P["cad_clf.2.running_var"].to(h.dtype)
    h = (h - mean) / torch.sqrt(var + EPS) * P["cad_clf.2.weight"] + P["cad_clf.2.bias"]
    return _lin(P, "cad_clf.4", h)


def gnn(P, L: int, x, ei):
    """models/cadence.py:121-139."""
    for i in range(L - 1):
        x = pyg_ref.sage_conv(P, f"convs.{i}.", x, x, ei)
        x = _ln(P, "normalize", F.relu(x))
    return pyg_ref.sage_conv(P, f"convs.{L - 1}.", x, x, ei)


def hierarchical_sage(P, pre, edge_types, L, x_dict, ei_dict, nodes_per_hop=None, edges_per_hop=None):
    for i in range(L):
        if edges_per_hop is not None:
            x_dict, ei_dict = pyg_ref.trim_to_layer(i, nodes_per_hop, edges_per_hop, x_dict, ei_dict)
        x_dict = pyg_ref.hetero_conv_sage(P, f"{pre}convs.{i}.", edge_types, x_dict, ei_dict, "sum")
        x_dict = {k: v.relu() for k, v in x_dict.items()}
    return _lin(P, pre + "lin", x_dict["note"]), ei_dict


def _join(P, x, src, dst, pool_rows, col_limit, skip_self, mids):
    u, _ = pool(x, src, dst, pool_rows, col_limit, skip_self)
    y = _ln(P, "norm", u)
    if mids is not None:
        mids.update({"mid.join_in": x, "mid.pooled": u, "mid.join_out": y})
    return y


def neighbor_encode(P, cfg, x_dict, ei_dict, nodes_per_hop=None, edges_per_hop=None, mids: Optional[dict] = None):
    x, ei_dict = hierarchical_sage(P, "gnn.", cfg["edge_types"], cfg["L"], x_dict, ei_dict, nodes_per_hop, edges_per_hop)
    ei = ei_dict[ONSET]
    n = x.shape[0]
    return _mlp5(P, "pool_mlp", _join(P, x, ei[0], ei[1], n, n, False, mids))


def pytorch_encode(P, cfg, x_dict, ei_dict, batch_size, mask_node=None, mask_edge=None, batch=None, pitch_spelling=None,
                   mids: Optional[dict] = None):
    x_dict = dict(x_dict)
    if cfg["use_ps"]:
        table = _ln(P, "pitch_spelling_emb.1", P["pitch_spelling_emb.0.weight"])
        z = torch.cat((x_dict["note"], table[pitch_spelling]), dim=-1)
        x_dict["note"] = _ln(P, "input_projection.2", F.relu(_lin(P, "input_projection.0", z)))
    x = encoders_ref.metrical_gnn(P, "gnn.", cfg["metadata"], cfg["L"], x_dict, ei_dict, batch_size, mask_node, mask_edge)
    if cfg["hybrid"]:
        b = batch if batch is not None else torch.zeros(x_dict["note"].shape[0], dtype=torch.long)
        z = encoders_ref.hybrid_branch(P, "", x_dict["note"][:batch_size], b[:batch_size])
        x = _lin(P, "cat_proj", torch.cat((x, z), dim=-1))
    ei = ei_dict[ONSET]
    return _mlp5(P, "pool_mlp", _join(P, x, ei[0], ei[1], batch_size, batch_size, True, mids))


# ---- the step functions -------------------------------------------------------------------------------------------------------------
def smoothed_ce(logits, y, eps: float = 0.1):
    lp = torch.log_softmax(logits, dim=1)
    return ((1 - eps) * (-lp.gather(1, y[:, None])[:, 0]) + eps * (-lp.mean(dim=1))).mean()


def feature_term(x, x_over, y_over, y, perms=None, cut: int = 100, threshold: float = 1.0):
    """mean(x^2) + per class of y_over the mean of clamp(min_j |q - c_j| - threshold, 0); a class with more than `cut` rows is cut
    to the first `cut` of its permutation (perms in the order smote.feature_penalty takes them)."""
    perms = list(perms) if perms is not None else []
    f = x.pow(2).mean()
    for c in torch.unique(y_over).tolist():
        xc, xo = x[y == c], x_over[y_over == c]
        if xc.shape[0] > cut:
            xc = xc[perms.pop(0)[:cut]]
        if xo.shape[0] > cut:
            xo = xo[perms.pop(0)[:cut]]
        d2 = (xo[:, None, :] - xc[None, :, :]).pow(2).sum(dim=-1).min(dim=1).values
        d = torch.sqrt(d2.clamp_min(1e-300))                 # an original meeting itself: distance 0, gradient 0 (not 0 / 0)
        f = f + torch.clamp(d - threshold, min=0).mean()
    return f


def training_loss(P, x, y, x_over, y_over, reg: float, epoch=None, perms=None):
    """The total of cadence_training_loss given the oversampled rows (x_over a function of x where gradients are wanted)."""
    ce = smoothed_ce(cad_clf(P, x_over, True), y_over)
    return ce + reg * feature_term(x, x_over, y_over, y, perms) * (1.0 if epoch is None else epoch * 0.01)


def metrics(logits, y):
    """(accuracy, macro F1 over the classes that occur in labels or predictions) in numpy."""
    p = logits.detach().cpu().double().numpy().argmax(axis=1)
    t = y.cpu().numpy()
    f = []
    for c in range(logits.shape[1]):
        tp, npred, nlab = int(((p == c) & (t == c)).sum()), int((p == c).sum()), int((t == c).sum())
        if npred + nlab:
            f.append(2.0 * tp / (npred + nlab))
    return float((p == t).mean()), float(np.mean(f))


# ---- the kernel tests' graph --------------------------------------------------------------------------------------------------------
def join_graph(n: int, seed: int = 0):
    """An edge list (src, dst) over n rows that holds, wherever n allows: an isolated row (row 0 when n > 1), a row whose only edge
    is a self loop (the last row), a repeated edge, sources at or beyond n - 2 (outside a col_limit of n - 2) — these first in the
    list, so that a cut of its end leaves them — and, for the rest, up to three random in-neighbours per row."""
    if n == 1:
        return torch.tensor([0]), torch.tensor([0])
    g = torch.Generator().manual_seed(1000 + 7 * n + seed)
    src: List[int] = [n - 1]                         # the last row: its self loop only
    dst: List[int] = [n - 1]
    if n >= 3:
        src += [2, 2, n - 1, n - 2]                  # a repeated edge into row 1, two sources beyond n - 2
        dst += [1, 1, 1, 1]
    for i in range(1, n - 1):
        for j in torch.randint(0, n, (int(torch.randint(0, 4, (1,), generator=g)),), generator=g).tolist():
            src.append(j)
            dst.append(i)
    return torch.tensor(src, dtype=torch.long), torch.tensor(dst, dtype=torch.long)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def load_case(name: str) -> Dict[str, np.ndarray]:
    """The arrays of a case, loaded once and shared; callers must not write into them."""
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, "cadence_" + name + ".npz")) as d:
            _CACHE[name] = {k: d[k] for k in d.files}
    return _CACHE[name]


def config(z) -> dict:
    kind = str(z["meta.kind"])
    in_feats, H, L, hybrid, use_ps, training = [int(v) for v in z["meta.cfg"]]
    cfg = dict(kind=kind, in_feats=in_feats, H=H, L=L, hybrid=bool(hybrid), use_ps=bool(use_ps), training=bool(training))
    if kind != "gnn":
        ets = [tuple(str(s) for s in row) for row in z["meta.edge_types"]]
        cfg.update(edge_types=ets, metadata=([str(t) for t in z["meta.node_types"]], ets))
    return cfg


def state(z, initial_running: Optional[bool] = None) -> Dict[str, torch.Tensor]:
    """The fixture's state_dict.  A training case recorded the running statistics AFTER its forward: they are put back at their
    initial values (what that forward started from); an eval case keeps what it read."""
    if initial_running is None:
        initial_running = bool(int(z["meta.cfg"][5]))
    sd = {}
    for k in z["meta.keys"]:
        v = torch.from_numpy(np.asarray(z["w." + str(k)]))
        if initial_running and (str(k).endswith("running_mean") or str(k).endswith("num_batches_tracked")):
            v = torch.zeros_like(v)
        elif initial_running and str(k).endswith("running_var"):
            v = torch.ones_like(v)
        sd[str(k)] = v
    return sd


def inputs(z, device="cpu") -> dict:
    cfg = config(z)
    long = lambda k: torch.from_numpy(np.asarray(z[k])).long().to(device)                                        # noqa: E731
    if cfg["kind"] == "gnn":
        return dict(x=torch.from_numpy(z["in.x.note"]).to(device), ei=long("in.ei"))
    I = dict(x_dict={t: torch.from_numpy(z["in.x." + t]).to(device) for t in cfg["metadata"][0]},
             ei_dict={et: long("in.ei." + "__".join(et)) for et in cfg["edge_types"]})
    if cfg["kind"] == "pytorch":
        I["mask_node"] = {t: long("in.mask_node." + t) for t in cfg["metadata"][0]}
        I["mask_edge"] = {et: long("in.mask_edge." + "__".join(et)) for et in cfg["edge_types"]}
        I["batch"] = long("in.batch")
        I["batch_size"] = int(z["in.batch_size"])
        I["ps"] = long("in.ps")
    else:
        I["nodes_per_hop"] = {t: [int(v) for v in z["in.nodes_per_hop." + t]] for t in cfg["metadata"][0]}
        I["edges_per_hop"] = {et: [int(v) for v in z["in.edges_per_hop." + "__".join(et)]] for et in cfg["edge_types"]}
    return I


def forward(P, cfg, I, mids: Optional[dict] = None):
    """(encode's output, the logits); `gnn`: (the stack's output, None)."""
    if cfg["kind"] == "gnn":
        return gnn(P, cfg["L"], I["x"], I["ei"]), None
    if cfg["kind"] == "pytorch":
        enc = pytorch_encode(P, cfg, I["x_dict"], I["ei_dict"], I["batch_size"], I["mask_node"], I["mask_edge"], I["batch"], I["ps"], mids)
    else:
        enc = neighbor_encode(P, cfg, I["x_dict"], I["ei_dict"], I["nodes_per_hop"], I["edges_per_hop"], mids)
    return enc, cad_clf(P, enc, cfg["training"])


def run_params(sd, cfg, I, cot_enc, cot_logits, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """One forward (dropout 0) and the backward of <enc, cot_enc> + <logits, cot_logits>: out.enc, out.logits, mid.*, grad.x (the
    note inputs), gw.* for every parameter that receives a gradient."""
    I = dict(I)
    if cfg["kind"] == "gnn":
        x = I["x"] = I["x"].to(dtype).clone().requires_grad_(True)
    else:
        I["x_dict"] = {k: v.to(dtype).clone().requires_grad_(k == "note") for k, v in I["x_dict"].items()}
        x = I["x_dict"]["note"]
    P = {k: (v.detach().to(dtype).clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v) for k, v in sd.items()}
    mids: dict = {}
    enc, logits = forward(P, cfg, I, mids)
    loss = (enc * cot_enc.to(dtype)).sum()
    if logits is not None:
        loss = loss + (logits * cot_logits.to(dtype)).sum()
    names = [k for k, v in P.items() if torch.is_tensor(v) and v.requires_grad]
    grads = torch.autograd.grad(loss, [x] + [P[k] for k in names], allow_unused=True)
    rec = {"out.enc": enc.detach(), "grad.x": grads[0]}
    if logits is not None:
        rec["out.logits"] = logits.detach()
    rec.update({k: v.detach() for k, v in mids.items()})
    for k, g in zip(names, grads[1:]):
        if g is not None:
            rec["gw." + k] = g
    return rec


def run_case(z, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    cot_l = torch.from_numpy(z["cot.logits"]) if "cot.logits" in z else None
    return run_params(state(z), config(z), inputs(z), torch.from_numpy(z["cot.enc"]), cot_l, dtype)
