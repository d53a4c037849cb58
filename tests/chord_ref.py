"""Plain-torch restatement of the ChordGNN model in the SCHEDULE the HIP path uses (analysisgnn_amd/chord.py): the
onset mean is taken over the untransformed rows and only then `trans` is applied, to the selected rows alone; the task heads'
first layers are one stacked product and their BatchNorms one set of per-column statistics over the stacked matrix.  TEST
INFRASTRUCTURE ONLY, CPU, any dtype: tests/test_chord_ref.py holds it against the fixtures the reference's own classes produced
(tests/gen_golden_chord.py) in float64, so the schedule change is pinned before any kernel is involved.

Parameters are a flat mapping name -> tensor under the reference's `state_dict` names.  The message-passing layers, the GRU and
the LSTM of JumpingKnowledge are the restatements of oracle/intree_ref.py and oracle/rnn_ref.py (pinned against the reference
there)."""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import intree_ref as R
from oracle import rnn_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RELS = ["onset", "consecutive", "during", "rests", "consecutive_rev", "during_rev", "rests_rev"]
CASES = ["chord_h16_whole", "chord_h16_windows", "chord_h16_metrical", "chord_h16_nade", "chord_h32_resgated"]
EPS, MOMENTUM = 1e-5, 0.1
_CACHE: dict = {}


GRAD_PART_BYTES = 900 * 1024     # the generator's cap on the arrays of one gradient file


def draw_weights(model, H, seed):
    """The weights of a case, away from their initialisation so that condition (b) can hold on 48 notes.  Right after
    initialisation the rows that reach a BatchNorm are nearly copies of each other (a handful of onsets, mean aggregation, a GRU
    whose update gate averages over time), and ReLU then leaves columns that are dead or nearly so.  So: every vector (biases,
    BatchNorm / LayerNorm scales and shifts) moves by 0.1 * randn; the biases in front of a ReLU -> BatchNorm pair move up (proj1 /
    proj2 by 0.5, the metrical layers' conv_out, normalised over a handful of beats or measures, by 1.0); the encoder GRU's
    matrices are tripled and its update-gate input bias lowered by 3 (states that follow their input, row by row); NADE's VtoH,
    which adds the same positive vector to every row, is scaled by 0.2."""
    gen = torch.Generator().manual_seed(seed + 1)
    Hh = H // 2
    with torch.no_grad():
        for name, p in model.named_parameters():
            if ".gru." in name:
                if p.dim() > 1:
                    p.mul_(3.0)
                elif "bias_ih" in name:
                    p[Hh:2 * Hh].add_(-3.0)
            elif "VtoH" in name:
                p.mul_(0.2)
            elif p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=gen) * 0.1)
                if name in ("encoder.proj1.bias", "encoder.proj2.bias"):
                    p.add_(0.5)
                elif name.endswith("conv_out.bias"):
                    p.add_(1.0)
        for p in model.parameters():                       # bf16 values held in fp32: the files' compression halves them
            p.copy_(p.bfloat16().float())


def load_case(name: str) -> Dict[str, np.ndarray]:
    """The arrays of a case (both files), loaded once and shared; callers must not write into them."""
    if name not in _CACHE:
        z = {}
        for f in [name + ".npz"] + sorted(f for f in os.listdir(GOLDEN) if f.startswith(name + "_grads")):
            with np.load(os.path.join(GOLDEN, f)) as d:
                z.update({k: d[k] for k in d.files})
        _CACHE[name] = z
    return _CACHE[name]


def config(z) -> dict:
    n_notes, n_graphs, H, L, _, seed, nade, jk, metrical = [int(v) for v in z["meta.cfg"]]
    tasks = {str(t): int(c) for t, c in zip(z["meta.tasks"], z["meta.classes"])}
    return dict(n_notes=n_notes, n_graphs=n_graphs, H=H, L=L, nade=bool(nade), jk=bool(jk), metrical=bool(metrical),
                block=str(z["meta.block"]), tasks=tasks, in_feats=int(z["in.x"].shape[1]) - 128)


def inputs(z, device="cpu") -> dict:
    t = lambda k: torch.from_numpy(np.asarray(z[k])).long().to(device)                                          # noqa: E731
    I = dict(x=torch.from_numpy(z["in.x"]).to(device), edge_index=t("in.edge_index"), edge_type=t("in.edge_type"),
             onset_index=t("in.onset_index"), onset_idx=t("in.onset_idx"), lengths=t("in.lengths") if "in.lengths" in z else None)
    I["extra"] = {k: (t("in." + k) if ("in." + k) in z else None) for k in ("beat_nodes", "measure_nodes", "beat_edges", "measure_edges")}
    return I


def initial_state(z) -> Dict[str, torch.Tensor]:
    """The fixture's state_dict with the running statistics back at their initial values (what the training forward started from)."""
    sd = {}
    for k in z["meta.keys"]:
        v = torch.from_numpy(np.asarray(z["w." + str(k)]))
        if str(k).endswith("running_mean"):
            v = torch.zeros_like(v)
        elif str(k).endswith("running_var"):
            v = torch.ones_like(v)
        elif str(k).endswith("num_batches_tracked"):
            v = torch.zeros_like(v)
        sd[str(k)] = v
    return sd


class _Run:
    """Collects the running statistics the training forward leaves behind."""

    def __init__(self):
        self.out: Dict[str, torch.Tensor] = {}

    def bn(self, P, pre: str, a: torch.Tensor) -> torch.Tensor:
        """Training-mode BatchNorm1d over the rows of a [n, C]; records `pre`running_mean / running_var / num_batches_tracked."""
        n = a.shape[0]
        mean = a.mean(dim=0)
        var = a.var(dim=0, unbiased=False)
        self.out[pre + "running_mean"] = (MOMENTUM * mean).detach()                       # from 0
        self.out[pre + "running_var"] = ((1 - MOMENTUM) + MOMENTUM * var * n / (n - 1)).detach()   # from 1
        self.out[pre + "num_batches_tracked"] = torch.tensor(1)
        return (a - mean) / torch.sqrt(var + EPS) * P[pre + "weight"] + P[pre + "bias"]


def _metrical_conv(run: _Run, P, pre, x_metrical, x, edges):
    """oracle.intree_ref.metrical_conv_layer for one sequence (lengths None), with the BatchNorm's running statistics recorded."""
    nm, in_dim = x_metrical.shape[0], x.shape[1]
    agg = R._segment_sum(R._lin(P, pre + "neigh", x)[edges[0]], edges[1], nm)
    zs = torch.cat([agg, x_metrical], dim=-1).view(1, nm, -1)
    hseq = rnn_ref.gru(P, pre + "seq.", agg.view(1, nm, in_dim), num_layers=1, bidirectional=True)
    h = F.relu(R._lin(P, pre + "conv_out", torch.cat([zs, hseq], dim=-1))).reshape(nm, -1)
    h = run.bn(P, pre + "normalize.", h)
    return R._segment_sum(h[edges[1]], edges[0], x.shape[0]), h


def metrical_gnn(run: _Run, P, pre, cfg, x, ei, et, extra):
    """core/hgnn.py:373-433 with any conv block, `jk` and `metrical` (oracle.intree_ref.metrical_gnn is the metrical SAGE case)."""
    conv = {"SageConv": R.sage_conv_scatter, "ResConv": R.res_gated_conv}[cfg["block"]]
    Pp = {k[len(pre):]: v for k, v in P.items() if k.startswith(pre)}
    n_convs = cfg["L"]
    if cfg["metrical"]:
        be, me = extra["beat_edges"], extra["measure_edges"]
        h_beat = R._segment_sum(R._lin(Pp, "emb_beats", x)[be[0]], be[1], extra["beat_nodes"].numel())
        h_meas = R._segment_sum(R._lin(Pp, "emb_measures", x)[me[0]], me[1], extra["measure_nodes"].numel())

    def block(k, h, h_beat, h_meas):
        bc, h_beat = _metrical_conv(run, P, f"{pre}beat_convs.{k}.", h_beat, h, be)
        mc, h_meas = _metrical_conv(run, P, f"{pre}measure_convs.{k}.", h_meas, h, me)
        h = R._lin(Pp, f"project_metrical.{k}", torch.cat([h, bc, mc], dim=-1))
        return F.normalize(F.relu(h), p=2.0, dim=-1), h_beat, h_meas

    h, hs = x, []
    for i in range(n_convs - 1):
        if i != 0 and cfg["metrical"]:
            h, h_beat, h_meas = block(i - 1, h, h_beat, h_meas)
        h = R.hetero_layer(Pp, f"convs.{i}.", RELS, conv, h, ei, et)
        h = F.relu(F.normalize(h, p=2.0, dim=-1))
        hs.append(h)
    if cfg["jk"]:
        h = R.jumping_knowledge(Pp, "jk.", hs)
    if cfg["metrical"]:
        h, h_beat, h_meas = block(n_convs - 2, h, h_beat, h_meas)
    return R.hetero_layer(Pp, f"convs.{n_convs - 1}.", RELS, conv, h, ei, et)


def unique_onsets(onsets: torch.Tensor) -> torch.Tensor:
    """First index of each distinct value, in ascending order of the values (plain loop: the specification)."""
    first: Dict[int, int] = {}
    for i, v in enumerate(onsets.tolist()):
        first.setdefault(v, i)
    return torch.tensor([first[v] for v in sorted(first)], dtype=torch.long)


def pool_then_select(a: torch.Tensor, onset_index: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """pooled[k] = (a[idx[k]] + sum_{e : dst[e] == idx[k]} a[src[e]]) / (1 + indeg(idx[k])), on the UNTRANSFORMED rows."""
    src, dst = onset_index[0], onset_index[1]
    s = a.index_add(0, dst, a[src]) if src.numel() else a
    deg = 1 + torch.bincount(dst, minlength=a.shape[0]).to(a.dtype)
    return (s / deg.unsqueeze(-1))[idx]


def literal_pool(a, W, b, onset_index, idx):
    """models/chord.py:284-287 as written: trans, scatter-mean with appended self loops over all rows, select."""
    t = a @ W.t() + b
    n = a.shape[0]
    loops = torch.arange(n)
    src, dst = torch.cat([onset_index[0], loops]), torch.cat([onset_index[1], loops])
    out = torch.zeros_like(t).index_add(0, dst, t[src])
    cnt = torch.bincount(dst, minlength=n).to(a.dtype)
    return (out / cnt.unsqueeze(-1))[idx]


def forward(P: Dict[str, torch.Tensor], cfg: dict, I: dict):
    """(logits per task, mids, running statistics) of one TRAINING forward (dropout 0) from freshly initialised running statistics."""
    run = _Run()
    x = I["x"]
    mids = {}
    h = R._lin(P, "encoder.embedding", x[:, 2:-1])
    h = torch.cat([h, P["encoder.pitch_embedding.weight"][x[:, 0].long()], P["encoder.spelling_embedding.weight"][x[:, 1].long()]], dim=-1)
    h = metrical_gnn(run, P, "encoder.encoder.", cfg, h, I["edge_index"], I["edge_type"], I["extra"])
    h = F.normalize(F.relu(h))
    mids["mid.pool_in"] = h                                # not in the fixtures: what a test of the pool alone feeds it
    idx = I["onset_idx"]
    h = R._lin(P, "encoder.pool.trans", pool_then_select(h, I["onset_index"], idx))             # pool, select, THEN transform
    mids["mid.pooled"] = h
    h = torch.cat([h, x[:, -1][idx].unsqueeze(-1)], dim=-1)
    a = F.relu(R._lin(P, "encoder.proj1", h))
    mids["mid.bn1_in"] = a                                 # what the BatchNorm module receives: after the ReLU
    h = run.bn(P, "encoder.layernorm1.", a)
    mids["mid.bn1_out"] = h
    h = run.bn(P, "encoder.layernorm2.", F.relu(R._lin(P, "encoder.proj2", h)))
    K, C = h.shape
    B = 1 if I["lengths"] is None else int(I["lengths"].numel())
    h = rnn_ref.gru(P, "encoder.gru.", h.view(B, K // B, C), num_layers=2, bidirectional=True)
    h = F.layer_norm(h, (h.shape[-1],), P["encoder.layernormgru.weight"], P["encoder.layernormgru.bias"]).reshape(K, -1)
    mids["mid.encoder"] = h
    tasks = list(cfg["tasks"].keys())
    H = cfg["H"]
    out = {}
    if cfg["nade"]:
        for t in tasks:
            pre = f"classifier.classifier.{t}."
            a = run.bn(P, pre + "HtoV.normalize.", F.relu(R._lin(P, pre + "HtoV.layers.0", h)))
            o = R._lin(P, pre + "HtoV.layers.1", a)
            out[t] = o
            h = h + torch.sigmoid(o) @ P[pre + "VtoH.weight"].t()
    else:                                                  # stacked heads: one product, one set of per-column statistics
        pres = [f"classifier.classifier.{t}." for t in tasks]
        W1 = torch.cat([P[p + "layers.0.weight"] for p in pres])
        a = F.relu(h @ W1.t())
        n = a.shape[0]
        mean, var = a.mean(dim=0), a.var(dim=0, unbiased=False)
        gamma = torch.cat([P[p + "normalize.weight"] for p in pres])
        beta = torch.cat([P[p + "normalize.bias"] for p in pres])
        y = (a - mean) / torch.sqrt(var + EPS) * gamma + beta
        for i, (t, p) in enumerate(zip(tasks, pres)):
            run.out[p + "normalize.running_mean"] = (MOMENTUM * mean[i * H:(i + 1) * H]).detach()
            run.out[p + "normalize.running_var"] = ((1 - MOMENTUM) + MOMENTUM * var[i * H:(i + 1) * H] * n / (n - 1)).detach()
            run.out[p + "normalize.num_batches_tracked"] = torch.tensor(1)
            out[t] = y[:, i * H:(i + 1) * H] @ P[p + "layers.1.weight"].t()
    return out, mids, run.out


def run_params(state: Dict[str, torch.Tensor], cfg: dict, I: dict, cots: Dict[str, torch.Tensor], dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """One training forward and backward of sum_t <logits_t, cots_t> from the state_dict `state` (running statistics at their
    initial values): out.*, mid.*, grad.x, gw.*, and the running statistics under w.*"""
    I = dict(I)
    I["x"] = I["x"].to(dtype).clone().requires_grad_(True)
    P = {}
    for k, v in state.items():
        P[k] = v.detach().to(dtype).clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v
    out, mids, running = forward(P, cfg, I)
    loss = sum((out[t] * cots[t].to(dtype)).sum() for t in out)
    names = [k for k, v in P.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [I["x"]] + [P[k] for k in names], allow_unused=True)
    rec = {"out." + t: v.detach() for t, v in out.items()}
    rec.update({k: v.detach() for k, v in mids.items()})
    rec["grad.x"] = grads[0]
    for k, g in zip(names, grads[1:]):
        if g is not None:
            rec["gw." + k] = g
    rec.update({"w." + k: v for k, v in running.items()})
    return rec


def run_case(z, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """Every tensor the fixture holds, recomputed."""
    return run_params(initial_state(z), config(z), inputs(z), {t: torch.from_numpy(z["cot." + t]) for t in config(z)["tasks"]}, dtype)


WIDE_TASKS = {"localkey": 38, "quality": 11, "inversion": 4}


def wide_case(H: int, seed: int):
    """A model at a width the fixtures do not have (the persistent GRU kernels at H = 128 / 256, the grouped projection at 128, the
    per-task last layers at 256), on the graph and inputs of chord_h16_whole: (module on the CPU with `draw_weights` applied, cfg,
    inputs, cotangents).  No reference run stands behind it: the float64 restatement above, which the fixtures pin, is the yardstick."""
    from analysisgnn_amd import chord
    z = load_case("chord_h16_whole")
    cfg = dict(config(z), H=H, tasks=dict(WIDE_TASKS))
    torch.manual_seed(seed)
    model = chord.MetricalChordPredictionModel(cfg["in_feats"], n_hidden=H, tasks=cfg["tasks"], n_layers=cfg["L"], dropout=0.0)
    draw_weights(model, H, seed)
    gen = torch.Generator().manual_seed(seed + 7)
    K = int(z["in.onset_idx"].shape[0])
    cots = {t: torch.randn(K, c, generator=gen) for t, c in cfg["tasks"].items()}
    return model, cfg, inputs(z), cots
