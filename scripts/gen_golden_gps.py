#!/usr/bin/env python
"""Record tests/golden/gps_*.npz: the REFERENCE'S OWN graph-transformer modules (`GPSLayer`, models/core/gnn.py:426-485;
`HGPSLayer` and `HGPS`, core/hgnn.py:220-320), run in float64 on the CPU, forward and backward.  TEST INFRASTRUCTURE ONLY: it
needs the reference tree (its path in AGNN_REFERENCE); the reference's `core` directory is mounted as oracle/gen_golden.py's
`load_reference_core` mounts it (oracle/scatter_ref.py stands in for torch_scatter) and its classes are executed, never copied:
only the numbers they give are committed.

Inputs and parameters are seeded and fp32-representable (drawn in fp32 with an explicit dtype, then widened; the cotangent too,
because torch.randn follows the default dtype).  The float64 pass runs under torch.set_default_dtype(torch.float64): the
reference's hetero wrapper allocates its `out` with the default dtype, and a module that was only cast with .double() then
fails in LayerNorm with mixed dtypes.  All runs are in eval() mode.  Each file holds
    x [N, F], edge_index [2, E] (int64), edge_type [E] (int64; the hetero modules)     the inputs
    p.<name>                       every state_dict entry, float32 (exactly what the float64 run used)
    gout                           the output gradient fed to backward
    out, dx, g.<name>              the float64 results, stored rounded to float32 (6e-8 relative: the files stay small)
    meta.fp32_vs_f64               see below
The same reference module is also run in fp32 on the CPU, and every result is ASSERTED to agree with the float64 run to 1e-5 of
that tensor's largest magnitude; the worst ratio is stored.  This keeps the inputs away from ReLU kinks (a flipped unit shows as
an error of the size of a whole activation), so the GPU test needs no flip attribution.  Change a seed if a case fails here.

    AGNN_REFERENCE=/path/to/reference python scripts/gen_golden_gps.py
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
REFERENCE = os.environ.get("AGNN_REFERENCE", "")

ETYPES4 = {"onset": 0, "consecutive": 1, "during": 2, "rests": 3}
ETYPES2 = {"onset": 0, "consecutive": 1}
# module: (class name, positional arguments, keyword arguments); width: of the input
CASES = {
    "gps_hlayer_h32": dict(module=("HGPSLayer", (24, 32, 4), dict(etypes=ETYPES4)), N=300, E=1200, width=24, seed=11),
    "gps_hlayer_h64": dict(module=("HGPSLayer", (64, 64, 4), dict(etypes=ETYPES2)), N=130, E=520, width=64, seed=12),
    "gps_layer_h32": dict(module=("GPSLayer", (32, 32, 4, F.relu), {}), N=200, E=800, width=32, seed=13),
    "gps_stack": dict(module=("HGPS", (24, 32, 32, 2), dict(etypes=ETYPES2, jk=False)), N=200, E=800, width=24, seed=14),
    "gps_stack_jk": dict(module=("HGPS", (24, 32, 32, 2), dict(etypes=ETYPES2, jk=True)), N=200, E=800, width=24, seed=15),
}
FP32_BOUND = 1e-5


def reference_modules():
    assert os.path.isdir(os.path.join(REFERENCE, "analysisgnn", "models", "core")), "set AGNN_REFERENCE to the reference tree"
    from oracle import gen_golden
    gen_golden.REF_CORE = os.path.join(REFERENCE, "analysisgnn", "models", "core")
    gnn, hgnn = gen_golden.load_reference_core()
    return {"GPSLayer": gnn.GPSLayer, "HGPSLayer": hgnn.HGPSLayer, "HGPS": hgnn.HGPS}


def forward_backward(m, x, edge_index, edge_type, gout):
    x = x.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(x, edge_index) if edge_type is None else m(x, edge_index, edge_type)
    out.backward(gout)
    res = {"out": out.detach(), "dx": x.grad}
    for n, p in m.named_parameters():
        res[f"g.{n}"] = p.grad
    return res


def run(classes, module, N: int, E: int, width: int, seed: int) -> dict:
    name, args, kwargs = module
    torch.manual_seed(seed)
    m32 = classes[name](*args, **kwargs).eval()         # fp32 initialisation: every parameter is fp32-representable
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(N, width, generator=g, dtype=torch.float32)
    edge_index = torch.randint(0, N, (2, E), generator=g, dtype=torch.int64)
    hetero = "etypes" in kwargs
    edge_type = torch.randint(0, len(kwargs["etypes"]), (E,), generator=g, dtype=torch.int64) if hetero else None
    out_w = m32(x, edge_index, edge_type).shape[1] if hetero else m32(x, edge_index).shape[1]
    gout = torch.randn(N, out_w, generator=g, dtype=torch.float32)
    r32 = forward_backward(m32, x, edge_index, edge_type, gout)
    torch.set_default_dtype(torch.float64)
    try:
        m64 = copy.deepcopy(m32).double().eval()
        r64 = forward_backward(m64, x.double(), edge_index, edge_type, gout.double())
    finally:
        torch.set_default_dtype(torch.float32)
    worst = 0.0
    for k, ref in r64.items():
        assert ref.dtype == torch.float64, k
        if k.endswith("jk.att.bias"):       # cancels in the softmax over the layers: a rounding-level residue around an exact zero
            assert float(ref.abs().max()) < 1e-12 and float(r32[k].abs().max()) < 1e-5, k
            continue
        ratio = float((r32[k].double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
        assert ratio <= FP32_BOUND, f"{k}: the reference's own fp32 run is {ratio:.2e} of max|.| away from float64: change the seed"
        worst = max(worst, ratio)
    rec = {"x": x.numpy(), "edge_index": edge_index.numpy(), "gout": gout.numpy(), "meta.fp32_vs_f64": np.float64(worst)}
    if hetero:
        rec["edge_type"] = edge_type.numpy()
    for n, p in m32.state_dict().items():
        assert torch.equal(p.double(), m64.state_dict()[n])
        rec[f"p.{n}"] = p.detach().numpy()
    for k, ref in r64.items():
        rec[k] = ref.numpy().astype(np.float32)
    return rec


def main() -> None:
    classes = reference_modules()
    for name, case in CASES.items():
        rec = run(classes, **case)
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        np.savez_compressed(path, **rec)
        print(f"wrote {path}: {os.path.getsize(path)} bytes, {sum(k.startswith('g.') for k in rec)} parameter gradients, "
              f"|out|max {np.abs(rec['out']).max():.4f}, fp32 vs f64 {float(rec['meta.fp32_vs_f64']):.2e}")


if __name__ == "__main__":
    main()
