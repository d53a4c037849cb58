"""The package's lazily created device state — side streams, resident values, kernel scratch — in one registry, keyed by device
INDEX ("cuda" and "cuda:0" are one device).  One rule while the current stream is capturing a hipGraph: nothing born under a
capture is cached, because its memory belongs to that graph's private pool and goes with the graph.
  value    must outlive any graph (host-built tables, dropout counter, status word, unit scalar): a missing one raises under
           capture; `fill=True` (the content is a plain fill) is handed out uncached instead
  scratch  a call's workspace, one per (device, lane, name) — two streams never share a ticket; under capture a missing / too
           small one is built uncached, and its zero fill becomes a node of the graph"""
from __future__ import annotations

from typing import Callable, Dict

import torch

FIFO = {"ones": 8}        # value families (a key's first element) that keep only their newest entries
_STREAMS: Dict[tuple, "torch.cuda.Stream"] = {}      # (device index, name)
_VALUES: Dict[tuple, object] = {}                    # (device index, key), in order of creation
_SCRATCH: Dict[tuple, torch.Tensor] = {}             # (device index, lane, name)


def device_index(device) -> int:
    """The HIP device index of a torch.device, a string or an int ("cuda": the current device); -1 for the CPU."""
    if isinstance(device, int):
        return device
    dev = torch.device(device)
    if dev.type != "cuda":
        return -1
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _capturing(idx: int) -> bool:
    with torch.cuda.device(idx):                     # the question goes to the current device: device `idx` (the CPU, -1: not asked)
        return idx >= 0 and torch.cuda.is_current_stream_capturing()


def stream(device, name: str, priority: int = 0) -> "torch.cuda.Stream":
    """THE side stream `name` of a device ("wgrad", "sequence", "types"), created on first use."""
    key = (device_index(device), name)
    if key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(device=key[0], priority=priority)
    return _STREAMS[key]


def lane(device) -> str:
    """The name of the current stream if it is one of `stream`'s, else "main" (any user stream, a capture's own stream)."""
    idx = device_index(device)
    cur = torch.cuda.current_stream(idx).cuda_stream if idx >= 0 else None
    return next((name for (i, name), s in _STREAMS.items() if i == idx and s.cuda_stream == cur), "main")


def value(device, key: tuple, make: Callable[[], object], fill: bool = False):
    """The resident entry `key` = (family, ...) of a device; `make()` builds it on first use."""
    idx = device_index(device)
    if (idx, key) in _VALUES:
        return _VALUES[(idx, key)]
    if _capturing(idx):
        if fill:
            return make()
        from ._lib import AgnnError                  # (here, not at the top: _lib itself keeps its status word in this registry)
        raise AgnnError(f"the resident {key[0]} of device {idx} must exist before a hipGraph capture starts (born under capture it "
                        "would belong to the graph's pool, and every replay would rebuild it): run the step once eagerly "
                        "first, or call its accessor before the capture")
    family = [k for k in _VALUES if k[1][0] == key[0]]           # a FIFO bound holds for the family over all devices together
    if key[0] in FIFO and len(family) >= FIFO[key[0]]:
        del _VALUES[family[0]]
    return _VALUES.setdefault((idx, key), make())


def scratch(device, name: str, nbytes: int, zeroed: bool) -> torch.Tensor:
    """uint8 workspace of at least `nbytes`, 256-byte aligned, of the current lane; `zeroed`: zero-filled when it is built (a
    ticket workspace: every call leaves it at zero).  Grows on demand.  Hold the returned tensor until the kernel is launched:
    under capture the registry keeps no reference, and a block freed inside a capture is handed out again within it."""
    idx = device_index(device)
    key = (idx, lane(idx), name)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        raw = (torch.zeros if zeroed else torch.empty)(nbytes + 255, dtype=torch.uint8, device="cpu" if idx < 0 else f"cuda:{idx}")
        buf = raw[-raw.data_ptr() % 256:][:nbytes]
        if not _capturing(idx):
            _SCRATCH[key] = buf
    return buf
