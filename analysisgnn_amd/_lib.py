"""ctypes binding of libagnn_hip.so, read from include/agnn.h (_abi.py): the header is the only statement of the structs, the
prototypes and the constants.  No CPU fallback: missing library or non-GPU tensors raise.  PyTorch is used only for device memory
and the current HIP stream."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

from . import resident
from ._abi import AgnnError, read_header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagnn_hip.so")
INT32_MAX = 2 ** 31 - 1

# CONSTS: every `#define AGNN_NAME <integer>`; STRUCTS: every `typedef struct { ... } name_t` as a ctypes.Structure (pointer
# members are c_void_p); SIGNATURES: every exported symbol, name -> (restype, argtypes), struct pointers as POINTER(struct),
# parameters the header marks `/* (host) */` as POINTER(scalar) / POINTER(c_void_p), every other pointer c_void_p.
CONSTS, STRUCTS, SIGNATURES = read_header()

MAX_SEG = CONSTS["AGNN_MAX_SEG"]
SPMM_MEAN = CONSTS["AGNN_SPMM_MEAN"]
SPMM_SKIP_SELF = CONSTS["AGNN_SPMM_SKIP_SELF"]
SPMM_ACCUM = CONSTS["AGNN_SPMM_ACCUM"]
ROWEND_MAX_ITEMS = CONSTS["AGNN_ROWEND_MAX_ITEMS"]
RELT_MAX_ITEMS = CONSTS["AGNN_RELT_MAX_ITEMS"]
HGT_MAX_DST = CONSTS["AGNN_HGT_MAX_DST"]
WGRAD_BATCH_MAX = 16          # host policy, not a library limit: products (weight gradients, column sums) per batched launch
WGRAD_BATCH_MAX_ITEMS = CONSTS["AGNN_WGRAD_BATCH_MAX_ITEMS"]    # a product in two column blocks (linear.linear2) is two items
PACK_MAX_SRC = CONSTS["AGNN_PACK_MAX_SRC"]
PACK_MAX_ITEMS = CONSTS["AGNN_PACK_MAX_ITEMS"]
GRAD_MAX_SUMS = CONSTS["AGNN_GRAD_MAX_SUMS"]
EMBED_MAX_TABLES = CONSTS["AGNN_EMBED_MAX_TABLES"]
LR_CONSTANT = CONSTS["AGNN_LR_CONSTANT"]
LR_WARMUP_COSINE = CONSTS["AGNN_LR_WARMUP_COSINE"]
LR_WARMUP_EXP = CONSTS["AGNN_LR_WARMUP_EXP"]
JK_MAX_T = CONSTS["AGNN_JK_MAX_T"]
ROWSEL_MAX_K = CONSTS["AGNN_ROWSEL_MAX_K"]
ROWSEL_COSINE = CONSTS["AGNN_ROWSEL_COSINE"]
ROWSEL_SQDIST = CONSTS["AGNN_ROWSEL_SQDIST"]

CooSeg = STRUCTS["agnn_coo_seg_t"]
RowendItem = STRUCTS["agnn_rowend_item_t"]
Sampler = STRUCTS["agnn_sampler_t"]
ReltItem = STRUCTS["agnn_relt_item_t"]
Rel = STRUCTS["agnn_rel_t"]
HgtSrcItem = STRUCTS["agnn_hgt_src_item_t"]
HgtDstItem = STRUCTS["agnn_hgt_dst_item_t"]
HgtRel = STRUCTS["agnn_hgt_rel_t"]
Gated = STRUCTS["agnn_gated_t"]
WgradItem = STRUCTS["agnn_wgrad_item_t"]
ColsumItem = STRUCTS["agnn_colsum_item_t"]
PackItem = STRUCTS["agnn_pack_item_t"]
GatherItem = STRUCTS["agnn_gather_item_t"]
GradDst = STRUCTS["agnn_grad_dst_t"]
GradItem = STRUCTS["agnn_grad_item_t"]
LrSchedule = STRUCTS["agnn_lr_schedule_t"]
LstmStep = STRUCTS["agnn_lstm_step_t"]
LstmCellBwd = STRUCTS["agnn_lstm_cell_bwd_t"]
SmotePlan = STRUCTS["agnn_smote_plan_t"]
LinkTask = STRUCTS["agnn_link_task_t"]
LinkBwd = STRUCTS["agnn_link_bwd_t"]
EdgeKeys = STRUCTS["agnn_edge_keys_t"]
EdgePair = STRUCTS["agnn_edge_pair_t"]
EdgePairBwd = STRUCTS["agnn_edge_pair_bwd_t"]
EdgeCe = STRUCTS["agnn_edge_ce_t"]
EdgeCeBwd = STRUCTS["agnn_edge_ce_bwd_t"]
ScoreGraphArgs = STRUCTS["agnn_score_graph_t"]
ScoreGroupsArgs = STRUCTS["agnn_score_groups_t"]
NoteFeaturesArgs = STRUCTS["agnn_note_features_t"]

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the HIP library or raise (the product path never degrades to a CPU implementation)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AgnnError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C analysisgnn_amd/csrc`). analysisgnn_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().agnn_last_error()
        raise AgnnError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def require_gpu(*tensors: Optional[torch.Tensor]) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise AgnnError("analysisgnn_amd ops need tensors on a HIP device (no CPU fallback); "
                            f"got a tensor on {t.device}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise AgnnError(f"tensors on different devices: {dev} vs {t.device}")
    if dev is None:
        raise AgnnError("no tensor given")
    return dev


def status_word(device: torch.device) -> torch.Tensor:
    """The device-side status word handed to kernels that can detect an inconsistent index (agnn_csr_build): int32[1],
    zero-initialised once per device, only ever incremented (a resident value: it must exist before a capture starts)."""
    return resident.value(device, ("status word",), lambda: torch.zeros(1, dtype=torch.int32, device=device))


def check_device_status(device: torch.device) -> None:
    """Synchronises and raises AgnnError when a kernel flagged an inconsistency since the word was created."""
    check(load().agnn_check_status(status_word(device).data_ptr(), stream_ptr(device)), "agnn_check_status")


def stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ---- operand layout: the one statement of what a kernel may read where it lies ("Operand layout") -----------------
def rows_ok(t: torch.Tensor, vec: int = 4) -> bool:
    """A float matrix a kernel can read in place with `vec`-float vectors: fp32, 2-D, unit column stride, a leading dimension
    that is a multiple of the vector and (with more than one row) not smaller than the row, and a vector-aligned base."""
    return (t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % vec == 0
            and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]) and t.data_ptr() % (4 * vec) == 0)


def rows16(t: torch.Tensor, vec: int = 4) -> torch.Tensor:
    """`t` itself when rows_ok(t, vec), otherwise a fresh dense copy (never `.contiguous()`: a contiguous view at an odd offset
    of a flat buffer is returned unchanged by it, and stays misaligned); a width that is no multiple of 4 gets rows padded to
    one.  `vec=1`: an operand its kernel reads float by float (the grouped projections' [N, sum of classes] side, whose width
    is whatever the tasks' class counts add up to).  Raises on a wrong dtype or rank."""
    if t.dtype != torch.float32:
        raise AgnnError(f"fp32 expected, got {t.dtype}")
    if t.dim() != 2:
        raise AgnnError(f"2-D feature matrix expected, got shape {tuple(t.shape)}")
    if rows_ok(t, vec):
        return t
    n, w = t.shape
    return torch.empty((n, (w + 3) & ~3), dtype=torch.float32, device=t.device)[:, :w].copy_(t)


def vec_ok(t: torch.Tensor, vec: int = 4) -> bool:
    """A parameter vector (gamma, beta, bias, stacked weights passed flat) a kernel can read in place: fp32, dense, base aligned."""
    return t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % (4 * vec) == 0


def vec16(t: torch.Tensor) -> torch.Tensor:
    """`t` itself when vec_ok(t), otherwise a fresh dense copy.  Raises on a wrong dtype."""
    if t.dtype != torch.float32:
        raise AgnnError(f"fp32 expected, got {t.dtype}")
    return t if vec_ok(t) else t.clone(memory_format=torch.contiguous_format)


def make_rels(items: Sequence[dict]):
    arr = (Rel * len(items))()
    for i, it in enumerate(items):
        arr[i].src = it["src"]
        arr[i].rowptr = it["rowptr"]
        arr[i].rowend = it.get("rowend")
        arr[i].col = it["col"]
        arr[i].ew = it.get("ew")
        arr[i].colscale = it.get("colscale")
        arr[i].ld_src = it["ld_src"]
    return arr


# ---- measurement aid: time stamps captured into the step's hipGraph (scripts/step_stamps.py; AGNN_STAMPS=1) ----------------
STAMPS = {"on": bool(os.environ.get("AGNN_STAMPS")), "names": [], "buf": None,
          "only": [w for w in os.environ.get("AGNN_STAMPS", "").split(",") if w not in ("", "1", "all")]}


def stamp(name: str, device) -> None:
    """With AGNN_STAMPS set: a one-lane kernel on the current stream stores the 100 MHz device counter under `name` (a call
    made while a hipGraph is being captured becomes a node of it: every replay refreshes the slot).  Otherwise nothing."""
    if not STAMPS["on"] or (STAMPS["only"] and not any(w in name for w in STAMPS["only"])):
        return                          # AGNN_STAMPS=1: all of them; AGNN_STAMPS=a,b: names containing a or b (every stamp is a graph node)
    if STAMPS["buf"] is None:
        STAMPS["buf"] = torch.zeros(256, dtype=torch.int64, device=device)
    if name not in STAMPS["names"]:
        STAMPS["names"].append(name)
    k = STAMPS["names"].index(name)
    check(load().agnn_debug_stamp(STAMPS["buf"].data_ptr() + 8 * k, stream_ptr(torch.device(device))), "agnn_debug_stamp")
