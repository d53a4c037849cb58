"""Known answers for the project's random stream (csrc/agnn_common.h): every mask and draw the kernels produce, rebuilt on the
CPU from oracle.sampler_ref.philox4x32_10 and the documented layout, and compared exactly.

    counter = (element index lo, element index hi, call id, step lo)        key = (seed lo, seed hi ^ step hi)
    keep    = word >= uint32(float64(float32(p)) * 2^32)                    kept value = 1 / (1 - p) in float32

Each consumer adds only its element index (the formulas are in the cases below).  The generator state is set to a seed and a
step that both have non-zero high 32 bits, so the `seed hi ^ step hi` half of the key is exercised everywhere."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.sampler_ref import philox4x32_10  # noqa: E402

DEV = "cuda:0"
M32 = 0xFFFFFFFF
SEED = 0x1234_5678_9ABC_DEF1
STEP = (0x0BAD_CAFE << 32) | 0x8000_0003


def bits(seed, step, call_id, idx):
    """The stream's four 32-bit words for element index idx (64 bits)."""
    return philox4x32_10((idx & M32, (idx >> 32) & M32, call_id & M32, step & M32), (seed & M32, ((seed >> 32) ^ (step >> 32)) & M32))


def keep4(words, p):
    """float32 keep factors of the four words: 0 below the threshold, 1 / (1 - p) at or above it."""
    p32 = np.float32(p)
    thr = int(np.float64(p32) * 4294967296.0)
    inv = np.float32(1.0) / (np.float32(1.0) - p32)
    return [inv if w >= thr else np.float32(0.0) for w in words]


@pytest.fixture
def rng():
    """The live device generator set to (SEED, STEP) for the test, put back afterwards -> the int64[2] device tensor."""
    from analysisgnn_amd import fused
    state = fused.rng_state(torch.device(DEV))
    saved = state.clone()
    state.copy_(torch.tensor([SEED, STEP], dtype=torch.int64))
    yield state
    state.copy_(saved)
    torch.cuda.synchronize()


def used_pair(used):
    seed, step = (int(v) for v in used.cpu())
    assert (seed, step) == (SEED, STEP)
    return seed, step


def test_dense_attention_keep(rng):
    """idx = (head N + q) N + key4: one counter for the four consecutive keys key4 .. key4 + 3 of a query row."""
    from analysisgnn_amd import attention
    N, D, heads, p, call_id = 65, 16, 2, 0.2, 4242
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(N, heads * D, generator=g).to(DEV) for _ in range(3))
    _, _, used = attention.forward_raw(q, k, v, heads, p, call_id)
    seed, step = used_pair(used)
    got = attention.dropout_keep(N, heads, p, used, call_id, DEV).cpu()
    want = np.zeros((heads, N, N), dtype=np.float32)
    for h in range(heads):
        for qr in range(N):
            for key4 in range(0, N, 4):
                f = keep4(bits(seed, step, call_id, (h * N + qr) * N + key4), p)
                want[h, qr, key4:key4 + 4] = f[:N - key4]
    assert torch.equal(got, torch.from_numpy(want))


def test_task_attention_keep(rng):
    """idx = ((n heads + h) 32 + i) 32 + 4 g: query i, key group g of (sequence n, head h), whatever T is."""
    from analysisgnn_amd import task_attention as ta
    n, T, heads, D, p, call_id = 5, 3, 4, 16, 0.3, 515151
    g = torch.Generator().manual_seed(12)
    qkv = torch.randn(n * T, 3 * heads * D, generator=g).to(DEV)
    _, _, used = ta.forward_raw(qkv, T, heads, p, call_id)
    seed, step = used_pair(used)
    got = ta.dropout_keep(n, T, heads, p, used, call_id, DEV).cpu()
    want = np.zeros((n, heads, T, T), dtype=np.float32)
    for s in range(n):
        for h in range(heads):
            for i in range(T):
                for grp in range((T + 3) // 4):
                    f = keep4(bits(seed, step, call_id, ((s * heads + h) * 32 + i) * 32 + 4 * grp), p)
                    want[s, h, i, 4 * grp:4 * grp + 4] = f[:T - 4 * grp]
    assert torch.equal(got, torch.from_numpy(want))


def row_masks(rows, H, p, call_id):
    """Kept (bool [rows, H]) of the row kernels: idx = row 256 + c4, c4 the index of the float4 within the row."""
    want = np.zeros((rows, H), dtype=bool)
    for r in range(rows):
        for c4 in range(H // 4):
            want[r, 4 * c4:4 * c4 + 4] = [f != 0 for f in keep4(bits(SEED, STEP, call_id, r * 256 + c4), p)]
    return torch.from_numpy(want)


def test_norm_act_mask(rng):
    """The mask is read off the output where the undropped output is positive, as test_gpu_fused does."""
    from analysisgnn_amd import fused
    H, rows, p, call_id = 256, 5, 0.3, 77
    torch.manual_seed(13)
    ln = torch.nn.LayerNorm(H).to(DEV)
    x = torch.randn(rows, H, device=DEV)
    base = fused._NormAct.apply(x, ln.weight, ln.bias, ln.eps, 0.0, fused.POST_RELU, call_id)
    y = fused._NormAct.apply(x, ln.weight, ln.bias, ln.eps, p, fused.POST_RELU, call_id)
    live = (base > 0).cpu()
    assert int(live.sum()) > rows * H // 4
    assert torch.equal((y != 0).cpu()[live], row_masks(rows, H, p, call_id)[live])


def test_mix_mask(rng):
    """The HGT layer's epilogue (agnn_skip_act_*) draws from the same index formula."""
    from analysisgnn_amd import fused
    H, rows, p, call_id = 256, 5, 0.25, 78
    torch.manual_seed(14)
    o = torch.randn(rows, H, device=DEV)
    z = fused._SkipAct.apply(o, None, None, True, p, call_id)
    live = (o > 0).cpu()
    assert torch.equal((z != 0).cpu()[live], row_masks(rows, H, p, call_id)[live])


def test_smote_draws(rng):
    """Gap: idx = s D4 + d4, value (word >> 8) 2^-24.  Choice: idx = 2^62 + s, value umulhi(word.x, k - 1)."""
    from analysisgnn_amd import smote
    S, D, k, call_id = 37, 128, 6, 9001
    D4 = D // 4
    choice, gap = smote.draws(S, D, k, call_id, rng=rng)
    want_gap = np.zeros((S, D), dtype=np.float32)
    want_choice = np.zeros((S,), dtype=np.int32)
    for s in range(S):
        for d4 in range(D4):
            want_gap[s, 4 * d4:4 * d4 + 4] = [np.float32(w >> 8) * np.float32(2.0 ** -24) for w in bits(SEED, STEP, call_id, s * D4 + d4)]
        want_choice[s] = (bits(SEED, STEP, call_id, (1 << 62) + s)[0] * (k - 1)) >> 32
    assert torch.equal(gap.cpu(), torch.from_numpy(want_gap))
    assert torch.equal(choice.cpu(), torch.from_numpy(want_choice))
