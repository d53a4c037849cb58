// Per-head relation transforms of HGTConv (PyG >= 2.3: `k_rel` / `v_rel` = HeteroLinear with one D x D matrix per
// (edge type, head); reached through graphmuse's HybridHGT, reference analysisgnn/models/analysis.py:445-453):
//     k'[n, r, h, :] = k[n, h, :] @ A[r, h]          for every relation r leaving the node type, every head h
// Round 1 ran them as ONE dense library GEMM against a block-diagonal [H, R*H] weight: 4x the useful FLOPs at heads = 4
// (12.6 GFLOP instead of 3.1 per operand and layer at the C3 shape) plus the launches that assemble the weight.
// Here they are what they are: R*heads independent [N, D] x [D, D] products, at every head width the attention kernels
// take (D = 4, 8, 16, 32, 64, 128, 256).  Per item the work is 2 N R H D FLOP over 4 N H (1 + R) + 4 R heads D^2 bytes,
// ~D/2 FLOP per byte against a ridge of ~25 (fp32 MFMA over HBM): D <= 32 is byte-bound, D = 64 sits at the ridge,
// D >= 128 is MFMA-bound — three kernel families, not one template stretched over the range.
//
// D = 64 (v_mfma_f32_32x32x2_f32: exact fp32, 64 FLOP/clk/SIMD):
//   k_relt<false>  forward: one workgroup = 128 rows x one head; a wave keeps its 32 x 64 slice of k in registers (the A
//                  operand of all R products) and walks the relations; A[r, h] (16 KB) is staged through LDS, double
//                  buffered, once per workgroup; the 32 x 64 result of every relation is written as whole 128-byte lines.
//   k_relt<true>   input gradient: dk[n, h, :] = sum_r dk'[n, r, h, :] @ A[r, h]^T — the same loop with the roles
//                  swapped (the A operand changes per relation, ONE accumulator is carried across the relations); the
//                  caller passes the transposed blocks.
//   k_relt_dw<64>  weight gradient: dA[r, h] = k[:, h, :]^T dk'[:, r, h, :], a 64 x 64 output with the reduction over N:
//                  one wave = one (relation, head, row slice), operands straight from global memory (already "k-major":
//                  one MFMA k-step = two consecutive rows, as in wgrad.hip), slices summed in a fixed order by
//                  agnn::launch_slab_reduce (no atomics).
// D = 128, 256 (the same instruction, the same pipeline, tiled over D):
//   k_relt_wide    a D x D block no longer fits the LDS (256 KB at D = 256), so the unit of work is one 64 x 64 piece of it:
//                  k-chunk kc x column tile ct.  A workgroup owns 128 rows, one head and ONE column tile (blockIdx.x walks
//                  the column tiles fastest, so the workgroups that share rows run together) and walks (relation, k-chunk);
//                  the 16 KB pieces go through the two LDS buffers exactly as A[r, h] does at D = 64, the wave's 32 x D
//                  row slice sits in registers as D/64 chunks.  Forward: the accumulator pair restarts with every
//                  relation and is stored after its last k-chunk; input gradient: it is carried to the end, and chunk kc
//                  of the next relation's dk' is loaded right behind the MFMAs that consumed chunk kc of this one.
//   k_relt_dw<D>   the D = 64 kernel, one wave per 64 x 64 TILE of dA[r, h]: (D/64)^2 tiles per (relation, head).
// D = 16, 32 (byte-bound; one MFMA tile IS the block: v_mfma_f32_16x16x4_f32 at D = 16, v_mfma_f32_32x32x2_f32 at D = 32 —
// no zero padding, no multiplied FLOPs; the multi-block forms would only pay with several heads per wave, which the
// item layout does not give: a head's block is D columns of a row, the next head's the next D):
//   k_relt_tile    one wave = D rows x one head (D/4 inputs of its row per lane: 16-byte loads), all relations' blocks of
//                  the head staged in LDS in passes of 8; D/(64/D) MFMAs per relation; input gradient with the next
//                  relation's operand loaded ahead.
//   k_relt_dw_tile one wave = one (relation, head, row slice), one accumulator tile, three register stages of loads.
// D = 4, 8 (a block is 64 or 256 bytes: plain VALU FMAs; even the smallest MFMA tile would be mostly zeros):
//   k_relt_valu    one thread = one output element; its D inputs in registers, the blocks of a pass of relations in LDS
//                  (consecutive lanes read consecutive words), D FMAs, consecutive lanes store consecutive words.
//   k_relt_dw_valu one thread = one ROW of a block gradient (D accumulators) over a row slice, rows in groups of 8 loads.
// Weight gradient slices (relt_dw_plan): S = min(S_max, ceil(N / rows_min)) row slices, rows per slice rounded up to a
// multiple of 4 (of 2 at D = 64, as ever), with (rows_min, S_max) = (64, 256) at D <= 8, (256, 64) at D = 16 / 32, (512, 32) at D = 64, (512, 8) at
// D = 128, (512, 2) at D = 256 (the slab of one slice grows with D^2, the tiles per (relation, head) with (D/64)^2).
// Workspace = n_items * S * n_rel * heads * D * D * 4 + 256 bytes (agnn_relt_dw_workspace_bytes is the authority).
// K and V (and anything else that shares the shape) go through ONE launch: up to 4 items per call.
#include "agnn_common.h"

namespace {

using agnn::f32x16;
using agnn::f32x4;

constexpr int kD = 64;

struct ReltItem {
  const float* x;     // fwd: [n, heads*D] (ld_x);  bwd: dy [n, n_rel*heads*D] (ld_x);  dw: x [n, heads*D]
  const float* w;     // fwd: A blocks [n_rel*heads][D][D];  bwd: the transposed blocks;  dw: dy [n, n_rel*heads*D] (ld_y)
  float* y;           // fwd: [n, n_rel*heads*D] (ld_y);  bwd: dx [n, heads*D] (ld_y);  dw: unused
  int64_t ld_x, ld_y;
};

struct ReltArgs {
  ReltItem it[AGNN_RELT_MAX_ITEMS];
  int32_t n_rel, heads;
  int64_t n_rows;
  // dw only
  float* slab;              // [items][S][n_rel*heads*D][D]
  int32_t S, rows_per_slice;
};

// ---------------------------------------------------------------------------------------------------------------------
// Stages shared by the MFMA kernels.  What each one had to learn is written here, once; the kernels bind a stage to their
// operands with a one-line lambda and otherwise only name it.

// C/D layout of both MFMAs (T = 32: v_mfma_f32_32x32x2_f32, 16 registers; T = 16: v_mfma_f32_16x16x4_f32, 4 registers):
// lane l, register q -> row (q&3) + 4*(64/T)*(q>>2) + 4*(l/T), column l % T.  `kk` = l / T; `base` (a first row, or 0) is added
// in its own type, first.  (T = 32 without a base is agnn::d_row32; this one stays: profiles/relt_isa_identity.md.)
template <int T, class B>
__device__ __forceinline__ constexpr B cd_row(B base, int q, int kk) { return base + (q & 3) + 4 * (64 / T) * (q >> 2) + 4 * kk; }

// 64 x 64 weights on their way global -> registers -> LDS, 4 x 16 bytes per thread (`src`: the thread's first 16 bytes, the
// others `stride` float4s apart; in LDS thread tid owns float4 tid + 256 j).  The registers are four NAMED float4s passed by
// reference, not an array: an array captured by the kernels' lambdas stayed in scratch memory (`scratch_store` right behind
// the loads, i.e. an s_waitcnt on them and on every store issued before them).
__device__ __forceinline__ void fetch_w(const float4* src, int stride, float4& w0, float4& w1, float4& w2, float4& w3) {
  w0 = src[0];
  w1 = src[stride];
  w2 = src[2 * stride];
  w3 = src[3 * stride];
}
__device__ __forceinline__ void put_w(float* buf, int tid, const float4& w0, const float4& w1, const float4& w2, const float4& w3) {
  float4* dst = reinterpret_cast<float4*>(buf) + tid;
  dst[0] = w0;
  dst[256] = w1;
  dst[512] = w2;
  dst[768] = w3;
}

// A operand of 64 MFMA k-steps: lane (row c32, half kk) holds the 32 consecutive inputs k = kk*32 .. kk*32 + 31 of its row
// (the k order inside a product is free as long as the B operand uses the same one): eight 16-byte loads from `src`.
// Where the operand is loop-invariant the kernel waits for it (wait_a) OUTSIDE the relation loop: left to the first MFMA
// that uses it, the compiler puts an `s_waitcnt vmcnt(8)` at the top of EVERY iteration (it cannot see that a previous
// iteration already waited), which also waits for the previous relation's 32 stores — one HBM write latency per relation,
// the MFMA pipe idle meanwhile.
__device__ __forceinline__ void load_a(float4 (&dst)[8], const float* src) {
#pragma unroll
  for (int u = 0; u < 8; ++u) dst[u] = reinterpret_cast<const float4*>(src)[u];
}
__device__ __forceinline__ void wait_a(float4 q) { asm volatile("" ::"v"(q.x), "v"(q.y), "v"(q.z), "v"(q.w)); }

// The 64 MFMAs of one 32 x 64 x 64 product.  The B operand B[k = kk*32 + s][j = c32 (+32)] comes from LDS (`sw` = the lane's
// B[kk*32][c32], rows LD floats apart) in chunks of 8 k-steps, the next chunk's 16 reads issued BEFORE the 16 MFMAs of the
// current one (left to the compiler, every k-step was `ds_read2 -> s_waitcnt lgkmcnt(0) -> 2 MFMAs` through one register
// pair: the LDS latency of every read exposed).
template <int LD>
__device__ __forceinline__ void product(const float4 (&av)[8], const float* sw, f32x16& acc0, f32x16& acc1) {
  float b0[2][8], b1[2][8];
  auto rd = [&](int c, int slot) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      b0[slot][u] = sw[(8 * c + u) * LD];
      b1[slot][u] = sw[(8 * c + u) * LD + 32];
    }
  };
  rd(0, 0);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c + 1 < 4) rd(c + 1, (c + 1) & 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float4 q = av[2 * c + (u >> 2)];
      const float as = (u & 3) == 0 ? q.x : (u & 3) == 1 ? q.y : (u & 3) == 2 ? q.z : q.w;
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(as, b0[c & 1][u], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(as, b1[c & 1][u], acc1, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The 32 x 64 accumulator pair of a wave (rows row0 .. row0 + 31) -> global memory.  `o` = the lane's (row row0 + 4*kk,
// column c32) of the output piece, rows `*ld` floats apart; `full` (wave-uniform): all 32 rows exist (the usual case).
// `ld` and `n_rows` point INTO the kernel arguments and are read at every use: taken by value or by reference the compiler
// reads them once up front, a different schedule from the one these kernels were measured with.
__device__ __forceinline__ void store_pair(const f32x16& acc0, const f32x16& acc1, float* o, const int64_t* ld, bool full,
                                           int64_t row0, int kk, const int64_t* n_rows) {
  if (full) {                                            // straight-line: 32 stores, no per-row branch
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float* oq = o + cd_row<32>(0, q, 0) * *ld;
      oq[0] = acc0[q];
      oq[32] = acc1[q];
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (cd_row<32>(row0, q, kk) < *n_rows) {
        float* oq = o + cd_row<32>(0, q, 0) * *ld;
        oq[0] = acc0[q];
        oq[32] = acc1[q];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Stages shared by the weight-gradient kernels.

// the D x D block (relation, head) = rh of (item, slice) in the slab [items][S][n_rel*heads*D][D]
template <int D>
__device__ __forceinline__ float* dw_slab(const ReltArgs& p, int item, int slice, int rh) {
  const int groups = p.n_rel * p.heads;
  return p.slab + ((static_cast<size_t>(item) * p.S + slice) * groups + rh) * D * D;
}

template <bool BWD>
__global__ __launch_bounds__(256) void k_relt(ReltArgs p) {
  constexpr int D = kD;
  __shared__ __attribute__((aligned(16))) float sW[2][D * D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c32 = lane & 31, kk = lane >> 5;
  const int h = blockIdx.y % p.heads, item = blockIdx.y / p.heads;
  const ReltItem& I = p.it[item];
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * 128 + wave * 32;
  int64_t rowc = row0 + c32;
  if (rowc > p.n_rows - 1) rowc = p.n_rows - 1;

  // the shared stages (above), bound to this kernel's operands
  float4 w0 = agnn::f4_zero(), w1 = w0, w2 = w0, w3 = w0;    // the next relation's weights
  auto fetch = [&](int r) { fetch_w(reinterpret_cast<const float4*>(I.w + static_cast<size_t>(r * p.heads + h) * D * D) + tid, 256, w0, w1, w2, w3); };
  auto put = [&](int buf) { put_w(sW[buf], tid, w0, w1, w2, w3); };
  const float* xrow = I.x + rowc * I.ld_x + kk * 32;
  auto load = [&](float4 (&dst)[8], int colbase) { load_a(dst, xrow + colbase); };
  const bool full = row0 + 32 <= p.n_rows;               // wave-uniform: all 32 rows of this wave exist (the usual case)
  float* const ybase = I.y + (row0 + 4 * kk) * I.ld_y + c32;
  auto store = [&](const f32x16& acc0, const f32x16& acc1, int colbase) { store_pair(acc0, acc1, ybase + colbase, &I.ld_y, full, row0, kk, &p.n_rows); };
  auto prod = [&](const float4 (&av)[8], int buf, f32x16& acc0, f32x16& acc1) { product<D>(av, sW[buf] + kk * 32 * D + c32, acc0, acc1); };

  fetch(0);
  put(0);
  float4 aA[8], aB[8];                                   // BWD: the A operand of relation r and of relation r + 1 (prefetched)
  load(aA, h * D);                                       // BWD: relation 0's block is (0*heads + h)*D = h*D as well
#pragma unroll
  for (int u = 0; u < 8; ++u) wait_a(aA[u]);             // FWD: loop-invariant (see load_a)
  f32x16 acc0 = {0}, acc1 = {0};
  __syncthreads();
  // one relation: [prefetch the next weights (global -> registers) and, for the input gradient, the next A operand]
  // -> 64 MFMAs -> [store] -> [weights registers -> the other LDS buffer] -> barrier
  auto relation = [&](int r, const float4 (&cur)[8], float4 (&nxt)[8]) {
    if (r + 1 < p.n_rel) {
      fetch(r + 1);
      if (BWD) load(nxt, ((r + 1) * p.heads + h) * D);
    }
    if (!BWD) {
      acc0 = f32x16{0};
      acc1 = f32x16{0};
    }
    prod(cur, r & 1, acc0, acc1);
    if (!BWD) store(acc0, acc1, (r * p.heads + h) * D);
    if (r + 1 < p.n_rel) put((r + 1) & 1);               // that buffer was last read in iteration r - 1 (barrier below)
    __syncthreads();
  };
  if (BWD) {
    for (int r = 0; r < p.n_rel; r += 2) {
      relation(r, aA, aB);
      if (r + 1 < p.n_rel) relation(r + 1, aB, aA);
    }
    store(acc0, acc1, h * D);
  } else {
    for (int r = 0; r < p.n_rel; ++r) relation(r, aA, aB);
  }
}

// dA[r, h][i][j] = sum_n x[n, h*D + i] * dy[n, (r*heads + h)*D + j].  One workgroup = (item, relation, row slice), one
// wave per head (the waves of a workgroup read ADJACENT 256-byte pieces of the same rows: whole 1 KiB row segments of x
// and of dy per workgroup); a wave's 64 x 64 output is four 32 x 32 accumulators; a lane loads TWO adjacent columns of
// both operands per row (8 bytes: columns 2*c32, 2*c32 + 1 feed the two tiles of that operand), the lane halves take the
// two rows of a k-step.  Three register stages in rotation (two chunks of loads in flight), as in wgrad.hip.
// D = 128, 256: a wave takes one 64 x 64 tile (ti, tj) of the D x D output, the four waves of a workgroup four consecutive
// (head, tile) jobs: at D = 128 the four tiles of one head, which share their two x and two dy pieces.
template <int D>
__global__ __launch_bounds__(256) void k_relt_dw(ReltArgs p) {
  constexpr int NT = D / 64;
  const int lane = threadIdx.x & 63, job = blockIdx.z * 4 + (threadIdx.x >> 6);    // up to four (head, tile) jobs per workgroup
  const int h = job / (NT * NT), ti = (job / NT) % NT, tj = job % NT;
  if (h >= p.heads) return;
  const int c32 = lane & 31, kk = lane >> 5;
  const int item = blockIdx.x / p.n_rel, r = blockIdx.x - item * p.n_rel;
  const int rh = r * p.heads + h;
  const ReltItem& I = p.it[item];
  const int slice = blockIdx.y;
  const int64_t r0 = static_cast<int64_t>(slice) * p.rows_per_slice;
  int64_t r1 = r0 + p.rows_per_slice;
  if (r1 > p.n_rows) r1 = p.n_rows;
  f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
  if (r0 < r1) {
    const float* xs = I.x + h * D + ti * 64 + 2 * c32;    // operand "A": rows of the 64 x 64 output = input feature i
    const float* ys = I.w + rh * D + tj * 64 + 2 * c32;   // operand "B": columns = output feature j
    constexpr int CH = 8;
    constexpr int STEP = 2 * CH;
    float2 a0[CH], b0[CH], a1[CH], b1[CH], a2[CH], b2[CH];
    auto fetch = [&](int64_t base, float2* ao, float2* bo) {
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        int64_t row = base + 2 * u + kk;
        if (row > p.n_rows - 1) row = p.n_rows - 1;
        ao[u] = *reinterpret_cast<const float2*>(xs + row * I.ld_x);
        bo[u] = *reinterpret_cast<const float2*>(ys + row * I.ld_y);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    auto mma = [&](const float2* ao, const float2* bo) {
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(ao[u].x, bo[u].x, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(ao[u].x, bo[u].y, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(ao[u].y, bo[u].x, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(ao[u].y, bo[u].y, acc11, 0, 0, 0);
      }
    };
    auto mma_tail = [&](int64_t base, const float2* ao, const float2* bo) {      // rows >= r1 contribute nothing
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const float m = (base + 2 * u + kk < r1) ? 1.f : 0.f;
        const float ax = ao[u].x * m, ay = ao[u].y * m;
        acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(ax, bo[u].x, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(ax, bo[u].y, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, bo[u].x, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, bo[u].y, acc11, 0, 0, 0);
      }
    };
    const int64_t nfull = (r1 - r0) / STEP, nchunks = (r1 - r0 + STEP - 1) / STEP;
    fetch(r0, a0, b0);
    fetch(r0 + STEP, a1, b1);
    int64_t c = 0;
    for (; c + 3 <= nfull; c += 3) {
      fetch(r0 + (c + 2) * STEP, a2, b2);
      mma(a0, b0);
      fetch(r0 + (c + 3) * STEP, a0, b0);
      mma(a1, b1);
      fetch(r0 + (c + 4) * STEP, a1, b1);
      mma(a2, b2);
    }
    fetch(r0 + (c + 2) * STEP, a2, b2);
    if (c < nchunks) mma_tail(r0 + c * STEP, a0, b0);
    if (c + 1 < nchunks) mma_tail(r0 + (c + 1) * STEP, a1, b1);
    if (c + 2 < nchunks) mma_tail(r0 + (c + 2) * STEP, a2, b2);
  }
  // accXY: rows = input features 2*i + X, columns = output features 2*j + Y (the stride-2 split of the float2 loads)
  float* slab = dw_slab<D>(p, item, slice, rh);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = cd_row<32>(0, q, kk);
    float* o = slab + (ti * 64 + 2 * i) * D + tj * 64 + 2 * c32;
    *reinterpret_cast<float2*>(o) = make_float2(acc00[q], acc01[q]);
    *reinterpret_cast<float2*>(o + D) = make_float2(acc10[q], acc11[q]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// D = 128, 256: forward and input gradient.  Everything inside a unit (one 64 x 64 piece of the block: rows kc*64 .. of it,
// columns ct*64 ..) is k_relt's relation, built from the same shared stages.  NC = D/64 is even, so the LDS buffer of unit
// (r, kc) is kc & 1 and the k-chunk loop unrolls with every register array indexed by a constant.
template <int D, bool BWD>
__global__ __launch_bounds__(256) void k_relt_wide(ReltArgs p) {
  constexpr int NC = D / 64;
  static_assert(NC >= 2 && NC % 2 == 0, "the LDS buffer parity relies on an even chunk count");
  __shared__ __attribute__((aligned(16))) float sW[2][64 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c32 = lane & 31, kk = lane >> 5;
  const int ct = blockIdx.x % NC;
  const int h = blockIdx.y % p.heads, item = blockIdx.y / p.heads;
  const ReltItem& I = p.it[item];
  const int64_t row0 = static_cast<int64_t>(blockIdx.x / NC) * 128 + wave * 32;
  int64_t rowc = row0 + c32;
  if (rowc > p.n_rows - 1) rowc = p.n_rows - 1;

  float4 w0 = agnn::f4_zero(), w1 = w0, w2 = w0, w3 = w0;
  const float* const wsrc = I.w + (tid >> 4) * D + ct * 64 + (tid & 15) * 4;      // this thread's 16 bytes of rows tid/16 + 16 j
  auto fetch = [&](int r, int kc) {
    fetch_w(reinterpret_cast<const float4*>(wsrc + (static_cast<size_t>(r * p.heads + h) * D + kc * 64) * D), 4 * D, w0, w1, w2, w3);
  };
  auto put = [&](int buf) { put_w(sW[buf], tid, w0, w1, w2, w3); };
  const float* xrow = I.x + rowc * I.ld_x + kk * 32;
  auto load = [&](float4 (&dst)[8], int colbase) { load_a(dst, xrow + colbase); };
  const bool full = row0 + 32 <= p.n_rows;
  float* const ybase = I.y + (row0 + 4 * kk) * I.ld_y + c32;
  auto store = [&](const f32x16& acc0, const f32x16& acc1, int colbase) { store_pair(acc0, acc1, ybase + colbase, &I.ld_y, full, row0, kk, &p.n_rows); };
  auto prod = [&](const float4 (&av)[8], int buf, f32x16& acc0, f32x16& acc1) { product<64>(av, sW[buf] + kk * 32 * 64 + c32, acc0, acc1); };

  fetch(0, 0);
  put(0);
  float4 a[NC][8];                                       // the wave's 32 x D row slice (BWD: of the current relation's dy block)
#pragma unroll
  for (int kc = 0; kc < NC; ++kc) load(a[kc], h * D + kc * 64);
  if (!BWD) {                                            // loop-invariant only in the forward
#pragma unroll
    for (int kc = 0; kc < NC; ++kc)
#pragma unroll
      for (int u = 0; u < 8; ++u) wait_a(a[kc][u]);
  }
  f32x16 acc0 = {0}, acc1 = {0};
  __syncthreads();
  for (int r = 0; r < p.n_rel; ++r) {
    const bool more = r + 1 < p.n_rel;
#pragma unroll
    for (int kc = 0; kc < NC; ++kc) {
      constexpr int kLast = NC - 1;
      if (kc < kLast) fetch(r, kc + 1);
      else if (more) fetch(r + 1, 0);
      if (!BWD && kc == 0) {
        acc0 = f32x16{0};
        acc1 = f32x16{0};
      }
      prod(a[kc], kc & 1, acc0, acc1);
      if (BWD && more) load(a[kc], ((r + 1) * p.heads + h) * D + kc * 64);
      if (!BWD && kc == kLast) store(acc0, acc1, (r * p.heads + h) * D + ct * 64);
      if (kc < kLast || more) put((kc + 1) & 1);         // that buffer was last read in the previous unit (barrier below)
      __syncthreads();
    }
  }
  if (BWD) store(acc0, acc1, h * D + ct * 64);
}

// ---------------------------------------------------------------------------------------------------------------------
// D = 16, 32: the block is one MFMA tile.  T = D; 64/T lane groups share a tile row, each holds T/(64/T) consecutive
// inputs of its row (the k order inside a product is free as long as both operands use the same one).
template <int T> struct TileMfma;
template <> struct TileMfma<32> {
  typedef f32x16 acc_t;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};
template <> struct TileMfma<16> {
  typedef f32x4 acc_t;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};

template <int T, bool BWD>
__global__ __launch_bounds__(256) void k_relt_tile(ReltArgs p) {
  constexpr int KL = 64 / T;                             // lane groups = inputs per MFMA step (2 / 4)
  constexpr int KS = T / KL;                             // MFMA steps per product = inputs per lane (16 / 4)
  constexpr int NQ = T * T / 64;                         // accumulator registers (16 / 4)
  constexpr int RC = 8;                                  // relations staged per pass
  typedef typename TileMfma<T>::acc_t acc_t;
  __shared__ __attribute__((aligned(16))) float sW[RC * T * T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane % T, kk = lane / T;
  const int h = blockIdx.y % p.heads, item = blockIdx.y / p.heads;
  const ReltItem& I = p.it[item];
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * (4 * T) + wave * T;
  int64_t rowc = row0 + c;
  if (rowc > p.n_rows - 1) rowc = p.n_rows - 1;
  const float* xrow = I.x + rowc * I.ld_x + kk * KS;
  auto load_a = [&](float4 (&dst)[KS / 4], int colbase) {
    const float4* src = reinterpret_cast<const float4*>(xrow + colbase);
#pragma unroll
    for (int u = 0; u < KS / 4; ++u) dst[u] = src[u];
  };
  float* const ybase = I.y + (row0 + 4 * kk) * I.ld_y + c;
  auto store = [&](const acc_t& acc, int colbase) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int rq = cd_row<T>(0, q, 0);
      if (row0 + rq + 4 * kk < p.n_rows) ybase[rq * I.ld_y + colbase] = acc[q];
    }
  };
  float4 cur[KS / 4], nxt[KS / 4];
  load_a(cur, h * T);                                    // BWD: relation 0's block is (0*heads + h)*T = h*T as well
  acc_t acc = {0};
  for (int r0 = 0; r0 < p.n_rel; r0 += RC) {
    const int nr = p.n_rel - r0 < RC ? p.n_rel - r0 : RC;
    __syncthreads();                                     // the previous pass has been read
    for (int rr = 0; rr < nr; ++rr) {
      const float4* src = reinterpret_cast<const float4*>(I.w + static_cast<size_t>((r0 + rr) * p.heads + h) * T * T);
      float4* dst = reinterpret_cast<float4*>(sW + rr * T * T);
      for (int i = tid; i < T * T / 4; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    for (int rr = 0; rr < nr; ++rr) {
      const int r = r0 + rr;
      if (BWD && r + 1 < p.n_rel) load_a(nxt, ((r + 1) * p.heads + h) * T);
      if (!BWD) acc = acc_t{0};
      const float* sw = sW + rr * T * T + kk * KS * T + c;
#pragma unroll
      for (int u = 0; u < KS; ++u) {
        const float4 q = cur[u >> 2];
        const float as = (u & 3) == 0 ? q.x : (u & 3) == 1 ? q.y : (u & 3) == 2 ? q.z : q.w;
        acc = TileMfma<T>::mma(as, sw[u * T], acc);
      }
      if (!BWD) store(acc, (r * p.heads + h) * T);
      if (BWD && r + 1 < p.n_rel) {
#pragma unroll
        for (int u = 0; u < KS / 4; ++u) cur[u] = nxt[u];
      }
    }
  }
  if (BWD) store(acc, h * T);
}

// dA[r, h] (T x T) = x[:, h, :]^T dy[:, r, h, :]: one wave = (item, relation, row slice, head), the heads of a workgroup read
// adjacent pieces of the same rows; one MFMA k-step = 64/T consecutive rows; three register stages in rotation as in k_relt_dw.
template <int T>
__global__ __launch_bounds__(256) void k_relt_dw_tile(ReltArgs p) {
  constexpr int KL = 64 / T, NQ = T * T / 64;
  typedef typename TileMfma<T>::acc_t acc_t;
  const int lane = threadIdx.x & 63, h = blockIdx.z * 4 + (threadIdx.x >> 6);
  if (h >= p.heads) return;
  const int c = lane % T, kk = lane / T;
  const int item = blockIdx.x / p.n_rel, r = blockIdx.x - item * p.n_rel;
  const int rh = r * p.heads + h;
  const ReltItem& I = p.it[item];
  const int slice = blockIdx.y;
  const int64_t r0 = static_cast<int64_t>(slice) * p.rows_per_slice;
  int64_t r1 = r0 + p.rows_per_slice;
  if (r1 > p.n_rows) r1 = p.n_rows;
  acc_t acc = {0};
  if (r0 < r1) {
    const float* xs = I.x + h * T + c;
    const float* ys = I.w + rh * T + c;
    constexpr int CH = 8;
    constexpr int STEP = KL * CH;
    float a0[CH], b0[CH], a1[CH], b1[CH], a2[CH], b2[CH];
    auto fetch = [&](int64_t base, float* ao, float* bo) {
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        int64_t row = base + KL * u + kk;
        if (row > p.n_rows - 1) row = p.n_rows - 1;
        ao[u] = xs[row * I.ld_x];
        bo[u] = ys[row * I.ld_y];
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    auto mma = [&](const float* ao, const float* bo) {
#pragma unroll
      for (int u = 0; u < CH; ++u) acc = TileMfma<T>::mma(ao[u], bo[u], acc);
    };
    auto mma_tail = [&](int64_t base, const float* ao, const float* bo) {       // rows >= r1 contribute nothing
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const float m = (base + KL * u + kk < r1) ? 1.f : 0.f;
        acc = TileMfma<T>::mma(ao[u] * m, bo[u], acc);
      }
    };
    const int64_t nfull = (r1 - r0) / STEP, nchunks = (r1 - r0 + STEP - 1) / STEP;
    fetch(r0, a0, b0);
    fetch(r0 + STEP, a1, b1);
    int64_t ch = 0;
    for (; ch + 3 <= nfull; ch += 3) {
      fetch(r0 + (ch + 2) * STEP, a2, b2);
      mma(a0, b0);
      fetch(r0 + (ch + 3) * STEP, a0, b0);
      mma(a1, b1);
      fetch(r0 + (ch + 4) * STEP, a1, b1);
      mma(a2, b2);
    }
    fetch(r0 + (ch + 2) * STEP, a2, b2);
    if (ch < nchunks) mma_tail(r0 + ch * STEP, a0, b0);
    if (ch + 1 < nchunks) mma_tail(r0 + (ch + 1) * STEP, a1, b1);
    if (ch + 2 < nchunks) mma_tail(r0 + (ch + 2) * STEP, a2, b2);
  }
  float* slab = dw_slab<T>(p, item, slice, rh);
#pragma unroll
  for (int q = 0; q < NQ; ++q) slab[cd_row<T>(0, q, kk) * T + c] = acc[q];
}

// ---------------------------------------------------------------------------------------------------------------------
// D = 4, 8: VALU.  The blocks of `valu_pass(...)` relations at a time in LDS (at most 32 KB; heads * D * D <= 4096 floats).
__host__ __device__ inline int valu_pass(int n_rel, int heads, int D) {
  int rc = 8192 / (heads * D * D);
  if (rc > n_rel) rc = n_rel;
  return rc < 1 ? 1 : rc;
}

template <int D, bool BWD>
__global__ __launch_bounds__(256) void k_relt_valu(ReltArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sWv[];       // [pass][heads][D][D]
  const int tid = threadIdx.x;
  const ReltItem& I = p.it[blockIdx.y];
  const int H = p.heads * D, per_rel = H * D;
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * 256 + tid;  // one output element of an [n, H] slab: (row, head, j)
  const int64_t row = gid / H;
  const int col = static_cast<int>(gid - row * H), h = col / D, j = col % D;
  const bool live = row < p.n_rows;
  const float* xrow = I.x + (live ? row : p.n_rows - 1) * I.ld_x;
  float xv[D];
  auto load_x = [&](int colbase) {
#pragma unroll
    for (int u = 0; u < D / 4; ++u) {
      const float4 q = reinterpret_cast<const float4*>(xrow + colbase)[u];
      xv[4 * u] = q.x;
      xv[4 * u + 1] = q.y;
      xv[4 * u + 2] = q.z;
      xv[4 * u + 3] = q.w;
    }
  };
  if (!BWD) load_x(h * D);
  const int rc = valu_pass(p.n_rel, p.heads, D);
  float acc = 0.f;
  for (int r0 = 0; r0 < p.n_rel; r0 += rc) {
    const int nr = p.n_rel - r0 < rc ? p.n_rel - r0 : rc;
    __syncthreads();                                     // the previous pass has been read
    const float4* src = reinterpret_cast<const float4*>(I.w + static_cast<size_t>(r0) * per_rel);
    for (int i = tid; i < nr * per_rel / 4; i += 256) reinterpret_cast<float4*>(sWv)[i] = src[i];
    __syncthreads();
    for (int rr = 0; rr < nr; ++rr) {
      const int blk = ((r0 + rr) * p.heads + h) * D;
      const float* wb = sWv + (rr * p.heads + h) * D * D + j;
      if (BWD) load_x(blk);
      else acc = 0.f;
#pragma unroll
      for (int i = 0; i < D; ++i) acc = fmaf(xv[i], wb[i * D], acc);
      if (!BWD && live) I.y[row * I.ld_y + blk + j] = acc;
    }
  }
  if (BWD && live) I.y[row * I.ld_y + col] = acc;
}

// thread (rh, i): row i of dA[r, h] = sum over the slice's rows of x[n, h*D + i] * dy[n, rh*D .. +D], rows in their order.
template <int D>
__global__ __launch_bounds__(256) void k_relt_dw_valu(ReltArgs p) {
  const int groups = p.n_rel * p.heads;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= groups * D) return;
  const int rh = t / D, i = t % D, h = rh % p.heads;
  const int item = blockIdx.z, slice = blockIdx.y;
  const ReltItem& I = p.it[item];
  const int64_t r0 = static_cast<int64_t>(slice) * p.rows_per_slice;
  int64_t r1 = r0 + p.rows_per_slice;
  if (r1 > p.n_rows) r1 = p.n_rows;
  const float* xs = I.x + h * D + i;
  const float* ys = I.w + rh * D;
  float acc[D];
#pragma unroll
  for (int j = 0; j < D; ++j) acc[j] = 0.f;
  constexpr int U = 8;
  for (int64_t n = r0; n < r1; n += U) {
    float xv[U];
    float2 yv[U][D / 2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = n + u < r1 ? n + u : r1 - 1;
      xv[u] = n + u < r1 ? xs[row * I.ld_x] : 0.f;
#pragma unroll
      for (int j = 0; j < D / 2; ++j) yv[u][j] = reinterpret_cast<const float2*>(ys + row * I.ld_y)[j];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < D / 2; ++j) {
        acc[2 * j] = fmaf(xv[u], yv[u][j].x, acc[2 * j]);
        acc[2 * j + 1] = fmaf(xv[u], yv[u][j].y, acc[2 * j + 1]);
      }
  }
  float* o = dw_slab<D>(p, item, slice, rh) + i * D;
#pragma unroll
  for (int j = 0; j < D / 2; ++j) reinterpret_cast<float2*>(o)[j] = make_float2(acc[2 * j], acc[2 * j + 1]);
}

constexpr int kWidths[] = {4, 8, 16, 32, 64, 128, 256};   // = check_shape's head widths in hgt.hip

int relt_check(const char* who, int n_items, const agnn_relt_item_t* items, int n_rel, int heads, int D, int64_t n_rows) {
  using namespace agnn;
  if (n_items <= 0 || n_items > AGNN_RELT_MAX_ITEMS || !items) return fail(AGNN_EINVAL, "%s: n_items=%d not in [1,%d]", who, n_items, AGNN_RELT_MAX_ITEMS);
  bool known = false;
  char widths[64];
  int len = 0;
  for (int w : kWidths) {
    known |= (D == w);
    len += snprintf(widths + len, sizeof(widths) - len, len ? ", %d" : "%d", w);
  }
  if (!known) return fail(AGNN_EINVAL, "%s: D=%d (the head width must be one of %s)", who, D, widths);
  if (n_rel <= 0 || n_rel > 64 || heads <= 0 || heads > 64) return fail(AGNN_EINVAL, "%s: n_rel=%d heads=%d", who, n_rel, heads);
  if (n_rows < 0 || n_rows >= (int64_t{1} << 31)) return fail(AGNN_EINVAL, "%s: n_rows=%lld", who, (long long)n_rows);
  return AGNN_OK;
}

// The per-item checks and the ReltArgs fill of the three entry points (after relt_check).  x and w must be `align` bytes
// aligned and ld_x a multiple of align/4 floats (16 and 4: the float4 loads of forward / input gradient; 8 and 2: the float2
// loads of the weight gradient), and so must ld_y where w is read by rows through it (`w_by_rows`: the weight gradient's dy).
// `rule` is the EALIGN message's account of all that.
int relt_fill(const char* who, int n_items, const agnn_relt_item_t* items, int n_rel, int heads, int64_t n_rows, unsigned align,
              bool w_by_rows, int64_t min_ld_x, int64_t min_ld_y, const char* rule, ReltArgs& p) {
  using namespace agnn;
  p.n_rel = n_rel; p.heads = heads; p.n_rows = n_rows;
  const int64_t ld_mask = align / 4 - 1;
  for (int i = 0; i < n_items; ++i) {
    const agnn_relt_item_t& t = items[i];
    if (!t.x || !t.w || !t.y) return fail(AGNN_EINVAL, "%s: item %d has a null pointer", who, i);
    if ((reinterpret_cast<uintptr_t>(t.x) & (align - 1)) || (reinterpret_cast<uintptr_t>(t.w) & (align - 1)) || (t.ld_x & ld_mask) ||
        (w_by_rows && (t.ld_y & ld_mask)) || t.ld_x < min_ld_x || t.ld_y < min_ld_y)
      return fail(AGNN_EALIGN, "%s: item %d: %s", who, i, rule);
    p.it[i] = ReltItem{t.x, t.w, t.y, t.ld_x, t.ld_y};
  }
  return AGNN_OK;
}

// forward (BWD = false) / input gradient (BWD = true): the kernel family of the head width
template <bool BWD>
int relt_launch(const char* who, const ReltArgs& p, int n_items, int D, hipStream_t s) {
  using namespace agnn;
  const int64_t n = p.n_rows;
  const unsigned gy = static_cast<unsigned>(p.heads * n_items);
  switch (D) {
    case 4:
    case 8: {
      const int64_t blocks = (n * p.heads * D + 255) / 256;
      if (blocks >= (int64_t{1} << 31)) return fail(AGNN_EINVAL, "%s: n_rows=%lld is too many at D=%d", who, (long long)n, D);
      const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(n_items));
      const size_t lds = static_cast<size_t>(valu_pass(p.n_rel, p.heads, D)) * p.heads * D * D * sizeof(float);
      if (D == 4) hipLaunchKernelGGL((k_relt_valu<4, BWD>), grid, dim3(256), lds, s, p);
      else hipLaunchKernelGGL((k_relt_valu<8, BWD>), grid, dim3(256), lds, s, p);
      break;
    }
    case 16: hipLaunchKernelGGL((k_relt_tile<16, BWD>), dim3(static_cast<unsigned>((n + 63) / 64), gy), dim3(256), 0, s, p); break;
    case 32: hipLaunchKernelGGL((k_relt_tile<32, BWD>), dim3(static_cast<unsigned>((n + 127) / 128), gy), dim3(256), 0, s, p); break;
    case 64: hipLaunchKernelGGL(k_relt<BWD>, dim3(static_cast<unsigned>((n + 127) / 128), gy), dim3(256), 0, s, p); break;
    case 128: hipLaunchKernelGGL((k_relt_wide<128, BWD>), dim3(static_cast<unsigned>((n + 127) / 128 * 2), gy), dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL((k_relt_wide<256, BWD>), dim3(static_cast<unsigned>((n + 127) / 128 * 4), gy), dim3(256), 0, s, p); break;
  }
  return check_launch(who);
}

// agnn_relt_fwd_f32 (x [n, H], y [n, n_rel*H]) and agnn_relt_bwd_f32 (x = dy [n, n_rel*H], w = the transposed blocks, y = dx [n, H])
template <bool BWD>
int relt_run(int n_items, const agnn_relt_item_t* items, int n_rel, int heads, int D, int64_t n_rows, agnn_stream_t stream_) {
  const char* who = BWD ? "relt_bwd" : "relt_fwd";
  if (int rc = relt_check(who, n_items, items, n_rel, heads, D, n_rows)) return rc;
  if (n_rows == 0) return AGNN_OK;
  const int64_t H = static_cast<int64_t>(heads) * D;
  ReltArgs p{};
  const char* rule = BWD ? "dy / wt must be 16-byte aligned, ld_dy % 4 == 0, ld_dy >= n_rel*heads*D, ld_dx >= heads*D"
                         : "x / w must be 16-byte aligned, ld_x % 4 == 0, ld_x >= heads*D, ld_y >= n_rel*heads*D";
  if (int rc = relt_fill(who, n_items, items, n_rel, heads, n_rows, 16, false, BWD ? H * n_rel : H, BWD ? H : H * n_rel, rule, p)) return rc;
  return relt_launch<BWD>(who, p, n_items, D, static_cast<hipStream_t>(stream_));
}

}  // namespace

extern "C" int agnn_relt_fwd_f32(int n_items, const agnn_relt_item_t* items, int32_t n_rel, int32_t heads, int32_t D, int64_t n_rows,
                                 agnn_stream_t stream_) {
  return relt_run<false>(n_items, items, n_rel, heads, D, n_rows, stream_);
}

extern "C" int agnn_relt_bwd_f32(int n_items, const agnn_relt_item_t* items, int32_t n_rel, int32_t heads, int32_t D, int64_t n_rows,
                                 agnn_stream_t stream_) {
  return relt_run<true>(n_items, items, n_rel, heads, D, n_rows, stream_);
}

namespace {
struct DwPlan { int S; int rows_per_slice; };
DwPlan relt_dw_plan(int64_t n_rows, int D) {
  // up to s_max row slices of at least ~rows_min rows.  D = 64: 32 slices of >= 512 rows, an even number of rows per slice
  // (unchanged: the slice plan fixes the order of the sum, i.e. the bits of the result).  The slab of one slice grows with
  // D^2 and the tiles per (relation, head) with (D/64)^2, so the wide blocks take fewer slices for the same number of waves;
  // the narrow ones have tiny slabs and little work per row, so they take more and shorter slices.
  const int rows_min = D <= 8 ? 64 : D <= 32 ? 256 : 512;
  const int s_max = D <= 8 ? 256 : D <= 32 ? 64 : D == 64 ? 32 : D == 128 ? 8 : 2;
  const int round = D == 64 ? 2 : 4;
  int S = static_cast<int>((n_rows + rows_min - 1) / rows_min);
  if (S > s_max) S = s_max;
  if (S < 1) S = 1;
  int rps = static_cast<int>((n_rows + S - 1) / S);
  rps = (rps + round - 1) / round * round;
  if (rps < round) rps = round;
  return DwPlan{S, rps};
}
}  // namespace

extern "C" size_t agnn_relt_dw_workspace_bytes(int n_items, int32_t n_rel, int32_t heads, int32_t D, int64_t n_rows) {
  if (n_items <= 0 || n_rel <= 0 || heads <= 0 || D <= 0 || n_rows <= 0) return 0;
  const DwPlan pl = relt_dw_plan(n_rows, D);
  return static_cast<size_t>(n_items) * pl.S * n_rel * heads * D * D * sizeof(float) + 256;
}

extern "C" int agnn_relt_dw_f32(int n_items, const agnn_relt_item_t* items, int32_t n_rel, int32_t heads, int32_t D, int64_t n_rows,
                                void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = relt_check("relt_dw", n_items, items, n_rel, heads, D, n_rows)) return rc;
  const int64_t H = static_cast<int64_t>(heads) * D;
  const int groups = n_rel * heads;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  if (n_rows == 0) {
    for (int i = 0; i < n_items; ++i) {
      if (!items[i].y) return fail(AGNN_EINVAL, "relt_dw: item %d has a null output", i);
      hipError_t e = hipMemsetAsync(items[i].y, 0, static_cast<size_t>(groups) * D * D * sizeof(float), s);
      if (e != hipSuccess) return fail(AGNN_ERUNTIME, "relt_dw: %s", hipGetErrorString(e));
    }
    return AGNN_OK;
  }
  const size_t need = agnn_relt_dw_workspace_bytes(n_items, n_rel, heads, D, n_rows);
  if (!workspace || workspace_bytes < need) return fail(AGNN_ENOMEM, "relt_dw: workspace %zu < %zu bytes", workspace_bytes, need);
  const DwPlan pl = relt_dw_plan(n_rows, D);
  ReltArgs p{};                                    // x = x [n, H] (ld_x), w = dy [n, n_rel*H] (ld_y), y = dA blocks [groups][D][D]
  p.S = pl.S; p.rows_per_slice = pl.rows_per_slice;
  p.slab = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t{255});
  if (int rc = relt_fill("relt_dw", n_items, items, n_rel, heads, n_rows, 8, true, H, H * n_rel, "x / dy must be 8-byte aligned with even leading dimensions", p))
    return rc;
  const unsigned S = static_cast<unsigned>(pl.S);
  if (D <= 8) {                                    // one thread per row of a block gradient
    const dim3 grid(static_cast<unsigned>((groups * D + 255) / 256), S, static_cast<unsigned>(n_items));
    if (D == 4) hipLaunchKernelGGL(k_relt_dw_valu<4>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_relt_dw_valu<8>, grid, dim3(256), 0, s, p);
  } else {                                         // one wave per job: a head (D <= 64) or a 64 x 64 tile of a head's block
    const int jobs = D <= 64 ? heads : heads * (D / 64) * (D / 64);
    const dim3 grid(static_cast<unsigned>(n_rel * n_items), S, static_cast<unsigned>((jobs + 3) / 4));
    const dim3 block(static_cast<unsigned>(64 * (jobs < 4 ? jobs : 4)));
    switch (D) {
      case 16: hipLaunchKernelGGL(k_relt_dw_tile<16>, grid, block, 0, s, p); break;
      case 32: hipLaunchKernelGGL(k_relt_dw_tile<32>, grid, block, 0, s, p); break;
      case 64: hipLaunchKernelGGL(k_relt_dw<64>, grid, block, 0, s, p); break;
      case 128: hipLaunchKernelGGL(k_relt_dw<128>, grid, block, 0, s, p); break;
      default: hipLaunchKernelGGL(k_relt_dw<256>, grid, block, 0, s, p); break;
    }
  }
  if (int rc = check_launch("relt_dw")) return rc;
  for (int i = 0; i < n_items; ++i) {
    const float* slab = p.slab + static_cast<size_t>(i) * pl.S * groups * D * D;
    if (int rc = launch_slab_reduce(slab, nullptr, pl.S, groups * D, D, groups * D, D, items[i].y, D, nullptr, s)) return rc;
  }
  return AGNN_OK;
}
