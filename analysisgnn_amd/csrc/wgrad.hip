// Weight-gradient GEMM for the projection layers:  dW[out, in] = sum_n dY[n, out] * X[n, in]  (+ db[out] = sum_n dY[n, out])
//
// Every projection of the encoder sees N = (#subgraphs x 500) rows, so its weight gradient is a GEMM with a SMALL
// output (256 x 256 ... 256 x 1024) and a HUGE reduction dimension (N = 16 000).  The library picks a
// 32 x 32-tile kernel without a K split for that shape — a few dozen workgroups on a 256-CU chip: 88 us per
// launch whatever the size, 19 launches per step (profiles/r01_c).  This kernel is built for the shape:
//   * fp32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32, 64 FLOP/clk/SIMD), no LDS at all — both operands are
//     already "K-major": one MFMA k-step needs dY[n, 32 cols] and X[n, 32 cols] for two consecutive n, which is
//     exactly one coalesced 8-byte-per-lane load of each (lane = column pair, lane half = n parity);
//   * a 128 x 128 block tile, 4 waves in 2 x 2, each wave 64 x 64 = four accumulators; output rows/cols are taken
//     with stride 2 inside a wave so the two floats a lane loads feed two different MFMA tiles without any shuffle;
//   * N is cut into S slices so that (#tiles x S) ~ 2 workgroups per CU; each workgroup writes its partial tile to
//     a slab and a second tiny kernel sums the S slabs in a fixed order (deterministic, no atomics);
//   * the bias gradient rides along (column sums of the dY values already in registers).
#include "agnn_common.h"

namespace {

using agnn::f32x16;

struct WgArgs {
  const float* dy;
  const float* x;
  int64_t ld_dy, ld_x;
  int32_t n, out_f, in_f;
  int32_t rows_per_slice;   // even
  int32_t tiles_in;         // number of 128-wide tiles along `in`
  float* slab;              // [S][out_pad][in_pad]
  float* slab_b;            // [S][out_pad] or nullptr
  int32_t out_pad, in_pad;
};

__device__ __forceinline__ void wgrad_tile(const WgArgs& a, const int tile, const int slice) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int to = tile / a.tiles_in, ti = tile - to * a.tiles_in;
  const int kk = lane >> 5, c32 = lane & 31;
  const int ocol = to * 128 + wm * 64 + 2 * c32;     // this lane's two output-feature columns of dY
  const int icol = ti * 128 + wn * 64 + 2 * c32;     // this lane's two input-feature columns of X
  const bool o_ok = ocol < a.out_f;                  // widths are even: a float2 is inside or outside as a whole
  const bool i_ok = icol < a.in_f;
  const int r0 = slice * a.rows_per_slice;
  int r1 = r0 + a.rows_per_slice;
  if (r1 > a.n) r1 = a.n;

  f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
  float bs0 = 0.f, bs1 = 0.f;
  // Loads are unconditional so the loop stays straight-line code and the compiler can wait on "all but the last two
  // chunks" (s_waitcnt vmcnt(N)) instead of draining the queue behind a branch: lanes whose columns lie past the
  // matrix read column 0 (their accumulator rows / columns are never read back), rows past the end of the matrix
  // are clamped, and rows past the end of the SLICE only occur in the last chunks, which multiply by a 0/1 mask.
  // Addresses: a per-slice base pointer (uniform -> SGPR pair) plus a 32-bit byte offset per lane (the C-ABI entry
  // point checks rows_per_slice * ld * 4 < 2^32), i.e. the "saddr + voffset" form: one multiply-add per load.
  const float* dy_s = a.dy + static_cast<int64_t>(r0) * a.ld_dy;
  const float* x_s = a.x + static_cast<int64_t>(r0) * a.ld_x;
  const uint32_t ldb_dy = static_cast<uint32_t>(a.ld_dy) * 4u, ldb_x = static_cast<uint32_t>(a.ld_x) * 4u;
  const uint32_t cb_dy = (o_ok ? ocol : 0) * 4u, cb_x = (i_ok ? icol : 0) * 4u;
  const int rel_last = a.n - 1 - r0;
  constexpr int CH = 8;                              // k-steps (row pairs) per chunk
  constexpr int STEP = 2 * CH;                       // rows per chunk
  // Three register stages in rotation: the loads of chunk c+2 are issued before the MFMAs of chunk c, so two whole
  // chunks of matrix work (2 x 32 MFMAs = 4096 cycles of one wave) cover an L2/HBM round trip even when a SIMD
  // holds a single wave (256 x 256 outputs give one workgroup per CU).  The scheduling barrier after each fetch
  // keeps the compiler from hoisting the bias-sum adds of a chunk right behind its loads (which drained the queue).
  float2 a0[CH], b0[CH], a1[CH], b1[CH], a2[CH], b2[CH];
  // Row offsets advance by two rows per k-step: running 32-bit byte offsets and ONE add per load.  (Computed from the row number
  // each time, every load cost a clamp and a 64-bit multiply-add — v_mad_u64_u32, quarter rate: 32 of them per 32 MFMAs, ~700 cycles
  // of address arithmetic per 2 048 cycles of matrix work in a wave that cannot issue an MFMA meanwhile.)  Chunks are fetched in
  // order, so the offsets only move forward; the last chunks, which may reach past the end of the MATRIX, take the clamped path.
  uint32_t o_dy = static_cast<uint32_t>(kk) * ldb_dy + cb_dy, o_x = static_cast<uint32_t>(kk) * ldb_x + cb_x;
  const uint32_t s_dy = 2u * ldb_dy, s_x = 2u * ldb_x;
  auto fetch_fast = [&](float2* ao, float2* bo) {     // the next chunk in order, entirely inside the matrix
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      ao[u] = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(dy_s) + o_dy);
      bo[u] = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(x_s) + o_x);
      o_dy += s_dy;
      o_x += s_x;
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto fetch = [&](int chunk, float2* ao, float2* bo) {
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const uint32_t rel = static_cast<uint32_t>(min(chunk * STEP + 2 * u + kk, rel_last));
      ao[u] = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(dy_s) + (rel * ldb_dy + cb_dy));
      bo[u] = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(x_s) + (rel * ldb_x + cb_x));
    }
    o_dy += CH * s_dy;                               // keeps the running offsets in step (not used past this point in practice)
    o_x += CH * s_x;
    __builtin_amdgcn_sched_barrier(0);
  };
  auto mma = [&](const float2* av, const float2* bv) {
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].x, bv[u].x, acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].x, bv[u].y, acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].y, bv[u].x, acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].y, bv[u].y, acc11, 0, 0, 0);
      // volatile asm: pins the bias-sum adds to this phase (plain adds were hoisted behind the loads of the chunk)
      asm volatile("v_add_f32 %0, %0, %1" : "+v"(bs0) : "v"(av[u].x));
      asm volatile("v_add_f32 %0, %0, %1" : "+v"(bs1) : "v"(av[u].y));
    }
  };
  auto mma_tail = [&](int chunk, const float2* av, const float2* bv) {     // rows >= r1 contribute nothing
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const float m = (r0 + chunk * STEP + 2 * u + kk < r1) ? 1.f : 0.f;
      const float ax = av[u].x * m, ay = av[u].y * m;
      acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(ax, bv[u].x, acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(ax, bv[u].y, acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, bv[u].x, acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(ay, bv[u].y, acc11, 0, 0, 0);
      bs0 += ax;
      bs1 += ay;
    }
  };
  const int nfull = (r1 - r0) / STEP;                // chunks that lie entirely inside the slice
  const int nchunks = (r1 - r0 + STEP - 1) / STEP;
  fetch(0, a0, b0);
  fetch(1, a1, b1);
  int c = 0;
  const int safe = (rel_last + 1) / STEP;            // chunks [0, safe) lie entirely inside the matrix: no clamp needed
  for (; c + 3 <= nfull && c + 5 <= safe; c += 3) {  // (the trip fetches chunks c + 2, c + 3, c + 4)
    fetch_fast(a2, b2);
    mma(a0, b0);
    fetch_fast(a0, b0);
    mma(a1, b1);
    fetch_fast(a1, b1);
    mma(a2, b2);
  }
  for (; c + 3 <= nfull; c += 3) {
    fetch(c + 2, a2, b2);
    mma(a0, b0);
    fetch(c + 3, a0, b0);
    mma(a1, b1);
    fetch(c + 4, a1, b1);
    mma(a2, b2);
  }
  fetch(c + 2, a2, b2);
  if (c < nchunks) mma_tail(c, a0, b0);
  if (c + 1 < nchunks) mma_tail(c + 1, a1, b1);
  if (c + 2 < nchunks) mma_tail(c + 2, a2, b2);
  // C/D layout of 32x32 MFMA: lane l, register r -> row i = (r&3) + 8*(r>>2) + 4*(l>>5), column j = l&31
  float* slab = a.slab + (static_cast<int64_t>(slice) * a.out_pad) * a.in_pad;
  const int ob = to * 128 + wm * 64, ib = ti * 128 + wn * 64;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = agnn::d_row32(r, kk);
    float* row0 = slab + static_cast<int64_t>(ob + 2 * i) * a.in_pad + ib + 2 * c32;          // output feature ob+2i   (tile c = 0)
    float* row1 = row0 + a.in_pad;                                                            // output feature ob+2i+1 (tile c = 1)
    *reinterpret_cast<float2*>(row0) = make_float2(acc00[r], acc01[r]);
    *reinterpret_cast<float2*>(row1) = make_float2(acc10[r], acc11[r]);
  }
  if (a.slab_b != nullptr && wn == 0) {
    bs0 += __shfl_xor(bs0, 32, 64);                  // the two lane halves hold the two n parities
    bs1 += __shfl_xor(bs1, 32, 64);
    if (kk == 0 && ti == 0)
      *reinterpret_cast<float2*>(a.slab_b + static_cast<int64_t>(slice) * a.out_pad + ocol) = make_float2(bs0, bs1);
  }
}

__global__ __launch_bounds__(256) void k_wgrad(WgArgs a) { wgrad_tile(a, blockIdx.x, blockIdx.y); }

// ---- several weight gradients in ONE launch (round 3) ------------------------------------------------------------------------
// A training step computes ~20 of these products, most of them small (256 x 256, 384 x 128, 128 x 128 ... outputs): alone, each
// needs up to 64 row slices to put a workgroup on every CU — 64 slabs written and read back per output, a 250-row K loop per
// workgroup, and a reduction launch of its own (20 x ~11 us per step).  The deferred weight gradients (dp.defer_weight_grads) are
// pending TOGETHER at the encoder's flush points, so they are issued together: the workgroups of all items fill the chip, every
// item gets by with the same few slices (384 / total tiles: 5 at the GNN stack's flush), K loops of thousands of rows, and ONE
// reduction launch serves all outputs.
constexpr int kWgBatchMax = AGNN_WGRAD_BATCH_MAX_ITEMS;   // 16 products, of which up to 8 may come as two column-block items (linear.weight_grad_batch)

struct WgBatch {
  WgArgs it[kWgBatchMax];
  int32_t first[kWgBatchMax + 1];        // first workgroup of item i (prefix sums of tiles_i * S_i)
  int32_t tiles[kWgBatchMax];
  int32_t n;
};

__global__ __launch_bounds__(256) void k_wgrad_batch(WgBatch b) {
  int i = 0;
  const int blk = blockIdx.x;
  while (i + 1 < b.n && blk >= b.first[i + 1]) ++i;              // workgroup-uniform
  const int local = blk - b.first[i];
  const int tiles = b.tiles[i];
  const int slice = local / tiles;
  wgrad_tile(b.it[i], local - slice * tiles, slice);
}


// dw[o][i] = sum_s slab[s][o][i] ;  db[o] = sum_s slab_b[s][o]   (fixed order: 8 interleaved partial sums, then a
// fixed tree).  A block = 32 float2 columns x 8 slab groups, so the S slab reads of one output element are
// spread over 8 threads with independent loads in flight instead of one thread walking S strided lines.
// `store_w(o, i, t)` receives the finished column pair (i, i + 1) of output row o, `store_b(e, t)` the bias sum of row e (only
// where `with_bias`): the one copy of the arithmetic serves the single destination below and the destination lists of the
// gradient epilogue at the end of this file.
template <typename StoreW, typename StoreB>
__device__ __forceinline__ void wgrad_reduce_sums(const float* __restrict__ slab, const float* __restrict__ slab_b, int S, int out_f, int in_f,
                                                  int out_pad, int in_pad, const bool with_bias, const int block, const int n_blocks,
                                                  StoreW store_w, StoreB store_b) {
  __shared__ float2 part[8][32];
  const int col = threadIdx.x & 31, sg = threadIdx.x >> 5;
  const int half_in = in_f >> 1;
  const int64_t total = static_cast<int64_t>(out_f) * half_in;
  const int64_t plane = static_cast<int64_t>(out_pad) * in_pad;
  for (int64_t e0 = static_cast<int64_t>(block) * 32; e0 < total; e0 += static_cast<int64_t>(n_blocks) * 32) {
    const int64_t e = e0 + col;
    float2 s = make_float2(0.f, 0.f);
    int o = 0, i = 0;
    if (e < total) {
      o = static_cast<int>(e / half_in);
      i = static_cast<int>(e - static_cast<int64_t>(o) * half_in) * 2;
      const float* p = slab + static_cast<int64_t>(o) * in_pad + i;
      for (int k = sg; k < S; k += 8) {
        const float2 v = *reinterpret_cast<const float2*>(p + k * plane);
        s.x += v.x;
        s.y += v.y;
      }
    }
    part[sg][col] = s;
    __syncthreads();
    if (sg == 0 && e < total) {
      float2 t = part[0][col];
#pragma unroll
      for (int g = 1; g < 8; ++g) { t.x += part[g][col].x; t.y += part[g][col].y; }
      store_w(o, i, t);
    }
    __syncthreads();
  }
  if (with_bias) {
    // same 32 x 8 decomposition for the bias slabs (a serial walk over S slabs cost ~19 us of load latency)
    __shared__ float partb[8][32];
    for (int e0 = block * 32; e0 < out_f; e0 += n_blocks * 32) {
      const int e = e0 + col;
      float s = 0.f;
      if (e < out_f)
        for (int k = sg; k < S; k += 8) s += slab_b[static_cast<int64_t>(k) * out_pad + e];
      partb[sg][col] = s;
      __syncthreads();
      if (sg == 0 && e < out_f) {
        float t = partb[0][col];
#pragma unroll
        for (int g = 1; g < 8; ++g) t += partb[g][col];
        store_b(e, t);
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ void wgrad_reduce_blocks(const float* __restrict__ slab, const float* __restrict__ slab_b, int S, int out_f, int in_f,
                                                    int out_pad, int in_pad, float* __restrict__ dw, int64_t ld_dw, float* __restrict__ db,
                                                    const int block, const int n_blocks) {
  wgrad_reduce_sums(slab, slab_b, S, out_f, in_f, out_pad, in_pad, db != nullptr, block, n_blocks,
                    [=](int o, int i, float2 t) { *reinterpret_cast<float2*>(dw + static_cast<int64_t>(o) * ld_dw + i) = t; },
                    [=](int e, float t) { db[e] = t; });
}

__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ slab, const float* __restrict__ slab_b, int S,
                                                      int out_f, int in_f, int out_pad, int in_pad, float* __restrict__ dw,
                                                      int64_t ld_dw, float* __restrict__ db) {
  wgrad_reduce_blocks(slab, slab_b, S, out_f, in_f, out_pad, in_pad, dw, ld_dw, db, blockIdx.x, gridDim.x);
}

struct RedItem {
  const float* slab;
  const float* slab_b;
  float* dw;
  float* db;
  int64_t ld_dw;
  int32_t S, out_f, in_f, out_pad, in_pad;
};
struct RedBatch {
  RedItem it[kWgBatchMax];
  int32_t first[kWgBatchMax + 1];
  int32_t n;
};

__global__ __launch_bounds__(256) void k_wgrad_reduce_batch(RedBatch b) {
  int i = 0;
  const int blk = blockIdx.x;
  while (i + 1 < b.n && blk >= b.first[i + 1]) ++i;
  const RedItem& r = b.it[i];
  wgrad_reduce_blocks(r.slab, r.slab_b, r.S, r.out_f, r.in_f, r.out_pad, r.in_pad, r.dw, r.ld_dw, r.db, blk - b.first[i], b.first[i + 1] - b.first[i]);
}

struct Plan {
  int tiles_out, tiles_in, S, rows_per_slice, out_pad, in_pad;
};

Plan make_plan(int64_t n, int out_f, int in_f) {
  Plan p;
  p.tiles_out = (out_f + 127) / 128;
  p.tiles_in = (in_f + 127) / 128;
  p.out_pad = p.tiles_out * 128;
  p.in_pad = p.tiles_in * 128;
  const int tiles = p.tiles_out * p.tiles_in;
  // two workgroups per CU, and never a few more than that: rounding the slice count UP gave 520 workgroups for 256 x 1280
  // (20 tiles x 26 slices) — a third round of 8 workgroups behind two full ones: 147 us instead of the ~110 its FLOPs take
  int64_t S = 512 / tiles;
  const int64_t max_s = (n + 63) / 64;              // at least 64 rows per slice
  if (S > max_s) S = max_s;
  if (S > 64) S = 64;                               // slab traffic: S * out * in * 4 B written and read back
  if (S < 1) S = 1;
  int64_t rps = (n + S - 1) / S;
  rps = (rps + 1) & ~int64_t{1};
  p.rows_per_slice = static_cast<int>(rps);
  p.S = static_cast<int>((n + rps - 1) / rps);
  return p;
}

}  // namespace

// dw[o][i] = sum_s slab[s][o][i] (in_f even), db[o] = sum_s slab_b[s][o]; shared with gproj.hip
int agnn::launch_slab_reduce(const float* slab, const float* slab_b, int S, int out_f, int in_f, int out_pad, int in_pad,
                             float* dw, int64_t ld_dw, float* db, hipStream_t s) {
  const int64_t total = static_cast<int64_t>(out_f) * (in_f >> 1);
  int blocks = static_cast<int>((total + 31) / 32);
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3(blocks), dim3(256), 0, s, slab, slab_b, S, out_f, in_f, out_pad, in_pad, dw, ld_dw, db);
  return check_launch("slab_reduce");
}

extern "C" size_t agnn_wgrad_workspace_bytes(int64_t n, int32_t out_f, int32_t in_f) {
  if (n <= 0 || out_f <= 0 || in_f <= 0) return 0;
  const Plan p = make_plan(n, out_f, in_f);
  return (static_cast<size_t>(p.S) * p.out_pad * p.in_pad + static_cast<size_t>(p.S) * p.out_pad) * sizeof(float) + 256;
}

extern "C" int agnn_wgrad_f32(const float* dy, int64_t ld_dy, const float* x, int64_t ld_x, int64_t n, int32_t out_f,
                              int32_t in_f, float* dw, int64_t ld_dw, float* db, void* workspace, size_t workspace_bytes,
                              agnn_stream_t stream_) {
  using namespace agnn;
  if (n <= 0 || n >= (int64_t{1} << 31) || out_f <= 0 || in_f <= 0) return fail(AGNN_EINVAL, "wgrad: bad sizes n=%lld out=%d in=%d", (long long)n, out_f, in_f);
  if ((out_f & 1) || (in_f & 1) || (ld_dy & 1) || (ld_x & 1) || (ld_dw & 1)) return fail(AGNN_EALIGN, "wgrad: widths and leading dimensions must be even");
  if (!dy || !x || !dw || !workspace) return fail(AGNN_EINVAL, "wgrad: null argument");
  if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dw) | reinterpret_cast<uintptr_t>(db)) & 7u)
    return fail(AGNN_EALIGN, "wgrad: pointers must be 8-byte aligned");
  if (ld_dy < out_f || ld_x < in_f || ld_dw < in_f) return fail(AGNN_EINVAL, "wgrad: leading dimension smaller than the width");
  const size_t need = agnn_wgrad_workspace_bytes(n, out_f, in_f);
  if (workspace_bytes < need) return fail(AGNN_ENOMEM, "wgrad: workspace %zu < %zu bytes", workspace_bytes, need);
  const Plan p = make_plan(n, out_f, in_f);
  if ((static_cast<int64_t>(p.rows_per_slice) + 128) * (ld_dy > ld_x ? ld_dy : ld_x) * 4 >= (int64_t{1} << 32))
    return fail(AGNN_EINVAL, "wgrad: a row slice (%d rows x ld) exceeds the kernel's 32-bit byte offsets", p.rows_per_slice);
  char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t{255});
  float* slab = reinterpret_cast<float*>(ws);
  float* slab_b = slab + static_cast<size_t>(p.S) * p.out_pad * p.in_pad;
  WgArgs a{dy, x, ld_dy, ld_x, static_cast<int32_t>(n), out_f, in_f, p.rows_per_slice, p.tiles_in, slab,
           db ? slab_b : nullptr, p.out_pad, p.in_pad};
  hipStream_t s = static_cast<hipStream_t>(stream_);
  // (an LDS-staged variant of the tile, round 2, was ~5 % faster alone and slower inside the training step, next to the
  // recurrence kernels whose workgroups hold most of a CU's LDS: profiles/r01_wgrad_mfma.md; it is not in the library)
  hipLaunchKernelGGL(k_wgrad, dim3(p.tiles_out * p.tiles_in, p.S), dim3(256), 0, s, a);
  if (int rc = check_launch("wgrad")) return rc;
  return launch_slab_reduce(slab, db ? slab_b : nullptr, p.S, out_f, in_f, p.out_pad, p.in_pad, dw, ld_dw, db, s);
}

namespace {
struct BatchPlan {
  int n;
  int tiles_out[kWgBatchMax], tiles_in[kWgBatchMax], S[kWgBatchMax], rps[kWgBatchMax];
  size_t slab_off[kWgBatchMax], slabb_off[kWgBatchMax], total_floats;
};

// one slice count for the whole batch: ~1.5 workgroups per CU over all items together, K loops of >= 64 rows.  The target was swept
// inside the training step (c2s, two runs each on one box): 256 -> 3.39 ms, 320 -> 3.27, 384 -> 3.19, 448 -> 3.28, 512 -> 3.29,
// 640 -> 3.21, 896 -> 3.22, 1280 -> 3.26 (one launch pair per product, as in round 2: 3.34)
int batch_plan(int n_items, const agnn_wgrad_item_t* items, BatchPlan& bp) {
  using namespace agnn;
  if (n_items <= 0 || n_items > kWgBatchMax || !items) return fail(AGNN_EINVAL, "wgrad_batch: %d items (1 .. %d)", n_items, kWgBatchMax);
  bp.n = n_items;
  int64_t tiles = 0;
  for (int i = 0; i < n_items; ++i) {
    const agnn_wgrad_item_t& it = items[i];
    if (it.n <= 0 || it.n >= (int64_t{1} << 31) || it.out_f <= 0 || it.in_f <= 0) return fail(AGNN_EINVAL, "wgrad_batch: item %d: bad sizes", i);
    bp.tiles_out[i] = (it.out_f + 127) / 128;
    bp.tiles_in[i] = (it.in_f + 127) / 128;
    tiles += static_cast<int64_t>(bp.tiles_out[i]) * bp.tiles_in[i];
  }
  int64_t S = 384 / tiles;
  if (S > 64) S = 64;
  if (S < 1) S = 1;
  size_t off = 0;
  for (int i = 0; i < n_items; ++i) {
    const agnn_wgrad_item_t& it = items[i];
    int64_t s_i = S;
    const int64_t max_s = (it.n + 63) / 64;
    if (s_i > max_s) s_i = max_s;
    int64_t rps = (it.n + s_i - 1) / s_i;
    rps = (rps + 1) & ~int64_t{1};
    bp.rps[i] = static_cast<int>(rps);
    bp.S[i] = static_cast<int>((it.n + rps - 1) / rps);
    const size_t plane = static_cast<size_t>(bp.tiles_out[i]) * 128 * bp.tiles_in[i] * 128;
    bp.slab_off[i] = off;
    off += static_cast<size_t>(bp.S[i]) * plane;
    bp.slabb_off[i] = off;
    off += static_cast<size_t>(bp.S[i]) * bp.tiles_out[i] * 128;
    off = (off + 63) & ~size_t{63};                 // every item's slabs start on a 256-byte boundary
  }
  bp.total_floats = off;
  return AGNN_OK;
}
}  // namespace

extern "C" size_t agnn_wgrad_batch_workspace_bytes(int32_t n_items, const agnn_wgrad_item_t* items) {
  BatchPlan bp;
  if (batch_plan(n_items, items, bp) != AGNN_OK) return 0;
  return bp.total_floats * sizeof(float) + 256;
}

extern "C" int agnn_wgrad_batch_f32(int32_t n_items, const agnn_wgrad_item_t* items, void* workspace, size_t workspace_bytes,
                                    agnn_stream_t stream_) {
  using namespace agnn;
  BatchPlan bp;
  if (int rc = batch_plan(n_items, items, bp)) return rc;
  if (!workspace || workspace_bytes < bp.total_floats * sizeof(float) + 256) return fail(AGNN_ENOMEM, "wgrad_batch: workspace too small");
  float* ws = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t{255});
  WgBatch wb{};
  RedBatch rb{};
  wb.n = rb.n = n_items;
  int wg = 0, red = 0;
  for (int i = 0; i < n_items; ++i) {
    const agnn_wgrad_item_t& it = items[i];
    if ((it.out_f & 1) || (it.in_f & 1) || (it.ld_dy & 1) || (it.ld_x & 1) || (it.ld_dw & 1)) return fail(AGNN_EALIGN, "wgrad_batch: item %d: widths and leading dimensions must be even", i);
    if (!it.dy || !it.x || !it.dw) return fail(AGNN_EINVAL, "wgrad_batch: item %d: null argument", i);
    if ((reinterpret_cast<uintptr_t>(it.dy) | reinterpret_cast<uintptr_t>(it.x) | reinterpret_cast<uintptr_t>(it.dw) | reinterpret_cast<uintptr_t>(it.db)) & 7u)
      return fail(AGNN_EALIGN, "wgrad_batch: item %d: pointers must be 8-byte aligned", i);
    if (it.ld_dy < it.out_f || it.ld_x < it.in_f || it.ld_dw < it.in_f) return fail(AGNN_EINVAL, "wgrad_batch: item %d: leading dimension smaller than the width", i);
    if ((static_cast<int64_t>(bp.rps[i]) + 128) * (it.ld_dy > it.ld_x ? it.ld_dy : it.ld_x) * 4 >= (int64_t{1} << 32))
      return fail(AGNN_EINVAL, "wgrad_batch: item %d: a row slice (%d rows x ld) exceeds the kernel's 32-bit byte offsets", i, bp.rps[i]);
    const int out_pad = bp.tiles_out[i] * 128, in_pad = bp.tiles_in[i] * 128;
    float* slab = ws + bp.slab_off[i];
    float* slab_b = ws + bp.slabb_off[i];
    wb.it[i] = WgArgs{it.dy, it.x, it.ld_dy, it.ld_x, static_cast<int32_t>(it.n), it.out_f, it.in_f, bp.rps[i], bp.tiles_in[i], slab,
                      it.db ? slab_b : nullptr, out_pad, in_pad};
    wb.tiles[i] = bp.tiles_out[i] * bp.tiles_in[i];
    wb.first[i] = wg;
    wg += wb.tiles[i] * bp.S[i];
    rb.it[i] = RedItem{slab, it.db ? slab_b : nullptr, it.dw, it.db, it.ld_dw, bp.S[i], it.out_f, it.in_f, out_pad, in_pad};
    rb.first[i] = red;
    int64_t blocks = (static_cast<int64_t>(it.out_f) * (it.in_f >> 1) + 31) / 32;
    if (blocks > 1024) blocks = 1024;
    red += static_cast<int>(blocks);
  }
  wb.first[n_items] = wg;
  rb.first[n_items] = red;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(k_wgrad_batch, dim3(static_cast<unsigned>(wg)), dim3(256), 0, s, wb);
  if (int rc = check_launch("wgrad_batch")) return rc;
  hipLaunchKernelGGL(k_wgrad_reduce_batch, dim3(static_cast<unsigned>(red)), dim3(256), 0, s, rb);
  return check_launch("wgrad_batch(reduce)");
}

// ---- gradient epilogue: slab sums and LayerNorm column sums stored straight into their final destinations ---------------------
// The products above only feed the optimizer, and so do the dgamma / dbeta column sums that are pending at the same flush points.
// Their results used to be written to temporaries and copied on: a fan-out launch for the SAGE layers' per-relation parameters
// (the summed root weight and bias replicated R times), a gather of every gradient into the flat buffer, a launch of their own
// for the column sums.  Here ONE reduction launch per flush serves the products and the column sums, and each result element is
// stored to every destination that wants it.  The arithmetic is that of wgrad_reduce_blocks / na_colsum_block (normact.hip), term
// for term; only the stores differ.
namespace {

constexpr int kEpiRecMax = 64;        // weight destinations per reduction launch; a call that names more (16 SAGE products of 4 relations
                                      // have 128) gets a further reduction launch per 64: same sums, one more launch
constexpr int kEpiDbMax = 48;         // bias destinations per reduction launch
constexpr int kEpiSumMax = AGNN_GRAD_MAX_SUMS;   // column sums per call (agnn_norm_act_colsum_batch_f32's limit as well)
constexpr int kEpiPartRows = 1024;    // partial rows agnn_norm_act_bwd_f32 leaves at most (normact.hip: kBwdBlocks)

struct EpiRec {
  float* p;
  int32_t ld, c0, c1, scalar;
};
struct EpiItem {
  const float* slab;
  const float* slab_b;
  int32_t S, out_f, in_f, out_pad, in_pad;
  int16_t rec0, rec1, db0, db1;
};
struct EpiSum {
  const float* part;
  float* dgamma;
  float* dbeta;
  int32_t n_rows, H;
};
struct EpiBatch {                     // a kernel argument: must stay below 4 KB
  EpiItem it[kWgBatchMax];
  EpiRec rec[kEpiRecMax];
  float* db[kEpiDbMax];
  EpiSum sum[kEpiSumMax];
  int32_t first[kWgBatchMax + kEpiSumMax + 1];
  int32_t n_items, n_all;
};
static_assert(sizeof(EpiBatch) <= 4096, "EpiBatch travels as a kernel argument");

// wgrad_reduce_sums with a destination list: every finished element goes to each record whose column range holds it
__device__ __forceinline__ void epi_product(const EpiBatch& b, const EpiItem& r, const int block, const int n_blocks) {
  const int rec0 = r.rec0, rec1 = r.rec1, db0 = r.db0, db1 = r.db1;
  wgrad_reduce_sums(
      r.slab, r.slab_b, r.S, r.out_f, r.in_f, r.out_pad, r.in_pad, db1 > db0, block, n_blocks,
      [&](int o, int i, float2 t) {
        for (int q = rec0; q < rec1; ++q) {                 // block-uniform trip count, records read through scalar loads
          const EpiRec d = b.rec[q];
          float* row = d.p + static_cast<int64_t>(o) * d.ld - d.c0;
          if (d.scalar) {                                   // odd column count: float by float, the range checked per column
            if (i >= d.c0 && i < d.c1) row[i] = t.x;
            if (i + 1 >= d.c0 && i + 1 < d.c1) row[i + 1] = t.y;
          } else if (i >= d.c0 && i < d.c1) {               // c0, c1 even: a column pair lies inside or outside as a whole
            *reinterpret_cast<float2*>(row + i) = t;
          }
        }
      },
      [&](int e, float t) {
        for (int q = db0; q < db1; ++q) b.db[q][e] = t;
      });
}

// na_colsum_block (normact.hip) on a 256-thread block: that kernel runs 32 chains of additions per column, chain `grp` adding
// part[grp + 32 k], k = 0 .. 31, in that order per pass of 1024 rows, and then sums the chains in index order.  Here a thread
// carries the four chains g8, g8 + 8, g8 + 16, g8 + 24 in four accumulators; every chain adds the same terms in the same order.
// (Not one function with na_colsum_block: the chains are laid out over the block differently.  The loads of the four chains are
// independent; in the c2s step both launches that carry column sums are shorter than the pairs they replace, 29.0 against 35.6
// and 11.5 against 16.0 us (profiles/grad_delivery.md).  tests/test_gpu_grad_delivery.py holds the bits together.)
__device__ __forceinline__ void epi_colsum(const EpiSum& c, const int block) {
  __shared__ float sm[32][33];
  const int col = threadIdx.x & 31, g8 = threadIdx.x >> 5;
  const int width = 2 * c.H, n_rows = c.n_rows;
  const int j = block * 32 + col;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (j < width) {
    for (int w00 = 0; w00 < n_rows; w00 += 32 * 32) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int w0 = w00 + g8 + 8 * q;
        if (w0 >= n_rows) continue;                       // (that chain makes no such pass in na_colsum_block either)
        float v[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) {
          const int w = w0 + 32 * k;
          v[k] = w < n_rows ? c.part[static_cast<int64_t>(w) * width + j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 32; ++k) s[q] += v[k];
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) sm[g8 + 8 * q][col] = s[q];
  __syncthreads();
  if (g8 == 0 && j < width) {
    float t = sm[0][col];
#pragma unroll
    for (int k = 1; k < 32; ++k) t += sm[k][col];
    if (j < c.H) c.dgamma[j] = t; else c.dbeta[j - c.H] = t;
  }
}

__global__ __launch_bounds__(256) void k_grad_epilogue(EpiBatch b) {
  int i = 0;
  const int blk = blockIdx.x;
  while (i + 1 < b.n_all && blk >= b.first[i + 1]) ++i;             // block-uniform: item type and trip counts are too
  const int local = blk - b.first[i];
  if (i < b.n_items) epi_product(b, b.it[i], local, b.first[i + 1] - b.first[i]);
  else epi_colsum(b.sum[i - b.n_items], local);
}

// one destination as the host sees it: `rows` segments of `cols` floats, `ld` apart
struct EpiSpan {
  const float* p;
  int64_t ld;
  int32_t rows, cols;
  int32_t item, c0, c1;             // item < 0: not a weight record (never a declared copy)
};

bool spans_overlap(const EpiSpan& a, const EpiSpan& b) {
  const float* a_end = a.p + static_cast<int64_t>(a.rows - 1) * a.ld + a.cols;
  const float* b_end = b.p + static_cast<int64_t>(b.rows - 1) * b.ld + b.cols;
  if (a_end <= b.p || b_end <= a.p) return false;
  if (a.rows > 1 && b.rows > 1 && a.ld == b.ld) {           // column blocks of one matrix: compare the column windows
    int64_t r = (b.p - a.p) % a.ld;
    if (r < 0) r += a.ld;
    if (r >= a.cols && r + b.cols <= a.ld) return false;
  }
  return true;                                              // (different strides with interleaved hulls: refused, not analysed)
}

}  // namespace

static void epi_as_wgrad(int32_t n_items, const agnn_grad_item_t* items, agnn_wgrad_item_t* out) {
  for (int i = 0; i < n_items; ++i) {
    const agnn_grad_item_t& g = items[i];
    out[i] = agnn_wgrad_item_t{g.dy, g.x, nullptr, nullptr, g.ld_dy, g.ld_x, g.in_f, g.n, g.out_f, g.in_f};
  }
}

extern "C" size_t agnn_grad_epilogue_workspace_bytes(int32_t n_items, const agnn_grad_item_t* items) {
  if (n_items <= 0 || n_items > kWgBatchMax || !items) return 0;
  agnn_wgrad_item_t w[kWgBatchMax];
  epi_as_wgrad(n_items, items, w);
  return agnn_wgrad_batch_workspace_bytes(n_items, w);
}

extern "C" int agnn_grad_epilogue_f32(int32_t n_items, const agnn_grad_item_t* items, int32_t n_sums, const agnn_colsum_item_t* sums,
                                      void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (n_items < 0 || n_items > kWgBatchMax || (n_items > 0 && !items)) return fail(AGNN_EINVAL, "grad_epilogue: %d products (0 .. %d)", n_items, kWgBatchMax);
  if (n_sums < 0 || n_sums > kEpiSumMax || (n_sums > 0 && !sums)) return fail(AGNN_EINVAL, "grad_epilogue: %d column sums (0 .. %d)", n_sums, kEpiSumMax);
  if (n_items == 0 && n_sums == 0) return AGNN_OK;
  BatchPlan bp;
  bp.n = 0;
  bp.total_floats = 0;
  float* ws = nullptr;
  if (n_items > 0) {
    agnn_wgrad_item_t w[kWgBatchMax];
    epi_as_wgrad(n_items, items, w);
    if (int rc = batch_plan(n_items, w, bp)) return rc;
    if (!workspace || workspace_bytes < bp.total_floats * sizeof(float) + 256) return fail(AGNN_ENOMEM, "grad_epilogue: workspace too small");
    ws = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t{255});
  }
  // ---- validation: operands as agnn_wgrad_batch_f32, then every destination, then overlaps
  static thread_local EpiSpan spans[kWgBatchMax * 2 * AGNN_PACK_MAX_SRC + 2 * kEpiSumMax];
  int n_spans = 0;
  for (int i = 0; i < n_items; ++i) {
    const agnn_grad_item_t& it = items[i];
    if ((it.out_f & 1) || (it.in_f & 1) || (it.ld_dy & 1) || (it.ld_x & 1)) return fail(AGNN_EALIGN, "grad_epilogue: item %d: widths and leading dimensions must be even", i);
    if (!it.dy || !it.x) return fail(AGNN_EINVAL, "grad_epilogue: item %d: null argument", i);
    if ((reinterpret_cast<uintptr_t>(it.dy) | reinterpret_cast<uintptr_t>(it.x)) & 7u) return fail(AGNN_EALIGN, "grad_epilogue: item %d: pointers must be 8-byte aligned", i);
    if (it.ld_dy < it.out_f || it.ld_x < it.in_f) return fail(AGNN_EINVAL, "grad_epilogue: item %d: leading dimension smaller than the width", i);
    if ((static_cast<int64_t>(bp.rps[i]) + 128) * (it.ld_dy > it.ld_x ? it.ld_dy : it.ld_x) * 4 >= (int64_t{1} << 32))
      return fail(AGNN_EINVAL, "grad_epilogue: item %d: a row slice (%d rows x ld) exceeds the kernel's 32-bit byte offsets", i, bp.rps[i]);
    if (it.n_dw < 0 || it.n_dw > AGNN_PACK_MAX_SRC || it.n_db < 0 || it.n_db > AGNN_PACK_MAX_SRC || it.n_dw + it.n_db == 0)
      return fail(AGNN_EINVAL, "grad_epilogue: item %d: %d weight and %d bias destinations (0 .. %d each, one at least)", i, it.n_dw, it.n_db, AGNN_PACK_MAX_SRC);
    for (int k = 0; k < it.n_dw; ++k) {
      const agnn_grad_dst_t& d = it.dw[k];
      const int cols = d.c1 - d.c0;
      if (!d.p || d.c0 < 0 || cols <= 0 || d.c1 > it.in_f || d.ld < cols || d.ld >= (int64_t{1} << 31))
        return fail(AGNN_EINVAL, "grad_epilogue: item %d: destination %d: columns [%d, %d) of %d, ld %lld", i, k, d.c0, d.c1, it.in_f, (long long)d.ld);
      if (reinterpret_cast<uintptr_t>(d.p) & 3u) return fail(AGNN_EALIGN, "grad_epilogue: item %d: destination %d is not a float pointer", i, k);
      if (!(cols & 1) && ((d.c0 & 1) || (d.ld & 1) || (reinterpret_cast<uintptr_t>(d.p) & 7u)))
        return fail(AGNN_EALIGN, "grad_epilogue: item %d: destination %d: an even column block needs an even c0, an even ld and an 8-byte aligned pointer", i, k);
      spans[n_spans++] = EpiSpan{d.p, d.ld, it.out_f, cols, i, d.c0, d.c1};
    }
    for (int k = 0; k < it.n_db; ++k) {
      if (!it.db[k]) return fail(AGNN_EINVAL, "grad_epilogue: item %d: null bias destination %d", i, k);
      if (reinterpret_cast<uintptr_t>(it.db[k]) & 3u) return fail(AGNN_EALIGN, "grad_epilogue: item %d: bias destination %d is not a float pointer", i, k);
      spans[n_spans++] = EpiSpan{it.db[k], it.out_f, 1, it.out_f, -1, 0, 0};
    }
  }
  for (int i = 0; i < n_sums; ++i) {
    const agnn_colsum_item_t& it = sums[i];
    if (it.n <= 0 || it.H <= 0 || (it.H & 3) || it.H > 2048 || !it.workspace || !it.dgamma || !it.dbeta)
      return fail(AGNN_EINVAL, "grad_epilogue: column sum %d: bad sizes or null argument", i);
    if (it.workspace_bytes < static_cast<size_t>(kEpiPartRows) * 2 * it.H * sizeof(float)) return fail(AGNN_ENOMEM, "grad_epilogue: column sum %d: workspace too small", i);
    if ((reinterpret_cast<uintptr_t>(it.dgamma) | reinterpret_cast<uintptr_t>(it.dbeta) | reinterpret_cast<uintptr_t>(it.workspace)) & 3u)
      return fail(AGNN_EALIGN, "grad_epilogue: column sum %d: misaligned", i);
    spans[n_spans++] = EpiSpan{it.dgamma, it.H, 1, it.H, -1, 0, 0};
    spans[n_spans++] = EpiSpan{it.dbeta, it.H, 1, it.H, -1, 0, 0};
  }
  for (int a = 0; a < n_spans; ++a)
    for (int c = a + 1; c < n_spans; ++c) {
      const EpiSpan &sa = spans[a], &sc = spans[c];
      // two records of one product that name the same range AND the same place receive the same value at every address
      if (sa.item >= 0 && sa.item == sc.item && sa.c0 == sc.c0 && sa.c1 == sc.c1 && sa.p == sc.p && sa.ld == sc.ld) continue;
      if (spans_overlap(sa, sc)) return fail(AGNN_EINVAL, "grad_epilogue: destinations %d and %d of the call overlap", a, c);
    }
  hipStream_t s = static_cast<hipStream_t>(stream_);
  // ---- the products: agnn_wgrad_batch_f32's launch, unchanged
  if (n_items > 0) {
    WgBatch wb{};
    wb.n = n_items;
    int wg = 0;
    for (int i = 0; i < n_items; ++i) {
      const agnn_grad_item_t& it = items[i];
      const int out_pad = bp.tiles_out[i] * 128, in_pad = bp.tiles_in[i] * 128;
      wb.it[i] = WgArgs{it.dy, it.x, it.ld_dy, it.ld_x, static_cast<int32_t>(it.n), it.out_f, it.in_f, bp.rps[i], bp.tiles_in[i], ws + bp.slab_off[i],
                        it.n_db > 0 ? ws + bp.slabb_off[i] : nullptr, out_pad, in_pad};
      wb.tiles[i] = bp.tiles_out[i] * bp.tiles_in[i];
      wb.first[i] = wg;
      wg += wb.tiles[i] * bp.S[i];
    }
    wb.first[n_items] = wg;
    hipLaunchKernelGGL(k_wgrad_batch, dim3(static_cast<unsigned>(wg)), dim3(256), 0, s, wb);
    if (int rc = check_launch("grad_epilogue(products)")) return rc;
  }
  // ---- the reduction: as many products per launch as the record tables hold, the column sums with the last
  int at = 0;
  do {
    EpiBatch eb{};
    int n = 0, n_rec = 0, n_db = 0, blocks = 0;
    while (at < n_items && n_rec + items[at].n_dw <= kEpiRecMax && n_db + items[at].n_db <= kEpiDbMax) {
      const agnn_grad_item_t& it = items[at];
      EpiItem& e = eb.it[n];
      e.slab = ws + bp.slab_off[at];
      e.slab_b = it.n_db > 0 ? ws + bp.slabb_off[at] : nullptr;
      e.S = bp.S[at];
      e.out_f = it.out_f;
      e.in_f = it.in_f;
      e.out_pad = bp.tiles_out[at] * 128;
      e.in_pad = bp.tiles_in[at] * 128;
      e.rec0 = static_cast<int16_t>(n_rec);
      for (int k = 0; k < it.n_dw; ++k) {
        const agnn_grad_dst_t& d = it.dw[k];
        eb.rec[n_rec++] = EpiRec{d.p, static_cast<int32_t>(d.ld), d.c0, d.c1, (d.c1 - d.c0) & 1};
      }
      e.rec1 = static_cast<int16_t>(n_rec);
      e.db0 = static_cast<int16_t>(n_db);
      for (int k = 0; k < it.n_db; ++k) eb.db[n_db++] = it.db[k];
      e.db1 = static_cast<int16_t>(n_db);
      eb.first[n] = blocks;
      int64_t rb = (static_cast<int64_t>(it.out_f) * (it.in_f >> 1) + 31) / 32;       // agnn_wgrad_batch_f32's block count
      if (rb > 1024) rb = 1024;
      blocks += static_cast<int>(rb);
      ++n;
      ++at;
    }
    eb.n_items = n;
    if (at == n_items)
      for (int i = 0; i < n_sums; ++i) {
        const agnn_colsum_item_t& it = sums[i];
        int nb = static_cast<int>((it.n + 3) / 4);
        if (nb > kEpiPartRows) nb = kEpiPartRows;
        eb.sum[i] = EpiSum{static_cast<const float*>(it.workspace), it.dgamma, it.dbeta, nb, it.H};
        eb.first[n++] = blocks;
        blocks += (2 * it.H + 31) / 32;
      }
    eb.first[n] = blocks;
    eb.n_all = n;
    if (blocks > 0) {
      hipLaunchKernelGGL(k_grad_epilogue, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, eb);
      if (int rc = check_launch("grad_epilogue(reduce)")) return rc;
    }
  } while (at < n_items);
  return AGNN_OK;
}
