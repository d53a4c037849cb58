// Dense multi-head self-attention over the N rows of one batch, exact fp32, flash style: forward and backward without
// anything of size N x N.  (The reference's graph-transformer layers call nn.MultiheadAttention on the whole batch as ONE
// sequence, models/core/gnn.py:471, core/hgnn.py:273: heads x N x N scores, 4 GB per layer and direction at N = 16 000.)
//
// All three kernels are built on v_mfma_f32_32x32x2_f32 and on one fact about it: a 32 x 32 result has its COLUMN on the lane
// and its rows in the 16 accumulator registers (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), and the B operand of a following
// product that sums over that row index is register r as it stands, when the A operand of k-step r is read at the two rows
// d_row32(r, 0) / d_row32(r, 1) by the two lane halves.  So no score ever moves between lanes or through LDS:
//
//   forward, one wave = 32 query rows (workgroup = 2 or 4 waves = 64 / 128 rows of one head), key tiles of 32:
//     S^T[key][query] = K Q^T            (A = K tile from LDS, B = Q in registers, pre-scaled by log2(e) / sqrt(D))
//     online softmax per lane: a query's 32 scores are 16 registers in each of the lanes c and c + 32
//     O^T[d][query] += V^T P^T           (A = V tile from LDS read at rows d_row32(r, h), B = the probabilities as they stand)
//   backward, pass 1, the same structure, one wave = 32 query rows:   dQ^T += K^T dS^T   with  S^T = K Q^T, dP^T = V dO^T
//   backward, pass 2, mirrored, one wave = 32 KEY rows, query tiles of 32 through LDS:
//     S = Q K^T, dP = dO V^T  (key on the lane),  dV^T += dO^T P~,  dK^T += Q^T dS
//   Seven products instead of five: dQ is complete in one workgroup, so no atomics, no zero-fill, no workgroup waits for
//   another, and every sum has a fixed order (bitwise reproducible).  delta = rowsum(dO o O) is a small launch of its own.
//
// K / V (pass 2: Q / dO) tiles are double-buffered in LDS: the next tile's global loads are issued before the products of the
// current one and written to the other buffer after them; one barrier per tile.  LDS rows have a stride of max(D, 32) + 2
// floats ((stride / 2) odd: the 32 rows of an operand read fall on 32 different even banks, the two lane halves on the odd
// ones).  D < 32 pads the d side of the 32 x 32 output tiles with zero columns, written once.
//
// Dropout (torch's MultiheadAttention: on the normalised probabilities; the row sum uses the undropped ones):
// Philox-4x32-10 with the project's (seed, step, call id) keying; one draw serves the four consecutive keys 4g .. 4g + 3 of a
// query row, counter = the 64-bit element index (head N + query) N + 4g in two counter words.  The backward is handed the
// forward's rng_used, and agnn_attn_dropout_keep_f32 exports the factors through the same device function.
#include <cmath>

#include "agnn_common.h"

namespace {

using agnn::f32x16;
using agnn::d_row32;

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

struct AttnArgs {
  const float* q;
  const float* k;
  const float* v;
  int64_t ld;              // common row stride of q, k, v
  int32_t N, heads;
  float scale, p;
  const int64_t* rng;      // device [2]: seed, step (NULL without dropout)
  uint32_t call_id;
};

// keep factors (0 or 1 / (1 - p)) of keys key4 .. key4 + 3 (key4 % 4 == 0) of query row `row` = head N + query
__device__ __forceinline__ float4 attn_keep4(uint64_t seed, uint64_t step, uint32_t call_id, uint64_t row, int64_t N, int key4, float p) {
  const uint64_t idx = row * static_cast<uint64_t>(N) + static_cast<uint32_t>(key4);
  return agnn::keep_factors(agnn::stream_bits(seed, step, call_id, idx), agnn::drop_threshold(p), 1.f / (1.f - p));
}

template <int D>
struct Tile {
  static constexpr int DP = D < 32 ? 32 : D;     // width of the d side of the output tiles
  static constexpr int LD = DP + 2;              // LDS row stride, floats
  static constexpr int DT = DP / 32;             // 32 x 32 output tiles along d
  static constexpr int KS = D / 2;               // k-steps of a product over d
  static constexpr int C4 = D / 4;               // float4 per row
  static constexpr int NLD = (32 * C4 + 127) / 128;   // float4 per thread and matrix of a 32-row tile at 128 threads
  static constexpr int FLOATS = 32 * LD;
};

// 32 rows x D floats of two matrices with one row stride, rows past N as zeros: global -> registers ...
template <int D>
__device__ __forceinline__ void tile_load(float4 (&sa)[Tile<D>::NLD], float4 (&sb)[Tile<D>::NLD], const float* __restrict__ A,
                                          const float* __restrict__ B, int64_t ld_a, int64_t ld_b, int row0, int N, int tid, int nthr) {
  using T = Tile<D>;
#pragma unroll
  for (int i = 0; i < T::NLD; ++i) {
    const int f = tid + i * nthr;
    const int r = f / T::C4, c4 = f % T::C4;
    const int row = row0 + r;
    const bool on = f < 32 * T::C4 && row < N;
    sa[i] = on ? *reinterpret_cast<const float4*>(A + static_cast<int64_t>(row) * ld_a + c4 * 4) : agnn::f4_zero();
    sb[i] = on ? *reinterpret_cast<const float4*>(B + static_cast<int64_t>(row) * ld_b + c4 * 4) : agnn::f4_zero();
  }
}

// ... -> LDS (rows are 8-byte aligned: two 8-byte writes per float4)
template <int D>
__device__ __forceinline__ void tile_store(const float4 (&sa)[Tile<D>::NLD], const float4 (&sb)[Tile<D>::NLD], float* __restrict__ la,
                                           float* __restrict__ lb, int tid, int nthr) {
  using T = Tile<D>;
#pragma unroll
  for (int i = 0; i < T::NLD; ++i) {
    const int f = tid + i * nthr;
    if (f >= 32 * T::C4) continue;
    const int o = (f / T::C4) * T::LD + (f % T::C4) * 4;
    *reinterpret_cast<float2*>(la + o) = make_float2(sa[i].x, sa[i].y);
    *reinterpret_cast<float2*>(la + o + 2) = make_float2(sa[i].z, sa[i].w);
    *reinterpret_cast<float2*>(lb + o) = make_float2(sb[i].x, sb[i].y);
    *reinterpret_cast<float2*>(lb + o + 2) = make_float2(sb[i].z, sb[i].w);
  }
}

// out^T[d][col] += A^T[d][row] x[row][col]: the rows of the 32 x 32 tile x are its 16 registers, A is an LDS tile [row][d]
template <int D>
__device__ __forceinline__ void acc_transposed(f32x16 (&out)[Tile<D>::DT], const float* __restrict__ la, const f32x16& x, int c, int h) {
  using T = Tile<D>;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float* rowp = la + d_row32(r, h) * T::LD + c;
#pragma unroll
    for (int t = 0; t < T::DT; ++t) out[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(rowp[32 * t], x[r], out[t], 0, 0, 0);
  }
}

// the lane's column of out^T (d on the registers) to row `row` of a [N, heads D] matrix, times s
template <int D>
__device__ __forceinline__ void store_transposed(const f32x16 (&out)[Tile<D>::DT], float* __restrict__ dst, float s, int h) {
  using T = Tile<D>;
#pragma unroll
  for (int t = 0; t < T::DT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * t + 8 * g + 4 * h;
      if (d < D) *reinterpret_cast<float4*>(dst + d) = make_float4(out[t][4 * g] * s, out[t][4 * g + 1] * s, out[t][4 * g + 2] * s, out[t][4 * g + 3] * s);
    }
}

template <int D>
__device__ __forceinline__ void lds_clear(float* sm, int n, int tid, int nthr) {
  if constexpr (D < 32) {                        // the zero columns d >= D of the padded tiles (the loaders never write them)
    for (int i = tid; i < n; i += nthr) sm[i] = 0.f;
    __syncthreads();
  }
}

// multiply the 16 probabilities of the lane (query row `row`, keys key0 + d_row32(r, h)) by their keep factors
__device__ __forceinline__ void apply_keep_keys(f32x16& x, uint64_t seed, uint64_t step, const AttnArgs& a, uint64_t row, int key0, int h) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 m = attn_keep4(seed, step, a.call_id, row, a.N, key0 + 8 * g + 4 * h, a.p);
    x[4 * g] *= m.x; x[4 * g + 1] *= m.y; x[4 * g + 2] *= m.z; x[4 * g + 3] *= m.w;
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void k_attn_fwd(AttnArgs a, float* __restrict__ o, int64_t ld_o, float* __restrict__ lse,
                                                  int64_t* __restrict__ rng_used) {
  using T = Tile<D>;
  __shared__ __align__(16) float sm[2][2][T::FLOATS];          // [buffer][K | V]
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, N = a.N;
  const int qrow = blockIdx.x * (nthr >> 1) + wave * 32 + c;
  const bool drop = a.p > 0.f;
  uint64_t seed = 0, step = 0;
  if (drop) { seed = static_cast<uint64_t>(a.rng[0]); step = static_cast<uint64_t>(a.rng[1]); }
  if (rng_used != nullptr && a.rng != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    rng_used[0] = a.rng[0];
    rng_used[1] = a.rng[1];
  }
  const float* kp = a.k + head * D;
  const float* vp = a.v + head * D;
  lds_clear<D>(&sm[0][0][0], 4 * T::FLOATS, tid, nthr);

  float q[T::KS];
  {
    const float qs = a.scale * kLog2e;
    const float* qp = a.q + static_cast<int64_t>(qrow < N ? qrow : 0) * a.ld + head * D + h;
#pragma unroll
    for (int s = 0; s < T::KS; ++s) q[s] = qrow < N ? qp[2 * s] * qs : 0.f;
  }
  f32x16 acc[T::DT];
#pragma unroll
  for (int t = 0; t < T::DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float m = -INFINITY, l = 0.f;

  float4 sa[T::NLD], sb[T::NLD];
  tile_load<D>(sa, sb, kp, vp, a.ld, a.ld, 0, N, tid, nthr);
  tile_store<D>(sa, sb, sm[0][0], sm[0][1], tid, nthr);
  __syncthreads();
  const int nt = (N + 31) / 32;
  for (int kt = 0; kt < nt; ++kt) {
    const int buf = kt & 1, key0 = kt * 32;
    const float* lk = sm[buf][0];
    const float* lv = sm[buf][1];
    if (kt + 1 < nt) tile_load<D>(sa, sb, kp, vp, a.ld, a.ld, key0 + 32, N, tid, nthr);
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < T::KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x2f32(lk[c * T::LD + 2 * ks + h], q[ks], s, 0, 0, 0);
    if (key0 + 32 > N) {                           // tail keys: out of the row maximum and the sums
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (key0 + d_row32(r, h) >= N) s[r] = -INFINITY;
    }
    float mx = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);                 // finite: key0 < N, so every tile has a key in range
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = __builtin_amdgcn_exp2f(s[r] - mn);
      rs += s[r];
    }
    rs += __shfl_xor(rs, 32, 64);
    l = l * alpha + rs;
    m = mn;
#pragma unroll
    for (int t = 0; t < T::DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] *= alpha;
    if (drop) apply_keep_keys(s, seed, step, a, static_cast<uint64_t>(head) * N + qrow, key0, h);
    acc_transposed<D>(acc, lv, s, c, h);
    if (kt + 1 < nt) tile_store<D>(sa, sb, sm[buf ^ 1][0], sm[buf ^ 1][1], tid, nthr);
    __syncthreads();
  }
  if (qrow < N) {
    store_transposed<D>(acc, o + static_cast<int64_t>(qrow) * ld_o + head * D, 1.f / l, h);
    if (h == 0) lse[static_cast<int64_t>(head) * N + qrow] = (m + __builtin_amdgcn_logf(l)) * kLn2;   // v_log_f32 is log2
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// delta[head][query] = sum_d dO o O
__global__ __launch_bounds__(256) void k_attn_delta(const float* __restrict__ dO, int64_t ld_do, const float* __restrict__ o, int64_t ld_o,
                                                    int N, int heads, int D, float* __restrict__ delta) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<int64_t>(N) * heads) return;
  const int row = static_cast<int>(i / heads), head = static_cast<int>(i % heads);
  const float4* a = reinterpret_cast<const float4*>(dO + row * ld_do + head * D);
  const float4* b = reinterpret_cast<const float4*>(o + row * ld_o + head * D);
  float s = 0.f;
  for (int j = 0; j < D / 4; ++j) {
    const float4 x = a[j], y = b[j];
    s += (x.x * y.x + x.y * y.y) + (x.z * y.z + x.w * y.w);
  }
  delta[static_cast<int64_t>(head) * N + row] = s;
}

// pass 1: dQ.  One wave = 32 query rows; K / V tiles through LDS.
template <int D>
__global__ __launch_bounds__(256) void k_attn_bwd_dq(AttnArgs a, const float* __restrict__ dO, int64_t ld_do, const float* __restrict__ lse,
                                                     const float* __restrict__ delta, float* __restrict__ dq, int64_t ld_dq) {
  using T = Tile<D>;
  __shared__ __align__(16) float sm[2][2][T::FLOATS];
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, N = a.N;
  const int qrow = blockIdx.x * (nthr >> 1) + wave * 32 + c;
  const bool drop = a.p > 0.f;
  uint64_t seed = 0, step = 0;
  if (drop) { seed = static_cast<uint64_t>(a.rng[0]); step = static_cast<uint64_t>(a.rng[1]); }
  const float* kp = a.k + head * D;
  const float* vp = a.v + head * D;
  lds_clear<D>(&sm[0][0][0], 4 * T::FLOATS, tid, nthr);

  float q[T::KS], g[T::KS];
  float lse2 = 0.f, dl = 0.f;
  {
    const float qs = a.scale * kLog2e;
    const int64_t rr = qrow < N ? qrow : 0;
    const float* qp = a.q + rr * a.ld + head * D + h;
    const float* gp = dO + rr * ld_do + head * D + h;
#pragma unroll
    for (int s = 0; s < T::KS; ++s) {
      q[s] = qrow < N ? qp[2 * s] * qs : 0.f;
      g[s] = qrow < N ? gp[2 * s] : 0.f;
    }
    if (qrow < N) {
      lse2 = lse[static_cast<int64_t>(head) * N + qrow] * kLog2e;
      dl = delta[static_cast<int64_t>(head) * N + qrow];
    }
  }
  f32x16 acc[T::DT];
#pragma unroll
  for (int t = 0; t < T::DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  float4 sa[T::NLD], sb[T::NLD];
  tile_load<D>(sa, sb, kp, vp, a.ld, a.ld, 0, N, tid, nthr);
  tile_store<D>(sa, sb, sm[0][0], sm[0][1], tid, nthr);
  __syncthreads();
  const int nt = (N + 31) / 32;
  for (int kt = 0; kt < nt; ++kt) {
    const int buf = kt & 1, key0 = kt * 32;
    const float* lk = sm[buf][0];
    const float* lv = sm[buf][1];
    if (kt + 1 < nt) tile_load<D>(sa, sb, kp, vp, a.ld, a.ld, key0 + 32, N, tid, nthr);
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = -lse2; dp[r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < T::KS; ++ks) {
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(lk[c * T::LD + 2 * ks + h], q[ks], s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(lv[c * T::LD + 2 * ks + h], g[ks], dp, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = (key0 + d_row32(r, h) < N) ? __builtin_amdgcn_exp2f(s[r]) : 0.f;
    if (drop) apply_keep_keys(dp, seed, step, a, static_cast<uint64_t>(head) * N + qrow, key0, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] *= dp[r] - dl;                    // dS = P o (dP o keep - delta)
    acc_transposed<D>(acc, lk, s, c, h);
    if (kt + 1 < nt) tile_store<D>(sa, sb, sm[buf ^ 1][0], sm[buf ^ 1][1], tid, nthr);
    __syncthreads();
  }
  if (qrow < N) store_transposed<D>(acc, dq + static_cast<int64_t>(qrow) * ld_dq + head * D, a.scale, h);
}

// pass 2: dK and dV.  One wave = 32 key rows (K, V in registers); Q / dO tiles, lse and delta through LDS.
template <int D>
__global__ __launch_bounds__(256) void k_attn_bwd_dkv(AttnArgs a, const float* __restrict__ dO, int64_t ld_do, const float* __restrict__ lse,
                                                      const float* __restrict__ delta, float* __restrict__ dk, float* __restrict__ dv,
                                                      int64_t ld_dkv) {
  using T = Tile<D>;
  __shared__ __align__(16) float sm[2][2][T::FLOATS];          // [buffer][Q | dO]
  __shared__ float4 srow[2][2][8];               // [buffer][lse log2(e) | delta][32 floats]
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, N = a.N;
  const int krow = blockIdx.x * (nthr >> 1) + wave * 32 + c;
  const bool drop = a.p > 0.f;
  uint64_t seed = 0, step = 0;
  if (drop) { seed = static_cast<uint64_t>(a.rng[0]); step = static_cast<uint64_t>(a.rng[1]); }
  const float* qp = a.q + head * D;
  const float* gp = dO + head * D;
  const float* lsep = lse + static_cast<int64_t>(head) * N;
  const float* dlp = delta + static_cast<int64_t>(head) * N;
  lds_clear<D>(&sm[0][0][0], 4 * T::FLOATS, tid, nthr);

  float kr[T::KS], vr[T::KS];
  {
    const float ks_ = a.scale * kLog2e;
    const int64_t rr = krow < N ? krow : 0;
    const float* kp = a.k + rr * a.ld + head * D + h;
    const float* vp = a.v + rr * a.ld + head * D + h;
#pragma unroll
    for (int s = 0; s < T::KS; ++s) {
      kr[s] = krow < N ? kp[2 * s] * ks_ : 0.f;
      vr[s] = krow < N ? vp[2 * s] : 0.f;
    }
  }
  f32x16 dka[T::DT], dva[T::DT];
#pragma unroll
  for (int t = 0; t < T::DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dka[t][r] = 0.f; dva[t][r] = 0.f; }

  float4 sa[T::NLD], sb[T::NLD];
  float rl = 0.f, rd = 0.f;                      // threads 0 .. 31: a tile row's lse (+inf past N: P = 0) and delta
  auto row_load = [&](int q0) {
    if (tid < 32) {
      const bool on = q0 + tid < N;
      rl = on ? lsep[q0 + tid] * kLog2e : INFINITY;
      rd = on ? dlp[q0 + tid] : 0.f;
    }
  };
  auto row_store = [&](int b) {
    if (tid < 32) {
      reinterpret_cast<float*>(srow[b][0])[tid] = rl;
      reinterpret_cast<float*>(srow[b][1])[tid] = rd;
    }
  };
  tile_load<D>(sa, sb, qp, gp, a.ld, ld_do, 0, N, tid, nthr);
  row_load(0);
  tile_store<D>(sa, sb, sm[0][0], sm[0][1], tid, nthr);
  row_store(0);
  __syncthreads();
  const int nt = (N + 31) / 32;
  for (int qt = 0; qt < nt; ++qt) {
    const int buf = qt & 1, q0 = qt * 32;
    const float* lq = sm[buf][0];
    const float* lg = sm[buf][1];
    if (qt + 1 < nt) {
      tile_load<D>(sa, sb, qp, gp, a.ld, ld_do, q0 + 32, N, tid, nthr);
      row_load(q0 + 32);
    }
    f32x16 s, dp;                                 // [query d_row32(r, h)][key c]
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 x = srow[buf][0][2 * g + h];
      s[4 * g] = -x.x; s[4 * g + 1] = -x.y; s[4 * g + 2] = -x.z; s[4 * g + 3] = -x.w;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < T::KS; ++ks) {
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(lq[c * T::LD + 2 * ks + h], kr[ks], s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(lg[c * T::LD + 2 * ks + h], vr[ks], dp, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(s[r]);   // -inf for a query past N
    f32x16 pt = s;                                // P~ = P o keep
    if (drop) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float4 mk = attn_keep4(seed, step, a.call_id, static_cast<uint64_t>(head) * N + (q0 + d_row32(r, h)), N, krow & ~3, a.p);
        const int w = krow & 3;
        const float kf = w == 0 ? mk.x : w == 1 ? mk.y : w == 2 ? mk.z : mk.w;
        pt[r] *= kf;
        dp[r] *= kf;
      }
    }
    acc_transposed<D>(dva, lg, pt, c, h);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 x = srow[buf][1][2 * g + h];
      s[4 * g] *= dp[4 * g] - x.x; s[4 * g + 1] *= dp[4 * g + 1] - x.y; s[4 * g + 2] *= dp[4 * g + 2] - x.z; s[4 * g + 3] *= dp[4 * g + 3] - x.w;
    }
    acc_transposed<D>(dka, lq, s, c, h);
    if (qt + 1 < nt) {
      tile_store<D>(sa, sb, sm[buf ^ 1][0], sm[buf ^ 1][1], tid, nthr);
      row_store(buf ^ 1);
    }
    __syncthreads();
  }
  if (krow < N) {
    store_transposed<D>(dka, dk + static_cast<int64_t>(krow) * ld_dkv + head * D, a.scale, h);
    store_transposed<D>(dva, dv + static_cast<int64_t>(krow) * ld_dkv + head * D, 1.f, h);
  }
}

// the keep factors as a dense [heads, N, N] matrix (inspection and tests at small N)
__global__ __launch_bounds__(256) void k_attn_keep(int N, int heads, float p, const int64_t* __restrict__ rng, uint32_t call_id,
                                                   float* __restrict__ keep) {
  const int g4 = (N + 3) / 4;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<int64_t>(heads) * N * g4) return;
  const int64_t row = i / g4;
  const int key4 = static_cast<int>(i % g4) * 4;
  float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
  if (p > 0.f) m = attn_keep4(static_cast<uint64_t>(rng[0]), static_cast<uint64_t>(rng[1]), call_id, static_cast<uint64_t>(row), N, key4, p);
  float* dst = keep + row * N + key4;
  dst[0] = m.x;
  if (key4 + 1 < N) dst[1] = m.y;
  if (key4 + 2 < N) dst[2] = m.z;
  if (key4 + 3 < N) dst[3] = m.w;
}

constexpr int kMaxN = 1 << 24;
constexpr int kMaxHeads = 65535;                 // gridDim.y

bool width_ok(int D) { return D == 8 || D == 16 || D == 32 || D == 64; }

int attn_check(const char* who, const void* q, const void* k, const void* v, int64_t ld, int64_t N, int32_t heads, int32_t D, float p,
               const void* rng, int32_t q_rows) {
  using namespace agnn;
  if (!width_ok(D)) return fail(AGNN_EINVAL, "%s: head width D=%d must be 8, 16, 32 or 64", who, D);
  if (heads < 1 || heads > kMaxHeads) return fail(AGNN_EINVAL, "%s: heads=%d must be in [1, %d]", who, heads, kMaxHeads);
  if (N < 1 || N > kMaxN) return fail(AGNN_EINVAL, "%s: N=%lld must be in [1, %d]", who, (long long)N, kMaxN);
  if (!(p >= 0.f && p < 1.f)) return fail(AGNN_EINVAL, "%s: dropout p=%f", who, p);
  if (q_rows != 0 && q_rows != 64 && q_rows != 128) return fail(AGNN_EINVAL, "%s: q_rows=%d must be 0 (automatic), 64 or 128", who, q_rows);
  if (ld < static_cast<int64_t>(heads) * D) return fail(AGNN_EINVAL, "%s: ld_qkv=%lld smaller than heads * D = %d", who, (long long)ld, heads * D);
  if (!q || !k || !v) return fail(AGNN_EINVAL, "%s: null argument", who);
  if (p > 0.f && !rng) return fail(AGNN_EINVAL, "%s: dropout needs the device rng state", who);
  if ((ld & 3) || !aligned16(q) || !aligned16(k) || !aligned16(v)) return fail(AGNN_EALIGN, "%s: q / k / v rows must be 16-byte aligned (ld_qkv=%lld)", who, (long long)ld);
  return 0;
}

int out_check(const char* who, const char* name, const void* p, int64_t ld, int width) {
  using namespace agnn;
  if (!p) return fail(AGNN_EINVAL, "%s: %s is null", who, name);
  if (ld < width) return fail(AGNN_EINVAL, "%s: leading dimension %lld of %s smaller than heads * D = %d", who, (long long)ld, name, width);
  if ((ld & 3) || !aligned16(p)) return fail(AGNN_EALIGN, "%s: rows of %s must be 16-byte aligned (ld=%lld)", who, name, (long long)ld);
  return 0;
}

// rows of one workgroup: 128 where that still gives every CU a workgroup, else 64
int block_rows(int64_t N, int heads, int q_rows) {
  if (q_rows) return q_rows;
  return ((N + 127) / 128) * heads >= 256 ? 128 : 64;
}

size_t round256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

}  // namespace

#define AGNN_ATTN_DISPATCH(KERN, ...)                                                        \
  do {                                                                                       \
    if (D == 8) hipLaunchKernelGGL(KERN<8>, grid, block, 0, s, __VA_ARGS__);                 \
    else if (D == 16) hipLaunchKernelGGL(KERN<16>, grid, block, 0, s, __VA_ARGS__);          \
    else if (D == 32) hipLaunchKernelGGL(KERN<32>, grid, block, 0, s, __VA_ARGS__);          \
    else hipLaunchKernelGGL(KERN<64>, grid, block, 0, s, __VA_ARGS__);                       \
  } while (0)

extern "C" int agnn_attn_fwd_f32(const float* q, const float* k, const float* v, int64_t ld_qkv, int64_t N, int32_t heads, int32_t D,
                                 float scale, float p, const int64_t* rng_state, uint32_t call_id, int32_t q_rows, float* o, int64_t ld_o,
                                 float* lse, int64_t* rng_used, agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = attn_check("attn_fwd", q, k, v, ld_qkv, N, heads, D, p, rng_state, q_rows)) return rc;
  if (int rc = out_check("attn_fwd", "o", o, ld_o, heads * D)) return rc;
  if (!lse) return fail(AGNN_EINVAL, "attn_fwd: lse is null");
  AttnArgs a{q, k, v, ld_qkv, static_cast<int32_t>(N), heads, scale, p, p > 0.f ? rng_state : nullptr, call_id};
  const int rows = block_rows(N, heads, q_rows);
  const dim3 grid(static_cast<unsigned>((N + rows - 1) / rows), static_cast<unsigned>(heads)), block(2 * rows);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  AGNN_ATTN_DISPATCH(k_attn_fwd, a, o, ld_o, lse, p > 0.f ? rng_used : nullptr);
  return check_launch("attn_fwd");
}

extern "C" size_t agnn_attn_bwd_workspace_bytes(int64_t N, int32_t heads) {
  if (N < 1 || heads < 1) return 256;
  return round256(static_cast<size_t>(N) * static_cast<size_t>(heads) * sizeof(float));
}

extern "C" int agnn_attn_bwd_f32(const float* q, const float* k, const float* v, int64_t ld_qkv, int64_t N, int32_t heads, int32_t D,
                                 float scale, float p, const int64_t* rng_used, uint32_t call_id, int32_t q_rows, const float* dO,
                                 int64_t ld_do, const float* o, int64_t ld_o, const float* lse, float* dq, float* dk, float* dv,
                                 int64_t ld_dqkv, void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = attn_check("attn_bwd", q, k, v, ld_qkv, N, heads, D, p, rng_used, q_rows)) return rc;
  const int E = heads * D;
  if (int rc = out_check("attn_bwd", "dO", dO, ld_do, E)) return rc;
  if (int rc = out_check("attn_bwd", "o", o, ld_o, E)) return rc;
  if (int rc = out_check("attn_bwd", "dq", dq, ld_dqkv, E)) return rc;
  if (int rc = out_check("attn_bwd", "dk", dk, ld_dqkv, E)) return rc;
  if (int rc = out_check("attn_bwd", "dv", dv, ld_dqkv, E)) return rc;
  if (!lse) return fail(AGNN_EINVAL, "attn_bwd: lse is null");
  if (!workspace || !aligned16(workspace)) return fail(AGNN_EINVAL, "attn_bwd: workspace is null or misaligned");
  if (workspace_bytes < agnn_attn_bwd_workspace_bytes(N, heads)) return fail(AGNN_ENOMEM, "attn_bwd: workspace too small");
  AttnArgs a{q, k, v, ld_qkv, static_cast<int32_t>(N), heads, scale, p, p > 0.f ? rng_used : nullptr, call_id};
  float* delta = static_cast<float*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(k_attn_delta, dim3(static_cast<unsigned>((N * heads + 255) / 256)), dim3(256), 0, s, dO, ld_do, o, ld_o,
                     static_cast<int>(N), heads, D, delta);
  if (int rc = check_launch("attn_bwd (delta)")) return rc;
  const int rows = block_rows(N, heads, q_rows);
  const dim3 grid(static_cast<unsigned>((N + rows - 1) / rows), static_cast<unsigned>(heads)), block(2 * rows);
  AGNN_ATTN_DISPATCH(k_attn_bwd_dq, a, dO, ld_do, lse, delta, dq, ld_dqkv);
  if (int rc = check_launch("attn_bwd (dq)")) return rc;
  AGNN_ATTN_DISPATCH(k_attn_bwd_dkv, a, dO, ld_do, lse, delta, dk, dv, ld_dqkv);
  return check_launch("attn_bwd (dk, dv)");
}

extern "C" int agnn_attn_dropout_keep_f32(int64_t N, int32_t heads, float p, const int64_t* rng, uint32_t call_id, float* keep,
                                          agnn_stream_t stream_) {
  using namespace agnn;
  if (heads < 1 || heads > kMaxHeads) return fail(AGNN_EINVAL, "attn_dropout_keep: heads=%d must be in [1, %d]", heads, kMaxHeads);
  if (N < 1 || N > 8192) return fail(AGNN_EINVAL, "attn_dropout_keep: N=%lld must be in [1, 8192] (a dense heads x N x N matrix)", (long long)N);
  if (!(p >= 0.f && p < 1.f)) return fail(AGNN_EINVAL, "attn_dropout_keep: dropout p=%f", p);
  if (!keep) return fail(AGNN_EINVAL, "attn_dropout_keep: keep is null");
  if (p > 0.f && !rng) return fail(AGNN_EINVAL, "attn_dropout_keep: dropout needs the rng state the forward used");
  const int64_t n = static_cast<int64_t>(heads) * N * ((N + 3) / 4);
  hipLaunchKernelGGL(k_attn_keep, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_),
                     static_cast<int>(N), heads, p, rng, call_id, keep);
  return check_launch("attn_dropout_keep");
}
