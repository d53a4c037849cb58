// Cross-task attention of the logit-fusion block (ref: CrossTaskTransformer, models/analysis.py:408-418): n_seq independent
// sequences of T <= 32 task tokens, `heads` heads of width D, exact fp32.  The opposite shape of attn.hip (one sequence of N
// rows): a whole sequence fits a corner of LDS, a query's T scores never leave its lane, and no matrix instruction is needed.
//
// Layout.  qkv is the packed in-projection [n_seq T, 3E] (q | k | v, head h in columns h D .. h D + D - 1 of each block), o is
// [n_seq T, E] with the heads side by side, dqkv is [n_seq T, 3E]: the GEMMs around the kernels read and write them as they
// stand.  A workgroup owns S consecutive sequences (S = 256 / (heads T), less where 64 KB of LDS hold fewer) and has one lane
// per (sequence, head, row): lane = (s heads + h) T + r, r fastest, so the lanes of one (s, h) read the same LDS row at the
// same time (a broadcast) and different (s, h) fall on different banks (row stride 2E + 4 floats).
//
//   forward   K | V of the S sequences -> LDS (coalesced float4).  Lane (s, h, i): q_i from global into registers, pre-scaled
//             by log2(e) scale; keys in groups of four (the group one dropout draw serves) with an online softmax per group:
//             4 scores, one rescale, o += p~ v.  Writes o and, when asked, lse (log2 units) [n_seq T, heads].
//   backward  pass 1, the same structure: lane (s, h, i) holds q_i, dO_i, delta_i = dO_i . o_i and lse_i; per key
//             P = exp2(s - lse), dP = (dO_i . v_j) keep, dS = P (dP - delta), dq += dS k_j.  It leaves lse_i, delta_i and the
//             row's 32 keep bits in LDS.  Then Q | dO replace K | V in LDS and pass 2 runs key-major: lane (s, h, j) holds
//             k_j, v_j and walks the queries: dv += P~ dO_i, dk += dS q_i.  S is computed twice, so dq, dk and dv are each
//             complete in one lane: no atomics, no cross-lane sums, one fixed order.
//
// Dropout as in attn.hip (torch's MultiheadAttention: on the normalised probabilities, the row sum uses the undropped ones):
// Philox-4x32-10 keyed by (seed, step, call id), one draw for keys 4g .. 4g + 3 of a query row, counter = the element index
// ((n heads + h) 32 + i) 32 + 4g, which names (sequence, head, query, group) and nothing of the launch.
#include <cmath>

#include "agnn_common.h"

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kThreads = 256;
constexpr int kLdsBytes = 64 * 1024;

struct TaskAttnArgs {
  const float* qkv;
  int64_t ld;
  int64_t n_seq;
  int32_t T, heads, S;       // S: sequences per workgroup
  float scale, p;
  const int64_t* rng;        // device [2]: seed, step (NULL without dropout)
  uint32_t call_id;
};

// keep factors (0 or 1 / (1 - p)) of keys 4g .. 4g + 3 of query row i of (sequence n, head h)
__device__ __forceinline__ float4 task_keep4(uint64_t seed, uint64_t step, uint32_t call_id, int64_t n, int heads, int h, int i, int g, float p) {
  const uint64_t idx = ((static_cast<uint64_t>(n) * static_cast<uint32_t>(heads) + static_cast<uint32_t>(h)) * 32u + static_cast<uint32_t>(i)) * 32u +
                       static_cast<uint32_t>(4 * g);
  return agnn::keep_factors(agnn::stream_bits(seed, step, call_id, idx), agnn::drop_threshold(p), 1.f / (1.f - p));
}

// `rows` rows of nc4 float4 from src (row stride ld) to LDS rows of ldr floats, at column col0
__device__ __forceinline__ void stage(float* __restrict__ sm, int ldr, int col0, const float* __restrict__ src, int64_t ld, int rows, int nc4,
                                      int tid) {
  for (int f = tid; f < rows * nc4; f += kThreads) {
    const int row = f / nc4, c4 = f - row * nc4;
    *reinterpret_cast<float4*>(sm + row * ldr + col0 + c4 * 4) = *reinterpret_cast<const float4*>(src + static_cast<int64_t>(row) * ld + c4 * 4);
  }
}

template <int D>
__device__ __forceinline__ void load_row(float (&x)[D], const float* __restrict__ p, float s) {
#pragma unroll
  for (int c = 0; c < D / 4; ++c) {
    const float4 t = reinterpret_cast<const float4*>(p)[c];
    x[4 * c] = t.x * s; x[4 * c + 1] = t.y * s; x[4 * c + 2] = t.z * s; x[4 * c + 3] = t.w * s;
  }
}

template <int D>
__device__ __forceinline__ float dot(const float (&x)[D], const float* __restrict__ p) {
  float a = 0.f, b = 0.f;
#pragma unroll
  for (int c = 0; c < D / 4; ++c) {
    const float4 t = reinterpret_cast<const float4*>(p)[c];
    a = fmaf(x[4 * c], t.x, a); b = fmaf(x[4 * c + 1], t.y, b);
    a = fmaf(x[4 * c + 2], t.z, a); b = fmaf(x[4 * c + 3], t.w, b);
  }
  return a + b;
}

template <int D>
__device__ __forceinline__ void axpy(float (&y)[D], float a, const float* __restrict__ p) {
#pragma unroll
  for (int c = 0; c < D / 4; ++c) {
    const float4 t = reinterpret_cast<const float4*>(p)[c];
    y[4 * c] = fmaf(a, t.x, y[4 * c]); y[4 * c + 1] = fmaf(a, t.y, y[4 * c + 1]);
    y[4 * c + 2] = fmaf(a, t.z, y[4 * c + 2]); y[4 * c + 3] = fmaf(a, t.w, y[4 * c + 3]);
  }
}

template <int D>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&x)[D], float s) {
#pragma unroll
  for (int c = 0; c < D / 4; ++c)
    reinterpret_cast<float4*>(p)[c] = make_float4(x[4 * c] * s, x[4 * c + 1] * s, x[4 * c + 2] * s, x[4 * c + 3] * s);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void k_taskattn_fwd(TaskAttnArgs a, float* __restrict__ o, int64_t ld_o, float* __restrict__ lse,
                                                           int64_t* __restrict__ rng_used) {
  extern __shared__ float4 sm4[];
  float* sm = reinterpret_cast<float*>(sm4);     // [S T][K | V], row stride 2E + 4
  const int tid = threadIdx.x, T = a.T, heads = a.heads;
  const int E = heads * D, ldr = 2 * E + 4;
  const int64_t n0 = static_cast<int64_t>(blockIdx.x) * a.S;
  const int ns = static_cast<int>(a.n_seq - n0 < a.S ? a.n_seq - n0 : a.S);
  const bool drop = a.p > 0.f;
  uint64_t seed = 0, step = 0;
  if (drop) { seed = static_cast<uint64_t>(a.rng[0]); step = static_cast<uint64_t>(a.rng[1]); }
  if (drop && rng_used != nullptr && blockIdx.x == 0 && tid == 0) {
    rng_used[0] = a.rng[0];
    rng_used[1] = a.rng[1];
  }
  stage(sm, ldr, 0, a.qkv + n0 * T * a.ld + E, a.ld, ns * T, E / 2, tid);
  __syncthreads();
  if (tid >= ns * heads * T) return;
  const int s = tid / (heads * T), hr = tid - s * heads * T, h = hr / T, i = hr - h * T;
  const int64_t n = n0 + s, row = n * T + i;

  float q[D], acc[D];
  load_row<D>(q, a.qkv + row * a.ld + h * D, a.scale * kLog2e);
#pragma unroll
  for (int d = 0; d < D; ++d) acc[d] = 0.f;
  float m = -INFINITY, l = 0.f;
  const float* kv = sm + s * T * ldr + h * D;    // key row j of this (s, h): kv + j ldr, its value row: + E
  for (int g = 0; 4 * g < T; ++g) {
    float sc[4];
    const float* rp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = 4 * g + u;
      rp[u] = kv + (j < T ? j : T - 1) * ldr;
      const float x = dot<D>(q, rp[u]);
      sc[u] = j < T ? x : -INFINITY;
    }
    const float mn = fmaxf(fmaxf(m, fmaxf(sc[0], sc[1])), fmaxf(sc[2], sc[3]));   // finite: key 4g is in range
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
#pragma unroll
    for (int u = 0; u < 4; ++u) sc[u] = __builtin_amdgcn_exp2f(sc[u] - mn);
    l = l * alpha + ((sc[0] + sc[1]) + (sc[2] + sc[3]));
    m = mn;
    if (drop) {
      const float4 kf = task_keep4(seed, step, a.call_id, n, heads, h, i, g, a.p);
      sc[0] *= kf.x; sc[1] *= kf.y; sc[2] *= kf.z; sc[3] *= kf.w;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] *= alpha;
#pragma unroll
    for (int u = 0; u < 4; ++u) axpy<D>(acc, sc[u], rp[u] + E);                   // keys past T: factor 0 on a valid row
  }
  store_row<D>(o + row * ld_o + h * D, acc, 1.f / l);
  if (lse != nullptr) lse[row * heads + h] = m + __builtin_amdgcn_logf(l);        // v_log_f32 is log2
}

// ---- backward --------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void k_taskattn_bwd(TaskAttnArgs a, const float* __restrict__ dO, int64_t ld_do,
                                                           const float* __restrict__ o, int64_t ld_o, const float* __restrict__ lse,
                                                           float* __restrict__ dqkv, int64_t ld_d) {
  extern __shared__ float4 sm4[];
  float* sm = reinterpret_cast<float*>(sm4);     // [S T][K | V], then [S T][Q | dO], row stride 2E + 4; then the row statistics
  const int tid = threadIdx.x, T = a.T, heads = a.heads;
  const int E = heads * D, ldr = 2 * E + 4;
  const int64_t n0 = static_cast<int64_t>(blockIdx.x) * a.S;
  const int ns = static_cast<int>(a.n_seq - n0 < a.S ? a.n_seq - n0 : a.S);
  float* st_lse = sm + a.S * T * ldr;            // [S heads T] each: lse (log2), delta, keep bits
  float* st_dl = st_lse + a.S * heads * T;
  uint32_t* st_keep = reinterpret_cast<uint32_t*>(st_dl + a.S * heads * T);
  const bool drop = a.p > 0.f;
  uint64_t seed = 0, step = 0;
  if (drop) { seed = static_cast<uint64_t>(a.rng[0]); step = static_cast<uint64_t>(a.rng[1]); }
  const float inv_keep = 1.f / (1.f - a.p);
  const bool on = tid < ns * heads * T;
  const int s = tid / (heads * T), hr = tid - s * heads * T, h = hr / T, r = hr - h * T;
  const int64_t n = n0 + s, row = n * T + r;
  const float* base = a.qkv + n0 * T * a.ld;
  float* rows = sm + s * T * ldr + h * D;        // row j of this (s, h): rows + j ldr (first block), + E (second block)

  stage(sm, ldr, 0, base + E, a.ld, ns * T, E / 2, tid);
  __syncthreads();
  if (on) {                                      // pass 1: query row r
    float q[D], g[D], dq[D];
    load_row<D>(q, a.qkv + row * a.ld + h * D, a.scale * kLog2e);
    load_row<D>(g, dO + row * ld_do + h * D, 1.f);
    const float dl = dot<D>(g, o + row * ld_o + h * D);
    const float l2 = lse[row * heads + h];
#pragma unroll
    for (int d = 0; d < D; ++d) dq[d] = 0.f;
    uint32_t bits = 0;
    float4 kf4 = make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll 1
    for (int j = 0; j < T; ++j) {
      const int u = j & 3;
      if (drop && u == 0) kf4 = task_keep4(seed, step, a.call_id, n, heads, h, r, j >> 2, a.p);
      const float kf = u == 0 ? kf4.x : u == 1 ? kf4.y : u == 2 ? kf4.z : kf4.w;
      const float* kp = rows + j * ldr;
      const float pr = __builtin_amdgcn_exp2f(dot<D>(q, kp) - l2);
      const float dp = dot<D>(g, kp + E) * kf;
      bits |= (kf != 0.f ? 1u : 0u) << j;
      axpy<D>(dq, pr * (dp - dl), kp);
    }
    store_row<D>(dqkv + row * ld_d + h * D, dq, a.scale);
    st_lse[tid] = l2;
    st_dl[tid] = dl;
    st_keep[tid] = bits;
  }
  __syncthreads();                               // every lane is done with K | V
  stage(sm, ldr, 0, base, a.ld, ns * T, E / 4, tid);
  stage(sm, ldr, E, dO + n0 * T * ld_do, ld_do, ns * T, E / 4, tid);
  __syncthreads();
  if (on) {                                      // pass 2: key row r
    float k[D], v[D], dk[D], dv[D];
    load_row<D>(k, a.qkv + row * a.ld + E + h * D, a.scale * kLog2e);
    load_row<D>(v, a.qkv + row * a.ld + 2 * E + h * D, 1.f);
#pragma unroll
    for (int d = 0; d < D; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
    const int t0 = tid - r;
#pragma unroll 1
    for (int i = 0; i < T; ++i) {
      const float* qp = rows + i * ldr;
      const float pr = __builtin_amdgcn_exp2f(dot<D>(k, qp) - st_lse[t0 + i]);
      const float kf = drop ? (((st_keep[t0 + i] >> r) & 1u) ? inv_keep : 0.f) : 1.f;
      const float dp = dot<D>(v, qp + E) * kf;
      axpy<D>(dv, pr * kf, qp + E);
      axpy<D>(dk, pr * (dp - st_dl[t0 + i]), qp);
    }
    store_row<D>(dqkv + row * ld_d + E + h * D, dk, a.scale);
    store_row<D>(dqkv + row * ld_d + 2 * E + h * D, dv, 1.f);
  }
}

// the keep factors as a dense [n_seq, heads, T, T] tensor (inspection and tests)
__global__ __launch_bounds__(256) void k_taskattn_keep(int64_t n_seq, int T, int heads, float p, const int64_t* __restrict__ rng, uint32_t call_id,
                                                       float* __restrict__ keep) {
  const int g4 = (T + 3) / 4;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= n_seq * heads * T * g4) return;
  const int g = static_cast<int>(idx % g4);
  const int64_t qrow = idx / g4;                 // (n heads + h) T + i
  const int i = static_cast<int>(qrow % T);
  const int64_t nh = qrow / T;
  float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
  if (p > 0.f)
    m = task_keep4(static_cast<uint64_t>(rng[0]), static_cast<uint64_t>(rng[1]), call_id, nh / heads, heads, static_cast<int>(nh % heads), i, g, p);
  float* dst = keep + qrow * T + 4 * g;
  dst[0] = m.x;
  if (4 * g + 1 < T) dst[1] = m.y;
  if (4 * g + 2 < T) dst[2] = m.z;
  if (4 * g + 3 < T) dst[3] = m.w;
}

constexpr int64_t kMaxSeq = 1 << 24;

int shape_check(const char* who, int64_t n_seq, int32_t T, int32_t heads, int32_t D, float p) {
  using namespace agnn;
  if (D != 8 && D != 16 && D != 32) return fail(AGNN_EINVAL, "%s: head width D=%d must be 8, 16 or 32", who, D);
  if (T < 1 || T > AGNN_MAX_SEG) return fail(AGNN_EINVAL, "%s: T=%d must be in [1, %d]", who, T, AGNN_MAX_SEG);
  if (heads < 1 || heads * D > 128 || heads * T > 256)
    return fail(AGNN_EINVAL, "%s: heads=%d must be at least 1 with heads * D <= 128 and heads * T <= 256 (D=%d, T=%d)", who, heads, D, T);
  if (n_seq < 0 || n_seq > kMaxSeq) return fail(AGNN_EINVAL, "%s: n_seq=%lld must be in [0, %lld]", who, (long long)n_seq, (long long)kMaxSeq);
  if (!(p >= 0.f && p < 1.f)) return fail(AGNN_EINVAL, "%s: dropout p=%f must be in [0, 1)", who, p);
  return 0;
}

int mat_check(const char* who, const char* name, const char* ld_name, const void* ptr, int64_t ld, int width) {
  using namespace agnn;
  if (!ptr) return fail(AGNN_EINVAL, "%s: %s is null", who, name);
  if (ld < width) return fail(AGNN_EINVAL, "%s: %s=%lld smaller than the %d columns of %s", who, ld_name, (long long)ld, width, name);
  if ((ld & 3) || !aligned16(ptr)) return fail(AGNN_EALIGN, "%s: rows of %s must be 16-byte aligned (%s=%lld)", who, name, ld_name, (long long)ld);
  return 0;
}

// sequences per workgroup: one lane per (sequence, head, row) of 256, as far as `extra` + the rows' LDS image fit
int seqs_per_block(int T, int heads, int D, size_t stat_bytes_per_lane, size_t* lds_bytes) {
  const size_t per_seq = static_cast<size_t>(T) * (2 * heads * D + 4) * sizeof(float) + stat_bytes_per_lane * heads * T;
  int S = kThreads / (heads * T);
  while (S > 1 && S * per_seq > static_cast<size_t>(kLdsBytes)) --S;
  *lds_bytes = S * per_seq;
  return S;
}

}  // namespace

#define AGNN_TASKATTN_DISPATCH(KERN, ...)                                                          \
  do {                                                                                             \
    if (D == 8) hipLaunchKernelGGL(KERN<8>, grid, dim3(kThreads), lds, s, __VA_ARGS__);            \
    else if (D == 16) hipLaunchKernelGGL(KERN<16>, grid, dim3(kThreads), lds, s, __VA_ARGS__);     \
    else hipLaunchKernelGGL(KERN<32>, grid, dim3(kThreads), lds, s, __VA_ARGS__);                  \
  } while (0)

extern "C" int agnn_taskattn_fwd_f32(const float* qkv, int64_t ld_qkv, int64_t n_seq, int32_t T, int32_t heads, int32_t D, float scale, float p,
                                     const int64_t* rng_state, uint32_t call_id, float* o, int64_t ld_o, float* lse, int64_t* rng_used,
                                     agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = shape_check("taskattn_fwd", n_seq, T, heads, D, p)) return rc;
  if (n_seq == 0) return AGNN_OK;
  const int E = heads * D;
  if (int rc = mat_check("taskattn_fwd", "qkv", "ld_qkv", qkv, ld_qkv, 3 * E)) return rc;
  if (int rc = mat_check("taskattn_fwd", "o", "ld_o", o, ld_o, E)) return rc;
  if (p > 0.f && !rng_state) return fail(AGNN_EINVAL, "taskattn_fwd: dropout needs the device rng_state");
  if (p > 0.f && !rng_used) return fail(AGNN_EINVAL, "taskattn_fwd: dropout needs rng_used to record what it drew from");
  size_t lds = 0;
  const int S = seqs_per_block(T, heads, D, 0, &lds);
  TaskAttnArgs a{qkv, ld_qkv, n_seq, T, heads, S, scale, p, p > 0.f ? rng_state : nullptr, call_id};
  const dim3 grid(static_cast<unsigned>((n_seq + S - 1) / S));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  AGNN_TASKATTN_DISPATCH(k_taskattn_fwd, a, o, ld_o, lse, p > 0.f ? rng_used : nullptr);
  return check_launch("taskattn_fwd");
}

extern "C" int agnn_taskattn_bwd_f32(const float* qkv, int64_t ld_qkv, int64_t n_seq, int32_t T, int32_t heads, int32_t D, float scale, float p,
                                     const int64_t* rng_used, uint32_t call_id, const float* dO, int64_t ld_do, const float* o, int64_t ld_o,
                                     const float* lse, float* dqkv, int64_t ld_dqkv, agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = shape_check("taskattn_bwd", n_seq, T, heads, D, p)) return rc;
  if (n_seq == 0) return AGNN_OK;
  const int E = heads * D;
  if (int rc = mat_check("taskattn_bwd", "qkv", "ld_qkv", qkv, ld_qkv, 3 * E)) return rc;
  if (int rc = mat_check("taskattn_bwd", "dO", "ld_do", dO, ld_do, E)) return rc;
  if (int rc = mat_check("taskattn_bwd", "o", "ld_o", o, ld_o, E)) return rc;
  if (int rc = mat_check("taskattn_bwd", "dqkv", "ld_dqkv", dqkv, ld_dqkv, 3 * E)) return rc;
  if (!lse) return fail(AGNN_EINVAL, "taskattn_bwd: lse is null");
  if (p > 0.f && !rng_used) return fail(AGNN_EINVAL, "taskattn_bwd: dropout needs the rng_used of the forward");
  size_t lds = 0;
  const int S = seqs_per_block(T, heads, D, 3 * sizeof(float), &lds);
  TaskAttnArgs a{qkv, ld_qkv, n_seq, T, heads, S, scale, p, p > 0.f ? rng_used : nullptr, call_id};
  const dim3 grid(static_cast<unsigned>((n_seq + S - 1) / S));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  AGNN_TASKATTN_DISPATCH(k_taskattn_bwd, a, dO, ld_do, o, ld_o, lse, dqkv, ld_dqkv);
  return check_launch("taskattn_bwd");
}

extern "C" int agnn_taskattn_dropout_keep_f32(int64_t n_seq, int32_t T, int32_t heads, float p, const int64_t* rng, uint32_t call_id, float* keep,
                                              agnn_stream_t stream_) {
  using namespace agnn;
  if (T < 1 || T > AGNN_MAX_SEG) return fail(AGNN_EINVAL, "taskattn_dropout_keep: T=%d must be in [1, %d]", T, AGNN_MAX_SEG);
  if (heads < 1 || heads * T > 256) return fail(AGNN_EINVAL, "taskattn_dropout_keep: heads=%d must be at least 1 with heads * T <= 256 (T=%d)", heads, T);
  if (n_seq < 0 || n_seq > kMaxSeq) return fail(AGNN_EINVAL, "taskattn_dropout_keep: n_seq=%lld must be in [0, %lld]", (long long)n_seq, (long long)kMaxSeq);
  if (!(p >= 0.f && p < 1.f)) return fail(AGNN_EINVAL, "taskattn_dropout_keep: dropout p=%f must be in [0, 1)", p);
  if (n_seq == 0) return AGNN_OK;
  if (!keep) return fail(AGNN_EINVAL, "taskattn_dropout_keep: keep is null");
  if (p > 0.f && !rng) return fail(AGNN_EINVAL, "taskattn_dropout_keep: dropout needs the rng state the forward used");
  const int64_t cnt = n_seq * heads * T * ((T + 3) / 4);
  hipLaunchKernelGGL(k_taskattn_keep, dim3(static_cast<unsigned>((cnt + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_), n_seq,
                     T, heads, p, rng, call_id, keep);
  return check_launch("taskattn_dropout_keep");
}
