// y = dropout_p( BatchNorm1d( act(x) ) ) over the ROWS of a [n, C] fp32 matrix, forward and backward (agnn_colnorm_*).
//
// The reference's chord models normalise over the row axis: `layernorm1/2` of MetricalChordEncoder are BatchNorm1d
// (models/chord.py:539-541, :569-570) and every task head is Linear -> act -> BatchNorm1d -> Dropout -> Linear (core/mlp.py:27-35).
// The statistics are per COLUMN, so the T heads' hidden layers, stacked side by side as [n, T * hidden], are one call.
// Geometry: a workgroup owns a slab of kSlab rows x 64 columns; 16 lanes run along the columns with one float4 each (a 256-byte
// piece of a row per row of lanes), 16 lanes run down the rows, so a thread holds kSlab / 16 = 8 float4 in registers.
// Training statistics: every thread reduces its 8 values of d = act(x) - K (K = act(x[0, column]), the shift) to (count, mean,
// M2) in two passes over its registers; the 16 row lanes' triples are joined pairwise in row-lane order (Chan, Golub, LeVeque
// 1979), the slab's (mean, M2) go to the workspace, and a final pass joins the slabs in slab order.  E[a^2] - mean^2 is never
// formed, and the mean is kept as hi + lo (hi = fl(K + mean_d)) so that (a - hi) - lo stays exact for |mean| >> std.
// Backward: slabs leave partial sums of g and g * xhat, a second launch adds them in slab order (the scheme of
// agnn_norm_act_colsum_f32), a third writes dx.  HBM-bound; no float atomics.
#include <cmath>

#include "agnn_common.h"

namespace {

constexpr int kSlab = AGNN_CN_SLAB;          // rows per workgroup
constexpr int kRowLanes = 16;                // lanes down the rows
constexpr int kPer = kSlab / kRowLanes;      // rows per thread
constexpr int kTileC = 64;                   // columns per workgroup (16 float4 lanes)
constexpr int kFinalLanes = AGNN_CN_FINAL_LANES;   // lanes per column of the final passes
static_assert(kPer * kRowLanes == kSlab && kRowLanes * (kTileC / 4) == 256, "tile geometry");

struct CnArgs {
  const float* x;
  int64_t ld_x;
  int64_t n;
  int32_t C;
  float p;
  uint32_t flags;
  const int64_t* rng;
  uint32_t call_id;
};

__device__ __forceinline__ float4 ldf4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void stf4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 act4(float4 v, bool relu) {
  return relu ? make_float4(agnn::relu_nan(v.x), agnn::relu_nan(v.y), agnn::relu_nan(v.z), agnn::relu_nan(v.w)) : v;
}
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// (nA, mA, qA) <- (nA, mA, qA) joined with (nB, mB, qB); q = sum of squared deviations.  An empty side changes nothing.
__device__ __forceinline__ void chan(float& nA, float& mA, float& qA, float nB, float mB, float qB) {
  if (nB == 0.f) return;
  if (nA == 0.f) { nA = nB; mA = mB; qA = qB; return; }
  const float n = nA + nB, d = mB - mA, f = nB / n;
  mA = fmaf(d, f, mA);
  qA = (qA + qB) + d * d * (nA * f);
  nA = n;
}
__device__ __forceinline__ void chan4(float& nA, float4& mA, float4& qA, float nB, const float4& mB, const float4& qB) {
  float n0 = nA, n1 = nA, n2 = nA, n3 = nA;
  chan(n0, mA.x, qA.x, nB, mB.x, qB.x);
  chan(n1, mA.y, qA.y, nB, mB.y, qB.y);
  chan(n2, mA.z, qA.z, nB, mB.z, qB.z);
  chan(n3, mA.w, qA.w, nB, mB.w, qB.w);
  nA = n0;
}

__device__ __forceinline__ float4 cn_keep(const CnArgs& a, int64_t row, int c, float scale) {
  const uint64_t idx = static_cast<uint64_t>(row) * static_cast<uint32_t>(a.C >> 2) + static_cast<uint32_t>(c >> 2);   // one counter per float4
  return agnn::keep_factors(agnn::stream_bits(static_cast<uint64_t>(a.rng[0]), static_cast<uint64_t>(a.rng[1]), a.call_id, idx),
                            agnn::drop_threshold(a.p), scale);
}

// part[slab][0 | 1][C] = mean | M2 of d = act(x) - K over the slab's rows
__global__ __launch_bounds__(256) void k_cn_stats(CnArgs a, float* __restrict__ part) {
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = static_cast<int>(blockIdx.y) * kTileC + cl * 4;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kSlab;
  const bool on = c < a.C, relu = a.flags & AGNN_CN_RELU;
  const float4 K = on ? act4(ldf4(a.x + c), relu) : agnn::f4_zero();
  float4 v[kPer];
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int64_t row = r0 + rl + kRowLanes * i;
    const bool live = row < a.n;
    v[i] = (live && on) ? sub4(act4(ldf4(a.x + row * a.ld_x + c), relu), K) : agnn::f4_zero();
    cnt += live ? 1 : 0;
  }
  float4 s = agnn::f4_zero();
#pragma unroll
  for (int i = 0; i < kPer; ++i) s = add4(s, v[i]);                 // rows past the end hold zeros
  const float fc = static_cast<float>(cnt), inv = cnt > 0 ? 1.f / fc : 0.f;
  float4 m = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv), q = agnn::f4_zero();
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    if (i < cnt) {
      const float4 d = sub4(v[i], m);
      q = make_float4(fmaf(d.x, d.x, q.x), fmaf(d.y, d.y, q.y), fmaf(d.z, d.z, q.z), fmaf(d.w, d.w, q.w));
    }
  }
  __shared__ float4 sm_m[256], sm_q[256];
  __shared__ float sm_n[kRowLanes];
  sm_m[threadIdx.x] = m;
  sm_q[threadIdx.x] = q;
  if (cl == 0) sm_n[rl] = fc;
  __syncthreads();
  if (rl == 0 && on) {
    float n = fc;
    for (int r = 1; r < kRowLanes; ++r) chan4(n, m, q, sm_n[r], sm_m[r * 16 + cl], sm_q[r * 16 + cl]);      // row-lane order
    float* pp = part + static_cast<int64_t>(blockIdx.x) * 2 * a.C;
    stf4(pp + c, m);
    stf4(pp + a.C + c, q);
  }
}

// joins the S slabs' triples of a column (16 lanes take slabs l, l + 16, ... in order, then lane order); stats, running statistics
__global__ __launch_bounds__(256) void k_cn_final(CnArgs a, const float* __restrict__ part, int S, float eps, float momentum,
                                                  float* __restrict__ stats, float* __restrict__ rmean, float* __restrict__ rvar,
                                                  int64_t* __restrict__ nbt) {
  const int cl = threadIdx.x & 15, ln = threadIdx.x >> 4;
  const int j = static_cast<int>(blockIdx.x) * 16 + cl;
  float n = 0.f, m = 0.f, q = 0.f;
  if (j < a.C) {
    for (int s = ln; s < S; s += kFinalLanes) {
      const int64_t left = a.n - static_cast<int64_t>(s) * kSlab;
      const float ns = static_cast<float>(left < kSlab ? left : kSlab);
      const float* pp = part + static_cast<int64_t>(s) * 2 * a.C;
      chan(n, m, q, ns, pp[j], pp[a.C + j]);
    }
  }
  __shared__ float sn[256], smm[256], sq[256];
  sn[threadIdx.x] = n;
  smm[threadIdx.x] = m;
  sq[threadIdx.x] = q;
  __syncthreads();
  if (ln == 0 && j < a.C) {
    for (int l = 1; l < kFinalLanes; ++l) chan(n, m, q, sn[l * 16 + cl], smm[l * 16 + cl], sq[l * 16 + cl]);
    const float k = (a.flags & AGNN_CN_RELU) ? agnn::relu_nan(a.x[j]) : a.x[j];
    const float hi = k + m;                              // the mean, as hi + lo
    const float lo = (k - hi) + m;                       // exact remainder of the sum when |k| >= |m|; otherwise small against std anyway
    const float fn = static_cast<float>(a.n);
    stats[j] = hi;
    stats[a.C + j] = lo;
    stats[2 * a.C + j] = 1.f / sqrtf(q / fn + eps);
    if (rmean != nullptr) {
      rmean[j] = (1.f - momentum) * rmean[j] + momentum * hi;
      rvar[j] = (1.f - momentum) * rvar[j] + momentum * (q / (fn - 1.f));
    }
  }
  if (nbt != nullptr && blockIdx.x == 0 && threadIdx.x == 0) nbt[0] += 1;
}

// y = dropout(gamma * xhat + beta).  STATS: hi / lo / rstd from stats (training); otherwise from the running statistics, which
// the first slab row of workgroups also copies into stats for backward.
template <bool TRAIN>
__global__ __launch_bounds__(256) void k_cn_apply(CnArgs a, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  float* __restrict__ stats, const float* __restrict__ rmean, const float* __restrict__ rvar,
                                                  float eps, float* __restrict__ y, int64_t ld_y, int64_t* __restrict__ rng_used) {
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = static_cast<int>(blockIdx.y) * kTileC + cl * 4;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kSlab;
  if (rng_used != nullptr && a.rng != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    rng_used[0] = a.rng[0];
    rng_used[1] = a.rng[1];
  }
  if (c >= a.C) return;
  const bool relu = a.flags & AGNN_CN_RELU, drop = a.p > 0.f;
  float4 hi, lo, rs;
  if (TRAIN) {
    hi = ldf4(stats + c);
    lo = ldf4(stats + a.C + c);
    rs = ldf4(stats + 2 * a.C + c);
  } else {
    hi = ldf4(rmean + c);
    lo = agnn::f4_zero();
    const float4 v = ldf4(rvar + c);
    rs = make_float4(1.f / sqrtf(v.x + eps), 1.f / sqrtf(v.y + eps), 1.f / sqrtf(v.z + eps), 1.f / sqrtf(v.w + eps));
    if (stats != nullptr && blockIdx.x == 0 && rl == 0) {
      stf4(stats + c, hi);
      stf4(stats + a.C + c, lo);
      stf4(stats + 2 * a.C + c, rs);
    }
  }
  const float4 g = ldf4(gamma + c), b = ldf4(beta + c);
  const float scale = drop ? 1.f / (1.f - a.p) : 1.f;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int64_t row = r0 + rl + kRowLanes * i;
    if (row >= a.n) break;
    const float4 v = sub4(sub4(act4(ldf4(a.x + row * a.ld_x + c), relu), hi), lo);
    float4 o = make_float4(fmaf(v.x * rs.x, g.x, b.x), fmaf(v.y * rs.y, g.y, b.y), fmaf(v.z * rs.z, g.z, b.z), fmaf(v.w * rs.w, g.w, b.w));
    if (drop) {
      const float4 k = cn_keep(a, row, c, scale);
      o.x *= k.x; o.y *= k.y; o.z *= k.z; o.w *= k.w;
    }
    stf4(y + row * ld_y + c, o);
  }
}

// part[slab][0 | 1][C] = sum g * xhat | sum g over the slab's rows, g = dy * dropout factor
__global__ __launch_bounds__(256) void k_cn_bwd_sums(CnArgs a, const float* __restrict__ stats, const float* __restrict__ dy, int64_t ld_dy,
                                                     float* __restrict__ part) {
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = static_cast<int>(blockIdx.y) * kTileC + cl * 4;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kSlab;
  const bool on = c < a.C, relu = a.flags & AGNN_CN_RELU, drop = a.p > 0.f;
  const float scale = drop ? 1.f / (1.f - a.p) : 1.f;
  float4 s1 = agnn::f4_zero(), s2 = agnn::f4_zero();
  if (on) {
    const float4 hi = ldf4(stats + c), lo = ldf4(stats + a.C + c), rs = ldf4(stats + 2 * a.C + c);
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int64_t row = r0 + rl + kRowLanes * i;
      if (row >= a.n) break;
      const float4 v = sub4(sub4(act4(ldf4(a.x + row * a.ld_x + c), relu), hi), lo);
      float4 g = ldf4(dy + row * ld_dy + c);
      if (drop) {
        const float4 k = cn_keep(a, row, c, scale);
        g.x *= k.x; g.y *= k.y; g.z *= k.z; g.w *= k.w;
      }
      s1 = make_float4(fmaf(g.x, v.x * rs.x, s1.x), fmaf(g.y, v.y * rs.y, s1.y), fmaf(g.z, v.z * rs.z, s1.z), fmaf(g.w, v.w * rs.w, s1.w));
      s2 = add4(s2, g);
    }
  }
  __shared__ float4 sm1[256], sm2[256];
  sm1[threadIdx.x] = s1;
  sm2[threadIdx.x] = s2;
  __syncthreads();
  if (rl == 0 && on) {
    for (int r = 1; r < kRowLanes; ++r) {                              // row-lane order
      s1 = add4(s1, sm1[r * 16 + cl]);
      s2 = add4(s2, sm2[r * 16 + cl]);
    }
    float* pp = part + static_cast<int64_t>(blockIdx.x) * 2 * a.C;
    stf4(pp + c, s1);
    stf4(pp + a.C + c, s2);
  }
}

// dgamma[j] | dbeta[j] = sum over slabs of part[s][0 | 1][j], lanes l take slabs l, l + 16, ... in order, then lane order
__global__ __launch_bounds__(256) void k_cn_colsum(const float* __restrict__ part, int S, int C, float* __restrict__ dgamma,
                                                   float* __restrict__ dbeta) {
  const int cl = threadIdx.x & 15, ln = threadIdx.x >> 4;
  const int j = static_cast<int>(blockIdx.x) * 16 + cl;
  float t1 = 0.f, t2 = 0.f;
  if (j < C) {
    for (int s = ln; s < S; s += kFinalLanes) {
      const float* pp = part + static_cast<int64_t>(s) * 2 * C;
      t1 += pp[j];
      t2 += pp[C + j];
    }
  }
  __shared__ float s1[256], s2[256];
  s1[threadIdx.x] = t1;
  s2[threadIdx.x] = t2;
  __syncthreads();
  if (ln == 0 && j < C) {
    for (int l = 1; l < kFinalLanes; ++l) {
      t1 += s1[l * 16 + cl];
      t2 += s2[l * 16 + cl];
    }
    dgamma[j] = t1;
    dbeta[j] = t2;
  }
}

__global__ __launch_bounds__(256) void k_cn_bwd_apply(CnArgs a, const float* __restrict__ gamma, const float* __restrict__ stats,
                                                      const float* __restrict__ dy, int64_t ld_dy, const float* __restrict__ dgamma,
                                                      const float* __restrict__ dbeta, float* __restrict__ dx, int64_t ld_dx) {
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = static_cast<int>(blockIdx.y) * kTileC + cl * 4;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kSlab;
  if (c >= a.C) return;
  const bool relu = a.flags & AGNN_CN_RELU, drop = a.p > 0.f, train = a.flags & AGNN_CN_TRAIN;
  const float scale = drop ? 1.f / (1.f - a.p) : 1.f;
  const float4 hi = ldf4(stats + c), lo = ldf4(stats + a.C + c), rs = ldf4(stats + 2 * a.C + c), gm = ldf4(gamma + c);
  const float invn = train ? 1.f / static_cast<float>(a.n) : 0.f;
  const float4 dg = ldf4(dgamma + c), db = ldf4(dbeta + c);
  const float4 m1 = make_float4(db.x * invn, db.y * invn, db.z * invn, db.w * invn);       // mean of g
  const float4 m2 = make_float4(dg.x * invn, dg.y * invn, dg.z * invn, dg.w * invn);       // mean of g * xhat
  const float4 w = make_float4(gm.x * rs.x, gm.y * rs.y, gm.z * rs.z, gm.w * rs.w);
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int64_t row = r0 + rl + kRowLanes * i;
    if (row >= a.n) break;
    const float4 xr = ldf4(a.x + row * a.ld_x + c);
    const float4 v = sub4(sub4(act4(xr, relu), hi), lo);
    float4 g = ldf4(dy + row * ld_dy + c);
    if (drop) {
      const float4 k = cn_keep(a, row, c, scale);
      g.x *= k.x; g.y *= k.y; g.z *= k.z; g.w *= k.w;
    }
    float4 o = make_float4(w.x * ((g.x - m1.x) - v.x * rs.x * m2.x), w.y * ((g.y - m1.y) - v.y * rs.y * m2.y),
                           w.z * ((g.z - m1.z) - v.z * rs.z * m2.z), w.w * ((g.w - m1.w) - v.w * rs.w * m2.w));
    if (relu) {
      if (xr.x <= 0.f) o.x = 0.f;
      if (xr.y <= 0.f) o.y = 0.f;
      if (xr.z <= 0.f) o.z = 0.f;
      if (xr.w <= 0.f) o.w = 0.f;
    }
    stf4(dx + row * ld_dx + c, o);
  }
}

inline int64_t slabs_of(int64_t n) { return n > 0 ? (n + kSlab - 1) / kSlab : 0; }

// 1: empty work (success), 0: go on, < 0: refused
int cn_check(const char* who, const void* x, int64_t ld_x, int64_t n, int32_t C, float p, const void* rng) {
  using namespace agnn;
  if (C < 4 || (C & 3)) return fail(AGNN_EINVAL, "%s: C=%d must be a multiple of 4, at least 4", who, C);
  if (n < 0) return fail(AGNN_EINVAL, "%s: n=%lld must not be negative", who, (long long)n);
  if (slabs_of(n) > INT32_MAX) return fail(AGNN_EINVAL, "%s: n=%lld: more than 2^31 - 1 slabs", who, (long long)n);
  if (!(p >= 0.f && p < 1.f)) return fail(AGNN_EINVAL, "%s: dropout p=%f must be in [0, 1)", who, p);
  if (n == 0) return 1;
  if (!x) return fail(AGNN_EINVAL, "%s: x is null", who);
  if (ld_x < C) return fail(AGNN_EINVAL, "%s: ld_x=%lld < C=%d", who, (long long)ld_x, C);
  if (ld_x & 3) return fail(AGNN_EALIGN, "%s: ld_x=%lld is not a multiple of 4", who, (long long)ld_x);
  if (!aligned16(x)) return fail(AGNN_EALIGN, "%s: x is not 16-byte aligned", who);
  if (p > 0.f && !rng) return fail(AGNN_EINVAL, "%s: dropout needs the device rng_state", who);
  return 0;
}

int cn_rows(const char* who, const char* name, const void* ptr, int64_t ld, int32_t C) {
  using namespace agnn;
  if (!ptr) return fail(AGNN_EINVAL, "%s: %s is null", who, name);
  if (ld < C) return fail(AGNN_EINVAL, "%s: ld_%s=%lld < C=%d", who, name, (long long)ld, C);
  if (ld & 3) return fail(AGNN_EALIGN, "%s: ld_%s=%lld is not a multiple of 4", who, name, (long long)ld);
  if (!aligned16(ptr)) return fail(AGNN_EALIGN, "%s: %s is not 16-byte aligned", who, name);
  return AGNN_OK;
}

int cn_vec(const char* who, const char* name, const void* ptr) {
  using namespace agnn;
  if (!ptr) return fail(AGNN_EINVAL, "%s: %s is null", who, name);
  if (!aligned16(ptr)) return fail(AGNN_EALIGN, "%s: %s is not 16-byte aligned", who, name);
  return AGNN_OK;
}

int cn_workspace(const char* who, const void* ws, size_t bytes, size_t need) {
  using namespace agnn;
  if (!ws) return fail(AGNN_EINVAL, "%s: workspace is null", who);
  if (bytes < need) return fail(AGNN_ENOMEM, "%s: workspace of %zu bytes, %zu needed", who, bytes, need);
  if (!aligned16(ws)) return fail(AGNN_EALIGN, "%s: workspace is not 16-byte aligned", who);
  return AGNN_OK;
}

}  // namespace

extern "C" size_t agnn_colnorm_workspace_bytes(int64_t n, int32_t C) {
  if (n <= 0 || C <= 0) return 0;
  return static_cast<size_t>(slabs_of(n)) * 2 * static_cast<size_t>(C) * sizeof(float);
}

extern "C" int agnn_colnorm_fwd_f32(const float* x, int64_t ld_x, int64_t n, int32_t C, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, int64_t* num_batches_tracked, float eps, float momentum,
                                    float p, uint32_t flags, const int64_t* rng_state, uint32_t call_id, float* y, int64_t ld_y,
                                    float* stats, int64_t* rng_used, void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  const char* who = "colnorm_fwd";
  if (int rc = cn_check(who, x, ld_x, n, C, p, rng_state)) return rc > 0 ? AGNN_OK : rc;
  const bool train = flags & AGNN_CN_TRAIN;
  if (flags & ~static_cast<uint32_t>(AGNN_CN_RELU | AGNN_CN_TRAIN)) return fail(AGNN_EINVAL, "%s: unknown flags %u", who, flags);
  if (!(eps >= 0.f)) return fail(AGNN_EINVAL, "%s: eps=%f", who, eps);
  if (train && n == 1) return fail(AGNN_EINVAL, "%s: n=1: batch statistics need more than one row", who);
  if (int rc = cn_vec(who, "gamma", gamma)) return rc;
  if (int rc = cn_vec(who, "beta", beta)) return rc;
  if (int rc = cn_rows(who, "y", y, ld_y, C)) return rc;
  const bool has_run = running_mean || running_var || num_batches_tracked;
  if (has_run && !(running_mean && running_var)) return fail(AGNN_EINVAL, "%s: running_mean and running_var go together", who);
  if (!train && !has_run) return fail(AGNN_EINVAL, "%s: running statistics are null without AGNN_CN_TRAIN", who);
  if (has_run) {
    if (int rc = cn_vec(who, "running_mean", running_mean)) return rc;
    if (int rc = cn_vec(who, "running_var", running_var)) return rc;
  }
  if (train || stats) {
    if (int rc = cn_vec(who, "stats", stats)) return rc;
  }
  if (train) {
    if (!(momentum >= 0.f && momentum <= 1.f)) return fail(AGNN_EINVAL, "%s: momentum=%f must be in [0, 1]", who, momentum);
    if (int rc = cn_workspace(who, workspace, workspace_bytes, agnn_colnorm_workspace_bytes(n, C))) return rc;
  }
  CnArgs a{x, ld_x, n, C, p, flags, rng_state, call_id};
  hipStream_t s = static_cast<hipStream_t>(stream_);
  const int S = static_cast<int>(slabs_of(n));
  const dim3 grid(static_cast<unsigned>(S), static_cast<unsigned>((C + kTileC - 1) / kTileC)), block(256);
  if (grid.y > 65535u) return fail(AGNN_EINVAL, "%s: C=%d: more than 65535 column tiles", who, C);
  if (train) {
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(k_cn_stats, grid, block, 0, s, a, part);
    hipLaunchKernelGGL(k_cn_final, dim3((C + 15) / 16), block, 0, s, a, part, S, eps, momentum, stats, running_mean, running_var,
                       num_batches_tracked);
    hipLaunchKernelGGL(k_cn_apply<true>, grid, block, 0, s, a, gamma, beta, stats, nullptr, nullptr, eps, y, ld_y, rng_used);
  } else {
    hipLaunchKernelGGL(k_cn_apply<false>, grid, block, 0, s, a, gamma, beta, stats, running_mean, running_var, eps, y, ld_y, rng_used);
  }
  return check_launch(who);
}

extern "C" int agnn_colnorm_bwd_f32(const float* x, int64_t ld_x, int64_t n, int32_t C, const float* gamma, const float* stats, float p,
                                    uint32_t flags, const int64_t* rng_state, uint32_t call_id, const float* dy, int64_t ld_dy,
                                    float* dx, int64_t ld_dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                    agnn_stream_t stream_) {
  using namespace agnn;
  const char* who = "colnorm_bwd";
  if (int rc = cn_check(who, x, ld_x, n, C, p, rng_state)) return rc > 0 ? AGNN_OK : rc;
  if (flags & ~static_cast<uint32_t>(AGNN_CN_RELU | AGNN_CN_TRAIN)) return fail(AGNN_EINVAL, "%s: unknown flags %u", who, flags);
  if ((flags & AGNN_CN_TRAIN) && n == 1) return fail(AGNN_EINVAL, "%s: n=1: batch statistics need more than one row", who);
  if (int rc = cn_vec(who, "gamma", gamma)) return rc;
  if (int rc = cn_vec(who, "stats", stats)) return rc;
  if (int rc = cn_rows(who, "dy", dy, ld_dy, C)) return rc;
  if (int rc = cn_rows(who, "dx", dx, ld_dx, C)) return rc;
  if (int rc = cn_vec(who, "dgamma", dgamma)) return rc;
  if (int rc = cn_vec(who, "dbeta", dbeta)) return rc;
  if (int rc = cn_workspace(who, workspace, workspace_bytes, agnn_colnorm_workspace_bytes(n, C))) return rc;
  CnArgs a{x, ld_x, n, C, p, flags, rng_state, call_id};
  hipStream_t s = static_cast<hipStream_t>(stream_);
  const int S = static_cast<int>(slabs_of(n));
  const dim3 grid(static_cast<unsigned>(S), static_cast<unsigned>((C + kTileC - 1) / kTileC)), block(256);
  if (grid.y > 65535u) return fail(AGNN_EINVAL, "%s: C=%d: more than 65535 column tiles", who, C);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(k_cn_bwd_sums, grid, block, 0, s, a, stats, dy, ld_dy, part);
  hipLaunchKernelGGL(k_cn_colsum, dim3((C + 15) / 16), block, 0, s, part, S, C, dgamma, dbeta);
  hipLaunchKernelGGL(k_cn_bwd_apply, grid, block, 0, s, a, gamma, stats, dy, ld_dy, dgamma, dbeta, dx, ld_dx);
  return check_launch(who);
}
