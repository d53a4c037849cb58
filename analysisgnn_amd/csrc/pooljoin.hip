// The join of the cadence models (agnn_pool_norm_f32, agnn_pool_bwd_f32; ref: models/cadence.py:204-205 and :324-330):
//   x = torch_scatter.scatter_mean(x[src], dst, dim=0, out=x.clone());  x = LayerNorm(x)
// One wave per row on rowwave.h, H any multiple of 4 up to 1024.  Forward, one launch: the wave walks row i of the onset
// relation's by-destination CSR, adds the valid neighbours to x_i in CSR order, divides by the count and normalises what it holds;
// it writes the pooled row u (what the LayerNorm's backward reads), y, the two statistics and 1 / count.  The row and its column
// ids are wave-uniform and live on the scalar unit; neighbours are taken four at a time and all four gathers are issued before
// the first is waited for, which for the onset relation (0 .. 3 neighbours) is the whole row.  Backward of the pooling, one
// launch on the transposed index; the LayerNorm's own backward is agnn_norm_act_bwd_f32 on (u, mean, rstd).  Sums run in CSR
// order, no float atomics: two runs give the same bits.  Byte/latency-bound gather work: no MFMA on purpose.
//
// The statistics are centred twice: mean, deviations, the mean of the deviations taken off again, then the variance.  For a row
// of level 1e3 and spread 1e-2 a mean rounded in fp32 is off by a percent of the spread; the second pass removes that error to
// first order.
#include "rowwave.h"

namespace {

using namespace agnn;

typedef const __attribute__((address_space(4))) int32_t* k_i32p;
typedef const __attribute__((address_space(4))) float* k_f32p;

struct PoolNormArgs {
  const int32_t* rowptr;
  const int32_t* rowend;     // per-row ends of a trimmed index, or NULL
  const int32_t* col;
  const float* x;
  int64_t ld_x;
  int32_t n;
  int32_t pool_rows;
  int32_t H;
  int32_t col_limit;         // <= n (host)
  int32_t skip_self;
  float eps;
  const float* gamma;
  const float* beta;
  float* u;
  int64_t ld_u;
  float* y;
  int64_t ld_y;
  float* mean;
  float* rstd;
  float* inv_cnt;
};

__device__ __forceinline__ float f4_sum(const float4& v) { return (v.x + v.y) + (v.z + v.w); }

template <int CH>
__global__ __launch_bounds__(256) void k_pool_norm(PoolNormArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = wave_row<true>();
  if (row >= a.n) return;
  bool on[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) on[c] = chunk_on(c, lane, a.H);

  float4 acc[CH];
  const float* xp = a.x + static_cast<int64_t>(row) * a.ld_x;
#pragma unroll
  for (int c = 0; c < CH; ++c) acc[c] = chunk_load(xp, c, lane, on[c]);
  int cnt = 0;
  if (row < a.pool_rows) {
    const k_i32p col = (k_i32p)a.col;
    const int start = ((k_i32p)a.rowptr)[row];
    const int end = a.rowend != nullptr ? ((k_i32p)a.rowend)[row] : ((k_i32p)a.rowptr)[row + 1];
    for (int p = start; p < end; p += 4) {
      // the four ids are independent scalar loads (positions beyond the row's end repeat its last one): one round trip, not four
      int ck[4];
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) ck[k] = col[p + k < end ? p + k : end - 1];
      asm volatile("" ::"s"(ck[0]), "s"(ck[1]), "s"(ck[2]), "s"(ck[3]));     // all four before the first use (left alone, each sinks to it)
#pragma unroll
      for (int k = 0; k < 4; ++k) ok[k] = p + k < end && ck[k] >= 0 && ck[k] < a.col_limit && !(a.skip_self && ck[k] == row);
      float4 v[4][CH];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (ok[k]) {
          const float* sp = a.x + static_cast<int64_t>(ck[k]) * a.ld_x;
#pragma unroll
          for (int c = 0; c < CH; ++c) v[k][c] = chunk_load(sp, c, lane, on[c]);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (ok[k]) {
          ++cnt;
#pragma unroll
          for (int c = 0; c < CH; ++c) acc4(acc[c], v[k][c]);
        }
      }
    }
  }
  const float denom = static_cast<float>(cnt > 1 ? cnt : 1);
  float* up = a.u + static_cast<int64_t>(row) * a.ld_u;
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    f4_div(acc[c], denom);                    // a true division, as torch_scatter's; by 1 it is exact
    if (on[c]) chunk_store(up, c, lane, acc[c]);
    sum += f4_sum(acc[c]);                    // lanes outside the row hold zeros
  }
  const float invH = 1.f / static_cast<float>(a.H);
  const float m0 = wave_sum_dpp(sum) * invH;
  float dsum = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    acc[c] = on[c] ? make_float4(acc[c].x - m0, acc[c].y - m0, acc[c].z - m0, acc[c].w - m0) : f4_zero();
    dsum += f4_sum(acc[c]);
  }
  const float m1 = wave_sum_dpp(dsum) * invH;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    acc[c] = on[c] ? make_float4(acc[c].x - m1, acc[c].y - m1, acc[c].z - m1, acc[c].w - m1) : f4_zero();
    q += fmaf(acc[c].x, acc[c].x, acc[c].y * acc[c].y) + fmaf(acc[c].z, acc[c].z, acc[c].w * acc[c].w);
  }
  const float rs = 1.f / sqrtf(fmaf(wave_sum_dpp(q), invH, a.eps));
  if (lane == 0) {
    a.mean[row] = m0 + m1;
    a.rstd[row] = rs;
    a.inv_cnt[row] = 1.f / denom;
  }
  float* yp = a.y + static_cast<int64_t>(row) * a.ld_y;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (!on[c]) continue;
    const float4 g = chunk_load(a.gamma, c, lane, true), b = chunk_load(a.beta, c, lane, true);
    chunk_store(yp, c, lane, make_float4(fmaf(acc[c].x * rs, g.x, b.x), fmaf(acc[c].y * rs, g.y, b.y), fmaf(acc[c].z * rs, g.z, b.z),
                                         fmaf(acc[c].w * rs, g.w, b.w)));
  }
}

struct PoolBwdArgs {
  const int32_t* rowptr;     // the transposed (by-source) index
  const int32_t* rowend;
  const int32_t* col;
  const float* du;
  int64_t ld_du;
  const float* inv_cnt;
  int32_t n;
  int32_t pool_rows;
  int32_t H;
  int32_t col_limit;         // <= n (host): rows at or beyond it were nobody's neighbour
  int32_t skip_self;
  float* dx;
  int64_t ld_dx;
};

template <int CH>
__global__ __launch_bounds__(256) void k_pool_bwd(PoolBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = wave_row<true>();
  if (row >= a.n) return;
  bool on[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) on[c] = chunk_on(c, lane, a.H);
  const k_f32p inv = (k_f32p)a.inv_cnt;

  float4 acc[CH];
  const float* dp = a.du + static_cast<int64_t>(row) * a.ld_du;
  const float s = row < a.pool_rows ? inv[row] : 1.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    acc[c] = chunk_load(dp, c, lane, on[c]);
    f4_scale(acc[c], s);
  }
  if (row < a.col_limit) {
    const k_i32p col = (k_i32p)a.col;
    const int start = ((k_i32p)a.rowptr)[row];
    const int end = a.rowend != nullptr ? ((k_i32p)a.rowend)[row] : ((k_i32p)a.rowptr)[row + 1];
    for (int p = start; p < end; p += 4) {
      int ck[4];
      float wk[4];
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) ck[k] = col[p + k < end ? p + k : end - 1];
      asm volatile("" ::"s"(ck[0]), "s"(ck[1]), "s"(ck[2]), "s"(ck[3]));     // all four before the first use (left alone, each sinks to it)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ok[k] = p + k < end && ck[k] >= 0 && ck[k] < a.pool_rows && !(a.skip_self && ck[k] == row);
        wk[k] = inv[ok[k] ? ck[k] : row];           // in bounds either way; a dropped edge's weight is not used
      }
      float4 v[4][CH];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (ok[k]) {
          const float* sp = a.du + static_cast<int64_t>(ck[k]) * a.ld_du;
#pragma unroll
          for (int c = 0; c < CH; ++c) v[k][c] = chunk_load(sp, c, lane, on[c]);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (ok[k]) {
#pragma unroll
          for (int c = 0; c < CH; ++c) f4_fma(acc[c], wk[k], v[k][c]);
        }
      }
    }
  }
  float* op = a.dx + static_cast<int64_t>(row) * a.ld_dx;
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (on[c]) chunk_store(op, c, lane, acc[c]);
}

// what both entry points ask of their sizes and of the index; 1: no row, nothing to do
int pool_check(const char* who, const agnn_rel_t* rel, int64_t n, int64_t pool_rows, int32_t H, int32_t col_limit, uint32_t flags) {
  if (int rc = check_wave_rows(who, n, H)) return rc;
  if (pool_rows < 1 || pool_rows > n) return fail(AGNN_EINVAL, "%s: pool_rows=%lld not in [1, n=%lld]", who, (long long)pool_rows, (long long)n);
  if (col_limit < 0) return fail(AGNN_EINVAL, "%s: col_limit=%d", who, col_limit);
  if (flags & ~AGNN_SPMM_SKIP_SELF) return fail(AGNN_EINVAL, "%s: flags 0x%x (AGNN_SPMM_SKIP_SELF is the only one)", who, flags);
  if (!rel || !rel->rowptr || !rel->col) return fail(AGNN_EINVAL, "%s: null index", who);
  if (rel->ew != nullptr) return fail(AGNN_EINVAL, "%s: per-edge weights are not supported", who);
  return AGNN_OK;
}

}  // namespace

extern "C" int agnn_pool_norm_f32(const agnn_rel_t* rel, const float* x, int64_t ld_x, int64_t n, int64_t pool_rows, int32_t H,
                                  int32_t col_limit, uint32_t flags, const float* gamma, const float* beta, float eps, float* u,
                                  int64_t ld_u, float* y, int64_t ld_y, float* mean, float* rstd, float* inv_cnt, agnn_stream_t stream_) {
  const char* who = "pool_norm";
  if (int rc = pool_check(who, rel, n, pool_rows, H, col_limit, flags)) return rc > 0 ? AGNN_OK : rc;
  if (int rc = check_matrix(who, "x", x, ld_x, H)) return rc;
  if (int rc = check_matrix(who, "u", u, ld_u, H)) return rc;
  if (int rc = check_matrix(who, "y", y, ld_y, H)) return rc;
  if (!gamma || !beta || !mean || !rstd || !inv_cnt) return fail(AGNN_EINVAL, "%s: gamma, beta, mean, rstd or inv_cnt is null", who);
  if (!aligned16(gamma) || !aligned16(beta)) return fail(AGNN_EALIGN, "%s: gamma and beta must be 16-byte aligned", who);
  if (u == x || y == x) return fail(AGNN_EINVAL, "%s: u and y must not be x (other rows still read it)", who);
  PoolNormArgs a{rel->rowptr, rel->rowend, rel->col, x, ld_x, static_cast<int32_t>(n), static_cast<int32_t>(pool_rows), H,
                 static_cast<int32_t>(col_limit < n ? col_limit : n), (flags & AGNN_SPMM_SKIP_SELF) ? 1 : 0, eps, gamma, beta, u, ld_u, y, ld_y,
                 mean, rstd, inv_cnt};
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  for_width(H, [&](auto ch) { hipLaunchKernelGGL((k_pool_norm<decltype(ch)::value>), dim3(grid_for(n)), dim3(256), 0, stream, a); });
  return check_launch(who);
}

extern "C" int agnn_pool_bwd_f32(const agnn_rel_t* rel_t, const float* du, int64_t ld_du, const float* inv_cnt, int64_t n,
                                 int64_t pool_rows, int32_t H, int32_t col_limit, uint32_t flags, float* dx, int64_t ld_dx,
                                 agnn_stream_t stream_) {
  const char* who = "pool_bwd";
  if (int rc = pool_check(who, rel_t, n, pool_rows, H, col_limit, flags)) return rc > 0 ? AGNN_OK : rc;
  if (int rc = check_matrix(who, "du", du, ld_du, H)) return rc;
  if (int rc = check_matrix(who, "dx", dx, ld_dx, H)) return rc;
  if (!inv_cnt) return fail(AGNN_EINVAL, "%s: inv_cnt is null", who);
  if (dx == du) return fail(AGNN_EINVAL, "%s: dx must not be du (other rows still read it)", who);
  PoolBwdArgs a{rel_t->rowptr, rel_t->rowend, rel_t->col, du, ld_du, inv_cnt, static_cast<int32_t>(n), static_cast<int32_t>(pool_rows), H,
                static_cast<int32_t>(col_limit < n ? col_limit : n), (flags & AGNN_SPMM_SKIP_SELF) ? 1 : 0, dx, ld_dx};
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  for_width(H, [&](auto ch) { hipLaunchKernelGGL((k_pool_bwd<decltype(ch)::value>), dim3(grid_for(n)), dim3(256), 0, stream, a); });
  return check_launch(who);
}
