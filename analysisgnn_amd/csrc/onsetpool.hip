// Onset pooling with row selection (agnn_onset_pool_*): the reference's OnsetEdgePoolingVersion2 (models/chord.py:284-287) is
//   h = scatter(trans(x)[cat(src, arange(n))], cat(dst, arange(n)), out=zeros, reduce='mean');  out = h[idx]
// a gather of E + n rows, a scatter over all n notes, and a second gather that keeps one row per distinct onset.  Here only the
// selected rows are computed, from the CSR by destination: a group of G = 4 .. 64 lanes (peredge.h's lane geometry) owns a
// selected row, reads the row itself and its in-neighbours with float4 loads in CSR order and writes the mean once.  The
// weights of a mean sum to one, so the Linear `trans` commutes with it and is applied by the caller to the n_sel pooled rows.
// Backward, one launch: a group owns a row j of da and walks j itself and j's out-edges (CSR by source); each visited node r
// contributes w(r) * sum of g[k] over the k with idx[k] == r (the CSR of idx by node), w(r) = 1 / (1 + indeg(r)).  Unselected
// destinations have an empty list and contribute nothing.  Fixed order, no atomics on floats.
#include "peredge.h"

namespace {

struct PoolFwd {
  const float* a;
  int64_t ld_a;
  int64_t n;
  int32_t H4;
  const int32_t* rowptr;
  const int32_t* col;
  const int64_t* idx;
  int64_t n_sel;
  float* out;
  int64_t ld_out;
  int32_t* status;
};

__global__ __launch_bounds__(256) void k_pool_fwd(PoolFwd p, int lg) {
  const agnn::Lanes L = agnn::lanes_of(lg);
  const int64_t k = static_cast<int64_t>(blockIdx.x) * L.gpb + L.grp;
  if (k >= p.n_sel) return;
  const int64_t r = p.idx[k];
  float* op = p.out + k * p.ld_out;
  if (r < 0 || r >= p.n) {                                     // nothing is read; the row is zeros
    for (int c4 = L.lig; c4 < p.H4; c4 += L.G) reinterpret_cast<float4*>(op)[c4] = agnn::f4_zero();
    if (L.lig == 0 && p.status != nullptr) atomicAdd(p.status, 1);
    return;
  }
  const int e0 = p.rowptr[r], e1 = p.rowptr[r + 1];
  int bad = 0;
  for (int c4 = L.lig; c4 < p.H4; c4 += L.G) {
    float4 s = reinterpret_cast<const float4*>(p.a + r * p.ld_a)[c4];            // the appended self loop
    int deg = 0;
    for (int e = e0; e < e1; ++e) {
      const int j = p.col[e];
      if (j < 0 || j >= p.n) { ++bad; continue; }
      agnn::acc4(s, reinterpret_cast<const float4*>(p.a + static_cast<int64_t>(j) * p.ld_a)[c4]);
      ++deg;
    }
    const float w = 1.f / static_cast<float>(1 + deg);
    agnn::f4_scale(s, w);
    reinterpret_cast<float4*>(op)[c4] = s;
  }
  if (L.lig == 0 && bad && p.status != nullptr) atomicAdd(p.status, 1);
}

struct PoolBwd {
  const float* g;
  int64_t ld_g;
  int64_t n_sel;
  int32_t H4;
  int64_t n;
  const int32_t* d_rowptr;
  const int32_t* s_rowptr;
  const int32_t* s_col;
  const int32_t* sel_rowptr;
  const int32_t* sel_k;
  float* da;
  int64_t ld_da;
};

// s += w(r) * sum_{k : idx[k] == r} g[k, c4]
__device__ __forceinline__ void add_node(const PoolBwd& p, int64_t r, int c4, float4& s) {
  const int k0 = p.sel_rowptr[r], k1 = p.sel_rowptr[r + 1];
  if (k0 >= k1) return;
  float4 t = agnn::f4_zero();
  for (int q = k0; q < k1; ++q) {
    const int k = p.sel_k[q];
    if (k < 0 || k >= p.n_sel) continue;
    agnn::acc4(t, reinterpret_cast<const float4*>(p.g + static_cast<int64_t>(k) * p.ld_g)[c4]);
  }
  const float w = 1.f / static_cast<float>(1 + (p.d_rowptr[r + 1] - p.d_rowptr[r]));
  s.x = fmaf(t.x, w, s.x); s.y = fmaf(t.y, w, s.y); s.z = fmaf(t.z, w, s.z); s.w = fmaf(t.w, w, s.w);
}

__global__ __launch_bounds__(256) void k_pool_bwd(PoolBwd p, int lg) {
  const agnn::Lanes L = agnn::lanes_of(lg);
  const int64_t j = static_cast<int64_t>(blockIdx.x) * L.gpb + L.grp;
  if (j >= p.n) return;
  const int e0 = p.s_rowptr[j], e1 = p.s_rowptr[j + 1];
  for (int c4 = L.lig; c4 < p.H4; c4 += L.G) {
    float4 s = agnn::f4_zero();
    add_node(p, j, c4, s);                                      // the appended self loop
    for (int e = e0; e < e1; ++e) {
      const int d = p.s_col[e];
      if (d < 0 || d >= p.n) continue;
      add_node(p, d, c4, s);
    }
    reinterpret_cast<float4*>(p.da + j * p.ld_da)[c4] = s;
  }
}

int pool_sizes(const char* who, int32_t H, int64_t n, int64_t n_sel) {
  using namespace agnn;
  if (int rc = check_h(who, H)) return rc;
  if (n < 0 || n >= INT32_MAX) return fail(AGNN_EINVAL, "%s: n=%lld must be in [0, 2^31 - 1)", who, (long long)n);
  if (n_sel < 0 || n_sel > INT32_MAX) return fail(AGNN_EINVAL, "%s: n_sel=%lld must be in [0, 2^31)", who, (long long)n_sel);
  return AGNN_OK;
}

}  // namespace

extern "C" int agnn_onset_pool_fwd_f32(const float* a, int64_t ld_a, int64_t n, int32_t H, const int32_t* d_rowptr, const int32_t* d_col,
                                       const int64_t* idx, int64_t n_sel, float* out, int64_t ld_out, int32_t* status, agnn_stream_t stream_) {
  using namespace agnn;
  const char* who = "onset_pool_fwd";
  if (int rc = pool_sizes(who, H, n, n_sel)) return rc;
  if (n_sel == 0) return AGNN_OK;
  if (n == 0) return fail(AGNN_EINVAL, "%s: n_sel=%lld rows selected out of n=0", who, (long long)n_sel);
  if (int rc = check_matrix(who, "a", a, ld_a, H)) return rc;
  if (int rc = check_matrix(who, "out", out, ld_out, H)) return rc;
  if (!d_rowptr || !d_col || !idx) return fail(AGNN_EINVAL, "%s: d_rowptr, d_col or idx is null", who);
  const int lg = group_log2(H / 4), gpb = 256 >> lg;
  PoolFwd p{a, ld_a, n, H / 4, d_rowptr, d_col, idx, n_sel, out, ld_out, status};
  hipLaunchKernelGGL(k_pool_fwd, dim3(static_cast<unsigned>((n_sel + gpb - 1) / gpb)), dim3(256), 0, static_cast<hipStream_t>(stream_), p, lg);
  return check_launch(who);
}

extern "C" int agnn_onset_pool_bwd_f32(const float* g, int64_t ld_g, int64_t n_sel, int32_t H, int64_t n, const int32_t* d_rowptr,
                                       const int32_t* s_rowptr, const int32_t* s_col, const int32_t* sel_rowptr, const int32_t* sel_k,
                                       float* da, int64_t ld_da, agnn_stream_t stream_) {
  using namespace agnn;
  const char* who = "onset_pool_bwd";
  if (int rc = pool_sizes(who, H, n, n_sel)) return rc;
  if (n == 0) return AGNN_OK;
  if (int rc = check_matrix(who, "da", da, ld_da, H)) return rc;
  if (n_sel > 0) {
    if (int rc = check_matrix(who, "g", g, ld_g, H)) return rc;
  }
  if (!d_rowptr || !s_rowptr || !s_col || !sel_rowptr || !sel_k) return fail(AGNN_EINVAL, "%s: an index array is null", who);
  const int lg = group_log2(H / 4), gpb = 256 >> lg;
  PoolBwd p{g, ld_g, n_sel, H / 4, n, d_rowptr, s_rowptr, s_col, sel_rowptr, sel_k, da, ld_da};
  hipLaunchKernelGGL(k_pool_bwd, dim3(static_cast<unsigned>((n + gpb - 1) / gpb)), dim3(256), 0, static_cast<hipStream_t>(stream_), p, lg);
  return check_launch(who);
}
