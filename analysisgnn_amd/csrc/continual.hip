// The two continual-learning terms of the reference's training step (analysisgnn/models/analysis.py:1039-1072), from the
// second task stage on: knowledge distillation against a frozen copy of the model, and the EWC penalty.
//
// Distillation (:1052-1062): per previous task `F.kl_div(log_softmax(student / tau), softmax(teacher / tau), 'batchmean')
// * tau^2`, the mean over the tasks, times lambda_dctn — about ten element-wise / softmax launches per task forward and as
// many backward.  Here the task logits of student and teacher live side by side in two [N, ld] matrices, as for the cross
// entropy (mtce.hip), and 16 lanes per row produce, for all tasks in one pass, the per-row KL terms and the FINISHED
// gradient w.r.t. the student logits:
//   q = softmax(s / tau), p = softmax(t / tau);  kl_row = sum_c p_c (log p_c - log q_c),  both logs as x / tau - lse
//   ds_c = w tau / (N T) (q_c - p_c);  kd[t] = tau^2 / N sum_n kl_row;  total = w / T sum_t kd[t]
// Memory-bound: each input matrix is read once, the gradient written once.  No atomics: per-row terms go to [T, N] and
// are summed per task in a fixed order.
//
// EWC (:1479-1495 `sum_n (fisher[n] * (p - mean[n])^2).sum()`, fisher from :1440-1455 `grad^2 / n_batches`): one pass over
// the flat parameter / gradient buffers (dp.FlatAdamW) in place of five whole-model passes and a per-parameter loop;
// per-block partial sums re-added in a fixed order, as k_gnorm does (adamw.hip).
#include <cmath>

#include "agnn_common.h"

namespace {

using agnn::row16_max;
using agnn::row16_sum;

// One task of one row, logits in registers (segments up to 64 classes: NK = 1..4 values per lane and matrix).
// The scaled logits are explicit single roundings (__fmul_rn): a contraction into the subtraction that follows would make
// log p - log q and q - p differ from exactly 0 when student and teacher hold the same numbers.
template <int NK, class PS, class PT, class PD>
__device__ __forceinline__ void kd_task_regs(PS sr, PT tr, PD dr, int a, int b, int sub, float inv_tau, float coef, float& kl) {
  float xs[NK], xt[NK];
  bool in[NK];
  float ms = -INFINITY, mt = -INFINITY;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    in[k] = a + sub + 16 * k < b;
    xs[k] = in[k] ? __fmul_rn(sr[a + sub + 16 * k], inv_tau) : -INFINITY;
    xt[k] = in[k] ? __fmul_rn(tr[a + sub + 16 * k], inv_tau) : -INFINITY;
    ms = fmaxf(ms, xs[k]);
    mt = fmaxf(mt, xt[k]);
  }
  ms = row16_max(ms);
  mt = row16_max(mt);
  float es[NK], et[NK], ses = 0.f, set = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    es[k] = __expf(xs[k] - ms);                        // exp(-inf) = 0 for absent classes
    et[k] = __expf(xt[k] - mt);
    ses += es[k];
    set += et[k];
  }
  ses = row16_sum(ses);
  set = row16_sum(set);
  const float lses = ms + __logf(ses), lset = mt + __logf(set);
  const float is = 1.f / ses, it = 1.f / set;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (in[k]) {
      const float p = __fmul_rn(et[k], it), q = __fmul_rn(es[k], is);
      acc = fmaf(p, (xt[k] - lset) - (xs[k] - lses), acc);      // p == 0 (underflow): 0 * finite = 0
      dr[a + sub + 16 * k] = coef * (q - p);
    }
  }
  kl = row16_sum(acc);
}

// All tasks of one row (16 lanes).  sr / tr = the row's student / teacher logits, dr = where the gradient goes (may be the
// student's memory: every element is read before the same lane overwrites it).  seg_end == nullptr: segment t ends where
// t + 1 starts; otherwise the columns [seg_end[t], off[t + 1]) between two segments belong to no task and are zeroed here.
template <class PS, class PT, class PD>
__device__ __forceinline__ void kd_row(PS sr, PT tr, PD dr, const int32_t* __restrict__ off, const int32_t* __restrict__ seg_end, int T,
                                       int64_t n_rows, int n_cols, int64_t row, int sub, float inv_tau, float coef,
                                       float* __restrict__ row_kl) {
  for (int t = 0; t < T; ++t) {
    int a = off[t], b = seg_end != nullptr ? seg_end[t] : off[t + 1];
    a = a < 0 ? 0 : a;                                      // (the host side checks the offsets; nothing here leaves the row)
    b = b > n_cols ? n_cols : b;
    const int C = b - a;
    float kl = 0.f;
    const int nk = (C + 15) >> 4;
    if (C <= 0) {}
    else if (nk == 1) kd_task_regs<1>(sr, tr, dr, a, b, sub, inv_tau, coef, kl);
    else if (nk == 2) kd_task_regs<2>(sr, tr, dr, a, b, sub, inv_tau, coef, kl);
    else if (nk == 3) kd_task_regs<3>(sr, tr, dr, a, b, sub, inv_tau, coef, kl);
    else if (nk == 4) kd_task_regs<4>(sr, tr, dr, a, b, sub, inv_tau, coef, kl);
    else {
      float ms = -INFINITY, mt = -INFINITY;
      for (int c = a + sub; c < b; c += 16) {
        ms = fmaxf(ms, __fmul_rn(sr[c], inv_tau));
        mt = fmaxf(mt, __fmul_rn(tr[c], inv_tau));
      }
      ms = row16_max(ms);
      mt = row16_max(mt);
      float ses = 0.f, set = 0.f;
      for (int c = a + sub; c < b; c += 16) {
        ses += __expf(__fmul_rn(sr[c], inv_tau) - ms);
        set += __expf(__fmul_rn(tr[c], inv_tau) - mt);
      }
      ses = row16_sum(ses);
      set = row16_sum(set);
      const float lses = ms + __logf(ses), lset = mt + __logf(set);
      const float is = 1.f / ses, it = 1.f / set;
      float acc = 0.f;
      for (int c = a + sub; c < b; c += 16) {
        const float xs = __fmul_rn(sr[c], inv_tau), xt = __fmul_rn(tr[c], inv_tau);
        const float p = __fmul_rn(__expf(xt - mt), it), q = __fmul_rn(__expf(xs - ms), is);
        acc = fmaf(p, (xt - lset) - (xs - lses), acc);
        dr[c] = coef * (q - p);
      }
      kl = row16_sum(acc);
    }
    if (sub == 0) row_kl[static_cast<int64_t>(t) * n_rows + row] = kl;       // task-major: the reduction reads contiguously
    if (seg_end != nullptr && t + 1 < T)
      for (int c = (b > 0 ? b : 0) + sub; c < off[t + 1] && c < n_cols; c += 16) dr[c] = 0.f;
  }
}

// Rows wider than the LDS image: straight from and to global memory, one round trip per task (the segments' second and third
// passes hit L1), then zeros for the columns of [0, n_cols) that no segment covers.
__global__ __launch_bounds__(128) void k_kd(const float* __restrict__ s, int64_t ld_s, const float* __restrict__ t, int64_t ld_t,
                                            const int32_t* __restrict__ off, const int32_t* __restrict__ seg_end, int T, int64_t n_rows,
                                            int n_cols, float inv_tau, float coef, float* __restrict__ ds, int64_t ld_d,
                                            float* __restrict__ row_kl) {
  const int lane = threadIdx.x & 63, sub = lane & 15;
  const int64_t row = (static_cast<int64_t>(blockIdx.x) * 2 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  if (row >= n_rows) return;                                // whole 16-lane rows drop out; DPP never crosses a row
  float* dr = ds + row * ld_d;
  kd_row(s + row * ld_s, t + row * ld_t, dr, off, seg_end, T, n_rows, n_cols, row, sub, inv_tau, coef, row_kl);
  const int lo = off[0], hi = seg_end != nullptr ? seg_end[T - 1] : off[T];
  for (int c = sub; c < lo && c < n_cols; c += 16) dr[c] = 0.f;
  for (int c = (hi > 0 ? hi : 0) + sub; c < n_cols; c += 16) dr[c] = 0.f;
}

// The same through LDS, as k_mtce_lds: the 16 lanes of a row first fetch BOTH rows whole (all loads in flight together), the
// task loop reads the two images and overwrites the student's with the gradient, and the gradient leaves as one pass of
// stores over [0, n_cols) — zeros outside [lo, hi).  Two images per row: 8 rows per workgroup (two waves), W <= 1024 columns
// in 64 KB (634 at C2: 40 KB, four workgroups per CU).  A row's lanes only touch their own LDS rows: no barrier, a
// wave-level fence between the phases.
constexpr int kKdMaxCols = 1024;

__global__ __launch_bounds__(128) void k_kd_lds(const float* __restrict__ s, int64_t ld_s, const float* __restrict__ t, int64_t ld_t,
                                                const int32_t* __restrict__ off, const int32_t* __restrict__ seg_end, int T, int64_t n_rows,
                                                int n_cols, float inv_tau, float coef, float* __restrict__ ds, int64_t ld_d,
                                                float* __restrict__ row_kl) {
  extern __shared__ float s_img[];                          // [8 rows][student | teacher][W], W = n_cols rounded up to even
  const int lane = threadIdx.x & 63, sub = lane & 15;
  const int slot = (threadIdx.x >> 6) * 4 + (lane >> 4);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 8 + slot;
  if (row >= n_rows) return;
  const int W = (n_cols + 1) & ~1;
  int lo = off[0], hi = seg_end != nullptr ? seg_end[T - 1] : off[T];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n_cols ? n_cols : hi;
  float* ss = s_img + static_cast<size_t>(slot) * 2 * W;
  float* st = ss + W;
  const float* sr = s + row * ld_s;
  const float* tr = t + row * ld_t;
  float* dr = ds + row * ld_d;
  // 8-byte pieces when the geometry allows (even strides and segment range, 8-byte aligned matrices): half the memory
  // instructions, twice the bytes in flight
  const bool vin = ((ld_s | ld_t | lo | hi) & 1) == 0 && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(t)) & 7u) == 0;
  if (vin) {
    for (int c0 = lo + 2 * sub; c0 < hi; c0 += 32 * 4) {    // eight loads in flight per lane and trip
      float2 u[4], v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = c0 + 32 * k < hi;
        u[k] = ok ? *reinterpret_cast<const float2*>(sr + c0 + 32 * k) : make_float2(0.f, 0.f);
        v[k] = ok ? *reinterpret_cast<const float2*>(tr + c0 + 32 * k) : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + 32 * k < hi) {
          *reinterpret_cast<float2*>(ss + c0 + 32 * k) = u[k];
          *reinterpret_cast<float2*>(st + c0 + 32 * k) = v[k];
        }
    }
  } else {
    for (int c0 = lo + sub; c0 < hi; c0 += 16 * 4) {
      float u[4], v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = c0 + 16 * k < hi;
        u[k] = ok ? sr[c0 + 16 * k] : 0.f;
        v[k] = ok ? tr[c0 + 16 * k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + 16 * k < hi) {
          ss[c0 + 16 * k] = u[k];
          st[c0 + 16 * k] = v[k];
        }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  kd_row(ss, st, ss, off, seg_end, T, n_rows, n_cols, row, sub, inv_tau, coef, row_kl);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const bool vout = ((ld_d | lo | hi | n_cols) & 1) == 0 && (reinterpret_cast<uintptr_t>(ds) & 7u) == 0;
  if (vout) {
    for (int c = 2 * sub; c < n_cols; c += 32)
      *reinterpret_cast<float2*>(dr + c) = (c >= lo && c < hi) ? *reinterpret_cast<const float2*>(ss + c) : make_float2(0.f, 0.f);
  } else {
    for (int c = sub; c < n_cols; c += 16) dr[c] = (c >= lo && c < hi) ? ss[c] : 0.f;
  }
}

// kd[t] = tau^2 / N * sum_n row_kl[t][n]: one block per task, fixed-order tree (bitwise reproducible), four loads in flight
__global__ __launch_bounds__(1024) void k_kd_reduce(const float* __restrict__ row_kl, int64_t n_rows, float scale, float* __restrict__ kd) {
  __shared__ float sl[1024];
  const float* rl = row_kl + static_cast<int64_t>(blockIdx.x) * n_rows;
  float a4[4] = {0.f, 0.f, 0.f, 0.f};
  int64_t i = threadIdx.x;
  for (; i + 3 * 1024 < n_rows; i += 4 * 1024) {
#pragma unroll
    for (int u = 0; u < 4; ++u) a4[u] += rl[i + u * 1024];
  }
  for (; i < n_rows; i += 1024) a4[0] += rl[i];
  sl[threadIdx.x] = (a4[0] + a4[1]) + (a4[2] + a4[3]);
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (static_cast<int>(threadIdx.x) < o) sl[threadIdx.x] += sl[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) kd[blockIdx.x] = sl[0] * scale;
}

// total = w / T * sum_t kd[t], in index order
__global__ __launch_bounds__(64) void k_kd_total(const float* __restrict__ kd, int T, float w_over_t, float* __restrict__ total) {
  if (threadIdx.x != 0) return;
  float a = 0.f;
  for (int t = 0; t < T; ++t) a += kd[t];
  *total = a * w_over_t;
}

// ---- EWC -----------------------------------------------------------------------------------------------------------------
constexpr int kEwcPartials = 1024;

// Block b owns the elements [b * per, (b + 1) * per), per a multiple of 4 that depends on n alone: the partial sums, and with
// them the penalty, do not depend on the grid or on which block runs when.
__global__ __launch_bounds__(256) void k_ewc(const float* __restrict__ p, const float* __restrict__ mean, const float* __restrict__ fisher,
                                             int64_t n, float two_lambda, float* __restrict__ g, float* __restrict__ partial) {
  __shared__ float sm[256];
  const int64_t per = ((n + kEwcPartials - 1) / kEwcPartials + 3) & ~int64_t{3};
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * per;
  int64_t b1 = b0 + per;
  if (b1 > n) b1 = n;
  float a = 0.f;
  if (b0 < b1) {
    const int64_t n4 = (b1 - b0) >> 2;                      // b0 is a multiple of 4: float4 accesses are 16-byte aligned
    const float4* p4 = reinterpret_cast<const float4*>(p + b0);
    const float4* m4 = reinterpret_cast<const float4*>(mean + b0);
    const float4* f4 = reinterpret_cast<const float4*>(fisher + b0);
    float4* g4 = reinterpret_cast<float4*>(g != nullptr ? g + b0 : nullptr);
    for (int64_t i = threadIdx.x; i < n4; i += 256) {
      const float4 pv = p4[i], mv = m4[i], fv = f4[i];
      const float dx = pv.x - mv.x, dy = pv.y - mv.y, dz = pv.z - mv.z, dw = pv.w - mv.w;
      a = fmaf(fv.x * dx, dx, a);
      a = fmaf(fv.y * dy, dy, a);
      a = fmaf(fv.z * dz, dz, a);
      a = fmaf(fv.w * dw, dw, a);
      if (g != nullptr) {
        float4 gv = g4[i];
        gv.x = fmaf(two_lambda * fv.x, dx, gv.x);
        gv.y = fmaf(two_lambda * fv.y, dy, gv.y);
        gv.z = fmaf(two_lambda * fv.z, dz, gv.z);
        gv.w = fmaf(two_lambda * fv.w, dw, gv.w);
        g4[i] = gv;
      }
    }
    const int64_t i = b0 + (n4 << 2) + threadIdx.x;         // tail of the last block (n not a multiple of 4)
    if (i < b1) {
      const float d = p[i] - mean[i], f = fisher[i];
      a = fmaf(f * d, d, a);
      if (g != nullptr) g[i] = fmaf(two_lambda * f, d, g[i]);
    }
  }
  sm[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (static_cast<int>(threadIdx.x) < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sm[0];
}

__global__ __launch_bounds__(256) void k_ewc_sum(const float* __restrict__ partial, float* __restrict__ penalty) {
  __shared__ float sm[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < kEwcPartials; i += 256) s += partial[i];
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (static_cast<int>(threadIdx.x) < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) penalty[0] = sm[0];
}

__global__ __launch_bounds__(256) void k_fisher_accum(const float* __restrict__ g, int64_t n, float scale, float* __restrict__ fisher) {
  const int64_t n4 = n >> 2;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n4; i += static_cast<int64_t>(gridDim.x) * 256) {
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 fv = reinterpret_cast<float4*>(fisher)[i];
    fv.x = fmaf(scale * gv.x, gv.x, fv.x);
    fv.y = fmaf(scale * gv.y, gv.y, fv.y);
    fv.z = fmaf(scale * gv.z, gv.z, fv.z);
    fv.w = fmaf(scale * gv.w, gv.w, fv.w);
    reinterpret_cast<float4*>(fisher)[i] = fv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {           // tail (n not a multiple of 4)
    const int64_t i = (n4 << 2) + threadIdx.x;
    fisher[i] = fmaf(scale * g[i], g[i], fisher[i]);
  }
}

}  // namespace

extern "C" size_t agnn_kd_workspace_bytes(int64_t n_rows, int32_t n_tasks) {
  if (n_rows <= 0 || n_tasks <= 0) return 0;
  return static_cast<size_t>(n_rows) * static_cast<size_t>(n_tasks) * sizeof(float);      // the per-row KL terms [T, N]
}

extern "C" int agnn_multitask_kd_f32(const float* student, int64_t ld_s, const float* teacher, int64_t ld_t, const int32_t* seg_off,
                                     const int32_t* seg_end, int32_t n_tasks, int64_t n_rows, int32_t n_cols, float temperature,
                                     float weight, float* dstudent, int64_t ld_d, float* kd, float* total, void* workspace,
                                     size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (n_tasks < 1) return fail(AGNN_EINVAL, "multitask_kd: n_tasks=%d", n_tasks);
  if (n_rows < 0 || n_cols < 1 || n_cols > ld_s || n_cols > ld_t || n_cols > ld_d)
    return fail(AGNN_EINVAL, "multitask_kd: n_rows=%lld n_cols=%d ld=(%lld, %lld, %lld)", (long long)n_rows, n_cols, (long long)ld_s,
                (long long)ld_t, (long long)ld_d);
  if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail(AGNN_EINVAL, "multitask_kd: temperature=%f", temperature);
  if (!std::isfinite(weight)) return fail(AGNN_EINVAL, "multitask_kd: weight=%f", weight);
  if (!student || !teacher || !seg_off || !dstudent || !kd || !total) return fail(AGNN_EINVAL, "multitask_kd: null argument");
  hipStream_t s = static_cast<hipStream_t>(stream_);
  if (n_rows == 0) {                                        // nothing to read: every term is 0
    if (hipMemsetAsync(kd, 0, sizeof(float) * n_tasks, s) != hipSuccess || hipMemsetAsync(total, 0, sizeof(float), s) != hipSuccess)
      return check_launch("multitask_kd/zero");
    return AGNN_OK;
  }
  if (!workspace) return fail(AGNN_EINVAL, "multitask_kd: null workspace");
  if ((reinterpret_cast<uintptr_t>(workspace) & 3u)) return fail(AGNN_EALIGN, "multitask_kd: workspace must be 4-byte aligned");
  if (workspace_bytes < agnn_kd_workspace_bytes(n_rows, n_tasks))
    return fail(AGNN_ENOMEM, "multitask_kd: workspace of %zu bytes, %zu needed", workspace_bytes, agnn_kd_workspace_bytes(n_rows, n_tasks));
  float* row_kl = static_cast<float*>(workspace);
  const float inv_tau = 1.f / temperature;
  const float coef = static_cast<float>(static_cast<double>(weight) * temperature / (static_cast<double>(n_rows) * n_tasks));
  const unsigned blocks = static_cast<unsigned>((n_rows + 7) / 8);      // 2 waves x 4 rows
  if (n_cols <= kKdMaxCols)
    hipLaunchKernelGGL(k_kd_lds, dim3(blocks), dim3(128), static_cast<size_t>(16) * ((n_cols + 1) & ~1) * sizeof(float), s, student, ld_s,
                       teacher, ld_t, seg_off, seg_end, n_tasks, n_rows, n_cols, inv_tau, coef, dstudent, ld_d, row_kl);
  else
    hipLaunchKernelGGL(k_kd, dim3(blocks), dim3(128), 0, s, student, ld_s, teacher, ld_t, seg_off, seg_end, n_tasks, n_rows, n_cols, inv_tau,
                       coef, dstudent, ld_d, row_kl);
  if (int rc = check_launch("multitask_kd")) return rc;
  const float scale = static_cast<float>(static_cast<double>(temperature) * temperature / static_cast<double>(n_rows));
  hipLaunchKernelGGL(k_kd_reduce, dim3(n_tasks), dim3(1024), 0, s, row_kl, n_rows, scale, kd);
  if (int rc = check_launch("multitask_kd/reduce")) return rc;
  hipLaunchKernelGGL(k_kd_total, dim3(1), dim3(64), 0, s, kd, n_tasks, weight / static_cast<float>(n_tasks), total);
  return check_launch("multitask_kd/total");
}

extern "C" size_t agnn_ewc_workspace_bytes(void) { return kEwcPartials * sizeof(float); }

extern "C" int agnn_ewc_f32(const float* p, const float* mean, const float* fisher, int64_t n, float lambda, float* g, float* penalty,
                            void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (n < 0) return fail(AGNN_EINVAL, "ewc: n=%lld", (long long)n);
  if (!penalty) return fail(AGNN_EINVAL, "ewc: null penalty");
  if (!std::isfinite(lambda)) return fail(AGNN_EINVAL, "ewc: lambda=%f", lambda);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  if (n == 0) {
    if (hipMemsetAsync(penalty, 0, sizeof(float), s) != hipSuccess) return check_launch("ewc/zero");
    return AGNN_OK;
  }
  if (!p || !mean || !fisher) return fail(AGNN_EINVAL, "ewc: null argument");
  if (!workspace) return fail(AGNN_EINVAL, "ewc: null workspace");
  if (!aligned16(p) || !aligned16(mean) || !aligned16(fisher) || !aligned16(g)) return fail(AGNN_EALIGN, "ewc: buffers must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(workspace) & 3u)) return fail(AGNN_EALIGN, "ewc: workspace must be 4-byte aligned");
  if (workspace_bytes < agnn_ewc_workspace_bytes()) return fail(AGNN_ENOMEM, "ewc: workspace of %zu bytes, %zu needed", workspace_bytes, agnn_ewc_workspace_bytes());
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(k_ewc, dim3(kEwcPartials), dim3(256), 0, s, p, mean, fisher, n, 2.f * lambda, g, partial);
  if (int rc = check_launch("ewc")) return rc;
  hipLaunchKernelGGL(k_ewc_sum, dim3(1), dim3(256), 0, s, partial, penalty);
  return check_launch("ewc/sum");
}

extern "C" int agnn_fisher_accum_f32(const float* g, int64_t n, float scale, float* fisher, agnn_stream_t stream_) {
  using namespace agnn;
  if (n < 0) return fail(AGNN_EINVAL, "fisher_accum: n=%lld", (long long)n);
  if (!std::isfinite(scale)) return fail(AGNN_EINVAL, "fisher_accum: scale=%f", scale);
  if (n == 0) return AGNN_OK;
  if (!g || !fisher) return fail(AGNN_EINVAL, "fisher_accum: null argument");
  if (!aligned16(g) || !aligned16(fisher)) return fail(AGNN_EALIGN, "fisher_accum: buffers must be 16-byte aligned");
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_fisher_accum, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream_), g, n, scale, fisher);
  return check_launch("fisher_accum");
}
