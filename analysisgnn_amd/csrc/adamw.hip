// Gradient-norm clipping + AdamW over the flat parameter / gradient buffers in two launches.
//
// The reference steps `torch.optim.AdamW` after Lightning's gradient clipping (analysisgnn/models/analysis.py:1380-1381,
// train/train_analysisgnn.py trainer flags).  Over one flat 5 M-element buffer that is still ~20 element-wise torch
// launches (norm, scale, clamp, mul, addcmul, sqrt, addcdiv, ...), each a full pass over 20 MB: 0.25 ms per step.
// Here: k_gnorm writes per-block partial sums of g^2 (fixed order), k_adamw re-adds the partials in the same fixed
// order in every block (bitwise identical coefficient everywhere, no atomics, no host round trip), and applies
//     g' = g * min(max_norm / (|g| + 1e-6), 1);  p *= 1 - lr*wd;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2
//     p -= lr * (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps)                      (torch.optim.AdamW's update)
// The step counter t lives on the device so a captured hipGraph advances it on every replay.
//
// agnn_adamw_sched_f32 is the same two launches with the learning rate as a closed form of that counter (lr_schedule_eval:
// one __host__ __device__ function, also behind agnn_lr_schedule_at): the lane that advances the counter evaluates it in
// double, rounds it to float once and hands it to the update launch through the workspace, with the SWA snapshot flag and
// the number of snapshots so far.  On a snapshot step the update pass also reads and writes the running average (9 streams
// instead of 7); every other step runs the update body of agnn_adamw_f32 (adam_update<false>), so a constant schedule
// gives its results bit for bit.
#include "agnn_common.h"

#include <cmath>

namespace {

constexpr int kPartials = 1024;
constexpr int kSchedSlots = 4;          // workspace floats behind the partial sums: lr, snapshot flag, snapshots before this step

// cos(pi x).  Device: cospi.  Host (no cospi in every libm): x is folded exactly into [0, 1] first, so the only rounding
// that cospi avoids, that of pi * x, is that of an argument no larger than pi.
__host__ __device__ inline double cos_pi(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return cospi(x);
#else
  x = fabs(x);
  x -= 2.0 * floor(0.5 * x);            // [0, 2), exact
  if (x > 1.0) x = 2.0 - x;             // cos(pi (2 - x)) = cos(pi x), exact
  return cos(3.14159265358979323846 * x);
#endif
}

// lr(k) for the step index k = optimizer steps already taken: the contract of include/agnn.h, operation for operation as the
// reference's classes and torch's SWALR write it.
__host__ __device__ inline double lr_base(const agnn_lr_schedule_t& s, int64_t k) {
  if (s.kind == AGNN_LR_CONSTANT) return s.base_lr;
  const int64_t c = k + s.count_offset;
  if (c < s.warmup_steps)
    return s.warmup_start_lr + (s.base_lr - s.warmup_start_lr) * (static_cast<double>(c) / static_cast<double>(s.warmup_steps));
  if (s.kind == AGNN_LR_WARMUP_COSINE)
    return s.eta_min + 0.5 * (s.base_lr - s.eta_min) * (1.0 + cos_pi((static_cast<double>(k) - s.cos_a) / (s.cos_b - s.cos_a)));
  const double d = s.base_lr * pow(s.gamma, static_cast<double>(c - s.warmup_steps) / s.decay_steps);
  return d > s.eta_min ? d : s.eta_min;
}

__host__ __device__ inline double lr_schedule_eval(const agnn_lr_schedule_t& s, int64_t k) {
  if (s.swa_start < 0 || k < s.swa_start) return lr_base(s, k);
  const int64_t e = (k - s.swa_start) / s.swa_period;
  double t = 1.0;                                                   // swa_anneal == 0: swa_lr from the first SWA step on
  if (s.swa_anneal > 0 && e < s.swa_anneal) t = static_cast<double>(e) / static_cast<double>(s.swa_anneal);
  const double alpha = (1.0 - cos_pi(t)) / 2.0;
  return s.swa_lr * alpha + lr_base(s, s.swa_start) * (1.0 - alpha);
}

__host__ __device__ inline bool swa_snapshot(const agnn_lr_schedule_t& s, int64_t k) {
  return s.swa_start >= 0 && k >= s.swa_start && (k - s.swa_start) % s.swa_period == 0;
}

// SCHED: the lane that advances the counter also evaluates the schedule at the counter's value before the increment.
template <bool SCHED>
__device__ __forceinline__ void gnorm_body(const float* __restrict__ g, int64_t n, float* __restrict__ partial, float* __restrict__ step,
                                           const agnn_lr_schedule_t* sched, float* __restrict__ state) {
  __shared__ float sm[256];
  const int64_t per = ((n + kPartials - 1) / kPartials + 3) & ~int64_t{3};
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * per;
  int64_t b1 = b0 + per;
  if (b1 > n) b1 = n;
  float a = 0.f;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) a = fmaf(g[i], g[i], a);
  sm[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (static_cast<int>(threadIdx.x) < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = sm[0];
    if (blockIdx.x == 0) {
      if constexpr (SCHED) {
        const int64_t k = static_cast<int64_t>(step[0]);
        const float lr = static_cast<float>(lr_schedule_eval(*sched, k));
        const bool snap = swa_snapshot(*sched, k);
        const float n_avg = state[1];
        partial[kPartials] = lr;
        partial[kPartials + 1] = snap ? 1.f : 0.f;
        partial[kPartials + 2] = n_avg;
        state[0] = lr;
        if (snap) state[1] = n_avg + 1.f;
      }
      step[0] += 1.f;
    }
  }
}

__global__ __launch_bounds__(256) void k_gnorm(const float* __restrict__ g, int64_t n, float* __restrict__ partial, float* __restrict__ step) {
  gnorm_body<false>(g, n, partial, step, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void k_gnorm_sched(const float* __restrict__ g, int64_t n, float* __restrict__ partial,
                                                     float* __restrict__ step, agnn_lr_schedule_t sched, float* __restrict__ state) {
  gnorm_body<true>(g, n, partial, step, &sched, state);
}

struct AdamArgs {
  float* p; float* g; float* m; float* v;
  int64_t n;
  float lr, b1, b2, eps, wd, max_norm;
  const float* partial; const float* step; float* norm_out;
  int write_g;
};

// The update pass of both entry points.  SWA: the parameters as they are BEFORE the update also enter the running average
// (first snapshot: avg = p; then avg += (p - avg) / (n_avg + 1), torch.optim.swa_utils.AveragedModel's default rule).
template <bool SWA>
__device__ __forceinline__ void adam_update(const AdamArgs& a, float* __restrict__ avg, float n_avg) {
  __shared__ float sm[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < kPartials; i += 256) s += a.partial[i];       // same order in every block
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (static_cast<int>(threadIdx.x) < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  const float norm = sqrtf(sm[0]);
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.norm_out != nullptr) a.norm_out[0] = norm;
  float coef = 1.f;
  if (a.max_norm > 0.f) {
    coef = a.max_norm / (norm + 1e-6f);
    if (coef > 1.f) coef = 1.f;
  }
  const float t = a.step[0];
  const float bc1 = 1.f - powf(a.b1, t), bc2 = 1.f - powf(a.b2, t);
  const float inv_bc1 = 1.f / bc1, inv_sqrt_bc2 = 1.f / sqrtf(bc2);
  const float decay = 1.f - a.lr * a.wd;
  [[maybe_unused]] const float n1 = n_avg + 1.f;
  const int64_t n4 = a.n >> 2;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n4; i += static_cast<int64_t>(gridDim.x) * 256) {
    float4 p = reinterpret_cast<float4*>(a.p)[i], g = reinterpret_cast<const float4*>(a.g)[i];
    float4 m = reinterpret_cast<float4*>(a.m)[i], v = reinterpret_cast<float4*>(a.v)[i];
    if constexpr (SWA) {
      float4 w = p;
      if (n_avg > 0.f) {
        w = reinterpret_cast<float4*>(avg)[i];
        w.x += (p.x - w.x) / n1; w.y += (p.y - w.y) / n1; w.z += (p.z - w.z) / n1; w.w += (p.w - w.w) / n1;
      }
      reinterpret_cast<float4*>(avg)[i] = w;
    }
#define AGNN_ADAM1(c)                                                          \
    {                                                                          \
      const float gc = g.c * coef;                                             \
      g.c = gc;                                                                \
      m.c = a.b1 * m.c + (1.f - a.b1) * gc;                                    \
      v.c = a.b2 * v.c + (1.f - a.b2) * gc * gc;                               \
      const float denom = sqrtf(v.c) * inv_sqrt_bc2 + a.eps;                   \
      p.c = p.c * decay - a.lr * (m.c * inv_bc1) / denom;                      \
    }
    AGNN_ADAM1(x) AGNN_ADAM1(y) AGNN_ADAM1(z) AGNN_ADAM1(w)
    reinterpret_cast<float4*>(a.p)[i] = p;
    reinterpret_cast<float4*>(a.m)[i] = m;
    reinterpret_cast<float4*>(a.v)[i] = v;
    if (a.write_g) reinterpret_cast<float4*>(a.g)[i] = g;
  }
  if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {                            // tail (n not a multiple of 4)
    const int64_t i = (n4 << 2) + threadIdx.x;
    if constexpr (SWA) avg[i] = n_avg > 0.f ? avg[i] + (a.p[i] - avg[i]) / n1 : a.p[i];
    const float gc = a.g[i] * coef;
    const float m = a.b1 * a.m[i] + (1.f - a.b1) * gc;
    const float v = a.b2 * a.v[i] + (1.f - a.b2) * gc * gc;
    a.m[i] = m;
    a.v[i] = v;
    a.p[i] = a.p[i] * decay - a.lr * (m * inv_bc1) / (sqrtf(v) * inv_sqrt_bc2 + a.eps);
    if (a.write_g) a.g[i] = gc;
  }
}
#undef AGNN_ADAM1

__global__ __launch_bounds__(256) void k_adamw(AdamArgs a) { adam_update<false>(a, nullptr, 0.f); }

// lr, the snapshot flag and the snapshot count come from the counter launch (workspace slots behind the partial sums).
__global__ __launch_bounds__(256) void k_adamw_sched(AdamArgs a, float* __restrict__ avg) {
  a.lr = a.partial[kPartials];
  if (a.partial[kPartials + 1] != 0.f) adam_update<true>(a, avg, a.partial[kPartials + 2]);
  else adam_update<false>(a, nullptr, 0.f);
}

unsigned adam_blocks(int64_t n) {
  int64_t blocks = ((n >> 2) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return static_cast<unsigned>(blocks);
}

int check_schedule(const agnn_lr_schedule_t* s) {
  using namespace agnn;
  if (!s) return fail(AGNN_EINVAL, "lr_schedule: null schedule");
  if (s->kind != AGNN_LR_CONSTANT && s->kind != AGNN_LR_WARMUP_COSINE && s->kind != AGNN_LR_WARMUP_EXP)
    return fail(AGNN_EINVAL, "lr_schedule: unknown kind %d", s->kind);
  if (s->warmup_steps < 0) return fail(AGNN_EINVAL, "lr_schedule: warmup_steps=%d", s->warmup_steps);
  if (!std::isfinite(s->base_lr) || !std::isfinite(s->warmup_start_lr) || !std::isfinite(s->eta_min))
    return fail(AGNN_EINVAL, "lr_schedule: non-finite rate (base_lr %g, warmup_start_lr %g, eta_min %g)", s->base_lr, s->warmup_start_lr,
                s->eta_min);
  if (s->kind == AGNN_LR_WARMUP_COSINE && !(std::isfinite(s->cos_a) && std::isfinite(s->cos_b) && s->cos_a != s->cos_b))
    return fail(AGNN_EINVAL, "lr_schedule: cosine over [%g, %g]", s->cos_a, s->cos_b);
  if (s->kind == AGNN_LR_WARMUP_EXP && !(s->decay_steps > 0.0 && std::isfinite(s->decay_steps)))
    return fail(AGNN_EINVAL, "lr_schedule: decay_steps=%g", s->decay_steps);
  if (s->kind == AGNN_LR_WARMUP_EXP && !(s->gamma > 0.0 && std::isfinite(s->gamma))) return fail(AGNN_EINVAL, "lr_schedule: gamma=%g", s->gamma);
  if (s->swa_start >= 0) {
    if (s->swa_period <= 0) return fail(AGNN_EINVAL, "lr_schedule: swa_period=%d", s->swa_period);
    if (s->swa_anneal < 0) return fail(AGNN_EINVAL, "lr_schedule: swa_anneal=%d", s->swa_anneal);
    if (!std::isfinite(s->swa_lr)) return fail(AGNN_EINVAL, "lr_schedule: non-finite rate (swa_lr %g)", s->swa_lr);
  }
  return AGNN_OK;
}

}  // namespace

extern "C" size_t agnn_adamw_workspace_bytes(void) { return kPartials * sizeof(float); }

extern "C" int agnn_adamw_f32(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                              float weight_decay, float max_norm, float* step, float* norm_out, int32_t write_clipped_grad,
                              void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (n < 0) return fail(AGNN_EINVAL, "adamw: n=%lld", (long long)n);
  if (n == 0) return AGNN_OK;
  if (!p || !g || !m || !v || !step || !workspace) return fail(AGNN_EINVAL, "adamw: null argument");
  if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v)) return fail(AGNN_EALIGN, "adamw: buffers must be 16-byte aligned");
  if (workspace_bytes < agnn_adamw_workspace_bytes()) return fail(AGNN_ENOMEM, "adamw: workspace too small");
  if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f)) return fail(AGNN_EINVAL, "adamw: betas (%f, %f)", beta1, beta2);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(k_gnorm, dim3(kPartials), dim3(256), 0, s, g, n, partial, step);
  if (int rc = check_launch("adamw_gnorm")) return rc;
  AdamArgs a{p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, max_norm, partial, step, norm_out, write_clipped_grad ? 1 : 0};
  hipLaunchKernelGGL(k_adamw, dim3(adam_blocks(n)), dim3(256), 0, s, a);
  return check_launch("adamw");
}

extern "C" double agnn_lr_schedule_at(const agnn_lr_schedule_t* sched, int64_t k) {
  if (check_schedule(sched) != AGNN_OK) return std::nan("");
  if (k < 0) {
    agnn::fail(AGNN_EINVAL, "lr_schedule: k=%lld", (long long)k);
    return std::nan("");
  }
  return lr_schedule_eval(*sched, k);
}

extern "C" size_t agnn_adamw_sched_workspace_bytes(void) { return (kPartials + kSchedSlots) * sizeof(float); }

extern "C" int agnn_adamw_sched_f32(float* p, float* g, float* m, float* v, int64_t n, const agnn_lr_schedule_t* sched, float beta1,
                                    float beta2, float eps, float weight_decay, float max_norm, float* step, float* swa_avg,
                                    float* state, float* norm_out, int32_t write_clipped_grad, void* workspace,
                                    size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (n < 0) return fail(AGNN_EINVAL, "adamw_sched: n=%lld", (long long)n);
  if (int rc = check_schedule(sched)) return rc;
  if (!state) return fail(AGNN_EINVAL, "adamw_sched: null state");
  if (sched->swa_start >= 0 && !swa_avg) return fail(AGNN_EINVAL, "adamw_sched: swa_start=%lld needs swa_avg", (long long)sched->swa_start);
  if (n == 0) return AGNN_OK;
  if (!p || !g || !m || !v || !step || !workspace) return fail(AGNN_EINVAL, "adamw_sched: null argument");
  if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v)) return fail(AGNN_EALIGN, "adamw_sched: buffers must be 16-byte aligned");
  if (sched->swa_start >= 0 && !aligned16(swa_avg)) return fail(AGNN_EALIGN, "adamw_sched: swa_avg must be 16-byte aligned");
  if (workspace_bytes < agnn_adamw_sched_workspace_bytes()) return fail(AGNN_ENOMEM, "adamw_sched: workspace too small");
  if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f)) return fail(AGNN_EINVAL, "adamw_sched: betas (%f, %f)", beta1, beta2);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(k_gnorm_sched, dim3(kPartials), dim3(256), 0, s, g, n, partial, step, *sched, state);
  if (int rc = check_launch("adamw_sched_gnorm")) return rc;
  AdamArgs a{p, g, m, v, n, 0.f, beta1, beta2, eps, weight_decay, max_norm, partial, step, norm_out, write_clipped_grad ? 1 : 0};
  hipLaunchKernelGGL(k_adamw_sched, dim3(adam_blocks(n)), dim3(256), 0, s, a, sched->swa_start >= 0 ? swa_avg : nullptr);
  return check_launch("adamw_sched");
}
