// Class-balanced cross entropy of the cadence models' validation steps (agnn_balanced_ce_f32), ref models/cadence.py:425-434 and
// :535-544:
//     weight = 1 / (bincount(y) + 1e-6);  loss = F.cross_entropy(logits, y, weight=weight)
// a bincount, a cat, an add, a reciprocal, a log-softmax, a gather, two weighted sums and a division.  The counts cannot depend on
// the logits, so there are two passes and a short fixed-order sum (as agnn_train_loss_f32 has):
//   1. one workgroup counts the labels (integer atomics in LDS: exact, order-free), writes the C weights and
//      W = sum_c count_c w_c = sum_r w_{y_r} in class order;
//   2. a thread owns a row: logsumexp, w_y (lse - z_y), and, where asked for, the row of dlogits scaled by w_y / W; a workgroup
//      adds its 256 terms in a fixed tree and writes one partial.  Reads and writes are strided by the leading dimension and the
//      loop over the classes is serial: right for the 2 .. 5 classes of a cadence head (a row is one or two sectors), legal but
//      slow towards AGNN_BCE_MAX_CLASSES;
//   3. one workgroup adds the partials in a fixed order and writes loss = sum / W (0 when no row is valid).
// No float atomics: two runs give the same bits.
#include <cmath>

#include "agnn_common.h"

namespace {

using namespace agnn;

constexpr int kHead = 64;                       // the weights start on a 256-byte line of the workspace; in front of them [0] = W
inline int64_t row_blocks(int64_t n_rows) { return (n_rows + 255) / 256; }

__global__ __launch_bounds__(1024) void k_bce_count(const int64_t* __restrict__ labels, int64_t n_rows, int C, int64_t ignore_index, float eps_w,
                                                    int64_t* __restrict__ class_count, float* __restrict__ weight, int32_t* status,
                                                    float* __restrict__ ws) {
  __shared__ int cnt[AGNN_BCE_MAX_CLASSES];
  __shared__ float wt[AGNN_BCE_MAX_CLASSES];
  __shared__ int bad;
  for (int c = threadIdx.x; c < C; c += blockDim.x) cnt[c] = 0;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int64_t r = threadIdx.x; r < n_rows; r += blockDim.x) {
    const int64_t y = labels[r];
    if (y == ignore_index) continue;
    if (y < 0 || y >= C) atomicAdd(&bad, 1);
    else atomicAdd(&cnt[static_cast<int>(y)], 1);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float w = 1.f / (static_cast<float>(cnt[c]) + eps_w);
    wt[c] = w;
    ws[kHead + c] = w;
    if (class_count != nullptr) class_count[c] = cnt[c];
    if (weight != nullptr) weight[c] = w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float W = 0.f;
    for (int c = 0; c < C; ++c) W += static_cast<float>(cnt[c]) * wt[c];
    ws[0] = W;
    if (bad != 0 && status != nullptr) atomicAdd(status, bad);
  }
}

__global__ __launch_bounds__(256) void k_bce_rows(const float* __restrict__ logits, int64_t ld, int64_t n_rows, int C,
                                                  const int64_t* __restrict__ labels, int64_t ignore_index, float* __restrict__ dlogits,
                                                  int64_t ld_d, float* __restrict__ ws) {
  __shared__ float red[256];
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  float term = 0.f;
  if (r < n_rows) {
    const int64_t y = labels[r];
    const bool valid = y != ignore_index && y >= 0 && y < C;
    float* dp = dlogits != nullptr ? dlogits + r * ld_d : nullptr;
    if (valid) {
      const float* z = logits + r * ld;
      float m = z[0];
      for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += expf(z[c] - m);
      const float wy = ws[kHead + static_cast<int>(y)];
      term = wy * ((m + logf(s)) - z[y]);
      if (dp != nullptr) {
        const float g = wy / ws[0], inv_s = 1.f / s;
        for (int c = 0; c < C; ++c) dp[c] = g * (expf(z[c] - m) * inv_s - (c == y ? 1.f : 0.f));
      }
    } else if (dp != nullptr) {
      for (int c = 0; c < C; ++c) dp[c] = 0.f;
    }
  }
  red[threadIdx.x] = term;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) ws[kHead + AGNN_BCE_MAX_CLASSES + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_bce_final(const float* __restrict__ ws, int64_t n_part, float* __restrict__ loss) {
  __shared__ float red[256];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n_part; i += 256) s += ws[kHead + AGNN_BCE_MAX_CLASSES + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = ws[0] > 0.f ? red[0] / ws[0] : 0.f;
}

}  // namespace

extern "C" size_t agnn_balanced_ce_workspace_bytes(int64_t n_rows) {
  return sizeof(float) * static_cast<size_t>(kHead + AGNN_BCE_MAX_CLASSES + (n_rows > 0 ? row_blocks(n_rows) : 0) + 1);
}

extern "C" int agnn_balanced_ce_f32(const float* logits, int64_t ld, int64_t n_rows, int32_t n_classes, const int64_t* labels,
                                    int64_t ignore_index, float eps_w, int64_t* class_count, float* weight, float* loss, float* dlogits,
                                    int64_t ld_d, int32_t* status, void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  const char* who = "balanced_ce";
  if (n_classes < 1 || n_classes > AGNN_BCE_MAX_CLASSES)
    return fail(AGNN_EINVAL, "%s: n_classes=%d outside [1, %d]", who, n_classes, AGNN_BCE_MAX_CLASSES);
  if (n_rows < 0 || n_rows >= (int64_t{1} << 31)) return fail(AGNN_EINVAL, "%s: n_rows=%lld", who, (long long)n_rows);
  if (!loss || !workspace) return fail(AGNN_EINVAL, "%s: loss or workspace is null", who);
  if (!(eps_w > 0.f)) return fail(AGNN_EINVAL, "%s: eps_w=%g must be positive (a class without rows divides by it)", who, eps_w);
  if (n_rows > 0) {
    if (!logits || !labels) return fail(AGNN_EINVAL, "%s: logits or labels is null", who);
    if (ld < n_classes || (dlogits != nullptr && ld_d < n_classes))
      return fail(AGNN_EINVAL, "%s: ld=%lld, ld_d=%lld < n_classes=%d", who, (long long)ld, (long long)ld_d, n_classes);
  }
  if ((reinterpret_cast<uintptr_t>(workspace) & 3u) != 0) return fail(AGNN_EALIGN, "%s: workspace is not 4-byte aligned", who);
  if (workspace_bytes < agnn_balanced_ce_workspace_bytes(n_rows))
    return fail(AGNN_ENOMEM, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, agnn_balanced_ce_workspace_bytes(n_rows));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  float* ws = static_cast<float*>(workspace);
  const int64_t nb = row_blocks(n_rows);
  hipLaunchKernelGGL(k_bce_count, dim3(1), dim3(1024), 0, s, labels, n_rows, n_classes, ignore_index, eps_w, class_count, weight, status, ws);
  if (nb > 0)
    hipLaunchKernelGGL(k_bce_rows, dim3(static_cast<unsigned>(nb)), dim3(256), 0, s, logits, ld, n_rows, n_classes, labels, ignore_index, dlogits,
                       ld_d, ws);
  hipLaunchKernelGGL(k_bce_final, dim3(1), dim3(256), 0, s, ws, nb, loss);
  return check_launch(who);
}
