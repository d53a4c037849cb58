// Validation / test metrics of the task heads: per-task argmax and the integer counters behind accuracy, macro F1, the
// chord-tone-gated accuracies and the joint Roman-numeral accuracies, in one pass over the side-by-side logits.
//
// The reference logs them per task with torchmetrics (`Accuracy(task="multiclass")`, `F1Score(average="macro")`,
// analysisgnn/models/analysis.py:890-891, :1143-1164, :1221-1282): per task an argmax, a compare, a sum and three bincounts,
// then boolean indexing with a host sync for the gated variants.  Here the task logits live side by side in one [N, ld] matrix,
// as for the cross entropy (mtce.hip), the labels as int64 [T, N], and 16 lanes per row produce every task's prediction; the
// same 16 lanes then count, one task per lane, into a per-block LDS histogram of int32, and the block adds its non-zero bins to
// the caller's int64 counters with integer atomics.  Integer sums do not depend on arrival order: bitwise reproducible, and
// no float atomic anywhere.  Memory-bound: the logits are read once, nothing is written per row but the optional predictions.
#include <climits>

#include "agnn_common.h"

namespace {

using agnn::dpp_u32;
// reductions inside a 16-lane row, as agnn::row16_max: every lane of the row ends with the result
__device__ __forceinline__ unsigned row16_umax(unsigned v) {
  v = max(v, dpp_u32<0xB1>(v));
  v = max(v, dpp_u32<0x4E>(v));
  v = max(v, dpp_u32<0x141>(v));
  v = max(v, dpp_u32<0x140>(v));
  return v;
}
__device__ __forceinline__ unsigned row16_umin(unsigned v) {
  v = min(v, dpp_u32<0xB1>(v));
  v = min(v, dpp_u32<0x4E>(v));
  v = min(v, dpp_u32<0x141>(v));
  v = min(v, dpp_u32<0x140>(v));
  return v;
}

// torch.argmax's order as an unsigned key: a NaN (either sign) is the largest value, -0 equals +0, everything else —
// infinities and denormals included — orders as the floats do.  The smallest key of a real entry is -inf's, 0x007FFFFF: 0 is
// free for "this lane holds no class".
__device__ __forceinline__ unsigned order_key(float x) {
  const unsigned u = __float_as_uint(x);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
  if ((u & 0x7FFFFFFFu) == 0u) return 0x80000000u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr int kEvalRows = 16;           // rows per workgroup and trip: 4 waves x 4 rows of 16 lanes
constexpr int kEvalMaxBlocks = 512;     // workgroups re-use their histogram over a grid-stride loop: fewer flushes
constexpr int kNoClass = INT_MAX;

// LDS pitch of a staged row: the smallest p >= w with p % 64 == 16, so the four rows of a wavefront read disjoint banks
__host__ __device__ inline int eval_pitch(int w) { return ((w + 47) / 64) * 64 + 16; }

// Dynamic LDS: [16 rows][pitch] floats (the staged logits) | seg_a[32], seg_b[32] | the histogram (counts != nullptr only),
// in the layout of `counts`: valid[T] correct[T] valid_g[T] correct_g[T] | 4 joint | tp[W] n_pred[W] n_label[W].
__global__ __launch_bounds__(256) void k_eval(const float* __restrict__ z, int64_t ld, const int32_t* __restrict__ off,
                                              const int32_t* __restrict__ seg_end, int T, int n_cols,
                                              const int64_t* __restrict__ labels, int64_t n_rows, int64_t ignore,
                                              const uint8_t* __restrict__ row_mask, int gate_task, unsigned group_mask,
                                              int32_t* __restrict__ pred, unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int pitch = eval_pitch(n_cols);
  int* s_a = reinterpret_cast<int*>(s_mem + kEvalRows * pitch);
  int* s_b = s_a + AGNN_MAX_SEG;
  int* hist = s_b + AGNN_MAX_SEG;
  const int nbins = 4 * T + 4 + 3 * n_cols;
  const int tid = threadIdx.x, lane = tid & 63, sub = lane & 15;
  const int slot = (tid >> 6) * 4 + (lane >> 4);
  if (tid < T) {                                            // clamped: whatever the offsets hold, nothing leaves the row or the bins
    int a = off[tid], b = seg_end != nullptr ? seg_end[tid] : off[tid + 1];
    a = a < 0 ? 0 : a;
    b = b > n_cols ? n_cols : b;
    s_a[tid] = a;
    s_b[tid] = b;
  }
  if (counts != nullptr)
    for (int i = tid; i < nbins; i += 256) hist[i] = 0;
  __syncthreads();
  int lo = n_cols, hi = 0;                                  // the columns the segments cover; only those are fetched
  for (int t = 0; t < T; ++t)
    if (s_b[t] > s_a[t]) {
      lo = min(lo, s_a[t]);
      hi = max(hi, s_b[t]);
    }
  if (hi < lo) lo = hi = 0;                                 // no segment holds a class: nothing to fetch
  const bool vec2 = (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(z) & 7u) == 0;
  lo = vec2 ? (lo & ~1) : lo;
  float* sr = s_mem + slot * pitch;
  int* h_valid = hist;
  int* h_correct = hist + T;
  int* h_valid_g = hist + 2 * T;
  int* h_correct_g = hist + 3 * T;
  int* h_joint = hist + 4 * T;
  int* h_tp = h_joint + 4;
  int* h_npred = h_tp + n_cols;
  int* h_nlabel = h_npred + n_cols;
  const int t0 = sub, t1 = sub + 16;                        // the two tasks this lane keeps and counts

  const int64_t n_groups = (n_rows + kEvalRows - 1) / kEvalRows;
  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int64_t row = g * kEvalRows + slot;
    if (row < n_rows) {                                     // whole 16-lane rows drop out; DPP never crosses a row
      const float* zr = z + row * ld;
      // labels of this lane's two tasks: in flight together with the row's logits
      int64_t y0 = ignore, y1 = ignore;
      bool part = false;
      if (counts != nullptr) {
        part = row_mask == nullptr || row_mask[row] != 0;
        if (t0 < T) y0 = labels[static_cast<int64_t>(t0) * n_rows + row];
        if (t1 < T) y1 = labels[static_cast<int64_t>(t1) * n_rows + row];
      }
      if (vec2) {                                           // 8-byte pieces: lo is even, the row base 8-byte aligned
        const int np = (hi - lo) >> 1;
        for (int i0 = sub; i0 < np; i0 += 16 * 8) {         // eight loads in flight per lane and trip
          float2 v[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = i0 + 16 * k < np ? *reinterpret_cast<const float2*>(zr + lo + 2 * (i0 + 16 * k)) : make_float2(0.f, 0.f);
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (i0 + 16 * k < np) *reinterpret_cast<float2*>(sr + lo + 2 * (i0 + 16 * k)) = v[k];
        }
        if (((hi - lo) & 1) && sub == 0) sr[hi - 1] = zr[hi - 1];
      } else {
        for (int c0 = lo + sub; c0 < hi; c0 += 16 * 8) {
          float v[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] = c0 + 16 * k < hi ? zr[c0 + 16 * k] : 0.f;
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (c0 + 16 * k < hi) sr[c0 + 16 * k] = v[k];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // ---- the predictions: max key, then the lowest index among the lanes that hold it --------------------------------------
      int p0 = 0, p1 = 0;
      for (int t = 0; t < T; ++t) {
        const int a = s_a[t], b = s_b[t];
        int p = 0;
        if (b > a) {
          unsigned bk = 0u;
          int bi = kNoClass;
          for (int c = a + sub; c < b; c += 16) {
            const unsigned k = order_key(sr[c]);
            if (k > bk) {                                   // strict: the lane keeps the first of its equal maxima
              bk = k;
              bi = c - a;
            }
          }
          const unsigned m = row16_umax(bk);
          p = static_cast<int>(row16_umin(bk == m ? static_cast<unsigned>(bi) : static_cast<unsigned>(kNoClass)));
        }
        if ((t & 15) == sub) {
          if (t < 16) p0 = p; else p1 = p;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (pred != nullptr) {
        if (t0 < T) pred[static_cast<int64_t>(t0) * n_rows + row] = p0;
        if (t1 < T) pred[static_cast<int64_t>(t1) * n_rows + row] = p1;
      }
      if (counts != nullptr) {
        // ---- the counters: one task per lane (two when T > 16) ---------------------------------------------------------------
        unsigned gate_hit = 0u;
        if (gate_task >= 0) {
          const int pg = gate_task < 16 ? p0 : p1;
          gate_hit = row16_umax((gate_task & 15) == sub && pg != 0 ? 1u : 0u);
        }
        unsigned miss = 0u, wrong = 0u;                     // over the group's tasks of this lane: an ignored label, a wrong prediction
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int t = j == 0 ? t0 : t1;
          const int64_t y = j == 0 ? y0 : y1;
          const int p = j == 0 ? p0 : p1;
          if (t >= T) continue;
          const int a = s_a[t], C = s_b[t] - a;
          const bool valid = y != ignore && C > 0;
          const bool in_range = valid && y >= 0 && y < C;
          const bool hit = in_range && static_cast<int64_t>(p) == y;
          if ((group_mask >> t) & 1u) {
            miss |= valid ? 0u : 1u;
            wrong |= hit ? 0u : 1u;
          }
          if (part && valid) {
            atomicAdd(&h_valid[t], 1);
            atomicAdd(&h_npred[a + p], 1);
            if (in_range) atomicAdd(&h_nlabel[a + static_cast<int>(y)], 1);
            if (hit) {
              atomicAdd(&h_correct[t], 1);
              atomicAdd(&h_tp[a + p], 1);
            }
            if (gate_hit) {
              atomicAdd(&h_valid_g[t], 1);
              if (hit) atomicAdd(&h_correct_g[t], 1);
            }
          }
        }
        if (group_mask != 0u) {
          miss = row16_umax(miss);
          wrong = row16_umax(wrong);
          if (sub == 0 && part && miss == 0u) {
            atomicAdd(&h_joint[0], 1);
            if (wrong == 0u) atomicAdd(&h_joint[1], 1);
            if (gate_hit) {
              atomicAdd(&h_joint[2], 1);
              if (wrong == 0u) atomicAdd(&h_joint[3], 1);
            }
          }
        }
      }
    }
  }
  if (counts != nullptr) {
    __syncthreads();
    for (int i = tid; i < nbins; i += 256) {
      const int v = hist[i];
      if (v != 0) atomicAdd(counts + i, static_cast<unsigned long long>(v));
    }
  }
}

}  // namespace

extern "C" size_t agnn_eval_counts_len(int32_t n_tasks, int32_t n_cols) {
  if (n_tasks < 0 || n_cols < 0) return 0;
  return static_cast<size_t>(4) * n_tasks + 4 + static_cast<size_t>(3) * n_cols;
}

extern "C" int agnn_multitask_eval_f32(const float* logits, int64_t ld, const int32_t* seg_off, const int32_t* seg_end, int32_t n_tasks,
                                       int32_t n_cols, const int64_t* labels, int64_t n_rows, int64_t ignore_index,
                                       const uint8_t* row_mask, int32_t gate_task, uint32_t group_mask, int32_t* pred, int64_t* counts,
                                       agnn_stream_t stream_) {
  using namespace agnn;
  if (n_tasks < 1 || n_tasks > AGNN_MAX_SEG) return fail(AGNN_EINVAL, "multitask_eval: n_tasks=%d (1 .. %d)", n_tasks, AGNN_MAX_SEG);
  if (n_rows < 0 || n_cols < 1 || n_cols > ld)
    return fail(AGNN_EINVAL, "multitask_eval: n_rows=%lld n_cols=%d ld=%lld", (long long)n_rows, n_cols, (long long)ld);
  if (gate_task < -1 || gate_task >= n_tasks) return fail(AGNN_EINVAL, "multitask_eval: gate_task=%d with n_tasks=%d", gate_task, n_tasks);
  if (n_tasks < 32 && (group_mask >> n_tasks) != 0u)
    return fail(AGNN_EINVAL, "multitask_eval: group_mask=0x%x names tasks at or above n_tasks=%d", group_mask, n_tasks);
  if (n_rows == 0) return AGNN_OK;
  if (!logits || !seg_off) return fail(AGNN_EINVAL, "multitask_eval: null argument");
  if (!pred && !counts) return fail(AGNN_EINVAL, "multitask_eval: neither pred nor counts given");
  if (counts && !labels) return fail(AGNN_EINVAL, "multitask_eval: counts without labels");
  if (counts && (reinterpret_cast<uintptr_t>(counts) & 7u)) return fail(AGNN_EALIGN, "multitask_eval: counts must be 8-byte aligned");
  if (pred && (reinterpret_cast<uintptr_t>(pred) & 3u)) return fail(AGNN_EALIGN, "multitask_eval: pred must be 4-byte aligned");
  if (n_cols > AGNN_EVAL_MAX_COLS)
    return fail(AGNN_EINVAL, "multitask_eval: n_cols=%d, at most AGNN_EVAL_MAX_COLS=%d (the staged rows and the %zu-bin histogram share 64 KiB of LDS)",
                n_cols, AGNN_EVAL_MAX_COLS, agnn_eval_counts_len(n_tasks, n_cols));
  const size_t lds = (static_cast<size_t>(kEvalRows) * eval_pitch(n_cols) + 2 * AGNN_MAX_SEG + (counts ? agnn_eval_counts_len(n_tasks, n_cols) : 0)) * 4;
  const int64_t groups = (n_rows + kEvalRows - 1) / kEvalRows;
  const unsigned blocks = static_cast<unsigned>(groups < kEvalMaxBlocks ? groups : kEvalMaxBlocks);
  hipLaunchKernelGGL(k_eval, dim3(blocks), dim3(256), lds, static_cast<hipStream_t>(stream_), logits, ld, seg_off, seg_end, n_tasks, n_cols,
                     labels, n_rows, ignore_index, row_mask, gate_task, group_mask, pred, reinterpret_cast<unsigned long long*>(counts));
  return check_launch("multitask_eval");
}
