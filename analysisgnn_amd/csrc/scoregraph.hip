// Score graph construction: note arrays (onset, duration in divs) -> the four note relations as int64 COO, and the metrical
// (beat / measure) nodes with their membership edges.  Replaces the reference's O(N^2) Python loop
// `hetero_graph_from_note_array` (analysisgnn/utils/hgraph.py:214-300) and the N x N masks of synth.make_score_graph.
//
// The notes of a score arrive sorted by onset (the reference sorts by (onset, pitch) before building, models/analysis.py:1534),
// so every destination list is a contiguous run of note ids and two binary searches in the score's own slice find it.  For source
// i with end = onset + duration, lb / ub = lower / upper bound inside the slice:
//   onset        [lb(onset_i), ub(onset_i))                      (i itself kept or not: AGNN_SG_SELF_LOOPS)
//   consecutive  [lb(end_i), ub(end_i))
//   during       [ub(onset_i), max(ub(onset_i), lb(end_i)))
//   rest         sources in stable order of end inside the score; a source contributes when no note of its score starts at its end
//                and a later onset exists; destinations = the onset group of the first onset > end
// Edge order (it becomes the summation order of agnn_csr_build): source-major, destinations ascending; rest by (end, source,
// destination) — the order of the reference's loops.
//   k_sg_init      score_start is checked (one block); the segments of the sort
//   k_sg_validate  per note: its score, value range, order; the sort key `end`
//   radix sort     (library, segmented by score) stable order by (score, end)
//   k_sg_count     per note four counts and run starts (rest: indexed by position in end order)
//   scan           (library) exclusive sum over the 4 N counts
//   k_sg_totals    the four totals
//   k_sg_fill      a group of 8 lanes per (relation, source) writes its run of (i, j) pairs; then padding and the overflow words
// Integer work only.  A score with a fault (agnn.h) gets no edge; no index leaves its slice whatever the input holds.
#include <hipcub/hipcub.hpp>

#include "agnn_common.h"

namespace {

constexpr int kGroup = 8;          // lanes per (relation, source) run of the fill pass: runs of a score graph hold 1 .. 4 edges
constexpr int64_t kBound = int64_t{1} << 31;

__device__ __forceinline__ int32_t lower_bound(const int64_t* __restrict__ a, int32_t lo, int32_t hi, int64_t x) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int32_t upper_bound(const int64_t* __restrict__ a, int32_t lo, int32_t hi, int64_t x) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// score of note i: the last s with score_start[s] <= i, kept inside [0, S - 1] whatever score_start holds
__device__ __forceinline__ int32_t score_of_note(const int32_t* __restrict__ start, int32_t S, int32_t i) {
  int32_t lo = 0, hi = S + 1;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (start[mid] <= i) lo = mid + 1; else hi = mid;
  }
  const int32_t s = lo - 1;
  return s < 0 ? 0 : (s > S - 1 ? S - 1 : s);
}

// bad[s] = 0 for every score; bad[S] = 1 when score_start does not tile [0, N), and the sort then gets empty segments
__global__ __launch_bounds__(256) void k_sg_init(const int32_t* __restrict__ start, int32_t S, int32_t N, int32_t* __restrict__ bad,
                                                 int32_t* __restrict__ seg, int32_t* __restrict__ faults) {
  int fail = 0;
  for (int32_t s = threadIdx.x; s < S; s += blockDim.x) {
    const int32_t a = start[s], b = start[s + 1];
    fail |= (a < 0 || b < a || b > N || (s == 0 && a != 0) || (s == S - 1 && b != N)) ? 1 : 0;
    bad[s] = 0;
  }
  fail = __syncthreads_or(fail);
  for (int32_t s = threadIdx.x; s <= S; s += blockDim.x) seg[s] = fail ? 0 : start[s];
  if (threadIdx.x == 0) {
    bad[S] = fail;
    if (fail) atomicAdd(faults + AGNN_SG_FAULT_SCORES, 1);
  }
}

__global__ void k_sg_validate(const int64_t* __restrict__ onset, const int64_t* __restrict__ dur, const int32_t* __restrict__ start,
                              int32_t S, int32_t N, int32_t* __restrict__ bad, int32_t* __restrict__ score_of,
                              uint32_t* __restrict__ keys, int32_t* __restrict__ vals, int64_t* __restrict__ note_score,
                              int32_t* __restrict__ faults) {
  const bool all_bad = bad[S] != 0;
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    vals[i] = i;
    if (all_bad) {
      score_of[i] = -1;
      keys[i] = 0u;
      if (note_score) note_score[i] = -1;
      continue;
    }
    const int32_t s = score_of_note(start, S, i);
    const int64_t on = onset[i], du = dur[i];
    const bool range = on < 0 || du < 0 || on >= kBound || du >= kBound || on + du >= kBound;
    const bool order = i > start[s] && onset[i - 1] > on;
    if (range) atomicAdd(faults + AGNN_SG_FAULT_RANGE, 1);
    if (order) atomicAdd(faults + AGNN_SG_FAULT_ORDER, 1);
    if (range || order) atomicOr(bad + s, 1);
    score_of[i] = s;
    keys[i] = range ? 0u : static_cast<uint32_t>(on + du);
    if (note_score) note_score[i] = s;
  }
}

// cnt / lo: [4, N]; rows 0 .. 2 indexed by the note, row 3 by the position in (score, end) order (source = order[t])
__global__ void k_sg_count(const int64_t* __restrict__ onset, const int64_t* __restrict__ dur, const int32_t* __restrict__ start,
                           int32_t N, const int32_t* __restrict__ bad, const int32_t* __restrict__ score_of,
                           const int32_t* __restrict__ order, uint32_t flags, int64_t* __restrict__ cnt, int32_t* __restrict__ lo_out) {
  const int64_t n = N;
  for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < N; t += gridDim.x * blockDim.x) {
    int32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, l0 = 0, l1 = 0, l2 = 0, l3 = 0;
    const int32_t s = score_of[t];
    if (s >= 0 && bad[s] == 0) {
      const int32_t a = start[s], b = start[s + 1];
      const int64_t on = onset[t], end = on + dur[t];
      const int32_t lb_on = lower_bound(onset, a, b, on), ub_on = upper_bound(onset, a, b, on);
      const int32_t lb_end = lower_bound(onset, end == on ? lb_on : ub_on, b, end);   // a grace note links to its own onset group
      const int32_t ub_end = upper_bound(onset, lb_end, b, end);
      l0 = lb_on;
      c0 = ub_on - lb_on - ((flags & AGNN_SG_SELF_LOOPS) ? 0 : 1);
      l1 = lb_end;
      c1 = ub_end - lb_end;
      l2 = ub_on;
      c2 = lb_end > ub_on ? lb_end - ub_on : 0;
    }
    const int32_t j = order[t];
    const int32_t s2 = (j >= 0 && j < N) ? score_of[j] : -1;
    if (s2 >= 0 && bad[s2] == 0) {
      const int32_t a = start[s2], b = start[s2 + 1];
      const int64_t end = onset[j] + dur[j];
      const int32_t lb_end = lower_bound(onset, a, b, end);
      if (lb_end < b && onset[lb_end] != end) {           // nobody starts at `end`, and a later onset exists
        l3 = lb_end;
        c3 = upper_bound(onset, lb_end, b, onset[lb_end]) - lb_end;
      }
    }
    cnt[t] = c0 < 0 ? 0 : c0;
    cnt[n + t] = c1;
    cnt[2 * n + t] = c2;
    cnt[3 * n + t] = c3;
    lo_out[t] = l0;
    lo_out[n + t] = l1;
    lo_out[2 * n + t] = l2;
    lo_out[3 * n + t] = l3;
  }
}

__global__ void k_sg_totals(const int64_t* __restrict__ off, int32_t N, int64_t* __restrict__ totals) {
  const int r = threadIdx.x;
  if (r < 4) totals[r] = off[static_cast<int64_t>(r + 1) * N] - off[static_cast<int64_t>(r) * N];
}

struct FillArgs {
  int64_t* edges[4];
  int64_t cap[4];
  uint32_t rev[4];        // a third row (= row 0 again) behind the two: rows 1 .. 2 are the reverse relation
};

__global__ __launch_bounds__(256) void k_sg_fill(FillArgs A, int32_t N, const int64_t* __restrict__ cnt,
                                                 const int64_t* __restrict__ off, const int32_t* __restrict__ lo,
                                                 const int32_t* __restrict__ order, uint32_t flags, int32_t* __restrict__ faults) {
  const int64_t n = N;
  const int lane = threadIdx.x & (kGroup - 1);
  const int64_t n_groups = static_cast<int64_t>(gridDim.x) * (blockDim.x / kGroup);
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * (blockDim.x / kGroup) + threadIdx.x / kGroup; item < 4 * n; item += n_groups) {
    const int r = static_cast<int>(item / n);
    const int32_t t = static_cast<int32_t>(item - r * n);
    const int64_t c = cnt[item];
    if (c == 0) continue;
    const int64_t o = off[item] - off[r * n], cap = A.cap[r];
    const int32_t l = lo[item];
    const int32_t src = r == 3 ? order[t] : t;
    const bool skip_self = r == 0 && !(flags & AGNN_SG_SELF_LOOPS);
    int64_t* e = A.edges[r];
    for (int64_t k = lane; k < c; k += kGroup) {
      const int64_t pos = o + k;
      if (pos >= cap) break;                               // counted below; nothing is written past the capacity
      int32_t j = l + static_cast<int32_t>(k);
      if (skip_self && j >= src) ++j;
      e[pos] = src;
      e[cap + pos] = j;
      if (A.rev[r]) e[2 * cap + pos] = src;
    }
  }
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x, nt = static_cast<int64_t>(gridDim.x) * blockDim.x;
#pragma unroll 1
  for (int r = 0; r < 4; ++r) {
    const int64_t total = off[(r + 1) * n] - off[r * n], cap = A.cap[r];
    if (tid == 0 && total > cap) atomicAdd(faults + AGNN_SG_FAULT_OVERFLOW + r, 1);
    int64_t* e = A.edges[r];
    for (int64_t pos = total + tid; pos < cap; pos += nt) {  // padding slots: (-1, -1), dropped by agnn_csr_build
      e[pos] = -1;
      e[cap + pos] = -1;
      if (A.rev[r]) e[2 * cap + pos] = -1;
    }
  }
}

// ---- metrical nodes -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t d) {
  const int64_t q = a / d;
  return (a % d != 0 && ((a < 0) != (d < 0))) ? q - 1 : q;
}

// flag[i] = 1 when note i opens a group (first note of its score, or a key that differs from its predecessor's); flag[N] = 0
__global__ void k_grp_flag(const int64_t* __restrict__ key, int64_t div, const int32_t* __restrict__ start, int32_t S, int32_t N,
                           int32_t* __restrict__ flag, int32_t* __restrict__ score_of, int32_t* __restrict__ faults) {
  for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= N; i += gridDim.x * blockDim.x) {
    if (i == N) {
      flag[i] = 0;
      continue;
    }
    const int32_t s = score_of_note(start, S, i);
    score_of[i] = s;
    int f = 1;
    if (i > 0 && i != start[s]) {
      const int64_t k0 = floor_div(key[i - 1], div), k1 = floor_div(key[i], div);
      f = k0 != k1 ? 1 : 0;
      if (k1 < k0) atomicAdd(faults + AGNN_SG_FAULT_ORDER, 1);
    }
    flag[i] = f;
  }
}

struct GroupOut {
  int64_t* note_edge;
  int64_t* group_score;
  int64_t* group_first;
  int64_t* parent_edge;
  const int64_t* parent_of;
  int64_t* per_score;
  int64_t* total;
  int64_t cap;
  int32_t rev;
};

// ex = exclusive sum of flag over [0, N]: the group of note i is ex[i + 1] - 1
__global__ void k_grp_write(GroupOut G, const int32_t* __restrict__ start, int32_t S, int32_t N, const int32_t* __restrict__ flag,
                            const int32_t* __restrict__ ex, const int32_t* __restrict__ score_of, int32_t* __restrict__ faults) {
  const int64_t n = N, cap = G.cap;
  const int32_t total = ex[N];
  const int32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  for (int32_t i = tid; i < N; i += nt) {
    const int64_t gid = ex[i + 1] - 1;
    G.note_edge[i] = i;
    G.note_edge[n + i] = gid;
    if (G.rev) G.note_edge[2 * n + i] = i;
    if (flag[i] && gid < cap) {
      if (G.group_score) G.group_score[gid] = score_of[i];
      if (G.group_first) G.group_first[gid] = i;
      if (G.parent_edge) {
        const int64_t p = G.parent_of[i];
        G.parent_edge[gid] = gid;
        G.parent_edge[cap + gid] = p;
        if (G.rev) G.parent_edge[2 * cap + gid] = gid;
      }
    }
  }
  for (int64_t g = static_cast<int64_t>(total) + tid; g < cap; g += nt) {   // padding groups
    if (G.group_score) G.group_score[g] = -1;
    if (G.group_first) G.group_first[g] = -1;
    if (G.parent_edge) {
      G.parent_edge[g] = -1;
      G.parent_edge[cap + g] = -1;
      if (G.rev) G.parent_edge[2 * cap + g] = -1;
    }
  }
  if (G.per_score)
    for (int32_t s = tid; s < S; s += nt) {
      int32_t a = start[s], b = start[s + 1];
      a = a < 0 ? 0 : (a > N ? N : a);
      b = b < a ? a : (b > N ? N : b);
      G.per_score[s] = ex[b] - ex[a];
    }
  if (tid == 0) {
    if (G.total) G.total[0] = total;
    if (total > cap) atomicAdd(faults + AGNN_SG_FAULT_GROUPS, 1);
  }
}

inline size_t align_up(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

constexpr int kKeyBits = 31;       // end < 2^31

struct Layout {
  size_t bad, seg, score_of, keys_in, keys_out, vals_in, vals_out, cnt, off, lo, temp, temp_bytes, total;
};

Layout make_layout(int64_t N, int32_t S) {
  Layout l;
  const size_t n = static_cast<size_t>(N);
  size_t off = 0;
  l.bad = off; off += align_up((static_cast<size_t>(S) + 1) * sizeof(int32_t));
  l.seg = off; off += align_up((static_cast<size_t>(S) + 1) * sizeof(int32_t));
  l.score_of = off; off += align_up(n * sizeof(int32_t));
  l.keys_in = off; off += align_up(n * sizeof(uint32_t));
  l.keys_out = off; off += align_up(n * sizeof(uint32_t));
  l.vals_in = off; off += align_up(n * sizeof(int32_t));
  l.vals_out = off; off += align_up(n * sizeof(int32_t));
  l.cnt = off; off += align_up((4 * n + 1) * sizeof(int64_t));
  l.off = off; off += align_up((4 * n + 1) * sizeof(int64_t));
  l.lo = off; off += align_up(4 * n * sizeof(int32_t));
  size_t sort_bytes = 0, scan_bytes = 0;
  (void)hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, sort_bytes, static_cast<const uint32_t*>(nullptr),
                                                    static_cast<uint32_t*>(nullptr), static_cast<const int32_t*>(nullptr),
                                                    static_cast<int32_t*>(nullptr), static_cast<int>(N), static_cast<int>(S),
                                                    static_cast<const int32_t*>(nullptr), static_cast<const int32_t*>(nullptr), 0,
                                                    kKeyBits, nullptr);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, static_cast<const int64_t*>(nullptr), static_cast<int64_t*>(nullptr),
                                         static_cast<int>(4 * N + 1), nullptr);
  l.temp = off;
  l.temp_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
  off += align_up(l.temp_bytes);
  l.total = off;
  return l;
}

struct GroupLayout {
  size_t flag, ex, score_of, temp, temp_bytes, total;
};

GroupLayout make_group_layout(int64_t N) {
  GroupLayout l;
  const size_t n = static_cast<size_t>(N);
  size_t off = 0;
  l.flag = off; off += align_up((n + 1) * sizeof(int32_t));
  l.ex = off; off += align_up((n + 1) * sizeof(int32_t));
  l.score_of = off; off += align_up(n * sizeof(int32_t));
  size_t scan_bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr),
                                         static_cast<int>(N + 1), nullptr);
  l.temp = off;
  l.temp_bytes = scan_bytes;
  off += align_up(scan_bytes);
  l.total = off;
  return l;
}

// 4 N + 1 scanned elements and 2^31 note ids bound N
constexpr int64_t kMaxNotes = (int64_t{1} << 29) - 1;

int check_graph(const agnn_score_graph_t* g, const void* workspace, size_t workspace_bytes, bool fill, const char* what) {
  using namespace agnn;
  if (!g) return fail(AGNN_EINVAL, "%s: g is null", what);
  if (g->n_scores < 1) return fail(AGNN_EINVAL, "%s: n_scores=%d", what, g->n_scores);
  if (g->n_notes < 1 || g->n_notes > kMaxNotes) return fail(AGNN_EINVAL, "%s: n_notes=%lld not in [1, %lld]", what, (long long)g->n_notes, (long long)kMaxNotes);
  if (!g->onset_div || !g->duration_div || !g->score_start) return fail(AGNN_EINVAL, "%s: null input (onset_div, duration_div, score_start)", what);
  if (!g->totals || !g->faults) return fail(AGNN_EINVAL, "%s: null totals or faults", what);
  if (fill)
    for (int r = 0; r < 4; ++r) {
      if (g->cap[r] < 0) return fail(AGNN_EINVAL, "%s: cap[%d]=%lld", what, r, (long long)g->cap[r]);
      if (g->cap[r] > 0 && !g->edges[r]) return fail(AGNN_EINVAL, "%s: edges[%d] is null", what, r);
    }
  if (!workspace) return fail(AGNN_EINVAL, "%s: workspace is null", what);
  const size_t need = agnn_score_graph_workspace_bytes(g->n_notes, g->n_scores);
  if (workspace_bytes < need) return fail(AGNN_ENOMEM, "%s: workspace %zu bytes, %zu needed", what, workspace_bytes, need);
  return AGNN_OK;
}

inline char* ws_base(void* workspace) {
  return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t{255});
}

inline int blocks_for(int64_t n, int threads, int cap) {
  int64_t b = (n + threads - 1) / threads;
  return static_cast<int>(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

extern "C" size_t agnn_score_graph_workspace_bytes(int64_t n_notes, int32_t n_scores) {
  if (n_notes < 1 || n_notes > kMaxNotes || n_scores < 1) return 0;
  return make_layout(n_notes, n_scores).total + 256;
}

extern "C" int agnn_score_graph_count(const agnn_score_graph_t* g, void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = check_graph(g, workspace, workspace_bytes, false, "score_graph_count")) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int32_t N = static_cast<int32_t>(g->n_notes), S = g->n_scores;
  const Layout l = make_layout(N, S);
  char* ws = ws_base(workspace);
  int32_t* bad = reinterpret_cast<int32_t*>(ws + l.bad);
  int32_t* score_of = reinterpret_cast<int32_t*>(ws + l.score_of);
  int32_t* seg = reinterpret_cast<int32_t*>(ws + l.seg);
  uint32_t* keys_in = reinterpret_cast<uint32_t*>(ws + l.keys_in);
  uint32_t* keys_out = reinterpret_cast<uint32_t*>(ws + l.keys_out);
  int32_t* vals_in = reinterpret_cast<int32_t*>(ws + l.vals_in);
  int32_t* vals_out = reinterpret_cast<int32_t*>(ws + l.vals_out);
  int64_t* cnt = reinterpret_cast<int64_t*>(ws + l.cnt);
  int64_t* off = reinterpret_cast<int64_t*>(ws + l.off);
  int32_t* lo = reinterpret_cast<int32_t*>(ws + l.lo);
  size_t temp_bytes = l.temp_bytes;
  const int threads = 256, blocks = blocks_for(N, threads, 4096);

  hipLaunchKernelGGL(k_sg_init, dim3(1), dim3(256), 0, stream, g->score_start, S, N, bad, seg, g->faults);
  if (int rc = check_launch("score_graph/init")) return rc;
  hipLaunchKernelGGL(k_sg_validate, dim3(blocks), dim3(threads), 0, stream, g->onset_div, g->duration_div, g->score_start, S, N, bad,
                     score_of, keys_in, vals_in, g->note_score, g->faults);
  if (int rc = check_launch("score_graph/validate")) return rc;
  // one segment per score: the notes of a score are contiguous, so (score, end) order is `end` order inside every slice
  hipError_t e = hipcub::DeviceSegmentedRadixSort::SortPairs(ws + l.temp, temp_bytes, keys_in, keys_out, vals_in, vals_out,
                                                             static_cast<int>(N), static_cast<int>(S), seg, seg + 1, 0, kKeyBits, stream);
  if (e != hipSuccess) return fail(AGNN_ERUNTIME, "score_graph/sort: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_sg_count, dim3(blocks), dim3(threads), 0, stream, g->onset_div, g->duration_div, g->score_start, N, bad, score_of,
                     vals_out, g->flags, cnt, lo);
  if (int rc = check_launch("score_graph/count")) return rc;
  temp_bytes = l.temp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(ws + l.temp, temp_bytes, cnt, off, static_cast<int>(4 * static_cast<int64_t>(N) + 1), stream);
  if (e != hipSuccess) return fail(AGNN_ERUNTIME, "score_graph/scan: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_sg_totals, dim3(1), dim3(64), 0, stream, off, N, g->totals);
  return check_launch("score_graph/totals");
}

extern "C" int agnn_score_graph_fill(const agnn_score_graph_t* g, void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = check_graph(g, workspace, workspace_bytes, true, "score_graph_fill")) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int32_t N = static_cast<int32_t>(g->n_notes);
  const Layout l = make_layout(N, g->n_scores);
  char* ws = ws_base(workspace);
  FillArgs A{};
  for (int r = 0; r < 4; ++r) {
    A.edges[r] = g->edges[r];
    A.cap[r] = g->cap[r];
    A.rev[r] = (g->rev_mask >> r) & 1u;
  }
  const int64_t groups = 4 * static_cast<int64_t>(N);
  hipLaunchKernelGGL(k_sg_fill, dim3(blocks_for(groups, 256 / kGroup, 4096)), dim3(256), 0, stream, A, N,
                     reinterpret_cast<const int64_t*>(ws + l.cnt), reinterpret_cast<const int64_t*>(ws + l.off),
                     reinterpret_cast<const int32_t*>(ws + l.lo), reinterpret_cast<const int32_t*>(ws + l.vals_out), g->flags, g->faults);
  return check_launch("score_graph/fill");
}

extern "C" int agnn_score_graph_build(const agnn_score_graph_t* g, void* workspace, size_t workspace_bytes, agnn_stream_t stream) {
  if (int rc = check_graph(g, workspace, workspace_bytes, true, "score_graph_build")) return rc;
  if (int rc = agnn_score_graph_count(g, workspace, workspace_bytes, stream)) return rc;
  return agnn_score_graph_fill(g, workspace, workspace_bytes, stream);
}

extern "C" size_t agnn_score_groups_workspace_bytes(int64_t n_notes) {
  if (n_notes < 1 || n_notes > kMaxNotes) return 0;
  return make_group_layout(n_notes).total + 256;
}

extern "C" int agnn_score_groups(const agnn_score_groups_t* g, void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (!g) return fail(AGNN_EINVAL, "score_groups: g is null");
  if (g->n_scores < 1) return fail(AGNN_EINVAL, "score_groups: n_scores=%d", g->n_scores);
  if (g->n_notes < 1 || g->n_notes > kMaxNotes) return fail(AGNN_EINVAL, "score_groups: n_notes=%lld not in [1, %lld]", (long long)g->n_notes, (long long)kMaxNotes);
  if (g->div < 1) return fail(AGNN_EINVAL, "score_groups: div=%lld", (long long)g->div);
  if (g->cap < 0) return fail(AGNN_EINVAL, "score_groups: cap=%lld", (long long)g->cap);
  if (!g->key || !g->score_start || !g->note_edge || !g->faults) return fail(AGNN_EINVAL, "score_groups: null argument (key, score_start, note_edge, faults)");
  if (g->parent_edge && !g->parent_of) return fail(AGNN_EINVAL, "score_groups: parent_edge without parent_of");
  if (!workspace) return fail(AGNN_EINVAL, "score_groups: workspace is null");
  const size_t need = agnn_score_groups_workspace_bytes(g->n_notes);
  if (workspace_bytes < need) return fail(AGNN_ENOMEM, "score_groups: workspace %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int32_t N = static_cast<int32_t>(g->n_notes), S = g->n_scores;
  const GroupLayout l = make_group_layout(N);
  char* ws = ws_base(workspace);
  int32_t* flag = reinterpret_cast<int32_t*>(ws + l.flag);
  int32_t* ex = reinterpret_cast<int32_t*>(ws + l.ex);
  int32_t* score_of = reinterpret_cast<int32_t*>(ws + l.score_of);
  size_t temp_bytes = l.temp_bytes;
  const int threads = 256;
  hipLaunchKernelGGL(k_grp_flag, dim3(blocks_for(static_cast<int64_t>(N) + 1, threads, 4096)), dim3(threads), 0, stream, g->key, g->div,
                     g->score_start, S, N, flag, score_of, g->faults);
  if (int rc = check_launch("score_groups/flag")) return rc;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(ws + l.temp, temp_bytes, flag, ex, static_cast<int>(N + 1), stream);
  if (e != hipSuccess) return fail(AGNN_ERUNTIME, "score_groups/scan: %s", hipGetErrorString(e));
  GroupOut G{g->note_edge, g->group_score, g->group_first, g->parent_edge, g->parent_of, g->per_score, g->total, g->cap, g->rev};
  const int64_t span = N > g->cap ? N : g->cap;
  hipLaunchKernelGGL(k_grp_write, dim3(blocks_for(span, threads, 4096)), dim3(threads), 0, stream, G, g->score_start, S, N, flag, ex,
                     score_of, g->faults);
  return check_launch("score_groups/write");
}
