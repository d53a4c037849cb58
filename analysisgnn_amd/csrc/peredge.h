// What the per-edge objectives share (linkpred.hip, edgedec.hip; not part of the C-ABI): one call serves up to AGNN_MAX_SEG
// segments (link tasks, relations) through a table passed as kernel argument; a group of G = 4 .. 64 lanes owns an edge or a row
// and covers its H / 4 float4 columns; an edge is alive when it lies inside its list and both ends lie in [0, limit); a tile of
// kTile edges leaves its loss sum and five counts in a slot, and a segment's slots are added in a fixed order.  A third objective
// brings its own per-edge arithmetic and its own row walk and takes everything else from here.
#pragma once
#include <algorithm>

#include "rowwave.h"

namespace agnn {

constexpr int kTile = 64;       // edges per workgroup of a forward (one lane of wave 0 each in the tile's reduction)
constexpr int kPartWords = 6;   // a tile's slot: loss sum (float bits) | alive, tp, fp, fn, tn

// A launch table: segment k owns the workgroups [t[k].first, t[k + 1].first)
template <typename Dev>
struct SegTable {
  int32_t n, pad;
  Dev t[AGNN_MAX_SEG];
};
// what the final pass of a forward needs of a segment: `tiles` slots from slot `first` on
struct FinalDev {
  float* loss;
  float* inv_cnt;
  int32_t* counts;
  int32_t first, tiles;
};
// an edge list by one of its ends: row = that end, col = the other end, perm = the edge's position in the list
struct CsrDev {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* perm;
};

// sums and flags cross a lane group by a butterfly, in a fixed order
__device__ __forceinline__ float group_sum(float v, int G) {
  for (int m = G >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ int group_or(int v, int G) {
  for (int m = G >> 1; m > 0; m >>= 1) v |= __shfl_xor(v, m);
  return v;
}

// The segment of this workgroup, through a reference: returning the index, or the entry (a reference the compiler may then read
// ahead of the kernel's own conditions), changes the kernels' assembly.
template <typename Dev>
__device__ __forceinline__ void find_segment(const SegTable<Dev>& tab, int& k) {
  k = 0;
  while (k + 1 < tab.n && static_cast<int>(blockIdx.x) >= tab.t[k + 1].first) ++k;
}

// this lane's place: G lanes per group, gpb groups per workgroup of 256, group grp, lane lig of the group
struct Lanes {
  int G, gpb, grp, lig;
};
__device__ __forceinline__ Lanes lanes_of(int lg) {
  const int tid = threadIdx.x, G = 1 << lg;
  return Lanes{G, 256 >> lg, tid >> lg, tid & (G - 1)};
}

// the row of a backward's output that this lane's group owns: gpb rows per workgroup, from the segment's first workgroup on
template <typename Dev>
__device__ __forceinline__ int64_t group_row(const Dev& T, int lg) {
  const int gpb = 256 >> lg;
  return static_cast<int64_t>(static_cast<int>(blockIdx.x) - T.first) * gpb + (static_cast<int>(threadIdx.x) >> lg);
}

// edge e of a segment with src, dst, E and limit: `in` the list, its ends (0, 0 outside the list: nothing is read), alive
struct Ends {
  int64_t s, d;
  bool in, alive;
};
template <typename Dev>
__device__ __forceinline__ Ends edge_ends(const Dev& T, int64_t e) {
  Ends x{0, 0, e < T.E, false};
  if (x.in) { x.s = T.src[e]; x.d = T.dst[e]; }
  x.alive = x.in && x.s >= 0 && x.d >= 0 && x.s < T.limit && x.d < T.limit;
  return x;
}

// The tile record.  An alive edge's code: bit 0 alive, then tp, fp, fn, tn of (predicted positive, labelled positive) ...
__device__ __forceinline__ int confusion_code(bool pos, bool hit) {
  return 1 | ((pos && hit) ? 2 : 0) | ((pos && !hit) ? 4 : 0) | ((!pos && hit) ? 8 : 0) | ((!pos && !hit) ? 16 : 0);
}
// ... and wave 0, lane = edge of tile `tile` of a segment whose first tile is `first` (loss 0 and code 0 where not alive), leaves
// the sums in the tile's slot
__device__ __forceinline__ void tile_record(uint32_t* __restrict__ part, int first, int tile, float loss, int code) {
  const float sum = wave_sum_dpp(loss);
  uint32_t* p = part + (static_cast<int64_t>(first) + tile) * kPartWords;
  const int c0 = __popcll(__ballot(code & 1)), c1 = __popcll(__ballot(code & 2)), c2 = __popcll(__ballot(code & 4));
  const int c3 = __popcll(__ballot(code & 8)), c4 = __popcll(__ballot(code & 16));
  if (threadIdx.x == 0) {
    p[0] = __float_as_uint(sum);
    p[1] = c0; p[2] = c1; p[3] = c2; p[4] = c3; p[5] = c4;
  }
}

// One segment's slots in a fixed order, by a whole workgroup of 256: lane t takes tiles t, t + 256, ..., then a tree in LDS; lane 0
// stores the mean loss (0 without an alive edge), 1 / alive and the five counts, and adds the mean to *total where one is kept.
// The counters are an array: with five scalars the last step of the tree reads LDS word by word (profiles/peredge_isa_identity.md).
__device__ __forceinline__ void segment_final(const FinalDev& T, const uint32_t* __restrict__ part, float* total = nullptr) {
  __shared__ float f_s[256];
  __shared__ int i_s[5][256];
  const int tid = threadIdx.x;
  float acc = 0.f;
  int c[5] = {0, 0, 0, 0, 0};
  for (int t = tid; t < T.tiles; t += 256) {
    const uint32_t* p = part + (static_cast<int64_t>(T.first) + t) * kPartWords;
    acc += __uint_as_float(p[0]);
#pragma unroll
    for (int k = 0; k < 5; ++k) c[k] += static_cast<int>(p[1 + k]);
  }
  f_s[tid] = acc;
#pragma unroll
  for (int k = 0; k < 5; ++k) i_s[k][tid] = c[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      f_s[tid] += f_s[tid + w];
#pragma unroll
      for (int k = 0; k < 5; ++k) i_s[k][tid] += i_s[k][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int alive = i_s[0][0];
    const float inv = alive > 0 ? 1.f / static_cast<float>(alive) : 0.f;
    const float mean = f_s[0] * inv;
    T.loss[0] = mean;
    T.inv_cnt[0] = inv;
#pragma unroll
    for (int k = 0; k < 5; ++k) T.counts[k] = i_s[k][0];
    if (total) *total += mean;
  }
}

// log2 of the lanes per edge / row: the power of two in [4, 64] that covers H4 float4 columns (64 above 64 columns)
inline int group_log2(int H4) {
  int lg = 2;
  while (lg < 6 && (1 << lg) < H4) ++lg;
  return lg;
}

// drop_threshold with 0 standing for "no dropout" in the kernels, so a p > 0 below 2^-32 still draws
inline uint32_t threshold_or_none(float p) { return p > 0.f ? std::max<uint32_t>(drop_threshold(p), 1u) : 0u; }

inline int64_t tiles_of(int64_t E, int tile) { return E > 0 ? (E + tile - 1) / tile : 0; }

// Host validators.  `who` is the entry point's name, `noun` what it calls a segment ("task", "relation").
inline int check_h(const char* who, int32_t H, int max_h = 0) {
  if (max_h == 0 && (H < 4 || H % 4 != 0)) return fail(AGNN_EINVAL, "%s: H=%d must be a positive multiple of 4", who, H);
  if (max_h != 0 && (H < 4 || H > max_h || H % 4 != 0)) return fail(AGNN_EINVAL, "%s: H=%d must be a multiple of 4 in [4, %d]", who, H, max_h);
  return AGNN_OK;
}

inline int check_segments(const char* who, const char* name, int32_t n) {
  if (n < 0 || n > AGNN_MAX_SEG) return fail(AGNN_EINVAL, "%s: %s=%d must be in [0, %d]", who, name, n, AGNN_MAX_SEG);
  return AGNN_OK;
}

// a list of E edges handled in tiles of `tile`, over n rows of which the first `limit` count
inline int check_sizes(const char* who, const char* noun, int i, int64_t E, int64_t n, int64_t limit, int tile) {
  if (E < 0 || E > INT32_MAX - tile) return fail(AGNN_EINVAL, "%s: %s %d: E=%lld must be in [0, 2^31 - %d)", who, noun, i, (long long)E, tile);
  if (n < 0 || n > INT32_MAX) return fail(AGNN_EINVAL, "%s: %s %d: n=%lld must be in [0, 2^31)", who, noun, i, (long long)n);
  if (limit < 0 || limit > n) return fail(AGNN_EINVAL, "%s: %s %d: limit=%lld must be in [0, n=%lld]", who, noun, i, (long long)limit, (long long)n);
  return AGNN_OK;
}

// a [rows, H] float matrix a kernel reads or writes with float4: rowwave.h's validator, the segment named in front of the operand
inline int check_rows(const char* who, const char* noun, int i, const char* name, const void* p, int64_t ld, int32_t H) {
  char where[96];
  snprintf(where, sizeof(where), "%s: %s %d", who, noun, i);
  return check_matrix(where, name, p, ld, H);
}

// a grid of `total` workgroups (tiles, slots): `what` names them in the message
inline int check_grid(const char* who, const char* what, int64_t total) {
  if (total > INT32_MAX) return fail(AGNN_EINVAL, "%s: more than 2^31 - 1 %s", who, what);
  return AGNN_OK;
}

inline int check_workspace(const char* who, const void* ws, size_t bytes, size_t need, unsigned align) {
  if (!ws) return fail(AGNN_EINVAL, "%s: workspace is null", who);
  if (bytes < need) return fail(AGNN_ENOMEM, "%s: workspace of %zu bytes, %zu needed", who, bytes, need);
  if ((reinterpret_cast<uintptr_t>(ws) & (align - 1u)) != 0) return fail(AGNN_EALIGN, "%s: workspace is not %u-byte aligned", who, align);
  return AGNN_OK;
}

}  // namespace agnn
