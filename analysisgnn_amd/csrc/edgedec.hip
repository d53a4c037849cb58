// Edge-consistency term of the continual trainer (ref: models/analysis.py:805-836 `EdgeDecoder`, :986-1019 in `common_step`):
// for every note-note relation r the selected edges e = (s, d) are classified "all five RNA labels agree at s and d" from
// embed_r(x[s]) * embed_r(x[d]) through the `fc` chain and a label-smoothed two-class cross entropy.  The reference gathers both
// end rows BEFORE `embed_r` (Linear, ReLU, LayerNorm, Dropout on up to 2 B gathered rows per relation, about 20 launches per
// relation) and scatters the gradient with two index_add_ launches of float atomics.  `embed_r` is row-wise up to its dropout, so
// here A_r = LN(ReLU(x W_r^T + b_r)) exists once per node (a column block of the stacked [B, R H] activation) and the dropout is
// applied per (edge, end, column) in the pair kernel.  One call serves every relation of the step, as a table passed as kernel
// argument; the conventions and their code are shared with linkpred.hip through peredge.h (groups of G = 4 .. 64 lanes covering
// H / 4 float4 columns, several column passes above 64 columns; "alive" = both ends in [0, limit); the tile record and the
// fixed-order final reduction; no float atomics).  Here: the keys draw, the masked product, pair_row and the cross entropy.
//
// Mask index.  The keep factors of edge e of relation r, end t (0 = source, 1 = destination), columns 4 q .. 4 q + 3 are the four
// words of  stream_bits(seed, step, call_id, ((pos0_r + e) * 2 + t) * (H / 4) + q),  pos0_r = the global position of the
// relation's first edge (the sum of the preceding relations' edge counts): every (edge, end, column) of a call has its own word,
// the two ends of an edge draw independent masks, as the reference's two Dropout calls do.  Backward regenerates them from the
// (seed, step) pair the forward launch wrote to `rng_used`; nothing is stored.
// agnn_edge_select_keys draws from the same stream at index pos0_r + e under a call id of its own.
#include <cmath>

#include "peredge.h"

using namespace agnn;

namespace {

constexpr int kBwdTile = 256;   // edges per workgroup of the cross entropy's backward
constexpr int kMaxH = 512;

struct KeysDev {
  const int64_t* src;
  const int64_t* dst;
  int64_t* key;
  int64_t pos0;
  int32_t E, limit, first, pad;
};
struct KeysTable : SegTable<KeysDev> {};

struct PairFwdDev {
  const float* a;
  int64_t ld_a;
  const int64_t* src;
  const int64_t* dst;
  float* f;
  int64_t ld_f;
  uint8_t* label;
  int64_t pos0;
  int32_t E, limit, first, pad;
};
struct PairFwdTable : SegTable<PairFwdDev> {};

struct PairBwdDev {
  const float* a;
  int64_t ld_a;
  const float* df;
  int64_t ld_df;
  CsrDev s, d;                  // the edges by source and by destination
  float* da;
  int64_t ld_da;
  int64_t pos0;
  int32_t n, E, limit, first;
};
struct PairBwdTable : SegTable<PairBwdDev> {};

struct CeFwdDev {
  const float* y;
  int64_t ld_y;
  const int64_t* src;
  const int64_t* dst;
  const uint8_t* label;
  float* logit;
  float* dlogit;
  int32_t E, limit, first, pad;
};
struct CeFwdTable : SegTable<CeFwdDev> {};
struct CeFinalTable : SegTable<FinalDev> {};

struct CeBwdDev {
  const float* y;
  int64_t ld_y;
  const float* dlogit;
  float* dy;
  int64_t ld_dy;
  int32_t E, first;
};
struct CeBwdTable : SegTable<CeBwdDev> {};
static_assert(sizeof(PairFwdTable) + 96 <= 4096 && sizeof(PairBwdTable) + 96 <= 4096 && sizeof(CeFwdTable) + 96 <= 4096 &&
              sizeof(CeBwdTable) + 96 <= 4096 && sizeof(KeysTable) + 96 <= 4096, "the tables travel as kernel arguments");

// keep factors of (global edge position, end, column quad); thr == 0: no dropout, no bits drawn
__device__ __forceinline__ float4 pair_mask(uint64_t seed, uint64_t step, uint32_t call_id, int64_t gpos, int end, int H4, int q,
                                            uint32_t thr, float kept) {
  const uint64_t idx = (static_cast<uint64_t>(gpos) * 2u + static_cast<uint64_t>(end)) * static_cast<uint64_t>(H4) + static_cast<uint64_t>(q);
  return agnn::keep_factors(agnn::stream_bits(seed, step, call_id, idx), thr, kept);
}

__global__ __launch_bounds__(256) void k_edge_keys(KeysTable tab, const int64_t* __restrict__ rng, uint32_t call_id) {
  int r;
  find_segment(tab, r);
  const KeysDev& T = tab.t[r];
  const int64_t e = static_cast<int64_t>(static_cast<int>(blockIdx.x) - T.first) * 256 + threadIdx.x;
  if (e >= T.E) return;                                    // one lane per edge and nothing after it: edge_ends' `in` has no use
  const int64_t s = T.src[e], d = T.dst[e];
  int64_t key = INT64_MAX;
  if (s >= 0 && d >= 0 && s < T.limit && d < T.limit) {
    const uint4 w = agnn::stream_bits(static_cast<uint64_t>(rng[0]), static_cast<uint64_t>(rng[1]), call_id, static_cast<uint64_t>(T.pos0 + e));
    key = static_cast<int64_t>((static_cast<uint64_t>(w.x) << 31) | static_cast<uint64_t>(e));
  }
  T.key[e] = key;
}

__global__ __launch_bounds__(256) void k_pair_fwd(PairFwdTable tab, int H4, int lg, const int64_t* __restrict__ labels, int K, int64_t ldl,
                                                  uint32_t thr, float kept, const int64_t* __restrict__ rng, uint32_t call_id,
                                                  int64_t* __restrict__ rng_used) {
  const int tid = threadIdx.x;
  uint64_t seed = 0, step = 0;
  if (thr != 0u) {
    seed = static_cast<uint64_t>(rng[0]);
    step = static_cast<uint64_t>(rng[1]);
    if (rng_used != nullptr && blockIdx.x == 0 && tid == 0) {
      rng_used[0] = static_cast<int64_t>(seed);
      rng_used[1] = static_cast<int64_t>(step);
    }
  }
  int r;
  find_segment(tab, r);
  const PairFwdDev& T = tab.t[r];
  const int tile = static_cast<int>(blockIdx.x) - T.first;
  const Lanes L = lanes_of(lg);
  const int G = L.G, lig = L.lig;
  for (int le = L.grp; le < kTile; le += L.gpb) {         // the same trip count for every lane of the workgroup
    const int64_t e = static_cast<int64_t>(tile) * kTile + le;
    const Ends x = edge_ends(T, e);
    const int64_t s = x.s, d = x.d;
    const bool in = x.in, alive = x.alive;
    int diff = 0;
    if (alive) {
      const float* as = T.a + s * T.ld_a;
      const float* ad = T.a + d * T.ld_a;
      float* fo = T.f + e * T.ld_f;
      for (int c = lig; c < H4; c += G) {
        float4 u = *reinterpret_cast<const float4*>(as + 4 * c);
        float4 v = *reinterpret_cast<const float4*>(ad + 4 * c);
        if (thr != 0u) {
          const float4 m1 = pair_mask(seed, step, call_id, T.pos0 + e, 0, H4, c, thr, kept);
          const float4 m2 = pair_mask(seed, step, call_id, T.pos0 + e, 1, H4, c, thr, kept);
          u = make_float4(m1.x * u.x, m1.y * u.y, m1.z * u.z, m1.w * u.w);
          v = make_float4(m2.x * v.x, m2.y * v.y, m2.z * v.z, m2.w * v.w);
        }
        *reinterpret_cast<float4*>(fo + 4 * c) = make_float4(u.x * v.x, u.y * v.y, u.z * v.z, u.w * v.w);
      }
      for (int k = lig; k < K; k += G) diff |= (labels[k * ldl + s] != labels[k * ldl + d]) ? 1 : 0;
    } else if (in) {
      float* fo = T.f + e * T.ld_f;
      for (int c = lig; c < H4; c += G) *reinterpret_cast<float4*>(fo + 4 * c) = agnn::f4_zero();
    }
    diff = agnn::group_or(diff, G);
    if (in && lig == 0) T.label[e] = static_cast<uint8_t>((alive && K > 0 && !diff) ? 1 : 0);
  }
}

// sum over row i of one CSR of df[perm] * m1 m2 * a[col], columns 4 c .. 4 c + 3, in list order
__device__ __forceinline__ void pair_row(const CsrDev& csr, int i, const PairBwdDev& T, int H4, int c, uint32_t thr, float kept, uint64_t seed,
                                         uint64_t step, uint32_t call_id, float4& acc) {
  const int32_t* __restrict__ rowptr = csr.rowptr;
  const int32_t* __restrict__ col = csr.col;
  const int32_t* __restrict__ perm = csr.perm;
  const int r1 = rowptr[i + 1];
  for (int j = rowptr[i]; j < r1; ++j) {
    const int e = perm[j], o = col[j];
    if (static_cast<unsigned>(e) >= static_cast<unsigned>(T.E) || static_cast<unsigned>(o) >= static_cast<unsigned>(T.limit)) continue;
    float4 g = *reinterpret_cast<const float4*>(T.df + static_cast<int64_t>(e) * T.ld_df + 4 * c);
    const float4 v = *reinterpret_cast<const float4*>(T.a + static_cast<int64_t>(o) * T.ld_a + 4 * c);
    if (thr != 0u) {
      const float4 m1 = pair_mask(seed, step, call_id, T.pos0 + e, 0, H4, c, thr, kept);
      const float4 m2 = pair_mask(seed, step, call_id, T.pos0 + e, 1, H4, c, thr, kept);
      g = make_float4(g.x * (m1.x * m2.x), g.y * (m1.y * m2.y), g.z * (m1.z * m2.z), g.w * (m1.w * m2.w));
    }
    acc.x = fmaf(g.x, v.x, acc.x); acc.y = fmaf(g.y, v.y, acc.y); acc.z = fmaf(g.z, v.z, acc.z); acc.w = fmaf(g.w, v.w, acc.w);
  }
}

__global__ __launch_bounds__(256) void k_pair_bwd(PairBwdTable tab, int H4, int lg, uint32_t thr, float kept, const int64_t* __restrict__ rng,
                                                  uint32_t call_id) {
  int r;
  find_segment(tab, r);
  const PairBwdDev& T = tab.t[r];
  const int64_t row = group_row(T, lg);
  if (row >= T.n) return;
  const int i = static_cast<int>(row);
  const Lanes L = lanes_of(lg);
  uint64_t seed = 0, step = 0;
  if (thr != 0u) {
    seed = static_cast<uint64_t>(rng[0]);
    step = static_cast<uint64_t>(rng[1]);
  }
  const bool live = T.E > 0 && i < T.limit;                // a row at or above the limit has no alive edge: zeros, no list is read
  for (int c = L.lig; c < H4; c += L.G) {                  // H > 256: the row's lists are walked once per column pass
    float4 acc = agnn::f4_zero();
    if (live) {
      pair_row(T.s, i, T, H4, c, thr, kept, seed, step, call_id, acc);
      pair_row(T.d, i, T, H4, c, thr, kept, seed, step, call_id, acc);
    }
    *reinterpret_cast<float4*>(T.da + row * T.ld_da + 4 * c) = acc;
  }
}

__global__ __launch_bounds__(256) void k_ce_fwd(CeFwdTable tab, int H4, int lg, const float* __restrict__ w4, const float* __restrict__ b4,
                                                float smoothing, uint32_t* __restrict__ part) {
  __shared__ float x0_s[kTile];
  __shared__ float x1_s[kTile];
  __shared__ int flag_s[kTile];
  const int tid = threadIdx.x;
  int r;
  find_segment(tab, r);
  const CeFwdDev& T = tab.t[r];
  const int first = T.first, tile = static_cast<int>(blockIdx.x) - first;   // read once: the tile record takes it again
  const Lanes L = lanes_of(lg);
  const int G = L.G, lig = L.lig;
  const int H = 4 * H4;
  for (int le = L.grp; le < kTile; le += L.gpb) {
    const int64_t e = static_cast<int64_t>(tile) * kTile + le;
    const Ends x = edge_ends(T, e);
    const bool in = x.in, alive = x.alive;
    float4 a0 = agnn::f4_zero(), a1 = agnn::f4_zero();
    if (alive) {
      const float* y = T.y + e * T.ld_y;
      for (int c = lig; c < H4; c += G) {
        const float4 v = *reinterpret_cast<const float4*>(y + 4 * c);
        const float4 p0 = *reinterpret_cast<const float4*>(w4 + 4 * c);
        const float4 p1 = *reinterpret_cast<const float4*>(w4 + H + 4 * c);
        a0.x = fmaf(v.x, p0.x, a0.x); a0.y = fmaf(v.y, p0.y, a0.y); a0.z = fmaf(v.z, p0.z, a0.z); a0.w = fmaf(v.w, p0.w, a0.w);
        a1.x = fmaf(v.x, p1.x, a1.x); a1.y = fmaf(v.y, p1.y, a1.y); a1.z = fmaf(v.z, p1.z, a1.z); a1.w = fmaf(v.w, p1.w, a1.w);
      }
    }
    const float x0 = agnn::group_sum((a0.x + a0.y) + (a0.z + a0.w), G);
    const float x1 = agnn::group_sum((a1.x + a1.y) + (a1.z + a1.w), G);
    if (lig == 0) {
      x0_s[le] = x0;
      x1_s[le] = x1;
      flag_s[le] = (in ? 1 : 0) | (alive ? 2 : 0);
    }
  }
  __syncthreads();
  if (tid < kTile) {                                       // wave 0: lane = edge of the tile
    const int flag = flag_s[tid];
    const bool in = flag & 1, alive = flag & 2;
    float z0 = 0.f, z1 = 0.f, g0 = 0.f, g1 = 0.f, loss = 0.f;
    int code = 0;
    if (alive) {
      const int64_t e = static_cast<int64_t>(tile) * kTile + tid;
      const bool hit = T.label[e] != 0;
      z0 = x0_s[tid] + b4[0];
      z1 = x1_s[tid] + b4[1];
      const float lse = fmaxf(z0, z1) + log1pf(expf(-fabsf(z0 - z1)));
      const float l0 = z0 - lse, l1 = z1 - lse;
      const float q1 = hit ? 1.f - 0.5f * smoothing : 0.5f * smoothing, q0 = 1.f - q1;
      loss = -(q0 * l0 + q1 * l1);
      g0 = expf(l0) - q0;
      g1 = expf(l1) - q1;
      code = confusion_code(z1 > z0, hit);
    }
    if (in) {
      const int64_t e = static_cast<int64_t>(tile) * kTile + tid;
      *reinterpret_cast<float2*>(T.logit + 2 * e) = make_float2(z0, z1);
      *reinterpret_cast<float2*>(T.dlogit + 2 * e) = make_float2(g0, g1);
    }
    tile_record(part, first, tile, loss, code);
  }
}

// one workgroup: relation after relation, then the mean of the relations' losses in table order
__global__ __launch_bounds__(256) void k_ce_final(CeFinalTable tab, const uint32_t* __restrict__ part, float* __restrict__ total) {
  const int tid = threadIdx.x;
  float tot = 0.f;
  for (int r = 0; r < tab.n; ++r) {
    segment_final(tab.t[r], part, &tot);
    __syncthreads();
  }
  if (tid == 0) total[0] = tot / static_cast<float>(tab.n);
}

// dy of a tile of kBwdTile edges; every group leaves its partial dw4 | db4 (2 H + 4 floats) in its own slot of the workspace
__global__ __launch_bounds__(256) void k_ce_bwd(CeBwdTable tab, int H4, int lg, const float* __restrict__ w4, const float* __restrict__ scale,
                                                float* __restrict__ slots) {
  int r;
  find_segment(tab, r);
  const CeBwdDev& T = tab.t[r];
  const int tile = static_cast<int>(blockIdx.x) - T.first;
  const Lanes L = lanes_of(lg);
  const int G = L.G, gpb = L.gpb, grp = L.grp, lig = L.lig;
  const int H = 4 * H4;
  const float sc = scale[r];
  const int c0 = lig, c1 = lig + G;                        // H <= 512: at most two column passes of a 64-lane group
  const bool has0 = c0 < H4, has1 = c1 < H4;
  float4 wa0 = agnn::f4_zero(), wb0 = agnn::f4_zero(), wa1 = agnn::f4_zero(), wb1 = agnn::f4_zero();
  if (has0) { wa0 = *reinterpret_cast<const float4*>(w4 + 4 * c0); wb0 = *reinterpret_cast<const float4*>(w4 + H + 4 * c0); }
  if (has1) { wa1 = *reinterpret_cast<const float4*>(w4 + 4 * c1); wb1 = *reinterpret_cast<const float4*>(w4 + H + 4 * c1); }
  float4 pa0 = agnn::f4_zero(), pb0 = agnn::f4_zero(), pa1 = agnn::f4_zero(), pb1 = agnn::f4_zero();
  float sb0 = 0.f, sb1 = 0.f;
  for (int le = grp; le < kBwdTile; le += gpb) {
    const int64_t e = static_cast<int64_t>(tile) * kBwdTile + le;
    if (e >= T.E) break;
    const float2 g = *reinterpret_cast<const float2*>(T.dlogit + 2 * e);
    const float d0 = sc * g.x, d1 = sc * g.y;
    const bool any = d0 != 0.f || d1 != 0.f;               // an edge that is not alive has the coefficient 0: its row of y is not read
    sb0 += d0;
    sb1 += d1;
    const float* y = T.y + e * T.ld_y;
    float* dy = T.dy + e * T.ld_dy;
    if (has0) {
      *reinterpret_cast<float4*>(dy + 4 * c0) = make_float4(fmaf(d0, wa0.x, d1 * wb0.x), fmaf(d0, wa0.y, d1 * wb0.y),
                                                            fmaf(d0, wa0.z, d1 * wb0.z), fmaf(d0, wa0.w, d1 * wb0.w));
      if (any) {
        const float4 v = *reinterpret_cast<const float4*>(y + 4 * c0);
        pa0.x = fmaf(d0, v.x, pa0.x); pa0.y = fmaf(d0, v.y, pa0.y); pa0.z = fmaf(d0, v.z, pa0.z); pa0.w = fmaf(d0, v.w, pa0.w);
        pb0.x = fmaf(d1, v.x, pb0.x); pb0.y = fmaf(d1, v.y, pb0.y); pb0.z = fmaf(d1, v.z, pb0.z); pb0.w = fmaf(d1, v.w, pb0.w);
      }
    }
    if (has1) {
      *reinterpret_cast<float4*>(dy + 4 * c1) = make_float4(fmaf(d0, wa1.x, d1 * wb1.x), fmaf(d0, wa1.y, d1 * wb1.y),
                                                            fmaf(d0, wa1.z, d1 * wb1.z), fmaf(d0, wa1.w, d1 * wb1.w));
      if (any) {
        const float4 v = *reinterpret_cast<const float4*>(y + 4 * c1);
        pa1.x = fmaf(d0, v.x, pa1.x); pa1.y = fmaf(d0, v.y, pa1.y); pa1.z = fmaf(d0, v.z, pa1.z); pa1.w = fmaf(d0, v.w, pa1.w);
        pb1.x = fmaf(d1, v.x, pb1.x); pb1.y = fmaf(d1, v.y, pb1.y); pb1.z = fmaf(d1, v.z, pb1.z); pb1.w = fmaf(d1, v.w, pb1.w);
      }
    }
  }
  float* slot = slots + ((static_cast<int64_t>(T.first) + tile) * gpb + grp) * (2 * H + 4);
  if (has0) { *reinterpret_cast<float4*>(slot + 4 * c0) = pa0; *reinterpret_cast<float4*>(slot + H + 4 * c0) = pb0; }
  if (has1) { *reinterpret_cast<float4*>(slot + 4 * c1) = pa1; *reinterpret_cast<float4*>(slot + H + 4 * c1) = pb1; }
  if (lig == 0) *reinterpret_cast<float4*>(slot + 2 * H) = make_float4(sb0, sb1, 0.f, 0.f);
}

// the slots in a fixed order: a workgroup owns four float4 columns of the 2 H + 4 wide slot; lane (sl, qi) adds slots sl, sl + 64,
// ... of column qi, then a tree over sl in LDS
__global__ __launch_bounds__(256) void k_ce_bwd_reduce(const float* __restrict__ slots, int64_t S, int H4, float* __restrict__ dw4,
                                                       float* __restrict__ db4) {
  __shared__ float4 s_s[64][4];
  const int tid = threadIdx.x;
  const int sl = tid >> 2, qi = tid & 3;
  const int Wq = 2 * H4 + 1;
  const int q = static_cast<int>(blockIdx.x) * 4 + qi;
  float4 acc = agnn::f4_zero();
  if (q < Wq) {
    for (int64_t s = sl; s < S; s += 64) {
      const float4 v = *reinterpret_cast<const float4*>(slots + s * (4 * Wq) + 4 * q);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  s_s[sl][qi] = acc;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (sl < w) {
      const float4 o = s_s[sl + w][qi];
      float4 m = s_s[sl][qi];
      m.x += o.x; m.y += o.y; m.z += o.z; m.w += o.w;
      s_s[sl][qi] = m;
    }
    __syncthreads();
  }
  if (sl == 0 && q < Wq) {
    const float4 v = s_s[0][qi];
    if (q < 2 * H4) {
      *reinterpret_cast<float4*>(dw4 + 4 * q) = v;
    } else {
      db4[0] = v.x;
      db4[1] = v.y;
    }
  }
}

const char* const kNoun = "relation";

// what every entry point checks of a relation's sizes
int check_rel(const char* who, int i, int64_t E, int64_t n, int64_t limit) { return check_sizes(who, kNoun, i, E, n, limit, kBwdTile); }

template <typename Rel>
int64_t tiles_of_all(int32_t n_rel, const Rel* rels, int tile) {
  int64_t tiles = 0;
  for (int i = 0; i < n_rel; ++i) tiles += tiles_of(rels[i].E, tile);
  return tiles;
}

}  // namespace

extern "C" int agnn_edge_select_keys(int32_t n_rel, const agnn_edge_keys_t* rels, const int64_t* rng_state, uint32_t call_id,
                                     agnn_stream_t stream_) {
  const char* who = "edge_select_keys";
  if (int rc = check_segments(who, "n_rel", n_rel)) return rc;
  if (n_rel == 0) return AGNN_OK;
  if (!rels) return fail(AGNN_EINVAL, "%s: rels is null", who);
  KeysTable tab;
  tab.n = n_rel;
  tab.pad = 0;
  int64_t blocks = 0;
  for (int i = 0; i < n_rel; ++i) {
    const agnn_edge_keys_t& t = rels[i];
    if (int rc = check_rel(who, i, t.E, INT32_MAX, t.limit)) return rc;
    if (t.pos0 < 0) return fail(AGNN_EINVAL, "%s: relation %d: pos0=%lld is negative", who, i, (long long)t.pos0);
    if (t.E > 0 && (!t.src || !t.dst || !t.key)) return fail(AGNN_EINVAL, "%s: relation %d: src / dst / key is null", who, i);
    const int64_t nb = (t.E + 255) / 256;
    if (int rc = check_grid(who, "workgroups", blocks + nb)) return rc;
    tab.t[i] = KeysDev{t.src, t.dst, t.key, t.pos0, static_cast<int32_t>(t.E), static_cast<int32_t>(t.limit), static_cast<int32_t>(blocks), 0};
    blocks += nb;
  }
  if (blocks == 0) return AGNN_OK;
  if (!rng_state) return fail(AGNN_EINVAL, "%s: rng_state is null", who);
  hipLaunchKernelGGL(k_edge_keys, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream_), tab, rng_state, call_id);
  return check_launch(who);
}

extern "C" int agnn_edge_pair_fwd_f32(int32_t n_rel, const agnn_edge_pair_t* rels, int32_t H, const int64_t* labels, int32_t K,
                                      int64_t ld_labels, float p, const int64_t* rng_state, uint32_t call_id, int64_t* rng_used,
                                      agnn_stream_t stream_) {
  const char* who = "edge_pair_fwd";
  if (int rc = check_h(who, H, kMaxH)) return rc;
  if (int rc = check_segments(who, "n_rel", n_rel)) return rc;
  if (!(p >= 0.f && p < 1.f)) return fail(AGNN_EINVAL, "%s: p=%g must be in [0, 1)", who, static_cast<double>(p));
  if (K < 0) return fail(AGNN_EINVAL, "%s: K=%d is negative", who, K);
  if (n_rel == 0) return AGNN_OK;
  if (!rels) return fail(AGNN_EINVAL, "%s: rels is null", who);
  if (!labels) K = 0;
  PairFwdTable tab;
  tab.n = n_rel;
  tab.pad = 0;
  int64_t tiles = 0;
  for (int i = 0; i < n_rel; ++i) {
    const agnn_edge_pair_t& t = rels[i];
    if (int rc = check_rel(who, i, t.E, t.n, t.limit)) return rc;
    if (t.pos0 < 0) return fail(AGNN_EINVAL, "%s: relation %d: pos0=%lld is negative", who, i, (long long)t.pos0);
    const int64_t nt = (t.E + kTile - 1) / kTile;
    if (t.E > 0) {
      if (!t.src || !t.dst) return fail(AGNN_EINVAL, "%s: relation %d: src / dst is null", who, i);
      if (!t.label) return fail(AGNN_EINVAL, "%s: relation %d: label is null", who, i);
      if (int rc = check_rows(who, kNoun, i, "f", t.f, t.ld_f, H)) return rc;
      if (t.limit > 0) {
        if (int rc = check_rows(who, kNoun, i, "a", t.a, t.ld_a, H)) return rc;
        if (K > 0 && ld_labels < t.limit)
          return fail(AGNN_EINVAL, "%s: relation %d: ld_labels=%lld < limit=%lld", who, i, (long long)ld_labels, (long long)t.limit);
      }
    }
    if (int rc = check_grid(who, "tiles of edges", tiles + nt)) return rc;
    tab.t[i] = PairFwdDev{t.a, t.ld_a, t.src, t.dst, t.f, t.ld_f, t.label, t.pos0, static_cast<int32_t>(t.E), static_cast<int32_t>(t.limit),
                          static_cast<int32_t>(tiles), 0};
    tiles += nt;
  }
  if (tiles == 0) return AGNN_OK;
  if (p > 0.f && !rng_state) return fail(AGNN_EINVAL, "%s: rng_state is null with p=%g", who, static_cast<double>(p));
  const uint32_t thr = threshold_or_none(p);
  hipLaunchKernelGGL(k_pair_fwd, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, static_cast<hipStream_t>(stream_), tab, H / 4,
                     agnn::group_log2(H / 4), labels, K, ld_labels, thr, 1.f / (1.f - p), rng_state, call_id, rng_used);
  return check_launch(who);
}

extern "C" int agnn_edge_pair_bwd_f32(int32_t n_rel, const agnn_edge_pair_bwd_t* rels, int32_t H, float p, const int64_t* rng_state,
                                      uint32_t call_id, agnn_stream_t stream_) {
  const char* who = "edge_pair_bwd";
  if (int rc = check_h(who, H, kMaxH)) return rc;
  if (int rc = check_segments(who, "n_rel", n_rel)) return rc;
  if (!(p >= 0.f && p < 1.f)) return fail(AGNN_EINVAL, "%s: p=%g must be in [0, 1)", who, static_cast<double>(p));
  if (n_rel == 0) return AGNN_OK;
  if (!rels) return fail(AGNN_EINVAL, "%s: rels is null", who);
  PairBwdTable tab;
  tab.n = n_rel;
  tab.pad = 0;
  const int lg = agnn::group_log2(H / 4), gpb = 256 >> lg;
  int64_t blocks = 0;
  for (int i = 0; i < n_rel; ++i) {
    const agnn_edge_pair_bwd_t& t = rels[i];
    if (int rc = check_rel(who, i, t.E, t.n, t.limit)) return rc;
    if (t.pos0 < 0) return fail(AGNN_EINVAL, "%s: relation %d: pos0=%lld is negative", who, i, (long long)t.pos0);
    const int64_t nb = (t.n + gpb - 1) / gpb;
    if (t.n > 0) {
      if (int rc = check_rows(who, kNoun, i, "da", t.da, t.ld_da, H)) return rc;
      if (t.E > 0 && t.limit > 0) {
        if (!t.s_rowptr || !t.d_rowptr) return fail(AGNN_EINVAL, "%s: relation %d: s_rowptr / d_rowptr is null", who, i);
        if (!t.s_col || !t.s_perm || !t.d_col || !t.d_perm) return fail(AGNN_EINVAL, "%s: relation %d: a col / perm array is null", who, i);
        if (int rc = check_rows(who, kNoun, i, "a", t.a, t.ld_a, H)) return rc;
        if (int rc = check_rows(who, kNoun, i, "df", t.df, t.ld_df, H)) return rc;
      }
    }
    if (int rc = check_grid(who, "workgroups", blocks + nb)) return rc;
    tab.t[i] = PairBwdDev{t.a, t.ld_a, t.df, t.ld_df, {t.s_rowptr, t.s_col, t.s_perm}, {t.d_rowptr, t.d_col, t.d_perm}, t.da, t.ld_da, t.pos0,
                          static_cast<int32_t>(t.n), static_cast<int32_t>(t.limit > 0 ? t.E : 0), static_cast<int32_t>(t.limit),
                          static_cast<int32_t>(blocks)};
    blocks += nb;
  }
  if (blocks == 0) return AGNN_OK;
  if (p > 0.f && !rng_state) return fail(AGNN_EINVAL, "%s: rng_state is null with p=%g", who, static_cast<double>(p));
  const uint32_t thr = threshold_or_none(p);
  hipLaunchKernelGGL(k_pair_bwd, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream_), tab, H / 4, lg, thr,
                     1.f / (1.f - p), rng_state, call_id);
  return check_launch(who);
}

extern "C" size_t agnn_edge_ce_workspace_bytes(int32_t n_rel, const agnn_edge_ce_t* rels) {
  if (n_rel <= 0 || n_rel > AGNN_MAX_SEG || !rels) return 0;
  return static_cast<size_t>(tiles_of_all(n_rel, rels, kTile)) * kPartWords * sizeof(uint32_t);
}

extern "C" int agnn_edge_ce_fwd_f32(int32_t n_rel, const agnn_edge_ce_t* rels, int32_t H, const float* w4, const float* b4, float smoothing,
                                    float* total, void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  const char* who = "edge_ce_fwd";
  if (int rc = check_h(who, H, kMaxH)) return rc;
  if (int rc = check_segments(who, "n_rel", n_rel)) return rc;
  if (!(smoothing >= 0.f && smoothing <= 1.f)) return fail(AGNN_EINVAL, "%s: smoothing=%g must be in [0, 1]", who, static_cast<double>(smoothing));
  if (n_rel == 0) return AGNN_OK;
  if (!rels) return fail(AGNN_EINVAL, "%s: rels is null", who);
  if (!total) return fail(AGNN_EINVAL, "%s: total is null", who);
  CeFwdTable tab;
  CeFinalTable fin;
  tab.n = fin.n = n_rel;
  tab.pad = fin.pad = 0;
  int64_t tiles = 0;
  for (int i = 0; i < n_rel; ++i) {
    const agnn_edge_ce_t& t = rels[i];
    if (int rc = check_rel(who, i, t.E, INT32_MAX, t.limit)) return rc;
    if (!t.loss || !t.inv_cnt || !t.counts) return fail(AGNN_EINVAL, "%s: relation %d: loss / inv_cnt / counts is null", who, i);
    const int64_t nt = (t.E + kTile - 1) / kTile;
    if (t.E > 0) {
      if (!t.src || !t.dst) return fail(AGNN_EINVAL, "%s: relation %d: src / dst is null", who, i);
      if (!t.logit || !t.dlogit) return fail(AGNN_EINVAL, "%s: relation %d: logit / dlogit is null", who, i);
      if ((reinterpret_cast<uintptr_t>(t.logit) & 7u) || (reinterpret_cast<uintptr_t>(t.dlogit) & 7u))
        return fail(AGNN_EALIGN, "%s: relation %d: logit / dlogit is not 8-byte aligned", who, i);
      if (t.limit > 0) {
        if (!t.label) return fail(AGNN_EINVAL, "%s: relation %d: label is null", who, i);
        if (int rc = check_rows(who, kNoun, i, "y", t.y, t.ld_y, H)) return rc;
      }
    }
    if (int rc = check_grid(who, "tiles of edges", tiles + nt)) return rc;
    tab.t[i] = CeFwdDev{t.y, t.ld_y, t.src, t.dst, t.label, t.logit, t.dlogit, static_cast<int32_t>(t.E), static_cast<int32_t>(t.limit),
                        static_cast<int32_t>(tiles), 0};
    fin.t[i] = FinalDev{t.loss, t.inv_cnt, t.counts, static_cast<int32_t>(tiles), static_cast<int32_t>(nt)};
    tiles += nt;
  }
  const size_t need = static_cast<size_t>(tiles) * kPartWords * sizeof(uint32_t);
  if (tiles > 0) {
    if (!w4 || !b4) return fail(AGNN_EINVAL, "%s: w4 / b4 is null", who);
    if (!aligned16(w4)) return fail(AGNN_EALIGN, "%s: w4 is not 16-byte aligned", who);
    if (int rc = check_workspace(who, workspace, workspace_bytes, need, 4)) return rc;
  }
  hipStream_t s = static_cast<hipStream_t>(stream_);
  uint32_t* part = static_cast<uint32_t*>(workspace);
  if (tiles > 0) {
    hipLaunchKernelGGL(k_ce_fwd, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, s, tab, H / 4, agnn::group_log2(H / 4), w4, b4, smoothing, part);
    if (int rc = check_launch(who)) return rc;
  }
  hipLaunchKernelGGL(k_ce_final, dim3(1), dim3(256), 0, s, fin, part, total);
  return check_launch("edge_ce_fwd (final pass)");
}

extern "C" size_t agnn_edge_ce_bwd_workspace_bytes(int32_t n_rel, const agnn_edge_ce_bwd_t* rels, int32_t H) {
  if (n_rel <= 0 || n_rel > AGNN_MAX_SEG || !rels || H < 4 || H > kMaxH || H % 4 != 0) return 0;
  return static_cast<size_t>(tiles_of_all(n_rel, rels, kBwdTile) * (256 >> group_log2(H / 4))) * (2 * H + 4) * sizeof(float);
}

extern "C" int agnn_edge_ce_bwd_f32(int32_t n_rel, const agnn_edge_ce_bwd_t* rels, int32_t H, const float* w4, const float* scale,
                                    float* dw4, float* db4, void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  const char* who = "edge_ce_bwd";
  if (int rc = check_h(who, H, kMaxH)) return rc;
  if (int rc = check_segments(who, "n_rel", n_rel)) return rc;
  if (n_rel == 0) return AGNN_OK;
  if (!rels) return fail(AGNN_EINVAL, "%s: rels is null", who);
  if (!dw4 || !db4) return fail(AGNN_EINVAL, "%s: dw4 / db4 is null", who);
  if (!aligned16(dw4)) return fail(AGNN_EALIGN, "%s: dw4 is not 16-byte aligned", who);
  CeBwdTable tab;
  tab.n = n_rel;
  tab.pad = 0;
  const int lg = agnn::group_log2(H / 4), gpb = 256 >> lg;
  int64_t tiles = 0;
  for (int i = 0; i < n_rel; ++i) {
    const agnn_edge_ce_bwd_t& t = rels[i];
    if (int rc = check_rel(who, i, t.E, INT32_MAX, 0)) return rc;
    const int64_t nt = (t.E + kBwdTile - 1) / kBwdTile;
    if (t.E > 0) {
      if (!t.dlogit) return fail(AGNN_EINVAL, "%s: relation %d: dlogit is null", who, i);
      if (reinterpret_cast<uintptr_t>(t.dlogit) & 7u) return fail(AGNN_EALIGN, "%s: relation %d: dlogit is not 8-byte aligned", who, i);
      if (int rc = check_rows(who, kNoun, i, "y", t.y, t.ld_y, H)) return rc;
      if (int rc = check_rows(who, kNoun, i, "dy", t.dy, t.ld_dy, H)) return rc;
    }
    if (int rc = check_grid(who, "partial slots", (tiles + nt) * gpb)) return rc;
    tab.t[i] = CeBwdDev{t.y, t.ld_y, t.dlogit, t.dy, t.ld_dy, static_cast<int32_t>(t.E), static_cast<int32_t>(tiles)};
    tiles += nt;
  }
  const int64_t S = tiles * gpb;
  const size_t need = static_cast<size_t>(S) * (2 * H + 4) * sizeof(float);
  if (tiles > 0) {
    if (!w4 || !scale) return fail(AGNN_EINVAL, "%s: w4 / scale is null", who);
    if (!aligned16(w4)) return fail(AGNN_EALIGN, "%s: w4 is not 16-byte aligned", who);
    if (int rc = check_workspace(who, workspace, workspace_bytes, need, 16)) return rc;
  }
  hipStream_t s = static_cast<hipStream_t>(stream_);
  float* slots = static_cast<float*>(workspace);
  if (tiles > 0) {
    hipLaunchKernelGGL(k_ce_bwd, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, s, tab, H / 4, lg, w4, scale, slots);
    if (int rc = check_launch(who)) return rc;
  }
  const int Wq = 2 * (H / 4) + 1;
  hipLaunchKernelGGL(k_ce_bwd_reduce, dim3(static_cast<unsigned>((Wq + 3) / 4)), dim3(256), 0, s, slots, S, H / 4, dw4, db4);
  return check_launch("edge_ce_bwd (reduction)");
}
