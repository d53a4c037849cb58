// PyG GraphNorm over the rows of a [n, C] fp32 matrix, per graph and per column, forward and backward (agnn_graphnorm_*):
//   m = mean_g(x), o = x - mean_scale * m, v = mean_g(o^2), y = weight * o / sqrt(v + eps) + bias.
// It sits between the encoder and both heads of the reference's PitchSpellingGNN (models/pitch_spelling.py:158, :222).
// The rows of graph g are rows[seg_ptr[g] .. seg_ptr[g + 1]) (the CSR of `batch`), so an unsorted batch takes the same path.
// Geometry as colnorm.hip: a workgroup owns a slab of at most kSlab positions of ONE graph x 64 columns, 16 lanes along the
// columns with one float4 each, 16 lanes down the positions, 8 float4 per thread.  The slab table (graph, first position,
// count) is written once per batch by agnn_graphnorm_slabs from seg_ptr; the grids are the host's bound ceil(n / kSlab) + G on
// the slab count, and a workgroup whose entry is empty exits.
// Forward: (a) per slab (count, mean, M2) of d = x - K, K = x[first row of the slab]; (b) one workgroup per graph and 16 columns
// joins the slabs' triples pairwise in slab order and fixed lane order (Chan, Golub, LeVeque 1979), each slab mean first moved
// to the graph's shift (K_slab - K_graph is exact for close values), then v = M2 / n + ((1 - mean_scale) m)^2, and the shift
// mean_scale * m goes to stats as hi + lo (the product's rounding error is recovered with an fma); (c) y.
// Backward: (a) per slab the sums of g * ohat, g and o; (b) per graph their join in slab order, the two per-graph constants of
// dx and the graph's three parameter-gradient terms; (c) dx, and one more row of workgroups adds the graphs' terms in a fixed
// order (lane l takes graphs l, l + 16, ... in order, then lane order).  m is neither stored nor divided out of hi + lo
// (mean_scale may be 0): it is (hi + lo) + mean_g(o).  HBM-bound; no float atomics; two runs give the same bits.
//
// Compiler figures (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; no kernel uses scratch):
//   kernel            VGPRs  SGPRs  LDS bytes
//   k_gn_slab_off        24     42      1024
//   k_gn_table           12     18         0
//   k_gn_stats           50     36      8256
//   k_gn_join            23     44      3072
//   k_gn_apply           34     23         0
//   k_gn_bwd_sums        58     44     12288
//   k_gn_bwd_join        33     28      3072
//   k_gn_bwd_apply       64     46     12288
#include <cmath>

#include "agnn_common.h"

namespace {

constexpr int kSlab = AGNN_GN_SLAB;          // positions per workgroup
constexpr int kRowLanes = 16;                // lanes down the positions
constexpr int kPer = kSlab / kRowLanes;      // positions per thread
constexpr int kTileC = 64;                   // columns per workgroup (16 float4 lanes)
constexpr int kJoinLanes = AGNN_GN_JOIN_LANES;   // lanes per column of the joins
static_assert(kPer * kRowLanes == kSlab && kRowLanes * (kTileC / 4) == 256 && kJoinLanes == 16, "tile geometry");

struct GnArgs {
  const float* x;
  int64_t ld_x;
  int32_t n, G, C, bound;
  const int32_t* seg_ptr;
  const int32_t* rows;
  const int32_t* slab_off;     // [G + 1] first slab of every graph
  const int4* table;           // [bound] (graph, first position, count, 0); count 0: no slab
};

__device__ __forceinline__ float4 ldf4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void stf4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }

// (nA, mA, qA) <- (nA, mA, qA) joined with (nB, mB, qB); q = sum of squared deviations.  An empty side changes nothing.
// The counts travel as floats: exact up to 2^24 rows in one graph, rounded join weights (relative 6e-8) beyond; the divisions by
// the graph's size use the integer.
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

// hi + lo = mean_scale * (K + m) with the product's rounding error included: p = fl(ms * K), its error by an fma, then a two-float
// sum.  Contraction is switched off here: left on, p + t and p - hi become fmas on the UNROUNDED product and count its error twice
// (the __f*_rn intrinsics are plain operators to this compiler and do not prevent it).
__device__ __forceinline__ void shift_hi_lo(float ms, float K, float m, float& hi, float& lo) {
#pragma clang fp contract(off)
  const float p = ms * K;
  const float t = fmaf(ms, m, fmaf(ms, K, -p));
  hi = p + t;
  lo = (p - hi) + t;                                    // exact remainder when |p| >= |t|; otherwise small against std anyway
}
// do - mean_scale * mean_g(do) with do = w * t rounded first, as launch (b) forms mean_g(do) by the same product: a one-row graph
// with mean_scale = 1 then gives the exact zero it has
__device__ __forceinline__ float dx_of(float w, float t, float msD) {
#pragma clang fp contract(off)
  const float d = w * t;
  return d - msD;
}

// seg_ptr is read through a clamp to [0, n], and a row index outside [0, n) is read as a row of zeros and never written: an
// inconsistent index gives wrong numbers, not an access outside the operands
__device__ __forceinline__ int gn_clamp(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }
__device__ __forceinline__ int gn_graph(const int32_t* seg_ptr, int g, int n, int& first) {
  first = gn_clamp(seg_ptr[g], n);
  const int end = gn_clamp(seg_ptr[g + 1], n);
  return end > first ? end - first : 0;
}
__device__ __forceinline__ bool gn_row_ok(int r, int n) { return static_cast<unsigned>(r) < static_cast<unsigned>(n); }

// slab_off[g] = number of slabs of the graphs before g (one workgroup; 256 graphs per round, the carry in a register)
__global__ __launch_bounds__(256) void k_gn_slab_off(const int32_t* __restrict__ seg_ptr, int G, int n, int bound,
                                                     int32_t* __restrict__ slab_off) {
  __shared__ int sm[256];
  const int t = threadIdx.x;
  int64_t carry = 0;
  for (int64_t g0 = 0; g0 < G; g0 += 256) {
    const int64_t g = g0 + t;
    int s = 0;
    if (g < G) {
      int first;
      s = (gn_graph(seg_ptr, static_cast<int>(g), n, first) + kSlab - 1) / kSlab;
    }
    sm[t] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                 // inclusive scan
      const int v = t >= d ? sm[t - d] : 0;
      __syncthreads();
      sm[t] += v;
      __syncthreads();
    }
    const int64_t before = carry + sm[t] - s;
    if (g < G) slab_off[g] = static_cast<int32_t>(before < bound ? before : bound);
    carry += sm[255];
    __syncthreads();
  }
  if (t == 0) slab_off[G] = static_cast<int32_t>(carry < bound ? carry : bound);
}

// table[s] = (graph, first position, count, 0) of slab s; (-1, 0, 0, 0) past the last slab
__global__ __launch_bounds__(256) void k_gn_table(const int32_t* __restrict__ seg_ptr, int G, int n, int bound,
                                                  const int32_t* __restrict__ slab_off, int4* __restrict__ table) {
  const int64_t s64 = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (s64 >= bound) return;
  const int s = static_cast<int>(s64);
  int4 e = make_int4(-1, 0, 0, 0);
  if (s < slab_off[G]) {
    int lo = 0, hi = G;                                 // the last g with slab_off[g] <= s (graphs without a slab are passed over)
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (slab_off[mid] <= s) lo = mid; else hi = mid;
    }
    int first;
    const int ng = gn_graph(seg_ptr, lo, n, first);
    const int64_t at = static_cast<int64_t>(s - slab_off[lo]) * kSlab;
    const int64_t left = ng - at;
    if (left > 0) e = make_int4(lo, static_cast<int>(first + at), static_cast<int>(left < kSlab ? left : kSlab), 0);
  }
  table[s] = e;
}

// part[slab][0 | 1][C] = mean | M2 of d = x - K over the slab's rows, K = x[first row of the slab]
__global__ __launch_bounds__(256) void k_gn_stats(GnArgs a, float* __restrict__ part) {
  const int4 e = a.table[blockIdx.x];
  if (e.z <= 0) return;
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = static_cast<int>(blockIdx.y) * kTileC + cl * 4;
  const bool on = c < a.C;
  const int rk = a.rows[e.y];
  const float4 K = (on && gn_row_ok(rk, a.n)) ? ldf4(a.x + rk * a.ld_x + c) : agnn::f4_zero();
  float4 v[kPer];
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int pos = rl + kRowLanes * i;
    const bool live = pos < e.z;
    const int r = live ? a.rows[e.y + pos] : 0;
    v[i] = (live && on && gn_row_ok(r, a.n)) ? sub4(ldf4(a.x + r * a.ld_x + c), K) : agnn::f4_zero();
    cnt += live ? 1 : 0;
  }
  float4 s = agnn::f4_zero();
#pragma unroll
  for (int i = 0; i < kPer; ++i) s = add4(s, v[i]);                 // positions past the end hold zeros
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
    float* pp = part + static_cast<int64_t>(blockIdx.x) * 3 * a.C;
    stf4(pp + c, m);
    stf4(pp + a.C + c, q);
  }
}

// one workgroup per (graph, 16 columns): 16 lanes take the graph's slabs l, l + 16, ... in order, then lane order; stats
__global__ __launch_bounds__(256) void k_gn_join(GnArgs a, const float* __restrict__ part, const float* __restrict__ mean_scale,
                                                 float eps, float* __restrict__ stats) {
  const int cl = threadIdx.x & 15, ln = threadIdx.x >> 4;
  const int g = static_cast<int>(blockIdx.x), j = static_cast<int>(blockIdx.y) * 16 + cl;
  int first;
  const int ng = gn_graph(a.seg_ptr, g, a.n, first);
  const int s0 = a.slab_off[g], S = a.slab_off[g + 1] - s0;
  float n = 0.f, m = 0.f, q = 0.f, Kg = 0.f;
  if (j < a.C && ng > 0) {
    const int rg = a.rows[first];
    Kg = gn_row_ok(rg, a.n) ? a.x[rg * a.ld_x + j] : 0.f;
    for (int s = ln; s < S; s += kJoinLanes) {
      const int left = ng - s * kSlab;
      const int rs = a.rows[first + s * kSlab];
      const float Ks = gn_row_ok(rs, a.n) ? a.x[rs * a.ld_x + j] : 0.f;
      const float* pp = part + static_cast<int64_t>(s0 + s) * 3 * a.C;
      chan(n, m, q, static_cast<float>(left < kSlab ? left : kSlab), (Ks - Kg) + pp[j], pp[a.C + j]);    // the mean about the graph's shift
    }
  }
  __shared__ float sn[256], smm[256], sq[256];
  sn[threadIdx.x] = n;
  smm[threadIdx.x] = m;
  sq[threadIdx.x] = q;
  __syncthreads();
  if (ln == 0 && j < a.C) {
    for (int l = 1; l < kJoinLanes; ++l) chan(n, m, q, sn[l * 16 + cl], smm[l * 16 + cl], sq[l * 16 + cl]);
    float* st = stats + static_cast<int64_t>(g) * 3 * a.C;
    float hi = 0.f, lo = 0.f, rstd = 0.f;                // a graph without rows: finite, and nothing reads them
    if (ng > 0) {
      const float ms = mean_scale[j];
      shift_hi_lo(ms, Kg, m, hi, lo);
      const float r = (1.f - ms) * (Kg + m);
      rstd = 1.f / sqrtf((q / static_cast<float>(ng) + r * r) + eps);
    }
    st[j] = hi;
    st[a.C + j] = lo;
    st[2 * a.C + j] = rstd;
  }
}

__global__ __launch_bounds__(256) void k_gn_apply(GnArgs a, const float* __restrict__ weight, const float* __restrict__ bias,
                                                  const float* __restrict__ stats, float* __restrict__ y, int64_t ld_y) {
  const int4 e = a.table[blockIdx.x];
  if (e.z <= 0) return;
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = static_cast<int>(blockIdx.y) * kTileC + cl * 4;
  if (c >= a.C) return;
  const float* st = stats + static_cast<int64_t>(e.x) * 3 * a.C;
  const float4 hi = ldf4(st + c), lo = ldf4(st + a.C + c), rs = ldf4(st + 2 * a.C + c);
  const float4 w = ldf4(weight + c), b = ldf4(bias + c);
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int pos = rl + kRowLanes * i;
    if (pos >= e.z) break;
    const int r = a.rows[e.y + pos];
    if (!gn_row_ok(r, a.n)) continue;
    const float4 o = sub4(sub4(ldf4(a.x + r * a.ld_x + c), hi), lo);
    stf4(y + r * ld_y + c, make_float4(fmaf(o.x * rs.x, w.x, b.x), fmaf(o.y * rs.y, w.y, b.y), fmaf(o.z * rs.z, w.z, b.z),
                                       fmaf(o.w * rs.w, w.w, b.w)));
  }
}

// part[slab][0 | 1 | 2][C] = sum g * ohat | sum g | sum o over the slab's rows
__global__ __launch_bounds__(256) void k_gn_bwd_sums(GnArgs a, const float* __restrict__ stats, const float* __restrict__ dy,
                                                     int64_t ld_dy, float* __restrict__ part) {
  const int4 e = a.table[blockIdx.x];
  if (e.z <= 0) return;
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = static_cast<int>(blockIdx.y) * kTileC + cl * 4;
  const bool on = c < a.C;
  float4 s1 = agnn::f4_zero(), s2 = agnn::f4_zero(), s3 = agnn::f4_zero();
  if (on) {
    const float* st = stats + static_cast<int64_t>(e.x) * 3 * a.C;
    const float4 hi = ldf4(st + c), lo = ldf4(st + a.C + c), rs = ldf4(st + 2 * a.C + c);
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int pos = rl + kRowLanes * i;
      if (pos >= e.z) break;
      const int r = a.rows[e.y + pos];
      if (!gn_row_ok(r, a.n)) continue;
      const float4 o = sub4(sub4(ldf4(a.x + r * a.ld_x + c), hi), lo);
      const float4 g = ldf4(dy + r * ld_dy + c);
      s1 = agnn::f4_madd(g, mul4(o, rs), s1);
      s2 = add4(s2, g);
      s3 = add4(s3, o);
    }
  }
  __shared__ float4 sm1[256], sm2[256], sm3[256];
  sm1[threadIdx.x] = s1;
  sm2[threadIdx.x] = s2;
  sm3[threadIdx.x] = s3;
  __syncthreads();
  if (rl == 0 && on) {
    for (int r = 1; r < kRowLanes; ++r) {                              // row-lane order
      s1 = add4(s1, sm1[r * 16 + cl]);
      s2 = add4(s2, sm2[r * 16 + cl]);
      s3 = add4(s3, sm3[r * 16 + cl]);
    }
    float* pp = part + static_cast<int64_t>(blockIdx.x) * 3 * a.C;
    stf4(pp + c, s1);
    stf4(pp + a.C + c, s2);
    stf4(pp + 2 * a.C + c, s3);
  }
}

// one workgroup per (graph, 16 columns): the slabs' sums in slab order (lanes l, l + 16, ..., then lane order);
// gconst[g][0 | 1][C] = mean_g(g * ohat) | mean_scale * mean_g(do), gterm[g][0 | 1 | 2][C] = the graph's share of dweight | dbias |
// dmean_scale
__global__ __launch_bounds__(256) void k_gn_bwd_join(GnArgs a, const float* __restrict__ part, const float* __restrict__ weight,
                                                     const float* __restrict__ mean_scale, const float* __restrict__ stats,
                                                     float* __restrict__ gconst, float* __restrict__ gterm) {
  const int cl = threadIdx.x & 15, ln = threadIdx.x >> 4;
  const int g = static_cast<int>(blockIdx.x), j = static_cast<int>(blockIdx.y) * 16 + cl;
  int first;
  const int ng = gn_graph(a.seg_ptr, g, a.n, first);
  const int s0 = a.slab_off[g], S = a.slab_off[g + 1] - s0;
  float t1 = 0.f, t2 = 0.f, t3 = 0.f;
  if (j < a.C) {
    for (int s = ln; s < S; s += kJoinLanes) {
      const float* pp = part + static_cast<int64_t>(s0 + s) * 3 * a.C;
      t1 += pp[j];
      t2 += pp[a.C + j];
      t3 += pp[2 * a.C + j];
    }
  }
  __shared__ float s1[256], s2[256], s3[256];
  s1[threadIdx.x] = t1;
  s2[threadIdx.x] = t2;
  s3[threadIdx.x] = t3;
  __syncthreads();
  if (ln == 0 && j < a.C) {
    for (int l = 1; l < kJoinLanes; ++l) {
      t1 += s1[l * 16 + cl];
      t2 += s2[l * 16 + cl];
      t3 += s3[l * 16 + cl];
    }
    float A = 0.f, msD = 0.f, dms = 0.f;
    if (ng > 0) {
      const float* st = stats + static_cast<int64_t>(g) * 3 * a.C;
      const float inv = 1.f / static_cast<float>(ng), ms = mean_scale[j], rs = st[2 * a.C + j];
      const float m = st[j] + (st[a.C + j] + t3 * inv);                // (hi + lo) + mean_g(o)
      A = t1 * inv;
      const float D = weight[j] * rs * (t2 * inv - rs * (1.f - ms) * m * A);       // mean_g(do)
      msD = ms * D;
      dms = -static_cast<float>(ng) * m * D;
    }
    float* gc = gconst + static_cast<int64_t>(g) * 2 * a.C;
    float* gt = gterm + static_cast<int64_t>(g) * 3 * a.C;
    gc[j] = A;
    gc[a.C + j] = msD;
    gt[j] = t1;
    gt[a.C + j] = t2;
    gt[2 * a.C + j] = dms;
  }
}

// dx per slab; the row of workgroups past the last slab adds the graphs' parameter-gradient terms (lane l takes graphs l, l + 16,
// ... in order, then lane order)
__global__ __launch_bounds__(256) void k_gn_bwd_apply(GnArgs a, const float* __restrict__ weight, const float* __restrict__ stats,
                                                      const float* __restrict__ dy, int64_t ld_dy, const float* __restrict__ gconst,
                                                      const float* __restrict__ gterm, float* __restrict__ dx, int64_t ld_dx,
                                                      float* __restrict__ dweight, float* __restrict__ dbias,
                                                      float* __restrict__ dmean_scale) {
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = static_cast<int>(blockIdx.y) * kTileC + cl * 4;
  if (static_cast<int>(blockIdx.x) == a.bound) {
    float4 t1 = agnn::f4_zero(), t2 = agnn::f4_zero(), t3 = agnn::f4_zero();
    if (c < a.C) {
      for (int g = rl; g < a.G; g += kRowLanes) {
        const float* gt = gterm + static_cast<int64_t>(g) * 3 * a.C;
        t1 = add4(t1, ldf4(gt + c));
        t2 = add4(t2, ldf4(gt + a.C + c));
        t3 = add4(t3, ldf4(gt + 2 * a.C + c));
      }
    }
    __shared__ float4 sm1[256], sm2[256], sm3[256];
    sm1[threadIdx.x] = t1;
    sm2[threadIdx.x] = t2;
    sm3[threadIdx.x] = t3;
    __syncthreads();
    if (rl == 0 && c < a.C) {
      for (int r = 1; r < kRowLanes; ++r) {
        t1 = add4(t1, sm1[r * 16 + cl]);
        t2 = add4(t2, sm2[r * 16 + cl]);
        t3 = add4(t3, sm3[r * 16 + cl]);
      }
      stf4(dweight + c, t1);
      stf4(dbias + c, t2);
      stf4(dmean_scale + c, t3);
    }
    return;
  }
  const int4 e = a.table[blockIdx.x];
  if (e.z <= 0 || c >= a.C) return;
  const float* st = stats + static_cast<int64_t>(e.x) * 3 * a.C;
  const float* gc = gconst + static_cast<int64_t>(e.x) * 2 * a.C;
  const float4 hi = ldf4(st + c), lo = ldf4(st + a.C + c), rs = ldf4(st + 2 * a.C + c);
  const float4 A = ldf4(gc + c), msD = ldf4(gc + a.C + c);
  const float4 w = mul4(ldf4(weight + c), rs);
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int pos = rl + kRowLanes * i;
    if (pos >= e.z) break;
    const int r = a.rows[e.y + pos];
    if (!gn_row_ok(r, a.n)) continue;
    const float4 o = sub4(sub4(ldf4(a.x + r * a.ld_x + c), hi), lo);
    const float4 g = ldf4(dy + r * ld_dy + c);
    stf4(dx + r * ld_dx + c, make_float4(dx_of(w.x, g.x - o.x * rs.x * A.x, msD.x), dx_of(w.y, g.y - o.y * rs.y * A.y, msD.y),
                                         dx_of(w.z, g.z - o.z * rs.z * A.z, msD.z), dx_of(w.w, g.w - o.w * rs.w * A.w, msD.w)));
  }
}

inline int64_t slab_bound(int64_t n, int64_t G) { return (n + kSlab - 1) / kSlab + G; }
inline int64_t off_words(int64_t G) { return (G + 1 + 3) & ~int64_t{3}; }        // slab_off, padded so that the entries are 16-byte aligned

// 1: empty work (success), 0: go on, < 0: refused
int gn_sizes(const char* who, int64_t n, int64_t G, int32_t C, bool with_C) {
  using namespace agnn;
  if (with_C && (C < 4 || (C & 3))) return fail(AGNN_EINVAL, "%s: C=%d must be a multiple of 4, at least 4", who, C);
  if (n < 0) return fail(AGNN_EINVAL, "%s: n=%lld must not be negative", who, (long long)n);
  if (G < 0) return fail(AGNN_EINVAL, "%s: G=%lld must not be negative", who, (long long)G);
  if (n > INT32_MAX) return fail(AGNN_EINVAL, "%s: n=%lld: row indices are int32", who, (long long)n);
  if (slab_bound(n, G) >= INT32_MAX) return fail(AGNN_EINVAL, "%s: n=%lld, G=%lld: more than 2^31 - 2 slabs", who, (long long)n, (long long)G);
  if (n == 0) return 1;
  if (G == 0) return fail(AGNN_EINVAL, "%s: G=0: n=%lld rows belong to no graph", who, (long long)n);
  return 0;
}

int gn_rows(const char* who, const char* name, const void* ptr, int64_t ld, int32_t C) {
  using namespace agnn;
  if (!ptr) return fail(AGNN_EINVAL, "%s: %s is null", who, name);
  if (ld < C) return fail(AGNN_EINVAL, "%s: ld_%s=%lld < C=%d", who, name, (long long)ld, C);
  if (ld & 3) return fail(AGNN_EALIGN, "%s: ld_%s=%lld is not a multiple of 4", who, name, (long long)ld);
  if (!aligned16(ptr)) return fail(AGNN_EALIGN, "%s: %s is not 16-byte aligned", who, name);
  return AGNN_OK;
}

int gn_vec(const char* who, const char* name, const void* ptr) {
  using namespace agnn;
  if (!ptr) return fail(AGNN_EINVAL, "%s: %s is null", who, name);
  if (!aligned16(ptr)) return fail(AGNN_EALIGN, "%s: %s is not 16-byte aligned", who, name);
  return AGNN_OK;
}

int gn_index(const char* who, const char* name, const void* ptr) {
  using namespace agnn;
  if (!ptr) return fail(AGNN_EINVAL, "%s: %s is null", who, name);
  if (reinterpret_cast<uintptr_t>(ptr) & 3u) return fail(AGNN_EALIGN, "%s: %s is not 4-byte aligned", who, name);
  return AGNN_OK;
}

int gn_buffer(const char* who, const char* name, const void* ptr, size_t bytes, size_t need) {
  using namespace agnn;
  if (!ptr) return fail(AGNN_EINVAL, "%s: %s is null", who, name);
  if (bytes < need) return fail(AGNN_ENOMEM, "%s: %s of %zu bytes, %zu needed", who, name, bytes, need);
  if (!aligned16(ptr)) return fail(AGNN_EALIGN, "%s: %s is not 16-byte aligned", who, name);
  return AGNN_OK;
}

int gn_common(const char* who, const float* x, int64_t ld_x, int64_t n, int64_t G, int32_t C, const int32_t* seg_ptr, const int32_t* rows,
              const int32_t* table, size_t table_bytes) {
  if (int rc = gn_rows(who, "x", x, ld_x, C)) return rc;
  if (int rc = gn_index(who, "seg_ptr", seg_ptr)) return rc;
  if (int rc = gn_index(who, "rows", rows)) return rc;
  if (int rc = gn_buffer(who, "table", table, table_bytes, agnn_graphnorm_table_bytes(n, G))) return rc;
  if ((C + 15) / 16 > 65535) return agnn::fail(AGNN_EINVAL, "%s: C=%d: more than 65535 column tiles", who, C);
  return AGNN_OK;
}

GnArgs gn_args(const float* x, int64_t ld_x, int64_t n, int64_t G, int32_t C, const int32_t* seg_ptr, const int32_t* rows,
               const int32_t* table) {
  return GnArgs{x, ld_x, static_cast<int32_t>(n), static_cast<int32_t>(G), C, static_cast<int32_t>(slab_bound(n, G)), seg_ptr, rows,
                table, reinterpret_cast<const int4*>(table + off_words(G))};
}

}  // namespace

extern "C" size_t agnn_graphnorm_table_bytes(int64_t n, int64_t G) {
  if (n <= 0 || G <= 0) return 0;
  return static_cast<size_t>(off_words(G) + 4 * slab_bound(n, G)) * sizeof(int32_t);
}

extern "C" size_t agnn_graphnorm_workspace_bytes(int64_t n, int64_t G, int32_t C) {
  if (n <= 0 || G <= 0 || C <= 0) return 0;
  return static_cast<size_t>(3 * slab_bound(n, G) + 5 * G) * static_cast<size_t>(C) * sizeof(float);
}

extern "C" int agnn_graphnorm_slabs(const int32_t* seg_ptr, int64_t n, int64_t G, int32_t* table, size_t table_bytes,
                                    agnn_stream_t stream_) {
  using namespace agnn;
  const char* who = "graphnorm_slabs";
  if (int rc = gn_sizes(who, n, G, 0, false)) return rc > 0 ? AGNN_OK : rc;
  if (int rc = gn_index(who, "seg_ptr", seg_ptr)) return rc;
  if (int rc = gn_buffer(who, "table", table, table_bytes, agnn_graphnorm_table_bytes(n, G))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  const int bound = static_cast<int>(slab_bound(n, G));
  hipLaunchKernelGGL(k_gn_slab_off, dim3(1), dim3(256), 0, s, seg_ptr, static_cast<int>(G), static_cast<int>(n), bound, table);
  hipLaunchKernelGGL(k_gn_table, dim3((bound + 255) / 256), dim3(256), 0, s, seg_ptr, static_cast<int>(G), static_cast<int>(n), bound,
                     table, reinterpret_cast<int4*>(table + off_words(G)));
  return check_launch(who);
}

extern "C" int agnn_graphnorm_fwd_f32(const float* x, int64_t ld_x, int64_t n, int64_t G, int32_t C, const int32_t* seg_ptr,
                                      const int32_t* rows, const int32_t* table, size_t table_bytes, const float* weight,
                                      const float* bias, const float* mean_scale, float eps, float* y, int64_t ld_y, float* stats,
                                      void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  const char* who = "graphnorm_fwd";
  if (int rc = gn_sizes(who, n, G, C, true)) return rc > 0 ? AGNN_OK : rc;
  if (!(eps >= 0.f)) return fail(AGNN_EINVAL, "%s: eps=%f must not be negative", who, eps);
  if (int rc = gn_common(who, x, ld_x, n, G, C, seg_ptr, rows, table, table_bytes)) return rc;
  if (int rc = gn_vec(who, "weight", weight)) return rc;
  if (int rc = gn_vec(who, "bias", bias)) return rc;
  if (int rc = gn_vec(who, "mean_scale", mean_scale)) return rc;
  if (int rc = gn_rows(who, "y", y, ld_y, C)) return rc;
  if (int rc = gn_vec(who, "stats", stats)) return rc;
  if (int rc = gn_buffer(who, "workspace", workspace, workspace_bytes, agnn_graphnorm_workspace_bytes(n, G, C))) return rc;
  const GnArgs a = gn_args(x, ld_x, n, G, C, seg_ptr, rows, table);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  const dim3 grid(static_cast<unsigned>(a.bound), static_cast<unsigned>((C + kTileC - 1) / kTileC)), block(256);
  const dim3 join(static_cast<unsigned>(G), static_cast<unsigned>((C + 15) / 16));
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(k_gn_stats, grid, block, 0, s, a, part);
  hipLaunchKernelGGL(k_gn_join, join, block, 0, s, a, part, mean_scale, eps, stats);
  hipLaunchKernelGGL(k_gn_apply, grid, block, 0, s, a, weight, bias, stats, y, ld_y);
  return check_launch(who);
}

extern "C" int agnn_graphnorm_bwd_f32(const float* x, int64_t ld_x, int64_t n, int64_t G, int32_t C, const int32_t* seg_ptr,
                                      const int32_t* rows, const int32_t* table, size_t table_bytes, const float* weight,
                                      const float* mean_scale, const float* stats, const float* dy, int64_t ld_dy, float* dx,
                                      int64_t ld_dx, float* dweight, float* dbias, float* dmean_scale, void* workspace,
                                      size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  const char* who = "graphnorm_bwd";
  if (int rc = gn_sizes(who, n, G, C, true)) return rc > 0 ? AGNN_OK : rc;
  if (int rc = gn_common(who, x, ld_x, n, G, C, seg_ptr, rows, table, table_bytes)) return rc;
  if (int rc = gn_vec(who, "weight", weight)) return rc;
  if (int rc = gn_vec(who, "mean_scale", mean_scale)) return rc;
  if (int rc = gn_vec(who, "stats", stats)) return rc;
  if (int rc = gn_rows(who, "dy", dy, ld_dy, C)) return rc;
  if (int rc = gn_rows(who, "dx", dx, ld_dx, C)) return rc;
  if (int rc = gn_vec(who, "dweight", dweight)) return rc;
  if (int rc = gn_vec(who, "dbias", dbias)) return rc;
  if (int rc = gn_vec(who, "dmean_scale", dmean_scale)) return rc;
  if (int rc = gn_buffer(who, "workspace", workspace, workspace_bytes, agnn_graphnorm_workspace_bytes(n, G, C))) return rc;
  const GnArgs a = gn_args(x, ld_x, n, G, C, seg_ptr, rows, table);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  const unsigned tiles = static_cast<unsigned>((C + kTileC - 1) / kTileC);
  const dim3 block(256), join(static_cast<unsigned>(G), static_cast<unsigned>((C + 15) / 16));
  float* part = static_cast<float*>(workspace);
  float* gconst = part + static_cast<int64_t>(a.bound) * 3 * C;
  float* gterm = gconst + G * 2 * C;
  hipLaunchKernelGGL(k_gn_bwd_sums, dim3(static_cast<unsigned>(a.bound), tiles), block, 0, s, a, stats, dy, ld_dy, part);
  hipLaunchKernelGGL(k_gn_bwd_join, join, block, 0, s, a, part, weight, mean_scale, stats, gconst, gterm);
  hipLaunchKernelGGL(k_gn_bwd_apply, dim3(static_cast<unsigned>(a.bound) + 1, tiles), block, 0, s, a, weight, stats, dy, ld_dy, gconst,
                     gterm, dx, ld_dx, dweight, dbias, dmean_scale);
  return check_launch(who);
}
