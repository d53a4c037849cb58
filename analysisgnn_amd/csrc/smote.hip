// SMOTE oversampling of the minority classes and the feature penalty's nearest original (ref: models/cadence.py:13-118,
// models/analysis.py:1412-1438).  The reference builds a T x T similarity matrix per class, argsorts it completely and then
// walks the minority rows in a Python loop of about eight launches each; here one launch selects the rows for every class,
// one writes the oversampled batch and one starts its gradient (the neighbour term goes through agnn_spmm_f32).
//
// agnn_rowsel_f32: a workgroup of 256 lanes serves kRsQ = 16 query rows of one segment: lane = (query tid % 16, candidate slice
//   tid / 16).  The queries stay in LDS ([16][D + 4]); the segment's candidates stream through LDS in tiles of 64 rows x 64
//   columns ([64][68]), every lane accumulating its 4 candidates of the tile (rows 4 slice .. 4 slice + 3) in float4 partial sums
//   (one per column residue: a 512-term sum is four 128-term sums).  Row strides of D + 4 and 68 floats put the 16 query rows and
//   the 4 candidate rows a wave reads at once on different banks.  Each lane keeps its KP best (score, index) pairs in
//   registers, sorted, by a compare-exchange chain with static indices; the 16 slices' lists meet in LDS and one lane per query
//   merges them.  The order is lexicographic in (score, index): ties go to the lower index whatever the visiting order, and two
//   runs give the same bits.  A NaN score is never selected.  Nothing of size queries x candidates is written.
// agnn_smote_synth_fwd_f32: one lane per float4 of the [N + S, D] output: the head is a copy of x, a synthetic row is
//   x_i + gap o (x_nb - x_i); y_over is written by the lane of column 0.
// agnn_smote_synth_bwd_f32: one lane per float4 of an oversampled original: its `copies` synthetic rows are consecutive, so
//   dx_i += sum_n (1 - gap) o g is a short loop, not a scatter; W = gap o g is left for the neighbour term.
// Draws: Philox-4x32-10 with the project's (seed, step, call id) keying; element index s D/4 + d4 for the four gap values of
// columns 4 d4 .. 4 d4 + 3 of synthetic row s, 2^62 + s for the row's neighbour choice.  agnn_smote_draws_f32 exports them by
// the same device functions.
#include <cmath>

#include "agnn_common.h"

namespace {

constexpr int kRsQ = 16;        // query rows per workgroup
constexpr int kRsSlices = 16;   // candidate slices per query (256 lanes)
constexpr int kRsTile = 64;     // candidate rows per tile
constexpr int kRsDc = 64;       // columns per tile
constexpr int kRsCs = kRsDc + 4;
constexpr int kMaxD = 512;

struct RowselSegs {
  int32_t n_seg;
  int32_t q_off[AGNN_MAX_SEG + 1];
  int32_t c_off[AGNN_MAX_SEG + 1];
};

__device__ __forceinline__ bool before(float v, int j, float w, int i) { return v < w || (v == w && j < i); }

template <int KP>
__device__ __forceinline__ void insert(float (&sv)[KP], int (&si)[KP], float v, int j) {
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    const bool b = before(v, j, sv[i], si[i]);
    const float tv = sv[i];
    const int ti = si[i];
    sv[i] = b ? v : tv;
    si[i] = b ? j : ti;
    v = b ? tv : v;
    j = b ? ti : j;
  }
}

template <int KP, int MODE>
__global__ __launch_bounds__(256) void k_rowsel(const float* __restrict__ q, int64_t ld_q, const int32_t* __restrict__ q_rows, int64_t q_n,
                                                const float* __restrict__ c, int64_t ld_c, const int32_t* __restrict__ c_rows, int64_t c_n,
                                                RowselSegs segs, int D, int ksel, int32_t* __restrict__ idx, float* __restrict__ score) {
  __shared__ float4 q_s[kRsQ * (kMaxD + 4) / 4];
  __shared__ float4 c_s[kRsTile * kRsCs / 4];
  const int tid = threadIdx.x;
  // (segment, query tile) of this workgroup: the grid has one spare workgroup per segment for the ragged ends
  int seg = 0, tile = blockIdx.x;
  while (seg < segs.n_seg) {
    const int nt = (segs.q_off[seg + 1] - segs.q_off[seg] + kRsQ - 1) / kRsQ;
    if (tile < nt) break;
    tile -= nt;
    ++seg;
  }
  if (seg >= segs.n_seg) return;
  const int q0 = segs.q_off[seg] + tile * kRsQ, q1 = min(q0 + kRsQ, segs.q_off[seg + 1]);
  const int cb = segs.c_off[seg], ce = segs.c_off[seg + 1];
  const int D4 = D >> 2, qs4 = D4 + 1;
  const float nanv = __int_as_float(0x7fc00000);

  for (int e = tid; e < kRsQ * D4; e += 256) {
    const int r = e / D4, f = e - r * D4;
    float4 v = agnn::f4_zero();
    if (q0 + r < q1) {
      const int64_t row = q_rows ? q_rows[q0 + r] : q0 + r;
      v = (row >= 0 && row < q_n) ? *reinterpret_cast<const float4*>(q + row * ld_q + 4 * f) : make_float4(nanv, nanv, nanv, nanv);
    }
    q_s[r * qs4 + f] = v;
  }
  __syncthreads();
  const int ql = tid & (kRsQ - 1), slice = tid >> 4;
  float qq = 0.f;
  if (MODE == 0) {
    float4 a = agnn::f4_zero();
    for (int f = 0; f < D4; ++f) {
      const float4 v = q_s[ql * qs4 + f];
      a.x = fmaf(v.x, v.x, a.x); a.y = fmaf(v.y, v.y, a.y); a.z = fmaf(v.z, v.z, a.z); a.w = fmaf(v.w, v.w, a.w);
    }
    qq = fmaxf(sqrtf((a.x + a.y) + (a.z + a.w)), 1e-12f);
  }

  float sv[KP];
  int si[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) { sv[i] = INFINITY; si[i] = -1; }

  for (int c0 = cb; c0 < ce; c0 += kRsTile) {
    float4 acc[4], nrm[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { acc[u] = agnn::f4_zero(); nrm[u] = agnn::f4_zero(); }
    for (int d0 = 0; d0 < D4; d0 += kRsDc / 4) {
      const int w4 = min(kRsDc / 4, D4 - d0);
      __syncthreads();
      for (int e = tid; e < kRsTile * w4; e += 256) {
        const int r = e / w4, f = e - r * w4;
        float4 v = agnn::f4_zero();
        if (c0 + r < ce) {
          const int64_t row = c_rows ? c_rows[c0 + r] : c0 + r;
          v = (row >= 0 && row < c_n) ? *reinterpret_cast<const float4*>(c + row * ld_c + 4 * (d0 + f)) : make_float4(nanv, nanv, nanv, nanv);
        }
        c_s[r * (kRsCs / 4) + f] = v;
      }
      __syncthreads();
      for (int f = 0; f < w4; ++f) {
        const float4 a = q_s[ql * qs4 + d0 + f];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 b = c_s[(slice * 4 + u) * (kRsCs / 4) + f];
          if (MODE == 0) {
            acc[u].x = fmaf(a.x, b.x, acc[u].x); acc[u].y = fmaf(a.y, b.y, acc[u].y);
            acc[u].z = fmaf(a.z, b.z, acc[u].z); acc[u].w = fmaf(a.w, b.w, acc[u].w);
            nrm[u].x = fmaf(b.x, b.x, nrm[u].x); nrm[u].y = fmaf(b.y, b.y, nrm[u].y);
            nrm[u].z = fmaf(b.z, b.z, nrm[u].z); nrm[u].w = fmaf(b.w, b.w, nrm[u].w);
          } else {
            const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, dw = a.w - b.w;
            acc[u].x = fmaf(dx, dx, acc[u].x); acc[u].y = fmaf(dy, dy, acc[u].y);
            acc[u].z = fmaf(dz, dz, acc[u].z); acc[u].w = fmaf(dw, dw, acc[u].w);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = c0 + slice * 4 + u;
      float s = (acc[u].x + acc[u].y) + (acc[u].z + acc[u].w);
      if (MODE == 0) s = s / (qq * fmaxf(sqrtf((nrm[u].x + nrm[u].y) + (nrm[u].z + nrm[u].w)), 1e-12f));
      if (j < ce) insert<KP>(sv, si, s, j);
    }
  }

  // the 16 slices' lists meet in LDS (the candidate tile's space); lane `ql` of slice 0 merges its query's
  __syncthreads();
  float* m_v = reinterpret_cast<float*>(c_s);
  int* m_i = reinterpret_cast<int*>(c_s) + kRsQ * kRsSlices * KP;
  static_assert(2 * kRsQ * kRsSlices * 8 * 4 <= kRsTile * kRsCs * 4, "merge lists fit the candidate tile");
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    m_v[(ql * kRsSlices + slice) * KP + i] = sv[i];
    m_i[(ql * kRsSlices + slice) * KP + i] = si[i];
  }
  __syncthreads();
  if (tid < kRsQ && q0 + tid < q1) {
#pragma unroll
    for (int i = 0; i < KP; ++i) { sv[i] = INFINITY; si[i] = -1; }
    for (int e = 0; e < kRsSlices * KP; ++e) {
      const int j = m_i[tid * kRsSlices * KP + e];
      if (j >= 0) insert<KP>(sv, si, m_v[tid * kRsSlices * KP + e], j);
    }
    const int64_t o = static_cast<int64_t>(q0 + tid) * ksel;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      if (i < ksel) { idx[o + i] = si[i]; score[o + i] = sv[i]; }
    }
  }
}

// ---- draws ------------------------------------------------------------------------------------------------------------------
// gap of columns 4 d4 .. 4 d4 + 3 of synthetic row s: uniform on [0, 1) in steps of 2^-24
__device__ __forceinline__ float4 smote_gap4(uint64_t seed, uint64_t step, uint32_t call_id, int64_t s, int D4, int d4) {
  const uint4 r = agnn::stream_bits(seed, step, call_id, static_cast<uint64_t>(s) * static_cast<uint64_t>(D4) + static_cast<uint64_t>(d4));
  const float sc = 1.f / 16777216.f;
  return make_float4((r.x >> 8) * sc, (r.y >> 8) * sc, (r.z >> 8) * sc, (r.w >> 8) * sc);
}
// neighbour choice of synthetic row s: uniform on 0 .. k - 2 (torch.randint(0, k - 1): the k-th neighbour is never used)
__device__ __forceinline__ int smote_choice(uint64_t seed, uint64_t step, uint32_t call_id, int64_t s, int k) {
  const uint4 r = agnn::stream_bits(seed, step, call_id, (1ull << 62) + static_cast<uint64_t>(s));
  return static_cast<int>(__umulhi(r.x, static_cast<uint32_t>(k - 1)));
}

__global__ __launch_bounds__(256) void k_smote_draws(int64_t S, int D4, int k, const int64_t* __restrict__ rng, uint32_t call_id,
                                                     int32_t* __restrict__ choice, float* __restrict__ gap) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= S * D4) return;
  const int64_t s = i / D4;
  const int d4 = static_cast<int>(i - s * D4);
  const uint64_t seed = static_cast<uint64_t>(rng[0]), step = static_cast<uint64_t>(rng[1]);
  *reinterpret_cast<float4*>(gap + i * 4) = smote_gap4(seed, step, call_id, s, D4, d4);
  if (d4 == 0) choice[s] = smote_choice(seed, step, call_id, s, k);
}

__device__ __forceinline__ int plan_seg(const agnn_smote_plan_t& p, int64_t s) {
  int seg = 0;
  while (seg + 1 < p.n_seg && s >= p.s_off[seg + 1]) ++seg;
  return seg;
}

__global__ __launch_bounds__(256) void k_smote_fwd(const float* __restrict__ x, int64_t ld_x, const int64_t* __restrict__ y, int64_t N,
                                                   int D4, agnn_smote_plan_t plan, const int32_t* __restrict__ rows,
                                                   const int32_t* __restrict__ nbr, int ld_nbr, int k, const int32_t* __restrict__ choice,
                                                   const float* __restrict__ gap, const int64_t* __restrict__ rng, uint32_t call_id,
                                                   float* __restrict__ xo, int64_t ld_o, int64_t* __restrict__ yo,
                                                   int32_t* __restrict__ nb_row, int64_t* __restrict__ rng_used) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t S = plan.n_seg > 0 ? plan.s_off[plan.n_seg] : 0;
  if (i == 0 && rng != nullptr && rng_used != nullptr) { rng_used[0] = rng[0]; rng_used[1] = rng[1]; }
  if (i >= (N + S) * D4) return;
  const int64_t r = i / D4;
  const int d4 = static_cast<int>(i - r * D4);
  if (r < N) {
    *reinterpret_cast<float4*>(xo + r * ld_o + 4 * d4) = *reinterpret_cast<const float4*>(x + r * ld_x + 4 * d4);
    if (d4 == 0 && yo != nullptr) yo[r] = y[r];
    return;
  }
  const int64_t s = r - N;
  const int seg = plan_seg(plan, s);
  const int T = plan.t_off[plan.n_seg];
  const int pos = plan.t_off[seg] + static_cast<int>((s - plan.s_off[seg]) / plan.copies[seg]);
  int ch;
  float4 gp;
  if (gap != nullptr) {
    ch = choice[s];
    gp = *reinterpret_cast<const float4*>(gap + (s * D4 + d4) * 4);
  } else {
    const uint64_t seed = static_cast<uint64_t>(rng[0]), step = static_cast<uint64_t>(rng[1]);
    ch = smote_choice(seed, step, call_id, s, k);
    gp = smote_gap4(seed, step, call_id, s, D4, d4);
  }
  // rank 0 of the table (the least similar row / the row itself) is dropped, as the reference's [:, 1:k+1] does; a choice or a
  // table entry out of range leaves the row on its original
  int own = rows[pos];
  if (own < 0 || own >= N) own = 0;
  int nb = own;
  if (ch >= 0 && ch < k - 1) {
    const int np = nbr[static_cast<int64_t>(pos) * ld_nbr + 1 + ch];
    if (np >= 0 && np < T) {
      const int nr = rows[np];
      if (nr >= 0 && nr < N) nb = nr;
    }
  }
  const float4 a = *reinterpret_cast<const float4*>(x + static_cast<int64_t>(own) * ld_x + 4 * d4);
  const float4 b = *reinterpret_cast<const float4*>(x + static_cast<int64_t>(nb) * ld_x + 4 * d4);
  // a + gap * (b - a) in the reference's order of operations
  *reinterpret_cast<float4*>(xo + r * ld_o + 4 * d4) =
      make_float4(a.x + gp.x * (b.x - a.x), a.y + gp.y * (b.y - a.y), a.z + gp.z * (b.z - a.z), a.w + gp.w * (b.w - a.w));
  if (d4 == 0) {
    if (yo != nullptr) yo[r] = plan.label[seg];
    if (nb_row != nullptr) nb_row[s] = nb;
  }
}

__global__ __launch_bounds__(256) void k_smote_bwd(const float* __restrict__ g, int64_t ld_g, int64_t N, int D4, agnn_smote_plan_t plan,
                                                   const int32_t* __restrict__ rows, const float* __restrict__ gap,
                                                   const int64_t* __restrict__ rng_used, uint32_t call_id, float* __restrict__ dx,
                                                   int64_t ld_dx, float* __restrict__ w, int64_t ld_w) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int T = plan.t_off[plan.n_seg];
  if (i >= static_cast<int64_t>(T) * D4) return;
  const int pos = static_cast<int>(i / D4);
  const int d4 = static_cast<int>(i - static_cast<int64_t>(pos) * D4);
  int seg = 0;
  while (seg + 1 < plan.n_seg && pos >= plan.t_off[seg + 1]) ++seg;
  const int copies = plan.copies[seg];
  const int64_t s0 = plan.s_off[seg] + static_cast<int64_t>(pos - plan.t_off[seg]) * copies;
  uint64_t seed = 0, step = 0;
  if (gap == nullptr) { seed = static_cast<uint64_t>(rng_used[0]); step = static_cast<uint64_t>(rng_used[1]); }
  float4 a = agnn::f4_zero();
  for (int n = 0; n < copies; ++n) {
    const int64_t s = s0 + n;
    const float4 gs = *reinterpret_cast<const float4*>(g + (N + s) * ld_g + 4 * d4);
    const float4 gp = gap != nullptr ? *reinterpret_cast<const float4*>(gap + (s * D4 + d4) * 4) : smote_gap4(seed, step, call_id, s, D4, d4);
    const float4 wv = make_float4(gp.x * gs.x, gp.y * gs.y, gp.z * gs.z, gp.w * gs.w);
    *reinterpret_cast<float4*>(w + s * ld_w + 4 * d4) = wv;
    a.x += gs.x - wv.x; a.y += gs.y - wv.y; a.z += gs.z - wv.z; a.w += gs.w - wv.w;
  }
  const int own = rows[pos];
  if (own < 0 || own >= N) return;
  float4* d = reinterpret_cast<float4*>(dx + static_cast<int64_t>(own) * ld_dx + 4 * d4);
  const float4 o = *d;
  *d = make_float4(o.x + a.x, o.y + a.y, o.z + a.z, o.w + a.w);
}

int check_plan(const char* who, const agnn_smote_plan_t* p) {
  using namespace agnn;
  if (!p) return fail(AGNN_EINVAL, "%s: plan is null", who);
  if (p->n_seg < 0 || p->n_seg > AGNN_MAX_SEG) return fail(AGNN_EINVAL, "%s: plan n_seg=%d must be in [0, %d]", who, p->n_seg, AGNN_MAX_SEG);
  if (p->n_seg > 0 && (p->t_off[0] != 0 || p->s_off[0] != 0)) return fail(AGNN_EINVAL, "%s: plan offsets must start at 0", who);
  for (int i = 0; i < p->n_seg; ++i) {
    const int64_t t = static_cast<int64_t>(p->t_off[i + 1]) - p->t_off[i];
    if (t < 1 || p->copies[i] < 1) return fail(AGNN_EINVAL, "%s: plan class %d has %lld rows and copies=%d (both must be >= 1)", who, i, (long long)t, p->copies[i]);
    if (t * p->copies[i] != static_cast<int64_t>(p->s_off[i + 1]) - p->s_off[i])
      return fail(AGNN_EINVAL, "%s: plan class %d: s_off does not advance by rows * copies", who, i);
  }
  return AGNN_OK;
}

int check_d(const char* who, int32_t D) {
  if (D < 4 || D > kMaxD || D % 4 != 0) return agnn::fail(AGNN_EINVAL, "%s: D=%d must be a multiple of 4 in [4, %d]", who, D, kMaxD);
  return AGNN_OK;
}

}  // namespace

extern "C" int agnn_rowsel_f32(const float* q, int64_t ld_q, const int32_t* q_rows, int64_t q_n, const float* c, int64_t ld_c,
                               const int32_t* c_rows, int64_t c_n, int32_t n_seg, const int32_t* q_off, const int32_t* c_off, int32_t D,
                               int32_t ksel, int32_t mode, int32_t* idx, float* score, agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = check_d("rowsel", D)) return rc;
  if (ksel < 1 || ksel > AGNN_ROWSEL_MAX_K) return fail(AGNN_EINVAL, "rowsel: ksel=%d must be in [1, %d]", ksel, AGNN_ROWSEL_MAX_K);
  if (mode != AGNN_ROWSEL_COSINE && mode != AGNN_ROWSEL_SQDIST) return fail(AGNN_EINVAL, "rowsel: mode=%d is neither cosine (0) nor squared distance (1)", mode);
  if (n_seg < 0 || n_seg > AGNN_MAX_SEG) return fail(AGNN_EINVAL, "rowsel: n_seg=%d must be in [0, %d]", n_seg, AGNN_MAX_SEG);
  if (n_seg == 0) return AGNN_OK;
  if (!q_off || !c_off) return fail(AGNN_EINVAL, "rowsel: q_off / c_off is null");
  RowselSegs segs;
  segs.n_seg = n_seg;
  int64_t tiles = 0;
  for (int i = 0; i <= n_seg; ++i) {
    segs.q_off[i] = q_off[i];
    segs.c_off[i] = c_off[i];
    if (q_off[i] < 0 || c_off[i] < 0 || (i > 0 && (q_off[i] < q_off[i - 1] || c_off[i] < c_off[i - 1])))
      return fail(AGNN_EINVAL, "rowsel: q_off / c_off must be non-negative and ascending (segment %d)", i);
    if (i > 0) tiles += (q_off[i] - q_off[i - 1] + kRsQ - 1) / kRsQ;
  }
  if (tiles == 0) return AGNN_OK;
  if (q_n < 0 || c_n < 0) return fail(AGNN_EINVAL, "rowsel: q_n=%lld, c_n=%lld", (long long)q_n, (long long)c_n);
  if (!q_rows && q_off[n_seg] > q_n) return fail(AGNN_EINVAL, "rowsel: q_off ends at %d beyond q_n=%lld", q_off[n_seg], (long long)q_n);
  if (!c_rows && c_off[n_seg] > c_n) return fail(AGNN_EINVAL, "rowsel: c_off ends at %d beyond c_n=%lld", c_off[n_seg], (long long)c_n);
  if (!q || !c) return fail(AGNN_EINVAL, "rowsel: q / c is null");
  if (!idx || !score) return fail(AGNN_EINVAL, "rowsel: idx / score is null");
  if (ld_q < D) return fail(AGNN_EINVAL, "rowsel: ld_q=%lld < D=%d", (long long)ld_q, D);
  if (ld_c < D) return fail(AGNN_EINVAL, "rowsel: ld_c=%lld < D=%d", (long long)ld_c, D);
  if (ld_q % 4 != 0) return fail(AGNN_EALIGN, "rowsel: ld_q=%lld is not a multiple of 4", (long long)ld_q);
  if (ld_c % 4 != 0) return fail(AGNN_EALIGN, "rowsel: ld_c=%lld is not a multiple of 4", (long long)ld_c);
  if (!aligned16(q)) return fail(AGNN_EALIGN, "rowsel: q is not 16-byte aligned");
  if (!aligned16(c)) return fail(AGNN_EALIGN, "rowsel: c is not 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream_);
  const dim3 grid(static_cast<unsigned>(tiles));
#define AGNN_ROWSEL_LAUNCH(KP)                                                                                                     \
  do {                                                                                                                             \
    if (mode == AGNN_ROWSEL_COSINE)                                                                                                \
      hipLaunchKernelGGL((k_rowsel<KP, 0>), grid, dim3(256), 0, s, q, ld_q, q_rows, q_n, c, ld_c, c_rows, c_n, segs, D, ksel, idx, score); \
    else                                                                                                                           \
      hipLaunchKernelGGL((k_rowsel<KP, 1>), grid, dim3(256), 0, s, q, ld_q, q_rows, q_n, c, ld_c, c_rows, c_n, segs, D, ksel, idx, score); \
  } while (0)
  if (ksel == 1) AGNN_ROWSEL_LAUNCH(1);
  else if (ksel <= 4) AGNN_ROWSEL_LAUNCH(4);
  else AGNN_ROWSEL_LAUNCH(8);
#undef AGNN_ROWSEL_LAUNCH
  return check_launch("rowsel");
}

extern "C" int agnn_smote_synth_fwd_f32(const float* x, int64_t ld_x, const int64_t* y, int64_t N, int32_t D, const agnn_smote_plan_t* plan,
                                        const int32_t* rows, const int32_t* nbr, int32_t ld_nbr, int32_t k, const int32_t* choice,
                                        const float* gap, const int64_t* rng, uint32_t call_id, float* x_over, int64_t ld_over,
                                        int64_t* y_over, int32_t* nb_row, int64_t* rng_used, agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = check_d("smote_synth_fwd", D)) return rc;
  if (int rc = check_plan("smote_synth_fwd", plan)) return rc;
  if (k < 2 || k >= AGNN_ROWSEL_MAX_K) return fail(AGNN_EINVAL, "smote_synth_fwd: k=%d must be in [2, %d]", k, AGNN_ROWSEL_MAX_K - 1);
  if (N < 0 || N > INT32_MAX) return fail(AGNN_EINVAL, "smote_synth_fwd: N=%lld must be in [0, 2^31)", (long long)N);
  const int64_t S = plan->n_seg > 0 ? plan->s_off[plan->n_seg] : 0;
  if (N + S == 0) return AGNN_OK;
  if (plan->n_seg > 0 && plan->t_off[plan->n_seg] > N) return fail(AGNN_EINVAL, "smote_synth_fwd: the plan names %d rows, x has N=%lld", plan->t_off[plan->n_seg], (long long)N);
  if (!x || !x_over) return fail(AGNN_EINVAL, "smote_synth_fwd: x / x_over is null");
  if (y_over && !y) return fail(AGNN_EINVAL, "smote_synth_fwd: y_over without y");
  if (ld_x < D) return fail(AGNN_EINVAL, "smote_synth_fwd: ld_x=%lld < D=%d", (long long)ld_x, D);
  if (ld_over < D) return fail(AGNN_EINVAL, "smote_synth_fwd: ld_over=%lld < D=%d", (long long)ld_over, D);
  if (ld_x % 4 != 0) return fail(AGNN_EALIGN, "smote_synth_fwd: ld_x=%lld is not a multiple of 4", (long long)ld_x);
  if (ld_over % 4 != 0) return fail(AGNN_EALIGN, "smote_synth_fwd: ld_over=%lld is not a multiple of 4", (long long)ld_over);
  if (!aligned16(x)) return fail(AGNN_EALIGN, "smote_synth_fwd: x is not 16-byte aligned");
  if (!aligned16(x_over)) return fail(AGNN_EALIGN, "smote_synth_fwd: x_over is not 16-byte aligned");
  if (S > 0) {
    if (!rows || !nbr) return fail(AGNN_EINVAL, "smote_synth_fwd: rows / nbr is null");
    if (ld_nbr < k) return fail(AGNN_EINVAL, "smote_synth_fwd: ld_nbr=%d < k=%d (ranks 0 .. k - 1 are read)", ld_nbr, k);
    if ((choice == nullptr) != (gap == nullptr)) return fail(AGNN_EINVAL, "smote_synth_fwd: choice and gap come together or not at all");
    if (!gap && !rng) return fail(AGNN_EINVAL, "smote_synth_fwd: neither draws nor rng state given");
    if (!gap && !rng_used) return fail(AGNN_EINVAL, "smote_synth_fwd: rng_used is null");
    if (gap && !aligned16(gap)) return fail(AGNN_EALIGN, "smote_synth_fwd: gap is not 16-byte aligned");
  }
  const int64_t n4 = (N + S) * (D / 4);
  hipLaunchKernelGGL(k_smote_fwd, dim3(static_cast<unsigned>((n4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_), x, ld_x, y, N,
                     D / 4, *plan, rows, nbr, ld_nbr, k, choice, gap, gap ? nullptr : rng, call_id, x_over, ld_over, y_over, nb_row, rng_used);
  return check_launch("smote_synth_fwd");
}

extern "C" int agnn_smote_synth_bwd_f32(const float* g, int64_t ld_g, int64_t N, int32_t D, const agnn_smote_plan_t* plan, const int32_t* rows,
                                        const float* gap, const int64_t* rng_used, uint32_t call_id, float* dx, int64_t ld_dx, float* w,
                                        int64_t ld_w, agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = check_d("smote_synth_bwd", D)) return rc;
  if (int rc = check_plan("smote_synth_bwd", plan)) return rc;
  if (N < 0 || N > INT32_MAX) return fail(AGNN_EINVAL, "smote_synth_bwd: N=%lld must be in [0, 2^31)", (long long)N);
  if (plan->n_seg == 0) return AGNN_OK;
  if (plan->t_off[plan->n_seg] > N) return fail(AGNN_EINVAL, "smote_synth_bwd: the plan names %d rows, x has N=%lld", plan->t_off[plan->n_seg], (long long)N);
  if (!g || !dx || !w) return fail(AGNN_EINVAL, "smote_synth_bwd: g / dx / w is null");
  if (!rows) return fail(AGNN_EINVAL, "smote_synth_bwd: rows is null");
  if (!gap && !rng_used) return fail(AGNN_EINVAL, "smote_synth_bwd: neither gap nor rng_used given");
  if (ld_g < D || ld_dx < D || ld_w < D) return fail(AGNN_EINVAL, "smote_synth_bwd: ld_g=%lld, ld_dx=%lld, ld_w=%lld must be >= D=%d", (long long)ld_g, (long long)ld_dx, (long long)ld_w, D);
  if (ld_g % 4 != 0 || ld_dx % 4 != 0 || ld_w % 4 != 0) return fail(AGNN_EALIGN, "smote_synth_bwd: ld_g=%lld, ld_dx=%lld, ld_w=%lld must be multiples of 4", (long long)ld_g, (long long)ld_dx, (long long)ld_w);
  if (!aligned16(g) || !aligned16(dx) || !aligned16(w) || (gap && !aligned16(gap))) return fail(AGNN_EALIGN, "smote_synth_bwd: g / dx / w / gap is not 16-byte aligned");
  const int64_t n4 = static_cast<int64_t>(plan->t_off[plan->n_seg]) * (D / 4);
  hipLaunchKernelGGL(k_smote_bwd, dim3(static_cast<unsigned>((n4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_), g, ld_g, N, D / 4,
                     *plan, rows, gap, rng_used, call_id, dx, ld_dx, w, ld_w);
  return check_launch("smote_synth_bwd");
}

extern "C" int agnn_smote_draws_f32(int64_t S, int32_t D, int32_t k, const int64_t* rng, uint32_t call_id, int32_t* choice, float* gap,
                                    agnn_stream_t stream_) {
  using namespace agnn;
  if (int rc = check_d("smote_draws", D)) return rc;
  if (k < 2 || k >= AGNN_ROWSEL_MAX_K) return fail(AGNN_EINVAL, "smote_draws: k=%d must be in [2, %d]", k, AGNN_ROWSEL_MAX_K - 1);
  if (S < 0 || S > INT32_MAX) return fail(AGNN_EINVAL, "smote_draws: S=%lld must be in [0, 2^31)", (long long)S);
  if (S == 0) return AGNN_OK;
  if (!rng) return fail(AGNN_EINVAL, "smote_draws: rng is null");
  if (!choice || !gap) return fail(AGNN_EINVAL, "smote_draws: choice / gap is null");
  if (!aligned16(gap)) return fail(AGNN_EALIGN, "smote_draws: gap is not 16-byte aligned");
  const int64_t n4 = S * (D / 4);
  hipLaunchKernelGGL(k_smote_draws, dim3(static_cast<unsigned>((n4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_), S, D / 4, k, rng,
                     call_id, choice, gap);
  return check_launch("smote_draws");
}
