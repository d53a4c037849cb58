// Multi-relation segmented gather-reduce ("hetero SpMM") for gfx950.
//
// One 64-lane wavefront owns one output row; a lane owns 4 consecutive floats of every
// 256-float chunk of the row, so a 1 KiB row (H = 256) is ONE global_load_dwordx4 per neighbour
// and one global_store_dwordx4 per relation slot.  Everything wave-uniform (row, rowptr, column
// ids, loop control, row base addresses) is kept on the scalar unit; blocks are renumbered so that
// each XCD works on a contiguous slab of rows (neighbours are close in index -> L2 hits; measured:
// FETCH_SIZE = the source matrix once).  Sums run in CSR order: bitwise reproducible, no atomics.
// HBM/L2-bound integer + fp32-add work: no MFMA here on purpose.
//
// Replaces: `h[edge_index[1]]` + torch_scatter.scatter(..., out=x.clone(), reduce='mean')
// (reference analysisgnn/models/core/gnn.py:70-74), the zero-initialised scatter_add calls
// (core/gnn.py:511,539; core/hgnn.py:406-407), PyG SAGEConv's mean aggregation
// (models/cadence.py:147-159) and the onset pooling (models/analysis.py:580-586).
#include "rowwave.h"

namespace {

struct RelTable {
  agnn_rel_t r[AGNN_MAX_SEG];
  int n_rel;
};

struct SpmmArgs {
  int32_t n_rows;
  int32_t H;
  float* out;
  int64_t ld_out;
  int64_t rel_stride;
  const float* self;
  int64_t ld_self;
  float* inv_cnt;
  int32_t col_limit;
  uint32_t flags;
  int32_t self_rows;   // rows of `self`; rows beyond take no self term (AGNN_SPMM_ROOT: the root slot may be shorter than the output)
  // the join block's two launches (k_spmm_fast7's EPI != 0; unused otherwise)
  int32_t pool_rows;   // rows at or beyond it have no neighbours
  float eps;           // EPI_JOIN: y = LayerNorm([self | out]) * gamma + beta over the 2H floats the wave holds
  const float* gamma;
  const float* beta;
  float* y;
  int64_t ld_y;
  float* mean;
  float* rstd;
  const float* self2;  // EPI_SELF2: one more addend, self2_scale[row] * self2[row]
  int64_t ld_self2;
  const float* self2_scale;
};

using namespace agnn;

// ------------------------------------------------------------------------------------------
// Generic kernel ("scalarised"): one wavefront per output row, and EVERYTHING that is the same for the 64
// lanes — row number, rowptr/rowend, column ids, edge weights, loop control, neighbour-row base
// addresses — lives on the scalar unit (s_load_* through the constant address space, SALU
// arithmetic).  The vector unit only issues what moves bytes: one global_load_dwordx4 per
// neighbour row chunk (scalar base + lane offset), 4 FMAs, one global_store_dwordx4 per slot.
// Handles every option of the C-ABI (trimming, edge weights, self-loop / column filters, any H % 4 == 0).
// History and measurements of the earlier variants: profiles/r01_spmm_kernel_study.md.
// ------------------------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) int32_t* k_i32p;
typedef const __attribute__((address_space(4))) float* k_f32p;

template <int CH, bool SHARED, bool SELF>
__global__ __launch_bounds__(256) void k_spmm_s(RelTable t, SpmmArgs a) {
  const int lane = threadIdx.x & 63;
  // wave_row<true>() and, below, the per-relation store are written out in this kernel and in k_spmm_fast7: through rowwave.h's
  // helpers some instantiations get other registers or another order (profiles/rowwave_isa_identity.md), and both kernels keep
  // the assembly they were measured with
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int vb = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);   // XCD-contiguous row slabs
  const int row = vb * 4 + wave;                                            // wave-uniform (SGPR)
  if (row >= a.n_rows) return;
  const bool mean = (a.flags & AGNN_SPMM_MEAN) != 0;
  const bool skip_self = (a.flags & AGNN_SPMM_SKIP_SELF) != 0;
  const bool accum = (a.flags & AGNN_SPMM_ACCUM) != 0;
  bool lane_on[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) lane_on[c] = chunk_on(c, lane, a.H);

  float4 selfv[SELF ? CH : 1];
  if (SELF) {
    const float* sp = a.self + static_cast<int64_t>(row) * a.ld_self;
#pragma unroll
    for (int c = 0; c < (SELF ? CH : 1); ++c) selfv[c] = chunk_load(sp, c, lane, lane_on[c]);
  }
  float4 tot[SHARED ? CH : 1];
#pragma unroll
  for (int c = 0; c < (SHARED ? CH : 1); ++c) tot[c] = f4_zero();

  for (int r = 0; r < t.n_rel; ++r) {
    const agnn_rel_t& R = t.r[r];
    const k_i32p rowptr = (k_i32p)R.rowptr;
    const k_i32p col = (k_i32p)R.col;
    const k_f32p ew = (k_f32p)R.ew;
    const k_f32p cs = (k_f32p)R.colscale;
    const float* src = R.src;
    const int64_t ld = R.ld_src;
    const int start = rowptr[row];
    const int end = (R.rowend != nullptr) ? ((k_i32p)R.rowend)[row] : rowptr[row + 1];
    float4 acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = f4_zero();
    int cnt = 0;
    for (int p = start; p < end; p += 4) {
      int ck[4];
      float wk[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ok[u] = false;
        ck[u] = 0;
        wk[u] = 1.f;
        if (p + u < end) {
          const int c0 = col[p + u];
          ok[u] = !(skip_self && c0 == row) && (c0 < a.col_limit) && (c0 >= 0);
          if (ok[u]) {
            ck[u] = c0;
            if (ew != nullptr) wk[u] = ew[p + u];
            if (cs != nullptr) wk[u] *= cs[c0];
          }
        }
      }
      float4 v[4][CH];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ok[u]) {
          const float* sp = src + static_cast<int64_t>(ck[u]) * ld;
#pragma unroll
          for (int c = 0; c < CH; ++c) v[u][c] = chunk_load(sp, c, lane, lane_on[c]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ok[u]) {
          ++cnt;
#pragma unroll
          for (int c = 0; c < CH; ++c) f4_fma(acc[c], wk[u], v[u][c]);
        }
      }
    }
    const float denom = static_cast<float>(cnt > 1 ? cnt : 1);
    if (a.inv_cnt != nullptr && lane == 0) a.inv_cnt[static_cast<int64_t>(r) * a.n_rows + row] = 1.f / denom;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (SELF) f4_add(acc[c], selfv[SELF ? c : 0]);
      if (mean) f4_div(acc[c], denom);
    }
    if (SHARED) {
#pragma unroll
      for (int c = 0; c < CH; ++c) f4_add(tot[SHARED ? c : 0], acc[c]);
    } else {
      float4* op = reinterpret_cast<float4*>(a.out + static_cast<int64_t>(row) * a.ld_out + static_cast<int64_t>(r) * a.rel_stride);
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if (!lane_on[c]) continue;
        float4 o = acc[c];
        if (accum) f4_add(o, op[c * 64 + lane]);
        op[c * 64 + lane] = o;
      }
    }
  }
  if (SHARED) {
    float* op = a.out + static_cast<int64_t>(row) * a.ld_out;
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (lane_on[c]) chunk_store(op, c, lane, tot[SHARED ? c : 0], accum);
  }
}


// ------------------------------------------------------------------------------------------
// Fast path (H exactly 256 or 512, no per-edge weight, no ACCUM: host-side check; everything else takes k_spmm_s above, same
// results up to the ulp of the v_rcp_f32 that stands for the division by the count here), straight-line index phase.  PMC on
// the generic kernel (profiles/r01_spmm_kernel_study.md): ~1000 instructions per row, the aggregation was INSTRUCTION-ISSUE
// bound (rows have ~1.6 neighbours per relation), not bandwidth bound.  PMC on this kernel's predecessor, which took the
// relations four at a time with a segment's column ids in one VGPR (second part of that study; the kernel itself is gone, its
// numbers are in the profiles): at full occupancy (8 waves / SIMD) a wave lives ~6 us, 55 % of it in s_waitcnt, and the launch
// takes two such rounds — bound by the LENGTH OF THE DEPENDENT-LOAD CHAIN of one row, not by bytes.  That chain was: per
// relation {pointer from the kernel-argument table -> rowptr[row] -> rowptr[row+1]} one after the other, then the column ids,
// then per relation {gather -> store}, with every later gather also waiting for the previous relation's store (vmcnt counts
// loads and stores in issue order).  Here:
//   * the table is a structure of arrays, so the four rowptr / rowend / col / src pointers come with one scalar load
//     each, and entries beyond n_rel repeat the last relation: no branch anywhere in the index phase;
//   * a row's end comes from its own pointer: the relation's `rowend` array when the batch is trimmed (PyG
//     trim_to_layer, what every training step of the reference passes: models/analysis.py:960-961, models/cadence.py:
//     167-173), `rowptr + 1` otherwise — the same two scalar loads either way, no branch;
//   * all four rowptr / rowend pairs are one batch of scalar loads, all four column-id vectors one batch of vector
//     loads, the first two neighbour rows of all four relations (8 loads; rows have ~1.6 neighbours per relation) one
//     batch, and the 1/deg column scales of the backward pass travel with that batch;
//   * nothing is stored before every gather of the row has been issued.
// A row therefore costs rowptr -> col -> gather.  Loads are unconditional: lanes beyond the neighbour count repeat
// the last neighbour (an L1 hit) or, for an empty segment, row 0, and what they fetch is dropped by a per-lane
// select (not a multiply by zero: a non-finite value must not leak).  Neighbours beyond the second (rare) take the
// two-at-a-time loop below the reduction: ids and scales by v_readlane from the segment's registers, or, for a row with
// more than 64 neighbours in one relation, by scalar loads.
// FILT adds the two per-edge predicates of the C-ABI (column < col_limit: the backward pass of a trimmed layer;
// column != row: the onset pooling, models/analysis.py:581-584).  They are evaluated once per column-id vector and kept
// as a 64-bit wave mask in SGPRs: a neighbour's "keep" bit is a scalar shift, the valid count one s_bcnt1.
// One row per wave: consecutive rows sharing one index phase measured slower (see launch_fast).
// EPI selects an epilogue for the join block between the encoder and project_enc (agnn_pool_cat_norm_f32 and its backward):
//   EPI_JOIN   (shared slot, self, mean): the wave holds x_i and pooled_i, i.e. the whole row u_i = [x_i | pooled_i] of the
//              concatenation in k_na_fwd's lane layout: it writes u_i, and LayerNorm(u_i) with its two statistics, in place of the
//              pooled row alone.  Rows at or beyond pool_rows have no neighbours and take pooled_i = x_i.
//   EPI_SELF2  (shared slot, root): out_i = root_i + (self2_scale[i] * self2_i + sum_r (...)), each step rounded — the pooling's
//              neighbour, self and cat gradients in one launch, summed as the three launches it replaces summed them.  Rows at or beyond pool_rows have no neighbours.
// ------------------------------------------------------------------------------------------
constexpr int EPI_NONE = 0, EPI_JOIN = 1, EPI_SELF2 = 2;
struct FastTable {
  const int32_t* rowptr[AGNN_MAX_SEG + 3];
  const int32_t* rowend[AGNN_MAX_SEG + 3];     // per-row ends: the relation's rowend array, or rowptr + 1
  const int32_t* col[AGNN_MAX_SEG + 3];
  const float* src[AGNN_MAX_SEG + 3];
  const float* colscale[AGNN_MAX_SEG + 3];
  uint32_t ldb[AGNN_MAX_SEG + 4];     // row stride in bytes (< 4 GiB, host-checked)
  int n_rel;
};

__device__ __forceinline__ int to_vgpr(int s) {
  int v;
  asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
  return v;
}

// root + (w * s + acc) with every step rounded (no fused multiply-add): k_spmm_self_grad's product and sum, then autograd's add
__device__ __forceinline__ float root_plus_self2(float root, float w, float s, float acc) {
#pragma clang fp contract(off)
  const float t = w * s;
  const float u = t + acc;
  return root + u;
}

template <int CH, bool HAS_CS, bool SHARED, bool SELF, bool FILT, int EPI = EPI_NONE>
__global__ __launch_bounds__(256) void k_spmm_fast7(FastTable t, SpmmArgs a) {
  static_assert(EPI == EPI_NONE || (SHARED && SELF && FILT), "the join block's epilogues sit on the shared-slot kernel with a self operand");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int vb = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);   // XCD-contiguous row slabs
  const int row = vb * 4 + wave;
  if (row >= a.n_rows) return;
  const bool mean = (a.flags & AGNN_SPMM_MEAN) != 0;
  const bool skip_self = FILT && (a.flags & AGNN_SPMM_SKIP_SELF) != 0;
  const uint32_t loff = static_cast<uint32_t>(lane) * 16u;

  // `self` is either the torch_scatter numerator term (added to every relation before the scale) or, with AGNN_SPMM_ROOT,
  // the root operand of a SAGE layer: an extra output slot behind the relations' (forward) / one more addend of the
  // shared sum for the rows it has (backward).  Uniform per launch: a scalar branch.
  const bool root = SELF && (a.flags & AGNN_SPMM_ROOT) != 0;
  float4 selfv[SELF ? CH : 1];
  if (SELF) {
    const bool has = row < a.self_rows;
    const char* sp = reinterpret_cast<const char*>(a.self + static_cast<int64_t>(has ? row : 0) * a.ld_self);
#pragma unroll
    for (int c = 0; c < (SELF ? CH : 1); ++c) selfv[c] = f4_keep(has, *reinterpret_cast<const float4*>(sp + (loff + c * 1024u)));
  }
  // rows without neighbours read the index of the last row that has some (in bounds) and mask its count to zero
  const int irow = EPI != EPI_NONE ? (row < a.pool_rows ? row : a.pool_rows - 1) : row;
  const int ilive = EPI != EPI_NONE ? (row < a.pool_rows ? -1 : 0) : -1;
  float4 s2v[EPI == EPI_SELF2 ? CH : 1];
  float s2w = 0.f;
  if (EPI == EPI_SELF2) {
    const char* sp = reinterpret_cast<const char*>(a.self2 + static_cast<int64_t>(row) * a.ld_self2);
#pragma unroll
    for (int c = 0; c < (EPI == EPI_SELF2 ? CH : 1); ++c) s2v[c] = *reinterpret_cast<const float4*>(sp + (loff + c * 1024u));
    s2w = ((k_f32p)a.self2_scale)[row];
  }
  float4 tot[SHARED ? CH : 1];
#pragma unroll
  for (int c = 0; c < (SHARED ? CH : 1); ++c) tot[c] = f4_zero();

  for (int r0 = 0; r0 < t.n_rel; r0 += 4) {
    // ---- index phase: no control flow; the empty asm statements pin "all pointers, then all rowptr / rowend entries,
    //      then all column ids" (left alone, the compiler sinks each scalar load to its first use: one trip per relation)
    k_i32p rpp[4], rep[4];
    const int32_t* cpp[4];
    const char* srcp[4];
    const float* csp[4];
    uint32_t ldbv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      rpp[u] = (k_i32p)t.rowptr[r0 + u];
      rep[u] = (k_i32p)t.rowend[r0 + u];
      cpp[u] = t.col[r0 + u];
      srcp[u] = reinterpret_cast<const char*>(t.src[r0 + u]);
      csp[u] = HAS_CS ? t.colscale[r0 + u] : nullptr;
      ldbv[u] = t.ldb[r0 + u];
    }
    asm volatile("" ::"s"(rpp[0]), "s"(rpp[1]), "s"(rpp[2]), "s"(rpp[3]), "s"(cpp[0]), "s"(cpp[1]), "s"(cpp[2]), "s"(cpp[3]));
    asm volatile("" ::"s"(rep[0]), "s"(rep[1]), "s"(rep[2]), "s"(rep[3]));
    asm volatile("" ::"s"(srcp[0]), "s"(srcp[1]), "s"(srcp[2]), "s"(srcp[3]), "s"(ldbv[0]), "s"(ldbv[1]), "s"(ldbv[2]), "s"(ldbv[3]));
    if (HAS_CS) asm volatile("" ::"s"(csp[0]), "s"(csp[1]), "s"(csp[2]), "s"(csp[3]));
    int beg[4], fin[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      beg[u] = rpp[u][irow];
      fin[u] = rep[u][irow];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) asm volatile("" ::"s"(beg[u]), "s"(fin[u]));
    int n[4], cntf[4];
    int colv[4];
    float wv[4];
    uint64_t okm[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int live = (r0 + u < t.n_rel ? -1 : 0) & ilive;   // mask, not a branch: the tail entries of the table are valid duplicates
      n[u] = (fin[u] - beg[u]) & live;
      colv[u] = 0;
      if (lane < n[u]) colv[u] = cpp[u][beg[u] + lane];
    }
    if (FILT) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool ok = lane < n[u] && colv[u] < a.col_limit && !(skip_self && colv[u] == row);
        okm[u] = __ballot(ok);
        colv[u] = ok ? colv[u] : 0;               // dropped neighbours are fetched from row 0 and discarded
        cntf[u] = 0;
      }
    }
#define AGNN_OVF(u) (n[u] > 64)     /* segment not (entirely) among the 64 ids held in registers */
#define AGNN_BIT(u, k) static_cast<int>((okm[u] >> (k)) & 1u)
    // the first two neighbour rows of every relation
    float4 v0[4][CH], v1[4][CH];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t ldb = ldbv[u];
      int step;                                    // 1 when the segment has >= 2 neighbours, else the second load repeats the first
      asm("s_sub_i32 %0, 1, %1\n\ts_lshr_b32 %0, %0, 31" : "=s"(step) : "s"(n[u]) : "scc");
      const uint32_t c0 = static_cast<uint32_t>(__builtin_amdgcn_readlane(colv[u], 0));
      const uint32_t c1 = static_cast<uint32_t>(__builtin_amdgcn_readlane(colv[u], step));
      const char* b0 = srcp[u] + c0 * ldb;         // column ids are non-negative: one s_mul + one s_mul_hi
      const char* b1 = srcp[u] + c1 * ldb;
#pragma unroll
      for (int c = 0; c < CH; ++c) v0[u][c] = *reinterpret_cast<const float4*>(b0 + (loff + c * 1024u));
#pragma unroll
      for (int c = 0; c < CH; ++c) v1[u][c] = *reinterpret_cast<const float4*>(b1 + (loff + c * 1024u));
      if (HAS_CS) {                                // the 1/deg scales travel with the gathers
        wv[u] = 0.f;
        if (lane < n[u]) wv[u] = csp[u][colv[u]];
      }
      __builtin_amdgcn_sched_barrier(0);           // every gather is issued before the first one is waited for, and
    }                                              // address registers are recycled from pair to pair
    // reduce (in place: v0 becomes the accumulator)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int k0s, k1s;
      if (FILT) {
        k0s = (AGNN_OVF(u) || n[u] < 1) ? 0 : AGNN_BIT(u, 0);
        k1s = (AGNN_OVF(u) || n[u] < 2) ? 0 : AGNN_BIT(u, 1);
      } else {
        const int nvs = AGNN_OVF(u) ? 0 : n[u];
        k0s = nvs > 0 ? 1 : 0;
        k1s = nvs > 1 ? 1 : 0;
      }
      const int k0v = to_vgpr(k0s), k1v = to_vgpr(k1s);
      float w0 = 1.f, w1 = 1.f;
      if (HAS_CS) {
        w0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv[u]), 0));
        w1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv[u]), 1));
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const float4 k0 = f4_keep(k0v != 0, v0[u][c]), k1 = f4_keep(k1v != 0, v1[u][c]);
        if (HAS_CS) {
          v0[u][c] = make_float4(w0 * k0.x, w0 * k0.y, w0 * k0.z, w0 * k0.w);
          f4_fma(v0[u][c], w1, k1);
        } else {
          v0[u][c] = make_float4(k0.x + k1.x, k0.y + k1.y, k0.z + k1.z, k0.w + k1.w);
        }
      }
    }
    // third and later neighbours (and segments whose ids are not in registers), two at a time
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int nn = n[u];
      if (nn > 2 || AGNN_OVF(u)) {
        const uint64_t ldb = ldbv[u];
        const bool in_regs = !AGNN_OVF(u);
        const k_i32p colg = (k_i32p)cpp[u] + beg[u];
        for (int k = in_regs ? 2 : 0; k < nn; k += 2) {
          const bool two = k + 1 < nn;
          const int ka = k, kb = two ? k + 1 : k;
          uint32_t c0, c1;
          float x0 = 1.f, x1 = 1.f;
          int keep0 = 1, keep1 = two ? 1 : 0;
          if (in_regs) {
            c0 = static_cast<uint32_t>(__builtin_amdgcn_readlane(colv[u], ka));
            c1 = static_cast<uint32_t>(__builtin_amdgcn_readlane(colv[u], kb));
            if (HAS_CS) {
              x0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv[u]), ka));
              x1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv[u]), kb));
            }
            if (FILT) {
              keep0 = AGNN_BIT(u, ka);
              keep1 &= AGNN_BIT(u, kb);
            }
          } else {                               // > 64 neighbours in this row of this relation: scalar loads
            c0 = static_cast<uint32_t>(colg[ka]);
            c1 = static_cast<uint32_t>(colg[kb]);
            if (FILT) {
              const int i0 = static_cast<int>(c0), i1 = static_cast<int>(c1);
              keep0 = (i0 < a.col_limit && !(skip_self && i0 == row)) ? 1 : 0;
              keep1 &= (i1 < a.col_limit && !(skip_self && i1 == row)) ? 1 : 0;
              c0 = keep0 ? c0 : 0u;
              c1 = keep1 ? c1 : 0u;
              cntf[u] += keep0 + keep1;
            }
            if (HAS_CS) {
              x0 = ((k_f32p)csp[u])[c0];
              x1 = ((k_f32p)csp[u])[c1];
            }
          }
          const char* b0 = srcp[u] + c0 * ldb;
          const char* b1 = srcp[u] + c1 * ldb;
          float4 q0[CH], q1[CH];
#pragma unroll
          for (int c = 0; c < CH; ++c) q0[c] = *reinterpret_cast<const float4*>(b0 + (loff + c * 1024u));
#pragma unroll
          for (int c = 0; c < CH; ++c) q1[c] = *reinterpret_cast<const float4*>(b1 + (loff + c * 1024u));
          const int k1v = to_vgpr(keep1);
          if (FILT) {
            const int k0v = to_vgpr(keep0);
#pragma unroll
            for (int c = 0; c < CH; ++c) {
              f4_fma(v0[u][c], x0, f4_keep(k0v != 0, q0[c]));
              f4_fma(v0[u][c], x1, f4_keep(k1v != 0, q1[c]));
            }
          } else {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
              f4_fma(v0[u][c], x0, q0[c]);
              f4_fma(v0[u][c], x1, f4_keep(k1v != 0, q1[c]));
            }
          }
        }
      }
    }
    // scale and store.  1 / max(count, 1) of the four relations is computed once, in lanes 0..3 (v_rcp_f32, <= 1 ulp),
    // stored by those lanes with one instruction and broadcast back as scalars.
    int nvec = 1;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int cnt = n[u];
      if (FILT) cnt = __builtin_amdgcn_readfirstlane(AGNN_OVF(u) ? cntf[u] : __builtin_popcountll(okm[u]));
      cnt = cnt > 1 ? cnt : 1;
      asm("v_writelane_b32 %0, %1, %2" : "+v"(nvec) : "s"(cnt), "n"(u));
    }
    const float invv = __builtin_amdgcn_rcpf(static_cast<float>(nvec));
    if (a.inv_cnt != nullptr && lane < 4 && r0 + lane < t.n_rel)
      a.inv_cnt[static_cast<int64_t>(r0 + lane) * a.n_rows + row] = invv;
    const float scalev = mean ? invv : 1.f;      // sums: x * 1.f is exact
    char* op = reinterpret_cast<char*>(a.out + static_cast<int64_t>(row) * a.ld_out + static_cast<int64_t>(r0) * a.rel_stride) + loff;
    const int64_t op_step = a.rel_stride * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (r0 + u >= t.n_rel) break;
      const float inv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(scalev), u));
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        float4& o = v0[u][c];
        if (SELF && !root) f4_add(o, selfv[SELF ? c : 0]);
        f4_scale(o, inv);
      }
      if (SHARED) {
#pragma unroll
        for (int c = 0; c < CH; ++c) f4_add(tot[SHARED ? c : 0], v0[u][c]);
      } else {
#pragma unroll
        for (int c = 0; c < CH; ++c) *reinterpret_cast<float4*>(op + c * 1024) = v0[u][c];
        op += op_step;
      }
    }
#undef AGNN_OVF
#undef AGNN_BIT
  }
  if (EPI == EPI_JOIN) {
    // u_i = [x_i | pooled_i]: chunks 0 .. CH-1 are the self operand, CH .. 2CH-1 the pooled row; statistics, formulas and
    // summation order are k_na_fwd<2 * CH>'s on that row
    constexpr int NV = 2 * CH;
    float4 v[NV];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      v[c] = selfv[SELF ? c : 0];
      v[CH + c] = row < a.pool_rows ? tot[SHARED ? c : 0] : selfv[SELF ? c : 0];
    }
    char* op = reinterpret_cast<char*>(a.out + static_cast<int64_t>(row) * a.ld_out);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      *reinterpret_cast<float4*>(op + (loff + c * 1024u)) = v[c];
      sum += (v[c].x + v[c].y) + (v[c].z + v[c].w);
    }
    const float invS = 1.f / static_cast<float>(2 * a.H);
    const float m = wave_sum_dpp(sum) * invS;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const float dx = v[c].x - m, dy = v[c].y - m, dz = v[c].z - m, dw = v[c].w - m;
      q += fmaf(dx, dx, dy * dy) + fmaf(dz, dz, dw * dw);     // spelled out as k_na_fwd's expression is contracted: the same bits
    }
    const float rs = 1.f / sqrtf(fmaf(wave_sum_dpp(q), invS, a.eps));
    if (lane == 0) { a.mean[row] = m; a.rstd[row] = rs; }
    char* yp = reinterpret_cast<char*>(a.y + static_cast<int64_t>(row) * a.ld_y);
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const float4 g = reinterpret_cast<const float4*>(a.gamma)[c * 64 + lane], b = reinterpret_cast<const float4*>(a.beta)[c * 64 + lane];
      *reinterpret_cast<float4*>(yp + (loff + c * 1024u)) =
          make_float4(fmaf((v[c].x - m) * rs, g.x, b.x), fmaf((v[c].y - m) * rs, g.y, b.y), fmaf((v[c].z - m) * rs, g.z, b.z), fmaf((v[c].w - m) * rs, g.w, b.w));
    }
  } else if (SHARED) {
    char* op = reinterpret_cast<char*>(a.out + static_cast<int64_t>(row) * a.ld_out);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      float4 o = tot[SHARED ? c : 0];
      if (EPI == EPI_SELF2) {
        // the order and the roundings of the three launches this one replaces: (neighbours + rounded scaled self term) + root
        const float4 s2 = s2v[EPI == EPI_SELF2 ? c : 0], rt = selfv[SELF ? c : 0];
        o.x = root_plus_self2(rt.x, s2w, s2.x, o.x);
        o.y = root_plus_self2(rt.y, s2w, s2.y, o.y);
        o.z = root_plus_self2(rt.z, s2w, s2.z, o.z);
        o.w = root_plus_self2(rt.w, s2w, s2.w, o.w);
      } else if (root) {
        f4_add(o, selfv[SELF ? c : 0]);
      }
      *reinterpret_cast<float4*>(op + (loff + c * 1024u)) = o;
    }
  } else if (root) {
    char* op = reinterpret_cast<char*>(a.out + static_cast<int64_t>(row) * a.ld_out + static_cast<int64_t>(t.n_rel) * a.rel_stride);
#pragma unroll
    for (int c = 0; c < CH; ++c) *reinterpret_cast<float4*>(op + (loff + c * 1024u)) = selfv[SELF ? c : 0];
  }
}

// the structure-of-arrays table of n_rel relations; the tail repeats the last one, so the kernel's unconditional loads stay valid
FastTable fast_table(const agnn_rel_t* rels, int n_rel) {
  FastTable f{};
  f.n_rel = n_rel;
  for (int r = 0; r < AGNN_MAX_SEG + 3; ++r) {
    const agnn_rel_t& R = rels[r < n_rel ? r : n_rel - 1];
    f.rowptr[r] = R.rowptr;
    f.rowend[r] = R.rowend != nullptr ? R.rowend : R.rowptr + 1;   // untrimmed: row i ends where row i + 1 starts
    f.col[r] = R.col;
    f.src[r] = R.src;
    f.colscale[r] = R.colscale;
    f.ldb[r] = static_cast<uint32_t>(R.ld_src * 4);
  }
  return f;
}

template <int CH>
void launch_fast(hipStream_t stream, const RelTable& t, const SpmmArgs& a, bool has_cs, bool filt) {
  const bool shared = a.rel_stride == 0, self = a.self != nullptr;
  // Rows per wave: one.  More than one (consecutive rows sharing one index phase) measured SLOWER at the C2 shape, both
  // with the rows' gathers in flight together (95 VGPRs -> 5 waves / SIMD: forward 17.1 us vs 15.5 us) and one row after
  // the other on the same registers (16.5 us; backward 18.1 vs 15.5 us): vmcnt counts in issue order, so the second
  // row's gathers cannot be consumed before the first row's stores are acknowledged, whereas a wave that ends after
  // its stores hands its slot to a new wave at once (round 1, profiles/r01_spmm_kernel_study.md).
  const dim3 grid(grid_for(a.n_rows));
  const FastTable f = fast_table(t.r, t.n_rel);
#define AGNN_FAST(CS, SH, SE)                                                                                     \
  do {                                                                                                            \
    if (filt) hipLaunchKernelGGL((k_spmm_fast7<CH, CS, SH, SE, true>), grid, dim3(256), 0, stream, f, a);         \
    else hipLaunchKernelGGL((k_spmm_fast7<CH, CS, SH, SE, false>), grid, dim3(256), 0, stream, f, a);             \
  } while (0)
  if (has_cs) {
    if (shared && self) AGNN_FAST(true, true, true); else if (shared) AGNN_FAST(true, true, false);
    else if (self) AGNN_FAST(true, false, true); else AGNN_FAST(true, false, false);
  } else {
    if (shared && self) AGNN_FAST(false, true, true); else if (shared) AGNN_FAST(false, true, false);
    else if (self) AGNN_FAST(false, false, true); else AGNN_FAST(false, false, false);
  }
#undef AGNN_FAST
}

template <int CH>
void launch_s(hipStream_t stream, const RelTable& t, const SpmmArgs& a) {
  const bool shared = a.rel_stride == 0, self = a.self != nullptr;
  const dim3 grid(grid_for(a.n_rows));
  if (shared && self) hipLaunchKernelGGL((k_spmm_s<CH, true, true>), grid, dim3(256), 0, stream, t, a);
  else if (shared) hipLaunchKernelGGL((k_spmm_s<CH, true, false>), grid, dim3(256), 0, stream, t, a);
  else if (self) hipLaunchKernelGGL((k_spmm_s<CH, false, true>), grid, dim3(256), 0, stream, t, a);
  else hipLaunchKernelGGL((k_spmm_s<CH, false, false>), grid, dim3(256), 0, stream, t, a);
}

}  // namespace

namespace {
__global__ __launch_bounds__(256) void k_spmm_self_grad(const float* __restrict__ dout, int64_t ld_dout, int64_t rel_stride, int n_rel,
                                                        const float* __restrict__ inv_cnt, int64_t ld_inv, int64_t n_rows, int H4,
                                                        float* __restrict__ out, int64_t ld_out, int accumulate) {
  const int64_t total = n_rows * H4;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t i = e / H4;
    const int c = static_cast<int>(e - i * H4) * 4;
    float4 acc = f4_zero();
    for (int r = 0; r < n_rel; ++r) {
      const float w = inv_cnt != nullptr ? inv_cnt[r * ld_inv + i] : 1.f;
      f4_fma(acc, w, *reinterpret_cast<const float4*>(dout + i * ld_dout + r * rel_stride + c));
    }
    float4* q = reinterpret_cast<float4*>(out + i * ld_out + c);
    if (accumulate) f4_add(acc, *q);
    *q = acc;
  }
}
}  // namespace

extern "C" int agnn_spmm_self_grad_f32(const float* dout, int64_t ld_dout, int64_t rel_stride, int32_t n_rel, const float* inv_cnt,
                                       int64_t ld_inv, int64_t n_rows, int32_t H, float* out, int64_t ld_out, int32_t accumulate,
                                       agnn_stream_t stream_) {
  if (n_rel <= 0 || n_rows < 0 || H <= 0 || (H & 3)) return fail(AGNN_EINVAL, "spmm_self_grad: n_rel=%d n_rows=%lld H=%d (H must be a multiple of 4)", n_rel, (long long)n_rows, H);
  if (n_rows == 0) return AGNN_OK;
  if (!dout || !out) return fail(AGNN_EINVAL, "spmm_self_grad: null argument");
  if (!f4_rows(dout, ld_dout, H) || !f4_rows(out, ld_out, H) || (rel_stride & 3))
    return fail(AGNN_EALIGN, "spmm_self_grad: operands must be 16-byte aligned with leading dimensions >= H");
  if (inv_cnt && ld_inv < n_rows) return fail(AGNN_EINVAL, "spmm_self_grad: ld_inv=%lld < n_rows", (long long)ld_inv);
  const int64_t total = n_rows * (H / 4);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_spmm_self_grad, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream_), dout, ld_dout,
                     rel_stride, n_rel, inv_cnt, ld_inv, n_rows, H / 4, out, ld_out, accumulate);
  return check_launch("spmm_self_grad");
}

namespace {
int spmm_entry(int n_rel, const agnn_rel_t* rels, int64_t n_rows, int32_t H, float* out, int64_t ld_out, int64_t rel_stride,
               const float* self, int64_t ld_self, int64_t self_rows, float* inv_cnt, int32_t col_limit, uint32_t flags,
               agnn_stream_t stream_);
}

extern "C" int agnn_spmm_f32(int n_rel, const agnn_rel_t* rels, int64_t n_rows, int32_t H, float* out,
                             int64_t ld_out, int64_t rel_stride, const float* self, int64_t ld_self,
                             float* inv_cnt, int32_t col_limit, uint32_t flags, agnn_stream_t stream_) {
  if (flags & AGNN_SPMM_ROOT) return fail(AGNN_EINVAL, "spmm: AGNN_SPMM_ROOT is agnn_spmm_root_f32's flag");
  return spmm_entry(n_rel, rels, n_rows, H, out, ld_out, rel_stride, self, ld_self, n_rows, inv_cnt, col_limit, flags, stream_);
}

extern "C" int agnn_spmm_root_f32(int n_rel, const agnn_rel_t* rels, int64_t n_rows, int32_t H, float* out, int64_t ld_out,
                                  int64_t rel_stride, const float* root, int64_t ld_root, int64_t root_rows, float* inv_cnt,
                                  int32_t col_limit, uint32_t flags, agnn_stream_t stream_) {
  if (!root || root_rows < 0) return fail(AGNN_EINVAL, "spmm_root: null root operand or root_rows=%lld", (long long)root_rows);
  if (rel_stride != 0 && root_rows < n_rows) return fail(AGNN_EINVAL, "spmm_root: the root slot needs a row per output row (root_rows=%lld < n_rows=%lld)", (long long)root_rows, (long long)n_rows);
  if (flags & (AGNN_SPMM_ACCUM | AGNN_SPMM_GENERIC)) return fail(AGNN_EINVAL, "spmm_root: flags 0x%x not supported", flags);
  if (H != 256 && H != 512) return fail(AGNN_EINVAL, "spmm_root: H=%d (256 or 512: the widths the specialised kernel is built for)", H);
  if (rel_stride != 0 && ld_out < n_rel * rel_stride + H) return fail(AGNN_EINVAL, "spmm_root: ld_out=%lld has no room for the root slot", (long long)ld_out);
  for (int r = 0; rels && r < n_rel && r < AGNN_MAX_SEG; ++r)
    if (rels[r].ew != nullptr) return fail(AGNN_EINVAL, "spmm_root: per-edge weights are not supported");
  return spmm_entry(n_rel, rels, n_rows, H, out, ld_out, rel_stride, root, ld_root, root_rows < n_rows ? root_rows : n_rows, inv_cnt,
                    col_limit, flags | AGNN_SPMM_ROOT, stream_);
}

namespace {
int spmm_entry(int n_rel, const agnn_rel_t* rels, int64_t n_rows, int32_t H, float* out, int64_t ld_out, int64_t rel_stride,
               const float* self, int64_t ld_self, int64_t self_rows, float* inv_cnt, int32_t col_limit, uint32_t flags,
               agnn_stream_t stream_) {
  if (n_rel <= 0 || n_rel > AGNN_MAX_SEG) return fail(AGNN_EINVAL, "spmm: n_rel=%d not in [1,%d]", n_rel, AGNN_MAX_SEG);
  if (int rc = check_wave_rows("spmm", n_rows, H)) return rc > 0 ? AGNN_OK : rc;
  if (!rels || !out) return fail(AGNN_EINVAL, "spmm: null argument");
  if (!aligned16(out) || (ld_out & 3) || (rel_stride & 3) || ld_out < H) return fail(AGNN_EALIGN, "spmm: out/ld_out/rel_stride must be 16-byte aligned and ld_out >= H");
  if (rel_stride != 0 && rel_stride < H) return fail(AGNN_EINVAL, "spmm: rel_stride=%lld < H", (long long)rel_stride);
  if (self && !f4_rows(self, ld_self, H)) return fail(AGNN_EALIGN, "spmm: self misaligned");
  RelTable t{};
  t.n_rel = n_rel;
  for (int r = 0; r < n_rel; ++r) {
    if (!rels[r].rowptr) return fail(AGNN_EINVAL, "spmm: relation %d has null rowptr", r);
    if (rels[r].src && !f4_rows(rels[r].src, rels[r].ld_src, H)) return fail(AGNN_EALIGN, "spmm: relation %d src misaligned or ld_src < H", r);
    t.r[r] = rels[r];
  }
  SpmmArgs a{static_cast<int32_t>(n_rows), H, out, ld_out, rel_stride, self, ld_self, inv_cnt, col_limit, flags, static_cast<int32_t>(self_rows)};
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!(flags & (AGNN_SPMM_GENERIC | AGNN_SPMM_ACCUM)) && (H == 256 || H == 512)) {
    // fast path: everything except per-edge weights and ACCUM; trimmed rows (rowend) cost nothing extra, the per-edge
    // predicates (SKIP_SELF, col_limit) select the FILT instantiation
    const bool filt = (flags & AGNN_SPMM_SKIP_SELF) != 0 || col_limit != INT32_MAX;
    bool plain = true, any_cs = false, all_cs = true;
    for (int r = 0; r < n_rel; ++r) {
      plain = plain && rels[r].ew == nullptr && rels[r].src != nullptr && rels[r].col != nullptr &&
              rels[r].ld_src < (int64_t{1} << 30);
      any_cs = any_cs || rels[r].colscale != nullptr;
      all_cs = all_cs && rels[r].colscale != nullptr;
    }
    if (plain && any_cs == all_cs) {
      if (H == 256) launch_fast<1>(stream, t, a, all_cs, filt);
      else launch_fast<2>(stream, t, a, all_cs, filt);
      return check_launch("spmm(fast)");
    }
  }
  if (flags & AGNN_SPMM_ROOT) return fail(AGNN_EINVAL, "spmm_root: this launch is outside the specialised kernel (missing src / col, or mixed column scales)");
  for_width(H, [&](auto ch) { launch_s<decltype(ch)::value>(stream, t, a); });
  return check_launch("spmm");
}
}  // namespace

// ------------------------------------------------------------------------------------------
// The join block between the encoder and project_enc (ref: models/analysis.py:580-587 and project_enc[0]).
// ------------------------------------------------------------------------------------------
namespace {
int join_check(const char* who, const agnn_rel_t* rel, int64_t n, int64_t pool_rows, int32_t H, int32_t col_limit) {
  if (H != 256 && H != 512) return fail(AGNN_EINVAL, "%s: H=%d (256 or 512: the widths the specialised kernel is built for)", who, H);
  if (n < 0 || n >= (int64_t{1} << 31) || pool_rows < 1 || pool_rows > n || col_limit < 0) return fail(AGNN_EINVAL, "%s: n=%lld pool_rows=%lld (1 <= pool_rows <= n) col_limit=%d", who, (long long)n, (long long)pool_rows, col_limit);
  if (!rel || !rel->rowptr || !rel->col) return fail(AGNN_EINVAL, "%s: null index", who);
  if (rel->ew != nullptr) return fail(AGNN_EINVAL, "%s: per-edge weights are not supported", who);
  return AGNN_OK;
}

template <int CH, bool HAS_CS, int EPI>
void launch_join(hipStream_t stream, const agnn_rel_t& R, const SpmmArgs& a) {
  hipLaunchKernelGGL((k_spmm_fast7<CH, HAS_CS, true, true, true, EPI>), dim3(grid_for(a.n_rows)), dim3(256), 0, stream, fast_table(&R, 1), a);
}
}  // namespace

extern "C" int agnn_pool_cat_norm_f32(const agnn_rel_t* rel, const float* x, int64_t ld_x, int64_t n, int64_t pool_rows, int32_t H,
                                      int32_t col_limit, const float* gamma, const float* beta, float eps, float* u, int64_t ld_u,
                                      float* y, int64_t ld_y, float* mean, float* rstd, float* inv_cnt, agnn_stream_t stream_) {
  if (n == 0) return AGNN_OK;
  if (int rc = join_check("pool_cat_norm", rel, n, pool_rows, H, col_limit)) return rc;
  if (!x || !gamma || !beta || !u || !y || !mean || !rstd) return fail(AGNN_EINVAL, "pool_cat_norm: null argument");
  if (!aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(u) || !aligned16(y) || (ld_x & 3) || (ld_u & 3) || (ld_y & 3) ||
      ld_x < H || ld_u < 2 * H || ld_y < 2 * H || ld_x >= (int64_t{1} << 30))
    return fail(AGNN_EALIGN, "pool_cat_norm: operands must be 16-byte aligned; ld_x >= H, ld_u and ld_y >= 2H, multiples of 4");
  agnn_rel_t R = *rel;
  R.src = x;
  R.ld_src = ld_x;
  R.colscale = nullptr;
  SpmmArgs a{};
  a.n_rows = static_cast<int32_t>(n);
  a.H = H;
  a.out = u;
  a.ld_out = ld_u;
  a.self = x;
  a.ld_self = ld_x;
  a.inv_cnt = inv_cnt;
  a.col_limit = col_limit;
  a.flags = AGNN_SPMM_MEAN | AGNN_SPMM_SKIP_SELF;
  a.self_rows = a.n_rows;
  a.pool_rows = static_cast<int32_t>(pool_rows);
  a.eps = eps;
  a.gamma = gamma;
  a.beta = beta;
  a.y = y;
  a.ld_y = ld_y;
  a.mean = mean;
  a.rstd = rstd;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (H == 256) launch_join<1, false, EPI_JOIN>(stream, R, a);
  else launch_join<2, false, EPI_JOIN>(stream, R, a);
  return check_launch("pool_cat_norm");
}

extern "C" int agnn_pool_cat_bwd_f32(const agnn_rel_t* rel_t, const float* du, int64_t ld_du, const float* inv_cnt, int64_t n,
                                     int64_t pool_rows, int32_t H, float* dx, int64_t ld_dx, agnn_stream_t stream_) {
  if (n == 0) return AGNN_OK;
  if (int rc = join_check("pool_cat_bwd", rel_t, n, pool_rows, H, 0)) return rc;
  if (!du || !inv_cnt || !dx) return fail(AGNN_EINVAL, "pool_cat_bwd: null argument");
  if (!aligned16(du) || !aligned16(dx) || (ld_du & 3) || (ld_dx & 3) || ld_du < 2 * H || ld_dx < H || ld_du >= (int64_t{1} << 30))
    return fail(AGNN_EALIGN, "pool_cat_bwd: operands must be 16-byte aligned; ld_du >= 2H, ld_dx >= H, multiples of 4");
  agnn_rel_t R = *rel_t;
  R.src = du + H;             // the pooled half of every row
  R.ld_src = ld_du;
  R.colscale = inv_cnt;       // 1 / count of the destination
  SpmmArgs a{};
  a.n_rows = static_cast<int32_t>(n);
  a.H = H;
  a.out = dx;
  a.ld_out = ld_dx;
  a.self = du;                // the x half: the cat's own gradient (the root operand)
  a.ld_self = ld_du;
  a.col_limit = static_cast<int32_t>(pool_rows);       // destinations the forward never computed take no part
  a.flags = AGNN_SPMM_SKIP_SELF | AGNN_SPMM_ROOT;
  a.self_rows = a.n_rows;
  a.pool_rows = static_cast<int32_t>(pool_rows);
  a.self2 = du + H;
  a.ld_self2 = ld_du;
  a.self2_scale = inv_cnt;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (H == 256) launch_join<1, true, EPI_SELF2>(stream, R, a);
  else launch_join<2, true, EPI_SELF2>(stream, R, a);
  return check_launch("pool_cat_bwd");
}
