// JumpingKnowledge (reference: models/core/gnn.py:345-365) on the matrix cores: a bidirectional LSTM over the T = 2 ... 8 layer
// outputs of every note, an attention score per layer, a softmax over the layers and the weighted sum.                  (gfx950)
//
// The "batch" of this LSTM is the M = 16 000 notes and its "sequence" the 3 - 4 layers, so one time step of one direction is one
// tall fp32 GEMM,  g[M, 4h] = [x_t | h_{t-1}] * [W_ih | W_hh]^T + b_ih + b_hh,  followed by the cell.  No recurrence runs inside
// a kernel, no workgroup waits for another one, nothing is atomic: every cross-tile sum goes through a partials buffer that is
// summed in a fixed order, so two runs give the same bits.
//
// k_lstm_step is csrc/gemm.hip's k_gemm_nt<128, false, TWO> (same 128 x 128 x 16 tile, same double-buffered LDS staging with the
// global loads two steps ahead, same XCD-aware tile order, same v_mfma_f32_32x32x2_f32 main loop) with
//   * a seam at k = K0 in BOTH operands: the A rows switch from x_t (ld_x) to h_{t-1} (ld_hprev), the W rows from W_ih (ld K0) to
//     W_hh (ld h) — the four nn.LSTM parameters of a direction are read where they lie;
//   * column c of column tile j reads weight row (c / 32) * h + 32 * j + (c % 32): a tile holds all four gates (PyTorch order
//     i, f, g, o) of 32 hidden units.  That is a per-lane base pointer computed once;
//   * the wave -> tile mapping 4 x 1 instead of 2 x 2: wave w owns rows 32 w ... 32 w + 31 and all 128 columns, i.e. accumulator g
//     of a lane is gate g of ONE (row, unit) pair per register — the cell is applied in registers.
//     Why 4 x 1 and not the 2 x 2 mapping with the tile staged through LDS: both keep the 64 accumulator VGPRs; for 4 x 1 the
//     compiler (-Rpass-analysis=kernel-resource-usage) reports 168 VGPRs (160 for the first step), no scratch, 40 KiB of LDS,
//     three waves per SIMD.  Its main loop reads 5 instead of 4 LDS fragments per 16 MFMAs (1 A + 4 W), and in exchange the
//     epilogue needs no 64 KiB of LDS (which would leave two workgroups per CU where three fit now), no extra barrier and no
//     second pass over the tile.  The LDS-staged variant was not built: its GPU timing is "not measured";
//   * the epilogue: c = sigmoid(f) cprev + sigmoid(i) tanh(g~), h = sigmoid(o) tanh(c); writes hout, cout, (training) the
//     post-nonlinearity gates act[M, 4h], and one attention partial per (row, column tile), part[m, j] = sum_{u in tile j}
//     att_w[u] hout[m, u], reduced over the 32 lanes of a row in a fixed DPP order.
// hprev == NULL is the first step: K = K0, cprev = 0 — the recurrent product and the cprev read are skipped.
// One launch takes one or both directions (blockIdx.y).
// D layout of the 32 x 32 tile: lane l, register r -> row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
#include "agnn_common.h"

namespace {

using agnn::f32x16;
using agnn::f32x4;
using agnn::ld4;
using agnn::st4;

constexpr int BM = 128, BN = 128, BK = 16, LDT = BK + 4;

// __expf and an IEEE divide: deliberately not gru.hip's v_rcp_f32 variant nor gated.hip's expf one (they differ numerically; do not merge)
__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + __expf(-v)); }
__device__ __forceinline__ float tanhf_(float v) { return 2.f / (1.f + __expf(-2.f * v)) - 1.f; }

struct StepArgs {
  agnn_lstm_step_t it[2];
  int32_t tiles_n;
};

template <bool TWO>
__global__ __launch_bounds__(256, 2) void k_lstm_step(StepArgs g) {
  __shared__ __attribute__((aligned(16))) float sA[2][BM * LDT];
  __shared__ __attribute__((aligned(16))) float sB[2][BN * LDT];
  const agnn_lstm_step_t& it = g.it[blockIdx.y];
  const int M = static_cast<int>(it.M), K0 = it.K0, h = it.h;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int tile_m, tile_n;
  agnn::xcd_tile(blockIdx.x, g.tiles_n, tile_m, tile_n);
  const int row0 = tile_m * BM;
  if (row0 >= M) return;

  // global -> LDS staging: thread t moves rows (t / 4) and 64 + (t / 4), k offset 4 * (t % 4), of both operands
  const int sr = tid >> 2, sk = 4 * (tid & 3);
  const int64_t ra0 = min(row0 + sr, M - 1), ra1 = min(row0 + 64 + sr, M - 1);          // rows past M: clamped, never stored
  const float* pa0 = it.x + ra0 * it.ld_x + sk;
  const float* pa1 = it.x + ra1 * it.ld_x + sk;
  const float* qa0 = TWO ? it.hprev + ra0 * it.ld_hprev + sk : nullptr;
  const float* qa1 = TWO ? it.hprev + ra1 * it.ld_hprev + sk : nullptr;
  // tile column c -> weight row (c / 32) h + 32 tile_n + (c % 32)
  const int64_t wr0 = static_cast<int64_t>(sr >> 5) * h + 32 * tile_n + (sr & 31), wr1 = wr0 + 2 * static_cast<int64_t>(h);
  const float* pw0 = it.w_ih + wr0 * K0 + sk;
  const float* pw1 = it.w_ih + wr1 * K0 + sk;
  const float* qw0 = TWO ? it.w_hh + wr0 * h + sk : nullptr;
  const float* qw1 = TWO ? it.w_hh + wr1 * h + sk : nullptr;
#define AT(p, q, k) agnn::seam_at<TWO>(p, q, k, K0)
  const int so0 = sr * LDT + sk, so1 = (64 + sr) * LDT + sk;

  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x16{0};

  const int nk = (TWO ? K0 + h : K0) / BK;
  // two staging register sets (X: even steps, Y: odd steps), requested TWO steps ahead; fragment sets F (kk = 0) and G (kk = 8)
  f32x4 xa0, xa1, xw0, xw1, ya0, ya1, yw0, yw1;
  f32x4 fa, fb0, fb1, fb2, fb3, ga, gb0, gb1, gb2, gb3;
  const int fr = lane & 31, fk = 4 * (lane >> 5);
  const int foa = (32 * wave + fr) * LDT + fk, fob = fr * LDT + fk;
#define FRAGS(BUF, KK, A, B0, B1, B2, B3)                                                                  \
  A = ld4(&sA[BUF][foa + (KK)]);                                                                           \
  B0 = ld4(&sB[BUF][fob + (KK)]); B1 = ld4(&sB[BUF][fob + 32 * LDT + (KK)]);                               \
  B2 = ld4(&sB[BUF][fob + 64 * LDT + (KK)]); B3 = ld4(&sB[BUF][fob + 96 * LDT + (KK)]);
  const int last = (nk - 1) * BK;
  xa0 = ld4(pa0); xa1 = ld4(pa1); xw0 = ld4(pw0); xw1 = ld4(pw1);
  {
    const int k1 = min(BK, last);
    ya0 = ld4(AT(pa0, qa0, k1)); ya1 = ld4(AT(pa1, qa1, k1)); yw0 = ld4(AT(pw0, qw0, k1)); yw1 = ld4(AT(pw1, qw1, k1));
  }
  st4(&sA[0][so0], xa0); st4(&sA[0][so1], xa1); st4(&sB[0][so0], xw0); st4(&sB[0][so1], xw1);
  {
    const int k2 = min(2 * BK, last);
    xa0 = ld4(AT(pa0, qa0, k2)); xa1 = ld4(AT(pa1, qa1, k2)); xw0 = ld4(AT(pw0, qw0, k2)); xw1 = ld4(AT(pw1, qw1, k2));
  }
  __syncthreads();
  FRAGS(0, 0, fa, fb0, fb1, fb2, fb3)

#define MFMA_BLOCK(A, B0, B1, B2, B3)                                                                      \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                          \
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[j], B0[j], acc[0], 0, 0, 0);                           \
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[j], B1[j], acc[1], 0, 0, 0);                           \
    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[j], B2[j], acc[2], 0, 0, 0);                           \
    acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[j], B3[j], acc[3], 0, 0, 0);                           \
  }
  // one K step out of LDS buffer CUR, as gemm.hip's: the staging set S* (the NEXT step's operands) goes to the other buffer
  // between the two MFMA blocks and is re-requested for step KB + 3 (indices clamped to the last step: no branch around a load)
#define STEP(CUR, KB, SA0, SA1, SW0, SW1)                                                                  \
  {                                                                                                        \
    FRAGS(CUR, 8, ga, gb0, gb1, gb2, gb3)                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    MFMA_BLOCK(fa, fb0, fb1, fb2, fb3)                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    st4(&sA[(CUR) ^ 1][so0], SA0); st4(&sA[(CUR) ^ 1][so1], SA1);                                          \
    st4(&sB[(CUR) ^ 1][so0], SW0); st4(&sB[(CUR) ^ 1][so1], SW1);                                          \
    {                                                                                                      \
      const int k3 = min(((KB) + 3) * BK, last);                                                           \
      SA0 = ld4(AT(pa0, qa0, k3)); SA1 = ld4(AT(pa1, qa1, k3));                                            \
      SW0 = ld4(AT(pw0, qw0, k3)); SW1 = ld4(AT(pw1, qw1, k3));                                            \
    }                                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    MFMA_BLOCK(ga, gb0, gb1, gb2, gb3)                                                                     \
    __syncthreads();                                                                                       \
    FRAGS((CUR) ^ 1, 0, fa, fb0, fb1, fb2, fb3)                                                            \
  }
  int kb = 0;
  for (; kb + 2 <= nk; kb += 2) {
    STEP(0, kb, ya0, ya1, yw0, yw1)
    STEP(1, kb + 1, xa0, xa1, xw0, xw1)
  }
  if (kb < nk) STEP(0, kb, ya0, ya1, yw0, yw1)
#undef STEP
#undef MFMA_BLOCK
#undef FRAGS
#undef AT

  // epilogue: the cell on the four gates of (row, unit) that this lane holds; 128-byte row pieces (lanes 0..31 = 32 units)
  const int u = 32 * tile_n + (lane & 31), rh = 4 * (lane >> 5);
  const float bi = it.b_ih[u] + it.b_hh[u], bf = it.b_ih[h + u] + it.b_hh[h + u];
  const float bg = it.b_ih[2 * h + u] + it.b_hh[2 * h + u], bo = it.b_ih[3 * h + u] + it.b_hh[3 * h + u];
  const float aw = it.att_w != nullptr ? it.att_w[u] : 0.f;
  const int64_t ld_act = 4 * static_cast<int64_t>(h);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = row0 + 32 * wave + agnn::d_row32(r, 0) + rh;
    const bool live = row < M;
    const int64_t rc = min(row, M - 1);
    const float gi = sigmoidf_(acc[0][r] + bi), gf = sigmoidf_(acc[1][r] + bf);
    const float gg = tanhf_(acc[2][r] + bg), go = sigmoidf_(acc[3][r] + bo);
    float c = gi * gg;
    if (TWO) c += gf * it.cprev[rc * it.ld_cprev + u];
    const float hv = go * tanhf_(c);
    if (live) {
      it.hout[rc * it.ld_hout + u] = hv;
      it.cout[rc * it.ld_cout + u] = c;
      if (it.act != nullptr) {
        float* a = it.act + rc * ld_act + u;
        a[0] = gi; a[h] = gf; a[2 * h] = gg; a[3 * h] = go;
      }
    }
    if (it.att_w != nullptr) {                   // wave-uniform
      // fixed order: the DPP tree inside each 16-lane row, then row 0 + row 1 (lanes 0..31) and row 2 + row 3 (lanes 32..63)
      const float s = agnn::row16_sum(aw * hv);
      const float lo = agnn::lane_value(s, 0) + agnn::lane_value(s, 16), hi = agnn::lane_value(s, 32) + agnn::lane_value(s, 48);
      if (live && (lane & 31) == 0) it.part[rc * g.tiles_n + tile_n] = lane ? hi : lo;
    }
  }
}

// ---- attention over the T steps ----------------------------------------------------------------------------------------------
struct CombineArgs {
  const float* x[AGNN_JK_MAX_T];
  float* dx[AGNN_JK_MAX_T];
  int64_t ld_x[AGNN_JK_MAX_T], ld_dx[AGNN_JK_MAX_T];
  const float* part;          // [n_dir][T][M][n_tiles]
  const float* dout;
  float* out;
  float* alpha;               // [M, T]
  float* dscore;              // [M, T]
  int64_t ld_out, ld_dout, M;
  int32_t T, H, n_dir, n_tiles;
};

// one wave per row; lane t < T sums the partials of step t (direction-major, then tile order), every lane then forms the softmax
template <bool VEC>
__global__ __launch_bounds__(256) void k_jk_combine_fwd(CombineArgs g) {
  const int lane = threadIdx.x & 63;
  const int64_t m = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (m >= g.M) return;
  float sc = 0.f;
  if (lane < g.T)
    for (int d = 0; d < g.n_dir; ++d) {
      const float* p = g.part + ((static_cast<int64_t>(d) * g.T + lane) * g.M + m) * g.n_tiles;
      for (int j = 0; j < g.n_tiles; ++j) sc += p[j];
    }
  float al[AGNN_JK_MAX_T];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < AGNN_JK_MAX_T; ++t) {
    al[t] = __shfl(sc, t);
    if (t < g.T) mx = fmaxf(mx, al[t]);
  }
  float den = 0.f;
#pragma unroll
  for (int t = 0; t < AGNN_JK_MAX_T; ++t) {
    al[t] = t < g.T ? __expf(al[t] - mx) : 0.f;
    den += al[t];
  }
  const float inv = 1.f / den;
#pragma unroll
  for (int t = 0; t < AGNN_JK_MAX_T; ++t) {
    al[t] *= inv;
    if (lane == t && t < g.T) g.alpha[m * g.T + t] = al[t];
  }
  float* o = g.out + m * g.ld_out;
  if (VEC) {
    for (int c = 4 * lane; c < g.H; c += 256) {
      f32x4 a = f32x4{0};
#pragma unroll
      for (int t = 0; t < AGNN_JK_MAX_T; ++t)
        if (t < g.T) a += al[t] * *reinterpret_cast<const f32x4*>(g.x[t] + m * g.ld_x[t] + c);
      *reinterpret_cast<f32x4*>(o + c) = a;
    }
  } else {
    for (int c = lane; c < g.H; c += 64) {
      float a = 0.f;
#pragma unroll
      for (int t = 0; t < AGNN_JK_MAX_T; ++t)
        if (t < g.T) a += al[t] * g.x[t][m * g.ld_x[t] + c];
      o[c] = a;
    }
  }
}

// dalpha_t = dout . x_t (lane partials in column order, then the fixed DPP tree), dscore = alpha (dalpha - sum alpha dalpha),
// dx_t = alpha_t dout
template <bool VEC>
__global__ __launch_bounds__(256) void k_jk_combine_bwd(CombineArgs g) {
  const int lane = threadIdx.x & 63;
  const int64_t m = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (m >= g.M) return;
  const float* go = g.dout + m * g.ld_dout;
  float da[AGNN_JK_MAX_T], al[AGNN_JK_MAX_T];
#pragma unroll
  for (int t = 0; t < AGNN_JK_MAX_T; ++t) {
    float a = 0.f;
    if (t < g.T) {
      const float* x = g.x[t] + m * g.ld_x[t];
      if (VEC) {
        for (int c = 4 * lane; c < g.H; c += 256) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(x + c), d = *reinterpret_cast<const f32x4*>(go + c);
          a += v[0] * d[0]; a += v[1] * d[1]; a += v[2] * d[2]; a += v[3] * d[3];
        }
      } else {
        for (int c = lane; c < g.H; c += 64) a += x[c] * go[c];
      }
    }
    da[t] = agnn::wave_sum_dpp(a);
    al[t] = t < g.T ? g.alpha[m * g.T + t] : 0.f;
  }
  float dot = 0.f;
#pragma unroll
  for (int t = 0; t < AGNN_JK_MAX_T; ++t) dot += al[t] * da[t];
#pragma unroll
  for (int t = 0; t < AGNN_JK_MAX_T; ++t)
    if (lane == t && t < g.T) g.dscore[m * g.T + t] = al[t] * (da[t] - dot);
#pragma unroll
  for (int t = 0; t < AGNN_JK_MAX_T; ++t) {
    if (t < g.T) {
      float* dx = g.dx[t] + m * g.ld_dx[t];
      if (VEC) {
        for (int c = 4 * lane; c < g.H; c += 256) *reinterpret_cast<f32x4*>(dx + c) = al[t] * *reinterpret_cast<const f32x4*>(go + c);
      } else {
        for (int c = lane; c < g.H; c += 64) dx[c] = al[t] * go[c];
      }
    }
  }
}

// ---- cell backward -----------------------------------------------------------------------------------------------------------
constexpr int CB_ROWS = 64;      // rows per workgroup = rows per partial of the att.weight gradient

struct CellBwdArgs {
  agnn_lstm_cell_bwd_t it[2];
};

// workgroup: 64 rows x 64 units; thread (tx = t % 16: units 4 tx .. 4 tx + 3, ty = t / 16: rows ty, ty + 16, ...), 16-byte accesses
__global__ __launch_bounds__(256) void k_lstm_cell_bwd(CellBwdArgs g) {
  __shared__ __attribute__((aligned(16))) float red[16][64];
  const agnn_lstm_cell_bwd_t& it = g.it[blockIdx.z];          // grid: (row blocks, unit blocks, items)
  const int h = it.h;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int u = 64 * blockIdx.y + 4 * tx;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * CB_ROWS;
  const bool col_ok = u < h;
  f32x4 wsum = f32x4{0};
  if (col_ok) {
    const f32x4 aw = *reinterpret_cast<const f32x4*>(it.att_w + u);
    const int64_t ld4 = 4 * static_cast<int64_t>(h);
#pragma unroll
    for (int i = 0; i < CB_ROWS / 16; ++i) {
      const int64_t m = r0 + ty + 16 * i;
      if (m >= it.M) break;
#define V4(p) (*reinterpret_cast<const f32x4*>(p))
      const float* a = it.act + m * ld4 + u;
      const f32x4 gi = V4(a), gf = V4(a + h), gg = V4(a + 2 * h), go = V4(a + 3 * h);
      const f32x4 c = V4(it.c + m * it.ld_c + u);
      const float ds = it.dscore[m * it.ld_dscore];
      f32x4 dh = ds * aw;
      if (it.dh != nullptr) dh += V4(it.dh + m * it.ld_dh + u);
      f32x4 tc, dc;
#pragma unroll
      for (int k = 0; k < 4; ++k) tc[k] = tanhf_(c[k]);
      dc = dh * go * (1.f - tc * tc);
      if (it.dc_next != nullptr) dc += V4(it.dc_next + m * it.ld_dc_next + u);
      const f32x4 d_o = dh * tc;
      f32x4 d_f = f32x4{0};
      if (it.cprev != nullptr) d_f = dc * V4(it.cprev + m * it.ld_cprev + u);
#undef V4
      float* dg = it.dgates + m * ld4 + u;
      *reinterpret_cast<f32x4*>(dg) = dc * gg * gi * (1.f - gi);
      *reinterpret_cast<f32x4*>(dg + h) = d_f * gf * (1.f - gf);
      *reinterpret_cast<f32x4*>(dg + 2 * h) = dc * gi * (1.f - gg * gg);
      *reinterpret_cast<f32x4*>(dg + 3 * h) = d_o * go * (1.f - go);
      if (it.dc_prev != nullptr) *reinterpret_cast<f32x4*>(it.dc_prev + m * it.ld_dc_prev + u) = dc * gf;
      wsum += ds * (go * tc);
    }
  }
  // att.weight partial of this row block: the 16 row lanes in order
  *reinterpret_cast<f32x4*>(&red[ty][4 * tx]) = wsum;
  __syncthreads();
  if (threadIdx.x < 64) {
    const int uu = 64 * blockIdx.y + threadIdx.x;
    if (uu < h) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) s += red[k][threadIdx.x];
      it.wpart[static_cast<int64_t>(blockIdx.x) * h + uu] = s;
    }
  }
}

// out[c] = sum_r parts[r, c] in a fixed order: 8 row lanes stride the rows, then the 8 lanes in order
__global__ __launch_bounds__(256) void k_colsum_parts(const float* parts, int64_t R, int32_t cols, float* out) {
  __shared__ float red[8][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c = 32 * blockIdx.x + tx;
  float s = 0.f;
  if (c < cols)
    for (int64_t r = ty; r < R; r += 8) s += parts[r * cols + c];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && c < cols) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][tx];
    out[c] = t;
  }
}

bool al4(const void* p, int64_t ld) { return agnn::aligned16(p) && (ld & 3) == 0; }

}  // namespace

extern "C" int agnn_lstm_step_f32(int32_t n_items, const agnn_lstm_step_t* items, agnn_stream_t stream_) {
  using namespace agnn;
  if (n_items < 1 || n_items > 2 || !items) return fail(AGNN_EINVAL, "lstm_step: n_items=%d must be 1 or 2", n_items);
  const agnn_lstm_step_t& a = items[0];
  if (a.M < 0 || a.M >= (int64_t{1} << 31) || a.K0 <= 0 || a.h <= 0 || a.K0 > (1 << 20) || a.h > (1 << 20))
    return fail(AGNN_EINVAL, "lstm_step: bad sizes M=%lld K0=%d h=%d", (long long)a.M, a.K0, a.h);
  if ((a.K0 % BK) || (a.h % 32)) return fail(AGNN_EINVAL, "lstm_step: K0=%d must be a multiple of %d and h=%d of 32", a.K0, BK, a.h);
  StepArgs g{};
  for (int i = 0; i < n_items; ++i) {
    const agnn_lstm_step_t& it = items[i];
    if (it.M != a.M || it.K0 != a.K0 || it.h != a.h || (it.hprev == nullptr) != (a.hprev == nullptr))
      return fail(AGNN_EINVAL, "lstm_step: the items of one launch share M, K0, h and are at the same step");
    if (a.M == 0) continue;
    if (!it.x || !it.w_ih || !it.b_ih || !it.b_hh || !it.hout || !it.cout || (it.hprev && (!it.w_hh || !it.cprev)) || (it.att_w && !it.part))
      return fail(AGNN_EINVAL, "lstm_step: null argument");
    if (!al4(it.x, it.ld_x) || it.ld_x < it.K0 || !aligned16(it.w_ih) || (it.hprev && (!al4(it.hprev, it.ld_hprev) || it.ld_hprev < it.h || !aligned16(it.w_hh))))
      return fail(AGNN_EALIGN, "lstm_step: x, hprev and the weights must be 16-byte aligned with leading dimensions that are multiples of 4 and cover a row");
    if (it.ld_hout < it.h || it.ld_cout < it.h || (it.hprev && it.ld_cprev < it.h)) return fail(AGNN_EINVAL, "lstm_step: a leading dimension does not cover h");
    g.it[i] = it;
  }
  if (a.M == 0) return AGNN_OK;
  g.tiles_n = a.h / 32;
  const int64_t tiles_m = (a.M + BM - 1) / BM, groups = (tiles_m + 7) / 8;
  const dim3 grid(static_cast<unsigned>(groups * 8 * g.tiles_n), static_cast<unsigned>(n_items));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  if (a.hprev) hipLaunchKernelGGL((k_lstm_step<true>), grid, dim3(256), 0, s, g);
  else hipLaunchKernelGGL((k_lstm_step<false>), grid, dim3(256), 0, s, g);
  return check_launch("lstm_step");
}

namespace {
int combine_args(const char* who, int32_t T, const float* const* xs, const int64_t* ld_xs, int64_t M, int32_t H, CombineArgs& g, bool& vec) {
  using namespace agnn;
  if (T < 2 || T > AGNN_JK_MAX_T || M < 0 || M >= (int64_t{1} << 31) || H <= 0) return fail(AGNN_EINVAL, "%s: bad sizes T=%d M=%lld H=%d", who, T, (long long)M, H);
  if (M == 0) return AGNN_OK;
  if (!xs || !ld_xs) return fail(AGNN_EINVAL, "%s: null argument", who);
  vec = (H % 4) == 0;
  for (int t = 0; t < T; ++t) {
    if (!xs[t] || ld_xs[t] < H) return fail(AGNN_EINVAL, "%s: x[%d] is null or its leading dimension does not cover H", who, t);
    g.x[t] = xs[t];
    g.ld_x[t] = ld_xs[t];
    vec = vec && al4(xs[t], ld_xs[t]);
  }
  g.T = T; g.H = H; g.M = M;
  return AGNN_OK;
}
}  // namespace

extern "C" int agnn_jk_combine_fwd_f32(int32_t T, const float* const* xs, const int64_t* ld_xs, int64_t M, int32_t H, const float* part,
                                       int32_t n_dir, int32_t n_tiles, float* alpha, float* out, int64_t ld_out, agnn_stream_t stream_) {
  using namespace agnn;
  CombineArgs g{};
  bool vec = false;
  if (int rc = combine_args("jk_combine_fwd", T, xs, ld_xs, M, H, g, vec)) return rc;
  if (n_dir < 1 || n_dir > 2 || n_tiles < 1) return fail(AGNN_EINVAL, "jk_combine_fwd: bad n_dir=%d n_tiles=%d", n_dir, n_tiles);
  if (M == 0) return AGNN_OK;
  if (!part || !alpha || !out || ld_out < H) return fail(AGNN_EINVAL, "jk_combine_fwd: null argument or ld_out < H");
  g.part = part; g.n_dir = n_dir; g.n_tiles = n_tiles; g.alpha = alpha; g.out = out; g.ld_out = ld_out;
  vec = vec && al4(out, ld_out);
  const dim3 grid(static_cast<unsigned>((M + 3) / 4));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  if (vec) hipLaunchKernelGGL((k_jk_combine_fwd<true>), grid, dim3(256), 0, s, g);
  else hipLaunchKernelGGL((k_jk_combine_fwd<false>), grid, dim3(256), 0, s, g);
  return check_launch("jk_combine_fwd");
}

extern "C" int agnn_jk_combine_bwd_f32(int32_t T, const float* const* xs, const int64_t* ld_xs, int64_t M, int32_t H, const float* alpha,
                                       const float* dout, int64_t ld_dout, float* dscore, float* const* dxs, const int64_t* ld_dxs,
                                       agnn_stream_t stream_) {
  using namespace agnn;
  CombineArgs g{};
  bool vec = false;
  if (int rc = combine_args("jk_combine_bwd", T, xs, ld_xs, M, H, g, vec)) return rc;
  if (M == 0) return AGNN_OK;
  if (!alpha || !dout || !dscore || !dxs || !ld_dxs || ld_dout < H) return fail(AGNN_EINVAL, "jk_combine_bwd: null argument or ld_dout < H");
  for (int t = 0; t < T; ++t) {
    if (!dxs[t] || ld_dxs[t] < H) return fail(AGNN_EINVAL, "jk_combine_bwd: dx[%d] is null or its leading dimension does not cover H", t);
    g.dx[t] = dxs[t];
    g.ld_dx[t] = ld_dxs[t];
    vec = vec && al4(dxs[t], ld_dxs[t]);
  }
  g.alpha = const_cast<float*>(alpha); g.dout = dout; g.ld_dout = ld_dout; g.dscore = dscore;
  vec = vec && al4(dout, ld_dout);
  const dim3 grid(static_cast<unsigned>((M + 3) / 4));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  if (vec) hipLaunchKernelGGL((k_jk_combine_bwd<true>), grid, dim3(256), 0, s, g);
  else hipLaunchKernelGGL((k_jk_combine_bwd<false>), grid, dim3(256), 0, s, g);
  return check_launch("jk_combine_bwd");
}

extern "C" int64_t agnn_lstm_cell_bwd_row_blocks(int64_t M) { return M <= 0 ? 0 : (M + CB_ROWS - 1) / CB_ROWS; }

extern "C" int agnn_lstm_cell_bwd_f32(int32_t n_items, const agnn_lstm_cell_bwd_t* items, agnn_stream_t stream_) {
  using namespace agnn;
  if (n_items < 1 || n_items > 2 || !items) return fail(AGNN_EINVAL, "lstm_cell_bwd: n_items=%d must be 1 or 2", n_items);
  const agnn_lstm_cell_bwd_t& a = items[0];
  if (a.M < 0 || a.M >= (int64_t{1} << 31) || a.h <= 0 || (a.h % 4) || a.h > (1 << 20))
    return fail(AGNN_EINVAL, "lstm_cell_bwd: bad sizes M=%lld h=%d (h a multiple of 4)", (long long)a.M, a.h);
  CellBwdArgs g{};
  for (int i = 0; i < n_items; ++i) {
    const agnn_lstm_cell_bwd_t& it = items[i];
    if (it.M != a.M || it.h != a.h) return fail(AGNN_EINVAL, "lstm_cell_bwd: the items of one launch share M and h");
    if (a.M == 0) continue;
    if (!it.act || !it.c || !it.dscore || !it.att_w || !it.dgates || !it.wpart) return fail(AGNN_EINVAL, "lstm_cell_bwd: null argument");
    if (!aligned16(it.act) || !aligned16(it.dgates) || !aligned16(it.att_w) || !al4(it.c, it.ld_c) || (it.cprev && !al4(it.cprev, it.ld_cprev)) ||
        (it.dh && !al4(it.dh, it.ld_dh)) || (it.dc_next && !al4(it.dc_next, it.ld_dc_next)) || (it.dc_prev && !al4(it.dc_prev, it.ld_dc_prev)))
      return fail(AGNN_EALIGN, "lstm_cell_bwd: operands must be 16-byte aligned with leading dimensions that are multiples of 4");
    if (it.ld_c < it.h || (it.cprev && it.ld_cprev < it.h) || (it.dh && it.ld_dh < it.h) || (it.dc_next && it.ld_dc_next < it.h) ||
        (it.dc_prev && it.ld_dc_prev < it.h) || it.ld_dscore < 1)
      return fail(AGNN_EINVAL, "lstm_cell_bwd: a leading dimension does not cover its row");
    g.it[i] = it;
  }
  if (a.M == 0) return AGNN_OK;
  const dim3 grid(static_cast<unsigned>((a.M + CB_ROWS - 1) / CB_ROWS), static_cast<unsigned>((a.h + 63) / 64), static_cast<unsigned>(n_items));
  hipLaunchKernelGGL(k_lstm_cell_bwd, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), g);
  return check_launch("lstm_cell_bwd");
}

extern "C" int agnn_colsum_parts_f32(const float* parts, int64_t n_rows, int32_t n_cols, float* out, agnn_stream_t stream_) {
  using namespace agnn;
  if (n_rows < 0 || n_cols <= 0) return fail(AGNN_EINVAL, "colsum_parts: bad sizes rows=%lld cols=%d", (long long)n_rows, n_cols);
  if (!out || (n_rows > 0 && !parts)) return fail(AGNN_EINVAL, "colsum_parts: null argument");
  hipLaunchKernelGGL(k_colsum_parts, dim3(static_cast<unsigned>((n_cols + 31) / 32)), dim3(256), 0, static_cast<hipStream_t>(stream_), parts, n_rows,
                     n_cols, out);
  return check_launch("colsum_parts");
}
