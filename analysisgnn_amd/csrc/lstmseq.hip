// Persistent bidirectional LSTM layer over long sequences — gfx950.
//
// The reference's `nn.LSTM(..., bidirectional=True, batch_first=True)` modules — PKSpell(cell_type="LSTM")
// (analysisgnn/models/pitch_spelling.py:50-151) and PostProcessingMLTModel (models/chord.py:751-783) — walk few sequences for
// hundreds of steps: a latency-bound chain, the opposite shape of lstm.hip's JumpingKnowledge cell (a tall GEMM per step over
// thousands of rows and 3-4 steps).  The schedule is gru.hip's: one 512-thread workgroup owns one (sequence, direction) chain
// for ALL T steps (grid 2*B), W_hh [4*HH, HH] lives in registers (128 floats per thread at HH = 128, where the GRU holds 96),
// h_{t-1} in LDS, c in a register of the unit's lane.  The input projection x W_ih^T + b_ih is a library GEMM done beforehand for
// all steps at once; the backward kernel walks the chain in reverse with W_hh^T in registers and emits ONE dg [B, T, 2, 4*HH]:
// an LSTM adds its input-side and hidden-side pre-activations before the non-linearity, so both have the same gradient and
// one matrix feeds dW_ih, dW_hh and both bias gradients (the GRU needs two: its n gate multiplies the hidden side by r).
// A time step is two phases with an LDS-only barrier after each; the step's operands come through gru.hip's loader role and
// LDS ring (the same four-slot ring, eight register sets forward; see k_lstm_seq_bwd for the backward's count).
// fp32 throughout (gru.hip's v_exp / v_rcp gate functions, ~3 ulp), no atomics, partial sums added in a fixed order: the same
// bits on every run.  Gate order i, f, g, o (torch).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage).  As built every kernel reports 256 VGPRs
// and 2 waves / SIMD, because it claims v255 (CLAIM_SIMD_REGISTERS); "VGPRs" below is what the allocator needs without the claim:
//   kernel                         VGPRs  SGPRs  scratch  LDS bytes
//   k_lstm_seq_fwd<128>              236     37        0      19456
//   k_lstm_seq_fwd<64>               108     37        0      13824
//   k_lstm_seq_bwd<128, true>        252     54        0      22528
//   k_lstm_seq_bwd<128, false>       252     38        0      22528
//   k_lstm_seq_bwd<64, true>         214     50        0      11264
//   k_lstm_seq_bwd<64, false>        214     38        0      11264
// 128 weight registers plus the working set fit 256 VGPRs at 512 threads, so no 1024-thread split was needed — in the backward
// kernel at HH = 128 only after three changes, each of which removed a spill to scratch (40-350 bytes per lane before): four
// loader register sets instead of eight, c_{t-1} taken from the next set's c_t instead of loaded, and the h_{t-1} copy moved
// from the loader to the storer lanes (see k_lstm_seq_bwd).
// Measured (scripts/time_lstm_seq.py, profiles/lstm_seq.md; B = 32, T = 500): forward 0.64 us per time step at HH = 128 (the GRU:
// 0.61) and 0.46 at HH = 64, backward 0.60 / 0.43.
#include "agnn_common.h"

// As in gru.hip: the recurrence is bound by VALU issue latency, and another kernel's waves on the same SIMD slow it down.
// Declaring v255 used makes every wave allocate 256 VGPRs, so the workgroup's 8 waves own their CU's register file.
#define CLAIM_SIMD_REGISTERS() asm volatile("" ::: "v255")

namespace {

// hidden size per direction: template parameter HH, 128 or 64.  256 does not fit a CU: W_hh = 1024 x 256 fp32 = 1 MiB against
// 512 KiB of registers + 160 KiB of LDS.
constexpr int NT = 512;        // threads per chain: 8 waves
constexpr int KC = 8;
using agnn::f32x2;

// Workgroup barrier that orders LDS traffic only (gru.hip): `__syncthreads()` would also wait for every outstanding global
// load / store and put a memory round trip on the critical path of EVERY time step.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// gru.hip's gate functions, copied so that the two recurrences round alike (v_exp_f32 and v_rcp_f32: ~3 ulp for sigmoid, 5
// instructions instead of ~40).  They sit on the serial chain of every step.  Not lstm.hip's IEEE-divide variant.
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return 2.f * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * x)) - 1.f; }

// gi   [B, T, 2, 4*HH]  x W_ih^T + b_ih, gate order i, f, g, o
// w_hh [2, 4*HH, HH], b_hh [2, 4*HH]
// y    [B, T, 2*HH]
// saved[B, T, 2, 5, HH]  = i, f, g, o (after their non-linearities), c_t
// ---- forward ---------------------------------------------------------------------------------------------------------
//   phase 1 (all 8 waves; wave = one k chunk of W_hh and one block of its rows, lane = four rows): the wave's h chunk from LDS
//            (one address for all lanes), 64 (HH = 128) / 16 (HH = 64) packed FMAs, four partial sums to LDS (part[ks][row]);
//   phase 2 (waves 0 and 1 — wave 0 alone at HH = 64 — one lane per hidden unit): add the KS partials per gate in a fixed
//            order, the four gates, c_t (a register of this lane), h_t to LDS, the seven outputs to memory.
// The unit lanes issue no global load: a LOADER wave pair brings the step's operands (gi x 4 and the dropout factor) memory ->
// registers (eight sets, requested up to 10 steps ahead) -> LDS ring `s_in` (2 steps ahead), in the window where it would wait
// at the barrier.  Every wave's loop is straight-line code with unconditional loads / stores.
// Without dropout the host passes drop = y (readable, that size), use = 0 and y2 = y; the factor is then SELECTED to 1: `drop`
// is read AHEAD of the walk, i.e. memory this kernel has not written yet, and 0 * NaN is NaN.  `y`, `drop` and `y2` may therefore
// name the same memory and carry no __restrict__.
template <int HH>
__global__ __launch_bounds__(NT) void k_lstm_seq_fwd(const float* __restrict__ gi, const float* __restrict__ w_hh,
                                                      const float* __restrict__ b_hh, int T, float* y,
                                                      float* __restrict__ saved, const float* drop, float use, float* y2) {
  constexpr int G4 = 4 * HH;             // rows of W_hh; part[ks][gate*HH + unit]
  // the 8 waves split the mat-vec KS ways along k and RS ways along the rows: HH = 128: 4 x 2 (phase 2, which carries the
  // serial chain, reads 16 partial sums per unit instead of 32); HH = 64: 8 x 1.  Four rows per lane either way.
  constexpr int KS = HH == 128 ? 4 : 8, RS = KC / KS;
  constexpr int RPL = G4 / (64 * RS);    // rows of W_hh per lane (4)
  constexpr int CPW = HH / KS;           // columns of W_hh per wave (32 / 8)
  static_assert(RPL == 4 && RPL * 64 * RS == G4 && CPW % 4 == 0, "split");
  __shared__ __attribute__((aligned(16))) float hbuf[2][HH];
  __shared__ __attribute__((aligned(16))) float part[KS * G4];
  __shared__ float s_in[4][5][HH];       // ring of 4 steps: gi_i, gi_f, gi_g, gi_o, dropout factor — written by the loader lanes
  CLAIM_SIMD_REGISTERS();
  const int b = blockIdx.x >> 1, d = blockIdx.x & 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kc = wv % KS;                                        // this WAVE's k chunk: its h values are wave-uniform
  const int row0 = (wv / KS) * (G4 / RS) + lane;                 // ... and its block of rows
  const float* W = w_hh + static_cast<size_t>(d) * G4 * HH;
  // lane -> the RPL rows {row0 + 64 i} of W_hh (row = gate*HH + unit), columns [CPW kc, CPW kc + CPW)
  f32x2 w[RPL][CPW / 2];
#pragma unroll
  for (int i = 0; i < RPL; ++i) {
    const float4* src = reinterpret_cast<const float4*>(W + static_cast<size_t>(row0 + 64 * i) * HH + CPW * kc);
#pragma unroll
    for (int v = 0; v < CPW / 4; ++v) {
      const float4 t4 = src[v];
      w[i][2 * v] = f32x2{t4.x, t4.y};
      w[i][2 * v + 1] = f32x2{t4.z, t4.w};
    }
  }
  if (tid < HH) { hbuf[0][tid] = 0.f; hbuf[1][tid] = 0.f; }
  // (the one __syncthreads before the time loop sits in each role's branch, behind the loader lanes' first LDS writes)

  auto phase1 = [&](int cur) {
    const float4* hp = reinterpret_cast<const float4*>(&hbuf[cur][CPW * kc]);     // same address in every lane: LDS broadcast
    f32x2 a[RPL];
#pragma unroll
    for (int i = 0; i < RPL; ++i) a[i] = f32x2{0.f, 0.f};
#pragma unroll
    for (int v = 0; v < CPW / 4; ++v) {
      const float4 t4 = hp[v];
      const f32x2 lo = {t4.x, t4.y}, hi = {t4.z, t4.w};
#pragma unroll
      for (int i = 0; i < RPL; ++i) {
        a[i] = __builtin_elementwise_fma(w[i][2 * v], lo, a[i]);
        a[i] = __builtin_elementwise_fma(w[i][2 * v + 1], hi, a[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < RPL; ++i) part[kc * G4 + row0 + 64 * i] = a[i].x + a[i].y;     // consecutive lanes, consecutive words
  };

  // ---- roles (gru.hip): unit lanes tid < HH; loader lanes tid 128 .. 128 + HH (waves 2, 3: SIMDs that idle during phase 2)
  const bool loader = tid >= 128 && tid < 128 + HH;
  const int hu = tid - 128;
  const size_t rowg = static_cast<size_t>(2) * G4;
  auto load_in = [&](int s_, float (&g)[5]) {
    const int sc = s_ < T ? s_ : T - 1;              // past the end: the last step again (a valid address, never used)
    const int t_ = d ? T - 1 - sc : sc;
    const float* p = gi + (static_cast<size_t>(b) * T + t_) * rowg + static_cast<size_t>(d) * G4 + hu;
    g[0] = p[0];
    g[1] = p[HH];
    g[2] = p[2 * HH];
    g[3] = p[3 * HH];
    g[4] = drop[(static_cast<size_t>(b) * T + t_) * 2 * HH + d * HH + hu];        // raw: arithmetic on a loaded value waits until put_in
  };
  auto put_in = [&](int s_, const float (&g)[5]) {
    float* q = &s_in[s_ & 3][0][hu];
    q[0] = g[0];
    q[HH] = g[1];
    q[2 * HH] = g[2];
    q[3 * HH] = g[3];
    q[4 * HH] = use != 0.f ? g[4] : 1.f;             // a SELECT: the stand-in's contents (NaN, Inf) never reach a result
  };
  // window s = while the unit lanes run phase 2 of step s
  if (loader) {
    float g0[5], g1[5], g2[5], g3[5], g4[5], g5[5], g6[5], g7[5];
    load_in(0, g0);
    load_in(1, g1);
    put_in(0, g0);
    put_in(1, g1);
    load_in(2, g2); load_in(3, g3); load_in(4, g4); load_in(5, g5); load_in(6, g6); load_in(7, g7);
    load_in(8, g0); load_in(9, g1);
    __syncthreads();
    int s = 0;
#define LSTM_FWD_WINDOW(I, G) phase1((I) & 1); lds_barrier(); put_in(s + 2 + (I), G); load_in(s + 10 + (I), G); lds_barrier();
    for (; s + 8 <= T; s += 8) {
      LSTM_FWD_WINDOW(0, g2) LSTM_FWD_WINDOW(1, g3) LSTM_FWD_WINDOW(2, g4) LSTM_FWD_WINDOW(3, g5)
      LSTM_FWD_WINDOW(4, g6) LSTM_FWD_WINDOW(5, g7) LSTM_FWD_WINDOW(6, g0) LSTM_FWD_WINDOW(7, g1)
    }
#undef LSTM_FWD_WINDOW
#define LSTM_FWD_LAST(I, G) if (s + (I) < T) { phase1((I) & 1); lds_barrier(); put_in(s + 2 + (I), G); lds_barrier(); }
    LSTM_FWD_LAST(0, g2) LSTM_FWD_LAST(1, g3) LSTM_FWD_LAST(2, g4) LSTM_FWD_LAST(3, g5) LSTM_FWD_LAST(4, g6) LSTM_FWD_LAST(5, g7) LSTM_FWD_LAST(6, g0)
#undef LSTM_FWD_LAST
    return;
  }
  if (tid >= HH) {                       // the other waves: mat-vec only
    __syncthreads();
    int s = 0;
    for (; s + 2 <= T; s += 2) {
      phase1(0); lds_barrier(); lds_barrier();
      phase1(1); lds_barrier(); lds_barrier();
    }
    if (s < T) { phase1(0); lds_barrier(); lds_barrier(); }
    return;
  }

  // waves 0, 1: lane = hidden unit
  const int u = tid;
  const float* bh = b_hh + d * G4 + u;
  const float bh0 = bh[0], bh1 = bh[HH], bh2 = bh[2 * HH], bh3 = bh[3 * HH];
  float c = 0.f;
  // running output pointers: time step 0 of this direction, then one row forward (reverse direction: backward) per step
  const int64_t t0 = d ? T - 1 : 0;
  const int64_t y_step = (d ? -1 : 1) * static_cast<int64_t>(2 * HH), sv_step = (d ? -1 : 1) * static_cast<int64_t>(2 * 5 * HH);
  float* y_p = y + (static_cast<size_t>(b) * T + t0) * 2 * HH + d * HH + u;
  float* y2_p = y2 + (static_cast<size_t>(b) * T + t0) * 2 * HH + d * HH + u;
  float* sv_p = saved + ((static_cast<size_t>(b) * T + t0) * 2 + d) * 5 * HH + u;
  auto gate_sum = [&](int gate, float bias) {       // fixed-shape tree (same order every run: bitwise reproducible)
    float p[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) p[k] = part[k * G4 + gate * HH + u];
    if (KS == 4) return ((p[0] + p[1]) + (p[2] + p[3])) + bias;
    return (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4 % KS] + p[5 % KS]) + (p[6 % KS] + p[7 % KS]))) + bias;
  };
  auto phase2 = [&](int cur, int slot) {         // cur = s & 1, slot = s & 3: constants in the unrolled loop below
    const float s0 = gate_sum(0, bh0), s1 = gate_sum(1, bh1), s2 = gate_sum(2, bh2), s3 = gate_sum(3, bh3);
    const float* in = &s_in[slot][0][u];
    const float gi0 = in[0], gi1 = in[HH], gi2 = in[2 * HH], gi3 = in[3 * HH], fac = in[4 * HH];
    const float ii = sigmoidf_(gi0 + s0);
    const float ff = sigmoidf_(gi1 + s1);
    const float gg = tanhf_(gi2 + s2);
    const float oo = sigmoidf_(gi3 + s3);
    c = ff * c + ii * gg;
    const float hnew = oo * tanhf_(c);
    hbuf[cur ^ 1][u] = hnew;
    // the unit lanes issue no load at all, so their stores are never waited for
    y_p[0] = hnew;
    y2_p[0] = hnew * fac;
    sv_p[0] = ii;
    sv_p[HH] = ff;
    sv_p[2 * HH] = gg;
    sv_p[3 * HH] = oo;
    sv_p[4 * HH] = c;
    y_p += y_step;
    y2_p += y_step;
    sv_p += sv_step;
  };
  __syncthreads();
  int s = 0;
  for (; s + 4 <= T; s += 4) {
    phase1(0); lds_barrier(); phase2(0, 0); lds_barrier();
    phase1(1); lds_barrier(); phase2(1, 1); lds_barrier();
    phase1(0); lds_barrier(); phase2(0, 2); lds_barrier();
    phase1(1); lds_barrier(); phase2(1, 3); lds_barrier();
  }
  if (s < T)     { phase1(0); lds_barrier(); phase2(0, 0); lds_barrier(); }
  if (s + 1 < T) { phase1(1); lds_barrier(); phase2(1, 1); lds_barrier(); }
  if (s + 2 < T) { phase1(0); lds_barrier(); phase2(0, 2); lds_barrier(); }
}

// dy [B, T, 2*HH]; saved (and y, for hp_out only) from the forward; output dg [B, T, 2, 4*HH]: the gradient of the four
// pre-activations, which is the gradient w.r.t. gi AND w.r.t. W_hh h + b_hh.
// ---- two-phase backward (gru.hip's split) ------------------------------------------------------------------------------
//   phase A (waves 0 and 1, one lane per hidden unit): dh = dy * factor + the 8 partial sums of W_hh^T dg left by phase B of
//            the previous step (fixed order); dc = dc_{t+1} f_{t+1} (a register of this lane) + dh o (1 - tanh^2 c_t); the four
//            gate gradients to LDS;
//   phase B (all 8 waves; wave = 4*HH / 8 rows of W_hh, lane = two hidden units): the wave's dg values from LDS (one address
//            for all lanes), packed FMAs, two partial sums to LDS.
// Helper lanes as in k_gru_bwd: a LOADER pair (operands memory -> registers -> ring `s_in`) and a
// STORER pair (gate gradients `s_out` -> memory one step later, and — with HP — the shifted copy of y that is `hp_out`).  The
// loader also computes tanh(c_t) — off the serial chain — and selects c_{t-1} = 0 at the chain's first step.  It holds SETS
// register sets of 7 loaded values beside its weight registers; see the constant below.
template <int HH, bool HP>
__global__ __launch_bounds__(NT) void k_lstm_seq_bwd(const float* __restrict__ dy, const float* __restrict__ y,
                                                      const float* __restrict__ saved, const float* __restrict__ w_hh, int T,
                                                      float* __restrict__ dg_out, const float* __restrict__ drop, float use,
                                                      float* __restrict__ hp_out) {
  constexpr int G4 = 4 * HH;
  // register sets of the loader.  HH = 128: eight sets beside the 128 weight registers spilled 208 bytes per lane to scratch;
  // four fit.  A request then leads its use by 6 steps (~3.6 us) instead of 10.  HH = 64 (64 weight registers): eight.
  constexpr int SETS = HH == 128 ? 4 : 8;
  static_assert(SETS % 2 == 0 && SETS >= 4, "the step parity (k & 1) and the 2-step lead of the ring assume it");
  __shared__ __attribute__((aligned(16))) float s_out[2][G4];         // per step parity: d i_pre | d f_pre | d g_pre | d o_pre
  __shared__ __attribute__((aligned(16))) float cpart[KC * HH];
  __shared__ float s_in[4][7][HH];                                     // ring of 4 steps: dy * factor, i, f, g, o, tanh c_t, c_{t-1}
  CLAIM_SIMD_REGISTERS();
  const int b = blockIdx.x >> 1, d = blockIdx.x & 1;
  const int tid = threadIdx.x;
  const int kc = __builtin_amdgcn_readfirstlane(tid >> 6);       // this WAVE's chunk of rows j of W_hh: dg[j] is wave-uniform
  const int u_raw = 2 * (tid & 63);                              // lane -> hidden units u0, u0 + 1
  const bool u_on = u_raw < HH;                                  // HH = 64: lanes 32..63 carry no units (they repeat a pair, store nothing)
  const int u0 = u_on ? u_raw : HH - 2;
  const float* W = w_hh + static_cast<size_t>(d) * G4 * HH;
  constexpr int JC = G4 / KC;       // 64 / 32 rows of W per wave
  f32x2 wa[JC / 2], wb[JC / 2];     // unit u0 / u0+1: (W[j][u], W[j+1][u]) pairs over the chunk's rows
#pragma unroll
  for (int j = 0; j < JC; j += 2) {
    const float2 v0 = *reinterpret_cast<const float2*>(W + static_cast<size_t>(JC * kc + j) * HH + u0);
    const float2 v1 = *reinterpret_cast<const float2*>(W + static_cast<size_t>(JC * kc + j + 1) * HH + u0);
    wa[j / 2] = f32x2{v0.x, v1.x};
    wb[j / 2] = f32x2{v0.y, v1.y};
  }
  for (int i = tid; i < KC * HH; i += NT) cpart[i] = 0.f;
  // The storer's window 0 has no finished step to store and stores step 0's slot as it stands (overwritten by the same lanes one
  // window later).  Skipping that store would put a branch around memory operations into every pass of the storer's loop (the
  // compiler then waits for all its outstanding loads and stores at the join); zeros in the slot cost one LDS write per launch.
  for (int i = tid; i < G4; i += NT) s_out[0][i] = 0.f;

  auto phaseB = [&](int cur) {
    f32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
    const float4* gp = reinterpret_cast<const float4*>(&s_out[cur][JC * kc]);
#pragma unroll
    for (int v = 0; v < JC / 4; ++v) {
      // HH = 128: the chunk's 64 dg values in two batches of 32 — hoisted above the FMAs all at once they took 64 registers
      // beside the 128 of the weights, and the loader lanes' register sets went to scratch
      if (JC == 64 && v == JC / 8) __builtin_amdgcn_sched_barrier(0);
      const float4 t4 = gp[v];
      const f32x2 lo = {t4.x, t4.y}, hi = {t4.z, t4.w};
      a0 = __builtin_elementwise_fma(wa[2 * v], lo, a0);
      a1 = __builtin_elementwise_fma(wb[2 * v], lo, a1);
      a0 = __builtin_elementwise_fma(wa[2 * v + 1], hi, a0);
      a1 = __builtin_elementwise_fma(wb[2 * v + 1], hi, a1);
    }
    if (u_on) *reinterpret_cast<float2*>(&cpart[kc * HH + u0]) = make_float2(a0.x + a0.y, a1.x + a1.y);
  };

  const bool loader = tid >= 128 && tid < 128 + HH;         // waves 2, 3: operands in
  const bool storer = tid >= 384 && tid < 384 + HH;         // waves 6, 7: gate gradients (and h_{t-1}) out
  const int hu = tid - (loader ? 128 : 384);
  struct StepIn { float dyv, dr, i, f, g, o, c; };      // raw loaded values: arithmetic on them waits until put_in
  auto load_in = [&](int s_, StepIn& o) {
    const int sc = s_ < T ? s_ : T - 1;          // past the end: the last step again (a valid address, never used)
    const int t_ = d ? sc : T - 1 - sc;          // reverse of the forward walk
    const size_t bt_ = static_cast<size_t>(b) * T + t_;
    o.dyv = dy[bt_ * 2 * HH + d * HH + hu];
    o.dr = drop[bt_ * 2 * HH + d * HH + hu];
    const float* sv = saved + (bt_ * 2 + d) * 5 * HH + hu;
    o.i = sv[0];
    o.f = sv[HH];
    o.g = sv[2 * HH];
    o.o = sv[3 * HH];
    o.c = sv[4 * HH];
  };
  // `nx` is the set of walk step s_ + 1, i.e. of the time step before this one in the forward walk: its c is this step's
  // c_{t-1} (no load of its own)
  auto put_in = [&](int s_, const StepIn& o, const StepIn& nx) {
    float* q = &s_in[s_ & 3][0][hu];
    q[0] = o.dyv * (use != 0.f ? o.dr : 1.f);    // dy is d(y * drop); a select: the stand-in operand is not a factor
    q[HH] = o.i;
    q[2 * HH] = o.f;
    q[3 * HH] = o.g;
    q[4 * HH] = o.o;
    q[5 * HH] = tanhf_(o.c);                     // the forward's function of the forward's c_t
    q[6 * HH] = s_ + 1 < T ? nx.c : 0.f;         // the chain's first step: c_{t-1} = 0
  };
  auto store_out = [&](int s_) {
    const int t = d ? s_ : T - 1 - s_;
    const float* o = &s_out[s_ & 1][hu];
    float* go = dg_out + ((static_cast<size_t>(b) * T + t) * 2 + d) * G4 + hu;
    const float v0 = o[0], v1 = o[HH], v2 = o[2 * HH], v3 = o[3 * HH];
    go[0] = v0;
    go[HH] = v1;
    go[2 * HH] = v2;
    go[3 * HH] = v3;
  };
  // hp_out: h_{t-1} of walk step s_ is y at walk step s_ + 1 — a shifted copy of y that the chain does not wait for.  The storer
  // lanes make it (the loader's registers are full at HH = 128): requested 4 windows ahead, stored unconditionally.
  auto load_hp = [&](int s_, float& v) {         // y of walk step s_ (clamped)
    const int sc = s_ < T ? s_ : T - 1;
    const int t_ = d ? sc : T - 1 - sc;
    v = y[(static_cast<size_t>(b) * T + t_) * 2 * HH + d * HH + hu];
  };
  auto store_hp = [&](int s_, float v) {         // s_ < T
    const int t_ = d ? s_ : T - 1 - s_;
    hp_out[((static_cast<size_t>(b) * T + t_) * 2 + d) * HH + hu] = s_ + 1 < T ? v : 0.f;
  };

  // window s = while the unit lanes run phase A of step s
  if (loader) {                          // step s' lives in register set s' % SETS: requested SETS + 2 steps ahead, to LDS 2 steps ahead
    StepIn in[SETS];                     // (every index below is a constant after unrolling: registers, not memory)
#pragma unroll
    for (int k = 0; k < SETS; ++k) load_in(k, in[k]);
    put_in(0, in[0], in[1]);
    put_in(1, in[1], in[2]);
    load_in(SETS, in[0]);
    load_in(SETS + 1, in[1]);
    __syncthreads();
    int s = 0;
    for (; s + SETS <= T; s += SETS) {
#pragma unroll
      for (int k = 0; k < SETS; ++k) {
        put_in(s + 2 + k, in[(2 + k) % SETS], in[(3 + k) % SETS]);
        load_in(s + 2 + k + SETS, in[(2 + k) % SETS]);
        lds_barrier(); phaseB(k & 1); lds_barrier();
      }
    }
#pragma unroll
    for (int k = 0; k < SETS - 1; ++k)
      if (s + k < T) { put_in(s + 2 + k, in[(2 + k) % SETS], in[(3 + k) % SETS]); lds_barrier(); phaseB(k & 1); lds_barrier(); }
    return;
  }
  if (storer) {                          // step s - 1's gradients leave while the unit lanes run phase A of step s
    float hv[4];                         // y of walk steps s + 1 .. s + 4 (hp_out only)
    if (HP) {
#pragma unroll
      for (int k = 0; k < 4; ++k) load_hp(1 + k, hv[k]);
    }
    __syncthreads();
    int s = 0;
    for (; s + 4 <= T; s += 4) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        store_out(s + k > 0 ? s + k - 1 : 0);    // (window 0: step 0's slot, zeros or what phase A has written of it so far; window 1 stores it again)
        if (HP) { store_hp(s + k, hv[k]); load_hp(s + k + 5, hv[k]); }
        lds_barrier(); phaseB(k & 1); lds_barrier();
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (s + k < T) {
        store_out(s + k > 0 ? s + k - 1 : 0);
        if (HP) store_hp(s + k, hv[k]);
        lds_barrier(); phaseB(k & 1); lds_barrier();
      }
    store_out(T - 1);
    return;
  }
  if (tid >= HH) {                       // the other waves: mat-vec only
    __syncthreads();
    int s = 0;
    for (; s + 2 <= T; s += 2) {
      lds_barrier(); phaseB(0); lds_barrier();
      lds_barrier(); phaseB(1); lds_barrier();
    }
    if (s < T) { lds_barrier(); phaseB(0); lds_barrier(); }
    return;
  }

  const int u = tid;
  float dcf = 0.f;                               // dc_{t+1} * f_{t+1}: what the next step of the forward walk hands back to c_t
  auto phaseA = [&](int cur, int slot) {         // cur = s & 1, slot = s & 3: constants in the unrolled loop below
    float cp[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) cp[k] = cpart[k * HH + u];
    const float* in = &s_in[slot][0][u];
    const float dyv = in[0], ii = in[HH], ff = in[2 * HH], gg = in[3 * HH], oo = in[4 * HH], tc = in[5 * HH], cprev = in[6 * HH];
    const float carry = ((cp[0] + cp[1]) + (cp[2] + cp[3])) + ((cp[4] + cp[5]) + (cp[6] + cp[7]));   // fixed-shape tree
    const float dh = dyv + carry;
    const float dc = dcf + dh * oo * (1.f - tc * tc);
    dcf = dc * ff;
    float* o = &s_out[cur][u];
    o[0] = dc * gg * ii * (1.f - ii);
    o[HH] = dc * cprev * ff * (1.f - ff);
    o[2 * HH] = dc * ii * (1.f - gg * gg);
    o[3 * HH] = dh * tc * oo * (1.f - oo);
  };
  __syncthreads();
  int s = 0;
  for (; s + 4 <= T; s += 4) {
    phaseA(0, 0); lds_barrier(); phaseB(0); lds_barrier();
    phaseA(1, 1); lds_barrier(); phaseB(1); lds_barrier();
    phaseA(0, 2); lds_barrier(); phaseB(0); lds_barrier();
    phaseA(1, 3); lds_barrier(); phaseB(1); lds_barrier();
  }
  if (s < T)     { phaseA(0, 0); lds_barrier(); phaseB(0); lds_barrier(); }
  if (s + 1 < T) { phaseA(1, 1); lds_barrier(); phaseB(1); lds_barrier(); }
  if (s + 2 < T) { phaseA(0, 2); lds_barrier(); phaseB(0); lds_barrier(); }
}

template <int HH>
void launch_fwd(const float* gi, const float* w_hh, const float* b_hh, int64_t B, int T, float* y, float* saved, const float* drop,
                float* y_drop, hipStream_t st) {
  hipLaunchKernelGGL(k_lstm_seq_fwd<HH>, dim3(static_cast<unsigned>(B * 2)), dim3(NT), 0, st, gi, w_hh, b_hh, T, y, saved,
                     drop ? drop : y, drop ? 1.f : 0.f, y_drop ? y_drop : y);
}

template <int HH>
void launch_bwd(const float* dy, const float* y, const float* saved, const float* w_hh, int64_t B, int T, float* dg, const float* drop,
                float* hprev, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(B * 2)), block(NT);
  const float* dr = drop ? drop : dy;            // stand-in: readable, that size; selected away in the kernel.  Both are only
                                                 // read, so two __restrict__ names for the same memory promise nothing false
  const float use = drop ? 1.f : 0.f;
  if (hprev) hipLaunchKernelGGL((k_lstm_seq_bwd<HH, true>), grid, block, 0, st, dy, y, saved, w_hh, T, dg, dr, use, hprev);
  else hipLaunchKernelGGL((k_lstm_seq_bwd<HH, false>), grid, block, 0, st, dy, y, saved, w_hh, T, dg, dr, use, hprev);
}

}  // namespace

extern "C" int agnn_lstm_seq_fwd_f32(const float* gi, const float* w_hh, const float* b_hh, int64_t B, int64_t T, int32_t hidden,
                                     float* y, float* saved, const float* drop_scale, float* y_drop, agnn_stream_t stream_) {
  using namespace agnn;
  if (hidden != 128 && hidden != 64) return fail(AGNN_EINVAL, "lstm_seq_fwd: hidden=%d unsupported (this build: 64, 128)", hidden);
  if (B <= 0 || T <= 0 || B * 2 >= (int64_t{1} << 31) || T >= (int64_t{1} << 31))
    return fail(AGNN_EINVAL, "lstm_seq_fwd: bad B=%lld T=%lld", (long long)B, (long long)T);
  if (!gi || !w_hh || !b_hh || !y || !saved) return fail(AGNN_EINVAL, "lstm_seq_fwd: null argument");
  if (!aligned16(gi) || !aligned16(w_hh) || !aligned16(y) || !aligned16(saved)) return fail(AGNN_EALIGN, "lstm_seq_fwd: pointers must be 16-byte aligned");
  if ((drop_scale == nullptr) != (y_drop == nullptr)) return fail(AGNN_EINVAL, "lstm_seq_fwd: drop_scale and y_drop go together");
  const hipStream_t st = static_cast<hipStream_t>(stream_);
  if (hidden == 128) launch_fwd<128>(gi, w_hh, b_hh, B, static_cast<int>(T), y, saved, drop_scale, y_drop, st);
  else launch_fwd<64>(gi, w_hh, b_hh, B, static_cast<int>(T), y, saved, drop_scale, y_drop, st);
  return check_launch("lstm_seq_fwd");
}

extern "C" int agnn_lstm_seq_bwd_f32(const float* dy, const float* y, const float* saved, const float* w_hh, int64_t B, int64_t T,
                                     int32_t hidden, float* dg, const float* drop_scale, float* hprev, agnn_stream_t stream_) {
  using namespace agnn;
  if (hidden != 128 && hidden != 64) return fail(AGNN_EINVAL, "lstm_seq_bwd: hidden=%d unsupported (this build: 64, 128)", hidden);
  if (B <= 0 || T <= 0 || B * 2 >= (int64_t{1} << 31) || T >= (int64_t{1} << 31))
    return fail(AGNN_EINVAL, "lstm_seq_bwd: bad B=%lld T=%lld", (long long)B, (long long)T);
  if (!dy || !saved || !w_hh || !dg) return fail(AGNN_EINVAL, "lstm_seq_bwd: null argument");
  if (hprev && !y) return fail(AGNN_EINVAL, "lstm_seq_bwd: hprev needs y (the forward's output)");
  if (!aligned16(dy) || !aligned16(y) || !aligned16(saved) || !aligned16(w_hh) || !aligned16(dg) || !aligned16(hprev))
    return fail(AGNN_EALIGN, "lstm_seq_bwd: pointers must be 16-byte aligned");
  const hipStream_t st = static_cast<hipStream_t>(stream_);
  if (hidden == 128) launch_bwd<128>(dy, y, saved, w_hh, B, static_cast<int>(T), dg, drop_scale, hprev, st);
  else launch_bwd<64>(dy, y, saved, w_hh, B, static_cast<int>(T), dg, drop_scale, hprev, st);
  return check_launch("lstm_seq_bwd");
}
