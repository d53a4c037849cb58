// Note descriptors: the note array -> x_note, the voice (25 columns) and cadence (25 + 31 columns) feature sets of the reference
// (descriptors/utils/note_features.py:176-226, descriptors/utils/cadence_features.py:6-119, an O(N^2) Python loop).
//
// The notes of a score arrive in (onset, pitch) order, so a note's onset run and its look-back windows are contiguous ranges that
// binary searches inside the score's own slice find, and everything the reference derives from the chord is a function of one small
// record per onset run, kept in the slot of the run's first note:
//   mask  12 bits, the pitch classes of the chord (bit 12: some note sounds through the onset)
//   lo/hi the chord's lowest / highest pitch;  cnt  its number of notes
// int_vec[k - 1] = popcount(mask & rot12(mask, k)) (halved for k = 6), the `rec` tests compare mask >> ctz(mask), prev4 / prev8 are
// two more 12-bit masks, and the previous onset of the note's voice is a 12-bit mask plus a 25-bit mask of pitch differences.
//   k_nf_init     score_start is checked (one block); per-score voice extremes reset; the segments of the sort
//   k_nf_prep     per note: score, faults, the searchable onset, its pitch-class bit, the sort key (its voice); group slots reset
//   radix sort    (library, stable, segmented by score) order by voice: every voice's notes, in onset order, side by side
//   k_nf_scatter  per note: its run [lb, ub); integer atomics put it into its own run's record and into the record of every later
//                 run it sounds through (as many steps as it has `during` edges); its position in the voice order
//   k_nf_rows     per note: the windows (as far back as 8 beats reach), the voice's previous / next onset (its own run and one run
//                 back / forth in the voice list), the 54 bits and 2 floats of the row; the block then writes its rows with 16-byte
//                 stores where x allows them
// The voice set needs k_nf_init and k_nf_rows only.  Integer atomics only (or / min / max / add): the result has one value
// whatever the order.  A faulty note (agnn.h) has pcbit = 0: it enters no record, no window and no voice list.
#include <hipcub/hipcub.hpp>

#include "agnn_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxNotes = (int64_t{1} << 29) - 1;
constexpr int kVoiceBits = 15;
constexpr uint32_t kFaultyKey = 1u << kVoiceBits;      // the faulty notes: one list behind every voice of their score
constexpr uint32_t kDuringBit = 1u << 12;
constexpr int32_t kNoPitch = 1 << 20;

struct NoteIn {
  const int64_t *onset, *dur, *pitch, *voice, *ts, *downbeat;
  const float *onset_beat, *dur_beat;
  const uint8_t* is_onset;
  const int32_t* start;
  int32_t N, S;
};

struct Work {
  int32_t* tile_bad;      // [1]
  int32_t *vmin, *vmax;   // [S] the score's lowest / highest voice: the reference's bass / high voice
  int32_t* seg;           // [S + 1] score_start, or zeros (empty segments) when it does not tile
  int32_t* score_of;      // [N]
  int64_t* on_s;          // [N] the onset the searches see: a note below its predecessor takes the predecessor's ...
  float* ob_s;            // [N] ... and its onset_beat
  uint32_t* pcbit;        // [N] 1 << (pitch % 12), 0 for a faulty note
  uint32_t *keys_in, *keys_out;
  int32_t *vals_in, *vals_out;
  int32_t *pos, *lb;      // [N] position in the voice order; first note of the onset run
  uint32_t* gmask;        // [N] the records, indexed by the run's first note
  int32_t *glo, *ghi, *gcnt;
};

template <typename T>
__device__ __forceinline__ int32_t lower_bound(const T* __restrict__ a, int32_t lo, int32_t hi, T x) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
template <typename T>
__device__ __forceinline__ int32_t upper_bound(const T* __restrict__ a, int32_t lo, int32_t hi, T x) {
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
__device__ __forceinline__ uint32_t rot12(uint32_t m, int k) {          // bit b -> bit (b + k) % 12, 0 <= k < 12
  return ((m << k) | (m >> (12 - k))) & 0xFFFu;
}
__device__ __forceinline__ int mod12(int v) {                            // the sign of the divisor, as numpy's %
  const int r = v % 12;
  return r < 0 ? r + 12 : r;
}
__device__ __forceinline__ int64_t end_of(int64_t on, int64_t du) {      // on + du, saturated
  int64_t e;
  if (__builtin_add_overflow(on, du, &e)) e = du > 0 ? INT64_MAX : INT64_MIN;
  return e;
}

__global__ __launch_bounds__(kThreads) void k_nf_init(const int32_t* __restrict__ start, int32_t S, int32_t N, int32_t* __restrict__ tile_bad,
                                                      int32_t* __restrict__ vmin, int32_t* __restrict__ vmax, int32_t* __restrict__ seg,
                                                      int32_t* __restrict__ faults) {
  int fail = 0;
  for (int32_t s = threadIdx.x; s < S; s += blockDim.x) {
    const int32_t a = start[s], b = start[s + 1];
    fail |= (a < 0 || b < a || b > N || (s == 0 && a != 0) || (s == S - 1 && b != N)) ? 1 : 0;
    if (vmin) {
      vmin[s] = INT32_MAX;
      vmax[s] = -1;
    }
  }
  fail = __syncthreads_or(fail);
  if (seg)
    for (int32_t s = threadIdx.x; s <= S; s += blockDim.x) seg[s] = fail ? 0 : start[s];
  if (threadIdx.x == 0) {
    tile_bad[0] = fail;
    if (fail) atomicAdd(faults + AGNN_NF_FAULT_SCORES, 1);
  }
}

// What both sets check per note, counted per kind.  Returns the note's score, or -1 for a faulty note; `below`: its onset is
// below its predecessor's.
__device__ __forceinline__ int32_t check_note(const NoteIn& A, int32_t i, int32_t* __restrict__ faults, bool& below) {
  const int32_t s = score_of_note(A.start, A.S, i);
  const int64_t p = A.pitch[i], ts = A.ts[i], on = A.onset[i];
  const bool bad_p = p < 0 || p >= 120, bad_ts = ts <= 0;
  bool bad_v = false, bad_o = false;
  if (A.voice) {
    const int64_t v = A.voice[i];
    bad_v = v < 0 || v >= (int64_t{1} << kVoiceBits);
  }
  if (i > A.start[s]) bad_o = A.onset[i - 1] > on;
  below = bad_o;
  if (bad_p) atomicAdd(faults + AGNN_NF_FAULT_PITCH, 1);
  if (bad_ts) atomicAdd(faults + AGNN_NF_FAULT_TS, 1);
  if (bad_v) atomicAdd(faults + AGNN_NF_FAULT_VOICE, 1);
  if (bad_o) atomicAdd(faults + AGNN_NF_FAULT_ORDER, 1);
  return (bad_p || bad_ts || bad_v || bad_o) ? -1 : s;
}

__global__ __launch_bounds__(kThreads) void k_nf_prep(NoteIn A, Work W, int32_t* __restrict__ faults) {
  const int32_t i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < A.N;
  const bool tiled = W.tile_bad[0] == 0;
  int32_t s = -1, ok_s = -1, voice = 0;
  if (live) {
    bool below = false;
    if (tiled) {
      s = score_of_note(A.start, A.S, i);
      ok_s = check_note(A, i, faults, below);
      if (ok_s >= 0) voice = static_cast<int32_t>(A.voice[i]);
    }
    W.score_of[i] = s;
    W.on_s[i] = A.onset[below ? i - 1 : i];
    W.ob_s[i] = A.onset_beat[below ? i - 1 : i];
    W.pcbit[i] = ok_s >= 0 ? 1u << static_cast<int>(A.pitch[i] % 12) : 0u;
    W.keys_in[i] = ok_s >= 0 ? static_cast<uint32_t>(voice) : kFaultyKey;
    W.vals_in[i] = i;
    W.gmask[i] = 0u;
    W.glo[i] = kNoPitch;
    W.ghi[i] = -1;
    W.gcnt[i] = 0;
  }
  // the score's voice extremes: one pair of atomics per wave where the wave lies inside one score
  int32_t lo = ok_s >= 0 ? voice : INT32_MAX, hi = ok_s >= 0 ? voice : -1;
  const int32_t s0 = __shfl(s, 0);
  if (__all(!live || s == s0)) {
    for (int m = 32; m > 0; m >>= 1) {
      lo = min(lo, __shfl_xor(lo, m));
      hi = max(hi, __shfl_xor(hi, m));
    }
    if ((threadIdx.x & 63) == 0 && s0 >= 0 && hi >= 0) {
      atomicMin(W.vmin + s0, lo);
      atomicMax(W.vmax + s0, hi);
    }
  } else if (ok_s >= 0) {
    atomicMin(W.vmin + ok_s, lo);
    atomicMax(W.vmax + ok_s, hi);
  }
}

__global__ __launch_bounds__(kThreads) void k_nf_scatter(NoteIn A, Work W) {
  const int32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= A.N || W.tile_bad[0] != 0) return;  // (the sort had empty segments: vals_out holds nothing)
  W.pos[W.vals_out[i]] = i;                    // vals_out permutes every score's slice
  const int32_t s = W.score_of[i];
  const uint32_t bit = W.pcbit[i];
  if (s < 0 || bit == 0u) {
    W.lb[i] = i;
    return;
  }
  const int32_t a = A.start[s], b = A.start[s + 1];
  const int64_t on = W.on_s[i];
  const int32_t lb = lower_bound(W.on_s, a, b, on);
  int32_t j = upper_bound(W.on_s, lb, b, on);
  W.lb[i] = lb;
  const int32_t p = static_cast<int32_t>(A.pitch[i]);
  atomicOr(W.gmask + lb, bit);
  atomicMin(W.glo + lb, p);
  atomicMax(W.ghi + lb, p);
  atomicAdd(W.gcnt + lb, 1);
  // the runs this note sounds through: onsets in (on, end), one step per run
  const int64_t end = end_of(on, A.dur[i]);
  const int32_t stop = end > on ? lower_bound(W.on_s, j, b, end) : j;
  while (j < stop) {
    atomicOr(W.gmask + j, bit | kDuringBit);
    atomicMin(W.glo + j, p);
    atomicMax(W.ghi + j, p);
    atomicAdd(W.gcnt + j, 1);
    j = upper_bound(W.on_s, j + 1, stop, W.on_s[j]);
  }
}

__device__ __forceinline__ uint32_t int_vec_code(uint32_t m) {          // int_vec as six 4-bit counts, class k in bits 4 (k - 1) ..
  uint32_t code = 0;
#pragma unroll
  for (int k = 1; k <= 6; ++k) {
    const uint32_t c = __popc(m & rot12(m, k)) >> (k == 6 ? 1 : 0);
    code |= c << (4 * (k - 1));
  }
  return code;
}
constexpr uint32_t iv(int a, int b, int c, int d, int e, int f) {
  return static_cast<uint32_t>(a | (b << 4) | (c << 8) | (d << 12) | (e << 16) | (f << 20));
}
constexpr uint32_t pcs(int a, int b = 0, int c = 0) { return (1u << a) | (1u << b) | (1u << c); }

// column c of the row is bit c of `bits`, columns 0 and 1 apart
template <bool CADENCE>
__global__ __launch_bounds__(kThreads) void k_nf_rows(NoteIn A, Work W, float* __restrict__ x, int64_t ld_x, int vec_ok,
                                                      int32_t* __restrict__ faults) {
  __shared__ float sh_f0[kThreads], sh_f1[kThreads];
  __shared__ uint64_t sh_bits[kThreads];
  const int32_t row0 = blockIdx.x * kThreads, i = row0 + threadIdx.x;
  float f0 = 0.f, f1 = 0.f;
  uint64_t bits = 0;
  if (i < A.N && W.tile_bad[0] == 0) {
    bool below;
    const int32_t s = CADENCE ? (W.pcbit[i] ? W.score_of[i] : -1) : check_note(A, i, faults, below);
    if (s >= 0) {
      const int32_t p = static_cast<int32_t>(A.pitch[i]);
      const int64_t ts = A.ts[i];
      const float ob = A.onset_beat[i];
      // the reference divides a float32 field by an int64 one: float64
      const double tsd = static_cast<double>(ts), obd = static_cast<double>(ob);
      f0 = static_cast<float>(1.0 - tanh(static_cast<double>(A.dur_beat[i]) / tsd));
      double r = fmod(obd, tsd);
      if (r < 0.0) r += tsd;
      if (r == 0.0) r = 0.0;                  // no negative zero
      f1 = static_cast<float>(r / tsd);
      if (fmodf(ob, 1.0f) == 0.0f) bits |= 1ull << 2;
      bits |= 1ull << (3 + p % 12);
      bits |= 1ull << (15 + p / 12);
      if (CADENCE) {
        const int32_t a = A.start[s], b = A.start[s + 1];
        const int32_t lb = W.lb[i];
        const uint32_t g = W.gmask[lb], mask = g & 0xFFFu;
        const int32_t lo = W.glo[lb], hi = W.ghi[lb], cnt = W.gcnt[lb];
        const uint32_t code = int_vec_code(mask), rec = mask >> __builtin_ctz(mask | 0x1000u);
        const bool triad = code == iv(0, 0, 1, 1, 1, 0) || code == iv(0, 0, 1, 0, 0, 0) || code == iv(0, 0, 0, 1, 0, 0) ||
                           code == iv(0, 0, 0, 0, 1, 0);
        const bool major = rec == pcs(0, 4, 7) || rec == pcs(0, 5, 9) || rec == pcs(0, 3, 8) || rec == pcs(0, 4) || rec == pcs(0, 8) ||
                           rec == pcs(0, 7) || rec == pcs(0, 5);
        const bool sus4 = code == iv(0, 1, 0, 0, 2, 0) || rec == pcs(0, 5);
        const bool v7 = code == iv(0, 1, 2, 1, 1, 1) || code == iv(0, 1, 0, 1, 0, 1) || code == iv(0, 1, 0, 0, 0, 0);
        const int span = mod12(hi - lo), own = mod12(p - lo);
        // the two windows, (ob - 8, ob) and (ob - 4, ob) on onset_beat, bounds in float32 as numpy computes them
        const float w4 = ob - 4.0f, w8 = ob - 8.0f;
        const int32_t w_end = lower_bound(W.ob_s, a, b, ob);
        uint32_t prev4 = 0, prev8 = 0;
        for (int32_t j = upper_bound(W.ob_s, a, w_end, w8); j < w_end; ++j) {
          const float oj = W.ob_s[j];
          const uint32_t bj = W.pcbit[j];
          if (oj < ob && oj > w8) prev8 |= bj;
          if (oj < ob && oj > w4) prev4 |= bj;
        }
        // the scale is the minor one only when the unreduced pitch + 3 is a pitch class of the chord
        const uint32_t scale = (p + 3 < 12 && ((mask >> (p + 3)) & 1u)) ? (pcs(2, 3, 5) | pcs(7, 8, 11)) : (pcs(2, 4, 5) | pcs(7, 9, 11));
        const int pc = p % 12;
        const bool compat = ((prev4 >> ((pc + 5) % 12)) & 1u) && ((prev4 >> ((pc + 11) % 12)) & 1u);
        const bool compat_scale = prev8 != 0u && (rot12(scale, pc) & ~prev8) == 0u;
        // the note's voice: its own onset run, then one run back (pv) and the first note further on (nv)
        const int32_t t = W.pos[i];
        const uint32_t key = W.keys_out[t];
        const int64_t on = A.onset[i];
        uint32_t pv12 = 0, pvd = 0;             // pv % 12 as a mask; pv - p + 12 as a mask, |pv - p| <= 12
        bool has_pv = false;
        int32_t u = t - 1;
        while (u >= a && W.keys_out[u] == key && A.onset[W.vals_out[u]] == on) --u;
        if (u >= a && W.keys_out[u] == key) {
          const int64_t P = A.onset[W.vals_out[u]];
          has_pv = P < on;
          while (has_pv && u >= a && W.keys_out[u] == key) {
            const int32_t q = W.vals_out[u];
            if (A.onset[q] != P) break;
            const int32_t d = static_cast<int32_t>(A.pitch[q]) - p;
            pv12 |= W.pcbit[q];
            if (d >= -12 && d <= 12) pvd |= 1u << (d + 12);
            --u;
          }
        }
        u = t + 1;
        while (u < b && W.keys_out[u] == key && A.onset[W.vals_out[u]] == on) ++u;
        const bool has_nv = u < b && W.keys_out[u] == key && A.onset[W.vals_out[u]] > on;
        const bool rest = has_nv && A.onset[W.vals_out[u]] > end_of(on, A.dur[i]);
        const uint32_t pvr = rot12(pv12, (12 - lo % 12) % 12);       // (pv - lo) % 12 as a mask
        const int32_t voice = static_cast<int32_t>(A.voice[i]);
        const bool is_bass = voice == W.vmin[s], is_high = voice == W.vmax[s];
        const bool from = has_pv && cnt > 1 && own == 0;
        const bool strong = (ts == 4 && fmodf(ob, 2.0f) == 0.0f) || fmod(obd, tsd) == 0.0;
        auto diff = [&](int d) { return ((pvd >> (d + 12)) & 1u) != 0u; };
        int c = 25;
        auto put = [&](bool v) { bits |= static_cast<uint64_t>(v ? 1 : 0) << c; ++c; };
        put(triad);
        put(triad && major);
        put(sus4);
        put(triad || sus4);
        put(span == 3 || span == 4);
        put(span == 0 && hi != lo);
        put(compat);
        put(compat_scale);
        put(from && ((pvr >> 11) & 1u));
        put(from && (pvr & 1u));
        put(from && ((pvr >> 2) & 1u));
        put(has_pv && ((pvr >> 5) & 1u) && (own == 3 || own == 4));
        put(has_pv && ((pvr >> 7) & 1u) && own == 7);
        put(strong);
        put((g & kDuringBit) != 0u);
        put(A.is_onset ? A.is_onset[i] != 0 : true);
        put(rest && is_high);
        put(rest && is_bass);
        put(rest && !is_high && !is_bass);
        put(!has_nv);
        put(A.downbeat[i] != 0);
        put(v7);
        put(v7 && ((rec >> 4) & 1u));
        put((rec >> 10) & 1u);
        put(((rec >> 1) & 1u) || ((rec >> 2) & 1u));
        put(is_bass);
        put(is_bass && (diff(1) || diff(-1)));
        put(is_bass && (diff(12) || diff(-12)));
        put(is_bass && (diff(7) || diff(-5)));
        put(is_bass && (diff(-7) || diff(5)));
        put(is_bass && (diff(2) || diff(-2)));
      }
    }
  }
  sh_f0[threadIdx.x] = f0;
  sh_f1[threadIdx.x] = f1;
  sh_bits[threadIdx.x] = bits;
  __syncthreads();
  // the block's rows, four columns per lane and step: consecutive lanes write consecutive 16-byte pieces of a row
  constexpr int kWidth = CADENCE ? AGNN_NF_CADENCE_WIDTH : AGNN_NF_VOICE_WIDTH, kPieces = (kWidth + 3) / 4;
  const int32_t rows = min(kThreads, A.N - row0);
  for (int item = threadIdx.x; item < rows * kPieces; item += kThreads) {
    const int r = item / kPieces, c0 = 4 * (item - r * kPieces);
    const uint64_t bt = sh_bits[r];
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = static_cast<float>((bt >> (c0 + k)) & 1ull);
    if (c0 == 0) {
      v[0] = sh_f0[r];
      v[1] = sh_f1[r];
    }
    float* dst = x + static_cast<int64_t>(row0 + r) * ld_x + c0;
    if (vec_ok && c0 + 4 <= kWidth) {
      agnn::st4(dst, agnn::f32x4{v[0], v[1], v[2], v[3]});
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < kWidth) dst[k] = v[k];
    }
  }
}

inline size_t align_up(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

constexpr int kKeyBits = kVoiceBits + 1;     // voices and kFaultyKey

struct Layout {
  size_t tile_bad, vmin, vmax, seg, score_of, on_s, ob_s, pcbit, keys_in, keys_out, vals_in, vals_out, pos, lb, gmask, glo, ghi, gcnt, temp,
      temp_bytes, total;
};

Layout make_layout(int64_t N, int32_t S, bool cadence) {
  Layout l{};
  const size_t n = static_cast<size_t>(N), s = static_cast<size_t>(S);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += align_up(bytes);
    return at;
  };
  l.tile_bad = take(sizeof(int32_t));
  if (cadence) {
    l.vmin = take(s * sizeof(int32_t));
    l.vmax = take(s * sizeof(int32_t));
    l.seg = take((s + 1) * sizeof(int32_t));
    l.score_of = take(n * sizeof(int32_t));
    l.on_s = take(n * sizeof(int64_t));
    l.ob_s = take(n * sizeof(float));
    l.pcbit = take(n * sizeof(uint32_t));
    l.keys_in = take(n * sizeof(uint32_t));
    l.keys_out = take(n * sizeof(uint32_t));
    l.vals_in = take(n * sizeof(int32_t));
    l.vals_out = take(n * sizeof(int32_t));
    l.pos = take(n * sizeof(int32_t));
    l.lb = take(n * sizeof(int32_t));
    l.gmask = take(n * sizeof(uint32_t));
    l.glo = take(n * sizeof(int32_t));
    l.ghi = take(n * sizeof(int32_t));
    l.gcnt = take(n * sizeof(int32_t));
    (void)hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, l.temp_bytes, static_cast<const uint32_t*>(nullptr),
                                                      static_cast<uint32_t*>(nullptr), static_cast<const int32_t*>(nullptr),
                                                      static_cast<int32_t*>(nullptr), static_cast<int>(N), static_cast<int>(S),
                                                      static_cast<const int32_t*>(nullptr), static_cast<const int32_t*>(nullptr), 0,
                                                      kKeyBits, nullptr);
    l.temp = take(l.temp_bytes);
  }
  l.total = off;
  return l;
}

inline bool known_set(int32_t set) { return set == AGNN_NF_VOICE || set == AGNN_NF_CADENCE; }

}  // namespace

extern "C" size_t agnn_note_features_workspace_bytes(int64_t n_notes, int32_t n_scores, int32_t feature_set) {
  if (n_notes < 1 || n_notes > kMaxNotes || n_scores < 1 || !known_set(feature_set)) return 0;
  return make_layout(n_notes, n_scores, feature_set == AGNN_NF_CADENCE).total + 256;
}

extern "C" int agnn_note_features_f32(const agnn_note_features_t* f, void* workspace, size_t workspace_bytes, agnn_stream_t stream_) {
  using namespace agnn;
  if (!f) return fail(AGNN_EINVAL, "note_features: f is null");
  if (!known_set(f->feature_set)) return fail(AGNN_EINVAL, "note_features: feature_set=%d is neither AGNN_NF_VOICE nor AGNN_NF_CADENCE", f->feature_set);
  const bool cadence = f->feature_set == AGNN_NF_CADENCE;
  const int width = cadence ? AGNN_NF_CADENCE_WIDTH : AGNN_NF_VOICE_WIDTH;
  if (f->n_scores < 1) return fail(AGNN_EINVAL, "note_features: n_scores=%d", f->n_scores);
  if (f->n_notes < 1 || f->n_notes > kMaxNotes) return fail(AGNN_EINVAL, "note_features: n_notes=%lld not in [1, %lld]", (long long)f->n_notes, (long long)kMaxNotes);
  if (!f->onset_div || !f->duration_div || !f->pitch || !f->ts_beats || !f->onset_beat || !f->duration_beat || !f->score_start)
    return fail(AGNN_EINVAL, "note_features: null input (onset_div, duration_div, pitch, ts_beats, onset_beat, duration_beat, score_start)");
  if (cadence && (!f->voice || !f->is_downbeat)) return fail(AGNN_EINVAL, "note_features: null input (the cadence set needs voice and is_downbeat)");
  if (!f->x || !f->faults) return fail(AGNN_EINVAL, "note_features: null x or faults");
  if (f->ld_x < width) return fail(AGNN_EINVAL, "note_features: ld_x=%lld below the %d columns of the set", (long long)f->ld_x, width);
  if (!workspace) return fail(AGNN_EINVAL, "note_features: workspace is null");
  const size_t need = agnn_note_features_workspace_bytes(f->n_notes, f->n_scores, f->feature_set);
  if (workspace_bytes < need) return fail(AGNN_ENOMEM, "note_features: workspace %zu bytes, %zu needed", workspace_bytes, need);

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int32_t N = static_cast<int32_t>(f->n_notes), S = f->n_scores;
  const Layout l = make_layout(N, S, cadence);
  char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~uintptr_t{255});
  auto at = [&](size_t off) { return cadence ? ws + off : nullptr; };
  Work W{};
  W.tile_bad = reinterpret_cast<int32_t*>(ws + l.tile_bad);
  W.vmin = reinterpret_cast<int32_t*>(at(l.vmin));
  W.vmax = reinterpret_cast<int32_t*>(at(l.vmax));
  W.seg = reinterpret_cast<int32_t*>(at(l.seg));
  W.score_of = reinterpret_cast<int32_t*>(at(l.score_of));
  W.on_s = reinterpret_cast<int64_t*>(at(l.on_s));
  W.ob_s = reinterpret_cast<float*>(at(l.ob_s));
  W.pcbit = reinterpret_cast<uint32_t*>(at(l.pcbit));
  W.keys_in = reinterpret_cast<uint32_t*>(at(l.keys_in));
  W.keys_out = reinterpret_cast<uint32_t*>(at(l.keys_out));
  W.vals_in = reinterpret_cast<int32_t*>(at(l.vals_in));
  W.vals_out = reinterpret_cast<int32_t*>(at(l.vals_out));
  W.pos = reinterpret_cast<int32_t*>(at(l.pos));
  W.lb = reinterpret_cast<int32_t*>(at(l.lb));
  W.gmask = reinterpret_cast<uint32_t*>(at(l.gmask));
  W.glo = reinterpret_cast<int32_t*>(at(l.glo));
  W.ghi = reinterpret_cast<int32_t*>(at(l.ghi));
  W.gcnt = reinterpret_cast<int32_t*>(at(l.gcnt));
  const NoteIn A{f->onset_div, f->duration_div, f->pitch, f->voice, f->ts_beats, f->is_downbeat, f->onset_beat, f->duration_beat,
                 f->is_note_onset, f->score_start, N, S};
  const int blocks = (N + kThreads - 1) / kThreads;
  const int vec_ok = (aligned16(f->x) && f->ld_x % 4 == 0) ? 1 : 0;

  hipLaunchKernelGGL(k_nf_init, dim3(1), dim3(kThreads), 0, stream, f->score_start, S, N, W.tile_bad, W.vmin, W.vmax, W.seg, f->faults);
  if (int rc = check_launch("note_features/init")) return rc;
  if (!cadence) {
    hipLaunchKernelGGL(k_nf_rows<false>, dim3(blocks), dim3(kThreads), 0, stream, A, W, f->x, f->ld_x, vec_ok, f->faults);
    return check_launch("note_features/rows");
  }
  hipLaunchKernelGGL(k_nf_prep, dim3(blocks), dim3(kThreads), 0, stream, A, W, f->faults);
  if (int rc = check_launch("note_features/prep")) return rc;
  size_t temp_bytes = l.temp_bytes;
  // one segment per score: the notes of a score stay in its slice, in stable order of voice
  hipError_t e = hipcub::DeviceSegmentedRadixSort::SortPairs(ws + l.temp, temp_bytes, W.keys_in, W.keys_out, W.vals_in, W.vals_out,
                                                             static_cast<int>(N), static_cast<int>(S), W.seg, W.seg + 1, 0, kKeyBits, stream);
  if (e != hipSuccess) return fail(AGNN_ERUNTIME, "note_features/sort: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_nf_scatter, dim3(blocks), dim3(kThreads), 0, stream, A, W);
  if (int rc = check_launch("note_features/scatter")) return rc;
  hipLaunchKernelGGL(k_nf_rows<true>, dim3(blocks), dim3(kThreads), 0, stream, A, W, f->x, f->ld_x, vec_ok, f->faults);
  return check_launch("note_features/rows");
}
