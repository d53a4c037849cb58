// Internal helpers shared by the kernel translation units (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "agnn.h"

namespace agnn {

char* last_error_buf();
constexpr int kErrBuf = 512;

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error_buf(), kErrBuf, fmt, ap);
  va_end(ap);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(AGNN_ERUNTIME, "%s: %s", what, hipGetErrorString(e));
  return AGNN_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

constexpr int kWave = 64;  // gfx950 wavefront

// Workgroups of a 256-thread, one-wave-per-row launch over n_rows rows, rounded up to whole rounds over the 8 XCDs
inline unsigned grid_for(int64_t n_rows) { return static_cast<unsigned>((((n_rows + 3) / 4) + 7) & ~int64_t{7}); }

#if defined(__HIPCC__)
// ReLU that lets a NaN through, as torch.relu does (fmaxf(NaN, 0) is 0: a poisoned row would come out of the forward pass as
// zeros, with a finite loss, and only show as non-finite GRADIENTS — seen in round 3 when an un-normalised stack overflowed)
__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
// float4 arithmetic, component by component, in place: a += w * v, a += v, a *= s, a /= d (a true division, as torch_scatter's
// out.div_(count)) ...
__device__ __forceinline__ void f4_fma(float4& a, float w, const float4& v) {
  a.x = fmaf(w, v.x, a.x);
  a.y = fmaf(w, v.y, a.y);
  a.z = fmaf(w, v.z, a.z);
  a.w = fmaf(w, v.w, a.w);
}
__device__ __forceinline__ void f4_add(float4& a, const float4& v) {
  a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
}
__device__ __forceinline__ void f4_scale(float4& a, float s) {
  a.x *= s; a.y *= s; a.z *= s; a.w *= s;
}
__device__ __forceinline__ void f4_div(float4& a, float d) {
  a.x /= d; a.y /= d; a.z /= d; a.w /= d;
}
// ... and by value: s += v (where the in-place form, whose second operand is a reference, compiles differently:
// profiles/rowwave_isa_identity.md), w * v + a of three float4, and v or zeros by a select (not a multiply by zero: a non-finite
// value must not leak)
__device__ __forceinline__ void acc4(float4& s, const float4 v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
__device__ __forceinline__ float4 f4_madd(float4 w, float4 v, float4 a) {
  return make_float4(fmaf(w.x, v.x, a.x), fmaf(w.y, v.y, a.y), fmaf(w.z, v.z, a.z), fmaf(w.w, v.w, a.w));
}
__device__ __forceinline__ float4 f4_keep(bool keep, const float4& v) {
  return make_float4(keep ? v.x : 0.f, keep ? v.y : 0.f, keep ? v.z : 0.f, keep ? v.w : 0.f);
}

// MFMA vocabulary: native vectors (operands, accumulators; a staging copy of one is a register move, where a float4 struct copy
// can become a memcpy through scratch), and the C/D layout of the 32 x 32 tile: lane l, register r -> row d_row32(r, l >> 5),
// column l & 31
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ int d_row32(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
// XCD-aware tile order: consecutive block ids go round-robin over the 8 XCDs; ids b, b + 8, ... (one XCD) take the `tiles_n`
// column tiles of the same row block one after the other
__device__ __forceinline__ void xcd_tile(int b, int tiles_n, int& tile_m, int& tile_n) {
  const int group = b / (8 * tiles_n), in_group = b - group * 8 * tiles_n;
  tile_m = group * 8 + (in_group & 7);
  tile_n = in_group >> 3;
}
// 16-byte moves of the GEMM K loops (gemm.hip, lstm.hip) ...
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
// ... and column k of a first operand [p | q] that is two matrices, never concatenated: q takes over at k = K0
template <bool TWO>
__device__ __forceinline__ const float* seam_at(const float* p, const float* q, int k, int K0) {
  return TWO ? (k < K0 ? p + k : q + (k - K0)) : p + k;
}


// Wave-wide reductions on the DPP cross-lane paths (no LDS round trip as with __shfl_xor / ds_bpermute):
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror reduce each 16-lane row; v_readlane joins the 4 rows.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v) {
  return static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float lane_value(float v, int lane) {   // lane must be wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x141>(v));
  v = fmaxf(v, dpp_mov<0x140>(v));
  return v;
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
  v = row16_sum(v);
  return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
}
__device__ __forceinline__ float wave_max_dpp(float v) {
  v = row16_max(v);
  return fmaxf(fmaxf(lane_value(v, 0), lane_value(v, 16)), fmaxf(lane_value(v, 32), lane_value(v, 48)));
}

// Philox-4x32-10 (Salmon et al. 2011): 4 x 32 random bits for counter (c0..c3), key (k0,k1).  The project's dropout masks:
// counter = (element index lo, hi, call id, training step lo), key = (seed lo, seed hi ^ step hi).
__device__ __forceinline__ uint4 philox(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c.x), l0 = 0xD2511F53u * c.x;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c.z), l1 = 0xCD9E8D57u * c.z;
    c = make_uint4(h1 ^ c.y ^ k.x, l1, h0 ^ c.w ^ k.y, l0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}
// The stream itself, written once: the four words of 64-bit element index idx (tests/test_gpu_random_streams.py holds its known
// answers).  A consumer owns only its index formula.
__device__ __forceinline__ uint4 stream_bits(uint64_t seed, uint64_t step, uint32_t call_id, uint64_t idx) {
  return philox(make_uint4(static_cast<uint32_t>(idx), static_cast<uint32_t>(idx >> 32), call_id, static_cast<uint32_t>(step)),
                make_uint2(static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32) ^ static_cast<uint32_t>(step >> 32)));
}
// Dropout at probability p drops a word below this threshold ...
__host__ __device__ __forceinline__ uint32_t drop_threshold(float p) { return static_cast<uint32_t>(static_cast<double>(p) * 4294967296.0); }
// ... and the factors of four words: 0 for a dropped element, `kept` (1 / (1 - p), or the caller's scale) otherwise
__device__ __forceinline__ float4 keep_factors(uint4 r, uint32_t thr, float kept) {
  return make_float4(r.x >= thr ? kept : 0.f, r.y >= thr ? kept : 0.f, r.z >= thr ? kept : 0.f, r.w >= thr ? kept : 0.f);
}
#endif

// wgrad.hip: fixed-order sum of S partial-result slabs (used by the weight-gradient kernels)
int launch_slab_reduce(const float* slab, const float* slab_b, int S, int out_f, int in_f, int out_pad, int in_pad, float* dw,
                       int64_t ld_dw, float* db, hipStream_t s);

}  // namespace agnn
