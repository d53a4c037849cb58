// What the row-per-wave kernels share (spmm.hip, gated.hip, reledge.hip, the row passes of hgt.hip; not part of the C-ABI): a
// workgroup of 256 is four 64-lane waves, a wave owns one output row and walks that row's CSR neighbours, and a lane holds 4
// consecutive floats of every 256-float chunk of a row, so a kernel built for CH chunks serves H <= 256 * CH.  Workgroups are
// renumbered so that each of the 8 XCDs works on a contiguous slab of rows (agnn::grid_for gives the matching grid).  A new
// kernel of this family brings its own walk and arithmetic and takes the rest from here.
#pragma once
#include <type_traits>

#include "agnn_common.h"

namespace agnn {

#if defined(__HIPCC__)
// The row of this wave in a grid of n_blocks workgroups (a multiple of 8) of which this is workgroup `block`: the whole grid, or
// a sub-range of it with a block index and count of the kernel's own.  UNIFORM reads the wave index through readfirstlane, which
// tells the compiler that the row is wave-uniform (scalar index loads); without it the row is a vector value.  The two compile
// differently: a kernel keeps the form it was measured with.
template <bool UNIFORM, typename B, typename G>
__device__ __forceinline__ int wave_row(B block, G n_blocks) {
  if (UNIFORM) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // read first: the order is the compiler's too
    const int vb = (block & 7) * (n_blocks >> 3) + (block >> 3);
    return vb * 4 + wave;
  }
  return ((block & 7) * (n_blocks >> 3) + (block >> 3)) * 4 + (threadIdx.x >> 6);
}
template <bool UNIFORM>
__device__ __forceinline__ int wave_row() {
  return wave_row<UNIFORM>(blockIdx.x, gridDim.x);      // the accessors themselves: read where the formula uses them
}

// The chunk layout, chunk by chunk (scalars and values only: a helper that takes the kernel's on[] or accumulator arrays by
// reference keeps them in memory until it is inlined, and the kernels then compile differently).  Chunk c of a row of H floats is
// this lane's when its 4 floats lie inside the row ...
__device__ __forceinline__ bool chunk_on(int c, int lane, int H) { return (c * 256 + lane * 4) < H; }
// ... its float4 of the row at `row`, zeros where the chunk is not the lane's ...
__device__ __forceinline__ float4 chunk_load(const float* row, int c, int lane, bool on) {
  return on ? reinterpret_cast<const float4*>(row)[c * 64 + lane] : f4_zero();
}
// ... and the store of a chunk that is the lane's; `add` puts v on top of what the row holds (the accumulate paths)
__device__ __forceinline__ void chunk_store(float* row, int c, int lane, float4 v, bool add = false) {
  float4* q = reinterpret_cast<float4*>(row);
  if (add) f4_add(v, q[c * 64 + lane]);
  q[c * 64 + lane] = v;
}
#endif

// Host side.  The instantiation for a width: f(std::integral_constant<int, CH>) with CH = 1, 2 or 4 chunks
template <typename F>
inline void for_width(int32_t H, F&& f) {
  if (H <= 256) f(std::integral_constant<int, 1>{});
  else if (H <= 512) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}

// The shape of a launch: AGNN_OK to go on, a negative code when refused, 1 when there is no row and nothing to do
inline int check_wave_rows(const char* who, int64_t n_rows, int32_t H) {
  if (n_rows < 0 || n_rows >= (int64_t{1} << 31)) return fail(AGNN_EINVAL, "%s: n_rows=%lld", who, (long long)n_rows);
  if (H <= 0 || (H & 3) != 0 || H > 1024) return fail(AGNN_EINVAL, "%s: H=%d must be a multiple of 4 in [4,1024]", who, H);
  return n_rows == 0 ? 1 : AGNN_OK;
}

// A [rows, >= H] float matrix that a kernel reads or writes with float4: the layout alone, for an entry point that reports
// several operands in one message of its own ...
inline bool f4_rows(const void* p, int64_t ld, int64_t H) { return aligned16(p) && (ld & 3) == 0 && ld >= H; }
// ... and the validator that names the operand (`who` may carry a segment: "link_bce_fwd: task 3")
inline int check_matrix(const char* who, const char* name, const void* p, int64_t ld, int32_t H) {
  if (!p) return fail(AGNN_EINVAL, "%s: %s is null", who, name);
  if (ld < H) return fail(AGNN_EINVAL, "%s: ld_%s=%lld < H=%d", who, name, (long long)ld, H);
  if (ld % 4 != 0) return fail(AGNN_EALIGN, "%s: ld_%s=%lld is not a multiple of 4", who, name, (long long)ld);
  if (!aligned16(p)) return fail(AGNN_EALIGN, "%s: %s is not 16-byte aligned", who, name);
  return AGNN_OK;
}

}  // namespace agnn
