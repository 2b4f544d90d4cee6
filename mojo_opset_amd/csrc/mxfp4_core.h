// Device helpers and constants shared by the MXFP4 units (mxfp4_gemm.hip, mxfp4_group_gemm.hip): the scaled
// fp4 matrix instruction, the loads of a super-tile's data and scale pieces, and the output vector store.  The super-tile cut
// (512 elements; lane group g owns the consecutive blocks 4g .. 4g+3) is described at the head of mxfp4_gemm.hip.
#pragma once

#include "common.h"

namespace mojo {
namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int MX_BLOCK = 32;                 // elements per scale
constexpr int MX_ST_BYTES = 256;             // data bytes per row and super-tile (512 elements, 16 blocks)
constexpr int MX_ST_BLOCKS = 16;
constexpr int MX_TILE = 128;                 // tile form: outputs per workgroup, both ways
constexpr int MX_THREADS = 256;
constexpr int MX_SKINNY_MAX_M = 32;
constexpr int MX_MAX_SPLIT = 16;
constexpr int MX_SKINNY_WAVES = 2048;        // waves a skinny launch aims at (8 per CU of the 256)

// D += W(16 x 128) x A(128 x 16) with fp4 operands: block scale byte OPSEL of sw / sa
template <int OPSEL>
__device__ __forceinline__ f32x4 mx_mma(u32x4 w, u32x4 a, f32x4 c, int sw, int sa) {
  const i32x8 w8 = {static_cast<int>(w[0]), static_cast<int>(w[1]), static_cast<int>(w[2]), static_cast<int>(w[3]), 0, 0, 0, 0};
  const i32x8 a8 = {static_cast<int>(a[0]), static_cast<int>(a[1]), static_cast<int>(a[2]), static_cast<int>(a[3]), 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w8, a8, c, 4, 4, OPSEL, sw, OPSEL, sa);
}

// scale bytes of blocks b0 .. b0+3 of a row of kb blocks as one dword (byte s = block b0 + s); a block past the row: 127
__device__ __forceinline__ int mx_scale4(const uint8_t* row, int b0, int kb) {
  if (b0 + 4 <= kb) {
    int v;
    __builtin_memcpy(&v, row + b0, 4);
    return v;
  }
  unsigned v = 0x7f7f7f7fu;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (b0 + s < kb) v = (v & ~(0xffu << (8 * s))) | (static_cast<unsigned>(row[b0 + s]) << (8 * s));
  return static_cast<int>(v);
}

// 16 data bytes at byte `off` of a row of k2 bytes (both multiples of 16); zeros past the row
__device__ __forceinline__ u32x4 mx_chunk(const uint8_t* row, int off, int k2) {
  return off < k2 ? *reinterpret_cast<const u32x4*>(row + off) : u32x4{0u, 0u, 0u, 0u};
}

template <typename TO>
__device__ __forceinline__ void mx_store4(TO* dst, f32x4 acc) {
  typename vec_of<TO, 4>::type o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = elt<TO>::from_f(acc[e]);
  *reinterpret_cast<typename vec_of<TO, 4>::type*>(dst) = o;
}

}  // namespace
}  // namespace mojo
