// What the quantising kernels share (norm_quant.hip, quant_elementwise.hip, dequant_swiglu_quant.hip): the row maximum of a
// 256-thread workgroup, the fp8 conversions, round_half_even(y / scale) with its reciprocal shortcut, and the clamp-and-pack of
// one vector of quantised values.
#pragma once
#include <math.h>

#include "common.h"

namespace mojo {

__device__ __forceinline__ float block_max256(float x, float* smem) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) smem[wave] = x;
  __syncthreads();
  const float r = fmaxf(fmaxf(smem[0], smem[1]), fmaxf(smem[2], smem[3]));
  __syncthreads();
  return r;
}

__device__ __forceinline__ unsigned char to_fp8_e4m3(float v) {
  // v_cvt_pk_fp8_f32: OCP e4m3 (the "fn" format) on gfx950, round to nearest even
  const int packed = __builtin_amdgcn_cvt_pk_fp8_f32(v, v, 0, false);
  return static_cast<unsigned char>(packed & 0xff);
}

// round_half_even(y / scale), bit-identical to the IEEE division, at the price of one multiply for almost every element:
// t = y * (1/scale) is within a few ulp of the true quotient, so rint(t) can only differ from rint(y / scale) when t sits
// within that distance of a rounding boundary (k + 0.5); only those elements take the real division.  |t| <= ~448.
__device__ __forceinline__ float round_quotient(float y, float scale, float inv_scale) {
  const float t = y * inv_scale;
  const float r = rintf(t);
  if (fabsf(fabsf(t - r) - 0.5f) < 1e-3f) return rintf(__fdiv_rn(y, scale));
  return r;
}

// OCP e4m3 byte -> float (v_cvt_f32_fp8, exact)
__device__ __forceinline__ float from_fp8_e4m3(unsigned char b) {
  return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(b), 0);
}

// clamp(rq, q_min, q_max) as int8, or as float8_e4m3fn of that integer value
__device__ __forceinline__ unsigned char quant_byte(float rq, float q_min, float q_max, int fp8) {
  const float c = fminf(fmaxf(rq, q_min), q_max);
  return fp8 ? to_fp8_e4m3(c) : static_cast<unsigned char>(static_cast<signed char>(static_cast<int>(c)));
}

// VEC quantised bytes to dst: one 8- or 4-byte store where VEC allows (dst aligned to VEC), byte stores otherwise
template <int VEC, bool NT>
__device__ __forceinline__ void store_quant_bytes(unsigned char* dst, const unsigned char (&q)[VEC]) {
  if constexpr (VEC == 8) {
    u32x2 w;
    w[0] = q[0] | (q[1] << 8) | (q[2] << 16) | (static_cast<unsigned>(q[3]) << 24);
    w[1] = q[4] | (q[5] << 8) | (q[6] << 16) | (static_cast<unsigned>(q[7]) << 24);
    if (NT) __builtin_nontemporal_store(w, reinterpret_cast<u32x2*>(dst)); else *reinterpret_cast<u32x2*>(dst) = w;
  } else if constexpr (VEC == 4) {
    const unsigned w = q[0] | (q[1] << 8) | (q[2] << 16) | (static_cast<unsigned>(q[3]) << 24);
    if (NT) __builtin_nontemporal_store(w, reinterpret_cast<unsigned*>(dst)); else *reinterpret_cast<unsigned*>(dst) = w;
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) dst[j] = q[j];
  }
}

// q = clamp(round_half_even(f / scale), q_min, q_max) of one vector, stored.  rint(f * (1 / scale)) with the exact-division
// fallback decided once per VECTOR (norm_quant_kernel's `emit`): |t - rint(t)| <= 0.5 always, so "within 1e-3 of a rounding
// boundary" is "its maximum over the vector > 0.499".
template <int VEC, bool NT>
__device__ __forceinline__ void quantise_store(unsigned char* dst, const float (&f)[VEC], float scale, float inv_scale,
                                               float q_min, float q_max, int fp8) {
  float rq[VEC];
  float near = 0.f;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const float t = f[j] * inv_scale;
    rq[j] = rintf(t);
    near = fmaxf(near, fabsf(t - rq[j]));
  }
  if (near > 0.499f) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) rq[j] = round_quotient(f[j], scale, inv_scale);
  }
  unsigned char q[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) q[j] = quant_byte(rq[j], q_min, q_max, fp8);
  store_quant_bytes<VEC, NT>(dst, q);
}

// VEC floats of a per-column fp32 vector, element v * VEC on (16-byte loads when VEC is a multiple of 4: p 16-byte aligned)
template <int VEC>
__device__ __forceinline__ void load_f32_vec(const float* p, int64_t v, float (&dst)[VEC]) {
  if constexpr (VEC % 4 == 0) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p + v * VEC + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) dst[4 * q + e] = t[e];
    }
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) dst[j] = p[v * VEC + j];
  }
}

}  // namespace mojo
