// The activation device functions of activation.hip, shared with the kernels that fuse one (causal_conv1d.hip): fp32 math on an
// fp32 argument, the caller rounds once to its storage type T.  T selects the form: the 16-bit forms use the hardware exp2 / rcp
// (1 ulp of fp32, far inside the output's last place), fp32 takes the library erfcf / expf and the IEEE division.
#pragma once
#include "common.h"

namespace mojo {

enum { ACT_GELU_ERF = 0, ACT_SILU = 1 };

// Two elements at a time: the fp32 pair operations of gfx950 (v_pk_mul / v_pk_add / v_pk_fma) halve the VALU work of the
// 16-bit forms, which would otherwise bound the kernel, not HBM.
__device__ __forceinline__ f32x2 exp2_pair(f32x2 x) { return f32x2{fast_exp2(x[0]), fast_exp2(x[1])}; }
__device__ __forceinline__ f32x2 rcp_pair(f32x2 x) { return f32x2{__builtin_amdgcn_rcpf(x[0]), __builtin_amdgcn_rcpf(x[1])}; }

template <typename T, int KIND>
__device__ __forceinline__ float activate(float x);

template <typename T, int KIND>
__device__ __forceinline__ f32x2 activate_pair(f32x2 x) {
  if constexpr (sizeof(T) == 2 && KIND == ACT_GELU_ERF) {
    // erfc(z) = t * exp(-z^2 + P(t)), t = 2 / (2 + z), z >= 0: the Chebyshev fit of Numerical Recipes (erfcc, section 6.2),
    // relative error below 1.2e-7 on the whole half line -- the library erfcf costs three times the instructions.  The
    // exponential is taken as the square of exp(arg / 2), which stays a normal number for every input whose result is
    // not zero in bf16 (the raw exp2 flushes subnormal results).  q * h = Phi(-|x|) = erfc(|x| / sqrt 2) / 2.
    const f32x2 z = __builtin_elementwise_abs(x) * 0.70710678118654752440f;
    const f32x2 t = rcp_pair(z + 2.0f) * 2.0f;
    f32x2 p = t * 0.17087277f + -0.82215223f;
    p = p * t + 1.48851587f;
    p = p * t + -1.13520398f;
    p = p * t + 0.27886807f;
    p = p * t + -0.18628806f;
    p = p * t + 0.09678418f;
    p = p * t + 0.37409196f;
    p = p * t + 1.00002368f;
    p = p * t + -1.26551223f;
    const f32x2 h = exp2_pair((p - z * z) * 0.72134752044448170368f);
    const f32x2 q = (t * 0.5f) * h;
    // x > 0: x * (1 - Phi(-x)) as x - x * Phi(-x), which is NaN at +inf (inf - inf * 0) as torch's gelu is.  Zeros of either
    // sign and NaN take `neg`, x * Phi(x): it keeps the sign of zero and NaN stays NaN.
    const f32x2 pos = x - x * (q * h), neg = (x * q) * h;
    return f32x2{x[0] > 0.f ? pos[0] : neg[0], x[1] > 0.f ? pos[1] : neg[1]};
  } else if constexpr (sizeof(T) == 2) {
    const f32x2 h = exp2_pair(__builtin_elementwise_abs(x) * -0.72134752044448170368f);    // exp(-|x| / 2)
    const f32x2 r = rcp_pair(h * h + 1.0f);
    const f32x2 m = f32x2{x[0] >= 0.f ? 1.0f : h[0], x[1] >= 0.f ? 1.0f : h[1]};           // NaN: h, which is NaN
    return ((x * m) * m) * r;
  } else if constexpr (KIND == ACT_GELU_ERF) {
    f32x2 y;
#pragma unroll
    for (int i = 0; i < 2; ++i) y[i] = activate<T, KIND>(x[i]);
    return y;
  } else {
    f32x2 y;
#pragma unroll
    for (int i = 0; i < 2; ++i) y[i] = activate<T, KIND>(x[i]);
    return y;
  }
}

template <typename T, int KIND>
__device__ __forceinline__ float activate(float x) {
  if constexpr (sizeof(T) == 2) {
    return activate_pair<T, KIND>(f32x2{x, x})[0];
  } else if constexpr (KIND == ACT_GELU_ERF) {
    const float half_x = __fmul_rn(x, 0.5f), tail = erfcf(__fmul_rn(fabsf(x), 0.70710678118654752440f));     // 2 Phi(-|x|)
    return x > 0.f ? x - half_x * tail : half_x * tail;     // +inf: NaN (inf - inf * 0), as torch's gelu; -0 stays -0
  } else {
    const float e = expf(-fabsf(x));
    return x >= 0.f ? x / (1.0f + e) : x * (e / (1.0f + e));
  }
}

}  // namespace mojo
