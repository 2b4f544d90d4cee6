// MojoGelu (erf form) / MojoSilu: one elementwise pass, fp32 math, ONE rounding to the storage type.
//   gelu(x) = x * 0.5 * (1 + erf(x * sqrt(1/2)))         silu(x) = x / (1 + exp(-x))
// Both are evaluated in forms that keep their relative accuracy in the negative tail, where the textbook forms lose it in
// fp32: 1 + erff(z) cancels (at x = -5 its error is a tenth of the result, which bf16 still represents), so the kernel takes
// 1 + erf(z) = erfc(-z); expf(-x) overflows from x = -88.8 on while x / (1 + exp(-x)) is still a normal bf16 number there, so
// for x < 0 the kernel takes x * e / (1 + e) with e = exp(x) <= 1.
// The 16-bit forms use the hardware exp2 / rcp (1 ulp of fp32, far inside the output's last place) on h = exp(arg / 2),
// which stays a normal number for every input whose result is not zero (e = h * h), and for GELU a Chebyshev fit of erfc
// (activate_pair); they work on pairs of elements.  fp32 outputs take the library erfcf / expf and the IEEE division.
//
// 16-byte vectors in a grid-stride loop when both pointers allow, single elements otherwise; the n % VEC tail by elements.
// `out` may be `in`: a thread reads its vector before it writes it and touches no other.
// Algorithmic bytes: n x elt read + the same written.
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

template <typename T, int VEC, int KIND, bool NT>
__global__ __launch_bounds__(256) void activation_kernel(const T* in, T* out, int64_t n) {
  typedef typename vec_of<T, VEC>::type V;
  const int64_t n_vec = n / VEC;
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t step = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t v = tid; v < n_vec; v += step) {
    const V x = NT ? load_vec_nt<T, VEC>(in + v * VEC) : load_vec<T, VEC>(in + v * VEC);
    V o;
    if constexpr (VEC > 1) {
#pragma unroll
      for (int j = 0; j < VEC; j += 2) {
        const f32x2 y = activate_pair<T, KIND>(f32x2{elt<T>::to_f(vget<T, VEC>(x, j)), elt<T>::to_f(vget<T, VEC>(x, j + 1))});
        vset<T, VEC>(o, j, elt<T>::from_f(y[0]));
        vset<T, VEC>(o, j + 1, elt<T>::from_f(y[1]));
      }
    } else {
      vset<T, VEC>(o, 0, elt<T>::from_f(activate<T, KIND>(elt<T>::to_f(vget<T, VEC>(x, 0)))));
    }
    if (NT) store_vec_nt<T, VEC>(out + v * VEC, o); else store_vec<T, VEC>(out + v * VEC, o);
  }
  if constexpr (VEC > 1) {                                              // the scalar tail: fewer than VEC elements
    const int64_t i = n_vec * VEC + tid;
    if (i < n) out[i] = elt<T>::from_f(activate<T, KIND>(elt<T>::to_f(in[i])));
  }
}

template <typename T, int KIND>
static int dispatch_activation(const void* in, void* out, int64_t n, hipStream_t s) {
  constexpr int WIDE = 16 / sizeof(T);
  const T* x = static_cast<const T*>(in);
  T* o = static_cast<T*>(out);
  const bool wide = aligned_to(in, 16) && aligned_to(out, 16);
  const bool nt = wide && stream_nt(2 * n * static_cast<long long>(sizeof(T)));
  int64_t blocks = ceil_div(wide ? ceil_div(n, WIDE) : n, 256);
  if (blocks > 256 * 32) blocks = 256 * 32;
  if (nt) hipLaunchKernelGGL((activation_kernel<T, WIDE, KIND, true>), dim3(blocks), dim3(256), 0, s, x, o, n);
  else if (wide) hipLaunchKernelGGL((activation_kernel<T, WIDE, KIND, false>), dim3(blocks), dim3(256), 0, s, x, o, n);
  else hipLaunchKernelGGL((activation_kernel<T, 1, KIND, false>), dim3(blocks), dim3(256), 0, s, x, o, n);
  MOJO_CHECK_LAUNCH("activation");
  note_launch("activation:%s:vec%d:%s", KIND == ACT_GELU_ERF ? "gelu_erf" : "silu", wide ? WIDE : 1, nt ? "nt" : "plain");
  return MOJO_OK;
}

template <typename T>
static int dispatch_activation_kind(const void* in, void* out, int64_t n, int kind, hipStream_t s) {
  return kind == ACT_GELU_ERF ? dispatch_activation<T, ACT_GELU_ERF>(in, out, n, s) : dispatch_activation<T, ACT_SILU>(in, out, n, s);
}

}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_activation(const void* in, void* out, int64_t n, int kind, int dtype, mojo_stream_t stream) {
  if (n == 0) return MOJO_OK;
  MOJO_REQUIRE(in && out && n > 0, MOJO_EINVAL, "activation: null pointer or negative size");
  MOJO_REQUIRE(kind == ACT_GELU_ERF || kind == ACT_SILU, MOJO_EINVAL, "activation: kind %d (0 = gelu_erf, 1 = silu)", kind);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MOJO_F32: return dispatch_activation_kind<float>(in, out, n, kind, s);
    case MOJO_F16: return dispatch_activation_kind<f16_t>(in, out, n, kind, s);
    case MOJO_BF16: return dispatch_activation_kind<bf16_t>(in, out, n, kind, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "activation: dtype %d not supported", dtype);
  }
}
