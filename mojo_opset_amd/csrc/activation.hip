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
#include "activation_math.h"
#include "common.h"

namespace mojo {

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
