// The two elementwise ends of the int8 / fp8 domain:
//   MojoStaticQuant  mojo_opset/core/operators/quantize.py:9-74
//     q = clamp(round_half_even(x.float() / scale.float()), q_min, q_max)  -> int8, or float8_e4m3fn of that INTEGER value
//   MojoDequant      mojo_opset/core/operators/quantize.py:77-117
//     out = round_to_T(q.float() * scale.float()),  T in {fp16, bf16, fp32}
//
// `scale` is fp32.  Trailing-dimensions form: the flattened element i uses scale[i % scale_len].  Per-token form (dequant
// only; what the dynamic quantisers return): element i uses scale[i / dim].  Grid-stride over vectors of VEC elements (16
// bytes of x for the quantiser; 8 quantised bytes, 16 or 32 bytes out, for the dequantiser); the scale index is computed per
// VECTOR, once with 64-bit arithmetic before the loop and by add-and-wrap per trip, so no thread divides inside the loop.  The
// wide forms need scale_len (resp. dim) to be a multiple of VEC: a vector then never wraps the scale (resp. crosses a row).
// The division and the product are the IEEE single operations, each value is rounded once: the bytes equal the golden's.
//
// Algorithmic bytes per element: static quant elt + 1, dequant 1 + elt (+ the scale, cache-resident).
#include <math.h>

#include "common.h"
#include "quant_common.h"

namespace mojo {

template <typename T, int VEC, bool NT>
__global__ __launch_bounds__(256) void static_quant_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                           unsigned char* __restrict__ out, int64_t n_vec, int64_t scale_vecs,
                                                           float q_min, float q_max, int fp8) {
  typedef typename vec_of<T, VEC>::type V;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  const int64_t step = stride % scale_vecs;                   // how far the scale index moves per trip
  int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  int64_t sv = v % scale_vecs;                                // index of the scale vector of x vector v
  for (; v < n_vec; v += stride) {
    const V xv = NT ? load_vec_nt<T, VEC>(x + v * VEC) : load_vec<T, VEC>(x + v * VEC);
    float s[VEC];
    load_f32_vec<VEC>(scale, sv, s);
    unsigned char q[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) q[j] = quant_byte(rintf(__fdiv_rn(elt<T>::to_f(vget<T, VEC>(xv, j)), s[j])), q_min, q_max, fp8);
    store_quant_bytes<VEC, NT>(out + v * VEC, q);
    sv += step;
    if (sv >= scale_vecs) sv -= scale_vecs;
  }
}

// PER_TOKEN: scale[i / dim] (row_vecs = dim / VEC vectors per row); otherwise scale[i % scale_len] (scale_vecs = scale_len / VEC)
template <typename T, int VEC, bool PER_TOKEN, bool NT>
__global__ __launch_bounds__(256) void dequant_kernel(const unsigned char* __restrict__ q, const float* __restrict__ scale,
                                                      T* __restrict__ out, int64_t n_vec, int64_t period_vecs, int fp8) {
  typedef typename vec_of<T, VEC>::type V;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  const int64_t step_rem = stride % period_vecs, step_quot = stride / period_vecs;
  int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  int64_t rem = v % period_vecs, quot = v / period_vecs;      // trailing: rem = scale vector; per token: quot = row
  for (; v < n_vec; v += stride) {
    unsigned char b[VEC];
    if constexpr (VEC == 8) {
      const u32x2 w = NT ? __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(q + v * 8)) : *reinterpret_cast<const u32x2*>(q + v * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = static_cast<unsigned char>(w[j >> 2] >> (8 * (j & 3)));
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) b[j] = q[v * VEC + j];
    }
    float s[VEC];
    if constexpr (PER_TOKEN) {
      const float row_scale = scale[quot];
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] = row_scale;
    } else {
      load_f32_vec<VEC>(scale, rem, s);
    }
    V o;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float f = fp8 ? from_fp8_e4m3(b[j]) : static_cast<float>(static_cast<signed char>(b[j]));
      float p = __fmul_rn(f, s[j]);
      // The product is rounded to fp32 and THEN to T, as the golden rounds it.  Left alone, hipcc folds the multiply and the
      // conversion to fp16 into one v_fma_mixlo_f16, which rounds the exact product once: 2 of 32768 random elements differed.
      asm volatile("" : "+v"(p));
      vset<T, VEC>(o, j, elt<T>::from_f(p));
    }
    if constexpr (VEC == 8 && sizeof(T) == 4) {                // 32 bytes: two 16-byte stores
      f32x4 lo, hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) { lo[j] = vget<T, VEC>(o, j); hi[j] = vget<T, VEC>(o, 4 + j); }
      f32x4* dst = reinterpret_cast<f32x4*>(out + v * 8);
      if (NT) { __builtin_nontemporal_store(lo, dst); __builtin_nontemporal_store(hi, dst + 1); } else { dst[0] = lo; dst[1] = hi; }
    } else {
      if (NT) store_vec_nt<T, VEC>(out + v * VEC, o); else store_vec<T, VEC>(out + v * VEC, o);
    }
    rem += step_rem;
    quot += step_quot;
    if (rem >= period_vecs) { rem -= period_vecs; quot += 1; }
  }
}

static unsigned elementwise_blocks(int64_t n_vec) {
  const int64_t want = ceil_div(n_vec, 256);
  return static_cast<unsigned>(want > 256 * 32 ? 256 * 32 : want);
}

template <typename T>
static int launch_static_quant(const void* input, const float* scale, void* out, int64_t n, int64_t scale_len, float q_min,
                               float q_max, int fp8, hipStream_t s) {
  constexpr int WIDE = 16 / sizeof(T);
  const bool wide = scale_len % WIDE == 0 && aligned_to(input, 16) && aligned_to(scale, 16) && aligned_to(out, WIDE);
  const bool nt = wide && stream_nt(n * static_cast<long long>(sizeof(T) + 1));     // (the scalar form has no non-temporal twin)
  const T* x = static_cast<const T*>(input);
  unsigned char* q = static_cast<unsigned char*>(out);
  // (n is a multiple of scale_len: the entry point checks it)
  if (nt) hipLaunchKernelGGL((static_quant_kernel<T, WIDE, true>), dim3(elementwise_blocks(n / WIDE)), dim3(256), 0, s, x, scale, q, n / WIDE, scale_len / WIDE, q_min, q_max, fp8);
  else if (wide) hipLaunchKernelGGL((static_quant_kernel<T, WIDE, false>), dim3(elementwise_blocks(n / WIDE)), dim3(256), 0, s, x, scale, q, n / WIDE, scale_len / WIDE, q_min, q_max, fp8);
  else hipLaunchKernelGGL((static_quant_kernel<T, 1, false>), dim3(elementwise_blocks(n)), dim3(256), 0, s, x, scale, q, n, scale_len, q_min, q_max, fp8);
  MOJO_CHECK_LAUNCH("static_quant");
  note_launch("static_quant:%s:%s", wide ? "wide" : "scalar", nt ? "nt" : "cached");
  return MOJO_OK;
}

template <typename T>
static int launch_dequant(const void* input, const float* scale, void* out, int64_t n, int64_t period, int per_token, int fp8,
                          hipStream_t s) {
  constexpr int WIDE = 8;
  const bool wide = period % WIDE == 0 && aligned_to(input, 8) && aligned_to(out, 16) && (per_token || aligned_to(scale, 16));
  const bool nt = wide && stream_nt(n * static_cast<long long>(sizeof(T) + 1));
  const unsigned char* q = static_cast<const unsigned char*>(input);
  T* o = static_cast<T*>(out);
#define DEQUANT(VEC_, TOKEN_, NT_) hipLaunchKernelGGL((dequant_kernel<T, VEC_, TOKEN_, NT_>), dim3(elementwise_blocks(n / VEC_)), dim3(256), 0, s, q, scale, o, n / VEC_, period / VEC_, fp8)
  if (per_token) { if (nt) DEQUANT(WIDE, true, true); else if (wide) DEQUANT(WIDE, true, false); else DEQUANT(1, true, false); }
  else { if (nt) DEQUANT(WIDE, false, true); else if (wide) DEQUANT(WIDE, false, false); else DEQUANT(1, false, false); }
#undef DEQUANT
  MOJO_CHECK_LAUNCH("dequant");
  note_launch("dequant:%s:%s:%s", per_token ? "token" : "trailing", wide ? "wide" : "scalar", nt ? "nt" : "cached");
  return MOJO_OK;
}

}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_static_quant(const void* input, const float* scale, void* out_q, int64_t n, int64_t scale_len, int dtype,
                                     int quant_dtype, mojo_stream_t stream) {
  if (n == 0) return MOJO_OK;
  MOJO_REQUIRE(input && scale && out_q, MOJO_EINVAL, "static_quant: null pointer");
  MOJO_REQUIRE(n > 0 && scale_len > 0 && n % scale_len == 0, MOJO_EINVAL,
               "static_quant: %lld elements are no whole number of scales of %lld", (long long)n, (long long)scale_len);
  MOJO_REQUIRE(quant_dtype == MOJO_I8 || quant_dtype == MOJO_F8E4M3, MOJO_EUNSUPPORTED,
               "static_quant: quant dtype %d (int8 / fp8-e4m3 only)", quant_dtype);
  const int fp8 = quant_dtype == MOJO_F8E4M3;
  const float q_max = fp8 ? 448.f : 127.f, q_min = fp8 ? -448.f : -128.f;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MOJO_F32: return launch_static_quant<float>(input, scale, out_q, n, scale_len, q_min, q_max, fp8, s);
    case MOJO_F16: return launch_static_quant<f16_t>(input, scale, out_q, n, scale_len, q_min, q_max, fp8, s);
    case MOJO_BF16: return launch_static_quant<bf16_t>(input, scale, out_q, n, scale_len, q_min, q_max, fp8, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "static_quant: dtype %d not supported", dtype);
  }
}

extern "C" int mojo_hip_dequant(const void* input, const float* scale, void* out, int64_t n, int64_t scale_len, int64_t token_dim,
                                int in_dtype, int out_dtype, mojo_stream_t stream) {
  if (n == 0) return MOJO_OK;
  MOJO_REQUIRE(input && scale && out, MOJO_EINVAL, "dequant: null pointer");
  MOJO_REQUIRE(in_dtype == MOJO_I8 || in_dtype == MOJO_F8E4M3, MOJO_EUNSUPPORTED, "dequant: input dtype %d (int8 / fp8-e4m3 only)", in_dtype);
  const int per_token = token_dim > 0;
  if (per_token)
    MOJO_REQUIRE(n > 0 && n % token_dim == 0 && scale_len == n / token_dim, MOJO_EINVAL,
                 "dequant: %lld elements in rows of %lld need %lld per-token scales, got %lld", (long long)n, (long long)token_dim,
                 (long long)(n / token_dim), (long long)scale_len);
  else
    MOJO_REQUIRE(n > 0 && scale_len > 0 && n % scale_len == 0, MOJO_EINVAL,
                 "dequant: %lld elements are no whole number of scales of %lld", (long long)n, (long long)scale_len);
  const int64_t period = per_token ? token_dim : scale_len;
  const int fp8 = in_dtype == MOJO_F8E4M3;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (out_dtype) {
    case MOJO_F32: return launch_dequant<float>(input, scale, out, n, period, per_token, fp8, s);
    case MOJO_F16: return launch_dequant<f16_t>(input, scale, out, n, period, per_token, fp8, s);
    case MOJO_BF16: return launch_dequant<bf16_t>(input, scale, out, n, period, per_token, fp8, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "dequant: output dtype %d not supported", out_dtype);
  }
}
