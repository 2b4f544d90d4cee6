// What the quantising kernels share (norm_quant.hip, quant_moe.hip, dequant_swiglu_quant.hip, quant_elementwise.hip): the fp8
// conversions, round_half_even(y / scale) with its reciprocal shortcut, the clamp-and-pack of one vector of quantised values,
// and the skeleton of the per-token ("row") quantisers with the launch form that goes with it.
//
// The row skeleton: a row per TPR threads (256: a workgroup; 64: a wave), the first CACHE vectors per thread of the row's fp32
// y in registers, the rest recomputed.  A kernel supplies `produce(v, f)`, which writes y of vector v (v < n_vec) into
// f[VEC], and gets
//   row_absmax    the cached slots filled — `fill(v, y[c], live)` at the clamped index v = min(tid + c * TPR, n_vec - 1): no
//                 branch around the loads, so they go out together (a branch per vector made hipcc wait for each before
//                 requesting the next: one 16-byte load in flight per lane); the slots past the row (`live` false) hold
//                 duplicates that nothing below reads — and the row maximum of |y| over the live slots and the re-read tail,
//                 reduced over the TPR threads
//   row_quantise  scale = max(amax, 1e-12) / q_max (1.0 where that is < 1e-6, if asked), written by thread 0, and the
//                 quantised row: cache, then tail
// and row_quant, the two in a row with fill = produce, for a kernel whose cache nothing else reads.  The two norm kernels fill
// the cache themselves from SummedRow, the `hidden (+ residual) rounded to T` row, take their statistics from it, and pass
// the step that finishes y in place as `fill`.
#pragma once
#include <math.h>

#include <initializer_list>

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
// fallback decided once per VECTOR (a divergent branch per element costs more vector instructions than the arithmetic it
// guards): |t - rint(t)| <= 0.5 always, so "within 1e-3 of a rounding boundary" is "its maximum over the vector > 0.499".
// The int8 / fp8 choice is made once per vector too (quant_byte with a constant format folds to one conversion; with the
// run-time one it is a select per element, ~13 instructions a vector).
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
  if (fp8) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) q[j] = quant_byte(rq[j], q_min, q_max, 1);
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) q[j] = quant_byte(rq[j], q_min, q_max, 0);
  }
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

// one vector of activations, by the cache policy of the launch form
template <typename T, int VEC, bool NT>
__device__ __forceinline__ typename vec_of<T, VEC>::type load_vec_as(const T* p) {
  if constexpr (NT) return load_vec_nt<T, VEC>(p); else return load_vec<T, VEC>(p);
}
template <typename T, int VEC, bool NT>
__device__ __forceinline__ void store_vec_as(T* p, typename vec_of<T, VEC>::type v) {
  if constexpr (NT) store_vec_nt<T, VEC>(p, v); else store_vec<T, VEC>(p, v);
}

// ---- the row skeleton (the header comment) ----------------------------------------------------------------------------------
// The thread's place in its row behind an empty asm, for a kernel to take INSIDE its loop of rows when it chooses to.  The
// per-slot offsets that follow from the place are invariant over that loop; left visible hipcc computes them all once and holds
// them across it as 64-bit pairs (dequant_swiglu_quant_kernel on fp32: 74 of 193 VGPRs); taken anew per row they cost a few
// VALU instructions a row instead.  norm_quant.hip and quant_moe.hip say why they take it; dequant_swiglu_quant.hip does not.
template <int TPR>
__device__ __forceinline__ int row_thread_per_row() {
  int t = TPR == 256 ? threadIdx.x : threadIdx.x % TPR;
  asm volatile("" : "+v"(t));
  return t;
}

// `tid`: the thread's place in its row; `red`: 4 floats of LDS (TPR == 256; a wave's maximum needs none, and no barrier).
// CLAMPED: the slots past the row are filled too, at the clamped index (the header comment); otherwise there is a branch around
// each slot's fill, which costs the batching of the loads and saves the fetch and the arithmetic of the dead slots.
template <int VEC, int CACHE, int TPR, bool CLAMPED = true, typename Fill, typename Produce>
__device__ __forceinline__ float row_absmax(float (&y)[CACHE][VEC], int tid, int n_vec, Fill&& fill, Produce&& produce, float* red) {
  __builtin_assume(n_vec > 0);
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < CACHE; ++c) {
    const bool live = tid + c * TPR < n_vec;
    if (CLAMPED || live) fill(min(tid + c * TPR, n_vec - 1), y[c], live);
    if (live) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) amax = fmaxf(amax, fabsf(y[c][j]));
    }
  }
  for (int v = tid + CACHE * TPR; v < n_vec; v += TPR) {
    float f[VEC];
    produce(v, f);
#pragma unroll
    for (int j = 0; j < VEC; ++j) amax = fmaxf(amax, fabsf(f[j]));
  }
  if constexpr (TPR == 256) {
    return block_max256(amax, red);
  } else {
    static_assert(TPR == 64, "a row per workgroup or per wave");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    return amax;
  }
}

// `tiny_scale_is_one`: MojoDynamicQuant's and MojoMoEDynamicQuant's `where(scale < 1e-6, 1.0, scale)`
template <int VEC, int CACHE, int TPR, bool NT, typename Produce>
__device__ __forceinline__ void row_quantise(unsigned char* q_row, float* out_scale, const float (&y)[CACHE][VEC], int tid,
                                             int n_vec, Produce&& produce, float amax, float q_min, float q_max, int fp8,
                                             int tiny_scale_is_one) {
  __builtin_assume(n_vec > 0);
  float scale = __fdiv_rn(fmaxf(amax, 1e-12f), q_max);
  if (tiny_scale_is_one && scale < 1e-6f) scale = 1.0f;
  if (tid == 0) *out_scale = scale;
  const float inv_scale = __fdiv_rn(1.0f, scale);
  unsigned char* dst = q_row + tid * VEC;
#pragma unroll
  for (int c = 0; c < CACHE; ++c, dst += TPR * VEC) {
    if (tid + c * TPR < n_vec) quantise_store<VEC, NT>(dst, y[c], scale, inv_scale, q_min, q_max, fp8);
  }
  for (int v = tid + CACHE * TPR; v < n_vec; v += TPR) {
    float f[VEC];
    produce(v, f);
    quantise_store<VEC, NT>(q_row + v * VEC, f, scale, inv_scale, q_min, q_max, fp8);
  }
}

template <int VEC, int CACHE, int TPR, bool NT, bool CLAMPED = true, typename Produce>
__device__ __forceinline__ void row_quant(unsigned char* q_row, float* out_scale, int tid, int n_vec, Produce&& produce,
                                          float q_min, float q_max, int fp8, int tiny_scale_is_one, float* red) {
  float y[CACHE][VEC];
  const float amax = row_absmax<VEC, CACHE, TPR, CLAMPED>(y, tid, n_vec, [&](int v, float (&f)[VEC], bool) { produce(v, f); }, produce, red);
  row_quantise<VEC, CACHE, TPR, NT>(q_row, out_scale, y, tid, n_vec, produce, amax, q_min, q_max, fp8, tiny_scale_is_one);
}

// x = hidden (+ residual, the sum rounded to T) of one row, and out_sum, which receives x where it is not nullptr.
template <typename T, int VEC, bool NT>
struct SummedRow {
  typedef typename vec_of<T, VEC>::type V;
  const T* hidden;
  const T* residual;         // or nullptr
  T* out_sum;                // or nullptr
  int64_t base;              // element offset of the row

  __device__ __forceinline__ V at(const T* p, int v) const { return load_vec_as<T, VEC, NT>(p + base + v * VEC); }
  static __device__ __forceinline__ void add(V& x, const V& r) {
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      vset<T, VEC>(x, j, elt<T>::from_f(elt<T>::to_f(vget<T, VEC>(x, j)) + elt<T>::to_f(vget<T, VEC>(r, j))));
  }
  // x of vector v as floats; `store`: the pass that owns out_sum
  __device__ __forceinline__ void load(int v, float (&f)[VEC], bool store = false) const {
    V x = at(hidden, v);
    if (residual) add(x, at(residual, v));
    if (store && out_sum) store_vec_as<T, VEC, NT>(out_sum + base + v * VEC, x);
#pragma unroll
    for (int j = 0; j < VEC; ++j) f[j] = elt<T>::to_f(vget<T, VEC>(x, j));
  }
  // The cached slots, out_sum stored: batched loads at the clamped index — all of hidden, then (one wave-uniform branch) all
  // of residual.  The slots past the row come out as zeros, so sums over the whole cache are sums over the row.
  template <int CACHE, int TPR>
  __device__ __forceinline__ void fill(float (&y)[CACHE][VEC], int tid, int n_vec) const {
    __builtin_assume(n_vec > 0);
    V xr[CACHE];
#pragma unroll
    for (int c = 0; c < CACHE; ++c) xr[c] = at(hidden, min(tid + c * TPR, n_vec - 1));
    if (residual) {
      V rr[CACHE];
#pragma unroll
      for (int c = 0; c < CACHE; ++c) rr[c] = at(residual, min(tid + c * TPR, n_vec - 1));
#pragma unroll
      for (int c = 0; c < CACHE; ++c) add(xr[c], rr[c]);
    }
    if (out_sum) {
#pragma unroll
      for (int c = 0; c < CACHE; ++c)
        if (tid + c * TPR < n_vec) store_vec_as<T, VEC, NT>(out_sum + base + (tid + c * TPR) * VEC, xr[c]);
    }
#pragma unroll
    for (int c = 0; c < CACHE; ++c) {
      const bool live = tid + c * TPR < n_vec;
#pragma unroll
      for (int j = 0; j < VEC; ++j) y[c][j] = live ? elt<T>::to_f(vget<T, VEC>(xr[c], j)) : 0.f;
    }
  }
};

// ---- the launch form of a row quantiser ---------------------------------------------------------------------------------------
struct AlignedPtr { const void* p; size_t align; };          // (nullptr, an optional tensor that is absent, passes)

struct RowLaunch {
  bool wide, nt;             // 16-byte vectors; non-temporal loads and stores (wide forms only: the scalar one has no twin)
  unsigned blocks;
  const char *width, *policy, *fit;        // the pieces of the launch tag: wide|scalar, nt|cached, resident|reread
};

// `wide_vec`: elements of a 16-byte vector; `moved`: the bytes the op reads and writes once (0: an op with no non-temporal
// form); `cached_wide` / `cached_scalar`: the vectors of a row that the two forms keep in registers.
inline RowLaunch row_launch(std::initializer_list<AlignedPtr> tensors, int64_t rows, int dim, int wide_vec, long long moved,
                            int cached_wide, int cached_scalar) {
  RowLaunch f;
  f.wide = dim % wide_vec == 0;
  for (const AlignedPtr& t : tensors) f.wide = f.wide && aligned_to(t.p, t.align);
  f.nt = f.wide && moved > 0 && stream_nt(moved);
  f.blocks = static_cast<unsigned>(rows > 256 * 32 ? 256 * 32 : rows);
  f.width = f.wide ? "wide" : "scalar";
  f.policy = f.nt ? "nt" : "cached";
  f.fit = (f.wide ? dim / wide_vec <= cached_wide : dim <= cached_scalar) ? "resident" : "reread";
  return f;
}

}  // namespace mojo
