// The two per-token quantisers of MojoQuantExperts (mojo_hip_moe_dynamic_quant):
//   MojoMoEDynamicQuant   mojo_opset/core/operators/quantize.py:178-247
//     y = x.float() * inv_smooth_scale[expert of the row]
//   the stage between the experts' two projections (core/operators/moe.py:452-667), glu = 1
//     y = silu(float(gate)) * float(up) * inv_smooth_scale[expert of the row]     (fc1 = [gate | up], gate FIRST; fp32 throughout:
//     the fp32 [M, I] activation the golden materialises lives in registers only)
//   scale = max(amax_row |y|, 1e-12) / 127, 1.0 where that is < 1e-6;   q = clamp(round_half_even(y / scale), -128, 127)
//
// The rows arrive sorted by expert; the expert of a row comes from the row counts ON THE DEVICE: every workgroup scans the
// counts into LDS (one wave, 64 counts per step) and searches it per row — no prefix launch, no host synchronisation.  Rows at
// or past sum(counts) produce int8 zeros and scale 1.  One row per 256-thread workgroup at a time, 16-byte loads, the row's y
// values stay in registers between the maximum and the quantisation (rows of up to 4 x 256 vectors; longer rows recompute).
// Products and the division are the IEEE single operations: with x.float() * inv_smooth the bytes equal the golden's.  The
// glu form's exp is the device library's, so its y can differ from a CPU silu in the last place (tests/test_hip_quant_moe.py).
//
// Algorithmic bytes per output element: elt + 1 (glu: 2 * elt + 1), + 4 for the smooth scale (L2-resident per expert).
#include <math.h>

#include "common.h"
#include "moe_row_expert.h"

namespace mojo {

__device__ __forceinline__ float moe_quant_block_max(float x, float* smem) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) smem[wave] = x;
  __syncthreads();
  const float r = fmaxf(fmaxf(smem[0], smem[1]), fmaxf(smem[2], smem[3]));
  __syncthreads();
  return r;
}

template <typename T, int VEC, bool GLU>
__global__ __launch_bounds__(256) void moe_quant_kernel(const T* __restrict__ x, const float* __restrict__ smooth,
                                                        const void* __restrict__ counts, int counts_i64, int E,
                                                        int8_t* __restrict__ out_q, float* __restrict__ out_scale, int64_t rows,
                                                        int dim) {
  constexpr int CACHE = 4;
  __shared__ long long s_start[MOE_QUANT_MAX_EXPERTS + 1];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  moe_scan_counts(counts, counts_i64, E, rows, s_start);           // (moe_row_expert.h)
  const int64_t live = s_start[E];
  const int n_vec = dim / VEC;
  const int64_t in_ld = GLU ? 2 * static_cast<int64_t>(dim) : dim;
  typedef typename vec_of<T, VEC>::type VT;
  typedef typename vec_of<float, VEC>::type VF;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    int8_t* q_row = out_q + row * dim;
    if (row >= live) {                                       // no expert owns the row
      for (int v = tid; v < n_vec; v += 256) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) q_row[v * VEC + j] = 0;
      }
      if (tid == 0) out_scale[row] = 1.0f;
      continue;
    }
    const int lo = moe_expert_of_row(s_start, E, row);       // largest e with s_start[e] <= row
    const T* x_row = x + row * in_ld;
    const float* sm_row = smooth + static_cast<int64_t>(lo) * dim;
    auto load_y = [&](int v, float (&f)[VEC]) {
      const VT a = *reinterpret_cast<const VT*>(x_row + v * VEC);
      const VF s = *reinterpret_cast<const VF*>(sm_row + v * VEC);
      if constexpr (GLU) {
        const VT u = *reinterpret_cast<const VT*>(x_row + dim + v * VEC);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float g = elt<T>::to_f(vget<T, VEC>(a, j));
          const float act = __fdiv_rn(g, 1.0f + expf(-g));
          f[j] = __fmul_rn(__fmul_rn(act, elt<T>::to_f(vget<T, VEC>(u, j))), vget<float, VEC>(s, j));
        }
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) f[j] = __fmul_rn(elt<T>::to_f(vget<T, VEC>(a, j)), vget<float, VEC>(s, j));
      }
    };
    float y[CACHE][VEC];
    float amax = 0.f;
#pragma unroll
    for (int c = 0; c < CACHE; ++c) {
      const int v = tid + c * 256;
      if (v < n_vec) {
        load_y(v, y[c]);
#pragma unroll
        for (int j = 0; j < VEC; ++j) amax = fmaxf(amax, fabsf(y[c][j]));
      }
    }
    for (int v = tid + CACHE * 256; v < n_vec; v += 256) {
      float f[VEC];
      load_y(v, f);
#pragma unroll
      for (int j = 0; j < VEC; ++j) amax = fmaxf(amax, fabsf(f[j]));
    }
    amax = moe_quant_block_max(amax, red);
    float scale = __fdiv_rn(fmaxf(amax, 1e-12f), 127.f);
    if (scale < 1e-6f) scale = 1.0f;
    if (tid == 0) out_scale[row] = scale;
    auto emit = [&](int v, const float (&f)[VEC]) {
      unsigned char q[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float r = rintf(__fdiv_rn(f[j], scale));
        q[j] = static_cast<unsigned char>(static_cast<signed char>(static_cast<int>(fminf(fmaxf(r, -128.f), 127.f))));
      }
      int8_t* dst = q_row + v * VEC;
      if constexpr (VEC == 8) {
        u32x2 w;
        w[0] = q[0] | (q[1] << 8) | (q[2] << 16) | (static_cast<unsigned>(q[3]) << 24);
        w[1] = q[4] | (q[5] << 8) | (q[6] << 16) | (static_cast<unsigned>(q[7]) << 24);
        *reinterpret_cast<u32x2*>(dst) = w;
      } else if constexpr (VEC == 4) {
        *reinterpret_cast<unsigned*>(dst) = q[0] | (q[1] << 8) | (q[2] << 16) | (static_cast<unsigned>(q[3]) << 24);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) dst[j] = static_cast<int8_t>(q[j]);
      }
    };
#pragma unroll
    for (int c = 0; c < CACHE; ++c) {
      const int v = tid + c * 256;
      if (v < n_vec) emit(v, y[c]);
    }
    for (int v = tid + CACHE * 256; v < n_vec; v += 256) {
      float f[VEC];
      load_y(v, f);
      emit(v, f);
    }
  }
}

template <typename T>
static int launch_moe_quant(const void* input, const float* smooth, const void* counts, int counts_i64, int experts, void* out_q,
                            float* out_scale, int64_t rows, int dim, int glu, hipStream_t s) {
  constexpr int WIDE = 16 / sizeof(T);
  const bool wide = dim % WIDE == 0 && aligned_to(input, 16) && aligned_to(smooth, 16) && aligned_to(out_q, WIDE);
  const unsigned blocks = static_cast<unsigned>(rows > 256 * 32 ? 256 * 32 : rows);
  const T* x = static_cast<const T*>(input);
  int8_t* q = static_cast<int8_t*>(out_q);
#define MOE_QUANT(VEC_, GLU_) hipLaunchKernelGGL((moe_quant_kernel<T, VEC_, GLU_>), dim3(blocks), dim3(256), 0, s, x, smooth, counts, counts_i64, experts, q, out_scale, rows, dim)
  if (glu) { if (wide) MOE_QUANT(WIDE, true); else MOE_QUANT(1, true); }
  else { if (wide) MOE_QUANT(WIDE, false); else MOE_QUANT(1, false); }
#undef MOE_QUANT
  MOJO_CHECK_LAUNCH("moe_dynamic_quant");
  note_launch("moe_quant:%s:%s", glu ? "swiglu" : "plain", wide ? "vec16" : "scalar");
  return MOJO_OK;
}

}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_moe_dynamic_quant(const void* input, const float* inv_smooth_scale, const void* token_count,
                                          int token_count_is_i64, void* out_q, float* out_scale, int64_t rows, int64_t dim,
                                          int64_t num_experts, int glu, int dtype, mojo_stream_t stream) {
  if (rows == 0) return MOJO_OK;
  MOJO_REQUIRE(input && inv_smooth_scale && token_count && out_q && out_scale, MOJO_EINVAL, "moe_dynamic_quant: null pointer");
  MOJO_REQUIRE(rows > 0 && dim > 0 && dim < (1LL << 30) && num_experts > 0, MOJO_EINVAL,
               "moe_dynamic_quant: bad shape rows=%lld dim=%lld experts=%lld", (long long)rows, (long long)dim, (long long)num_experts);
  MOJO_REQUIRE(num_experts <= MOE_QUANT_MAX_EXPERTS, MOJO_EUNSUPPORTED, "moe_dynamic_quant: more than %d experts", MOE_QUANT_MAX_EXPERTS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int e = static_cast<int>(num_experts), d = static_cast<int>(dim);
  switch (dtype) {
    case MOJO_F32: return launch_moe_quant<float>(input, inv_smooth_scale, token_count, token_count_is_i64, e, out_q, out_scale, rows, d, glu, s);
    case MOJO_F16: return launch_moe_quant<f16_t>(input, inv_smooth_scale, token_count, token_count_is_i64, e, out_q, out_scale, rows, d, glu, s);
    case MOJO_BF16: return launch_moe_quant<bf16_t>(input, inv_smooth_scale, token_count, token_count_is_i64, e, out_q, out_scale, rows, d, glu, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "moe_dynamic_quant: dtype %d not supported", dtype);
  }
}
