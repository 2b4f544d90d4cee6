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
// or past sum(counts) produce int8 zeros and scale 1.  The kernel is the row skeleton of quant_common.h around `load_y`: one row
// per 256-thread workgroup at a time, 16-byte loads, the row's y values in registers between the maximum and the quantisation
// (rows of up to 4 x 256 vectors; longer rows recompute), round_half_even(y / scale) by the reciprocal shortcut with its
// exact-division fallback.  The products are single IEEE operations and the rounded quotient equals the division's: with
// x.float() * inv_smooth the bytes equal the golden's.  The glu form's exp is the device library's, so its y can differ from a
// CPU silu in the last place (tests/test_hip_quant_moe.py).
//
// Algorithmic bytes per output element: elt + 1 (glu: 2 * elt + 1), + 4 for the smooth scale (L2-resident per expert).
#include <math.h>

#include "common.h"
#include "moe_row_expert.h"
#include "quant_common.h"

namespace mojo {

template <typename T, int VEC, bool GLU>
__global__ __launch_bounds__(256) void moe_quant_kernel(const T* __restrict__ x, const float* __restrict__ smooth,
                                                        const void* __restrict__ counts, int counts_i64, int E,
                                                        int8_t* __restrict__ out_q, float* __restrict__ out_scale, int64_t rows,
                                                        int dim) {
  constexpr int CACHE = 4;
  __shared__ long long s_start[MOE_QUANT_MAX_EXPERTS + 1];
  __shared__ float red[4];
  moe_scan_counts(counts, counts_i64, E, rows, s_start);           // (moe_row_expert.h)
  const int64_t live = s_start[E];
  const int n_vec = dim / VEC;
  const int64_t in_ld = GLU ? 2 * static_cast<int64_t>(dim) : dim;
  typedef typename vec_of<T, VEC>::type VT;
  typedef typename vec_of<float, VEC>::type VF;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    unsigned char* q_row = reinterpret_cast<unsigned char*>(out_q) + row * dim;
    if (row >= live) {
      moe_zero_unowned_row<VEC>(q_row, out_scale + row, n_vec);
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
    // Not CLAMPED: a branch around each cached slot, as this kernel has always had.  At the widths the experts have (4096
    // columns of 16-bit input: 512 vectors) half of the four slots lie past the row, and fetching and scaling the last vector
    // again for them measured 2 % slower (8192 x 4096 bf16: 32.8 us against 32.1) than not batching the loads of the other two.
    // The place in the row per row: with the offsets held across rows the 16-bit scalar glu form needs 104-106 SGPRs and
    // loses a wave per SIMD (7 for 8).
    row_quant<VEC, CACHE, 256, false, /* CLAMPED */ false>(q_row, out_scale + row, row_thread_per_row<256>(), n_vec, load_y, -128.f,
                                                           127.f, 0, 1, red);
  }
}

template <typename T>
static int launch_moe_quant(const void* input, const float* smooth, const void* counts, int counts_i64, int experts, void* out_q,
                            float* out_scale, int64_t rows, int dim, int glu, hipStream_t s) {
  constexpr int WIDE = 16 / sizeof(T);
  const RowLaunch f = row_launch({{input, 16}, {smooth, 16}, {out_q, WIDE}}, rows, dim, WIDE, 0, 4 * 256, 4 * 256);
  const T* x = static_cast<const T*>(input);
  int8_t* q = static_cast<int8_t*>(out_q);
#define MOE_QUANT(VEC_, GLU_) hipLaunchKernelGGL((moe_quant_kernel<T, VEC_, GLU_>), dim3(f.blocks), dim3(256), 0, s, x, smooth, counts, counts_i64, experts, q, out_scale, rows, dim)
  if (glu) { if (f.wide) MOE_QUANT(WIDE, true); else MOE_QUANT(1, true); }
  else { if (f.wide) MOE_QUANT(WIDE, false); else MOE_QUANT(1, false); }
#undef MOE_QUANT
  MOJO_CHECK_LAUNCH("moe_dynamic_quant");
  note_launch("moe_quant:%s:%s", glu ? "swiglu" : "plain", f.wide ? "vec16" : "scalar");
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
