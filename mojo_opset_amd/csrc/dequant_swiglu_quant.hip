// MojoDequantSwiGLUQuant (mojo_opset/core/operators/quantize.py:250-354): the stage between fc1 and fc2 of a W8A8 MLP in one
// pass — the GEMM's accumulators are dequantised, activated, smoothed and quantised again without the fp32 [T, 2H] activation
// ever reaching memory.  Per row t of expert e, in the golden's order, every step one IEEE single operation:
//   y     = float(x[t, :]) * weight_scale[e, :]          x int32 (v_cvt_f32_i32: round to nearest even, as int32.float()),
//                                                        fp32, fp16 or bf16
//   y     = y * activation_scale[t]                      (optional)
//   y     = y + bias[:] or bias[e, :]                    (optional)
//   z     = silu(right) * left   (activate_left: silu(left) * right),   left = y[:H], right = y[H:],
//           silu(g) = g / (1 + expf(-g))                 moe_quant_kernel's form; expf is the device library's
//   z     = z * quant_scale[e, :]
//   scale = max(amax|z|, 1e-12) / 127                    (no "1.0 where tiny" here, unlike MojoDynamicQuant)
//   q     = clamp(round_half_even(z / scale), -128, 127)
//
// The expert of a row comes from token_count on the device (moe_row_expert.h, shared with moe_quant_kernel); rows at or past
// sum(token_count) give int8 zeros and scale 1; token_count == nullptr: one expert owns every row.  One row per 256-thread
// workgroup at a time, 16-byte loads of x and of the three per-column vectors, and the row's z stays in registers between the
// maximum and the quantisation: 56 floats per thread, 14336 columns, in both element widths (an int32 / fp32 row is twice as
// wide per output as a 16-bit one, so its vectors hold 4 outputs where those hold 8 and it caches twice as many of them).
// Longer rows recompute what does not fit.
//
// Algorithmic bytes per output element: 2 * elt + 1 (+ 12 of scales per column, cache-resident per expert).
#include <math.h>

#include "common.h"
#include "moe_row_expert.h"
#include "quant_common.h"

namespace mojo {

struct DequantSwigluQuantArgs {
  const void* x;                // [rows, 2H] T
  const float* weight_scale;    // [E, 2H]
  const float* act_scale;       // [rows] or nullptr
  const float* bias;            // [2H] or [E, 2H] or nullptr
  const float* quant_scale;     // [E, H]
  const void* counts;           // [E] int32 / int64 or nullptr
  int8_t* out_q;                // [rows, H]
  float* out_scale;             // [rows]
  int64_t rows;
  int hidden;                   // H
  int experts;
  int counts_i64, bias_grouped, activate_left;
};

template <typename T> struct acc_elt { static __device__ __forceinline__ float to_f(T v) { return elt<T>::to_f(v); } };
template <> struct acc_elt<int32_t> { static __device__ __forceinline__ float to_f(int32_t v) { return static_cast<float>(v); } };

// The 16-bit wide forms are held to 168 VGPRs (three workgroups per CU instead of two) and take 159; the 32-bit ones, whose
// loads are twice as many per output, take 153 uncapped.  The thread's place in the row is the plain threadIdx.x: hidden per
// row (row_thread_per_row) the forms need 131 and 119 VGPRs, and the 16-bit one, whose cap fixes its occupancy either way,
// measured 1-2 % slower for the offsets it recomputes (8192 x 14336 bf16, 8 groups: 181.2 us against 178.9).
template <typename T, int VEC, int CACHE, bool NT>
__global__ __launch_bounds__(256, (VEC > 1 && sizeof(T) == 2) ? 3 : 1) void dequant_swiglu_quant_kernel(DequantSwigluQuantArgs a) {
  typedef typename vec_of<T, VEC>::type VT;
  __shared__ long long s_start[MOE_QUANT_MAX_EXPERTS + 1];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int H = a.hidden;
  int64_t live = a.rows;
  if (a.counts) {
    moe_scan_counts(a.counts, a.counts_i64, a.experts, a.rows, s_start);
    live = s_start[a.experts];
  }
  const int n_vec = H / VEC;
  const T* x = static_cast<const T*>(a.x);
  for (int64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
    unsigned char* q_row = reinterpret_cast<unsigned char*>(a.out_q) + row * H;
    if (row >= live) {
      moe_zero_unowned_row<VEC>(q_row, a.out_scale + row, n_vec);
      continue;
    }
    const int e = a.counts ? moe_expert_of_row(s_start, a.experts, row) : 0;
    const T* x_row = x + row * 2 * static_cast<int64_t>(H);
    const float* ws = a.weight_scale + static_cast<int64_t>(e) * 2 * H;
    const float* qs = a.quant_scale + static_cast<int64_t>(e) * H;
    const float* bs = a.bias ? a.bias + (a.bias_grouped ? static_cast<int64_t>(e) * 2 * H : 0) : nullptr;
    const bool has_act = a.act_scale != nullptr;
    const float act = has_act ? a.act_scale[row] : 1.0f;
    const bool left_gate = a.activate_left != 0;
    auto load_z = [&](int v, float (&f)[VEC]) {                // z of vector v (v < n_vec)
      const VT l = load_vec_as<T, VEC, NT>(x_row + v * VEC), r = load_vec_as<T, VEC, NT>(x_row + H + v * VEC);
      float wl[VEC], wr[VEC], sq[VEC];
      load_f32_vec<VEC>(ws, v, wl);
      load_f32_vec<VEC>(ws + H, v, wr);
      load_f32_vec<VEC>(qs, v, sq);
      float yl[VEC], yr[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        yl[j] = __fmul_rn(acc_elt<T>::to_f(vget<T, VEC>(l, j)), wl[j]);
        yr[j] = __fmul_rn(acc_elt<T>::to_f(vget<T, VEC>(r, j)), wr[j]);
      }
      if (has_act) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) { yl[j] = __fmul_rn(yl[j], act); yr[j] = __fmul_rn(yr[j], act); }
      }
      if (bs) {
        float bl[VEC], br[VEC];
        load_f32_vec<VEC>(bs, v, bl);
        load_f32_vec<VEC>(bs + H, v, br);
#pragma unroll
        for (int j = 0; j < VEC; ++j) { yl[j] = __fadd_rn(yl[j], bl[j]); yr[j] = __fadd_rn(yr[j], br[j]); }
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float g = left_gate ? yl[j] : yr[j], u = left_gate ? yr[j] : yl[j];
        const float s = __fdiv_rn(g, __fadd_rn(1.0f, expf(-g)));
        f[j] = __fmul_rn(__fmul_rn(s, u), sq[j]);
      }
    };
    row_quant<VEC, CACHE, 256, NT>(q_row, a.out_scale + row, tid, n_vec, load_z, -128.f, 127.f, 0, 0, red);
  }
}

template <typename T>
static int launch_dequant_swiglu_quant(const DequantSwigluQuantArgs& a, hipStream_t s) {
  constexpr int WIDE = 16 / sizeof(T);                       // outputs per 16-byte vector of x
  constexpr int RESIDENT = 56;                               // floats of z a thread keeps
  const int H = a.hidden;
  const long long moved = a.rows * static_cast<long long>(H) * (2 * static_cast<long long>(sizeof(T)) + 1);
  const RowLaunch f = row_launch({{a.x, 16}, {a.weight_scale, 16}, {a.quant_scale, 16}, {a.bias, 16}, {a.out_q, WIDE}}, a.rows, H, WIDE,
                                 moved, RESIDENT / WIDE * 256, 16 * 256);
  if (f.nt) hipLaunchKernelGGL((dequant_swiglu_quant_kernel<T, WIDE, RESIDENT / WIDE, true>), dim3(f.blocks), dim3(256), 0, s, a);
  else if (f.wide) hipLaunchKernelGGL((dequant_swiglu_quant_kernel<T, WIDE, RESIDENT / WIDE, false>), dim3(f.blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((dequant_swiglu_quant_kernel<T, 1, 16, false>), dim3(f.blocks), dim3(256), 0, s, a);
  MOJO_CHECK_LAUNCH("dequant_swiglu_quant");
  note_launch("dequant_swiglu_quant:%s:%s:%s", f.width, f.fit, f.policy);
  return MOJO_OK;
}

}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_dequant_swiglu_quant(const void* x, const float* weight_scale, const float* activation_scale,
                                             const float* bias, int bias_is_grouped, const float* quant_scale,
                                             const void* token_count, int token_count_is_i64, void* out_q, float* out_scale,
                                             int64_t rows, int64_t hidden, int64_t num_experts, int activate_left, int dtype,
                                             mojo_stream_t stream) {
  if (rows == 0) return MOJO_OK;
  MOJO_REQUIRE(x && weight_scale && quant_scale && out_q && out_scale, MOJO_EINVAL, "dequant_swiglu_quant: null pointer");
  MOJO_REQUIRE(rows > 0 && hidden > 0 && hidden < (1LL << 29) && num_experts > 0, MOJO_EINVAL,
               "dequant_swiglu_quant: bad shape rows=%lld hidden=%lld experts=%lld", (long long)rows, (long long)hidden, (long long)num_experts);
  MOJO_REQUIRE(num_experts <= MOE_QUANT_MAX_EXPERTS, MOJO_EUNSUPPORTED, "dequant_swiglu_quant: more than %d experts", MOE_QUANT_MAX_EXPERTS);
  MOJO_REQUIRE(token_count || num_experts == 1, MOJO_EINVAL, "dequant_swiglu_quant: %lld experts need token_count", (long long)num_experts);
  DequantSwigluQuantArgs a{};
  a.x = x; a.weight_scale = weight_scale; a.act_scale = activation_scale; a.bias = bias; a.quant_scale = quant_scale;
  a.counts = token_count; a.out_q = static_cast<int8_t*>(out_q); a.out_scale = out_scale;
  a.rows = rows; a.hidden = static_cast<int>(hidden); a.experts = static_cast<int>(num_experts);
  a.counts_i64 = token_count_is_i64; a.bias_grouped = bias_is_grouped; a.activate_left = activate_left;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MOJO_I32: return launch_dequant_swiglu_quant<int32_t>(a, s);
    case MOJO_F32: return launch_dequant_swiglu_quant<float>(a, s);
    case MOJO_F16: return launch_dequant_swiglu_quant<f16_t>(a, s);
    case MOJO_BF16: return launch_dequant_swiglu_quant<bf16_t>(a, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "dequant_swiglu_quant: dtype %d not supported", dtype);
  }
}
