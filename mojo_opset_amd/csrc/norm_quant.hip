// Per-token activation quantisers that feed MojoQuantGemm:
//   MojoDynamicQuant            mojo_opset/core/operators/quantize.py:153-169
//   MojoResidualAddRMSNormQuant mojo_opset/core/operators/normalization.py:493-526
//
//   y     = x.float() [* inv_smooth]                                   (dynamic quant)
//   y     = rms_norm((h + r rounded to T).float(), w, eps) [* smooth]  (norm + quant; fp32 all the way, never rounded to T)
//   scale = max(amax_row |y|, 1e-12) / q_max        (dynamic quant only: 1.0 where that is < 1e-6)
//   q     = clamp(round_half_even(y / scale), q_min, q_max)  -> int8, or float8_e4m3fn of that INTEGER value
//
// One row per 256-thread block; the row's y values stay in registers between the two reductions (sum of squares, row
// maximum) and the quantisation, so every input byte is read once.  Products and the division are the IEEE single
// operations (no FMA contraction, no reciprocal): with the same row statistics the quantised bytes equal the golden's.
//
// Algorithmic bytes per element: dynamic quant elt + 1; norm+quant (pre) 3*elt + 1 (+ weight, smooth once).
//
// MojoRMSNormQuant (normalization.py:136-213) is the norm+quant arithmetic with no residual and no sum output: the same kernel
// with residual == nullptr, behind an entry point of its own (mojo_hip_rmsnorm_quant) whose launch tags say `rmsnorm_quant`.
//
// MojoLayerNormQuant / MojoResidualAddLayerNormQuant (normalization.py:216-305, :536-646): layernorm_quant_kernel, the centred
// form of the same design.  Three reductions over the register-resident row: the sum (mean), the sum of squared deviations
// from that mean (biased variance; not E[x^2] - mean^2, which cancels), the row maximum.  rstd = 1 / sqrt(var + eps) with the
// IEEE division and square root.  The elementwise form: torch's CPU layer_norm, fed the statistics it reports itself
// (native_layer_norm), is reproduced bit for bit by
//     y = fma((x - mean) * rstd, w, b)          (affine)          y = (x - mean) * rstd          (no affine)
// on every element of 64 rows of 128, 257, 1000, 4096 and 20000 columns; with a separately rounded `* w` then `+ b` 23 % of the
// elements differ in the last place, and the scaled form (x * rstd + (-mean * rstd)) * w + b misses about a third with and
// without the affine pair.  So the last multiply-add is ONE fused operation here, on purpose, and the only one.  The
// statistics themselves differ from torch's in summation order (last place of mean and rstd), which is what the test bound
// of one quantisation step on at most 2e-3 of the elements covers.
#include <math.h>

#include "common.h"
#include "quant_common.h"

namespace mojo {

struct NormQuantArgs {
  const void* hidden;        // [rows, dim] T
  const void* residual;      // [rows, dim] T or nullptr
  const float* weight;       // [dim] fp32 or nullptr (no normalisation: dynamic quant)
  const float* smooth;       // [dim] fp32 or nullptr
  void* out_q;               // [rows, dim] int8 / fp8
  void* out_sum;             // [rows, dim] T or nullptr      (norm_pos = pre: hidden + residual)
  float* out_normed;         // [rows, dim] fp32 or nullptr   (norm_pos = post: the normed tensor before smoothing)
  float* out_scale;          // [rows]
  int64_t rows;
  int dim;
  float eps, q_max, q_min;
  int fp8;                   // 0: int8, 1: float8_e4m3fn
  int tiny_scale_is_one;     // MojoDynamicQuant's `where(scale < 1e-6, 1.0, scale)`
};

// TPR = threads per row: 256 (a row per workgroup) or 64 (a row per WAVE, four rows per workgroup, no LDS and no barrier:
// dynamic quant only — the row maximum is exact in any order, a sum of squares is not).  Many short rows on a workgroup each
// cost ~2 ns of workgroup turnover per row (32 768 rows x 2048: 70 us for 200 MB; x 128: 54 us for 13 MB).
template <typename T, int VEC, int CACHE, bool NT = false /* stream_nt(): activations by-pass the caches */, int TPR = 256>
__global__ __launch_bounds__(256) void norm_quant_kernel(NormQuantArgs a) {
  __shared__ float red[4];
  const int n_vec = a.dim / VEC;
  constexpr int RPB = 256 / TPR;                     // rows per workgroup at a time
  unsigned char* out_q = static_cast<unsigned char*>(a.out_q);

  for (int64_t row = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / TPR; row < a.rows; row += static_cast<int64_t>(gridDim.x) * RPB) {
    const int tid = row_thread_per_row<TPR>();       // (per row: the fp32 wide forms take 98-106 VGPRs with the offsets held, 5 -> 4 workgroups per CU)
    const SummedRow<T, VEC, NT> x{static_cast<const T*>(a.hidden), static_cast<const T*>(a.residual), static_cast<T*>(a.out_sum), row * a.dim};
    // ---- pass 1: the row into registers, its sum of squares -----------------------------------------------------------
    float y[CACHE][VEC];
    x.template fill<CACHE, TPR>(y, tid, n_vec);
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < CACHE; ++c)
#pragma unroll
      for (int j = 0; j < VEC; ++j) ss = fmaf(y[c][j], y[c][j], ss);
    for (int v = tid + CACHE * TPR; v < n_vec; v += TPR) {
      float f[VEC];
      x.load(v, f, true);
#pragma unroll
      for (int j = 0; j < VEC; ++j) ss = fmaf(f[j], f[j], ss);
    }
    float rstd = 1.f;
    if (a.weight) {
      ss = block_sum<4>(ss, red);
      __syncthreads();
      rstd = rsqrtf(ss / static_cast<float>(a.dim) + a.eps);
    }
    // ---- pass 2: y = ((x * rstd) * w) [* smooth], single IEEE multiplies in the golden's order; the row maximum ---------
    auto finish = [&](int v, float (&f)[VEC], bool store_normed) {
      if (a.weight) {
        float w[VEC];
        load_f32_vec<VEC>(a.weight, v, w);
#pragma unroll
        for (int j = 0; j < VEC; ++j) f[j] = __fmul_rn(__fmul_rn(f[j], rstd), w[j]);
        if (store_normed && a.out_normed) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) a.out_normed[x.base + v * VEC + j] = f[j];
        }
      }
      if (a.smooth) {
        float sm[VEC];
        load_f32_vec<VEC>(a.smooth, v, sm);
#pragma unroll
        for (int j = 0; j < VEC; ++j) f[j] = __fmul_rn(f[j], sm[j]);
      }
    };
    const float amax = row_absmax<VEC, CACHE, TPR>(y, tid, n_vec, finish, [&](int v, float (&f)[VEC]) { x.load(v, f); finish(v, f, true); }, red);
    // ---- pass 3: quantise (the tail's normed tensor was stored in pass 2) ---------------------------------------------
    row_quantise<VEC, CACHE, TPR, NT>(out_q + x.base, a.out_scale + row, y, tid, n_vec,
                                      [&](int v, float (&f)[VEC]) { x.load(v, f); finish(v, f, false); }, amax, a.q_min, a.q_max,
                                      a.fp8, a.tiny_scale_is_one);
  }
}

struct LayerNormQuantArgs {
  const void* hidden;        // [rows, dim] T
  const void* residual;      // [rows, dim] T or nullptr
  const float* weight;       // [dim] fp32, or nullptr together with bias (elementwise_affine = False)
  const float* bias;         // [dim] fp32 or nullptr
  const float* smooth;       // [dim] fp32 or nullptr
  void* out_q;               // [rows, dim] int8 / fp8
  void* out_sum;             // [rows, dim] T or nullptr: hidden + residual (both norm_pos)
  float* out_scale;          // [rows]
  int64_t rows;
  int dim;
  float eps, q_max, q_min;
  int fp8;
};

// LayerNorm + quant: a row per 256-thread workgroup, the row's (summed) x in registers from the first load to the quantised
// store; rows of more than CACHE * 256 vectors re-read (and re-add) what does not fit.  The wide forms are held to 128 VGPRs
// (four workgroups per CU).  With the thread's place in the row taken per row they need 60 (fp32) to 99 (bf16) and the cap
// does not bind; with the per-slot offsets held across the loop of rows they sit at the cap and spill 4 to 12 VGPRs, which
// is why this kernel takes the place per row.
template <typename T, int VEC, int CACHE, bool NT>
__global__ __launch_bounds__(256, VEC > 1 ? 4 : 1) void layernorm_quant_kernel(LayerNormQuantArgs a) {
  __shared__ float red[4];
  const int n_vec = a.dim / VEC;
  unsigned char* out_q = static_cast<unsigned char*>(a.out_q);
  const float dim_f = static_cast<float>(a.dim);

  for (int64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const int tid = row_thread_per_row<256>();               // (the comment above)
    const SummedRow<T, VEC, NT> x{static_cast<const T*>(a.hidden), static_cast<const T*>(a.residual), static_cast<T*>(a.out_sum), row * a.dim};
    // ---- pass 1: the row into registers, its sum ------------------------------------------------------------------------
    float y[CACHE][VEC];
    x.template fill<CACHE, 256>(y, tid, n_vec);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CACHE; ++c)
#pragma unroll
      for (int j = 0; j < VEC; ++j) sum += y[c][j];
    for (int v = tid + CACHE * 256; v < n_vec; v += 256) {
      float f[VEC];
      x.load(v, f, true);
#pragma unroll
      for (int j = 0; j < VEC; ++j) sum += f[j];
    }
    sum = block_sum<4>(sum, red);
    __syncthreads();
    const float mean = __fdiv_rn(sum, dim_f);
    // ---- pass 2: the sum of squared deviations -------------------------------------------------------------------------
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < CACHE; ++c) {
      if (tid + c * 256 < n_vec) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float d = __fsub_rn(y[c][j], mean);
          ss = fmaf(d, d, ss);
        }
      }
    }
    for (int v = tid + CACHE * 256; v < n_vec; v += 256) {
      float f[VEC];
      x.load(v, f);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float d = __fsub_rn(f[j], mean);
        ss = fmaf(d, d, ss);
      }
    }
    ss = block_sum<4>(ss, red);
    __syncthreads();
    const float rstd = __fdiv_rn(1.0f, sqrtf(__fadd_rn(__fdiv_rn(ss, dim_f), a.eps)));
    // ---- pass 3: y, row maximum; pass 4: quantise -------------------------------------------------------------------------
    auto finish = [&](int v, float (&f)[VEC]) {                // x -> y of vector v (v < n_vec)
#pragma unroll
      for (int j = 0; j < VEC; ++j) f[j] = __fmul_rn(__fsub_rn(f[j], mean), rstd);
      if (a.weight) {
        float w[VEC], b[VEC];
        load_f32_vec<VEC>(a.weight, v, w);
        load_f32_vec<VEC>(a.bias, v, b);
#pragma unroll
        for (int j = 0; j < VEC; ++j) f[j] = fmaf(f[j], w[j], b[j]);       // fused on purpose: the header comment
      }
      if (a.smooth) {
        float sm[VEC];
        load_f32_vec<VEC>(a.smooth, v, sm);
#pragma unroll
        for (int j = 0; j < VEC; ++j) f[j] = __fmul_rn(f[j], sm[j]);
      }
    };
    auto y_of = [&](int v, float (&f)[VEC]) { x.load(v, f); finish(v, f); };
    const float amax = row_absmax<VEC, CACHE, 256>(y, tid, n_vec, [&](int v, float (&f)[VEC], bool) { finish(v, f); }, y_of, red);
    row_quantise<VEC, CACHE, 256, NT>(out_q + x.base, a.out_scale + row, y, tid, n_vec, y_of, amax, a.q_min, a.q_max, a.fp8, 0);
  }
}

// The launch form of both kernels: 4 vectors of 16 bytes per thread in registers, or 8 single elements.  `bias`: LayerNorm's.
template <typename T, typename Args>
static RowLaunch norm_row_launch(const Args& a, const float* bias = nullptr) {
  constexpr int WIDE = 16 / sizeof(T);
  const long long moved = a.rows * static_cast<long long>(a.dim) * (static_cast<long long>(sizeof(T)) * (1 + (a.residual ? 1 : 0) + (a.out_sum ? 1 : 0)) + 1);
  return row_launch({{a.hidden, 16}, {a.residual, 16}, {a.out_sum, 16}, {a.out_q, WIDE}, {a.weight, 16}, {bias, 16}, {a.smooth, 16}},
                    a.rows, a.dim, WIDE, moved, 4 * 256, 8 * 256);
}

template <typename T>
static int launch_layernorm_quant(const LayerNormQuantArgs& a, hipStream_t s) {
  constexpr int WIDE = 16 / sizeof(T);
  const RowLaunch f = norm_row_launch<T>(a, a.bias);
  if (f.nt) hipLaunchKernelGGL((layernorm_quant_kernel<T, WIDE, 4, true>), dim3(f.blocks), dim3(256), 0, s, a);
  else if (f.wide) hipLaunchKernelGGL((layernorm_quant_kernel<T, WIDE, 4, false>), dim3(f.blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((layernorm_quant_kernel<T, 1, 8, false>), dim3(f.blocks), dim3(256), 0, s, a);
  MOJO_CHECK_LAUNCH("layernorm_quant");
  note_launch("layernorm_quant:%s:%s:%s", f.width, f.fit, f.policy);
  return MOJO_OK;
}

template <typename T>
static int launch_norm_quant(const NormQuantArgs& a, hipStream_t s, const char* op) {
  constexpr int WIDE = 16 / sizeof(T);
  const RowLaunch f = norm_row_launch<T>(a);
  // a row per wave: dynamic quant (no normalisation: no sum of squares) of many rows that fit one wave's registers
  if (f.wide && !a.weight && a.dim / WIDE <= 4 * 64 && a.rows >= 2048) {
    const int64_t groups = ceil_div(a.rows, 4);
    const unsigned blocks = static_cast<unsigned>(groups > 256 * 32 ? 256 * 32 : groups);
    if (f.nt) hipLaunchKernelGGL((norm_quant_kernel<T, WIDE, 4, true, 64>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((norm_quant_kernel<T, WIDE, 4, false, 64>), dim3(blocks), dim3(256), 0, s, a);
    MOJO_CHECK_LAUNCH("norm_quant");
    note_launch("%s:wide:tpr64:%s", op, f.policy);
    return MOJO_OK;
  }
  if (f.nt) hipLaunchKernelGGL((norm_quant_kernel<T, WIDE, 4, true>), dim3(f.blocks), dim3(256), 0, s, a);
  else if (f.wide) hipLaunchKernelGGL((norm_quant_kernel<T, WIDE, 4>), dim3(f.blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((norm_quant_kernel<T, 1, 8>), dim3(f.blocks), dim3(256), 0, s, a);
  MOJO_CHECK_LAUNCH("norm_quant");
  note_launch("%s:%s:tpr256:%s", op, f.width, f.policy);
  return MOJO_OK;
}

// `op`: the first field of the launch tag (`norm_quant` for the two ops that have always come here)
static int dispatch_norm_quant(const NormQuantArgs& a, int dtype, hipStream_t s, const char* op = "norm_quant") {
  switch (dtype) {
    case MOJO_F32: return launch_norm_quant<float>(a, s, op);
    case MOJO_F16: return launch_norm_quant<f16_t>(a, s, op);
    case MOJO_BF16: return launch_norm_quant<bf16_t>(a, s, op);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "norm_quant: dtype %d not supported", dtype);
  }
}

// The shape and quantised-dtype checks of every entry point, and the fields of its arguments that follow from them.
template <typename Args>
static int set_shape_and_range(Args& a, const char* op, int64_t rows, int64_t dim, int quant_dtype, float q_min, float eps) {
  MOJO_REQUIRE(rows > 0 && dim > 0 && dim < (1LL << 30), MOJO_EINVAL, "%s: bad shape rows=%lld dim=%lld", op, (long long)rows,
               (long long)dim);
  MOJO_REQUIRE(quant_dtype == MOJO_I8 || quant_dtype == MOJO_F8E4M3, MOJO_EUNSUPPORTED,
               "%s: quant dtype %d (int8 / fp8-e4m3 only)", op, quant_dtype);
  a.rows = rows; a.dim = static_cast<int>(dim);
  a.eps = eps; a.fp8 = quant_dtype == MOJO_F8E4M3;
  a.q_max = a.fp8 ? 448.f : 127.f;
  a.q_min = q_min;
  return MOJO_OK;
}

}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_dynamic_quant(const void* input, const float* inv_smooth_scale, void* out_q, float* out_scale,
                                      int64_t rows, int64_t dim, int dtype, mojo_stream_t stream) {
  if (rows == 0) return MOJO_OK;
  MOJO_REQUIRE(input && out_q && out_scale, MOJO_EINVAL, "dynamic_quant: null pointer");
  NormQuantArgs a{};
  a.hidden = input; a.smooth = inv_smooth_scale; a.out_q = out_q; a.out_scale = out_scale;
  a.tiny_scale_is_one = 1;
  if (const int rc = set_shape_and_range(a, "dynamic_quant", rows, dim, MOJO_I8, -128.f, 0.f)) return rc;
  return dispatch_norm_quant(a, dtype, static_cast<hipStream_t>(stream));
}

extern "C" int mojo_hip_residual_add_rmsnorm_quant(const void* hidden, const void* residual, const float* weight,
                                                   const float* smooth_scale, void* out_q, void* out_sum,
                                                   float* out_normed, float* out_scale, int64_t rows, int64_t dim,
                                                   int dtype, int quant_dtype, float q_min, float eps,
                                                   mojo_stream_t stream) {
  if (rows == 0) return MOJO_OK;
  MOJO_REQUIRE(hidden && weight && out_q && out_scale, MOJO_EINVAL, "rmsnorm_quant: null pointer");
  NormQuantArgs a{};
  a.hidden = hidden; a.residual = residual; a.weight = weight; a.smooth = smooth_scale;
  a.out_q = out_q; a.out_sum = out_sum; a.out_normed = out_normed; a.out_scale = out_scale;
  if (const int rc = set_shape_and_range(a, "rmsnorm_quant", rows, dim, quant_dtype, q_min, eps)) return rc;
  return dispatch_norm_quant(a, dtype, static_cast<hipStream_t>(stream));
}

extern "C" int mojo_hip_rmsnorm_quant(const void* hidden, const float* weight, const float* smooth_scale, void* out_q,
                                      float* out_scale, int64_t rows, int64_t dim, int dtype, int quant_dtype, float q_min,
                                      float eps, mojo_stream_t stream) {
  if (rows == 0) return MOJO_OK;
  MOJO_REQUIRE(hidden && weight && out_q && out_scale, MOJO_EINVAL, "rmsnorm_quant: null pointer");
  NormQuantArgs a{};
  a.hidden = hidden; a.weight = weight; a.smooth = smooth_scale; a.out_q = out_q; a.out_scale = out_scale;
  if (const int rc = set_shape_and_range(a, "rmsnorm_quant", rows, dim, quant_dtype, q_min, eps)) return rc;
  return dispatch_norm_quant(a, dtype, static_cast<hipStream_t>(stream), "rmsnorm_quant");
}

extern "C" int mojo_hip_layernorm_quant(const void* hidden, const void* residual, const float* weight, const float* bias,
                                        const float* smooth_scale, void* out_q, void* out_sum, float* out_scale, int64_t rows,
                                        int64_t dim, int dtype, int quant_dtype, float q_min, float eps, mojo_stream_t stream) {
  if (rows == 0) return MOJO_OK;
  MOJO_REQUIRE(hidden && out_q && out_scale, MOJO_EINVAL, "layernorm_quant: null pointer");
  MOJO_REQUIRE((weight == nullptr) == (bias == nullptr), MOJO_EINVAL, "layernorm_quant: weight and bias come together or not at all");
  LayerNormQuantArgs a{};
  a.hidden = hidden; a.residual = residual; a.weight = weight; a.bias = bias; a.smooth = smooth_scale;
  a.out_q = out_q; a.out_sum = out_sum; a.out_scale = out_scale;
  if (const int rc = set_shape_and_range(a, "layernorm_quant", rows, dim, quant_dtype, q_min, eps)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MOJO_F32: return launch_layernorm_quant<float>(a, s);
    case MOJO_F16: return launch_layernorm_quant<f16_t>(a, s);
    case MOJO_BF16: return launch_layernorm_quant<bf16_t>(a, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "layernorm_quant: dtype %d not supported", dtype);
  }
}
