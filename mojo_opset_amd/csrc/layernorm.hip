// MojoLayerNorm / MojoResidualAddLayerNorm (16-bit and fp32 outputs; the quantising pair lives in norm_quant.hip).
//   sum    = round_T(hidden + residual)                                  (residual optional)
//   mean   = sum(sum) / D,  var = mean((sum - mean)^2),  rstd = rsqrt(var + eps)          -- fp32
//   normed = round_T(fma((sum - mean) * rstd, weight, bias))             (weight and bias optional, together)
// fp32 math over the row held in registers, ONE rounding of the result: the structure of rmsnorm_kernel with a second
// reduction.  The variance is the mean of squared deviations, never E[x^2] - mean^2, which loses every digit of a row
// whose mean is large against its spread.  The first reduction's mean carries the rounding of a D-term fp32 sum (1e-7 of
// the mean: 1e-4 of the spread for a row at 1000 +- 1), so the deviation pass also sums the deviations themselves and
// the mean is corrected by their mean, delta: d = (x - mean0) - delta, var = mean((x - mean0)^2) - delta^2 (the
// corrected two-pass form; delta^2 is a rounding-sized term, not a cancellation).  Both sums ride one reduction.
//
// One row per TPR threads as in rmsnorm.hip; a thread keeps kLnCache vectors of its row, rows too long for that (only
// TPR = 256 has such) re-read the tail in the deviation and the output pass.
//
// Algorithmic bytes per row (pre, with residual): 2 reads + 2 writes of D x elt, + weight and bias once.
#include "common.h"

namespace mojo {

constexpr int kLnCache = 4;          // vectors of its row a thread keeps in registers (mojo_hip_layernorm_cache_vectors)

struct LayerNormArgs {
  const void* hidden;        // rows h_stride elements apart
  const void* residual;      // rows r_stride elements apart, or nullptr
  const void* weight;        // [dim] T, or nullptr together with bias
  const void* bias;
  void* normed;              // [rows, dim] dense
  void* summed;              // [rows, dim] dense or nullptr
  int64_t rows, h_stride, r_stride;
  int dim;
  float eps;
};

template <typename T, int VEC, int TPR, int CACHE, bool RESIDUAL, bool AFFINE, bool NT /* stream_nt(): activations by-pass the caches */>
__global__ __launch_bounds__(256) void layernorm_kernel(LayerNormArgs a) {
  typedef typename vec_of<T, VEC>::type V;
  constexpr int ROWS_PER_BLOCK = 256 / TPR;
  constexpr int NW = TPR / 64;
  __shared__ float red[2][4];
  const int sub = threadIdx.x / TPR;
  const int tid = threadIdx.x % TPR;
  const int n_vec = a.dim / VEC;
  const float inv_dim = 1.0f / static_cast<float>(a.dim);
  const T* weight = static_cast<const T*>(a.weight);
  const T* bias = static_cast<const T*>(a.bias);

  // the row's sum over its TPR threads, for two values at once; valid in every thread of the row
  auto row_sum2 = [&](float& p, float& q) {
    p = wave_sum(p);
    q = wave_sum(q);
    if constexpr (NW > 1) {
      const int wave = threadIdx.x >> 6;
      if ((threadIdx.x & 63) == 0) { red[0][wave] = p; red[1][wave] = q; }
      __syncthreads();
      float tp = 0.f, tq = 0.f;
#pragma unroll
      for (int i = 0; i < NW; ++i) { tp += red[0][sub * NW + i]; tq += red[1][sub * NW + i]; }
      p = tp; q = tq;
      __syncthreads();                // `red` is reused by the next reduction
    }
  };

  // A thread serves the same vectors of every row it meets: their weight and bias are loaded once, ahead of the first row's
  // reductions (per row, after the reductions, they were a third and a fourth stream from L2 on the critical path).
  V wc[CACHE], bc[CACHE];
  if constexpr (AFFINE) {
#pragma unroll
    for (int c = 0; c < CACHE; ++c) {
      const int v = tid + c * TPR;
      if (v < n_vec) { wc[c] = load_vec<T, VEC>(weight + v * VEC); bc[c] = load_vec<T, VEC>(bias + v * VEC); }
    }
  }

  // (the trip count is the same for every thread of the block -- the NW > 1 forms synchronise inside the loop; a row group
  // past the end recomputes the last row and stores nothing)
  for (int64_t row0 = static_cast<int64_t>(blockIdx.x) * ROWS_PER_BLOCK; row0 < a.rows;
       row0 += static_cast<int64_t>(gridDim.x) * ROWS_PER_BLOCK) {
    const bool live = row0 + sub < a.rows;
    const int64_t row = live ? row0 + sub : a.rows - 1;
    const T* h = static_cast<const T*>(a.hidden) + row * a.h_stride;
    const T* r = RESIDUAL ? static_cast<const T*>(a.residual) + row * a.r_stride : nullptr;
    T* so = a.summed ? static_cast<T*>(a.summed) + row * a.dim : nullptr;
    T* no = static_cast<T*>(a.normed) + row * a.dim;

    // vector v of the (summed) row; `first`: the streaming load, and the sum is stored
    auto load_row = [&](int v, bool first) -> V {
      V x = (NT && first) ? load_vec_nt<T, VEC>(h + v * VEC) : load_vec<T, VEC>(h + v * VEC);
      if constexpr (RESIDUAL) {
        const V y = (NT && first) ? load_vec_nt<T, VEC>(r + v * VEC) : load_vec<T, VEC>(r + v * VEC);
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          vset<T, VEC>(x, j, elt<T>::from_f(elt<T>::to_f(vget<T, VEC>(x, j)) + elt<T>::to_f(vget<T, VEC>(y, j))));
        if (first && so && live) {
          if (NT) store_vec_nt<T, VEC>(so + v * VEC, x); else store_vec<T, VEC>(so + v * VEC, x);
        }
      }
      return x;
    };

    // ---- pass 1: the row into registers, its sum ------------------------------------------------------------------------
    V cache[CACHE];
    float s0 = 0.f, unused = 0.f;
#pragma unroll
    for (int c = 0; c < CACHE; ++c) {
      const int v = tid + c * TPR;
      if (v < n_vec) {
        cache[c] = load_row(v, true);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s0 += elt<T>::to_f(vget<T, VEC>(cache[c], j));
      }
    }
    for (int v = tid + CACHE * TPR; v < n_vec; v += TPR) {
      const V x = load_row(v, true);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s0 += elt<T>::to_f(vget<T, VEC>(x, j));
    }
    row_sum2(s0, unused);
    const float mean0 = s0 * inv_dim;

    // ---- pass 2: deviations from mean0: their sum (the mean's correction) and their squares ------------------------------
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < CACHE; ++c) {
      if (tid + c * TPR < n_vec) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float d = elt<T>::to_f(vget<T, VEC>(cache[c], j)) - mean0;
          s1 += d;
          s2 = fmaf(d, d, s2);
        }
      }
    }
    for (int v = tid + CACHE * TPR; v < n_vec; v += TPR) {
      const V x = load_row(v, false);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float d = elt<T>::to_f(vget<T, VEC>(x, j)) - mean0;
        s1 += d;
        s2 = fmaf(d, d, s2);
      }
    }
    row_sum2(s1, s2);
    const float delta = s1 * inv_dim;
    const float var = fmaxf(fmaf(-delta, delta, s2 * inv_dim), 0.f);
    const float rstd = rsqrtf(var + a.eps);

    // ---- pass 3: the output ----------------------------------------------------------------------------------------------
    auto finish = [&](int v, const V& x, const V& w, const V& b) {
      V o;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float y = ((elt<T>::to_f(vget<T, VEC>(x, j)) - mean0) - delta) * rstd;
        if constexpr (AFFINE) y = fmaf(y, elt<T>::to_f(vget<T, VEC>(w, j)), elt<T>::to_f(vget<T, VEC>(b, j)));
        vset<T, VEC>(o, j, elt<T>::from_f(y));
      }
      if (live) {
        if (NT) store_vec_nt<T, VEC>(no + v * VEC, o); else store_vec<T, VEC>(no + v * VEC, o);
      }
    };
#pragma unroll
    for (int c = 0; c < CACHE; ++c) {
      const int v = tid + c * TPR;
      if (v < n_vec) finish(v, cache[c], wc[c], bc[c]);
    }
    for (int v = tid + CACHE * TPR; v < n_vec; v += TPR) {
      V w, b;
      if constexpr (AFFINE) { w = load_vec<T, VEC>(weight + v * VEC); b = load_vec<T, VEC>(bias + v * VEC); }
      finish(v, load_row(v, false), w, b);
    }
  }
}

struct LnForm { int vec, tpr; bool reread, nt; };   // the template choice a launch took (its mojo_hip_last_launch() tag)

template <typename T, int VEC, int TPR, bool NT>
static void launch_ln_form(const LayerNormArgs& a, int64_t blocks, hipStream_t s) {
  if (blocks > 256 * 32) blocks = 256 * 32;
#define MOJO_LN_GO(R, A) hipLaunchKernelGGL((layernorm_kernel<T, VEC, TPR, kLnCache, R, A, NT>), dim3(blocks), dim3(256), 0, s, a)
  if (a.residual) { if (a.weight) MOJO_LN_GO(true, true); else MOJO_LN_GO(true, false); }
  else { if (a.weight) MOJO_LN_GO(false, true); else MOJO_LN_GO(false, false); }
#undef MOJO_LN_GO
}

template <typename T, int VEC>
static LnForm launch_ln(const LayerNormArgs& a, hipStream_t s) {
  constexpr bool WIDE = VEC * sizeof(T) == 16;
  const int64_t n_vec = a.dim / VEC;
  // the non-temporal forms exist for the 16-byte vectors only: a tensor large enough to want them is not read by elements
  const bool nt = WIDE && stream_nt(a.rows * a.dim * static_cast<long long>(sizeof(T)) * (a.residual ? (a.summed ? 4 : 3) : 2));
  const int tpr = WIDE ? rms_threads_per_row(a.rows, n_vec) : (n_vec <= 64 * 4 ? 64 : (n_vec <= 128 * 4 ? 128 : 256));
  auto go = [&](auto tpr_tag, int64_t blocks) {
    constexpr int TPR = decltype(tpr_tag)::value;
    if constexpr (WIDE) {
      if (nt) { launch_ln_form<T, VEC, TPR, true>(a, blocks, s); return; }
    }
    launch_ln_form<T, VEC, TPR, false>(a, blocks, s);
  };
  if (tpr == 64) go(std::integral_constant<int, 64>{}, ceil_div(a.rows, 4));          // short rows: one wave per row, 4 rows per block
  else if (tpr == 128) go(std::integral_constant<int, 128>{}, ceil_div(a.rows, 2));   // two waves per row, two rows per block
  else go(std::integral_constant<int, 256>{}, a.rows);
  return {VEC, tpr, n_vec > static_cast<int64_t>(tpr) * kLnCache, nt};
}

template <typename T>
static int dispatch_ln(const LayerNormArgs& a, hipStream_t s) {
  constexpr int WIDE = 16 / sizeof(T);
  auto ok = [&](int vec) {
    const size_t al = vec * sizeof(T);
    return a.dim % vec == 0 && a.h_stride % vec == 0 && aligned_to(a.hidden, al) && aligned_to(a.normed, al) &&
           (!a.residual || (a.r_stride % vec == 0 && aligned_to(a.residual, al))) && (!a.summed || aligned_to(a.summed, al)) &&
           (!a.weight || (aligned_to(a.weight, al) && aligned_to(a.bias, al)));
  };
  LnForm f;
  if (ok(WIDE)) f = launch_ln<T, WIDE>(a, s);
  else if (ok(2)) f = launch_ln<T, 2>(a, s);
  else f = launch_ln<T, 1>(a, s);
  MOJO_CHECK_LAUNCH("layernorm");
  note_launch("layernorm:vec%d:tpr%d:%s:%s", f.vec, f.tpr, f.reread ? "reread" : "cached", f.nt ? "nt" : "plain");
  return MOJO_OK;
}

}  // namespace mojo

using namespace mojo;

extern "C" int64_t mojo_hip_layernorm_cache_vectors(void) { return kLnCache; }

extern "C" int mojo_hip_layernorm(const void* hidden, const void* residual, const void* weight, const void* bias,
                                  void* normed_out, void* sum_out, int64_t rows, int64_t dim, int64_t hidden_row_stride,
                                  int64_t residual_row_stride, int dtype, float eps, mojo_stream_t stream) {
  if (rows == 0) return MOJO_OK;
  MOJO_REQUIRE(hidden && normed_out, MOJO_EINVAL, "layernorm: null pointer");
  MOJO_REQUIRE(rows > 0 && dim > 0 && dim < (1LL << 30), MOJO_EINVAL, "layernorm: bad shape rows=%lld dim=%lld",
               (long long)rows, (long long)dim);
  MOJO_REQUIRE((weight == nullptr) == (bias == nullptr), MOJO_EINVAL, "layernorm: weight and bias come together or not at all");
  MOJO_REQUIRE(hidden_row_stride >= dim && (!residual || residual_row_stride >= dim), MOJO_EINVAL,
               "layernorm: a row stride is shorter than the row (dim=%lld)", (long long)dim);
  MOJO_REQUIRE(residual || !sum_out, MOJO_EINVAL, "layernorm: sum_out without a residual");
  LayerNormArgs a;
  a.hidden = hidden; a.residual = residual; a.weight = weight; a.bias = bias; a.normed = normed_out; a.summed = sum_out;
  a.rows = rows; a.h_stride = hidden_row_stride; a.r_stride = residual ? residual_row_stride : 0;
  a.dim = static_cast<int>(dim); a.eps = eps;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MOJO_F32: return dispatch_ln<float>(a, s);
    case MOJO_F16: return dispatch_ln<f16_t>(a, s);
    case MOJO_BF16: return dispatch_ln<bf16_t>(a, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "layernorm: dtype %d not supported", dtype);
  }
}
