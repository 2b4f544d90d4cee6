// MojoVisionRotaryEmbedding2D: the (cos, sin) rows of a vision tower's 2-D rotary embedding, one launch for a batch of images.
//
// Sample b is a grid of (H_b, W_b) patches and owns the rows [first_b, first_b + H_b * W_b).  Patch order is the adapooling
// regrouping: with pooling factor f the grid is cut into f x f windows, the windows are walked row-major and the patches of a
// window row-major inside it, so token i of a sample is
//   window (bh, bw) = (i / (f * f)) / (W / f), (i / (f * f)) % (W / f);   inside it (ih, iw) = (i % (f * f)) / f, (i % (f * f)) % f
//   (h, w) = (bh * f + ih, bw * f + iw)
// The row is [h-angles (rope_dim / 4) | w-angles (rope_dim / 4)] twice: angle = float(pos) * inv_freq[j], ONE fp32 product
// rounded once (the golden's `outer`), then cosf / sinf.  The reference builds a max_grid x rope_dim / 4 table on the host and
// gathers from it per sample; here every token computes its own position from its index.
//
// `samples` is an int64 [B, 3] device array of (first row, H, W), written by the host from the one grid_hw read the op's
// contract already contains (the output size is a host quantity).
#include "common.h"

namespace mojo {

__global__ __launch_bounds__(256) void vision_rotary_2d_kernel(float* __restrict__ cos_out, float* __restrict__ sin_out,
                                                               const int64_t* __restrict__ samples, int64_t batch,
                                                               int64_t tokens, int rope_dim, int pool,
                                                               const float* __restrict__ inv_freq) {
  const int half = rope_dim / 2, quarter = rope_dim / 4;
  const int64_t total = tokens * half;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t tok = idx / half;
    const int j = static_cast<int>(idx - tok * half);
    int64_t lo = 0, hi = batch;                            // the sample that owns the row: first_lo <= tok < first_(lo + 1)
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (samples[mid * 3] <= tok) lo = mid; else hi = mid;
    }
    const int64_t i = tok - samples[lo * 3];
    const int64_t gw = samples[lo * 3 + 2];
    const int64_t win = i / (pool * pool), in = i - win * (pool * pool);
    const int64_t wins_w = gw / pool;
    const int64_t bh = win / wins_w, bw = win - bh * wins_w;
    const int64_t ih = in / pool, iw = in - ih * pool;
    const int64_t pos = j < quarter ? bh * pool + ih : bw * pool + iw;
    const float ang = __fmul_rn(static_cast<float>(pos), inv_freq[j < quarter ? j : j - quarter]);
    const float c = cosf(ang), s = sinf(ang);
    float* co = cos_out + tok * rope_dim;
    float* so = sin_out + tok * rope_dim;
    co[j] = c; co[half + j] = c;
    so[j] = s; so[half + j] = s;
  }
}

}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_vision_rotary_2d(float* cos_out, float* sin_out, const int64_t* samples, int64_t batch,
                                         int64_t tokens, int64_t rope_dim, int64_t adapooling_factor,
                                         const float* inv_freq, mojo_stream_t stream) {
  if (tokens == 0 || batch == 0) return MOJO_OK;
  MOJO_REQUIRE(cos_out && sin_out && samples && inv_freq, MOJO_EINVAL, "vision_rotary_2d: null pointer");
  MOJO_REQUIRE(batch > 0 && tokens > 0, MOJO_EINVAL, "vision_rotary_2d: negative size");
  MOJO_REQUIRE(rope_dim > 0 && rope_dim % 4 == 0 && rope_dim < (1LL << 20), MOJO_EINVAL,
               "vision_rotary_2d: rope_dim %lld must be a positive multiple of 4", (long long)rope_dim);
  MOJO_REQUIRE(adapooling_factor >= 1 && adapooling_factor < (1LL << 15), MOJO_EINVAL,
               "vision_rotary_2d: adapooling_factor %lld must be >= 1", (long long)adapooling_factor);
  int64_t blocks = ceil_div(tokens * (rope_dim / 2), 256);
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(vision_rotary_2d_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     cos_out, sin_out, samples, batch, tokens, static_cast<int>(rope_dim), static_cast<int>(adapooling_factor),
                     inv_freq);
  MOJO_CHECK_LAUNCH("vision_rotary_2d");
  note_launch("vision_rotary_2d:pool%d", static_cast<int>(adapooling_factor));
  return MOJO_OK;
}
