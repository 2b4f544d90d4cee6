// MojoGridRoPE: rotary embedding over a (F, H, W) grid with precomputed complex frequencies (the Wan2.2 DiT's q and k).
//   out[i, t, n, 2j : 2j + 2] = (a * c - b * s, a * s + b * c)      for t < F_i * H_i * W_i
//   out[i, t, n, :]           = x[i, t, n, :]                        for the padding tokens behind it
// with (a, b) = x[i, t, n, 2j : 2j + 2] and (c, s) = freqs_i[t, j].  Each product and each sum is rounded on its own in fp32
// (no FMA contraction, as apply_rope_kernel) and the result once to the storage type: the golden's complex product.
//
// x is read in the caller's layout through 64-bit strides (the [B, L, N, D] view of a projection, a slice of a fused QKV
// buffer), out is dense.  The grid sizes are read on the device: no host synchronisation.  The frequencies are the fp32
// pairs of a complex64 tensor, [rows, D / 2, 2]: the VEC elements a thread rotates and the VEC floats it needs sit at the
// same offset of their rows.  A sample's rows are [first, first + count) of one buffer (a table entry per sample, or rows
// [0, shared_rows) for all); a token at or past `count` is copied, so no row outside an entry is ever read.
//
// Algorithmic bytes per token: N x D x elt read + the same written + D x 4 of frequencies (shared by the N heads).
#include "common.h"

namespace mojo {

struct GridRopeArgs {
  const void* x;
  void* out;
  const float* freqs;
  const void* grid;            // [batch, 3] int32 / int64 on the device
  int grid_i64;
  const int64_t* table;        // [batch, 2] (first row, rows) on the device, or nullptr
  int64_t shared_rows;
  int64_t tokens;
  int heads, head_dim;
  int64_t s_b, s_t, s_n;       // strides of x (elements)
};

// A "row" is one (t, head) vector of head_dim elements of sample blockIdx.y; (1 << lg) >= items threads serve one row.
template <typename T, int VEC, bool NT>
__global__ __launch_bounds__(256) void grid_rope_kernel(GridRopeArgs a, int items, int lg) {
  typedef typename vec_of<T, VEC>::type V;
  static_assert(VEC % 2 == 0, "a vector holds whole pairs");
  const int64_t b = blockIdx.y;
  int64_t g[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    g[i] = a.grid_i64 ? static_cast<const int64_t*>(a.grid)[b * 3 + i] : static_cast<int64_t>(static_cast<const int32_t*>(a.grid)[b * 3 + i]);
  int64_t n_rot = 0;
  if (g[0] > 0 && g[1] > 0 && g[2] > 0) {
    // (factors clamped to the token count first: the product of three such stays inside 64 bits for every legal launch)
    const int64_t cap = a.tokens;
    const int64_t p = (g[0] < cap ? g[0] : cap) * (g[1] < cap ? g[1] : cap);
    n_rot = (p < cap ? p : cap) * (g[2] < cap ? g[2] : cap);
    if (n_rot > cap) n_rot = cap;
  }
  const int64_t f_first = a.table ? a.table[b * 2] : 0;
  const int64_t f_rows = a.table ? a.table[b * 2 + 1] : a.shared_rows;
  if (n_rot > f_rows) n_rot = f_rows;

  const unsigned heads = static_cast<unsigned>(a.heads);
  const unsigned n_rows = static_cast<unsigned>(a.tokens) * heads;        // < 2^31 (checked by the host)
  const unsigned rows_per_block = 256u >> lg;
  const int item = threadIdx.x & ((1 << lg) - 1);
  if (item >= items) return;
  const T* src_b = static_cast<const T*>(a.x) + b * a.s_b;
  T* dst_b = static_cast<T*>(a.out) + b * a.tokens * a.heads * a.head_dim;
  for (unsigned row = blockIdx.x * rows_per_block + (threadIdx.x >> lg); row < n_rows; row += gridDim.x * rows_per_block) {
    const unsigned t = row / heads;
    const unsigned n = row - t * heads;
    const T* src = src_b + static_cast<int64_t>(t) * a.s_t + static_cast<int64_t>(n) * a.s_n + item * VEC;
    T* dst = dst_b + static_cast<int64_t>(row) * a.head_dim + item * VEC;
    const V x = NT ? load_vec_nt<T, VEC>(src) : load_vec<T, VEC>(src);
    V o = x;
    if (static_cast<int64_t>(t) < n_rot) {
      const float* f = a.freqs + (f_first + t) * a.head_dim + item * VEC;
#pragma unroll
      for (int j = 0; j < VEC; j += 2) {
        const f32x2 cs = *reinterpret_cast<const f32x2*>(f + j);
        const float re_in = elt<T>::to_f(vget<T, VEC>(x, j));
        const float im_in = elt<T>::to_f(vget<T, VEC>(x, j + 1));
        const float re = __fsub_rn(__fmul_rn(re_in, cs[0]), __fmul_rn(im_in, cs[1]));
        const float im = __fadd_rn(__fmul_rn(re_in, cs[1]), __fmul_rn(im_in, cs[0]));
        vset<T, VEC>(o, j, elt<T>::from_f(re));
        vset<T, VEC>(o, j + 1, elt<T>::from_f(im));
      }
    }
    if (NT) store_vec_nt<T, VEC>(dst, o); else store_vec<T, VEC>(dst, o);
  }
}

template <typename T>
static int dispatch_grid_rope(const GridRopeArgs& a, int64_t batch, hipStream_t s) {
  constexpr int WIDE = 16 / sizeof(T);
  const bool wide = a.head_dim % WIDE == 0 && aligned_to(a.x, 16) && aligned_to(a.out, 16) && a.s_b % WIDE == 0 &&
                    a.s_t % WIDE == 0 && a.s_n % WIDE == 0;
  const size_t pair = 2 * sizeof(T);
  MOJO_REQUIRE(wide || (aligned_to(a.x, pair) && aligned_to(a.out, pair) && a.s_b % 2 == 0 && a.s_t % 2 == 0 && a.s_n % 2 == 0),
               MOJO_EUNSUPPORTED, "grid_rope: x and its strides must keep the (even, odd) pairs aligned to a pair");
  const int vec = wide ? WIDE : 2;
  const int items = a.head_dim / vec;
  int lg = 0;
  while ((1 << lg) < items) ++lg;
  MOJO_REQUIRE(lg <= 8, MOJO_EUNSUPPORTED, "grid_rope: head_dim %d too large for this kernel", a.head_dim);
  const int64_t n_rows = a.tokens * a.heads;
  const long long bytes = 2LL * batch * n_rows * a.head_dim * static_cast<long long>(sizeof(T));
  const bool nt = wide && stream_nt(bytes);
  int64_t blocks = ceil_div(n_rows, 256 >> lg);
  if (blocks > 256 * 32) blocks = 256 * 32;
  const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(batch));
  if (nt) hipLaunchKernelGGL((grid_rope_kernel<T, WIDE, true>), grid, dim3(256), 0, s, a, items, lg);
  else if (wide) hipLaunchKernelGGL((grid_rope_kernel<T, WIDE, false>), grid, dim3(256), 0, s, a, items, lg);
  else hipLaunchKernelGGL((grid_rope_kernel<T, 2, false>), grid, dim3(256), 0, s, a, items, lg);
  MOJO_CHECK_LAUNCH("grid_rope");
  note_launch("grid_rope:vec%d:%s", vec, nt ? "nt" : "plain");
  return MOJO_OK;
}

}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_grid_rope(const void* x, void* out, const float* freqs, const void* grid_sizes, int grid_sizes_is_i64,
                                  const int64_t* freq_table, int64_t shared_freq_rows, int64_t batch, int64_t tokens,
                                  int64_t heads, int64_t head_dim, const int64_t x_strides[3], int dtype,
                                  mojo_stream_t stream) {
  if (batch == 0 || tokens == 0 || heads == 0 || head_dim == 0) return MOJO_OK;
  MOJO_REQUIRE(x && out && freqs && grid_sizes && x_strides, MOJO_EINVAL, "grid_rope: null pointer");
  MOJO_REQUIRE(batch > 0 && tokens > 0 && heads > 0 && head_dim > 0, MOJO_EINVAL, "grid_rope: negative size");
  MOJO_REQUIRE(head_dim % 2 == 0, MOJO_EINVAL, "grid_rope: head_dim %lld must be even (complex pairs)", (long long)head_dim);
  MOJO_REQUIRE(batch <= 65535 && tokens * heads < (1LL << 31) && head_dim < (1LL << 20), MOJO_EUNSUPPORTED,
               "grid_rope: batch %lld / tokens x heads %lld outside the launch's range", (long long)batch, (long long)(tokens * heads));
  MOJO_REQUIRE(freq_table || shared_freq_rows >= 0, MOJO_EINVAL, "grid_rope: negative frequency row count");
  MOJO_REQUIRE(aligned_to(freqs, 8), MOJO_EINVAL, "grid_rope: the frequencies must be aligned to a (cos, sin) pair");
  GridRopeArgs a;
  a.x = x; a.out = out; a.freqs = freqs; a.grid = grid_sizes; a.grid_i64 = grid_sizes_is_i64; a.table = freq_table;
  a.shared_rows = shared_freq_rows; a.tokens = tokens; a.heads = static_cast<int>(heads); a.head_dim = static_cast<int>(head_dim);
  a.s_b = x_strides[0]; a.s_t = x_strides[1]; a.s_n = x_strides[2];
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MOJO_F32: return dispatch_grid_rope<float>(a, batch, s);
    case MOJO_F16: return dispatch_grid_rope<f16_t>(a, batch, s);
    case MOJO_BF16: return dispatch_grid_rope<bf16_t>(a, batch, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "grid_rope: dtype %d not supported", dtype);
  }
}
