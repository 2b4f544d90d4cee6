// MojoMRoPE / MojoMRoPEInplace: the multimodal rotary embedding of a Qwen-VL decoder (temporal, height and width positions).
//   out[t, n, i]        = h1 * c - h2 * s          i < half = sum(mrope_section)
//   out[t, n, half + i] = h2 * c + h1 * s
//   out[t, n, j]        = x[t, n, j]               j >= 2 * half  (out of place: copied; in place: not touched)
// with h1 = x[t, n, i], h2 = x[t, n, half + i] and (c, s) = (cos, sin)[table(i)][t, i].  Each product is rounded on its own in
// fp32 (no FMA contraction, as apply_rope_kernel), the sum once, and the result once to the storage type.
//
// Tables are [3, T, half] (temporal / height / width) or [T, half] (already merged); for the 3-D form the kernel picks the
// table per element and never materialises a merged one:
//   chunked:      table(i) = 0 / 1 / 2 for i in [0, s0) / [s0, s0 + s1) / [s0 + s1, half)
//   interleaved:  table(i) = 1 where i % 3 == 1 and i < 3 * s1, 2 where i % 3 == 2 and i < 3 * s2, else 0
// fp32, fp16 or bf16 tables; a 16-bit table is converted on read.
//
// query [T, Hq * hd] and key [T, Hk * hd] are addressed by a row stride (a slice of a fused QKV row is read, and in the
// in-place form written, where it is).  One launch serves q and k.
//
// Algorithmic bytes per token: (Hq + Hk) x rope_dim x elt read + the same written (+ the pass-through tail out of place)
// + 2 x half x table elt.
#include "common.h"

namespace mojo {

struct MRopeArgs {
  const void* src[2];
  void* dst[2];
  int64_t s_t[2], d_t[2];      // row strides (elements)
  int heads[2];
  const void* cos;
  const void* sin;
  int table_kind;              // MOJO_F32 / MOJO_F16 / MOJO_BF16
  int64_t tab_sec, tab_t;      // strides of the tables (elements): section (0 for a merged [T, half] table), token
  int64_t tokens;
  int head_dim, half;
  int sec0, sec1, sec2;
  int interleaved;
};

static __device__ __forceinline__ float mrope_tab(const void* p, int kind, int64_t i) {
  if (kind == MOJO_F32) return static_cast<const float*>(p)[i];
  if (kind == MOJO_F16) return elt<f16_t>::to_f(static_cast<const f16_t*>(p)[i]);
  return elt<bf16_t>::to_f(static_cast<const bf16_t*>(p)[i]);
}

// A "row" is one (t, head) vector.  Work items per row: half / VEC rotation pairs, then (out of place only) the
// (head_dim - 2 half) / VEC pass-through vectors.  (1 << lg) >= items threads serve one row.
// A workgroup takes `tpb` consecutive tokens at a time.  It first merges their (cos, sin) rows into LDS — the per-element
// table choice is made there, once per token, not once per head — and every head then reads its VEC values as vectors:
// with the choice inside the row loop each thread issued 2 VEC scalar loads beside its two 16-byte data loads, and the
// kernel ran at 3.3 TB/s where apply_rope_kernel reaches 5.6 on the same bytes.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void mrope_kernel(MRopeArgs a, int items_rot, int items_pass, int lg, int tpb, int hs /* LDS row: half rounded up to 4 floats */) {
  typedef typename vec_of<T, VEC>::type V;
  extern __shared__ __attribute__((aligned(16))) float s_tab[];     // [tpb][cos | sin][hs]
  const int rows_per_block = 256 >> lg;
  const int item = threadIdx.x & ((1 << lg) - 1);
  const int heads_total = a.heads[0] + a.heads[1];
  for (int64_t t0 = static_cast<int64_t>(blockIdx.x) * tpb; t0 < a.tokens; t0 += static_cast<int64_t>(gridDim.x) * tpb) {
    const int nt = static_cast<int>(min(static_cast<int64_t>(tpb), a.tokens - t0));
    __syncthreads();                                       // the readers of the previous group are done
    for (int e = threadIdx.x; e < nt * a.half; e += 256) {
      const int tt = e / a.half, i = e - tt * a.half;
      int tb;
      if (a.interleaved) tb = (i % 3 == 1 && i < 3 * a.sec1) ? 1 : ((i % 3 == 2 && i < 3 * a.sec2) ? 2 : 0);
      else tb = i < a.sec0 ? 0 : (i < a.sec0 + a.sec1 ? 1 : 2);
      const int64_t ti = tb * a.tab_sec + (t0 + tt) * a.tab_t + i;
      s_tab[(tt * 2) * hs + i] = mrope_tab(a.cos, a.table_kind, ti);
      s_tab[(tt * 2 + 1) * hs + i] = mrope_tab(a.sin, a.table_kind, ti);
    }
    __syncthreads();
    if (item >= items_rot + items_pass) continue;
    for (int r = threadIdx.x >> lg; r < nt * heads_total; r += rows_per_block) {
      const int tt = r / heads_total;
      int hh = r - tt * heads_total;
      const int which = hh >= a.heads[0];
      if (which) hh -= a.heads[0];
      const int64_t t = t0 + tt;
      const T* src = static_cast<const T*>(a.src[which]) + t * a.s_t[which] + static_cast<int64_t>(hh) * a.head_dim;
      T* dst = static_cast<T*>(a.dst[which]) + t * a.d_t[which] + static_cast<int64_t>(hh) * a.head_dim;
      if (item >= items_rot) {
        const int j0 = 2 * a.half + (item - items_rot) * VEC;
        store_vec<T, VEC>(dst + j0, load_vec<T, VEC>(src + j0));
        continue;
      }
      const int i0 = item * VEC;
      const V x1 = load_vec<T, VEC>(src + i0);
      const V x2 = load_vec<T, VEC>(src + a.half + i0);
      const float* cr = s_tab + (tt * 2) * hs + i0;
      const float* sr = cr + hs;
      float c[VEC], s[VEC];
      if constexpr (VEC % 4 == 0) {                          // (i0 and hs are multiples of 4: 16-byte LDS reads)
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {
          const f32x4 cv = *reinterpret_cast<const f32x4*>(cr + 4 * q), sv = *reinterpret_cast<const f32x4*>(sr + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) { c[4 * q + e] = cv[e]; s[4 * q + e] = sv[e]; }
        }
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) { c[j] = cr[j]; s[j] = sr[j]; }
      }
      V o1, o2;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float h1 = elt<T>::to_f(vget<T, VEC>(x1, j));
        const float h2 = elt<T>::to_f(vget<T, VEC>(x2, j));
        const float r1 = __fsub_rn(__fmul_rn(h1, c[j]), __fmul_rn(h2, s[j]));
        const float r2 = __fadd_rn(__fmul_rn(h2, c[j]), __fmul_rn(h1, s[j]));
        vset<T, VEC>(o1, j, elt<T>::from_f(r1));
        vset<T, VEC>(o2, j, elt<T>::from_f(r2));
      }
      store_vec<T, VEC>(dst + i0, o1);
      store_vec<T, VEC>(dst + a.half + i0, o2);
    }
  }
}

template <typename T>
static int dispatch_mrope(const MRopeArgs& a, bool inplace, hipStream_t s) {
  const int pass = a.head_dim - 2 * a.half;
  auto ok = [&](int vec) {
    if (a.half % vec || pass % vec || a.head_dim % vec) return false;
    const size_t al = vec * sizeof(T);
    for (int w = 0; w < 2; ++w) {
      if (!aligned_to(a.src[w], al) || !aligned_to(a.dst[w], al)) return false;
      if (a.s_t[w] % vec || a.d_t[w] % vec) return false;
    }
    return true;
  };
  int vec = 1;
  for (int v : {static_cast<int>(16 / sizeof(T)), static_cast<int>(8 / sizeof(T)), 2})
    if (v > 1 && ok(v)) { vec = v; break; }
  const int items_rot = a.half / vec, items_pass = inplace ? 0 : pass / vec;
  int lg = 0;
  while ((1 << lg) < items_rot + items_pass) ++lg;
  MOJO_REQUIRE(lg <= 8, MOJO_EUNSUPPORTED, "mrope: head_dim %d too large for this kernel", a.head_dim);
  // tokens per workgroup pass: as many as its row slots hold (at least one), as long as their merged rows fit 32 KiB of LDS
  const int heads_total = a.heads[0] + a.heads[1];
  const int hs = (a.half + 3) & ~3;
  MOJO_REQUIRE(2 * hs * 4 <= 32768, MOJO_EUNSUPPORTED, "mrope: rope_dim %d too large for this kernel", 2 * a.half);
  int tpb = (256 >> lg) / heads_total;
  tpb = tpb < 1 ? 1 : tpb;
  while (tpb > 1 && tpb * 2 * hs * 4 > 32768) --tpb;
  const size_t lds = static_cast<size_t>(tpb) * 2 * hs * sizeof(float);
  int64_t blocks = ceil_div(a.tokens, static_cast<int64_t>(tpb));
  if (blocks > 256 * 32) blocks = 256 * 32;
#define LAUNCH(V) hipLaunchKernelGGL((mrope_kernel<T, V>), dim3(static_cast<unsigned>(blocks)), dim3(256), lds, s, a, items_rot, items_pass, lg, tpb, hs)
  if (vec == 16 / sizeof(T)) LAUNCH(16 / sizeof(T));
  else if (vec == 8 / sizeof(T)) LAUNCH(8 / sizeof(T));
  else if (vec == 2) LAUNCH(2);
  else LAUNCH(1);
#undef LAUNCH
  MOJO_CHECK_LAUNCH("mrope");
  note_launch("mrope:vec%d:%s:%s", vec, inplace ? "inplace" : "copy", a.tab_sec == 0 ? "merged" : (a.interleaved ? "interleaved" : "chunked"));
  return MOJO_OK;
}

}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_mrope(const void* query, const void* key, void* query_out, void* key_out, const void* cos_table,
                              const void* sin_table, int64_t tokens, int64_t q_heads, int64_t k_heads, int64_t head_dim,
                              int64_t q_row_stride, int64_t k_row_stride, int64_t qo_row_stride, int64_t ko_row_stride,
                              int64_t table_section_stride, int64_t table_token_stride, const int64_t mrope_section[3],
                              int is_interleaved, int table_dtype, int dtype, mojo_stream_t stream) {
  if (tokens == 0 || q_heads + k_heads == 0) return MOJO_OK;
  MOJO_REQUIRE(query && key && query_out && key_out && cos_table && sin_table && mrope_section, MOJO_EINVAL, "mrope: null pointer");
  MOJO_REQUIRE(tokens > 0 && q_heads >= 0 && k_heads >= 0 && head_dim > 0 && head_dim < (1LL << 20), MOJO_EINVAL, "mrope: bad sizes");
  const int64_t s0 = mrope_section[0], s1 = mrope_section[1], s2 = mrope_section[2];
  MOJO_REQUIRE(s0 >= 0 && s1 >= 0 && s2 >= 0 && s0 + s1 + s2 > 0 && 2 * (s0 + s1 + s2) <= head_dim, MOJO_EINVAL,
               "mrope: mrope_section (%lld, %lld, %lld) must be non-negative with 2 * sum <= head_dim %lld", (long long)s0,
               (long long)s1, (long long)s2, (long long)head_dim);
  MOJO_REQUIRE(table_dtype == MOJO_F32 || table_dtype == MOJO_F16 || table_dtype == MOJO_BF16, MOJO_EUNSUPPORTED,
               "mrope: table dtype %d (f32, f16, bf16)", table_dtype);
  MOJO_REQUIRE(table_section_stride >= 0 && table_token_stride >= 0, MOJO_EINVAL, "mrope: negative table stride");
  const bool inplace = query_out == query && key_out == key;
  MOJO_REQUIRE(inplace || (query_out != query && key_out != key), MOJO_EINVAL, "mrope: either both outputs alias their inputs or neither");
  MOJO_REQUIRE(!inplace || (qo_row_stride == q_row_stride && ko_row_stride == k_row_stride), MOJO_EINVAL,
               "mrope: the in-place form takes one row stride per tensor");
  MRopeArgs a;
  a.src[0] = query; a.src[1] = key; a.dst[0] = query_out; a.dst[1] = key_out;
  a.s_t[0] = q_row_stride; a.s_t[1] = k_row_stride; a.d_t[0] = qo_row_stride; a.d_t[1] = ko_row_stride;
  a.heads[0] = static_cast<int>(q_heads); a.heads[1] = static_cast<int>(k_heads);
  a.cos = cos_table; a.sin = sin_table; a.table_kind = table_dtype;
  a.tab_sec = table_section_stride; a.tab_t = table_token_stride;
  a.tokens = tokens; a.head_dim = static_cast<int>(head_dim); a.half = static_cast<int>(s0 + s1 + s2);
  a.sec0 = static_cast<int>(s0); a.sec1 = static_cast<int>(s1); a.sec2 = static_cast<int>(s2);
  a.interleaved = is_interleaved ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MOJO_F32: return dispatch_mrope<float>(a, inplace, s);
    case MOJO_F16: return dispatch_mrope<f16_t>(a, inplace, s);
    case MOJO_BF16: return dispatch_mrope<bf16_t>(a, inplace, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "mrope: dtype %d not supported", dtype);
  }
}
