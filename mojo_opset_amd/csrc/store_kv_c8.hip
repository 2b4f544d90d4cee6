// MojoStorePagedKVCacheC8: quantise new K/V tokens [T,Hkv,D] (bf16 / fp16) with per-channel scales [Hkv,D] and write them
// as int8 into the paged caches [N,Hkv,page,D].  Per element the golden computes
//     round(state / scale).clamp(-128, 127).to(int8)
// under torch's type promotion, and the kernel restates that chain bit for bit: a correctly rounded fp32 division (the build
// has no fast-math flag); when state and scale have the SAME 16-bit dtype the quotient is rounded to that dtype first (torch
// returns bf16 for bf16 / bf16; with any other pair of dtypes the quotient stays fp32); round half to even; clamp; convert.
// A lane reads 16 B of a (token, head) row (8 states) and writes 8 B.  Same two addressing forms and the same refusal of
// rows that would write outside the pools as store_kv.hip.
//
// Algorithmic bytes per stored token: 2 tensors x Hkv x D x (elt read + 1 written) (+ the scales, once).
#include "common.h"

namespace mojo {

struct StoreC8Args {
  const char* ks;
  const char* vs;
  char* kc;
  char* vc;
  const void* kscale;
  const void* vscale;
  int64_t tokens, heads, dim, num_blocks, page;
  int64_t src_tok, src_head;          // bytes
  int64_t c_blk, c_head, c_tok;       // bytes (int8 elements)
  int state_bf16;                     // states: 1 = bf16, 0 = fp16
  int scale_dtype;                    // MOJO_F32 / MOJO_F16 / MOJO_BF16
};

// eight states of head h at dims d0 .. d0 + 7 -> eight int8
__device__ __forceinline__ void c8_quant_piece(const StoreC8Args& a, const char* src, char* dst, const void* scale, int64_t sidx) {
  const u32x4 raw = *reinterpret_cast<const u32x4*>(src);
  const bool same16 = (a.state_bf16 && a.scale_dtype == MOJO_BF16) || (!a.state_bf16 && a.scale_dtype == MOJO_F16);
  float sc[8];
  load_coded_f32_vec<8>(scale, a.scale_dtype, sidx, sc);
  unsigned out[2] = {0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const unsigned short bits = static_cast<unsigned short>(raw[e >> 1] >> ((e & 1) * 16));
    const float x = a.state_bf16 ? static_cast<float>(__builtin_bit_cast(bf16_t, bits)) : static_cast<float>(__builtin_bit_cast(f16_t, bits));
    float q = x / sc[e];
    if (same16) q = a.state_bf16 ? static_cast<float>(static_cast<bf16_t>(q)) : static_cast<float>(static_cast<f16_t>(q));
    q = fminf(fmaxf(rintf(q), -128.f), 127.f);
    const int v = static_cast<int>(q);
    out[e >> 2] |= (static_cast<unsigned>(v) & 0xffu) << ((e & 3) * 8);
  }
  *reinterpret_cast<u32x2*>(dst) = u32x2{out[0], out[1]};
}

// One plan row per blockIdx.x; blockIdx.y slices the row's work.  Work item = (tensor, token in chunk, head, 8-element piece).
__global__ __launch_bounds__(256) void store_c8_plan_kernel(StoreC8Args a, const int32_t* __restrict__ plan, int64_t num_chunks) {
  const int pieces = static_cast<int>(a.dim / 8);
  for (int64_t c = blockIdx.x; c < num_chunks; c += gridDim.x) {
    const int32_t src0 = plan[4 * c + 0], blk = plan[4 * c + 1], off = plan[4 * c + 2], len = plan[4 * c + 3];
    // refuse rows that would write outside the pools (the torch golden would raise IndexError)
    if (len <= 0 || blk < 0 || blk >= a.num_blocks || off < 0 || off + len > a.page || src0 < 0 || src0 + len > a.tokens)
      continue;
    const int64_t per_tensor = static_cast<int64_t>(len) * a.heads * pieces;
    const int64_t total = 2 * per_tensor;
    for (int64_t w = static_cast<int64_t>(blockIdx.y) * blockDim.x + threadIdx.x; w < total;
         w += static_cast<int64_t>(gridDim.y) * blockDim.x) {
      const int which = w >= per_tensor;
      int64_t r = which ? w - per_tensor : w;
      const int p = static_cast<int>(r % pieces);
      r /= pieces;
      const int h = static_cast<int>(r % a.heads);
      const int t = static_cast<int>(r / a.heads);
      const char* src = (which ? a.vs : a.ks) + (src0 + t) * a.src_tok + h * a.src_head + p * 16;
      char* dst = (which ? a.vc : a.kc) + blk * a.c_blk + h * a.c_head + (off + t) * a.c_tok + p * 8;
      c8_quant_piece(a, src, dst, which ? a.vscale : a.kscale, h * a.dim + p * 8);
    }
  }
}

// Legacy arguments evaluated per token on the device (no host-side plan, no sync): one wave per token.
__global__ __launch_bounds__(256) void store_c8_layout_kernel(StoreC8Args a, const int32_t* __restrict__ table, int64_t table_stride,
                                                              int64_t max_pages, const int32_t* __restrict__ cu_q,
                                                              const int32_t* __restrict__ ctx_lens, int64_t batch) {
  const int pieces = static_cast<int>(a.dim / 8);
  const int64_t per_tensor = a.heads * pieces;
  const int tok_per_block = blockDim.x / 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * tok_per_block + wave; t < a.tokens;
       t += static_cast<int64_t>(gridDim.x) * tok_per_block) {
    int64_t seq, pos;
    if (cu_q == nullptr) {                                   // decode mode: token t is sequence t
      if (t >= batch) continue;
      seq = t;
      const int32_t c = ctx_lens[seq];
      if (c < 0) continue;
      pos = c;
    } else {
      if (t >= cu_q[batch] || t < cu_q[0]) continue;
      int64_t lo = 0, hi = batch;                            // largest seq with cu_q[seq] <= t (skips empty sequences)
      while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (cu_q[mid] <= t) lo = mid; else hi = mid;
      }
      seq = lo;
      const int32_t c = ctx_lens[seq];
      if (c < 0) continue;
      pos = c + (t - cu_q[seq]);
    }
    const int64_t lp = pos / a.page;
    if (lp >= max_pages) continue;
    const int32_t blk = table[seq * table_stride + lp];
    if (blk < 0 || blk >= a.num_blocks) continue;
    const int64_t slot = pos - lp * a.page;
    for (int64_t w = lane; w < 2 * per_tensor; w += 64) {
      const int which = w >= per_tensor;
      const int64_t r = which ? w - per_tensor : w;
      const int p = static_cast<int>(r % pieces);
      const int h = static_cast<int>(r / pieces);
      const char* src = (which ? a.vs : a.ks) + t * a.src_tok + h * a.src_head + p * 16;
      char* dst = (which ? a.vc : a.kc) + blk * a.c_blk + h * a.c_head + slot * a.c_tok + p * 8;
      c8_quant_piece(a, src, dst, which ? a.vscale : a.kscale, h * a.dim + p * 8);
    }
  }
}

static int fill_c8(StoreC8Args& a, const void* ks, const void* vs, void* kc, void* vc, const void* kscale, const void* vscale,
                   int64_t tokens, int64_t heads, int64_t dim, int64_t num_blocks, int64_t page, int state_dtype, int scale_dtype,
                   int64_t s_tok, int64_t s_head, int64_t c_blk, int64_t c_head, int64_t c_tok) {
  MOJO_REQUIRE(ks && vs && kc && vc && kscale && vscale, MOJO_EINVAL, "store_paged_kv_c8: null pointer");
  MOJO_REQUIRE(state_dtype == MOJO_BF16 || state_dtype == MOJO_F16, MOJO_EUNSUPPORTED,
               "store_paged_kv_c8: state dtype %d (bf16/fp16 only)", state_dtype);
  MOJO_REQUIRE(scale_dtype == MOJO_BF16 || scale_dtype == MOJO_F16 || scale_dtype == MOJO_F32, MOJO_EUNSUPPORTED,
               "store_paged_kv_c8: scale dtype %d (bf16/fp16/fp32 only)", scale_dtype);
  MOJO_REQUIRE(heads > 0 && dim > 0 && page > 0 && num_blocks >= 0 && tokens >= 0, MOJO_EINVAL, "store_paged_kv_c8: bad shape");
  MOJO_REQUIRE(dim % 8 == 0 && s_tok % 8 == 0 && s_head % 8 == 0 && c_blk % 8 == 0 && c_head % 8 == 0 && c_tok % 8 == 0 &&
                   aligned_to(ks, 16) && aligned_to(vs, 16) && aligned_to(kc, 8) && aligned_to(vc, 8) &&
                   aligned_to(kscale, 16) && aligned_to(vscale, 16),
               MOJO_EUNSUPPORTED, "store_paged_kv_c8: head_dim and strides must be multiples of 8 elements, states and scales 16-byte and caches 8-byte aligned");
  a.ks = static_cast<const char*>(ks); a.vs = static_cast<const char*>(vs);
  a.kc = static_cast<char*>(kc); a.vc = static_cast<char*>(vc);
  a.kscale = kscale; a.vscale = vscale;
  a.tokens = tokens; a.heads = heads; a.dim = dim; a.num_blocks = num_blocks; a.page = page;
  a.src_tok = s_tok * 2; a.src_head = s_head * 2;
  a.c_blk = c_blk; a.c_head = c_head; a.c_tok = c_tok;
  a.state_bf16 = state_dtype == MOJO_BF16 ? 1 : 0;
  a.scale_dtype = scale_dtype;
  return MOJO_OK;
}

}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_store_paged_kv_c8_plan(const void* key_states, const void* value_states, void* key_cache,
                                               void* value_cache, const void* key_scale, const void* value_scale,
                                               const int32_t* plan, int64_t num_chunks, int64_t num_tokens,
                                               int64_t num_kv_heads, int64_t head_dim, int64_t num_blocks,
                                               int64_t block_size, int state_dtype, int scale_dtype,
                                               int64_t src_token_stride, int64_t src_head_stride,
                                               int64_t cache_block_stride, int64_t cache_head_stride,
                                               int64_t cache_token_stride, mojo_stream_t stream) {
  if (num_chunks == 0) return MOJO_OK;
  StoreC8Args a{};
  const int rc = fill_c8(a, key_states, value_states, key_cache, value_cache, key_scale, value_scale, num_tokens, num_kv_heads,
                         head_dim, num_blocks, block_size, state_dtype, scale_dtype, src_token_stride, src_head_stride,
                         cache_block_stride, cache_head_stride, cache_token_stride);
  if (rc) return rc;
  MOJO_REQUIRE(plan != nullptr && num_chunks > 0, MOJO_EINVAL, "store_paged_kv_c8_plan: null plan");
  // a chunk holds at most `block_size` tokens: slice it so that each block handles ~1024 pieces
  const int64_t max_items = 2 * block_size * num_kv_heads * (head_dim / 8);
  int64_t gy = ceil_div(max_items, 256 * 4);
  if (gy > 64) gy = 64;
  const int64_t gx = num_chunks > 65535 ? 65535 : num_chunks;
  hipLaunchKernelGGL(store_c8_plan_kernel, dim3(static_cast<unsigned>(gx), static_cast<unsigned>(gy)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, plan, num_chunks);
  MOJO_CHECK_LAUNCH("store_paged_kv_c8_plan");
  note_launch("store_kv:plan:kv8");
  return MOJO_OK;
}

extern "C" int mojo_hip_store_paged_kv_c8_layout(const void* key_states, const void* value_states, void* key_cache,
                                                 void* value_cache, const void* key_scale, const void* value_scale,
                                                 const int32_t* block_table, int64_t block_table_stride,
                                                 int64_t max_blocks_per_seq, const int32_t* cu_q_lens,
                                                 const int32_t* context_kv_lens, int64_t batch, int64_t num_tokens,
                                                 int64_t num_kv_heads, int64_t head_dim, int64_t num_blocks,
                                                 int64_t block_size, int state_dtype, int scale_dtype,
                                                 int64_t src_token_stride, int64_t src_head_stride,
                                                 int64_t cache_block_stride, int64_t cache_head_stride,
                                                 int64_t cache_token_stride, mojo_stream_t stream) {
  if (num_tokens == 0 || batch == 0 || max_blocks_per_seq == 0) return MOJO_OK;
  StoreC8Args a{};
  const int rc = fill_c8(a, key_states, value_states, key_cache, value_cache, key_scale, value_scale, num_tokens, num_kv_heads,
                         head_dim, num_blocks, block_size, state_dtype, scale_dtype, src_token_stride, src_head_stride,
                         cache_block_stride, cache_head_stride, cache_token_stride);
  if (rc) return rc;
  MOJO_REQUIRE(block_table != nullptr && context_kv_lens != nullptr, MOJO_EINVAL,
               "store_paged_kv_c8_layout: block_table and context_kv_lens are required");
  int64_t gx = ceil_div(num_tokens, 4);
  if (gx > 8192) gx = 8192;
  hipLaunchKernelGGL(store_c8_layout_kernel, dim3(static_cast<unsigned>(gx)), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                     block_table, block_table_stride, max_blocks_per_seq, cu_q_lens, context_kv_lens, batch);
  MOJO_CHECK_LAUNCH("store_paged_kv_c8_layout");
  note_launch("store_kv:layout:kv8");
  return MOJO_OK;
}
