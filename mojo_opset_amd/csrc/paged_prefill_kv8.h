// MojoPagedPrefillGQAWithKVDequant — the simple route: a dequantising page gather, then the 16-bit prefill on its pages.
// Included at the end of paged_prefill_gqa.hip (calls paged_prefill of that file).
//
// gather_kv8_kernel reads the int8 pages a sequence's block table names, multiplies by the per-channel scales
// (K8 * key_scale, V8 * value_scale: fp32 products rounded to the query dtype) and writes compact 16-bit scratch pages:
// page lp of sequence b lands at scratch page b * ppb + lp, which is also what the scratch table the same kernel writes says
// (-1 for an id outside the pool — the prefill kernel reads such a page as zeros — and for every page past the sequence's
// length, which is not gathered; scratch page 0, which the prefill kernel loads for a negative id, is zero-filled when it is
// not gathered).  ppb =ceil(min(max_total_seq_len hint, page * table width) / page), sized without a host sync: a caller who
// omits the hint on a wide table pays for the table's capacity in workspace (not in bytes moved).
// The gather moves three int8-cache-sizes of bytes (1 read + 2 written) per gathered element, once per call.
#pragma once

namespace mojo {

struct GatherKv8Args {
  const char* kc;
  const char* vc;
  const void* kscale;
  const void* vscale;
  void* ks_out;                       // [B * ppb][Hkv][page][D] 16-bit
  void* vs_out;
  int32_t* table_out;                 // [B][ppb]
  const int32_t* tables;
  const int32_t* cu_q;
  const int32_t* cu_kv;               // may be null: the query lengths
  int64_t table_stride, c_blk, c_head, c_tok, num_blocks;
  int hkv, dim, page, ppb, max_pages, scale_dtype, out_bf16;
};

// grid = (B * ppb, Hkv); a work item = 16 int8 of a token row of K or of V
__global__ __launch_bounds__(256) void gather_kv8_kernel(GatherKv8Args a) {
  const int sp = blockIdx.x, h = blockIdx.y;
  const int b = sp / a.ppb, lp = sp - b * a.ppb;
  const int32_t* cu = a.cu_kv ? a.cu_kv : a.cu_q;
  const int kv_len = min(max(cu[b + 1] - cu[b], 0), a.ppb * a.page);
  const int needed = (kv_len + a.page - 1) / a.page;
  const int phys = lp < a.max_pages ? a.tables[static_cast<int64_t>(b) * a.table_stride + lp] : -1;
  const bool ok = phys >= 0 && phys < a.num_blocks;
  // a scratch page is present only where it is written: inside the row's length and named by an id of the pool
  if (h == 0 && threadIdx.x == 0) a.table_out[sp] = (ok && lp < needed) ? sp : -1;
  const int pieces = a.dim / 16;
  const int per_tensor = a.page * pieces;
  const int64_t dst_base = (static_cast<int64_t>(sp) * a.hkv + h) * a.page * a.dim;
  if (!ok || lp >= needed) {
    // Scratch page 0 is the page the prefill kernel loads for every absent id (it clamps the id to 0 and gives those keys a
    // probability of zero): when it is not gathered itself it must still hold finite numbers — 0 * NaN of an unwritten
    // workspace would reach the output.  No other absent page is ever addressed.
    if (sp == 0) {
      const u32x4 z = {0u, 0u, 0u, 0u};
      for (int w = threadIdx.x; w < 2 * per_tensor; w += blockDim.x) {
        const int which = w >= per_tensor;
        char* dst = static_cast<char*>(which ? a.vs_out : a.ks_out) + (dst_base + static_cast<int64_t>(which ? w - per_tensor : w) * 16) * 2;
        *reinterpret_cast<u32x4*>(dst) = z;
        *reinterpret_cast<u32x4*>(dst + 16) = z;
      }
    }
    return;
  }
  const int64_t src_base = static_cast<int64_t>(phys) * a.c_blk + static_cast<int64_t>(h) * a.c_head;
  for (int w = threadIdx.x; w < 2 * per_tensor; w += blockDim.x) {
    const int which = w >= per_tensor;
    const int r = which ? w - per_tensor : w;
    const int t = r / pieces, p = r - t * pieces;
    const u32x4 raw = *reinterpret_cast<const u32x4*>((which ? a.vc : a.kc) + src_base + static_cast<int64_t>(t) * a.c_tok + p * 16);
    const void* scale = which ? a.vscale : a.kscale;
    const int64_t sidx = static_cast<int64_t>(h) * a.dim + p * 16;
    float sc[2][8];
    load_coded_f32_vec<8>(scale, a.scale_dtype, sidx, sc[0]);
    load_coded_f32_vec<8>(scale, a.scale_dtype, sidx + 8, sc[1]);
    unsigned short o[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int x = static_cast<int>(static_cast<signed char>(raw[e >> 2] >> ((e & 3) * 8)));
      const float v = static_cast<float>(x) * sc[e >> 3][e & 7];
      o[e] = a.out_bf16 ? __builtin_bit_cast(unsigned short, static_cast<bf16_t>(v)) : __builtin_bit_cast(unsigned short, static_cast<f16_t>(v));
    }
    u32x4 lo, hi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lo[e] = static_cast<unsigned>(o[2 * e]) | (static_cast<unsigned>(o[2 * e + 1]) << 16);
      hi[e] = static_cast<unsigned>(o[8 + 2 * e]) | (static_cast<unsigned>(o[8 + 2 * e + 1]) << 16);
    }
    char* dst = static_cast<char*>(which ? a.vs_out : a.ks_out) + (dst_base + static_cast<int64_t>(t) * a.dim + p * 16) * 2;
    *reinterpret_cast<u32x4*>(dst) = lo;
    *reinterpret_cast<u32x4*>(dst + 16) = hi;
  }
}

struct PrefillKv8Plan { int64_t ppb, ws_inner, off_table, off_k, off_v, total; };

// `g`: the call's geometry over the int8 cache.  `inner`: the same over the scratch pages, what the 16-bit prefill is planned on.
static PrefillKv8Plan prefill_kv8_plan(const PrefillGeom& g, PrefillGeom& inner) {
  PrefillKv8Plan p{};
  int64_t cap = g.page * g.max_pages;
  if (g.max_kv_hint > 0 && g.max_kv_hint < cap) cap = g.max_kv_hint;
  p.ppb = g.page > 0 ? ceil_div(cap, g.page) : 0;
  if (p.ppb < 1) p.ppb = 1;                              // (a table without columns: one scratch page per row, marked absent)
  inner = g;
  inner.max_pages = p.ppb;
  p.ws_inner = prefill_plan(inner).query_bytes;
  auto up = [](int64_t x) { return (x + 255) & ~int64_t{255}; };
  p.off_table = up(p.ws_inner);
  p.off_k = p.off_table + up(g.batch * p.ppb * 4);
  const int64_t pool = up(g.batch * p.ppb * g.kv_heads * g.page * g.head_dim * 2);
  p.off_v = p.off_k + pool;
  p.total = p.off_v + pool;
  return p;
}

}  // namespace mojo

extern "C" int64_t mojo_hip_paged_prefill_gqa_kv8_workspace_bytes(int64_t total_tokens, int64_t batch, int64_t q_heads,
                                                                  int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                                                  int64_t max_blocks_per_seq, int64_t max_q_len_hint,
                                                                  int64_t max_kv_len_hint) {
  if (total_tokens <= 0 || batch <= 0 || q_heads <= 0 || kv_heads <= 0 || q_heads % kv_heads) return 0;
  mojo::PrefillGeom inner;
  return mojo::prefill_kv8_plan({total_tokens, batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_q_len_hint,
                                 max_kv_len_hint}, inner).total;
}

extern "C" int mojo_hip_paged_prefill_gqa_kv8(const void* query, const void* key_cache, const void* key_scale,
                                              const void* value_cache, const void* value_scale, const int32_t* cu_q_lens,
                                              const int32_t* cu_total_seq_lens, const int32_t* block_tables, void* out,
                                              int64_t total_tokens, int64_t batch, int64_t q_heads, int64_t kv_heads,
                                              int64_t head_dim, int64_t num_blocks, int64_t block_size,
                                              int64_t max_blocks_per_seq, int64_t block_table_stride,
                                              int64_t cache_block_stride, int64_t cache_head_stride,
                                              int64_t cache_token_stride, int64_t max_q_len_hint, int64_t max_kv_len_hint,
                                              float softmax_scale, int layout_abab, int dtype, int scale_dtype,
                                              void* workspace, int64_t workspace_bytes, mojo_stream_t stream) {
  using namespace mojo;
  if (total_tokens == 0) return MOJO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MOJO_REQUIRE(query && key_cache && value_cache && key_scale && value_scale && cu_q_lens && block_tables && out, MOJO_EINVAL,
               "paged_prefill_gqa_kv8: null pointer");
  MOJO_REQUIRE(q_heads > 0 && kv_heads > 0 && q_heads % kv_heads == 0 && batch >= 0, MOJO_EINVAL,
               "paged_prefill_gqa_kv8: bad head counts Hq=%lld Hkv=%lld", (long long)q_heads, (long long)kv_heads);
  MOJO_REQUIRE(dtype == MOJO_BF16 || dtype == MOJO_F16, MOJO_EUNSUPPORTED, "paged_prefill_gqa_kv8: query dtype %d (bf16/fp16 only)", dtype);
  MOJO_REQUIRE(scale_dtype == MOJO_BF16 || scale_dtype == MOJO_F16 || scale_dtype == MOJO_F32, MOJO_EUNSUPPORTED,
               "paged_prefill_gqa_kv8: scale dtype %d (bf16/fp16/fp32 only)", scale_dtype);
  const int64_t G = q_heads / kv_heads;
  MOJO_REQUIRE((G == 1 || G == 2 || G == 4 || G == 8) && (head_dim == 64 || head_dim == 96 || head_dim == 128), MOJO_EUNSUPPORTED,
               "paged_prefill_gqa_kv8: group size %lld / head_dim %lld (groups 1, 2, 4, 8; head_dim 64, 96, 128)", (long long)G,
               (long long)head_dim);
  MOJO_REQUIRE(block_size > 0 && block_size % 4 == 0, MOJO_EUNSUPPORTED, "paged_prefill_gqa_kv8: block_size %lld must be a multiple of 4",
               (long long)block_size);
  MOJO_REQUIRE(cache_token_stride % 16 == 0 && cache_head_stride % 16 == 0 && cache_block_stride % 16 == 0 &&
                   aligned_to(key_cache, 16) && aligned_to(value_cache, 16) && aligned_to(query, 16) && aligned_to(out, 16) &&
                   aligned_to(key_scale, 16) && aligned_to(value_scale, 16),
               MOJO_EUNSUPPORTED, "paged_prefill_gqa_kv8: tensors must be 16-byte aligned with 16-byte row strides");
  // the 16-bit prefill over the scratch pages: dense [page][Hkv][token][D] pools and the scratch table, one row of ppb ids each
  PrefillCall c;
  c.query = query; c.cu_q_lens = cu_q_lens; c.cu_total_seq_lens = cu_total_seq_lens; c.out = out;
  c.softmax_scale = softmax_scale; c.layout_abab = layout_abab; c.dtype = dtype; c.stream = stream;
  const PrefillGeom geom{total_tokens, batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_q_len_hint, max_kv_len_hint};
  if (batch == 0) {                                      // no sequences: the 16-bit entry point's own treatment (zeros)
    c.g = geom; c.g.max_pages = 0;
    c.key_cache = key_cache; c.value_cache = value_cache; c.block_tables = block_tables; c.block_table_stride = block_table_stride;
    c.cache_block_stride = c.cache_head_stride = c.cache_token_stride = 16;
    return paged_prefill(c);
  }
  const PrefillKv8Plan p = prefill_kv8_plan(geom, c.g);
  MOJO_REQUIRE(workspace && workspace_bytes >= p.total, MOJO_EWORKSPACE, "paged_prefill_gqa_kv8: workspace %lld B < required %lld B",
               (long long)workspace_bytes, (long long)p.total);
  MOJO_REQUIRE(aligned_to(workspace, 256), MOJO_EINVAL, "paged_prefill_gqa_kv8: workspace must be 256-byte aligned");
  MOJO_REQUIRE(batch * p.ppb < (int64_t{1} << 31) && kv_heads <= 65535 && block_size * p.ppb < (int64_t{1} << 31), MOJO_EUNSUPPORTED,
               "paged_prefill_gqa_kv8: grid limit");
  char* ws = static_cast<char*>(workspace);
  GatherKv8Args g{};
  g.kc = static_cast<const char*>(key_cache); g.vc = static_cast<const char*>(value_cache);
  g.kscale = key_scale; g.vscale = value_scale;
  g.ks_out = ws + p.off_k; g.vs_out = ws + p.off_v; g.table_out = reinterpret_cast<int32_t*>(ws + p.off_table);
  g.tables = block_tables; g.cu_q = cu_q_lens; g.cu_kv = cu_total_seq_lens;
  g.table_stride = block_table_stride; g.c_blk = cache_block_stride; g.c_head = cache_head_stride; g.c_tok = cache_token_stride;
  g.num_blocks = num_blocks;
  g.hkv = static_cast<int>(kv_heads); g.dim = static_cast<int>(head_dim); g.page = static_cast<int>(block_size);
  g.ppb = static_cast<int>(p.ppb); g.max_pages = static_cast<int>(max_blocks_per_seq);
  g.scale_dtype = scale_dtype; g.out_bf16 = dtype == MOJO_BF16 ? 1 : 0;
  hipLaunchKernelGGL(gather_kv8_kernel, dim3(static_cast<unsigned>(batch * p.ppb), static_cast<unsigned>(kv_heads)), dim3(256), 0, s, g);
  MOJO_CHECK_LAUNCH("paged_prefill_gqa_kv8(gather)");
  c.key_cache = ws + p.off_k; c.value_cache = ws + p.off_v; c.block_tables = g.table_out; c.block_table_stride = p.ppb;
  c.cache_block_stride = kv_heads * block_size * head_dim; c.cache_head_stride = block_size * head_dim; c.cache_token_stride = head_dim;
  c.workspace = p.ws_inner > 0 ? ws : nullptr; c.workspace_bytes = p.ws_inner;
  const int rc = paged_prefill(c);
  if (rc != MOJO_OK) return rc;
  note_launch("gather:kv8+%s", "prefill");
  return MOJO_OK;
}
