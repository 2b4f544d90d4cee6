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
//
// MojoPagedPrefillSWAWithKVDequant — the same two stages with a window: gather_kv8_swa_kernel, then the SWA 16-bit prefill.
// A sequence of kv_len keys and q_len queries sees the union [0, min(global, kv_len)) + [max(0, kv_len - q_len - local), kv_len);
// only the logical pages that intersect it are read from the int8 cache.  The scratch is COMPACT: a row owns cpb pool pages,
// cpb = ceil(global / page) + ceil((q_bound + local + 1) / page) + 2 capped by ppb, q_bound = the max_q_len hint or the token
// count — whatever the context and the table's width (see GatherWin: the sequence is rebased onto its visible pages, so the
// scratch table is [B][cpb] too).  The SWA prefill kernel never addresses a page outside the union of its rows (pages of
// >= 16 tokens, paged_prefill_gqa.hip), and pool page 0 — what it loads for a negative id — is zero-filled when nothing is
// gathered into it: no byte the gather did not write reaches the output.
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
  // windowed gather only: pool pages per row, local (< 0: none) / global (<= 0: none) window, sequences, rebased cu_kv [B + 1]
  int cpb = 0, local_win = -1, global_win = 0, batch = 0;
  int32_t* cu_out = nullptr;
};

// 16-byte work items of one page of one kv head, K then V: 16 int8 -> 16 scaled 16-bit numbers each
__device__ __forceinline__ void gather_kv8_page(const GatherKv8Args& a, int phys, int h, int64_t dst_base) {
  const int pieces = a.dim / 16;
  const int per_tensor = a.page * pieces;
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

__device__ __forceinline__ void gather_kv8_zero(const GatherKv8Args& a, int64_t dst_base) {
  const int per_tensor = a.page * (a.dim / 16);
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int w = threadIdx.x; w < 2 * per_tensor; w += blockDim.x) {
    const int which = w >= per_tensor;
    char* dst = static_cast<char*>(which ? a.vs_out : a.ks_out) + (dst_base + static_cast<int64_t>(which ? w - per_tensor : w) * 16) * 2;
    *reinterpret_cast<u32x4*>(dst) = z;
    *reinterpret_cast<u32x4*>(dst + 16) = z;
  }
}

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
  const int64_t dst_base = (static_cast<int64_t>(sp) * a.hkv + h) * a.page * a.dim;
  if (!ok || lp >= needed) {
    // Scratch page 0 is the page the prefill kernel loads for every absent id (it clamps the id to 0 and gives those keys a
    // probability of zero): when it is not gathered itself it must still hold finite numbers — 0 * NaN of an unwritten
    // workspace would reach the output.  No other absent page is ever addressed.
    if (sp == 0) gather_kv8_zero(a, dst_base);
    return;
  }
  gather_kv8_page(a, phys, h, dst_base);
}

// The windowed gather REBASES a sequence: the pages [gp, lp0) between its global pages [0, gp) and the first page lp0 of its
// local range hold keys no row of it sees, so they are cut out — the 16-bit prefill runs on a sequence of kv_len - shift keys
// (shift = (lp0 - gp) * page) whose page i is pool page i of the row: the global pages in order, then the local ones.  Every row
// keeps its distance to the local keys and stays behind the global ones, so each (row, kept key) pair is exactly as visible as
// before (global keys: j < global either way, and never local; local keys: j - shift against p - shift).  Without a local
// window the rows' own positions stand in for the local range (their pages keep the positions apart and are never read).
struct GatherWin { int gp, lp0, needed, count, kv_rebased; };
__device__ __forceinline__ GatherWin gather_kv8_win(const GatherKv8Args& a, int b) {
  const int32_t* cu = a.cu_kv ? a.cu_kv : a.cu_q;
  const int kv_raw = max(cu[b + 1] - cu[b], 0);
  const int q_len = max(a.cu_q[b + 1] - a.cu_q[b], 0);
  const int kv_len = min(kv_raw, a.ppb * a.page);       // (a length above the hint: truncated, as the unwindowed gather)
  GatherWin w;
  w.needed = q_len > 0 ? (kv_len + a.page - 1) / a.page : 0;    // (a row without queries reads nothing)
  const int lstart = max(kv_raw - q_len - max(a.local_win, 0), 0);   // first key of the first row's local window
  const int gend = min(max(a.global_win, 0), kv_len);
  w.gp = min((gend + a.page - 1) / a.page, w.needed);
  w.lp0 = min(lstart / a.page, w.needed);
  if (w.lp0 <= w.gp) { w.gp = w.needed; w.lp0 = w.needed; }     // the ranges meet: one run of pages, nothing cut
  w.count = min(w.gp + w.needed - w.lp0, a.cpb);               // (cpb bounds it when the hints hold; a row beyond them is cut)
  w.kv_rebased = kv_raw - (w.lp0 - w.gp) * a.page;
  return w;
}

// grid = (B * cpb + 1, Hkv): pool page (b, i) gathers page i of the rebased sequence b and writes its entry of the scratch
// table ([B][cpb]: the pool page itself, or -1).  The one workgroup behind the last pool page writes the rebased cumulative kv
// lengths ([B + 1]) and nothing else, so that no gathering workgroup waits for it.
__global__ __launch_bounds__(256) void gather_kv8_swa_kernel(GatherKv8Args a) {
  const int sp = blockIdx.x, h = blockIdx.y;
  const int b = sp / a.cpb, idx = sp - b * a.cpb;
  if (sp == a.batch * a.cpb) {                          // (workgroup-uniform)
    if (h != 0) return;
    __shared__ int s_len[256];
    int carry = 0;
    for (int b0 = 0; b0 < a.batch; b0 += 256) {
      const int bb = b0 + static_cast<int>(threadIdx.x);
      s_len[threadIdx.x] = bb < a.batch ? gather_kv8_win(a, bb).kv_rebased : 0;
      __syncthreads();
      if (threadIdx.x == 0) {
        if (b0 == 0) a.cu_out[0] = 0;
        const int n = min(256, a.batch - b0);
        for (int i = 0; i < n; ++i) { carry += s_len[i]; a.cu_out[b0 + i + 1] = carry; }
      }
      __syncthreads();
    }
    return;
  }
  const GatherWin w = gather_kv8_win(a, b);
  const int lp = idx < w.gp ? idx : w.lp0 + (idx - w.gp);
  // (no local window: the pages behind the global ones only keep the rows' positions apart — never read, not gathered)
  const bool wanted = idx < w.count && lp < a.max_pages && (a.local_win >= 0 || idx < w.gp);
  const int phys = wanted ? a.tables[static_cast<int64_t>(b) * a.table_stride + lp] : -1;
  const bool ok = phys >= 0 && phys < a.num_blocks;
  if (h == 0 && threadIdx.x == 0) a.table_out[sp] = ok ? sp : -1;
  const int64_t dst_base = (static_cast<int64_t>(sp) * a.hkv + h) * a.page * a.dim;
  if (!ok) {
    if (sp == 0) gather_kv8_zero(a, dst_base);          // pool page 0 stays finite (see gather_kv8_kernel)
    return;
  }
  gather_kv8_page(a, phys, h, dst_base);
}

// cpb: pool pages and table entries per row (= ppb without a window); off_cu: the rebased cumulative kv lengths (window only)
struct PrefillKv8Plan { int64_t ppb, cpb, ws_inner, off_table, off_cu, off_k, off_v, total; bool swa; };

// `g`: the call's geometry over the int8 cache.  `inner`: the same over the scratch pages, what the 16-bit prefill is planned on.
static PrefillKv8Plan prefill_kv8_plan(const PrefillGeom& g, PrefillGeom& inner) {
  PrefillKv8Plan p{};
  int64_t cap = g.page * g.max_pages;
  if (g.max_kv_hint > 0 && g.max_kv_hint < cap) cap = g.max_kv_hint;
  p.ppb = g.page > 0 ? ceil_div(cap, g.page) : 0;
  if (p.ppb < 1) p.ppb = 1;                              // (a table without columns: one scratch page per row, marked absent)
  p.cpb = p.ppb;
  p.swa = g.local_window >= 0 || g.global_window > 0;
  if (p.swa && g.page > 0) {   // window: the pages a row's visible union can touch
    const int64_t q_bound = (g.max_q_hint > 0 && g.max_q_hint < g.total_tokens) ? g.max_q_hint : g.total_tokens;
    int64_t vis = 2;
    if (g.global_window > 0) vis += ceil_div(g.global_window, g.page);
    vis += ceil_div(q_bound + (g.local_window >= 0 ? g.local_window : 0) + 1, g.page);   // (no local window: the rows' own pages, table entries only)
    if (vis < p.cpb) p.cpb = vis;
  }
  inner = g;
  inner.max_pages = p.cpb;
  p.ws_inner = prefill_plan(inner).query_bytes;
  auto up = [](int64_t x) { return (x + 255) & ~int64_t{255}; };
  p.off_table = up(p.ws_inner);
  p.off_cu = p.off_table + up(g.batch * p.cpb * 4);
  p.off_k = p.off_cu + (p.swa ? up((g.batch + 1) * 4) : 0);
  const int64_t pool = up(g.batch * p.cpb * g.kv_heads * g.page * g.head_dim * 2);
  p.off_v = p.off_k + pool;
  p.total = p.off_v + pool;
  return p;
}

}  // namespace mojo

// The int8-cache prefill entry points share one body: a window selects the windowed gather and the SWA prefill on its pages.
static int paged_prefill_kv8(const void* query, const void* key_cache, const void* key_scale, const void* value_cache,
                             const void* value_scale, const int32_t* cu_q_lens, const int32_t* cu_total_seq_lens,
                             const int32_t* block_tables, void* out, int64_t total_tokens, int64_t batch, int64_t q_heads,
                             int64_t kv_heads, int64_t head_dim, int64_t num_blocks, int64_t block_size, int64_t max_blocks_per_seq,
                             int64_t block_table_stride, int64_t cache_block_stride, int64_t cache_head_stride,
                             int64_t cache_token_stride, int64_t max_q_len_hint, int64_t max_kv_len_hint, float softmax_scale,
                             int layout_abab, int dtype, int scale_dtype, void* workspace, int64_t workspace_bytes,
                             int64_t local_window, int64_t global_window, mojo_stream_t stream) {
  using namespace mojo;
  if (total_tokens == 0) return MOJO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool swa = local_window >= 0 || global_window > 0;
  if (!swa) { local_window = -1; global_window = 0; }
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
  // (the SWA prefill kernel stays inside the union of its rows' windows only with pages of whole 16-key staging groups)
  MOJO_REQUIRE(!swa || block_size % 16 == 0, MOJO_EUNSUPPORTED, "paged_prefill_swa_kv8: block_size %lld must be a multiple of 16",
               (long long)block_size);
  MOJO_REQUIRE(cache_token_stride % 16 == 0 && cache_head_stride % 16 == 0 && cache_block_stride % 16 == 0 &&
                   aligned_to(key_cache, 16) && aligned_to(value_cache, 16) && aligned_to(query, 16) && aligned_to(out, 16) &&
                   aligned_to(key_scale, 16) && aligned_to(value_scale, 16),
               MOJO_EUNSUPPORTED, "paged_prefill_gqa_kv8: tensors must be 16-byte aligned with 16-byte row strides");
  // the 16-bit prefill over the scratch pages: dense [page][Hkv][token][D] pools and the scratch table, one row of cpb ids each
  PrefillCall c;
  c.query = query; c.cu_q_lens = cu_q_lens; c.cu_total_seq_lens = cu_total_seq_lens; c.out = out;
  c.softmax_scale = softmax_scale; c.layout_abab = layout_abab; c.dtype = dtype; c.stream = stream;
  const PrefillGeom geom{total_tokens, batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_q_len_hint, max_kv_len_hint,
                         local_window, global_window};
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
  MOJO_REQUIRE(batch * p.cpb < (int64_t{1} << 31), MOJO_EUNSUPPORTED, "paged_prefill_gqa_kv8: grid limit");
  MOJO_REQUIRE(!swa || (local_window < (int64_t{1} << 29) && global_window < (int64_t{1} << 29) && block_size * p.ppb < (int64_t{1} << 29)),
               MOJO_EUNSUPPORTED, "paged_prefill_swa_kv8: lengths and windows must stay below 2^29");
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
  if (swa) {
    g.cpb = static_cast<int>(p.cpb); g.batch = static_cast<int>(batch);
    g.cu_out = reinterpret_cast<int32_t*>(ws + p.off_cu);
    c.cu_total_seq_lens = g.cu_out;                      // the rebased lengths (GatherWin)
    g.local_win = local_window >= 0 ? static_cast<int>(local_window) : -1;
    g.global_win = global_window > 0 ? static_cast<int>(global_window) : 0;
    hipLaunchKernelGGL(gather_kv8_swa_kernel, dim3(static_cast<unsigned>(batch * p.cpb + 1), static_cast<unsigned>(kv_heads)), dim3(256), 0, s, g);
    MOJO_CHECK_LAUNCH("paged_prefill_swa_kv8(gather)");
  } else {
    hipLaunchKernelGGL(gather_kv8_kernel, dim3(static_cast<unsigned>(batch * p.ppb), static_cast<unsigned>(kv_heads)), dim3(256), 0, s, g);
    MOJO_CHECK_LAUNCH("paged_prefill_gqa_kv8(gather)");
  }
  c.key_cache = ws + p.off_k; c.value_cache = ws + p.off_v; c.block_tables = g.table_out; c.block_table_stride = p.cpb;
  c.cache_block_stride = kv_heads * block_size * head_dim; c.cache_head_stride = block_size * head_dim; c.cache_token_stride = head_dim;
  c.workspace = p.ws_inner > 0 ? ws : nullptr; c.workspace_bytes = p.ws_inner;
  const int rc = paged_prefill(c);
  if (rc != MOJO_OK) return rc;
  note_launch(swa ? "gather:kv8:swa+%s" : "gather:kv8+%s", "prefill");
  return MOJO_OK;
}

extern "C" int64_t mojo_hip_paged_prefill_gqa_kv8_workspace_bytes(int64_t total_tokens, int64_t batch, int64_t q_heads,
                                                                  int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                                                  int64_t max_blocks_per_seq, int64_t max_q_len_hint,
                                                                  int64_t max_kv_len_hint) {
  if (total_tokens <= 0 || batch <= 0 || q_heads <= 0 || kv_heads <= 0 || q_heads % kv_heads) return 0;
  mojo::PrefillGeom inner;
  return mojo::prefill_kv8_plan({total_tokens, batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_q_len_hint,
                                 max_kv_len_hint}, inner).total;
}

extern "C" int64_t mojo_hip_paged_prefill_swa_kv8_workspace_bytes(int64_t total_tokens, int64_t batch, int64_t q_heads,
                                                                  int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                                                  int64_t max_blocks_per_seq, int64_t max_q_len_hint,
                                                                  int64_t max_kv_len_hint, int64_t local_window,
                                                                  int64_t global_window) {
  if (total_tokens <= 0 || batch <= 0 || q_heads <= 0 || kv_heads <= 0 || q_heads % kv_heads) return 0;
  if (local_window < 0 && global_window <= 0) { local_window = -1; global_window = 0; }
  mojo::PrefillGeom inner;
  return mojo::prefill_kv8_plan({total_tokens, batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_q_len_hint,
                                 max_kv_len_hint, local_window, global_window}, inner).total;
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
  return paged_prefill_kv8(query, key_cache, key_scale, value_cache, value_scale, cu_q_lens, cu_total_seq_lens, block_tables, out,
                           total_tokens, batch, q_heads, kv_heads, head_dim, num_blocks, block_size, max_blocks_per_seq,
                           block_table_stride, cache_block_stride, cache_head_stride, cache_token_stride, max_q_len_hint,
                           max_kv_len_hint, softmax_scale, layout_abab, dtype, scale_dtype, workspace, workspace_bytes, -1, 0, stream);
}

extern "C" int mojo_hip_paged_prefill_swa_kv8(const void* query, const void* key_cache, const void* key_scale,
                                              const void* value_cache, const void* value_scale, const int32_t* cu_q_lens,
                                              const int32_t* cu_total_seq_lens, const int32_t* block_tables, void* out,
                                              int64_t total_tokens, int64_t batch, int64_t q_heads, int64_t kv_heads,
                                              int64_t head_dim, int64_t num_blocks, int64_t block_size,
                                              int64_t max_blocks_per_seq, int64_t block_table_stride,
                                              int64_t cache_block_stride, int64_t cache_head_stride,
                                              int64_t cache_token_stride, int64_t max_q_len_hint, int64_t max_kv_len_hint,
                                              float softmax_scale, int layout_abab, int dtype, int scale_dtype,
                                              void* workspace, int64_t workspace_bytes, int64_t local_window,
                                              int64_t global_window, mojo_stream_t stream) {
  return paged_prefill_kv8(query, key_cache, key_scale, value_cache, value_scale, cu_q_lens, cu_total_seq_lens, block_tables, out,
                           total_tokens, batch, q_heads, kv_heads, head_dim, num_blocks, block_size, max_blocks_per_seq,
                           block_table_stride, cache_block_stride, cache_head_stride, cache_token_stride, max_q_len_hint,
                           max_kv_len_hint, softmax_scale, layout_abab, dtype, scale_dtype, workspace, workspace_bytes, local_window,
                           global_window, stream);
}
