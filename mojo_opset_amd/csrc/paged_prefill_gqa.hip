// MojoPagedPrefillGQA / MojoPagedPrefillSWA — the C entry points of the paged prefill and its paged kernel instances.  The
// kernels, the launch chain and the plan are paged_prefill_body.h (shared with swa_packed.hip, which instantiates the linear
// forms); the int8-cache entry points follow at the end (paged_prefill_kv8.h).
#include "paged_prefill_body.h"

using namespace mojo;

static int paged_prefill(const PrefillCall& c) {
  if (c.g.total_tokens == 0) return MOJO_OK;
  const PrefillPlan p = prefill_plan(c.g);               // (p.swa: a call without a window is the GQA op itself)
  return !p.swa ? paged_prefill_planned<false>(c, p) : paged_prefill_planned<true>(c, p);
}

extern "C" int64_t mojo_hip_paged_prefill_gqa_workspace_bytes(int64_t total_tokens, int64_t batch, int64_t q_heads,
                                                              int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                                              int64_t max_blocks_per_seq, int64_t max_q_len_hint,
                                                              int64_t max_kv_len_hint) {
  return prefill_plan({total_tokens, batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_q_len_hint,
                       max_kv_len_hint}).query_bytes;
}

extern "C" int64_t mojo_hip_paged_prefill_swa_workspace_bytes(int64_t total_tokens, int64_t batch, int64_t q_heads,
                                                              int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                                              int64_t max_blocks_per_seq, int64_t max_q_len_hint,
                                                              int64_t max_kv_len_hint, int64_t local_window,
                                                              int64_t global_window) {
  return prefill_plan({total_tokens, batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_q_len_hint,
                       max_kv_len_hint, local_window, global_window}).query_bytes;
}

extern "C" int mojo_hip_paged_prefill_gqa(const void* query, const void* key_cache, const void* value_cache,
                                          const int32_t* cu_q_lens, const int32_t* cu_total_seq_lens,
                                          const int32_t* block_tables, void* out, int64_t total_tokens, int64_t batch,
                                          int64_t q_heads, int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                          int64_t max_blocks_per_seq, int64_t block_table_stride,
                                          int64_t cache_block_stride, int64_t cache_head_stride,
                                          int64_t cache_token_stride, int64_t max_q_len_hint, int64_t max_kv_len_hint,
                                          float softmax_scale, int layout_abab, int dtype, void* workspace,
                                          int64_t workspace_bytes, mojo_stream_t stream) {
  PrefillCall c;
  c.query = query; c.key_cache = key_cache; c.value_cache = value_cache; c.cu_q_lens = cu_q_lens; c.cu_total_seq_lens = cu_total_seq_lens;
  c.block_tables = block_tables; c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.g = {total_tokens, batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_q_len_hint, max_kv_len_hint};
  c.block_table_stride = block_table_stride; c.cache_block_stride = cache_block_stride; c.cache_head_stride = cache_head_stride;
  c.cache_token_stride = cache_token_stride; c.softmax_scale = softmax_scale; c.layout_abab = layout_abab; c.dtype = dtype;
  return paged_prefill(c);
}

extern "C" int mojo_hip_paged_prefill_swa(const void* query, const void* key_cache, const void* value_cache,
                                          const int32_t* cu_q_lens, const int32_t* cu_total_seq_lens,
                                          const int32_t* block_tables, void* out, int64_t total_tokens, int64_t batch,
                                          int64_t q_heads, int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                          int64_t max_blocks_per_seq, int64_t block_table_stride,
                                          int64_t cache_block_stride, int64_t cache_head_stride,
                                          int64_t cache_token_stride, int64_t max_q_len_hint, int64_t max_kv_len_hint,
                                          float softmax_scale, int layout_abab, int dtype, void* workspace,
                                          int64_t workspace_bytes, int64_t local_window, int64_t global_window,
                                          mojo_stream_t stream) {
  PrefillCall c;
  c.query = query; c.key_cache = key_cache; c.value_cache = value_cache; c.cu_q_lens = cu_q_lens; c.cu_total_seq_lens = cu_total_seq_lens;
  c.block_tables = block_tables; c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.g = {total_tokens, batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_q_len_hint, max_kv_len_hint,
         local_window, global_window};
  c.block_table_stride = block_table_stride; c.cache_block_stride = cache_block_stride; c.cache_head_stride = cache_head_stride;
  c.cache_token_stride = cache_token_stride; c.softmax_scale = softmax_scale; c.layout_abab = layout_abab; c.dtype = dtype;
  return paged_prefill(c);
}

#if defined(PF_STAMPS) || defined(PF_WG_STAMPS)
extern "C" int mojo_hip_debug_prefill_stamps(unsigned* host_out, int64_t count) {
  if (hipDeviceSynchronize() != hipSuccess) return MOJO_ELAUNCH;
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(mojo::g_pf_stamps), static_cast<size_t>(count) * 4) == hipSuccess ? MOJO_OK : MOJO_ELAUNCH;
}
#endif

#include "paged_prefill_kv8.h"
