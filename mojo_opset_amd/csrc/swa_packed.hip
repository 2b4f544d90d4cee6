// MojoSWA — packed var-len attention over CONTIGUOUS K/V (the attention of a first prefill: K and V have just left the QKV
// projection and sit in one buffer).  The LINEAR instances of prefill_kernel (paged_prefill_body.h): the tile loop, online
// softmax, windowed walk, key split + merge and zero fill of the paged prefill, with the key rows addressed by arithmetic
// (base + (cu_total_seq_lens[b] + key) * token stride) where the paged op walks a block table.  No window: plain causal
// var-len flash attention (the un-windowed instances).
//
// A translation unit of its own so that the linear instances (as many as the paged ones) compile beside them.
// (The in-kernel stamps of -DPF_STAMPS / -DPF_WG_STAMPS are a timing tool of paged_prefill_gqa.hip, which owns their buffer and
// its read-out: this unit is built without them.)
#undef PF_STAMPS
#undef PF_WG_STAMPS
#include "paged_prefill_body.h"

using namespace mojo;

static PrefillGeom swa_packed_geom(int64_t total_q_tokens, int64_t total_kv_tokens, int64_t batch, int64_t q_heads,
                                   int64_t kv_heads, int64_t head_dim, int64_t max_q_len_hint, int64_t max_kv_len_hint,
                                   int64_t local_window, int64_t global_window) {
  PrefillGeom g;
  g.total_tokens = total_q_tokens; g.batch = batch; g.q_heads = q_heads; g.kv_heads = kv_heads; g.head_dim = head_dim;
  g.max_q_hint = max_q_len_hint; g.max_kv_hint = max_kv_len_hint; g.local_window = local_window; g.global_window = global_window;
  g.total_kv_tokens = total_kv_tokens < 0 ? 0 : total_kv_tokens;   // sizes the key split: min(max_kv_len_hint, Tk)
  g.page = PF_KEYS;                                                // (never read by a linear instance; keeps the shared checks defined)
  return g;
}

extern "C" int64_t mojo_hip_swa_packed_workspace_bytes(int64_t total_q_tokens, int64_t total_kv_tokens, int64_t batch,
                                                       int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                                                       int64_t max_q_len_hint, int64_t max_kv_len_hint,
                                                       int64_t local_window, int64_t global_window) {
  return prefill_plan(swa_packed_geom(total_q_tokens, total_kv_tokens, batch, q_heads, kv_heads, head_dim, max_q_len_hint,
                                      max_kv_len_hint, local_window, global_window)).query_bytes;
}

extern "C" int mojo_hip_swa_packed(const void* query, const void* key, const void* value, const int32_t* cu_q_lens,
                                   const int32_t* cu_total_seq_lens, void* out, int64_t total_q_tokens,
                                   int64_t total_kv_tokens, int64_t batch, int64_t q_heads, int64_t kv_heads,
                                   int64_t head_dim, int64_t kv_token_stride, int64_t kv_head_stride,
                                   int64_t max_q_len_hint, int64_t max_kv_len_hint, float softmax_scale, int layout_abab,
                                   int dtype, void* workspace, int64_t workspace_bytes, int64_t local_window,
                                   int64_t global_window, mojo_stream_t stream) {
  if (total_q_tokens == 0) return MOJO_OK;
  PrefillCall c;
  c.query = query; c.key_cache = key; c.value_cache = value; c.cu_q_lens = cu_q_lens; c.cu_total_seq_lens = cu_total_seq_lens;
  c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.g = swa_packed_geom(total_q_tokens, total_kv_tokens, batch, q_heads, kv_heads, head_dim, max_q_len_hint, max_kv_len_hint,
                        local_window, global_window);
  c.cache_token_stride = kv_token_stride; c.cache_head_stride = kv_head_stride;
  c.softmax_scale = softmax_scale; c.layout_abab = layout_abab; c.dtype = dtype;
  const PrefillPlan p = prefill_plan(c.g);               // (p.swa: a call without a window runs the un-windowed instances)
  return !p.swa ? paged_prefill_planned<false, true>(c, p) : paged_prefill_planned<true, true>(c, p);
}
