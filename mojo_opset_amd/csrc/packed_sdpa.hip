// MojoPackedSdpa — packed var-len BIDIRECTIONAL attention over contiguous K/V (the attention of a vision tower: every sequence
// is one image or one window, and every query row of a sequence sees every key of it).  The NODIAG instances of prefill_kernel
// (paged_prefill_body.h): the arguments of MojoSWA's linear instances — cu_q_lens / cu_total_seq_lens, key rows addressed by
// arithmetic, the clamp of cu_total_seq_lens to [0, Tk], zero fill of the rows no sequence owns and of the rows past the
// max_q_len hint, key split + merge — and the walk of MojoSdpa's: no offset, every whole key tile in the unmasked fast-staged
// loop, only the tail tile masked (key >= kv_len).  q_len and kv_len of a sequence are independent; kv_len < q_len is legal.
//
// A translation unit of its own so that its instances compile beside the paged, the packed causal and the strided ones.
#undef PF_STAMPS
#undef PF_WG_STAMPS
#include "paged_prefill_body.h"

using namespace mojo;

static PrefillGeom packed_sdpa_geom(int64_t total_q_tokens, int64_t total_kv_tokens, int64_t batch, int64_t q_heads,
                                    int64_t kv_heads, int64_t head_dim, int64_t max_q_len_hint, int64_t max_kv_len_hint) {
  PrefillGeom g;
  g.total_tokens = total_q_tokens; g.batch = batch; g.q_heads = q_heads; g.kv_heads = kv_heads; g.head_dim = head_dim;
  g.max_q_hint = max_q_len_hint; g.max_kv_hint = max_kv_len_hint;
  g.total_kv_tokens = total_kv_tokens < 0 ? 0 : total_kv_tokens;   // sizes the key split: min(max_kv_len_hint, Tk)
  g.page = PF_KEYS;                                                // (never read by a linear instance; keeps the shared checks defined)
  return g;
}

extern "C" int64_t mojo_hip_packed_sdpa_workspace_bytes(int64_t total_q_tokens, int64_t total_kv_tokens, int64_t batch,
                                                        int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                                                        int64_t max_q_len_hint, int64_t max_kv_len_hint) {
  return prefill_plan(packed_sdpa_geom(total_q_tokens, total_kv_tokens, batch, q_heads, kv_heads, head_dim, max_q_len_hint,
                                       max_kv_len_hint)).query_bytes;
}

extern "C" int mojo_hip_packed_sdpa(const void* query, const void* key, const void* value, const int32_t* cu_q_lens,
                                    const int32_t* cu_total_seq_lens, void* out, int64_t total_q_tokens,
                                    int64_t total_kv_tokens, int64_t batch, int64_t q_heads, int64_t kv_heads,
                                    int64_t head_dim, int64_t kv_token_stride, int64_t kv_head_stride,
                                    int64_t max_q_len_hint, int64_t max_kv_len_hint, float softmax_scale, int layout_abab,
                                    int dtype, void* workspace, int64_t workspace_bytes, mojo_stream_t stream) {
  if (total_q_tokens == 0) return MOJO_OK;
  PrefillCall c;
  c.query = query; c.key_cache = key; c.value_cache = value; c.cu_q_lens = cu_q_lens; c.cu_total_seq_lens = cu_total_seq_lens;
  c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.g = packed_sdpa_geom(total_q_tokens, total_kv_tokens, batch, q_heads, kv_heads, head_dim, max_q_len_hint, max_kv_len_hint);
  c.cache_token_stride = kv_token_stride; c.cache_head_stride = kv_head_stride;
  c.softmax_scale = softmax_scale; c.layout_abab = layout_abab; c.dtype = dtype;
  return paged_prefill_planned<false, true, true>(c, prefill_plan(c.g));
}
