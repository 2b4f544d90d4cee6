/* mojo_hip.h — C ABI of libmojo_hip.so, the MI355X (gfx950) kernel library behind the
 * `HIP<Op>` backend classes of mojo_opset_amd.
 *
 * The reference (XPU-Forces/mojo_opset) has no native code: each accelerated backend class
 * (e.g. `TTXPagedDecodeGQA.forward`, mojo_opset/backends/ttx/operators/attention.py:143-176)
 * calls a Python kernel launcher.  Every entry point below replaces one such launcher call; the
 * comment above it names the reference operator (golden `forward`) whose semantics it implements
 * and the accelerated call site it stands in for.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in `_host`;
 *   - shapes/strides are int64 in ELEMENTS; the innermost dimension is always contiguous;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued, never synchronised;
 *   - no allocation, no host sync, re-entrant; scratch comes from the caller (`workspace`);
 *   - return 0 on success, a negative MOJO_E* code otherwise; `mojo_hip_last_error()` returns a
 *     thread-local message for the last failure on the calling thread.
 */
#ifndef MOJO_HIP_H
#define MOJO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mojo_stream_t;

enum mojo_dtype { MOJO_F32 = 0, MOJO_F16 = 1, MOJO_BF16 = 2, MOJO_I8 = 3, MOJO_F8E4M3 = 4,
                  MOJO_I32 = 5 /* int32 GEMM accumulators: mojo_hip_dequant_swiglu_quant only */ };

enum mojo_status {
  MOJO_OK = 0,
  MOJO_EINVAL = -1,        /* malformed arguments (-> AssertionError / ValueError in the shim) */
  MOJO_EUNSUPPORTED = -2,  /* legal but not implemented for this shape/dtype (-> NotImplementedError) */
  MOJO_ELAUNCH = -3,       /* HIP launch failure (-> RuntimeError) */
  MOJO_EWORKSPACE = -4     /* workspace too small (-> RuntimeError) */
};

const char* mojo_hip_version(void);
const char* mojo_hip_last_error(void);

/* ---- Run-time switches (MOJO_HIP_* environment variables; the table is INTEGRATION.md section 5).  The reference reads its
 *      switches where it uses them (`MOJO_BACKEND` in `MojoOperator.__new__`, core/operator.py:45-47); a native library
 *      cannot afford getenv() per launch, so every switch is LATCHED the first time a launcher reads it and
 *      `mojo_hip_reload_env()` drops all latched values (the next call re-reads the environment).  Call it after changing a
 *      variable, with no operator call in flight.  `mojo_hip_switches()` writes "NAME=value" (space-separated, "NAME=" when
 *      unset) for every switch read so far into `buf` and returns their count.  `mojo_hip_last_launch()`: a short description
 *      of the kernel form the calling thread's last operator call launched ("decode_mfma:paired:nt", "gemm256:staged:KN",
 *      ...) — a debug / test query with which an A/B test proves that its two legs took different forms;
 *      `mojo_hip_launch_history(clear)`: the same notes of every launch of this thread since the last clear, '|'-separated
 *      (a composite operator — absorb projection, latent attention, output projection — leaves several).               */
void mojo_hip_reload_env(void);
int64_t mojo_hip_switches(char* buf, int64_t capacity);
const char* mojo_hip_last_launch(void);
const char* mojo_hip_launch_history(int clear);

/* ---- MojoStorePagedKVCache (core/operators/kv_cache.py:104-171; replaces store_paged_kv(),
 *      backends/ttx/operators/kv_cache.py:40-46).  Bit-exact copy, token-major -> head-major.
 *      plan rows = (src_token_start, dst_block_id, dst_block_offset, chunk_len) int32.          */
int mojo_hip_store_paged_kv_plan(const void* key_states, const void* value_states,
                                 void* key_cache, void* value_cache,
                                 const int32_t* plan, int64_t num_chunks,
                                 int64_t num_tokens, int64_t num_kv_heads, int64_t head_dim,
                                 int64_t num_blocks, int64_t block_size, int64_t elt_bytes,
                                 int64_t src_token_stride, int64_t src_head_stride,
                                 int64_t cache_block_stride, int64_t cache_head_stride,
                                 int64_t cache_token_stride, mojo_stream_t stream);

/*      Same op, legacy arguments (block_table, cu_q_lens|NULL, context_kv_lens): the plan of
 *      build_paged_kv_chunk_metadata (kv_cache.py:33-101) is evaluated per token on the device, so
 *      there is no host sync.  cu_q_lens == NULL selects decode mode (one token per sequence).  */
int mojo_hip_store_paged_kv_layout(const void* key_states, const void* value_states,
                                   void* key_cache, void* value_cache,
                                   const int32_t* block_table, int64_t block_table_stride,
                                   int64_t max_blocks_per_seq,
                                   const int32_t* cu_q_lens, const int32_t* context_kv_lens,
                                   int64_t batch, int64_t num_tokens, int64_t num_kv_heads,
                                   int64_t head_dim, int64_t num_blocks, int64_t block_size,
                                   int64_t elt_bytes, int64_t src_token_stride,
                                   int64_t src_head_stride, int64_t cache_block_stride,
                                   int64_t cache_head_stride, int64_t cache_token_stride,
                                   mojo_stream_t stream);

/* ---- MojoSwiGLU (core/operators/activation.py:38-66; replaces swiglu_fwd,
 *      backends/ttx/operators/activation.py).  Flat contiguous tensors of n elements.           */
int mojo_hip_swiglu(const void* gate, const void* up, void* out, int64_t n, int dtype,
                    float swiglu_limit, mojo_stream_t stream);
/*      Row-strided form: gate / up / out are [rows, cols] views with row strides in elements (the two halves of a fused
 *      [rows, 2*cols] projection, core/operators/moe.py:441-445).                                              */
int mojo_hip_swiglu_rows(const void* gate, const void* up, void* out, int64_t rows, int64_t cols,
                         int64_t ld_gate, int64_t ld_up, int64_t ld_out, int dtype, float swiglu_limit,
                         mojo_stream_t stream);

/* ---- MojoResidualAddRMSNorm / MojoRMSNorm (core/operators/normalization.py:308-362, :71-111;
 *      replaces fused_add_rmsnorm / rmsnorm launchers, backends/ttx/operators/normalization.py:35-47).
 *      residual == NULL: plain RMSNorm.  sum_out may be NULL (norm_pos="post").
 *      sum = round_dtype(hidden + residual); normed = round_dtype(sum * rsqrt(mean(sum^2)+eps) * w).
 *      normed_out may be the same buffer as hidden: MojoRMSNormInplace(inplace=True)
 *      (experimental/operators/normalization.py:95-140).                                            */
int mojo_hip_residual_add_rmsnorm(const void* hidden, const void* residual, const void* weight,
                                  void* normed_out, void* sum_out, int64_t rows, int64_t dim,
                                  int dtype, float eps, mojo_stream_t stream);

/* ---- MojoApplyRoPE (core/operators/position_embedding.py:98-175; replaces rope_fwd,
 *      backends/ttx/operators/position_embedding.py).  q/k are addressed as [B][T][N][D] through
 *      explicit strides (so head-first and token-first layouts are read in place); cos/sin are
 *      fp32 [.., rope_dim] addressed as [B][T] with strides (cos_b_stride may be 0).             */
int mojo_hip_apply_rope(const void* q, const void* k, void* q_out, void* k_out,
                        const float* cos, const float* sin,
                        int64_t batch, int64_t tokens, int64_t q_heads, int64_t k_heads,
                        int64_t head_dim, int64_t rope_dim,
                        const int64_t q_strides[3], const int64_t k_strides[3],
                        const int64_t qo_strides[3], const int64_t ko_strides[3],
                        int64_t cos_b_stride, int64_t cos_t_stride, int dtype,
                        mojo_stream_t stream);

/* ---- Block allocator of the paged KV cache (replaces the host loop of PagedDummyCache.update,
 *      modeling/qwen3/mojo_qwen3_dense.py:84-123: `.item()` per sequence + Python slices of the free list).
 *      extend: every sequence i with seq_lens[i] >= 0 and new_i > 0 (new_lens[i], or new_len_uniform when new_lens is NULL)
 *      gains ceil((len+new)/page) - ceil(len/page) blocks, taken from the END of free_blocks[0 .. num_free) sequence by
 *      sequence, written to block_table[i, ceil(len/page) ...] — the tables the reference would build, entry for entry.
 *      pool_state int32[4] = {num_free, error, high-water of used blocks, 0}; when the blocks (error 1) or the table
 *      columns (error 2) do not suffice the launch changes nothing and sets `error` (sticky; the host resets it).
 *      store_ctx_out (nullable, int32 [batch]) receives the `context_kv_lens` the KV store must be called with: the
 *      row's length before the append, or -1 (= skip, kv_cache.py:56-74) for rows that append nothing / a refused launch.
 *      advance: seq_lens[i] += new_i for the same rows (no-op while `error` is set).  No host sync: capturable.        */
int mojo_hip_page_pool_extend(int32_t* block_table, int64_t block_table_stride, int64_t max_blocks_per_seq,
                              const int32_t* seq_lens, const int32_t* new_lens, int64_t new_len_uniform,
                              const int32_t* free_blocks, int32_t* pool_state, int32_t* store_ctx_out,
                              int64_t batch, int64_t block_size, int64_t total_blocks,
                              mojo_stream_t stream);
int mojo_hip_page_pool_advance(int32_t* seq_lens, const int32_t* new_lens, int64_t new_len_uniform,
                               const int32_t* pool_state, int64_t batch, mojo_stream_t stream);

/* ---- MojoRotaryEmbedding (core/operators/position_embedding.py:9-95; replaces rot_pos_embed,
 *      backends/ttx/kernels/ilu/rope.py:634-675 — a host loop with .item() per sequence).
 *      mode 0: positions = position_ids[i];  mode 1: positions = i (padded prefill);
 *      mode 2: positions from cu_q_lens (+ total_seq_lens or NULL), tokens outside every
 *              sequence get position -1 (python-style: last table row / angle -inv_freq).
 *      cos_table/sin_table == NULL: compute cos/sin(pos * inv_freq) * scaling on the fly.        */
int mojo_hip_rotary_embedding(float* cos_out, float* sin_out, int64_t n_pos, int64_t rope_dim,
                              int mode, const int32_t* position_ids, const int32_t* cu_q_lens,
                              const int32_t* total_seq_lens, int64_t batch,
                              const float* cos_table, const float* sin_table, int64_t table_len,
                              const float* inv_freq, float attention_scaling,
                              mojo_stream_t stream);

/* ---- MojoPagedDecodeGQA (core/operators/attention.py:113-232; replaces paged_attention_decode,
 *      backends/ttx/operators/attention.py:166-174).  Split-KV flash decoding; the q-heads of one
 *      kv-head share every K/V load.  layout_abab: 0 = "AABB", 1 = "ABAB".
 *      max_seq_len_hint <= 0: derive the split count from max_blocks_per_seq * block_size.  Lengths above
 *      min(hint, block_size * max_blocks_per_seq) are truncated to that capacity (nothing is indexed past what
 *      the launch was sized for).  leave_empty_rows: 0 = rows with total_seq_lens <= 0 are written as zeros (the
 *      eager golden, attention.py:184-185); 1 = such rows of `out` are left untouched — the graph-replay contract
 *      of padded rows (tests/accuracy/operators/test_attention.py:318-353; the reference's ILU kernel switches on
 *      `not is_current_stream_capturing()`, backends/ttx/kernels/ilu/flash_attention.py:816,425-428).             */
int64_t mojo_hip_paged_decode_gqa_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                  int64_t head_dim, int64_t block_size,
                                                  int64_t max_blocks_per_seq,
                                                  int64_t max_seq_len_hint);
int mojo_hip_paged_decode_gqa(const void* query, const void* key_cache, const void* value_cache,
                              const int32_t* total_seq_lens, const int32_t* block_tables,
                              void* out, void* workspace, int64_t workspace_bytes,
                              int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                              int64_t block_size, int64_t max_blocks_per_seq,
                              int64_t block_table_stride, int64_t cache_block_stride,
                              int64_t cache_head_stride, int64_t cache_token_stride,
                              int64_t max_seq_len_hint, float softmax_scale, int layout_abab,
                              int leave_empty_rows, int dtype, mojo_stream_t stream);

/* ---- MojoGroupGemm (core/operators/gemm.py:59-124; replaces m_grouped_matmul,
 *      backends/ttx/operators/gemm.py:51-92).  out[rows of g] = input[rows of g] @ W[g];
 *      group_list = per-group ROW COUNTS on the device (int32, or int64 when group_list_is_i64);
 *      offsets are prefix-summed on the device (no host sync, graph-capturable).
 *      trans_weight = 0: weight [G,K,N];  1: weight [G,N,K].  bf16/fp16 with K % 64 == 0 run on the
 *      MFMA kernel, everything else (fp32, odd K/N) on a generic kernel.                            */
int64_t mojo_hip_group_gemm_workspace_bytes(int64_t num_groups);
int mojo_hip_group_gemm(const void* input, const void* weight, void* out, const void* group_list,
                        int group_list_is_i64, int64_t m_total, int64_t k, int64_t n,
                        int64_t num_groups, int trans_weight, int dtype, void* workspace,
                        int64_t workspace_bytes, mojo_stream_t stream);

/*      MojoExperts' first projection with the SwiGLU fused into the epilogue (mojo_opset/core/operators/moe.py:402-449:
 *      GroupGemm -> SwiGLU -> GroupGemm): weight [G, 2*inter, K] (trans_weight) or [G, K, 2*inter], columns [gate | up];
 *      out [m_total, inter] = round(round(silu(round(gate))) * round(up)) — the roundings of the two-op golden path — so
 *      the [m_total, 2*inter] product never goes to HBM.  bf16 / fp16, inter % 128 == 0 and the 256x256 MFMA kernel's
 *      layout preconditions; MOJO_EUNSUPPORTED otherwise — and where the library's time model prefers the unfused route (the
 *      product on 128-row tiles: few small experts, groups of about a hundred rows) — callers fall back to group_gemm +
 *      swiglu_rows (same bits).                                                                                         */
int mojo_hip_group_gemm_swiglu(const void* input, const void* weight, void* out, const void* group_list,
                               int group_list_is_i64, int64_t m_total, int64_t k, int64_t inter,
                               int64_t num_groups, int trans_weight, int dtype, void* workspace,
                               int64_t workspace_bytes, mojo_stream_t stream);

/*      Same kernel with explicit strides (elements): input row stride lda, output row stride ldc, weight
 *      element (g,k,n) at weight + g*w_group_stride + k*w_k_stride + n*w_n_stride, and optional row maps
 *      {rc, ml, off, mul} (NULL = identity): logical row m reads input row (m/rc)*ml + off + (m%rc)*mul and
 *      writes the output row given by c_map.  Used by the MLA ops to multiply by the two halves of kv_b_proj in
 *      place, one group per head, reading/writing token-major [T,H,*] tensors directly (rc=T, ml=1, mul=H).
 *      group_list == NULL means num_groups equal groups of m_total / num_groups rows (no prefix pass).      */
int mojo_hip_group_gemm_strided(const void* input, const void* weight, void* out, const void* group_list,
                                int group_list_is_i64, int64_t m_total, int64_t k, int64_t n,
                                int64_t num_groups, int64_t lda, int64_t ldc, int64_t w_group_stride,
                                int64_t w_k_stride, int64_t w_n_stride, const int64_t a_map[4],
                                const int64_t c_map[4], int dtype, void* workspace,
                                int64_t workspace_bytes, mojo_stream_t stream);

/* ---- MojoPagedDecodeMLA / MojoPagedPrefillMLA (experimental/operators/attention.py:131-227, :325-447; the
 *      reference has no accelerated kernel for either).  Attention over the COMPRESSED cache in the
 *      weight-absorbed form: q_lat [Tq,H,r(+rope)] = [q_nope @ W_kn (| q_rope)], o_lat [Tq,H,r] = sum_s p c_kv[s].
 *      q_lat rows are q_lat_stride elements apart; the rope part is read from q_rope (row stride q_rope_stride)
 *      when q_rope != NULL, else from q_lat columns r.. .
 *      decode : total_seq_lens != NULL, cu_q_lens == NULL, Tq == batch (one token per sequence)
 *      prefill: cu_q_lens != NULL (cu_total_seq_lens optional), token t sees keys 0 .. kv_len-q_len+t
 *      attn_sink: optional fp32 [H] extra softmax logit (probability mass only).                           */
int64_t mojo_hip_mla_latent_attn_workspace_bytes(int64_t q_tokens, int64_t heads, int64_t kv_lora_rank,
                                                 int64_t max_kv_len);
int mojo_hip_mla_latent_attn(const void* q_lat, int64_t q_lat_stride, const void* q_rope, int64_t q_rope_stride,
                             const void* ckv_cache, const void* kpe_cache,
                             const int32_t* total_seq_lens, const int32_t* cu_q_lens,
                             const int32_t* cu_total_seq_lens, const int32_t* block_tables,
                             const float* attn_sink, void* o_lat, void* workspace,
                             int64_t workspace_bytes, int64_t q_tokens, int64_t batch, int64_t heads,
                             int64_t kv_lora_rank, int64_t rope_dim, int64_t block_size,
                             int64_t max_blocks_per_seq, int64_t block_table_stride,
                             int64_t ckv_block_stride, int64_t ckv_token_stride,
                             int64_t kpe_block_stride, int64_t kpe_token_stride, int64_t max_kv_len,
                             float softmax_scale, int dtype, mojo_stream_t stream);

/* ---- dense GEMM used by the GEMM+collective operators (core/operators/compute_with_comm.py:12-24,
 *      `_gemm`): out[M,N] = input[M,K] @ W (+ bias).  W element (k,n) at weight + k*w_k_stride +
 *      n*w_n_stride (one of the two strides is 1).  bias (optional, [N]) is added after the product
 *      has been rounded to the storage type, as the golden's two separate ops do.  Decode-sized M with
 *      K-major weights streams the weight (gemm_skinny.hip), cut along K into fp32 slabs in the workspace
 *      when there are few column tiles (slabs summed in fixed order).                                    */
int64_t mojo_hip_gemm_workspace_bytes(int64_t m, int64_t k, int64_t n);
int mojo_hip_gemm(const void* input, const void* weight, const void* bias, void* out, int64_t m,
                  int64_t k, int64_t n, int64_t lda, int64_t ldc, int64_t w_k_stride,
                  int64_t w_n_stride, int dtype, void* workspace, int64_t workspace_bytes,
                  mojo_stream_t stream);

/*      Decode-sized fusions of a decoder layer's dense chain (the op sequence of core/operators/moe.py:402-449 and of
 *      modeling/*: linear -> MojoSwiGLU, linear -> MojoResidualAddRMSNorm).  Results are bit-identical to the separate
 *      calls (mojo_hip_gemm, mojo_hip_swiglu_rows, mojo_hip_residual_add_rmsnorm): the fused kernels round where
 *      those round (gemm_swiglu never cuts K; where the separate projection would, the fp32 sums differ in order).
 *      gemm_swiglu: weight = [gate | up] rows, [2*inter, k] K-major (row stride w_n_stride); out [m, inter] =
 *      silu(x @ gate^T) * (x @ up^T).  m <= 64: ONE launch, wave units dealt evenly over the CUs; otherwise the
 *      product goes through the workspace.                                                                        */
int64_t mojo_hip_gemm_swiglu_workspace_bytes(int64_t m, int64_t k, int64_t inter);
int mojo_hip_gemm_swiglu(const void* input, const void* weight, void* out, int64_t m, int64_t k,
                         int64_t inter, int64_t lda, int64_t ldc, int64_t w_n_stride, int dtype,
                         void* workspace, int64_t workspace_bytes, mojo_stream_t stream);
/*      gemm_residual_rmsnorm: normed_out = RMSNorm(x @ W (+ bias) + residual) * norm_weight, sum_out (may be NULL) =
 *      the sum, gemm_out (may be NULL) = the product.  With a K split (decode-sized m, few column tiles) the
 *      fp32 K-slice slabs are summed by the norm kernel itself: the product makes no round trip through HBM.      */
int64_t mojo_hip_gemm_residual_rmsnorm_workspace_bytes(int64_t m, int64_t k, int64_t n);
int mojo_hip_gemm_residual_rmsnorm(const void* input, const void* weight, const void* bias,
                                   const void* residual, const void* norm_weight, void* normed_out,
                                   void* sum_out, void* gemm_out, int64_t m, int64_t k, int64_t n,
                                   int64_t lda, int64_t w_k_stride, int64_t w_n_stride, int dtype,
                                   float eps, void* workspace, int64_t workspace_bytes,
                                   mojo_stream_t stream);

/*      qkv_rope_store: one decode step's fused QKV projection (weight [(Hq + 2 Hkv) * D, k] K-major, heads in q | k | v
 *      order) -> MojoApplyRoPE on q and k (rotate-half over the whole head; cos / sin fp32 [batch, D], one row per
 *      sequence: core/operators/position_embedding.py) -> q_out [batch, Hq, D] -> MojoStorePagedKVCache in decode mode
 *      (one token per sequence at position context_kv_lens[b]; kv_cache.py:33-101).  With a K split the slice sums are
 *      taken by the kernel that rotates and stores: two launches for the chain's five.  Same bits as the separate calls. */
int64_t mojo_hip_qkv_rope_store_workspace_bytes(int64_t m, int64_t k, int64_t n);
int mojo_hip_qkv_rope_store(const void* input, const void* weight, const void* bias, const float* cos,
                            const float* sin, int64_t cos_sin_row_stride, void* q_out, void* key_cache,
                            void* value_cache, const int32_t* block_table, int64_t block_table_stride,
                            int64_t max_blocks_per_seq, const int32_t* context_kv_lens, int64_t batch,
                            int64_t k, int64_t q_heads, int64_t kv_heads, int64_t head_dim, int64_t lda,
                            int64_t w_n_stride, int64_t num_blocks, int64_t block_size,
                            int64_t cache_block_stride, int64_t cache_head_stride,
                            int64_t cache_token_stride, int dtype, void* workspace,
                            int64_t workspace_bytes, mojo_stream_t stream);

/*      Same with row maps {rc, ml, off} (NULL or rc == 0: identity): logical row m reads A row
 *      (m / rc) * ml + off + m % rc, and likewise for the C row it writes.  One launch can thus consume or
 *      produce the "c-th sub-chunk of every rank" view of the chunked reduce-scatter / all-gather pipelines. */
int mojo_hip_gemm_rowmap(const void* input, const void* weight, const void* bias, void* out, int64_t m,
                         int64_t k, int64_t n, int64_t lda, int64_t ldc, int64_t w_k_stride,
                         int64_t w_n_stride, const int64_t a_map[3], const int64_t c_map[3], int dtype,
                         void* workspace, int64_t workspace_bytes, mojo_stream_t stream);

/* ---- MojoQuantGemm (core/operators/gemm.py:127-231; the reference's accelerated int8 kernel is
 *      backends/ttx/kernels/ilu/int8_gemm.py:18-66).  out = (A_q @ W_q) * input_scale[m] * weight_scale[n]
 *      input [M,K] and weight ([K,N], or [N,K] when trans_weight) are int8 (MOJO_I8) or OCP fp8-e4m3
 *      (MOJO_F8E4M3, an extension: no reference implementation, parity unpinned); input_scale fp32 [M];
 *      weight_scale bf16 [N]; out_dtype in {f32, f16, bf16}.  Decode-sized M is cut along K into slices
 *      whose raw accumulators go to the workspace and are summed in a fixed order (deterministic).          */
int64_t mojo_hip_quant_gemm_workspace_bytes(int64_t m, int64_t k, int64_t n);
int mojo_hip_quant_gemm(const void* input, const void* weight, const float* input_scale,
                        const void* weight_scale, void* out, int64_t m, int64_t k, int64_t n,
                        int trans_weight, int quant_dtype, int out_dtype, void* workspace,
                        int64_t workspace_bytes, mojo_stream_t stream);

/* ---- MojoPagedPrefillGQA (core/operators/attention.py:315-451; replaces paged_attention_prefill,
 *      backends/ttx/operators/attention.py).  Packed var-len queries [T,Hq,D], causal with offset
 *      kv_len - q_len; cu_total_seq_lens may be NULL (kv_len = q_len).  `out` is fully written: rows of
 *      empty sequences / padding tokens are zeroed.  max_q_len_hint <= 0: use total_tokens as the bound.
 *      Launches of few, long blocks (a chunked prefill against a long cache) are cut along the keys: every (query block,
 *      kv head, sequence) workgroup becomes several that walk a slice of its key tiles and leave fp32 partials in the
 *      workspace, combined by a merge kernel in slice order.  workspace_bytes() == 0: the launch is not split (workspace may
 *      be NULL); a workspace that is too small runs the launch unsplit.  max_kv_len_hint <= 0: block_size * max_blocks.   */
int64_t mojo_hip_paged_prefill_gqa_workspace_bytes(int64_t total_tokens, int64_t batch, int64_t q_heads,
                                                   int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                                   int64_t max_blocks_per_seq, int64_t max_q_len_hint,
                                                   int64_t max_kv_len_hint);
int mojo_hip_paged_prefill_gqa(const void* query, const void* key_cache, const void* value_cache,
                               const int32_t* cu_q_lens, const int32_t* cu_total_seq_lens,
                               const int32_t* block_tables, void* out, int64_t total_tokens,
                               int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                               int64_t block_size, int64_t max_blocks_per_seq,
                               int64_t block_table_stride, int64_t cache_block_stride,
                               int64_t cache_head_stride, int64_t cache_token_stride,
                               int64_t max_q_len_hint, int64_t max_kv_len_hint, float softmax_scale,
                               int layout_abab, int dtype, void* workspace, int64_t workspace_bytes,
                               mojo_stream_t stream);

/* ---- MojoPagedDecodeSWA / MojoPagedPrefillSWA (core/operators/attention.py:507-744; replace the TTX backend's
 *      sliding-window kernels, backends/ttx/operators/attention.py:240, :340).  The arguments of the GQA pair plus
 *      local_window (< 0: none) and global_window (<= 0: none).  Query row i of a sequence of q_len queries over kv_len keys
 *      sits at position p = kv_len - q_len + i (decode: p = kv_len - 1) and sees key j iff j <= p and
 *      (j >= p - local_window or j < global_window); with neither window this is the GQA op (these entry points call it).
 *      Only the key tiles of the two ranges are walked and the launch is sized on the visible keys (decode: at most
 *      ceil16(global) + local + 16 per row), so a 4k window over a 32k context moves the bytes of a 4k context.
 *      Pages outside the visible set are never read: their table entries may be -1 or name recycled pages (decode: pages of
 *      the row's window; prefill: of the union of the windows of a sequence's query rows, for pages of >= 16 tokens; smaller
 *      pages may be read at the window edges, and their keys never reach the output).  There is no hole scan: a negative
 *      entry INSIDE the visible set reads page 0.  Everything else — hints, workspace, leave_empty_rows, zeroed rows — is
 *      that of the GQA entry point.                                                                                        */
int64_t mojo_hip_paged_decode_swa_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                  int64_t head_dim, int64_t block_size,
                                                  int64_t max_blocks_per_seq, int64_t max_seq_len_hint,
                                                  int64_t local_window, int64_t global_window);
int mojo_hip_paged_decode_swa(const void* query, const void* key_cache, const void* value_cache,
                              const int32_t* total_seq_lens, const int32_t* block_tables,
                              void* out, void* workspace, int64_t workspace_bytes,
                              int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                              int64_t block_size, int64_t max_blocks_per_seq,
                              int64_t block_table_stride, int64_t cache_block_stride,
                              int64_t cache_head_stride, int64_t cache_token_stride,
                              int64_t max_seq_len_hint, float softmax_scale, int layout_abab,
                              int leave_empty_rows, int dtype, int64_t local_window,
                              int64_t global_window, mojo_stream_t stream);
int64_t mojo_hip_paged_prefill_swa_workspace_bytes(int64_t total_tokens, int64_t batch, int64_t q_heads,
                                                   int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                                   int64_t max_blocks_per_seq, int64_t max_q_len_hint,
                                                   int64_t max_kv_len_hint, int64_t local_window,
                                                   int64_t global_window);
int mojo_hip_paged_prefill_swa(const void* query, const void* key_cache, const void* value_cache,
                               const int32_t* cu_q_lens, const int32_t* cu_total_seq_lens,
                               const int32_t* block_tables, void* out, int64_t total_tokens,
                               int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                               int64_t block_size, int64_t max_blocks_per_seq,
                               int64_t block_table_stride, int64_t cache_block_stride,
                               int64_t cache_head_stride, int64_t cache_token_stride,
                               int64_t max_q_len_hint, int64_t max_kv_len_hint, float softmax_scale,
                               int layout_abab, int dtype, void* workspace, int64_t workspace_bytes,
                               int64_t local_window, int64_t global_window, mojo_stream_t stream);

/* ---- MojoSWA (core/operators/attention.py:747-838): packed var-len queries [total_q_tokens][q_heads][head_dim] against
 *      CONTIGUOUS packed keys and values [total_kv_tokens][kv_heads][head_dim] — no cache, no table.  Sequence b owns query
 *      rows [cu_q_lens[b], cu_q_lens[b+1]) and K/V rows [cu_total_seq_lens[b], cu_total_seq_lens[b+1]); cu_q_lens[0] == 0,
 *      cu_total_seq_lens[0] may be positive, kv_len >= q_len per sequence.  Causal, with the visibility rule and the
 *      windows of mojo_hip_paged_prefill_swa (local_window < 0: none, global_window <= 0: none; neither: plain var-len
 *      flash attention).  key and value share kv_token_stride and kv_head_stride (elements, multiples of 8; head_dim dense;
 *      both bases 16-byte aligned), so views into a fused QKV projection are read in place; offsets are 64-bit.  The kernel
 *      is the paged prefill's with the row of a key computed, not looked up: the same bits as mojo_hip_paged_prefill_gqa /
 *      _swa on the same tokens at the same key split.  Hints, workspace and key split as there, the key capacity being
 *      min(max_kv_len_hint, total_kv_tokens).  Rows of sequences without keys and rows at or past cu_q_lens[batch] are
 *      zeros.  Every cu_total_seq_lens entry is clamped to [0, total_kv_tokens] by the kernel: no read leaves the tensors. */
int64_t mojo_hip_swa_packed_workspace_bytes(int64_t total_q_tokens, int64_t total_kv_tokens, int64_t batch,
                                            int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                                            int64_t max_q_len_hint, int64_t max_kv_len_hint, int64_t local_window,
                                            int64_t global_window);
int mojo_hip_swa_packed(const void* query, const void* key, const void* value, const int32_t* cu_q_lens,
                        const int32_t* cu_total_seq_lens, void* out, int64_t total_q_tokens,
                        int64_t total_kv_tokens, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                        int64_t kv_token_stride, int64_t kv_head_stride, int64_t max_q_len_hint,
                        int64_t max_kv_len_hint, float softmax_scale, int layout_abab, int dtype, void* workspace,
                        int64_t workspace_bytes, int64_t local_window, int64_t global_window, mojo_stream_t stream);

/* ---- MojoSdpa (core/operators/attention.py:456-504): bidirectional scaled-dot-product attention, query [batch][q_heads]
 *      [q_len][head_dim] against key / value [batch][kv_heads][kv_len][head_dim], every row seeing every key; kv_len < q_len is
 *      legal (cross-attention).  All four tensors are addressed by batch / head / token strides in elements (64-bit offsets,
 *      non-negative multiples of 8; head_dim dense; bases 16-byte aligned); key and value share theirs.  q head h reads kv head
 *      h / (q_heads / kv_heads) (the grouping of repeat_interleave).  mask_kind 0: no mask (mask = NULL).  1: boolean mask, one
 *      byte per score, 0 hides the key.  2 / 3: a bias in the query's dtype / fp32, added to the scaled score (-inf allowed).
 *      The mask is read in place as [batch][q_heads][q_len][kv_len] through its strides in elements; any of them may be 0
 *      (a broadcast dimension), the last dimension is dense, and one (batch, head) plane stays below 2^31 elements.  A row
 *      with no visible key stores zeros.  bf16 / fp16, head_dim 64 / 96 / 128, q_heads / kv_heads 1 / 2 / 4 / 8, lengths
 *      below 2^30.  The kernel is the prefill's (mojo_hip_swa_packed) without its diagonal; workspace and key split as there,
 *      sized on kv_len.  kv_len must be positive.  No host sync.                                                            */
int64_t mojo_hip_sdpa_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len, int64_t kv_len,
                                      int64_t head_dim);
int mojo_hip_sdpa(const void* query, const void* key, const void* value, const void* mask, void* out, int64_t batch,
                  int64_t q_heads, int64_t kv_heads, int64_t q_len, int64_t kv_len, int64_t head_dim,
                  int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride, int64_t out_batch_stride,
                  int64_t out_head_stride, int64_t out_token_stride, int64_t kv_batch_stride, int64_t kv_head_stride,
                  int64_t kv_token_stride, int mask_kind, int64_t mask_batch_stride, int64_t mask_head_stride,
                  int64_t mask_row_stride, float softmax_scale, int dtype, void* workspace, int64_t workspace_bytes,
                  mojo_stream_t stream);

/* ---- MojoPagedDecodeNstepSWA (experimental/operators/attention.py:1154-1262): `steps` query rows per sequence (draft
 *      verification, multi-token prediction) in one pass over the paged cache.  The arguments of mojo_hip_paged_decode_swa
 *      plus `steps`; query and out are [batch][steps][q_heads][head_dim] dense, total_seq_lens counts the `steps` new tokens.
 *      Step j sits at position p = len - steps + j and sees key t iff t <= p and (no window, or t >= p - local_window, or
 *      t < global_window).  Rows of length <= 0 are zeros (left untouched with leave_empty_rows); a step with p < 0
 *      (0 < len < steps) sees no key and stores zeros.  With no window negative page ids are holes as in the GQA op (zero
 *      K/V from the first one on); with a window there is no hole scan, as in the SWA op.
 *      steps == 1 IS mojo_hip_paged_decode_swa (same plan, same workspace, bit for bit).  steps > 1 runs on the matrix-core
 *      decode kernel alone: head_dim 64 / 128, power-of-two pages of >= 16 tokens, groups of <= 16 heads, and
 *      MOJO_HIP_DECODE_MFMA != 0.  For every other geometry the workspace query answers -1 and the entry point returns
 *      MOJO_EUNSUPPORTED: the caller composes `steps` single-step calls on lengths len - (steps - 1 - j).                  */
int64_t mojo_hip_paged_decode_nstep_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                    int64_t head_dim, int64_t block_size,
                                                    int64_t max_blocks_per_seq, int64_t max_seq_len_hint,
                                                    int64_t local_window, int64_t global_window, int64_t steps);
int mojo_hip_paged_decode_nstep(const void* query, const void* key_cache, const void* value_cache,
                                const int32_t* total_seq_lens, const int32_t* block_tables,
                                void* out, void* workspace, int64_t workspace_bytes,
                                int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                                int64_t block_size, int64_t max_blocks_per_seq,
                                int64_t block_table_stride, int64_t cache_block_stride,
                                int64_t cache_head_stride, int64_t cache_token_stride,
                                int64_t max_seq_len_hint, float softmax_scale, int layout_abab,
                                int leave_empty_rows, int dtype, int64_t local_window,
                                int64_t global_window, int64_t steps, mojo_stream_t stream);

/* ---- int8 paged KV cache with per-channel scales ("C8"; experimental/operators/kv_cache.py:109-184,
 *      experimental/operators/attention.py:461-800).  Caches are int8 [N, Hkv, page, D] (strides in elements = bytes, 16-byte
 *      rows), scales [Hkv, D] dense, scale_dtype one of MOJO_BF16 / MOJO_F16 / MOJO_F32, taken as given (no cast launch).
 *      store: per element round(state / scale).clamp(-128, 127) under torch's type promotion, bit for bit — fp32 division,
 *      the quotient rounded to the state dtype first when state and scale share a 16-bit dtype, round half to even.  States
 *      bf16 / fp16 (state_dtype), strides in elements; plan and legacy forms, refusals and padded rows as
 *      mojo_hip_store_paged_kv_plan / _layout.
 *      decode: q' = q * key_scale (rounded to fp16), S = softmax_scale * q' K8^T, O = value_scale * (P V8) / l; both
 *      contractions on the matrix cores in fp16 whatever the query dtype (int8 -> fp16 is exact), outputs in the query dtype
 *      (`dtype`: MOJO_BF16 / MOJO_F16).  head_dim 64 / 80 / 96 / 128, pages of a multiple of 16 tokens, groups of 1..16 query
 *      heads; hints, workspace, leave_empty_rows, holes, empty rows and truncation as mojo_hip_paged_decode_gqa.
 *      prefill: one dequantising gather (the pages inside each sequence's length -> 16-bit scratch pages holding K8 * key_scale
 *      and V8 * value_scale rounded to the query dtype, and a scratch block table) followed by the code path of
 *      mojo_hip_paged_prefill_gqa on the scratch; envelope of that entry point (groups 1 / 2 / 4 / 8; head_dim 64 / 96 / 128).
 *      The workspace (256-byte aligned) holds batch * ceil(min(max_kv_len_hint, page * max_blocks_per_seq) / page) scratch
 *      pages of K and of V: without the hint a wide table is paid for at its capacity.  max_kv_len_hint, when > 0, MUST be
 *      an upper bound of every sequence's kv length (it sizes the scratch: keys past it are not gathered and read as zero
 *      keys; in the 16-bit entry point the hint only steers planning).  num_blocks bounds the page ids (an id outside
 *      [0, num_blocks) reads as zeros).  decode: q' is fp16 also for bf16 queries, so |q * key_scale| saturates at 65504 and
 *      is subnormal below 6.1e-5.  The decode entry point obeys MOJO_HIP_DECODE_FUSE, MOJO_HIP_DECODE_CHUNK and
 *      MOJO_HIP_STREAM_NT; the prefill one the prefill switches, through the code path it shares.                          */
int mojo_hip_store_paged_kv_c8_plan(const void* key_states, const void* value_states, void* key_cache,
                                    void* value_cache, const void* key_scale, const void* value_scale,
                                    const int32_t* plan, int64_t num_chunks, int64_t num_tokens,
                                    int64_t num_kv_heads, int64_t head_dim, int64_t num_blocks,
                                    int64_t block_size, int state_dtype, int scale_dtype,
                                    int64_t src_token_stride, int64_t src_head_stride,
                                    int64_t cache_block_stride, int64_t cache_head_stride,
                                    int64_t cache_token_stride, mojo_stream_t stream);
int mojo_hip_store_paged_kv_c8_layout(const void* key_states, const void* value_states, void* key_cache,
                                      void* value_cache, const void* key_scale, const void* value_scale,
                                      const int32_t* block_table, int64_t block_table_stride,
                                      int64_t max_blocks_per_seq, const int32_t* cu_q_lens,
                                      const int32_t* context_kv_lens, int64_t batch, int64_t num_tokens,
                                      int64_t num_kv_heads, int64_t head_dim, int64_t num_blocks,
                                      int64_t block_size, int state_dtype, int scale_dtype,
                                      int64_t src_token_stride, int64_t src_head_stride,
                                      int64_t cache_block_stride, int64_t cache_head_stride,
                                      int64_t cache_token_stride, mojo_stream_t stream);
int64_t mojo_hip_paged_decode_gqa_kv8_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                      int64_t head_dim, int64_t block_size,
                                                      int64_t max_blocks_per_seq, int64_t max_seq_len_hint);
int mojo_hip_paged_decode_gqa_kv8(const void* query, const void* key_cache, const void* key_scale,
                                  const void* value_cache, const void* value_scale,
                                  const int32_t* total_seq_lens, const int32_t* block_tables, void* out,
                                  void* workspace, int64_t workspace_bytes, int64_t batch, int64_t q_heads,
                                  int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                  int64_t max_blocks_per_seq, int64_t block_table_stride,
                                  int64_t cache_block_stride, int64_t cache_head_stride,
                                  int64_t cache_token_stride, int64_t max_seq_len_hint, float softmax_scale,
                                  int layout_abab, int leave_empty_rows, int dtype, int scale_dtype,
                                  mojo_stream_t stream);
int64_t mojo_hip_paged_prefill_gqa_kv8_workspace_bytes(int64_t total_tokens, int64_t batch, int64_t q_heads,
                                                       int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                                       int64_t max_blocks_per_seq, int64_t max_q_len_hint,
                                                       int64_t max_kv_len_hint);
int mojo_hip_paged_prefill_gqa_kv8(const void* query, const void* key_cache, const void* key_scale,
                                   const void* value_cache, const void* value_scale, const int32_t* cu_q_lens,
                                   const int32_t* cu_total_seq_lens, const int32_t* block_tables, void* out,
                                   int64_t total_tokens, int64_t batch, int64_t q_heads, int64_t kv_heads,
                                   int64_t head_dim, int64_t num_blocks, int64_t block_size,
                                   int64_t max_blocks_per_seq, int64_t block_table_stride,
                                   int64_t cache_block_stride, int64_t cache_head_stride,
                                   int64_t cache_token_stride, int64_t max_q_len_hint, int64_t max_kv_len_hint,
                                   float softmax_scale, int layout_abab, int dtype, int scale_dtype,
                                   void* workspace, int64_t workspace_bytes, mojo_stream_t stream);
/*      The same two ops with a sliding window (MojoPagedDecodeSWAWithKVDequant / MojoPagedPrefillSWAWithKVDequant): the
 *      arguments of their _gqa_kv8 siblings plus local_window (< 0: none) and global_window (<= 0: none), with the
 *      visibility rule of mojo_hip_paged_decode_swa / mojo_hip_paged_prefill_swa.  With neither window they run the
 *      _gqa_kv8 op itself.  Decode walks (and sizes its launch on) the visible keys only; pages outside a row's visible
 *      set are never read and may carry any VALID id or -1.  Prefill gathers only the pages that intersect a sequence's
 *      visible union into a compact scratch (block_size a multiple of 16 with a window).                              */
int64_t mojo_hip_paged_decode_swa_kv8_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                      int64_t head_dim, int64_t block_size,
                                                      int64_t max_blocks_per_seq, int64_t max_seq_len_hint,
                                                      int64_t local_window, int64_t global_window);
int mojo_hip_paged_decode_swa_kv8(const void* query, const void* key_cache, const void* key_scale,
                                  const void* value_cache, const void* value_scale,
                                  const int32_t* total_seq_lens, const int32_t* block_tables, void* out,
                                  void* workspace, int64_t workspace_bytes, int64_t batch, int64_t q_heads,
                                  int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                  int64_t max_blocks_per_seq, int64_t block_table_stride,
                                  int64_t cache_block_stride, int64_t cache_head_stride,
                                  int64_t cache_token_stride, int64_t max_seq_len_hint, float softmax_scale,
                                  int layout_abab, int leave_empty_rows, int dtype, int scale_dtype,
                                  int64_t local_window, int64_t global_window, mojo_stream_t stream);
int64_t mojo_hip_paged_prefill_swa_kv8_workspace_bytes(int64_t total_tokens, int64_t batch, int64_t q_heads,
                                                       int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                                       int64_t max_blocks_per_seq, int64_t max_q_len_hint,
                                                       int64_t max_kv_len_hint, int64_t local_window,
                                                       int64_t global_window);
int mojo_hip_paged_prefill_swa_kv8(const void* query, const void* key_cache, const void* key_scale,
                                   const void* value_cache, const void* value_scale, const int32_t* cu_q_lens,
                                   const int32_t* cu_total_seq_lens, const int32_t* block_tables, void* out,
                                   int64_t total_tokens, int64_t batch, int64_t q_heads, int64_t kv_heads,
                                   int64_t head_dim, int64_t num_blocks, int64_t block_size,
                                   int64_t max_blocks_per_seq, int64_t block_table_stride,
                                   int64_t cache_block_stride, int64_t cache_head_stride,
                                   int64_t cache_token_stride, int64_t max_q_len_hint, int64_t max_kv_len_hint,
                                   float softmax_scale, int layout_abab, int dtype, int scale_dtype,
                                   void* workspace, int64_t workspace_bytes, int64_t local_window,
                                   int64_t global_window, mojo_stream_t stream);

/* ---- MojoPagedDecodeNstepSWAWithKVDequant: `steps` query rows per sequence over the int8 cache.  The arguments of
 *      mojo_hip_paged_decode_swa_kv8 plus `steps`; query and out are [batch][steps][q_heads][head_dim] dense; lengths, step
 *      positions, visibility, empty rows, dead steps (0 < len < steps: zeros) and holes as mojo_hip_paged_decode_nstep; the
 *      arithmetic is that of the single-step int8 kernel.  steps == 1 IS mojo_hip_paged_decode_swa_kv8 (same plan, same
 *      workspace, bit for bit).  steps > 1 takes the geometries of the single-step int8 kernel (head_dim 64 / 80 / 96 / 128,
 *      pages of a multiple of 16 tokens, groups of <= 16 heads) with MOJO_HIP_DECODE_MFMA != 0; for every other geometry the
 *      workspace query answers -1 and the entry point returns MOJO_EUNSUPPORTED: the caller composes `steps` single-step
 *      calls on lengths len - (steps - 1 - j).  batch * kv_heads * ceil(steps / (16 / group)) above 65535: MOJO_EUNSUPPORTED. */
int64_t mojo_hip_paged_decode_nstep_kv8_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                        int64_t head_dim, int64_t block_size,
                                                        int64_t max_blocks_per_seq, int64_t max_seq_len_hint,
                                                        int64_t local_window, int64_t global_window, int64_t steps);
int mojo_hip_paged_decode_nstep_kv8(const void* query, const void* key_cache, const void* key_scale,
                                    const void* value_cache, const void* value_scale,
                                    const int32_t* total_seq_lens, const int32_t* block_tables, void* out,
                                    void* workspace, int64_t workspace_bytes, int64_t batch, int64_t q_heads,
                                    int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                    int64_t max_blocks_per_seq, int64_t block_table_stride,
                                    int64_t cache_block_stride, int64_t cache_head_stride,
                                    int64_t cache_token_stride, int64_t max_seq_len_hint, float softmax_scale,
                                    int layout_abab, int leave_empty_rows, int dtype, int scale_dtype,
                                    int64_t local_window, int64_t global_window, int64_t steps, mojo_stream_t stream);

/* ---- MoE routing either side of the grouped GEMM (core/operators/moe.py).
 *      gating (:299-316): softmax(hidden.float() @ gate_weight [hidden, E] fp32) over all experts, top-k in descending
 *      order (ties: lowest expert id), gates renormalised to sum 1.  top_k <= min(E, 64), E <= 1024.  With many
 *      experts and tokens (16-bit activations) the logits run on MFMA as x @ w_hi + x @ w_lo, w = w_hi + w_lo split
 *      into the activation dtype (error ~2^-16 relative); that route takes its scratch from the workspace.
 *      dispatch (:344-400): stable counting sort of the tokens*top_k routing slots by expert id (the reference leaves
 *      the order inside a bucket undefined; this one keeps flat-slot order, so the op is deterministic).  Outputs:
 *      sorted_hidden [slots, H], tokens_per_expert int32 [E], sorted_gates fp32 [slots] (viewed [slots,1]),
 *      token_indices int32 [slots].  Ids outside [0, E) are dropped.
 *      combine (:687-716): out[t] = sum of expert_outputs[j] (* sorted_gates[j]; NULL = no gates) over the rows j with
 *      token_indices[j] == t, fp32 from zero in ascending j, product and sum rounded separately — bit-identical to the
 *      reference's fp32 scatter-add.  Tokens nobody routes to are zero.                                         */
int64_t mojo_hip_moe_gating_workspace_bytes(int64_t tokens, int64_t hidden_size, int64_t num_experts, int dtype);
int mojo_hip_moe_gating(const void* hidden, const float* gate_weight, int32_t* top_k_indices, float* top_k_gates,
                        int64_t tokens, int64_t hidden_size, int64_t num_experts, int64_t top_k, int dtype,
                        void* workspace, int64_t workspace_bytes, mojo_stream_t stream);
int64_t mojo_hip_moe_dispatch_workspace_bytes(int64_t slots, int64_t num_experts);
int mojo_hip_moe_dispatch(const void* hidden, const float* top_k_gates, const int32_t* top_k_indices,
                          void* sorted_hidden, int32_t* tokens_per_expert, float* sorted_gates,
                          int32_t* token_indices, int64_t tokens, int64_t hidden_size, int64_t top_k,
                          int64_t num_experts, int dtype, void* workspace, int64_t workspace_bytes,
                          mojo_stream_t stream);
int64_t mojo_hip_moe_combine_workspace_bytes(int64_t tokens, int64_t rows);
int mojo_hip_moe_combine(const void* expert_outputs, const float* sorted_gates, const int32_t* token_indices,
                         void* out, int64_t tokens, int64_t rows, int64_t hidden_size, int dtype,
                         void* workspace, int64_t workspace_bytes, mojo_stream_t stream);

/* ---- Per-token activation quantisers feeding MojoQuantGemm.
 *      dynamic_quant (core/operators/quantize.py:153-169): y = x.float() [* inv_smooth_scale[K] fp32, nullable];
 *      scale = max(amax|y|, 1e-12) / 127, 1.0 where that is < 1e-6; q = clamp(round_half_even(y / scale), -128, 127).
 *      residual_add_rmsnorm_quant (core/operators/normalization.py:493-526): s = hidden + residual (rounded to the
 *      input dtype; residual nullable), y = rms_norm(s.float(), weight fp32, eps) [* smooth_scale fp32, nullable] kept
 *      in fp32, scale = max(amax|y|, 1e-12) / q_max (127 or 448), q = clamp(round_half_even(y / scale), q_min, q_max)
 *      as int8 or as float8_e4m3fn of that integer value.  out_sum (T, nullable) receives s (norm_pos = "pre"),
 *      out_normed (fp32, nullable) the normed tensor before smoothing (norm_pos = "post").  out_scale is fp32 [rows]. */
int mojo_hip_dynamic_quant(const void* input, const float* inv_smooth_scale, void* out_q, float* out_scale,
                           int64_t rows, int64_t dim, int dtype, mojo_stream_t stream);
int mojo_hip_residual_add_rmsnorm_quant(const void* hidden, const void* residual, const float* weight,
                                        const float* smooth_scale, void* out_q, void* out_sum, float* out_normed,
                                        float* out_scale, int64_t rows, int64_t dim, int dtype, int quant_dtype,
                                        float q_min, float eps, mojo_stream_t stream);

/* ---- The dense W8A8 quantiser ops (QUANT_DENSE_OPS).  Every per-column vector (weight, bias, smooth_scale, scale,
 *      weight_scale, quant_scale) and activation_scale are fp32; nothing synchronises with the host.
 *      rmsnorm_quant (core/operators/normalization.py:136-213): residual_add_rmsnorm_quant's arithmetic and kernels with
 *      no residual and no sum output; its launch tags start with `rmsnorm_quant`.
 *      layernorm_quant (:216-305, :536-646): s = hidden [+ residual, rounded to the input dtype; residual nullable],
 *      y = layer_norm(s.float(), weight, bias, eps) [* smooth_scale, nullable] in fp32 (mean and biased variance over the
 *      row; weight and bias both given or both NULL), scale = max(amax|y|, 1e-12) / q_max (127 or 448),
 *      q = clamp(round_half_even(y / scale), q_min, q_max) as int8 or as float8_e4m3fn of that integer.  out_sum (T,
 *      nullable) receives s — for BOTH norm_pos of MojoResidualAddLayerNormQuant.  out_scale is fp32 [rows].
 *      static_quant (core/operators/quantize.py:9-74): q[i] = clamp(round_half_even(float(x[i]) / scale[i % scale_len]),
 *      -128, 127) as int8 (or +-448 as float8_e4m3fn); n a multiple of scale_len; input dtype in {f32, f16, bf16}.
 *      dequant (:77-117): out[i] = round_to_out_dtype(float(q[i]) * scale[...]); input MOJO_I8 or MOJO_F8E4M3; out_dtype in
 *      {f32, f16, bf16}.  token_dim == 0: scale[i % scale_len] (a tensor of trailing dimensions); token_dim > 0: per-token
 *      scale[i / token_dim] (rows of token_dim elements, scale_len == n / token_dim).
 *      dequant_swiglu_quant (:250-354): x [rows, 2 * hidden] of dtype MOJO_I32 (GEMM accumulators), f32, f16 or bf16;
 *      y = float(x) * weight_scale[e] ([E, 2 * hidden]) [* activation_scale[row], nullable] [+ bias, nullable: [2 * hidden],
 *      or [E, 2 * hidden] when bias_is_grouped]; z = silu(y[hidden:]) * y[:hidden] (activate_left != 0: silu(y[:hidden]) *
 *      y[hidden:]) * quant_scale[e] ([E, hidden]); scale = max(amax|z|, 1e-12) / 127; q = clamp(round_half_even(z / scale),
 *      -128, 127).  e is the row's expert: rows sorted by expert, token_count int32 / int64 [E] on the device, scanned inside
 *      the kernel (negative counts read as zero); rows at or past sum(token_count): int8 zeros, scale 1.  token_count NULL:
 *      num_experts must be 1 and that expert owns every row.  out_q int8 [rows, hidden], out_scale fp32 [rows]; at most
 *      1024 experts.                                                                                                    */
int mojo_hip_rmsnorm_quant(const void* hidden, const float* weight, const float* smooth_scale, void* out_q,
                           float* out_scale, int64_t rows, int64_t dim, int dtype, int quant_dtype, float q_min,
                           float eps, mojo_stream_t stream);
int mojo_hip_layernorm_quant(const void* hidden, const void* residual, const float* weight, const float* bias,
                             const float* smooth_scale, void* out_q, void* out_sum, float* out_scale, int64_t rows,
                             int64_t dim, int dtype, int quant_dtype, float q_min, float eps, mojo_stream_t stream);
int mojo_hip_static_quant(const void* input, const float* scale, void* out_q, int64_t n, int64_t scale_len, int dtype,
                          int quant_dtype, mojo_stream_t stream);
int mojo_hip_dequant(const void* input, const float* scale, void* out, int64_t n, int64_t scale_len, int64_t token_dim,
                     int in_dtype, int out_dtype, mojo_stream_t stream);
int mojo_hip_dequant_swiglu_quant(const void* x, const float* weight_scale, const float* activation_scale,
                                  const float* bias, int bias_is_grouped, const float* quant_scale,
                                  const void* token_count, int token_count_is_i64, void* out_q, float* out_scale,
                                  int64_t rows, int64_t hidden, int64_t num_experts, int activate_left, int dtype,
                                  mojo_stream_t stream);

/* ---- MojoQuantExperts / MojoMoEDynamicQuant (core/operators/moe.py:452-667, quantize.py:178-247): W8A8 experts.
 *      group_quant_gemm: out[rows of g] = round_out( float(A8[rows of g] @ W8[g]^T) * weight_scale[g][n] * input_scale[m] )
 *      — the column scale FIRST (the experts' order; MojoQuantGemm's is row first, and with two fp32 roundings the bits
 *      differ).  input int8 [m_total, K]; weight int8 [G, N, K] (trans_weight != 0, the experts' layout; [G, K, N] returns
 *      MOJO_EUNSUPPORTED); input_scale fp32 [m_total]; weight_scale bf16 [G, N]; out_dtype in {f32, f16, bf16}; group_list
 *      int32 / int64 row counts on the device, prefix-summed on the device.  Rows [sum(counts), m_total) of out are
 *      written as zeros.  int32 accumulation: every kernel form, tile shape and K split gives the same bits.
 *      moe_dynamic_quant: the arithmetic of dynamic_quant with inv_smooth_scale fp32 [E, dim] selected by the row's
 *      expert (rows sorted by expert; token_count int32 / int64 [E] on the device, scanned inside the kernel).  glu != 0:
 *      input is the dequantised first projection [rows, 2 * dim] = [gate | up] and y = silu(float(gate)) * float(up)
 *      * inv_smooth_scale[e], all in fp32.  Rows at or past sum(token_count): int8 zeros, scale 1.  out_q int8
 *      [rows, dim], out_scale fp32 [rows]; input dtype in {f32, f16, bf16}; at most 1024 experts.                       */
int64_t mojo_hip_group_quant_gemm_workspace_bytes(int64_t m_total, int64_t k, int64_t n, int64_t num_groups);
int mojo_hip_group_quant_gemm(const void* input, const void* weight, const float* input_scale,
                              const void* weight_scale, void* out, const void* group_list, int group_list_is_i64,
                              int64_t m_total, int64_t k, int64_t n, int64_t num_groups, int trans_weight,
                              int out_dtype, void* workspace, int64_t workspace_bytes, mojo_stream_t stream);
int mojo_hip_moe_dynamic_quant(const void* input, const float* inv_smooth_scale, const void* token_count,
                               int token_count_is_i64, void* out_q, float* out_scale, int64_t rows, int64_t dim,
                               int64_t num_experts, int glu, int dtype, mojo_stream_t stream);

/* ---- MojoStorePagedMLAKVCache (experimental/operators/kv_cache.py:13-106): bit-exact copy of the new latent
 *      tokens compressed_kv_states [T, r] and k_pe_states [T, rope] into compressed_kv_cache [N,1,page,r] and
 *      k_pe_cache [N,1,page,rope] at positions context_kv_lens[b].. (cu_q_lens == NULL: one token per sequence).
 *      Per sequence the reference stops at the first negative page id and skips sequences whose first table entry or
 *      context length is negative; evaluated per token on the device, no host sync.  Strides in elements.        */
int mojo_hip_store_paged_mla_kv(const void* compressed_kv_states, const void* k_pe_states,
                                void* compressed_kv_cache, void* k_pe_cache, const int32_t* block_table,
                                int64_t block_table_stride, int64_t max_blocks_per_seq,
                                const int32_t* cu_q_lens, const int32_t* context_kv_lens, int64_t batch,
                                int64_t num_tokens, int64_t kv_lora_rank, int64_t rope_dim, int64_t num_blocks,
                                int64_t block_size, int64_t elt_bytes, int64_t ckv_src_token_stride,
                                int64_t kpe_src_token_stride, int64_t ckv_block_stride, int64_t ckv_token_stride,
                                int64_t kpe_block_stride, int64_t kpe_token_stride, mojo_stream_t stream);

/* ---- MojoPagedPrefillMLA in the golden's own formulation (experimental/operators/attention.py:405-447):
 *      mla_unpage: flat row cu[b] + t <- cache[table[b, t / page], 0, t % page, :] for t < kv_len_b (cu = cu_total_seq_lens, or
 *      cu_q_lens when that is NULL), for the compressed latent [.., kv_lora_rank] and the positional key [.., rope_dim];
 *      strides in elements; max_tokens_per_seq only sizes the grid; flat rows are relative to cu[0] (the pointers may address a
 *      slice of the batch) and total_keys_out (nullable, int32 [1]) receives min(cu[batch] - cu[0], capacity_rows), the
 *      decompression GEMM's device-side row count.  capacity_rows = rows the flat buffers hold: the lengths live on the device
 *      and the host sizes the buffers without a sync, so a row at or past the capacity is neither written by mla_unpage nor
 *      read by mla_prefill_attn (a sequence longer than max_tokens_per_seq is cut at that bound, per sequence, by both calls).  The decompression kv = c_kv @ kv_b_proj^T is
 *      mojo_hip_group_gemm with one group whose row count is the device-side total.
 *      mla_prefill_attn: causal flash attention per head over K = [kv[t, h, :nope] | k_pe[t, :]] and V = kv[t, h, nope:],
 *      kv [T_kv, heads, nope + v_dim] and k_pe [T_kv, rope] contiguous, sequence b's keys at rows cu[b] ..; optional fp32
 *      sink logit per head in the softmax denominator; rows of empty sequences read as zeros, and so do the padding rows
 *      behind cu_q_lens[batch] when zero_padding_rows is set (the last slice of a batch processed in slices).
 *      round_scaled_scores: 0 = scores rounded to the storage type, scaled in fp32 (the prefill golden, :425); 1 = the scaled
 *      scores are rounded to the storage type once more (the DECODE golden multiplies storage-type tensors, :215) — used by
 *      the golden-rounding decode route of MojoPagedDecodeMLA (one query token per sequence).  mla_prefill_supported: 1 when (nope, rope, v_dim, dtype) has an instantiation.                  */
int mojo_hip_mla_prefill_supported(int64_t nope, int64_t rope, int64_t v_dim, int dtype);
int mojo_hip_mla_unpage(const void* compressed_kv_cache, const void* k_pe_cache, void* ckv_out, void* kpe_out,
                        const int32_t* cu_q_lens, const int32_t* cu_total_seq_lens, const int32_t* block_tables,
                        int64_t block_table_stride, int64_t max_blocks_per_seq, int64_t batch,
                        int64_t kv_lora_rank, int64_t rope_dim, int64_t block_size, int64_t elt_bytes,
                        int64_t ckv_block_stride, int64_t ckv_token_stride, int64_t kpe_block_stride,
                        int64_t kpe_token_stride, int64_t max_tokens_per_seq, int64_t capacity_rows,
                        int32_t* total_keys_out, mojo_stream_t stream);
int mojo_hip_mla_prefill_attn(const void* query, const void* kv_decompressed, const void* k_pe_flat,
                              const float* attn_sink, void* out, const int32_t* cu_q_lens,
                              const int32_t* cu_total_seq_lens, int64_t total_tokens, int64_t batch,
                              int64_t heads, int64_t head_begin, int64_t head_count, int64_t nope, int64_t rope,
                              int64_t v_dim, int64_t max_q_len,
                              int64_t max_tokens_per_seq, int64_t capacity_rows, float softmax_scale, int round_scaled_scores,
                              int zero_padding_rows, int dtype, mojo_stream_t stream);

/* ---- Direct reduce-scatter / all-gather over HIP-IPC peer buffers: the exchange step of MojoGemmAllReduce /
 *      MojoGemmReduceScatter without a ring (core/operators/compute_with_comm.py:57-116, :264-340; role of
 *      runtime/comm_context.py:107-153 `allocate_peer_mem` + the pull-and-add loops of
 *      backends/ttx/kernels/npu/a2/gemm_allreduce.py:85-145 and gemm_reduce_scatter.py:108-156).
 *      Set-up (the only entry points of this library that allocate or synchronise): each rank allocates ONE buffer
 *      [2 x capacity data | 4 KiB | ctrl words], exports a 64-byte handle, opens every peer's handle.
 *      peer_data[r] / peer_flags[r] = this process's pointer to rank r's data area / control words (own entry = local).
 *      Exchange steps only enqueue kernels.  epoch grows by one per operator call (never reset); flag kind 0 = "partial
 *      product of (rank, chunk) is in memory", kind 1 = "reduced share of (rank, chunk) is in memory".
 *      reduce: dst[rows, n] = sum over ranks of the contiguous [rows, n] block at src_offset_bytes of every rank's data
 *      area (fp32 sum in rank order, one rounding), after waiting for every rank's kind-0 flag of `chunk`; write_back = 1
 *      also stores the result over the own block and raises this rank's kind-1 flag at every peer when the launch is done.
 *      gather: for every other rank p, after its kind-1 flag: rows [rows*p/ws, rows*(p+1)/ws) of the [rows, n] chunk at
 *      chunk_offset_bytes of rank p's data area -> the same rows of dst.
 *      Every wait is bounded (MOJO_HIP_PEER_TIMEOUT_MS, default 20 s; mojo_hip_peer_set_timeout_ms overrides it for the
 *      steps enqueued afterwards and returns the previous override, 0 = none): on expiry the sticky error word is set, the
 *      affected output is filled with NaN and the grid drains; mojo_hip_peer_error reads (and clears) the word.        */
int64_t mojo_hip_peer_ctrl_bytes(void);
int64_t mojo_hip_peer_max_ranks(void);
int64_t mojo_hip_peer_max_chunks(void);
int64_t mojo_hip_peer_handle_bytes(void);
int64_t mojo_hip_peer_set_timeout_ms(int64_t milliseconds);
int mojo_hip_peer_alloc(void** ptr_out, int64_t bytes, int uncached);
int mojo_hip_peer_free(void* ptr);
int mojo_hip_peer_export(void* ptr, void* handle_out);
int mojo_hip_peer_open(const void* handle, void** ptr_out);
int mojo_hip_peer_close(void* ptr);
int mojo_hip_peer_error(void* local_flags, int clear, int32_t* error_out);
/*      Captured mode (HIP-graph replay).  Every exchange step below takes the call's epoch; epoch 0 means "the epoch
 *      word of this rank's control area", which mojo_hip_peer_begin advances once per call after waiting (bounded) until
 *      every peer has raised flag kind 2 ("finished reading this rank's data") for the previous call.  A captured call is
 *      begin -> steps with epoch 0 on ONE data area (no parity halves) -> mojo_hip_peer_signal(kind 2, chunk 0, epoch 0).  */
int mojo_hip_peer_begin(void* const* peer_data, void* const* peer_flags, int64_t world, int64_t rank,
                        mojo_stream_t stream);
/* set-up check: `bytes` of a peer's buffer (opened mapping) copied to host memory by the runtime; synchronises */
int mojo_hip_peer_peek(const void* peer_ptr, void* host_out, int64_t bytes);
int mojo_hip_peer_signal(void* const* peer_data, void* const* peer_flags, int64_t world, int64_t rank,
                         int kind, int64_t chunk, uint32_t epoch, mojo_stream_t stream);
int mojo_hip_peer_reduce(void* const* peer_data, void* const* peer_flags, int64_t world, int64_t rank,
                         int64_t chunk, uint32_t epoch, int64_t src_offset_bytes, int64_t rows, int64_t n,
                         void* dst, int64_t ld_dst, int write_back, int dtype, mojo_stream_t stream);
int mojo_hip_peer_gather(void* const* peer_data, void* const* peer_flags, int64_t world, int64_t rank,
                         int64_t chunk, uint32_t epoch, int64_t chunk_offset_bytes, int64_t rows, int64_t n,
                         void* dst, int64_t ld_dst, int dtype, mojo_stream_t stream);
/*      pull (the all-gather of MojoAllGatherGemm, compute_with_comm.py:119-184): slot p of dst (dst + p * dst_stride_bytes)
 *      <- `bytes` at src_offset_bytes of rank p's data area, for every rank (include_self) or every other rank, each after
 *      rank p's flag (kind, flag_chunk) reached `epoch` (the own block needs no wait).                                   */
int mojo_hip_peer_pull(void* const* peer_data, void* const* peer_flags, int64_t world, int64_t rank, int kind,
                       int64_t flag_chunk, uint32_t epoch, int64_t src_offset_bytes, int64_t bytes, void* dst,
                       int64_t dst_stride_bytes, int include_self, mojo_stream_t stream);

/* ---- The sampling step (core/operators/sampling.py: MojoTopKSampling, MojoTopPSampling, MojoTopPFilter,
 *      MojoApplyPenaltiesTempurate, MojoRejectSampling, MojoJoinProbRejectSampling).
 *      Top-K stage: the K largest of each row of logits [rows, vocab] (f32 / f16 / bf16, dense, read once) in descending
 *      order; among equal values the lower index first, a tie across position K keeps the lower indices.  Exact and
 *      deterministic; k <= vocab and k <= sampling_max_k (MOJO_EUNSUPPORTED above).  -inf is legal, NaN / +inf are not.
 *      Nucleus mask over the K sorted values v: p = softmax(v); over = running_sum(p) > top_p; the first
 *      min_tokens_to_keep - 1 positions of `over` cleared; removed = over moved one position right, position 0 kept; removed
 *      positions take filter_value (it may be finite); final = softmax of the result.
 *      top_p_filter writes final (in `dtype`) and the int64 indices, both [rows, k].
 *      sample_with_uniforms picks per row the first position whose running sum of final exceeds uniforms[row] * total
 *      (fp32 uniforms in [0, 1)), held to the last position of non-zero probability, and writes its probability (fp32 [rows])
 *      and token (int64 [rows]); nucleus == 0: final is the plain softmax of the K values (top_p, min_tokens_to_keep and
 *      filter_value unused).  Two launches, no host synchronisation, nothing allocated: capturable in a graph.
 *      `slices`: workgroups per row of the first pass, 0 = the library chooses; every count gives the same bits.  The
 *      workspace query (host only) takes the same count; the workspace must be 8-byte aligned.
 *      apply_penalties: one elementwise launch over [rows, vocab] (rows < 65536), out may be logits itself.  row_table is a
 *      device array of rows x 32 bytes: float frequency, presence, repetition, temperature; int32 flags (1 frequency, 2
 *      presence, 4 repetition, 8 temperature: which steps run); int32 padding; the 64-bit device address of the row's
 *      frequency vector [vocab] (unused without flags 1 | 2 | 4).  freq_kind: 0 int32, 1 int64, 2 fp32, one for all rows.
 *      Per element in fp32, each operation rounded on its own: l -= frequency * f; l -= presence * (f > 0); by the sign of
 *      l * f: l * repetition (negative) or l / repetition (positive); l /= temperature.
 *      reject_sampling: target_probs [batch, steps + 1, vocab] and draft_probs [batch, steps] in `dtype`, draft_tokens int64
 *      [batch, steps], fp32 uniforms [batch] (joint == 0) or [batch, steps] (joint != 0).  next_tokens int64
 *      [batch, steps + 1] = [draft_tokens | 0].  joint == 0: accepted_len int64 [batch], the first j with target / draft < u,
 *      else steps.  joint != 0: accepted_len int32 [batch], one past the last j where NOT cumprod(clamp(target / draft, 0, 1))
 *      [j] < cumprod(u)[j], else 0.  One launch, one thread per row, products left to right.                             */
int64_t mojo_hip_sampling_max_k(void);
int64_t mojo_hip_sampling_workspace_bytes(int64_t rows, int64_t vocab, int64_t k, int64_t slices);
int mojo_hip_top_p_filter(const void* logits, void* probs, int64_t* indices, int64_t rows, int64_t vocab, int64_t k,
                          float top_p, int64_t min_tokens_to_keep, float filter_value, int64_t slices, int dtype,
                          void* workspace, int64_t workspace_bytes, mojo_stream_t stream);
int mojo_hip_sample_with_uniforms(const void* logits, const float* uniforms, float* next_probs, int64_t* next_tokens,
                                  int64_t rows, int64_t vocab, int64_t k, int nucleus, float top_p,
                                  int64_t min_tokens_to_keep, float filter_value, int64_t slices, int dtype,
                                  void* workspace, int64_t workspace_bytes, mojo_stream_t stream);
int mojo_hip_apply_penalties(const void* logits, void* out, const void* row_table, int64_t rows, int64_t vocab, int dtype,
                             int freq_kind, mojo_stream_t stream);
int mojo_hip_reject_sampling(const void* target_probs, const int64_t* draft_tokens, const void* draft_probs,
                             const float* uniforms, int64_t* next_tokens, void* accepted_len, int64_t batch,
                             int64_t steps, int64_t vocab, int joint, int dtype, mojo_stream_t stream);

/* ---- The DiT block ops (DIT_BLOCK_OPS: MojoLayerNorm, MojoResidualAddLayerNorm, MojoGelu, MojoSilu, MojoGridRoPE).
 *      layernorm (core/operators/normalization.py:19-68, :365-432): s = hidden [+ residual, rounded to the input dtype;
 *      residual nullable]; mean = sum(s) / dim in fp32 over the row held in registers; var = mean((s - mean)^2), never
 *      E[s^2] - mean^2; rstd = rsqrt(var + eps); normed = round_T(fma((s - mean) * rstd, weight, bias)), or
 *      round_T((s - mean) * rstd) when weight and bias are NULL (both given or both NULL, in the activation dtype).
 *      sum_out (nullable, norm_pos = "pre") receives s.  hidden / residual rows are row_stride elements apart (>= dim, the
 *      last dimension dense); normed_out and sum_out are dense [rows, dim].  dtype in {f32, f16, bf16}.  Launch tags are
 *      `layernorm:vec<V>:tpr<64|128|256>:<cached|reread>:<nt|plain>`.  V is the widest of {16 bytes, 2 elements, 1 element}
 *      that dim, the row strides and every pointer allow; threads per row follow the RMSNorm kernels (64 up to 256
 *      vectors, 128 up to 512, else 256; with rows <= 128 the 16-byte form takes 256 from 256 vectors on).  A thread keeps
 *      layernorm_cache_vectors() vectors of its row in registers: rows of more than tpr x that many vectors (only tpr256
 *      has such) re-read their tail in the second and third pass (`reread`).
 *      activation: out[i] = round_T(f(float(in[i]))), one rounding; kind 0 = GELU in the erf form
 *      x * 0.5 * (1 + erff(x * sqrt(1/2))), kind 1 = SiLU x / (1 + expf(-x)).  in and out dense, out may be in.  16-byte
 *      vectors when both pointers allow (tag `activation:<gelu_erf|silu>:vec<V>:<nt|plain>`, V = 1 otherwise), a scalar tail.
 *      grid_rope (experimental/operators/position_embedding.py:80-118): x [batch, tokens, heads, head_dim] read through
 *      x_strides (batch, token, head; elements; the last dimension dense), out dense.  Token t of sample i is rotated iff
 *      t < F_i * H_i * W_i (grid_sizes [batch, 3], int32 or int64, ON THE DEVICE) and t < that sample's frequency rows;
 *      every other token is copied.  freqs is fp32 [rows, head_dim / 2, 2] = (cos, sin) interleaved (a complex64 tensor
 *      seen through view_as_real).  freq_table NULL: every sample reads rows [0, shared_freq_rows); else an int64
 *      [batch, 2] device table of (first row, row count) per sample.  Adjacent pairs (a, b) = (x[2j], x[2j + 1]):
 *      re = a * c - b * s, im = a * s + b * c, each product and sum rounded on its own in fp32, one rounding to T.      */
int64_t mojo_hip_layernorm_cache_vectors(void);
int mojo_hip_layernorm(const void* hidden, const void* residual, const void* weight, const void* bias,
                       void* normed_out, void* sum_out, int64_t rows, int64_t dim, int64_t hidden_row_stride,
                       int64_t residual_row_stride, int dtype, float eps, mojo_stream_t stream);
int mojo_hip_activation(const void* in, void* out, int64_t n, int kind, int dtype, mojo_stream_t stream);
int mojo_hip_grid_rope(const void* x, void* out, const float* freqs, const void* grid_sizes, int grid_sizes_is_i64,
                       const int64_t* freq_table, int64_t shared_freq_rows, int64_t batch, int64_t tokens,
                       int64_t heads, int64_t head_dim, const int64_t x_strides[3], int dtype, mojo_stream_t stream);

/* ---- The vision-tower ops (VISION_TOWER_OPS: MojoPackedSdpa, MojoVisionRotaryEmbedding2D, MojoApplyVisionRoPE2D, MojoMRoPE,
 *      MojoMRoPEInplace).
 *      packed_sdpa: the semantics of MojoSWA(is_causal=False) (core/operators/attention.py:747-835): the arguments of
 *      mojo_hip_swa_packed without the windows, and no causal edge — every query row of sequence b sees every key of
 *      [cu_total_seq_lens[b], cu_total_seq_lens[b + 1]).  q_len and kv_len of a sequence are independent (kv_len < q_len is
 *      legal).  The kernel is the prefill's with the walk of mojo_hip_sdpa: the same bits as mojo_hip_sdpa on the same tokens
 *      at the same key split.  Hints, workspace and key split as mojo_hip_swa_packed; a sequence longer than max_q_len_hint
 *      has its rows past the hint written as zeros, and keys at or past max_kv_len_hint are not seen.  Rows of sequences
 *      without keys and rows at or past cu_q_lens[batch] are zeros.  Every cu_total_seq_lens entry is clamped to
 *      [0, total_kv_tokens] by the kernel: no read leaves the tensors.  Launch tags `packed_sdpa:default:<fast_stage|
 *      general_stage>:ksplit<n>`.
 *      (MojoApplyVisionRoPE2D, core/operators/position_embedding.py:366-407, is mojo_hip_apply_rope with rope_dim = head_dim
 *      on token-first tensors: the same fp32 products and sum, bit for bit.)
 *      vision_rotary_2d (core/operators/position_embedding.py:281-363): cos_out / sin_out fp32 [tokens][rope_dim] dense.
 *      samples: int64 [batch][3] ON THE DEVICE, (first row, H, W) per image, first rows ascending from 0 and
 *      first + H * W <= tokens; H and W multiples of adapooling_factor.  Token i of a sample sits at
 *      (h, w) = (bh * f + ih, bw * f + iw) with (bh, bw) the f x f window i / f^2 in row-major window order and (ih, iw)
 *      the patch i % f^2 inside it.  Row = [h * inv_freq | w * inv_freq] twice (inv_freq: fp32 [rope_dim / 4]); each angle is
 *      one fp32 product, then cosf / sinf.  Tag `vision_rotary_2d:pool<f>`.
 *      mrope (core/operators/position_embedding.py:178-278, experimental/operators/position_embedding.py:121-236): query
 *      [tokens][q_heads * head_dim] and key [tokens][k_heads * head_dim] by a row stride in elements; half = sum of
 *      mrope_section (host array of 3), 2 * half <= head_dim.  out[i] = h1 * c - h2 * s, out[half + i] = h2 * c + h1 * s,
 *      each product and the sum rounded on their own in fp32, one rounding to dtype.  In place when query_out == query and
 *      key_out == key (elements at or past 2 * half are not touched); otherwise both outputs are distinct tensors and those
 *      elements are copied.  Tables (table_dtype f32 / f16 / bf16, converted on read) are [3][tokens][half] addressed by
 *      table_section_stride / table_token_stride, or one merged [tokens][half] table with table_section_stride = 0; the
 *      kernel picks the table per element: chunked (is_interleaved = 0): 0 / 1 / 2 by the section i falls in; interleaved:
 *      1 where i % 3 == 1 and i < 3 * section[1], 2 where i % 3 == 2 and i < 3 * section[2], else 0.  Tags
 *      `mrope:vec<V>:<inplace|copy>:<merged|chunked|interleaved>`.  No host sync.                                        */
int64_t mojo_hip_packed_sdpa_workspace_bytes(int64_t total_q_tokens, int64_t total_kv_tokens, int64_t batch,
                                             int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                                             int64_t max_q_len_hint, int64_t max_kv_len_hint);
int mojo_hip_packed_sdpa(const void* query, const void* key, const void* value, const int32_t* cu_q_lens,
                         const int32_t* cu_total_seq_lens, void* out, int64_t total_q_tokens,
                         int64_t total_kv_tokens, int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t head_dim,
                         int64_t kv_token_stride, int64_t kv_head_stride, int64_t max_q_len_hint,
                         int64_t max_kv_len_hint, float softmax_scale, int layout_abab, int dtype, void* workspace,
                         int64_t workspace_bytes, mojo_stream_t stream);
int mojo_hip_vision_rotary_2d(float* cos_out, float* sin_out, const int64_t* samples, int64_t batch, int64_t tokens,
                              int64_t rope_dim, int64_t adapooling_factor, const float* inv_freq, mojo_stream_t stream);
int mojo_hip_mrope(const void* query, const void* key, void* query_out, void* key_out, const void* cos_table,
                   const void* sin_table, int64_t tokens, int64_t q_heads, int64_t k_heads, int64_t head_dim,
                   int64_t q_row_stride, int64_t k_row_stride, int64_t qo_row_stride, int64_t ko_row_stride,
                   int64_t table_section_stride, int64_t table_token_stride, const int64_t mrope_section[3],
                   int is_interleaved, int table_dtype, int dtype, mojo_stream_t stream);

/* ---- The input-embedding ops (EMBEDDING_OPS: MojoEmbedding, MojoParallelEmbedding, MojoOverEncodingNGram, MojoOverEncoding,
 *      MojoNF4DequantEmbedding; core/operators/embedding.py, core/operators/over_encoding.py).  Ids, q_lens and the layer's
 *      three vocabulary arrays are read ON THE DEVICE: no host synchronisation, graph-capturable.  An index outside its table
 *      never reads out of bounds and never traps: it selects a row of zeros.
 *      embedding: out[t] = table[ids[t] - vocab_start] when that index is in [0, rows), else zeros.  ids int32 / int64
 *      (ids_i64) dense [tokens]; table and out by a row stride in elements, dtype f32 / f16 / bf16 (a byte copy).  16-byte
 *      vectors when the row bytes, both strides and both base pointers are multiples of 16, single elements otherwise.  Tags
 *      `embedding:<vec16|scalar>:lanes<L>`.
 *      nf4_embedding: the same indexing into a packed-NF4 table: qweight [rows][dim / 2] bytes dense (int8 or uint8: the bits),
 *      element 2j the low and 2j + 1 the high nibble of byte j; scale / mean [rows][dim / group_size] dense in scale_dtype
 *      (f32 / f16 / bf16); codebook: the 16 levels as fp16 on the device (the reference holds them ROUNDED to fp16).  The value
 *      is fp32(codebook[nibble]) * fp32(scale) + fp32(mean), the product and the sum each rounded in fp32 (no fused
 *      multiply-add), rounded once to out_dtype.  group_size: any positive divisor of dim, taken per element (odd sizes
 *      split a byte between two groups).  Tags `nf4_embedding:<vec8|scalar>:lanes<L>`.
 *      oe_ngram: out[t][g] = id + oe_vocab_offsets[g] with id = x[t], carry = ori_vocab_size, and for i in 1 .. oe_grams[g] - 1:
 *      id = (id + p(i) * carry) mod V, carry = carry * ori_vocab_size mod V (V = oe_vocab_sizes[g]; torch's floor modulus; sums
 *      and products wrap in 64 bits; the first carry is not reduced; a gram of 1 applies no modulus).  p(i) = x[t - i] inside
 *      the sequence, history[seq][hist_len + pos - i] before its start (the history is read from its END; hist_len >=
 *      max_gram - 1 or MOJO_EINVAL).  seq_len == 0: packed, input_ids [tokens] with q_lens [batch] (negative: 0; a token at or
 *      past sum(q_lens) gets id 0, in the concatenation a row of zeros); seq_len > 0: batched, input_ids [batch][seq_len]
 *      dense, tokens == batch * seq_len.  history [batch][hist_len] by hist_stride.  A gram above max_gram is clamped to it.
 *      index_flags: bit 0 input_ids, 1 history, 2 q_lens, 3 oe_vocab_sizes, 4 oe_grams, 5 oe_vocab_offsets is int64 (else
 *      int32).  out has the dtype of input_ids, [tokens][num_grams] dense.  num_grams <= 255.  Tags `oe_ngram:<packed|batched>`.
 *      over_encoding_concat: one launch writes out[t] = [ori_table row of x[t] | mega row of id(t, 0) | ... | mega row of
 *      id(t, G - 1)], ori_dim + G * mega_dim elements by out_row_stride; the ids are those of oe_ngram and are not written
 *      anywhere.  ori_table [ori_rows][ori_dim] by ori_row_stride; the mega table dense [mega_rows][mega_dim] by
 *      mega_row_stride in dtype (mega_nf4 = 0; scale / mean / codebook unused) or packed NF4 as in nf4_embedding (mega_nf4 = 1;
 *      mega_row_stride unused), indexed by id - mega_vocab_start.  The 16-byte path needs every segment start (ori_dim + g *
 *      mega_dim elements) and every row on a 16-byte boundary; else single elements.  Tags
 *      `oe_concat:<dense|nf4>:<vec|scalar>:<packed|batched>`.                                                              */
int mojo_hip_embedding(const void* ids, int ids_i64, const void* table, void* out, int64_t tokens, int64_t rows, int64_t dim,
                       int64_t vocab_start, int64_t table_row_stride, int64_t out_row_stride, int dtype,
                       mojo_stream_t stream);
int mojo_hip_nf4_embedding(const void* ids, int ids_i64, const void* qweight, const void* scale, const void* mean,
                           const void* codebook, void* out, int64_t tokens, int64_t rows, int64_t dim, int64_t group_size,
                           int64_t vocab_start, int64_t out_row_stride, int scale_dtype, int out_dtype, mojo_stream_t stream);
int mojo_hip_oe_ngram(const void* input_ids, const void* history, const void* q_lens, const void* oe_vocab_sizes,
                      const void* oe_grams, const void* oe_vocab_offsets, void* out, int64_t tokens, int64_t batch,
                      int64_t seq_len, int64_t hist_len, int64_t hist_stride, int64_t num_grams, int64_t max_gram,
                      int64_t ori_vocab_size, int index_flags, mojo_stream_t stream);
int mojo_hip_over_encoding_concat(const void* input_ids, const void* history, const void* q_lens, const void* oe_vocab_sizes,
                                  const void* oe_grams, const void* oe_vocab_offsets, int64_t tokens, int64_t batch,
                                  int64_t seq_len, int64_t hist_len, int64_t hist_stride, int64_t num_grams, int64_t max_gram,
                                  int64_t ori_vocab_size, int index_flags, const void* ori_table, int64_t ori_rows,
                                  int64_t ori_dim, int64_t ori_row_stride, const void* mega_table, const void* mega_scale,
                                  const void* mega_mean, const void* codebook, int64_t mega_rows, int64_t mega_dim,
                                  int64_t mega_row_stride, int64_t group_size, int64_t mega_vocab_start, int mega_nf4,
                                  int scale_dtype, void* out, int64_t out_row_stride, int dtype, mojo_stream_t stream);

/* ---- The short-convolution ops (SHORT_CONV_OPS: MojoCausalConv1dUpdateState, MojoCausalConv1d; core/operators/convolution.py):
 *      the depthwise causal convolution of width 2..4 in front of a linear-attention or state-space mixer, forward only.
 *      For every sequence s and channel d, with cat = [state_in[s][d][0 .. S) | x[s][0 .. T)] (state_in == NULL: S zeros):
 *        out[s][t][d]      = act(bias[d] + sum_k weight[d][k] * cat[S + t - (W - 1) + k])        k = 0 .. W - 1
 *        state_out[s][d][j] = cat[T + j]                                                          j = 0 .. S - 1
 *      fp32 arithmetic in ONE order: acc = bias (or +0.0), then acc = acc + weight[k] * cat[..] for k = 0 .. W - 1, the product and
 *      the sum each rounded on their own (no fused multiply-add); silu != 0 applies SiLU to the fp32 accumulator
 *      (mojo_hip_activation's function); one rounding to dtype; then, with residual, storage(out) + residual in fp32 rounded again.
 *      x, weight [dim][width] dense, bias [dim], states, residual and out share dtype (f32 / f16 / bf16).  width 2, 3 or 4;
 *      width - 1 <= state_len <= 8; anything else MOJO_EUNSUPPORTED.
 *      Batched (cu_seqlens == NULL): batch sequences of seq_len tokens.  Packed: cu_seqlens int32 / int64 (cu_i64) [batch + 1] ON
 *      THE DEVICE (no host synchronisation, graph-capturable), seq_len = the packed token count, the batch strides unused; a bound
 *      is clamped into [0, seq_len], a token outside every sequence gets zeros, and no tap crosses a sequence start.
 *      x, out and residual are addressed by (batch, time, dim) strides in elements; the states [batch][dim][state_len] by
 *      (batch, dim) strides with the columns dense.  The kernel follows x: x_time_stride == 1 (batched) takes the
 *      time-contiguous forms and needs out / residual time strides of 1; else x_dim_stride == 1 takes the channel-contiguous
 *      form and needs out / residual dim strides of 1; anything else MOJO_EINVAL (the caller makes x dense).
 *      Channel-contiguous: a thread owns one vector of channels (16 bytes, else 8, else 4, else one element, by what dim, bases
 *      and strides allow) and walks a run of run_tokens() consecutive tokens with the last W - 1 inputs in registers.  Tags
 *      `causal_conv1d:channel:vec<V>:<batched|packed>`.
 *      Time-contiguous: seq_len <= row_thread_max_t() one thread per (sequence, channel) row (`causal_conv1d:time:row`); longer
 *      rows in 16-byte vectors with the head and tail of every row peeled when x, out and residual rows are misaligned alike
 *      (`causal_conv1d:time:vec<V>`), single elements otherwise (`causal_conv1d:time:vec1`).
 *      state_out may be state_in in the BATCHED forms (the in-place update of MojoCausalConv1dUpdateState): the one thread
 *      that reads a row's old state is the one that writes its new state, after its reads, and no other thread touches that
 *      row.  Packed: MOJO_EINVAL when they are the same pointer (the caller must reject any overlap).  seq_len == 0 writes
 *      nothing in the batched forms (the state stays); packed, every sequence is empty and state_out = state_in or zeros. */
int64_t mojo_hip_causal_conv1d_run_tokens(void);
int64_t mojo_hip_causal_conv1d_row_thread_max_t(void);
int mojo_hip_causal_conv1d(const void* x, const void* weight, const void* bias, const void* residual, const void* state_in,
                           void* state_out, void* out, const void* cu_seqlens, int cu_i64, int64_t batch, int64_t seq_len,
                           int64_t dim, int64_t width, int64_t state_len, int64_t x_batch_stride, int64_t x_time_stride,
                           int64_t x_dim_stride, int64_t out_batch_stride, int64_t out_time_stride, int64_t out_dim_stride,
                           int64_t res_batch_stride, int64_t res_time_stride, int64_t res_dim_stride,
                           int64_t state_in_batch_stride, int64_t state_in_dim_stride, int64_t state_out_batch_stride,
                           int64_t state_out_dim_stride, int silu, int dtype, mojo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MOJO_HIP_H */
