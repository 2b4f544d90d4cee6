// MojoSdpa — bidirectional scaled-dot-product attention with an optional bias / boolean mask: the FULL instances of
// prefill_kernel (paged_prefill_body.h).  The linear walk of MojoSWA without its diagonal: every row of a batch entry sees the
// keys [0, Sk), every whole key tile runs the unmasked (fast-staged) loop and only the partial tail tile runs the masked variant,
// which hides key >= Sk.  Sq and Sk are uniform over the batch (kernel arguments: no cu_* arrays), Sk < Sq is legal
// (cross-attention), and Q, K, V and out are addressed by 64-bit batch / head / token strides, so the token-major view
// ([B,S,H,D] memory seen as [B,H,S,D]) and a contiguous [B,H,S,D] tensor are both read and written in place.  Heads are
// grouped as repeat_interleave groups them (q head h reads kv head h / G).
//
// The MASK instances add a bias (the query's dtype or fp32, -inf allowed) to the scaled score, or hide the keys a boolean mask
// marks False, read in place through the mask's own strides (0 = broadcast).  A row with no visible key stores zeros.
//
// Key split, merge kernel and plan are the prefill's (prefill_plan / prefill_ksplit, MOJO_HIP_PREFILL_KSPLIT forces).
// A translation unit of its own so that its instances compile beside the paged and the packed ones.
#undef PF_STAMPS
#undef PF_WG_STAMPS
#include "paged_prefill_body.h"

using namespace mojo;

static PrefillGeom sdpa_geom(int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len, int64_t kv_len, int64_t head_dim) {
  PrefillGeom g;
  g.total_tokens = q_len; g.batch = batch; g.q_heads = q_heads; g.kv_heads = kv_heads; g.head_dim = head_dim;
  g.total_kv_tokens = kv_len < 0 ? 0 : kv_len;          // sizes the key split: the keys every block walks
  g.page = PF_KEYS;
  return g;
}

template <typename T, int G, int DK, bool MASK>
static void launch_sdpa(const SdpaArgs& a, dim3 grid, hipStream_t s) {
  static std::atomic<uint64_t> attr_set{0};
  if (first_call_on_device(attr_set)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&prefill_kernel<T, G, DK, false, false, true, true, MASK>), hipFuncAttributeMaxDynamicSharedMemorySize, PF_LDS);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&prefill_kernel<T, G, DK, true, false, true, true, MASK>), hipFuncAttributeMaxDynamicSharedMemorySize, PF_LDS);
  }
  if (a.ksplit > 1) {
    hipLaunchKernelGGL((prefill_kernel<T, G, DK, true, false, true, true, MASK>), grid, dim3(256), PF_LDS, s, a);
    hipLaunchKernelGGL((prefill_merge_kernel<T, G, true>), dim3(static_cast<unsigned>(a.n_qb * a.hkv * a.batch * PF_MERGE_SPLIT)), dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL((prefill_kernel<T, G, DK, false, false, true, true, MASK>), grid, dim3(256), PF_LDS, s, a);
  }
}

template <typename T, int G, bool MASK>
static int sdpa_dk(const SdpaArgs& a, dim3 grid, hipStream_t s) {
  switch (a.dim) {
    case 64: launch_sdpa<T, G, 2, MASK>(a, grid, s); break;
    case 96: launch_sdpa<T, G, 3, MASK>(a, grid, s); break;
    case 128: launch_sdpa<T, G, 4, MASK>(a, grid, s); break;
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "sdpa: head_dim %d (64, 96, 128)", a.dim);
  }
  MOJO_CHECK_LAUNCH("sdpa");
  note_launch(MASK ? "sdpa:default:%s:ksplit%d:mask" : "sdpa:default:%s:ksplit%d", a.fast_stage ? "fast_stage" : "general_stage", a.ksplit);
  return MOJO_OK;
}

template <typename T, bool MASK>
static int sdpa_g(const SdpaArgs& a, int G, dim3 grid, hipStream_t s) {
  switch (G) {
    case 1: return sdpa_dk<T, 1, MASK>(a, grid, s);
    case 2: return sdpa_dk<T, 2, MASK>(a, grid, s);
    case 4: return sdpa_dk<T, 4, MASK>(a, grid, s);
    case 8: return sdpa_dk<T, 8, MASK>(a, grid, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "sdpa: group size %d (1, 2, 4, 8)", G);
  }
}

extern "C" int64_t mojo_hip_sdpa_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len,
                                                 int64_t kv_len, int64_t head_dim) {
  return prefill_plan(sdpa_geom(batch, q_heads, kv_heads, q_len, kv_len, head_dim)).query_bytes;
}

extern "C" int mojo_hip_sdpa(const void* query, const void* key, const void* value, const void* mask, void* out,
                             int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len, int64_t kv_len,
                             int64_t head_dim, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride,
                             int64_t out_batch_stride, int64_t out_head_stride, int64_t out_token_stride,
                             int64_t kv_batch_stride, int64_t kv_head_stride, int64_t kv_token_stride, int mask_kind,
                             int64_t mask_batch_stride, int64_t mask_head_stride, int64_t mask_row_stride,
                             float softmax_scale, int dtype, void* workspace, int64_t workspace_bytes,
                             mojo_stream_t stream) {
  if (batch == 0 || q_len == 0 || q_heads == 0) return MOJO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MOJO_REQUIRE(query && key && value && out, MOJO_EINVAL, "sdpa: null pointer");
  MOJO_REQUIRE(batch > 0 && q_len > 0 && kv_len > 0, MOJO_EINVAL, "sdpa: batch %lld, Sq %lld, Sk %lld must be positive",
               (long long)batch, (long long)q_len, (long long)kv_len);
  MOJO_REQUIRE(q_heads > 0 && kv_heads > 0 && q_heads % kv_heads == 0, MOJO_EINVAL, "sdpa: bad head counts Hq=%lld Hkv=%lld",
               (long long)q_heads, (long long)kv_heads);
  MOJO_REQUIRE(dtype == MOJO_BF16 || dtype == MOJO_F16, MOJO_EUNSUPPORTED, "sdpa: dtype %d (bf16/fp16 only)", dtype);
  MOJO_REQUIRE(kv_len < (int64_t{1} << 30) && q_len < (int64_t{1} << 30), MOJO_EUNSUPPORTED,
               "sdpa: Sq %lld, Sk %lld (below 2^30 each)", (long long)q_len, (long long)kv_len);
  const int64_t strides[] = {q_batch_stride, q_head_stride, q_token_stride, out_batch_stride, out_head_stride, out_token_stride,
                             kv_batch_stride, kv_head_stride, kv_token_stride};
  for (const int64_t st : strides)
    MOJO_REQUIRE(st >= 0 && st % 8 == 0, MOJO_EUNSUPPORTED, "sdpa: strides must be non-negative multiples of 8 elements (16-byte rows)");
  MOJO_REQUIRE(aligned_to(query, 16) && aligned_to(key, 16) && aligned_to(value, 16) && aligned_to(out, 16), MOJO_EUNSUPPORTED,
               "sdpa: tensors must be 16-byte aligned");
  MOJO_REQUIRE(mask_kind >= 0 && mask_kind <= 3 && (mask_kind == 0) == (mask == nullptr), MOJO_EINVAL,
               "sdpa: mask_kind %d (0 none, 1 bool, 2 the query's dtype, 3 fp32) does not match the mask pointer", mask_kind);
  const PrefillGeom g = sdpa_geom(batch, q_heads, kv_heads, q_len, kv_len, head_dim);
  const PrefillPlan p = prefill_plan(g);
  const int G = static_cast<int>(q_heads / kv_heads);
  MOJO_REQUIRE(G == 1 || G == 2 || G == 4 || G == 8, MOJO_EUNSUPPORTED, "sdpa: group size %d (1, 2, 4, 8)", G);
  SdpaArgs a{};
  a.q = query; a.kc = key; a.vc = value; a.out = out;
  a.hq = static_cast<int>(q_heads); a.hkv = static_cast<int>(kv_heads); a.dim = static_cast<int>(head_dim);
  a.page = PF_KEYS; a.page_shift = 6; a.max_pages = static_cast<int>(kv_len);
  a.c_head = kv_head_stride; a.c_tok = kv_token_stride; a.kv_bs = kv_batch_stride;
  a.q_bs = q_batch_stride; a.q_hs = q_head_stride; a.q_ts = q_token_stride;
  a.o_bs = out_batch_stride; a.o_hs = out_head_stride; a.o_ts = out_token_stride;
  a.sq = static_cast<int>(q_len); a.sk = static_cast<int>(kv_len);
  a.scale_log2 = softmax_scale * 1.4426950408889634f;
  a.abab = 0;
  a.batch = static_cast<int>(batch);
  a.n_qb = static_cast<int>(p.n_qb);
  a.skew = 1;
  if (mask_kind) {
    // the lane's offset inside a (batch, head) plane of the mask is a 32-bit element count
    MOJO_REQUIRE(mask_batch_stride >= 0 && mask_head_stride >= 0 && mask_row_stride >= 0 &&
                     (q_len - 1) * mask_row_stride + kv_len + PF_KEYS < (int64_t{1} << 31),
                 MOJO_EUNSUPPORTED, "sdpa: a (batch, head) plane of the mask must stay below 2^31 elements");
    const size_t esz = mask_kind == 1 ? 1 : (mask_kind == 2 ? 2 : 4);
    a.mask = mask; a.mask_kind = mask_kind;
    a.m_bs = mask_batch_stride; a.m_hs = mask_head_stride; a.m_rs = mask_row_stride;
    a.mask_vec = (mask_batch_stride % 4 == 0 && mask_head_stride % 4 == 0 && mask_row_stride % 4 == 0 && aligned_to(mask, 4 * esz)) ? 1 : 0;
  }
  const bool no_fs = MOJO_SWITCH("MOJO_HIP_PREFILL_FAST_STAGE", 1) == 0;        // 0: general staging everywhere (tests)
  a.fast_stage = (kv_token_stride * 16 * 2 + 256 < (int64_t{1} << 31) && !no_fs) ? 1 : 0;
  const bool split = p.ksplit > 1 && workspace && workspace_bytes >= p.bytes && aligned_to(workspace, 16);
  a.ksplit = split ? p.ksplit : 1;
  a.ws_o = split ? static_cast<float*>(workspace) : nullptr;
  a.ws_ml = split ? a.ws_o + p.rows * head_dim : nullptr;
  const int64_t blocks = p.n_qb * kv_heads * batch * a.ksplit;
  MOJO_REQUIRE(blocks < (int64_t{1} << 31), MOJO_EUNSUPPORTED, "sdpa: grid limit");
  const dim3 grid(static_cast<unsigned>(blocks));
  if (dtype == MOJO_BF16) return mask_kind ? sdpa_g<bf16_t, true>(a, G, grid, s) : sdpa_g<bf16_t, false>(a, G, grid, s);
  return mask_kind ? sdpa_g<f16_t, true>(a, G, grid, s) : sdpa_g<f16_t, false>(a, G, grid, s);
}
