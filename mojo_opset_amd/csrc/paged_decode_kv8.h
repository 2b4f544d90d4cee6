// decode_kv8_kernel: MojoPagedDecodeGQAWithKVDequant — paged decode over an int8 K/V cache with per-channel scales.
// Included at the end of paged_decode_gqa.hip: shares DecodeArgs, the chunking rules, decode_head and the merge kernel with the
// 16-bit op, and through paged_decode_common.h the row prologue, the hole scan, the in-LDS merge, the split epilogue and the
// softmax step (fp16 probabilities: dec_mma<f16_t>::pack); the entry points fill the 16-bit ops' DecodeCall.
//
// The scales never meet a K or V element:
//   q'[h, d] = q[h, d] * key_scale[kvh, d]             once per wave, fp32 product rounded to fp16
//   S[h, t]  = softmax_scale * sum_d q'[h, d] K8[t, d]
//   O[h, d]  = value_scale[kvh, d] * sum_t P[h, t] V8[t, d] / l[h]       (applied to the fp32 sums of a wave, before the merge)
// Both contractions run on the matrix cores in fp16 WHATEVER the query dtype: an int8 x is the fp16 number
// (0x6400 | (x ^ 0x80)) - 1152 exactly, so one v_perm_b32 and one packed subtract unpack two elements.  Outputs leave in the
// query dtype.  fp16 probabilities are finer than the golden's bf16 ones.  RANGE: q' lives in fp16 also for bf16 queries —
// |q * key_scale| above 65504 saturates and below 6.1e-5 loses bits as a subnormal (below 6e-8: zero), a restriction the
// 16-bit op and the golden do not have; realistic products (|q| ~ 1..100, key_scale = amax / 127 ~ 1e-3..1) are far inside.
//
//   S^T[16 tokens x 16 heads] = K Q'^T   v_mfma_f32_16x16x32_f16: lane (token tl = l & 15, k-group g4 = l >> 4) loads the
//                                        16-byte pieces g4 + 4 i of its token's row (i < NI); a piece is two k-slices of 8.
//                                        The query operand holds the same dims in the same slots; pieces past the head
//                                        (head_dim 80 / 96) meet a zero query slice.
//   O^T[D x 16 heads] += V^T P^T         v_mfma_f32_16x16x16_f16: P is the accumulator of S^T as it lies; V^T comes from a
//                                        wave-private fp16 image of the tile ([16 tokens][2 D + 32 bytes]: the 32-byte pad
//                                        spreads the rows of a transposed read over the banks) read with ds_read_b64_tr_b16.
// V is loaded in whole rows (at head_dim 128 a load instruction moves eight 128-byte lines).  A step is 32 tokens
// (two sub-tiles), three steps in flight.  Launch forms: FUSED (<= 8 chunks per row: one workgroup, merged in LDS) and
// split + decode_merge_kernel; no paired and no grouped form.
//
// SWA (MojoPagedDecodeSWAWithKVDequant): the windowed instance walks the VIRTUAL key range of DecodeWin — the row length, the
// chunking, both launch forms and the tail mask all run on it.  Each 16-token sub-tile of a step maps virtual -> real on its
// own (g_al is a multiple of 16, not of the 32-token step: one step can hold the last global sub-tile and the first local
// one); the sub-tiles holding g1 or lo get the per-key visibility mask on their scores.  Every sub-tile walked holds a
// visible key, so only pages of the visible set are addressed: there is no hole scan, pages outside the window may be -1 or
// recycled, and a negative id inside the visible set reads page 0 (as the 16-bit SWA op).  Invisible V rows are not zeroed:
// int8 -> fp16 is always finite and their probabilities are exact zeros.
#pragma once

namespace mojo {

struct Kv8Args {
  DecodeArgs a;
  const void* kscale;            // [Hkv][D]
  const void* vscale;            // [Hkv][D]
  int scale_dtype;               // MOJO_F32 / MOJO_F16 / MOJO_BF16
  int q_bf16;                    // query / output dtype: 1 = bf16, 0 = fp16
};

// the output store of the shared merge and split epilogue, in the query's run-time dtype
struct Kv8Store {
  void* out;
  int bf16;
  __device__ __forceinline__ void operator()(int64_t at, f32x4 x) const {
    if (bf16) Store16<bf16_t>{out}(at, x);
    else Store16<f16_t>{out}(at, x);
  }
};

// four int8 of a dword -> four fp16 (exact): elements 0, 1 in `lo`, 2, 3 in `hi`
__device__ __forceinline__ void kv8_unpack4(unsigned w, f16x2& lo, f16x2& hi) {
  const unsigned x = w ^ 0x80808080u;
  const f16x2 bias = {static_cast<f16_t>(1152.0f), static_cast<f16_t>(1152.0f)};
  lo = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0x64646464u, x, 0x04010400u)) - bias;
  hi = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0x64646464u, x, 0x04030402u)) - bias;
}
__device__ __forceinline__ f16x8 kv8_unpack8(unsigned w0, unsigned w1) {
  f16x2 a, b, c, d;
  kv8_unpack4(w0, a, b);
  kv8_unpack4(w1, c, d);
  const f16x8 r = {a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
  return r;
}

constexpr int KV8_NS = 2;                      // sub-tiles of 16 tokens per loop step
constexpr int KV8_STEP = 16 * KV8_NS;

// floats of the partial area in front of the V images (rounded so that the images stay 16-byte aligned)
__host__ __device__ constexpr int kv8_part_floats(int waves, int G, int D) { return (waves * G * (D + 2) + 3) & ~3; }

template <int CPR /* head_dim / 16 */, bool NT, bool FUSED, bool SWA = false>
__global__ __launch_bounds__(512) void decode_kv8_kernel(Kv8Args ka, int G) {   // (512 for the one-wave form too: two waves per SIMD)
  const DecodeArgs& a = ka.a;
  constexpr int D = CPR * 16, ND = CPR;
  constexpr int NI = (CPR + 3) / 4;                     // K pieces per lane
  constexpr int NS = KV8_NS, STEP = KV8_STEP;
  constexpr int RPI = 64 / CPR > 16 ? 16 : 64 / CPR;    // V rows per load instruction (16, 12, 10, 8)
  constexpr int NV = (16 + RPI - 1) / RPI;              // V load instructions per sub-tile
  constexpr int VSTRIDE = D * 2 + 32;                   // bytes of an image row
  constexpr int IMG = 16 * VSTRIDE;
  const int lane = threadIdx.x & 63;
  const int tl = lane & 15, g4 = lane >> 4;
  const int wave_id = FUSED ? __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)) : 0;
  const int chunk = FUSED ? wave_id : static_cast<int>(blockIdx.x);
  const int b = blockIdx.y / a.hkv;
  const int kvh = blockIdx.y % a.hkv;

  DecodeWin win;                                        // (SWA only; the row's length is then the virtual one)
  const DecodeRow row = decode_row(a, b, chunk, decode_row_len<SWA>(a, b, win));
  const int tok_begin = row.tok_begin, tok_end = row.tok_end;
  const bool has_work = row.has_work;
  if (!FUSED && !has_work) return;

  // query operand: lane (head tl, k-group g4), piece g4 + 4 i, half hh -> dims 16 (g4 + 4 i) + 8 hh .. + 7, scaled
  const int hq_l = min(tl, G - 1);                      // lanes past the group repeat its last head (computed, never stored)
  f16x8 qf[NI][2];
  {
    const int h = decode_head(a, kvh, hq_l, G);
    const int64_t qrow = (static_cast<int64_t>(b) * a.hq + h) * D;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int c = g4 + 4 * i;
        const bool ok = c < CPR;
        const int d0 = 16 * min(c, CPR - 1) + 8 * hh;
        float qv[8], sv[8];
        load_coded_f32_vec<8>(a.q, ka.q_bf16 ? MOJO_BF16 : MOJO_F16, qrow + d0, qv);
        load_coded_f32_vec<8>(ka.kscale, ka.scale_dtype, static_cast<int64_t>(kvh) * D + d0, sv);
        f16x8 x;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          // (fp16 range: a product beyond +-65504 saturates instead of turning into inf and a NaN row; below 6e-5 it is subnormal)
          const float v = qv[e] * sv[e];
          x[e] = ok ? static_cast<f16_t>(fminf(fmaxf(v, -65504.0f), 65504.0f)) : static_cast<f16_t>(0.0f);
        }
        qf[i][hh] = x;
      }
  }

  f32x4 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  const int32_t* table = a.tables + static_cast<int64_t>(b) * a.table_stride;
  // holes: as the 16-bit kernels — the pages at and behind the first negative id read as zeros; the scan does not gate the loads
  DecodeHoles holes(a, tok_end);
  if (!SWA && has_work) holes.issue(table, lane, 0);    // (SWA: no hole scan — pages outside the window may hold anything)

  const int vr = lane / CPR, vc = lane % CPR;           // V: row vr of a load instruction, piece vc of the row
  const bool v_lane = vr < RPI;
  const char* kbase = static_cast<const char*>(a.kc) + static_cast<int64_t>(kvh) * a.c_head + static_cast<int64_t>(tl) * a.c_tok;
  const char* vbase = static_cast<const char*>(a.vc) + static_cast<int64_t>(kvh) * a.c_head + vc * 16;
  int koff[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) koff[i] = 16 * min(g4 + 4 * i, CPR - 1);
  int64_t voff[NV];
  bool v_ok[NV];
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int row = RPI * u + min(vr, RPI - 1);
    v_ok[u] = v_lane && row < 16;
    voff[u] = static_cast<int64_t>(min(row, 15)) * a.c_tok;
  }
  const int last_tile = ((tok_end - 1) / 16) * 16;      // first token of the last non-empty sub-tile (SWA: virtual)
  const int last_page = a.max_pages - 1;

  struct Tile { u32x4 k[NS][NI]; u32x4 v[NS][NV]; int lp[NS]; };
  auto ld = [&](const char* p) -> u32x4 {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    else return *reinterpret_cast<const u32x4*>(p);
  };
  // Branch-free: every load is issued, clamped to an address that certainly exists (a sub-tile lies in one page: 16 | page)
  auto load_tile = [&](Tile& t, int t0) {
#pragma unroll
    for (int ss = 0; ss < NS; ++ss) {
      int tu = min(t0 + 16 * ss, last_tile);            // wave-uniform
      if constexpr (SWA) tu = decode_swa_real(win, tu); // (16-aligned cuts: the sub-tile stays whole, in one page)
      const int lp = a.page_shift >= 0 ? (tu >> a.page_shift) : tu / a.page;
      t.lp[ss] = lp;
      const int phys = max(table[min(lp, last_page)], 0);
      const int64_t pg = static_cast<int64_t>(phys) * a.c_blk + static_cast<int64_t>(tu - lp * a.page) * a.c_tok;
#pragma unroll
      for (int i = 0; i < NI; ++i) t.k[ss][i] = ld(kbase + pg + koff[i]);
#pragma unroll
      for (int u = 0; u < NV; ++u) t.v[ss][u] = ld(vbase + pg + voff[u]);
    }
  };

  extern __shared__ float s_part[];                     // [waves][G][D + 2] partials (FUSED), then [waves][NS] V images
  const int n_waves = FUSED ? static_cast<int>(blockDim.x >> 6) : 1;
  char* const v_img = reinterpret_cast<char*>(s_part + (FUSED ? kv8_part_floats(n_waves, G, D) : 0)) + wave_id * (NS * IMG);
  const unsigned v_u32 = static_cast<unsigned>(reinterpret_cast<size_t>(v_img));
  // transposed read of d tile dt: lane (g4, tl) reads 8 bytes of row 4 g4 + (tl >> 2) at columns 16 dt + 4 (tl & 3) .. + 3 and
  // receives d = 16 dt + tl of the tokens 4 g4 .. 4 g4 + 3
  const unsigned r_base = v_u32 + (4 * g4 + (tl >> 2)) * VSTRIDE + (tl & 3) * 8;

  auto process = [&](Tile& t, int t0) {
    if constexpr (!SWA) {
#pragma unroll
    for (int ss = 0; ss < NS; ++ss)
      if (t.lp[ss] >= holes.first_neg) {                     // rare: pages behind a hole read as zeros
        const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < NI; ++i) t.k[ss][i] = z;
#pragma unroll
        for (int u = 0; u < NV; ++u) t.v[ss][u] = z;
      }
    }
    const bool full = t0 + STEP <= tok_end;             // wave-uniform
    float x[NS][4];
#pragma unroll
    for (int ss = 0; ss < NS; ++ss) {
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(kv8_unpack8(t.k[ss][i][0], t.k[ss][i][1]), qf[i][0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(kv8_unpack8(t.k[ss][i][2], t.k[ss][i][3]), qf[i][1], c, 0, 0, 0);
      }
      // stage V as fp16 while the scores come out of the matrix pipe.  Rows past the length hold int8 of whatever page the
      // clamped load read: finite as fp16, and their probabilities are exact zeros.
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        if (v_ok[u]) {
          const int row = RPI * u + vr;
          char* dst = v_img + ss * IMG + row * VSTRIDE + vc * 32;
          *reinterpret_cast<f16x8*>(dst) = kv8_unpack8(t.v[ss][u][0], t.v[ss][u][1]);
          *reinterpret_cast<f16x8*>(dst + 16) = kv8_unpack8(t.v[ss][u][2], t.v[ss][u][3]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) x[ss][i] = c[i] * a.scale_log2;   // token 16 ss + 4 g4 + i, head tl
    }
    if (!full) {
#pragma unroll
      for (int ss = 0; ss < NS; ++ss)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (!(t0 + 16 * ss + 4 * g4 + i < tok_end)) x[ss][i] = -INFINITY;
    }
    if constexpr (SWA) {                                // the sub-tiles holding g1 or lo: per-key visibility (real positions)
#pragma unroll
      for (int ss = 0; ss < NS; ++ss) {
        const int rt0 = decode_swa_real(win, t0 + 16 * ss);
        if (decode_swa_edge(win, rt0)) {                // wave-uniform
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (!decode_swa_vis(win, rt0 + 4 * g4 + i)) x[ss][i] = -INFINITY;
        }
      }
    }
    f16x4 pf[NS];
    decode_softmax_step<dec_mma<f16_t>>(x, m, l, o, pf);   // (fp16 probabilities whatever the query dtype; below 2^8)
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int ss = 0; ss < NS; ++ss) {
        const s16x4 vt = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            reinterpret_cast<__attribute__((address_space(3))) s16x4*>(static_cast<uintptr_t>(r_base + ss * IMG + dt * 32)));
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, vt), pf[ss], o[dt], 0, 0, 0);
      }
  };

  Tile ta, tb, tc;
  if (has_work) {
    load_tile(ta, tok_begin);
    if (tok_begin + STEP < tok_end) load_tile(tb, tok_begin + STEP);
    if constexpr (!SWA) holes.finish(table, lane);
    for (int t0 = tok_begin; t0 < tok_end; t0 += 3 * STEP) {
      if (t0 + 2 * STEP < tok_end) load_tile(tc, t0 + 2 * STEP);
      process(ta, t0);
      if (t0 + STEP >= tok_end) break;
      if (t0 + 3 * STEP < tok_end) load_tile(ta, t0 + 3 * STEP);
      process(tb, t0 + STEP);
      if (t0 + 2 * STEP >= tok_end) break;
      if (t0 + 4 * STEP < tok_end) load_tile(tb, t0 + 4 * STEP);
      process(tc, t0 + 2 * STEP);
    }
  }

  l = xor_sum_16_32(l);
  // lane holds head tl, dims 16 dt + 4 g4 + i: the value scales meet the fp32 sums here, once
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) {
    float sv[4];
    load_coded_f32_vec<4>(ka.vscale, ka.scale_dtype, static_cast<int64_t>(kvh) * D + 16 * dt + 4 * g4, sv);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[dt][i] *= sv[i];
  }
  const Kv8Store store{a.out, ka.q_bf16};
  if constexpr (FUSED) {
    if (tl < G) {
      float* dst = s_part + (wave_id * G + tl) * (D + 2);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[dt * 16 + 4 * g4 + i] = o[dt][i];
      if (g4 == 0) { dst[D] = m; dst[D + 1] = l; }
    }
    decode_lds_merge<false, false>(a, s_part, D, G, kvh, row, DecodePair{}, store);
    return;
  }
  decode_split_finish(a, G, kvh, row, tl, g4, o, m, l, store);
}

template <int CPR, bool NT, bool SWA>
static int launch_decode_kv8_cpr(const Kv8Args& ka, int64_t batch, int G, hipStream_t s) {
  const DecodeArgs& a = ka.a;
  constexpr int D = CPR * 16;
  constexpr size_t IMG = static_cast<size_t>(KV8_NS) * 16 * (D * 2 + 32);
  const char* nt_tag = NT ? "nt" : "cached";
  const char* swa_tag = SWA ? ":swa" : "";
  const unsigned rows = static_cast<unsigned>(batch * a.hkv);
  if (a.n_chunks <= 8 && MOJO_SWITCH("MOJO_HIP_DECODE_FUSE", 1) != 0) {
    const size_t lds = static_cast<size_t>(kv8_part_floats(a.n_chunks, G, D)) * sizeof(float) + a.n_chunks * IMG;
    static std::atomic<uint64_t> attr_set{0};           // (per instantiation: dynamic LDS beyond 64 KiB needs the attribute)
    if (first_call_on_device(attr_set))
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&decode_kv8_kernel<CPR, NT, true, SWA>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL((decode_kv8_kernel<CPR, NT, true, SWA>), dim3(1, rows), dim3(static_cast<unsigned>(64 * a.n_chunks)), lds, s, ka, G);
    MOJO_CHECK_LAUNCH("paged_decode_gqa_kv8(fused)");
    note_launch("decode_mfma:fused:%s:kv8%s", nt_tag, swa_tag);
    return MOJO_OK;
  }
  hipLaunchKernelGGL((decode_kv8_kernel<CPR, NT, false, SWA>), dim3(static_cast<unsigned>(a.n_chunks), rows), dim3(64), IMG, s, ka, G);
  MOJO_CHECK_LAUNCH("paged_decode_gqa_kv8(split)");
  if (ka.q_bf16) hipLaunchKernelGGL((decode_merge_kernel<bf16_t, SWA>), dim3(rows, G), dim3(256), 0, s, a, G);
  else hipLaunchKernelGGL((decode_merge_kernel<f16_t, SWA>), dim3(rows, G), dim3(256), 0, s, a, G);
  MOJO_CHECK_LAUNCH("paged_decode_gqa_kv8(merge)");
  note_launch("decode_mfma:split+merge:%s:kv8%s", nt_tag, swa_tag);
  return MOJO_OK;
}

template <bool NT, bool SWA>
static int launch_decode_kv8(const Kv8Args& ka, int64_t batch, int G, hipStream_t s) {
  switch (ka.a.dim) {
    case 64: return launch_decode_kv8_cpr<4, NT, SWA>(ka, batch, G, s);
    case 80: return launch_decode_kv8_cpr<5, NT, SWA>(ka, batch, G, s);
    case 96: return launch_decode_kv8_cpr<6, NT, SWA>(ka, batch, G, s);
    case 128: return launch_decode_kv8_cpr<8, NT, SWA>(ka, batch, G, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "paged_decode_gqa_kv8: head_dim %d (supported: 64, 80, 96, 128)", ka.a.dim);
  }
  return MOJO_OK;
}

}  // namespace mojo

// What the int8-cache entry points check (`op`: the entry point's name in the messages).
static int decode_kv8_check_call(const DecodeCall& c, const char* op) {
  using namespace mojo;
  const DecodeGeom& g = c.g;
  if (const int rc = decode_check_call(c, op); rc != MOJO_OK) return rc;
  MOJO_REQUIRE(c.scale_dtype == MOJO_BF16 || c.scale_dtype == MOJO_F16 || c.scale_dtype == MOJO_F32, MOJO_EUNSUPPORTED,
               "%s: scale dtype %d (bf16/fp16/fp32 only)", op, c.scale_dtype);
  MOJO_REQUIRE(g.head_dim == 64 || g.head_dim == 80 || g.head_dim == 96 || g.head_dim == 128, MOJO_EUNSUPPORTED,
               "%s: head_dim %lld (supported: 64, 80, 96, 128)", op, (long long)g.head_dim);
  MOJO_REQUIRE(g.page > 0 && g.page % 16 == 0, MOJO_EUNSUPPORTED,
               "%s: block_size %lld must be a multiple of 16", op, (long long)g.page);
  MOJO_REQUIRE(g.q_heads / g.kv_heads <= 16, MOJO_EUNSUPPORTED, "%s: group size %lld (supported: 1..16)", op,
               (long long)(g.q_heads / g.kv_heads));
  MOJO_REQUIRE(c.cache_token_stride % 16 == 0 && c.cache_head_stride % 16 == 0 && c.cache_block_stride % 16 == 0 &&
                   aligned_to(c.key_cache, 16) && aligned_to(c.value_cache, 16) && aligned_to(c.query, 16) && aligned_to(c.out, 16) &&
                   aligned_to(c.key_scale, 16) && aligned_to(c.value_scale, 16),
               MOJO_EUNSUPPORTED, "%s: tensors must be 16-byte aligned with 16-byte row strides", op);
  return MOJO_OK;
}

// The kernel arguments of a planned int8-cache call.
static int decode_kv8_fill_args(mojo::Kv8Args& ka, const DecodeCall& c, const mojo::DecodePlan& p) {
  using namespace mojo;
  if (p.swa) {
    if (const int rc = decode_set_window(ka.a, c, p, "paged_decode_swa_kv8"); rc != MOJO_OK) return rc;
  }
  if (const int rc = decode_fill_args(ka.a, c, p, "paged_decode_gqa_kv8"); rc != MOJO_OK) return rc;
  ka.kscale = c.key_scale; ka.vscale = c.value_scale; ka.scale_dtype = c.scale_dtype; ka.q_bf16 = c.dtype == MOJO_BF16 ? 1 : 0;
  return MOJO_OK;
}

// The int8-cache entry points share one body: a window (local >= 0 or global > 0) selects the windowed instances, planned on
// the visible capacity (decode_swa_cap); none runs the unwindowed op, whichever entry point was called.
static int paged_decode_kv8(const DecodeCall& c) {
  using namespace mojo;
  const DecodeGeom& g = c.g;
  if (g.batch == 0) return MOJO_OK;
  if (const int rc = decode_kv8_check_call(c, "paged_decode_gqa_kv8"); rc != MOJO_OK) return rc;
  const DecodePlan p = decode_plan(g);
  Kv8Args ka{};
  if (const int rc = decode_kv8_fill_args(ka, c, p); rc != MOJO_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(c.stream);
  const bool nt = MOJO_SWITCH("MOJO_HIP_STREAM_NT", -1) != 0;
  if (p.swa) return nt ? launch_decode_kv8<true, true>(ka, g.batch, p.G, s) : launch_decode_kv8<false, true>(ka, g.batch, p.G, s);
  return nt ? launch_decode_kv8<true, false>(ka, g.batch, p.G, s) : launch_decode_kv8<false, false>(ka, g.batch, p.G, s);
}

extern "C" int64_t mojo_hip_paged_decode_gqa_kv8_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                                 int64_t head_dim, int64_t block_size,
                                                                 int64_t max_blocks_per_seq, int64_t max_seq_len_hint) {
  return mojo::decode_plan({batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_seq_len_hint, -1, 0, /*kv8=*/true}).query_bytes;
}

extern "C" int64_t mojo_hip_paged_decode_swa_kv8_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                                 int64_t head_dim, int64_t block_size,
                                                                 int64_t max_blocks_per_seq, int64_t max_seq_len_hint,
                                                                 int64_t local_window, int64_t global_window) {
  return mojo::decode_plan({batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_seq_len_hint, local_window,
                            global_window, /*kv8=*/true}).query_bytes;
}

extern "C" int mojo_hip_paged_decode_swa_kv8(const void* query, const void* key_cache, const void* key_scale,
                                             const void* value_cache, const void* value_scale,
                                             const int32_t* total_seq_lens, const int32_t* block_tables, void* out,
                                             void* workspace, int64_t workspace_bytes, int64_t batch, int64_t q_heads,
                                             int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                             int64_t max_blocks_per_seq, int64_t block_table_stride,
                                             int64_t cache_block_stride, int64_t cache_head_stride,
                                             int64_t cache_token_stride, int64_t max_seq_len_hint, float softmax_scale,
                                             int layout_abab, int leave_empty_rows, int dtype, int scale_dtype,
                                             int64_t local_window, int64_t global_window, mojo_stream_t stream) {
  DecodeCall c;
  c.query = query; c.key_cache = key_cache; c.value_cache = value_cache; c.total_seq_lens = total_seq_lens; c.block_tables = block_tables;
  c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.g = {batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_seq_len_hint, local_window, global_window, /*kv8=*/true};
  c.block_table_stride = block_table_stride; c.cache_block_stride = cache_block_stride; c.cache_head_stride = cache_head_stride;
  c.cache_token_stride = cache_token_stride; c.softmax_scale = softmax_scale; c.layout_abab = layout_abab;
  c.leave_empty_rows = leave_empty_rows; c.dtype = dtype;
  c.key_scale = key_scale; c.value_scale = value_scale; c.scale_dtype = scale_dtype;
  return paged_decode_kv8(c);
}

extern "C" int mojo_hip_paged_decode_gqa_kv8(const void* query, const void* key_cache, const void* key_scale,
                                             const void* value_cache, const void* value_scale,
                                             const int32_t* total_seq_lens, const int32_t* block_tables, void* out,
                                             void* workspace, int64_t workspace_bytes, int64_t batch, int64_t q_heads,
                                             int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                             int64_t max_blocks_per_seq, int64_t block_table_stride,
                                             int64_t cache_block_stride, int64_t cache_head_stride,
                                             int64_t cache_token_stride, int64_t max_seq_len_hint, float softmax_scale,
                                             int layout_abab, int leave_empty_rows, int dtype, int scale_dtype,
                                             mojo_stream_t stream) {
  // (no window: the windowed entry point runs the unwindowed op itself)
  return mojo_hip_paged_decode_swa_kv8(query, key_cache, key_scale, value_cache, value_scale, total_seq_lens, block_tables, out, workspace,
                                       workspace_bytes, batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq,
                                       block_table_stride, cache_block_stride, cache_head_stride, cache_token_stride, max_seq_len_hint,
                                       softmax_scale, layout_abab, leave_empty_rows, dtype, scale_dtype, /*local_window=*/-1,
                                       /*global_window=*/0, stream);
}
