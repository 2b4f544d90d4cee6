// decode_kv8_nstep_kernel: MojoPagedDecodeNstepSWAWithKVDequant — `S` query rows per sequence over the int8 K/V cache.
// Included at the end of paged_decode_gqa.hip, behind paged_decode_kv8.h.
//
// It is decode_kv8_kernel — tile layouts, loads, ring, unpacking and softmax step as there, written out again: with one body
// included into both kernels, 20 of the 32 single-step instances were allocated other registers — with the
// n-step pieces of decode_mfma_nstep_kernel (DecodeSteps) in place:
//   grid     a row is a block of SB = 16 / G steps of one (sequence, kv head): decode_nstep_row; `steps` and the hole-scan
//            flag travel in the `int G` argument (decode_nstep_arg) — Kv8Args and DecodeArgs stay as they are
//   query    column tl = (step tl / G, head tl % G); a lane's slice comes from decode_col_at, is scaled by key_scale and clamped
//            to the fp16 range as in the single-step kernel; columns failing decode_col_ok are computed and never stored
//   mask     the block walks the DecodeWin of its last step from the lower edge of its first; a 16-token sub-tile is an edge
//            tile per decode_nstep_edge, and there a lane masks its four scores against its own step's upper and lower edge.
//            No window runs as a local window of the capacity, with the hole scan on
//   epilogue value_scale meets the fp32 sums once; decode_lds_merge_nstep / decode_split_finish_nstep with Kv8Store; the
//            split form ends with decode_merge_nstep_kernel
// Launch forms: FUSED (<= 8 chunks per row) and split + merge, as the single-step int8 kernel; with S > SB the blocks go on
// the grid and each streams K/V itself.  LDS of the fused form at head_dim 128: 8 waves x 16 columns x 130 floats of
// partials + 8 x 2 V images of 16 x 288 bytes = 140 288 bytes, inside the 160 KiB the family requests.
#pragma once

namespace mojo {

// `G` arrives as decode_nstep_arg(heads per kv head, steps, scan_holes)
template <int CPR /* head_dim / 16 */, bool NT, bool FUSED>
__global__ __launch_bounds__(512) void decode_kv8_nstep_kernel(Kv8Args ka, int G) {
  const int steps = (G >> 8) & 0xffff;                  // (G arrives as decode_nstep_arg)
  const bool scan_holes = (G >> 24) != 0;
  G &= 0xff;
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

  DecodeWin win;                                        // the block's window; the row's length is the virtual one
  DecodeSteps st;                                       // a grid row is a block of steps of one (sequence, kv head)
  const int vlen = decode_nstep_row(a, blockIdx.y, G, steps, win, st);
  const int b = st.b, kvh = st.kvh;
  const DecodeRow row = decode_row(a, b, chunk, a.max_pages > 0 ? vlen : 0);
  const int tok_begin = row.tok_begin, tok_end = row.tok_end;
  const bool has_work = row.has_work;
  if (!FUSED && !has_work) return;

  // query operand: lane (column tl = (step, head), k-group g4), piece g4 + 4 i, half hh -> dims 16 (g4 + 4 i) + 8 hh .. + 7,
  // scaled.  Lanes past the block's columns repeat its last one (computed, never stored).  The lane's step sees the keys
  // t <= vis_hi with t < st.gl or t >= vis_lo.
  const int NC = (16 / G) * G;                          // columns of a partial
  const int col_l = min(tl, st.nst * G - 1);
  const int vis_hi = win.len - st.nst + col_l / G;
  const int vis_lo = a.local_win >= 0 ? max(vis_hi - a.local_win, 0) : 0x7fffffff;
  f16x8 qf[NI][2];
  {
    const int64_t qrow = decode_col_at(a, st, col_l);
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
  // holes (no window set: virtual = real tokens): the pages at and behind the first negative id read as zeros; the scan does
  // not gate the loads.  With a window there is no scan — pages outside it may hold anything
  DecodeHoles holes(a, tok_end);
  if (scan_holes && has_work) holes.issue(table, lane, 0);

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
  const int last_tile = ((tok_end - 1) / 16) * 16;      // first token of the last non-empty sub-tile (virtual)
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
      tu = decode_swa_real(win, tu);                    // (16-aligned cuts: the sub-tile stays whole, in one page)
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

  extern __shared__ float s_part[];                     // [waves][NC][D + 2] partials (FUSED), then [waves][NS] V images
  const int n_waves = FUSED ? static_cast<int>(blockDim.x >> 6) : 1;
  char* const v_img = reinterpret_cast<char*>(s_part + (FUSED ? kv8_part_floats(n_waves, NC, D) : 0)) + wave_id * (NS * IMG);
  const unsigned v_u32 = static_cast<unsigned>(reinterpret_cast<size_t>(v_img));
  // transposed read of d tile dt: lane (g4, tl) reads 8 bytes of row 4 g4 + (tl >> 2) at columns 16 dt + 4 (tl & 3) .. + 3 and
  // receives d = 16 dt + tl of the tokens 4 g4 .. 4 g4 + 3
  const unsigned r_base = v_u32 + (4 * g4 + (tl >> 2)) * VSTRIDE + (tl & 3) * 8;

  auto process = [&](Tile& t, int t0) {
#pragma unroll
    for (int ss = 0; ss < NS; ++ss)
      if (t.lp[ss] >= holes.first_neg) {                // rare: pages behind a hole read as zeros (with a window: never)
        const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < NI; ++i) t.k[ss][i] = z;
#pragma unroll
        for (int u = 0; u < NV; ++u) t.v[ss][u] = z;
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
    // the sub-tiles not every step of the block sees whole: the lane's own step decides (real positions)
#pragma unroll
    for (int ss = 0; ss < NS; ++ss) {
      const int rt0 = decode_swa_real(win, t0 + 16 * ss);
      if (decode_nstep_edge(win, st, rt0)) {            // wave-uniform
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = rt0 + 4 * g4 + i;
          if (!(t <= vis_hi && (t < st.gl || t >= vis_lo))) x[ss][i] = -INFINITY;
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
    if (scan_holes) holes.finish(table, lane);
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
  // The epilogue reads its arguments from the kernel-argument segment again, through an opaque copy of the segment's address:
  // the two dozen scalars it alone needs (output, value scales, workspace, head counts, ...) are then not held from the
  // kernel's entry across the loop, where together with the block's DecodeSteps they went past the scalar registers a wave
  // has (1 to 12 of them were parked in lanes of a vector register).
  auto late = __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(late));
  const Kv8Args& ke = *(const Kv8Args*)late;            // (the first kernel argument: offset 0)
  const DecodeArgs& ae = ke.a;
  // lane holds column tl, dims 16 dt + 4 g4 + i: the value scales meet the fp32 sums here, once
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) {
    float sv[4];
    load_coded_f32_vec<4>(ke.vscale, ke.scale_dtype, static_cast<int64_t>(kvh) * D + 16 * dt + 4 * g4, sv);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[dt][i] *= sv[i];
  }
  const Kv8Store store{ae.out, ke.q_bf16};
  if constexpr (FUSED) {
    if (tl < NC) {
      float* dst = s_part + (wave_id * NC + tl) * (D + 2);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[dt * 16 + 4 * g4 + i] = o[dt][i];
      if (g4 == 0) { dst[D] = m; dst[D + 1] = l; }
    }
    decode_lds_merge_nstep(ae, s_part, D, NC, row, st, store);
    return;
  }
  decode_split_finish_nstep(ae, NC, row, st, tl, g4, o, m, l, store);
}

template <int CPR, bool NT>
static int launch_decode_kv8_nstep_cpr(const Kv8Args& ka, const DecodePlan& p, int64_t batch, hipStream_t s) {
  const DecodeArgs& a = ka.a;
  constexpr int D = CPR * 16;
  constexpr size_t IMG = static_cast<size_t>(KV8_NS) * 16 * (D * 2 + 32);
  const char* nt_tag = NT ? "nt" : "cached";
  const unsigned rows = static_cast<unsigned>(batch * a.hkv * p.row_blocks);
  const int arg = decode_nstep_arg(p.G, p.steps, p.scan_holes);
  if (a.n_chunks <= 8 && MOJO_SWITCH("MOJO_HIP_DECODE_FUSE", 1) != 0) {
    const size_t lds = static_cast<size_t>(kv8_part_floats(a.n_chunks, p.cols, D)) * sizeof(float) + a.n_chunks * IMG;
    static std::atomic<uint64_t> attr_set{0};           // (per instantiation: dynamic LDS beyond 64 KiB needs the attribute)
    if (first_call_on_device(attr_set))
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&decode_kv8_nstep_kernel<CPR, NT, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL((decode_kv8_nstep_kernel<CPR, NT, true>), dim3(1, rows), dim3(static_cast<unsigned>(64 * a.n_chunks)), lds, s, ka, arg);
    MOJO_CHECK_LAUNCH("paged_decode_nstep_kv8(fused)");
    note_launch("decode_mfma:fused:%s:kv8:nstep", nt_tag);
    return MOJO_OK;
  }
  hipLaunchKernelGGL((decode_kv8_nstep_kernel<CPR, NT, false>), dim3(static_cast<unsigned>(a.n_chunks), rows), dim3(64), IMG, s, ka, arg);
  MOJO_CHECK_LAUNCH("paged_decode_nstep_kv8(split)");
  if (ka.q_bf16) hipLaunchKernelGGL((decode_merge_nstep_kernel<bf16_t>), dim3(rows, p.cols), dim3(256), 0, s, a, p.G, p.steps);
  else hipLaunchKernelGGL((decode_merge_nstep_kernel<f16_t>), dim3(rows, p.cols), dim3(256), 0, s, a, p.G, p.steps);
  MOJO_CHECK_LAUNCH("paged_decode_nstep_kv8(merge)");
  note_launch("decode_mfma:split+merge:%s:kv8:nstep", nt_tag);
  return MOJO_OK;
}

template <bool NT>
static int launch_decode_kv8_nstep(const Kv8Args& ka, const DecodePlan& p, int64_t batch, hipStream_t s) {
  switch (ka.a.dim) {
    case 64: return launch_decode_kv8_nstep_cpr<4, NT>(ka, p, batch, s);
    case 80: return launch_decode_kv8_nstep_cpr<5, NT>(ka, p, batch, s);
    case 96: return launch_decode_kv8_nstep_cpr<6, NT>(ka, p, batch, s);
    case 128: return launch_decode_kv8_nstep_cpr<8, NT>(ka, p, batch, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "paged_decode_nstep_kv8: head_dim %d (supported: 64, 80, 96, 128)", ka.a.dim);
  }
  return MOJO_OK;
}

}  // namespace mojo

// N-step decode over the int8 cache: the swa_kv8 entry point's arguments plus `steps`; query and out are
// [batch][steps][q_heads][head_dim].
extern "C" int64_t mojo_hip_paged_decode_nstep_kv8_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                                   int64_t head_dim, int64_t block_size,
                                                                   int64_t max_blocks_per_seq, int64_t max_seq_len_hint,
                                                                   int64_t local_window, int64_t global_window, int64_t steps) {
  if (steps < 1) return -1;
  mojo::DecodeGeom g = {batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_seq_len_hint, local_window,
                        global_window, /*kv8=*/true};
  g.steps = steps;
  return mojo::decode_plan(g).query_bytes;
}

extern "C" int mojo_hip_paged_decode_nstep_kv8(const void* query, const void* key_cache, const void* key_scale,
                                               const void* value_cache, const void* value_scale,
                                               const int32_t* total_seq_lens, const int32_t* block_tables, void* out,
                                               void* workspace, int64_t workspace_bytes, int64_t batch, int64_t q_heads,
                                               int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                               int64_t max_blocks_per_seq, int64_t block_table_stride,
                                               int64_t cache_block_stride, int64_t cache_head_stride,
                                               int64_t cache_token_stride, int64_t max_seq_len_hint, float softmax_scale,
                                               int layout_abab, int leave_empty_rows, int dtype, int scale_dtype,
                                               int64_t local_window, int64_t global_window, int64_t steps,
                                               mojo_stream_t stream) {
  using namespace mojo;
  MOJO_REQUIRE(steps >= 1 && steps < (int64_t{1} << 16), MOJO_EINVAL, "paged_decode_nstep_kv8: steps %lld", (long long)steps);
  if (steps == 1)                                         // one step: the single-step op itself, same plan, bit for bit
    return mojo_hip_paged_decode_swa_kv8(query, key_cache, key_scale, value_cache, value_scale, total_seq_lens, block_tables, out,
                                         workspace, workspace_bytes, batch, q_heads, kv_heads, head_dim, block_size,
                                         max_blocks_per_seq, block_table_stride, cache_block_stride, cache_head_stride,
                                         cache_token_stride, max_seq_len_hint, softmax_scale, layout_abab, leave_empty_rows, dtype,
                                         scale_dtype, local_window, global_window, stream);
  DecodeCall c;
  c.query = query; c.key_cache = key_cache; c.value_cache = value_cache; c.total_seq_lens = total_seq_lens; c.block_tables = block_tables;
  c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.g = {batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_seq_len_hint, local_window, global_window, /*kv8=*/true};
  c.g.steps = steps;
  c.block_table_stride = block_table_stride; c.cache_block_stride = cache_block_stride; c.cache_head_stride = cache_head_stride;
  c.cache_token_stride = cache_token_stride; c.softmax_scale = softmax_scale; c.layout_abab = layout_abab;
  c.leave_empty_rows = leave_empty_rows; c.dtype = dtype;
  c.key_scale = key_scale; c.value_scale = value_scale; c.scale_dtype = scale_dtype;
  if (batch == 0) return MOJO_OK;
  if (const int rc = decode_kv8_check_call(c, "paged_decode_nstep_kv8"); rc != MOJO_OK) return rc;
  const DecodePlan p = decode_plan(c.g);
  MOJO_REQUIRE(p.query_bytes >= 0, MOJO_EUNSUPPORTED,
               "paged_decode_nstep_kv8: not a geometry of the n-step kernel (head_dim 64 / 80 / 96 / 128, pages of a multiple of 16, "
               "groups <= 16, MOJO_HIP_DECODE_MFMA != 0): compose single-step calls");
  MOJO_REQUIRE(batch * kv_heads * p.row_blocks <= 65535, MOJO_EUNSUPPORTED,
               "paged_decode_nstep_kv8: batch*kv_heads*step blocks %lld exceeds the grid limit", (long long)(batch * kv_heads * p.row_blocks));
  Kv8Args ka{};
  if (const int rc = decode_kv8_fill_args(ka, c, p); rc != MOJO_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(c.stream);
  return MOJO_SWITCH("MOJO_HIP_STREAM_NT", -1) != 0 ? launch_decode_kv8_nstep<true>(ka, p, batch, s)
                                                    : launch_decode_kv8_nstep<false>(ka, p, batch, s);
}
