// The body of decode_mfma_kernel and decode_mfma_nstep_kernel (paged_decode_mfma.h), included inside each of them — NOT a
// header of its own.  In scope: the template parameters T, DK, NT, MODE, SWA, the constant NSTEP, and the arguments a and G.
  int steps = 1;                                        // (NSTEP only: G arrives as decode_nstep_arg)
  bool scan_holes = false;
  if constexpr (NSTEP) { steps = (G >> 8) & 0xffff; scan_holes = (G >> 24) != 0; G &= 0xff; }
  constexpr bool FUSED = MODE != DEC_SPLIT;
  constexpr bool PAIRED = MODE == DEC_PAIRED;
  static_assert(!(SWA && PAIRED), "the paired form takes no window");
  static_assert(!NSTEP || SWA, "the n-step instances walk a DecodeWin");
  constexpr int D = DK * 32, ND = D / 16;               // head_dim, 16-wide d tiles of O^T
  constexpr int ROWB = D * 2;                           // bytes of a token row
  constexpr int NP = D / 16;                            // 32-byte pairs per row
  constexpr int RPB = 8 / NP;                           // rows per 256-byte bank row (1 at D = 128, 2 at D = 64)
  constexpr int NS = DK == 2 ? 2 : 1;                   // sub-tiles per loop step: a step moves 8 KiB of K/V whatever the head_dim (at
                                                        // head_dim 64 one sub-tile per step left the loop's fixed part — maximum, reference,
                                                        // rescale test, branches — on half the bytes: 0.68 of HBM against 0.80 at 128)
  constexpr int STEP = DECM_TILE * NS;
  typedef typename pack8<T>::vec V8;
  typedef dec_mma<T> MM;
  const int lane = threadIdx.x & 63;
  const int tl = lane & 15, g4 = lane >> 4;             // K / V loads: token tl of the tile, dim chunk g4 of each k-step
  const int wave_id = FUSED ? __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)) : 0;
  // (grouped form, DecodeArgs::fuse_group: workgroup x of a row owns chunks [x * waves, (x + 1) * waves) of it)
  const int chunk0 = FUSED ? static_cast<int>(blockIdx.x) * static_cast<int>(blockDim.x >> 6) + wave_id : static_cast<int>(blockIdx.x);
  const int b0 = blockIdx.y / a.hkv;                    // (paired form: the pair index; n-step: see DecodeSteps)
  int kvh = blockIdx.y % a.hkv;

  DecodeWin win;                                        // (SWA only)
  DecodeSteps st;                                       // (NSTEP only)
  DecodePair pr;                                        // (PAIRED only)
  DecodeRow row;
  if constexpr (NSTEP) {
    const int vlen = decode_nstep_row(a, blockIdx.y, G, steps, win, st);
    kvh = st.kvh;
    row = decode_row(a, st.b, chunk0, a.max_pages > 0 ? vlen : 0);
  } else if constexpr (PAIRED) { pr = decode_pair(a, lane, b0); row = decode_row(pr, wave_id); }
  else row = decode_row(a, b0, chunk0, decode_row_len<SWA>(a, b0, win));
  const int b = row.b, tok_begin = row.tok_begin, tok_end = row.tok_end;
  const bool has_work = row.has_work;
  if (!FUSED && !has_work) return;

  // query slices: B operand, lane = (head tl, dims 32 s + 8 g4 .. + 7)
  const int hq_l = min(tl, G - 1);                      // lanes past the group repeat its last head (computed, never stored)
  // NSTEP: lane = (column tl = (step, head)); lanes past the block's columns repeat its last one.  The lane's step sees the
  // keys t <= vis_hi with t < st.gl or t >= vis_lo.
  const int NC = NSTEP ? (16 / G) * G : G;              // columns of a partial
  int col_l = 0, vis_hi = 0, vis_lo = 0;
  if constexpr (NSTEP) {
    col_l = min(tl, st.nst * G - 1);
    vis_hi = win.len - st.nst + col_l / G;
    vis_lo = a.local_win >= 0 ? max(vis_hi - a.local_win, 0) : 0x7fffffff;
  }
  // B operands: line L (128 bytes = 8 chunks) of the row, parity p: lane k-group g4 holds the dims of chunk 8 L + 2 g4 + p
  constexpr int NL = D / 64;                            // 128-byte lines per token row
  typename MM::frag8 qf[NL][2];                         // (loaded below, with the page ids)

  f32x4 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  const int32_t* table = a.tables + static_cast<int64_t>(b) * a.table_stride;
  DecodeHoles holes(a, tok_end);

  // K: instruction (token group j, line L) = tokens 8 j + (l & 7), chunk 8 L + (l >> 3);  V: whole rows, RPI rows per instruction
  constexpr int CPR = D / 8;                            // 16-byte chunks per row
  constexpr int RPI = 64 / CPR;                         // V rows per load instruction (4 at D = 128, 8 at D = 64)
  constexpr int NV = 16 / RPI;                          // V load instructions per tile
  const int kt8 = lane & 7, kc8 = lane >> 3;
  const int vr = lane / CPR, vc = lane % CPR;
  const T* kbase = static_cast<const T*>(a.kc) + (kvh >> a.hshift) * a.c_head + kc8 * 8;
  const T* vbase = static_cast<const T*>(a.vc) + (kvh >> a.hshift) * a.c_head + vc * 8;
  const int last_tile = ((tok_end - 1) / DECM_TILE) * DECM_TILE;      // first token of the last non-empty tile
  const int last_page = a.max_pages - 1;

  // Page ids: one register per window of the chunk.  Lane i of the window at sub-tile `base` holds the table entry of
  // sub-tile base + i (with the clamps of the tile itself: last tile, window jump, last table column), so the id of a
  // tile is a lane read at a wave-uniform index: no load sits between a tile landing and the next request.  A round of
  // the steady loop (three tiles, 3 NS sub-tiles) requests up to 2 NS sub-tiles past its own, and windows change between
  // rounds only, so consecutive windows start IDW = 60 sub-tiles apart (a whole number of rounds) and overlap in their
  // last four lanes.  `idw` is the window in use, `idn` the next one: requested when the ring
  // enters `idw`, at least one round (24 tile loads) before its first use.  Lanes past the chunk's last tile repeat
  // that tile's entry: nothing past the chunk's pages is fetched, let alone used.
  constexpr int IDW = 60;
  static_assert(IDW % (3 * NS) == 0 && IDW + 2 * NS <= 64, "windows change between rounds; a round's requests stay inside one");
  auto id_window = [&](int s_base) -> int {
    int tu = min(tok_begin + DECM_TILE * (s_base + lane), last_tile);
    if constexpr (SWA) tu = decode_swa_real(win, tu);
    return table[min(tu >> a.page_shift, last_page)];
  };
  {                                                     // waited for in front of the first S^T product only
    const int h = decode_head(a, kvh, hq_l, G);
    const T* qp = static_cast<const T*>(a.q) + (NSTEP ? decode_col_at(a, st, col_l) : (static_cast<int64_t>(b) * a.hq + h) * a.dim);
#pragma unroll
    for (int L = 0; L < NL; ++L)
#pragma unroll
      for (int p = 0; p < 2; ++p) qf[L][p] = *reinterpret_cast<const typename MM::frag8*>(qp + (8 * L + 2 * g4 + p) * 8);
  }
  int idw = 0, idn = 0, id_base = 0;                    // (id_base: first sub-tile of idw)
  // Prologue: the query slices, the two id windows and the hole scan are requested together — the first two tiles go out
  // back to back as soon as window 0 has landed, with window 1 and the scan still on their way.
  if (has_work) {
    idw = id_window(0);
    idn = id_window(IDW);
    if constexpr (!SWA) holes.issue(table, lane, 0);   // (SWA: no hole scan — pages outside the window may hold anything)
    if constexpr (NSTEP) { if (scan_holes) holes.issue(table, lane, 0); }   // (no window set: virtual = real tokens)
  }
  struct Tile { V8 k[NS][2][NL]; V8 v[NS][NV]; int lp[NS]; };
  auto ld = [&](const T* p) -> V8 {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const V8*>(p));
    else return *reinterpret_cast<const V8*>(p);
  };
  auto load_tile = [&](Tile& t, int t0) {
    const int s0 = __builtin_amdgcn_readfirstlane((t0 - tok_begin) / DECM_TILE) - id_base;   // lane of the window in use
#pragma unroll
    for (int ss = 0; ss < NS; ++ss) {
      int tu = min(t0 + DECM_TILE * ss, last_tile);         // wave-uniform; 16 | page: the sub-tile lies in one page
      if constexpr (SWA) tu = decode_swa_real(win, tu);
      const int lp = tu >> a.page_shift;
      t.lp[ss] = lp;
      const int phys = max(__builtin_amdgcn_readlane(idw, s0 + ss), 0);
      const int64_t pg = static_cast<int64_t>(phys) * a.c_blk + static_cast<int64_t>(tu - (lp << a.page_shift)) * a.c_tok;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int L = 0; L < NL; ++L) t.k[ss][j][L] = ld(kbase + pg + static_cast<int64_t>(8 * j + kt8) * a.c_tok + L * 64);
#pragma unroll
      for (int u = 0; u < NV; ++u) t.v[ss][u] = ld(vbase + pg + static_cast<int64_t>(RPI * u + vr) * a.c_tok);
    }
  };

  // wave-private V images, one per sub-tile: [16 tokens][ROWB bytes], 32-byte pair pp of row t at pp ^ ((t / RPB) & (NP - 1))
  extern __shared__ float s_part[];                      // [waves][NC][D + 2] partials, then [waves][16 x ROWB] V images
  const int n_waves = FUSED ? static_cast<int>(blockDim.x >> 6) : 1;
  char* const v_img = reinterpret_cast<char*>(s_part + (FUSED ? n_waves * NC * (D + 2) : 0)) + wave_id * (NS * 16 * ROWB);
  const unsigned v_u32 = static_cast<unsigned>(reinterpret_cast<size_t>(v_img));
  unsigned w_off[NV];                                    // write of load instruction u: chunk vc of row RPI u + vr
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int row = RPI * u + vr;
    const int fw = (row / RPB) & (NP - 1);
    w_off[u] = row * ROWB + (((vc >> 1) ^ fw) << 5) + (vc & 1) * 16;
  }
  // transposed read of d tile dt: lane (group g4, i = tl): row = token 4 g4 + (i >> 2), columns 16 dt + 4 (i & 3) .. + 3
  const int rrow = 4 * g4 + (tl >> 2);
  const int fr = (rrow / RPB) & (NP - 1);
  const unsigned r_base = v_u32 + rrow * ROWB + (tl & 3) * 8;      // + ((dt ^ fr) << 5)

  auto process = [&](Tile& t, int t0) {
#pragma unroll
    for (int ss = 0; ss < NS; ++ss)
      if (t.lp[ss] >= holes.first_neg) {                      // rare: pages behind a hole read as zeros
        V8 z = {};
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int L = 0; L < NL; ++L) t.k[ss][j][L] = z;
#pragma unroll
        for (int u = 0; u < NV; ++u) t.v[ss][u] = z;
      }
    const bool full = t0 + STEP <= tok_end;              // wave-uniform
    int rt[NS];                                          // SWA: real first token of each sub-tile, and whether it holds a window edge
    bool edge[NS], any_edge = false;
#pragma unroll
    for (int ss = 0; ss < NS; ++ss) {
      rt[ss] = t0 + DECM_TILE * ss;
      edge[ss] = false;
      if constexpr (SWA) {
        rt[ss] = decode_swa_real(win, rt[ss]);
        edge[ss] = NSTEP ? decode_nstep_edge(win, st, rt[ss]) : decode_swa_edge(win, rt[ss]);
        any_edge = any_edge || edge[ss];
      }
    }
    float x[NS][4];
#pragma unroll
    for (int ss = 0; ss < NS; ++ss) {
      // c[j][p]: token group j (8 tokens), parity p; valid rows: (token, p)
      f32x4 c[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          c[j][p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int L = 0; L < NL; ++L) c[j][p] = MM::qk(__builtin_bit_cast(typename MM::frag8, t.k[ss][j][L]), qf[L][p], c[j][p]);
        }
      // stage V while the scores come out of the matrix pipe (rows past the length may hold NaN / Inf: zeros)
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        // (SWA edge tiles: their invisible rows are keys of this sequence in a page it still uses — finite, and their scores are
        // masked below; only rows past the length may hold anything)
        const bool vrow_ok = full || (t0 + DECM_TILE * ss + RPI * u + vr) < tok_end;
        V8 z = {};
        *reinterpret_cast<V8*>(v_img + ss * (16 * ROWB) + w_off[u]) = vrow_ok ? t.v[ss][u] : z;
      }
      // S[token] = C0[row token] + C1[row token + 8]; rows 0-7 live in lanes 0-31, rows 8-15 in lanes 32-63 (row = 4 (l >> 4) + i).
      // Tokens 0-7 (group 0) end up in lanes 0-31, tokens 8-15 (group 1) in lanes 32-63: token 4 (l >> 4) + i, as in the 16-row form.
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // X = C1 of group 0 (its upper half is needed below), Y = C0 of group 1;  X' = [X.lo, Y.lo], Y' = [X.hi, Y.hi].
        // The builtin, not inline asm: the operands come straight out of the matrix pipe, and only the compiler's hazard
        // recogniser knows how many wait states an MFMA result needs before a lane swap may read it.
        // (floats first: __builtin_bit_cast applied to a vector-element lvalue reads element 0 whatever the index)
        const float xa = c[0][1][i], ya = c[1][0][i];
        const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, xa), __builtin_bit_cast(unsigned, ya), false, false);
        const float own = lane < 32 ? c[0][0][i] : c[1][1][i];
        const float oth = __builtin_bit_cast(float, lane < 32 ? sw[1] : sw[0]);
        x[ss][i] = (own + oth) * a.scale_log2;
      }
    }
    if (!full || any_edge) {
#pragma unroll
      for (int ss = 0; ss < NS; ++ss)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          bool ok = t0 + DECM_TILE * ss + 4 * g4 + i < tok_end;
          if constexpr (NSTEP) {
            const int t = rt[ss] + 4 * g4 + i;
            ok = ok && (!edge[ss] || (t <= vis_hi && (t < st.gl || t >= vis_lo)));
          } else if constexpr (SWA) ok = ok && (!edge[ss] || decode_swa_vis(win, rt[ss] + 4 * g4 + i));
          if (!ok) x[ss][i] = -INFINITY;
        }
    }
    typename MM::frag4 pf[NS];
    decode_softmax_step<MM>(x, m, l, o, pf);
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
      for (int ss = 0; ss < NS; ++ss) {
        const s16x4 vt = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            reinterpret_cast<__attribute__((address_space(3))) s16x4*>(static_cast<uintptr_t>(r_base + ss * (16 * ROWB) + ((dt ^ fr) << 5))));
        o[dt] = MM::pv(MM::from_lds(vt), pf[ss], o[dt]);
      }
  };

  Tile ta, tb, tc;
  if (has_work) {
    auto scan_rest = [&]() {
      if constexpr (!SWA) holes.finish(table, lane);
      if constexpr (NSTEP) { if (scan_holes) holes.finish(table, lane); }
    };
    int t0 = tok_begin;
    load_tile(ta, tok_begin);
    if (tok_begin + 4 * STEP < tok_end) {
      load_tile(tb, tok_begin + STEP);                   // (unconditional on the way into the loop: its waits count on both tiles)
      scan_rest();
      // steady state: every request is unconditional, so the waits of process() are counted — tile t waits for its own
      // eight loads and leaves those of tiles t + 1 and t + 2 outstanding (no wait of the loop goes below vmcnt(12)).  One round = three tiles; the id window
      // changes between rounds, after at least one round in the window before it.
      for (;;) {
        const int t_win = tok_begin + DECM_TILE * (id_base + IDW);    // first round of the next window
        do {
          load_tile(tc, t0 + 2 * STEP);
          process(ta, t0);
          load_tile(ta, t0 + 3 * STEP);
          process(tb, t0 + STEP);
          load_tile(tb, t0 + 4 * STEP);
          process(tc, t0 + 2 * STEP);
          t0 += 3 * STEP;
        } while (t0 + 4 * STEP < tok_end && t0 < t_win);
        if (t0 < t_win) break;
        // (also in front of the tail: its requests lie in the new window.  The copy is an instruction of its own so that it
        // stands in FRONT of the request, which then lands in the register the copy freed: as a plain assignment it is
        // placed behind the request, and the copy out of a third register waits for vmcnt(0) with two tiles in flight)
        asm volatile("v_mov_b32 %0, %1" : "=v"(idw) : "v"(idn));
        id_base += IDW;
        idn = id_window(id_base + IDW);
        if (t0 + 4 * STEP >= tok_end) break;
      }
    } else {
      if (tok_begin + STEP < tok_end) load_tile(tb, tok_begin + STEP);
      scan_rest();
    }
    // the last one to four tiles (ta and tb, where they exist, are on their way)
    if (t0 + 2 * STEP < tok_end) load_tile(tc, t0 + 2 * STEP);
    process(ta, t0);
    if (t0 + STEP < tok_end) {
      if (t0 + 3 * STEP < tok_end) load_tile(ta, t0 + 3 * STEP);
      process(tb, t0 + STEP);
      if (t0 + 2 * STEP < tok_end) {
        process(tc, t0 + 2 * STEP);
        if (t0 + 3 * STEP < tok_end) process(ta, t0 + 3 * STEP);
      }
    }
  }

  // the row sums of the four token groups of a head meet (the reference maximum is already common to them)
  l = xor_sum_16_32(l);
  // lane holds head tl, dims 16 dt + 4 g4 + i
  if constexpr (FUSED) {
    if (tl < NC) {
      float* dst = s_part + (wave_id * NC + tl) * (D + 2);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) *reinterpret_cast<f32x4*>(dst + dt * 16 + 4 * g4) = o[dt];
      if (g4 == 0) { dst[D] = m; dst[D + 1] = l; }
    }
    if constexpr (NSTEP) decode_lds_merge_nstep(a, s_part, D, NC, row, st, Store16<T>{a.out});
    else decode_lds_merge<PAIRED, !PAIRED>(a, s_part, D, G, kvh, row, pr, Store16<T>{a.out});
    return;
  }
  if constexpr (NSTEP) decode_split_finish_nstep(a, NC, row, st, tl, g4, o, m, l, Store16<T>{a.out});
  else decode_split_finish(a, G, kvh, row, tl, g4, o, m, l, Store16<T>{a.out});
