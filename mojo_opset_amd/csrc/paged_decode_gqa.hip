// MojoPagedDecodeGQA — split-KV flash decoding for gfx950.
//
// Work decomposition
//   grid = (chunks, B * Hkv); one 64-lane wave per (sequence, kv-head, chunk of the KV range).
//   The G = Hq/Hkv query heads that share a kv-head are processed together, so every K/V byte is
//   read from HBM exactly once (the reference's Triton kernel launches (B, Hq) and re-reads the
//   cache G times: backends/ttx/kernels/ilu/flash_attention.py:818).
//
// Data layout in the wave
//   A (page, head) slab of the cache is [page tokens][D] contiguous.  LPT = 16 lanes cover one token
//   row with 16 B (8 elements) each, so one wave-wide load instruction moves 64/LPT = 4 consecutive
//   tokens = up to 1 KiB fully coalesced.  A tile is 4 such loads of K and 4 of V (16 tokens);
//   two tiles are kept in flight (register double buffer) — K/V go straight to VGPRs, there is no
//   reuse to stage through LDS.
//   lane = r * LPT + j :  r = token slot inside a load (0..3), j = 8-element slice of the head dim.
//   Each lane row r runs its own online softmax over tokens {4i + r}; the 4 partial states are merged
//   once at the end.  Scores: v_dot2c_f32_bf16 partial dots + a 4-step DPP butterfly inside the row.
//
// Numerics: fp32 scores/softmax/accumulators; the golden rounds scores and probabilities to the
// storage dtype, so parity is by tolerance (atol = rtol = 2e-2 in the reference test).
//
// Algorithmic bytes per launch: sum_b len_b * Hkv * D * 2(K,V) * elt  +  2 * B * Hq * D * elt
//                               + 4 * B * (max_blocks + 1).
//
// This file: DecodeArgs, the window (DecodeWin), the chunking rules and decode_head; paged_decode_common.h — what the three
// decode kernels share on the device (paired prologue, row and chunk of a wave, hole scan, in-LDS merge, split epilogue, softmax
// step of the matrix-core kernels); decode_split_kernel (vector units); paged_decode_mfma.h (16-bit matrix-core kernel); the
// merge kernel; the planner; one launch selection for both 16-bit routes (launch_decode_nt); the entry points, which fill a
// DecodeCall; paged_decode_kv8.h (int8-cache kernel and its entry points); paged_decode_kv8_nstep.h (its n-step form).
#include <math.h>
#include <stdlib.h>

#include "common.h"

namespace mojo {

constexpr int DEC_LPT = 16;               // lanes per token row
constexpr int DEC_TPL = 64 / DEC_LPT;     // tokens per wave-wide load
constexpr int DEC_LOADS = 4;              // loads per tile
constexpr int DEC_TILE = DEC_TPL * DEC_LOADS;   // 16 tokens

template <typename T> struct pack8;
template <> struct pack8<bf16_t> {
  typedef bf16x8 vec;
  typedef bf16x2 pair;
  static __device__ __forceinline__ float dot2(pair a, pair b, float c) {
    return __builtin_amdgcn_fdot2_f32_bf16(a, b, c, false);
  }
};
template <> struct pack8<f16_t> {
  typedef f16x8 vec;
  typedef f16x2 pair;
  static __device__ __forceinline__ float dot2(pair a, pair b, float c) { return __builtin_amdgcn_fdot2(a, b, c, false); }
};

struct DecodeArgs {
  const void* q;
  const void* kc;
  const void* vc;
  const int32_t* seq_lens;
  const int32_t* tables;
  void* out;
  float* ws_acc;     // [B*Hkv][chunks][G][D] fp32, un-normalised
  float* ws_ml;      // [B*Hkv][chunks][G][2]  (running max in log2 units, running sum)
  int hq, hkv, dim, page, page_shift, max_pages, batch;   // hkv: kv heads the GRID sees (= real kv heads << hshift)
  int hshift;                     // 1: groups of 8 query heads run as two 4-head halves of one kv head (see launch), else 0
  int64_t table_stride, c_blk, c_head, c_tok;
  int chunk_tokens, n_chunks;     // launch-wide bound: no sequence is cut into more than n_chunks pieces of <= chunk_tokens
  float scale_log2;
  int abab;
  int leave_empty;                // rows with seq_len <= 0: 1 = leave the output row untouched (graph replay contract), 0 = zeros
  int fuse_group = 0;             // > 0: GROUPED form — workgroups of this many waves each own that many consecutive chunks of a row,
                                  // merge them in LDS and leave ONE partial per workgroup (slot = workgroup index along x) for the
                                  // merge launch; a row whose chunks fit one workgroup is finished there
  // sliding window (the SWA instances only; see DecodeWin): real-length capacity, local window (< 0: none), global window (<= 0: none)
  int swa_cap = 0, local_win = -1, global_win = 0;
};

// Sliding window (MojoPagedDecodeSWA).  Row of `len` keys, query at position len - 1: key t is visible iff t < g1 or
// lo <= t < len, with lo = max(0, len - 1 - local) (len without a local window) and g1 = min(global, lo).  The kernels walk
// a VIRTUAL key range of vlen tokens: [0, g_al) is the global range rounded up to the 16-token tile, then the local range from
// its tile start lo_al = lo & ~15 on — virtual token v is real token v + gap past g_al (gap = lo_al - g_al, 0 when the two
// ranges overlap and collapse into one).  Both cuts are tile-aligned, so a tile never straddles them; the tiles holding g1
// or lo are masked per key ("edge" tiles).  Chunking, pairing of chunks and merging all run on vlen, which is at most
// ceil16(global) + local + 16 whatever the context: the host sizes the launch on that, not on the table's capacity.
struct DecodeWin { int len = 0, g1 = 0, lo = 0, g_al = 0, gap = 0; };
__device__ __forceinline__ int decode_swa_row(const DecodeArgs& a, int b, DecodeWin& w) {
  const int len = max(min(a.seq_lens[b], a.swa_cap), 0);
  w.len = len;
  w.lo = a.local_win >= 0 ? max(len - 1 - a.local_win, 0) : len;
  w.g1 = min(max(a.global_win, 0), w.lo);
  w.g_al = (w.g1 + DEC_TILE - 1) & ~(DEC_TILE - 1);
  w.gap = 0;
  int vlen = len;
  if (w.lo >= len) {
    vlen = w.g1;                                         // no local range: the global range alone
  } else {
    const int lo_al = w.lo & ~(DEC_TILE - 1);
    if (lo_al > w.g_al) { w.gap = lo_al - w.g_al; vlen = len - w.gap; }
  }
  // (row-uniform: pinned to scalar registers — held in vector registers they spilled the fused matrix-core instance)
  w.len = __builtin_amdgcn_readfirstlane(w.len);
  w.g1 = __builtin_amdgcn_readfirstlane(w.g1);
  w.lo = __builtin_amdgcn_readfirstlane(w.lo);
  w.g_al = __builtin_amdgcn_readfirstlane(w.g_al);
  w.gap = __builtin_amdgcn_readfirstlane(w.gap);
  return __builtin_amdgcn_readfirstlane(min(vlen, a.n_chunks * a.chunk_tokens));
}
__device__ __forceinline__ int decode_swa_real(const DecodeWin& w, int v) { return v >= w.g_al ? v + w.gap : v; }
__device__ __forceinline__ bool decode_swa_edge(const DecodeWin& w, int rt0) { return rt0 < w.lo && rt0 + DEC_TILE > w.g1; }
__device__ __forceinline__ bool decode_swa_vis(const DecodeWin& w, int t) { return t < w.g1 || (t >= w.lo && t < w.len); }

// Chunking is PER SEQUENCE: a sequence of `len` tokens is cut into n_chunks equal pieces (whole tiles, at least 128 tokens,
// never more than the launch-wide chunk_tokens), so the waves of a short row of a ragged batch all work (and finish early)
// instead of some of them idling while the others walk max_len / n_chunks tokens.  Lengths beyond what the launch was sized
// for (the caller's max_total_seq_len hint, or page * max_blocks) are truncated to that capacity: the grid, the LDS image and
// the workspace hold n_chunks slots per row and nothing may index past them.
__device__ __forceinline__ int decode_seq_len(const DecodeArgs& a, int b) {
  return min(a.seq_lens[b], a.n_chunks * a.chunk_tokens);
}
__device__ __forceinline__ int decode_seq_chunk(const DecodeArgs& a, int seq_len) {
  int c = (seq_len + a.n_chunks - 1) / a.n_chunks;
  c = max(c, 128);
  c = ((c + DEC_TILE - 1) / DEC_TILE) * DEC_TILE;
  return min(c, a.chunk_tokens);
}

// MODE 1 (fused): one workgroup = all chunks of one (sequence, kv-head), one wave per chunk (n_chunks <= 8); the partial
// states meet in LDS and the workgroup writes the final output itself — no partials in HBM, no merge launch.
// MODE 2 (fused, paired): an 8-wave workgroup owns TWO sequences of one kv-head — the one of rank p and the one of rank
// B-1-p when the batch is ordered by length — and deals its waves between them in proportion to their lengths.  Every wave
// of the launch is resident at once, so a launch lasts as long as its busiest wave: with four waves per sequence that is
// max_len / 4 tokens; a long row paired with a short one leaves every wave ~(len_long + len_short) / 8, the batch mean / 4.
// A uniform batch gets 4 + 4 waves per pair, i.e. exactly the MODE 1 work per wave.
constexpr int DEC_SPLIT = 0, DEC_FUSED = 1, DEC_PAIRED = 2;
// The `int G` argument of decode_mfma_nstep_kernel: heads per kv head, query rows per sequence (< 2^16), and whether the hole scan
// runs (no window set) — see DecodeSteps for why these are not fields of DecodeArgs.
constexpr int decode_nstep_arg(int G, int steps, int scan_holes) { return G | (steps << 8) | (scan_holes << 24); }

// query head of (grid kv head kvh, head g of the kernel's G).  With hshift = 1 the grid's kv heads are the halves of the real
// ones: real kv head kvh >> 1, heads (kvh & 1) * G + g of its 2 G.
__device__ __forceinline__ int decode_head(const DecodeArgs& a, int kvh, int g, int G) {
  if (!a.abab) return kvh * G + g;                        // AABB: (real kv head, half, g) is already kvh * G + g
  const int real = kvh >> a.hshift, half = kvh & ((1 << a.hshift) - 1);
  return (half * G + g) * (a.hkv >> a.hshift) + real;
}

// N-step decode (MojoPagedDecodeNstepSWA): S query rows per sequence, step j at position len - S + j; key t is
// visible to it iff t <= len - S + j and (no window, or t < global, or t >= len - S + j - local).  The 16 columns of the
// matrix-core kernel's score product hold (step, head) pairs: a grid row owns a BLOCK of SB = 16 / G consecutive steps of one
// (sequence, kv head), column c = (step c / G of the block, head c % G), C = SB * G columns in all.  With S > SB the blocks of
// a (sequence, kv head) are grid rows of their own — row y = ((b * hkv) + kvh) * blocks + block — and each streams K/V itself.
// A block of `nst` steps whose last step sees `len_e` keys is an nst-step problem on len_e keys, so the window of a block is a
// DecodeWin with `lo` the lower edge of its FIRST step and the local range running to len_e: both staircases (the last
// nst - 1 keys, and the local window's lower edges lo_k = max(len_e - nst + k - local, 0)) lie inside the walked range and are
// masked per lane, a lane owning one column.  No window runs as a local window of the launch capacity (lo = 0, no gap).
// S is an argument of the n-step kernels, not a field of DecodeArgs: a longer DecodeArgs moves the kernel arguments of every
// decode kernel, and the compiler then groups their loads differently — the single-step instances would not compile to what
// they compile to today.
struct DecodeSteps {
  int S = 1;                        // query rows per sequence
  int b = 0, kvh = 0;               // sequence and grid kv head of the row
  int j0 = 0, nst = 1;              // first step of the block, steps in it
  int len = 0;                      // the sequence's length (len <= 0: an empty row, left or zeroed as a whole)
  int lo_last = 0, gl = 0;          // lower edge of the block's last step; the global window as given (>= 0)
  int G = 1;                        // query heads per kv head
};
__device__ __forceinline__ int decode_nstep_blocks(int steps, int G) { const int sb = 16 / G; return (steps + sb - 1) / sb; }
__device__ __forceinline__ int decode_nstep_row(const DecodeArgs& a, int y, int G, int steps, DecodeWin& w, DecodeSteps& st) {
  st.G = G;
  st.S = steps;
  const int sb = 16 / G, nb = decode_nstep_blocks(steps, G);
  const int bh = y / nb, blk = y - bh * nb;
  st.b = bh / a.hkv;
  st.kvh = bh - st.b * a.hkv;
  st.j0 = blk * sb;
  st.nst = min(sb, steps - st.j0);
  st.len = __builtin_amdgcn_readfirstlane(max(min(a.seq_lens[st.b], a.swa_cap), 0));
  const int len_e = max(st.len - (steps - st.j0 - st.nst), 0);     // keys the block's last step sees
  w.lo = a.local_win >= 0 ? max(len_e - st.nst - a.local_win, 0) : len_e;
  st.lo_last = __builtin_amdgcn_readfirstlane(a.local_win >= 0 ? max(len_e - 1 - a.local_win, 0) : len_e);
  st.gl = max(a.global_win, 0);
  // the virtual range: as decode_swa_row, on len_e keys from the first step's lower edge
  w.len = len_e;
  w.g1 = min(st.gl, w.lo);
  w.g_al = (w.g1 + DEC_TILE - 1) & ~(DEC_TILE - 1);
  w.gap = 0;
  int vlen = len_e;
  if (w.lo >= len_e) {
    vlen = w.g1;                                         // no local range: the global range alone
  } else {
    const int lo_al = w.lo & ~(DEC_TILE - 1);
    if (lo_al > w.g_al) { w.gap = lo_al - w.g_al; vlen = len_e - w.gap; }
  }
  w.len = __builtin_amdgcn_readfirstlane(w.len);
  w.g1 = __builtin_amdgcn_readfirstlane(w.g1);
  w.lo = __builtin_amdgcn_readfirstlane(w.lo);
  w.g_al = __builtin_amdgcn_readfirstlane(w.g_al);
  w.gap = __builtin_amdgcn_readfirstlane(w.gap);
  return __builtin_amdgcn_readfirstlane(min(vlen, a.n_chunks * a.chunk_tokens));
}
// column c of a block: valid (it holds a step of the block), its step within the block, its head
__device__ __forceinline__ bool decode_col_ok(const DecodeSteps& st, int c) { return c < st.nst * st.G; }
// element offset of column c's row in the [B][S][Hq][D] query / output (c valid)
__device__ __forceinline__ int64_t decode_col_at(const DecodeArgs& a, const DecodeSteps& st, int c) {
  const int k = c / st.G, g = c - k * st.G;
  return ((static_cast<int64_t>(st.b) * st.S + st.j0 + k) * a.hq + decode_head(a, st.kvh, g, st.G)) * a.dim;
}
// a tile at real token rt0 every key of which every step of the block sees (else it is masked per lane)
__device__ __forceinline__ bool decode_nstep_edge(const DecodeWin& w, const DecodeSteps& st, int rt0) {
  const bool all_vis = rt0 + DEC_TILE <= w.len - st.nst + 1 && (rt0 + DEC_TILE <= st.gl || rt0 >= st.lo_last);
  return !all_vis;
}

}  // namespace mojo
#include "paged_decode_common.h"
namespace mojo {

template <typename T, int G, bool NT, int MODE, bool SWA = false>
__global__ __launch_bounds__(MODE != DEC_SPLIT ? 512 : 64) void decode_split_kernel(DecodeArgs a) {
  constexpr bool FUSED = MODE != DEC_SPLIT;
  constexpr bool PAIRED = MODE == DEC_PAIRED;
  static_assert(!(SWA && PAIRED), "the paired form takes no window");
  typedef typename pack8<T>::vec V8;
  typedef typename pack8<T>::pair V2;
  const int lane = threadIdx.x & 63;
  const int r = lane / DEC_LPT;
  const int j = lane % DEC_LPT;
  // (readfirstlane: the wave index must be a scalar, or every page-table lookup below turns into a vector load)
  const int wave_id = FUSED ? __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)) : 0;
  const int chunk0 = FUSED ? wave_id : static_cast<int>(blockIdx.x);
  const int b0 = blockIdx.y / a.hkv;                     // (paired form: the pair index)
  const int kvh = blockIdx.y % a.hkv;

  DecodeWin win;                                         // (SWA only)
  DecodePair pr;                                         // (PAIRED only)
  DecodeRow row;
  if constexpr (PAIRED) { pr = decode_pair(a, lane, b0); row = decode_row(pr, wave_id); }
  else row = decode_row(a, b0, chunk0, decode_row_len<SWA>(a, b0, win));
  const int b = row.b, chunk = row.chunk, tok_begin = row.tok_begin, tok_end = row.tok_end;
  const bool has_work = row.has_work;
  if (!FUSED && !has_work) return;
  const bool dim_ok = j * 8 < a.dim;
  const int jd = dim_ok ? j * 8 : a.dim - 8;          // lanes past a short head re-read its last slice

  // query slices for the G heads of this kv-head (AABB: h = kvh*G + g, ABAB: h = g*Hkv + kvh).  The 8-head instance of the
  // workgroup forms parks them in LDS (its own 16 lanes x 16 B per head, read back four heads at a time): with them in
  // registers it needs ~10 more than a wave has at two waves per SIMD.
  constexpr bool Q_LDS = FUSED && G >= 8;
  V8 qv[Q_LDS ? 1 : G];
  extern __shared__ float s_part[];                      // [waves][G][dim + 2] partials (+ [waves][G][16 lanes] query slices)
  V8* const q_lds = reinterpret_cast<V8*>(s_part + (blockDim.x >> 6) * G * (a.dim + 2)) + (wave_id * G) * DEC_LPT + j;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int h = decode_head(a, kvh, g, G);
    V8 z = {};
    const V8 x = *reinterpret_cast<const V8*>(static_cast<const T*>(a.q) + (static_cast<int64_t>(b) * a.hq + h) * a.dim + jd);
    if constexpr (Q_LDS) { if (r == 0) q_lds[g * DEC_LPT] = dim_ok ? x : z; }
    else qv[g] = dim_ok ? x : z;
  }

  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
  }

  const int32_t* table = a.tables + static_cast<int64_t>(b) * a.table_stride;
  DecodeHoles holes(a, tok_end);
  if (!SWA && has_work) holes.issue(table, lane, 0);    // (SWA: no hole scan — pages outside the window may hold anything)

  const T* kbase = static_cast<const T*>(a.kc) + (kvh >> a.hshift) * a.c_head + jd;
  const T* vbase = static_cast<const T*>(a.vc) + (kvh >> a.hshift) * a.c_head + jd;
  const int last_load = ((tok_end - 1) / DEC_TPL) * DEC_TPL;   // first token of the last non-empty load
  const int last_page = a.max_pages - 1;

  struct Tile { V8 k[DEC_LOADS]; V8 v[DEC_LOADS]; int lp[DEC_LOADS]; };

  auto ld = [&](const T* p) -> V8 {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const V8*>(p));
    else return *reinterpret_cast<const V8*>(p);
  };

  // Branch-free: every load is issued (clamped to an address that certainly exists); its logical page is kept so that
  // `process` can tell which loads must read as zero (pages at or behind the first negative id).
  auto load_tile = [&](Tile& t, int t0) {
#pragma unroll
    for (int u = 0; u < DEC_LOADS; ++u) {
      int tu = min(t0 + u * DEC_TPL, last_load);          // wave-uniform; TPL | page
      if constexpr (SWA) {
        tu = decode_swa_real(win, tu);
        if (tu >= win.g1 && tu + DEC_TPL <= win.lo) tu = win.lo & ~(DEC_TPL - 1);   // a load no key of which is visible: read
      }                                                                               // the page of `lo` instead (masked below)
      const int lp = a.page_shift >= 0 ? (tu >> a.page_shift) : tu / a.page;
      t.lp[u] = lp;
      const int phys = max(table[min(lp, last_page)], 0);
      const int64_t off = static_cast<int64_t>(phys) * a.c_blk + static_cast<int64_t>(tu - lp * a.page + r) * a.c_tok;
      t.k[u] = ld(kbase + off);
      t.v[u] = ld(vbase + off);
    }
  };

  auto process = [&](Tile& t, int t0) {
    if (t.lp[DEC_LOADS - 1] >= holes.first_neg) {              // rare: pages behind a hole read as zeros (lp grows with u)
#pragma unroll
      for (int u = 0; u < DEC_LOADS; ++u)
        if (t.lp[u] >= holes.first_neg) { V8 z = {}; t.k[u] = z; t.v[u] = z; }
    }
    const bool full = t0 + DEC_TILE <= tok_end;          // wave-uniform
    bool edge = false;                                   // SWA: the tile holds a window edge (wave-uniform)
    int rt0 = t0;
    if constexpr (SWA) { rt0 = decode_swa_real(win, t0); edge = decode_swa_edge(win, rt0); }
    if (!full || edge) {                                 // last tile of the chunk: slots past the length may hold NaN/Inf
#pragma unroll
      for (int u = 0; u < DEC_LOADS; ++u) {
        V8 z = {};
        bool ok = (t0 + u * DEC_TPL + r) < tok_end;
        if constexpr (SWA) ok = ok && (!edge || decode_swa_vis(win, rt0 + u * DEC_TPL + r));
        if (!ok) t.v[u] = z;
      }
    }
    // Heads in blocks of GB = 4: eight heads at once need 32 score registers on top of 64 accumulators, 32 query registers
    // and the tile ring — more than a wave has at two waves per SIMD (the 8-head instance spilled: B 64, ctx 4096, 64 / 8
    // heads 876 us).  Scores and probabilities of one block are dead before the next block's are formed.
    constexpr int GB = G < 4 ? G : 4;
#pragma unroll
    for (int g0 = 0; g0 < G; g0 += GB) {
      float s[DEC_LOADS][GB];
      V8 qb[GB];
#pragma unroll
      for (int gg = 0; gg < GB; ++gg) {
        if constexpr (Q_LDS) qb[gg] = q_lds[(g0 + gg) * DEC_LPT];   // (written by this wave's own lanes 0-15: no barrier)
        else qb[gg] = qv[g0 + gg];
      }
#pragma unroll
      for (int u = 0; u < DEC_LOADS; ++u) {
#pragma unroll
        for (int gg = 0; gg < GB; ++gg) {
          float d = 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            V2 qa = {qb[gg][2 * e], qb[gg][2 * e + 1]};
            V2 ka = {t.k[u][2 * e], t.k[u][2 * e + 1]};
            d = pack8<T>::dot2(qa, ka, d);
          }
          s[u][gg] = row16_sum(d) * a.scale_log2;
        }
      }
      if (!full || edge) {                               // mask the tail (and the window edges)
#pragma unroll
        for (int u = 0; u < DEC_LOADS; ++u) {
          bool valid = (t0 + u * DEC_TPL + r) < tok_end;
          if constexpr (SWA) valid = valid && (!edge || decode_swa_vis(win, rt0 + u * DEC_TPL + r));
#pragma unroll
          for (int gg = 0; gg < GB; ++gg) s[u][gg] = valid ? s[u][gg] : -INFINITY;
        }
      }
#pragma unroll
      for (int gg = 0; gg < GB; ++gg) {
        const int g = g0 + gg;
        float mx = m[g];
#pragma unroll
        for (int u = 0; u < DEC_LOADS; ++u) mx = fmaxf(mx, s[u][gg]);
        const float ms = mx == -INFINITY ? 0.f : mx;     // row r may not have seen a valid token yet
        const float alpha = exp2f(m[g] - ms);
        m[g] = mx;
        float p[DEC_LOADS];
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < DEC_LOADS; ++u) {
          p[u] = exp2f(s[u][gg] - ms);
          ps += p[u];
        }
        l[g] = l[g] * alpha + ps;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float x = acc[g][e] * alpha;
#pragma unroll
          for (int u = 0; u < DEC_LOADS; ++u) x = fmaf(p[u], static_cast<float>(t.v[u][e]), x);
          acc[g][e] = x;
        }
      }
      if constexpr (GB < G) asm volatile("" ::: "memory");   // keep the blocks apart (the scheduler would interleave them again)
    }
  };

  // register ring of tiles: three (prefetch distance two tiles, 16 KiB in flight per wave) — two for the 8-head instance, whose
  // accumulators take the third tile's registers
  constexpr int RING = G >= 8 ? 2 : 3;
  Tile ta, tb, tc;
  if (has_work) {
  load_tile(ta, tok_begin);
  if (tok_begin + DEC_TILE < tok_end) load_tile(tb, tok_begin + DEC_TILE);
  if constexpr (!SWA) holes.finish(table, lane);
  if constexpr (RING == 3) {
    for (int t0 = tok_begin; t0 < tok_end; t0 += 3 * DEC_TILE) {
      if (t0 + 2 * DEC_TILE < tok_end) load_tile(tc, t0 + 2 * DEC_TILE);
      process(ta, t0);
      if (t0 + DEC_TILE >= tok_end) break;
      if (t0 + 3 * DEC_TILE < tok_end) load_tile(ta, t0 + 3 * DEC_TILE);
      process(tb, t0 + DEC_TILE);
      if (t0 + 2 * DEC_TILE >= tok_end) break;
      if (t0 + 4 * DEC_TILE < tok_end) load_tile(tb, t0 + 4 * DEC_TILE);
      process(tc, t0 + 2 * DEC_TILE);
    }
  } else {
    for (int t0 = tok_begin; t0 < tok_end; t0 += 2 * DEC_TILE) {
      process(ta, t0);
      if (t0 + DEC_TILE >= tok_end) break;
      if (t0 + 2 * DEC_TILE < tok_end) load_tile(ta, t0 + 2 * DEC_TILE);
      process(tb, t0 + DEC_TILE);
      if (t0 + 3 * DEC_TILE < tok_end) load_tile(tb, t0 + 3 * DEC_TILE);
    }
  }
  }

  // merge the DEC_TPL lane rows (lanes j, j+16, j+32, j+48 hold the same head-dim slice)
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float mx = m[g];
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float ms = mx == -INFINITY ? 0.f : mx;
    const float w = exp2f(m[g] - ms);
    float lw = l[g] * w;
    lw += __shfl_xor(lw, 16);
    lw += __shfl_xor(lw, 32);
    l[g] = lw;
    m[g] = mx;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float x = acc[g][e] * w;
      x += __shfl_xor(x, 16);
      x += __shfl_xor(x, 32);
      acc[g][e] = x;
    }
  }

  if constexpr (FUSED) {
    if (r == 0 && dim_ok) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float* dst = s_part + (wave_id * G + g) * (a.dim + 2);     // (wave_id == chunk in the unpaired form)
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[j * 8 + e] = acc[g][e];
        if (j == 0) { dst[a.dim] = m[g]; dst[a.dim + 1] = l[g]; }
      }
    }
    decode_lds_merge<PAIRED, false>(a, s_part, a.dim, G, kvh, row, pr, Store16<T>{a.out});
    return;
  }
  if (r != 0 || !dim_ok) return;
  if (row.n_chunks_seq() == 1) {
    // single chunk: finish here, the merge kernel skips this row
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int h = decode_head(a, kvh, g, G);
      const float inv = 1.0f / l[g];
      V8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = static_cast<T>(acc[g][e] * inv);
      *reinterpret_cast<V8*>(static_cast<T*>(a.out) + (static_cast<int64_t>(b) * a.hq + h) * a.dim + j * 8) = o;
    }
    return;
  }
  const int64_t slot = (static_cast<int64_t>(blockIdx.y) * a.n_chunks + chunk) * G;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float* dst = a.ws_acc + (slot + g) * a.dim + j * 8;
    *reinterpret_cast<f32x4*>(dst) = f32x4{acc[g][0], acc[g][1], acc[g][2], acc[g][3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{acc[g][4], acc[g][5], acc[g][6], acc[g][7]};
    if (j == 0) {
      a.ws_ml[(slot + g) * 2 + 0] = m[g];
      a.ws_ml[(slot + g) * 2 + 1] = l[g];
    }
  }
}

}  // namespace mojo
#include "paged_decode_mfma.h"
namespace mojo {

// Merge the chunk partials: grid = (B*Hkv, G), a workgroup of 8 chunk lanes x 32 threads (4 output elements each); rows with
// seq_len <= 0 become zeros (golden semantics), single-chunk rows were finished by the split kernel.  Chunk lane j takes
// the chunks j, j + 8, ...; the eight partial sums meet in LDS and are added in lane order (fixed, so the bits do not depend
// on timing).  (One thread used to walk all chunks of a row through dependent loads: a single long sequence — B = 1,
// 16K tokens, 128 chunks — spent ~38 of its 54 us here.)
template <typename T, bool SWA = false>
__global__ __launch_bounds__(256) void decode_merge_kernel(DecodeArgs a, int G) {
  __shared__ float s_mx[8], s_den[8];
  __shared__ f32x4 s_num[8][32];
  const int b = blockIdx.x / a.hkv;
  const int kvh = blockIdx.x % a.hkv;
  const int g = blockIdx.y;
  int seq_len;
  if constexpr (SWA) { DecodeWin w; seq_len = decode_swa_row(a, b, w); }
  else seq_len = decode_seq_len(a, b);
  const int chunk_tokens = decode_seq_chunk(a, seq_len);
  int n_chunks_seq = seq_len <= 0 ? 0 : (seq_len + chunk_tokens - 1) / chunk_tokens;   // <= a.n_chunks by construction
  if (a.fuse_group > 0) n_chunks_seq = (n_chunks_seq + a.fuse_group - 1) / a.fuse_group;   // grouped form: one partial per workgroup
  if (n_chunks_seq == 1) return;                         // (workgroup-uniform)
  const int h = decode_head(a, kvh, g, G);
  const int cl = threadIdx.x >> 5, dt = threadIdx.x & 31;
  const int d0 = dt * 4;
  const bool live = d0 < a.dim;
  T* dst = static_cast<T*>(a.out) + (static_cast<int64_t>(b) * a.hq + h) * a.dim + d0;
  typedef typename vec_of<T, 4>::type V4;
  if (n_chunks_seq == 0) {
    if (a.leave_empty || cl != 0 || !live) return;
    V4 z = {};
    *reinterpret_cast<V4*>(dst) = z;
    return;
  }
  const int64_t base = static_cast<int64_t>(blockIdx.x) * a.n_chunks * G + g;
  float mx = -INFINITY;
  for (int c = cl; c < n_chunks_seq; c += 8) mx = fmaxf(mx, a.ws_ml[(base + static_cast<int64_t>(c) * G) * 2]);
  if (dt == 0) s_mx[cl] = mx;
  __syncthreads();
  mx = s_mx[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) mx = fmaxf(mx, s_mx[j]);
  f32x4 num = {0.f, 0.f, 0.f, 0.f};
  float den = 0.f;
#pragma unroll 4
  for (int c = cl; c < n_chunks_seq; c += 8) {
    const int64_t slot = base + static_cast<int64_t>(c) * G;
    const float w = exp2f(a.ws_ml[slot * 2] - mx);
    den = fmaf(w, a.ws_ml[slot * 2 + 1], den);
    if (live) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(a.ws_acc + slot * a.dim + d0);
      num += x * w;
    }
  }
  s_num[cl][dt] = num;
  if (dt == 0) s_den[cl] = den;
  __syncthreads();
  if (cl != 0 || !live) return;
#pragma unroll
  for (int j = 1; j < 8; ++j) { num += s_num[j][dt]; den += s_den[j]; }
  const float inv = 1.0f / den;
  V4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = static_cast<T>(num[e] * inv);
  *reinterpret_cast<V4*>(dst) = o;
}

// The merge of the n-step launches: grid = (B*Hkv*blocks, C) — a row is a block of steps (DecodeSteps), blockIdx.y a column of
// it, G the heads per kv head; otherwise decode_merge_kernel.  A step that saw no key (0 < len < steps) stores zeros.
template <typename T>
__global__ __launch_bounds__(256) void decode_merge_nstep_kernel(DecodeArgs a, int G, int steps) {
  __shared__ float s_mx[8], s_den[8];
  __shared__ f32x4 s_num[8][32];
  const int c = blockIdx.y, cols = static_cast<int>(gridDim.y);
  DecodeWin w;
  DecodeSteps st;
  const int seq_len = decode_nstep_row(a, blockIdx.x, G, steps, w, st);
  if (!decode_col_ok(st, c)) return;                     // (workgroup-uniform, like every return in front of the barriers)
  const int chunk_tokens = decode_seq_chunk(a, seq_len);
  int n_chunks_seq = seq_len <= 0 ? 0 : (seq_len + chunk_tokens - 1) / chunk_tokens;
  if (a.fuse_group > 0) n_chunks_seq = (n_chunks_seq + a.fuse_group - 1) / a.fuse_group;
  if (n_chunks_seq == 1) return;
  const int cl = threadIdx.x >> 5, dt = threadIdx.x & 31;
  const int d0 = dt * 4;
  const bool live = d0 < a.dim;
  T* dst = static_cast<T*>(a.out) + decode_col_at(a, st, c) + d0;
  typedef typename vec_of<T, 4>::type V4;
  if (n_chunks_seq == 0) {
    if ((a.leave_empty && st.len <= 0) || cl != 0 || !live) return;
    V4 z = {};
    *reinterpret_cast<V4*>(dst) = z;
    return;
  }
  const int64_t base = static_cast<int64_t>(blockIdx.x) * a.n_chunks * cols + c;
  float mx = -INFINITY;
  for (int k = cl; k < n_chunks_seq; k += 8) mx = fmaxf(mx, a.ws_ml[(base + static_cast<int64_t>(k) * cols) * 2]);
  if (dt == 0) s_mx[cl] = mx;
  __syncthreads();
  mx = s_mx[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) mx = fmaxf(mx, s_mx[j]);
  if (mx == -INFINITY) mx = 0.f;                         // no key in any chunk: weights exp2(-inf) = 0, not NaN
  f32x4 num = {0.f, 0.f, 0.f, 0.f};
  float den = 0.f;
#pragma unroll 4
  for (int k = cl; k < n_chunks_seq; k += 8) {
    const int64_t slot = base + static_cast<int64_t>(k) * cols;
    const float wt = exp2f(a.ws_ml[slot * 2] - mx);
    den = fmaf(wt, a.ws_ml[slot * 2 + 1], den);
    if (live) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(a.ws_acc + slot * a.dim + d0);
      num += x * wt;
    }
  }
  s_num[cl][dt] = num;
  if (dt == 0) s_den[cl] = den;
  __syncthreads();
  if (cl != 0 || !live) return;
#pragma unroll
  for (int j = 1; j < 8; ++j) { num += s_num[j][dt]; den += s_den[j]; }
  const float inv = den > 0.f ? 1.0f / den : 0.f;
  V4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = static_cast<T>(num[e] * inv);
  *reinterpret_cast<V4*>(dst) = o;
}

static int decode_chunk_tokens(int64_t batch, int64_t kv_heads, int64_t max_len, bool grouped = false) {
  {                                                            // tuning override
    const int v = static_cast<int>(MOJO_SWITCH("MOJO_HIP_DECODE_CHUNK", 0));
    if (v >= DEC_TILE) return (v / DEC_TILE) * DEC_TILE;
  }
  // The split kernel holds 2 waves per SIMD (register-ring bound), i.e. 2048 resident waves on 256
  // CUs.  Cut each sequence into as few chunks as still fill those slots once: long-lived waves
  // amortise their ramp-up and leave few partials to merge.  Never below 128 tokens per chunk.
  const int64_t units = batch * kv_heads > 0 ? batch * kv_heads : 1;
  int64_t splits = (256 * 8) / units;
  if (splits < 1) splits = 1;
  const int64_t len = max_len > 0 ? max_len : 1;
  int64_t chunk = ceil_div(len, splits);
  if (chunk < 128) chunk = 128;
  chunk = ceil_div(chunk, DEC_TILE) * DEC_TILE;
  // More than 8 chunks per (sequence, kv-head) take the split + merge form: single-wave workgroups and a merge launch whose
  // cost grows with the chunk count.  There 1 024 waves measured best, not 2 048 (round 3, scripts/probes/decode_tp8_chunk_ab.py,
  // matrix-core kernel: 8 q / 1 kv heads B 64 ctx 4096 39.8 -> 34.3 us, B 16 ctx 16384 52.1 -> 38.9 us, 64 / 8 heads B 8 ctx 8192
  // 64.2 -> 57.4 us, 32 / 8 heads B 8 ctx 4096 36.8 -> 32.6 us; 512 waves: 1.5-2 x slower) - but never fewer than 8 chunks.
  if (ceil_div(len, chunk) > 8) {
    // (grouped form: the partials are merged in LDS eight at a time, so the 2 048 waves that fill the chip cost no more partials
    // than 256 single-wave workgroups per row would)
    int64_t s2 = (grouped ? 2048 : 1024) / units;
    if (s2 < 8) s2 = 8;
    chunk = ceil_div(len, s2);
    if (chunk < 128) chunk = 128;
    chunk = ceil_div(chunk, DEC_TILE) * DEC_TILE;
  }
  return static_cast<int>(chunk);
}

static int64_t decode_max_len(int64_t page, int64_t max_pages, int64_t hint) {
  const int64_t cap = page * max_pages;
  return (hint > 0 && hint < cap) ? hint : cap;
}

// Sliding window: the most virtual tokens (DecodeWin) a row of a launch of real capacity `max_len` can walk — the global
// range rounded up to a tile plus the local window's local + 1 keys and the tile they start in.  With `steps` query rows
// (DecodeSteps) the local range of a block runs from its first step's lower edge to its last step's key: steps - 1 more.
static int64_t decode_swa_cap(int64_t max_len, int64_t local_window, int64_t global_window, int64_t steps = 1) {
  int64_t span = global_window > 0 ? ceil_div(global_window, DEC_TILE) * DEC_TILE : 0;
  if (local_window >= 0) span += local_window + DEC_TILE + (steps - 1);
  return span < max_len ? span : max_len;
}

// The matrix-core kernel (paged_decode_mfma.h): power-of-two pages of >= 16 tokens, head_dim 64 / 128, groups of <= 16 heads.
// MOJO_HIP_DECODE_MFMA: unset = where it measured faster (B 64, ctx 4096, page 16, graph replay, vector-unit -> matrix-core):
// groups of 8 heads (Llama-3-70B 64 / 8: 356 -> 170 us; 8 / 1: 79 -> 39 us), head_dim 64 (149 -> 99 us), groups of 4 at
// head_dim 128 (headline 179 -> 169 us, ctx 1024 51 -> 47 us, ragged 150 -> 139 us; B 8: 34.5 -> 32.6 us with the chunk rule
// of decode_chunk_tokens), and the group sizes the vector-unit kernel has no instance for.  Groups of 1 and 2 heads at head_dim 128
// stay on the vector-unit kernel (163 vs 168 us, 167 vs 169 us).  1 = wherever it applies, 0 = never.
static bool decode_use_mfma(int64_t G, int64_t head_dim, int64_t page) {
  const bool pow2 = page > 0 && (page & (page - 1)) == 0;
  if (!pow2 || page < 16 || (head_dim != 64 && head_dim != 128) || G > 16) return false;
  const long long e = MOJO_SWITCH("MOJO_HIP_DECODE_MFMA", -1);
  if (e == 0) return false;
  if (e == 1) return true;
  return G >= 4 || head_dim == 64 || (G != 1 && G != 2);
}

// What a decode launch is sized on: the shapes alone (no pointers), so the workspace queries and the launchers plan alike.
// A window makes the op the SWA one; none (local < 0 and global <= 0) leaves the GQA op, whichever entry point was called.
struct DecodeGeom {
  int64_t batch = 0, q_heads = 0, kv_heads = 0, head_dim = 0, page = 0, max_pages = 0, len_hint = 0;
  int64_t local_window = -1, global_window = 0;
  bool kv8 = false;                 // the int8-cache op (paged_decode_kv8.h): its own kernel, never grouped, paired or halved
  int64_t steps = 1;                // query rows per sequence (> 1: the n-step op, DecodeSteps; matrix-core kernels only)
};

struct DecodePlan {
  bool swa = false;                 // the windowed instances run
  bool mfma = false;                // the 16-bit matrix-core kernel runs (decode_use_mfma)
  int64_t capacity = 0;             // tokens of a row the launch can address: the hint, or page * table width
  int64_t max_len = 0;              // tokens of a row the launch walks: the capacity, or what a window leaves visible of it
  int chunk_tokens = 0, n_chunks = 0, fuse_group = 0;   // (DecodeArgs)
  int hshift = 0, grid_kv_heads = 0, G = 0;             // kv heads the grid sees (= kv_heads << hshift) and query heads per grid kv head
  int64_t slots = 0;                // partials the launch may write: batch * grid_kv_heads * n_chunks * G
  int64_t bytes = 0;                // workspace the launch needs
  int64_t query_bytes = 0;          // what the workspace query answers (0: degenerate geometry; -1: no n-step kernel for it)
  bool nstep = false;               // the n-step instances run (steps > 1): grid rows are blocks of steps, partials hold `cols` columns
  int row_blocks = 1, cols = 0;     // blocks of steps per (sequence, kv head); columns of a partial (single step: G)
  int steps = 1, scan_holes = 0;    // the n-step kernels' own arguments (decode_nstep_arg)
};

// The n-step op runs on the matrix-core kernels alone (their 16 columns are what holds the steps): the geometries the 16-bit
// kernel takes, or with the int8 cache those of decode_kv8_kernel (paged_decode_kv8_nstep.h), and MOJO_HIP_DECODE_MFMA as for
// the single-step op — 0 = never (callers then compose single-step launches), 1 = wherever it applies, unset = where it
// measured faster than `steps` single-step launches.
static bool decode_nstep_fused(const DecodeGeom& g) {
  if (g.kv_heads <= 0 || g.q_heads % g.kv_heads != 0) return false;
  const int64_t G = g.q_heads / g.kv_heads;
  if (g.kv8) {
    const bool dim_ok = g.head_dim == 64 || g.head_dim == 80 || g.head_dim == 96 || g.head_dim == 128;
    if (!dim_ok || g.page <= 0 || g.page % 16 != 0 || G > 16) return false;
  } else {
    const bool pow2 = g.page > 0 && (g.page & (g.page - 1)) == 0;
    if (!pow2 || g.page < 16 || (g.head_dim != 64 && g.head_dim != 128) || G > 16) return false;
  }
  return MOJO_SWITCH("MOJO_HIP_DECODE_MFMA", -1) != 0;
}


static DecodePlan decode_plan(const DecodeGeom& g) {
  DecodePlan p;
  const bool window = g.local_window >= 0 || g.global_window > 0;
  p.nstep = g.steps > 1;
  p.swa = window || p.nstep;                              // (the n-step instances are windowed ones: no window = the capacity)
  if (g.batch <= 0 || g.kv_heads <= 0 || g.q_heads <= 0) return p;
  if (p.nstep && !decode_nstep_fused(g)) { p.query_bytes = -1; return p; }   // not a geometry of the n-step kernel
  p.capacity = decode_max_len(g.page, g.max_pages, g.len_hint);
  p.max_len = !p.swa ? p.capacity : decode_swa_cap(p.capacity, window ? g.local_window : p.capacity, g.global_window, g.steps);
  const int64_t heads = g.q_heads / g.kv_heads;
  p.cols = static_cast<int>(heads);
  if (p.nstep) {
    const int64_t sb = 16 / heads;                        // steps of a block (DecodeSteps)
    p.row_blocks = static_cast<int>(ceil_div(g.steps, sb));
    p.cols = static_cast<int>(sb * heads);
    p.steps = static_cast<int>(g.steps);
    p.scan_holes = window ? 0 : 1;                        // no window: negative page ids are holes, as in the GQA op
  }
  // One form of the launch: the heads of a kv head together (hshift 0) or as two halves on twice the grid heads (hshift 1).
  auto form = [&](int hshift, DecodePlan& f) {
    f.hshift = hshift;
    f.grid_kv_heads = static_cast<int>(g.kv_heads << hshift);
    f.G = static_cast<int>(heads >> hshift);
    f.mfma = !g.kv8 && (p.nstep || decode_use_mfma(f.G, g.head_dim, g.page));   // (int8 cache: its own kernel, never grouped)
    // The grouped form (DecodeArgs::fuse_group; matrix-core kernel only) — MOJO_HIP_DECODE_GROUPED=0 restores the split + merge form.
    // Measured (scripts/probes/decode_grouped_ab.py, profiles/r4_decode_grouped_ab.txt; split + merge form -> grouped form, graph
    // replay): 8 q / 1 kv heads B 64 ctx 4096 (Llama-3-70B under TP 8) 33.6 -> 28.1 us, B 16 ctx 16384 38.2 -> 29.8 us; 32 / 8 heads
    // B 8 ctx 4096 31.3 -> 27.5 us; 64 / 8 heads B 8 ctx 8192 56.1 -> 49.8 us; head_dim 64 B 8 ctx 8192 33.7 -> 28.6 us.
    // (the grouped launch exists in the fused form only: without MOJO_HIP_DECODE_FUSE the chunks are sized, written and merged
    // one by one — ADVICE r4: the merge kernel divided the chunk count by the group size although every chunk had its partial)
    const bool grouped = f.mfma && MOJO_SWITCH("MOJO_HIP_DECODE_GROUPED", 1) != 0 && MOJO_SWITCH("MOJO_HIP_DECODE_FUSE", 1) != 0;
    f.chunk_tokens = decode_chunk_tokens(g.batch * p.row_blocks, f.grid_kv_heads, p.max_len, grouped);
    f.n_chunks = static_cast<int>(ceil_div(p.max_len > 0 ? p.max_len : 1, f.chunk_tokens));
    f.fuse_group = grouped && f.n_chunks > 8 ? 8 : 0;    // (the merge divides by it: set only where the grouped launch is taken)
    f.slots = g.batch * g.kv_heads * p.row_blocks * f.n_chunks * p.cols;
  };
  // Groups of 8 query heads per kv head (Llama-3-70B: 64 / 8).  Round 2 ran them as two 4-head halves on twice as many grid
  // heads (twice the K/V bytes: 360 us at B 64, ctx 4096) because the 8-head instance spilled; the instance now walks its heads
  // in blocks of four over a two-tile ring with the query slices parked in LDS (232 registers, no spill) and reads K/V once.
  // MOJO_HIP_DECODE_G8_HALVES=1 selects the halves again (A/B; experiments build only).
  const bool can_halve = !p.swa && !g.kv8 && heads == 8;
  int hshift = 0;
#ifdef MOJO_HIP_BUILD_EXPERIMENTS
  if (can_halve && MOJO_SWITCH("MOJO_HIP_DECODE_G8_HALVES", 0) == 1) hshift = 1;
#endif
  form(hshift, p);
  const int64_t slot_bytes = (g.head_dim + 2) * static_cast<int64_t>(sizeof(float));
  p.bytes = p.slots * slot_bytes;
  int64_t most = p.slots;               // the query sizes for whichever of the two forms cuts the sequences finer
  if (can_halve) {
    DecodePlan other;
    form(1 - hshift, other);
    if (other.slots > most) most = other.slots;
  }
  p.query_bytes = most * slot_bytes + 256;
  return p;
}

// (`cols`: columns of a partial — G, or the n-step block's 16 / G * G)
template <typename T, bool NT, int MODE, bool SWA, bool NSTEP = false>
static void launch_decode_mfma(const DecodeArgs& a, dim3 grid, dim3 block, int G, int cols, hipStream_t s) {
  const size_t waves = block.x / 64;
  const size_t lds = (MODE != DEC_SPLIT ? waves * cols * (a.dim + 2) * sizeof(float) : 0) + waves * 4096;   // + one 4 KiB V image (set) per wave
  static std::atomic<uint64_t> attr_set{0};             // (per instantiation: dynamic LDS beyond 64 KiB needs the attribute)
  if constexpr (NSTEP) {
    if (first_call_on_device(attr_set)) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&decode_mfma_nstep_kernel<T, 4, NT, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&decode_mfma_nstep_kernel<T, 2, NT, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    if (a.dim == 128) hipLaunchKernelGGL((decode_mfma_nstep_kernel<T, 4, NT, MODE>), grid, block, lds, s, a, G);
    else hipLaunchKernelGGL((decode_mfma_nstep_kernel<T, 2, NT, MODE>), grid, block, lds, s, a, G);
    return;
  }
  if (first_call_on_device(attr_set)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&decode_mfma_kernel<T, 4, NT, MODE, SWA>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&decode_mfma_kernel<T, 2, NT, MODE, SWA>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  if (a.dim == 128) hipLaunchKernelGGL((decode_mfma_kernel<T, 4, NT, MODE, SWA>), grid, block, lds, s, a, G);
  else hipLaunchKernelGGL((decode_mfma_kernel<T, 2, NT, MODE, SWA>), grid, block, lds, s, a, G);
}

// The vector-unit kernel's instance for a run-time group size: f(std::integral_constant<int, G>) for G in 1, 2, 4, 8.
template <typename F>
static int dispatch_G(int G, F&& f) {
  switch (G) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "paged_decode_gqa: group size %d (supported: 1,2,4,8)", G);
  }
  return MOJO_OK;
}

// One launch of kernel mode MODE on either route (`what`: the launch's name in an error message).
template <typename T, bool NT, int MODE, bool SWA, bool NSTEP = false>
static int launch_decode_mode(const DecodeArgs& a, const DecodePlan& p, dim3 grid, dim3 block, const char* what, hipStream_t s) {
  if constexpr (NSTEP) {                                // (planned on the matrix-core kernel alone)
    launch_decode_mfma<T, NT, MODE, SWA, true>(a, grid, block, decode_nstep_arg(p.G, p.steps, p.scan_holes), p.cols, s);
  } else if (p.mfma) {
    launch_decode_mfma<T, NT, MODE, SWA>(a, grid, block, p.G, p.cols, s);
  } else {
    const size_t waves = block.x / 64;                  // [waves][G][dim + 2] partials, and the 8-head instance's query slices
    const size_t lds = MODE == DEC_SPLIT ? 0 : waves * p.G * (a.dim + 2) * sizeof(float) + (p.G >= 8 ? waves * p.G * DEC_LPT * 16 : 0);
    const int rc = dispatch_G(p.G, [&](auto g) {
      hipLaunchKernelGGL((decode_split_kernel<T, decltype(g)::value, NT, MODE, SWA>), grid, block, lds, s, a);
      return MOJO_OK;
    });
    if (rc != MOJO_OK) return rc;
  }
  MOJO_CHECK_LAUNCH(what);
  return MOJO_OK;
}

template <typename T, bool NT, bool SWA, bool NSTEP>
static int launch_decode_nt(const DecodeArgs& a, const DecodePlan& p, hipStream_t s) {
  const int64_t batch = a.batch;
  const bool fuse = MOJO_SWITCH("MOJO_HIP_DECODE_FUSE", 1) != 0;
  const bool pair = MOJO_SWITCH("MOJO_HIP_DECODE_PAIR", 1) != 0;
  // The form of the launch, decided once for both routes.  The workgroup forms of the vector-unit kernel store four outputs
  // per thread: head dims that are no multiple of 4 take its split form.
  const bool wg_forms = fuse && (p.mfma || a.dim % 4 == 0);
  enum { PAIRED, FUSED, GROUPED, SPLIT } form = SPLIT;
  // paired: four waves per sequence fill the chip once — pair the sequences by length rank, deal each pair's 8 waves by length
  if (!SWA && wg_forms && pair && a.n_chunks == 4 && batch >= 2 && batch <= 64) form = PAIRED;
  // fused: all chunks of a (sequence, kv-head) in one workgroup, merged in LDS
  else if (wg_forms && a.n_chunks <= 8) form = FUSED;
  // grouped (matrix-core kernel): small grids (few (sequence, kv-head) rows, many chunks each) — eight-wave workgroups merge
  // their chunks in LDS and leave one partial each, so the launch keeps two waves per SIMD busy and the merge reads
  // n_chunks / 8 partials per row
  else if (wg_forms && p.mfma && a.fuse_group > 0) form = GROUPED;
  const unsigned rows = static_cast<unsigned>(batch * a.hkv * p.row_blocks);
  static const char* const tags[] = {"paired", "fused", "grouped+merge", "split+merge"};
  static const char* const whats[2][4] = {
      {"paged_decode_gqa(paired)", "paged_decode_gqa(fused)", "paged_decode_gqa(grouped)", "paged_decode_gqa(split)"},
      {"paged_decode_gqa(mfma, paired)", "paged_decode_gqa(mfma, fused)", "paged_decode_gqa(mfma, grouped)", "paged_decode_gqa(mfma, split)"}};
  const char* const what = whats[p.mfma ? 1 : 0][form];
  int rc = MOJO_OK;
  switch (form) {
    case PAIRED:                                       // (never with a window: the windowed instances have no paired form)
      rc = launch_decode_mode<T, NT, DEC_PAIRED, false>(a, p, dim3(1, static_cast<unsigned>(((batch + 1) / 2) * a.hkv)), dim3(512), what, s);
      break;
    case FUSED:
      rc = launch_decode_mode<T, NT, DEC_FUSED, SWA, NSTEP>(a, p, dim3(1, rows), dim3(static_cast<unsigned>(64 * a.n_chunks)), what, s);
      break;
    case GROUPED:
      rc = launch_decode_mode<T, NT, DEC_FUSED, SWA, NSTEP>(a, p, dim3(static_cast<unsigned>((a.n_chunks + a.fuse_group - 1) / a.fuse_group), rows),
                                                     dim3(static_cast<unsigned>(64 * a.fuse_group)), what, s);
      break;
    case SPLIT:
      rc = launch_decode_mode<T, NT, DEC_SPLIT, SWA, NSTEP>(a, p, dim3(static_cast<unsigned>(a.n_chunks), rows), dim3(64), what, s);
      break;
  }
  if (rc != MOJO_OK) return rc;
  if (form == GROUPED || form == SPLIT) {
    if constexpr (NSTEP) hipLaunchKernelGGL((decode_merge_nstep_kernel<T>), dim3(rows, p.cols), dim3(256), 0, s, a, p.G, p.steps);
    else hipLaunchKernelGGL((decode_merge_kernel<T, SWA>), dim3(rows, p.G), dim3(256), 0, s, a, p.G);
    MOJO_CHECK_LAUNCH("paged_decode_gqa(merge)");
  }
  note_launch("%s:%s:%s%s", p.mfma ? "decode_mfma" : "decode_valu", tags[form], NT ? "nt" : "cached",
              NSTEP ? ":nstep" : SWA ? ":swa" : "");
  return MOJO_OK;
}

template <typename T, bool SWA, bool NSTEP = false>
static int launch_decode(const DecodeArgs& a, const DecodePlan& p, hipStream_t s) {
  // K/V are read exactly once: non-temporal loads keep them from displacing the block tables and
  // partials in L2/MALL (measured on MI355X, B=64 ctx=4096: 204 -> 190 us).  MOJO_HIP_STREAM_NT=0 disables (the switch of every
  // streaming kernel, common.h stream_nt()).
  const bool nt = MOJO_SWITCH("MOJO_HIP_STREAM_NT", -1) != 0;
  return nt ? launch_decode_nt<T, true, SWA, NSTEP>(a, p, s) : launch_decode_nt<T, false, SWA, NSTEP>(a, p, s);
}

}  // namespace mojo

using namespace mojo;

// The C arguments the decode entry points share, named: an entry point fills it, the bodies read it.
struct DecodeCall {
  const void *query = nullptr, *key_cache = nullptr, *value_cache = nullptr;
  const int32_t *total_seq_lens = nullptr, *block_tables = nullptr;
  void *out = nullptr, *workspace = nullptr;
  DecodeGeom g;
  int64_t workspace_bytes = 0, block_table_stride = 0, cache_block_stride = 0, cache_head_stride = 0, cache_token_stride = 0;
  float softmax_scale = 0.f;
  int layout_abab = 0, leave_empty_rows = 0, dtype = 0;
  mojo_stream_t stream = nullptr;
  const void *key_scale = nullptr, *value_scale = nullptr;   // the int8-cache ops (g.kv8): per-channel scales [Hkv][D] and their dtype
  int scale_dtype = 0;
};

// What every decode entry point checks first (`op`: the entry point's name in the messages).
static int decode_check_call(const DecodeCall& c, const char* op) {
  const DecodeGeom& g = c.g;
  MOJO_REQUIRE(c.query && c.key_cache && c.value_cache && c.total_seq_lens && c.block_tables && c.out &&
                   (!g.kv8 || (c.key_scale && c.value_scale)), MOJO_EINVAL, "%s: null pointer", op);
  MOJO_REQUIRE(g.batch > 0 && g.q_heads > 0 && g.kv_heads > 0 && g.q_heads % g.kv_heads == 0, MOJO_EINVAL,
               "%s: bad head counts Hq=%lld Hkv=%lld", op, (long long)g.q_heads, (long long)g.kv_heads);
  MOJO_REQUIRE(c.dtype == MOJO_BF16 || c.dtype == MOJO_F16, MOJO_EUNSUPPORTED, "%s: %sdtype %d (bf16/fp16 only)", op,
               g.kv8 ? "query " : "", c.dtype);
  // (the 16-bit op may run a kv head as two halves on twice the grid heads)
  MOJO_REQUIRE(g.max_pages >= 0 && g.batch * g.kv_heads * (g.kv8 ? 1 : 2) <= 65535, MOJO_EUNSUPPORTED,
               "%s: batch*kv_heads %lld exceeds the grid limit", op, (long long)(g.batch * g.kv_heads));
  return MOJO_OK;
}

// The window of a planned windowed call (p.swa), in the kernel's 32-bit terms.
static int decode_set_window(DecodeArgs& a, const DecodeCall& c, const DecodePlan& p, const char* op) {
  const DecodeGeom& g = c.g;
  MOJO_REQUIRE(p.capacity < (int64_t{1} << 30) && g.local_window < (int64_t{1} << 30) && g.global_window < (int64_t{1} << 30),
               MOJO_EUNSUPPORTED, "%s: lengths and windows must stay below 2^30", op);
  a.swa_cap = static_cast<int>(p.capacity);
  a.local_win = g.local_window >= 0 ? static_cast<int>(g.local_window) : -1;
  a.global_win = g.global_window > 0 ? static_cast<int>(g.global_window) : 0;
  if (p.nstep && p.scan_holes) a.local_win = static_cast<int>(p.capacity);   // no window: a local window of the capacity
  return MOJO_OK;
}

// The kernel arguments of a planned call, its workspace bound (`op`: the entry point's name in the messages).
static int decode_fill_args(DecodeArgs& a, const DecodeCall& c, const DecodePlan& p, const char* op) {
  const DecodeGeom& g = c.g;
  a.q = c.query; a.kc = c.key_cache; a.vc = c.value_cache; a.seq_lens = c.total_seq_lens; a.tables = c.block_tables; a.out = c.out;
  a.hq = static_cast<int>(g.q_heads); a.hkv = p.grid_kv_heads; a.hshift = p.hshift; a.dim = static_cast<int>(g.head_dim);
  a.page = static_cast<int>(g.page); a.max_pages = static_cast<int>(g.max_pages); a.batch = static_cast<int>(g.batch);
  a.page_shift = (g.page & (g.page - 1)) == 0 ? __builtin_ctzll(g.page) : -1;
  a.table_stride = c.block_table_stride; a.c_blk = c.cache_block_stride; a.c_head = c.cache_head_stride; a.c_tok = c.cache_token_stride;
  a.chunk_tokens = p.chunk_tokens; a.n_chunks = p.n_chunks; a.fuse_group = p.fuse_group;
  a.scale_log2 = c.softmax_scale * 1.4426950408889634f; a.abab = c.layout_abab ? 1 : 0; a.leave_empty = c.leave_empty_rows ? 1 : 0;
  MOJO_REQUIRE(c.workspace && c.workspace_bytes >= p.bytes, MOJO_EWORKSPACE, "%s: workspace %lld B < required %lld B", op,
               (long long)c.workspace_bytes, (long long)p.bytes);
  MOJO_REQUIRE(aligned_to(c.workspace, 16), MOJO_EINVAL, "%s: workspace must be 16-byte aligned", op);
  a.ws_acc = static_cast<float*>(c.workspace);
  a.ws_ml = a.ws_acc + p.slots * g.head_dim;
  return MOJO_OK;
}

// The GQA and SWA entry points share one body: with SWA the launch is planned on the visible capacity (decode_swa_cap), the
// windowed kernel instances run, and the paired and halved forms are not taken.
template <bool SWA, bool NSTEP = false>
static int paged_decode_planned(const DecodeCall& c, const DecodePlan& p) {
  const DecodeGeom& g = c.g;
  if (const int rc = decode_check_call(c, "paged_decode_gqa"); rc != MOJO_OK) return rc;
  MOJO_REQUIRE(g.head_dim % 8 == 0 && g.head_dim >= 8 && g.head_dim <= 8 * DEC_LPT, MOJO_EUNSUPPORTED,
               "paged_decode_gqa: head_dim %lld (multiple of 8, <= %d)", (long long)g.head_dim, 8 * DEC_LPT);
  MOJO_REQUIRE(g.page % DEC_TPL == 0, MOJO_EUNSUPPORTED, "paged_decode_gqa: block_size %lld must be a multiple of %d",
               (long long)g.page, DEC_TPL);
  MOJO_REQUIRE(c.cache_token_stride % 8 == 0 && c.cache_head_stride % 8 == 0 && c.cache_block_stride % 8 == 0 &&
                   aligned_to(c.key_cache, 16) && aligned_to(c.value_cache, 16) && aligned_to(c.query, 16) &&
                   aligned_to(c.out, 16),
               MOJO_EUNSUPPORTED, "paged_decode_gqa: tensors must be 16-byte aligned with 16-byte row strides");
  DecodeArgs a;
  if constexpr (SWA) {
    if (const int rc = decode_set_window(a, c, p, "paged_decode_swa"); rc != MOJO_OK) return rc;
  }
  if (const int rc = decode_fill_args(a, c, p, "paged_decode_gqa"); rc != MOJO_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(c.stream);
  return c.dtype == MOJO_BF16 ? launch_decode<bf16_t, SWA, NSTEP>(a, p, s) : launch_decode<f16_t, SWA, NSTEP>(a, p, s);
}

static int paged_decode(const DecodeCall& c) {
  if (c.g.batch == 0) return MOJO_OK;
  const DecodePlan p = decode_plan(c.g);                 // (p.swa: a call without a window is the GQA op itself)
  return !p.swa ? paged_decode_planned<false>(c, p) : paged_decode_planned<true>(c, p);
}

extern "C" int64_t mojo_hip_paged_decode_gqa_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                             int64_t head_dim, int64_t block_size,
                                                             int64_t max_blocks_per_seq, int64_t max_seq_len_hint) {
  return decode_plan({batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_seq_len_hint}).query_bytes;
}

extern "C" int64_t mojo_hip_paged_decode_swa_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                             int64_t head_dim, int64_t block_size,
                                                             int64_t max_blocks_per_seq, int64_t max_seq_len_hint,
                                                             int64_t local_window, int64_t global_window) {
  return decode_plan({batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_seq_len_hint, local_window,
                      global_window}).query_bytes;
}

extern "C" int mojo_hip_paged_decode_gqa(const void* query, const void* key_cache, const void* value_cache,
                                         const int32_t* total_seq_lens, const int32_t* block_tables, void* out,
                                         void* workspace, int64_t workspace_bytes, int64_t batch, int64_t q_heads,
                                         int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                         int64_t max_blocks_per_seq, int64_t block_table_stride,
                                         int64_t cache_block_stride, int64_t cache_head_stride,
                                         int64_t cache_token_stride, int64_t max_seq_len_hint, float softmax_scale,
                                         int layout_abab, int leave_empty_rows, int dtype, mojo_stream_t stream) {
  // (no window: the windowed entry point runs the GQA op itself)
  return mojo_hip_paged_decode_swa(query, key_cache, value_cache, total_seq_lens, block_tables, out, workspace, workspace_bytes, batch,
                                   q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, block_table_stride,
                                   cache_block_stride, cache_head_stride, cache_token_stride, max_seq_len_hint, softmax_scale,
                                   layout_abab, leave_empty_rows, dtype, /*local_window=*/-1, /*global_window=*/0, stream);
}

extern "C" int mojo_hip_paged_decode_swa(const void* query, const void* key_cache, const void* value_cache,
                                         const int32_t* total_seq_lens, const int32_t* block_tables, void* out,
                                         void* workspace, int64_t workspace_bytes, int64_t batch, int64_t q_heads,
                                         int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                         int64_t max_blocks_per_seq, int64_t block_table_stride,
                                         int64_t cache_block_stride, int64_t cache_head_stride,
                                         int64_t cache_token_stride, int64_t max_seq_len_hint, float softmax_scale,
                                         int layout_abab, int leave_empty_rows, int dtype, int64_t local_window,
                                         int64_t global_window, mojo_stream_t stream) {
  DecodeCall c;
  c.query = query; c.key_cache = key_cache; c.value_cache = value_cache; c.total_seq_lens = total_seq_lens; c.block_tables = block_tables;
  c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.g = {batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_seq_len_hint, local_window, global_window};
  c.block_table_stride = block_table_stride; c.cache_block_stride = cache_block_stride; c.cache_head_stride = cache_head_stride;
  c.cache_token_stride = cache_token_stride; c.softmax_scale = softmax_scale; c.layout_abab = layout_abab;
  c.leave_empty_rows = leave_empty_rows; c.dtype = dtype;
  return paged_decode(c);
}

// N-step decode: the SWA entry point's arguments plus `steps`; query and out are [batch][steps][q_heads][head_dim].
extern "C" int64_t mojo_hip_paged_decode_nstep_workspace_bytes(int64_t batch, int64_t q_heads, int64_t kv_heads,
                                                               int64_t head_dim, int64_t block_size,
                                                               int64_t max_blocks_per_seq, int64_t max_seq_len_hint,
                                                               int64_t local_window, int64_t global_window, int64_t steps) {
  if (steps < 1) return -1;
  DecodeGeom g = {batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_seq_len_hint, local_window, global_window};
  g.steps = steps;
  return decode_plan(g).query_bytes;
}

extern "C" int mojo_hip_paged_decode_nstep(const void* query, const void* key_cache, const void* value_cache,
                                           const int32_t* total_seq_lens, const int32_t* block_tables, void* out,
                                           void* workspace, int64_t workspace_bytes, int64_t batch, int64_t q_heads,
                                           int64_t kv_heads, int64_t head_dim, int64_t block_size,
                                           int64_t max_blocks_per_seq, int64_t block_table_stride,
                                           int64_t cache_block_stride, int64_t cache_head_stride,
                                           int64_t cache_token_stride, int64_t max_seq_len_hint, float softmax_scale,
                                           int layout_abab, int leave_empty_rows, int dtype, int64_t local_window,
                                           int64_t global_window, int64_t steps, mojo_stream_t stream) {
  MOJO_REQUIRE(steps >= 1 && steps < (int64_t{1} << 16), MOJO_EINVAL, "paged_decode_nstep: steps %lld", (long long)steps);
  if (steps == 1)                                         // one step: the single-step op itself, same plan, bit for bit
    return mojo_hip_paged_decode_swa(query, key_cache, value_cache, total_seq_lens, block_tables, out, workspace, workspace_bytes,
                                     batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, block_table_stride,
                                     cache_block_stride, cache_head_stride, cache_token_stride, max_seq_len_hint, softmax_scale,
                                     layout_abab, leave_empty_rows, dtype, local_window, global_window, stream);
  DecodeCall c;
  c.query = query; c.key_cache = key_cache; c.value_cache = value_cache; c.total_seq_lens = total_seq_lens; c.block_tables = block_tables;
  c.out = out; c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  c.g = {batch, q_heads, kv_heads, head_dim, block_size, max_blocks_per_seq, max_seq_len_hint, local_window, global_window};
  c.g.steps = steps;
  c.block_table_stride = block_table_stride; c.cache_block_stride = cache_block_stride; c.cache_head_stride = cache_head_stride;
  c.cache_token_stride = cache_token_stride; c.softmax_scale = softmax_scale; c.layout_abab = layout_abab;
  c.leave_empty_rows = leave_empty_rows; c.dtype = dtype;
  if (batch == 0) return MOJO_OK;
  if (const int rc = decode_check_call(c, "paged_decode_nstep"); rc != MOJO_OK) return rc;
  const DecodePlan p = decode_plan(c.g);
  MOJO_REQUIRE(p.query_bytes >= 0, MOJO_EUNSUPPORTED,
               "paged_decode_nstep: not a geometry of the n-step kernel (head_dim 64 / 128, power-of-two pages >= 16, groups <= 16, "
               "MOJO_HIP_DECODE_MFMA != 0): compose single-step calls");
  MOJO_REQUIRE(batch * kv_heads * p.row_blocks <= 65535, MOJO_EUNSUPPORTED, "paged_decode_nstep: batch*kv_heads*step blocks %lld exceeds the grid limit",
               (long long)(batch * kv_heads * p.row_blocks));
  return paged_decode_planned<true, true>(c, p);
}

#include "paged_decode_kv8.h"
#include "paged_decode_kv8_nstep.h"
