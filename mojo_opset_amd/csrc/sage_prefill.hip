// MojoPagedPrefillSageGQA (SAGE_ATTN_OPS): causal paged prefill with an int8 query (per-token scales), an int8 K
// cache (per-token scales) and an int8 V cache (per-channel scales).  Both contractions run on v_mfma_i32_16x16x64_i8 with
// int32 accumulators; the probabilities are quantised to [0, 127] against the FINAL row maximum, so the integers that enter
// P.V and the row sum are the golden's and no accumulator is ever rescaled.
//
// Work split.  One workgroup of four waves owns one sequence, one kv head and 64 score rows; a score row is a (query token,
// head of the GQA group) pair, row r = token r / G, head r % G, so the G heads of a group share every staged K tile and every
// transposed V tile.  Wave w owns rows [16w, 16w + 16).  Heavy (late) row tiles take the low block indices.
//
// Two passes over the key tiles of 64 keys, both ended by the causal bound of the tile's last token:
//   pass 1  S^T = K . Q^T, keeps the row maxima m;
//   pass 2  the same S^T with the same fp32 expression, p = rint(exp(s - m) * 127), O^T += V^T . P^T, sum += p.
//
// Operand layouts (lane l: l15 = l % 16, g = l / 16).  The int8 MFMA contracts 64 slots; lane (l15, g) supplies the 16 bytes
// of slots (g, 0..15) of row / column l15 for either operand, and only the PAIRING of slots matters.
//   S^T:  A = K tile (row = key 16 st + l15, the 16 bytes of D-chunk 4 kk + g), B = Q (column = score row l15, the same chunk,
//         in registers for the whole kernel).  Lane (l15, g) ends with the scores of keys 16 st + 4 g + r, r = 0..3, of row l15.
//   O^T:  after exp / round / pack those four are one dword, and the four dwords of st = 0..3 are the B operand of P.V as they
//         stand: slot (g, 4 st + r) holds key 16 st + 4 g + r.  The A operand is V^T, written to LDS as [d][slot], so a lane reads
//         its 16 slots of row d = 16 db + l15 as one 16-byte vector.  The result holds d = 16 db + 4 g + r of score row l15.
//
// LDS.  K rows are padded from D to D + 16 bytes and V^T rows from 64 to 80 bytes: the 16 lanes of a slot group read 16
// consecutive rows with one ds_read_b128 each, and a row stride of 4 * odd dwords (36 / 20 for K, 20 for V^T) puts those rows on
// 16 distinct 4-bank groups of the 64 banks; unpadded (32 or 16 dwords) every second or fourth row would share its banks.
// Two buffers of (K 64 x (D + 16)) + (V^T D x 80) + 64 key scales: 39 428 bytes at D = 128, 20 996 at D = 64.  The next tile's
// global loads are issued before the MFMAs of the current tile and written to the other buffer behind them: one barrier a tile.
#include "common.h"

namespace mojo {
namespace {

constexpr int SG_KEYS = 64;           // keys per tile
constexpr int SG_ROWS = 64;           // score rows per workgroup
constexpr int SG_VSTR = SG_KEYS + 16; // bytes per V^T row in LDS
constexpr int64_t SG_MAX_KV = 132104; // 127 * 128 * kv_len < 2^31

struct SageArgs {
  const int8_t* q; const float* q_scale; const int8_t* kc; const float* k_scale; const int8_t* vc; const float* v_scale;
  const int* cu_q; const int* cu_kv; const int* tables; bf16_t* out;
  int tokens, hq, hkv, n_blocks, page, max_pages, n_qt, kv_cap, abab;
  int64_t table_stride, c_blk, c_head, c_tok;
  float scale;
};

// the score of one key, the expression of both passes: every product rounded on its own, in this order
__device__ __forceinline__ float sage_score(int dot, float scale, float qs, float ks) {
  return __fmul_rn(__fmul_rn(__fmul_rn(static_cast<float>(dot), scale), qs), ks);
}

// 4 x 4 byte transpose: in[k] holds bytes d0..d3 of key k; out[i] holds byte i of keys 0..3
__device__ __forceinline__ void transpose4x4(const unsigned (&in)[4], unsigned (&out)[4]) {
  const unsigned t0 = __builtin_amdgcn_perm(in[1], in[0], 0x05010400u), t1 = __builtin_amdgcn_perm(in[1], in[0], 0x07030602u);
  const unsigned u0 = __builtin_amdgcn_perm(in[3], in[2], 0x05010400u), u1 = __builtin_amdgcn_perm(in[3], in[2], 0x07030602u);
  out[0] = __builtin_amdgcn_perm(u0, t0, 0x05040100u);
  out[1] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);
  out[2] = __builtin_amdgcn_perm(u1, t1, 0x05040100u);
  out[3] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);
}

template <int D, int G>
__global__ __launch_bounds__(256) void sage_prefill_kernel(const SageArgs a) {
  constexpr int KK = D / 64;              // MFMAs per 16-key score sub-tile
  constexpr int DB = D / 16;              // 16-channel blocks of the output
  constexpr int KSTR = D + 16;            // bytes per K row in LDS
  constexpr int KCH = D / 16;             // 16-byte chunks per K row
  constexpr int KPT = SG_KEYS * KCH / 256;// K chunks per thread and tile
  constexpr int DW = D / 64;              // V dwords per thread and key
  constexpr int TOK = SG_ROWS / G;        // query tokens per workgroup
  constexpr int K_BYTES = SG_KEYS * KSTR, V_BYTES = D * SG_VSTR;

  __shared__ __attribute__((aligned(16))) unsigned char s_k[2][K_BYTES];
  __shared__ __attribute__((aligned(16))) unsigned char s_v[2][V_BYTES];
  __shared__ __attribute__((aligned(16))) float s_ks[2][SG_KEYS];
  __shared__ int s_fn;

  const int qt = a.n_qt - 1 - static_cast<int>(blockIdx.x), kvh = blockIdx.y, b = blockIdx.z;
  const int q_start = max(a.cu_q[b], 0), q_len = min(a.cu_q[b + 1], a.tokens) - q_start;
  const int kv_len = min(a.cu_kv ? a.cu_kv[b + 1] - a.cu_kv[b] : q_len, a.kv_cap);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, l15 = lane & 15;

  auto head_of = [&](int gi) { return a.abab ? gi * a.hkv + kvh : kvh * G + gi; };
  // rows [pos0, pos1) of this sequence, the G heads of this kv head, written as zeros
  auto zero_rows = [&](int pos0, int pos1) {
    constexpr int CH = D / 8;
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int i = threadIdx.x; i < (pos1 - pos0) * G * CH; i += 256) {
      const int c = i % CH, gi = (i / CH) % G, pos = pos0 + i / (CH * G);
      *reinterpret_cast<u32x4*>(a.out + (static_cast<int64_t>(q_start + pos) * a.hq + head_of(gi)) * D + c * 8) = z;
    }
  };
  // rows no tile of the launch covers read as zeros: those of a sequence longer than the max_q_len hint, and the padding
  // tokens behind the last sequence
  if (qt == a.n_qt - 1)
    zero_rows(max(min(q_len, a.n_qt * TOK), 0), b == static_cast<int>(gridDim.z) - 1 ? a.tokens - q_start : q_len);
  if (qt * TOK >= q_len) return;
  const int pos_end = min(q_len, (qt + 1) * TOK);
  const int offset = kv_len - q_len;                       // query position i sees keys 0 .. offset + i
  const int kv_hi = min(kv_len, offset + pos_end);         // keys [0, kv_hi) are visible to some row of the tile
  if (kv_hi <= 0) {                                        // no keys, or none that a row of this tile sees
    zero_rows(qt * TOK, pos_end);
    return;
  }
  const int n_tiles = (kv_hi + SG_KEYS - 1) / SG_KEYS;

  // ---- the first hole: a page id that is negative or outside the pool.  Every key from there on is a zero K / V row (score 0,
  // counted in the row sum), as in the 16-bit prefill.  (kv_hi <= kv_cap <= page * max_pages: the scan stays inside the table.)
  const int* table = a.tables + static_cast<int64_t>(b) * a.table_stride;
  int first_hole_key = 0x7fffffff;
  {
    const int p1 = (kv_hi + a.page - 1) / a.page;
    if (threadIdx.x == 0) s_fn = 0x7fffffff;
    __syncthreads();
    for (int i = threadIdx.x; i < p1; i += 256) {
      const int id = table[i];
      if (id < 0 || id >= a.n_blocks) { atomicMin(&s_fn, i); break; }   // (an LDS minimum: the same value whatever the order)
    }
    __syncthreads();
    const int fn = s_fn;
    if (fn != 0x7fffffff) first_hole_key = fn * a.page;
  }

  // ---- this lane's score row and its Q fragments
  const int row = wave * 16 + l15, pos = qt * TOK + row / G, head = head_of(row % G);
  const bool row_ok = pos < q_len;
  const int limit = row_ok ? offset + pos : -1;            // the last visible key of the row
  const int wave_pos_last = min(pos_end - 1, qt * TOK + (wave * 16 + 15) / G);
  const int wave_limit = qt * TOK + (wave * 16) / G < q_len ? offset + wave_pos_last : -1;   // wave-uniform
  const int64_t row_off = (static_cast<int64_t>(q_start + (row_ok ? pos : 0)) * a.hq + head) * D;
  i32x4 qf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    const i32x4 z = {0, 0, 0, 0};
    qf[kk] = row_ok ? *reinterpret_cast<const i32x4*>(a.q + row_off + (kk * 4 + g) * 16) : z;
  }
  const float qs = row_ok ? a.q_scale[static_cast<int64_t>(head) * a.tokens + q_start + pos] : 0.f;

  // ---- staging: global -> registers (issued a tile ahead) -> LDS
  const int64_t head_base = static_cast<int64_t>(kvh) * a.c_head;
  // the cache row of key `key` (clamped into the visible range), -1 for a hole
  auto key_row = [&](int key, int& lp, int& in_page) -> int64_t {
    key = min(key, kv_hi - 1);
    lp = key / a.page;
    in_page = key - lp * a.page;
    if (key >= first_hole_key) return -1;
    return static_cast<int64_t>(table[lp]) * a.c_blk + head_base + static_cast<int64_t>(in_page) * a.c_tok;
  };
  u32x4 kreg[KPT];
  unsigned vreg[DW][4];
  float ksreg = 0.f;
  auto load_tile = [&](int t, bool with_v) {
    int lp, ip;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int c = threadIdx.x + i * 256, kl = c / KCH, ch = c % KCH;
      const int64_t r = key_row(t * SG_KEYS + kl, lp, ip);
      const u32x4 z = {0u, 0u, 0u, 0u};
      kreg[i] = r >= 0 ? *reinterpret_cast<const u32x4*>(a.kc + r + ch * 16) : z;
    }
    if (threadIdx.x < SG_KEYS) {
      const int64_t r = key_row(t * SG_KEYS + threadIdx.x, lp, ip);
      ksreg = r >= 0 ? a.k_scale[(static_cast<int64_t>(table[lp]) * a.hkv + kvh) * a.page + ip] : 0.f;
    }
    if (with_v) {
      const int kg = threadIdx.x >> 4, cu = threadIdx.x & 15;     // keys 4 kg .. 4 kg + 3, dwords cu * DW .. of their rows
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t r = key_row(t * SG_KEYS + kg * 4 + k, lp, ip);
#pragma unroll
        for (int w = 0; w < DW; ++w)
          vreg[w][k] = r >= 0 ? *reinterpret_cast<const unsigned*>(a.vc + r + (cu * DW + w) * 4) : 0u;
      }
    }
  };
  auto store_tile = [&](int buf, bool with_v) {
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int c = threadIdx.x + i * 256, kl = c / KCH, ch = c % KCH;
      *reinterpret_cast<u32x4*>(&s_k[buf][kl * KSTR + ch * 16]) = kreg[i];
    }
    if (threadIdx.x < SG_KEYS) s_ks[buf][threadIdx.x] = ksreg;
    if (with_v) {
      const int kg = threadIdx.x >> 4, cu = threadIdx.x & 15;
      const int slot = (kg & 3) * 16 + (kg >> 2) * 4;      // keys 16 st + 4 g + r sit at slots 16 g + 4 st + r
#pragma unroll
      for (int w = 0; w < DW; ++w) {
        unsigned tr[4];
        transpose4x4(vreg[w], tr);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<unsigned*>(&s_v[buf][((cu * DW + w) * 4 + i) * SG_VSTR + slot]) = tr[i];
      }
    }
  };

  // ---- the scores of one 16-key sub-tile of the staged tile
  auto sub_scores = [&](int buf, int st, float (&s)[4]) {
    i32x4 acc = {0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const i32x4 kf = *reinterpret_cast<const i32x4*>(&s_k[buf][(st * 16 + l15) * KSTR + (kk * 4 + g) * 16]);
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(kf, qf[kk], acc, 0, 0, 0);
    }
    const f32x4 ks = *reinterpret_cast<const f32x4*>(&s_ks[buf][st * 16 + g * 4]);
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = sage_score(acc[r], a.scale, qs, ks[r]);
  };

  // ---- pass 1: the row maxima
  float m = -__builtin_inff();
  load_tile(0, false);
  store_tile(0, false);
  __syncthreads();
  for (int t = 0; t < n_tiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < n_tiles) load_tile(t + 1, false);
    if (t * SG_KEYS <= wave_limit) {
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        float s[4];
        sub_scores(buf, st, s);
        const int key0 = t * SG_KEYS + st * 16 + g * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) m = key0 + r <= limit ? fmaxf(m, s[r]) : m;      // a select: a hidden NaN never enters
      }
    }
    if (t + 1 < n_tiles) store_tile(buf ^ 1, false);
    __syncthreads();
  }
  m = xor_max_16_32(m);

  // ---- pass 2: quantised probabilities against m, integer P.V and row sum
  i32x4 o[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) o[db] = i32x4{0, 0, 0, 0};
  int psum = 0;
  load_tile(0, true);
  store_tile(0, true);
  __syncthreads();
  for (int t = 0; t < n_tiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < n_tiles) load_tile(t + 1, true);
    if (t * SG_KEYS <= wave_limit) {
      i32x4 pf;
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        float s[4];
        sub_scores(buf, st, s);
        const int key0 = t * SG_KEYS + st * 16 + g * 4;
        unsigned packed = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = key0 + r <= limit ? static_cast<int>(__builtin_rintf(__fmul_rn(expf(s[r] - m), 127.0f))) : 0;
          psum += p;
          packed |= static_cast<unsigned>(p) << (8 * r);
        }
        pf[st] = static_cast<int>(packed);
      }
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const i32x4 vf = *reinterpret_cast<const i32x4*>(&s_v[buf][(db * 16 + l15) * SG_VSTR + g * 16]);
        o[db] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pf, o[db], 0, 0, 0);
      }
    }
    if (t + 1 < n_tiles) store_tile(buf ^ 1, true);
    __syncthreads();
  }
  psum += __shfl_xor(psum, 16);
  psum += __shfl_xor(psum, 32);

  // ---- epilogue: float(acc) * value_scale / float(sum), one rounding; a row that saw no key stores zeros
  if (!row_ok) return;
  const float den = static_cast<float>(psum);
  bf16_t* orow = a.out + row_off;
#pragma unroll
  for (int db = 0; db < DB; ++db) {
    const int d0 = db * 16 + g * 4;
    const f32x4 vs = *reinterpret_cast<const f32x4*>(a.v_scale + kvh * D + d0);
    bf16x4 w;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      w[r] = static_cast<bf16_t>(psum > 0 ? __fdiv_rn(__fmul_rn(static_cast<float>(o[db][r]), vs[r]), den) : 0.f);
    *reinterpret_cast<bf16x4*>(orow + d0) = w;
  }
}

template <int D, int G>
int sage_launch(const SageArgs& a, int batch, hipStream_t stream) {
  hipLaunchKernelGGL((sage_prefill_kernel<D, G>), dim3(a.n_qt, a.hkv, batch), dim3(256), 0, stream, a);
  MOJO_CHECK_LAUNCH("paged_prefill_sage_gqa");
  note_launch("sage_prefill:d%d:g%d", D, G);
  return 0;
}

template <int D>
int sage_dispatch_group(const SageArgs& a, int group, int batch, hipStream_t stream) {
  switch (group) {
    case 1: return sage_launch<D, 1>(a, batch, stream);
    case 2: return sage_launch<D, 2>(a, batch, stream);
    case 4: return sage_launch<D, 4>(a, batch, stream);
    default: return sage_launch<D, 8>(a, batch, stream);
  }
}

}  // namespace
}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_paged_prefill_sage_gqa(const void* query, const void* query_scale, const void* key_cache,
                                               const void* key_scale, const void* value_cache, const void* value_scale,
                                               const void* cu_q_lens, const void* cu_total_seq_lens, const void* block_tables,
                                               void* out, int64_t tokens, int64_t batch, int64_t hq, int64_t hkv, int64_t dim,
                                               int64_t n_blocks, int64_t page, int64_t max_pages, int64_t table_stride,
                                               int64_t cache_block_stride, int64_t cache_head_stride, int64_t cache_token_stride,
                                               int64_t max_q_len, int64_t max_total_seq_len, float softmax_scale, int abab,
                                               mojo_stream_t stream) {
  const char* what = "paged_prefill_sage_gqa";
  MOJO_REQUIRE(tokens >= 0 && batch >= 0 && hq > 0 && hkv > 0 && hq % hkv == 0, MOJO_EINVAL, "%s: bad sizes", what);
  const int64_t group = hq / hkv;
  MOJO_REQUIRE(dim == 64 || dim == 128, MOJO_EUNSUPPORTED, "%s: head_dim %lld (64 and 128 are compiled)", what, (long long)dim);
  MOJO_REQUIRE(page > 0 && page % 16 == 0 && page <= 256, MOJO_EUNSUPPORTED, "%s: page %lld (a multiple of 16, at most 256)", what,
               (long long)page);
  MOJO_REQUIRE(group == 1 || group == 2 || group == 4 || group == 8, MOJO_EUNSUPPORTED, "%s: group %lld (1, 2, 4, 8)", what,
               (long long)group);
  MOJO_REQUIRE(cache_block_stride % 16 == 0 && cache_head_stride % 16 == 0 && cache_token_stride % 16 == 0 && cache_token_stride >= dim,
               MOJO_EUNSUPPORTED, "%s: cache strides must be multiples of 16 bytes", what);
  MOJO_REQUIRE(batch < 65536 && hkv < 65536 && tokens < (int64_t{1} << 23) && n_blocks < (int64_t{1} << 31) &&
               max_pages >= 0 && max_pages < (int64_t{1} << 31) / 256, MOJO_EUNSUPPORTED, "%s: sizes beyond the launch's range", what);
  int64_t kv_cap = page * max_pages;
  if (max_total_seq_len > 0 && max_total_seq_len < kv_cap) kv_cap = max_total_seq_len;
  MOJO_REQUIRE(kv_cap <= SG_MAX_KV, MOJO_EUNSUPPORTED,
               "%s: up to %lld keys a sequence (int32 accumulators: 127 * 128 * kv_len < 2^31); min(max_total_seq_len, page * "
               "table width) is %lld", what, (long long)SG_MAX_KV, (long long)kv_cap);
  if (tokens == 0 || batch == 0) return 0;
  MOJO_REQUIRE(query && query_scale && key_cache && key_scale && value_cache && value_scale && cu_q_lens && block_tables && out,
               MOJO_EINVAL, "%s: null pointer", what);
  MOJO_REQUIRE(aligned_to(query, 16) && aligned_to(key_cache, 16) && aligned_to(value_cache, 16) && aligned_to(value_scale, 16) &&
               aligned_to(out, 16), MOJO_EINVAL, "%s: query, caches, value_scale and out must be 16-byte aligned", what);
  SageArgs a;
  a.q = static_cast<const int8_t*>(query); a.q_scale = static_cast<const float*>(query_scale);
  a.kc = static_cast<const int8_t*>(key_cache); a.k_scale = static_cast<const float*>(key_scale);
  a.vc = static_cast<const int8_t*>(value_cache); a.v_scale = static_cast<const float*>(value_scale);
  a.cu_q = static_cast<const int*>(cu_q_lens); a.cu_kv = static_cast<const int*>(cu_total_seq_lens);
  a.tables = static_cast<const int*>(block_tables); a.out = static_cast<bf16_t*>(out);
  a.tokens = static_cast<int>(tokens); a.hq = static_cast<int>(hq); a.hkv = static_cast<int>(hkv);
  a.n_blocks = static_cast<int>(n_blocks); a.page = static_cast<int>(page); a.max_pages = static_cast<int>(max_pages);
  const int64_t q_cap = max_q_len > 0 && max_q_len < tokens ? max_q_len : tokens;
  const int64_t tok_per_tile = SG_ROWS / group;
  a.n_qt = static_cast<int>(ceil_div(q_cap, tok_per_tile));
  a.kv_cap = static_cast<int>(kv_cap); a.abab = abab ? 1 : 0;
  a.table_stride = table_stride; a.c_blk = cache_block_stride; a.c_head = cache_head_stride; a.c_tok = cache_token_stride;
  a.scale = softmax_scale;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dim == 64 ? sage_dispatch_group<64>(a, static_cast<int>(group), static_cast<int>(batch), s)
                   : sage_dispatch_group<128>(a, static_cast<int>(group), static_cast<int>(batch), s);
}
