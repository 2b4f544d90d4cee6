// MojoPrefillNSA / MojoPagedPrefillNSA (NSA_PREFILL_OPS): native sparse attention for packed var-len queries.
// Row r of a sequence sees the first t_kv(r) keys (causal: kv_len - q_len + r + 1, else kv_len) and is the decode step of
// nsa_decode.hip on them.  The two identities of §4.28 hold per row: q . mean(k) = mean(q . k), and the three branches and the
// gate collapse into ONE weight per (row, key),
//     w = g0 * pc[t / cr] / cr  +  g1 * psel_t  +  g2 * pwin_t,
// so prefill is S = scale * Q K^T on the matrix cores, a row-wise map S -> W, and O = W V on the matrix cores.  A row with
// 0 < t_kv < cr is the same formula with groups of one key (the reference does not compress such a context).
//
// Work split: a workgroup of NW waves (4, 2 or 1, chosen by nsa_prefill_plan() from the shapes) owns one (sequence, head) and
// 16 * NW consecutive query rows, a wave 16 of them; workgroups are queued longest row tile first.  Everything is transposed
// (v_mfma_f32_16x16x32): S^T[key][q] = K Q^T and O^T[d][q] += V^T W^T, so lane (q = lane % 16, grp = lane / 16) holds keys
// 16 t + 4 grp + r of row q: a row's statistics live in four lanes, and W^T feeds the second product in the accumulators' own
// key order (V^T is read in the same order by transposed LDS reads).  K / V tiles of 64 keys go through LDS, 256-byte rows,
// the 16-byte chunk c of key r at c ^ (r & 15) for K (fragment reads) and at c ^ ((r & 7) << 1) for V (transposed reads); a
// 16-key piece of a tile never crosses a page.
//
// Two walks over K, S is never materialised:
//   statistics  per (row, selection block) TWO fp32 values in LDS, both log-sum-exps in log2 units: over the block's complete
//               groups (the block score: its order is the order of the reference's sums of probabilities, and the row's pc
//               normaliser is the log-sum-exp of them) and over the block's visible keys (what a taken block adds to the
//               selected softmax's normaliser).  compress_ratio divides 16, so a group lies in one lane (cr <= 4) or in two or
//               four lanes of one 16-key piece (cr 8, 16: two shuffles).  The block index depends on the key alone, so the lanes
//               accumulate the current block's partials and the wave writes them when the block changes: no read-modify-write.
//               The window softmax's maximum and sum are lane partials of the same walk.
//   select      per row, on its four lanes: the pc normaliser, min(nsel, nb_r) rounds of arg-max over (score, index) — the
//               lower index wins among equals —, a taken entry is marked +inf and its key statistic joins the selected
//               normaliser; the gate.
//   weights     S^T again, W^T in registers from the three known normalisers, one rounding to the storage type, the second
//               product, fp32 accumulation, one rounding of the output.  The selected and the window term are skipped on 16-key
//               pieces where a ballot shows no row of the wave has them.  On a 32-key step where a ballot shows a weight of 2^-4
//               or more, the residual of W's rounding takes a second product: a row with one to three keys has weights near
//               g0 + g1 + g2, and 2^-9 of that times |v| is more than the output's own rounding.
// No atomics on floats and every merge in a fixed order: two calls give the same bits.
//
// The contiguous operator is the computed-row-address instance (PAGED = false): key j of sequence b is row cu_q[b] + j.
// Keys from the first negative or out-of-pool page id on are zero K / V rows: score 0, counted by every softmax, nothing added
// to the output; such a page is never read, and nothing behind the last visible key of a row tile is read.
#include "common.h"

namespace mojo {
namespace {

constexpr int NP_KEYS = 64;                       // keys per tile
constexpr int NP_TILE_BYTES = NP_KEYS * 256;      // one K or V tile
constexpr int NP_MAX_SEL = 64;
constexpr int64_t NP_STAT_BYTES = 120 * 1024;     // the two statistics arrays of a workgroup
constexpr float NP_LOG2E = 1.4426950408889634f;
constexpr float NP_FLOOR = -1.0e30f;              // "no key yet" of a running maximum (finite: differences stay finite)

typedef __attribute__((address_space(3))) char np_lds;

struct NsaPrefillArgs {
  const void* q; const void* k; const void* v; const void* gate; void* out;
  const int* cu_q; const int* cu_kv; const int* tables;
  int heads, batch, n_qt, n_blocks, page, max_pages, cr, bs, nsel, ws, causal, gate_f32, nbs;
  int64_t table_stride, blk_stride, head_stride, tok_stride;
  float scale_log2;
};

template <typename T> struct np_mfma;
template <> struct np_mfma<bf16_t> {
  typedef bf16x8 frag;
  static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct np_mfma<f16_t> {
  typedef f16x8 frag;
  static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

// a running (maximum, sum of 2^(x - maximum)) pair
struct NpLse {
  float m = NP_FLOOR, l = 0.f;
  __device__ __forceinline__ void add4(const float (&x)[4], const bool (&on)[4]) {
    float mx = m;
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = on[r] ? fmaxf(mx, x[r]) : mx;
    float s = l * fast_exp2(m - mx);
#pragma unroll
    for (int r = 0; r < 4; ++r) s += on[r] ? fast_exp2(x[r] - mx) : 0.f;
    m = mx; l = s;
  }
  __device__ __forceinline__ void add_lse(float x) {           // x: a log-sum-exp (may be -inf: adds nothing)
    const float mx = fmaxf(m, x);
    l = l * fast_exp2(m - mx) + fast_exp2(x - mx);
    m = mx;
  }
  // the four lanes of a row, in a fixed order; every lane returns the row's log-sum-exp (-inf without a term)
  __device__ __forceinline__ float row_lse() const {
    float mx = fmaxf(m, __shfl_xor(m, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float s = l * fast_exp2(m - mx);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    return s > 0.f ? mx + __log2f(s) : -INFINITY;
  }
};

// the mean of the group of `cr` keys (cr divides 16) that each of the lane's four keys 4 grp + r of a 16-key piece lies in
__device__ __forceinline__ void np_group_means(const float (&s)[4], int cr, float (&g)[4]) {
  if (cr == 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) g[r] = s[r];
  } else if (cr == 2) {
    g[0] = g[1] = (s[0] + s[1]) * 0.5f;
    g[2] = g[3] = (s[2] + s[3]) * 0.5f;
  } else {
    float x = (s[0] + s[1]) + (s[2] + s[3]);
    if (cr >= 8) x += __shfl_xor(x, 16);
    if (cr == 16) x += __shfl_xor(x, 32);
    x *= 1.0f / static_cast<float>(cr);
#pragma unroll
    for (int r = 0; r < 4; ++r) g[r] = x;
  }
}

template <typename T, int D, bool PAGED>
__global__ __launch_bounds__(256) void nsa_prefill_kernel(NsaPrefillArgs a) {
  typedef typename np_mfma<T>::frag frag;
  typedef typename vec_of<T, 8>::type V8;
  constexpr int DK = D / 32, DT = D / 16, CH = D / 8;
  extern __shared__ __attribute__((aligned(1024))) char np_smem[];
  __shared__ int s_first_bad;
  np_lds* smem = (np_lds*)np_smem;
  const int nthreads = blockDim.x, rows_wg = nthreads >> 2;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int l15 = lane & 15, grp = lane >> 4;

  // longest first: the row tile is the slow coordinate, descending
  const int inner = a.heads * a.batch;
  const int qt = a.n_qt - 1 - static_cast<int>(blockIdx.x) / inner;
  const int rem = static_cast<int>(blockIdx.x) % inner;
  const int h = rem % a.heads, b = rem / a.heads;
  const int q0 = a.cu_q[b], q_len = a.cu_q[b + 1] - q0;
  if (qt * rows_wg >= q_len) return;
  int kv_len = a.cu_kv ? a.cu_kv[b + 1] - a.cu_kv[b] : q_len;
  kv_len = kv_len < 0 ? 0 : kv_len;
  if (kv_len > a.page * a.max_pages) kv_len = a.page * a.max_pages;                // (the capacity the statistics are sized on)
  const int last = (qt + 1) * rows_wg < q_len ? (qt + 1) * rows_wg : q_len;        // one past the tile's last row
  int kv_hi = a.causal ? kv_len - q_len + last : kv_len;                            // keys [0, kv_hi) are seen by some row
  kv_hi = kv_hi < 0 ? 0 : (kv_hi > kv_len ? kv_len : kv_hi);

  // this lane's row
  const int pos = qt * rows_wg + wave * 16 + l15;
  const bool row_ok = pos < q_len;
  int t_kv = a.causal ? kv_len - q_len + pos + 1 : kv_len;
  t_kv = !row_ok || t_kv < 0 ? 0 : (t_kv > kv_len ? kv_len : t_kv);
  const bool quirk = t_kv < a.cr;                                                   // groups of one key
  const int cre = quirk ? 1 : a.cr;
  const int win0 = t_kv > a.ws ? t_kv - a.ws : 0;
  const T* qrow = static_cast<const T*>(a.q) + (static_cast<int64_t>(q0 + (row_ok ? pos : q_len - 1)) * a.heads + h) * D;
  frag qf[DK];
#pragma unroll
  for (int ks = 0; ks < DK; ++ks) qf[ks] = *reinterpret_cast<const frag*>(qrow + ks * 32 + grp * 8);

  // keys with a K / V row: up to the first page that is not there
  int stage_end = kv_hi;
  if constexpr (PAGED) {
    if (threadIdx.x == 0) s_first_bad = 0x7fffffff;
    __syncthreads();
    const int n_pages = (kv_hi + a.page - 1) / a.page;
    for (int j = threadIdx.x; j < n_pages; j += nthreads) {
      const int id = a.tables[b * a.table_stride + j];
      if (id < 0 || id >= a.n_blocks) atomicMin(&s_first_bad, j);                  // (an integer minimum: order-free)
    }
    __syncthreads();
    const int64_t keys = static_cast<int64_t>(s_first_bad) * a.page;
    if (keys < stage_end) stage_end = static_cast<int>(keys);
  }

  // ---- staging: tile [t0, t0 + 64) of `src` into the image at `dst`; zeros past stage_end -------------------------------------------
  auto stage = [&](const void* srcv, np_lds* dst, bool is_v, int t0) {
    const T* src = static_cast<const T*>(srcv);
    for (int j = 0; j < 4; ++j) {
      const int k0 = t0 + 16 * j;
      int64_t base = 0;
      if (k0 < stage_end) {
        if constexpr (PAGED) {
          const int pi = k0 / a.page;
          base = a.tables[b * a.table_stride + pi] * a.blk_stride + h * a.head_stride + (k0 - pi * a.page) * a.tok_stride;
        } else {
          base = (static_cast<int64_t>(q0) + k0) * a.tok_stride + h * a.head_stride;
        }
      }
      for (int i = threadIdx.x; i < 16 * CH; i += nthreads) {
        const int r = i / CH, c = i % CH, row = 16 * j + r;
        V8 x;
        if (k0 + r < stage_end) {
          x = load_vec<T, 8>(src + base + r * a.tok_stride + c * 8);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = elt<T>::from_f(0.f);
        }
        const int at = is_v ? c ^ ((row & 7) << 1) : c ^ (row & 15);
        *reinterpret_cast<__attribute__((address_space(3))) V8*>(dst + row * 256 + at * 16) = x;
      }
    }
  };
  np_lds* k_img = smem;
  np_lds* v_img = smem + NP_TILE_BYTES;
  float* blk_lse = reinterpret_cast<float*>(np_smem + 2 * NP_TILE_BYTES) + (wave * 16 + l15) * a.nbs;   // this row's block scores
  float* key_lse = blk_lse + rows_wg * a.nbs;                                                           // ... and key statistics

  // S^T of 16-key piece t of the staged tile, in log2 units: s[r] = key 16 t + 4 grp + r of row l15
  auto scores = [&](int t, float (&s)[4]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < DK; ++ks) {
      const frag kf = *reinterpret_cast<const __attribute__((address_space(3))) frag*>(
          k_img + (t * 16 + l15) * 256 + (((ks * 4 + grp) ^ l15) * 16));
      acc = np_mfma<T>::run(kf, qf[ks], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = acc[r] * a.scale_log2;
  };

  const int n_tiles = (kv_hi + NP_KEYS - 1) / NP_KEYS;

  // ---- walk 1: statistics -----------------------------------------------------------------------------------------------------------
  NpLse win, grp_acc, key_acc;
  int cb = -1;                                                   // the block the lane partials belong to (wave-uniform)
  auto flush = [&]() {
    const float gl = grp_acc.row_lse(), kl = key_acc.row_lse();
    if (grp == 0) { blk_lse[cb] = gl; key_lse[cb] = kl; }
    grp_acc = NpLse(); key_acc = NpLse();
  };
  for (int tile = 0; tile < n_tiles; ++tile) {
    __syncthreads();
    stage(a.k, k_img, false, tile * NP_KEYS);
    __syncthreads();
    for (int t = 0; t < 4; ++t) {
      const int k0 = tile * NP_KEYS + 16 * t;
      if (k0 >= kv_hi) break;
      float s[4], g[4];
      scores(t, s);
      np_group_means(s, a.cr, g);
      const int key = k0 + 4 * grp;
      bool seen[4], in_win[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        seen[r] = key + r < t_kv;
        in_win[r] = seen[r] && key + r >= win0;
        if (quirk) g[r] = s[r];
      }
      if (__any(in_win[0] || in_win[1] || in_win[2] || in_win[3])) win.add4(s, in_win);
      const int k1 = (k0 + 16 < kv_hi ? k0 + 16 : kv_hi) - 1;
      for (int blk = k0 / a.bs; blk <= k1 / a.bs; ++blk) {
        if (blk != cb) {
          if (cb >= 0) flush();
          cb = blk;
        }
        bool on_key[4], on_grp[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          on_key[r] = seen[r] && key + r >= blk * a.bs && key + r < (blk + 1) * a.bs;
          on_grp[r] = on_key[r] && ((key + r) & (cre - 1)) == cre - 1;      // the group's last key: the group is complete
        }
        key_acc.add4(s, on_key);
        grp_acc.add4(g, on_grp);
      }
    }
  }
  if (cb >= 0) flush();
  const float lse_win = win.row_lse();
  __syncthreads();

  // ---- select: this row on its four lanes, entry i by lane i % 4 -----------------------------------------------------------------
  const int nb_r = (t_kv + a.bs - 1) / a.bs;
  float lse_c, lse_s, gate[3];
  {
    NpLse all;
    for (int i = grp; i < nb_r; i += 4) all.add_lse(blk_lse[i]);
    lse_c = all.row_lse();
    NpLse taken;
    const int n_sel = a.nsel < nb_r ? a.nsel : nb_r;
    for (int round = 0; round < a.nsel; ++round) {
      if (!__any(round < n_sel)) break;
      float best = -INFINITY;
      int at = 0x7fffffff;
      for (int i = grp; i < nb_r; i += 4) {
        const float x = blk_lse[i];
        if (x != INFINITY && (at == 0x7fffffff || x > best)) { best = x; at = i; }
      }
#pragma unroll
      for (int m = 16; m <= 32; m <<= 1) {
        const float o = __shfl_xor(best, m);
        const int oi = __shfl_xor(at, m);
        if (oi != 0x7fffffff && (at == 0x7fffffff || o > best || (o == best && oi < at))) { best = o; at = oi; }
      }
      if (round < n_sel && at != 0x7fffffff && (at & 3) == grp) {
        taken.add_lse(key_lse[at]);
        blk_lse[at] = INFINITY;                                  // taken
      }
    }
    lse_s = taken.row_lse();
    if (lse_s == -INFINITY) lse_s = INFINITY;                    // nothing taken: the term vanishes
    float gsum[3] = {0.f, 0.f, 0.f};
    for (int d = grp * (D / 4); d < (grp + 1) * (D / 4); ++d) {
      const float qd = elt<T>::to_f(qrow[d]);
      const int64_t g_at = (static_cast<int64_t>(h) * D + d) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        gsum[c] = fmaf(qd, a.gate_f32 ? static_cast<const float*>(a.gate)[g_at + c] : elt<T>::to_f(static_cast<const T*>(a.gate)[g_at + c]), gsum[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      gsum[c] += __shfl_xor(gsum[c], 16);
      gsum[c] += __shfl_xor(gsum[c], 32);
      gate[c] = 1.0f / (1.0f + fast_exp2(-gsum[c] * NP_LOG2E));
    }
    gate[0] *= 1.0f / static_cast<float>(cre);
  }

  // ---- walk 2: weights and the second product ----------------------------------------------------------------------------------------
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tq = l15 >> 2, tp = l15 & 3;
  for (int tile = 0; tile < n_tiles; ++tile) {
    __syncthreads();                                             // (the first one also publishes the taken marks)
    stage(a.k, k_img, false, tile * NP_KEYS);
    stage(a.v, v_img, true, tile * NP_KEYS);
    __syncthreads();
    float w[4][4];
    for (int t = 0; t < 4; ++t) {
      const int k0 = tile * NP_KEYS + 16 * t;
#pragma unroll
      for (int r = 0; r < 4; ++r) w[t][r] = 0.f;
      if (k0 >= kv_hi) continue;
      float s[4], g[4];
      scores(t, s);
      np_group_means(s, a.cr, g);
      const int key = k0 + 4 * grp;
      bool seen[4], in_win[4], in_sel[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        seen[r] = key + r < t_kv;
        in_win[r] = seen[r] && key + r >= win0;
        in_sel[r] = false;
        if (quirk) g[r] = s[r];
        if (seen[r] && ((key + r) | (cre - 1)) < t_kv) w[t][r] = gate[0] * fast_exp2(g[r] - lse_c);
      }
      const int k1 = (k0 + 16 < kv_hi ? k0 + 16 : kv_hi) - 1;
      for (int blk = k0 / a.bs; blk <= k1 / a.bs; ++blk) {
        const bool is_taken = blk < nb_r && blk_lse[blk] == INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) in_sel[r] = in_sel[r] || (is_taken && seen[r] && key + r >= blk * a.bs && key + r < (blk + 1) * a.bs);
      }
      if (__any(in_sel[0] || in_sel[1] || in_sel[2] || in_sel[3])) {
#pragma unroll
        for (int r = 0; r < 4; ++r) w[t][r] += in_sel[r] ? gate[1] * fast_exp2(s[r] - lse_s) : 0.f;
      }
      if (__any(in_win[0] || in_win[1] || in_win[2] || in_win[3])) {
#pragma unroll
        for (int r = 0; r < 4; ++r) w[t][r] += in_win[r] ? gate[2] * fast_exp2(s[r] - lse_win) : 0.f;
      }
    }
    // O^T += V^T W^T: a 32-key step takes the lane's keys of pieces 2 kk and 2 kk + 1; V^T is read in that order
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      // W^T rounded once to the storage type; where a weight of the step is 2^-4 or more (a row with few keys, a sharp row) the
      // residual of that rounding goes through the matrix cores as well.  Below it a residual moves an output by less than
      // 2^-13 |v| a key, and the step is one product.
      frag wf, wr;
      bool large = false;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const float x = w[2 * kk + half][r];
          const T hi = elt<T>::from_f(x);
          wf[4 * half + r] = hi;
          wr[4 * half + r] = elt<T>::from_f(x - elt<T>::to_f(hi));
          large = large || x >= 0.0625f;
        }
      }
      const bool residual = __any(large);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        s16x4 part[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int row = (2 * kk + half) * 16 + 4 * grp + tq;
          np_lds* at = v_img + row * 256 + (((2 * dt + (tp >> 1)) ^ ((row & 7) << 1)) * 16) + (tp & 1) * 8;
          part[half] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<__attribute__((address_space(3))) s16x4*>(at));
        }
        const s16x8 both = {part[0][0], part[0][1], part[0][2], part[0][3], part[1][0], part[1][1], part[1][2], part[1][3]};
        o[dt] = np_mfma<T>::run(__builtin_bit_cast(frag, both), wf, o[dt]);
        if (residual) o[dt] = np_mfma<T>::run(__builtin_bit_cast(frag, both), wr, o[dt]);
      }
    }
  }

  // O^T[d = 16 dt + 4 grp + r][q = l15]; a row without a key stores zeros
  if (row_ok) {
    typedef typename vec_of<T, 4>::type V4;
    T* orow = static_cast<T*>(a.out) + (static_cast<int64_t>(q0 + pos) * a.heads + h) * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      V4 x;
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] = elt<T>::from_f(o[dt][r]);
      *reinterpret_cast<V4*>(orow + dt * 16 + grp * 4) = x;
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// What a launch is sized on: the shapes alone, so the workspace query and the entry point plan alike.
struct NsaPrefillPlan {
  int status = 0;
  const char* why = "";
  int waves = 4, n_qt = 0, nbs = 1;
  int64_t lds = 0, grid = 0, max_blocks = 0;
};

constexpr int64_t NP_MAX_BLOCKS = NP_STAT_BYTES / (2 * 16 * 4) - 1;      // 959: what one wave's 16 rows can hold

NsaPrefillPlan nsa_prefill_plan(int64_t total_q, int64_t batch, int64_t heads, int64_t dim, int64_t cap, int64_t cr, int64_t bs) {
  NsaPrefillPlan p;
  p.max_blocks = NP_MAX_BLOCKS;
  auto refuse = [&](int code, const char* why) { p.status = code; p.why = why; return p; };
  if (total_q < 0 || batch < 0 || heads <= 0 || cap < 0 || cr <= 0 || bs <= 0) return refuse(MOJO_EINVAL, "bad sizes");
  if (dim != 64 && dim != 128) return refuse(MOJO_EUNSUPPORTED, "head_dim 64 and 128 are compiled");
  if (bs % cr != 0) return refuse(MOJO_EUNSUPPORTED, "block_size must be a multiple of compress_ratio");
  if (16 % cr != 0) return refuse(MOJO_EUNSUPPORTED, "compress_ratio must divide 16");
  if (cap >= (int64_t{1} << 30) || total_q >= (int64_t{1} << 30)) return refuse(MOJO_EUNSUPPORTED, "sizes beyond the launch's range");
  const int64_t blocks = ceil_div(cap, bs) > 0 ? ceil_div(cap, bs) : 1;
  if (blocks > NP_MAX_BLOCKS) return refuse(MOJO_EUNSUPPORTED, "more than 959 selection blocks in a sequence's capacity");
  p.nbs = static_cast<int>(blocks | 1);                                   // (an odd row stride: the rows spread over the banks)
  while (p.waves > 1 && int64_t{2} * 16 * p.waves * p.nbs * 4 > NP_STAT_BYTES) p.waves >>= 1;
  p.lds = 2 * NP_TILE_BYTES + int64_t{2} * 16 * p.waves * p.nbs * 4;
  p.n_qt = static_cast<int>(ceil_div(total_q, 16 * p.waves));
  p.grid = p.n_qt * heads * batch;
  if (p.grid >= (int64_t{1} << 31)) return refuse(MOJO_EUNSUPPORTED, "sizes beyond the launch's range");
  return p;
}

template <typename T, int D, bool PAGED>
int nsa_prefill_launch(const NsaPrefillArgs& a, const NsaPrefillPlan& p, hipStream_t s) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&nsa_prefill_kernel<T, D, PAGED>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(2 * NP_TILE_BYTES + NP_STAT_BYTES));
  hipLaunchKernelGGL((nsa_prefill_kernel<T, D, PAGED>), dim3(static_cast<unsigned>(p.grid)), dim3(64 * p.waves),
                     static_cast<size_t>(p.lds), s, a);
  MOJO_CHECK_LAUNCH("nsa_prefill");
  note_launch("nsa_prefill:w%d:d%d", p.waves, D);
  return 0;
}

template <typename T>
int nsa_prefill_dispatch(const NsaPrefillArgs& a, const NsaPrefillPlan& p, int dim, bool paged, hipStream_t s) {
  if (dim == 64) return paged ? nsa_prefill_launch<T, 64, true>(a, p, s) : nsa_prefill_launch<T, 64, false>(a, p, s);
  return paged ? nsa_prefill_launch<T, 128, true>(a, p, s) : nsa_prefill_launch<T, 128, false>(a, p, s);
}

}  // namespace
}  // namespace mojo

using namespace mojo;

extern "C" int64_t mojo_hip_nsa_prefill_workspace_bytes(int64_t total_q, int64_t batch, int64_t heads, int64_t head_dim,
                                                        int64_t kv_capacity, int64_t compress_ratio, int64_t block_size) {
  const NsaPrefillPlan p = nsa_prefill_plan(total_q, batch, heads, head_dim, kv_capacity, compress_ratio, block_size);
  return p.status != 0 ? -1 : 0;                   // (every statistic lives in LDS: the launch needs no workspace)
}

extern "C" int mojo_hip_nsa_prefill(const void* query, const void* key, const void* value, const void* gate_proj,
                                    const int32_t* cu_q_lens, const int32_t* cu_total_seq_lens, const int32_t* block_tables,
                                    void* out, void* workspace, int64_t workspace_bytes, int64_t total_q, int64_t batch,
                                    int64_t heads, int64_t head_dim, int64_t num_blocks, int64_t page, int64_t max_pages,
                                    int64_t table_stride, int64_t kv_block_stride, int64_t kv_head_stride, int64_t kv_token_stride,
                                    int64_t compress_ratio, int64_t block_size, int64_t num_selected_blocks, int64_t window_size,
                                    int is_causal, float softmax_scale, int dtype, int gate_dtype, mojo_stream_t stream) {
  const char* what = "nsa_prefill";
  (void)workspace; (void)workspace_bytes;
  const bool paged = block_tables != nullptr;
  MOJO_REQUIRE(page >= 0 && max_pages >= 0 && num_selected_blocks >= 0 && window_size >= 0, MOJO_EINVAL, "%s: bad sizes", what);
  MOJO_REQUIRE(dtype == MOJO_BF16 || dtype == MOJO_F16, MOJO_EUNSUPPORTED, "%s: bf16 and fp16 only", what);
  MOJO_REQUIRE(gate_dtype == dtype || gate_dtype == MOJO_F32, MOJO_EUNSUPPORTED, "%s: gate_proj in the query's dtype or fp32", what);
  MOJO_REQUIRE(num_selected_blocks <= NP_MAX_SEL, MOJO_EUNSUPPORTED, "%s: num_selected_blocks %lld (at most %d)", what,
               (long long)num_selected_blocks, NP_MAX_SEL);
  MOJO_REQUIRE(!paged || (page > 0 && page % 16 == 0 && page <= 256), MOJO_EUNSUPPORTED, "%s: page %lld (a multiple of 16, at most 256)",
               what, (long long)page);
  MOJO_REQUIRE(kv_block_stride % 8 == 0 && kv_head_stride % 8 == 0 && kv_token_stride % 8 == 0 && kv_token_stride >= head_dim,
               MOJO_EUNSUPPORTED, "%s: K/V strides must be multiples of 16 bytes", what);
  MOJO_REQUIRE(paged ? (num_blocks >= 0 && num_blocks < (int64_t{1} << 31) && max_pages < (int64_t{1} << 31) / 256)
                     : (max_pages == 1 && cu_total_seq_lens == nullptr),
               MOJO_EINVAL, "%s: bad page pool (contiguous K/V: one page, kv_len = q_len)", what);
  const NsaPrefillPlan p = nsa_prefill_plan(total_q, batch, heads, head_dim, page * max_pages, compress_ratio, block_size);
  MOJO_REQUIRE(p.status == 0, p.status, "%s: %s", what, p.why);
  if (p.grid == 0) return 0;
  MOJO_REQUIRE(query && gate_proj && out && cu_q_lens && key && value, MOJO_EINVAL, "%s: null pointer", what);
  MOJO_REQUIRE(aligned_to(query, 16) && aligned_to(key, 16) && aligned_to(value, 16) && aligned_to(out, 8), MOJO_EINVAL,
               "%s: query, key and value must be 16-byte aligned", what);
  NsaPrefillArgs a;
  a.q = query; a.k = key; a.v = value; a.gate = gate_proj; a.out = out;
  a.cu_q = cu_q_lens; a.cu_kv = cu_total_seq_lens; a.tables = block_tables;
  a.heads = static_cast<int>(heads); a.batch = static_cast<int>(batch); a.n_qt = p.n_qt; a.n_blocks = static_cast<int>(num_blocks);
  a.page = static_cast<int>(page); a.max_pages = static_cast<int>(max_pages); a.cr = static_cast<int>(compress_ratio);
  a.bs = static_cast<int>(block_size); a.nsel = static_cast<int>(num_selected_blocks);
  a.ws = static_cast<int>(window_size < (int64_t{1} << 30) ? window_size : (int64_t{1} << 30));
  a.causal = is_causal ? 1 : 0; a.gate_f32 = gate_dtype == MOJO_F32 ? 1 : 0; a.nbs = p.nbs;
  a.table_stride = table_stride; a.blk_stride = kv_block_stride; a.head_stride = kv_head_stride; a.tok_stride = kv_token_stride;
  a.scale_log2 = softmax_scale * NP_LOG2E;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == MOJO_BF16 ? nsa_prefill_dispatch<bf16_t>(a, p, static_cast<int>(head_dim), paged, s)
                            : nsa_prefill_dispatch<f16_t>(a, p, static_cast<int>(head_dim), paged, s);
}
