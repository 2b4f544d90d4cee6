// MojoDecodeNSA / MojoPagedDecodeNSA (NSA_ATTN_OPS): one decode step of native sparse attention — a compressed,
// a selected and a sliding-window branch over the same K/V, blended by a per-head sigmoid gate.  MHA: K/V have the query's heads.
//
// Two identities carry the design.  q . mean(k_t) = mean(q . k_t), so ONE walk over K gives every score the three branches
// need: s_t = scale * q . k_t in fp32, and the compressed score of a group is the mean of its `cr` token scores.  And
// out_comp = sum_j pc_j * mean_t(v_t), so branches and gate collapse into ONE weight per key,
//     w_t = g0 * pc[t / cr] / cr  (t < C * cr)  +  g1 * psel_t  (t in a selected block)  +  g2 * pwin_t  (t >= sl - ws),
// and one walk over V finishes the step: out = sum_t w_t v_t.  K is read once and V once, the bytes of a dense decode, and no
// [C, H, D] tensor of group means is ever formed.
//
// Three phases per (sequence, head):
//   scores  s_t of every key into an fp32 row.  A key row of D 16-bit elements is D / 8 lanes x 16 bytes, so a wave loads
//           64 / (D / 8) keys per instruction; a tile is 16 keys (never across a page: pages are multiples of 16 tokens), a
//           wave keeps two tiles in flight, the D / 8 lanes of a key add up by DPP.
//   select  on the row: group means, the compressed softmax, the block scores (sums of unnormalised group probabilities: the
//           order is that of the normalised ones), min(nsel, nb) rounds of arg-max in wave 0 — among equal scores the LOWER
//           block index wins —, the maxima and sums of the selected and the window softmax, then s_t is overwritten by w_t.
//   values  sum_t w_t v_t with the load layout of the scores, fp32 accumulators, lanes of one D-chunk merged by shuffles and
//           the waves through LDS, one rounding to the output dtype.
// One query row per head shares no K between heads: there is no second matrix dimension, so no matrix instruction fits.
//
// Two launch forms, chosen by nsa_plan() from the shapes alone.  FUSED: one workgroup of four waves per (b, h), all three
// phases in one launch, the row, the group array and the block scores in dynamic LDS; the waves split the tiles round-robin.
// SPLIT: scores and values on a grid (b * h, key slice), select per (b, h) on 1024 threads, a fourth launch adds the slices'
// partial outputs in slice order; the rows, groups and partials live in the caller's workspace.  No atomics in either form:
// two calls give the same bits.
//
// The contiguous operator is the computed-row-address instance (PAGED = false: `page` is the whole sequence, the "page id" is
// the batch index), the paged one looks the tile's page up in the table.  Keys from the first negative or out-of-pool page
// id on are zero K / V rows: score 0, still counted by every softmax, nothing added to the output; such a page is never read.
#include "common.h"

namespace mojo {
namespace {

constexpr int NSA_THREADS = 256;            // fused form; scores and values of the split form
constexpr int NSA_WAVES = NSA_THREADS / 64;
constexpr int NSA_SELECT_THREADS = 1024;    // select launch of the split form
constexpr int NSA_TILE = 16;                // keys per tile
constexpr int NSA_MAX_SEL = 64;             // num_selected_blocks
constexpr int64_t NSA_MAX_BLOCKS = 8192;    // selection blocks of a row (their scores are 32 KiB of LDS)
constexpr int64_t NSA_FUSED_LDS = 56 * 1024;   // dynamic LDS of the fused form, beside ~3 KiB of merge buffers
constexpr int64_t NSA_CUS = 256;
constexpr int64_t NSA_MIN_SLICE_TILES = 16; // a planned slice walks at least 256 keys
constexpr float NSA_LOG2E = 1.4426950408889634f;

struct NsaArgs {
  const void* q; const void* k; const void* v; const void* gate; const int* lens; const int* tables; void* out;
  float* rows; float* groups; float* partials; int* ends;                 // workspace (split form)
  int heads, dim, n_blocks, page, cap, cr, bs, nsel, ws, gate_f32, ns;
  int row_stride, group_stride;                                           // floats of a (b, h) row / group array
  int64_t table_stride, blk_stride, head_stride, tok_stride;
  float scale;
};

struct NsaShared {
  float red[2][NSA_SELECT_THREADS / 64];
  int red_i[NSA_SELECT_THREADS / 64];
  int sel[NSA_MAX_SEL];
  float gate[3];
};

__device__ __forceinline__ int nsa_len(const NsaArgs& a, int b) {
  const int sl = a.lens ? a.lens[b] : a.cap;
  return sl < 0 ? 0 : (sl > a.cap ? a.cap : sl);
}

__device__ __forceinline__ int nsa_wave() { return __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)); }

// element offset of the first key row of the tile at key t0 (a multiple of 16) for head h, -1 for a page that is not there
template <bool PAGED>
__device__ __forceinline__ int64_t nsa_tile_base(const NsaArgs& a, int b, int h, int t0) {
  if constexpr (PAGED) {
    const int pi = t0 / a.page;                                           // < table width: t0 < cap = page * width
    const int id = a.tables[b * a.table_stride + pi];
    if (id < 0 || id >= a.n_blocks) return -1;
    return id * a.blk_stride + h * a.head_stride + (t0 - pi * a.page) * a.tok_stride;
  } else {
    return b * a.blk_stride + h * a.head_stride + t0 * a.tok_stride;
  }
}

template <int LPK>
__device__ __forceinline__ float nsa_key_sum(float x) {
  if constexpr (LPK == 16) return row16_sum(x); else return row8_sum(x);
}

// The U vectors a lane holds of one tile: key t0 + u * KPW + sub, elements [8 * chunk, 8 * chunk + 8); zeros past `end`
// and for a page that is not there.
template <typename T, int D, bool PAGED>
struct NsaTile {
  static constexpr int LPK = D / 8, KPW = 64 / LPK, U = NSA_TILE / KPW;
  typename vec_of<T, 8>::type x[U];
  __device__ __forceinline__ void load(const NsaArgs& a, const T* src, int b, int h, int t0, int end, int sub, int chunk) {
    const int64_t base = nsa_tile_base<PAGED>(a, b, h, t0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = u * KPW + sub;
      if (base >= 0 && t0 + r < end) {
        x[u] = load_vec<T, 8>(src + base + r * a.tok_stride + chunk * 8);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[u][e] = elt<T>::from_f(0.f);
      }
    }
  }
};

// ---- phase 1: s_t = scale * q . k_t for the keys of tiles [tile0, tile1), tile `wave` of every NSA_WAVES -----------------------
template <typename T, int D, bool PAGED>
__device__ __forceinline__ void nsa_scores(const NsaArgs& a, int b, int h, int sl, int tile0, int tile1, float* row) {
  typedef NsaTile<T, D, PAGED> Tile;
  const int lane = threadIdx.x & 63, wave = nsa_wave();
  const int sub = lane / Tile::LPK, chunk = lane % Tile::LPK;
  const T* kp = static_cast<const T*>(a.k);
  float q[8];
  {
    const auto qv = load_vec<T, 8>(static_cast<const T*>(a.q) + (static_cast<int64_t>(b) * a.heads + h) * D + chunk * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = elt<T>::to_f(qv[e]);
  }
  auto finish = [&](const Tile& tile, int t0) {
#pragma unroll
    for (int u = 0; u < Tile::U; ++u) {
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) dot = fmaf(q[e], elt<T>::to_f(tile.x[u][e]), dot);
      dot = nsa_key_sum<Tile::LPK>(dot) * a.scale;
      const int t = t0 + u * Tile::KPW + sub;
      if (chunk == 0 && t < sl) row[t] = dot;
    }
  };
  for (int tile = tile0 + wave; tile < tile1; tile += 2 * NSA_WAVES) {
    Tile t_a, t_b;
    const int second = tile + NSA_WAVES;
    t_a.load(a, kp, b, h, tile * NSA_TILE, sl, sub, chunk);
    if (second < tile1) t_b.load(a, kp, b, h, second * NSA_TILE, sl, sub, chunk);
    finish(t_a, tile * NSA_TILE);
    if (second < tile1) finish(t_b, second * NSA_TILE);
  }
}

// ---- phase 3: acc[e] = sum_t w_t v_t[8 * chunk + e] over this lane's keys of tiles [tile0, tile1), t < end ------------------------
template <typename T, int D, bool PAGED>
__device__ __forceinline__ void nsa_values(const NsaArgs& a, int b, int h, int end, int tile0, int tile1, const float* row,
                                           float (&acc)[8]) {
  typedef NsaTile<T, D, PAGED> Tile;
  const int lane = threadIdx.x & 63, wave = nsa_wave();
  const int sub = lane / Tile::LPK, chunk = lane % Tile::LPK;
  const T* vp = static_cast<const T*>(a.v);
  auto finish = [&](const Tile& tile, int t0) {
#pragma unroll
    for (int u = 0; u < Tile::U; ++u) {
      const int t = t0 + u * Tile::KPW + sub;
      const float w = t < end ? row[t] : 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(w, elt<T>::to_f(tile.x[u][e]), acc[e]);
    }
  };
  for (int tile = tile0 + wave; tile < tile1; tile += 2 * NSA_WAVES) {
    Tile t_a, t_b;
    const int second = tile + NSA_WAVES;
    t_a.load(a, vp, b, h, tile * NSA_TILE, end, sub, chunk);
    if (second < tile1) t_b.load(a, vp, b, h, second * NSA_TILE, end, sub, chunk);
    finish(t_a, tile * NSA_TILE);
    if (second < tile1) finish(t_b, second * NSA_TILE);
  }
}

// The lanes of one D-chunk by shuffles, then the waves through `merge` [NSA_WAVES][D]; thread d < D returns element d.
template <int D>
__device__ __forceinline__ float nsa_merge_waves(float (&acc)[8], float (*merge)[D]) {
  constexpr int LPK = D / 8;
  const int lane = threadIdx.x & 63, wave = nsa_wave();
#pragma unroll
  for (int m = LPK; m < 64; m <<= 1) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], m);
  }
  if (lane < LPK) {
#pragma unroll
    for (int e = 0; e < 8; ++e) merge[wave][lane * 8 + e] = acc[e];
  }
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x < D) {
#pragma unroll
    for (int w = 0; w < NSA_WAVES; ++w) r += merge[w][threadIdx.x];
  }
  return r;
}

// ---- phase 2 ----------------------------------------------------------------------------------------------------------------------
struct NsaMax { __device__ __forceinline__ float operator()(float x, float y) const { return fmaxf(x, y); } };
struct NsaSum { __device__ __forceinline__ float operator()(float x, float y) const { return x + y; } };

// two block-wide reductions at once, in a fixed order; every thread returns with both results
template <int NT, typename Op>
__device__ __forceinline__ void nsa_reduce2(float& x, float& y, NsaShared& sh, Op op) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    x = op(x, __shfl_xor(x, m));
    y = op(y, __shfl_xor(y, m));
  }
  __syncthreads();                                   // (the previous results have been read)
  if ((threadIdx.x & 63) == 0) { sh.red[0][threadIdx.x >> 6] = x; sh.red[1][threadIdx.x >> 6] = y; }
  __syncthreads();
  x = sh.red[0][0]; y = sh.red[1][0];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) { x = op(x, sh.red[0][i]); y = op(y, sh.red[1][i]); }
}

// Turns the scores of `row` [0, sl) into the weights w_t and returns the number of keys that have a V row (sl, or the first
// key of the first page that is not there).  `groups`: ceil(sl / cr) floats, `bscore`: ceil(sl / bs) floats (LDS).
// Called by all NT threads of the block, after a barrier behind the last score; ends with a barrier.
template <typename T, bool PAGED, int NT>
__device__ __forceinline__ int nsa_select(const NsaArgs& a, int b, int h, int sl, float* row, float* groups, float* bscore,
                                          NsaShared& sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = nsa_wave();
  const int cr = a.cr, bs = a.bs;
  const int n_groups = sl / cr, gpb = bs / cr, nb = (sl + bs - 1) / bs;
  const int n_sel = a.nsel < nb ? a.nsel : nb;
  const int win0 = sl > a.ws ? sl - a.ws : 0;
  const float inv_cr = 1.0f / static_cast<float>(cr);

  // keys with a V row
  int end = sl;
  if constexpr (PAGED) {
    const int n_pages = (sl + a.page - 1) / a.page;
    int first = n_pages;
    for (int j = tid; j < n_pages; j += NT) {
      const int id = a.tables[b * a.table_stride + j];
      if ((id < 0 || id >= a.n_blocks) && j < first) first = j;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(first, m); first = o < first ? o : first; }
    if (lane == 0) sh.red_i[wave] = first;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) first = sh.red_i[i] < first ? sh.red_i[i] : first;
    const int64_t keys = static_cast<int64_t>(first) * a.page;
    if (keys < sl) end = static_cast<int>(keys);
    for (int t = end + tid; t < sl; t += NT) row[t] = 0.f;              // (pages behind the first hole may have been read)
  }
  // the gate, by the last wave
  if (wave == NT / 64 - 1) {
    const T* qp = static_cast<const T*>(a.q) + (static_cast<int64_t>(b) * a.heads + h) * a.dim;
    float g[3] = {0.f, 0.f, 0.f};
    for (int d = lane; d < a.dim; d += 64) {
      const float qd = elt<T>::to_f(qp[d]);
      const int64_t at = (static_cast<int64_t>(h) * a.dim + d) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        g[c] = fmaf(qd, a.gate_f32 ? static_cast<const float*>(a.gate)[at + c] : elt<T>::to_f(static_cast<const T*>(a.gate)[at + c]), g[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) g[c] += __shfl_xor(g[c], m);
      if (lane == 0) sh.gate[c] = __builtin_amdgcn_rcpf(1.0f + fast_exp2(-g[c] * NSA_LOG2E));
    }
  }
  __syncthreads();

  // compressed branch: group scores, their softmax (unnormalised in `groups`), block scores
  float m_c = -3.0e38f, unused = 0.f;
  for (int j = tid; j < n_groups; j += NT) {
    float c = 0.f;
    for (int i = 0; i < cr; ++i) c += row[j * cr + i];
    c *= inv_cr;
    groups[j] = c;
    m_c = fmaxf(m_c, c);
  }
  nsa_reduce2<NT>(m_c, unused, sh, NsaMax());
  float l_c = 0.f;
  for (int j = tid; j < n_groups; j += NT) {
    const float e = fast_exp2((groups[j] - m_c) * NSA_LOG2E);
    groups[j] = e;
    l_c += e;
  }
  nsa_reduce2<NT>(l_c, unused, sh, NsaSum());                           // (its barriers publish `groups`)
  for (int blk = tid; blk < nb; blk += NT) {
    const int j1 = (blk + 1) * gpb < n_groups ? (blk + 1) * gpb : n_groups;
    float s = 0.f;
    for (int j = blk * gpb; j < j1; ++j) s += groups[j];
    bscore[blk] = s;                                                    // >= 0; a taken block becomes -1
  }
  __syncthreads();

  // selection: n_sel rounds of arg-max in wave 0, the lower index among equals
  if (wave == 0) {
    for (int r = 0; r < n_sel; ++r) {
      float best = -2.f;
      int at = 0x7fffffff;
      for (int blk = lane; blk < nb; blk += 64) {
        const float s = bscore[blk];
        if (s > best) { best = s; at = blk; }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const float o = __shfl_xor(best, m);
        const int oi = __shfl_xor(at, m);
        if (o > best || (o == best && oi < at)) { best = o; at = oi; }
      }
      if ((at & 63) == lane) bscore[at] = -1.f;                         // by the lane that reads it in the next round
      if (lane == 0) sh.sel[r] = at;
    }
  }
  __syncthreads();

  // maxima and sums of the selected and the window softmax
  const int sel_keys = n_sel * bs;
  float m_s = -3.0e38f, m_w = -3.0e38f;
  for (int i = tid; i < sel_keys; i += NT) {
    const int r = i / bs, t = sh.sel[r] * bs + (i - r * bs);
    if (t < sl) m_s = fmaxf(m_s, row[t]);
  }
  for (int t = win0 + tid; t < sl; t += NT) m_w = fmaxf(m_w, row[t]);
  nsa_reduce2<NT>(m_s, m_w, sh, NsaMax());
  float l_s = 0.f, l_w = 0.f;
  for (int i = tid; i < sel_keys; i += NT) {
    const int r = i / bs, t = sh.sel[r] * bs + (i - r * bs);
    if (t < sl) l_s += fast_exp2((row[t] - m_s) * NSA_LOG2E);
  }
  for (int t = win0 + tid; t < sl; t += NT) l_w += fast_exp2((row[t] - m_w) * NSA_LOG2E);
  nsa_reduce2<NT>(l_s, l_w, sh, NsaSum());

  // one weight per key, group by group (a group lies in one block: bs % cr == 0)
  const float f_c = l_c > 0.f ? sh.gate[0] * inv_cr / l_c : 0.f;
  const float f_s = l_s > 0.f ? sh.gate[1] / l_s : 0.f;
  const float f_w = l_w > 0.f ? sh.gate[2] / l_w : 0.f;
  const int n_slots = (sl + cr - 1) / cr;
  for (int j = tid; j < n_slots; j += NT) {
    const float w_c = j < n_groups ? f_c * groups[j] : 0.f;
    const bool chosen = bscore[(j * cr) / bs] < 0.f;
    for (int i = 0; i < cr; ++i) {
      const int t = j * cr + i;
      if (t >= sl) break;
      const float s = row[t];
      float w = w_c;
      if (chosen) w = fmaf(f_s, fast_exp2((s - m_s) * NSA_LOG2E), w);
      if (t >= win0) w = fmaf(f_w, fast_exp2((s - m_w) * NSA_LOG2E), w);
      row[t] = w;
    }
  }
  __syncthreads();
  return end;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------------
template <typename T, int D, bool PAGED>
__global__ __launch_bounds__(NSA_THREADS) void nsa_fused_kernel(NsaArgs a) {
  extern __shared__ float nsa_lds[];
  __shared__ float merge[NSA_WAVES][D];
  __shared__ NsaShared sh;
  float* row = nsa_lds;
  float* groups = row + a.row_stride;
  float* bscore = groups + a.group_stride;
  const int b = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
  T* out = static_cast<T*>(a.out) + static_cast<int64_t>(blockIdx.x) * D;
  const int sl = nsa_len(a, b);
  if (sl <= 0) {
    if (threadIdx.x < D) out[threadIdx.x] = elt<T>::from_f(0.f);
    return;
  }
  nsa_scores<T, D, PAGED>(a, b, h, sl, 0, (sl + NSA_TILE - 1) / NSA_TILE, row);
  __syncthreads();
  const int end = nsa_select<T, PAGED, NSA_THREADS>(a, b, h, sl, row, groups, bscore, sh);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  nsa_values<T, D, PAGED>(a, b, h, end, 0, (end + NSA_TILE - 1) / NSA_TILE, row, acc);
  const float r = nsa_merge_waves<D>(acc, merge);
  if (threadIdx.x < D) out[threadIdx.x] = elt<T>::from_f(r);
}

// tiles [tile0, tile1) of slice blockIdx.y of a row of sl keys: every slice of a row takes the same number of tiles
__device__ __forceinline__ void nsa_slice(const NsaArgs& a, int sl, int& tile0, int& tile1) {
  const int tiles = (sl + NSA_TILE - 1) / NSA_TILE;
  const int per = (tiles + a.ns - 1) / a.ns;
  tile0 = blockIdx.y * per;
  tile1 = tile0 + per < tiles ? tile0 + per : tiles;
}

template <typename T, int D, bool PAGED>
__global__ __launch_bounds__(NSA_THREADS) void nsa_scores_kernel(NsaArgs a) {
  const int b = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
  const int sl = nsa_len(a, b);
  int tile0, tile1;
  nsa_slice(a, sl, tile0, tile1);
  nsa_scores<T, D, PAGED>(a, b, h, sl, tile0, tile1, a.rows + static_cast<int64_t>(blockIdx.x) * a.row_stride);
}

template <typename T, bool PAGED>
__global__ __launch_bounds__(NSA_SELECT_THREADS) void nsa_select_kernel(NsaArgs a) {
  extern __shared__ float nsa_lds[];
  __shared__ NsaShared sh;
  const int b = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
  const int sl = nsa_len(a, b);
  int end = 0;
  if (sl > 0)
    end = nsa_select<T, PAGED, NSA_SELECT_THREADS>(a, b, h, sl, a.rows + static_cast<int64_t>(blockIdx.x) * a.row_stride,
                                                   a.groups + static_cast<int64_t>(blockIdx.x) * a.group_stride, nsa_lds, sh);
  if (threadIdx.x == 0) a.ends[blockIdx.x] = end;
}

template <typename T, int D, bool PAGED>
__global__ __launch_bounds__(NSA_THREADS) void nsa_values_kernel(NsaArgs a) {
  __shared__ float merge[NSA_WAVES][D];
  const int b = blockIdx.x / a.heads, h = blockIdx.x % a.heads;
  const int sl = nsa_len(a, b), end = a.ends[blockIdx.x];
  int tile0, tile1;
  nsa_slice(a, sl, tile0, tile1);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  nsa_values<T, D, PAGED>(a, b, h, end, tile0, tile1, a.rows + static_cast<int64_t>(blockIdx.x) * a.row_stride, acc);
  const float r = nsa_merge_waves<D>(acc, merge);
  if (threadIdx.x < D) a.partials[(static_cast<int64_t>(blockIdx.x) * a.ns + blockIdx.y) * D + threadIdx.x] = r;
}

// the slices' partial outputs in slice order, one rounding
template <typename T>
__global__ void nsa_merge_kernel(NsaArgs a) {
  const float* p = a.partials + static_cast<int64_t>(blockIdx.x) * a.ns * a.dim + threadIdx.x;
  float r = 0.f;
  for (int s = 0; s < a.ns; ++s) r += p[static_cast<int64_t>(s) * a.dim];
  static_cast<T*>(a.out)[static_cast<int64_t>(blockIdx.x) * a.dim + threadIdx.x] = elt<T>::from_f(r);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// What a launch is sized on: the shapes alone, so the workspace query and the entry point plan alike.
struct NsaPlan {
  int status = 0;                   // 0, or the MOJO_E* code the entry point returns
  const char* why = "";
  bool fused = false;
  int ns = 1;
  int64_t row_stride = 0, group_stride = 0, n_blocks_cap = 0, lds = 0;
  int64_t off_groups = 0, off_partials = 0, off_ends = 0, bytes = 0;       // workspace of the split form (floats / bytes)
};

NsaPlan nsa_plan(int64_t batch, int64_t heads, int64_t dim, int64_t cap, int64_t cr, int64_t bs, int64_t num_splits) {
  NsaPlan p;
  auto refuse = [&](int code, const char* why) { p.status = code; p.why = why; return p; };
  if (batch < 0 || heads <= 0 || cap < 0 || cr <= 0 || bs <= 0 || num_splits < 0) return refuse(MOJO_EINVAL, "bad sizes");
  if (dim != 64 && dim != 128) return refuse(MOJO_EUNSUPPORTED, "head_dim 64 and 128 are compiled");
  if (bs % cr != 0) return refuse(MOJO_EUNSUPPORTED, "block_size must be a multiple of compress_ratio");
  if (batch * heads >= (int64_t{1} << 31) || cap >= (int64_t{1} << 30)) return refuse(MOJO_EUNSUPPORTED, "sizes beyond the launch's range");
  p.row_stride = ceil_div(cap, NSA_TILE) * NSA_TILE;
  p.group_stride = ceil_div(ceil_div(cap, cr), 4) * 4;
  p.n_blocks_cap = ceil_div(cap, bs);
  if (p.n_blocks_cap > NSA_MAX_BLOCKS) return refuse(MOJO_EUNSUPPORTED, "more than 8192 selection blocks in a row");
  const int64_t fused_lds = (p.row_stride + p.group_stride + p.n_blocks_cap) * static_cast<int64_t>(sizeof(float));
  const bool fits = fused_lds <= NSA_FUSED_LDS;
  const int64_t tiles = p.row_stride / NSA_TILE > 0 ? p.row_stride / NSA_TILE : 1;
  const int64_t rows = batch * heads;
  if (num_splits == 1) {
    if (!fits) return refuse(MOJO_EUNSUPPORTED, "num_splits = 1: the score row does not fit the fused form's LDS");
    p.fused = true;
  } else if (num_splits > 1) {
    p.ns = static_cast<int>(num_splits < tiles ? num_splits : tiles);
  } else if (fits && rows >= NSA_CUS) {
    p.fused = true;
  } else {
    int64_t ns = rows > 0 ? ceil_div(2 * NSA_CUS, rows) : 1;
    const int64_t most = tiles / NSA_MIN_SLICE_TILES > 0 ? tiles / NSA_MIN_SLICE_TILES : 1;
    p.ns = static_cast<int>(ns < most ? ns : most);
  }
  if (p.ns > 65535) p.ns = 65535;
  if (p.fused) { p.lds = fused_lds; return p; }
  p.lds = p.n_blocks_cap * static_cast<int64_t>(sizeof(float));
  p.off_groups = rows * p.row_stride;
  p.off_partials = p.off_groups + rows * p.group_stride;
  p.off_ends = p.off_partials + rows * p.ns * dim;
  p.bytes = (p.off_ends + rows) * static_cast<int64_t>(sizeof(float)) + 256;
  return p;
}

template <typename T, int D, bool PAGED>
int nsa_launch(NsaArgs& a, const NsaPlan& p, int64_t rows, hipStream_t s) {
  const dim3 grid_rows(static_cast<unsigned>(rows));
  if (p.fused) {
    hipLaunchKernelGGL((nsa_fused_kernel<T, D, PAGED>), grid_rows, dim3(NSA_THREADS), static_cast<size_t>(p.lds), s, a);
    MOJO_CHECK_LAUNCH("nsa_decode");
    note_launch("nsa_decode:fused:d%d", D);
    return 0;
  }
  const dim3 grid_slices(static_cast<unsigned>(rows), static_cast<unsigned>(p.ns));
  hipLaunchKernelGGL((nsa_scores_kernel<T, D, PAGED>), grid_slices, dim3(NSA_THREADS), 0, s, a);
  MOJO_CHECK_LAUNCH("nsa_decode (scores)");
  hipLaunchKernelGGL((nsa_select_kernel<T, PAGED>), grid_rows, dim3(NSA_SELECT_THREADS), static_cast<size_t>(p.lds), s, a);
  MOJO_CHECK_LAUNCH("nsa_decode (select)");
  hipLaunchKernelGGL((nsa_values_kernel<T, D, PAGED>), grid_slices, dim3(NSA_THREADS), 0, s, a);
  MOJO_CHECK_LAUNCH("nsa_decode (values)");
  hipLaunchKernelGGL((nsa_merge_kernel<T>), grid_rows, dim3(D), 0, s, a);
  MOJO_CHECK_LAUNCH("nsa_decode (merge)");
  note_launch("nsa_decode:split%d:d%d", p.ns, D);
  return 0;
}

template <typename T>
int nsa_dispatch(NsaArgs& a, const NsaPlan& p, int64_t rows, bool paged, hipStream_t s) {
  if (a.dim == 64) return paged ? nsa_launch<T, 64, true>(a, p, rows, s) : nsa_launch<T, 64, false>(a, p, rows, s);
  return paged ? nsa_launch<T, 128, true>(a, p, rows, s) : nsa_launch<T, 128, false>(a, p, rows, s);
}

}  // namespace
}  // namespace mojo

using namespace mojo;

extern "C" int64_t mojo_hip_nsa_decode_workspace_bytes(int64_t batch, int64_t heads, int64_t head_dim, int64_t kv_capacity,
                                                       int64_t compress_ratio, int64_t block_size, int64_t num_splits) {
  const NsaPlan p = nsa_plan(batch, heads, head_dim, kv_capacity, compress_ratio, block_size, num_splits);
  return p.status != 0 ? -1 : p.bytes;
}

extern "C" int mojo_hip_nsa_decode(const void* query, const void* key, const void* value, const void* gate_proj,
                                   const int32_t* total_seq_lens, const int32_t* block_tables, void* out, void* workspace,
                                   int64_t workspace_bytes, int64_t batch, int64_t heads, int64_t head_dim, int64_t num_blocks,
                                   int64_t page, int64_t max_pages, int64_t table_stride, int64_t kv_block_stride,
                                   int64_t kv_head_stride, int64_t kv_token_stride, int64_t compress_ratio, int64_t block_size,
                                   int64_t num_selected_blocks, int64_t window_size, float softmax_scale, int dtype,
                                   int gate_dtype, int64_t num_splits, mojo_stream_t stream) {
  const char* what = "nsa_decode";
  const bool paged = block_tables != nullptr;
  MOJO_REQUIRE(page > 0 && max_pages >= 0 && num_selected_blocks >= 0 && window_size >= 0, MOJO_EINVAL, "%s: bad sizes", what);
  MOJO_REQUIRE(dtype == MOJO_BF16 || dtype == MOJO_F16, MOJO_EUNSUPPORTED, "%s: bf16 and fp16 only", what);
  MOJO_REQUIRE(gate_dtype == dtype || gate_dtype == MOJO_F32, MOJO_EUNSUPPORTED, "%s: gate_proj in the query's dtype or fp32", what);
  MOJO_REQUIRE(num_selected_blocks <= NSA_MAX_SEL, MOJO_EUNSUPPORTED, "%s: num_selected_blocks %lld (at most %d)", what,
               (long long)num_selected_blocks, NSA_MAX_SEL);
  MOJO_REQUIRE(!paged || (page % 16 == 0 && page <= 256), MOJO_EUNSUPPORTED, "%s: page %lld (a multiple of 16, at most 256)", what,
               (long long)page);
  MOJO_REQUIRE(kv_block_stride % 8 == 0 && kv_head_stride % 8 == 0 && kv_token_stride % 8 == 0 && kv_token_stride >= head_dim,
               MOJO_EUNSUPPORTED, "%s: K/V strides must be multiples of 16 bytes", what);
  MOJO_REQUIRE(paged ? (num_blocks >= 0 && num_blocks < (int64_t{1} << 31) && max_pages < (int64_t{1} << 31) / 256) : max_pages == 1,
               MOJO_EINVAL, "%s: bad page pool (contiguous K/V: one page per sequence)", what);
  const int64_t cap = page * max_pages;
  const NsaPlan p = nsa_plan(batch, heads, head_dim, cap, compress_ratio, block_size, num_splits);
  MOJO_REQUIRE(p.status == 0, p.status, "%s: %s", what, p.why);
  const int64_t rows = batch * heads;
  if (rows == 0) return 0;
  MOJO_REQUIRE(query && gate_proj && out && (cap == 0 || (key && value)), MOJO_EINVAL, "%s: null pointer", what);
  MOJO_REQUIRE(aligned_to(query, 16) && aligned_to(key, 16) && aligned_to(value, 16), MOJO_EINVAL,
               "%s: query, key and value must be 16-byte aligned", what);
  NsaArgs a;
  a.q = query; a.k = key; a.v = value; a.gate = gate_proj; a.lens = total_seq_lens; a.tables = block_tables; a.out = out;
  a.rows = a.groups = a.partials = nullptr; a.ends = nullptr;
  if (!p.fused) {
    MOJO_REQUIRE(workspace && workspace_bytes >= p.bytes, MOJO_EWORKSPACE, "%s: the split form needs %lld workspace bytes, got %lld",
                 what, (long long)p.bytes, (long long)workspace_bytes);
    float* base = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
    a.rows = base; a.groups = base + p.off_groups; a.partials = base + p.off_partials;
    a.ends = reinterpret_cast<int*>(base + p.off_ends);
  }
  a.heads = static_cast<int>(heads); a.dim = static_cast<int>(head_dim); a.n_blocks = static_cast<int>(num_blocks);
  a.page = static_cast<int>(page); a.cap = static_cast<int>(cap); a.cr = static_cast<int>(compress_ratio);
  a.bs = static_cast<int>(block_size); a.nsel = static_cast<int>(num_selected_blocks);
  a.ws = static_cast<int>(window_size < cap ? window_size : cap); a.gate_f32 = gate_dtype == MOJO_F32 ? 1 : 0; a.ns = p.ns;
  a.row_stride = static_cast<int>(p.row_stride); a.group_stride = static_cast<int>(p.group_stride);
  a.table_stride = table_stride; a.blk_stride = kv_block_stride; a.head_stride = kv_head_stride; a.tok_stride = kv_token_stride;
  a.scale = softmax_scale;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dtype == MOJO_BF16 ? nsa_dispatch<bf16_t>(a, p, rows, paged, s) : nsa_dispatch<f16_t>(a, p, rows, paged, s);
}
