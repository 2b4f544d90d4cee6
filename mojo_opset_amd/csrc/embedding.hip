// The input-embedding ops (EMBEDDING_OPS): token ids to hidden states.
//
//   mojo_hip_embedding             out[t] = table[ids[t] - vocab_start], a row of zeros when that index is outside [0, rows)
//   mojo_hip_nf4_embedding         the same lookup in a packed-NF4 table, dequantised on the fly
//   mojo_hip_oe_ngram              the n-gram ids of the over-encoding layer
//   mojo_hip_over_encoding_concat  ids, the original table's row and the G mega rows of every token in ONE launch, written
//                                  straight into the concatenation the up projection reads
//
// Everything here is integer arithmetic and copies, except the NF4 value fp32(codebook[nibble]) * fp32(scale) + fp32(mean): the
// product and the sum are rounded on their own (__fmul_rn / __fadd_rn: the unit is built with -ffp-contract=on, and a fused
// multiply-add changes one fp32 result in seven), and the codebook is the reference's fp16 tensor, read from the module.
//
// An index out of range never reads out of bounds and never traps: it selects a row of zeros.  Every id is read on the device
// (no host synchronisation; the launches can be captured in a graph).
//
// Work items.  A row is cut into items of 16 bytes (dense tables) or 8 elements (NF4: one 32-bit word of nibbles) when sizes,
// strides and base pointers allow it, and into single elements otherwise.  The item bodies below are shared by the row
// kernels and by the fused concatenation, which maps a flat item index of the wide row to (segment, column).
#include "common.h"

namespace mojo {

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;            // 8 resident blocks of 256 on each of 256 CUs: kernels with a per-block prologue walk a grid stride

__device__ __forceinline__ int64_t load_index(const void* p, bool is_i64, int64_t i) {
  return is_i64 ? static_cast<const int64_t*>(p)[i] : static_cast<int64_t>(static_cast<const int32_t*>(p)[i]);
}

// local row of an id, or -1 when it lies outside the table
__device__ __forceinline__ int64_t local_row(int64_t id, int64_t vocab_start, int64_t rows) {
  // (the subtraction in unsigned arithmetic: an id near the ends of int64 wraps instead of overflowing, and then fails the test)
  const int64_t r = static_cast<int64_t>(static_cast<uint64_t>(id) - static_cast<uint64_t>(vocab_start));
  return (r >= 0 && r < rows) ? r : -1;
}

// ---- item bodies ------------------------------------------------------------------------------------------------------
// `total` 16-byte items walked by the whole block, four loads in flight per thread before the first store; `map(w, src, dst)`
// names item w's source (nullptr: zeros) and destination
template <typename MAP>
__device__ __forceinline__ void copy_items16(int64_t first, int64_t total, int64_t step, MAP map) {
  for (int64_t w = first; w < total; w += 4 * step) {
    u32x4 v[4];
    char* d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t wi = w + u * step;
      v[u] = u32x4{0u, 0u, 0u, 0u};
      d[u] = nullptr;
      if (wi < total) {
        const char* src = nullptr;
        map(wi, src, d[u]);
        if (src) v[u] = *reinterpret_cast<const u32x4*>(src);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (d[u]) *reinterpret_cast<u32x4*>(d[u]) = v[u];
  }
}

// one element of `esize` (2 or 4) bytes
__device__ __forceinline__ void copy_elem(const char* src, char* dst, int esize) {
  if (esize == 4) {
    *reinterpret_cast<uint32_t*>(dst) = src ? *reinterpret_cast<const uint32_t*>(src) : 0u;
  } else {
    *reinterpret_cast<uint16_t*>(dst) = src ? *reinterpret_cast<const uint16_t*>(src) : static_cast<uint16_t>(0);
  }
}

__device__ __forceinline__ float load_coded(const void* p, int code, int64_t i) {
  if (code == MOJO_F32) return static_cast<const float*>(p)[i];
  if (code == MOJO_F16) return static_cast<float>(static_cast<const f16_t*>(p)[i]);
  return static_cast<float>(static_cast<const bf16_t*>(p)[i]);
}

// A row of a packed-NF4 table: nibbles, and its scale / mean rows ([dim / group_size], dtype by code)
struct Nf4Row {
  const uint8_t* q;            // nullptr: the row of zeros
  const void* scale;
  const void* mean;
  int64_t group_base;          // first entry of the row in scale / mean
};

__device__ __forceinline__ float nf4_value(const float* cb, unsigned nibble, float s, float m) {
  return __fadd_rn(__fmul_rn(cb[nibble], s), m);
}

// element `col` of the row
template <typename TO>
__device__ __forceinline__ void nf4_elem(const Nf4Row& r, int col, int group_size, int sm_code, const float* cb, TO* dst) {
  if (!r.q) {
    *dst = elt<TO>::from_f(0.f);
    return;
  }
  const unsigned byte = r.q[col >> 1];
  const unsigned nib = (col & 1) ? (byte >> 4) : (byte & 15u);
  const int64_t g = r.group_base + col / group_size;
  *dst = elt<TO>::from_f(nf4_value(cb, nib, load_coded(r.scale, sm_code, g), load_coded(r.mean, sm_code, g)));
}

// elements [col, col + 8), col a multiple of 8: one aligned 32-bit word of nibbles, 16-byte stores
template <typename TO>
__device__ __forceinline__ void nf4_item8(const Nf4Row& r, int col, int group_size, int sm_code, const float* cb, TO* dst) {
  float v[8];
  if (!r.q) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
  } else {
    const uint32_t word = *reinterpret_cast<const uint32_t*>(r.q + (col >> 1));
    if (group_size % 8 == 0) {                                     // the 8 elements share one group
      const int64_t g = r.group_base + col / group_size;
      const float s = load_coded(r.scale, sm_code, g), m = load_coded(r.mean, sm_code, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = nf4_value(cb, (word >> (4 * e)) & 15u, s, m);
    } else {                                                       // the group per element (odd sizes and 1 included)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t g = r.group_base + (col + e) / group_size;
        v[e] = nf4_value(cb, (word >> (4 * e)) & 15u, load_coded(r.scale, sm_code, g), load_coded(r.mean, sm_code, g));
      }
    }
  }
  if constexpr (sizeof(TO) == 4) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
  } else {
    typename vec_of<TO, 8>::type o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = elt<TO>::from_f(v[e]);
    store_vec<TO, 8>(dst, o);
  }
}

// the reference's fp16 codebook, widened once per block
__device__ __forceinline__ void load_codebook(const f16_t* codebook, float* cb) {
  if (threadIdx.x < 16) cb[threadIdx.x] = static_cast<float>(codebook[threadIdx.x]);
  __syncthreads();
}

// ---- the sequence of a packed token -----------------------------------------------------------------------------------
// q_lens [B] lives on the device.  A block cuts it into 256 chunks, keeps the exclusive prefix sums of the chunk totals in LDS
// and finds a token's sequence by a binary search over them and a walk inside one chunk.  Negative lengths read as zero.
struct SeqFinder {
  int64_t part[kBlock + 1];
  int64_t wave_total[kBlock / 64];
};

__device__ __forceinline__ int64_t q_len_at(const void* q_lens, bool is_i64, int64_t b) {
  const int64_t n = load_index(q_lens, is_i64, b);
  return n > 0 ? n : 0;
}

__device__ __forceinline__ void seq_finder_init(SeqFinder& f, const void* q_lens, bool is_i64, int64_t batch) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t chunk = (batch + kBlock - 1) / kBlock;
  int64_t sum = 0;
  for (int64_t b = tid * chunk; b < (tid + 1) * chunk && b < batch; ++b) sum += q_len_at(q_lens, is_i64, b);
  long long scan = sum;                                            // inclusive scan over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long up = __shfl_up(scan, d);
    if (lane >= d) scan += up;
  }
  if (lane == 63) f.wave_total[wave] = scan;
  if (tid == 0) f.part[0] = 0;
  __syncthreads();
  int64_t before = 0;
  for (int w = 0; w < wave; ++w) before += f.wave_total[w];
  f.part[tid + 1] = before + scan;
  __syncthreads();
}

// sequence and position of packed token t; false when t lies at or past sum(q_lens)
__device__ __forceinline__ bool seq_find(const SeqFinder& f, const void* q_lens, bool is_i64, int64_t batch, int64_t t,
                                         int64_t& seq, int64_t& pos) {
  if (t >= f.part[kBlock]) return false;
  int lo = 0, hi = kBlock;                                         // part[lo] <= t < part[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (f.part[mid] <= t) lo = mid; else hi = mid;
  }
  const int64_t chunk = (batch + kBlock - 1) / kBlock;
  int64_t run = f.part[lo];
  if (chunk == 1) {                                                // up to 256 sequences: the chunk is the sequence
    seq = lo;
    pos = t - run;
    return true;
  }
  for (int64_t b = lo * chunk; b < (lo + 1) * chunk && b < batch; ++b) {
    const int64_t n = q_len_at(q_lens, is_i64, b);
    if (t < run + n) {
      seq = b;
      pos = t - run;
      return true;
    }
    run += n;
  }
  return false;
}

// ---- the n-gram id ----------------------------------------------------------------------------------------------------
constexpr int kIdsI64 = 1, kHistI64 = 2, kQLensI64 = 4, kSizesI64 = 8, kGramsI64 = 16, kOffsetsI64 = 32;

struct NgramArgs {
  const void* ids;             // [tokens] (packed) or [batch][seq_len] dense
  const void* history;         // [batch][hist_len] by hist_stride
  const void* q_lens;          // [batch]; unused in the batched form
  const void* sizes;           // [G]
  const void* grams;           // [G]
  const void* offsets;         // [G]
  int64_t tokens, batch, seq_len /* 0: packed */, hist_len, hist_stride, ori_vocab;
  int num_grams, max_gram, flags;
};

// torch's `%` on integers: the result takes the sign of the divisor
__device__ __forceinline__ int64_t floor_mod(int64_t a, int64_t v) {
  if (v == 0) return a;
  if (v == -1) return 0;
  int64_t r = a % v;
  if (r != 0 && ((r < 0) != (v < 0))) r += v;
  return r;
}

// products and sums wrap in 64 bits, as the reference's int64 tensors do
__device__ __forceinline__ int64_t wrap_mul(int64_t a, int64_t b) {
  return static_cast<int64_t>(static_cast<uint64_t>(a) * static_cast<uint64_t>(b));
}
__device__ __forceinline__ int64_t wrap_add(int64_t a, int64_t b) {
  return static_cast<int64_t>(static_cast<uint64_t>(a) + static_cast<uint64_t>(b));
}

// x mod v for 0 <= x < 2^63 and v > 0 by one multiply-high with m = floor((2^64 - 1) / v): q = floor(x * m / 2^64) lies at most 2
// below floor(x / v), so the remainder is corrected by at most two subtractions.  The compiler's 64-bit `%` is a subroutine of
// about a hundred instructions, and a gram of 7 chains twelve of them.
__device__ __forceinline__ uint64_t barrett_mod(uint64_t x, uint64_t v, uint64_t m) {
  uint64_t r = x - __umul64hi(x, m) * v;
  while (r >= v) r -= v;
  return r;
}

// id of flat token t = (seq, pos) in vocabulary g.  A predecessor before the sequence start is the history row read from its
// end; one before the start of the history reads as 0 (the host refuses a history shorter than max gram - 1).  While id, the
// predecessor and the carry are all in [0, 2^31) — every real vocabulary — the sum id + p * carry stays below 2^63 and takes the
// multiply-high reduction; anything else (negative ids, sizes past 2^31, a size <= 0) takes the exact wrapping form.
__device__ __forceinline__ int64_t ngram_prev(const NgramArgs& a, int64_t t, int64_t seq, int64_t pos, int64_t i) {
  if (pos - i >= 0) return load_index(a.ids, a.flags & kIdsI64, t - i);
  if (a.hist_len + pos - i >= 0) return load_index(a.history, a.flags & kHistI64, seq * a.hist_stride + a.hist_len + pos - i);
  return 0;
}

__device__ __forceinline__ void ngram_step(int64_t& id, int64_t& carry, int64_t prev, int64_t v, uint64_t m, int64_t ori_vocab) {
  if (v > 0 && static_cast<uint64_t>(id | prev | carry | ori_vocab) < (uint64_t{1} << 31)) {
    id = static_cast<int64_t>(barrett_mod(static_cast<uint64_t>(id) + static_cast<uint64_t>(prev) * static_cast<uint64_t>(carry),
                                          static_cast<uint64_t>(v), m));
    carry = static_cast<int64_t>(barrett_mod(static_cast<uint64_t>(carry) * static_cast<uint64_t>(ori_vocab),
                                             static_cast<uint64_t>(v), m));
  } else {
    id = floor_mod(wrap_add(id, wrap_mul(prev, carry)), v);
    carry = floor_mod(wrap_mul(carry, ori_vocab), v);
  }
}

// The first kPreload predecessors are loaded before the chain starts: they do not depend on it, and a load inside the loop
// would put one memory latency into every step.
constexpr int kPreload = 8;

__device__ __forceinline__ int64_t ngram_id(const NgramArgs& a, int64_t t, int64_t seq, int64_t pos, int g) {
  const int64_t v = load_index(a.sizes, a.flags & kSizesI64, g);
  int64_t n = load_index(a.grams, a.flags & kGramsI64, g);
  const int64_t offset = load_index(a.offsets, a.flags & kOffsetsI64, g);
  int64_t id = load_index(a.ids, a.flags & kIdsI64, t);
  int64_t prevs[kPreload];
#pragma unroll
  for (int i = 1; i <= kPreload; ++i) prevs[i - 1] = i < a.max_gram ? ngram_prev(a, t, seq, pos, i) : 0;
  if (n > a.max_gram) n = a.max_gram;
  int64_t carry = a.ori_vocab;
  const uint64_t m = (n > 1 && v > 0) ? ~uint64_t{0} / static_cast<uint64_t>(v) : 0;
#pragma unroll
  for (int i = 1; i <= kPreload; ++i)
    if (i < n) ngram_step(id, carry, prevs[i - 1], v, m, a.ori_vocab);
  for (int64_t i = kPreload + 1; i < n; ++i) ngram_step(id, carry, ngram_prev(a, t, seq, pos, i), v, m, a.ori_vocab);
  return wrap_add(id, offset);
}

// (seq, pos) of flat token t in either form
__device__ __forceinline__ bool locate(const NgramArgs& a, const SeqFinder& f, int64_t t, int64_t& seq, int64_t& pos) {
  if (a.seq_len > 0) {
    seq = t / a.seq_len;
    pos = t - seq * a.seq_len;
    return seq < a.batch;
  }
  return seq_find(f, a.q_lens, a.flags & kQLensI64, a.batch, t, seq, pos);
}

// ---- kernels ----------------------------------------------------------------------------------------------------------
// `lanes` threads walk one row; a block holds kBlock / lanes rows.
template <bool VEC16>
__global__ __launch_bounds__(kBlock) void embedding_kernel(const void* __restrict__ ids, int ids_i64,
                                                           const char* __restrict__ table, char* __restrict__ out,
                                                           int64_t tokens, int64_t rows, int64_t row_bytes, int64_t vocab_start,
                                                           int64_t table_stride_bytes, int64_t out_stride_bytes, int esize,
                                                           int lanes) {
  const int lane = threadIdx.x % lanes, sub = threadIdx.x / lanes, per_block = kBlock / lanes;
  const int64_t items = VEC16 ? row_bytes >> 4 : row_bytes / esize;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * per_block + sub; t < tokens;
       t += static_cast<int64_t>(gridDim.x) * per_block) {
    const int64_t r = local_row(load_index(ids, ids_i64, t), vocab_start, rows);
    const char* src = r < 0 ? nullptr : table + r * table_stride_bytes;
    char* dst = out + t * out_stride_bytes;
    if constexpr (VEC16) {
      copy_items16(lane, items, lanes, [&](int64_t i, const char*& s, char*& d) {
        s = src ? src + (i << 4) : nullptr;
        d = dst + (i << 4);
      });
    } else {
      for (int64_t i = lane; i < items; i += lanes) copy_elem(src ? src + i * esize : nullptr, dst + i * esize, esize);
    }
  }
}

template <typename TO, bool VEC8>
__global__ __launch_bounds__(kBlock) void nf4_embedding_kernel(const void* __restrict__ ids, int ids_i64,
                                                               const uint8_t* __restrict__ qweight,
                                                               const void* __restrict__ scale, const void* __restrict__ mean,
                                                               const f16_t* __restrict__ codebook, TO* __restrict__ out,
                                                               int64_t tokens, int64_t rows, int dim, int group_size,
                                                               int64_t vocab_start, int64_t out_stride, int sm_code, int lanes) {
  __shared__ float cb[16];
  load_codebook(codebook, cb);
  const int lane = threadIdx.x % lanes, sub = threadIdx.x / lanes, per_block = kBlock / lanes;
  const int groups = dim / group_size;
  const int items = VEC8 ? dim >> 3 : dim;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * per_block + sub; t < tokens;
       t += static_cast<int64_t>(gridDim.x) * per_block) {
    const int64_t r = local_row(load_index(ids, ids_i64, t), vocab_start, rows);
    const Nf4Row row = {r < 0 ? nullptr : qweight + r * (dim >> 1), scale, mean, r < 0 ? 0 : r * groups};
    TO* dst = out + t * out_stride;
    for (int i = lane; i < items; i += lanes) {
      if constexpr (VEC8) nf4_item8<TO>(row, i << 3, group_size, sm_code, cb, dst + (i << 3));
      else nf4_elem<TO>(row, i, group_size, sm_code, cb, dst + i);
    }
  }
}

// one thread per (token, vocabulary)
__global__ __launch_bounds__(kBlock) void oe_ngram_kernel(NgramArgs a, void* __restrict__ out) {
  __shared__ SeqFinder finder;
  if (a.seq_len == 0) seq_finder_init(finder, a.q_lens, a.flags & kQLensI64, a.batch);
  const int64_t total = a.tokens * a.num_grams;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; idx < total;
       idx += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t t = idx / a.num_grams;
    const int g = static_cast<int>(idx - t * a.num_grams);
    int64_t seq = 0, pos = 0, id = 0;                              // a token no sequence owns: 0
    if (locate(a, finder, t, seq, pos)) id = ngram_id(a, t, seq, pos, g);
    if (a.flags & kIdsI64) static_cast<int64_t*>(out)[idx] = id;
    else static_cast<int32_t*>(out)[idx] = static_cast<int32_t>(id);
  }
}

struct ConcatArgs {
  const char* ori_table;       // [ori_rows][ori_dim] by ori_stride_bytes
  const char* mega_table;      // dense: [mega_rows][mega_dim] by mega_stride_bytes; NF4: [mega_rows][mega_dim / 2] bytes
  const void* mega_scale;      // NF4: [mega_rows][mega_dim / group_size]
  const void* mega_mean;
  const f16_t* codebook;
  int64_t ori_rows, ori_stride_bytes, mega_rows, mega_stride_bytes, mega_vocab_start, out_stride;
  int ori_dim, mega_dim, group_size, sm_code;
};

// A block walks `tok_per_pass` tokens at a time (the id chain of a gram of 7 is microseconds of dependent work: it is paid once
// per pass, not once per token).  (a) one thread per (token, vocabulary) computes the n-gram id — never written to memory; (b)
// meanwhile every thread copies items of the original rows, which need the token alone; (c) every thread copies or dequantises
// items of the mega segments.  VEC instances move 16 bytes of a dense table or 8 elements of an NF4 one per item, scalar
// instances one element.
constexpr int kSegRows = 2048;             // (tokens per pass) x (G + 1) rows kept in LDS

template <typename TO, bool NF4, bool VEC>
__global__ __launch_bounds__(kBlock) void over_encoding_concat_kernel(NgramArgs a, ConcatArgs c, TO* __restrict__ out,
                                                                      int tok_per_pass) {
  __shared__ SeqFinder finder;
  __shared__ int64_t seg_row[kSegRows];                            // [k * G + g] the mega row, -1: zeros
  __shared__ float cb[16];
  constexpr int kEsize = sizeof(TO);
  constexpr int kPer16 = 16 / kEsize;
  if constexpr (NF4) load_codebook(c.codebook, cb);
  if (a.seq_len == 0) seq_finder_init(finder, a.q_lens, a.flags & kQLensI64, a.batch);
  const int G = a.num_grams;
  const int tid = threadIdx.x;
  const int groups = NF4 ? c.mega_dim / c.group_size : 0;
  const int64_t owned = a.seq_len == 0 ? finder.part[kBlock] : a.tokens;    // packed tokens at or past sum(q_lens): zeros
  // the original table's row of token t: the token alone decides it
  auto ori_row = [&](int64_t t) -> int64_t {
    return t < owned ? local_row(load_index(a.ids, a.flags & kIdsI64, t), 0, c.ori_rows) : -1;
  };
  for (int64_t t0 = static_cast<int64_t>(blockIdx.x) * tok_per_pass; t0 < a.tokens;
       t0 += static_cast<int64_t>(gridDim.x) * tok_per_pass) {
    const int ntok = a.tokens - t0 < tok_per_pass ? static_cast<int>(a.tokens - t0) : tok_per_pass;
    __syncthreads();                                               // the previous pass's rows are no longer read
    for (int p = tid; p < ntok * G; p += kBlock) {                 // (a)
      const int k = p / G, g = p - k * G;
      int64_t seq = 0, pos = 0, row = -1;
      if (locate(a, finder, t0 + k, seq, pos)) row = local_row(ngram_id(a, t0 + k, seq, pos, g), c.mega_vocab_start, c.mega_rows);
      seg_row[p] = row;
    }
    if constexpr (VEC) {                                           // (b)
      const int ori_vecs = c.ori_dim / kPer16;
      copy_items16(tid, static_cast<int64_t>(ntok) * ori_vecs, kBlock, [&](int64_t w, const char*& s, char*& d) {
        const int k = static_cast<int>(w / ori_vecs), i = static_cast<int>(w - static_cast<int64_t>(k) * ori_vecs);
        const int64_t r = ori_row(t0 + k);
        s = r < 0 ? nullptr : c.ori_table + r * c.ori_stride_bytes + (i << 4);
        d = reinterpret_cast<char*>(out + (t0 + k) * c.out_stride) + (i << 4);
      });
    } else {
      for (int w = tid; w < ntok * c.ori_dim; w += kBlock) {
        const int k = w / c.ori_dim, e = w - k * c.ori_dim;
        const int64_t r = ori_row(t0 + k);
        copy_elem(r < 0 ? nullptr : c.ori_table + r * c.ori_stride_bytes + static_cast<int64_t>(e) * kEsize,
                  reinterpret_cast<char*>(out + (t0 + k) * c.out_stride + e), kEsize);
      }
    }
    __syncthreads();                                               // (c)
    constexpr int ITEM = !VEC ? 1 : (NF4 ? 8 : kPer16);
    const int mega_items = G * c.mega_dim / ITEM;
    if constexpr (VEC && !NF4) {
      copy_items16(tid, static_cast<int64_t>(ntok) * mega_items, kBlock, [&](int64_t w, const char*& s, char*& d) {
        const int k = static_cast<int>(w / mega_items), e = static_cast<int>(w - static_cast<int64_t>(k) * mega_items) * ITEM;
        const int g = e / c.mega_dim, col = e - g * c.mega_dim;
        const int64_t r = seg_row[k * G + g];
        s = r < 0 ? nullptr : c.mega_table + r * c.mega_stride_bytes + static_cast<int64_t>(col) * kEsize;
        d = reinterpret_cast<char*>(out + (t0 + k) * c.out_stride + c.ori_dim + e);
      });
    } else {
      for (int w = tid; w < ntok * mega_items; w += kBlock) {
        const int k = w / mega_items, e = (w - k * mega_items) * ITEM;
        const int g = e / c.mega_dim, col = e - g * c.mega_dim;
        const int64_t r = seg_row[k * G + g];
        TO* dst = out + (t0 + k) * c.out_stride + c.ori_dim + e;
        if constexpr (NF4) {
          const Nf4Row row = {r < 0 ? nullptr : reinterpret_cast<const uint8_t*>(c.mega_table) + r * (c.mega_dim >> 1),
                              c.mega_scale, c.mega_mean, r < 0 ? 0 : r * groups};
          if constexpr (VEC) nf4_item8<TO>(row, col, c.group_size, c.sm_code, cb, dst);
          else nf4_elem<TO>(row, col, c.group_size, c.sm_code, cb, dst);
        } else {
          copy_elem(r < 0 ? nullptr : c.mega_table + r * c.mega_stride_bytes + static_cast<int64_t>(col) * kEsize,
                    reinterpret_cast<char*>(dst), kEsize);
        }
      }
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------
int elem_size(int dtype) { return dtype == MOJO_F32 ? 4 : ((dtype == MOJO_F16 || dtype == MOJO_BF16) ? 2 : 0); }

// threads per row: a power of two, about four items per thread, between 16 and a whole block
int lanes_for(int64_t items) {
  int lanes = 16;
  while (lanes < kBlock && static_cast<int64_t>(lanes) * 4 < items) lanes <<= 1;
  return lanes;
}

unsigned grid_for(int64_t work_blocks, int64_t cap = kMaxGrid) {
  return static_cast<unsigned>(work_blocks < 1 ? 1 : (work_blocks > cap ? cap : work_blocks));
}

int check_ngram(const char* what, const NgramArgs& a) {
  MOJO_REQUIRE(a.ids && (a.history || a.hist_len == 0) && a.sizes && a.grams && a.offsets, MOJO_EINVAL, "%s: null pointer", what);
  MOJO_REQUIRE(a.tokens > 0 && a.batch > 0 && a.seq_len >= 0 && a.hist_len >= 0 && a.hist_stride >= a.hist_len, MOJO_EINVAL,
               "%s: bad sizes (tokens %lld, batch %lld, seq_len %lld, history %lld by %lld)", what, (long long)a.tokens,
               (long long)a.batch, (long long)a.seq_len, (long long)a.hist_len, (long long)a.hist_stride);
  MOJO_REQUIRE(a.seq_len == 0 ? a.q_lens != nullptr : a.tokens == a.batch * a.seq_len, MOJO_EINVAL,
               "%s: the packed form needs q_lens, the batched form tokens == batch * seq_len", what);
  MOJO_REQUIRE(a.num_grams >= 1 && a.num_grams <= kBlock - 1, MOJO_EUNSUPPORTED,
               "%s: %d n-gram vocabularies; 1 .. %d supported", what, a.num_grams, kBlock - 1);
  MOJO_REQUIRE(a.max_gram >= 1 && a.hist_len >= a.max_gram - 1, MOJO_EINVAL,
               "%s: the history holds %lld tokens per sequence, fewer than max gram - 1 = %d", what, (long long)a.hist_len,
               a.max_gram - 1);
  return MOJO_OK;
}

}  // namespace

}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_embedding(const void* ids, int ids_i64, const void* table, void* out, int64_t tokens, int64_t rows,
                                  int64_t dim, int64_t vocab_start, int64_t table_row_stride, int64_t out_row_stride,
                                  int dtype, mojo_stream_t stream) {
  if (tokens == 0 || dim == 0) return MOJO_OK;
  const int esize = elem_size(dtype);
  MOJO_REQUIRE(esize != 0, MOJO_EUNSUPPORTED, "embedding: dtype code %d; f32, f16 and bf16 supported", dtype);
  MOJO_REQUIRE(ids && out && (table || rows == 0), MOJO_EINVAL, "embedding: null pointer");
  MOJO_REQUIRE(tokens > 0 && rows >= 0 && dim > 0 && table_row_stride >= dim && out_row_stride >= dim, MOJO_EINVAL,
               "embedding: bad sizes (tokens %lld, rows %lld, dim %lld, strides %lld / %lld)", (long long)tokens,
               (long long)rows, (long long)dim, (long long)table_row_stride, (long long)out_row_stride);
  const int64_t row_bytes = dim * esize, ts = table_row_stride * esize, os = out_row_stride * esize;
  const bool vec = row_bytes % 16 == 0 && ts % 16 == 0 && os % 16 == 0 && aligned_to(table, 16) && aligned_to(out, 16);
  const int lanes = lanes_for(vec ? row_bytes / 16 : dim);
  const unsigned grid = grid_for(ceil_div(tokens, kBlock / lanes), 1 << 20);      // (no per-block prologue: one pass per block)
  auto kernel = vec ? embedding_kernel<true> : embedding_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), ids, ids_i64,
                     static_cast<const char*>(table), static_cast<char*>(out), tokens, rows, row_bytes, vocab_start, ts, os,
                     esize, lanes);
  MOJO_CHECK_LAUNCH("embedding");
  note_launch("embedding:%s:lanes%d", vec ? "vec16" : "scalar", lanes);
  return MOJO_OK;
}

extern "C" int mojo_hip_nf4_embedding(const void* ids, int ids_i64, const void* qweight, const void* scale, const void* mean,
                                      const void* codebook, void* out, int64_t tokens, int64_t rows, int64_t dim,
                                      int64_t group_size, int64_t vocab_start, int64_t out_row_stride, int scale_dtype,
                                      int out_dtype, mojo_stream_t stream) {
  if (tokens == 0 || dim == 0) return MOJO_OK;
  const int esize = elem_size(out_dtype);
  MOJO_REQUIRE(esize != 0 && elem_size(scale_dtype) != 0, MOJO_EUNSUPPORTED,
               "nf4_embedding: dtype codes %d (scale / mean) and %d (output); f32, f16 and bf16 supported", scale_dtype, out_dtype);
  MOJO_REQUIRE(ids && out && codebook && ((qweight && scale && mean) || rows == 0), MOJO_EINVAL, "nf4_embedding: null pointer");
  MOJO_REQUIRE(tokens > 0 && rows >= 0 && dim > 0 && dim % 2 == 0 && dim < (1LL << 30) && out_row_stride >= dim, MOJO_EINVAL,
               "nf4_embedding: bad sizes (tokens %lld, rows %lld, dim %lld even, out stride %lld)", (long long)tokens,
               (long long)rows, (long long)dim, (long long)out_row_stride);
  MOJO_REQUIRE(group_size > 0 && dim % group_size == 0, MOJO_EINVAL,
               "nf4_embedding: group_size %lld must be a positive divisor of dim %lld", (long long)group_size, (long long)dim);
  const bool vec = dim % 8 == 0 && aligned_to(qweight, 4) && aligned_to(out, 16) && (out_row_stride * esize) % 16 == 0;
  const int lanes = lanes_for(vec ? dim / 8 : dim);
  const unsigned grid = grid_for(ceil_div(tokens, kBlock / lanes));
#define MOJO_NF4_LAUNCH(TO, VEC)                                                                                            \
  hipLaunchKernelGGL((nf4_embedding_kernel<TO, VEC>), dim3(grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), ids,   \
                     ids_i64, static_cast<const uint8_t*>(qweight), scale, mean, static_cast<const f16_t*>(codebook),       \
                     static_cast<TO*>(out), tokens, rows, static_cast<int>(dim), static_cast<int>(group_size), vocab_start, \
                     out_row_stride, scale_dtype, lanes)
  if (out_dtype == MOJO_F32) { if (vec) MOJO_NF4_LAUNCH(float, true); else MOJO_NF4_LAUNCH(float, false); }
  else if (out_dtype == MOJO_F16) { if (vec) MOJO_NF4_LAUNCH(f16_t, true); else MOJO_NF4_LAUNCH(f16_t, false); }
  else { if (vec) MOJO_NF4_LAUNCH(bf16_t, true); else MOJO_NF4_LAUNCH(bf16_t, false); }
#undef MOJO_NF4_LAUNCH
  MOJO_CHECK_LAUNCH("nf4_embedding");
  note_launch("nf4_embedding:%s:lanes%d", vec ? "vec8" : "scalar", lanes);
  return MOJO_OK;
}

extern "C" int mojo_hip_oe_ngram(const void* input_ids, const void* history, const void* q_lens, const void* oe_vocab_sizes,
                                 const void* oe_grams, const void* oe_vocab_offsets, void* out, int64_t tokens, int64_t batch,
                                 int64_t seq_len, int64_t hist_len, int64_t hist_stride, int64_t num_grams, int64_t max_gram,
                                 int64_t ori_vocab_size, int index_flags, mojo_stream_t stream) {
  if (tokens == 0 || num_grams == 0) return MOJO_OK;
  MOJO_REQUIRE(num_grams > 0 && num_grams < (1 << 20) && max_gram < (1 << 20), MOJO_EINVAL, "oe_ngram: bad vocabulary count or gram");
  const NgramArgs a = {input_ids, history, q_lens, oe_vocab_sizes, oe_grams, oe_vocab_offsets, tokens, batch, seq_len,
                       hist_len, hist_stride, ori_vocab_size, static_cast<int>(num_grams), static_cast<int>(max_gram),
                       index_flags};
  if (int rc = check_ngram("oe_ngram", a)) return rc;
  MOJO_REQUIRE(out, MOJO_EINVAL, "oe_ngram: null pointer");
  hipLaunchKernelGGL(oe_ngram_kernel, dim3(grid_for(ceil_div(tokens * num_grams, kBlock))), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), a, out);
  MOJO_CHECK_LAUNCH("oe_ngram");
  note_launch("oe_ngram:%s", seq_len == 0 ? "packed" : "batched");
  return MOJO_OK;
}

extern "C" int mojo_hip_over_encoding_concat(const void* input_ids, const void* history, const void* q_lens,
                                             const void* oe_vocab_sizes, const void* oe_grams, const void* oe_vocab_offsets,
                                             int64_t tokens, int64_t batch, int64_t seq_len, int64_t hist_len,
                                             int64_t hist_stride, int64_t num_grams, int64_t max_gram, int64_t ori_vocab_size,
                                             int index_flags, const void* ori_table, int64_t ori_rows, int64_t ori_dim,
                                             int64_t ori_row_stride, const void* mega_table, const void* mega_scale,
                                             const void* mega_mean, const void* codebook, int64_t mega_rows, int64_t mega_dim,
                                             int64_t mega_row_stride, int64_t group_size, int64_t mega_vocab_start,
                                             int mega_nf4, int scale_dtype, void* out, int64_t out_row_stride, int dtype,
                                             mojo_stream_t stream) {
  if (tokens == 0) return MOJO_OK;
  MOJO_REQUIRE(num_grams > 0 && num_grams < (1 << 20) && max_gram < (1 << 20), MOJO_EINVAL,
               "over_encoding_concat: bad vocabulary count or gram");
  const NgramArgs a = {input_ids, history, q_lens, oe_vocab_sizes, oe_grams, oe_vocab_offsets, tokens, batch, seq_len,
                       hist_len, hist_stride, ori_vocab_size, static_cast<int>(num_grams), static_cast<int>(max_gram),
                       index_flags};
  if (int rc = check_ngram("over_encoding_concat", a)) return rc;
  const int esize = elem_size(dtype);
  MOJO_REQUIRE(esize != 0, MOJO_EUNSUPPORTED, "over_encoding_concat: dtype code %d; f32, f16 and bf16 supported", dtype);
  MOJO_REQUIRE(out && (ori_table || ori_rows == 0) && (mega_table || mega_rows == 0), MOJO_EINVAL,
               "over_encoding_concat: null pointer");
  MOJO_REQUIRE(ori_dim > 0 && mega_dim > 0 && ori_rows >= 0 && mega_rows >= 0 && ori_row_stride >= ori_dim, MOJO_EINVAL,
               "over_encoding_concat: bad table sizes");
  const int64_t width = ori_dim + num_grams * mega_dim;
  MOJO_REQUIRE(width < (1LL << 30) && out_row_stride >= width, MOJO_EINVAL,
               "over_encoding_concat: row of %lld elements, out stride %lld", (long long)width, (long long)out_row_stride);
  if (mega_nf4) {
    MOJO_REQUIRE(mega_scale && mega_mean && codebook && elem_size(scale_dtype) != 0, MOJO_EINVAL,
                 "over_encoding_concat: the NF4 table needs scale, mean (f32, f16 or bf16) and the codebook");
    MOJO_REQUIRE(mega_dim % 2 == 0 && group_size > 0 && mega_dim % group_size == 0, MOJO_EINVAL,
                 "over_encoding_concat: NF4 rows of %lld elements in groups of %lld", (long long)mega_dim, (long long)group_size);
  } else {
    MOJO_REQUIRE(mega_row_stride >= mega_dim, MOJO_EINVAL, "over_encoding_concat: mega row stride below its width");
  }
  const ConcatArgs c = {static_cast<const char*>(ori_table), static_cast<const char*>(mega_table), mega_scale, mega_mean,
                        static_cast<const f16_t*>(codebook), ori_rows, ori_row_stride * esize, mega_rows,
                        mega_row_stride * esize, mega_vocab_start, out_row_stride, static_cast<int>(ori_dim),
                        static_cast<int>(mega_dim), static_cast<int>(group_size), scale_dtype};
  // the 16-byte path only where every segment starts, and every source row lies, on a 16-byte boundary
  const int item = mega_nf4 ? 8 : 16 / esize;
  bool vec = ori_dim % item == 0 && mega_dim % item == 0 && aligned_to(out, 16) && (out_row_stride * esize) % 16 == 0 &&
             aligned_to(ori_table, 16) && c.ori_stride_bytes % 16 == 0;
  if (mega_nf4) vec = vec && aligned_to(mega_table, 4);
  else vec = vec && aligned_to(mega_table, 16) && c.mega_stride_bytes % 16 == 0;
  // tokens per pass: the id chain is paid once per pass, but a short input still has to fill the chip with blocks
  // A heuristic on the token count alone, measured on ONE shape (8192 tokens, dims 1536 / 192, 12 vocabularies, bf16: 1 / 2 / 4 /
  // 8 / 16 / 32 tokens per pass 51 / 35 / 27 / 24 / 28 / 41 us; at 128 tokens 7.6 / 8.5 / 9.7 / 12.6 us for 1 / 2 / 4 / 8).  Row
  // bytes and the number of vocabularies do not enter it; other shapes are unmeasured.
  int tok_per_pass = tokens >= 8192 ? 8 : (tokens >= 2048 ? 4 : (tokens >= 512 ? 2 : 1));
  if (tok_per_pass > kSegRows / num_grams) tok_per_pass = static_cast<int>(kSegRows / num_grams);
  if (tok_per_pass < 1) tok_per_pass = 1;
  MOJO_REQUIRE(width * tok_per_pass < (1LL << 31), MOJO_EUNSUPPORTED,
               "over_encoding_concat: %d tokens of %lld elements per pass pass the kernel's 32-bit item index", tok_per_pass,
               (long long)width);
  const unsigned grid = grid_for(ceil_div(tokens, tok_per_pass));
#define MOJO_CONCAT_LAUNCH(TO, NF4, VEC)                                                                                     \
  hipLaunchKernelGGL((over_encoding_concat_kernel<TO, NF4, VEC>), dim3(grid), dim3(kBlock), 0,                               \
                     static_cast<hipStream_t>(stream), a, c, static_cast<TO*>(out), tok_per_pass)
#define MOJO_CONCAT_DTYPE(TO)                                                                                                \
  do {                                                                                                                       \
    if (mega_nf4) { if (vec) MOJO_CONCAT_LAUNCH(TO, true, true); else MOJO_CONCAT_LAUNCH(TO, true, false); }                 \
    else { if (vec) MOJO_CONCAT_LAUNCH(TO, false, true); else MOJO_CONCAT_LAUNCH(TO, false, false); }                        \
  } while (0)
  if (dtype == MOJO_F32) MOJO_CONCAT_DTYPE(float);
  else if (dtype == MOJO_F16) MOJO_CONCAT_DTYPE(f16_t);
  else MOJO_CONCAT_DTYPE(bf16_t);
#undef MOJO_CONCAT_DTYPE
#undef MOJO_CONCAT_LAUNCH
  MOJO_CHECK_LAUNCH("over_encoding_concat");
  note_launch("oe_concat:%s:%s:%s", mega_nf4 ? "nf4" : "dense", vec ? "vec" : "scalar", seq_len == 0 ? "packed" : "batched");
  return MOJO_OK;
}
