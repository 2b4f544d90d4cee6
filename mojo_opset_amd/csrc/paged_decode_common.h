// What the three paged-decode kernels share on the device: decode_split_kernel (vector units, paged_decode_gqa.hip),
// decode_mfma_kernel (16-bit matrix cores, paged_decode_mfma.h) and decode_kv8_kernel (int8 cache, paged_decode_kv8.h).
// Included by paged_decode_gqa.hip behind DecodeArgs, DecodeWin, the chunking rules and decode_head, in front of the first
// kernel.  Every piece is a forced-inline function or a small struct of registers: a kernel compiles to what it compiled to
// with the piece written out in its body.
//
//   DecodePair / decode_pair      the two rows of a paired workgroup and how its eight waves are dealt between them
//   DecodeRow  / decode_row       the row and the chunk of a wave: lengths, chunk size, token range (DecodeWin with a window)
//   DecodeHoles                   the hole scan: the first negative page id among the pages of the chunk
//   decode_lds_merge              a workgroup's partials meet in LDS: merge, normalise, store (or one partial, grouped form)
//   decode_split_finish           split form of the matrix-core kernels: finish a single-chunk row, else leave a partial
//   decode_softmax_step           online softmax of a matrix-core step, scores -> packed probabilities
//   decode_lds_merge_nstep / decode_split_finish_nstep   the two epilogues over the (step, head) columns of DecodeSteps
//                                 (functions of their own: the single-step ones, and with them every existing instance, stay
//                                 exactly as they compile today)
//   Store16                       the 16-bit kernels' output store (the int8 kernel has Kv8Store)
#pragma once

namespace mojo {

// ---- paired form: an 8-wave workgroup owns the rows of rank p and B-1-p when the batch is ordered by length ----------------
struct DecodePair {
  int b[2] = {0, -1};                         // the two sequences (-1: an odd batch's middle row has no partner)
  int len[2] = {0, 0};                        // their lengths, clamped to the launch's capacity
  int chunk[2] = {DEC_TILE, DEC_TILE};        // tokens per wave of each
  int n_first = 8;                            // waves dealt to the first; the rest work on the second
};
// (a select, not an index: an array indexed at run time would live in scratch)
__device__ __forceinline__ int decode_pick(const int (&v)[2], int u) { return u ? v[1] : v[0]; }

__device__ __forceinline__ DecodePair decode_pair(const DecodeArgs& a, int lane, int p) {
  DecodePair pr;
  const int cap = a.n_chunks * a.chunk_tokens;
  int len = -1;                                        // lanes past the batch rank behind every sequence
  if (lane < a.batch) len = a.max_pages > 0 ? max(min(a.seq_lens[lane], cap), 0) : 0;
  int rank = lane;                                     // position of sequence `lane` when ordered by length, longest first
  if (__ballot(lane < a.batch && len != __builtin_amdgcn_readfirstlane(len)) != 0) {   // (a uniform batch keeps its order)
    rank = 0;
    for (int o = 0; o < a.batch; ++o) {
      const int lo = __builtin_amdgcn_readlane(len, o);
      rank += (lo > len || (lo == len && o < lane)) ? 1 : 0;
    }
  }
  const unsigned long long first = __ballot(lane < a.batch && rank == p);
  const unsigned long long second = __ballot(lane < a.batch && rank == a.batch - 1 - p && a.batch - 1 - p > p);
  pr.b[0] = __builtin_ctzll(first);
  pr.len[0] = __builtin_amdgcn_readlane(len, pr.b[0]);
  if (second) {
    pr.b[1] = __builtin_ctzll(second);
    pr.len[1] = __builtin_amdgcn_readlane(len, pr.b[1]);
  }
  const int sum = pr.len[0] + pr.len[1];
  pr.n_first = pr.len[1] <= 0 ? 8 : min(max((8 * pr.len[0] + sum / 2) / sum, 1), 7);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int n_u = u ? 8 - pr.n_first : pr.n_first;
    int c = n_u > 0 ? (pr.len[u] + n_u - 1) / n_u : DEC_TILE;
    c = max(c, 128);
    pr.chunk[u] = ((c + DEC_TILE - 1) / DEC_TILE) * DEC_TILE;
  }
  return pr;
}

// ---- the row and the chunk a wave works on ---------------------------------------------------------------------------------
struct DecodeRow {
  int b = 0, chunk = 0;                       // sequence, chunk of it
  int seq_len = 0, chunk_tokens = 0;          // (with a window: the VIRTUAL length of DecodeWin)
  int tok_begin = 0, tok_end = 0;             // the chunk's tokens; without work one token, so that every address exists
  bool has_work = false;

  __device__ __forceinline__ void cut() {
    tok_begin = chunk * chunk_tokens;
    has_work = seq_len > 0 && tok_begin < seq_len;
    tok_end = has_work ? min(seq_len, tok_begin + chunk_tokens) : tok_begin + 1;
  }
  __device__ __forceinline__ int n_chunks_seq() const { return (seq_len + chunk_tokens - 1) / chunk_tokens; }
};

// a row's length as the launch walks it (clamped to its capacity; with a window the virtual length, and `win` is filled)
template <bool SWA>
__device__ __forceinline__ int decode_row_len(const DecodeArgs& a, int b, DecodeWin& win) {
  if constexpr (SWA) return a.max_pages > 0 ? decode_swa_row(a, b, win) : 0;
  else return a.max_pages > 0 ? decode_seq_len(a, b) : 0;          // (no table columns: nothing to attend over)
}
// unpaired forms: chunk `chunk` of sequence b, `seq_len` = decode_row_len (an argument, not a call from here: with the two
// nested the int8 split instances at head_dim 80 were allocated two more registers)
__device__ __forceinline__ DecodeRow decode_row(const DecodeArgs& a, int b, int chunk, int seq_len) {
  DecodeRow r;
  r.b = b;
  r.chunk = chunk;
  r.seq_len = seq_len;
  r.chunk_tokens = decode_seq_chunk(a, seq_len);
  r.cut();
  return r;
}

// paired form: wave `wave_id` of the workgroup
__device__ __forceinline__ DecodeRow decode_row(const DecodePair& pr, int wave_id) {
  DecodeRow r;
  const int u = wave_id < pr.n_first ? 0 : 1;
  r.b = decode_pick(pr.b, u);
  r.chunk = u ? wave_id - pr.n_first : wave_id;
  r.seq_len = r.b >= 0 ? decode_pick(pr.len, u) : 0;
  r.chunk_tokens = decode_pick(pr.chunk, u);
  if (r.b < 0) r.b = pr.b[0];                          // a wave without a sequence: valid addresses, no work
  r.cut();
  return r;
}

// ---- hole scan -------------------------------------------------------------------------------------------------------------
// The golden walks the pages in order and stops at the first negative id, leaving every later row zero
// (core/operators/attention.py:195-198).  `first_neg` = that page index among the pages up to the end of this chunk
// (a chunk reaching past the table: its width).  The scan (64 table entries per load, one ballot each) does NOT gate the K/V
// loads: a load only needs its own table entry (a negative id is clamped to page 0, an address that certainly exists) and
// remembers its logical page; whether it must read as zero (logical page >= first_neg) is decided when the tile is consumed.
// So the prologue is one round trip — scan batch, query and the first tiles in flight together — instead of up to four
// dependent ones in front of the first K/V byte (measured fixed cost per call before: ~18 us).
// The loads are unconditional, at min(idx, p1 - 1), and the range test sits in the ballot: a guarded load is waited for on the
// spot.  Only a wave with work scans, and work means tok_end >= 1 and max_pages >= 1, so p1 >= 1 and the clamped index
// exists; a lane past p1 re-reads the last entry and is masked out of the ballot, so the result is that of guarded loads.
struct DecodeHoles {
  static constexpr int SCAN = 4;                       // table loads in flight per scan step (256 pages)
  int p1, first_neg = 0x7fffffff;
  int v[SCAN];

  __device__ __forceinline__ DecodeHoles(const DecodeArgs& a, int tok_end) : p1((tok_end + a.page - 1) / a.page) {
    if (p1 > a.max_pages) { first_neg = a.max_pages; p1 = a.max_pages; }
  }
  __device__ __forceinline__ void issue(const int32_t* table, int lane, int base) {
#pragma unroll
    for (int u = 0; u < SCAN; ++u) v[u] = table[min(base + u * 64 + lane, p1 - 1)];
  }
  __device__ __forceinline__ void reduce(int lane, int base) {
#pragma unroll
    for (int u = 0; u < SCAN; ++u) {
      const unsigned long long neg = __ballot(v[u] < 0 && base + u * 64 + lane < p1);
      if (neg && first_neg == 0x7fffffff) first_neg = base + u * 64 + __builtin_ctzll(neg);
    }
  }
  // what the prologue requested (issue(.., 0)), then the rest of a long row (contexts past 256 pages)
  __device__ __forceinline__ void finish(const int32_t* table, int lane) {
    reduce(lane, 0);
    for (int base = 64 * SCAN; base < p1 && first_neg == 0x7fffffff; base += 64 * SCAN) {
      issue(table, lane, base);
      reduce(lane, base);
    }
  }
};

// ---- output stores: four consecutive outputs from element `at` of the [B][Hq][D] output on ---------------------------------
template <typename T>
struct Store16 {
  void* out;
  __device__ __forceinline__ void operator()(int64_t at, f32x4 x) const {
    typename vec_of<T, 4>::type o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = static_cast<T>(x[e]);
    *reinterpret_cast<typename vec_of<T, 4>::type*>(static_cast<T*>(out) + at) = o;
  }
};

// ---- in-LDS merge of a workgroup's partials --------------------------------------------------------------------------------
// Every wave has written its partial to s_part[wave][g][D + 2] (D sums, then the maximum in log2 units and the row sum) in
// its own register layout.  From the barrier on: every thread of the workgroup takes (row of the pair, head g, 4 output
// elements) items, merges the row's chunks, normalises and stores.  A row without tokens gives zeros, or is left untouched
// with a.leave_empty.  PAIRED: the workgroup holds the two rows of `pr` (else `row` alone).  GROUPED: the instance may run
// the grouped form (a.fuse_group > 0) — the workgroup's chunks are not the whole row, and it leaves ONE un-normalised
// partial (slot = workgroup index along x) for the merge launch; compile-time, so that the other instances test nothing.
template <bool PAIRED, bool GROUPED, typename Store>
__device__ __forceinline__ void decode_lds_merge(const DecodeArgs& a, const float* s_part, int D, int G, int kvh,
                                                 const DecodeRow& row, const DecodePair& pr, Store store) {
  static_assert(!(PAIRED && GROUPED), "the paired form is never grouped");
  const int stride = D + 2;
  __syncthreads();
  const int per_head = D / 4;
  constexpr int UNITS = PAIRED ? 2 : 1;
  for (int item = threadIdx.x; item < UNITS * G * per_head; item += blockDim.x) {
    const int u = item / (G * per_head);
    const int rest = item - u * (G * per_head);
    const int g = rest / per_head, d0 = (rest - g * per_head) * 4;
    int ub, ulen, uchunk, slot0, uwaves;
    if constexpr (PAIRED) {
      ub = decode_pick(pr.b, u); ulen = decode_pick(pr.len, u); uchunk = decode_pick(pr.chunk, u);
      slot0 = u ? pr.n_first : 0;
      uwaves = u ? 8 - pr.n_first : pr.n_first;
      if (ub < 0) continue;                              // odd batch: the middle sequence has no partner
    } else {
      ub = row.b; ulen = row.seq_len; uchunk = row.chunk_tokens; slot0 = 0; uwaves = static_cast<int>(blockDim.x >> 6);
    }
    int n_chunks_seq = ulen <= 0 ? 0 : min((ulen + uchunk - 1) / uchunk, uwaves);
    bool partial = false;                                // grouped form: this workgroup's chunks are not the whole row
    if constexpr (GROUPED) {
      if (a.fuse_group > 0) {
        const int total = ulen <= 0 ? 0 : (ulen + uchunk - 1) / uchunk;
        partial = total > uwaves;
        n_chunks_seq = min(max(total - static_cast<int>(blockIdx.x) * uwaves, 0), uwaves);
        if (blockIdx.x > 0 && n_chunks_seq == 0) continue;   // a workgroup past the row's last chunk: nothing to leave
      }
    }
    if (n_chunks_seq == 0 && a.leave_empty) continue;
    const int h = decode_head(a, kvh, g, G);
    float mx = -INFINITY;
    for (int c = 0; c < n_chunks_seq; ++c) mx = fmaxf(mx, s_part[((slot0 + c) * G + g) * stride + D]);
    f32x4 num = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    for (int c = 0; c < n_chunks_seq; ++c) {
      const float* src = s_part + ((slot0 + c) * G + g) * stride;
      const float w = exp2f(src[D] - mx);
      den = fmaf(w, src[D + 1], den);
      num += f32x4{src[d0], src[d0 + 1], src[d0 + 2], src[d0 + 3]} * w;
    }
    if (partial) {                                         // un-normalised sums against this workgroup's maximum, for the merge launch
      const int64_t slot = (static_cast<int64_t>(blockIdx.y) * a.n_chunks + blockIdx.x) * G + g;
      *reinterpret_cast<f32x4*>(a.ws_acc + slot * D + d0) = num;
      if (d0 == 0) { a.ws_ml[slot * 2 + 0] = mx; a.ws_ml[slot * 2 + 1] = den; }
      continue;
    }
    const float inv = n_chunks_seq > 0 ? 1.0f / den : 0.f;      // empty sequence: zeros (golden semantics)
    store((static_cast<int64_t>(ub) * a.hq + h) * D + d0, num * inv);
  }
}

// ---- split form of the matrix-core kernels: lane (head tl, dims 16 dt + 4 g4 .. + 3 of every d tile) -----------------------
// A row of a single chunk is finished here (the merge kernel skips it); else the fp32 sums and (m, l) go to the workspace.
template <int ND, typename Store>
__device__ __forceinline__ void decode_split_finish(const DecodeArgs& a, int G, int kvh, const DecodeRow& row, int tl, int g4,
                                                    const f32x4 (&o)[ND], float m, float l, Store store) {
  constexpr int D = ND * 16;
  if (tl >= G) return;
  if (row.n_chunks_seq() == 1) {
    const int h = decode_head(a, kvh, tl, G);
    const float inv = 1.0f / l;
    const int64_t at = (static_cast<int64_t>(row.b) * a.hq + h) * D + 4 * g4;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) store(at + dt * 16, o[dt] * inv);
    return;
  }
  const int64_t slot = (static_cast<int64_t>(blockIdx.y) * a.n_chunks + row.chunk) * G + tl;
  float* dst = a.ws_acc + slot * D + 4 * g4;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) *reinterpret_cast<f32x4*>(dst + dt * 16) = o[dt];
  if (g4 == 0) {
    a.ws_ml[slot * 2 + 0] = m;
    a.ws_ml[slot * 2 + 1] = l;
  }
}

// ---- the n-step epilogues (DecodeSteps) -------------------------------------------------------------------------------------
// As decode_lds_merge<false, true> and decode_split_finish, over the NC columns of the block `st`: slot
// s_part[wave][column][D + 2], a column's output row from decode_col_at.  A column without a step (decode_col_ok) is
// skipped; a step that saw no key in any chunk (0 < len < steps) has maximum -inf and sum 0 and stores zeros — no weight
// exp2(-inf - -inf), no 1 / 0; only a sequence without keys (st.len <= 0) is an empty row that a.leave_empty leaves alone.
template <typename Store>
__device__ __forceinline__ void decode_lds_merge_nstep(const DecodeArgs& a, const float* s_part, int D, int NC, const DecodeRow& row,
                                                       const DecodeSteps& st, Store store) {
  const int stride = D + 2;
  __syncthreads();
  const int per_col = D / 4;
  const int uwaves = static_cast<int>(blockDim.x >> 6);
  const int total = row.seq_len <= 0 ? 0 : row.n_chunks_seq();
  int n_chunks_seq = min(total, uwaves);
  bool partial = false;                                  // grouped form: this workgroup's chunks are not the whole row
  if (a.fuse_group > 0) {
    partial = total > uwaves;
    n_chunks_seq = min(max(total - static_cast<int>(blockIdx.x) * uwaves, 0), uwaves);
    if (blockIdx.x > 0 && n_chunks_seq == 0) return;     // a workgroup past the row's last chunk: nothing to leave
  }
  if (n_chunks_seq == 0 && a.leave_empty && st.len <= 0) return;
  for (int item = threadIdx.x; item < NC * per_col; item += blockDim.x) {
    const int c = item / per_col, d0 = (item - c * per_col) * 4;
    if (!decode_col_ok(st, c)) continue;
    float mx = -INFINITY;
    for (int w = 0; w < n_chunks_seq; ++w) mx = fmaxf(mx, s_part[(w * NC + c) * stride + D]);
    if (mx == -INFINITY) mx = 0.f;
    f32x4 num = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    for (int w = 0; w < n_chunks_seq; ++w) {
      const float* src = s_part + (w * NC + c) * stride;
      const float wt = exp2f(src[D] - mx);
      den = fmaf(wt, src[D + 1], den);
      num += f32x4{src[d0], src[d0 + 1], src[d0 + 2], src[d0 + 3]} * wt;
    }
    if (partial) {                                       // un-normalised sums against this workgroup's maximum, for the merge launch
      const int64_t slot = (static_cast<int64_t>(blockIdx.y) * a.n_chunks + blockIdx.x) * NC + c;
      *reinterpret_cast<f32x4*>(a.ws_acc + slot * D + d0) = num;
      if (d0 == 0) { a.ws_ml[slot * 2 + 0] = mx; a.ws_ml[slot * 2 + 1] = den; }
      continue;
    }
    store(decode_col_at(a, st, c) + d0, num * (den > 0.f ? 1.0f / den : 0.f));
  }
}

template <int ND, typename Store>
__device__ __forceinline__ void decode_split_finish_nstep(const DecodeArgs& a, int NC, const DecodeRow& row, const DecodeSteps& st,
                                                          int tl, int g4, const f32x4 (&o)[ND], float m, float l, Store store) {
  constexpr int D = ND * 16;
  if (!decode_col_ok(st, tl)) return;
  if (row.n_chunks_seq() == 1) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    const int64_t at = decode_col_at(a, st, tl) + 4 * g4;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) store(at + dt * 16, o[dt] * inv);
    return;
  }
  const int64_t slot = (static_cast<int64_t>(blockIdx.y) * a.n_chunks + row.chunk) * NC + tl;
  float* dst = a.ws_acc + slot * D + 4 * g4;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) *reinterpret_cast<f32x4*>(dst + dt * 16) = o[dt];
  if (g4 == 0) {
    a.ws_ml[slot * 2 + 0] = m;
    a.ws_ml[slot * 2 + 1] = l;
  }
}

// ---- online softmax of a matrix-core step ----------------------------------------------------------------------------------
// x[ss][i]: masked scores (log2 units) of head tl, token 16 ss + 4 g4 + i.  The step's maximum over all four token groups, a
// lazy reference (O and the sum are rescaled only when the maximum grows by 2^8, so probabilities stay below 2^8), the
// probabilities packed as the B operand of the P V product (MM::pack: dec_mma<T>).  m, l and o[] are the kernel's own.
template <typename MM, int NS, int ND>
__device__ __forceinline__ void decode_softmax_step(const float (&x)[NS][4], float& m, float& l, f32x4 (&o)[ND],
                                                    typename MM::frag4 (&pf)[NS]) {
  float mx = fmaxf(fmaxf(x[0][0], x[0][1]), fmaxf(x[0][2], x[0][3]));
#pragma unroll
  for (int ss = 1; ss < NS; ++ss) mx = fmaxf(mx, fmaxf(fmaxf(x[ss][0], x[ss][1]), fmaxf(x[ss][2], x[ss][3])));
  mx = xor_max_16_32(mx);                              // the head's maximum over the step (all four token groups)
  float ref = m;
  if (mx - m > 8.0f) ref = mx;                         // m = -inf: any finite score; NaN (-inf - -inf): keep
  if (!__all(ref == m)) {
    const float alpha = m == ref ? 1.f : fast_exp2(m - ref);        // m = -inf: 0 (O and the sum are 0)
    l *= alpha;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o[dt] *= alpha;
    m = ref;
  }
  const float ms = m == -INFINITY ? 0.f : m;
#pragma unroll
  for (int ss = 0; ss < NS; ++ss) {
    float p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = fast_exp2(x[ss][i] - ms);
    l += (p[0] + p[1]) + (p[2] + p[3]);
    pf[ss] = MM::pack(p[0], p[1], p[2], p[3]);
  }
}

}  // namespace mojo
