// What the latent-attention kernels share on the device: mla_latent_kernel (mla_attn.hip), mla512_oct_kernel (mla512_oct.h),
// mla512_ps_kernel (mla512_ps.h), the opt-in mla512_pair_kernel / mla512_pp_kernel (experiments/) and mla_merge_kernel.
// Included by mla_attn.hip behind MlaArgs, in front of the first kernel.  Every piece is a forced-inline function or a small
// struct of registers: a kernel compiles to what it compiled to with the piece written out in its body
// (profiles/mla_common_kernel_metadata.md).
//
//   MlaRow / mla_row        the row of a workgroup: padding token or not, its block-table row, the visible keys n_vis after
//                           the cut at the first negative page id                       all five attention kernels
//   MlaWindow               the LDS window of page ids: fill, the refill test in front of a tile, lookup
//                                                                                       latent, oct, pair, pp (ps: scalar loads)
//   mla_finish              single-split finish: the normaliser with the sink logit folded in, zero for a row without keys
//                                                                                       all five attention kernels
//   mla_merge_sink / mla_sink_share / mla_merge_inv   the same finish split around the sum over the splits   mla_merge_kernel
//   mla_slot                index of a (token, split, head) partial in part_o / part_ml  all six
//
// What stays in the kernels: the split's key range and tile count (tile sizes differ), staging, LDS images, softmax, the MFMA
// loops and the epilogue stores.
#pragma once

namespace mojo {

constexpr float MLA_LOG2E = 1.4426950408889634f;

// ---- the row ----------------------------------------------------------------------------------------------------------------
struct MlaRow {
  bool padding = false;                       // prefill: a token no sequence owns; its output stays zero (workgroup-uniform)
  const int32_t* table = nullptr;             // the sequence's block-table row
  int n_vis = 0;                              // keys the token sees: causal, cut at the first negative page id
};

// decode: tile == sequence.  prefill: tile == query token t of sequence b (binary search over cu_q), which sees the keys
// 0 .. kv_len - q_len + t.  The golden drops the pages behind the first negative id, and so does the cut here: every lane of
// the wave must call this (the scan is a ballot over 64 table entries at a time).
__device__ __forceinline__ MlaRow mla_row(const MlaArgs& a, int tile, int lane) {
  MlaRow row;
  int b, n_vis;
  if (a.cu_q == nullptr) {
    b = tile;
    n_vis = a.seq_lens[b];
  } else {
    if (tile < a.cu_q[0] || tile >= a.cu_q[a.batch]) {
      row.padding = true;
      return row;
    }
    int lo = 0, hi = a.batch;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.cu_q[mid] <= tile) lo = mid; else hi = mid;
    }
    b = lo;
    const int q_len = a.cu_q[b + 1] - a.cu_q[b];
    const int kv_len = a.cu_kv ? a.cu_kv[b + 1] - a.cu_kv[b] : q_len;
    n_vis = min(kv_len, kv_len - q_len + (tile - a.cu_q[b]) + 1);
  }
  const int32_t* table = a.tables + static_cast<int64_t>(b) * a.table_stride;
  if (n_vis > 0) {
    int p1 = (n_vis + a.page - 1) / a.page;
    int fn = -1;
    if (p1 > a.max_pages) { fn = a.max_pages; p1 = a.max_pages; }
    for (int base = 0; base < p1; base += 64) {
      const int idx = base + lane;
      const int v = idx < p1 ? table[idx] : 0;
      const unsigned long long neg = __ballot(v < 0);
      if (neg) { fn = base + __builtin_ctzll(neg); break; }
    }
    if (fn >= 0) n_vis = min(n_vis, fn * a.page);
  }
  row.table = table;
  row.n_vis = n_vis;
  return row;
}

// ---- the page-id window -----------------------------------------------------------------------------------------------------
// ENTRIES page ids of the row live in LDS, refilled when the key loop walks past them: no dependent global load — and no FLAT
// load, which hipcc guards with vmcnt(0)/lgkmcnt(0) — sits in front of the LDS-DMA.  THREADS = the workgroup's size; fill and
// ahead hold a workgroup barrier, so every thread calls them with the same arguments.
template <int ENTRIES, int THREADS>
struct MlaWindow {
  int* ids;                                   // the window in LDS
  unsigned ids_u32;                           // its LDS byte address (for lookups written as ds_read)
  const MlaArgs& a;
  const int32_t* table;
  int base;

  __device__ __forceinline__ MlaWindow(char* lds, const MlaArgs& a_, const int32_t* table_)
      : ids(reinterpret_cast<int*>(lds)), ids_u32(static_cast<unsigned>(reinterpret_cast<size_t>((lds_m*)lds))), a(a_), table(table_),
        base(0) {}
  __device__ __forceinline__ void fill(int p0) {
    for (int i = threadIdx.x; i < ENTRIES; i += THREADS) ids[i] = (p0 + i < a.max_pages) ? table[p0 + i] : -1;
    base = p0;
    __syncthreads();
  }
  // in front of a tile of the keys k_first .. k_last (page_of: the kernel's key -> logical page; keys, not pages: with both
  // pages worked out in front of the test oct, pair and pp were allocated one register less and the r = 32 instance one
  // scalar register more than with the window written out)
  template <typename PageOf>
  __device__ __forceinline__ void ahead(int k_first, int k_last, PageOf page_of) {
    const int p_last = page_of(k_last);
    if (p_last >= base + ENTRIES) {
      __syncthreads();
      fill(page_of(k_first));
    }
  }
  __device__ __forceinline__ int id(int page) const { return ids[page - base]; }
  __device__ __forceinline__ unsigned addr(int page) const { return ids_u32 + 4 * (page - base); }
};

// ---- the finish -------------------------------------------------------------------------------------------------------------
// Each kernel keeps its own exponential: the general kernel and the merge exp2f, the r = 512 kernels the hardware's.
struct MlaExp2 { __device__ __forceinline__ float operator()(float x) const { return exp2f(x); } };
struct MlaFastExp2 { __device__ __forceinline__ float operator()(float x) const { return fast_exp2(x); } };

// One split: what the un-normalised row is multiplied by.  m2 = the row's reference maximum in log2 units, no_keys = that
// maximum is still -inf (the caller's test: the r = 512 kernels hold the maximum before the scale and test it there),
// lsum = its sum of 2^(score - m2).  The optional sink logit (natural-log units) joins the denominator only.  A row without
// keys and without a sink becomes zeros (nan_to_num).
template <typename Exp>
__device__ __forceinline__ float mla_finish(float m2, bool no_keys, float lsum, const float* sink, int head) {
  float den = lsum;
  float w = 1.f;
  if (sink) {
    const float sk = sink[head] * MLA_LOG2E;
    const float M = fmaxf(m2, sk);
    w = no_keys ? 0.f : Exp{}(m2 - M);
    den = lsum * w + Exp{}(sk - M);
  }
  return den > 0.f ? w / den : 0.f;
}

// Several splits (the merge): the sink logit joins the maximum over the splits in front of the sum over them ...
__device__ __forceinline__ float mla_merge_sink(const float* sink, int head, float& M) {
  float sk = 0.f;
  if (sink) {
    sk = sink[head] * MLA_LOG2E;
    M = fmaxf(M, sk);
  }
  return sk;
}
// ... its share of the denominator opens that sum, and the normaliser closes it.
__device__ __forceinline__ float mla_sink_share(const float* sink, float sk, float M) { return sink ? exp2f(sk - M) : 0.f; }
__device__ __forceinline__ float mla_merge_inv(float den) { return den > 0.f ? 1.0f / den : 0.f; }

// ---- the partial of (token, split, head): part_o[slot * r ..], part_ml[slot * 2 ..] -----------------------------------------
__device__ __forceinline__ int64_t mla_slot(const MlaArgs& a, int tile, int split, int head) {
  return (static_cast<int64_t>(tile) * a.n_splits + split) * a.heads + head;
}

}  // namespace mojo
