// The sampling step: exact top-K over the vocabulary with the nucleus (top-p) mask and the inverse-CDF draw fused behind it,
// the penalties / temperature pass, and the two speculative acceptance steps (core/operators/sampling.py).
//
// Selection is exact and deterministic: every value becomes an order-preserving 32-bit key, a candidate is the 64-bit
// composite (key << 32 | ~index), so "larger composite" means "larger value, and among equal values the lower index".  All
// composites of a row are distinct, the top K of them are unique, and nothing depends on the order in which threads arrive:
// the only atomics are integer histogram counts and output slots of a list that is sorted afterwards.
//
//   pass A  select_segments_kernel, one workgroup per (row, slice): the slice is staged once in LDS as keys (16-byte global
//           loads), in segments of at most kSegKeys keys; a radix select (12 + 10 + 10 key bits, then the index bits only when a
//           tie straddles the cut) finds the segment's own top min(K, length) and writes the composites to the workspace.
//   pass B  finish_rows_kernel, one workgroup of 1024 per row: radix-selects the exact top K among the segments' candidates
//           (read from the workspace, L2-resident), sorts them with a bitonic network, then softmax, running sum, mask,
//           second softmax and either the filter's outputs or the inverse-CDF pick, in the same workgroup.
//
// The slice count only changes how the candidates are found, never which K win or their order, so every slice count gives
// the same bits.  The arithmetic over the K sorted values (exponentials, sums, running sums) is fp64 in a fixed tree order,
// rounded to fp32 where the golden holds an fp32 tensor.  -inf logits are legal; NaN and +inf are not supported.
//
// Algorithmic bytes: rows x vocab x element size, read once.
#include "common.h"

namespace mojo {
namespace sampling {

constexpr int kMaxK = 1024;            // K of the fused path: one sorted candidate per thread of pass B
constexpr int kSegKeys = 16384;        // keys of one staged segment (64 KiB of LDS)
constexpr int kBins = 4096;            // histogram of the widest digit (12 bits)
constexpr int kSelThreads = 512;       // pass A
constexpr int kRowThreads = 1024;      // pass B
constexpr int kCtlInts = 32;
constexpr int kCUs = 256;
constexpr size_t kSelLdsBytes = (kSegKeys + kBins + kCtlInts) * sizeof(uint32_t);

// How a row is cut: `slices` workgroups per row, each walking `sub` segments of `seg_len` keys (a multiple of 64).
struct Geometry {
  int64_t vocab, slice_len, seg_len;
  int slices, sub, nseg, kcap;         // kcap = min(K, seg_len): workspace slots per segment
  int64_t candidates;                  // sum over the segments of min(K, length)
};

static inline int64_t round_up(int64_t a, int64_t b) { return ceil_div(a, b) * b; }

__host__ __device__ __forceinline__ void segment_range(const Geometry& g, int seg, int64_t& start, int64_t& end) {
  const int s = seg / g.sub, j = seg - s * g.sub;
  const int64_t s0 = static_cast<int64_t>(s) * g.slice_len;
  const int64_t s1 = s0 + g.slice_len < g.vocab ? s0 + g.slice_len : g.vocab;
  start = s0 + static_cast<int64_t>(j) * g.seg_len;
  end = start + g.seg_len < s1 ? start + g.seg_len : s1;
  if (end < start) end = start;
}

static Geometry make_geometry(int64_t rows, int64_t vocab, int64_t k, int64_t slices_req) {
  Geometry g{};
  g.vocab = vocab;
  int64_t slices = slices_req;
  if (slices <= 0) {
    // every CU a workgroup, but slices no shorter than 4 K (else pass A keeps most of what it reads), and short enough to stage whole
    slices = ceil_div(kCUs, rows > 0 ? rows : 1);
    const int64_t widest = vocab / (4 * k) > 1 ? vocab / (4 * k) : 1;
    if (slices > widest) slices = widest;
    if (slices < ceil_div(vocab, kSegKeys)) slices = ceil_div(vocab, kSegKeys);
  }
  if (slices > ceil_div(vocab, 64)) slices = ceil_div(vocab, 64);
  if (slices > 4096) slices = 4096;
  g.slice_len = round_up(ceil_div(vocab, slices), 64);
  g.slices = static_cast<int>(ceil_div(vocab, g.slice_len));
  g.sub = static_cast<int>(ceil_div(g.slice_len, kSegKeys));
  g.seg_len = round_up(ceil_div(g.slice_len, g.sub), 64);
  g.nseg = g.slices * g.sub;
  g.kcap = static_cast<int>(k < g.seg_len ? k : g.seg_len);
  g.candidates = 0;
  for (int seg = 0; seg < g.nseg; ++seg) {
    int64_t a, b;
    segment_range(g, seg, a, b);
    g.candidates += (b - a) < k ? (b - a) : k;
  }
  return g;
}

// fp32 -> key with the order of the values (-0.0 reads as +0.0: the golden's sort holds them equal); and back
__device__ __forceinline__ uint32_t key_of(float v) {
  uint32_t u = __builtin_bit_cast(uint32_t, v);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t key) {
  return __builtin_bit_cast(float, (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
__device__ __forceinline__ uint64_t composite(uint32_t key, uint32_t index) {
  return (static_cast<uint64_t>(key) << 32) | static_cast<uint32_t>(~index);
}

// exclusive prefix sum of x over the NT threads of the workgroup (wsum: NT / 64 ints)
template <int NT>
__device__ __forceinline__ int block_exclusive_sum(int x, int* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(incl, d);
    if (lane >= d) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  return base + incl - x;
}

// The threshold T with exactly `need` of the candidates >= T.  get(i, c) -> whether slot i of [0, n_slots) holds a candidate,
// and its composite; n_valid candidates in all.  Digits from the top: 12 + 10 + 10 bits of the key, then of ~index; a pass
// whose chosen bin holds exactly what is still needed ends the search (everything under the prefix is taken), which without
// a tie at the cut happens inside the key.  Called by all NT threads; hist: kBins ints, ctl: kCtlInts ints.
template <int NT, typename Get>
__device__ __forceinline__ uint64_t select_threshold(Get get, int n_slots, int n_valid, int need, int* hist, int* ctl) {
  if (need >= n_valid) return 0;
  uint64_t prefix = 0, mask = 0;
  int shift = 64;
#pragma unroll 1
  for (int pass = 0; pass < 6; ++pass) {
    const int w = (pass % 3 == 0) ? 12 : 10;
    const int bins = 1 << w;
    shift -= w;
    for (int b = threadIdx.x; b < bins; b += NT) hist[b] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n_slots; i += NT) {
      uint64_t c;
      if (get(i, c) && (c & mask) == prefix) atomicAdd(&hist[static_cast<int>(c >> shift) & (bins - 1)], 1);
    }
    __syncthreads();
    // thread 0 owns the highest bins: the exclusive prefix sum over threads is the count above a thread's bins
    const int per = bins / NT;
    const int first = (NT - 1 - static_cast<int>(threadIdx.x)) * per;
    int mine = 0;
    for (int q = 0; q < per; ++q) mine += hist[first + q];
    const int above = block_exclusive_sum<NT>(mine, ctl + 8);
    if (above < need && need <= above + mine) {              // exactly one thread
      int a = above;
      for (int q = per - 1; q >= 0; --q) {
        const int h = hist[first + q];
        if (need <= a + h) {
          ctl[0] = first + q;
          ctl[1] = need - a;
          ctl[2] = h;
          break;
        }
        a += h;
      }
    }
    __syncthreads();
    const int digit = ctl[0], count = ctl[2];
    need = ctl[1];
    prefix |= static_cast<uint64_t>(digit) << shift;
    mask |= static_cast<uint64_t>(bins - 1) << shift;
    __syncthreads();
    if (count == need) break;
  }
  return prefix;
}

// ---- pass A ---------------------------------------------------------------------------------------------------------
template <typename T, bool WIDE>
__global__ __launch_bounds__(kSelThreads) void select_segments_kernel(const T* __restrict__ logits, uint64_t* __restrict__ ws,
                                                                      Geometry g, int k) {
  extern __shared__ uint32_t lds[];
  uint32_t* keys = lds;
  int* hist = reinterpret_cast<int*>(lds + kSegKeys);
  int* ctl = hist + kBins;
  constexpr int VEC = 16 / sizeof(T);
  const int64_t row = blockIdx.x / g.slices;
  const int slice = blockIdx.x - static_cast<int>(row) * g.slices;
  const T* x = logits + row * g.vocab;
  for (int j = 0; j < g.sub; ++j) {
    const int seg = slice * g.sub + j;
    int64_t start, end;
    segment_range(g, seg, start, end);
    const int n = static_cast<int>(end - start);
    if (n <= 0) continue;                                        // (the same for every thread)
    if constexpr (WIDE) {                                        // vocab % VEC == 0 and a 16-byte aligned base: so is every segment
      const int nv = n / VEC;
#pragma unroll 4
      for (int v = threadIdx.x; v < nv; v += kSelThreads) {
        const typename vec_of<T, VEC>::type val = load_vec<T, VEC>(x + start + static_cast<int64_t>(v) * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) keys[v * VEC + e] = key_of(elt<T>::to_f(vget<T, VEC>(val, e)));
      }
    } else {
      for (int i = threadIdx.x; i < n; i += kSelThreads) keys[i] = key_of(elt<T>::to_f(x[start + i]));
    }
    if (threadIdx.x == 0) ctl[4] = 0;
    __syncthreads();
    const uint32_t base = static_cast<uint32_t>(start);
    auto get = [&](int i, uint64_t& c) { c = composite(keys[i], base + i); return true; };
    const int take = k < n ? k : n;
    const uint64_t threshold = select_threshold<kSelThreads>(get, n, n, take, hist, ctl);
    uint64_t* dst = ws + (row * g.nseg + seg) * static_cast<int64_t>(g.kcap);
    for (int i = threadIdx.x; i < n; i += kSelThreads) {
      const uint64_t c = composite(keys[i], base + i);
      if (c >= threshold) {
        const int pos = atomicAdd(&ctl[4], 1);
        if (pos < take) dst[pos] = c;
      }
    }
    __syncthreads();                                             // the next segment overwrites keys and ctl
  }
}

// ---- pass B ---------------------------------------------------------------------------------------------------------
template <typename V, typename Op>
__device__ __forceinline__ V block_reduce(V x, Op op, V* scratch /* 16 */) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x = op(x, __shfl_xor(x, d));
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = x;
  __syncthreads();
  V r = scratch[0];
#pragma unroll
  for (int w = 1; w < kRowThreads / 64; ++w) r = op(r, scratch[w]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ double block_inclusive_sum(double x, double* scratch /* 16 */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) scratch[wave] = x;
  __syncthreads();
  double base = 0.0;
  for (int w = 0; w < wave; ++w) base += scratch[w];
  __syncthreads();
  return base + x;
}

struct FinishArgs {
  const uint64_t* ws;
  Geometry g;
  int k, padded;                  // padded: K raised to a power of two, the width of the sorting network
  float top_p, filter_value;
  int min_keep, nucleus;          // nucleus == 0: the distribution is the plain softmax of the K values
  // filter form (probs != NULL): [rows, K] probabilities in `dtype`, [rows, K] int64 indices
  void* probs;
  int64_t* indices;
  int dtype;
  // sampling form (uniforms != NULL): one fp32 uniform per row -> the picked probability and token
  const float* uniforms;
  float* next_prob;
  int64_t* next_token;
};

__global__ __launch_bounds__(kRowThreads) void finish_rows_kernel(FinishArgs a) {
  __shared__ uint64_t sorted[kMaxK];
  __shared__ int hist[kBins];
  __shared__ int ctl[kCtlInts];
  __shared__ double dscratch[kRowThreads / 64];
  __shared__ int iscratch[kRowThreads / 64];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int k = a.k;
  const Geometry& g = a.g;
  const uint64_t* src = a.ws + row * g.nseg * static_cast<int64_t>(g.kcap);
  const int n_slots = g.nseg * g.kcap;
  auto get = [&](int i, uint64_t& c) {
    const int seg = i / g.kcap, j = i - seg * g.kcap;
    int64_t s, e;
    segment_range(g, seg, s, e);
    const int64_t len = e - s;
    if (j >= (len < k ? len : k)) return false;
    c = src[i];
    return true;
  };
  if (tid == 0) ctl[4] = 0;
  __syncthreads();
  const uint64_t threshold = select_threshold<kRowThreads>(get, n_slots, static_cast<int>(g.candidates), k, hist, ctl);
  for (int i = tid; i < n_slots; i += kRowThreads) {
    uint64_t c;
    if (get(i, c) && c >= threshold) {
      const int pos = atomicAdd(&ctl[4], 1);
      if (pos < k) sorted[pos] = c;
    }
  }
  if (tid >= k && tid < a.padded) sorted[tid] = 0;               // below every candidate
  __syncthreads();
  // bitonic network, descending
  for (int size = 2; size <= a.padded; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (tid < (a.padded >> 1)) {
        const int lo = 2 * tid - (tid & (stride - 1));
        const int hi = lo + stride;
        const bool descending = (lo & size) == 0;
        const uint64_t p = sorted[lo], q = sorted[hi];
        if ((p < q) == descending) {
          sorted[lo] = q;
          sorted[hi] = p;
        }
      }
      __syncthreads();
    }
  }
  const bool live = tid < k;
  const uint64_t me = sorted[live ? tid : 0];
  const float v = value_of(static_cast<uint32_t>(me >> 32));
  const int64_t index = static_cast<int64_t>(static_cast<uint32_t>(~static_cast<uint32_t>(me)));
  const float v0 = value_of(static_cast<uint32_t>(sorted[0] >> 32));
  auto add = [](double x, double y) { return x + y; };
  auto imin = [](int x, int y) { return x < y ? x : y; };
  auto imax = [](int x, int y) { return x > y ? x : y; };

  // first softmax (the maximum is position 0) and where its running sum first exceeds top_p
  // (exponentials, sums and quotients in fp64, rounded once: K values per row, and the result is the correctly rounded fp32)
  const double e1 = live ? exp(static_cast<double>(v) - static_cast<double>(v0)) : 0.0;
  const float p1 = static_cast<float>(e1 / block_reduce(e1, add, dscratch));
  float final_p = p1;
  if (a.nucleus) {
    const float cum = static_cast<float>(block_inclusive_sum(static_cast<double>(p1), dscratch));
    const int cut = block_reduce((live && cum > a.top_p) ? tid : k, imin, iscratch);
    // removed = over shifted right by one, with the first min_keep - 1 positions of `over` cleared and position 0 kept
    int kept = (cut > a.min_keep - 1 ? cut : a.min_keep - 1) + 1;
    if (kept > k) kept = k;
    const float x = tid < kept ? v : a.filter_value;
    const float m = kept < k ? fmaxf(v0, a.filter_value) : v0;
    const double e2 = live ? exp(static_cast<double>(x) - static_cast<double>(m)) : 0.0;
    final_p = static_cast<float>(e2 / block_reduce(e2, add, dscratch));
  }
  if (a.probs != nullptr && live) {
    const int64_t o = row * k + tid;
    if (a.dtype == MOJO_F32) static_cast<float*>(a.probs)[o] = final_p;
    else if (a.dtype == MOJO_F16) static_cast<f16_t*>(a.probs)[o] = static_cast<f16_t>(final_p);
    else static_cast<bf16_t*>(a.probs)[o] = static_cast<bf16_t>(final_p);
    a.indices[o] = index;
  }
  if (a.uniforms != nullptr) {
    // inverse CDF: the first position whose running sum exceeds u x total, held to the last position of non-zero probability
    const double run = block_inclusive_sum(live ? static_cast<double>(final_p) : 0.0, dscratch);
    if (tid == k - 1) dscratch[0] = run;
    __syncthreads();
    const double target = static_cast<double>(a.uniforms[row]) * dscratch[0];
    __syncthreads();
    int pick = block_reduce((live && run > target) ? tid : k, imin, iscratch);
    const int last = block_reduce((live && final_p > 0.f) ? tid : -1, imax, iscratch);
    if (pick > last) pick = last;
    if (pick < 0) pick = 0;
    if (tid == pick) {
      a.next_prob[row] = final_p;
      a.next_token[row] = index;
    }
  }
}

static int check_select(const void* logits, const void* workspace, int64_t workspace_bytes, int64_t rows, int64_t vocab, int64_t k,
                        int64_t min_keep, int64_t slices, int dtype, const char* what) {
  MOJO_REQUIRE(rows >= 0 && vocab >= 1 && k >= 1 && slices >= 0, MOJO_EINVAL, "%s: bad sizes (rows %lld, vocab %lld, k %lld, slices %lld)",
               what, (long long)rows, (long long)vocab, (long long)k, (long long)slices);
  MOJO_REQUIRE(k <= vocab, MOJO_EINVAL, "%s: k %lld above the vocabulary %lld (clamp it first)", what, (long long)k, (long long)vocab);
  MOJO_REQUIRE(k <= kMaxK, MOJO_EUNSUPPORTED, "%s: k %lld is above the cap of %d of the fused path", what, (long long)k, kMaxK);
  MOJO_REQUIRE(vocab < (1LL << 31) && rows < (1LL << 18) && min_keep < (1LL << 31), MOJO_EUNSUPPORTED, "%s: more than 2^18 rows or 2^31 columns", what);
  MOJO_REQUIRE(dtype == MOJO_F32 || dtype == MOJO_F16 || dtype == MOJO_BF16, MOJO_EUNSUPPORTED, "%s: dtype %d not supported", what, dtype);
  if (rows == 0) return MOJO_OK;
  MOJO_REQUIRE(logits != nullptr, MOJO_EINVAL, "%s: null logits", what);
  const int64_t need = mojo_hip_sampling_workspace_bytes(rows, vocab, k, slices);
  MOJO_REQUIRE(workspace != nullptr && workspace_bytes >= need && aligned_to(workspace, 8), MOJO_EWORKSPACE,
               "%s: workspace of %lld bytes, %lld needed (8-byte aligned)", what, (long long)workspace_bytes, (long long)need);
  return MOJO_OK;
}

template <typename T>
static int launch_select(const void* logits, uint64_t* ws, const Geometry& g, int64_t rows, int k, hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  const bool wide = g.vocab % VEC == 0 && aligned_to(logits, 16);
  const dim3 grid(static_cast<unsigned>(rows * g.slices));
  static std::atomic<uint64_t> attr_wide{0}, attr_narrow{0};
  if (wide) {
    auto* fn = select_segments_kernel<T, true>;
    if (first_call_on_device(attr_wide))
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, kSelLdsBytes);
    hipLaunchKernelGGL(fn, grid, dim3(kSelThreads), kSelLdsBytes, s, static_cast<const T*>(logits), ws, g, k);
  } else {
    auto* fn = select_segments_kernel<T, false>;
    if (first_call_on_device(attr_narrow))
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, kSelLdsBytes);
    hipLaunchKernelGGL(fn, grid, dim3(kSelThreads), kSelLdsBytes, s, static_cast<const T*>(logits), ws, g, k);
  }
  MOJO_CHECK_LAUNCH("sampling_select");
  return MOJO_OK;
}

static int run_select_finish(const void* logits, int64_t rows, int64_t vocab, int64_t k, int64_t slices, int dtype, void* workspace,
                             FinishArgs a, const char* form, hipStream_t s) {
  const Geometry g = make_geometry(rows, vocab, k, slices);
  uint64_t* ws = static_cast<uint64_t*>(workspace);
  int rc;
  switch (dtype) {
    case MOJO_F32: rc = launch_select<float>(logits, ws, g, rows, static_cast<int>(k), s); break;
    case MOJO_F16: rc = launch_select<f16_t>(logits, ws, g, rows, static_cast<int>(k), s); break;
    default: rc = launch_select<bf16_t>(logits, ws, g, rows, static_cast<int>(k), s); break;
  }
  if (rc != MOJO_OK) return rc;
  a.ws = ws;
  a.g = g;
  a.k = static_cast<int>(k);
  a.padded = 2;
  while (a.padded < a.k) a.padded <<= 1;
  hipLaunchKernelGGL(finish_rows_kernel, dim3(static_cast<unsigned>(rows)), dim3(kRowThreads), 0, s, a);
  MOJO_CHECK_LAUNCH("sampling_finish");
  note_launch("sampling:%s:%s:slices%dx%d", form, a.nucleus ? "top_p" : "top_k", g.slices, g.sub);
  return MOJO_OK;
}

// ---- penalties and temperature --------------------------------------------------------------------------------------
struct PenaltyRow {                 // 32 bytes, built by the caller on the host (include/mojo_hip.h)
  float frequency, presence, repetition, temperature;
  int32_t flags, pad;
  const void* freq;
};
enum { PEN_FREQUENCY = 1, PEN_PRESENCE = 2, PEN_REPETITION = 4, PEN_TEMPERATURE = 8 };

// Every product, difference and quotient is rounded on its own, as the golden's separate torch operations are (the library
// is built with -ffp-contract=on, which would fuse `l - p * f`).
template <typename F>
__device__ __forceinline__ float penalise(float l, const PenaltyRow& r, const F* freq, int64_t col) {
  if (r.flags & (PEN_FREQUENCY | PEN_PRESENCE | PEN_REPETITION)) {
    const F raw = freq[col];
    const float f = static_cast<float>(raw);
    if (r.flags & PEN_FREQUENCY) l = __fsub_rn(l, __fmul_rn(r.frequency, f));
    if (r.flags & PEN_PRESENCE) l = __fsub_rn(l, __fmul_rn(r.presence, raw > F(0) ? 1.f : 0.f));
    if (r.flags & PEN_REPETITION) {
      const float sign = __fmul_rn(l, f);
      l = sign < 0.f ? __fmul_rn(l, r.repetition) : (sign > 0.f ? __fdiv_rn(l, r.repetition) : l);
    }
  }
  if (r.flags & PEN_TEMPERATURE) l = __fdiv_rn(l, r.temperature);
  return l;
}

template <typename T, typename F, int VEC>
__global__ __launch_bounds__(256) void penalties_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                        const PenaltyRow* __restrict__ table, int64_t vocab) {
  const int64_t row = blockIdx.y;
  const PenaltyRow r = table[row];
  if (r.flags == 0 && in == out) return;                         // nothing to do for this row
  const F* freq = static_cast<const F*>(r.freq);
  const int64_t n_vec = vocab / VEC;
  const T* x = in + row * vocab;
  T* y = out + row * vocab;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n_vec; i += static_cast<int64_t>(gridDim.x) * 256) {
    typename vec_of<T, VEC>::type v = load_vec<T, VEC>(x + i * VEC);
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      vset<T, VEC>(v, e, elt<T>::from_f(penalise<F>(elt<T>::to_f(vget<T, VEC>(v, e)), r, freq, i * VEC + e)));
    store_vec<T, VEC>(y + i * VEC, v);
  }
}

template <typename T, typename F>
static int launch_penalties(const void* in, void* out, const void* table, int64_t rows, int64_t vocab, hipStream_t s) {
  constexpr int WIDE = 16 / sizeof(T);
  const bool wide = vocab % WIDE == 0 && aligned_to(in, 16) && aligned_to(out, 16);
  const int64_t n_vec = wide ? vocab / WIDE : vocab;
  int64_t bx = ceil_div(n_vec, 256);
  if (bx > 1024) bx = 1024;
  const dim3 grid(static_cast<unsigned>(bx), static_cast<unsigned>(rows));
  if (wide)
    hipLaunchKernelGGL((penalties_kernel<T, F, WIDE>), grid, dim3(256), 0, s, static_cast<const T*>(in), static_cast<T*>(out),
                       static_cast<const PenaltyRow*>(table), vocab);
  else
    hipLaunchKernelGGL((penalties_kernel<T, F, 1>), grid, dim3(256), 0, s, static_cast<const T*>(in), static_cast<T*>(out),
                       static_cast<const PenaltyRow*>(table), vocab);
  MOJO_CHECK_LAUNCH("apply_penalties");
  note_launch("penalties:%s", wide ? "vec16" : "scalar");
  return MOJO_OK;
}

template <typename T>
static int launch_penalties_f(const void* in, void* out, const void* table, int64_t rows, int64_t vocab, int freq_kind, hipStream_t s) {
  switch (freq_kind) {
    case 0: return launch_penalties<T, int32_t>(in, out, table, rows, vocab, s);
    case 1: return launch_penalties<T, int64_t>(in, out, table, rows, vocab, s);
    default: return launch_penalties<T, float>(in, out, table, rows, vocab, s);
  }
}

// ---- speculative acceptance: one thread per row, left to right ----------------------------------------------------------
// The running products follow the golden's cumprod: accumulated in fp64 for fp32 inputs (fp32 for 16-bit ones) and rounded to
// the tensor's dtype at every position; the uniforms are fp32.
template <typename T>
__global__ __launch_bounds__(64) void reject_kernel(const T* __restrict__ target, const int64_t* __restrict__ tokens,
                                                    const T* __restrict__ draft, const float* __restrict__ uniforms,
                                                    int64_t* __restrict__ next_tokens, void* __restrict__ accepted, int64_t batch,
                                                    int64_t steps, int64_t vocab, int joint) {
  typedef typename std::conditional<std::is_same<T, float>::value, double, float>::type acc_t;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
  if (row >= batch) return;
  acc_t pi = 1;
  double run_u = 1.0;
  int64_t first_rejected = steps;
  int last_kept = 0;
  for (int64_t j = 0; j < steps; ++j) {
    const int64_t tok = tokens[row * steps + j];
    next_tokens[row * (steps + 1) + j] = tok;
    const bool inside = tok >= 0 && tok < vocab;                 // (the golden's gather raises; here the ratio reads as 0)
    const float t = inside ? elt<T>::to_f(target[(row * (steps + 1) + j) * vocab + tok]) : 0.f;
    const float ratio = elt<T>::to_f(elt<T>::from_f(__fdiv_rn(t, elt<T>::to_f(draft[row * steps + j]))));
    if (!joint) {
      if (first_rejected == steps && ratio < uniforms[row]) first_rejected = j;
    } else {
      const float clamped = ratio < 0.f ? 0.f : (ratio > 1.f ? 1.f : ratio);      // keeps a NaN, as torch.clamp does
      pi *= static_cast<acc_t>(clamped);
      run_u *= static_cast<double>(uniforms[row * steps + j]);
      const float lhs = elt<T>::to_f(elt<T>::from_f(static_cast<float>(pi)));
      if (!(lhs < static_cast<float>(run_u))) last_kept = static_cast<int>(j) + 1;
    }
  }
  next_tokens[row * (steps + 1) + steps] = 0;
  if (joint) static_cast<int32_t*>(accepted)[row] = last_kept;
  else static_cast<int64_t*>(accepted)[row] = first_rejected;
}

}  // namespace sampling
}  // namespace mojo

using namespace mojo;
using namespace mojo::sampling;

extern "C" int64_t mojo_hip_sampling_max_k(void) { return kMaxK; }

extern "C" int64_t mojo_hip_sampling_workspace_bytes(int64_t rows, int64_t vocab, int64_t k, int64_t slices) {
  if (rows <= 0 || vocab <= 0 || k <= 0) return 0;
  if (k > vocab) k = vocab;
  const Geometry g = make_geometry(rows, vocab, k, slices);
  return rows * g.nseg * static_cast<int64_t>(g.kcap) * static_cast<int64_t>(sizeof(uint64_t));
}

extern "C" int mojo_hip_top_p_filter(const void* logits, void* probs, int64_t* indices, int64_t rows, int64_t vocab, int64_t k,
                                     float top_p, int64_t min_tokens_to_keep, float filter_value, int64_t slices, int dtype,
                                     void* workspace, int64_t workspace_bytes, mojo_stream_t stream) {
  const int rc = check_select(logits, workspace, workspace_bytes, rows, vocab, k, min_tokens_to_keep, slices, dtype, "top_p_filter");
  if (rc != MOJO_OK || rows == 0) return rc;
  MOJO_REQUIRE(probs && indices, MOJO_EINVAL, "top_p_filter: null output");
  FinishArgs a{};
  a.top_p = top_p;
  a.filter_value = filter_value;
  a.min_keep = static_cast<int>(min_tokens_to_keep);
  a.nucleus = 1;
  a.probs = probs;
  a.indices = indices;
  a.dtype = dtype;
  return run_select_finish(logits, rows, vocab, k, slices, dtype, workspace, a, "filter", static_cast<hipStream_t>(stream));
}

extern "C" int mojo_hip_sample_with_uniforms(const void* logits, const float* uniforms, float* next_probs, int64_t* next_tokens,
                                             int64_t rows, int64_t vocab, int64_t k, int nucleus, float top_p,
                                             int64_t min_tokens_to_keep, float filter_value, int64_t slices, int dtype,
                                             void* workspace, int64_t workspace_bytes, mojo_stream_t stream) {
  const int rc = check_select(logits, workspace, workspace_bytes, rows, vocab, k, min_tokens_to_keep, slices, dtype, "sample_with_uniforms");
  if (rc != MOJO_OK || rows == 0) return rc;
  MOJO_REQUIRE(uniforms && next_probs && next_tokens, MOJO_EINVAL, "sample_with_uniforms: null pointer");
  FinishArgs a{};
  a.top_p = top_p;
  a.filter_value = filter_value;
  a.min_keep = static_cast<int>(min_tokens_to_keep);
  a.nucleus = nucleus ? 1 : 0;
  a.uniforms = uniforms;
  a.next_prob = next_probs;
  a.next_token = next_tokens;
  return run_select_finish(logits, rows, vocab, k, slices, dtype, workspace, a, "sample", static_cast<hipStream_t>(stream));
}

extern "C" int mojo_hip_apply_penalties(const void* logits, void* out, const void* row_table, int64_t rows, int64_t vocab, int dtype,
                                        int freq_kind, mojo_stream_t stream) {
  if (rows == 0 || vocab == 0) return MOJO_OK;
  MOJO_REQUIRE(logits && out && row_table && rows > 0 && vocab > 0 && rows < 65536, MOJO_EINVAL, "apply_penalties: bad arguments");
  MOJO_REQUIRE(freq_kind >= 0 && freq_kind <= 2, MOJO_EINVAL, "apply_penalties: freq_kind %d (0 int32, 1 int64, 2 fp32)", freq_kind);
  MOJO_REQUIRE(aligned_to(row_table, 8), MOJO_EINVAL, "apply_penalties: the row table must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MOJO_F32: return launch_penalties_f<float>(logits, out, row_table, rows, vocab, freq_kind, s);
    case MOJO_F16: return launch_penalties_f<f16_t>(logits, out, row_table, rows, vocab, freq_kind, s);
    case MOJO_BF16: return launch_penalties_f<bf16_t>(logits, out, row_table, rows, vocab, freq_kind, s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "apply_penalties: dtype %d not supported", dtype);
  }
}

extern "C" int mojo_hip_reject_sampling(const void* target_probs, const int64_t* draft_tokens, const void* draft_probs,
                                        const float* uniforms, int64_t* next_tokens, void* accepted_len, int64_t batch,
                                        int64_t steps, int64_t vocab, int joint, int dtype, mojo_stream_t stream) {
  if (batch == 0) return MOJO_OK;
  MOJO_REQUIRE(batch > 0 && steps >= 0 && vocab > 0, MOJO_EINVAL, "reject_sampling: bad sizes");
  MOJO_REQUIRE(target_probs && next_tokens && accepted_len && (steps == 0 || (draft_tokens && draft_probs && uniforms)), MOJO_EINVAL,
               "reject_sampling: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(ceil_div(batch, 64)));
#define REJECT(T)                                                                                                          \
  hipLaunchKernelGGL(reject_kernel<T>, grid, dim3(64), 0, s, static_cast<const T*>(target_probs), draft_tokens,            \
                     static_cast<const T*>(draft_probs), uniforms, next_tokens, accepted_len, batch, steps, vocab, joint)
  switch (dtype) {
    case MOJO_F32: REJECT(float); break;
    case MOJO_F16: REJECT(f16_t); break;
    case MOJO_BF16: REJECT(bf16_t); break;
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "reject_sampling: dtype %d not supported", dtype);
  }
#undef REJECT
  MOJO_CHECK_LAUNCH("reject_sampling");
  note_launch("reject:%s", joint ? "joint" : "single");
  return MOJO_OK;
}
