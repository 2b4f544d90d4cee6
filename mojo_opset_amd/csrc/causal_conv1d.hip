// The short-convolution ops (SHORT_CONV_OPS): the depthwise causal convolution of width 2..4 in front of a linear-attention or
// state-space mixer (MojoCausalConv1dUpdateState, MojoCausalConv1d), forward only.
//
//   cat = [state_in (S columns, or S zeros) | x (T columns)]            per (sequence, channel)
//   out[t]       = act(bias + sum_k w[k] * cat[S + t - (W - 1) + k])    k = 0 .. W - 1
//   state_out[j] = cat[T + j]                                           j = 0 .. S - 1
//
// Arithmetic is fp32 in one fixed order: acc = bias (or +0.0), then acc = acc + w[k] * input for k = 0 .. W - 1, the product and
// the sum rounded on their own (__fmul_rn / __fadd_rn: the unit is built with -ffp-contract=on), SiLU on the fp32 accumulator
// (activation_math.h: the function mojo_hip_activation applies), one rounding to storage, then the optional residual added to
// the ROUNDED value (a second rounding, as the reference does).
//
// Pure HBM streaming.  Two layouts, chosen by which stride of x is 1:
//   channel-contiguous  a thread owns one vector of channels and walks a run of kRunTokens consecutive tokens with the last
//                       W - 1 inputs in registers; taps and bias stay in registers; every x is read once, apart from a W - 1
//                       token halo at a run's start.  Packed sequences: the runs cut the packed axis at fixed positions and a
//                       thread finds its first token's sequence in cu_seqlens by a binary search, then follows the bounds as
//                       it walks; at a sequence start the window is reloaded from that sequence's state (or zeros), so no
//                       tap ever reads the previous sequence.  A bound is clamped into [0, tokens] and every token is checked
//                       against its sequence, so a malformed cu_seqlens cannot index outside x.  The search reads the raw
//                       values and assumes them ascending: with a cu_seqlens that is not, WHICH sequence a token is given to
//                       (or whether it gets zeros) is undefined; only memory safety holds.
//   time-contiguous     T <= kRowThreadMaxT (decode): one thread per (sequence, channel) row, so a wave's state and x accesses
//                       are contiguous across channels.  Longer rows: 16-byte vectors along time; T and the row base are in
//                       general unaligned, so every row peels its own head and tail by elements; a vector's W - 1 halo is
//                       re-read by elements (cache hits: its neighbour's vector).
//
// The in-place state (state_out == state_in, MojoCausalConv1dUpdateState).  A row of the state is read and written by ONE
// THREAD, in program order: in the channel form the thread of the sequence's first run (a later run starts at token
// kRunTokens >= W - 1 and never reaches the state), in the long time form the thread of the row's slot 0, which takes the
// head elements, vector 0, the tail elements and then the state (a later vector starts at or past W - 1), in the short time
// form the row's only thread.  That thread reads what it needs of the old state for its outputs first; the new state's
// column j is old column T + j (read before column T + j is written: j ascends) or x[T + j - S], re-read from the input.
// In the packed channel form the states are written by jobs of their own (a sequence may have no token at all), which read
// state_in while the run jobs do: there state_out must not overlap state_in (the entry point refuses the same pointer).
#include "activation_math.h"
#include "common.h"

namespace mojo {

namespace {

constexpr int kBlock = 256;
constexpr int kRunTokens = 32;            // channel form: tokens a thread walks; the halo re-read is (W - 1) / 32 of x
constexpr int kRowThreadMaxT = 16;        // time form: rows up to this length take one thread each
constexpr int kMaxState = 8;

struct ConvArgs {
  const void* x;
  const void* weight;
  const void* bias;
  const void* residual;
  const void* state_in;
  void* state_out;
  void* out;
  const void* cu;                          // nullptr: batched
  int cu_i64;
  int64_t batch, seq_len, dim;             // packed: sequences, packed tokens
  int64_t sxb, sxt, sxd, sob, sot, sod, srb, srt, srd;
  int64_t sib, sid, stb, std_;             // state_in / state_out (batch, dim) strides
  int state_len, silu;
};

template <typename T, int VEC>
__device__ __forceinline__ void silu_all(float (&y)[VEC]) {
  if constexpr (VEC > 1) {
#pragma unroll
    for (int e = 0; e < VEC; e += 2) {
      const f32x2 r = activate_pair<T, ACT_SILU>(f32x2{y[e], y[e + 1]});
      y[e] = r[0];
      y[e + 1] = r[1];
    }
  } else {
    y[0] = activate<T, ACT_SILU>(y[0]);
  }
}

// one rounding to storage, then the residual on the rounded value
template <typename T>
__device__ __forceinline__ T to_storage(float y, const T* res) {
  T o = elt<T>::from_f(y);
  if (res) o = elt<T>::from_f(__fadd_rn(elt<T>::to_f(o), elt<T>::to_f(*res)));
  return o;
}

__device__ __forceinline__ int64_t cu_at(const ConvArgs& a, int64_t i) {
  return a.cu_i64 ? static_cast<const int64_t*>(a.cu)[i] : static_cast<int64_t>(static_cast<const int32_t*>(a.cu)[i]);
}

// [bos, eos) of sequence seq, clamped into [0, tokens] and to eos >= bos
__device__ __forceinline__ void seq_bounds(const ConvArgs& a, int64_t seq, int64_t& bos, int64_t& eos) {
  int64_t b = cu_at(a, seq), e = cu_at(a, seq + 1);
  b = b < 0 ? 0 : (b > a.seq_len ? a.seq_len : b);
  e = e < b ? b : (e > a.seq_len ? a.seq_len : e);
  bos = b;
  eos = e;
}

// ---- the channel-contiguous form ---------------------------------------------------------------------------------------

// the input at position pos of a sequence (pos < 0: column S + pos of its state, zeros without one), channels c .. c + VEC.
// xs: the sequence's token 0 at channel c; si: the state row of channel c or nullptr
template <typename T, int VEC>
__device__ __forceinline__ void channel_input(const ConvArgs& a, const T* xs, const T* si, int64_t pos, float (&v)[VEC]) {
  if (pos >= 0) {
    const typename vec_of<T, VEC>::type raw = load_vec<T, VEC>(xs + pos * a.sxt);
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = elt<T>::to_f(vget<T, VEC>(raw, e));
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = si ? elt<T>::to_f(si[e * a.sid + a.state_len + pos]) : 0.f;
  }
}

// state_out[seq][c .. c + VEC][j] = cat[len + j]: the old state's column len + j, or x[len + j - S].  j ascends, so with
// state_out == state_in column len + j is read before it is written (len == 0 rewrites every column with itself)
template <typename T, int VEC>
__device__ __forceinline__ void channel_state(const ConvArgs& a, int64_t seq, int64_t c, const T* xs, int64_t len) {
  const int S = a.state_len;
  const T* si = a.state_in ? static_cast<const T*>(a.state_in) + seq * a.sib + c * a.sid : nullptr;
  T* so = static_cast<T*>(a.state_out) + seq * a.stb + c * a.std_;
  for (int j = 0; j < S; ++j) {
    const int64_t i = len + j;
    if (i >= S) {
      const typename vec_of<T, VEC>::type raw = load_vec<T, VEC>(xs + (i - S) * a.sxt);
#pragma unroll
      for (int e = 0; e < VEC; ++e) so[e * a.std_ + j] = vget<T, VEC>(raw, e);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) so[e * a.std_ + j] = si ? si[e * a.sid + i] : elt<T>::from_f(0.f);
    }
  }
}

template <typename T, int VEC, int W>
__global__ __launch_bounds__(kBlock) void conv_channel_kernel(ConvArgs a, int64_t n_cvec, int64_t runs_per_seq, int64_t n_runs,
                                                              int64_t n_jobs) {
  typedef typename vec_of<T, VEC>::type V;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t job = g / n_cvec;
  if (job >= n_jobs) return;
  const int64_t c = (g - job * n_cvec) * VEC;
  const bool packed = a.cu != nullptr;
  const T* x = static_cast<const T*>(a.x) + c;

  if (job >= n_runs) {                                              // packed: the state of sequence job - n_runs
    const int64_t seq = job - n_runs;
    int64_t bos, eos;
    seq_bounds(a, seq, bos, eos);
    channel_state<T, VEC>(a, seq, c, x + bos * a.sxt, eos - bos);
    return;
  }

  float w[W][VEC], bias[VEC];
  {
    const T* wt = static_cast<const T*>(a.weight) + c * W;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
#pragma unroll
      for (int k = 0; k < W; ++k) w[k][e] = elt<T>::to_f(wt[e * W + k]);
      bias[e] = a.bias ? elt<T>::to_f(static_cast<const T*>(a.bias)[c + e]) : 0.f;
    }
  }

  // tokens [first, first + n) of the time axis that `x`, `out` and `res` are indexed along: a sequence's own positions
  // (batched, bos = 0) or the packed axis
  int64_t seq, bos, eos, first, n, n_seq;
  T* out = static_cast<T*>(a.out) + c;
  const T* res = a.residual ? static_cast<const T*>(a.residual) + c : nullptr;
  if (packed) {
    first = job * kRunTokens;
    n = a.seq_len - first < kRunTokens ? a.seq_len - first : kRunTokens;
    n_seq = a.batch;
    int64_t lo = 0, hi = n_seq;                                     // the last sequence whose raw start is <= first
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (cu_at(a, mid) <= first) lo = mid; else hi = mid;
    }
    seq = lo;
    bos = eos = 0;
    if (n_seq > 0) seq_bounds(a, seq, bos, eos);
  } else {
    seq = job / runs_per_seq;
    first = (job - seq * runs_per_seq) * kRunTokens;
    n = a.seq_len - first < kRunTokens ? a.seq_len - first : kRunTokens;
    n_seq = seq + 1;
    bos = 0;
    eos = a.seq_len;
    x += seq * a.sxb;
    out += seq * a.sob;
    if (res) res += seq * a.srb;
  }

  float win[W - 1][VEC];
  bool reload = true;
  for (int64_t i = 0; i < n; i += 4) {
    V raw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u < n) raw[u] = load_vec<T, VEC>(x + (first + i + u) * a.sxt);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + u >= n) break;
      const int64_t t = first + i + u;
      while (seq < n_seq && t >= eos) {                             // packed: follow the bounds (zero-length sequences too)
        ++seq;
        reload = true;
        if (seq < n_seq) seq_bounds(a, seq, bos, eos);
      }
      V o;
      if (seq >= n_seq || t < bos) {                                // a token outside every sequence: zeros
#pragma unroll
        for (int e = 0; e < VEC; ++e) vset<T, VEC>(o, e, elt<T>::from_f(0.f));
        reload = true;
      } else {
        if (reload) {                                               // a run's or a sequence's start: the W - 1 inputs before t
          const T* si = a.state_in ? static_cast<const T*>(a.state_in) + seq * a.sib + c * a.sid : nullptr;
#pragma unroll
          for (int j = 0; j < W - 1; ++j) channel_input<T, VEC>(a, x + bos * a.sxt, si, t - bos - (W - 1) + j, win[j]);
          reload = false;
        }
        float cur[VEC], acc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          cur[e] = elt<T>::to_f(vget<T, VEC>(raw[u], e));
          acc[e] = bias[e];
#pragma unroll
          for (int k = 0; k < W - 1; ++k) acc[e] = __fadd_rn(acc[e], __fmul_rn(w[k][e], win[k][e]));
          acc[e] = __fadd_rn(acc[e], __fmul_rn(w[W - 1][e], cur[e]));
#pragma unroll
          for (int k = 0; k + 1 < W - 1; ++k) win[k][e] = win[k + 1][e];
          win[W - 2][e] = cur[e];
        }
        if (a.silu) silu_all<T, VEC>(acc);
        V r;
        if (res) r = load_vec<T, VEC>(res + t * a.srt);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const T re = res ? vget<T, VEC>(r, e) : elt<T>::from_f(0.f);
          vset<T, VEC>(o, e, to_storage<T>(acc[e], res ? &re : nullptr));
        }
      }
      store_vec<T, VEC>(out + t * a.sot, o);
    }
  }
  // batched: the thread of a sequence's first run read its old state above; it alone writes the new one
  if (!packed && first == 0 && a.state_out) channel_state<T, VEC>(a, seq, c, x, a.seq_len);
}

// ---- the time-contiguous forms -----------------------------------------------------------------------------------------

template <typename T>
__device__ __forceinline__ void time_row(const ConvArgs& a, int64_t row, const T*& x, const T*& res, const T*& si, T*& so, T*& out) {
  const int64_t b = row / a.dim, d = row - b * a.dim;
  x = static_cast<const T*>(a.x) + b * a.sxb + d * a.sxd;
  out = static_cast<T*>(a.out) + b * a.sob + d * a.sod;
  res = a.residual ? static_cast<const T*>(a.residual) + b * a.srb + d * a.srd : nullptr;
  si = a.state_in ? static_cast<const T*>(a.state_in) + b * a.sib + d * a.sid : nullptr;
  so = a.state_out ? static_cast<T*>(a.state_out) + b * a.stb + d * a.std_ : nullptr;
}

template <typename T>
__device__ __forceinline__ float time_input(const T* x, const T* si, int S, int64_t pos) {
  if (pos >= 0) return elt<T>::to_f(x[pos]);
  return si ? elt<T>::to_f(si[S + pos]) : 0.f;
}

// the new state of a row; j ascends (see channel_state)
template <typename T>
__device__ __forceinline__ void time_state(const T* x, const T* si, T* so, int S, int64_t len) {
  for (int j = 0; j < S; ++j) {
    const int64_t i = len + j;
    so[j] = i >= S ? x[i - S] : (si ? si[i] : elt<T>::from_f(0.f));
  }
}

template <typename T, int W>
__device__ __forceinline__ void load_taps(const ConvArgs& a, int64_t d, float (&w)[W], float& bias) {
#pragma unroll
  for (int k = 0; k < W; ++k) w[k] = elt<T>::to_f(static_cast<const T*>(a.weight)[d * W + k]);
  bias = a.bias ? elt<T>::to_f(static_cast<const T*>(a.bias)[d]) : 0.f;
}

// out[t] of a row by elements
template <typename T, int W>
__device__ __forceinline__ void time_element(const ConvArgs& a, const T* x, const T* res, const T* si, T* out, const float (&w)[W],
                                             float bias, int64_t t) {
  float acc = bias;
#pragma unroll
  for (int k = 0; k < W; ++k) acc = __fadd_rn(acc, __fmul_rn(w[k], time_input<T>(x, si, a.state_len, t - (W - 1) + k)));
  if (a.silu) acc = activate<T, ACT_SILU>(acc);
  out[t] = to_storage<T>(acc, res ? res + t : nullptr);
}

// T <= kRowThreadMaxT: one thread per row
template <typename T, int W>
__global__ __launch_bounds__(kBlock) void conv_time_row_kernel(ConvArgs a, int64_t rows) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (row >= rows) return;
  const T *x, *res, *si;
  T *so, *out;
  time_row<T>(a, row, x, res, si, so, out);
  float w[W], bias;
  load_taps<T, W>(a, row % a.dim, w, bias);
  float win[W - 1];
#pragma unroll
  for (int j = 0; j < W - 1; ++j) win[j] = time_input<T>(x, si, a.state_len, j - (W - 1));
  for (int64_t t = 0; t < a.seq_len; ++t) {
    const float cur = elt<T>::to_f(x[t]);
    float acc = bias;
#pragma unroll
    for (int k = 0; k < W - 1; ++k) acc = __fadd_rn(acc, __fmul_rn(w[k], win[k]));
    acc = __fadd_rn(acc, __fmul_rn(w[W - 1], cur));
#pragma unroll
    for (int k = 0; k + 1 < W - 1; ++k) win[k] = win[k + 1];
    win[W - 2] = cur;
    if (a.silu) acc = activate<T, ACT_SILU>(acc);
    out[t] = to_storage<T>(acc, res ? res + t : nullptr);
  }
  if (so) time_state<T>(x, si, so, a.state_len, a.seq_len);
}

// T > kRowThreadMaxT: a row is `slots` slots; slot v takes the row's aligned vector v (VEC elements from element head + v * VEC,
// head = the elements in front of the row's first 16-byte boundary; x, out and residual rows are misaligned alike, the host
// checked); slot 0 also takes the head and tail elements and, last, the state.  VEC == 1: the first W - 1 elements are the
// head, so that slot 0 alone reads the state.
template <typename T, int VEC, int W>
__global__ __launch_bounds__(kBlock) void conv_time_vec_kernel(ConvArgs a, int64_t rows, int64_t slots) {
  typedef typename vec_of<T, VEC>::type V;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t row = g / slots;
  if (row >= rows) return;
  const int64_t v = g - row * slots;
  const T *x, *res, *si;
  T *so, *out;
  time_row<T>(a, row, x, res, si, so, out);
  const int64_t len = a.seq_len;
  int64_t head = VEC > 1 ? static_cast<int64_t>((VEC - (reinterpret_cast<uintptr_t>(x) / sizeof(T)) % VEC) % VEC) : W - 1;
  if (head > len) head = len;
  const int64_t nv = (len - head) / VEC, tail = head + nv * VEC;
  if (v >= nv && v != 0) return;
  float w[W], bias;
  load_taps<T, W>(a, row % a.dim, w, bias);
  if (v < nv) {
    const int64_t t0 = head + v * VEC;
    float in[VEC + W - 1];
    const V raw = load_vec<T, VEC>(x + t0);
#pragma unroll
    for (int j = 0; j < W - 1; ++j) in[j] = time_input<T>(x, si, a.state_len, t0 - (W - 1) + j);
#pragma unroll
    for (int e = 0; e < VEC; ++e) in[W - 1 + e] = elt<T>::to_f(vget<T, VEC>(raw, e));
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[e] = bias;
#pragma unroll
      for (int k = 0; k < W; ++k) acc[e] = __fadd_rn(acc[e], __fmul_rn(w[k], in[e + k]));
    }
    if (a.silu) silu_all<T, VEC>(acc);
    V r, o;
    if (res) r = load_vec<T, VEC>(res + t0);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const T re = res ? vget<T, VEC>(r, e) : elt<T>::from_f(0.f);
      vset<T, VEC>(o, e, to_storage<T>(acc[e], res ? &re : nullptr));
    }
    store_vec<T, VEC>(out + t0, o);
  }
  if (v == 0) {
    for (int64_t t = 0; t < head; ++t) time_element<T, W>(a, x, res, si, out, w, bias, t);
    for (int64_t t = tail; t < len; ++t) time_element<T, W>(a, x, res, si, out, w, bias, t);
    if (so) time_state<T>(x, si, so, a.state_len, len);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

static bool mult(int64_t v, int64_t m) { return v % m == 0; }

// the widest channel vector (in elements) that dim, the bases and every stride in use allow
template <typename T>
static int channel_vec(const ConvArgs& a) {
  const bool packed = a.cu != nullptr;
  for (int bytes = 16; bytes > static_cast<int>(sizeof(T)); bytes /= 2) {
    const int v = bytes / static_cast<int>(sizeof(T));
    bool ok = mult(a.dim, v) && aligned_to(a.x, bytes) && aligned_to(a.out, bytes) && (!a.residual || aligned_to(a.residual, bytes));
    if (a.seq_len > 1) ok = ok && mult(a.sxt, v) && mult(a.sot, v) && (!a.residual || mult(a.srt, v));
    if (!packed && a.batch > 1) ok = ok && mult(a.sxb, v) && mult(a.sob, v) && (!a.residual || mult(a.srb, v));
    if (ok) return v;
  }
  return 1;
}

// 16-byte vectors along time need the rows of x, out and residual misaligned alike
template <typename T>
static bool time_rows_alike(const ConvArgs& a) {
  const int v = 16 / static_cast<int>(sizeof(T));
  auto alike = [&](const void* p, int64_t sb, int64_t sd) {
    const intptr_t diff = reinterpret_cast<intptr_t>(p) - reinterpret_cast<intptr_t>(a.x);
    return diff % 16 == 0 && (a.batch <= 1 || mult(sb - a.sxb, v)) && (a.dim <= 1 || mult(sd - a.sxd, v));
  };
  return alike(a.out, a.sob, a.sod) && (!a.residual || alike(a.residual, a.srb, a.srd));
}

template <typename T, int VEC, int W>
static int launch_channel(const ConvArgs& a, hipStream_t s) {
  const bool packed = a.cu != nullptr;
  const int64_t n_cvec = a.dim / VEC;
  const int64_t runs_per_seq = ceil_div(a.seq_len, kRunTokens);
  const int64_t n_runs = packed ? runs_per_seq : a.batch * runs_per_seq;
  const int64_t n_jobs = n_runs + (packed && a.state_out ? a.batch : 0);
  const int64_t blocks = ceil_div(n_jobs * n_cvec, kBlock);
  if (blocks == 0) return MOJO_OK;
  MOJO_REQUIRE(blocks < (int64_t{1} << 31), MOJO_EUNSUPPORTED, "causal_conv1d: %lld workgroups", static_cast<long long>(blocks));
  hipLaunchKernelGGL((conv_channel_kernel<T, VEC, W>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s, a, n_cvec,
                     runs_per_seq, n_runs, n_jobs);
  MOJO_CHECK_LAUNCH("causal_conv1d");
  note_launch("causal_conv1d:channel:vec%d:%s", VEC, packed ? "packed" : "batched");
  return MOJO_OK;
}

template <typename T, int W>
static int launch_width(const ConvArgs& a, hipStream_t s) {
  constexpr int WIDE = 16 / sizeof(T);
  if (a.sxt == 1 && !a.cu) {                                        // time-contiguous
    const int64_t rows = a.batch * a.dim;
    MOJO_REQUIRE(rows < (int64_t{1} << 38), MOJO_EUNSUPPORTED, "causal_conv1d: %lld rows", static_cast<long long>(rows));
    if (a.seq_len <= kRowThreadMaxT) {
      hipLaunchKernelGGL((conv_time_row_kernel<T, W>), dim3(static_cast<unsigned>(ceil_div(rows, kBlock))), dim3(kBlock), 0, s, a, rows);
      MOJO_CHECK_LAUNCH("causal_conv1d");
      note_launch("causal_conv1d:time:row");
      return MOJO_OK;
    }
    const bool wide = time_rows_alike<T>(a);
    const int64_t slots = wide ? a.seq_len / WIDE : a.seq_len;
    const int64_t blocks = ceil_div(rows * slots, kBlock);
    MOJO_REQUIRE(blocks < (int64_t{1} << 31), MOJO_EUNSUPPORTED, "causal_conv1d: %lld workgroups", static_cast<long long>(blocks));
    if (wide) hipLaunchKernelGGL((conv_time_vec_kernel<T, WIDE, W>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s, a, rows, slots);
    else hipLaunchKernelGGL((conv_time_vec_kernel<T, 1, W>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s, a, rows, slots);
    MOJO_CHECK_LAUNCH("causal_conv1d");
    note_launch("causal_conv1d:time:vec%d", wide ? WIDE : 1);
    return MOJO_OK;
  }
  const int vec = channel_vec<T>(a);
  if (vec == WIDE) return launch_channel<T, WIDE, W>(a, s);
  if constexpr (WIDE >= 4) {
    if (vec == WIDE / 2) return launch_channel<T, WIDE / 2, W>(a, s);
  }
  if constexpr (WIDE >= 8) {
    if (vec == WIDE / 4) return launch_channel<T, WIDE / 4, W>(a, s);
  }
  return launch_channel<T, 1, W>(a, s);
}

template <typename T>
static int launch_dtype(const ConvArgs& a, int width, hipStream_t s) {
  switch (width) {
    case 2: return launch_width<T, 2>(a, s);
    case 3: return launch_width<T, 3>(a, s);
    default: return launch_width<T, 4>(a, s);
  }
}

}  // namespace

}  // namespace mojo

using namespace mojo;

extern "C" int64_t mojo_hip_causal_conv1d_run_tokens(void) { return kRunTokens; }
extern "C" int64_t mojo_hip_causal_conv1d_row_thread_max_t(void) { return kRowThreadMaxT; }

extern "C" int mojo_hip_causal_conv1d(const void* x, const void* weight, const void* bias, const void* residual, const void* state_in,
                                      void* state_out, void* out, const void* cu_seqlens, int cu_i64, int64_t batch, int64_t seq_len,
                                      int64_t dim, int64_t width, int64_t state_len, int64_t x_batch_stride, int64_t x_time_stride,
                                      int64_t x_dim_stride, int64_t out_batch_stride, int64_t out_time_stride, int64_t out_dim_stride,
                                      int64_t res_batch_stride, int64_t res_time_stride, int64_t res_dim_stride,
                                      int64_t state_in_batch_stride, int64_t state_in_dim_stride, int64_t state_out_batch_stride,
                                      int64_t state_out_dim_stride, int silu, int dtype, mojo_stream_t stream) {
  MOJO_REQUIRE(width >= 2 && width <= 4, MOJO_EUNSUPPORTED, "causal_conv1d: width %lld (2, 3 and 4 are compiled)",
               static_cast<long long>(width));
  MOJO_REQUIRE(state_len >= width - 1 && state_len <= kMaxState, MOJO_EUNSUPPORTED,
               "causal_conv1d: state_len %lld outside [width - 1, %d]", static_cast<long long>(state_len), kMaxState);
  MOJO_REQUIRE(batch >= 0 && seq_len >= 0 && dim >= 0, MOJO_EINVAL, "causal_conv1d: negative size");
  const bool packed = cu_seqlens != nullptr;
  if (dim == 0 || (seq_len == 0 && !(packed && state_out)) || (batch == 0 && !packed)) return MOJO_OK;
  MOJO_REQUIRE(weight && ((x && out) || seq_len == 0), MOJO_EINVAL, "causal_conv1d: null pointer");
  MOJO_REQUIRE(!(packed && state_out && state_out == state_in), MOJO_EINVAL,
               "causal_conv1d: packed sequences need a state_out that does not overlap state_in");
  ConvArgs a;
  a.x = x; a.weight = weight; a.bias = bias; a.residual = residual; a.state_in = state_in; a.state_out = state_out; a.out = out;
  a.cu = cu_seqlens; a.cu_i64 = cu_i64;
  a.batch = batch; a.seq_len = seq_len; a.dim = dim;
  a.sxb = x_batch_stride; a.sxt = x_time_stride; a.sxd = x_dim_stride;
  a.sob = out_batch_stride; a.sot = out_time_stride; a.sod = out_dim_stride;
  a.srb = res_batch_stride; a.srt = res_time_stride; a.srd = res_dim_stride;
  a.sib = state_in_batch_stride; a.sid = state_in_dim_stride; a.stb = state_out_batch_stride; a.std_ = state_out_dim_stride;
  a.state_len = static_cast<int>(state_len); a.silu = silu ? 1 : 0;
  if (a.sxt == 1 && !packed) {
    MOJO_REQUIRE(a.sot == 1 && (!residual || a.srt == 1), MOJO_EINVAL,
                 "causal_conv1d: a time-contiguous x needs time-contiguous out and residual");
  } else {
    MOJO_REQUIRE(a.sxd == 1, MOJO_EINVAL, "causal_conv1d: x must be dense along time (batched) or along the channels");
    MOJO_REQUIRE(a.sod == 1 && (!residual || a.srd == 1), MOJO_EINVAL,
                 "causal_conv1d: a channel-contiguous x needs channel-contiguous out and residual");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case MOJO_F32: return launch_dtype<float>(a, static_cast<int>(width), s);
    case MOJO_F16: return launch_dtype<f16_t>(a, static_cast<int>(width), s);
    case MOJO_BF16: return launch_dtype<bf16_t>(a, static_cast<int>(width), s);
    default: MOJO_REQUIRE(false, MOJO_EUNSUPPORTED, "causal_conv1d: dtype %d not supported", dtype);
  }
}
