// The gated delta rule (LINEAR_ATTN_OPS: MojoGatedDeltaRule, MojoGatedDeltaRuleUpdateState): a linear recurrence
// over an fp32 state S [Dk][Dv] per (sequence, value head),
//     S = exp(g_t) S;   d = beta_t (v_t - S^T k_t);   S += k_t (x) d;   o_t = scale S^T q_t.
//
// gd_prefill_kernel: the chunked (WY) form on the matrix cores.  One workgroup of four waves owns (sequence, value head, slice
// of DVS state columns) and walks the sequence in chunks of 64 tokens with its state slice in MFMA accumulators.  With
// G_i = sum_{j<=i} g_j inside the chunk (every exponent below is <= 0; nothing above the diagonal is ever formed):
//     A   = strict_lower(beta_i (K K^T)_ij exp(G_i - G_j))            Tm = (I + A)^-1
//     R   = beta (.) (V - exp(G) (.) (K S))                           Vn = Tm R        (= U - W S of the textbook form:
//                                                                       Tm (beta V) - Tm (beta exp(G) K) S, W never formed)
//     O   = scale [ exp(G) (.) (Q S) + lower_incl(Q K^T (.) Gamma) Vn ]
//     S   = exp(G_C) S + (exp(G_C - G) (.) K)^T Vn
// Every matrix product is v_mfma_f32_16x16x32_bf16 on bf16 operands read from LDS with fp32 accumulators; Gamma, beta and the
// masks are applied to accumulators; Tm is inverted in fp32 (16 x 16 diagonal blocks by forward substitution, then block
// rows) and rounded once.  A tail chunk is padded with k = q = v = 0, beta = 0, g = 0 rows, which leave the state untouched.
//
// gd_update_kernel: 1..8 tokens, a streaming kernel.  One workgroup owns (sequence, head, 32 state columns), holds its rows in
// registers as 16-byte vectors, and per token reduces the partial S^T k and S^T q over the row segments through LDS in one
// fixed order.  The state is read once and written once.  S^T k and d are fp64 (d is a difference of nearly equal numbers once
// the state has learned the key); the decay (its factor carried as two floats) and the rank-one update round each state
// element once per token; S^T q is fp32, one rounding of the output.
#include "common.h"

namespace mojo {
namespace {

constexpr int GD_C = 64;                     // tokens per chunk
constexpr int GD_THREADS = 256;
constexpr int GD_TS = GD_C + 8;              // row stride (elements) of the bf16 arrays whose rows run over a chunk's tokens
constexpr int GD_AS = GD_C + 1;              // row stride (floats) of A / Tm
constexpr int GD_CUS = 256;
constexpr int GD_MAX_UPDATE_T = 8;
constexpr int GD_UCOLS = 32;                 // state columns per workgroup of the update kernel

struct GdArgs {
  const bf16_t *q, *k, *v;
  const void *g, *beta, *cu;
  const float* s_in;
  float* s_out;
  bf16_t* out;
  int64_t q_bs, q_ts, q_hs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, tokens;
  int hk, hv, dv, norm, gb_f32, cu_i64;
  float scale;
};

__device__ __forceinline__ float gd_load_gb(const void* p, int64_t i, int f32) {
  return f32 ? static_cast<const float*>(p)[i] : static_cast<float>(static_cast<const bf16_t*>(p)[i]);
}

// rows row0 + (lane & 15), elements k0 + 8 (lane >> 4) .. + 8 of a row-major bf16 array: the A operand of a 16 x 32 tile
// [m][k], and the B operand of a 32 x 16 tile stored as [n][k]
__device__ __forceinline__ bf16x8 gd_frag(const bf16_t* base, int stride, int row0, int k0) {
  const int lane = threadIdx.x & 63;
  return *reinterpret_cast<const bf16x8*>(base + (row0 + (lane & 15)) * stride + k0 + 8 * (lane >> 4));
}
// C[m][n] += sum_k A[m][k] B[k][n]; the lane holds n = lane & 15, m = 4 (lane >> 4) + r
__device__ __forceinline__ f32x4 gd_mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

__device__ __forceinline__ bf16x4 gd_round4(f32x4 x) {
  bf16x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = static_cast<bf16_t>(x[r]);
  return o;
}

template <int DK, int DVS>
struct GdLds {
  static constexpr int KS = DK + 8, VS = DVS + 8;
  static constexpr int kh = 0;                                   // K^ [64][KS] bf16
  static constexpr int qh = kh + GD_C * KS * 2;                   // Q^ [64][KS] bf16
  static constexpr int kdt = qh + GD_C * KS * 2;                  // (exp(G_C - G) K^)^T [DK][72] bf16
  static constexpr int st = kdt + DK * GD_TS * 2;                 // S^T [DVS][KS] bf16, the state at the chunk's start
  static constexpr int vs = st + DVS * KS * 2;                    // V [64][VS] bf16
  static constexpr int rt = vs + GD_C * VS * 2;                   // R^T [DVS][72] bf16
  static constexpr int vnt = rt + DVS * GD_TS * 2;                // Vn^T [DVS][72] bf16
  static constexpr int af = vnt + DVS * GD_TS * 2;                // A, then Tm, [64][65] fp32
  static constexpr int ms = af + GD_C * GD_AS * 4;                // one block row of products [16][65] fp32
  static constexpr int tmb = ms + 16 * GD_AS * 4;                 // Tm [64][72] bf16
  static constexpr int pb = tmb + GD_C * GD_TS * 2;               // lower_incl(Q K^T Gamma) [64][72] bf16
  static constexpr int gs = pb + GD_C * GD_TS * 2;                // G [64], beta [64] fp32
  static constexpr int bytes = gs + 2 * GD_C * 4;
};

template <int DK, int DVS>
__global__ __launch_bounds__(GD_THREADS) void gd_prefill_kernel(GdArgs a) {
  typedef GdLds<DK, DVS> Lds;
  constexpr int KS = Lds::KS, VS = Lds::VS, DTW = DK / 64 /* state row tiles per wave */, CT = DVS / 16, KST = DK / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* kh = reinterpret_cast<bf16_t*>(smem + Lds::kh);
  bf16_t* qh = reinterpret_cast<bf16_t*>(smem + Lds::qh);
  bf16_t* kdt = reinterpret_cast<bf16_t*>(smem + Lds::kdt);
  bf16_t* st = reinterpret_cast<bf16_t*>(smem + Lds::st);
  bf16_t* vs = reinterpret_cast<bf16_t*>(smem + Lds::vs);
  bf16_t* rt = reinterpret_cast<bf16_t*>(smem + Lds::rt);
  bf16_t* vnt = reinterpret_cast<bf16_t*>(smem + Lds::vnt);
  float* af = reinterpret_cast<float*>(smem + Lds::af);
  float* ms = reinterpret_cast<float*>(smem + Lds::ms);
  bf16_t* tmb = reinterpret_cast<bf16_t*>(smem + Lds::tmb);
  bf16_t* pb = reinterpret_cast<bf16_t*>(smem + Lds::pb);
  float* gs = reinterpret_cast<float*>(smem + Lds::gs);
  float* bs = gs + GD_C;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, grp = lane >> 4;
  const int slices = a.dv / DVS;
  const int sl = static_cast<int>(blockIdx.x % slices);
  const int hv = static_cast<int>((blockIdx.x / slices) % a.hv);
  const int64_t seq = blockIdx.x / (static_cast<unsigned>(slices) * a.hv);
  const int hk = hv / (a.hv / a.hk), c0 = sl * DVS;

  int64_t b = seq, t0 = 0, t1 = a.tokens;
  if (a.cu) {                                                     // packed: the bounds are read here, clamped into the buffer
    b = 0;
    t0 = a.cu_i64 ? static_cast<const int64_t*>(a.cu)[seq] : static_cast<const int32_t*>(a.cu)[seq];
    t1 = a.cu_i64 ? static_cast<const int64_t*>(a.cu)[seq + 1] : static_cast<const int32_t*>(a.cu)[seq + 1];
    t0 = t0 < 0 ? 0 : (t0 > a.tokens ? a.tokens : t0);
    t1 = t1 < t0 ? t0 : (t1 > a.tokens ? a.tokens : t1);
  }
  const int64_t len = t1 - t0;
  const bf16_t* qp = a.q + b * a.q_bs + t0 * a.q_ts + hk * a.q_hs;
  const bf16_t* kp = a.k + b * a.k_bs + t0 * a.k_ts + hk * a.k_hs;
  const bf16_t* vp = a.v + b * a.v_bs + t0 * a.v_ts + hv * a.v_hs + c0;
  const int64_t gb0 = (b * a.tokens + t0) * a.hv + hv;           // g / beta [B][T][Hv], dense
  bf16_t* op = a.out + ((b * a.tokens + t0) * a.hv + hv) * a.dv + c0;
  const int64_t s_off = ((seq * a.hv + hv) * DK) * a.dv + c0;

  // the state slice: rows d = 16 (DTW wave + x) + 4 grp + r, columns c = 16 ct + l15
  f32x4 S[DTW][CT];
#pragma unroll
  for (int x = 0; x < DTW; ++x)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 16 * (DTW * wave + x) + 4 * grp + r;
        S[x][ct][r] = a.s_in ? a.s_in[s_off + static_cast<int64_t>(d) * a.dv + 16 * ct + l15] : 0.f;
      }
  auto publish_state = [&]() {                                    // S^T in bf16: the operand of K S and Q S
#pragma unroll
    for (int x = 0; x < DTW; ++x)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        *reinterpret_cast<bf16x4*>(st + (16 * ct + l15) * KS + 16 * (DTW * wave + x) + 4 * grp) = gd_round4(S[x][ct]);
  };
  publish_state();
  for (int i = tid; i < GD_C * GD_TS / 2; i += GD_THREADS) reinterpret_cast<unsigned*>(pb)[i] = 0u;   // the tiles above the diagonal stay zero

  for (int64_t cs = 0; cs < len; cs += GD_C) {
    const int n = static_cast<int>(len - cs < GD_C ? len - cs : GD_C);
    // ---- 0: g, beta and the prefix sum of g (one wave, one token per lane)
    if (wave == 0) {
      float gsum = lane < n ? gd_load_gb(a.g, gb0 + (cs + lane) * a.hv, a.gb_f32) : 0.f;
      const float beta = lane < n ? gd_load_gb(a.beta, gb0 + (cs + lane) * a.hv, a.gb_f32) : 0.f;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const float up = __shfl_up(gsum, off);
        if (lane >= off) gsum += up;
      }
      gs[lane] = gsum;
      bs[lane] = beta;
    }
    __syncthreads();
    const float g_end = gs[GD_C - 1];
    // ---- 1: stage K^, Q^ (the l2 norm in fp32), the decayed K^ transposed, and the V slice
    {
      constexpr int LPR = DK / 8, RPP = GD_THREADS / LPR;
      const int seg = tid % LPR;
#pragma unroll
      for (int p = 0; p < GD_C / RPP; ++p) {
        const int row = p * RPP + tid / LPR;
        bf16x8 kv, qv;
#pragma unroll
        for (int e = 0; e < 8; ++e) kv[e] = qv[e] = static_cast<bf16_t>(0.f);
        if (row < n) {
          kv = *reinterpret_cast<const bf16x8*>(kp + (cs + row) * a.k_ts + seg * 8);
          qv = *reinterpret_cast<const bf16x8*>(qp + (cs + row) * a.q_ts + seg * 8);
        }
        float kf[8], qf[8], ssk = 0.f, ssq = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          kf[e] = static_cast<float>(kv[e]);
          qf[e] = static_cast<float>(qv[e]);
          ssk += kf[e] * kf[e];
          ssq += qf[e] * qf[e];
        }
        if (a.norm) {
          ssk = LPR == 16 ? row16_sum(ssk) : row8_sum(ssk);
          ssq = LPR == 16 ? row16_sum(ssq) : row8_sum(ssq);
          const float rk = __builtin_amdgcn_rsqf(ssk + 1e-6f), rq = __builtin_amdgcn_rsqf(ssq + 1e-6f);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            kf[e] *= rk;
            qf[e] *= rq;
          }
        }
        const float decay = __expf(g_end - gs[row]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          kv[e] = static_cast<bf16_t>(kf[e]);
          qv[e] = static_cast<bf16_t>(qf[e]);
          kdt[(seg * 8 + e) * GD_TS + row] = static_cast<bf16_t>(kf[e] * decay);
        }
        *reinterpret_cast<bf16x8*>(kh + row * KS + seg * 8) = kv;
        *reinterpret_cast<bf16x8*>(qh + row * KS + seg * 8) = qv;
      }
      constexpr int VPR = DVS / 8;
#pragma unroll
      for (int i = 0; i < GD_C * VPR / GD_THREADS; ++i) {
        const int idx = tid + i * GD_THREADS, row = idx / VPR, vseg = idx % VPR;
        bf16x8 vv;
#pragma unroll
        for (int e = 0; e < 8; ++e) vv[e] = static_cast<bf16_t>(0.f);
        if (row < n) vv = *reinterpret_cast<const bf16x8*>(vp + (cs + row) * a.v_ts + vseg * 8);
        *reinterpret_cast<bf16x8*>(vs + row * VS + vseg * 8) = vv;
      }
    }
    __syncthreads();
    // ---- 2a: R = beta (V - exp(G) (K^ S)), rows 16 wave .. + 16, transposed into LDS
    {
      bf16x8 ka[KST];
#pragma unroll
      for (int ks = 0; ks < KST; ++ks) ka[ks] = gd_frag(kh, KS, 16 * wave, 32 * ks);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) acc = gd_mfma(ka[ks], gd_frag(st, KS, 16 * ct, 32 * ks), acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * wave + 4 * grp + r;
          acc[r] = bs[i] * (static_cast<float>(vs[i * VS + 16 * ct + l15]) - __expf(gs[i]) * acc[r]);
        }
        *reinterpret_cast<bf16x4*>(rt + (16 * ct + l15) * GD_TS + 16 * wave + 4 * grp) = gd_round4(acc);
      }
    }
    // ---- 2b: the ten tiles on and below the diagonal of K^ K^T (-> A, fp32) and of Q^ K^T (-> P, bf16)
    for (int t = wave; t < 10; t += 4) {
      const int ti = t >= 6 ? 3 : (t >= 3 ? 2 : (t >= 1 ? 1 : 0)), tj = t - ti * (ti + 1) / 2;
      f32x4 kk = {0.f, 0.f, 0.f, 0.f}, qk = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KST; ++ks) {
        const bf16x8 kj = gd_frag(kh, KS, 16 * tj, 32 * ks);
        kk = gd_mfma(gd_frag(kh, KS, 16 * ti, 32 * ks), kj, kk);        // [m = i][n = j]
        qk = gd_mfma(kj, gd_frag(qh, KS, 16 * ti, 32 * ks), qk);        // [m = j][n = i]: four consecutive j per lane
      }
      {
        const int j = 16 * tj + l15;
        const float gj = gs[j];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * ti + 4 * grp + r;
          af[i * GD_AS + j] = j < i ? bs[i] * kk[r] * __expf(fminf(gs[i] - gj, 0.f)) : 0.f;
        }
      }
      {
        const int i = 16 * ti + l15;
        const float gi = gs[i];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * tj + 4 * grp + r;
          qk[r] = j <= i ? qk[r] * __expf(fminf(gi - gs[j], 0.f)) : 0.f;
        }
        *reinterpret_cast<bf16x4*>(pb + i * GD_TS + 16 * tj + 4 * grp) = gd_round4(qk);
      }
    }
    __syncthreads();
    // ---- 3: Tm = (I + A)^-1 in fp32, in place.  Diagonal blocks: wave w inverts block w, a lane per column
    {
      float tcol[16];
      const int base = 16 * wave;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float s = r == l15 ? 1.f : 0.f;
#pragma unroll
        for (int k2 = 0; k2 < r; ++k2) s -= af[(base + r) * GD_AS + base + k2] * tcol[k2];
        tcol[r] = s;
      }
      __syncthreads();
      if (lane < 16) {
#pragma unroll
        for (int r = 0; r < 16; ++r) af[(base + r) * GD_AS + base + l15] = tcol[r];
      }
    }
    __syncthreads();
    // block rows 1..3: M_IJ = sum_{K = J}^{I - 1} A_IK Tm_KJ, then Tm_IJ = -Tm_II M_IJ over A_IJ
    {
      const int r = tid >> 4, c = tid & 15;
      for (int bi = 1; bi < 4; ++bi) {
        for (int bj = 0; bj < bi; ++bj) {
          float m = 0.f;
          for (int k2 = 16 * bj; k2 < 16 * bi; ++k2) m += af[(16 * bi + r) * GD_AS + k2] * af[k2 * GD_AS + 16 * bj + c];
          ms[r * GD_AS + 16 * bj + c] = m;
        }
        __syncthreads();
        for (int bj = 0; bj < bi; ++bj) {
          float t = 0.f;
#pragma unroll
          for (int k2 = 0; k2 < 16; ++k2) t -= af[(16 * bi + r) * GD_AS + 16 * bi + k2] * ms[k2 * GD_AS + 16 * bj + c];
          af[(16 * bi + r) * GD_AS + 16 * bj + c] = t;
        }
        __syncthreads();
      }
    }
    {                                                             // the one rounding of Tm; blocks above the diagonal are zero
      const int row = tid >> 2, cb = tid & 3;
      bf16x8 lo, hi;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        lo[e] = static_cast<bf16_t>(cb <= (row >> 4) ? af[row * GD_AS + 16 * cb + e] : 0.f);
        hi[e] = static_cast<bf16_t>(cb <= (row >> 4) ? af[row * GD_AS + 16 * cb + 8 + e] : 0.f);
      }
      *reinterpret_cast<bf16x8*>(tmb + row * GD_TS + 16 * cb) = lo;
      *reinterpret_cast<bf16x8*>(tmb + row * GD_TS + 16 * cb + 8) = hi;
    }
    __syncthreads();
    // ---- 4: Vn = Tm R, rows 16 wave .. + 16, transposed into LDS
    {
      const bf16x8 t0f = gd_frag(tmb, GD_TS, 16 * wave, 0), t1f = gd_frag(tmb, GD_TS, 16 * wave, 32);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = gd_mfma(t0f, gd_frag(rt, GD_TS, 16 * ct, 0), acc);
        acc = gd_mfma(t1f, gd_frag(rt, GD_TS, 16 * ct, 32), acc);
        *reinterpret_cast<bf16x4*>(vnt + (16 * ct + l15) * GD_TS + 16 * wave + 4 * grp) = gd_round4(acc);
      }
    }
    __syncthreads();
    // ---- 5: O^T [c][i] for the tokens i = 16 wave + l15 (four consecutive columns per lane), then the state
    {
      const int i = 16 * wave + l15;
      const float eg = __expf(gs[i]);
      bf16x8 qb[KST];
#pragma unroll
      for (int ks = 0; ks < KST; ++ks) qb[ks] = gd_frag(qh, KS, 16 * wave, 32 * ks);
      const bf16x8 p0 = gd_frag(pb, GD_TS, 16 * wave, 0), p1 = gd_frag(pb, GD_TS, 16 * wave, 32);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KST; ++ks) acc = gd_mfma(gd_frag(st, KS, 16 * ct, 32 * ks), qb[ks], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= eg;
        acc = gd_mfma(gd_frag(vnt, GD_TS, 16 * ct, 0), p0, acc);
        acc = gd_mfma(gd_frag(vnt, GD_TS, 16 * ct, 32), p1, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= a.scale;
        if (i < n) *reinterpret_cast<bf16x4*>(op + (cs + i) * a.hv * a.dv + 16 * ct + 4 * grp) = gd_round4(acc);
      }
      const float ec = __expf(g_end);
#pragma unroll
      for (int x = 0; x < DTW; ++x) {
        const bf16x8 k0f = gd_frag(kdt, GD_TS, 16 * (DTW * wave + x), 0), k1f = gd_frag(kdt, GD_TS, 16 * (DTW * wave + x), 32);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          f32x4 acc = S[x][ct];
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] *= ec;
          acc = gd_mfma(k0f, gd_frag(vnt, GD_TS, 16 * ct, 0), acc);
          S[x][ct] = gd_mfma(k1f, gd_frag(vnt, GD_TS, 16 * ct, 32), acc);
        }
      }
    }
    __syncthreads();                                              // every read of this chunk's LDS is done
    publish_state();
  }
  if (a.s_out) {
#pragma unroll
    for (int x = 0; x < DTW; ++x)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int d = 16 * (DTW * wave + x) + 4 * grp + r;
          a.s_out[s_off + static_cast<int64_t>(d) * a.dv + 16 * ct + l15] = S[x][ct][r];
        }
  }
}

struct GdUpdateArgs {
  const void *q, *k, *v, *g, *beta;
  float* state;
  void* out;
  int64_t q_bs, q_ts, q_hs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs;
  int tokens, hk, hv, dv, norm, gb_f32;
  float scale;
};

template <typename T, int DK>
__global__ __launch_bounds__(GD_THREADS) void gd_update_kernel(GdUpdateArgs a) {
  constexpr int RPT = DK / 32;                                    // state rows per thread: row = 32 rr + seg
  __shared__ float qs[GD_MAX_UPDATE_T][DK], ks[GD_MAX_UPDATE_T][DK];
  __shared__ double ks64[GD_MAX_UPDATE_T][DK];                    // k^ for the fp64 sum S^T k^
  __shared__ __attribute__((aligned(16))) float red[4][GD_UCOLS];
  __shared__ __attribute__((aligned(16))) double red64[4][GD_UCOLS];
  typedef typename vec_of<T, 4>::type T4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cv = tid & 7, seg = tid >> 3;
  const int slices = a.dv / GD_UCOLS;
  const int c0 = static_cast<int>(blockIdx.x % slices) * GD_UCOLS + 4 * cv;
  const int hv = static_cast<int>((blockIdx.x / slices) % a.hv);
  const int64_t b = blockIdx.x / (static_cast<unsigned>(slices) * a.hv);
  const int hk = hv / (a.hv / a.hk);
  const T* qp = static_cast<const T*>(a.q) + b * a.q_bs + hk * a.q_hs;
  const T* kp = static_cast<const T*>(a.k) + b * a.k_bs + hk * a.k_hs;
  const T* vp = static_cast<const T*>(a.v) + b * a.v_bs + hv * a.v_hs + c0;
  T* op = static_cast<T*>(a.out) + ((b * a.tokens) * a.hv + hv) * a.dv + c0;
  float* sp = a.state + ((b * a.hv + hv) * DK) * a.dv + c0;

  f32x4 S[RPT];
#pragma unroll
  for (int rr = 0; rr < RPT; ++rr) S[rr] = *reinterpret_cast<const f32x4*>(sp + static_cast<int64_t>(32 * rr + seg) * a.dv);
  for (int t = wave; t < a.tokens; t += 4) {                      // q^ (fp32) and k^ (fp64) of every token: a wave per token
    float qf[DK / 64], kf[DK / 64], ssq = 0.f;
    double ssk = 0.0;
#pragma unroll
    for (int x = 0; x < DK / 64; ++x) {
      qf[x] = static_cast<float>(qp[t * a.q_ts + lane + 64 * x]);
      kf[x] = static_cast<float>(kp[t * a.k_ts + lane + 64 * x]);
      ssq += qf[x] * qf[x];
      ssk += static_cast<double>(kf[x]) * static_cast<double>(kf[x]);
    }
    float rq = 1.f;
    double rk = 1.0;
    if (a.norm) {
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) ssk += __shfl_xor(ssk, off);
      rq = __builtin_amdgcn_rsqf(wave_sum(ssq) + 1e-6f);
      rk = 1.0 / sqrt(ssk + 1e-6);
    }
#pragma unroll
    for (int x = 0; x < DK / 64; ++x) {
      const double kn = static_cast<double>(kf[x]) * rk;
      qs[t][lane + 64 * x] = qf[x] * rq;
      ks64[t][lane + 64 * x] = kn;
      ks[t][lane + 64 * x] = static_cast<float>(kn);
    }
  }
  __syncthreads();
  // sum over the 32 row segments of four column partials: lanes 8 apart inside a wave, then the four waves in order
  auto reduce = [&](auto (&p)[4], auto (&buf)[4][GD_UCOLS]) {
#pragma unroll
    for (int off = 8; off < 64; off <<= 1)
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] += __shfl_xor(p[e], off);
    if (lane < 8) {
#pragma unroll
      for (int e = 0; e < 4; ++e) buf[wave][4 * cv + e] = p[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = ((buf[0][4 * cv + e] + buf[1][4 * cv + e]) + buf[2][4 * cv + e]) + buf[3][4 * cv + e];
  };
  for (int t = 0; t < a.tokens; ++t) {
    const int64_t gi = (b * a.tokens + t) * a.hv + hv;
    // exp(g) through fp64, once per token, carried as two floats: the decay multiplies every state element, so an error of the
    // factor (two units in the last place for the one-instruction exponential, half a unit for a correctly rounded float) is an
    // error of the whole state, on top of the one rounding the update makes
    const double eg64 = exp(static_cast<double>(
        a.gb_f32 ? static_cast<const float*>(a.g)[gi] : static_cast<float>(static_cast<const T*>(a.g)[gi])));
    const float eg = static_cast<float>(eg64), eg_lo = static_cast<float>(eg64 - static_cast<double>(eg));
    const double beta = a.gb_f32 ? static_cast<const float*>(a.beta)[gi] : static_cast<float>(static_cast<const T*>(a.beta)[gi]);
    const T4 vv = *reinterpret_cast<const T4*>(vp + t * a.v_ts);
    // S^T k^ of the undecayed state, (exp(g) S)^T k^ = exp(g) (S^T k^), summed in fp64: once the state has learned a key, v and
    // S^T k^ nearly cancel, and an fp32 sum's error, small against the sum, is large against their difference d
    double sk[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr)
#pragma unroll
      for (int e = 0; e < 4; ++e) sk[e] = fma(static_cast<double>(S[rr][e]), ks64[t][32 * rr + seg], sk[e]);
    reduce(sk, red64);
    f32x4 d;
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = static_cast<float>(beta * (static_cast<double>(static_cast<float>(vv[e])) - eg64 * sk[e]));
    float so[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
      const f32x4 kd = d * ks[t][32 * rr + seg];
#pragma unroll
      for (int e = 0; e < 4; ++e) {                              // decay and rank-one update: one rounding of the state
        S[rr][e] = __builtin_fmaf(eg, S[rr][e], __builtin_fmaf(eg_lo, S[rr][e], kd[e]));
        so[e] = __builtin_fmaf(S[rr][e], qs[t][32 * rr + seg], so[e]);
      }
    }
    reduce(so, red);
    if (seg == 0) {
      T4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = static_cast<T>(so[e] * a.scale);
      *reinterpret_cast<T4*>(op + static_cast<int64_t>(t) * a.hv * a.dv) = o;
    }
  }
#pragma unroll
  for (int rr = 0; rr < RPT; ++rr) *reinterpret_cast<f32x4*>(sp + static_cast<int64_t>(32 * rr + seg) * a.dv) = S[rr];
}

template <int DK, int DVS>
int gd_launch_prefill(const GdArgs& a, int64_t sequences, hipStream_t s) {
  static std::atomic<uint64_t> attr_set{0};
  if (first_call_on_device(attr_set))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gd_prefill_kernel<DK, DVS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              GdLds<DK, DVS>::bytes);
  const int64_t grid = sequences * a.hv * (a.dv / DVS);
  hipLaunchKernelGGL((gd_prefill_kernel<DK, DVS>), dim3(static_cast<unsigned>(grid)), dim3(GD_THREADS),
                     static_cast<size_t>(GdLds<DK, DVS>::bytes), s, a);
  MOJO_CHECK_LAUNCH("gated_delta_rule");
  note_launch("gated_delta_rule:chunk%d:dk%d:dvs%d:%s", GD_C, DK, DVS, a.cu ? "packed" : "batched");
  return 0;
}

bool gd_strides_ok(const void* p, int64_t bs, int64_t ts, int64_t hs) {
  return aligned_to(p, 16) && bs % 8 == 0 && ts % 8 == 0 && hs % 8 == 0;
}

}  // namespace
}  // namespace mojo

using namespace mojo;

extern "C" int64_t mojo_hip_gated_delta_rule_dv_slice(int64_t sequences, int64_t value_heads, int64_t dv, int64_t dv_slice) {
  if (dv_slice == 32 || dv_slice == 64) return dv_slice;
  if (dv_slice != 0) return -1;
  return sequences * value_heads * (dv / 64) >= GD_CUS ? 64 : 32;   // whole 64-column slices once they alone fill the CUs
}

extern "C" int mojo_hip_gated_delta_rule(const void* q, const void* k, const void* v, const void* g, const void* beta,
                                         const float* initial_state, float* final_state, void* out, const void* cu_seqlens,
                                         int cu_i64, int64_t sequences, int64_t tokens, int64_t key_heads, int64_t value_heads,
                                         int64_t dk, int64_t dv, int64_t q_batch_stride, int64_t q_token_stride,
                                         int64_t q_head_stride, int64_t k_batch_stride, int64_t k_token_stride,
                                         int64_t k_head_stride, int64_t v_batch_stride, int64_t v_token_stride,
                                         int64_t v_head_stride, float scale, int use_qk_l2norm, int gate_dtype, int dtype,
                                         int64_t dv_slice, mojo_stream_t stream) {
  const char* what = "gated_delta_rule";
  MOJO_REQUIRE(sequences >= 0 && tokens >= 0 && key_heads > 0 && value_heads > 0, MOJO_EINVAL, "%s: bad sizes", what);
  MOJO_REQUIRE(dtype == MOJO_BF16, MOJO_EUNSUPPORTED, "%s: bf16 only", what);
  MOJO_REQUIRE(gate_dtype == MOJO_F32 || gate_dtype == dtype, MOJO_EUNSUPPORTED, "%s: g / beta in fp32 or the query's dtype", what);
  MOJO_REQUIRE((dk == 64 || dk == 128) && (dv == 64 || dv == 128), MOJO_EUNSUPPORTED, "%s: Dk %lld / Dv %lld (64 and 128 are compiled)",
               what, (long long)dk, (long long)dv);
  MOJO_REQUIRE(value_heads % key_heads == 0, MOJO_EUNSUPPORTED, "%s: %lld value heads are no multiple of %lld key heads", what,
               (long long)value_heads, (long long)key_heads);
  const int64_t dvs = mojo_hip_gated_delta_rule_dv_slice(sequences, value_heads, dv, dv_slice);
  MOJO_REQUIRE(dvs > 0, MOJO_EINVAL, "%s: dv_slice %lld (0 = planned, 32 or 64)", what, (long long)dv_slice);
  MOJO_REQUIRE(sequences * value_heads * (dv / dvs) < (int64_t{1} << 31) && tokens < (int64_t{1} << 31), MOJO_EUNSUPPORTED,
               "%s: sizes beyond the launch's range", what);
  if (sequences == 0) return 0;
  MOJO_REQUIRE(tokens == 0 || (q && k && v && g && beta && out), MOJO_EINVAL, "%s: null pointer", what);
  MOJO_REQUIRE(gd_strides_ok(q, q_batch_stride, q_token_stride, q_head_stride) &&
               gd_strides_ok(k, k_batch_stride, k_token_stride, k_head_stride) &&
               gd_strides_ok(v, v_batch_stride, v_token_stride, v_head_stride) && aligned_to(out, 16),
               MOJO_EUNSUPPORTED, "%s: q / k / v must be 16-byte aligned with strides that are multiples of 16 bytes", what);
  MOJO_REQUIRE(final_state == nullptr || final_state != initial_state, MOJO_EINVAL, "%s: final_state must not be initial_state", what);
  GdArgs a;
  a.q = static_cast<const bf16_t*>(q); a.k = static_cast<const bf16_t*>(k); a.v = static_cast<const bf16_t*>(v);
  a.g = g; a.beta = beta; a.cu = cu_seqlens; a.s_in = initial_state; a.s_out = final_state; a.out = static_cast<bf16_t*>(out);
  a.q_bs = q_batch_stride; a.q_ts = q_token_stride; a.q_hs = q_head_stride;
  a.k_bs = k_batch_stride; a.k_ts = k_token_stride; a.k_hs = k_head_stride;
  a.v_bs = v_batch_stride; a.v_ts = v_token_stride; a.v_hs = v_head_stride; a.tokens = tokens;
  a.hk = static_cast<int>(key_heads); a.hv = static_cast<int>(value_heads); a.dv = static_cast<int>(dv);
  a.norm = use_qk_l2norm ? 1 : 0; a.gb_f32 = gate_dtype == MOJO_F32 ? 1 : 0; a.cu_i64 = cu_i64 ? 1 : 0; a.scale = scale;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dk == 64) return dvs == 64 ? gd_launch_prefill<64, 64>(a, sequences, s) : gd_launch_prefill<64, 32>(a, sequences, s);
  return dvs == 64 ? gd_launch_prefill<128, 64>(a, sequences, s) : gd_launch_prefill<128, 32>(a, sequences, s);
}

extern "C" int mojo_hip_gated_delta_rule_update(const void* q, const void* k, const void* v, const void* g, const void* beta,
                                                float* state, void* out, int64_t batch, int64_t tokens, int64_t key_heads,
                                                int64_t value_heads, int64_t dk, int64_t dv, int64_t q_batch_stride,
                                                int64_t q_token_stride, int64_t q_head_stride, int64_t k_batch_stride,
                                                int64_t k_token_stride, int64_t k_head_stride, int64_t v_batch_stride,
                                                int64_t v_token_stride, int64_t v_head_stride, float scale, int use_qk_l2norm,
                                                int gate_dtype, int dtype, mojo_stream_t stream) {
  const char* what = "gated_delta_rule_update";
  MOJO_REQUIRE(batch >= 0 && key_heads > 0 && value_heads > 0, MOJO_EINVAL, "%s: bad sizes", what);
  MOJO_REQUIRE(tokens >= 1 && tokens <= GD_MAX_UPDATE_T, MOJO_EUNSUPPORTED, "%s: %lld tokens (1 to %d)", what, (long long)tokens,
               GD_MAX_UPDATE_T);
  MOJO_REQUIRE(dtype == MOJO_BF16 || dtype == MOJO_F16, MOJO_EUNSUPPORTED, "%s: bf16 and fp16 only", what);
  MOJO_REQUIRE(gate_dtype == MOJO_F32 || gate_dtype == dtype, MOJO_EUNSUPPORTED, "%s: g / beta in fp32 or the query's dtype", what);
  MOJO_REQUIRE((dk == 64 || dk == 128) && (dv == 64 || dv == 128), MOJO_EUNSUPPORTED, "%s: Dk %lld / Dv %lld (64 and 128 are compiled)",
               what, (long long)dk, (long long)dv);
  MOJO_REQUIRE(value_heads % key_heads == 0, MOJO_EUNSUPPORTED, "%s: %lld value heads are no multiple of %lld key heads", what,
               (long long)value_heads, (long long)key_heads);
  const int64_t grid = batch * value_heads * (dv / GD_UCOLS);
  MOJO_REQUIRE(grid < (int64_t{1} << 31), MOJO_EUNSUPPORTED, "%s: sizes beyond the launch's range", what);
  if (batch == 0) return 0;
  MOJO_REQUIRE(q && k && v && g && beta && state && out, MOJO_EINVAL, "%s: null pointer", what);
  MOJO_REQUIRE(gd_strides_ok(q, q_batch_stride, q_token_stride, q_head_stride) &&
               gd_strides_ok(k, k_batch_stride, k_token_stride, k_head_stride) &&
               gd_strides_ok(v, v_batch_stride, v_token_stride, v_head_stride) && aligned_to(out, 16) && aligned_to(state, 16),
               MOJO_EUNSUPPORTED, "%s: q / k / v must be 16-byte aligned with strides that are multiples of 16 bytes", what);
  GdUpdateArgs a;
  a.q = q; a.k = k; a.v = v; a.g = g; a.beta = beta; a.state = state; a.out = out;
  a.q_bs = q_batch_stride; a.q_ts = q_token_stride; a.q_hs = q_head_stride;
  a.k_bs = k_batch_stride; a.k_ts = k_token_stride; a.k_hs = k_head_stride;
  a.v_bs = v_batch_stride; a.v_ts = v_token_stride; a.v_hs = v_head_stride;
  a.tokens = static_cast<int>(tokens); a.hk = static_cast<int>(key_heads); a.hv = static_cast<int>(value_heads);
  a.dv = static_cast<int>(dv); a.norm = use_qk_l2norm ? 1 : 0; a.gb_f32 = gate_dtype == MOJO_F32 ? 1 : 0; a.scale = scale;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 g3(static_cast<unsigned>(grid)), b3(GD_THREADS);
  if (dtype == MOJO_BF16) {
    if (dk == 64) hipLaunchKernelGGL((gd_update_kernel<bf16_t, 64>), g3, b3, 0, s, a);
    else hipLaunchKernelGGL((gd_update_kernel<bf16_t, 128>), g3, b3, 0, s, a);
  } else {
    if (dk == 64) hipLaunchKernelGGL((gd_update_kernel<f16_t, 64>), g3, b3, 0, s, a);
    else hipLaunchKernelGGL((gd_update_kernel<f16_t, 128>), g3, b3, 0, s, a);
  }
  MOJO_CHECK_LAUNCH(what);
  note_launch("gated_delta_rule_update:dk%d:t%d", static_cast<int>(dk), static_cast<int>(tokens));
  return 0;
}
