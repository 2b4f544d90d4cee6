// MXFP4 (MXFP4_OPS: MojoMXFP4Quant, MojoMXFP4Gemm): OCP microscaling fp4, E2M1 elements with one E8M0 scale per
// 32 elements along K.  A row of K elements is K / 2 data bytes (element 2j in the low nibble of byte j) and K / 32 scale bytes.
//
// The product runs on v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz:4 blgp:4 (both operands fp4): a lane's operand is 16 bytes,
// 32 elements, EXACTLY ONE BLOCK, and its scale is one byte of a VGPR, chosen by op_sel.  Lane l = 16 g + r holds row r of its
// operand tile and the g-th of the instruction's four blocks; the instruction multiplies the blocks of equal g, scales each
// product by both lanes' scale bytes and sums over g and over the 32 elements in fp32.  Which K the four blocks are is the
// kernel's choice as long as both operands are cut alike, so a SUPER-TILE of 512 elements (256 data bytes, 16 scale bytes per
// row) is cut so that lane group g owns the four CONSECUTIVE blocks 4g .. 4g+3: a lane reads 64 contiguous data bytes and
// ONE scale dword per row and super-tile, and the four instructions of a super-tile walk op_sel 0..3 over that dword.  Nobody's
// scales need an offline shuffle.  No dequantised operand is ever formed.
//
// First operand = weight rows, second = activation rows: a lane's four accumulators are out[m = r][n = 4g .. 4g+3], four
// consecutive columns, one vector store.
//
// Two forms, planned from the shapes alone (mx_plan):
//   tile (M > 32): 128 x 128 outputs per workgroup of four waves (2 x 2, 64 x 64 each).  Data goes global -> registers -> LDS
//     one super-tile ahead of the MFMAs (64 KiB: 128 + 128 rows x 256 bytes; the 16-byte chunk c of row r is stored at chunk
//     c ^ (r & 15), so the sixteen rows a ds_read_b128 touches at one chunk index fall into sixteen different bank groups).
//     The SCALES stay out of LDS: they are 1/16 of the data's bytes, a lane needs exactly one dword per row and super-tile, and
//     the sixteen lanes of a group read sixteen rows' dwords that the sixteen rows' neighbours (g = 0..3) complete to whole
//     16-byte pieces, so the request is as wide as an LDS image of it would be, without the store, the barrier and the read.
//     They are requested one super-tile ahead like the data.
//   skinny (M <= 32, decode; bound by the weight bytes): no LDS.  A wave owns 16 weight rows and a slice of K; every weight
//     byte is read exactly once, 64 contiguous bytes per lane, the activation rows (one or two groups of 16) are the columns
//     of the product and come through the caches.  K is split so that the launch fills the chip; partial sums go to the
//     workspace as fp32 and one merge kernel adds them IN SPLIT ORDER (no atomics: two calls give the same bits).
// A K that is no multiple of 512 ends in a partial super-tile: 16-byte pieces past the row are zeros in registers (never read),
// scale bytes past the row are 127, so the tail blocks add exact zeros.  Rows past M are clamped to row M - 1 on the way in
// and masked on the way out.  Row offsets are 64-bit.
//
// The quantiser is one streaming launch: four lanes share a block, each reads one 16-byte vector (8 elements), the block's
// largest magnitude is two quad exchanges on the integer image of |x| (monotone for non-negative floats; Inf / NaN are the
// largest images, so the exponent field 255 of the maximum IS the block's "holds Inf or NaN"), every lane writes its 4 data
// bytes, the first of the four the scale byte.  Plain C++ arithmetic on exact values: bit-identical to the golden by construction.
#include <algorithm>

#include "common.h"
#include "mxfp4_core.h"

namespace mojo {
namespace {

struct MxArgs {
  const uint8_t* a; const uint8_t* sa; const uint8_t* w; const uint8_t* sw;
  void* out; float* ws;
  int64_t M;
  int N, K2 /* data bytes per row */, KB /* blocks per row */, nst /* super-tiles */, S, per;
};

// ---- tile form ------------------------------------------------------------------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(MX_THREADS) void mx_tile_kernel(MxArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * MX_TILE * MX_ST_BYTES];   // activation image | weight image
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 15, g = lane >> 4;
  const int64_t m0 = static_cast<int64_t>(blockIdx.y) * MX_TILE;
  const int n0 = blockIdx.x * MX_TILE;
  const int64_t m_last = p.M - 1;
  const int n_last = p.N - 1;

  // staging: thread -> chunk tid & 15 of rows (tid >> 4) + 16 q, q = 0..7, of both images
  const int sc = tid & 15, sr = tid >> 4;
  const int st_off = sr * MX_ST_BYTES + ((sc ^ sr) << 4);                 // (+ q * 16 rows; (row & 15) == sr)
  u32x4 stage_a[8], stage_w[8];
  auto request = [&](int st) {
    const int off = st * MX_ST_BYTES + sc * 16;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t am = min(m0 + sr + 16 * q, m_last);
      const int wr = min(n0 + sr + 16 * q, n_last);
      stage_a[q] = mx_chunk(p.a + am * p.K2, off, p.K2);
      stage_w[q] = mx_chunk(p.w + static_cast<int64_t>(wr) * p.K2, off, p.K2);
    }
  };
  // scales: a lane's four activation rows and four weight rows, one dword each per super-tile
  int sa_next[4], sw_next[4], sa_cur[4], sw_cur[4];
  auto request_scales = [&](int st) {
    const int b0 = st * MX_ST_BLOCKS + 4 * g;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t am = min(m0 + wm * 64 + i * 16 + r, m_last);
      const int wr = min(n0 + wn * 64 + i * 16 + r, n_last);
      sa_next[i] = mx_scale4(p.sa + am * p.KB, b0, p.KB);
      sw_next[i] = mx_scale4(p.sw + static_cast<int64_t>(wr) * p.KB, b0, p.KB);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const unsigned char* img_a = lds + (wm * 64 + r) * MX_ST_BYTES;
  const unsigned char* img_w = lds + MX_TILE * MX_ST_BYTES + (wn * 64 + r) * MX_ST_BYTES;

  request(0);
  request_scales(0);
  for (int st = 0; st < p.nst; ++st) {
    __syncthreads();                                                       // every wave is done with the previous images
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      *reinterpret_cast<u32x4*>(lds + st_off + q * 16 * MX_ST_BYTES) = stage_a[q];
      *reinterpret_cast<u32x4*>(lds + MX_TILE * MX_ST_BYTES + st_off + q * 16 * MX_ST_BYTES) = stage_w[q];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { sa_cur[i] = sa_next[i]; sw_cur[i] = sw_next[i]; }
    __syncthreads();
    if (st + 1 < p.nst) {                                                  // in flight under this super-tile's MFMAs
      request(st + 1);
      request_scales(st + 1);
    }
    static_for<4>([&](auto s_c) {
      constexpr int s = decltype(s_c)::value;
      const int col = ((4 * g + s) ^ r) << 4;
      u32x4 fa[4], fw[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fa[i] = *reinterpret_cast<const u32x4*>(img_a + i * 16 * MX_ST_BYTES + col);
        fw[i] = *reinterpret_cast<const u32x4*>(img_w + i * 16 * MX_ST_BYTES + col);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mx_mma<s>(fw[j], fa[i], acc[i][j], sw_cur[j], sa_cur[i]);
    });
  }

  TO* out = static_cast<TO*>(p.out);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + wm * 64 + i * 16 + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + 4 * g;
      if (m < p.M && n < p.N) mx_store4<TO>(out + m * p.N + n, acc[i][j]);
    }
  }
}

// ---- skinny form ----------------------------------------------------------------------------------------------------------
template <int MG>
struct MxSkinnyRegs { u32x4 w[4]; u32x4 a[MG][4]; int sw; int sa[MG]; };

template <typename TO, int MG>
__global__ __launch_bounds__(MX_THREADS) void mx_skinny_kernel(MxArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n_tiles = p.N / 16;
  const int item = blockIdx.x * (MX_THREADS / 64) + wave;
  if (item >= n_tiles * p.S) return;
  const int split = item / n_tiles, n0 = (item % n_tiles) * 16;
  const int st_begin = split * p.per, st_end = min(p.nst, st_begin + p.per);

  const uint8_t* w_row = p.w + static_cast<int64_t>(n0 + r) * p.K2;
  const uint8_t* sw_row = p.sw + static_cast<int64_t>(n0 + r) * p.KB;
  const uint8_t* a_row[MG];
  const uint8_t* sa_row[MG];
#pragma unroll
  for (int mg = 0; mg < MG; ++mg) {
    const int64_t m = min(static_cast<int64_t>(mg * 16 + r), p.M - 1);
    a_row[mg] = p.a + m * p.K2;
    sa_row[mg] = p.sa + m * p.KB;
  }
  auto request = [&](int st, MxSkinnyRegs<MG>& x) {
    const int off = st * MX_ST_BYTES + g * 64, b0 = st * MX_ST_BLOCKS + 4 * g;
#pragma unroll
    for (int s = 0; s < 4; ++s) x.w[s] = mx_chunk(w_row, off + 16 * s, p.K2);
    x.sw = mx_scale4(sw_row, b0, p.KB);
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) {
#pragma unroll
      for (int s = 0; s < 4; ++s) x.a[mg][s] = mx_chunk(a_row[mg], off + 16 * s, p.K2);
      x.sa[mg] = mx_scale4(sa_row[mg], b0, p.KB);
    }
  };

  f32x4 acc[MG];
#pragma unroll
  for (int mg = 0; mg < MG; ++mg) acc[mg] = f32x4{0.f, 0.f, 0.f, 0.f};
  MxSkinnyRegs<MG> cur, next;
  request(st_begin, cur);
  for (int st = st_begin; st < st_end; ++st) {
    if (st + 1 < st_end) request(st + 1, next);
    static_for<4>([&](auto s_c) {
      constexpr int s = decltype(s_c)::value;
#pragma unroll
      for (int mg = 0; mg < MG; ++mg) acc[mg] = mx_mma<s>(cur.w[s], cur.a[mg][s], acc[mg], cur.sw, cur.sa[mg]);
    });
    if (st + 1 < st_end) cur = next;
  }

#pragma unroll
  for (int mg = 0; mg < MG; ++mg) {
    const int64_t m = mg * 16 + r;
    if (m >= p.M) continue;
    const int n = n0 + 4 * g;
    if (p.S == 1) mx_store4<TO>(static_cast<TO*>(p.out) + m * p.N + n, acc[mg]);
    else *reinterpret_cast<f32x4*>(p.ws + (static_cast<int64_t>(split) * p.M + m) * p.N + n) = acc[mg];
  }
}

// out = round(sum over splits, in split order) for four consecutive columns per thread
template <typename TO>
__global__ __launch_bounds__(MX_THREADS) void mx_merge_kernel(MxArgs p) {
  const int64_t quads = p.M * p.N / 4;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * MX_THREADS + threadIdx.x;
  if (idx >= quads) return;
  f32x4 sum = *reinterpret_cast<const f32x4*>(p.ws + idx * 4);
  for (int s = 1; s < p.S; ++s) sum += *reinterpret_cast<const f32x4*>(p.ws + (static_cast<int64_t>(s) * quads + idx) * 4);
  mx_store4<TO>(static_cast<TO*>(p.out) + idx * 4, sum);
}

// ---- the quantiser --------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(MX_THREADS) void mx_quant_kernel(const T* x, uint8_t* data, uint8_t* scale, int64_t m, int k,
                                                              int64_t row_stride) {
  const int vecs = k / 8;                                                  // 16-byte vectors per row, a multiple of 4
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * MX_THREADS + threadIdx.x;
  if (idx >= m * vecs) return;                                             // (whole quads leave together)
  const int64_t row = idx / vecs;
  const int v = static_cast<int>(idx - row * vecs);
  const typename vec_of<T, 8>::type in = load_vec<T, 8>(x + row * row_stride + v * 8);
  unsigned bits[8];
  unsigned amax = 0u;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bits[e] = __builtin_bit_cast(unsigned, static_cast<float>(in[e]));     // (16 bits to fp32: exact)
    amax = max(amax, bits[e] & 0x7fffffffu);
  }
  amax = max(amax, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(amax), DPP_QUAD_XOR1, 0xF, 0xF, true)));
  amax = max(amax, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(amax), DPP_QUAD_XOR2, 0xF, 0xF, true)));
  const int field = static_cast<int>(amax >> 23);                          // biased floor(log2 amax); 0: zero or below 2^-126
  unsigned packed = 0u;
  int byte = 0xFF;
  if (field != 255) {
    byte = max(field - 2, 0);                                              // e + 127 with e = max(field - 127 - 2, -127)
    const float up = __builtin_bit_cast(float, static_cast<unsigned>(254 - byte) << 23);   // 2^-e, a normal number
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float a = __builtin_bit_cast(float, bits[e] & 0x7fffffffu) * up;   // exact (or below every threshold)
      const unsigned code = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
      packed |= (code | ((bits[e] >> 31) << 3)) << (4 * e);
    }
  }
  *reinterpret_cast<unsigned*>(data + row * (k / 2) + v * 4) = packed;
  if ((v & 3) == 0) scale[row * (k / MX_BLOCK) + (v >> 2)] = static_cast<uint8_t>(byte);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct MxPlan { bool skinny; int mg, S, per, nst; };

MxPlan mx_plan(int64_t m, int64_t k, int64_t n) {
  MxPlan pl;
  pl.nst = static_cast<int>(ceil_div(k, 2 * MX_ST_BYTES));
  pl.skinny = m <= MX_SKINNY_MAX_M;
  pl.mg = m <= 16 ? 1 : 2;
  pl.S = 1;
  pl.per = pl.nst;
  if (pl.skinny) {
    const int64_t want = std::max<int64_t>(1, MX_SKINNY_WAVES / (n / 16));
    const int s = static_cast<int>(std::min<int64_t>(std::min<int64_t>(want, pl.nst), MX_MAX_SPLIT));
    pl.per = static_cast<int>(ceil_div(pl.nst, s));
    pl.S = static_cast<int>(ceil_div(pl.nst, pl.per));                    // (no empty split)
  }
  return pl;
}

template <typename TO>
int mx_launch(const MxPlan& pl, MxArgs& a, hipStream_t s) {
  if (!pl.skinny) {
    const dim3 grid(static_cast<unsigned>(ceil_div(a.N, MX_TILE)), static_cast<unsigned>(ceil_div(a.M, MX_TILE)));
    hipLaunchKernelGGL((mx_tile_kernel<TO>), grid, dim3(MX_THREADS), 0, s, a);
    MOJO_CHECK_LAUNCH("mxfp4_gemm(tile)");
    note_launch("mxfp4_gemm:tile128");
    return 0;
  }
  const dim3 grid(static_cast<unsigned>(ceil_div(static_cast<int64_t>(a.N / 16) * pl.S, MX_THREADS / 64)));
  if (pl.mg == 1) hipLaunchKernelGGL((mx_skinny_kernel<TO, 1>), grid, dim3(MX_THREADS), 0, s, a);
  else hipLaunchKernelGGL((mx_skinny_kernel<TO, 2>), grid, dim3(MX_THREADS), 0, s, a);
  MOJO_CHECK_LAUNCH("mxfp4_gemm(skinny)");
  if (pl.S > 1) {
    hipLaunchKernelGGL((mx_merge_kernel<TO>), dim3(static_cast<unsigned>(ceil_div(a.M * a.N / 4, MX_THREADS))), dim3(MX_THREADS),
                       0, s, a);
    MOJO_CHECK_LAUNCH("mxfp4_gemm(merge)");
  }
  note_launch("mxfp4_gemm:skinny:mg%d:splitk%d", pl.mg, pl.S);
  return 0;
}

}  // namespace
}  // namespace mojo

using namespace mojo;

extern "C" int mojo_hip_mxfp4_quant(const void* x, void* data, void* scale, int64_t m, int64_t k, int64_t row_stride, int dtype,
                                    mojo_stream_t stream) {
  const char* what = "mxfp4_quant";
  MOJO_REQUIRE(m >= 0 && k > 0 && k % MX_BLOCK == 0, MOJO_EINVAL, "%s: k %lld must be a positive multiple of %d", what, (long long)k,
               MX_BLOCK);
  MOJO_REQUIRE(dtype == MOJO_BF16 || dtype == MOJO_F16, MOJO_EUNSUPPORTED, "%s: bf16 and fp16 only", what);
  MOJO_REQUIRE(k < (int64_t{1} << 31) && ceil_div(m * (k / 8), MX_THREADS) < (int64_t{1} << 31), MOJO_EUNSUPPORTED,
               "%s: sizes beyond the launch's range", what);
  if (m == 0) return 0;
  MOJO_REQUIRE(x && data && scale, MOJO_EINVAL, "%s: null pointer", what);
  MOJO_REQUIRE(aligned_to(x, 16) && aligned_to(data, 16) && row_stride >= k && (m == 1 || row_stride % 8 == 0), MOJO_EUNSUPPORTED,
               "%s: x and data must be 16-byte aligned, the row stride a multiple of 8 elements", what);
  const dim3 grid(static_cast<unsigned>(ceil_div(m * (k / 8), MX_THREADS)));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == MOJO_BF16)
    hipLaunchKernelGGL((mx_quant_kernel<bf16_t>), grid, dim3(MX_THREADS), 0, s, static_cast<const bf16_t*>(x),
                       static_cast<uint8_t*>(data), static_cast<uint8_t*>(scale), m, static_cast<int>(k), row_stride);
  else
    hipLaunchKernelGGL((mx_quant_kernel<f16_t>), grid, dim3(MX_THREADS), 0, s, static_cast<const f16_t*>(x),
                       static_cast<uint8_t*>(data), static_cast<uint8_t*>(scale), m, static_cast<int>(k), row_stride);
  MOJO_CHECK_LAUNCH(what);
  note_launch("mxfp4_quant");
  return 0;
}

extern "C" int64_t mojo_hip_mxfp4_gemm_workspace_bytes(int64_t m, int64_t k, int64_t n) {
  if (m <= 0 || k <= 0 || n < 16) return 16;
  const MxPlan pl = mx_plan(m, k, n);
  return 16 + (pl.skinny && pl.S > 1 ? static_cast<int64_t>(pl.S) * m * n * 4 : 0);
}

extern "C" int mojo_hip_mxfp4_gemm(const void* input, const void* input_scale, const void* weight, const void* weight_scale,
                                   void* out, int64_t m, int64_t k, int64_t n, int out_dtype, void* workspace,
                                   int64_t workspace_bytes, mojo_stream_t stream) {
  const char* what = "mxfp4_gemm";
  MOJO_REQUIRE(m >= 0 && n > 0 && k > 0 && k % MX_BLOCK == 0, MOJO_EINVAL, "%s: k %lld must be a positive multiple of %d", what,
               (long long)k, MX_BLOCK);
  MOJO_REQUIRE(n % 16 == 0, MOJO_EUNSUPPORTED, "%s: n %lld (multiples of 16 are supported)", what, (long long)n);
  MOJO_REQUIRE(out_dtype == MOJO_F32 || out_dtype == MOJO_F16 || out_dtype == MOJO_BF16, MOJO_EUNSUPPORTED,
               "%s: fp32, fp16 and bf16 outputs only", what);
  MOJO_REQUIRE(k < (int64_t{1} << 31) && n < (int64_t{1} << 31) && ceil_div(m, MX_TILE) < 65536 &&
               ceil_div(m * n / 4, MX_THREADS) < (int64_t{1} << 31), MOJO_EUNSUPPORTED, "%s: sizes beyond the launch's range", what);
  if (m == 0) return 0;
  MOJO_REQUIRE(input && input_scale && weight && weight_scale && out, MOJO_EINVAL, "%s: null pointer", what);
  MOJO_REQUIRE(aligned_to(input, 16) && aligned_to(weight, 16) && aligned_to(out, 16), MOJO_EUNSUPPORTED,
               "%s: input, weight and out must be 16-byte aligned", what);
  MOJO_REQUIRE(workspace && workspace_bytes >= mojo_hip_mxfp4_gemm_workspace_bytes(m, k, n) && aligned_to(workspace, 16),
               MOJO_EWORKSPACE, "%s: workspace too small", what);
  const MxPlan pl = mx_plan(m, k, n);
  MxArgs a;
  a.a = static_cast<const uint8_t*>(input); a.sa = static_cast<const uint8_t*>(input_scale);
  a.w = static_cast<const uint8_t*>(weight); a.sw = static_cast<const uint8_t*>(weight_scale);
  a.out = out; a.ws = static_cast<float*>(workspace);
  a.M = m; a.N = static_cast<int>(n); a.K2 = static_cast<int>(k / 2); a.KB = static_cast<int>(k / MX_BLOCK);
  a.nst = pl.nst; a.S = pl.S; a.per = pl.per;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (out_dtype == MOJO_F32) return mx_launch<float>(pl, a, s);
  if (out_dtype == MOJO_F16) return mx_launch<f16_t>(pl, a, s);
  return mx_launch<bf16_t>(pl, a, s);
}
