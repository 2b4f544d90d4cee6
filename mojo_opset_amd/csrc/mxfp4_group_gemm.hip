// MXFP4 MoE experts (MXFP4_MOE_OPS: MojoMXFP4GroupGemm, MojoMXFP4SwiGLUQuant, MojoMXFP4Experts): the grouped a4w4
// product over ragged row groups against [G, N, K / 2] weights, with the stage between the two expert GEMMs, re-quantising
// silu(gate) * up to MXFP4, either in the product's own epilogue or as a streaming kernel.  Format, instruction and super-tile
// cut are those of mxfp4_gemm.hip (helpers in mxfp4_core.h).
//
// SPLITTING THE WORK.  `group_list` (row counts) stays on the device.  A one-workgroup PLAN kernel clamps the counts (negative: 0;
// the running sum is cut at M), prefix-sums them and writes two work tables into the workspace:
//   tiles  {group, first row, end row}: the 128-row tiles of every group with MORE than 32 rows, then the tiles of the slack rows
//          [sum(counts), M) with group -1 (they run no K loop, so their zero accumulators go through the same epilogue and the rows
//          come out as zeros: data bytes 0 and scale byte 0 in the fused form);
//   skinny {group, first row, rows, first partial row}: every group with 1..32 rows.
// The host sizes both launches from bounds it knows without a sync, ceil(M / 128) + G row tiles and min(G, M) skinny groups;
// a workgroup (a wave) whose index is not below the table's length in the header leaves.  The dealing is per group, not per
// call: a decode step's 4 rows per expert take the weight-streaming form while a hot expert of the same call takes tiles.  Both
// launches are always issued (capture-safe), every row of the output is written by exactly one of them, there are no atomics.
//
// TILE FORM: mx_tile_kernel's super-tile walk, swizzled 64 KiB LDS image and register-resident scales, with weight rows offset
// by g * N and rows clamped / masked to the group's range.
// SKINNY FORM: one wave per (group, 16 weight rows, K slice), the weight streamed once; the split over K is planned from the
// shapes alone and merged in split order through fp32 partials indexed by the group's first partial row, so the partials of a
// call take min(M, 32 min(G, M)) rows and the merge touches rows of skinny groups only.
//
// THE FUSED STAGE (swiglu_quant; N = 2 I, weight rows [gate | up]).  A tile workgroup's 128 weight rows are the 64 gate rows
// [c0, c0 + 64) and the 64 up rows [I + c0, I + c0 + 64); wave (wm, wn) multiplies the gate column tiles c0 + 32 wn + 16 j,
// j = 0, 1, in its first two accumulator columns and the matching up tiles in the other two.  Lane 16 g + r holds
// out[r][4g .. 4g+3] of each, so the wave holds, for each of its 64 rows, both factors of 32 consecutive activation columns:
// one MXFP4 block.  The epilogue forms h = silu(gate) * up in fp32, reduces max |h| over j and over the four lane groups (two
// lane-row swaps on the integer image, on which Inf / NaN are the largest), derives the scale byte by the quantiser's rule, codes
// the nibbles against the seven tie thresholds and stores 2 x 2 data bytes per lane and one scale byte per row and block.  The
// [M, 2I] product never reaches memory.  In the skinny form a wave owns 16 gate rows and their 16 up rows (two weight streams,
// two accumulators per row group) and writes fp32 partials; the merge sums the splits in order and applies the same epilogue
// (eight lanes a block), also when there is one split.  mojo_hip_mxfp4_swiglu_quant is that merge over a stored x.
// silu is x / (1 + expf(-x)) with the library's expf and an IEEE division, the golden's formula: an epilogue, not a hot loop.
#include <algorithm>

#include "common.h"
#include "mxfp4_core.h"

namespace mojo {
namespace {

constexpr int MXG_MAX_GROUPS = 4 * MX_THREADS;   // the plan kernel scans at most four consecutive groups per thread
constexpr int MXG_HEADER_BYTES = 16;             // {tile entries, skinny entries}

struct MxgArgs {
  const uint8_t* a; const uint8_t* sa; const uint8_t* w; const uint8_t* sw;
  void* out; uint8_t* out_scale;
  const int* counts;
  int* header; int4* tiles; int4* skinny; float* part;
  int M, G, N, I /* fused: N / 2 */, K2, KB, nst, S, per, nt /* tile entries allocated */, ns /* skinny entries */, part_rows;
};

// ---- the fused stage's arithmetic -------------------------------------------------------------------------------------------
__device__ __forceinline__ float mx_swiglu(float gate, float up) { return gate / (1.0f + expf(-gate)) * up; }

// the scale byte of a block from the integer image of its largest magnitude; 0xFF: the block holds Inf or NaN
__device__ __forceinline__ int mx_scale_byte(unsigned amax) {
  const int field = static_cast<int>(amax >> 23);
  return field == 255 ? 0xFF : max(field - 2, 0);
}

// sign and E2M1 code of the value with image `bits` in a block of scale byte `byte` (not 0xFF)
__device__ __forceinline__ unsigned mx_nibble(unsigned bits, int byte) {
  const float up = __builtin_bit_cast(float, static_cast<unsigned>(254 - byte) << 23);      // 2^-e, a normal number
  const float a = __builtin_bit_cast(float, bits & 0x7fffffffu) * up;                        // exact (or below every threshold)
  const unsigned code = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
  return code | ((bits >> 31) << 3);
}

__device__ __forceinline__ unsigned short mx_nibbles4(const unsigned* bits, int byte) {
  if (byte == 0xFF) return 0;
  unsigned v = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) v |= mx_nibble(bits[e], byte) << (4 * e);
  return static_cast<unsigned short>(v);
}

// max over lanes l, l ^ 16, l ^ 32, l ^ 48 of an unsigned (xor_max_16_32 on the integer image)
__device__ __forceinline__ unsigned xor_umax_16_32(unsigned x) {
  unsigned p = x, q = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(p), "+v"(q));
  const unsigned h = max(p, q);
  p = h; q = h;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(p), "+v"(q));
  return max(p, q);
}

// Eight consecutive lanes share a block: each holds four gate and four up values of columns 4 l8 .. 4 l8 + 3 of the block, and
// stores its two data bytes at `data`; lane 0 of the eight stores the scale byte.  Whole eights call this together.
__device__ __forceinline__ void mx_swiglu_quant8(f32x4 gate, f32x4 up, uint8_t* data, uint8_t* scale, bool first) {
  unsigned bits[4];
  unsigned amax = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bits[e] = __builtin_bit_cast(unsigned, mx_swiglu(gate[e], up[e]));
    amax = max(amax, bits[e] & 0x7fffffffu);
  }
  amax = max(amax, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(amax), DPP_QUAD_XOR1, 0xF, 0xF, true)));
  amax = max(amax, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(amax), DPP_QUAD_XOR2, 0xF, 0xF, true)));
  amax = max(amax, static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(amax), DPP_ROW_HALF_MIRROR, 0xF, 0xF, true)));
  const int byte = mx_scale_byte(amax);
  *reinterpret_cast<unsigned short*>(data) = mx_nibbles4(bits, byte);
  if (first) *scale = static_cast<uint8_t>(byte);
}

// ---- plan -------------------------------------------------------------------------------------------------------------------
// exclusive prefix of one value per thread over the workgroup, and the total (a serial walk over LDS: 256 broadcast reads)
__device__ __forceinline__ long long mxg_scan(long long v, long long* smem, long long& total) {
  __syncthreads();                                                         // (the previous scan's reads are done)
  smem[threadIdx.x] = v;
  __syncthreads();
  long long before = 0, all = 0;
  for (int t = 0; t < MX_THREADS; ++t) {
    if (t == static_cast<int>(threadIdx.x)) before = all;
    all += smem[t];
  }
  total = all;
  return before;
}

__global__ __launch_bounds__(MX_THREADS) void mxg_plan_kernel(MxgArgs p) {
  __shared__ long long smem[MX_THREADS];
  const int tid = threadIdx.x;
  const int each = (p.G + MX_THREADS - 1) / MX_THREADS;
  const int g_begin = min(p.G, tid * each), g_end = min(p.G, g_begin + each);
  const long long M = p.M;
  auto count = [&](int g) { return static_cast<long long>(min(max(p.counts[g], 0), p.M)); };

  long long rows = 0, total_rows, total_tiles, total_slots, total_part;
  for (int g = g_begin; g < g_end; ++g) rows += count(g);
  const long long first = mxg_scan(rows, smem, total_rows);
  long long tiles = 0, slots = 0, part = 0, at = first;
  for (int g = g_begin; g < g_end; ++g) {
    const int b = static_cast<int>(min(at, M)), e = static_cast<int>(min(at + count(g), M));
    at += count(g);
    const int n = e - b;
    if (n > MX_SKINNY_MAX_M) tiles += (n + MX_TILE - 1) / MX_TILE;
    else if (n > 0) { slots += 1; part += n; }
  }
  int tile_at = static_cast<int>(mxg_scan(tiles, smem, total_tiles));
  int slot_at = static_cast<int>(mxg_scan(slots, smem, total_slots));
  int part_at = static_cast<int>(mxg_scan(part, smem, total_part));
  at = first;
  for (int g = g_begin; g < g_end; ++g) {
    const int b = static_cast<int>(min(at, M)), e = static_cast<int>(min(at + count(g), M));
    at += count(g);
    const int n = e - b;
    if (n > MX_SKINNY_MAX_M) {
      for (int m0 = b; m0 < e; m0 += MX_TILE, ++tile_at)
        if (tile_at < p.nt) p.tiles[tile_at] = make_int4(g, m0, e, 0);
    } else if (n > 0) {
      if (slot_at < p.ns) p.skinny[slot_at] = make_int4(g, b, n, part_at);
      ++slot_at;
      part_at += n;
    }
  }
  // the slack rows [sum, M): tiles without a group
  const int sum = static_cast<int>(min(total_rows, M));
  const int slack_tiles = (p.M - sum + MX_TILE - 1) / MX_TILE;
  for (int i = tid; i < slack_tiles; i += MX_THREADS)
    if (static_cast<int>(total_tiles) + i < p.nt) p.tiles[static_cast<int>(total_tiles) + i] = make_int4(-1, sum + i * MX_TILE, p.M, 0);
  if (tid == 0) {
    p.header[0] = min(static_cast<int>(total_tiles) + slack_tiles, p.nt);
    p.header[1] = min(static_cast<int>(total_slots), p.ns);
  }
}

// ---- tile form ------------------------------------------------------------------------------------------------------------
// the row of the workgroup's 128-row weight image that accumulator column j of wave column wn multiplies
template <bool FUSED>
__device__ __forceinline__ int mxg_image_row(int wn, int j) {
  return FUSED ? (j >> 1) * 64 + wn * 32 + (j & 1) * 16 : wn * 64 + j * 16;
}
// the weight row (within the group's N rows) behind row `row` of the image of the workgroup at blockIdx.x; clamped into the matrix
template <bool FUSED>
__device__ __forceinline__ int mxg_weight_row(const MxgArgs& p, int row) {
  if (FUSED) {
    const int c = min(static_cast<int>(blockIdx.x) * 64 + (row & 63), p.I - 1);
    return row < 64 ? c : p.I + c;
  }
  return min(static_cast<int>(blockIdx.x) * MX_TILE + row, p.N - 1);
}

template <typename TO, bool FUSED>
__global__ __launch_bounds__(MX_THREADS) void mxg_tile_kernel(MxgArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * MX_TILE * MX_ST_BYTES];   // activation image | weight image
  if (static_cast<int>(blockIdx.y) >= p.header[0]) return;
  const int4 entry = p.tiles[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 15, g = lane >> 4;
  const int m0 = entry.y, m_end = entry.z, m_last = m_end - 1;
  const int nst = entry.x < 0 ? 0 : p.nst;                                 // slack rows: no K loop, zero accumulators
  const int64_t w_base = static_cast<int64_t>(max(entry.x, 0)) * p.N;     // the group's first weight row

  // staging: thread -> chunk tid & 15 of rows (tid >> 4) + 16 q, q = 0..7, of both images
  const int sc = tid & 15, sr = tid >> 4;
  const int st_off = sr * MX_ST_BYTES + ((sc ^ sr) << 4);                 // (+ q * 16 rows; (row & 15) == sr)
  u32x4 stage_a[8], stage_w[8];
  auto request = [&](int st) {
    const int off = st * MX_ST_BYTES + sc * 16;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t am = min(m0 + sr + 16 * q, m_last);
      const int64_t wr = w_base + mxg_weight_row<FUSED>(p, sr + 16 * q);
      stage_a[q] = mx_chunk(p.a + am * p.K2, off, p.K2);
      stage_w[q] = mx_chunk(p.w + wr * p.K2, off, p.K2);
    }
  };
  // scales: a lane's four activation rows and four weight rows, one dword each per super-tile
  int sa_next[4], sw_next[4], sa_cur[4], sw_cur[4];
  auto request_scales = [&](int st) {
    const int b0 = st * MX_ST_BLOCKS + 4 * g;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t am = min(m0 + wm * 64 + i * 16 + r, m_last);
      const int64_t wr = w_base + mxg_weight_row<FUSED>(p, mxg_image_row<FUSED>(wn, i) + r);
      sa_next[i] = mx_scale4(p.sa + am * p.KB, b0, p.KB);
      sw_next[i] = mx_scale4(p.sw + wr * p.KB, b0, p.KB);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const unsigned char* img_a = lds + (wm * 64 + r) * MX_ST_BYTES;
  const unsigned char* img_w = lds + MX_TILE * MX_ST_BYTES + r * MX_ST_BYTES;

  if (nst > 0) {
    request(0);
    request_scales(0);
  }
  for (int st = 0; st < nst; ++st) {
    __syncthreads();                                                       // every wave is done with the previous images
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      *reinterpret_cast<u32x4*>(lds + st_off + q * 16 * MX_ST_BYTES) = stage_a[q];
      *reinterpret_cast<u32x4*>(lds + MX_TILE * MX_ST_BYTES + st_off + q * 16 * MX_ST_BYTES) = stage_w[q];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { sa_cur[i] = sa_next[i]; sw_cur[i] = sw_next[i]; }
    __syncthreads();
    if (st + 1 < nst) {                                                    // in flight under this super-tile's MFMAs
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
        fw[i] = *reinterpret_cast<const u32x4*>(img_w + mxg_image_row<FUSED>(wn, i) * MX_ST_BYTES + col);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mx_mma<s>(fw[j], fa[i], acc[i][j], sw_cur[j], sa_cur[i]);
    });
  }

  if constexpr (!FUSED) {
    TO* out = static_cast<TO*>(p.out);
    const int n0 = blockIdx.x * MX_TILE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t m = m0 + wm * 64 + i * 16 + r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + j * 16 + 4 * g;
        if (m < m_end && n < p.N) mx_store4<TO>(out + m * p.N + n, acc[i][j]);
      }
    }
  } else {
    uint8_t* data = static_cast<uint8_t*>(p.out);
    const int c = blockIdx.x * 64 + wn * 32;                               // the wave's block of activation columns
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t m = m0 + wm * 64 + i * 16 + r;
      unsigned bits[2][4];
      unsigned amax = 0u;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bits[j][e] = __builtin_bit_cast(unsigned, mx_swiglu(acc[i][j][e], acc[i][j + 2][e]));
          amax = max(amax, bits[j][e] & 0x7fffffffu);
        }
      const int byte = mx_scale_byte(xor_umax_16_32(amax));                // (every lane takes part, masked or not)
      if (m < m_end && c < p.I) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
          *reinterpret_cast<unsigned short*>(data + m * (p.I / 2) + (c + 16 * j + 4 * g) / 2) = mx_nibbles4(bits[j], byte);
        if (g == 0) p.out_scale[m * (p.I / MX_BLOCK) + c / MX_BLOCK] = static_cast<uint8_t>(byte);
      }
    }
  }
}

// ---- skinny form ----------------------------------------------------------------------------------------------------------
template <int MG, int NW>
struct MxgSkinnyRegs { u32x4 w[NW][4]; u32x4 a[MG][4]; int sw[NW]; int sa[MG]; };

template <typename TO, int MG, bool FUSED>
__device__ __forceinline__ void mxg_skinny_body(const MxgArgs& p, int4 entry, int split, int n0, int r, int g) {
  constexpr int NW = FUSED ? 2 : 1;                                        // weight streams: the rows, or gate rows and up rows
  const int row0 = entry.y, rows = entry.z;
  const int st_begin = split * p.per, st_end = min(p.nst, st_begin + p.per);
  const uint8_t* w_row[NW];
  const uint8_t* sw_row[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const int64_t wr = static_cast<int64_t>(entry.x) * p.N + w * p.I + n0 + r;
    w_row[w] = p.w + wr * p.K2;
    sw_row[w] = p.sw + wr * p.KB;
  }
  const uint8_t* a_row[MG];
  const uint8_t* sa_row[MG];
#pragma unroll
  for (int mg = 0; mg < MG; ++mg) {
    const int64_t m = row0 + min(mg * 16 + r, rows - 1);
    a_row[mg] = p.a + m * p.K2;
    sa_row[mg] = p.sa + m * p.KB;
  }
  auto request = [&](int st, MxgSkinnyRegs<MG, NW>& x) {
    const int off = st * MX_ST_BYTES + g * 64, b0 = st * MX_ST_BLOCKS + 4 * g;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
#pragma unroll
      for (int s = 0; s < 4; ++s) x.w[w][s] = mx_chunk(w_row[w], off + 16 * s, p.K2);
      x.sw[w] = mx_scale4(sw_row[w], b0, p.KB);
    }
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) {
#pragma unroll
      for (int s = 0; s < 4; ++s) x.a[mg][s] = mx_chunk(a_row[mg], off + 16 * s, p.K2);
      x.sa[mg] = mx_scale4(sa_row[mg], b0, p.KB);
    }
  };

  f32x4 acc[NW][MG];
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) acc[w][mg] = f32x4{0.f, 0.f, 0.f, 0.f};
  MxgSkinnyRegs<MG, NW> cur, next;
  request(st_begin, cur);
  for (int st = st_begin; st < st_end; ++st) {
    if (st + 1 < st_end) request(st + 1, next);
    static_for<4>([&](auto s_c) {
      constexpr int s = decltype(s_c)::value;
#pragma unroll
      for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) acc[w][mg] = mx_mma<s>(cur.w[w][s], cur.a[mg][s], acc[w][mg], cur.sw[w], cur.sa[mg]);
    });
    if (st + 1 < st_end) cur = next;
  }

#pragma unroll
  for (int mg = 0; mg < MG; ++mg) {
    const int local = mg * 16 + r;
    if (local >= rows) continue;
    const int n = n0 + 4 * g;
    if (!FUSED && p.S == 1) {
      mx_store4<TO>(static_cast<TO*>(p.out) + static_cast<int64_t>(row0 + local) * p.N + n, acc[0][mg]);
      continue;
    }
    float* part = p.part + (static_cast<int64_t>(split) * p.part_rows + entry.w + local) * p.N + n;
#pragma unroll
    for (int w = 0; w < NW; ++w) *reinterpret_cast<f32x4*>(part + w * p.I) = acc[w][mg];
  }
}

// one wave per (skinny entry, split, 16 weight rows): item = (entry * S + split) * tiles16 + tile
template <typename TO, bool FUSED>
__global__ __launch_bounds__(MX_THREADS) void mxg_skinny_kernel(MxgArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles16 = (FUSED ? p.I : p.N) / 16;
  const int64_t item = static_cast<int64_t>(blockIdx.x) * (MX_THREADS / 64) + wave;
  const int slot = static_cast<int>(item / (static_cast<int64_t>(tiles16) * p.S));
  if (slot >= p.header[1]) return;
  const int rest = static_cast<int>(item - static_cast<int64_t>(slot) * tiles16 * p.S);
  const int4 entry = p.skinny[slot];
  if (entry.z <= 16) mxg_skinny_body<TO, 1, FUSED>(p, entry, rest / tiles16, (rest % tiles16) * 16, lane & 15, lane >> 4);
  else mxg_skinny_body<TO, 2, FUSED>(p, entry, rest / tiles16, (rest % tiles16) * 16, lane & 15, lane >> 4);
}

// sum of the splits, in split order, of four consecutive columns of a partial row
__device__ __forceinline__ f32x4 mxg_merged(const MxgArgs& p, int64_t part_row, int col) {
  f32x4 sum = *reinterpret_cast<const f32x4*>(p.part + part_row * p.N + col);
  for (int s = 1; s < p.S; ++s) sum += *reinterpret_cast<const f32x4*>(p.part + (static_cast<int64_t>(s) * p.part_rows + part_row) * p.N + col);
  return sum;
}

// blockIdx.y: skinny entry; a thread: four consecutive columns of one of its rows
template <typename TO>
__global__ __launch_bounds__(MX_THREADS) void mxg_merge_kernel(MxgArgs p) {
  if (static_cast<int>(blockIdx.y) >= p.header[1]) return;
  const int4 entry = p.skinny[blockIdx.y];
  const int quads = p.N / 4, idx = blockIdx.x * MX_THREADS + threadIdx.x;
  if (idx >= entry.z * quads) return;
  const int local = idx / quads, col = (idx % quads) * 4;
  mx_store4<TO>(static_cast<TO*>(p.out) + static_cast<int64_t>(entry.y + local) * p.N + col, mxg_merged(p, entry.w + local, col));
}

// the same walk over the I / 4 column quads of the activation: eight lanes a block
__global__ __launch_bounds__(MX_THREADS) void mxg_merge_swiglu_kernel(MxgArgs p) {
  if (static_cast<int>(blockIdx.y) >= p.header[1]) return;
  const int4 entry = p.skinny[blockIdx.y];
  const int quads = p.I / 4, idx = blockIdx.x * MX_THREADS + threadIdx.x;  // (quads is a multiple of 8: whole eights leave together)
  if (idx >= entry.z * quads) return;
  const int local = idx / quads, col = (idx % quads) * 4;
  const int64_t m = entry.y + local;
  mx_swiglu_quant8(mxg_merged(p, entry.w + local, col), mxg_merged(p, entry.w + local, p.I + col),
                   static_cast<uint8_t*>(p.out) + m * (p.I / 2) + col / 2, p.out_scale + m * (p.I / MX_BLOCK) + col / MX_BLOCK,
                   col % MX_BLOCK == 0);
}

// ---- the stand-alone stage --------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(MX_THREADS) void mx_swiglu_quant_kernel(const T* x, uint8_t* data, uint8_t* scale, int64_t m, int inter,
                                                                     int64_t row_stride) {
  const int quads = inter / 4;                                             // a multiple of 8
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * MX_THREADS + threadIdx.x;
  if (idx >= m * quads) return;
  const int64_t row = idx / quads;
  const int col = static_cast<int>(idx - row * quads) * 4;
  const typename vec_of<T, 4>::type gate = load_vec<T, 4>(x + row * row_stride + col);
  const typename vec_of<T, 4>::type up = load_vec<T, 4>(x + row * row_stride + inter + col);
  f32x4 gate_f, up_f;
#pragma unroll
  for (int e = 0; e < 4; ++e) { gate_f[e] = elt<T>::to_f(gate[e]); up_f[e] = elt<T>::to_f(up[e]); }
  mx_swiglu_quant8(gate_f, up_f, data + row * (inter / 2) + col / 2, scale + row * (inter / MX_BLOCK) + col / MX_BLOCK,
                   col % MX_BLOCK == 0);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct MxgPlan { int nst, S, per, nt, ns, part_rows; int64_t tiles_at, skinny_at, part_at, bytes; };

MxgPlan mxg_plan(int64_t m, int64_t k, int64_t n, int64_t groups, bool fused) {
  MxgPlan pl;
  pl.nst = static_cast<int>(ceil_div(k, 2 * MX_ST_BYTES));
  pl.nt = static_cast<int>(ceil_div(m, MX_TILE) + groups);
  pl.ns = static_cast<int>(std::min(groups, m));
  pl.part_rows = static_cast<int>(std::min<int64_t>(m, static_cast<int64_t>(MX_SKINNY_MAX_M) * pl.ns));
  const int64_t waves = std::max<int64_t>(1, (fused ? n / 2 : n) / 16 * pl.ns);        // of one split, every entry in use
  const int s = static_cast<int>(std::min<int64_t>(std::min<int64_t>(std::max<int64_t>(1, MX_SKINNY_WAVES / waves), pl.nst), MX_MAX_SPLIT));
  pl.per = static_cast<int>(ceil_div(pl.nst, s));
  pl.S = static_cast<int>(ceil_div(pl.nst, pl.per));                      // (no empty split)
  pl.tiles_at = MXG_HEADER_BYTES;
  pl.skinny_at = pl.tiles_at + static_cast<int64_t>(pl.nt) * 16;
  pl.part_at = pl.skinny_at + static_cast<int64_t>(pl.ns) * 16;
  pl.bytes = pl.part_at + (fused || pl.S > 1 ? static_cast<int64_t>(pl.S) * pl.part_rows * n * 4 : 0);
  return pl;
}

template <typename TO, bool FUSED>
int mxg_launch(const MxgPlan& pl, MxgArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(mxg_plan_kernel, dim3(1), dim3(MX_THREADS), 0, s, a);
  MOJO_CHECK_LAUNCH("mxfp4_group_gemm(plan)");
  const dim3 tile_grid(static_cast<unsigned>(FUSED ? ceil_div(a.I, 64) : ceil_div(a.N, MX_TILE)), static_cast<unsigned>(pl.nt));
  hipLaunchKernelGGL((mxg_tile_kernel<TO, FUSED>), tile_grid, dim3(MX_THREADS), 0, s, a);
  MOJO_CHECK_LAUNCH("mxfp4_group_gemm(tile)");
  const int64_t items = static_cast<int64_t>(pl.ns) * pl.S * ((FUSED ? a.I : a.N) / 16);
  hipLaunchKernelGGL((mxg_skinny_kernel<TO, FUSED>), dim3(static_cast<unsigned>(ceil_div(items, MX_THREADS / 64))), dim3(MX_THREADS),
                     0, s, a);
  MOJO_CHECK_LAUNCH("mxfp4_group_gemm(skinny)");
  if (FUSED) {
    const dim3 grid(static_cast<unsigned>(ceil_div(static_cast<int64_t>(MX_SKINNY_MAX_M) * (a.I / 4), MX_THREADS)), static_cast<unsigned>(pl.ns));
    hipLaunchKernelGGL(mxg_merge_swiglu_kernel, grid, dim3(MX_THREADS), 0, s, a);
    MOJO_CHECK_LAUNCH("mxfp4_group_gemm(merge)");
  } else if (pl.S > 1) {
    const dim3 grid(static_cast<unsigned>(ceil_div(static_cast<int64_t>(MX_SKINNY_MAX_M) * (a.N / 4), MX_THREADS)), static_cast<unsigned>(pl.ns));
    hipLaunchKernelGGL((mxg_merge_kernel<TO>), grid, dim3(MX_THREADS), 0, s, a);
    MOJO_CHECK_LAUNCH("mxfp4_group_gemm(merge)");
  }
  note_launch("mxfp4_group_gemm:%s:splitk%d", FUSED ? "swiglu" : "plain", pl.S);
  return 0;
}

bool mxg_shape_ok(int64_t m, int64_t k, int64_t n, int64_t groups) {
  return m >= 0 && k > 0 && n > 0 && groups > 0 && k % MX_BLOCK == 0;
}

}  // namespace
}  // namespace mojo

using namespace mojo;

extern "C" int64_t mojo_hip_mxfp4_group_gemm_workspace_bytes(int64_t m_total, int64_t k, int64_t n, int64_t num_groups, int swiglu_quant) {
  if (!mxg_shape_ok(m_total, k, n, num_groups) || m_total == 0 || num_groups > MXG_MAX_GROUPS || m_total >= (int64_t{1} << 31) ||
      n >= (int64_t{1} << 31))
    return 16;
  return mxg_plan(m_total, k, n, num_groups, swiglu_quant != 0).bytes;
}

extern "C" int mojo_hip_mxfp4_group_gemm(const void* input, const void* input_scale, const void* weight, const void* weight_scale,
                                         void* out, void* out_scale, const void* group_list, int64_t m_total, int64_t k, int64_t n,
                                         int64_t num_groups, int swiglu_quant, int out_dtype, void* workspace, int64_t workspace_bytes,
                                         mojo_stream_t stream) {
  const char* what = "mxfp4_group_gemm";
  const bool fused = swiglu_quant != 0;
  MOJO_REQUIRE(mxg_shape_ok(m_total, k, n, num_groups), MOJO_EINVAL, "%s: bad shape (k %lld must be a positive multiple of %d)", what,
               (long long)k, MX_BLOCK);
  MOJO_REQUIRE(n % 16 == 0, MOJO_EUNSUPPORTED, "%s: n %lld (multiples of 16 are supported)", what, (long long)n);
  MOJO_REQUIRE(!fused || n % (2 * MX_BLOCK) == 0, MOJO_EINVAL, "%s: swiglu_quant wants n = 2 I with I a multiple of %d, got n %lld", what,
               MX_BLOCK, (long long)n);
  MOJO_REQUIRE(fused || out_dtype == MOJO_F32 || out_dtype == MOJO_F16 || out_dtype == MOJO_BF16, MOJO_EUNSUPPORTED,
               "%s: fp32, fp16 and bf16 outputs only", what);
  MOJO_REQUIRE(num_groups <= MXG_MAX_GROUPS, MOJO_EUNSUPPORTED, "%s: %lld groups (at most %d)", what, (long long)num_groups, MXG_MAX_GROUPS);
  MOJO_REQUIRE(k < (int64_t{1} << 31) && n < (int64_t{1} << 31) && m_total < (int64_t{1} << 31) &&
               ceil_div(m_total, MX_TILE) + num_groups < 65536 &&
               std::min(num_groups, m_total) * MX_MAX_SPLIT * (n / 16) < (int64_t{1} << 31), MOJO_EUNSUPPORTED,
               "%s: sizes beyond the launch's range", what);
  if (m_total == 0) return 0;
  MOJO_REQUIRE(input && input_scale && weight && weight_scale && out && group_list && (!fused || out_scale), MOJO_EINVAL,
               "%s: null pointer", what);
  MOJO_REQUIRE(aligned_to(input, 16) && aligned_to(weight, 16) && aligned_to(out, 16) && aligned_to(group_list, 4), MOJO_EUNSUPPORTED,
               "%s: input, weight and out must be 16-byte aligned", what);
  const MxgPlan pl = mxg_plan(m_total, k, n, num_groups, fused);
  MOJO_REQUIRE(workspace && workspace_bytes >= pl.bytes && aligned_to(workspace, 16), MOJO_EWORKSPACE, "%s: workspace too small", what);
  MxgArgs a;
  a.a = static_cast<const uint8_t*>(input); a.sa = static_cast<const uint8_t*>(input_scale);
  a.w = static_cast<const uint8_t*>(weight); a.sw = static_cast<const uint8_t*>(weight_scale);
  a.out = out; a.out_scale = static_cast<uint8_t*>(out_scale);
  a.counts = static_cast<const int*>(group_list);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  a.header = reinterpret_cast<int*>(ws); a.tiles = reinterpret_cast<int4*>(ws + pl.tiles_at);
  a.skinny = reinterpret_cast<int4*>(ws + pl.skinny_at); a.part = reinterpret_cast<float*>(ws + pl.part_at);
  a.M = static_cast<int>(m_total); a.G = static_cast<int>(num_groups); a.N = static_cast<int>(n); a.I = fused ? static_cast<int>(n / 2) : 0;
  a.K2 = static_cast<int>(k / 2); a.KB = static_cast<int>(k / MX_BLOCK);
  a.nst = pl.nst; a.S = pl.S; a.per = pl.per; a.nt = pl.nt; a.ns = pl.ns; a.part_rows = pl.part_rows;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (fused) return mxg_launch<float, true>(pl, a, s);
  if (out_dtype == MOJO_F32) return mxg_launch<float, false>(pl, a, s);
  if (out_dtype == MOJO_F16) return mxg_launch<f16_t, false>(pl, a, s);
  return mxg_launch<bf16_t, false>(pl, a, s);
}

extern "C" int mojo_hip_mxfp4_swiglu_quant(const void* x, void* data, void* scale, int64_t m, int64_t inter, int64_t row_stride,
                                           int dtype, mojo_stream_t stream) {
  const char* what = "mxfp4_swiglu_quant";
  MOJO_REQUIRE(m >= 0 && inter > 0 && inter % MX_BLOCK == 0, MOJO_EINVAL, "%s: inter %lld must be a positive multiple of %d", what,
               (long long)inter, MX_BLOCK);
  MOJO_REQUIRE(dtype == MOJO_F32 || dtype == MOJO_BF16 || dtype == MOJO_F16, MOJO_EUNSUPPORTED, "%s: fp32, bf16 and fp16 only", what);
  MOJO_REQUIRE(inter < (int64_t{1} << 30) && ceil_div(m * (inter / 4), MX_THREADS) < (int64_t{1} << 31), MOJO_EUNSUPPORTED,
               "%s: sizes beyond the launch's range", what);
  if (m == 0) return 0;
  MOJO_REQUIRE(x && data && scale, MOJO_EINVAL, "%s: null pointer", what);
  MOJO_REQUIRE(aligned_to(x, 16) && aligned_to(data, 2) && row_stride >= 2 * inter && (m == 1 || row_stride % 4 == 0), MOJO_EUNSUPPORTED,
               "%s: x must be 16-byte aligned, the row stride a multiple of 4 elements and at least 2 inter", what);
  const dim3 grid(static_cast<unsigned>(ceil_div(m * (inter / 4), MX_THREADS)));
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* d = static_cast<uint8_t*>(data);
  uint8_t* sc = static_cast<uint8_t*>(scale);
  if (dtype == MOJO_F32)
    hipLaunchKernelGGL((mx_swiglu_quant_kernel<float>), grid, dim3(MX_THREADS), 0, s, static_cast<const float*>(x), d, sc, m,
                       static_cast<int>(inter), row_stride);
  else if (dtype == MOJO_BF16)
    hipLaunchKernelGGL((mx_swiglu_quant_kernel<bf16_t>), grid, dim3(MX_THREADS), 0, s, static_cast<const bf16_t*>(x), d, sc, m,
                       static_cast<int>(inter), row_stride);
  else
    hipLaunchKernelGGL((mx_swiglu_quant_kernel<f16_t>), grid, dim3(MX_THREADS), 0, s, static_cast<const f16_t*>(x), d, sc, m,
                       static_cast<int>(inter), row_stride);
  MOJO_CHECK_LAUNCH(what);
  note_launch("mxfp4_swiglu_quant");
  return 0;
}
