// decode_mfma_kernel: MojoPagedDecodeGQA with the two contractions on the matrix cores (round 3).
// Included by paged_decode_gqa.hip (shares DecodeArgs, the chunking rules, decode_head, the merge kernel and the launch forms;
// the paired prologue, the row prologue, the hole scan, the in-LDS merge, the split epilogue and the softmax step are those of
// paged_decode_common.h — this file holds the tile layouts, the ring and the id windows).
//
// The vector-unit kernel (decode_split_kernel) spends ~600 vector instructions per 16-token tile for four query heads and
// ~1 070 for eight (dot products, DPP butterflies, exponentials and the P V sums, all of them per head): with two waves per
// SIMD that is a latency-bound stream — groups of eight query heads (Llama-3-70B: 64 / 8) ran at 3.0 TB/s however the K/V
// bytes were shared.  Here a tile costs ~60 vector instructions whatever the group size:
//
//   S^T[16 tokens x 16 heads] = K Q^T      v_mfma_f32_16x16x32: A = the K registers AS LOADED, and loaded in WHOLE 128-byte lines (a
//                                          load instruction = 8 tokens x one line; 64-byte runs stream at about half the rate):
//                                          lane l holds chunk (l >> 3) of token (l & 7), which the MFMA sees as row
//                                          (token, parity p = chunk & 1) with k-group g = chunk >> 1.  Row (token, p) meets the
//                                          right query dims only in the product whose B operand holds the chunks 2 g + p: every
//                                          register feeds TWO products (p = 0, 1), each valid in 8 of its 16 rows, and
//                                          S[token] = C0[row token] + C1[row token + 8] — one v_permlane32_swap per score
//                                          register puts two 8-token halves side by side in exactly the layout of the 16-row form.
//                                          B = the query slices (head = l & 15; lanes past the group repeat its last head)
//   online softmax                         lane = (head, tokens 4 g .. 4 g + 3 of every tile): in-lane maximum, one cross-group
//                                          maximum (two lane-row swaps), lazy reference (rescale O only when it grows by 2^8)
//   O^T[D x 16 heads] += V^T P^T           v_mfma_f32_16x16x16: B = the four probabilities of the lane (the accumulator layout of
//                                          S^T IS the B layout: no lane movement), A = V^T from a wave-private 4 KiB LDS image of
//                                          the tile read with ds_read_b64_tr_b16 (32-byte pairs XOR-swizzled by the token: the
//                                          eight row blocks of a half-wave land in eight bank slots)
//
// The LDS image belongs to ONE wave (LDS operations of a wave execute in order): no barrier anywhere in the loop.  Pages must
// hold a multiple of 16 tokens (a tile then lies in one page), head_dim 64 or 128, group size <= 16; everything else takes the
// vector-unit kernel.  Chunking, pairing, in-LDS merge, workspace layout and hole / empty-row semantics are that kernel's: one definition.
//
// The K/V stream is a ring of three tiles (8 KiB each) in registers.  From five tiles on, a wave runs rounds of three tiles
// in which every request is unconditional: the compiler then counts the loads, and processing tile t waits for t's own eight
// loads, vmcnt(23) .. (16), with the loads of t + 1 and t + 2 still outstanding (at head_dim 128 the compiler also puts the
// first selects of the hole zeroing, vmcnt(15) .. (12), in front of the request for t + 2: DESIGN 4.1); the last one to four
// tiles go through a tail of conditional requests.  Page ids never cost a round trip inside the stream: they sit in registers, 60 sub-tiles per window, and are read
// by lane (see `id_window`).  As first written — a loop of conditional requests, the id of every tile fetched by a load —
// the compiled loop waited vmcnt(0) for each id and vmcnt(7) .. (0) right after each request: one tile in flight, none
// while the id travelled.  scripts/check_decode_ring.py reads the waits of the compiled loop (tests/test_isa_decode_ring.py).
#pragma once

namespace mojo {

template <typename T> struct dec_mma;
template <> struct dec_mma<bf16_t> {
  typedef bf16x8 frag8;
  typedef s16x4 frag4;
  static __device__ __forceinline__ f32x4 qk(frag8 a, frag8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ f32x4 pv(frag4 a, frag4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ frag4 pack(float p0, float p1, float p2, float p3) {
    const bf16x4 v = {static_cast<bf16_t>(p0), static_cast<bf16_t>(p1), static_cast<bf16_t>(p2), static_cast<bf16_t>(p3)};
    return __builtin_bit_cast(frag4, v);
  }
  static __device__ __forceinline__ frag4 from_lds(s16x4 v) { return v; }
};
template <> struct dec_mma<f16_t> {
  typedef f16x8 frag8;
  typedef f16x4 frag4;
  static __device__ __forceinline__ f32x4 qk(frag8 a, frag8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ f32x4 pv(frag4 a, frag4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ frag4 pack(float p0, float p1, float p2, float p3) {
    const f16x4 v = {static_cast<f16_t>(p0), static_cast<f16_t>(p1), static_cast<f16_t>(p2), static_cast<f16_t>(p3)};
    return v;
  }
  static __device__ __forceinline__ frag4 from_lds(s16x4 v) { return __builtin_bit_cast(f16x4, v); }
};

constexpr int DECM_TILE = 16;                 // tokens of a sub-tile (one S^T product set, one V image)

//
// decode_mfma_nstep_kernel (MojoPagedDecodeNstepSWA, DecodeSteps): the 16 columns hold (step, head) pairs of a block of 16 / G query
// steps instead of G heads and 16 - G repeats; a grid row is a (sequence, kv head, block of steps).  The instance walks a
// DecodeWin like the windowed ones (SWA is set; no window: a local window of the launch capacity, and the hole scan runs),
// masks both staircases per lane, and leaves partials of NC = (16 / G) G columns.
//
// The two kernels share one body, paged_decode_mfma_body.h, included into each: as a function called by both, the body is
// optimised on its own before it is inlined, and the single-step instances no longer compile to the code they compiled to
// (their symbols and that code are pinned: tests/test_isa_decode_ring.py counts and reads them).
template <typename T, int DK /* head_dim / 32 */, bool NT, int MODE, bool SWA = false /* sliding window: DecodeWin */>
__global__ __launch_bounds__(MODE != DEC_SPLIT ? 512 : 64) void decode_mfma_kernel(DecodeArgs a, int G) {
  constexpr bool NSTEP = false;
#include "paged_decode_mfma_body.h"
}

// MODE: DEC_SPLIT or DEC_FUSED; `G` arrives as decode_nstep_arg(heads per kv head, steps, scan_holes)
template <typename T, int DK, bool NT, int MODE>
__global__ __launch_bounds__(MODE != DEC_SPLIT ? 512 : 64) void decode_mfma_nstep_kernel(DecodeArgs a, int G) {
  constexpr bool NSTEP = true, SWA = true;
#include "paged_decode_mfma_body.h"
}

}  // namespace mojo
