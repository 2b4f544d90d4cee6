// The expert of a row, found on the device from the per-expert row counts: what moe_quant_kernel (quant_moe.hip) and
// dequant_swiglu_quant_kernel (dequant_swiglu_quant.hip) share.  The rows arrive sorted by expert; every workgroup scans the
// counts into LDS (one wave, 64 counts per step) and searches the scan per row — no prefix launch, no host synchronisation.
// Negative counts read as zero; the scan is clamped to the rows there are; the rows past it get zeros and scale 1.
#pragma once
#include "common.h"

namespace mojo {

constexpr int MOE_QUANT_MAX_EXPERTS = 1024;

// Exclusive scan of `counts` [E] (int32, or int64 when `counts_i64`) into s_start[0..E]; s_start[E] is the number of rows an
// expert owns.  Called by every thread of a 256-thread workgroup; ends with a barrier.
__device__ __forceinline__ void moe_scan_counts(const void* __restrict__ counts, int counts_i64, int E, int64_t rows,
                                                long long* s_start) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 64) {                                            // exclusive scan of the counts, clamped to the rows there are
    long long carry = 0;
    for (int base = 0; base < E; base += 64) {
      const int g = base + lane;
      long long c = 0;
      if (g < E) c = counts_i64 ? static_cast<long long>(static_cast<const int64_t*>(counts)[g]) : static_cast<long long>(static_cast<const int32_t*>(counts)[g]);
      if (c < 0) c = 0;
      long long incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const long long v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
      }
      if (g < E) s_start[g] = min(carry + incl - c, static_cast<long long>(rows));
      carry += __shfl(incl, 63);
    }
    if (lane == 0) s_start[E] = min(carry, static_cast<long long>(rows));
  }
  __syncthreads();
}

// The largest e with s_start[e] <= row, for a row below s_start[E].
__device__ __forceinline__ int moe_expert_of_row(const long long* s_start, int E, int64_t row) {
  int lo = 0, hi = E;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s_start[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

// A row at or past s_start[E], which no expert owns: int8 zeros and scale 1.  Called by every thread of the workgroup.
template <int VEC>
__device__ __forceinline__ void moe_zero_unowned_row(unsigned char* q_row, float* out_scale, int n_vec) {
  for (int v = threadIdx.x; v < n_vec; v += 256) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) q_row[v * VEC + j] = 0;
  }
  if (threadIdx.x == 0) *out_scale = 1.0f;
}

}  // namespace mojo
