// The one total order of the selections (segment_topk / segment_rank in recommend.hip, the short lists of mips.hip).
#pragma once
#include "common.h"

constexpr int TOPK_MAX = 2 * OCN_WAVE;                       // the longest sorted list a wave keeps: two slots per lane

// The order of the contract as ONE unsigned comparison (larger = better): the high word is the score's monotone image —
// -0.0 is folded onto +0.0 first, every NaN goes to 0, below -inf (0x007fffff) — the low word is ~(position in the segment),
// so that among equal scores (and among NaNs) the lower position wins.  A segment has fewer than 2^32 - 1 entries: no entry
// has the key 0, which marks an empty slot.
__device__ __forceinline__ unsigned topk_image(float x) {    // the high word alone (segment_keep.hip selects on it)
  unsigned b = __float_as_uint(x);
  if (b == 0x80000000u) b = 0u;
  unsigned u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  if (x != x) u = 0u;
  return u;
}

__device__ __forceinline__ u64 topk_key(float x, unsigned rel) {
  return ((u64)topk_image(x) << 32) | (u64)(0xffffffffu - rel);
}

__device__ __forceinline__ u64 topk_shfl_up1(u64 v) {
  const unsigned lo = __shfl_up((unsigned)v, 1, OCN_WAVE), hi = __shfl_up((unsigned)(v >> 32), 1, OCN_WAVE);
  return ((u64)hi << 32) | lo;
}
