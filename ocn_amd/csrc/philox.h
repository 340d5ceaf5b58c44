// Philox4x32-10 and the counter streams of everything random in the library: the structured negative samplers
// (neg_sample.hip), the random-walk retrieval (rw_retrieve.hip) and the capped pooling's strata (cn_pool_cap.hip).  One generator, one key rule, one stream word per use.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants)
// ---------------------------------------------------------------------------------------------
constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr unsigned PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr unsigned SAMPLE_STREAM_PAIRS = 1u, SAMPLE_STREAM_ROWS = 2u;      // counter word 3: the samplers never share a word
constexpr unsigned SAMPLE_STREAM_TWO_HOP = 3u, SAMPLE_STREAM_TWO_HOP_ID = 4u;
constexpr unsigned SAMPLE_STREAM_RW_A = 5u, SAMPLE_STREAM_RW_B = 6u;       // random-walk retrieval: steps 1 | 2 of a walk, step 3
constexpr unsigned SAMPLE_STREAM_CN_CAP = 7u;                              // capped pooling: the pick of stratum t of candidate (i, j)

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = __umulhi(PHILOX_M0, c.x), lo0 = PHILOX_M0 * c.x;
    const unsigned hi1 = __umulhi(PHILOX_M1, c.z), lo1 = PHILOX_M1 * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return c;
}

// r = floor(u * m / 2^64) for the 64-bit word of a counter: uniform over [0, m) up to a bias below m / 2^64
__device__ __forceinline__ u64 sample_rank(uint4 ctr, u64 seed, u64 m) {
  const uint4 w = philox4x32_10(ctr, (unsigned)seed, (unsigned)(seed >> 32));
  return __umul64hi((u64)w.x | ((u64)w.y << 32), m);
}

// The capped pooling's sample (cn_pool_cap.hip, cn_pool_q8.hip; include/ocn_hip.h states it).  The multiplier of the member
// of rank r among u > d members: its stratum's size where it is the stratum's pick, else 0.  T: an unsigned type that holds
// u * d.
template <typename T>
__device__ __forceinline__ int32_t cap_multiplier(T r, T u, T d, unsigned i, unsigned j, u64 seed) {
  const T t = r * d / u;                                   // the stratum of rank r
  const T lo = (t * u + d - 1) / d, hi = ((t + 1) * u + d - 1) / d;
  const T s = hi - lo;                                     // floor(u / d) or ceil(u / d), never 0
  const u64 pick = (u64)lo + sample_rank(make_uint4(i, j, (unsigned)t, SAMPLE_STREAM_CN_CAP), seed, (u64)s);
  return (u64)r == pick ? (int32_t)s : 0;
}
