// One window of a 2-hop row difference as a bitmap in LDS: steps 1 - 3 of two_hop_diff_kernel (recommend.hip), shared with the
// sampler that selects from the same bitmap (neg_sample.hip) so that the two cannot disagree about a candidate set.
#pragma once
#include "common.h"

// first position of the sorted row a[0..n) whose column is not below key; the same steps and the same loads in every lane
// (not common.h's sorted_has: it returns the position, and the key is a 64-bit window bound)
__device__ __forceinline__ i64 th_lower_bound(const int32_t* __restrict__ a, i64 n, i64 key) {
  i64 lo = 0, hi = n;
  while (lo < hi) {
    const i64 mid = lo + ((hi - lo) >> 1);
    if ((i64)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// bm[0..words) = the part of ( U_{m in A[s,:]} A[m,:] ) \ M[s,:] inside the columns [w0, w1), without s under drop_self; bit k of the
// bitmap is column w0 + k.  a0, da / m0, dm: start and length of row s in A / in M; words = (w1 - w0 + 31) >> 5.
//   1. the bitmap is cleared;
//   2. a wave takes a neighbour m of s, finds where row m enters the window (binary search, skipped for the first window)
//      and sets a bit per column below w1 — LDS atomicOr: the lanes of a wave, and the waves, do meet in one word;
//   3. the bits of M[s,:] inside the window, and of s itself under drop_self, are cleared (atomicAnd).
// Called by the whole workgroup (three barriers, the last one behind step 3: the bitmap is ready on return); the caller puts
// a barrier between its last read of the bitmap and the next call.  A column outside [w0, w1) never touches the bitmap,
// whatever the rows hold.
__device__ __forceinline__ void th_window_bitmap(unsigned* bm, const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
                                                 i64 a0, i64 da, const int32_t* __restrict__ colM, i64 m0, i64 dm, i64 s,
                                                 int drop_self, i64 w0, i64 w1, int words) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int w = threadIdx.x; w < words; w += OCN_BLOCK) bm[w] = 0u;
  __syncthreads();
  for (i64 t = wave; t < da; t += OCN_WPB) {
    const i64 m = colA[a0 + t];
    const i64 b0 = rowptrA[m], db = rowptrA[m + 1] - b0;
    const i64 lo = w0 > 0 ? th_lower_bound(colA + b0, db, w0) : 0;
    for (i64 p = lo + lane; p < db; p += OCN_WAVE) {
      const i64 c = colA[b0 + p];
      if (c >= w1) break;                                // (sorted: so is every later column of this lane)
      if (c >= w0) {
        const unsigned k = (unsigned)(c - w0);
        atomicOr(&bm[k >> 5], 1u << (k & 31u));
      }
    }
  }
  __syncthreads();
  const i64 lo_m = w0 > 0 ? th_lower_bound(colM + m0, dm, w0) : 0;
  for (i64 p = lo_m + threadIdx.x; p < dm; p += OCN_BLOCK) {
    const i64 c = colM[m0 + p];
    if (c >= w1) break;
    if (c >= w0) {
      const unsigned k = (unsigned)(c - w0);
      atomicAnd(&bm[k >> 5], ~(1u << (k & 31u)));
    }
  }
  if (drop_self && threadIdx.x == 0 && s >= w0 && s < w1) {
    const unsigned k = (unsigned)(s - w0);
    atomicAnd(&bm[k >> 5], ~(1u << (k & 31u)));
  }
  __syncthreads();
}

// Step 4's first half: the bits of this thread's contiguous words [t0, t1) of the window's bitmap — ascending columns in thread
// order, so the block scan of these counts places a thread's columns behind those of the threads below it.
__device__ __forceinline__ i64 th_thread_bits(const unsigned* bm, int words, int& t0, int& t1) {
  const int wpt = (words + OCN_BLOCK - 1) / OCN_BLOCK;
  t0 = (int)threadIdx.x * wpt < words ? (int)threadIdx.x * wpt : words;
  t1 = (t0 + wpt) < words ? (t0 + wpt) : words;
  i64 c = 0;
  for (int w = t0; w < t1; ++w) c += __popc(bm[w]);
  return c;
}
