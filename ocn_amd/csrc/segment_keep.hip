// Short lists beyond the wave-wide top-k: the m best entries of every segment of a flat score vector as a SET, in position
// order, for any m.  See include/ocn_hip.h (ocn_segment_keep_best).  A short list is not a ranking: it needs the cut — the
// min(m, len)-th best key in the one total order (topk_key.h) — and the entries that are not worse than it, in the order they
// already have.  So nothing is sorted and no [Q, m] rectangle is formed: a radix select finds the cut, one ordered compaction
// emits the survivors.
#include "common.h"
#include "topk_key.h"

constexpr int KEEP_BINS = 256;                               // 8 bits of the image per pass, four passes, MSB first
constexpr int KEEP_PER_THREAD = 4;                           // consecutive entries a thread takes of a compaction tile
constexpr int KEEP_TILE = OCN_BLOCK * KEEP_PER_THREAD;

// the smallest key of the workgroup (copied-through segments report their worst entry): waves by shuffle, then through LDS
__device__ __forceinline__ u64 keep_block_min(u64 v, u64* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, OCN_WAVE), hi = __shfl_xor((unsigned)(v >> 32), o, OCN_WAVE);
    const u64 t = ((u64)hi << 32) | lo;
    v = t < v ? t : v;
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 r = sh[0];
#pragma unroll
  for (int i = 1; i < OCN_WPB; ++i) r = sh[i] < r ? sh[i] : r;
  __syncthreads();
  return r;
}

// A workgroup owns segment q, grid-stride over Q (the longest segment sets the tail of the launch, as it does for
// segment_topk and segment_rank: a segment is not split over workgroups).
//   len <= m: every entry is kept — positions copied through, no selection.
//   else    : the image of the m-th best entry is found 8 bits at a time, MSB first.  Pass j counts, in a 256-bin LDS
//             histogram, byte 3 - j of every image whose higher bytes equal the prefix fixed so far (integer LDS atomics: a
//             count does not depend on their order); the bins are then walked downwards — one bin per thread, best bin in
//             thread 0, a block scan gives every bin the count of the better ones — to the bin that holds the `want`-th
//             best, which extends the prefix; `want` drops by the entries of the better bins.  After four passes the prefix
//             is the cut image U and want = r >= 1: the r FIRST entries with image U are kept (the tie rule of topk_key, and
//             the rule among NaNs, whose image is 0).
//             One ordered pass then compacts: an entry is kept if its image is above U, or equals U with fewer than r equal
//             entries before it.  The scan carries both counts in one word (better in the high half, equal in the low), so
//             the place of a kept entry is base + better-before + min(equal-before, r): one block scan per tile.
// Every barrier is reached by the whole workgroup: the branches and trip counts around them depend on q, len, m and the
// kernel arguments alone.  A store is bounded by the segment's own [ptr_m[q], ptr_m[q + 1]) whatever the scores hold.
__global__ __launch_bounds__(OCN_BLOCK) void segment_keep_kernel(
    const float* __restrict__ scores, const i64* __restrict__ ptr, i64 Q, i64 m, const i64* __restrict__ ptr_m,
    i64* __restrict__ keep_pos, u64* __restrict__ cut) {
  __shared__ unsigned s_hist[KEEP_BINS];
  __shared__ i64 sh[2 * OCN_WPB];
  __shared__ unsigned s_sel[2];                              // the chosen bin, what is still wanted inside it
  static_assert(KEEP_BINS == OCN_BLOCK, "the bucket walk gives every thread one bin");
  const int tid = threadIdx.x;
  for (i64 q = blockIdx.x; q < Q; q += gridDim.x) {
    const i64 b = ptr[q], n = ptr[q + 1] - b;
    const i64 o0 = ptr_m[q], o1 = ptr_m[q + 1];
    if (n <= m) {                                            // copied through (n <= 0: nothing, and the cut of nothing is 0)
      u64 worst = ~0ull;
      for (i64 p = tid; p < n; p += OCN_BLOCK) {
        const i64 at = o0 + p;
        if (at < o1) keep_pos[at] = b + p;
        if (cut) { const u64 key = topk_key(scores[b + p], (unsigned)p); worst = key < worst ? key : worst; }
      }
      if (cut) {
        worst = keep_block_min(worst, (u64*)sh);
        if (tid == 0) cut[q] = n > 0 ? worst : 0ull;
      }
      continue;
    }
    // ---- the cut: (U, r) ----
    unsigned prefix = 0u, want = (unsigned)m;                // (m < n < 2^32 - 1)
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
      const unsigned fixed = shift == 24 ? 0u : ~0u << (shift + 8);      // the bits of the prefix that are decided
      s_hist[tid] = 0u;
      __syncthreads();
      for (i64 p = tid; p < n; p += OCN_BLOCK) {
        const unsigned u = topk_image(scores[b + p]);
        if (((u ^ prefix) & fixed) == 0u) atomicAdd(&s_hist[(u >> shift) & 255u], 1u);
      }
      __syncthreads();
      const unsigned bin = (unsigned)(KEEP_BINS - 1 - tid);  // thread 0 holds the best bin
      const i64 h = (i64)s_hist[bin];
      i64 tot;
      const i64 better = block_excl_scan(h, sh, &tot);       // the entries of the bins above this one
      if (better < (i64)want && (i64)want <= better + h) { s_sel[0] = bin; s_sel[1] = want - (unsigned)better; }
      __syncthreads();                                       // (exactly one bin qualifies: the prefix's class holds >= want)
      prefix |= s_sel[0] << shift;
      want = s_sel[1];
      __syncthreads();                                       // the next pass's clear and s_sel stay behind these reads
    }
    const unsigned U = prefix;
    const i64 r = (i64)want;
    // ---- ordered compaction ----
    i64 better_seen = 0, equal_seen = 0;
    for (i64 c0 = 0; c0 < n; c0 += KEEP_TILE) {
      const i64 p0 = c0 + (i64)tid * KEEP_PER_THREAD;
      unsigned u[KEEP_PER_THREAD];
      i64 v = 0;
#pragma unroll
      for (int i = 0; i < KEEP_PER_THREAD; ++i) {
        const i64 p = p0 + i;
        u[i] = p < n ? topk_image(scores[b + p]) : 0u;
        if (p < n) v += u[i] > U ? (1ll << 32) : (u[i] == U ? 1ll : 0ll);
      }
      i64 tot;
      const i64 ex = block_excl_scan(v, sh, &tot);
      i64 gt = better_seen + (ex >> 32), eq = equal_seen + (ex & 0xffffffffll);
#pragma unroll
      for (int i = 0; i < KEEP_PER_THREAD; ++i) {
        const i64 p = p0 + i;
        if (p < n) {
          const bool above = u[i] > U, same = u[i] == U;
          if (above || (same && eq < r)) {
            const i64 at = o0 + gt + (eq < r ? eq : r);
            if (at >= o0 && at < o1) keep_pos[at] = b + p;
            if (cut && same && eq == r - 1) cut[q] = ((u64)U << 32) | (u64)(0xffffffffu - (unsigned)p);
          }
          gt += above ? 1 : 0;
          eq += same ? 1 : 0;
        }
      }
      better_seen += tot >> 32;
      equal_seen += tot & 0xffffffffll;
    }
  }
}

extern "C" {

int ocn_segment_keep_best(const float* scores, const int64_t* ptr, int64_t Q, int64_t m, const int64_t* ptr_m,
                          int64_t* keep_pos, uint64_t* cut, void* stream) {
  if (Q < 0 || m < 1 || m > 0x7fffffffll || !ptr || !ptr_m || !keep_pos) return OCN_EINVAL;
  if (Q == 0) return 0;
  if (!scores) return OCN_EINVAL;
  hipLaunchKernelGGL(segment_keep_kernel, dim3((unsigned)grid_for(Q, 256 * 8)), dim3(OCN_BLOCK), 0, (hipStream_t)stream, scores,
                     (const i64*)ptr, (i64)Q, (i64)m, (const i64*)ptr_m, (i64*)keep_pos, (u64*)cut);
  return launch_status();
}

}  // extern "C"
