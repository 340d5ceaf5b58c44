// The windowed sweep of a source's candidate columns through a bitmap in LDS, one body per step.  Four kernels sweep this way
// and promise the same set, in the same ascending order, under the same `off` protocol: two_hop_diff_kernel and
// two_hop_sums_kernel (recommend.hip), frontier_kernel (frontier.hip), sample_two_hop_kernel (neg_sample.hip).  Per window
// [w0, w1) of the column range, bit k of the bitmap being column w0 + k:
//   1. the bitmap is cleared                                                        ws_clear
//   2. the members' bits are set, with a sum per column where one is kept           per kernel (ws_set / ws_add)
//   3. the bits of M[s,:] inside the window, and of s under drop_self, are cleared  ws_mask
//   4. every thread counts the bits of its contiguous words, a block scan places    th_thread_bits, ws_emit
//      them behind the query's running base, and the pairs are written
// Step 2 is each kernel's own, on purpose: waves striding the neighbours (th_window_bitmap below), quarters with a search per
// lane (the sums), quarters with a claim table (the frontier) are three algorithms.  The host half below resolves a launch's
// window and raises a kernel's dynamic LDS limit.
#pragma once
#include <atomic>

#include "common.h"

// ---------------------------------------------------------------------------------------------
// lower bounds: the same steps and the same loads in every lane that searches the same list
// ---------------------------------------------------------------------------------------------
// first position of the sorted row a[0..n) whose column is not below key
// (not common.h's sorted_has: it returns the position, and the key is a 64-bit window bound)
__device__ __forceinline__ i64 ws_lower_bound(const int32_t* __restrict__ a, i64 n, i64 key) {
  i64 lo = 0, hi = n;
  while (lo < hi) {
    const i64 mid = lo + ((hi - lo) >> 1);
    if ((i64)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the same over the nodes (the second word of every pair) of the pair list a[b .. b + n); the position counts from b
__device__ __forceinline__ i64 ws_pair_lower_bound(const longlong2* __restrict__ a, i64 b, i64 n, i64 key) {
  i64 lo = 0, hi = n;
  while (lo < hi) {
    const i64 mid = lo + ((hi - lo) >> 1);
    if (a[b + mid].y < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------
// the window's geometry
// ---------------------------------------------------------------------------------------------
// the columns a launch sizes LDS for: the window, or the whole (padded) column range where that is narrower — a small graph
// keeps several workgroups per CU.  The one definition the host's byte count and the kernel's accumulator address share.
__host__ __device__ __forceinline__ i64 ws_span(i64 window, i64 n_cols) {
  const i64 padded = (n_cols + 63) / 64 * 64;
  return window < padded ? window : padded;
}

// the accumulators lie behind the bitmap's span / 32 words (only where the launch asked for them)
__device__ __forceinline__ float* ws_accumulators(unsigned* bm, i64 window, i64 n_cols) {
  return reinterpret_cast<float*>(bm + (ws_span(window, n_cols) >> 5));
}

__device__ __forceinline__ i64 ws_window_end(i64 w0, i64 window, i64 n_cols) { return (w0 + window) < n_cols ? (w0 + window) : n_cols; }
__device__ __forceinline__ int ws_words(i64 w0, i64 w1) { return (int)((w1 - w0 + 31) >> 5); }

// the window's columns dealt to the workgroup's waves in contiguous quarters [q0, q1)  (an empty quarter: q1 <= q0)
__device__ __forceinline__ void ws_quarter(i64 w0, i64 w1, int wave, i64& q0, i64& q1) {
  const i64 quarter = (w1 - w0 + OCN_WPB - 1) / OCN_WPB;
  q0 = w0 + wave * quarter;
  q1 = (q0 + quarter) < w1 ? (q0 + quarter) : w1;
}

// ---------------------------------------------------------------------------------------------
// steps 1 - 3
// ---------------------------------------------------------------------------------------------
// Step 1.  No barrier inside: the caller puts one between its last read of the bitmap and this call, and one behind it.
__device__ __forceinline__ void ws_clear(unsigned* bm, int words) {
  for (int w = threadIdx.x; w < words; w += OCN_BLOCK) bm[w] = 0u;
}

// one member of column k (relative to the window): its presence bit, and the bit taken back (LDS atomics: the lanes of a wave,
// and the waves, do meet in one word)
__device__ __forceinline__ void ws_set(unsigned* bm, unsigned k) { atomicOr(&bm[k >> 5], 1u << (k & 31u)); }
__device__ __forceinline__ void ws_unset(unsigned* bm, unsigned k) { atomicAnd(&bm[k >> 5], ~(1u << (k & 31u))); }

// a member where sums are kept: the presence bit and the accumulator's next partial sum.  The atomicOr's return value tells the
// first member of a column, which adds to 0.0f, from the later ones — so no accumulator is ever cleared.
__device__ __forceinline__ void ws_add(unsigned* bm, float* acc, unsigned k, float f) {
  // Read whatever the bit will say, so that a member costs one LDS round trip, not two.  For a column's first member the slot
  // holds whatever the last window or query left there: that value is only ever SELECTED AWAY below, it never enters the add.
  // (Reading after the atomicOr instead would be as correct and a round trip slower.)
  const unsigned bit = 1u << (k & 31u);
  const float prev = acc[k];
  const unsigned old = atomicOr(&bm[k >> 5], bit);
  acc[k] = __fadd_rn((old & bit) ? prev : 0.0f, f);
}

// Step 3: the bits of M[s,:] inside [w0, w1), and of s itself under drop_self, are cleared (atomicAnd).  m0, dm: start and
// length of row s in M.  No barrier inside: the caller puts one behind its step 2 before this call, and one behind it.
__device__ __forceinline__ void ws_mask(unsigned* bm, const int32_t* __restrict__ colM, i64 m0, i64 dm, i64 s, int drop_self,
                                        i64 w0, i64 w1) {
  const i64 lo_m = w0 > 0 ? ws_lower_bound(colM + m0, dm, w0) : 0;
  for (i64 p = lo_m + threadIdx.x; p < dm; p += OCN_BLOCK) {
    const i64 c = colM[m0 + p];
    if (c >= w1) break;                                      // (sorted: so is every later column of this thread)
    if (c >= w0) ws_unset(bm, (unsigned)(c - w0));
  }
  if (drop_self && threadIdx.x == 0 && s >= w0 && s < w1) ws_unset(bm, (unsigned)(s - w0));
}

// Steps 1 - 3 of the unvalued 2-hop row difference, for the kernels that owe no order to a sum (two_hop_diff_kernel, and the
// sampler that selects from the same bitmap): bm[0..words) = the part of ( U_{m in A[s,:]} A[m,:] ) \ M[s,:] inside [w0, w1),
// without s under drop_self.  a0, da / m0, dm: start and length of row s in A / in M.
//   2. a wave takes a neighbour m of s, finds where row m enters the window (binary search, skipped for the first window)
//      and sets a bit per column below w1.
// Called by the whole workgroup.  Three barriers inside — behind the clear, behind step 2, behind the mask: the bitmap is ready
// on return; the caller puts a barrier between its last read of the bitmap and the next call.  A column outside [w0, w1) never
// touches the bitmap, whatever the rows hold.
__device__ __forceinline__ void th_window_bitmap(unsigned* bm, const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
                                                 i64 a0, i64 da, const int32_t* __restrict__ colM, i64 m0, i64 dm, i64 s,
                                                 int drop_self, i64 w0, i64 w1, int words) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  ws_clear(bm, words);
  __syncthreads();
  for (i64 t = wave; t < da; t += OCN_WPB) {
    const i64 m = colA[a0 + t];
    const i64 b0 = rowptrA[m], db = rowptrA[m + 1] - b0;
    const i64 lo = w0 > 0 ? ws_lower_bound(colA + b0, db, w0) : 0;
    for (i64 p = lo + lane; p < db; p += OCN_WAVE) {
      const i64 c = colA[b0 + p];
      if (c >= w1) break;                                // (sorted: so is every later column of this lane)
      if (c >= w0) ws_set(bm, (unsigned)(c - w0));
    }
  }
  __syncthreads();
  ws_mask(bm, colM, m0, dm, s, drop_self, w0, w1);
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// step 4
// ---------------------------------------------------------------------------------------------
// The bits of this thread's contiguous words [t0, t1) of the window's bitmap — ascending columns in thread order, so the block
// scan of these counts places a thread's columns behind those of the threads below it.
__device__ __forceinline__ i64 th_thread_bits(const unsigned* bm, int words, int& t0, int& t1) {
  const int wpt = (words + OCN_BLOCK - 1) / OCN_BLOCK;
  t0 = (int)threadIdx.x * wpt < words ? (int)threadIdx.x * wpt : words;
  t1 = (t0 + wpt) < words ? (t0 + wpt) : words;
  i64 c = 0;
  for (int w = t0; w < t1; ++w) c += __popc(bm[w]);
  return c;
}

// The pairs (s, column) of this thread's words, ascending, from edges[at] on — at = the query's running base + the thread's
// scan prefix — and beside every pair its accumulator (VAL).  Nothing is written at or past `end`: offsets of another input
// write nothing past their own segment.
template <bool VAL>
__device__ __forceinline__ void ws_emit(const unsigned* bm, const float* acc, int t0, int t1, i64 s, i64 w0, i64 at, i64 end,
                                        longlong2* __restrict__ edges, float* __restrict__ val) {
  for (int w = t0; w < t1; ++w) {
    unsigned bits = bm[w];
    while (bits) {
      const int b = __ffs((int)bits) - 1;
      bits &= bits - 1;
      if (at < end) {
        edges[at] = make_longlong2(s, w0 + ((i64)w << 5) + b);
        if (VAL) val[at] = acc[(w << 5) + b];
      }
      ++at;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host: a launch's window, a kernel's LDS limit
// ---------------------------------------------------------------------------------------------
// OCN_EINVAL unless n_cols is in [1, 2^31) and window_cols is 0 (= limit, the entry's default window) or a positive multiple
// of 64 up to limit; else 0, the window and the span LDS is sized for (span / 8 bytes of bitmap, span * 4 of accumulators).
static inline int ws_resolve_window(int64_t n_cols, int64_t window_cols, i64 limit, i64* window, i64* span) {
  if (n_cols <= 0 || n_cols >= ((int64_t)1 << 31)) return OCN_EINVAL;
  if (window_cols < 0 || window_cols % 64 != 0 || window_cols > limit) return OCN_EINVAL;
  *window = window_cols ? (i64)window_cols : limit;
  *span = ws_span(*window, (i64)n_cols);
  return 0;
}

// The dynamic LDS limit of a kernel is raised ONCE per device, to `bytes` = what the entry's default window takes — never per
// launch to that launch's size: two host threads that launch graphs of different widths would race between the set and the
// launch.  (Setting the same value twice, by two first callers, is harmless.)  `raised`: the caller's own bit per device, one
// per kernel instance; a device numbered 64 or above has no bit and sets the limit every time.  Returns 0 or the HIP error.
static inline int ws_raise_lds_once(const void* kernel, size_t bytes, std::atomic<unsigned long long>& raised) {
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return (int)err;
  if (dev >= 64 || !((raised.load(std::memory_order_acquire) >> dev) & 1ull)) {
    err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return (int)err;
    if (dev < 64) raised.fetch_or(1ull << dev, std::memory_order_release);
  }
  return 0;
}
