// Structured negative sampling: pairs that are guaranteed not to be links, drawn exactly uniformly and without a rejection
// loop.  For a row s of a square `known` matrix the excluded set is X(s) = known[s,:] U {s} and a sample is the r-th
// smallest column outside it, r = floor(u * m_s / 2^64) for one 64-bit Philox4x32-10 word u and m_s = n - |X(s)|.  The r-th
// member of the complement of a sorted row x_0 < x_1 < ... is r + i with i the first index where x_i - i > r (x_i - i = the
// number of free columns below x_i, a non-decreasing sequence): one binary search on the CSR row, whatever its length.
// Every sample is a function of (seed, its own index, known) alone: no atomics, no workspace, no launch geometry in the result.
// See include/ocn_hip.h (ocn_philox4x32, ocn_complement_count, ocn_sample_complement_rows, ocn_sample_complement_pairs).
// Hard negatives are drawn the same way from the candidate set that is served: the r-th smallest member of a source's 2-hop row
// difference, selected in the LDS bitmap the 2-hop expansion builds, without ever listing the set (ocn_sample_two_hop).
#include "common.h"
#include "philox.h"       // the generator, sample_rank and the counter streams
#include "window_sweep.h"

// ---------------------------------------------------------------------------------------------
// selection in the complement of a sorted row
// ---------------------------------------------------------------------------------------------
// number of leading positions k of the sorted row a[0..n) with a[k] - k <= r  (= the first index i with a[i] - i > r, n if
// there is none).  The steps depend on n alone and every load is in bounds for any r.
// (not common.h's sorted_has: it searches the derived sequence a[k] - k and returns a count, in fixed trips)
template <typename Row>
__device__ __forceinline__ i64 free_below(Row a, i64 n, i64 r) {
  i64 at = 0;
  for (i64 len = n; len > 1;) {
    const i64 half = len >> 1;
    const i64 k = at + half - 1;
    at += ((i64)a[k] - k <= r) ? half : 0;
    len -= half;
  }
  return at + ((n > 0 && (i64)a[at] - at <= r) ? 1 : 0);
}

// position of `key` in the sorted row (the number of columns below it) and whether the row stores it
// (not common.h's sorted_has: it returns the position beside the membership, in fixed trips with in-bounds loads)
template <typename Row>
__device__ __forceinline__ i64 row_lower_bound(Row a, i64 n, i64 key, bool& found) {
  i64 at = 0;
  for (i64 len = n; len > 1;) {
    const i64 half = len >> 1;
    at += ((i64)a[at + half - 1] < key) ? half : 0;
    len -= half;
  }
  at += (n > 0 && (i64)a[at] < key) ? 1 : 0;
  found = at < n && (i64)a[at] == key;
  return at;
}

// A row with the source spliced in virtually: `below` columns lie under s and s is counted once, stored or not.
struct SelfSplice {
  i64 m;          // members of the complement of row U {s}
  i64 self_rank;  // rank of s among the columns the row leaves free; -1 where the row stores s (nothing to skip)
};

template <typename Row>
__device__ __forceinline__ SelfSplice splice_self(Row a, i64 d, i64 s, i64 n_cols) {
  bool stored;
  const i64 below = row_lower_bound(a, d, s, stored);
  SelfSplice sp;
  sp.m = n_cols - d - (stored ? 0 : 1);
  sp.self_rank = stored ? -1 : s - below;
  return sp;
}

// the r-th smallest column (0-based) outside row U {s}: the row's own complement with the rank of s stepped over
template <typename Row>
__device__ __forceinline__ i64 complement_select(Row a, i64 d, const SelfSplice& sp, i64 r) {
  const i64 rr = r + ((sp.self_rank >= 0 && r >= sp.self_rank) ? 1 : 0);
  return rr + free_below(a, d, rr);
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OCN_BLOCK) void philox4x32_kernel(const uint4* __restrict__ ctr, unsigned k0, unsigned k1, i64 n,
                                                               uint4* __restrict__ out) {
  for (i64 t = (i64)blockIdx.x * OCN_BLOCK + threadIdx.x; t < n; t += (i64)gridDim.x * OCN_BLOCK)
    out[t] = philox4x32_10(ctr[t], k0, k1);
}

__global__ __launch_bounds__(OCN_BLOCK) void complement_count_kernel(const i64* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                     i64 n_cols, int32_t* __restrict__ count) {
  for (i64 s = (i64)blockIdx.x * OCN_BLOCK + threadIdx.x; s < n_cols; s += (i64)gridDim.x * OCN_BLOCK) {
    const i64 k0 = rowptr[s], d = rowptr[s + 1] - k0;
    const i64 m = splice_self(col + k0, d, s, n_cols).m;
    count[s] = (int32_t)(m > 0 ? m : 0);
  }
}

// Columns of a row a wave stages in LDS: 2 KiB per wave, 8 KiB per workgroup, as the row difference of recommend.hip keeps
// (eight workgroups per CU take 64 of the CU's 160 KiB).  A longer row is a hub: it is searched where it lies, and the top of
// its search tree stays in L1 / L2 for the wave's 64 lanes.
constexpr int NS_STAGE = 512;

// A wave owns one (query, 64-sample chunk): it stages the query's row once, every lane draws one word and searches the row
// for its own rank, and the wave stores 64 consecutive int64 (512 contiguous bytes).  No workgroup barrier anywhere: the item
// loop runs on the wave's index and kernel arguments alone.
__global__ __launch_bounds__(OCN_BLOCK) void sample_rows_kernel(
    const i64* __restrict__ rowptr, const int32_t* __restrict__ col, i64 n_cols, const i64* __restrict__ rows, i64 Q, i64 per,
    i64 q0, u64 seed, i64* __restrict__ out) {
  __shared__ int32_t s_row[OCN_WPB][NS_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t* sr = s_row[wave];
  const i64 chunks = (per + OCN_WAVE - 1) / OCN_WAVE;
  const i64 items = Q * chunks;
  for (i64 it = (i64)blockIdx.x * OCN_WPB + wave; it < items; it += (i64)gridDim.x * OCN_WPB) {
    const i64 q = it / chunks, j = (it - q * chunks) * OCN_WAVE + lane;
    const i64 s = rows[q];
    const i64 k0 = rowptr[s], d = rowptr[s + 1] - k0;
    const bool staged = d <= NS_STAGE;
    if (staged) {
      for (i64 t = lane; t < d; t += OCN_WAVE) sr[t] = col[k0 + t];
      wave_lds_sync();
    }
    const SelfSplice sp = staged ? splice_self(sr, d, s, n_cols) : splice_self(col + k0, d, s, n_cols);
    const u64 qq = (u64)(q0 + q);
    i64 v = -1;
    if (sp.m > 0) {
      const i64 r = (i64)sample_rank(make_uint4((unsigned)j, (unsigned)qq, (unsigned)(qq >> 32), SAMPLE_STREAM_ROWS), seed, (u64)sp.m);
      v = staged ? complement_select(sr, d, sp, r) : complement_select(col + k0, d, sp, r);
    }
    if (j < per) out[q * per + j] = v;
    if (staged) wave_lds_sync();                          // the next item's staging writes stay behind this one's reads
  }
}

// One thread per sample: a rank in [0, M) over all ordered non-edge, non-self pairs, the row that holds it (the last row
// whose prefix does not exceed it: a row with an empty complement is never that), the column by the in-row selection.
__global__ __launch_bounds__(OCN_BLOCK) void sample_pairs_kernel(
    const i64* __restrict__ rowptr, const int32_t* __restrict__ col, i64 n_cols, const i64* __restrict__ cptr, i64 T, i64 t0,
    u64 seed, i64* __restrict__ out) {
  const i64 M = cptr[n_cols];
  for (i64 t = (i64)blockIdx.x * OCN_BLOCK + threadIdx.x; t < T; t += (i64)gridDim.x * OCN_BLOCK) {
    i64 s = -1, c = -1;
    if (M > 0) {                                             // (no pair to draw, or a scan that gave up: -1, nothing searched)
      const u64 tt = (u64)(t0 + t);
      const i64 r = (i64)sample_rank(make_uint4((unsigned)tt, (unsigned)(tt >> 32), 0u, SAMPLE_STREAM_PAIRS), seed, (u64)M);
      i64 at = 0;
      for (i64 len = n_cols; len > 1;) {                     // the largest row with cptr[row] <= r; steps depend on n_cols alone
        const i64 half = len >> 1;
        at += (cptr[at + half] <= r) ? half : 0;
        len -= half;
      }
      s = at;
      const i64 k0 = rowptr[s], d = rowptr[s + 1] - k0;
      c = complement_select(col + k0, d, splice_self(col + k0, d, s, n_cols), r - cptr[s]);
    }
    out[t] = s;
    out[T + t] = c;
  }
}

// ---------------------------------------------------------------------------------------------
// selection in a 2-hop row difference: H_q = ( U_{m in A[s,:]} A[m,:] ) \ M[s,:]
// ---------------------------------------------------------------------------------------------
// The default window: the bitmap kernel's (recommend.hip: TH_WINDOW) less the 2 KiB the thread prefixes are rounded up to.
// 1 277 952 columns, a multiple of 64.
constexpr i64 S2_WINDOW = (i64)(160 * 1024 - 4096) * 8;

// the n-th set bit (0-based) of a word that has more than n
__device__ __forceinline__ int nth_set_bit(unsigned bits, int n) {
  for (int k = 0; k < n; ++k) bits &= bits - 1;
  return __ffs((int)bits) - 1;
}

// the rank slot i draws among m candidates: one 64-bit word of its own counter
__device__ __forceinline__ i64 two_hop_rank(const i64* __restrict__ sid, i64 i, i64 slot0, u64 qq, u64 seed, i64 m) {
  uint4 ctr;
  if (sid) {
    const u64 id = (u64)sid[i];
    ctr = make_uint4((unsigned)id, (unsigned)(id >> 32), 0u, SAMPLE_STREAM_TWO_HOP_ID);
  } else {
    ctr = make_uint4((unsigned)(i - slot0), (unsigned)qq, (unsigned)(qq >> 32), SAMPLE_STREAM_TWO_HOP);
  }
  return (i64)sample_rank(ctr, seed, (u64)m);
}

// A workgroup owns query q and sweeps the column range in windows, as two_hop_diff_kernel does: th_window_bitmap leaves the
// window's part of H_q as a bitmap in LDS, every thread counts the bits of its contiguous words and the block scan of these
// counts — the thread prefixes, kept in LDS — orders the window's members.  Then a thread per slot, OCN_BLOCK slots at a time:
// it draws its rank r again from its counter, and where base <= r < base + the window's total it finds the thread whose
// words hold member r - base (a search of the prefixes in fixed trips), walks that thread's words by popcount and takes the
// n-th set bit of the word.  A slot is written by exactly one window, or with -1 where H_q is empty.
// The rank needs c_q = |H_q| before the first selection: when the whole column range is one window (`window >= n_cols`, a
// kernel argument) its total is c_q and one expansion serves both; else a first sweep counts and a second one selects.
// Every barrier is reached by the whole workgroup: the query and the window loops run on blockIdx and kernel arguments, the
// slot loop (which holds no barrier) on sptr[q], sptr[q + 1], which every thread reads alike — never on a row length.
__global__ __launch_bounds__(OCN_BLOCK) void sample_two_hop_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrM, const int32_t* __restrict__ colM, i64 n_cols,
    const i64* __restrict__ rows, i64 Q, int drop_self, i64 window,
    const i64* __restrict__ sptr, const i64* __restrict__ sid, i64 q0, u64 seed,
    int32_t* __restrict__ count, i64* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned th_bm[];
  __shared__ i64 sh[2 * OCN_WPB];
  __shared__ int s_pre[OCN_BLOCK];                           // members of the window in the words of the threads below (< 2^21)
  const bool one_window = window >= n_cols;
  for (i64 q = blockIdx.x; q < Q; q += gridDim.x) {
    const i64 slot0 = sptr[q], slot1 = sptr[q + 1];
    if (slot1 <= slot0 && !count) continue;                  // (the same in every thread: nothing to write for this query)
    const i64 s = rows[q];
    const i64 a0 = rowptrA[s], da = rowptrA[s + 1] - a0;
    const i64 m0 = rowptrM[s], dm = rowptrM[s + 1] - m0;
    const u64 qq = (u64)(q0 + q);
    i64 cq = 0;
    if (!one_window) {                                       // the counting sweep: two_hop_diff_kernel<false>
      for (i64 w0 = 0; w0 < n_cols; w0 += window) {
        const i64 w1 = ws_window_end(w0, window, n_cols);
        const int words = ws_words(w0, w1);
        th_window_bitmap(th_bm, rowptrA, colA, a0, da, colM, m0, dm, s, drop_self, w0, w1, words);
        int t0, t1;
        i64 tot;
        block_excl_scan(th_thread_bits(th_bm, words, t0, t1), sh, &tot);
        cq += tot;                                           // (the scan's last barrier keeps the next clear behind these reads)
      }
    }
    if (one_window || (cq > 0 && slot1 > slot0)) {           // the selecting sweep (the same in every thread)
      i64 base = 0;
      for (i64 w0 = 0; w0 < n_cols; w0 += window) {
        const i64 w1 = ws_window_end(w0, window, n_cols);
        const int words = ws_words(w0, w1);
        th_window_bitmap(th_bm, rowptrA, colA, a0, da, colM, m0, dm, s, drop_self, w0, w1, words);
        int t0, t1;
        i64 tot;
        s_pre[threadIdx.x] = (int)block_excl_scan(th_thread_bits(th_bm, words, t0, t1), sh, &tot);
        if (one_window) cq = tot;
        __syncthreads();                                     // the prefixes of all threads, before any slot searches them
        if (tot > 0) {
          const int wpt = (words + OCN_BLOCK - 1) / OCN_BLOCK;
          for (i64 i = slot0 + threadIdx.x; i < slot1; i += OCN_BLOCK) {
            const i64 r = two_hop_rank(sid, i, slot0, qq, seed, cq) - base;
            if (r < 0 || r >= tot) continue;                 // another window's member
            int at = 0;                                      // the last thread whose prefix does not exceed r: its words hold it
            for (int step = OCN_BLOCK >> 1; step > 0; step >>= 1) at += (s_pre[at + step] <= (int)r) ? step : 0;
            int left = (int)r - s_pre[at];
            const int e = (at + 1) * wpt < words ? (at + 1) * wpt : words;
            i64 v = -1;
            for (int w = at * wpt; w < e; ++w) {
              const unsigned bits = th_bm[w];
              const int pc = __popc(bits);
              if (left < pc) { v = w0 + ((i64)w << 5) + nth_set_bit(bits, left); break; }
              left -= pc;
            }
            out[i] = v;
          }
        }
        base += tot;
        __syncthreads();                                     // the next window's clear and prefixes stay behind these reads
      }
    }
    if (cq == 0)
      for (i64 i = slot0 + threadIdx.x; i < slot1; i += OCN_BLOCK) out[i] = -1;
    if (count && threadIdx.x == 0) count[q] = (int32_t)cq;
  }
}

static inline bool ns_cols_ok(int64_t n_cols) { return n_cols >= 1 && n_cols < ((int64_t)1 << 31); }
static inline unsigned ns_thread_grid(i64 items) { return (unsigned)grid_for((items + OCN_BLOCK - 1) / OCN_BLOCK, 256 * 8); }

extern "C" {

int ocn_philox4x32(const uint32_t* ctr, uint32_t key0, uint32_t key1, int64_t n, uint32_t* out, void* stream) {
  if (n < 0 || !ctr || !out) return OCN_EINVAL;
  if ((((uintptr_t)ctr) | ((uintptr_t)out)) & 15u) return OCN_EINVAL;
  if (n == 0) return 0;
  hipLaunchKernelGGL(philox4x32_kernel, dim3(ns_thread_grid(n)), dim3(OCN_BLOCK), 0, (hipStream_t)stream, (const uint4*)ctr,
                     (unsigned)key0, (unsigned)key1, (i64)n, (uint4*)out);
  return launch_status();
}

int ocn_complement_count(const int64_t* rowptrK, const int32_t* colK, int64_t n_cols, int32_t* count, void* stream) {
  if (!rowptrK || !colK || !count || !ns_cols_ok(n_cols)) return OCN_EINVAL;
  hipLaunchKernelGGL(complement_count_kernel, dim3(ns_thread_grid(n_cols)), dim3(OCN_BLOCK), 0, (hipStream_t)stream,
                     (const i64*)rowptrK, colK, (i64)n_cols, count);
  return launch_status();
}

int32_t ocn_sample_stage_cols(void) { return NS_STAGE; }

int ocn_sample_complement_rows(const int64_t* rowptrK, const int32_t* colK, int64_t n_cols, const int64_t* rows, int64_t Q,
                               int64_t per, int64_t q0, uint64_t seed, int64_t* out, void* stream) {
  if (!rowptrK || !colK || !rows || !out || !ns_cols_ok(n_cols)) return OCN_EINVAL;
  if (Q < 0 || q0 < 0 || per < 1 || per >= ((int64_t)1 << 31)) return OCN_EINVAL;
  if (q0 > INT64_MAX - Q) return OCN_EINVAL;                 // (the query counter q0 + q stays a non-negative int64)
  if (Q == 0) return 0;
  const i64 chunks = (per + OCN_WAVE - 1) / OCN_WAVE;
  if (Q > INT64_MAX / chunks) return OCN_EINVAL;
  const i64 items = Q * chunks;
  hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)grid_for((items + OCN_WPB - 1) / OCN_WPB, 256 * 8)), dim3(OCN_BLOCK), 0,
                     (hipStream_t)stream, (const i64*)rowptrK, colK, (i64)n_cols, (const i64*)rows, (i64)Q, (i64)per, (i64)q0,
                     (u64)seed, (i64*)out);
  return launch_status();
}

int ocn_sample_complement_pairs(const int64_t* rowptrK, const int32_t* colK, int64_t n_cols, const int64_t* cptr, int64_t T,
                                int64_t t0, uint64_t seed, int64_t* out, void* stream) {
  if (!rowptrK || !colK || !cptr || !out || !ns_cols_ok(n_cols)) return OCN_EINVAL;
  if (T < 0 || t0 < 0 || t0 > INT64_MAX - T) return OCN_EINVAL;
  if (T == 0) return 0;
  hipLaunchKernelGGL(sample_pairs_kernel, dim3(ns_thread_grid(T)), dim3(OCN_BLOCK), 0, (hipStream_t)stream, (const i64*)rowptrK,
                     colK, (i64)n_cols, (const i64*)cptr, (i64)T, (i64)t0, (u64)seed, (i64*)out);
  return launch_status();
}

int64_t ocn_sample_two_hop_window_cols(void) { return S2_WINDOW; }

int ocn_sample_two_hop(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM, int64_t n_cols,
                       const int64_t* rows, int64_t Q, int32_t drop_self, int64_t window_cols, const int64_t* sptr,
                       const int64_t* sid, int64_t q0, uint64_t seed, int32_t* count, int64_t* out, void* stream) {
  if (!rowptrA || !colA || !rowptrM || !colM || !rows || !sptr || !out || !ns_cols_ok(n_cols)) return OCN_EINVAL;
  if (Q < 0 || q0 < 0 || q0 > INT64_MAX - Q) return OCN_EINVAL;             // (the query counter q0 + q stays a non-negative int64)
  i64 window, span;
  if (ws_resolve_window(n_cols, window_cols, S2_WINDOW, &window, &span)) return OCN_EINVAL;
  if (Q == 0) return 0;
  static std::atomic<unsigned long long> lds_raised{0ull};
  if (const int rc = ws_raise_lds_once((const void*)sample_two_hop_kernel, (size_t)(S2_WINDOW / 8), lds_raised)) return rc;
  hipLaunchKernelGGL(sample_two_hop_kernel, dim3((unsigned)grid_for(Q, 256 * 16)), dim3(OCN_BLOCK), (size_t)(span / 8),
                     (hipStream_t)stream, (const i64*)rowptrA, colA, (const i64*)rowptrM, colM, (i64)n_cols, (const i64*)rows, (i64)Q,
                     (int)drop_self, window, (const i64*)sptr, (const i64*)sid, (i64)q0, (u64)seed, count, (i64*)out);
  return launch_status();
}

}  // extern "C"
