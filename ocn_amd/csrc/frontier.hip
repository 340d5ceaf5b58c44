// Frontier expansion with ordered path sums: the generalisation of the scored 2-hop expansion (recommend.hip,
// two_hop_sums_kernel) from "the row of s, weighted by w[m]" to an explicit per-query frontier list with explicit weights, and
// an optional seed list of starting values.  Chained, it walks a source's neighbourhood one hop per launch: the candidates
// within three hops with the local path index A² + decay·A³ (or its AA / RA weighted forms) are two launches of it.
// See include/ocn_hip.h (ocn_frontier_count / ocn_frontier_sums_fill).
#include <atomic>

#include "common.h"

// A window column keeps a presence bit and an fp32 accumulator (33 bits) in the CU's 160 KiB without the 2 KiB left to the scan's
// words and the runtime and the 4 KiB of the waves' claim tables below: 38 208 columns.
constexpr int FR_TAGS = 256;                                 // claim slots per wave
constexpr i64 FR_WINDOW = (i64)(160 * 1024 - 2048 - OCN_WPB * FR_TAGS * 4) * 8 / 33 / 64 * 64;
constexpr unsigned FR_FREE = 0xffffffffu;                    // a claim slot nobody bids for

// first position of the sorted row a[0..n) whose column is not below key (two_hop_window.h keeps its own copy: th_lower_bound)
__device__ __forceinline__ i64 fr_lower_bound(const int32_t* __restrict__ a, i64 n, i64 key) {
  i64 lo = 0, hi = n;
  while (lo < hi) {
    const i64 mid = lo + ((hi - lo) >> 1);
    if ((i64)a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the same over the nodes of a pair list (the second word of every pair)
__device__ __forceinline__ i64 fr_pair_lower_bound(const longlong2* __restrict__ a, i64 n, i64 key) {
  i64 lo = 0, hi = n;
  while (lo < hi) {
    const i64 mid = lo + ((hi - lo) >> 1);
    if (a[mid].y < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ i64 fr_readlane(i64 v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l), hi = __builtin_amdgcn_readlane((unsigned)((u64)v >> 32), l);
  return (i64)(((u64)hi << 32) | lo);
}

// one member of column k (relative to the window): the presence bit and, where sums are kept, the accumulator's next partial sum.
// The first member of an unseeded column adds to 0.0f, so no accumulator is ever cleared: the slot is read before the bit says
// whether it counts, and a stale value is only ever selected away (as ts_add of recommend.hip).
template <bool VAL>
__device__ __forceinline__ void fr_add(unsigned* bm, float* acc, unsigned k, float f) {
  const unsigned bit = 1u << (k & 31u);
  if (VAL) {
    const float prev = acc[k];
    const unsigned old = atomicOr(&bm[k >> 5], bit);
    acc[k] = __fadd_rn((old & bit) ? prev : 0.0f, f);
  } else {
    atomicOr(&bm[k >> 5], bit);
  }
}

// One body for the three passes, so they cannot disagree: FILL == false leaves the size of every query's set in count[q];
// FILL == true writes the pairs (s, t) from edges[off[q]] on, ascending in t; VAL == true keeps an accumulator per column and
// writes val beside the pairs.  A workgroup owns query q and sweeps the column range in windows [w0, w1):
//   1. the bitmap is cleared;
//   2. the window's columns are dealt to the four waves in contiguous quarters.  A wave first enters the seed entries of its
//      quarter (bit set, accumulator = the seed value), then walks the WHOLE frontier in ascending order, 64 entries at a time, a
//      lane each: where the entry's row enters the quarter (a search per lane), its first column there, and whether that is its
//      only one.  Most (entry, quarter) pairs miss, most hits are that one column.  The hits are then taken in lane order:
//        - a run of consecutive one-column hits is added by its own lanes side by side.  Two of them may name the same column,
//          and their adds must not swap: every pending lane bids for the column's slot of the wave's claim table with its lane
//          id (LDS atomicMin), the lowest bidder of a slot adds and frees it, the others bid again.  Lanes with one column share
//          one slot, so they add in ascending lane order, which is ascending c; distinct columns that share a slot only wait;
//        - an entry with several columns in the quarter is walked by the whole wave, its lanes on consecutive entries.
//      An accumulator is only ever touched by one wave, the lanes of one instruction touch distinct columns, and LDS executes a
//      wave's instructions in order: a plain read-add-write per member is the ascending-c sum.  Without accumulators (VAL ==
//      false) no order is owed and every lane sets the bits of its own entry's columns;
//   3. the bits of M[s,:] inside the window, and of s itself under drop_self, are cleared;
//   4. every thread counts the bits of its contiguous words, a block scan places its columns behind the query's running base.
// Every barrier is reached by the whole workgroup: the query loop and the window loop run on blockIdx and kernel arguments
// alone.  A column outside [w0, w1) never touches LDS, whatever the lists and rows hold.
template <bool FILL, bool VAL>
__global__ __launch_bounds__(OCN_BLOCK) void frontier_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrM, const int32_t* __restrict__ colM, i64 n_cols,
    const i64* __restrict__ rows, i64 Q, int drop_self, i64 window,
    const i64* __restrict__ ptrF, const longlong2* __restrict__ nodeF, const float* __restrict__ valF,
    const i64* __restrict__ ptrS, const longlong2* __restrict__ nodeS, const float* __restrict__ valS,
    int32_t* __restrict__ count, const i64* __restrict__ off, longlong2* __restrict__ edges, float* __restrict__ val) {
  extern __shared__ __attribute__((aligned(16))) unsigned fr_bm[];
  __shared__ i64 sh[2 * OCN_WPB];
  __shared__ unsigned s_tag[VAL ? OCN_WPB : 1][VAL ? FR_TAGS : 1];
  const i64 span = window < (n_cols + 63) / 64 * 64 ? window : (n_cols + 63) / 64 * 64;   // the columns the launch sized LDS for
  float* acc = reinterpret_cast<float*>(fr_bm + (span >> 5));                             // (VAL only: no LDS behind the bitmap otherwise)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* tag = s_tag[VAL ? wave : 0];
  if (VAL) {
    for (int t = lane; t < FR_TAGS; t += OCN_WAVE) tag[t] = FR_FREE;
    wave_lds_sync();
  }
  for (i64 q = blockIdx.x; q < Q; q += gridDim.x) {
    const i64 s = rows[q];
    const i64 f0 = ptrF[q], df = ptrF[q + 1] - f0;
    const i64 s0 = ptrS ? ptrS[q] : 0, ds = ptrS ? ptrS[q + 1] - s0 : 0;
    const i64 m0 = rowptrM[s], dm = rowptrM[s + 1] - m0;
    i64 base = FILL ? off[q] : 0;
    const i64 end = FILL ? off[q + 1] : 0;
    for (i64 w0 = 0; w0 < n_cols; w0 += window) {
      const i64 w1 = (w0 + window) < n_cols ? (w0 + window) : n_cols;
      const int words = (int)((w1 - w0 + 31) >> 5);
      for (int t = threadIdx.x; t < words; t += OCN_BLOCK) fr_bm[t] = 0u;
      __syncthreads();
      const i64 quarter = (w1 - w0 + OCN_WPB - 1) / OCN_WPB;
      const i64 q0 = w0 + wave * quarter;
      const i64 q1 = (q0 + quarter) < w1 ? (q0 + quarter) : w1;            // (an empty quarter: q1 <= q0, nothing passes below)
      if (ds > 0 && q0 < q1) {                               // the seeds of the quarter: distinct columns, before any frontier add
        const i64 lo = q0 > 0 ? fr_pair_lower_bound(nodeS + s0, ds, q0) : 0;
        for (i64 p = lo + lane; p < ds; p += OCN_WAVE) {
          const i64 c = nodeS[s0 + p].y;
          if (c >= q1) break;                                // (sorted: so is every later node of this lane)
          if (c >= q0) {
            const unsigned k = (unsigned)(c - w0);
            atomicOr(&fr_bm[k >> 5], 1u << (k & 31u));
            if (VAL) acc[k] = valS[s0 + p];
          }
        }
        if (VAL) wave_lds_sync();
      }
      for (i64 t0 = 0; t0 < df; t0 += OCN_WAVE) {
        const i64 tt = t0 + lane;
        i64 lb = 0, le = 0;
        i64 c0 = n_cols;                                     // the entry's first column inside the quarter (n_cols: it has none)
        bool one = false;                                    // ... and it is the only one
        float lf = 0.0f;
        if (tt < df) {
          const i64 c = nodeF[f0 + tt].y;
          const i64 b0 = rowptrA[c];
          le = rowptrA[c + 1];
          lb = b0 + (q0 > 0 ? fr_lower_bound(colA + b0, le - b0, q0) : 0);
          if (lb < le) {
            c0 = colA[lb];
            one = lb + 1 >= le || (i64)colA[lb + 1] >= q1;
          }
          if (VAL) lf = valF ? valF[f0 + tt] : 1.0f;
        }
        const bool hit = c0 < q1;
        if (!VAL) {                                          // bits only: no order is owed, a lane takes its own entry
          if (hit)
            for (i64 p = lb; p < le; ++p) {
              const i64 c = colA[p];
              if (c >= q1) break;
              fr_add<false>(fr_bm, acc, (unsigned)(c - w0), 0.0f);
            }
          continue;
        }
        u64 live = __ballot(hit);
        const u64 ones = __ballot(hit && one);
        while (live) {                                       // ascending lanes: ascending c (the same trips in every lane)
          const int j = __ffsll((long long)live) - 1;
          if (!((ones >> j) & 1ull)) {                       // several columns in the quarter: the wave walks the entry's row
            live &= live - 1;
            const i64 pe = fr_readlane(le, j);
            const float f = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(lf), j));
            for (i64 p = fr_readlane(lb, j) + lane; p < pe; p += OCN_WAVE) {
              const i64 c = colA[p];
              if (c >= q1) break;                            // (sorted: so is every later column of this lane)
              fr_add<true>(fr_bm, acc, (unsigned)(c - w0), f);
            }
            wave_lds_sync();                                 // the next entry's reads stay behind this one's writes
            continue;
          }
          // the run of one-column hits from lane j up to the next entry with several columns
          const u64 multi_above = live & ~ones;              // (lanes below j have left `live`)
          const int lim = multi_above ? __ffsll((long long)multi_above) - 1 : 64;
          const u64 run = live & (lim < 64 ? ((1ull << lim) - 1ull) : ~0ull);
          live &= ~run;
          bool pend = (run >> lane) & 1ull;
          const unsigned k = pend ? (unsigned)(c0 - w0) : 0u;
          if ((run & (run - 1)) == 0ull) {                   // a run of one
            if (pend) fr_add<true>(fr_bm, acc, k, lf);
            wave_lds_sync();
            continue;
          }
          const unsigned slot = k & (FR_TAGS - 1);
          while (__ballot(pend)) {
            if (pend) atomicMin(&tag[slot], (unsigned)lane);
            wave_lds_sync();
            const bool win = pend && tag[slot] == (unsigned)lane;
            if (win) fr_add<true>(fr_bm, acc, k, lf);        // (winners hold distinct slots, so distinct columns)
            wave_lds_sync();
            if (win) { tag[slot] = FR_FREE; pend = false; }
            wave_lds_sync();
          }
        }
      }
      __syncthreads();
      const i64 lo_m = w0 > 0 ? fr_lower_bound(colM + m0, dm, w0) : 0;
      for (i64 p = lo_m + threadIdx.x; p < dm; p += OCN_BLOCK) {
        const i64 c = colM[m0 + p];
        if (c >= w1) break;
        if (c >= w0) {
          const unsigned k = (unsigned)(c - w0);
          atomicAnd(&fr_bm[k >> 5], ~(1u << (k & 31u)));
        }
      }
      if (drop_self && threadIdx.x == 0 && s >= w0 && s < w1) {
        const unsigned k = (unsigned)(s - w0);
        atomicAnd(&fr_bm[k >> 5], ~(1u << (k & 31u)));
      }
      __syncthreads();
      const int wpt = (words + OCN_BLOCK - 1) / OCN_BLOCK;   // contiguous words per thread: ascending columns in thread order
      const int t0 = (int)threadIdx.x * wpt < words ? (int)threadIdx.x * wpt : words;
      const int t1 = (t0 + wpt) < words ? (t0 + wpt) : words;
      i64 c = 0;
      for (int t = t0; t < t1; ++t) c += __popc(fr_bm[t]);
      i64 tot;
      const i64 ex = block_excl_scan(c, sh, &tot);
      if (FILL) {
        i64 at = base + ex;
        for (int t = t0; t < t1; ++t) {
          unsigned bits = fr_bm[t];
          while (bits) {
            const int b = __ffs((int)bits) - 1;
            bits &= bits - 1;
            if (at < end) {                                  // (at < end: offsets of another input write nothing past their own segment)
              edges[at] = make_longlong2(s, w0 + ((i64)t << 5) + b);
              if (VAL) val[at] = acc[(t << 5) + b];
            }
            ++at;
          }
        }
      }
      base += tot;
      __syncthreads();                                       // the next window's clear stays behind this one's reads
    }
    if (!FILL && threadIdx.x == 0) count[q] = (int32_t)base;
  }
}

extern "C" {

int64_t ocn_frontier_window_cols(void) { return FR_WINDOW; }

// mode 0: count, 1: fill without values, 2: fill with values
static int frontier_launch(int mode, const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM,
                           int64_t n_cols, const int64_t* rows, int64_t Q, int32_t drop_self, int64_t window_cols,
                           const int64_t* ptrF, const int64_t* nodeF, const float* valF, const int64_t* ptrS, const int64_t* nodeS,
                           const float* valS, int32_t* count, const int64_t* off, int64_t* edges, float* val, void* stream) {
  if (Q < 0 || !rowptrA || !colA || !rowptrM || !colM || !rows || !ptrF || !nodeF) return OCN_EINVAL;
  if ((ptrS != nullptr) != (nodeS != nullptr)) return OCN_EINVAL;
  if (mode == 0 ? !count : (!off || !edges)) return OCN_EINVAL;
  if (mode == 2 && ptrS && !valS) return OCN_EINVAL;
  if (n_cols <= 0 || n_cols >= ((int64_t)1 << 31)) return OCN_EINVAL;
  if (window_cols < 0 || window_cols % 64 != 0 || window_cols > FR_WINDOW) return OCN_EINVAL;
  if (Q == 0) return 0;
  const i64 window = window_cols ? (i64)window_cols : FR_WINDOW;
  const i64 padded = (n_cols + 63) / 64 * 64;
  const i64 span = window < padded ? window : padded;                         // a small graph keeps several workgroups per CU
  const size_t lds = (size_t)(span / 8 + (mode == 2 ? span * 4 : 0));         // the bitmap, then the accumulators
  // at most 16 workgroups per CU's worth of queries in flight; a longer list is taken grid-stride
  const dim3 grid((unsigned)grid_for(Q, 256 * 16));
#define FR_ARGS                                                                                                                \
  (const i64*)rowptrA, colA, (const i64*)rowptrM, colM, (i64)n_cols, (const i64*)rows, (i64)Q, (int)drop_self, window,        \
      (const i64*)ptrF, (const longlong2*)nodeF, valF, (const i64*)ptrS, (const longlong2*)nodeS, valS, count, (const i64*)off, \
      (longlong2*)edges, val
  if (mode == 2) {
    // The LDS limit of the valued kernel is raised ONCE per device, to what the default window takes, never per launch to that
    // launch's size: two host threads that launch graphs of different widths would race between the set and the launch.  (The
    // bitmap alone, 4 776 bytes at the most, stays below the limit every kernel has.)
    static std::atomic<unsigned long long> lds_raised{0ull};
    int dev = 0;
    hipError_t err = hipGetDevice(&dev);
    if (err != hipSuccess) return (int)err;
    if (dev >= 64 || !((lds_raised.load(std::memory_order_acquire) >> dev) & 1ull)) {
      err = hipFuncSetAttribute((const void*)frontier_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(FR_WINDOW / 8 + FR_WINDOW * 4));
      if (err != hipSuccess) return (int)err;
      if (dev < 64) lds_raised.fetch_or(1ull << dev, std::memory_order_release);
    }
    hipLaunchKernelGGL((frontier_kernel<true, true>), grid, dim3(OCN_BLOCK), lds, (hipStream_t)stream, FR_ARGS);
  } else if (mode == 1) {
    hipLaunchKernelGGL((frontier_kernel<true, false>), grid, dim3(OCN_BLOCK), lds, (hipStream_t)stream, FR_ARGS);
  } else {
    hipLaunchKernelGGL((frontier_kernel<false, false>), grid, dim3(OCN_BLOCK), lds, (hipStream_t)stream, FR_ARGS);
  }
#undef FR_ARGS
  return launch_status();
}

int ocn_frontier_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM, int64_t n_cols,
                       const int64_t* rows, int64_t Q, int32_t drop_self, int64_t window_cols, const int64_t* ptrF,
                       const int64_t* nodeF, const int64_t* ptrS, const int64_t* nodeS, int32_t* count, void* stream) {
  return frontier_launch(0, rowptrA, colA, rowptrM, colM, n_cols, rows, Q, drop_self, window_cols, ptrF, nodeF, nullptr, ptrS,
                         nodeS, nullptr, count, nullptr, nullptr, nullptr, stream);
}

int ocn_frontier_sums_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM,
                           int64_t n_cols, const int64_t* rows, int64_t Q, int32_t drop_self, int64_t window_cols,
                           const int64_t* ptrF, const int64_t* nodeF, const float* valF, const int64_t* ptrS,
                           const int64_t* nodeS, const float* valS, const int64_t* off, int64_t* edges, float* val, void* stream) {
  return frontier_launch(val ? 2 : 1, rowptrA, colA, rowptrM, colM, n_cols, rows, Q, drop_self, window_cols, ptrF, nodeF, valF,
                         ptrS, nodeS, valS, nullptr, off, edges, val, stream);
}

}  // extern "C"
