// Frontier expansion with ordered path sums: the generalisation of the scored 2-hop expansion (recommend.hip,
// two_hop_sums_kernel) from "the row of s, weighted by w[m]" to an explicit per-query frontier list with explicit weights, and
// an optional seed list of starting values.  Chained, it walks a source's neighbourhood one hop per launch: the candidates
// within three hops with the local path index A² + decay·A³ (or its AA / RA weighted forms) are two launches of it.
// See include/ocn_hip.h (ocn_frontier_count / ocn_frontier_sums_fill).
#include "common.h"
#include "window_sweep.h"

// A window column keeps a presence bit and an fp32 accumulator (33 bits) in the CU's 160 KiB without the 2 KiB left to the scan's
// words and the runtime and the 4 KiB of the waves' claim tables below: 38 208 columns.
constexpr int FR_TAGS = 256;                                 // claim slots per wave
constexpr i64 FR_WINDOW = (i64)(160 * 1024 - 2048 - OCN_WPB * FR_TAGS * 4) * 8 / 33 / 64 * 64;
constexpr unsigned FR_FREE = 0xffffffffu;                    // a claim slot nobody bids for

// One body for the three passes, so they cannot disagree: FILL == false leaves the size of every query's set in count[q];
// FILL == true writes the pairs (s, t) from edges[off[q]] on, ascending in t; VAL == true keeps an accumulator per column and
// writes val beside the pairs.  A workgroup owns query q and sweeps the column range in windows [w0, w1); steps 1, 3 and 4 are
// the bodies of window_sweep.h that the 2-hop kernels of recommend.hip run, step 2 is this kernel's own:
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
  float* acc = ws_accumulators(fr_bm, window, n_cols);       // (VAL only: no LDS behind the bitmap otherwise)
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
      const i64 w1 = ws_window_end(w0, window, n_cols);
      const int words = ws_words(w0, w1);
      ws_clear(fr_bm, words);
      __syncthreads();
      i64 q0, q1;                                            // (an empty quarter: q1 <= q0, nothing passes below)
      ws_quarter(w0, w1, wave, q0, q1);
      if (ds > 0 && q0 < q1) {                               // the seeds of the quarter: distinct columns, before any frontier add
        const i64 lo = q0 > 0 ? ws_pair_lower_bound(nodeS, s0, ds, q0) : 0;
        for (i64 p = lo + lane; p < ds; p += OCN_WAVE) {
          const i64 c = nodeS[s0 + p].y;
          if (c >= q1) break;                                // (sorted: so is every later node of this lane)
          if (c >= q0) {
            const unsigned k = (unsigned)(c - w0);
            ws_set(fr_bm, k);
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
          lb = b0 + (q0 > 0 ? ws_lower_bound(colA + b0, le - b0, q0) : 0);
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
              ws_set(fr_bm, (unsigned)(c - w0));
            }
          continue;
        }
        u64 live = __ballot(hit);
        const u64 ones = __ballot(hit && one);
        while (live) {                                       // ascending lanes: ascending c (the same trips in every lane)
          const int j = __ffsll((long long)live) - 1;
          if (!((ones >> j) & 1ull)) {                       // several columns in the quarter: the wave walks the entry's row
            live &= live - 1;
            const i64 pe = wave_readlane64(le, j);
            const float f = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(lf), j));
            for (i64 p = wave_readlane64(lb, j) + lane; p < pe; p += OCN_WAVE) {
              const i64 c = colA[p];
              if (c >= q1) break;                            // (sorted: so is every later column of this lane)
              ws_add(fr_bm, acc, (unsigned)(c - w0), f);
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
            if (pend) ws_add(fr_bm, acc, k, lf);
            wave_lds_sync();
            continue;
          }
          const unsigned slot = k & (FR_TAGS - 1);
          while (__ballot(pend)) {
            if (pend) atomicMin(&tag[slot], (unsigned)lane);
            wave_lds_sync();
            const bool win = pend && tag[slot] == (unsigned)lane;
            if (win) ws_add(fr_bm, acc, k, lf);              // (winners hold distinct slots, so distinct columns)
            wave_lds_sync();
            if (win) { tag[slot] = FR_FREE; pend = false; }
            wave_lds_sync();
          }
        }
      }
      __syncthreads();
      ws_mask(fr_bm, colM, m0, dm, s, drop_self, w0, w1);
      __syncthreads();
      int t0, t1;                                            // contiguous words per thread: ascending columns in thread order
      const i64 c = th_thread_bits(fr_bm, words, t0, t1);
      i64 tot;
      const i64 ex = block_excl_scan(c, sh, &tot);
      if (FILL) ws_emit<VAL>(fr_bm, acc, t0, t1, s, w0, base + ex, end, edges, val);
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
  i64 window, span;
  if (ws_resolve_window(n_cols, window_cols, FR_WINDOW, &window, &span)) return OCN_EINVAL;
  if (Q == 0) return 0;
  const size_t lds = (size_t)(span / 8 + (mode == 2 ? span * 4 : 0));         // the bitmap, then the accumulators
  // at most 16 workgroups per CU's worth of queries in flight; a longer list is taken grid-stride
  const dim3 grid((unsigned)grid_for(Q, 256 * 16));
#define FR_ARGS                                                                                                                \
  (const i64*)rowptrA, colA, (const i64*)rowptrM, colM, (i64)n_cols, (const i64*)rows, (i64)Q, (int)drop_self, window,        \
      (const i64*)ptrF, (const longlong2*)nodeF, valF, (const i64*)ptrS, (const longlong2*)nodeS, valS, count, (const i64*)off, \
      (longlong2*)edges, val
  if (mode == 2) {
    // only the valued kernel needs its limit raised: the bitmap alone, 4 776 bytes at the most, stays below the limit every kernel has
    static std::atomic<unsigned long long> lds_raised{0ull};
    const size_t lds_max = (size_t)(FR_WINDOW / 8 + FR_WINDOW * 4);
    if (const int rc = ws_raise_lds_once((const void*)frontier_kernel<true, true>, lds_max, lds_raised)) return rc;
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
