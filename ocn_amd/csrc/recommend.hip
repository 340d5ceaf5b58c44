// Link recommendation: the candidate set of a source as a row difference of two CSR matrices (its 2-hop neighbourhood
// that is not yet linked: pattern(A² row s) \ (N(s) ∪ {s})), and the k best entries of every segment of a flat score
// vector.  Both are ragged and row-parallel: a wave owns a query / a segment from its first load to its last store, no
// atomics, no workspace, and the output of every row is fixed by its input alone.
// See include/ocn_hip.h (ocn_row_diff_count / ocn_row_diff_fill, ocn_segment_topk).  ocn_segment_rank answers the inverse
// question in the same order: the place a given node takes in its segment, however far down.
// Where A² is not stored (more columns than the A*A pattern takes, or simply too large) the same candidate set is expanded
// from A itself: a workgroup owns a query and keeps the union of its neighbours' rows as a bitmap in LDS, one window of the
// column range at a time (ocn_two_hop_diff_count / ocn_two_hop_diff_fill).
#include "common.h"
#include "window_sweep.h"
#include "topk_key.h"

// ---------------------------------------------------------------------------------------------
// row difference P[s,:] \ M[s,:]
// ---------------------------------------------------------------------------------------------
// Columns of the M row a wave stages in LDS: 2 KiB per wave, 8 KiB per workgroup — eight workgroups per CU keep 64 of the
// CU's 160 KiB, so the staging never lowers the occupancy the registers allow.  M is an adjacency: rows beyond 512 entries
// are the few hubs of a power-law graph, and those are searched where they lie (their top-of-tree lines stay in L1 / L2).
constexpr int RD_STAGE = 512;

// membership of key in the sorted row a[0..n): the number of steps depends on n alone, which every lane of the wave shares,
// and every load is in bounds for any key (a lane without a column carries -1, which no row holds)
// (not common.h's sorted_has: fixed trips for the row length and 32-bit positions, so that a lane carrying -1 runs along)
template <typename Row>
__device__ __forceinline__ bool rd_row_has(Row a, int n, int32_t key) {
  if (n <= 0) return false;
  int base = 0;
  for (int len = n; len > 1;) {
    const int half = len >> 1;
    base += (a[base + half] <= key) ? half : 0;
    len -= half;
  }
  return a[base] == key;
}

// One body for both passes, so they cannot disagree: FILL == false leaves the size of every query's set in count[q],
// FILL == true writes the (s, c) pairs of query q from edges[off[q]] on, in ascending column order.  The P row is streamed
// 64 columns at a time; each lane searches its column in the M row, a ballot of the columns that stay gives every such
// lane its place (the popcount of the lanes below it) and the wave's running base moves on by the popcount of the ballot.
template <bool FILL>
__global__ __launch_bounds__(OCN_BLOCK) void row_diff_kernel(
    const i64* __restrict__ rowptrP, const int32_t* __restrict__ colP,
    const i64* __restrict__ rowptrM, const int32_t* __restrict__ colM,
    const i64* __restrict__ rows, i64 Q, int drop_self,
    int32_t* __restrict__ count, const i64* __restrict__ off, longlong2* __restrict__ edges) {
  __shared__ int32_t s_m[OCN_WPB][RD_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t* sm = s_m[wave];
  for (i64 q = (i64)blockIdx.x * OCN_WPB + wave; q < Q; q += (i64)gridDim.x * OCN_WPB) {
    const i64 s = rows[q];
    const i64 p0 = rowptrP[s], dp = rowptrP[s + 1] - p0;
    const i64 m0 = rowptrM[s];
    const int dm = (int)(rowptrM[s + 1] - m0);               // (columns are distinct int32 ids: a row has fewer than 2^31)
    const bool staged = dm <= RD_STAGE;
    if (staged) {
      for (int t = lane; t < dm; t += OCN_WAVE) sm[t] = colM[m0 + t];
      wave_lds_sync();
    }
    const int32_t self = drop_self ? (int32_t)s : -1;
    i64 base = FILL ? off[q] : 0;
    const i64 end = FILL ? off[q + 1] : 0;
    for (i64 c0 = 0; c0 < dp; c0 += OCN_WAVE) {
      const i64 p = c0 + lane;
      const int32_t cv = colP[p0 + (p < dp ? p : dp - 1)];
      const int32_t c = p < dp ? cv : -1;
      const bool in_m = staged ? rd_row_has(sm, dm, c) : rd_row_has(colM + m0, dm, c);
      const bool keep = (c >= 0) & !in_m & (c != self);
      const u64 mask = __ballot(keep);
      if (FILL) {
        const i64 at = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && at < end) edges[at] = make_longlong2(s, (i64)c);       // (at < end: offsets of another input write nothing past their own segment)
      }
      base += __popcll(mask);
    }
    if (!FILL && lane == 0) count[q] = (int32_t)base;
    if (staged) wave_lds_sync();                          // the next query's staging writes stay behind this one's reads
  }
}

// ---------------------------------------------------------------------------------------------
// 2-hop row difference ( U_{m in A[s,:]} A[m,:] ) \ M[s,:], expanded from A
// ---------------------------------------------------------------------------------------------
// The default window: what the A*A pattern kernel keeps of the CU's 160 KiB (2 KiB are left to the scan's words and the
// runtime), as bits.  1 294 336 columns, a multiple of 64.
constexpr i64 TH_WINDOW = (i64)(160 * 1024 - 2048) * 8;

// One body for both passes, so they cannot disagree.  A workgroup owns query q; the column range is swept in windows
// [w0, w1) of `window` columns, the window's part of the set as a bitmap in LDS (window_sweep.h: one body per step, shared with
// the valued sibling below, the frontier expansion and the 2-hop sampler; steps 1 - 3 are its th_window_bitmap):
//   1. the bitmap is cleared;
//   2. a wave takes a neighbour m of s, finds where row m enters the window (binary search, skipped for the first window)
//      and sets a bit per column below w1 — LDS atomicOr: the lanes of a wave, and the waves, do meet in one word;
//   3. the bits of M[s,:] inside the window, and of s itself under drop_self, are cleared (atomicAnd);
//   4. every thread counts the bits of its contiguous words; the block scan of these counts (wave prefixes through LDS) places
//      the thread's columns behind the query's running base, which moves on by the window's total.
// Every barrier is reached by the whole workgroup: the query loop and the window loop run on blockIdx and kernel arguments
// alone, never on a row length.  A column outside [w0, w1) never touches the bitmap, whatever the rows hold.
template <bool FILL>
__global__ __launch_bounds__(OCN_BLOCK) void two_hop_diff_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrM, const int32_t* __restrict__ colM, i64 n_cols,
    const i64* __restrict__ rows, i64 Q, int drop_self, i64 window,
    int32_t* __restrict__ count, const i64* __restrict__ off, longlong2* __restrict__ edges) {
  extern __shared__ __attribute__((aligned(16))) unsigned th_bm[];
  __shared__ i64 sh[2 * OCN_WPB];
  for (i64 q = blockIdx.x; q < Q; q += gridDim.x) {
    const i64 s = rows[q];
    const i64 a0 = rowptrA[s], da = rowptrA[s + 1] - a0;
    const i64 m0 = rowptrM[s], dm = rowptrM[s + 1] - m0;
    i64 base = FILL ? off[q] : 0;
    const i64 end = FILL ? off[q + 1] : 0;
    for (i64 w0 = 0; w0 < n_cols; w0 += window) {
      const i64 w1 = ws_window_end(w0, window, n_cols);
      const int words = ws_words(w0, w1);
      th_window_bitmap(th_bm, rowptrA, colA, a0, da, colM, m0, dm, s, drop_self, w0, w1, words);   // steps 1 - 3
      int t0, t1;                                            // contiguous words per thread: ascending columns in thread order
      const i64 c = th_thread_bits(th_bm, words, t0, t1);
      i64 tot;
      const i64 ex = block_excl_scan(c, sh, &tot);
      if (FILL) ws_emit<false>(th_bm, nullptr, t0, t1, s, w0, base + ex, end, edges, nullptr);
      base += tot;
      __syncthreads();                                       // the next window's clear stays behind this one's reads
    }
    if (!FILL && threadIdx.x == 0) count[q] = (int32_t)base;
  }
}

// ---------------------------------------------------------------------------------------------
// the same set with a path sum per member: val(s, c) = sum of w[m] over the m in A[s,:] whose row holds c
// ---------------------------------------------------------------------------------------------
// A window column keeps a presence bit and an fp32 accumulator (33 bits) in the LDS the bitmap kernel keeps: 39 168 columns.
constexpr i64 TS_WINDOW = (i64)(160 * 1024 - 2048) * 8 / 33 / 64 * 64;

// The valued sibling of two_hop_diff_kernel<true>: the same windows, the same bitmap, the same steps 3 and 4 — so the pairs,
// their order and the `off` protocol are those of the fill pass — and beside every pair its sum.  Step 2 differs, because the
// sum of a column must add its members in ascending m, whatever the launch:
//   2. the window's columns are dealt to the four waves in contiguous quarters, and EVERY wave walks ALL neighbours m of s in
//      ascending order, taking of row m the part inside its own quarter, its lanes on consecutive entries.  (The rows of 64
//      neighbours are looked up at once, a lane each — here ws_lower_bound runs per lane — and the wave then visits, in lane
//      order, those that have a column in the quarter.)  An accumulator is therefore only ever touched by one wave, the lanes of one
//      instruction touch distinct columns, and LDS executes a wave's instructions in order: a plain read-add-write per member
//      is the ascending-m sum, with no accumulator atomics and no barrier between neighbours.  The presence bit is set by an
//      atomicOr (lanes, and at a quarter's edge waves, do meet in one word) whose return value tells the first member of a
//      column from the later ones: the first one adds to 0.0f, so the accumulators are never cleared.
// A member counts by its bit, never by its value: a weight may be zero or negative.  w == nullptr: every weight is 1.0f.
__global__ __launch_bounds__(OCN_BLOCK) void two_hop_sums_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrM, const int32_t* __restrict__ colM, i64 n_cols,
    const i64* __restrict__ rows, i64 Q, int drop_self, i64 window, const float* __restrict__ w, int wcol,
    const i64* __restrict__ off, longlong2* __restrict__ edges, float* __restrict__ val) {
  extern __shared__ __attribute__((aligned(16))) unsigned th_bm[];
  __shared__ i64 sh[2 * OCN_WPB];
  float* acc = ws_accumulators(th_bm, window, n_cols);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (i64 q = blockIdx.x; q < Q; q += gridDim.x) {
    const i64 s = rows[q];
    const i64 a0 = rowptrA[s], da = rowptrA[s + 1] - a0;
    const i64 m0 = rowptrM[s], dm = rowptrM[s + 1] - m0;
    i64 base = off[q];
    const i64 end = off[q + 1];
    for (i64 w0 = 0; w0 < n_cols; w0 += window) {
      const i64 w1 = ws_window_end(w0, window, n_cols);
      const int words = ws_words(w0, w1);
      ws_clear(th_bm, words);
      __syncthreads();
      i64 q0, q1;                                            // (an empty quarter: q1 <= q0, nothing passes below)
      ws_quarter(w0, w1, wave, q0, q1);
      for (i64 t0 = 0; t0 < da; t0 += OCN_WAVE) {
        // 64 neighbours at a time, one per lane: where its row enters the quarter (a search per lane, 64 side by side), where
        // it ends, its weight, and whether it has a column in the quarter at all — most rows miss most quarters of a wide graph
        const i64 tt = t0 + lane;
        i64 lb = 0, le = 0;
        float lw = 0.0f;
        if (tt < da) {
          const i64 m = colA[a0 + tt];
          const i64 b0 = rowptrA[m];
          le = rowptrA[m + 1];
          lb = b0 + (q0 > 0 ? ws_lower_bound(colA + b0, le - b0, q0) : 0);
          lw = w ? w[m * 4 + wcol] : 1.0f;
        }
        u64 live = __ballot(lb < le && (i64)colA[lb < le ? lb : a0] < q1);   // (a0: in bounds, da > 0 here; the value is not used)
        while (live) {                                       // ascending lanes: ascending m (the same trips in every lane)
          const int j = __ffsll((long long)live) - 1;
          live &= live - 1;
          const i64 pe = wave_readlane64(le, j);
          const float wm = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(lw), j));
          for (i64 p = wave_readlane64(lb, j) + lane; p < pe; p += OCN_WAVE) {
            const i64 c = colA[p];
            if (c >= q1) break;                              // (sorted: so is every later column of this lane)
            ws_add(th_bm, acc, (unsigned)(c - w0), wm);
          }
          wave_lds_sync();                                   // the next neighbour's reads stay behind this one's writes
        }
      }
      __syncthreads();
      ws_mask(th_bm, colM, m0, dm, s, drop_self, w0, w1);
      __syncthreads();
      int t0, t1;                                            // contiguous words per thread: ascending columns in thread order
      const i64 c = th_thread_bits(th_bm, words, t0, t1);
      i64 tot;
      const i64 ex = block_excl_scan(c, sh, &tot);
      ws_emit<true>(th_bm, acc, t0, t1, s, w0, base + ex, end, edges, val);
      base += tot;
      __syncthreads();                                       // the next window's clear stays behind this one's reads
    }
  }
}

// ---------------------------------------------------------------------------------------------
// segmented top-k
// ---------------------------------------------------------------------------------------------
constexpr int TOPK_AHEAD = 4;                                // chunks of 64 scores loaded ahead of their tests

// A wave keeps the best keys of its segment sorted, best first, across its lanes: slot j lives in lane j & 63, register
// j >> 6 (NS registers: one for k <= 64, two up to 128).  The segment is consumed 64 scores at a time; a chunk none of whose
// keys beats the k-th best costs one ballot.  Otherwise the keys that do are inserted one by one, in lane order: every slot
// keeps its key if that beats the new one, else it takes the new key or its upper neighbour's, whichever is smaller — one
// shuffle per register — and the k-th best is read again, so a later key of the chunk that no longer beats it is dropped
// unseen.  Keys are distinct, so the list, and with it the output, is fixed by the segment alone.
template <int NS>
__global__ __launch_bounds__(OCN_BLOCK) void segment_topk_kernel(
    const float* __restrict__ scores, const i64* __restrict__ ptr, i64 Q, int k,
    float* __restrict__ top_val, i64* __restrict__ top_pos) {
  const int lane = threadIdx.x & 63;
  const int kl = (k - 1) & 63;                               // the k-th best lives in this lane of the last register
  for (i64 q = (i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6); q < Q; q += (i64)gridDim.x * OCN_WPB) {
    const i64 b = ptr[q], n = ptr[q + 1] - b;
    u64 v[NS];
#pragma unroll
    for (int r = 0; r < NS; ++r) v[r] = 0ull;
    u64 thr = 0ull;
    for (i64 c0 = 0; c0 < n; c0 += (i64)OCN_WAVE * TOPK_AHEAD) {
      float x[TOPK_AHEAD];
#pragma unroll
      for (int t = 0; t < TOPK_AHEAD; ++t) {
        const i64 p = c0 + t * OCN_WAVE + lane;
        x[t] = scores[b + (p < n ? p : n - 1)];
      }
#pragma unroll
      for (int t = 0; t < TOPK_AHEAD; ++t) {
        const i64 p = c0 + t * OCN_WAVE + lane;
        const u64 key = p < n ? topk_key(x[t], (unsigned)p) : 0ull;
        u64 m = __ballot(key > thr);
        while (m) {                                          // (the same trip count in every lane)
          const int sl = __ffsll((long long)m) - 1;
          m &= m - 1;
          const u64 nk = wave_readlane64(key, sl);
          if (nk <= thr) continue;
          u64 up[NS];
#pragma unroll
          for (int r = 0; r < NS; ++r) up[r] = topk_shfl_up1(v[r]);
          if (NS == 2) { const u64 carry = wave_readlane64(v[0], 63); if (lane == 0) up[NS - 1] = carry; }
          if (lane == 0) up[0] = ~0ull;
#pragma unroll
          for (int r = 0; r < NS; ++r) v[r] = v[r] > nk ? v[r] : (up[r] > nk ? nk : up[r]);
          thr = wave_readlane64(v[NS - 1], kl);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      const int j = r * OCN_WAVE + lane;
      if (j < k) {
        const bool has = v[r] != 0ull;
        const i64 at = b + (i64)(0xffffffffu - (unsigned)v[r]);
        top_val[q * k + j] = has ? scores[at] : -__builtin_inff();
        top_pos[q * k + j] = has ? at : -1;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// segmented rank
// ---------------------------------------------------------------------------------------------
// Where a given node stands in the order above: a wave owns target j.  Its segment is the last q with tptr[q] <= j (a search
// of the wave's own index: empty target lists are stepped over, and no index leaves [0, Q) whatever tptr holds); the node is
// looked up in the segment's ascending ids (the second of every pair: a lower bound, the same loads in every lane); then the
// segment's scores are streamed as the top-k streams them — TOPK_AHEAD chunks loaded ahead of their tests, the tail clamped —
// and every lane counts the keys that beat the target's.  Keys are distinct, so 1 + that count is the place the entry takes
// in an unbounded top-k.  Every branch below is taken by the whole wave; no LDS, no barrier, no atomics.
__global__ __launch_bounds__(OCN_BLOCK) void segment_rank_kernel(
    const float* __restrict__ scores, const i64* __restrict__ ptr, const longlong2* __restrict__ edges, i64 Q,
    const i64* __restrict__ tptr, const i64* __restrict__ tnode, i64 P, i64* __restrict__ rank, i64* __restrict__ pos) {
  const int lane = threadIdx.x & 63;
  for (i64 j = (i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6); j < P; j += (i64)gridDim.x * OCN_WPB) {
    i64 q = 0;
    for (i64 len = Q; len > 1;) {                            // the last q in [0, Q) with tptr[q] <= j (0 if there is none)
      const i64 half = len >> 1;
      q += (tptr[q + half] <= j) ? half : 0;
      len -= half;
    }
    const i64 b = ptr[q], n = ptr[q + 1] - b;
    const i64 node = tnode[j];
    const i64 lo = ws_pair_lower_bound(edges, b, n, node);  // the first entry whose id is not below node
    if (lo >= n || edges[b + lo].y != node) {                // any int64 that is no id of the segment, an empty segment
      if (lane == 0) { rank[j] = 0; pos[j] = -1; }
      continue;
    }
    const u64 tk = topk_key(scores[b + lo], (unsigned)lo);
    unsigned ahead = 0u;                                     // (a lane tests fewer than 2^26 entries)
    for (i64 c0 = 0; c0 < n; c0 += (i64)OCN_WAVE * TOPK_AHEAD) {
      float x[TOPK_AHEAD];
#pragma unroll
      for (int t = 0; t < TOPK_AHEAD; ++t) {
        const i64 p = c0 + t * OCN_WAVE + lane;
        x[t] = scores[b + (p < n ? p : n - 1)];
      }
#pragma unroll
      for (int t = 0; t < TOPK_AHEAD; ++t) {
        const i64 p = c0 + t * OCN_WAVE + lane;
        ahead += (p < n && topk_key(x[t], (unsigned)p) > tk) ? 1u : 0u;
      }
    }
    const i64 total = wave_sum((i64)ahead);
    if (lane == 0) { rank[j] = total + 1; pos[j] = b + lo; }
  }
}

static inline unsigned wave_grid(i64 items) { return (unsigned)grid_for((items + OCN_WPB - 1) / OCN_WPB, 256 * 8); }

// both passes of the 2-hop row difference (a template: outside the C linkage block).  Each instance of the kernel has its own
// LDS limit, raised once; the LDS a launch asks for is that launch's span / 8.
template <bool FILL>
static int two_hop_launch(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM,
                          int64_t n_cols, const int64_t* rows, int64_t Q, int32_t drop_self, int64_t window_cols, int32_t* count,
                          const int64_t* off, int64_t* edges, void* stream) {
  if (Q < 0 || !rowptrA || !colA || !rowptrM || !colM || !rows) return OCN_EINVAL;
  if (FILL ? (!off || !edges) : !count) return OCN_EINVAL;
  i64 window, span;
  if (ws_resolve_window(n_cols, window_cols, TH_WINDOW, &window, &span)) return OCN_EINVAL;
  if (Q == 0) return 0;
  static std::atomic<unsigned long long> lds_raised{0ull};
  if (const int rc = ws_raise_lds_once((const void*)two_hop_diff_kernel<FILL>, (size_t)(TH_WINDOW / 8), lds_raised)) return rc;
  hipLaunchKernelGGL(two_hop_diff_kernel<FILL>, dim3((unsigned)grid_for(Q)), dim3(OCN_BLOCK), (size_t)(span / 8),
                     (hipStream_t)stream, (const i64*)rowptrA, colA, (const i64*)rowptrM, colM, (i64)n_cols, (const i64*)rows,
                     (i64)Q, (int)drop_self, window, count, (const i64*)off, (longlong2*)edges);
  return launch_status();
}

extern "C" {

int32_t ocn_row_diff_stage_cols(void) { return RD_STAGE; }

static int row_diff_launch(bool fill, const int64_t* rowptrP, const int32_t* colP, const int64_t* rowptrM, const int32_t* colM,
                           const int64_t* rows, int64_t Q, int32_t drop_self, int32_t* count, const int64_t* off, int64_t* edges,
                           void* stream) {
  if (Q < 0 || !rowptrP || !colP || !rowptrM || !colM || !rows) return OCN_EINVAL;
  if (fill ? (!off || !edges) : !count) return OCN_EINVAL;
  if (Q == 0) return 0;
  const dim3 grid(wave_grid(Q));
  if (fill)
    hipLaunchKernelGGL(row_diff_kernel<true>, grid, dim3(OCN_BLOCK), 0, (hipStream_t)stream, (const i64*)rowptrP, colP,
                       (const i64*)rowptrM, colM, (const i64*)rows, (i64)Q, (int)drop_self, (int32_t*)nullptr, (const i64*)off,
                       (longlong2*)edges);
  else
    hipLaunchKernelGGL(row_diff_kernel<false>, grid, dim3(OCN_BLOCK), 0, (hipStream_t)stream, (const i64*)rowptrP, colP,
                       (const i64*)rowptrM, colM, (const i64*)rows, (i64)Q, (int)drop_self, count, (const i64*)nullptr,
                       (longlong2*)nullptr);
  return launch_status();
}

int ocn_row_diff_count(const int64_t* rowptrP, const int32_t* colP, const int64_t* rowptrM, const int32_t* colM,
                       const int64_t* rows, int64_t Q, int32_t drop_self, int32_t* count, void* stream) {
  return row_diff_launch(false, rowptrP, colP, rowptrM, colM, rows, Q, drop_self, count, nullptr, nullptr, stream);
}

int ocn_row_diff_fill(const int64_t* rowptrP, const int32_t* colP, const int64_t* rowptrM, const int32_t* colM,
                      const int64_t* rows, int64_t Q, int32_t drop_self, const int64_t* off, int64_t* edges, void* stream) {
  return row_diff_launch(true, rowptrP, colP, rowptrM, colM, rows, Q, drop_self, nullptr, off, edges, stream);
}

int64_t ocn_two_hop_window_cols(void) { return TH_WINDOW; }

int ocn_two_hop_diff_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM,
                           int64_t n_cols, const int64_t* rows, int64_t Q, int32_t drop_self, int64_t window_cols,
                           int32_t* count, void* stream) {
  return two_hop_launch<false>(rowptrA, colA, rowptrM, colM, n_cols, rows, Q, drop_self, window_cols, count, nullptr, nullptr,
                               stream);
}

int ocn_two_hop_diff_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM,
                          int64_t n_cols, const int64_t* rows, int64_t Q, int32_t drop_self, int64_t window_cols,
                          const int64_t* off, int64_t* edges, void* stream) {
  return two_hop_launch<true>(rowptrA, colA, rowptrM, colM, n_cols, rows, Q, drop_self, window_cols, nullptr, off, edges,
                              stream);
}

int64_t ocn_two_hop_sums_window_cols(void) { return TS_WINDOW; }

int ocn_two_hop_sums_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM,
                          int64_t n_cols, const int64_t* rows, int64_t Q, int32_t drop_self, int64_t window_cols, const float* w,
                          int32_t wcol, const int64_t* off, int64_t* edges, float* val, void* stream) {
  if (Q < 0 || !rowptrA || !colA || !rowptrM || !colM || !rows || !off || !edges || !val) return OCN_EINVAL;
  i64 window, span;
  if (ws_resolve_window(n_cols, window_cols, TS_WINDOW, &window, &span)) return OCN_EINVAL;
  if (w && (wcol < 0 || wcol > 3)) return OCN_EINVAL;
  if (Q == 0) return 0;
  const size_t lds = (size_t)(span / 8 + span * 4);                           // the bitmap, then the accumulators
  static std::atomic<unsigned long long> lds_raised{0ull};
  const size_t lds_max = (size_t)(TS_WINDOW / 8 + TS_WINDOW * 4);
  if (const int rc = ws_raise_lds_once((const void*)two_hop_sums_kernel, lds_max, lds_raised)) return rc;
  // at most 16 workgroups per CU's worth of queries in flight: a request of a few thousand sources is dealt a workgroup per
  // source by the hardware, a longer list is taken grid-stride
  hipLaunchKernelGGL(two_hop_sums_kernel, dim3((unsigned)grid_for(Q, 256 * 16)), dim3(OCN_BLOCK), lds, (hipStream_t)stream,
                     (const i64*)rowptrA, colA, (const i64*)rowptrM, colM, (i64)n_cols, (const i64*)rows, (i64)Q, (int)drop_self,
                     window, w, (int)(w ? wcol : 0), (const i64*)off, (longlong2*)edges, val);
  return launch_status();
}

int32_t ocn_segment_topk_max_k(void) { return TOPK_MAX; }

int ocn_segment_topk(const float* scores, const int64_t* ptr, int64_t Q, int32_t k, float* top_val, int64_t* top_pos,
                     void* stream) {
  if (Q < 0 || k < 1 || k > TOPK_MAX || !ptr || !top_val || !top_pos) return OCN_EINVAL;
  if (Q == 0) return 0;
  if (!scores) return OCN_EINVAL;
  const dim3 grid(wave_grid(Q));
  if (k <= OCN_WAVE)
    hipLaunchKernelGGL(segment_topk_kernel<1>, grid, dim3(OCN_BLOCK), 0, (hipStream_t)stream, scores, (const i64*)ptr, (i64)Q,
                       (int)k, top_val, (i64*)top_pos);
  else
    hipLaunchKernelGGL(segment_topk_kernel<2>, grid, dim3(OCN_BLOCK), 0, (hipStream_t)stream, scores, (const i64*)ptr, (i64)Q,
                       (int)k, top_val, (i64*)top_pos);
  return launch_status();
}

int ocn_segment_rank(const float* scores, const int64_t* ptr, const int64_t* edges, int64_t Q, const int64_t* tptr,
                     const int64_t* tnode, int64_t P, int64_t* rank, int64_t* pos, void* stream) {
  if (Q < 0 || P < 0 || !scores || !ptr || !edges || !tptr || !tnode || !rank || !pos) return OCN_EINVAL;
  if (Q == 0 || P == 0) return 0;
  hipLaunchKernelGGL(segment_rank_kernel, dim3(wave_grid(P)), dim3(OCN_BLOCK), 0, (hipStream_t)stream, scores, (const i64*)ptr,
                     (const longlong2*)edges, (i64)Q, (const i64*)tptr, (const i64*)tnode, (i64)P, (i64*)rank, (i64*)pos);
  return launch_status();
}

}  // extern "C"
