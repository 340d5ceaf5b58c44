// Edge insertion into a resident graph: A' = A U D as a row-wise union of two CSR patterns, and the exact update of the
// dense bit rows of A² from the identity
//
//   pattern(A'·A') = pattern(A·A) U pattern(D·A') U pattern(A'·D)          (D = the new entries, a subset of A')
//
// Row u of D·A' is the OR of the A' rows of u's new neighbours; A'·D sets bit v in every row that has u as a neighbour,
// for each new entry (u, v).  The work is one row length of A' per new entry — thousands of bit sets where the product
// from scratch rewrites every bit row.  OR is idempotent: D may overlap A or repeat itself.
// See include/ocn_hip.h (ocn_csr_union_count / ocn_csr_union_fill, ocn_bitrows_insert).
//
// Edge removal, further down: A' = A \ D as a row-wise difference, and the bit rows of A² turned into those of A'·A' by
// deciding again every bit that had a witness walk through a removed entry — bit (r, k) stays exactly when row r of A' and
// row k of A'^T share a column (ocn_csr_minus_count / ocn_csr_minus_fill, ocn_bitrows_remove).
//
// Which rows of the encoder output an update can reach, last: the closed neighbourhood of a row list as one bit row, on the
// same chunked schedule, and a bit row as an ascending id list (ocn_rows_neighbourhood, ocn_bitlist_count / _fill).
#include "common.h"

// ---------------------------------------------------------------------------------------------
// row-wise union and difference of two CSR patterns
// ---------------------------------------------------------------------------------------------
// Columns of the shorter row (the difference: of B's row) a wave stages in LDS (2 KiB per wave, as the row difference of
// recommend.hip): the searches of the longer row's elements then stay on chip.  A longer "short" row is searched where it lies.
constexpr int UN_STAGE = 512;

// first position of the sorted row a[0..n) whose column is not below key; every load is inside the row
template <typename Row>
__device__ __forceinline__ int un_lower_bound(Row a, int n, int32_t key) {
  int base = 0;
  for (int len = n; len > 0;) {
    const int half = len >> 1;
    if (a[base + half] < key) { base += half + 1; len -= half + 1; } else len = half;
  }
  return base;
}

// Streams the row x[0..nx) 64 columns at a time against the sorted row y[0..ny).  An element that y holds too is a
// duplicate; the ballot of the duplicates gives every lane the number of duplicates before its own element, the wave's
// running count carries it across rounds.  MODE 0 and 1 are the two halves of a union: x[i] lands at i + (elements of y below
// it) - (duplicates before it), its own index plus the smaller elements of the other row that are not duplicates; MODE 0
// writes the duplicate itself, MODE 1 leaves it to the other half.  MODE 2 is the difference: the elements of y do not
// enter the place and a duplicate is dropped.  Returns the number of duplicates.
template <bool FILL, int MODE, typename RowY>
__device__ __forceinline__ int set_stream(const int32_t* __restrict__ x, int nx, RowY y, int ny, int lane,
                                          int32_t* __restrict__ out, i64 cap) {
  int dups = 0;
  for (int i0 = 0; i0 < nx; i0 += OCN_WAVE) {
    const int i = i0 + lane;
    bool dup = false;
    int lb = 0;
    int32_t v = 0;
    if (i < nx) {
      v = x[i];
      lb = un_lower_bound(y, ny, v);
      dup = lb < ny && y[lb] == v;
    }
    const u64 m = __ballot(dup);
    if (FILL && i < nx && (MODE == 0 || !dup)) {
      // (at >= 0: at most i duplicates come before element i; at < cap: offsets of another input write nothing past
      // their own segment)
      const i64 at = (i64)i + (MODE == 2 ? 0 : lb) - (dups + __popcll(m & ((1ull << lane) - 1ull)));
      if (at < cap) out[at] = v;
    }
    dups += __popcll(m);
  }
  return dups;
}

// C[r, :] = A[r, :] U B[r, :], or A[r, :] \ B[r, :] under MINUS.  One body for both passes, so they cannot disagree:
// FILL == false leaves the size of every row's result in count[r], FILL == true writes its columns, ascending, from
// colC[rowptrC[r]] on.  A wave owns a row.  The union is symmetric in its operands: L is the longer row, S the shorter.  The
// difference always has L = A's row and S = B's.  S empty (nearly every row: D has few entries) is a coalesced copy of L.
// Otherwise S is staged in LDS when it fits.  Union: L is streamed against S and keeps its duplicates, S is streamed against L
// and drops them.  Difference: L is streamed against S and drops them.  Every element computes its own place from binary
// searches: no sequential merge, no atomics, nothing written at or past rowptrC[r + 1].
template <bool FILL, bool MINUS>
__global__ __launch_bounds__(OCN_BLOCK) void csr_setop_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrB, const int32_t* __restrict__ colB, i64 n_rows,
    int32_t* __restrict__ count, const i64* __restrict__ rowptrC, int32_t* __restrict__ colC) {
  __shared__ int32_t s_s[OCN_WPB][UN_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t* ss = s_s[wave];
  for (i64 r = (i64)blockIdx.x * OCN_WPB + wave; r < n_rows; r += (i64)gridDim.x * OCN_WPB) {
    const i64 a0 = rowptrA[r], b0 = rowptrB[r];
    const int da = (int)(rowptrA[r + 1] - a0), db = (int)(rowptrB[r + 1] - b0);   // (distinct int32 columns: fewer than 2^31)
    const bool a_long = MINUS || da >= db;
    const int32_t* L = a_long ? colA + a0 : colB + b0;
    const int32_t* S = a_long ? colB + b0 : colA + a0;
    const int nl = a_long ? da : db, ns = a_long ? db : da;
    int32_t* out = FILL ? colC + rowptrC[r] : nullptr;
    const i64 cap = FILL ? rowptrC[r + 1] - rowptrC[r] : 0;
    if (ns <= 0 || (MINUS && nl <= 0)) {
      if (FILL) {
        for (int i = lane; i < nl && i < cap; i += OCN_WAVE) out[i] = L[i];
      } else if (lane == 0) {
        count[r] = nl > 0 ? nl : 0;
      }
      continue;
    }
    const bool staged = ns <= UN_STAGE;
    if (staged) {
      for (int t = lane; t < ns; t += OCN_WAVE) ss[t] = S[t];
      wave_lds_sync();
    }
    if (MINUS) {
      const int dups = staged ? set_stream<FILL, 2>(L, nl, (const int32_t*)ss, ns, lane, out, cap)
                              : set_stream<FILL, 2>(L, nl, S, ns, lane, out, cap);
      if (!FILL && lane == 0) count[r] = nl - dups;
    } else if (FILL) {
      if (staged) set_stream<true, 0>(L, nl, (const int32_t*)ss, ns, lane, out, cap);
      else set_stream<true, 0>(L, nl, S, ns, lane, out, cap);
      set_stream<true, 1>(S, ns, L, nl, lane, out, cap);
    } else {
      const int dups = set_stream<false, 1>(S, ns, L, nl, lane, (int32_t*)nullptr, 0);
      if (lane == 0) count[r] = nl + ns - dups;
    }
    if (staged) wave_lds_sync();                          // the next row's staging writes stay behind this one's reads
  }
}

// ---------------------------------------------------------------------------------------------
// D·A' and A'·D into dense bit rows
// ---------------------------------------------------------------------------------------------
// Elements of a row per work item: four wave rounds.  A hub row of A' (tens of thousands of entries) becomes many items,
// which the grid's waves take in turn, instead of one wave's serial loop.
constexpr int BI_CHUNK = 256;

static inline int64_t bi_align(int64_t b) { return (b + 15) / 16 * 16; }

__global__ __launch_bounds__(OCN_BLOCK) void bi_zero_kernel(int32_t* __restrict__ a, i64 n) {
  for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (i64)gridDim.x * blockDim.x) a[q] = 0;
}

// One wave per row of D: entry e = (u, v) of D learns its row (erow[e] = u) and the number of its items of either kind —
// items[2e] = chunks of A' row v (kind a: OR that row into bit row u), items[2e + 1] = chunks of A'^T row u (kind b: set bit v
// in every row that has u as a neighbour).
__global__ __launch_bounds__(OCN_BLOCK) void bi_items_kernel(const i64* __restrict__ rowptrA, const i64* __restrict__ rowptrT,
                                                             const i64* __restrict__ rowptrD, const int32_t* __restrict__ colD,
                                                             i64 n, i64 nnzD, int32_t* __restrict__ erow, int32_t* __restrict__ items) {
  const int lane = threadIdx.x & 63;
  for (i64 u = (i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6); u < n; u += (i64)gridDim.x * OCN_WPB) {
    const i64 d0 = rowptrD[u], d1 = rowptrD[u + 1];
    if (d1 <= d0) continue;
    const i64 lt = rowptrT[u + 1] - rowptrT[u];
    const int32_t ct = (int32_t)((lt + BI_CHUNK - 1) / BI_CHUNK);
    for (i64 e = d0 + lane; e < d1 && e < nnzD; e += OCN_WAVE) {
      const i64 v = colD[e];
      const bool ok = v >= 0 && v < n;                     // (a column outside the matrix has no items: nothing is indexed with it)
      const i64 la = ok ? rowptrA[v + 1] - rowptrA[v] : 0;
      erow[e] = (int32_t)u;
      items[2 * e] = (int32_t)((la + BI_CHUNK - 1) / BI_CHUNK);
      items[2 * e + 1] = ok ? ct : 0;
    }
  }
}

// Work item w of the bit-row schedule: the last k with off[k] <= w names entry e = k / 2 of D and the kind (k even: a, odd:
// b), w - off[k] the chunk of that item's row.  Returns k.
__device__ __forceinline__ i64 bi_item(const i64* off, i64 n_off, i64 w, i64& chunk) {
  i64 lo = 0, hi = n_off;                                  // off[0] = 0 <= w < off[n_off]: the answer is in [0, n_off)
  while (hi - lo > 1) {
    const i64 mid = (lo + hi) >> 1;
    if (off[mid] <= w) lo = mid; else hi = mid;
  }
  chunk = w - off[lo];
  return lo;
}

// [p0, p1): the positions of that chunk of row `row`, clipped to the row's end.  Returns p0.
__device__ __forceinline__ i64 bi_chunk(const i64* rowptr, i64 row, i64 chunk, i64& p1) {
  const i64 p0 = rowptr[row] + chunk * BI_CHUNK;
  p1 = (p0 + BI_CHUNK) < rowptr[row + 1] ? (p0 + BI_CHUNK) : rowptr[row + 1];
  return p0;
}

// A wave takes work item w (grid stride): the last k with off[k] <= w names entry e = k / 2 and its kind, w - off[k] the
// chunk.  Bits are set with atomicOr on the 32-bit word; a bit is new exactly when the word that came back did not have it —
// exact when two items set the same bit (one of them sees it set) and when it was set before.  Kind a: all lanes work on bit
// row u, their new-bit votes go through a ballot into one count per item, added to added[u] with one atomic.  Kind b: every
// lane has another row, and adds one to its row's count.
__global__ __launch_bounds__(OCN_BLOCK) void bi_apply_kernel(const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
                                                             const i64* __restrict__ rowptrT, const int32_t* __restrict__ colT,
                                                             const int32_t* __restrict__ colD, const int32_t* __restrict__ erow,
                                                             const i64* __restrict__ off, i64 n_off, i64 n,
                                                             unsigned* __restrict__ bits, i64 stride, int32_t* __restrict__ added) {
  const int lane = threadIdx.x & 63;
  const i64 total = off[n_off];
  for (i64 w = (i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6); w < total; w += (i64)gridDim.x * OCN_WPB) {
    i64 chunk;
    const i64 lo = bi_item(off, n_off, w, chunk);
    const i64 e = lo >> 1;
    const i64 u = erow[e], v = colD[e];
    if (!(lo & 1)) {
      i64 p1;
      const i64 p0 = bi_chunk(rowptrA, v, chunk, p1);
      unsigned* row = bits + u * stride;
      int fresh = 0;
      for (i64 q0 = p0; q0 < p1; q0 += OCN_WAVE) {
        const i64 q = q0 + lane;
        bool is_new = false;
        if (q < p1) {
          const i64 k = colA[q];
          if (k >= 0 && k < n) {
            const unsigned bit = 1u << (k & 31);
            is_new = !(atomicOr(row + (k >> 5), bit) & bit);
          }
        }
        fresh += __popcll(__ballot(is_new));
      }
      if (lane == 0 && fresh) atomicAdd(added + u, fresh);
    } else {
      i64 p1;
      const i64 p0 = bi_chunk(rowptrT, u, chunk, p1);
      const unsigned bit = 1u << (v & 31);
      for (i64 q = p0 + lane; q < p1; q += OCN_WAVE) {
        const i64 r = colT[q];
        if (r >= 0 && r < n && !(atomicOr(bits + r * stride + (v >> 5), bit) & bit)) atomicAdd(added + r, 1);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// the bits of A² that lose their last witness
// ---------------------------------------------------------------------------------------------
// Length of the shorter list up to which a candidate is decided by its own lane (a serial walk of that list, one narrowing
// lower-bound search of the longer list per element); beyond it the whole wave decides the candidate, lanes striding the
// shorter list.  The lane form makes the wave wait for its longest candidate, the wave form takes the candidates one after
// the other: 32 is a GUESS at where the second gets cheaper, not a measurement ("Removing edges").
constexpr int BR_LANE_MAX = 32;

// Do the sorted rows s[0..ns) and l[0..nl) (ns <= nl) share a column?  One lane, early exit on the first witness; every
// search starts where the last one ended.
__device__ __forceinline__ bool br_lane_meets(const int32_t* __restrict__ s, int ns, const int32_t* __restrict__ l, int nl) {
  int base = 0;
  for (int i = 0; i < ns && base < nl; ++i) {
    const int32_t key = s[i];
    base += un_lower_bound(l + base, nl - base, key);
    if (base < nl && l[base] == key) return true;
  }
  return false;
}

// The schedule of bi_apply_kernel — a wave takes work item w by grid stride, the last k with off[k] <= w names entry
// e = k / 2 = (u, v) of D and the kind, w - off[k] the chunk — over the rows of the OLD matrix: kind a enumerates the
// candidates (u, k) for k in row v of A (the walks u -> v -> k), kind b the candidates (r, v) for r in row u of A^T (the walks
// r -> u -> v).  Every lane holds one candidate per round.  A candidate whose bit is set now is decided on A' = (rowptrA, colA)
// and its transpose, which nothing writes: the bit stays when row r of A' and row k of A'^T share a column, else it is cleared
// with atomicAnd, and counts as removed exactly when the word that came back still had it — exact when two items reach the same
// bit (one of them sees it gone) and when D repeats itself.  The decision never depends on what another item did, so neither
// do the bits or the counts.  Kind a: all lanes work on bit row u, their votes go through a ballot into one atomic per round.
__global__ __launch_bounds__(OCN_BLOCK) void br_apply_kernel(const i64* __restrict__ rowptrA0, const int32_t* __restrict__ colA0,
                                                             const i64* __restrict__ rowptrT0, const int32_t* __restrict__ colT0,
                                                             const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
                                                             const i64* __restrict__ rowptrT, const int32_t* __restrict__ colT,
                                                             const int32_t* __restrict__ colD, const int32_t* __restrict__ erow,
                                                             const i64* __restrict__ off, i64 n_off, i64 n,
                                                             unsigned* __restrict__ bits, i64 stride, int32_t* __restrict__ removed) {
  const int lane = threadIdx.x & 63;
  const i64 total = off[n_off];
  for (i64 w = (i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6); w < total; w += (i64)gridDim.x * OCN_WPB) {
    i64 chunk;
    const i64 lo = bi_item(off, n_off, w, chunk);
    const i64 e = lo >> 1;
    const i64 u = erow[e], v = colD[e];
    if (u < 0 || u >= n || v < 0 || v >= n) continue;      // (such an entry has no items; nothing is indexed with it)
    const bool kind_a = !(lo & 1);
    const i64* rp0 = kind_a ? rowptrA0 : rowptrT0;
    const int32_t* col0 = kind_a ? colA0 : colT0;
    const i64 row0 = kind_a ? v : u;
    i64 p1;
    const i64 p0 = bi_chunk(rp0, row0, chunk, p1);
    for (i64 q0 = p0; q0 < p1; q0 += OCN_WAVE) {           // (wave-uniform bounds: every lane takes every round)
      const i64 q = q0 + lane;
      i64 r = -1, k = -1;
      if (q < p1) {
        const i64 x = col0[q];
        r = kind_a ? u : x;
        k = kind_a ? x : v;
      }
      unsigned* word = nullptr;
      unsigned bit = 0;
      const int32_t *S = nullptr, *L = nullptr;            // the shorter and the longer of A' row r and A'^T row k
      int ns = 0, nl = 0;
      bool clear = false, heavy = false;
      if (r >= 0 && r < n && k >= 0 && k < n) {
        word = bits + r * stride + (k >> 5);
        bit = 1u << (k & 31);
        if (*word & bit) {                                 // (a bit that is not set now has nothing to decide)
          const i64 a0 = rowptrA[r], t0 = rowptrT[k];
          const int la = (int)(rowptrA[r + 1] - a0), lt = (int)(rowptrT[k + 1] - t0);
          const bool a_short = la <= lt;
          S = a_short ? colA + a0 : colT + t0;
          L = a_short ? colT + t0 : colA + a0;
          ns = a_short ? la : lt;
          nl = a_short ? lt : la;
          if (ns <= BR_LANE_MAX) clear = !br_lane_meets(S, ns, L, nl);
          else heavy = true;
        }
      }
      for (u64 todo = __ballot(heavy); todo; todo &= todo - 1) {   // the whole wave on one candidate at a time
        const int src = __ffsll((long long)todo) - 1;
        const int32_t* s = (const int32_t*)__shfl((u64)S, src, OCN_WAVE);
        const int32_t* l = (const int32_t*)__shfl((u64)L, src, OCN_WAVE);
        const int cs = __shfl(ns, src, OCN_WAVE), cl = __shfl(nl, src, OCN_WAVE);
        bool met = false;
        for (int i0 = 0; i0 < cs && !met; i0 += OCN_WAVE) {
          const int i = i0 + lane;
          met = __any(i < cs && sorted_has(l, (i64)cl, s[i]));
        }
        if (lane == src) clear = !met;
      }
      bool gone = false;
      if (clear) gone = (atomicAnd(word, ~bit) & bit) != 0;
      if (kind_a) {
        const int cnt = __popcll(__ballot(gone));
        if (lane == 0 && cnt) atomicAdd(removed + u, cnt);
      } else if (gone) {
        atomicAdd(removed + r, 1);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// the closed neighbourhood of a row list, as bits; bits as an ascending id list
// ---------------------------------------------------------------------------------------------
// Listed row i learns the number of its items, the chunks of its row of (rowptrT, colT), and sets its own bit.  An id outside
// [0, n) has no items and no bit.
__global__ __launch_bounds__(OCN_BLOCK) void rn_items_kernel(const i64* __restrict__ rowptrT, const i64* __restrict__ rows, i64 n_list,
                                                             i64 n, int32_t* __restrict__ items, unsigned* __restrict__ bits) {
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_list; i += (i64)gridDim.x * blockDim.x) {
    const i64 r = rows[i];
    int32_t c = 0;
    if (r >= 0 && r < n) {
      c = (int32_t)((rowptrT[r + 1] - rowptrT[r] + BI_CHUNK - 1) / BI_CHUNK);
      atomicOr(bits + (r >> 5), 1u << (r & 31));
    }
    items[i] = c;
  }
}

// The schedule of bi_apply_kernel over a row list: a wave takes work item w by grid stride, the last i with off[i] <= w names
// the listed row, w - off[i] the chunk of at most BI_CHUNK of its elements; every lane sets the bit of one column per round.
__global__ __launch_bounds__(OCN_BLOCK) void rn_apply_kernel(const i64* __restrict__ rowptrT, const int32_t* __restrict__ colT,
                                                             const i64* __restrict__ rows, const i64* __restrict__ off, i64 n_list,
                                                             i64 n, unsigned* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const i64 total = off[n_list];
  for (i64 w = (i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6); w < total; w += (i64)gridDim.x * OCN_WPB) {
    i64 chunk;
    const i64 i = bi_item(off, n_list, w, chunk);
    const i64 r = rows[i];
    if (r < 0 || r >= n) continue;                         // (such a row has no items; nothing is indexed with it)
    i64 p1;
    const i64 p0 = bi_chunk(rowptrT, r, chunk, p1);
    for (i64 q = p0 + lane; q < p1; q += OCN_WAVE) {
      const i64 k = colT[q];
      if (k >= 0 && k < n) atomicOr(bits + (k >> 5), 1u << (k & 31));
    }
  }
}

// One thread per 32-bit word of a bit vector of n_bits bits: FILL == false leaves the word's population in count[w] (bits at
// or past n_bits do not count), FILL == true writes the ids of its bits, ascending, from out[off[w]] on.
template <bool FILL>
__global__ __launch_bounds__(OCN_BLOCK) void bitlist_kernel(const unsigned* __restrict__ bits, i64 n_bits, int32_t* __restrict__ count,
                                                            const i64* __restrict__ off, i64* __restrict__ out) {
  const i64 words = (n_bits + 31) >> 5;
  for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (i64)gridDim.x * blockDim.x) {
    unsigned b = bits[w];
    const i64 left = n_bits - (w << 5);
    if (left < 32) b &= (1u << left) - 1u;
    if (!FILL) {
      count[w] = __popc(b);
    } else {
      i64* o = out + off[w];
      const i64 end = off[w + 1];                          // (offsets of another vector write nothing past their own segment)
      while (b && o < out + end) {
        const int q = __ffs((int)b) - 1;
        b &= b - 1;
        *o++ = (w << 5) + q;
      }
    }
  }
}

// One launch for the four set-operation entries: which kernel, and which of its outputs must be there.
static int csr_setop_launch(bool minus, bool fill, const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB,
                            const int32_t* colB, int64_t n_rows, int32_t* count, const int64_t* rowptrC, int32_t* colC,
                            void* stream) {
  if (n_rows < 0 || !rowptrA || !colA || !rowptrB || !colB) return OCN_EINVAL;
  if (fill ? (!rowptrC || !colC) : !count) return OCN_EINVAL;
  if (n_rows == 0) return 0;
  static constexpr decltype(&csr_setop_kernel<false, false>) kernels[] = {   // [2 * minus + fill]
      csr_setop_kernel<false, false>, csr_setop_kernel<true, false>, csr_setop_kernel<false, true>, csr_setop_kernel<true, true>};
  hipLaunchKernelGGL(kernels[2 * minus + fill], dim3(grid_for((n_rows + OCN_WPB - 1) / OCN_WPB, 1 << 16)), dim3(OCN_BLOCK), 0,
                     (hipStream_t)stream, (const i64*)rowptrA, colA, (const i64*)rowptrB, colB, (i64)n_rows, count,
                     (const i64*)rowptrC, colC);
  return launch_status();
}

// What both bit-row updates do first: check the arguments they share, carve the workspace (items int32[2 nnzD] |
// off int64[2 nnzD + 1] | erow int32[nnzD] | scan state), leave every entry's row in erow and the running item count in off —
// the chunks per entry and kind counted on the rows (rowptrA, rowptrT) the caller's apply kernel enumerates, then scanned.
// off stays null where there is nothing to apply (no rows, or no entries of D).
static int bi_schedule(const int64_t* rowptrA, const int64_t* rowptrT, const int64_t* rowptrD, const int32_t* colD, int64_t n,
                       int64_t nnzD, const uint32_t* bits, int64_t bm_stride_words, const int32_t* changed, void* workspace,
                       void* stream, const int32_t*& erow_out, const i64*& off_out) {
  if (n < 0 || nnzD < 0 || nnzD > 0x3fffffffll || bm_stride_words < 0 || bm_stride_words * 32 < n) return OCN_EINVAL;
  if (!rowptrA || !rowptrT || !rowptrD || !colD || !bits || !changed || !workspace) return OCN_EINVAL;
  if (n == 0 || nnzD == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int32_t* items = (int32_t*)ws;
  i64* off = (i64*)(ws + bi_align(2 * nnzD * 4));
  int32_t* erow = (int32_t*)((char*)off + bi_align((2 * nnzD + 1) * 8));
  int32_t* scan_ws = (int32_t*)((char*)erow + bi_align(nnzD * 4));
  const i64 sw = bi_align(ocn_scan_workspace_bytes(2 * nnzD));
  // items of entries no row of D reaches (a rowptrD that does not cover colD) stay zero; the scan state starts zero
  hipLaunchKernelGGL(bi_zero_kernel, dim3(grid_for((2 * nnzD + OCN_BLOCK - 1) / OCN_BLOCK, 1024)), dim3(OCN_BLOCK), 0, st, items,
                     (i64)(2 * nnzD));
  hipLaunchKernelGGL(bi_zero_kernel, dim3(grid_for((nnzD + OCN_BLOCK - 1) / OCN_BLOCK, 1024)), dim3(OCN_BLOCK), 0, st, erow, (i64)nnzD);
  hipLaunchKernelGGL(bi_zero_kernel, dim3(1), dim3(OCN_BLOCK), 0, st, scan_ws, (i64)(sw / 4));
  hipLaunchKernelGGL(bi_items_kernel, dim3(grid_for((n + OCN_WPB - 1) / OCN_WPB, 1 << 16)), dim3(OCN_BLOCK), 0, st,
                     (const i64*)rowptrA, (const i64*)rowptrT, (const i64*)rowptrD, colD, (i64)n, (i64)nnzD, erow, items);
  const int rc = ocn_scan_i32(items, 2 * nnzD, (int64_t*)off, scan_ws, stream);
  if (rc) return rc;
  erow_out = erow;
  off_out = off;
  return 0;
}

extern "C" {

int ocn_csr_union_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB, const int32_t* colB,
                        int64_t n_rows, int32_t* count, void* stream) {
  return csr_setop_launch(false, false, rowptrA, colA, rowptrB, colB, n_rows, count, nullptr, nullptr, stream);
}

int ocn_csr_union_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB, const int32_t* colB,
                       int64_t n_rows, const int64_t* rowptrC, int32_t* colC, void* stream) {
  return csr_setop_launch(false, true, rowptrA, colA, rowptrB, colB, n_rows, nullptr, rowptrC, colC, stream);
}

int64_t ocn_bitrows_insert_workspace_bytes(int64_t nnzD) {
  // items int32[2 nnzD] | off int64[2 nnzD + 1] | erow int32[nnzD] | scan state
  if (nnzD < 0) return 0;
  return bi_align(2 * nnzD * 4) + bi_align((2 * nnzD + 1) * 8) + bi_align(nnzD * 4) + bi_align(ocn_scan_workspace_bytes(2 * nnzD)) + 64;
}

int ocn_bitrows_insert(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT, const int32_t* colT,
                       const int64_t* rowptrD, const int32_t* colD, int64_t n, int64_t nnzD, uint32_t* bits,
                       int64_t bm_stride_words, int32_t* added, void* workspace, void* stream) {
  if (!colA || !colT) return OCN_EINVAL;
  const int32_t* erow = nullptr;
  const i64* off = nullptr;
  const int rc = bi_schedule(rowptrA, rowptrT, rowptrD, colD, n, nnzD, bits, bm_stride_words, added, workspace, stream, erow, off);
  if (rc || !off) return rc;
  hipLaunchKernelGGL(bi_apply_kernel, dim3(grid_for((2 * nnzD + OCN_WPB - 1) / OCN_WPB, 2048)), dim3(OCN_BLOCK), 0,
                     (hipStream_t)stream, (const i64*)rowptrA, colA, (const i64*)rowptrT, colT, colD, erow, off,
                     (i64)(2 * nnzD), (i64)n, (unsigned*)bits, (i64)bm_stride_words, added);
  return launch_status();
}

int ocn_csr_minus_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB, const int32_t* colB,
                        int64_t n_rows, int32_t* count, void* stream) {
  return csr_setop_launch(true, false, rowptrA, colA, rowptrB, colB, n_rows, count, nullptr, nullptr, stream);
}

int ocn_csr_minus_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB, const int32_t* colB,
                       int64_t n_rows, const int64_t* rowptrC, int32_t* colC, void* stream) {
  return csr_setop_launch(true, true, rowptrA, colA, rowptrB, colB, n_rows, nullptr, rowptrC, colC, stream);
}

int64_t ocn_bitrows_remove_workspace_bytes(int64_t nnzD) {
  // the layout of ocn_bitrows_insert: items int32[2 nnzD] | off int64[2 nnzD + 1] | erow int32[nnzD] | scan state
  return ocn_bitrows_insert_workspace_bytes(nnzD);
}

int ocn_bitrows_remove(const int64_t* rowptrA0, const int32_t* colA0, const int64_t* rowptrT0, const int32_t* colT0,
                       const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT, const int32_t* colT,
                       const int64_t* rowptrD, const int32_t* colD, int64_t n, int64_t nnzD, uint32_t* bits,
                       int64_t bm_stride_words, int32_t* removed, void* workspace, void* stream) {
  if (!colA0 || !colT0 || !rowptrA || !colA || !rowptrT || !colT) return OCN_EINVAL;
  // the candidates are enumerated from the OLD rows: the same count of chunks per entry and kind as the insertion's, read
  // off the old row pointers
  const int32_t* erow = nullptr;
  const i64* off = nullptr;
  const int rc = bi_schedule(rowptrA0, rowptrT0, rowptrD, colD, n, nnzD, bits, bm_stride_words, removed, workspace, stream, erow, off);
  if (rc || !off) return rc;
  hipLaunchKernelGGL(br_apply_kernel, dim3(grid_for((2 * nnzD + OCN_WPB - 1) / OCN_WPB, 2048)), dim3(OCN_BLOCK), 0,
                     (hipStream_t)stream, (const i64*)rowptrA0, colA0, (const i64*)rowptrT0, colT0, (const i64*)rowptrA, colA,
                     (const i64*)rowptrT, colT, colD, erow, off, (i64)(2 * nnzD), (i64)n, (unsigned*)bits,
                     (i64)bm_stride_words, removed);
  return launch_status();
}

int64_t ocn_rows_neighbourhood_workspace_bytes(int64_t n_list) {
  // items int32[n_list] | off int64[n_list + 1] | scan state
  if (n_list < 0) return 0;
  return bi_align(n_list * 4) + bi_align((n_list + 1) * 8) + bi_align(ocn_scan_workspace_bytes(n_list)) + 64;
}

int ocn_rows_neighbourhood(const int64_t* rowptrT, const int32_t* colT, int64_t n, const int64_t* rows, int64_t n_list,
                           uint32_t* bits, void* workspace, void* stream) {
  if (n < 0 || n_list < 0 || n_list > 0x3fffffffll) return OCN_EINVAL;
  if (!rowptrT || !colT || !rows || !bits || !workspace) return OCN_EINVAL;
  if (n == 0 || n_list == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int32_t* items = (int32_t*)ws;
  i64* off = (i64*)(ws + bi_align(n_list * 4));
  int32_t* scan_ws = (int32_t*)((char*)off + bi_align((n_list + 1) * 8));
  const i64 sw = bi_align(ocn_scan_workspace_bytes(n_list));
  hipLaunchKernelGGL(bi_zero_kernel, dim3(1), dim3(OCN_BLOCK), 0, st, scan_ws, (i64)(sw / 4));   // the scan state starts zero
  hipLaunchKernelGGL(rn_items_kernel, dim3(grid_for((n_list + OCN_BLOCK - 1) / OCN_BLOCK, 1024)), dim3(OCN_BLOCK), 0, st,
                     (const i64*)rowptrT, (const i64*)rows, (i64)n_list, (i64)n, items, (unsigned*)bits);
  const int rc = ocn_scan_i32(items, n_list, (int64_t*)off, scan_ws, stream);
  if (rc) return rc;
  // (the item count is known on the device only: at least 256 workgroups, so that one listed hub row is not four waves' work)
  const i64 blocks = (n_list + OCN_WPB - 1) / OCN_WPB;
  hipLaunchKernelGGL(rn_apply_kernel, dim3(grid_for(blocks < 256 ? 256 : blocks, 2048)), dim3(OCN_BLOCK), 0, st,
                     (const i64*)rowptrT, colT, (const i64*)rows, (const i64*)off, (i64)n_list, (i64)n, (unsigned*)bits);
  return launch_status();
}

int ocn_bitlist_count(const uint32_t* bits, int64_t n_bits, int32_t* count, void* stream) {
  if (n_bits < 0 || !bits || !count) return OCN_EINVAL;
  if (n_bits == 0) return 0;
  const i64 words = (n_bits + 31) / 32;
  hipLaunchKernelGGL((bitlist_kernel<false>), dim3(grid_for((words + OCN_BLOCK - 1) / OCN_BLOCK, 4096)), dim3(OCN_BLOCK), 0,
                     (hipStream_t)stream, (const unsigned*)bits, (i64)n_bits, count, (const i64*)nullptr, (i64*)nullptr);
  return launch_status();
}

int ocn_bitlist_fill(const uint32_t* bits, int64_t n_bits, const int64_t* off, int64_t* out, void* stream) {
  if (n_bits < 0 || !bits || !off || !out) return OCN_EINVAL;
  if (n_bits == 0) return 0;
  const i64 words = (n_bits + 31) / 32;
  hipLaunchKernelGGL((bitlist_kernel<true>), dim3(grid_for((words + OCN_BLOCK - 1) / OCN_BLOCK, 4096)), dim3(OCN_BLOCK), 0,
                     (hipStream_t)stream, (const unsigned*)bits, (i64)n_bits, (int32_t*)nullptr, (const i64*)off, (i64*)out);
  return launch_status();
}

}  // extern "C"
