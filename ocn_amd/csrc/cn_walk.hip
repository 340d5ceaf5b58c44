// The common-neighbour stage, K1 (walk-count route): per-candidate two-sided sweeps.  The grouped form is walk_group.hip;
// which endpoint sweeps, and the size of a work item, are common.h's (walk_reverse, walk_group).
// See include/ocn_hip.h for the reference call sites.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// K1 (walk counts): the pygho route of NeighborOverlap_large_ppa.py:147-173 without A².
// cn1 = N(i) ∩ N(j); cn2[e,k] = |N(k) ∩ N(j)| for k in N(i) (number of 2-walks j -> k), kept if > 0.
// ---------------------------------------------------------------------------------------------
// The probed neighbour set is a 256 Kbit Bloom-style bitmap in LDS (one multiplicative hash): building
// it is one atomicOr per member, probing one LDS read, and it does not care how long the row is (an
// 8 300-neighbour hub gives 3 % false positives, a typical row 0.1 %).  Elements that pass it — the
// true hits (~1 % of the swept elements) plus the false positives — are queued in LDS and resolved in
// bulk, one per thread, by binary search in the sorted CSR row; done inline that search would run with
// a handful of live lanes on nearly every wave iteration.
// (WALK_BM_BITS and the hash walk_bit: common.h)
#define WALK_BM_WORDS (1 << (WALK_BM_BITS - 5))
constexpr int WALK_Q = 1024;      /* queue entries; flushed when half full, overflow resolves in place */
// The probed row itself is kept in LDS beside its bitmap (it passes through the workgroup's hands anyway when the bitmap
// is built): resolving a queued element, and the cn1 test of the finalise step, are then binary searches in LDS —
// ~10 dependent LDS reads instead of ~10 dependent trips to L2, which were two thirds of an item's chain of dependent
// loads.  Rows longer than WALK_SET (hubs) keep the search in memory.  The room comes from halving the bitmap
// (128 Kbit: twice the false positives, each now one cheap LDS search).
constexpr int WALK_SET = 4096;

__device__ __forceinline__ void walk_bm_add(unsigned* bm, int32_t v) {
  const unsigned b = walk_bit(v);
  atomicOr(&bm[b >> 5], 1u << (b & 31));
}
__device__ __forceinline__ bool walk_bm_maybe(const unsigned* bm, int32_t v) {
  const unsigned b = walk_bit(v);
  return (bm[b >> 5] >> (b & 31)) & 1u;
}

// position of key in the sorted row a[0..n), or -1 (not common.h's sorted_has: the callers need the position)
__device__ __forceinline__ i64 sorted_find(const int32_t* __restrict__ a, i64 n, int32_t key) {
  i64 lo = 0, hi = n;
  while (lo < hi) {
    const i64 mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && a[lo] == key) ? lo : -1;
}

// position of key in the probed row (LDS copy when it fits, else the CSR row in memory), or -1
__device__ __forceinline__ i64 walk_set_find(const int32_t* s_set, const int32_t* __restrict__ set_g, i64 ds, int32_t key) {
  if (ds <= WALK_SET) {
    int lo = 0, hi = (int)ds;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_set[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < (int)ds && s_set[lo] == key) ? lo : -1;
  }
  return sorted_find(set_g, ds, key);
}

constexpr int WALK_THREADS = 512;   /* threads per walk work item */
#define WALK_WAVES (WALK_THREADS / OCN_WAVE)
#define WALK_ROWS (WALK_WAVES * WALK_CHUNK)   /* rows a forward item can take: one 64-row chunk per wave */

// The rows of one item, flattened.  Wave w loads the ids / starts / lengths of rows [64w, 64w+64) of
// the item (`first` = index of the item's first row id in colA) and scans the lengths; after the
// barrier the chunk totals are folded in, so that element x of the concatenation belongs to the last
// row t with s_pre[t] <= x (s_pre[n_rows] = INT_MAX).  Returns the number of elements.
__device__ __forceinline__ int walk_item_rows(const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
                                              i64 first, int n_rows, int* s_pre, i64* s_r0, int32_t* s_r,
                                              int* s_ctot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int t = threadIdx.x;                 // WALK_THREADS == WALK_ROWS: one row per thread
  int32_t r = 0;
  i64 r0 = 0, dr = 0;
  if (t < n_rows) { r = colA[first + t]; r0 = rowptrA[r]; dr = rowptrA[r + 1] - r0; }
  const i64 incl = wave_incl_scan(dr, lane);                 // an item's elements stay far below 2^31
  if (lane == OCN_WAVE - 1) s_ctot[w] = (int)incl;
  s_r[t] = r; s_r0[t] = r0;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int q = 0; q < WALK_WAVES; ++q) {
    const int c = s_ctot[q];
    if (q < w) before += c;
    total += c;
  }
  s_pre[t] = t < n_rows ? before + (int)(incl - dr) : 0x7fffffff;
  if (t == 0) s_pre[WALK_ROWS] = 0x7fffffff;
  __syncthreads();
  return total;
}

// One work item of either direction: `rows` = the neighbours of the sweeping endpoint prepared by
// walk_item_rows, `set_g[0..ds)` = the sorted neighbour row of the other endpoint whose bitmap is in
// s_bm.  Calls hit(key, row_in_item, position_in_set) for every swept element that is a member of
// the set.
template <typename Hit>
__device__ __forceinline__ void walk_sweep(const int32_t* __restrict__ colA, const unsigned* s_bm, const int* s_pre,
                                           const i64* s_r0, int total, const int32_t* s_set, const int32_t* __restrict__ set_g, i64 ds,
                                           int32_t* s_qk, uint16_t* s_qr, int* s_nq, Hit hit) {
  constexpr int WU = 8;                      // independent element loads in flight per thread
  int lo = 0;                                // a thread's elements come in increasing x: the row pointer only moves forward
  for (int x0 = 0; x0 < total; x0 += WU * WALK_THREADS) {              // workgroup-uniform trip count
    int row[WU];
    int32_t m[WU];
#pragma unroll
    for (int u = 0; u < WU; ++u) {
      const int x = x0 + u * WALK_THREADS + threadIdx.x;
      m[u] = -1;
      if (x < total) {
        while (s_pre[lo + 1] <= x) ++lo;     // <= WALK_ROWS advances over the whole item
        m[u] = colA[s_r0[lo] + (x - s_pre[lo])];
      }
      row[u] = lo;
    }
#pragma unroll
    for (int u = 0; u < WU; ++u) {
      if (m[u] >= 0 && walk_bm_maybe(s_bm, m[u])) {
        const int q = atomicAdd(s_nq, 1);
        if (q < WALK_Q) { s_qk[q] = m[u]; s_qr[q] = (uint16_t)row[u]; }
        else {                                                      // queue full (dense overlap): resolve in place
          const i64 pos = walk_set_find(s_set, set_g, ds, m[u]);
          if (pos >= 0) hit(m[u], row[u], pos);
        }
      }
    }
    // The flush decision must be workgroup-uniform (the branch holds barriers): every thread reads
    // the queue fill inside the barrier itself, before any wave can append for the next round.
    const int flush = __syncthreads_or(*s_nq > WALK_Q / 2 || x0 + WU * WALK_THREADS >= total);
    if (flush) {
      const int nq = *s_nq < WALK_Q ? *s_nq : WALK_Q;
      for (int q = threadIdx.x; q < nq; q += WALK_THREADS) {
        const i64 pos = walk_set_find(s_set, set_g, ds, s_qk[q]);
        if (pos >= 0) hit(s_qk[q], (int)s_qr[q], pos);
      }
      __syncthreads();
      if (threadIdx.x == 0) *s_nq = 0;
      __syncthreads();
    }
  }
}

#define WALK_SHARED                                     \
  __shared__ unsigned s_bm[WALK_BM_WORDS];              \
  __shared__ int32_t s_set[WALK_SET];                   \
  __shared__ int s_pre[WALK_ROWS + 1];                  \
  __shared__ i64 s_r0[WALK_ROWS];                       \
  __shared__ int32_t s_r[WALK_ROWS];                    \
  __shared__ int s_ctot[WALK_WAVES];                    \
  __shared__ int32_t s_qk[WALK_Q];                      \
  __shared__ uint16_t s_qr[WALK_Q];                     \
  __shared__ int s_nq;                                  \
  __shared__ i64 s_slot, s_item

// draw the next work item (ticket counter) and find its batch slot, while the other waves clear the bitmap
#define WALK_NEXT_ITEM(TICKET, ITEM_OFF)                                                             \
  if (w == 0) {                                                                                      \
    i64 t = 0;                                                                                       \
    if (lane == 0) t = atomicAdd((TICKET), 1);                                                       \
    t = __shfl(t, 0, OCN_WAVE);                                                                      \
    const i64 sl = t < n_items ? walk_item_slot((ITEM_OFF), B, t, lane) : 0;                         \
    if (lane == 0) { s_item = t; s_slot = sl; s_nq = 0; }                                            \
  } else {                                                                                           \
    for (int q = threadIdx.x - OCN_WAVE; q < WALK_BM_WORDS; q += WALK_THREADS - OCN_WAVE) s_bm[q] = 0u; \
  }                                                                                                  \
  __syncthreads();                                                                                   \
  const i64 item = s_item;                                                                           \
  if (item >= n_items) break;                                                                        \
  const i64 slot = s_slot;                                                                           \
  const i64 e = order ? order[slot] : slot;                                                          \
  const i64 i = src[e], j = dst[e];                                                                  \
  const i64 a0 = rowptrA[i], da = rowptrA[i + 1] - a0;                                               \
  const i64 b0 = rowptrA[j], db = rowptrA[j + 1] - b0;                                               \
  const i64 base = off[e]

// Reverse sweep (runs first, only for the batch rows walk_reverse() selects): work item = (batch row,
// chunk of WALK_REV_CHUNK neighbours m of j).  The members k' of the rows N(m) are probed against
// N(i); a hit adds one walk to wc[off[e] + position of k' in N(i)] (wc is zero on entry).  The forward
// kernel's items of that batch row then only finalise it.  Items differ 100x in cost: workgroups draw
// them from a ticket counter.
__global__ __launch_bounds__(WALK_THREADS) void cn_walk_rev_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const i64* __restrict__ rev_off, const i64* __restrict__ off, int32_t* __restrict__ wc, i64 cap,
    int32_t* __restrict__ ticket) {
  WALK_SHARED;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const i64 n_items = rev_off[B];
  for (;;) {
    WALK_NEXT_ITEM(ticket, rev_off);
    const i64 p_lo = (item - rev_off[slot]) * WALK_REV_CHUNK;
    const int nm = (int)(((p_lo + WALK_REV_CHUNK) < db ? (p_lo + WALK_REV_CHUNK) : db) - p_lo);
    const int32_t* ni_g = colA + a0;
    for (i64 q = threadIdx.x; q < da; q += WALK_THREADS) {
      const int32_t v = ni_g[q];
      walk_bm_add(s_bm, v);
      if (q < WALK_SET) s_set[q] = v;
    }
    int total = walk_item_rows(rowptrA, colA, b0 + p_lo, nm, s_pre, s_r0, s_r, s_ctot);
    if (base + da > cap) total = 0;
    int32_t* wrow = wc + base;
    walk_sweep(colA, s_bm, s_pre, s_r0, total, s_set, ni_g, da, s_qk, s_qr, &s_nq,
               [wrow](int32_t, int, i64 pos) { atomicAdd(wrow + pos, 1); });
    __syncthreads();
  }
}

// Forward sweep.  Work item = (batch row, group of <= WALK_WAVES consecutive 64-row chunks of N(i));
// items are enumerated through the exclusive scan chunk_off[] so that a hub source node is spread
// over many workgroups instead of serialising one, while a light row is a single item (one round of
// dependent loads for all its rows).  The members of the item's rows N(k) are FLATTENED: the threads
// sweep the concatenation of the rows, so short rows do not idle lanes, no load waits on a per-row
// pointer chase, and a hub k costs what its length costs; each is probed against N(j), and a hit
// bumps the row's counter with an LDS atomic.  For a batch row the reverse sweep has already counted
// (walk_reverse()), the item only reads its counts back from wc and finalises flags, histogram and
// per-edge counts.
__global__ __launch_bounds__(WALK_THREADS) void cn_walk_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA, const i64* __restrict__ nds,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const i64* __restrict__ chunk_off, const i64* __restrict__ off, uint8_t* __restrict__ flags,
    int32_t* __restrict__ wc, i64 cap, u64* __restrict__ hist, int32_t* __restrict__ cnt1,
    int32_t* __restrict__ cnt2, int32_t* __restrict__ status) {   // status[0] flags, [1] / [2] item tickets (zero on entry)
  WALK_SHARED;
  __shared__ int s_walks[WALK_ROWS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    status_raise(status, off[B], cap);
    if (chunk_off[B] < 0) status_raise(status, chunk_off[B], cap);
  }
  const i64 n_items = chunk_off[B];
  for (;;) {
    WALK_NEXT_ITEM(status + 1, chunk_off);
    const bool rev = walk_reverse(nds, i, j, da, db);      // workgroup-uniform
    const int32_t* nj_g = colA + b0;
    for (i64 q = threadIdx.x; q < db; q += WALK_THREADS) {
      const int32_t v = nj_g[q];
      walk_bm_add(s_bm, v);
      if (q < WALK_SET) s_set[q] = v;
    }
    const i64 n_chunks = (da + WALK_CHUNK - 1) / WALK_CHUNK;
    const i64 cg = walk_group(nds, i, da);
    const i64 p_lo = (item - chunk_off[slot]) * cg * WALK_CHUNK;
    const i64 p_hi = p_lo + cg * WALK_CHUNK < da ? p_lo + cg * WALK_CHUNK : da;
    (void)n_chunks;
    const int nk = (int)(p_hi - p_lo);
    const bool in_cap = base + da <= cap;
    s_walks[threadIdx.x] = 0;
    int total = walk_item_rows(rowptrA, colA, a0 + p_lo, nk, s_pre, s_r0, s_r, s_ctot);
    if (rev) total = 0;
    int* walks_of = s_walks;
    walk_sweep(colA, s_bm, s_pre, s_r0, total, s_set, nj_g, db, s_qk, s_qr, &s_nq,
               [walks_of](int32_t, int row, i64) { atomicAdd(walks_of + row, 1); });
    __syncthreads();
    {                                          // finalise: one row per thread
      const int t = threadIdx.x;
      bool f1 = false, f2 = false;
      if (t < nk) {
        const int32_t k = s_r[t];
        const int walks = rev ? (in_cap ? wc[base + p_lo + t] : 0) : s_walks[t];
        f1 = walk_bm_maybe(s_bm, k) && walk_set_find(s_set, nj_g, db, k) >= 0;
        f2 = walks > 0;
        if (in_cap) {
          flags[base + p_lo + t] = (uint8_t)((f1 ? OCN_F_CN1 : 0u) | (f2 ? OCN_F_CN2 : 0u));
          if (!rev) wc[base + p_lo + t] = walks;
        }
        if (f1 | f2) {
          atomicAdd(hist + 2 * (i64)k, (u64)f1 | ((u64)f2 << HF_BITS) | (1ull << (2 * HF_BITS)));
          if (f2) atomicAdd(hist + 2 * (i64)k + 1, (u64)walks);
        }
      }
      const int c1 = __popcll(__ballot(f1)), c2 = __popcll(__ballot(f2));
      if (lane == 0) {                         // cnt1 / cnt2 are zero on entry; a row spans several waves and items
        if (c1) atomicAdd(cnt1 + e, c1);
        if (c2) atomicAdd(cnt2 + e, c2);
      }
    }
    __syncthreads();
  }
}

// wc[0 .. min(off[B], cap)) = 0: the reverse sweep accumulates into it
__global__ __launch_bounds__(OCN_BLOCK) void walk_zero_kernel(const i64* __restrict__ off, i64 B, i64 cap,
                                                              int32_t* __restrict__ wc) {
  i64 n = off[B];
  if (n > cap) n = cap;
  for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (i64)gridDim.x * blockDim.x) wc[q] = 0;
}

// nds[v] = Σ_{u ∈ N(v)} deg(u): the number of elements a sweep of v's neighbour rows touches
__global__ __launch_bounds__(OCN_BLOCK) void neighbor_degree_sum_kernel(const i64* __restrict__ rowptr,
                                                                        const int32_t* __restrict__ col, i64 n,
                                                                        i64* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (i64 v = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; v < n; v += ((i64)gridDim.x * blockDim.x) >> 6) {
    i64 s = 0;
    for (i64 p = rowptr[v] + lane; p < rowptr[v + 1]; p += OCN_WAVE) {
      const int32_t u = col[p];
      s += rowptr[u + 1] - rowptr[u];
    }
    s = wave_sum(s);
    if (lane == 0) out[v] = s;
  }
}

extern "C" {

int ocn_cn_walk_flags(const int64_t* rowptrA, const int32_t* colA, const int64_t* nds, const int64_t* src,
                      const int64_t* dst, const int64_t* order, int64_t B, const int64_t* chunk_off,
                      const int64_t* rev_off, const int64_t* off, int64_t max_row_len, uint8_t* flags, int32_t* wc,
                      int64_t flags_cap, uint64_t* hist, int32_t* cnt1, int32_t* cnt2, int32_t* status,
                      void* stream) {
  if (B < 0 || flags_cap < 0 || B > (int64_t)HF_MASK) return OCN_EINVAL;
  if (B == 0) return 0;
  if (!rowptrA || !src || !dst || !chunk_off || !off || !hist || !cnt1 || !cnt2 || !status) return OCN_EINVAL;
  if (flags_cap > 0 && (!flags || !wc)) return OCN_EINVAL;
  if ((nds == nullptr) != (rev_off == nullptr)) return OCN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  (void)max_row_len;
  // the item counts live on the device (chunk_off[B], rev_off[B]); fixed grids stride over them
  const int grid = grid_for(4 * B, 256 * 4);   // what can be resident; the items are drawn from a ticket counter
  if (nds && flags_cap > 0) {
    hipLaunchKernelGGL(walk_zero_kernel, dim3(grid_for((flags_cap + OCN_BLOCK - 1) / OCN_BLOCK, 2048)),
                       dim3(OCN_BLOCK), 0, st, (const i64*)off, (i64)B, (i64)flags_cap, wc);
    hipLaunchKernelGGL(cn_walk_rev_kernel, dim3(grid), dim3(WALK_THREADS), 0, st,
                       (const i64*)rowptrA, colA, (const i64*)src, (const i64*)dst, (const i64*)order, (i64)B,
                       (const i64*)rev_off, (const i64*)off, wc, (i64)flags_cap, status + 2);
  }
  hipLaunchKernelGGL(cn_walk_kernel, dim3(grid), dim3(WALK_THREADS), 0, st,
                     (const i64*)rowptrA, colA, (const i64*)nds, (const i64*)src,
                     (const i64*)dst, (const i64*)order, (i64)B, (const i64*)chunk_off, (const i64*)off, flags, wc,
                     (i64)flags_cap, (u64*)hist, cnt1, cnt2, status);
  return launch_status();
}

int ocn_neighbor_degree_sum(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t* out, void* stream) {
  if (n_rows < 0 || (n_rows > 0 && (!rowptr || !out))) return OCN_EINVAL;
  if (n_rows == 0) return 0;
  hipLaunchKernelGGL(neighbor_degree_sum_kernel, dim3(grid_for((n_rows + OCN_WPB - 1) / OCN_WPB, 1 << 16)),
                     dim3(OCN_BLOCK), 0, (hipStream_t)stream, (const i64*)rowptr, col, (i64)n_rows, (i64*)out);
  return launch_status();
}

int32_t ocn_walk_chunk(void) { return WALK_CHUNK; }

}  // extern "C"
