// Edge insertion into a resident graph: A' = A U D as a row-wise union of two CSR patterns, and the exact update of the
// dense bit rows of A² from the identity
//
//   pattern(A'·A') = pattern(A·A) U pattern(D·A') U pattern(A'·D)          (D = the new entries, a subset of A')
//
// Row u of D·A' is the OR of the A' rows of u's new neighbours; A'·D sets bit v in every row that has u as a neighbour,
// for each new entry (u, v).  The work is one row length of A' per new entry — thousands of bit sets where the product
// from scratch rewrites every bit row.  OR is idempotent: D may overlap A or repeat itself.
// See include/ocn_hip.h (ocn_csr_union_count / ocn_csr_union_fill, ocn_bitrows_insert).
#include "common.h"

// ---------------------------------------------------------------------------------------------
// row-wise union of two CSR patterns
// ---------------------------------------------------------------------------------------------
// Columns of the shorter row a wave stages in LDS (2 KiB per wave, as the row difference of recommend.hip): the searches of
// the longer row's elements then stay on chip.  A longer "short" row is searched where it lies.
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
// running count carries it across rounds.  With KEEP_DUP the element x[i] lands at i + (elements of y below it) - (duplicates
// before it): its own index plus the smaller elements of the other row that are not duplicates.  Without, duplicates are
// dropped and x[i] lands at (elements of y below it) + i - (duplicates before it).  Both are the same expression; what
// differs is whether the duplicate itself is written.  Returns the number of duplicates.
template <bool FILL, bool KEEP_DUP, typename RowY>
__device__ __forceinline__ int un_stream(const int32_t* __restrict__ x, int nx, RowY y, int ny, int lane,
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
    if (FILL && i < nx && (KEEP_DUP || !dup)) {
      const i64 at = (i64)i + lb - (dups + __popcll(m & ((1ull << lane) - 1ull)));
      if (at < cap) out[at] = v;                          // (at < cap: offsets of another input write nothing past their own segment)
    }
    dups += __popcll(m);
  }
  return dups;
}

// One body for both passes, so they cannot disagree: FILL == false leaves the size of every row's union in count[r],
// FILL == true writes its columns, ascending, from colC[rowptrC[r]] on.  A wave owns a row.  The union is symmetric in its
// operands: L is the longer row, S the shorter.  S empty (nearly every row: D has few entries) is a coalesced copy of L.
// Otherwise L is streamed against S (staged in LDS when it fits) and keeps its duplicates, S is streamed against L and drops
// them: every element computes its own place from binary searches, no sequential merge, no atomics.
template <bool FILL>
__global__ __launch_bounds__(OCN_BLOCK) void csr_union_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrB, const int32_t* __restrict__ colB, i64 n_rows,
    int32_t* __restrict__ count, const i64* __restrict__ rowptrC, int32_t* __restrict__ colC) {
  __shared__ int32_t s_s[OCN_WPB][UN_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t* ss = s_s[wave];
  for (i64 r = (i64)blockIdx.x * OCN_WPB + wave; r < n_rows; r += (i64)gridDim.x * OCN_WPB) {
    const i64 a0 = rowptrA[r], b0 = rowptrB[r];
    const int da = (int)(rowptrA[r + 1] - a0), db = (int)(rowptrB[r + 1] - b0);   // (distinct int32 columns: fewer than 2^31)
    const bool a_long = da >= db;
    const int32_t* L = a_long ? colA + a0 : colB + b0;
    const int32_t* S = a_long ? colB + b0 : colA + a0;
    const int nl = a_long ? da : db, ns = a_long ? db : da;
    int32_t* out = FILL ? colC + rowptrC[r] : nullptr;
    const i64 cap = FILL ? rowptrC[r + 1] - rowptrC[r] : 0;
    if (ns <= 0) {
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
    if (FILL) {
      if (staged) un_stream<true, true>(L, nl, (const int32_t*)ss, ns, lane, out, cap);
      else un_stream<true, true>(L, nl, S, ns, lane, out, cap);
      un_stream<true, false>(S, ns, L, nl, lane, out, cap);
    } else {
      const int dups = un_stream<false, false>(S, ns, L, nl, lane, (int32_t*)nullptr, 0);
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
    i64 lo = 0, hi = n_off;                                // off[0] = 0 <= w < off[n_off]: the answer is in [0, n_off)
    while (hi - lo > 1) {
      const i64 mid = (lo + hi) >> 1;
      if (off[mid] <= w) lo = mid; else hi = mid;
    }
    const i64 e = lo >> 1;
    const i64 chunk = w - off[lo];
    const i64 u = erow[e], v = colD[e];
    if (!(lo & 1)) {
      const i64 p0 = rowptrA[v] + chunk * BI_CHUNK;
      const i64 p1 = (p0 + BI_CHUNK) < rowptrA[v + 1] ? (p0 + BI_CHUNK) : rowptrA[v + 1];
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
      const i64 p0 = rowptrT[u] + chunk * BI_CHUNK;
      const i64 p1 = (p0 + BI_CHUNK) < rowptrT[u + 1] ? (p0 + BI_CHUNK) : rowptrT[u + 1];
      const unsigned bit = 1u << (v & 31);
      for (i64 q = p0 + lane; q < p1; q += OCN_WAVE) {
        const i64 r = colT[q];
        if (r >= 0 && r < n && !(atomicOr(bits + r * stride + (v >> 5), bit) & bit)) atomicAdd(added + r, 1);
      }
    }
  }
}

extern "C" {

int ocn_csr_union_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB, const int32_t* colB,
                        int64_t n_rows, int32_t* count, void* stream) {
  if (n_rows < 0 || !rowptrA || !colA || !rowptrB || !colB || !count) return OCN_EINVAL;
  if (n_rows == 0) return 0;
  hipLaunchKernelGGL((csr_union_kernel<false>), dim3(grid_for((n_rows + OCN_WPB - 1) / OCN_WPB, 1 << 16)), dim3(OCN_BLOCK), 0,
                     (hipStream_t)stream, (const i64*)rowptrA, colA, (const i64*)rowptrB, colB, (i64)n_rows, count,
                     (const i64*)nullptr, (int32_t*)nullptr);
  return launch_status();
}

int ocn_csr_union_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrB, const int32_t* colB,
                       int64_t n_rows, const int64_t* rowptrC, int32_t* colC, void* stream) {
  if (n_rows < 0 || !rowptrA || !colA || !rowptrB || !colB || !rowptrC || !colC) return OCN_EINVAL;
  if (n_rows == 0) return 0;
  hipLaunchKernelGGL((csr_union_kernel<true>), dim3(grid_for((n_rows + OCN_WPB - 1) / OCN_WPB, 1 << 16)), dim3(OCN_BLOCK), 0,
                     (hipStream_t)stream, (const i64*)rowptrA, colA, (const i64*)rowptrB, colB, (i64)n_rows, (int32_t*)nullptr,
                     (const i64*)rowptrC, colC);
  return launch_status();
}

int64_t ocn_bitrows_insert_workspace_bytes(int64_t nnzD) {
  // items int32[2 nnzD] | off int64[2 nnzD + 1] | erow int32[nnzD] | scan state
  if (nnzD < 0) return 0;
  return bi_align(2 * nnzD * 4) + bi_align((2 * nnzD + 1) * 8) + bi_align(nnzD * 4) + bi_align(ocn_scan_workspace_bytes(2 * nnzD)) + 64;
}

int ocn_bitrows_insert(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT, const int32_t* colT,
                       const int64_t* rowptrD, const int32_t* colD, int64_t n, int64_t nnzD, uint32_t* bits,
                       int64_t bm_stride_words, int32_t* added, void* workspace, void* stream) {
  if (n < 0 || nnzD < 0 || nnzD > 0x3fffffffll || bm_stride_words < 0 || bm_stride_words * 32 < n) return OCN_EINVAL;
  if (!rowptrA || !colA || !rowptrT || !colT || !rowptrD || !colD || !bits || !added || !workspace) return OCN_EINVAL;
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
  hipLaunchKernelGGL(bi_apply_kernel, dim3(grid_for((2 * nnzD + OCN_WPB - 1) / OCN_WPB, 2048)), dim3(OCN_BLOCK), 0, st,
                     (const i64*)rowptrA, colA, (const i64*)rowptrT, colT, colD, (const int32_t*)erow, (const i64*)off,
                     (i64)(2 * nnzD), (i64)n, (unsigned*)bits, (i64)bm_stride_words, added);
  return launch_status();
}

}  // extern "C"
