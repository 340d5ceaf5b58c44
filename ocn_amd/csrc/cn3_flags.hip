// The common-neighbour stage, K1 for the 3-hop predictor cn6 without a stored A³: the cn3 flags of a candidate batch from
// A, Aᵀ and the dense bit rows of A².  See include/ocn_hip.h (ocn_cn3_flags) for the contract.
//
// For a candidate (i, j) the p-th neighbour k of i is a cn3 entry exactly when A³[j, k] != 0, i.e. when some m with
// A[m, k] != 0 has A²[j, m] != 0: when row k of Aᵀ holds a column whose bit is set in bit row j of A².  A membership test is
// one probe of that bit row; a neighbour is settled by its first hit.
#include "common.h"

constexpr int CN3_UNROLL = 4;      /* independent (column id, probe) load pairs in flight per lane */

// Work item = (batch row, walk_group() consecutive 64-neighbour chunks of N(i)): the items of ocn_chunk_offsets, so a hub
// source spreads over many waves and a light one is a single item (common.h: walk_group, WALK_ITEM_ELEMS).  A WAVE owns an
// item and takes its chunks one after the other.  The rows Aᵀ[k] of a chunk's 64 neighbours are FLATTENED: lane t keeps the
// start and the running offset of neighbour t's row in the wave's LDS slice and the lanes sweep the concatenation with
// consecutive (coalesced) colT loads, so short rows do not idle lanes; every element is probed against bit row j, a hit
// marks its neighbour in LDS (an idempotent store), and elements of a marked neighbour are skipped from the next round on.
// One lane per neighbour stores its flag byte; the per-candidate count (one ballot per chunk) and the column histogram
// take integer atomics: the outputs do not depend on which wave ran which item.  No workgroup barrier.
__global__ __launch_bounds__(OCN_BLOCK) void cn3_flags_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrT, const int32_t* __restrict__ colT,
    const unsigned* __restrict__ bmP, i64 bm_stride, const i64* __restrict__ nds,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const i64* __restrict__ chunk_off, const i64* __restrict__ off, uint8_t* __restrict__ flags, i64 cap,
    u64* __restrict__ hist, int32_t* __restrict__ cnt3, int32_t* __restrict__ status) {
  __shared__ i64 s_pre[OCN_WPB][OCN_WAVE + 1];
  __shared__ i64 s_r0[OCN_WPB][OCN_WAVE];
  __shared__ int s_hit[OCN_WPB][OCN_WAVE];
  const int lane = threadIdx.x % OCN_WAVE, w = __builtin_amdgcn_readfirstlane(threadIdx.x / OCN_WAVE);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    status_raise(status, off[B], cap);
    if (chunk_off[B] < 0) status_raise(status, chunk_off[B], cap);
  }
  // offsets from a scan that gave up (ocn_hip.h: OCN_SCAN_POISON): the batch is treated as empty
  const i64 n_items = (off[B] < 0 || chunk_off[B] < 0) ? 0 : chunk_off[B];
  i64* pre = s_pre[w];
  i64* rs = s_r0[w];
  int* hit = s_hit[w];
  for (i64 item = xcd_block() * OCN_WPB + w; item < n_items; item += (i64)gridDim.x * OCN_WPB) {    // wave-uniform
    const i64 slot = walk_item_slot(chunk_off, B, item, lane);
    const i64 e = order ? order[slot] : slot;
    const i64 i = src[e], j = dst[e];
    const i64 a0 = rowptrA[i], da = rowptrA[i + 1] - a0;
    const i64 base = off[e];
    const i64 cg = walk_group(nds, i, da);
    const i64 p_lo = (item - chunk_off[slot]) * cg * WALK_CHUNK;
    const i64 p_hi = p_lo + cg * WALK_CHUNK < da ? p_lo + cg * WALK_CHUNK : da;
    const bool fits = base + da <= cap;
    const unsigned* __restrict__ bm_row = bmP + j * bm_stride;
    int c = 0;
    for (i64 p0 = p_lo; p0 < p_hi; p0 += OCN_WAVE) {
      const int nk = (int)(p_hi - p0 < OCN_WAVE ? p_hi - p0 : OCN_WAVE);
      int32_t k = 0;
      i64 r0 = 0, d = 0;
      if (lane < nk) { k = colA[a0 + p0 + lane]; r0 = rowptrT[k]; d = rowptrT[k + 1] - r0; }
      const i64 incl = wave_incl_scan(d, lane);
      const i64 total = __shfl(incl, OCN_WAVE - 1, OCN_WAVE);
      // element x of the concatenation belongs to the last neighbour t with pre[t] <= x (lanes past nk: pre = total)
      pre[lane] = incl - d;
      if (lane == 0) pre[OCN_WAVE] = 0x7fffffffffffffffll;
      rs[lane] = r0;
      hit[lane] = 0;
      wave_lds_sync();
      int lo = 0;                              // a lane's elements come in increasing x: the row pointer only moves forward
      for (i64 x0 = 0; x0 < total; x0 += CN3_UNROLL * OCN_WAVE) {       // wave-uniform trip count
        int row[CN3_UNROLL];
        int32_t m[CN3_UNROLL];
#pragma unroll
        for (int u = 0; u < CN3_UNROLL; ++u) {
          const i64 x = x0 + u * OCN_WAVE + lane;
          m[u] = -1;
          if (x < total) {
            while (pre[lo + 1] <= x) ++lo;     // <= 64 advances over the whole chunk
            if (!hit[lo]) m[u] = colT[rs[lo] + (x - pre[lo])];
          }
          row[u] = lo;
        }
#pragma unroll
        for (int u = 0; u < CN3_UNROLL; ++u)
          if (m[u] >= 0 && ((bm_row[m[u] >> 5] >> (m[u] & 31)) & 1u)) hit[row[u]] = 1;
        wave_lds_sync();                       // (the next round reads the marks)
      }
      const bool f = lane < nk && hit[lane] != 0;
      if (fits && lane < nk) flags[base + p0 + lane] = (uint8_t)(f ? OCN_F_CN1 : 0u);
      if (f) atomicAdd(hist + 2 * (i64)k, 1ull | (1ull << (2 * HF_BITS)));      // n1 and n_union of column k
      c += __popcll(__ballot(f));
      wave_lds_sync();                         // (the next chunk overwrites the slice)
    }
    if (lane == 0 && c) atomicAdd(cnt3 + e, c);      // zero on entry; a row spans several items
  }
}

extern "C" {

int ocn_cn3_flags(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT, const int32_t* colT,
                  const uint32_t* bitmapP, int64_t bm_stride_words, const int64_t* src, const int64_t* dst,
                  const int64_t* order, int64_t B, int64_t n_cols, const int64_t* off, uint8_t* flags, int64_t flags_cap,
                  uint64_t* hist, int32_t* cnt3, int32_t* status, const int64_t* nds, const int64_t* chunk_off,
                  void* stream) {
  if (B < 0 || n_cols < 0 || flags_cap < 0 || bm_stride_words < 0 || B > (int64_t)HF_MASK) return OCN_EINVAL;
  if (bm_stride_words * 32 < n_cols) return OCN_EINVAL;
  if (B == 0) return 0;
  if (!rowptrA || !rowptrT || !bitmapP || !src || !dst || !off || !hist || !cnt3 || !status || !chunk_off) return OCN_EINVAL;
  if (flags_cap > 0 && !flags) return OCN_EINVAL;
  // col pointers may legitimately be NULL for an adjacency with no entries; the item count lives on the device
  // (chunk_off[B]): a fixed grid of what can be resident strides over the items
  const int grid = grid_for(B, 256 * 8);
  hipLaunchKernelGGL(cn3_flags_kernel, dim3(grid), dim3(OCN_BLOCK), 0, (hipStream_t)stream,
                     (const i64*)rowptrA, colA, (const i64*)rowptrT, colT, (const unsigned*)bitmapP, (i64)bm_stride_words,
                     (const i64*)nds, (const i64*)src, (const i64*)dst, (const i64*)order, (i64)B, (const i64*)chunk_off,
                     (const i64*)off, flags, (i64)flags_cap, (u64*)hist, cnt3, status);
  return launch_status();
}

}  // extern "C"
