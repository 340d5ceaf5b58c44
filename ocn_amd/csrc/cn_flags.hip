// The common-neighbour stage, K1 (pattern route): the intersection pass.  It leaves the flag bytes, the column histogram, the
// per-candidate counts and — for the pooling (cn_pool.hip) — the slot records and group costs whose layout common.h fixes.
// See include/ocn_hip.h for the reference call sites.
#include "common.h"

// (sorted_has, wave_lds_sync and the slot record / schedule constants: common.h)

// Two-level search of a long row: `samp` (LDS) holds the row's elements at positions (s*n)>>6,
// s = 0..63; six LDS probes pick the segment, the remaining log2(n/64) probes go to memory.
__device__ __forceinline__ bool sampled_has(const int32_t* samp, const int32_t* __restrict__ row, i64 n,
                                            int32_t key) {
  int lo = 0, hi = OCN_WAVE;                 // upper bound: lo = number of samples <= key
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (samp[mid] <= key) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return false;
  const int s = lo - 1;
  const i64 p0 = ((i64)s * n) >> 6, p1 = ((i64)(s + 1) * n) >> 6;
  return sorted_has(row + p0, p1 - p0, key);
}

// ---------------------------------------------------------------------------------------------
// K1 (pattern): flags for N(src) against the rows of dst in T1 (and T2)
// ---------------------------------------------------------------------------------------------
#define T1_CAP 1024

// One wave per candidate edge, four candidates per workgroup.  Narrower groups (32 / 16 / 8 lanes per candidate, several
// candidates per wave) measured 242 / 327 / 494 us against 208 on the collab-shaped batch and no caller
// used them: the kernel is bound by the number of distinct cache lines its scattered probes touch per wave instruction —
// lanes that search the SAME rows share the top-of-tree lines, lanes of different edges do not — so one edge per wave wins
// although most source rows are < 64 long.  A wave therefore owns its slot from the first load to the last store: its
// LDS slice is ordered by wave_lds_sync(), and a hub candidate delays none of its three neighbours.
// LH: the column histogram of this workgroup is kept in LDS (n_cols <= LH_MAX_COLS, i.e. Cora /
// Citeseer / ddi-sized graphs, where tens of millions of CN entries would otherwise hammer a few
// thousand global addresses) and flushed once at the end of the workgroup's grid-stride loop.
// RECIN: words 0 - 2 of the slot's record and the flag offset in word 3 were written by the prep pass
// (ocn_order_by_node_finish_rec): the slot is ONE 32-byte load away instead of order -> src / dst -> rowptr / off.
#define LH_MAX_COLS 8192

// a value every lane of the wave holds alike, moved to scalar registers (the loads it addresses become scalar too)
__device__ __forceinline__ i64 wave_uniform(i64 v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(u64)v), hi = __builtin_amdgcn_readfirstlane((unsigned)((u64)v >> 32));
  return (i64)(((u64)hi << 32) | lo);
}
// membership of key in a sorted row of at most 64 entries held one per lane (t = INT_MAX beyond its end): lower bound in
// six cross-lane reads and one more for the element itself.  Every lane of the wave must call it.
__device__ __forceinline__ bool lanes_have(int32_t t, int32_t key) {
  int pos = 0;
#pragma unroll
  for (int step = OCN_WAVE / 2; step > 0; step >>= 1)
    if (__shfl(t, pos + step - 1, OCN_WAVE) < key) pos += step;
  return __shfl(t, pos, OCN_WAVE) == key;
}

template <bool HAS_T2, bool LH, bool RECIN>
__global__ __launch_bounds__(OCN_BLOCK) void cn_flags_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrT1, const int32_t* __restrict__ colT1,
    const i64* __restrict__ rowptrT2, const int32_t* __restrict__ colT2,
    const unsigned* __restrict__ bmT1, i64 bm1_stride, const unsigned* __restrict__ bmT2, i64 bm_stride,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    i64 n_cols, const i64* __restrict__ off, uint8_t* __restrict__ flags, i64 cap,
    u64* __restrict__ hist, int32_t* __restrict__ cnt1, int32_t* __restrict__ cnt2,
    int32_t* __restrict__ status, u64* rec, int32_t* __restrict__ gcost) {
  constexpr int GPB = OCN_WPB;
  __shared__ int s_cost[2][GPB];
  __shared__ int32_t s_t1[GPB][T1_CAP];
  __shared__ int32_t s_t2[GPB][OCN_WAVE];
  extern __shared__ __attribute__((aligned(16))) u64 s_hist[];      // LH only: n_cols words
  const int gl = threadIdx.x % OCN_WAVE, g = __builtin_amdgcn_readfirstlane(threadIdx.x / OCN_WAVE);
  if (blockIdx.x == 0 && threadIdx.x == 0) status_raise(status, off[B], cap);
  const bool void_batch = off[B] < 0;        // the offsets come from a scan that gave up (ocn_hip.h: OCN_SCAN_POISON): the batch is treated as
                                             // empty — zero counts, empty slot records — so that nothing behind this pass indexes with them
  if (LH) {
    for (i64 c = threadIdx.x; c < n_cols; c += OCN_BLOCK) s_hist[c] = 0ull;
    __syncthreads();
  }
  int par = 0;
  for (i64 e0 = (i64)blockIdx.x * GPB; e0 < B; e0 += (i64)gridDim.x * GPB, par ^= 1) {
    const i64 slot = e0 + g;                  // processing slot; `order` maps it to a batch row
    const bool act = slot < B;
    i64 e = 0, i = 0, j = 0, a0 = 0, da = 0, b0 = 0, db = 0, c0 = 0, dc = 0, base = 0;
    const unsigned* bm_row = nullptr;         // bit row of dst in T2, when T2 comes with a dense bitmap
    const unsigned* bm1_row = nullptr;        // ... and in T1 (small dense graphs: a membership test is one probe)
    if (act) {
      if (RECIN) {
        const ulonglong2* rp = reinterpret_cast<const ulonglong2*>(rec + 4 * slot);
        const ulonglong2 ra = rp[0], rb = rp[1];
        e = wave_uniform((i64)ra.x);
        i = wave_uniform((i64)(ra.y & 0xffffffffull)); j = wave_uniform((i64)(ra.y >> 32));
        a0 = wave_uniform((i64)(rb.x & ((1ull << REC_LEN_SHIFT) - 1))); da = wave_uniform((i64)(rb.x >> REC_LEN_SHIFT));
        base = wave_uniform((i64)rb.y);
      } else {
        e = order ? order[slot] : slot;
        i = src[e]; j = dst[e];
        a0 = rowptrA[i]; da = rowptrA[i + 1] - a0;
        base = off[e];
      }
      if (bmT1) bm1_row = bmT1 + j * bm1_stride;
      else { b0 = rowptrT1[j]; db = rowptrT1[j + 1] - b0; }
      if (HAS_T2) {
        if (bmT2) bm_row = bmT2 + j * bm_stride;
        if (rowptrT2 && (LH || !bmT2)) { c0 = rowptrT2[j]; dc = rowptrT2[j + 1] - c0; }   // (small graphs with bit rows too: a FULL row — a dense A², ogbl-ddi —
                                                                                  // needs no probe at all; on large graphs the two loads would only lengthen the chain)
      }
      if (void_batch) { da = 0; db = 0; dc = 0; base = 0; }
    }
    // the target row: up to 64 entries stay in the wave's registers, one per lane; a longer one, up to T1_CAP, goes to
    // this wave's LDS slice; beyond that the search runs in memory
    const bool t1_reg = db <= OCN_WAVE, t1_lds = db <= T1_CAP;
    int32_t t1 = 0x7fffffff;
    if (t1_reg) { if (gl < db) t1 = colT1[b0 + gl]; }
    else if (t1_lds)
      for (i64 q = gl; q < db; q += OCN_WAVE) s_t1[g][q] = colT1[b0 + q];
    const bool t2_full = HAS_T2 && rowptrT2 && dc == n_cols;   // a full row (dense A², e.g. ddi) contains every column
    if (HAS_T2 && !t2_full && !bmT2) {
      if (dc > OCN_WAVE) s_t2[g][gl] = colT2[c0 + (((i64)gl * dc) >> 6)];      // a 64-point sample of the long row
      else if (gl < dc) s_t2[g][gl] = colT2[c0 + gl];
    }
    wave_lds_sync();
    const bool fits = base + da <= cap;
    int c1 = 0, c2 = 0;
    for (i64 p0 = 0; p0 < da; p0 += OCN_WAVE) {      // (wave-uniform trips: lanes_have needs every lane)
      const i64 p = p0 + gl;
      const bool in = p < da;
      const int32_t k = in ? colA[a0 + p] : 0;
      unsigned w2 = 0;
      if (HAS_T2 && bmT2 && !t2_full && in) w2 = bm_row[k >> 5];    // one probe, in flight while the cn1 search runs
      bool f1;
      if (bmT1) f1 = in && ((bm1_row[k >> 5] >> (k & 31)) & 1u);
      else if (t1_reg) f1 = lanes_have(t1, k) && in;
      else f1 = in && (t1_lds ? sorted_has(&s_t1[g][0], db, k) : sorted_has(colT1 + b0, db, k));
      bool f2 = false;
      if (HAS_T2 && in) {
        if (t2_full) f2 = true;
        else if (bmT2) f2 = (w2 >> (k & 31)) & 1u;
        else f2 = dc > OCN_WAVE ? sampled_has(&s_t2[g][0], colT2 + c0, dc, k) : sorted_has(&s_t2[g][0], dc, k);
      }
      if (fits && in) flags[base + p] = (uint8_t)((f1 ? OCN_F_CN1 : 0u) | (f2 ? OCN_F_CN2 : 0u));
      if (f1 | f2) {
        const u64 inc = (u64)f1 | ((u64)f2 << HF_BITS) | (1ull << (2 * HF_BITS));
        if (LH) atomicAdd(s_hist + k, inc); else atomicAdd(hist + 2 * (i64)k, inc);
      }
      c1 += f1;
      c2 += f2;
    }
    wave_lds_sync();                          // (the next slot's row may overwrite this one's)
#pragma unroll
    for (int o = OCN_WAVE / 2; o > 0; o >>= 1) {
      c1 += __shfl_xor(c1, o, OCN_WAVE);
      c2 += __shfl_xor(c2, o, OCN_WAVE);
    }
    if (act && gl == 0) {
      cnt1[e] = c1;
      if (cnt2) cnt2[e] = c2;
      if (rec) {                              // what the pooling needs to know about this slot, in ONE 32-byte record
        u64* r = rec + 4 * slot;
        if (!RECIN) {
          r[0] = (u64)e;
          r[1] = (u64)i | ((u64)j << 32);
        }
        if (!RECIN || void_batch) r[2] = (u64)a0 | ((u64)da << REC_LEN_SHIFT);
        r[3] = (u64)base | ((u64)(da > 0 && (i64)c2 == da) << REC_FULL2_BIT) | ((u64)(c1 > 0) << 62) | ((u64)(c2 > 0) << 63);
      }
    }
    if (gcost) {
      // what this group of GPB consecutive slots will cost the pooling (entries to gather): the pooling visits its
      // groups longest first (ocn_gather_schedule), so that no straggler ends its kernel.  The one workgroup barrier of
      // an iteration, at its very end: s_cost alternates between two sets, so a wave that runs ahead into the next
      // iteration writes the other set and stops at that iteration's barrier, which thread 0 reaches after this read.
      if (gl == 0) s_cost[par][g] = act ? c1 + c2 : 0;
      __syncthreads();
      if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int q = 0; q < GPB; ++q) t = SCHED_COST(t, s_cost[par][q]);
        gcost[e0 / GPB] = t;
      }
    }
  }
  if (LH) {
    __syncthreads();
    for (i64 c = threadIdx.x; c < n_cols; c += OCN_BLOCK) {
      const u64 v = s_hist[c];
      if (v) atomicAdd(hist + 2 * c, v);
    }
  }
}

extern "C" {

int32_t ocn_cn_flags_small_graph_cols(void) { return LH_MAX_COLS; }

// rec_in: the records come half written from ocn_order_by_node_finish_rec (ocn_cn_flags_rec)
static int cn_flags_launch(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT1,
                           const int32_t* colT1, const int64_t* rowptrT2, const int32_t* colT2,
                           const uint32_t* bitmapT1, int64_t bm1_stride_words, const uint32_t* bitmapT2, int64_t bm_stride_words,
                           const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                           int64_t n_cols, const int64_t* off, uint8_t* flags, int64_t flags_cap, uint64_t* hist,
                           int32_t* cnt1, int32_t* cnt2, int32_t* status, uint64_t* rec, int32_t* gcost, bool rec_in, void* stream) {
  if (B < 0 || flags_cap < 0 || B > (int64_t)HF_MASK) return OCN_EINVAL;
  if (B == 0) return 0;
  if (!rowptrA || (!rowptrT1 && !bitmapT1) || !src || !dst || !off || !hist || !cnt1 || !status) return OCN_EINVAL;
  if (rec_in && (!rec || !order)) return OCN_EINVAL;
  if ((bitmapT1 && bm1_stride_words * 32 < n_cols) || (bitmapT2 && bm_stride_words * 32 < n_cols)) return OCN_EINVAL;
  // col pointers may legitimately be NULL for an adjacency with no entries
  constexpr int GPB = OCN_WPB;
  hipStream_t st = (hipStream_t)stream;
  const bool lh = n_cols > 0 && n_cols <= LH_MAX_COLS;
  const size_t lds = lh ? (size_t)n_cols * sizeof(u64) : 0;
  // LH: a persistent grid (a few workgroups per CU) so that each LDS histogram absorbs many edges
  const int grid = lh ? grid_for((B + GPB - 1) / GPB, 256 * 3) : grid_for((B + GPB - 1) / GPB);
  if (lh) {                                   // static (target rows) + dynamic (histogram) LDS can pass 64 KiB
    static bool raised_dev[64] = {};          // the attribute is per device (function objects are per device)
    int devid = 0;
    if (hipGetDevice(&devid) != hipSuccess || devid < 0 || devid >= 64) return OCN_EINVAL;
    bool& raised = raised_dev[devid];
    if (!raised) {
      const void* fns[4] = {(const void*)cn_flags_kernel<true, true, false>, (const void*)cn_flags_kernel<false, true, false>,
                            (const void*)cn_flags_kernel<true, true, true>, (const void*)cn_flags_kernel<false, true, true>};
      for (const void* fn : fns) {
        hipError_t e1 = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, LH_MAX_COLS * (int)sizeof(u64));
        if (e1 != hipSuccess) return (int)e1;
      }
      raised = true;
    }
  }
#define CN_FLAGS_ARGS(T2P, T2C)                                                                      \
  (const i64*)rowptrA, colA, (const i64*)rowptrT1, colT1, (const i64*)(T2P), (T2C),                   \
      (const unsigned*)bitmapT1, (i64)bm1_stride_words, (const unsigned*)bitmapT2, (i64)bm_stride_words, (const i64*)src, \
      (const i64*)dst, (const i64*)order, (i64)B, (i64)n_cols, (const i64*)off, flags, (i64)flags_cap, \
      (u64*)hist, cnt1, cnt2, status, (u64*)rec, gcost
#define CN_FLAGS_LAUNCH(T2, LHV, RI, T2P, T2C)                                                        \
  hipLaunchKernelGGL((cn_flags_kernel<T2, LHV, RI>), dim3(grid), dim3(OCN_BLOCK), (LHV) ? lds : 0, st, CN_FLAGS_ARGS(T2P, T2C))
#define CN_FLAGS_PICK(T2, T2P, T2C)                                                                   \
  do {                                                                                                \
    if (lh) { if (rec_in) CN_FLAGS_LAUNCH(T2, true, true, T2P, T2C); else CN_FLAGS_LAUNCH(T2, true, false, T2P, T2C); }   \
    else { if (rec_in) CN_FLAGS_LAUNCH(T2, false, true, T2P, T2C); else CN_FLAGS_LAUNCH(T2, false, false, T2P, T2C); }    \
  } while (0)
  if (!rowptrT2 && bitmapT2 && lh) return OCN_EINVAL;      // (small graphs read T2's row lengths beside its bit rows)
  if (rowptrT2 || bitmapT2) CN_FLAGS_PICK(true, rowptrT2, colT2);      // T2 by its bit rows alone: a product whose rows are built on demand
  else CN_FLAGS_PICK(false, nullptr, (const int32_t*)nullptr);
#undef CN_FLAGS_PICK
#undef CN_FLAGS_LAUNCH
  return launch_status();
}

int ocn_cn_flags(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT1,
                 const int32_t* colT1, const int64_t* rowptrT2, const int32_t* colT2,
                 const uint32_t* bitmapT1, int64_t bm1_stride_words, const uint32_t* bitmapT2, int64_t bm_stride_words,
                 const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                 int64_t n_cols, const int64_t* off, uint8_t* flags, int64_t flags_cap, uint64_t* hist,
                 int32_t* cnt1, int32_t* cnt2, int32_t* status, uint64_t* rec, int32_t* gcost, void* stream) {
  return cn_flags_launch(rowptrA, colA, rowptrT1, colT1, rowptrT2, colT2, bitmapT1, bm1_stride_words, bitmapT2, bm_stride_words,
                         src, dst, order, B, n_cols, off, flags, flags_cap, hist, cnt1, cnt2, status, rec, gcost, false, stream);
}

int ocn_cn_flags_rec(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT1,
                     const int32_t* colT1, const int64_t* rowptrT2, const int32_t* colT2,
                     const uint32_t* bitmapT1, int64_t bm1_stride_words, const uint32_t* bitmapT2, int64_t bm_stride_words,
                     const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                     int64_t n_cols, const int64_t* off, uint8_t* flags, int64_t flags_cap, uint64_t* hist,
                     int32_t* cnt1, int32_t* cnt2, int32_t* status, uint64_t* rec, int32_t* gcost, void* stream) {
  return cn_flags_launch(rowptrA, colA, rowptrT1, colT1, rowptrT2, colT2, bitmapT1, bm1_stride_words, bitmapT2, bm_stride_words,
                         src, dst, order, B, n_cols, off, flags, flags_cap, hist, cnt1, cnt2, status, rec, gcost, true, stream);
}

}  // extern "C"
