// The common-neighbour stage, K1 (pattern route): the intersection pass.  It leaves the flag bytes, the column histogram, the
// per-candidate counts and — for the pooling (cn_pool.hip) — the slot records (slot_rec.h) and the group costs (common.h).
// See include/ocn_hip.h for the reference call sites.
#include "slot_rec.h"

// (sorted_has, wave_lds_sync and the schedule constants: common.h)

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

// (wave_uniform: common.h)
// membership of key in a sorted row of at most 64 entries held one per lane (t = INT_MAX beyond its end): lower bound in
// six cross-lane reads and one more for the element itself.  Every lane of the wave must call it.
__device__ __forceinline__ bool lanes_have(int32_t t, int32_t key) {
  int pos = 0;
#pragma unroll
  for (int step = OCN_WAVE / 2; step > 0; step >>= 1)
    if (__shfl(t, pos + step - 1, OCN_WAVE) < key) pos += step;
  return __shfl(t, pos, OCN_WAVE) == key;
}

// NS: slots per wave.  1: as above.  2 (large graphs at large batches, cn_flags_launch): wave g of workgroup b owns the
// consecutive slots 8b + 2g and 8b + 2g + 1 and makes every trip for both at once — both records, both target rows, both
// chunks of N(src), both probes are issued before the first of them is waited for — so that a CU holds 64 slots in flight
// where its 32 waves held 32.  Slots are in source order: a pair mostly shares its source (one colA load serves both, and
// one histogram add carries both increments).  The pair shares the wave's LDS slices: a long target row takes the whole slice
// when the partner's row sits in registers (or needs none), its own half when it fits there, and is searched in memory
// otherwise.  A workgroup is then NS schedule groups (SCHED_GROUP slots = GPB / NS waves each).  Every output is what NS = 1
// writes.
// cover (wave-uniform): T2 is certified as the full pattern of A·A for a symmetric A (ocn_hip.h: ocn_cn_flags_cover).  A candidate
// (i, j) that is a stored entry of A then has every k of N(i) in T2 row j through the wedge j - i - k: the slot behaves as a
// full row does (t2_full) — no probe, no search, f2 = in.  Whether j is in N(i) is found beside loads the slot makes anyway: a
// source row of one chunk answers it with a ballot over the chunk just loaded; a longer one, up to COVER_MAX_ROW entries, with
// a two-level search of the sorted row (64 samples, then the one segment of at most 64) whose loads fly beside the record's
// follow-up and the target row's and are back before chunk 0's probes would go out.  Longer rows probe as without it.
#define COVER_MAX_ROW 4096
template <bool HAS_T2, bool LH, bool RECIN, int NS>
__global__ __launch_bounds__(OCN_BLOCK) void cn_flags_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrT1, const int32_t* __restrict__ colT1,
    const i64* __restrict__ rowptrT2, const int32_t* __restrict__ colT2,
    const unsigned* __restrict__ bmT1, i64 bm1_stride, const unsigned* __restrict__ bmT2, i64 bm_stride,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    i64 n_cols, const i64* __restrict__ off, uint8_t* __restrict__ flags, i64 cap,
    u64* __restrict__ hist, int32_t* __restrict__ cnt1, int32_t* __restrict__ cnt2,
    int32_t* __restrict__ status, u64* rec, int32_t* __restrict__ gcost, int cover) {
  constexpr int GPB = OCN_WPB, SPB = GPB * NS;                  // waves, slots per workgroup
  constexpr int T1_PART = T1_CAP / NS, T2_PART = OCN_WAVE / NS;  // a slot's share of its wave's slices when both slots need them
  static_assert(NS == 1 || (NS == 2 && !LH), "slot pairs: large-graph forms only");
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
  for (i64 e0 = (i64)blockIdx.x * SPB; e0 < B; e0 += (i64)gridDim.x * SPB, par ^= 1) {
    // Every per-slot quantity is an [NS] array, every loop over s fully unrolled; within a phase the loads of all slots are
    // issued before the first use.  A slot past the end of the batch (an odd tail) is an empty one: no separate path.
    i64 slot[NS];                             // processing slots; `order` maps one to a batch row
    bool act[NS];
    i64 e[NS], i[NS], j[NS], a0[NS], da[NS], b0[NS], db[NS], c0[NS], dc[NS], base[NS];
    const unsigned* bm_row[NS];               // bit row of dst in T2, when T2 comes with a dense bitmap
    const unsigned* bm1_row[NS];              // ... and in T1 (small dense graphs: a membership test is one probe)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      slot[s] = e0 + NS * g + s;
      act[s] = slot[s] < B;
      e[s] = i[s] = j[s] = a0[s] = da[s] = b0[s] = db[s] = c0[s] = dc[s] = base[s] = 0;
      bm_row[s] = bm1_row[s] = nullptr;
    }
    // NS > 1: the slots' records are consecutive: one lane-spread load for all of them, a field is read from its lane
    u64 recw = 0;
    if (RECIN && NS > 1) recw = rec_load_spread<NS>(rec, slot[0], B, gl);
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (act[s]) {
        if (RECIN) {
          u64 w[OCN_REC_WORDS];
          if (NS == 1) rec_load(rec, slot[s], w); else rec_spread_words(recw, s, w);
          // (field by field into scalar registers: unpacked into a struct first, the NS = 2 instances keep their instruction
          // count but not their schedule)
          e[s] = wave_uniform(rec_row(w));
          i[s] = wave_uniform(rec_src(w)); j[s] = wave_uniform(rec_dst(w));
          a0[s] = wave_uniform(rec_start(w)); da[s] = wave_uniform(rec_len(w));
          base[s] = wave_uniform(rec_base_started(w));
        } else {                              // (no records: small batches and training — a slot's chain runs on its own)
          e[s] = order ? order[slot[s]] : slot[s];
          i[s] = src[e[s]]; j[s] = dst[e[s]];
          a0[s] = rowptrA[i[s]]; da[s] = rowptrA[i[s] + 1] - a0[s];
          base[s] = off[e[s]];
        }
        if (bmT1) bm1_row[s] = bmT1 + j[s] * bm1_stride;
        else { b0[s] = rowptrT1[j[s]]; db[s] = rowptrT1[j[s] + 1] - b0[s]; }
        if (HAS_T2) {
          if (bmT2) bm_row[s] = bmT2 + j[s] * bm_stride;
          if (rowptrT2 && (LH || !bmT2)) { c0[s] = rowptrT2[j[s]]; dc[s] = rowptrT2[j[s] + 1] - c0[s]; }   // (small graphs with bit rows too: a FULL row — a dense A², ogbl-ddi —
                                                                                  // needs no probe at all; on large graphs the two loads would only lengthen the chain)
        }
        if (void_batch) { da[s] = 0; db[s] = 0; dc[s] = 0; base[s] = 0; }
      }
    // certified T2: the 64-point sample of a long source row, for the search of j in it (a pair of one source shares it)
    const bool same = NS > 1 && i[0] == i[NS - 1];   // one source (wave-uniform): one row of A, one chunk load, one histogram add
    bool seek[NS], skip2[NS];                 // j is looked for in the long row N(i); the slot's cn2 flags are known without T2
    int32_t smp[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      seek[s] = HAS_T2 && cover && da[s] > OCN_WAVE && da[s] <= COVER_MAX_ROW;
      smp[s] = 0x7fffffff;
      if (seek[s]) smp[s] = (s > 0 && same) ? smp[0] : colA[a0[s] + (((i64)gl * da[s]) >> 6)];
    }
    // the target row: up to 64 entries stay in the wave's registers, one per lane; a longer one, up to T1_CAP (NS = 2: while
    // the partner's sits in registers, else up to T1_PART in the slot's own part), goes to this wave's LDS slice; beyond that
    // the search runs in memory
    bool t1_reg[NS], t1_lds[NS], t2_full[NS], t2_lds[NS];
    int t1_at[NS], t2_at[NS];
    int32_t t1[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int o = (s + 1) % NS;             // the partner
      const bool whole1 = NS == 1 || db[o] <= OCN_WAVE;
      t1_reg[s] = db[s] <= OCN_WAVE; t1_lds[s] = db[s] <= (whole1 ? T1_CAP : T1_PART);
      t1_at[s] = whole1 ? 0 : s * T1_PART;
      t1[s] = 0x7fffffff;
      if (t1_reg[s]) { if (gl < db[s]) t1[s] = colT1[b0[s] + gl]; }
      else if (t1_lds[s])
        for (i64 q = gl; q < db[s]; q += OCN_WAVE) s_t1[g][t1_at[s] + q] = colT1[b0[s] + q];
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int o = (s + 1) % NS;
      t2_full[s] = HAS_T2 && rowptrT2 && dc[s] == n_cols;   // a full row (dense A², e.g. ddi) contains every column
      skip2[s] = t2_full[s];
      const bool whole2 = NS == 1 || (HAS_T2 && rowptrT2 && dc[o] == n_cols) || dc[o] == 0;
      t2_lds[s] = whole2 || dc[s] <= T2_PART;
      t2_at[s] = whole2 ? 0 : s * T2_PART;
      if (HAS_T2 && !t2_full[s] && !bmT2 && t2_lds[s]) {
        if (dc[s] > OCN_WAVE) s_t2[g][gl] = colT2[c0[s] + (((i64)gl * dc[s]) >> 6)];      // a 64-point sample of the long row (it has the whole slice)
        else if (gl < dc[s]) s_t2[g][t2_at[s] + gl] = colT2[c0[s] + gl];
      }
    }
    // ... and the one segment of the row that can hold j: samples <= j number the segment (the row is sorted, its sample
    // positions (l * da) >> 6 strictly ascending for da > 64), at most ceil(da / 64) <= 64 entries, inside the row
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (seek[s]) {
        const int nle = __popcll(__ballot(smp[s] <= (int32_t)j[s]));
        if (nle > 0) {
          const i64 q0 = ((i64)(nle - 1) * da[s]) >> 6, q1 = ((i64)nle * da[s]) >> 6;
          const int32_t v = q0 + gl < q1 ? colA[a0[s] + q0 + gl] : -1;
          skip2[s] = skip2[s] || __ballot(v == (int32_t)j[s]) != 0;
        }
      }
    wave_lds_sync();
    bool fits[NS];
    int c1[NS], c2[NS];
    i64 da_max = da[0];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      fits[s] = base[s] + da[s] <= cap;
      c1[s] = c2[s] = 0;
      if (s > 0 && da[s] > da_max) da_max = da[s];
    }
    for (i64 p0 = 0; p0 < da_max; p0 += OCN_WAVE) {      // (wave-uniform trips: lanes_have needs every lane)
      const i64 p = p0 + gl;
      bool in[NS], f1[NS], f2[NS];
      int32_t k[NS];
      unsigned w2[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        in[s] = p < da[s];
        if (s > 0 && same) k[s] = k[0];       // (unused where !in[s]: an empty partner of the same source id)
        else k[s] = in[s] ? colA[a0[s] + p] : 0;
      }
      if (HAS_T2 && cover && p0 == 0) {        // a source row of one chunk: is j in the chunk just loaded?
#pragma unroll
        for (int s = 0; s < NS; ++s)
          if (da[s] <= OCN_WAVE) skip2[s] = skip2[s] || __ballot(in[s] && k[s] == (int32_t)j[s]) != 0;
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        w2[s] = 0;
        if (HAS_T2 && bmT2 && !skip2[s] && in[s]) w2[s] = bm_row[s][k[s] >> 5];    // one probe, in flight while the cn1 search runs
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (bmT1) f1[s] = in[s] && ((bm1_row[s][k[s] >> 5] >> (k[s] & 31)) & 1u);
        else if (t1_reg[s]) f1[s] = lanes_have(t1[s], k[s]) && in[s];
        else f1[s] = in[s] && (t1_lds[s] ? sorted_has(&s_t1[g][t1_at[s]], db[s], k[s]) : sorted_has(colT1 + b0[s], db[s], k[s]));
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        f2[s] = false;
        if (HAS_T2 && in[s]) {
          if (skip2[s]) f2[s] = true;
          else if (bmT2) f2[s] = (w2[s] >> (k[s] & 31)) & 1u;
          else if (!t2_lds[s]) f2[s] = sorted_has(colT2 + c0[s], dc[s], k[s]);
          else f2[s] = dc[s] > OCN_WAVE ? sampled_has(&s_t2[g][0], colT2 + c0[s], dc[s], k[s]) : sorted_has(&s_t2[g][t2_at[s]], dc[s], k[s]);
        }
        if (fits[s] && in[s]) flags[base[s] + p] = (uint8_t)((f1[s] ? OCN_F_CN1 : 0u) | (f2[s] ? OCN_F_CN2 : 0u));
      }
      if (NS > 1 && same) {                   // k[s] == k[0]: the column's increments of all slots in one add
        u64 inc = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) inc += (u64)f1[s] | ((u64)f2[s] << HF_BITS) | ((u64)(f1[s] | f2[s]) << (2 * HF_BITS));
        if (inc) atomicAdd(hist + 2 * (i64)k[0], inc);
      } else {
#pragma unroll
        for (int s = 0; s < NS; ++s)
          if (f1[s] | f2[s]) {
            const u64 inc = (u64)f1[s] | ((u64)f2[s] << HF_BITS) | (1ull << (2 * HF_BITS));
            if (LH) atomicAdd(s_hist + k[s], inc); else atomicAdd(hist + 2 * (i64)k[s], inc);
          }
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        c1[s] += __popcll(__ballot(f1[s]));   // (wave-uniform counts)
        c2[s] += __popcll(__ballot(f2[s]));
      }
    }
    wave_lds_sync();                          // (the next slot's row may overwrite this one's)
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (act[s] && gl == 0) {
        cnt1[e[s]] = c1[s];
        if (cnt2) cnt2[e[s]] = c2[s];
        if (rec) {                              // what the pooling needs to know about this slot, in ONE 32-byte record
          u64* r = rec_at(rec, slot[s]);
          if (!RECIN) rec_pack_head(r, e[s], i[s], j[s], a0[s], da[s]);
          else if (void_batch) r[2] = rec_word2(a0[s], da[s]);      // (a started record's length is the real one)
          r[3] = rec_word3(base[s], da[s] > 0 && (i64)c2[s] == da[s], c1[s] > 0, c2[s] > 0);
        }
      }
    if (gcost) {
      // what each group of SCHED_GROUP consecutive slots will cost the pooling (entries to gather): the pooling visits its
      // groups longest first (ocn_gather_schedule), so that no straggler ends its kernel.  The one workgroup barrier of
      // an iteration, at its very end: s_cost alternates between two sets, so a wave that runs ahead into the next
      // iteration writes the other set and stops at that iteration's barrier, which thread 0 reaches after this read.
      // A wave folds its own slots first (SCHED_COST is associative), so s_cost stays one word per wave.
      int cost = act[0] ? c1[0] + c2[0] : 0;
#pragma unroll
      for (int s = 1; s < NS; ++s) cost = SCHED_COST(cost, act[s] ? c1[s] + c2[s] : 0);
      if (gl == 0) s_cost[par][g] = cost;
      __syncthreads();
      if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q)          // group q of this workgroup: waves q * GPB / NS ... (gcost has ceil(B / SCHED_GROUP) words)
          if (NS == 1 || e0 + q * SCHED_GROUP < B) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < GPB / NS; ++w) t = SCHED_COST(t, s_cost[par][q * (GPB / NS) + w]);
            gcost[e0 / SCHED_GROUP + q] = t;
          }
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

// Large-graph batches of at least this many candidates take the slot-pair form (NS = 2): B / 2 waves must still fill the
// chip's 8 192 wave slots several times over.  Process-wide; see ocn_hip.h.
static int64_t g_flags_pair_min_batch = 32768;

int64_t ocn_cn_flags_pair_min_batch(int64_t min_rows) {
  const int64_t prev = g_flags_pair_min_batch;
  if (min_rows >= 0) g_flags_pair_min_batch = min_rows;
  return prev;
}

// rec_in: the records come half written from ocn_order_by_node_finish_rec (ocn_cn_flags_rec)
static int cn_flags_launch(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT1,
                           const int32_t* colT1, const int64_t* rowptrT2, const int32_t* colT2,
                           const uint32_t* bitmapT1, int64_t bm1_stride_words, const uint32_t* bitmapT2, int64_t bm_stride_words,
                           const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                           int64_t n_cols, const int64_t* off, uint8_t* flags, int64_t flags_cap, uint64_t* hist,
                           int32_t* cnt1, int32_t* cnt2, int32_t* status, uint64_t* rec, int32_t* gcost, bool rec_in, bool cover, void* stream) {
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
  const bool pairs = !lh && B >= g_flags_pair_min_batch;      // two slots per wave (cn_flags_kernel: NS)
  const int spb = pairs ? 2 * GPB : GPB;
  const int grid = lh ? grid_for((B + GPB - 1) / GPB, 256 * 3) : grid_for((B + spb - 1) / spb);
  if (lh) {                                   // static (target rows) + dynamic (histogram) LDS can pass 64 KiB
    static bool raised_dev[64] = {};          // the attribute is per device (function objects are per device)
    int devid = 0;
    if (hipGetDevice(&devid) != hipSuccess || devid < 0 || devid >= 64) return OCN_EINVAL;
    bool& raised = raised_dev[devid];
    if (!raised) {
      const void* fns[4] = {(const void*)cn_flags_kernel<true, true, false, 1>, (const void*)cn_flags_kernel<false, true, false, 1>,
                            (const void*)cn_flags_kernel<true, true, true, 1>, (const void*)cn_flags_kernel<false, true, true, 1>};
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
      (u64*)hist, cnt1, cnt2, status, (u64*)rec, gcost, (int)cover
#define CN_FLAGS_LAUNCH(T2, LHV, RI, NSV, T2P, T2C)                                                   \
  hipLaunchKernelGGL((cn_flags_kernel<T2, LHV, RI, NSV>), dim3(grid), dim3(OCN_BLOCK), (LHV) ? lds : 0, st, CN_FLAGS_ARGS(T2P, T2C))
#define CN_FLAGS_PICK(T2, T2P, T2C)                                                                   \
  do {                                                                                                \
    if (lh) { if (rec_in) CN_FLAGS_LAUNCH(T2, true, true, 1, T2P, T2C); else CN_FLAGS_LAUNCH(T2, true, false, 1, T2P, T2C); }   \
    else if (pairs) { if (rec_in) CN_FLAGS_LAUNCH(T2, false, true, 2, T2P, T2C); else CN_FLAGS_LAUNCH(T2, false, false, 2, T2P, T2C); }   \
    else { if (rec_in) CN_FLAGS_LAUNCH(T2, false, true, 1, T2P, T2C); else CN_FLAGS_LAUNCH(T2, false, false, 1, T2P, T2C); }    \
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
                         src, dst, order, B, n_cols, off, flags, flags_cap, hist, cnt1, cnt2, status, rec, gcost, false, false, stream);
}

int ocn_cn_flags_rec(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT1,
                     const int32_t* colT1, const int64_t* rowptrT2, const int32_t* colT2,
                     const uint32_t* bitmapT1, int64_t bm1_stride_words, const uint32_t* bitmapT2, int64_t bm_stride_words,
                     const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                     int64_t n_cols, const int64_t* off, uint8_t* flags, int64_t flags_cap, uint64_t* hist,
                     int32_t* cnt1, int32_t* cnt2, int32_t* status, uint64_t* rec, int32_t* gcost, void* stream) {
  return cn_flags_launch(rowptrA, colA, rowptrT1, colT1, rowptrT2, colT2, bitmapT1, bm1_stride_words, bitmapT2, bm_stride_words,
                         src, dst, order, B, n_cols, off, flags, flags_cap, hist, cnt1, cnt2, status, rec, gcost, true, false, stream);
}

int ocn_cn_flags_cover(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrT1,
                       const int32_t* colT1, const int64_t* rowptrT2, const int32_t* colT2,
                       const uint32_t* bitmapT1, int64_t bm1_stride_words, const uint32_t* bitmapT2, int64_t bm_stride_words,
                       const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B,
                       int64_t n_cols, const int64_t* off, uint8_t* flags, int64_t flags_cap, uint64_t* hist,
                       int32_t* cnt1, int32_t* cnt2, int32_t* status, uint64_t* rec, int32_t* gcost, int32_t rec_in,
                       int32_t t2_cover, void* stream) {
  return cn_flags_launch(rowptrA, colA, rowptrT1, colT1, rowptrT2, colT2, bitmapT1, bm1_stride_words, bitmapT2, bm_stride_words,
                         src, dst, order, B, n_cols, off, flags, flags_cap, hist, cnt1, cnt2, status, rec, gcost, rec_in != 0,
                         t2_cover != 0 && (rowptrT2 || bitmapT2), stream);
}

}  // extern "C"
