// The common-neighbour stage, K3 forward: the pooling of cn5 / cn7 (packed, wave, long-row and generic forms) and the
// three-vector pooling of cn6.  The slot records it reads are the intersection pass's (cn_flags.hip), the visiting order
// cn_sched.hip's; slot_rec.h and common.h (sched_followed) fix them.  See include/ocn_hip.h for the reference call sites.
#include "lane_group.h"
#include "slot_rec.h"

// ---------------------------------------------------------------------------------------------
// K3: pooling — gather embedding rows over the flagged neighbours
// ---------------------------------------------------------------------------------------------
// (entry_weights: common.h)

// Pool the flagged neighbours at positions [p_begin, p_end) of the source row into acc1 / acc2, in
// ascending position (= column) order: the lane-group walk of lane_group.h.  LPE lanes cooperate; each lane owns NV
// float4 of the H = LPE*NV*4 features; four embedding rows are in flight per group.
constexpr int GATHER_UNR = 4;

// The accumulate step of one embedding row: the {xcn1, xcn2} pairs of a lane's four features take w * x, component by component
// in the order x, y, z, w (pool_range and the pair form share it).
__device__ __forceinline__ void axpy_pair4(f32x2 (&a)[4], const f32x2 w, const float x0, const float x1, const float x2,
                                           const float x3) {
  axpy_pair(a[0], w, x0);
  axpy_pair(a[1], w, x1);
  axpy_pair(a[2], w, x2);
  axpy_pair(a[3], w, x3);
}
// (eight for the one-wave-per-candidate layout of H >= 256 — one candidate's gathers are all a wave has in flight:
// 0.214 -> 0.206 ms at the collab shape; four where several candidates share a wave)
template <int LPE, int NV, int UNR = (LPE >= 64 ? 2 * GATHER_UNR : GATHER_UNR)>
__device__ __forceinline__ void pool_range(i64 p_begin, i64 p_end, i64 a0, i64 base, int gl, int gbase,
                                           const int32_t* __restrict__ colA, const uint8_t* __restrict__ flags,
                                           const int32_t* __restrict__ wc, const float4* __restrict__ weights,
                                           const float4* __restrict__ h4, i64 rowq, float4 (&acc1)[NV],
                                           float4 (&acc2)[NV], bool full2 = false) {
  // Narrow groups (small H) would otherwise pay one dependent load chain (column id -> column weights)
  // per LPE positions: a lane fetches PT positions per round, so a round always covers 64 of them
  // (hub rows of the ppa shape: 101 -> 40 us).
  constexpr int PT = lane_group<LPE>::PT;
  f32x2 acc[NV][4];                          // {acc1, acc2} component pairs: one packed multiply + add per pair
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    acc[v][0] = f32x2{acc1[v].x, acc2[v].x}; acc[v][1] = f32x2{acc1[v].y, acc2[v].y};
    acc[v][2] = f32x2{acc1[v].z, acc2[v].z}; acc[v][3] = f32x2{acc1[v].w, acc2[v].w};
  }
  for (i64 p0 = p_begin; p0 < p_end; p0 += LPE * PT) {
    int32_t k[PT];
    unsigned f[PT];
    int32_t cv[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      const i64 p = p0 + t * LPE + gl;
      k[t] = 0; f[t] = 0; cv[t] = 1;
      if (p < p_end) {
        k[t] = colA[a0 + p]; f[t] = flags[base + p];
        if (wc) cv[t] = wc[base + p];
      }
      if (full2) f[t] &= ~OCN_F_CN2;           // the whole row is cn2: its pooled vector is the row sum (rowsum), not summed here
    }
    float wa[PT], wb[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      wa[t] = wb[t] = 0.f;
      if (f[t]) entry_weights(f[t], weights[k[t]], (float)cv[t], wa[t], wb[t]);
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {             // ascending position order: tile t, then lane
      const bool need = (wa[t] != 0.f) | (wb[t] != 0.f);
      unsigned long long m = lane_group_mask<LPE>(need, gbase);
      while (m) {
        int bsel[UNR];
        lane_group_take(m, bsel);
        int32_t kk[UNR];
        float wwa[UNR], wwb[UNR];
        float4 x[UNR][NV];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int sl = lane_group_src(gbase, bsel[u]);
          kk[u] = __shfl(k[t], sl, OCN_WAVE);
          wwa[u] = __shfl(wa[t], sl, OCN_WAVE);
          wwb[u] = __shfl(wb[t], sl, OCN_WAVE);
          lane_group_row<LPE>(bsel[u], kk[u], h4, rowq, gl, x[u]);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          if (bsel[u] >= 0) {
            const f32x2 w = {wwa[u], wwb[u]};
#pragma unroll
            for (int v = 0; v < NV; ++v) axpy_pair4(acc[v], w, x[u][v].x, x[u][v].y, x[u][v].z, x[u][v].w);
          }
        }
      }
    }
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    acc1[v] = make_float4(acc[v][0].x, acc[v][1].x, acc[v][2].x, acc[v][3].x);
    acc2[v] = make_float4(acc[v][0].y, acc[v][1].y, acc[v][2].y, acc[v][3].y);
  }
}

// Source rows longer than this are pooled by a whole workgroup (cn_gather_long_kernel; a wave of cn_gather_wave_kernel for
// narrow embeddings in a large batch): its other lanes only FETCH the rows, one wave adds them in rank order.  So these
// rows, like the ones up to LONG_ROW, keep the strictly sequential ascending-column sum of the reference's spmm.
#define LONG_ROW 1024

// LPE lanes cooperate on one edge (64/LPE edges per wave).
template <int LPE, int NV>
__global__ __launch_bounds__(OCN_BLOCK) void cn_gather_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const i64* __restrict__ off, const uint8_t* __restrict__ flags, const int32_t* __restrict__ wc,
    const float4* __restrict__ weights, const float* __restrict__ h, int H,
    float* __restrict__ xcn1, float* __restrict__ xcn2, float* __restrict__ xij,
    const i64* __restrict__ out_row,     // out_row[batch row] = output row (class-major heads), or NULL
    const int32_t* __restrict__ cnt1, const int32_t* __restrict__ cnt2,     // per-row CN counts, or NULL
    const u64* __restrict__ rec,         // slot records of the intersection pass (then order/src/dst/off/cnt are not read), or NULL
    const int32_t* __restrict__ perm,    // ocn_gather_schedule's visiting order of the slot groups (longest first per XCD), or NULL
    const float* __restrict__ rowsum) {  // (A h)[i] rows for candidates whose whole source row is cn2 with weight 1 (ocn_hip.h), or NULL
  constexpr int GPW = lane_group<LPE>::GPW;
  const int lane = threadIdx.x & 63;       // (lane_group<LPE>'s gl, gbase and slot, written out: through the struct the narrow
  const int gl = lane % LPE;               // instances come out 9 - 15 instructions shorter, and no longer the measured ones)
  const int gbase = lane - gl;
  // Workgroups are dealt round-robin over the 8 XCDs (each with its own L2).  The batch rows are
  // visited in source-node order, so give every XCD one contiguous eighth of that order: rows
  // with neighbouring sources then share an L2 instead of being spread over all eight.
  // (One feature slice per XCD instead — every row slice with one home L2 — was bit-identical but 0.76 ms against 0.22 ms
  // at the collab shape: eight candidates share a wave and run in lockstep to the longest of them)
  i64 bid = blockIdx.x;
  if ((gridDim.x & 7) == 0) {             // (common.h's xcd_block(), written out: the schedule's lookup shares its test)
    bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);
    // ... and inside its eighth an XCD takes the groups in the order of the schedule: the longest jobs first (groups of
    // one source have one cost and stay neighbours: the L2 locality of the source order is kept)
    if (perm) bid = perm[bid];
  }
  const i64 slot = (bid * OCN_WPB + (threadIdx.x >> 6)) * GPW + lane / LPE;
  if (slot >= B) return;                    // whole group leaves together
  // One dependent load instead of three (order -> src / dst / off / counts -> rowptr) in front of the first gather:
  // the intersection pass left everything about this slot in a 32-byte record.
  i64 e, i, j, a0, da, base;
  bool has1, has2, full2;
  if (rec) {
    const slot_rec r = rec_read_finished(rec, slot);
    e = r.e; i = r.i; j = r.j; a0 = r.a0; da = r.da;
    base = r.base; has1 = r.has1; has2 = r.has2;
    full2 = rowsum && r.full2;
  } else {
    e = order ? order[slot] : slot;
    i = src[e]; j = dst[e];
    a0 = rowptrA[i]; da = rowptrA[i + 1] - a0;
    base = off[e];
    // a candidate without any CN entry (half of an evaluation batch) has nothing to pool; with class-major
    // output rows the heads never read its xcn1 / xcn2 rows (nor the xcn1 row of one without cn1 entries)
    has1 = !cnt1 || cnt1[e] > 0; has2 = !cnt2 || cnt2[e] > 0;
    full2 = rowsum && cnt2 && da > 0 && (i64)cnt2[e] == da;
  }
  if (da > LONG_ROW && !full2) return;      // cn_gather_long_kernel's (a hub row whose cn2 is the whole row only has its cn1 entries left)
  const float4* h4 = reinterpret_cast<const float4*>(h);
  const i64 rowq = H >> 2;                  // float4 per row
  float4 acc1[NV], acc2[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc1[v] = acc2[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (has1 | (has2 & !full2)) pool_range<LPE, NV>(0, da, a0, base, gl, gbase, colA, flags, wc, weights, h4, rowq, acc1, acc2, full2);
  if (full2) {
    const float4* rs = reinterpret_cast<const float4*>(rowsum) + i * rowq + gl;
#pragma unroll
    for (int v = 0; v < NV; ++v) acc2[v] = rs[v * LPE];
  }
  pool_store<LPE, NV>(out_row ? out_row[e] : e, i, j, gl, h4, rowq, acc1, acc2, xcn1, xcn2, xij,
                      !out_row || has1, !out_row || has1 || has2);
}

// lane l's float in every lane, as a scalar (l wave-uniform)
__device__ __forceinline__ float lane_f32(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// The pair form of cn_gather_kernel<64, 1> (H = 256, record-fed, pattern route without the row-sum shortcut; large batches:
// ocn_cn_gather_pair_min_batch): a wave owns TWO neighbouring slots of one schedule group and makes every trip to memory
// for both at once — one load of both records, both chunks of N(src) and of the flag bytes, both column-weight lookups,
// PAIR_UNR embedding rows per slot (eight per wave, the lone candidate's figure), both candidates' endpoint rows — so that a
// light candidate's chain of dependent trips is filled with its neighbour's.  Two HEAVY slots (more than PAIR_UNR live entries
// each in a round, more than eight in a shared source's union) take sixteen rows per trip: a trip is one round of latency, and
// at eight the pair made twice the trips of its heavier member alone and ended the launch as its straggler.
// A slot that has positions left beside one that has none walks on alone, eight rows wide.  A workgroup is two schedule groups: workgroup
// b of the XCD-contiguous order takes groups perm[2b] and perm[2b + 1] (2b and 2b + 1 without a schedule), wave w the slots
// 2(w & 1) and 2(w & 1) + 1 of group w >> 1.  Slots are in source order, so a pair mostly shares its source: the positions
// then coincide, the union of the two live masks is walked in ascending position, each row is loaded once and added into
// whichever of the two accumulator sets flagged it.  A slot that is finished, empty, past the batch's end or cn_gather_long_kernel's
// is skipped by wave-uniform branches; every load inside them is unconditional, from a clamped index, and its use is
// predicated (compiler lessons).  Each slot's sums are the strictly ascending-column sums of separately
// rounded products that the one-slot form makes: every output bit is the same.
constexpr int PAIR_UNR = 4;                  // embedding rows in flight per slot where both slots have some
template <int V> struct pair_const { static constexpr int value = V; };

// The index of a lane's column-weight lookup: its own column where it has an entry, else the column of the first lane that
// has one — a line the wave fetches anyway (lane 0's where none has: the loads are unconditional).
__device__ __forceinline__ int32_t pair_weight_index(unsigned f, int32_t k) {
  const unsigned long long any = __ballot(f != 0);
  const int32_t kd = __builtin_amdgcn_readlane(k, any ? __ffsll((long long)any) - 1 : 0);
  return f ? k : kd;
}
// a lane's entry weights (0, 0 without an entry) and the wave's mask of the entries to pool
__device__ __forceinline__ unsigned long long pair_live(unsigned f, const float4& cw, float& wa, float& wb) {
  float a = 0.f, b = 0.f;
  entry_weights(f, cw, 1.0f, a, b);
  wa = f ? a : 0.f; wb = f ? b : 0.f;
  return __ballot((wa != 0.f) | (wb != 0.f));
}
// the next W set bits of m, ascending (-1 past its last); the caller knows of at least LIVE
template <int W, int LIVE>
__device__ __forceinline__ void pair_take(unsigned long long& m, int (&sel)[W]) {
#pragma unroll
  for (int t = 0; t < W; ++t) {
    sel[t] = m ? (__ffsll((long long)m) - 1) : -1;
    if (t < LIVE) __builtin_assume(sel[t] >= 0);
    m &= m - 1;                              // no-op once m == 0
  }
}
// A trip is straight-line code — W requests, then the adds — in an instance per width, so that a light candidate's trip
// requests what it adds and nothing else (a request past the last entry, in the widest instances only, repeats the trip's
// first row, in flight already, and is not added).
// ... of one slot:
template <int W, int LIVE>
__device__ __forceinline__ void pair_trip_one(unsigned long long& m, int32_t k, float wa, float wb, const float4* __restrict__ h4,
                                              int lane, f32x2 (&acc)[4]) {
  int sel[W];
  pair_take<W, LIVE>(m, sel);
  float4 x[W];
#pragma unroll
  for (int t = 0; t < W; ++t) x[t] = h4[(i64)__builtin_amdgcn_readlane(k, sel[t] < 0 ? sel[0] : sel[t]) * OCN_WAVE + lane];
#pragma unroll
  for (int t = 0; t < W; ++t)                // (the entry's weights are read from its lane here, behind the requests)
    if (sel[t] >= 0) axpy_pair4(acc, f32x2{lane_f32(wa, sel[t]), lane_f32(wb, sel[t])}, x[t].x, x[t].y, x[t].z, x[t].w);
}
__device__ __forceinline__ void pair_rows_one(unsigned long long m, int32_t k, float wa, float wb, const float4* __restrict__ h4,
                                              int lane, f32x2 (&acc)[4]) {
  while (m) {
    const int c = __popcll(m);
    if (c > 4) pair_trip_one<2 * PAIR_UNR, 5>(m, k, wa, wb, h4, lane, acc);
    else if (c == 4) pair_trip_one<4, 4>(m, k, wa, wb, h4, lane, acc);
    else if (c == 3) pair_trip_one<3, 3>(m, k, wa, wb, h4, lane, acc);
    else if (c == 2) pair_trip_one<2, 2>(m, k, wa, wb, h4, lane, acc);
    else pair_trip_one<1, 1>(m, k, wa, wb, h4, lane, acc);
  }
}
// ... of two slots of one source: the union mu of their masks m0, m1; a row is loaded once and added where it is flagged
template <int W, int LIVE>
__device__ __forceinline__ void pair_trip_same(unsigned long long& mu, unsigned long long m0, unsigned long long m1, int32_t k,
                                               float wa0, float wb0, float wa1, float wb1, const float4* __restrict__ h4, int lane,
                                               f32x2 (&acc0)[4], f32x2 (&acc1)[4]) {
  int sel[W];
  pair_take<W, LIVE>(mu, sel);
  float4 x[W];
#pragma unroll
  for (int t = 0; t < W; ++t) x[t] = h4[(i64)__builtin_amdgcn_readlane(k, sel[t] < 0 ? sel[0] : sel[t]) * OCN_WAVE + lane];
#pragma unroll
  for (int t = 0; t < W; ++t)
    if (sel[t] >= 0) {
      if ((m0 >> sel[t]) & 1ull) axpy_pair4(acc0, f32x2{lane_f32(wa0, sel[t]), lane_f32(wb0, sel[t])}, x[t].x, x[t].y, x[t].z, x[t].w);
      if ((m1 >> sel[t]) & 1ull) axpy_pair4(acc1, f32x2{lane_f32(wa1, sel[t]), lane_f32(wb1, sel[t])}, x[t].x, x[t].y, x[t].z, x[t].w);
    }
}
// ... of two slots of two sources: W0 + W1 requests
template <int W0, int LIVE0, int W1, int LIVE1>
__device__ __forceinline__ void pair_trip_two(unsigned long long& m0, unsigned long long& m1, int32_t k0, int32_t k1, float wa0,
                                              float wb0, float wa1, float wb1, const float4* __restrict__ h4, int lane,
                                              f32x2 (&acc0)[4], f32x2 (&acc1)[4]) {
  int s0[W0], s1[W1];
  pair_take<W0, LIVE0>(m0, s0);
  pair_take<W1, LIVE1>(m1, s1);
  float4 x0[W0], x1[W1];
#pragma unroll
  for (int t = 0; t < W0; ++t) x0[t] = h4[(i64)__builtin_amdgcn_readlane(k0, s0[t] < 0 ? s0[0] : s0[t]) * OCN_WAVE + lane];
#pragma unroll
  for (int t = 0; t < W1; ++t) x1[t] = h4[(i64)__builtin_amdgcn_readlane(k1, s1[t] < 0 ? s1[0] : s1[t]) * OCN_WAVE + lane];
#pragma unroll
  for (int t = 0; t < W0; ++t)
    if (s0[t] >= 0) axpy_pair4(acc0, f32x2{lane_f32(wa0, s0[t]), lane_f32(wb0, s0[t])}, x0[t].x, x0[t].y, x0[t].z, x0[t].w);
#pragma unroll
  for (int t = 0; t < W1; ++t)
    if (s1[t] >= 0) axpy_pair4(acc1, f32x2{lane_f32(wa1, s1[t]), lane_f32(wb1, s1[t])}, x1[t].x, x1[t].y, x1[t].z, x1[t].w);
}
template <int W0, int LIVE0>
__device__ __forceinline__ void pair_trip_two_pick(unsigned long long& m0, unsigned long long& m1, int32_t k0, int32_t k1,
                                                   float wa0, float wb0, float wa1, float wb1, const float4* __restrict__ h4,
                                                   int lane, f32x2 (&acc0)[4], f32x2 (&acc1)[4]) {
  const int c = __popcll(m1);
  if (c > 2) pair_trip_two<W0, LIVE0, PAIR_UNR, 3>(m0, m1, k0, k1, wa0, wb0, wa1, wb1, h4, lane, acc0, acc1);
  else if (c == 2) pair_trip_two<W0, LIVE0, 2, 2>(m0, m1, k0, k1, wa0, wb0, wa1, wb1, h4, lane, acc0, acc1);
  else pair_trip_two<W0, LIVE0, 1, 1>(m0, m1, k0, k1, wa0, wb0, wa1, wb1, h4, lane, acc0, acc1);
}

__global__ __launch_bounds__(OCN_BLOCK) void cn_gather_pair_kernel(
    const int32_t* __restrict__ colA, i64 B, const uint8_t* __restrict__ flags, const float4* __restrict__ weights,
    const float* __restrict__ h, float* __restrict__ xcn1, float* __restrict__ xcn2, float* __restrict__ xij,
    const i64* __restrict__ out_row, const u64* __restrict__ rec, const int32_t* __restrict__ perm) {
  constexpr int NS = 2;
  constexpr i64 rowq = OCN_WAVE;             // float4 per row: one per lane
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  i64 bid = blockIdx.x;
  if ((gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);      // (xcd_block(): an XCD's eighth of the pairs of groups)
  i64 grp = 2 * bid + (w >> 1);
  if (perm) grp = perm[grp];                 // (the launch passes a schedule only where an eighth is whole pairs of groups)
  const i64 slot0 = grp * SCHED_GROUP + 2 * (w & 1);
  if (slot0 >= B) return;                    // whole wave leaves together
  // both records in one load: lane l holds word l of the eight.  (slot_rec.h's rec_load_spread<NS>, then per slot
  // rec_unpack_finished, restated: through the former this kernel comes out 2 instructions longer, through the latter — or
  // through the per-field functions — 28, and is no longer the measured one.  Every constant is slot_rec.h's.)
  u64 recw = 0;
  if (lane < OCN_REC_WORDS * NS && slot0 + (lane >> 2) < B) recw = rec[OCN_REC_WORDS * slot0 + lane];
  // A slot that takes no part (past the batch's end, or a row of cn_gather_long_kernel's, which writes all three output
  // rows) keeps zeros: the endpoint rows loaded for it below are row 0's and are never stored.
  i64 e[NS], i[NS], j[NS], a0[NS], base[NS], n[NS];
  bool live[NS], has1[NS], has2[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    u64 q[OCN_REC_WORDS];
    rec_spread_words(recw, s, q);
    const i64 da = (i64)(q[2] >> OCN_REC_LEN_SHIFT);
    live[s] = slot0 + s < B && da <= LONG_ROW;
    e[s] = live[s] ? (i64)q[0] : 0;
    i[s] = live[s] ? (i64)(q[1] & 0xffffffffull) : 0; j[s] = live[s] ? (i64)(q[1] >> 32) : 0;
    a0[s] = (i64)(q[2] & REC_LEN_MASK);
    base[s] = (i64)(q[3] & REC_BASE_MASK); has1[s] = (q[3] >> OCN_REC_HAS1_BIT) & 1ull; has2[s] = q[3] >> OCN_REC_HAS2_BIT;
    n[s] = live[s] && (has1[s] | has2[s]) ? da : 0;       // positions to walk: none for a candidate without CN entries
  }
  const bool same = live[0] && live[1] && i[0] == i[1];   // one source: one row of A (its start and length agree)
  const float4* h4 = reinterpret_cast<const float4*>(h);
  f32x2 acc[NS][4];                          // {acc1, acc2} component pairs of the lane's four features
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[s][c] = f32x2{0.f, 0.f};
  // A round of 64 positions comes in an instance per case — both slots have positions left (one source / two sources), or
  // one of them has — picked by wave-uniform tests, so that each instance is straight-line code down to the rows' trips and
  // every load in it is unconditional: a lane past the row's end reads the last position and its flag byte is dropped.
  auto round_two = [&](auto one_source, const i64 p0) {
    constexpr bool SAME = decltype(one_source)::value != 0;
    const i64 p = p0 + lane;
    int32_t k[NS];
    unsigned f[NS];
    k[0] = colA[a0[0] + (p < n[0] ? p : n[0] - 1)];
    k[1] = k[0];
    if (!SAME) k[1] = colA[a0[1] + (p < n[1] ? p : n[1] - 1)];
#pragma unroll
    for (int s = 0; s < NS; ++s) f[s] = flags[base[s] + (p < n[s] ? p : n[s] - 1)];
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (p >= n[s]) f[s] = 0;
    int32_t wi[NS] = {pair_weight_index(SAME ? (f[0] | f[1]) : f[0], k[0]), SAME ? 0 : pair_weight_index(f[1], k[1])};
    asm volatile("" : "+v"(wi[0]), "+v"(wi[1]));      // both indices before the first lookup: left alone, the compiler forms the second
                                                      // in the first one's unused w register and waits for that load to do so
    float4 cw[NS];
    cw[0] = weights[wi[0]];
    cw[1] = cw[0];
    if (!SAME) cw[1] = weights[wi[1]];
    float wa[NS], wb[NS];
    unsigned long long m[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) m[s] = pair_live(f[s], cw[s], wa[s], wb[s]);
#define PAIR_SAME_TRIP(W, LIVE) pair_trip_same<W, LIVE>(mu, m[0], m[1], k[0], wa[0], wb[0], wa[1], wb[1], h4, lane, acc[0], acc[1])
#define PAIR_TWO_TRIP(W, LIVE) pair_trip_two_pick<W, LIVE>(m[0], m[1], k[0], k[1], wa[0], wb[0], wa[1], wb[1], h4, lane, acc[0], acc[1])
    if constexpr (SAME) {
      unsigned long long mu = m[0] | m[1];   // the union of the live positions, ascending
      while (mu) {
        const int c = __popcll(mu);
        if (c > 8) PAIR_SAME_TRIP(4 * PAIR_UNR, 9);          // a heavy pair: as many trips as one heavy candidate alone makes
        else if (c > 4) PAIR_SAME_TRIP(2 * PAIR_UNR, 5);
        else if (c == 4) PAIR_SAME_TRIP(4, 4);
        else if (c == 3) PAIR_SAME_TRIP(3, 3);
        else if (c == 2) PAIR_SAME_TRIP(2, 2);
        else PAIR_SAME_TRIP(1, 1);
      }
    } else {
      while (m[0] && m[1]) {
        const int c = __popcll(m[0]);
        if (c > 4 && __popcll(m[1]) > 4)                      // a heavy pair: as many trips as one heavy candidate alone makes
          pair_trip_two<2 * PAIR_UNR, 5, 2 * PAIR_UNR, 5>(m[0], m[1], k[0], k[1], wa[0], wb[0], wa[1], wb[1], h4, lane, acc[0], acc[1]);
        else if (c > 2) PAIR_TWO_TRIP(PAIR_UNR, 3);
        else if (c == 2) PAIR_TWO_TRIP(2, 2);
        else PAIR_TWO_TRIP(1, 1);
      }
      pair_rows_one(m[0], k[0], wa[0], wb[0], h4, lane, acc[0]);      // what one slot has beyond the other: on its own, eight wide
      pair_rows_one(m[1], k[1], wa[1], wb[1], h4, lane, acc[1]);
    }
#undef PAIR_SAME_TRIP
#undef PAIR_TWO_TRIP
  };
  auto round_one = [&](auto which, const i64 p0) {
    constexpr int S = decltype(which)::value;
    const i64 p = p0 + lane;
    const int32_t k = colA[a0[S] + (p < n[S] ? p : n[S] - 1)];
    unsigned f = flags[base[S] + (p < n[S] ? p : n[S] - 1)];
    if (p >= n[S]) f = 0;
    const float4 cw = weights[pair_weight_index(f, k)];
    float wa, wb;
    const unsigned long long m = pair_live(f, cw, wa, wb);
    pair_rows_one(m, k, wa, wb, h4, lane, acc[S]);
  };
  const i64 n_max = n[0] > n[1] ? n[0] : n[1];
  for (i64 p0 = 0; p0 < n_max; p0 += OCN_WAVE) {
    const bool on0 = p0 < n[0], on1 = p0 < n[1];
    if (on0 && on1) {
      if (same) round_two(pair_const<1>{}, p0);
      else round_two(pair_const<0>{}, p0);
    } else if (on0) round_one(pair_const<0>{}, p0);
    else round_one(pair_const<1>{}, p0);
  }
  // both output rows and the endpoint rows, then the stores
  i64 oe[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) oe[s] = out_row ? out_row[e[s]] : e[s];
  float4 xi[NS], xj[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) { xi[s] = h4[i[s] * rowq + lane]; xj[s] = h4[j[s] * rowq + lane]; }      // (one source: its row twice, one line)
#pragma unroll
  for (int s = 0; s < NS; ++s)
    if (live[s])
      pool_emit(reinterpret_cast<float4*>(xcn1) + oe[s] * rowq + lane, reinterpret_cast<float4*>(xcn2) + oe[s] * rowq + lane,
                reinterpret_cast<float4*>(xij) + oe[s] * rowq + lane,
                make_float4(acc[s][0].x, acc[s][1].x, acc[s][2].x, acc[s][3].x),
                make_float4(acc[s][0].y, acc[s][1].y, acc[s][2].y, acc[s][3].y), xi[s], xj[s], !out_row || has1[s],
                !out_row || has1[s] || has2[s]);
}

// The sequential sum of ranks [0, nr) of a compacted round: acc += w[r] * x[r], one multiply and one add per entry and
// accumulator, in rank order.  Eight entries' operands are read from LDS ahead of their adds — a rolled loop would pay
// the LDS latency once per entry (the hub rows of the citation2 shape: 0.45 ms -> see DESIGN.md).
template <int FPL, int HF>
__device__ __forceinline__ void chain_rows(const float2* __restrict__ w, const float* __restrict__ xs, int nr,
                                           float (&acc1)[FPL], float (&acc2)[FPL]) {
  constexpr int BLK = FPL >= 4 ? 2 : 8 / FPL;       // entries per block: 2 * BLK * FPL operand registers per lane
  f32x2 acc[FPL];
#pragma unroll
  for (int q = 0; q < FPL; ++q) acc[q] = f32x2{acc1[q], acc2[q]};
  auto load = [&](int r, float2 (&w8)[BLK], float (&x8)[BLK][FPL]) {
#pragma unroll
    for (int u = 0; u < BLK; ++u) {
      w8[u] = w[r + u];
#pragma unroll
      for (int q = 0; q < FPL; ++q) x8[u][q] = xs[(r + u) * HF + q];
    }
  };
  auto add = [&](const float2 (&w8)[BLK], const float (&x8)[BLK][FPL]) {
#pragma unroll
    for (int u = 0; u < BLK; ++u)
#pragma unroll
      for (int q = 0; q < FPL; ++q) axpy_pair_lds(acc[q], f32x2{w8[u].x, w8[u].y}, x8[u][q]);
  };
  const int nb = nr / BLK;                   // blocks of BLK entries, two register sets: block b + 1 is read while b is added
  if (nb > 0) {
    float2 wa[BLK], wb[BLK];
    float xa[BLK][FPL], xb[BLK][FPL];
    load(0, wa, xa);
    int b = 0;
    for (; b + 2 <= nb; b += 2) {
      load((b + 1) * BLK, wb, xb);
      add(wa, xa);
      if (b + 2 < nb) load((b + 2) * BLK, wa, xa);
      add(wb, xb);
    }
    if (b < nb) add(wa, xa);
  }
  for (int r = nb * BLK; r < nr; ++r) {
    const float2 wr = w[r];
#pragma unroll
    for (int q = 0; q < FPL; ++q) axpy_pair_lds(acc[q], f32x2{wr.x, wr.y}, xs[r * HF + q]);
  }
#pragma unroll
  for (int q = 0; q < FPL; ++q) { acc1[q] = acc[q].x; acc2[q] = acc[q].y; }
}

// Small batches of narrow embeddings (ppa / citation2: B = 2048, H = 32..64) leave the packed kernel
// above with a few hundred waves, each lane group walking its row 4 gathers at a time.  Here ONE WAVE
// takes one batch row: per round of 64 positions the live entries are compacted (rank = position among
// the live ones), the 64/LPE lane groups fetch all their embedding rows at once (up to 64 gathers in
// flight per wave) into the wave's LDS slab, and lane group 0 accumulates them in rank order — the
// same sequential ascending-column fp32 sum as the packed kernel, bit for bit.
// LONG: the same kernel over the batch rows whose source row is LONGER than LONG_ROW only (large batches of narrow
// embeddings on a dense graph — ogbl-ddi: a third of the candidates have such a source; a lane group of the packed
// kernel would walk 2 000 positions four gathers at a time).
// (waves per workgroup: the slabs of four waves at H = 64 would be 70 KiB of static LDS, above the 64 KiB a workgroup gets without
// an opt-in; two waves there.  The wrong H = 64 sums beside another stream's kernels were not the slab — halving it left their rate
// unchanged — but the packed multiply-add form that axpy_pair_lds replaces: DESIGN.md section 6)
template <int LPE, int NV, bool LONG>
constexpr int gather_wave_wpb() { return LONG ? 1 : ((size_t)OCN_WPB * OCN_WAVE * (LPE * NV * 16 + 24) > 65536 ? 2 : OCN_WPB); }

template <int LPE, int NV, bool LONG = false, int WPB = gather_wave_wpb<LPE, NV, LONG>()>
__global__ __launch_bounds__(WPB * OCN_WAVE) void cn_gather_wave_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const i64* __restrict__ off, const uint8_t* __restrict__ flags, const int32_t* __restrict__ wc,
    const float4* __restrict__ weights, const float* __restrict__ h, int H,
    float* __restrict__ xcn1, float* __restrict__ xcn2, float* __restrict__ xij,
    const i64* __restrict__ out_row,     // out_row[batch row] = output row (class-major heads), or NULL
    const int32_t* __restrict__ cnt2, const float* __restrict__ rowsum) {   // see cn_gather_kernel
  // WPB waves per workgroup: ONE for the LONG pass — most batch rows are not its and leave at once, and a wave that
  // has left frees its LDS slab only when it is a workgroup of its own.
  constexpr int G = OCN_WAVE / LPE;
  constexpr int UNR = LPE;                  // G * UNR = 64 rows: a whole round in flight
  constexpr int HF = LPE * NV * 4;          // features: lane l < HF accumulates feature l (all lanes busy at H = 64,
  static_assert(HF <= OCN_WAVE, "");        // a quarter of the VALU work per entry of a float4-per-lane layout)
  __shared__ float4 s_x[WPB][OCN_WAVE][LPE * NV];
  __shared__ int32_t s_k[WPB][2][OCN_WAVE];
  __shared__ float2 s_w[WPB][2][OCN_WAVE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gl = lane % LPE, g = lane / LPE;
  const i64 slot = (i64)blockIdx.x * WPB + wv;
  if (slot >= B) return;                    // whole wave leaves together (no workgroup barriers below)
  const i64 e = order ? order[slot] : slot;
  const i64 i = src[e], j = dst[e];
  const i64 a0 = rowptrA[i], da = rowptrA[i + 1] - a0;
  const bool full2 = rowsum && cnt2 && da > 0 && (i64)cnt2[e] == da;
  if (LONG ? (da <= LONG_ROW || full2) : (da > LONG_ROW && !full2)) return;       // the other launch's rows
  const i64 base = off[e];
  const float4* h4 = reinterpret_cast<const float4*>(h);
  const i64 rowq = H >> 2;
  float acc1[1] = {0.f}, acc2[1] = {0.f};
  // Software pipeline over the 64-position rounds: a round needs column id -> column weights -> rows, three dependent
  // trips to memory, then the sequential sum.  The ids of round r+2 and the weights of round r+1 are requested before
  // round r's rows are; round r+1 is compacted and its rows requested (into registers) before round r is summed.
  int32_t k_n = 0, k_nn = 0, cv_n = 1, cv_nn = 1;
  unsigned f_n = 0, f_nn = 0;
  const unsigned fmask = full2 ? ~OCN_F_CN2 : ~0u;          // (full2: the row's cn2 pool is rowsum[i])
  if (lane < da) { k_n = colA[a0 + lane]; f_n = flags[base + lane] & fmask; if (wc) cv_n = wc[base + lane]; }
  if (OCN_WAVE + lane < da) {
    k_nn = colA[a0 + OCN_WAVE + lane]; f_nn = flags[base + OCN_WAVE + lane] & fmask;
    if (wc) cv_nn = wc[base + OCN_WAVE + lane];
  }
  float4 w_n = make_float4(0.f, 0.f, 0.f, 0.f);
  if (f_n) w_n = weights[k_n];
  f32x4 x[UNR][NV];
  // compact the round at positions [p0, p0 + 64) into half `b` of s_k / s_w (rank = position among the live entries),
  // advance the id / weight prefetch, request the round's rows; returns its number of live entries
  auto stage = [&](i64 p0, int b) -> int {
    const int32_t k = k_n, cv = cv_n;
    const unsigned f = f_n;
    const float4 wk = w_n;
    k_n = k_nn; f_n = f_nn; cv_n = cv_nn;
    w_n = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f_n) w_n = weights[k_n];
    k_nn = 0; f_nn = 0; cv_nn = 1;
    if (p0 + 2 * OCN_WAVE + lane < da) {
      k_nn = colA[a0 + p0 + 2 * OCN_WAVE + lane]; f_nn = flags[base + p0 + 2 * OCN_WAVE + lane] & fmask;
      if (wc) cv_nn = wc[base + p0 + 2 * OCN_WAVE + lane];
    }
    float wa = 0.f, wb = 0.f;
    if (f) entry_weights(f, wk, (float)cv, wa, wb);
    const bool need = (wa != 0.f) | (wb != 0.f);
    const unsigned long long m = __ballot(need);
    const int n = __popcll(m);
    if (need) {
      const int rank = __popcll(m & ((1ull << lane) - 1ull));
      s_k[wv][b][rank] = k;
      s_w[wv][b][rank] = make_float2(wa, wb);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int u = 0; u < UNR; ++u) {          // unconditional loads (a predicated one is followed by a wait for it): ranks past
      const int r = u * G + g;               // the last live entry read row 0 and are never stored
      const int32_t kr = r < n ? s_k[wv][b][r] : 0;
      const f32x4* row = reinterpret_cast<const f32x4*>(h4 + (i64)kr * rowq + gl);
#pragma unroll
      for (int v = 0; v < NV; ++v) x[u][v] = row[v * LPE];
    }
    return n;
  };
  int n = stage(0, 0);
  int b = 0;
  for (i64 p0 = 0; p0 < da; p0 += OCN_WAVE, b ^= 1) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {          // the rows requested a round ago -> this wave's slab
      const int r = u * G + g;
      if (r < n) {
#pragma unroll
        for (int v = 0; v < NV; ++v) *reinterpret_cast<f32x4*>(&s_x[wv][r][gl + v * LPE]) = x[u][v];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int n_next = p0 + OCN_WAVE < da ? stage(p0 + OCN_WAVE, b ^ 1) : 0;
    if (lane < HF)                           // rank order = ascending column, one feature per lane
      chain_rows<1, HF>(&s_w[wv][b][0], reinterpret_cast<const float*>(&s_x[wv][0][0]) + lane, n, acc1, acc2);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    n = n_next;
  }
  if (lane < HF) {
    const i64 o = (out_row ? out_row[e] : e) * H + lane;
    xcn1[o] = acc1[0];
    xcn2[o] = full2 ? rowsum[i * H + lane] : acc2[0];
    xij[o] = __fmul_rn(h[i * H + lane], h[j * H + lane]);
  }
}

// cn_gather_long_kernel's fetching lane groups: request the rows of sub-round u into registers / store them into a slab
// half.  The loads are unconditional (a predicated load is followed by a wait for it): slots past the sub-round's rows
// read row 0 and are never stored.
template <int LPE, int NV, int RPG, int FG, int SLAB>
__device__ __forceinline__ void long_request(f32x4 (&x)[RPG][NV], const int32_t* __restrict__ s_k, int u, int n, int fg,
                                             int gl, const float4* __restrict__ h4, i64 rowq) {
  const int r0 = u * SLAB;
  const int nr = n - r0;                                        // <= 0 past the last sub-round
#pragma unroll
  for (int q = 0; q < RPG; ++q) {
    const int r = fg + q * FG;
    const bool ok = r < SLAB && r < nr;
    const int32_t kr = s_k[ok ? r0 + r : 0];
    const f32x4* row = reinterpret_cast<const f32x4*>(h4 + (i64)(ok ? kr : 0) * rowq + gl);
#pragma unroll
    for (int v = 0; v < NV; ++v) x[q][v] = row[v * LPE];
  }
}

template <int LPE, int NV, int RPG, int FG, int SLAB>
__device__ __forceinline__ void long_store(const f32x4 (&x)[RPG][NV], float4* __restrict__ half, int nr, int fg, int gl) {
#pragma unroll
  for (int q = 0; q < RPG; ++q) {
    const int r = fg + q * FG;
    if (r < SLAB && r < nr) {
#pragma unroll
      for (int v = 0; v < NV; ++v) *reinterpret_cast<f32x4*>(half + r * (LPE * NV) + gl + v * LPE) = x[q][v];
    }
  }
}

// One workgroup per batch row whose source row is longer than LONG_ROW (hub sources; 8 403 neighbours at the citation2
// shape).  The sum stays the reference's: strictly sequential in ascending column order.  What a workgroup adds is
// the memory parallelism: per round of LONG_THREADS positions the live entries are compacted by rank; waves 1.. fetch
// their embedding rows into one half of a double-buffered LDS slab while wave 0 accumulates the other half in rank
// order — bit for bit the sum cn_gather_kernel forms for a short row.  The fetch is itself pipelined: a step writes
// the rows requested two steps earlier into the slab and requests a later sub-round's into the registers they
// leave, so a barrier never waits for a load issued in its own step.  Wave 0 holds the H features spread over its
// lanes (one per lane at H <= 64, H/64 from there): the sequential chain costs a multiply and an add per lane and
// entry and accumulator, not a float4's worth of them on a quarter of the lanes.
// LONG_THREADS: 1024 for small batches (few hub rows, each as parallel as a workgroup gets), 256 for large ones (one
// workgroup is launched per batch row and all but the hub rows' leave at once).
constexpr int LONG_SMALL_THREADS = 1024;   /* hub-row workgroup of a small batch (B <= 4096); 512 (two per CU) measured 5 % slower */
#define LONG_SLAB_BYTES(threads) ((threads) >= 512 ? 32768 : 16384)   /* per half; dynamic LDS = two halves */
template <int LPE, int NV, int LONG_THREADS>
__global__ __launch_bounds__(LONG_THREADS) void cn_gather_long_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ src, const i64* __restrict__ dst, i64 B,
    const i64* __restrict__ off, const uint8_t* __restrict__ flags, const int32_t* __restrict__ wc,
    const float4* __restrict__ weights, const float* __restrict__ h, int H,
    float* __restrict__ xcn1, float* __restrict__ xcn2, float* __restrict__ xij,
    const i64* __restrict__ out_row,     // out_row[batch row] = output row (class-major heads), or NULL
    const int32_t* __restrict__ cnt2, const float* __restrict__ rowsum) {   // see cn_gather_kernel
  constexpr int FG = (LONG_THREADS - OCN_WAVE) / LPE;          // fetching lane groups (waves 1..)
  constexpr int ROWQ = LPE * NV;                               // float4 per embedding row
  constexpr int HF = ROWQ * 4;                                 // features
  constexpr int FPL = HF >= OCN_WAVE ? HF / OCN_WAVE : 1;      // features per lane of wave 0
  constexpr int AL = HF / FPL;                                 // its active lanes
  constexpr int SLAB = LONG_SLAB_BYTES(LONG_THREADS) / (16 * ROWQ);   // rows per sub-round
  constexpr int RPG = (SLAB + FG - 1) / FG;                    // rows a fetching lane group requests per sub-round
  constexpr int WAVES = LONG_THREADS / OCN_WAVE;
  static_assert(FG >= 1 && SLAB >= 1, "");
  extern __shared__ __attribute__((aligned(16))) float4 s_x[];          // [2][SLAB][ROWQ]
  __shared__ int32_t s_k[LONG_THREADS];
  __shared__ float2 s_w[LONG_THREADS];
  __shared__ int s_wcnt[WAVES];
  const i64 e = blockIdx.x;
  const i64 i = src[e], j = dst[e];
  const i64 a0 = rowptrA[i], da = rowptrA[i + 1] - a0;
  if (da <= LONG_ROW) return;               // whole workgroup leaves together
  if (rowsum && cnt2 && (i64)cnt2[e] == da) return;            // ... also for a row pooled from rowsum by the other launch
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gl = threadIdx.x % LPE, fg = ((int)threadIdx.x - OCN_WAVE) / LPE;
  const i64 base = off[e];
  const float4* h4 = reinterpret_cast<const float4*>(h);
  const i64 rowq = H >> 2;
  float acc1[FPL], acc2[FPL];
#pragma unroll
  for (int q = 0; q < FPL; ++q) acc1[q] = acc2[q] = 0.f;
  for (i64 p0 = 0; p0 < da; p0 += LONG_THREADS) {
    const i64 p = p0 + threadIdx.x;
    int32_t k = 0, cv = 1;
    unsigned f = 0;
    if (p < da) { k = colA[a0 + p]; f = flags[base + p]; if (wc) cv = wc[base + p]; }
    float wa = 0.f, wb = 0.f;
    if (f) entry_weights(f, weights[k], (float)cv, wa, wb);
    const bool need = (wa != 0.f) | (wb != 0.f);
    const unsigned long long m = __ballot(need);
    if (lane == 0) s_wcnt[wv] = __popcll(m);
    __syncthreads();
    int before = 0, n = 0;
#pragma unroll
    for (int q = 0; q < WAVES; ++q) {
      const int c = s_wcnt[q];
      if (q < wv) before += c;
      n += c;
    }
    if (need) {                               // compaction by rank: ascending position = ascending column
      const int rank = before + __popcll(m & ((1ull << lane) - 1ull));
      s_k[rank] = k;
      s_w[rank] = make_float2(wa, wb);
    }
    __syncthreads();
    const int nsr = (n + SLAB - 1) / SLAB;
    // Sub-round u lives in register set u & 1 of the fetching waves from its request until it is stored two steps
    // later.  Step t: waves 1.. store sub-round t + 1 and request t + 3 into the set it leaves; wave 0 sums sub-round t
    // from the slab half t & 1; barrier.
    f32x4 xa[RPG][NV], xb[RPG][NV];
    if (wv > 0) {
      long_request<LPE, NV, RPG, FG, SLAB>(xa, s_k, 0, n, fg, gl, h4, rowq);
      long_request<LPE, NV, RPG, FG, SLAB>(xb, s_k, 1, n, fg, gl, h4, rowq);
    }
    for (int t = -1; t < nsr; t += 2) {
      // t + 1 is even: set a
      if (wv > 0) {
        long_store<LPE, NV, RPG, FG, SLAB>(xa, s_x + (size_t)((t + 1) & 1) * SLAB * ROWQ, n - (t + 1) * SLAB, fg, gl);
        long_request<LPE, NV, RPG, FG, SLAB>(xa, s_k, t + 3, n, fg, gl, h4, rowq);
      } else if (t >= 0 && lane < AL) {
        const int r0 = t * SLAB;
        chain_rows<FPL, HF>(s_w + r0, reinterpret_cast<const float*>(s_x + (size_t)(t & 1) * SLAB * ROWQ) + lane * FPL,
                            n - r0 < SLAB ? n - r0 : SLAB, acc1, acc2);
      }
      __syncthreads();
      if (t + 1 < nsr) {                                        // uniform: every thread takes the same barriers
        if (wv > 0) {
          long_store<LPE, NV, RPG, FG, SLAB>(xb, s_x + (size_t)((t + 2) & 1) * SLAB * ROWQ, n - (t + 2) * SLAB, fg, gl);
          long_request<LPE, NV, RPG, FG, SLAB>(xb, s_k, t + 4, n, fg, gl, h4, rowq);
        } else if (lane < AL) {
          const int r0 = (t + 1) * SLAB;
          chain_rows<FPL, HF>(s_w + r0, reinterpret_cast<const float*>(s_x + (size_t)((t + 1) & 1) * SLAB * ROWQ) + lane * FPL,
                              n - r0 < SLAB ? n - r0 : SLAB, acc1, acc2);
        }
        __syncthreads();
      }
    }
  }
  if (wv == 0 && lane < AL) {
    const i64 o = (out_row ? out_row[e] : e) * H + lane * FPL;
#pragma unroll
    for (int q = 0; q < FPL; ++q) {
      xcn1[o + q] = acc1[q];
      xcn2[o + q] = acc2[q];
      xij[o + q] = __fmul_rn(h[i * H + lane * FPL + q], h[j * H + lane * FPL + q]);
    }
  }
}

// cn6 pooling: three pooled vectors.  flagsA carries the cn1 / cn2 bits, flagsB's bit 0 the cn3 bit (two
// intersection passes over the same source rows, so the same `off`); per entry
//   w1 = [cn1]*inv1,  w2 = ([cn2] - t*[cn1])*inv2,  w3 = (([cn3] - t*[cn1]) - nip*w2)*inv3,
// each product / difference rounded separately, pooled in ascending column order.  The walk of lane_group.h,
// a round of LPE positions; LPE lanes per batch row, like cn_gather_kernel (no hub-row split: every row keeps the sequential order).
template <int LPE, int NV>
__global__ __launch_bounds__(OCN_BLOCK) void cn_gather3_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const i64* __restrict__ off, const uint8_t* __restrict__ flagsA, const uint8_t* __restrict__ flagsB,
    const float4* __restrict__ wA, const float4* __restrict__ wB, const float* __restrict__ nip_p,
    const float* __restrict__ h, int H, float* __restrict__ xcn1, float* __restrict__ xcn2,
    float* __restrict__ xcn3, float* __restrict__ xij) {
  constexpr int UNR = 4;
  const lane_group<LPE> g;
  const int gl = g.gl, gbase = g.gbase;
  const i64 slot = g.slot((i64)blockIdx.x);
  if (slot >= B) return;
  const i64 e = order ? order[slot] : slot;
  const i64 i = src[e], j = dst[e];
  const i64 a0 = rowptrA[i], da = rowptrA[i + 1] - a0;
  const i64 base = off[e];
  const float nip = nip_p[0];
  const float4* h4 = reinterpret_cast<const float4*>(h);
  const i64 rowq = H >> 2;
  float4 acc1[NV], acc2[NV], acc3[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc1[v] = acc2[v] = acc3[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (i64 p0 = 0; p0 < da; p0 += LPE) {
    const i64 p = p0 + gl;
    int32_t k = 0;
    unsigned fa = 0, fb = 0;
    if (p < da) { k = colA[a0 + p]; fa = flagsA[base + p]; fb = flagsB[base + p] & OCN_F_CN1; }
    float w1 = 0.f, w2 = 0.f, w3 = 0.f;
    if (fa | fb) {
      const float4 a = wA[k];
      const float inv3 = wB[k].x;
      const float tt = (fa & OCN_F_CN1) ? a.y : 0.f;
      w1 = (fa & OCN_F_CN1) ? a.x : 0.f;
      w2 = __fmul_rn(__fsub_rn((fa & OCN_F_CN2) ? 1.0f : 0.f, tt), a.z);
      w3 = __fmul_rn(__fsub_rn(__fsub_rn(fb ? 1.0f : 0.f, tt), __fmul_rn(nip, w2)), inv3);
    }
    const bool need = (w1 != 0.f) | (w2 != 0.f) | (w3 != 0.f);
    unsigned long long m = lane_group_mask<LPE>(need, gbase);
    while (m) {
      int bsel[UNR];
      lane_group_take(m, bsel);
      float ww1[UNR], ww2[UNR], ww3[UNR];
      float4 x[UNR][NV];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int sl = lane_group_src(gbase, bsel[u]);
        const int32_t kk = __shfl(k, sl, OCN_WAVE);
        ww1[u] = __shfl(w1, sl, OCN_WAVE);
        ww2[u] = __shfl(w2, sl, OCN_WAVE);
        ww3[u] = __shfl(w3, sl, OCN_WAVE);
        lane_group_row<LPE>(bsel[u], kk, h4, rowq, gl, x[u]);
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (bsel[u] >= 0) {
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            axpy4(acc1[v], ww1[u], x[u][v]);
            axpy4(acc2[v], ww2[u], x[u][v]);
            axpy4(acc3[v], ww3[u], x[u][v]);
          }
        }
      }
    }
  }
  pool_store<LPE, NV>(e, i, j, gl, h4, rowq, acc1, acc2, xcn1, xcn2, xij);
  float4* o3 = reinterpret_cast<float4*>(xcn3) + e * rowq + gl;
#pragma unroll
  for (int v = 0; v < NV; ++v) o3[v * LPE] = acc3[v];
}

// any H: one wave per edge, one feature per lane per 64-wide chunk (re-walks the flags per chunk)
__global__ __launch_bounds__(OCN_BLOCK) void cn_gather_generic(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const i64* __restrict__ off, const uint8_t* __restrict__ flags, const int32_t* __restrict__ wc,
    const float4* __restrict__ weights, const float* __restrict__ h, int H,
    float* __restrict__ xcn1, float* __restrict__ xcn2, float* __restrict__ xij,
    const i64* __restrict__ out_row) {   // out_row[batch row] = output row (class-major heads), or NULL
  const int lane = threadIdx.x & 63;
  const i64 slot = (i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6);
  if (slot >= B) return;
  const i64 e = order ? order[slot] : slot;
  const i64 i = src[e], j = dst[e];
  const i64 a0 = rowptrA[i], da = rowptrA[i + 1] - a0;
  const i64 base = off[e];
  for (int f0 = 0; f0 < H; f0 += OCN_WAVE) {
    const int ft = f0 + lane;
    const bool fin = ft < H;
    float acc1 = 0.f, acc2 = 0.f;
    for (i64 p0 = 0; p0 < da; p0 += OCN_WAVE) {
      const i64 p = p0 + lane;
      int32_t k = 0;
      unsigned f = 0;
      if (p < da) { k = colA[a0 + p]; f = flags[base + p]; }
      float wa = 0.f, wb = 0.f;
      if (f) entry_weights(f, weights[k], wc ? (float)wc[base + p] : 1.0f, wa, wb);
      unsigned long long m = __ballot((wa != 0.f) | (wb != 0.f));
      while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int32_t kk = __shfl(k, b, OCN_WAVE);
        const float a = __shfl(wa, b, OCN_WAVE), bb = __shfl(wb, b, OCN_WAVE);
        if (fin) {
          const float x = h[(i64)kk * H + ft];
          acc1 = __fadd_rn(acc1, __fmul_rn(a, x));
          acc2 = __fadd_rn(acc2, __fmul_rn(bb, x));
        }
      }
    }
    if (fin) {
      const i64 oe = out_row ? out_row[e] : e;
      xcn1[oe * H + ft] = acc1;
      xcn2[oe * H + ft] = acc2;
      xij[oe * H + ft] = __fmul_rn(h[i * H + ft], h[j * H + ft]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// H = 256 batches of at least this many candidates take the pair form (cn_gather_pair_kernel): B / 2 waves must still fill
// the chip's wave slots several times over.  Process-wide; see ocn_hip.h.
static int64_t g_gather_pair_min_batch = 32768;

template <int LPE, int NV>
static void launch_gather(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                          const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flags,
                          const int32_t* wc, const float* weights, const float* h, int32_t H, int64_t max_row_len,
                          float* xcn1, float* xcn2, float* xij, const int64_t* out_row, const int32_t* cnt1,
                          const int32_t* cnt2, const uint64_t* rec, const int32_t* perm, const float* rowsum, hipStream_t st) {
  const int32_t* sched = sched_followed(perm, rec, B, LPE);      // the schedule to follow, or nullptr (common.h)
  bool packed = true;
  if constexpr (LPE <= 16) {
    if (B * LPE < 262144) {                  // the packed form would not fill the SIMDs
      constexpr int WW = gather_wave_wpb<LPE, NV, false>();
      hipLaunchKernelGGL((cn_gather_wave_kernel<LPE, NV>), dim3((unsigned)((B + WW - 1) / WW)),
                         dim3(WW * OCN_WAVE), 0, st, (const i64*)rowptrA, colA, (const i64*)src, (const i64*)dst,
                         (const i64*)order, (i64)B, (const i64*)off, flags, wc, (const float4*)weights, h, (int)H,
                         xcn1, xcn2, xij, (const i64*)out_row, cnt2, rowsum);
      packed = false;
    }
  }
#define PACKED_ARGS (const i64*)rowptrA, colA, (const i64*)src, (const i64*)dst, (const i64*)order, (i64)B, \
                    (const i64*)off, flags, wc, (const float4*)weights, h, (int)H, xcn1, xcn2, xij,           \
                    (const i64*)out_row, cnt1, cnt2, (const u64*)rec
  if constexpr (LPE == OCN_WAVE && NV == 1) {
    // two slots per wave (cn_gather_pair_kernel): record-fed pattern batches without the row-sum shortcut, from the bound on.
    // A workgroup is two schedule groups, so a schedule is followed only where an XCD's eighth is whole pairs of groups — an odd
    // eighth keeps the one-slot form; without a schedule the pairs are consecutive groups of the source order.
    static_assert(lane_group_epb(LPE) == SCHED_GROUP, "the pair form's workgroup: two schedule groups");
    const i64 n_groups = sched_groups(B);
    if (rec && !wc && !rowsum && B >= g_gather_pair_min_batch && (!sched || (n_groups / SCHED_EIGHTHS) % 2 == 0)) {
      hipLaunchKernelGGL(cn_gather_pair_kernel, dim3((unsigned)((n_groups + 1) / 2)), dim3(OCN_BLOCK), 0, st, colA, (i64)B, flags,
                         (const float4*)weights, h, xcn1, xcn2, xij, (const i64*)out_row, (const u64*)rec, sched);
      packed = false;
    }
  }
  if (packed)
    hipLaunchKernelGGL((cn_gather_kernel<LPE, NV>), dim3(lane_group_blocks(B, LPE)), dim3(OCN_BLOCK), 0, st,
                       PACKED_ARGS, sched, rowsum);
#undef PACKED_ARGS
#define LONG_ARGS (const i64*)rowptrA, colA, (const i64*)src, (const i64*)dst, (i64)B, (const i64*)off, flags, wc, \
                  (const float4*)weights, h, (int)H, xcn1, xcn2, xij, (const i64*)out_row, cnt2, rowsum
  if (max_row_len > LONG_ROW) {
    // (H = 512 — two float4 per lane — does not fit the 128 registers a 1024-thread workgroup leaves a lane: 104 spilled
    // VGPRs in round 3; it takes the 256-thread form at every batch size)
    bool small = false;
    if constexpr (NV == 1) {
      if (B <= 4096) {
        static bool raised_dev[64] = {};        // 2 x 64 KiB of slab: above the default dynamic-LDS limit (attribute is per device)
        int devid = 0;
        if (hipGetDevice(&devid) == hipSuccess && devid >= 0 && devid < 64 && !raised_dev[devid]) {
          if (hipFuncSetAttribute((const void*)cn_gather_long_kernel<LPE, NV, LONG_SMALL_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  2 * LONG_SLAB_BYTES(LONG_SMALL_THREADS)) == hipSuccess) raised_dev[devid] = true;
        }
        hipLaunchKernelGGL((cn_gather_long_kernel<LPE, NV, LONG_SMALL_THREADS>), dim3((unsigned)B), dim3(LONG_SMALL_THREADS), 2 * LONG_SLAB_BYTES(LONG_SMALL_THREADS), st, LONG_ARGS);
        small = true;
      }
    }
    if (!small) {
      bool by_wave = false;
      if constexpr (LPE <= 16) {             // narrow embeddings: a wave per hub row, 64 gathers in flight each
        hipLaunchKernelGGL((cn_gather_wave_kernel<LPE, NV, true>), dim3((unsigned)B), dim3(OCN_WAVE), 0, st, (const i64*)rowptrA, colA, (const i64*)src, (const i64*)dst,
                           (const i64*)order, (i64)B, (const i64*)off, flags, wc, (const float4*)weights, h, (int)H,
                           xcn1, xcn2, xij, (const i64*)out_row, cnt2, rowsum);
        by_wave = true;
      }
      if (!by_wave) hipLaunchKernelGGL((cn_gather_long_kernel<LPE, NV, 256>), dim3((unsigned)B), dim3(256), 2 * LONG_SLAB_BYTES(256), st, LONG_ARGS);
    }
  }
#undef LONG_ARGS
}

extern "C" {

#define GATHER_ARGS (const i64*)rowptrA, colA, (const i64*)src, (const i64*)dst, (const i64*)order, (i64)B, (const i64*)off, \
                    flags, wc, (const float4*)weights, h, (int)H, xcn1, xcn2, xij, (const i64*)out_row
#define LAUNCH_GATHER(LPE, NV)                                                                      \
  launch_gather<LPE, NV>(rowptrA, colA, src, dst, order, B, off, flags, wc, weights, h, H, max_row_len, xcn1, xcn2, xij, out_row, cnt1, cnt2, rec, perm, rowsum, st)

int ocn_cn_gather(const int64_t* rowptrA, const int32_t* colA, const int64_t* src,
                  const int64_t* dst, const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flags,
                  const int32_t* wc, const float* weights, const float* h, int32_t H,
                  int64_t max_row_len, float* xcn1, float* xcn2, float* xij, const int64_t* out_row,
                  const int32_t* cnt1, const int32_t* cnt2, const uint64_t* rec, const int32_t* perm, const float* rowsum,
                  void* stream) {
  if (B < 0 || H <= 0) return OCN_EINVAL;
  if (B == 0) return 0;
  if (!rowptrA || !src || !dst || !off || !weights || !h || !xcn1 || !xcn2 || !xij) return OCN_EINVAL;
  if (rowsum && (wc || !cnt2)) return OCN_EINVAL;          // the shortcut is the pattern route's, and needs the per-row counts
  hipStream_t st = (hipStream_t)stream;
  switch (H) {
    case 16:  LAUNCH_GATHER(4, 1); break;
    case 32:  LAUNCH_GATHER(8, 1); break;
    case 64:  LAUNCH_GATHER(16, 1); break;
    case 128: LAUNCH_GATHER(32, 1); break;
    case 256: LAUNCH_GATHER(POOL_LPE, (64 / POOL_LPE)); break;
    case 512: LAUNCH_GATHER(64, 2); break;
    default:   /* generic widths: every row by one wave, no long-row split */
      hipLaunchKernelGGL(cn_gather_generic, dim3((unsigned)((B + OCN_WPB - 1) / OCN_WPB)),
                         dim3(OCN_BLOCK), 0, st, GATHER_ARGS);
  }
  return launch_status();
}

int64_t ocn_cn_gather_pair_min_batch(int64_t min_rows) {
  const int64_t prev = g_gather_pair_min_batch;
  if (min_rows >= 0) g_gather_pair_min_batch = min_rows;
  return prev;
}

#define LAUNCH_GATHER3(LPE, NV)                                                                     \
  hipLaunchKernelGGL((cn_gather3_kernel<LPE, NV>),                                                   \
                     dim3(lane_group_blocks(B, LPE)),                                                \
                     dim3(OCN_BLOCK), 0, (hipStream_t)stream, (const i64*)rowptrA, colA, (const i64*)src,      \
                     (const i64*)dst, (const i64*)order, (i64)B, (const i64*)off, flagsA, flagsB,             \
                     (const float4*)weightsA, (const float4*)weightsB, nip, h, (int)H, xcn1, xcn2, xcn3, xij)

int ocn_cn_gather3(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                   const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flagsA,
                   const uint8_t* flagsB, const float* weightsA, const float* weightsB, const float* nip,
                   const float* h, int32_t H, float* xcn1, float* xcn2, float* xcn3, float* xij, void* stream) {
  if (B < 0 || H <= 0) return OCN_EINVAL;
  if (B == 0) return 0;
  if (!rowptrA || !src || !dst || !off || !weightsA || !weightsB || !nip || !h || !xcn1 || !xcn2 || !xcn3 || !xij)
    return OCN_EINVAL;
  OCN_SWITCH_WIDTH(H, LAUNCH_GATHER3)
  return launch_status();
}

}  // extern "C"
