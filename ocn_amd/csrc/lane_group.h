// The lane-group walk: what the kernels that gather embedding rows over a candidate's common-neighbour list share — pool_range
// and cn_gather3_kernel (cn_pool.hip), cn8_pool_kernel, cn_pool_frozen_kernel, cn_attr_kernel.  LPE lanes cooperate on one
// candidate (64 / LPE candidates per wave); a lane owns NV float4 of the H = LPE * NV * 4 features (OCN_SWITCH_WIDTH, common.h).
// A round covers LPE * PT positions of the source row N(i), PT per lane; the entries to fetch are then walked in ascending
// position, UNR embedding rows in flight per group:
//   unsigned long long m = lane_group_mask<LPE>(need, gbase);          // the group's ballot
//   while (m) {
//     lane_group_take(m, bsel);                                        // the next UNR entries
//     for u: sl = lane_group_src(gbase, bsel[u]); kk = __shfl(k, sl);  // ... their lanes and column ids (and whatever else
//            lane_group_row<LPE>(bsel[u], kk, h4, rowq, gl, x[u]);     //     the kernel needs from lane sl); all UNR rows requested
//     for u: if (bsel[u] >= 0) ... x[u] ...                            // ... before the first is used
//   }
// What a kernel does with a row is its own, and the two loops stay in the kernels: as one template that takes the body as a
// callable, no kernel kept the machine code it was measured with ("One lane-group walk").
#pragma once
#include "common.h"

// ---- geometry
template <int LPE>
struct lane_group {
  static constexpr int GPW = OCN_WAVE / LPE;       // candidates per wave
  static constexpr int PT = GPW < 8 ? GPW : 8;     // positions per lane and round: narrow groups would otherwise pay one
                                                   // dependent load chain per LPE positions (hub rows of ppa: 101 -> 40 us)
  int lane, gl, gbase;                             // the lane, its place in its group, the group's first lane
  __device__ __forceinline__ lane_group() {
    lane = threadIdx.x & 63;
    gl = lane % LPE;
    gbase = lane - gl;
  }
  // The group's candidate slot; a group whose slot is past the batch leaves as a whole.  `bid` is the workgroup's place in
  // the processing order: xcd_block(), cn_gather_kernel's schedule lookup, or blockIdx.x.
  __device__ __forceinline__ i64 slot(i64 bid) const { return (bid * OCN_WPB + (threadIdx.x >> 6)) * GPW + lane / LPE; }
};

// ---- the walk
// One position per lane: the group's ballot of `need`, bit b = lane gbase + b (the same in all of the group's lanes).
template <int LPE>
__device__ __forceinline__ unsigned long long lane_group_mask(bool need, int gbase) {
  unsigned long long m = __ballot(need);
  if (LPE < 64) m = (m >> gbase) & ((1ull << (LPE & 63)) - 1ull);
  return m;
}

// The next UNR set bits of m, ascending (-1 past its last), taken out of m.
template <int UNR>
__device__ __forceinline__ void lane_group_take(unsigned long long& m, int (&bsel)[UNR]) {
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    bsel[u] = m ? (__ffsll((long long)m) - 1) : -1;
    m &= m - 1;                                // no-op once m == 0
  }
}

// the wave lane that owns bit b of the group's mask (the group's first lane for b = -1: a shuffle from it is always defined)
__device__ __forceinline__ int lane_group_src(int gbase, int b) { return gbase + (b < 0 ? 0 : b); }

// This lane's NV float4 of row h[kk], requested where b >= 0 (b, kk: an entry of lane_group_take and its column id,
// shuffled from lane_group_src).  A caller issues all UNR of them before it uses the first.
template <int LPE, int NV>
__device__ __forceinline__ void lane_group_row(int b, int32_t kk, const float4* h4, i64 rowq, int gl, float4 (&x)[NV]) {
  if (b >= 0) {
    const float4* row = h4 + (i64)kk * rowq + gl;
#pragma unroll
    for (int v = 0; v < NV; ++v) x[v] = row[v * LPE];
  }
}

// ---- the one-pass kernels (cn8_pool_kernel, cn_pool_frozen_kernel): the candidate and its membership probe; T1 / T2 come as
// bit rows (bm != NULL) or as CSR rows, each on its own
struct lane_group_pair {
  i64 e, i, j, a0, da;                         // batch row, endpoints, the source row N(i)
  const unsigned *bm1_row, *bm2_row;           // row j of T1 / T2 as bits, or NULL
  const int32_t *colT1, *colT2;                // ... else as the sorted row [b0, b0 + db) / [c0, c0 + dc) of these
  i64 b0, db, c0, dc;

  // order -> src / dst -> rowptr -> bit rows or CSR rows
  __device__ __forceinline__ lane_group_pair(
      i64 slot, const i64* __restrict__ rowptrA, const i64* __restrict__ rowptrT1, const int32_t* __restrict__ colT1_,
      const i64* __restrict__ rowptrT2, const int32_t* __restrict__ colT2_, const unsigned* __restrict__ bmT1, i64 bm1_stride,
      const unsigned* __restrict__ bmT2, i64 bm2_stride, const i64* __restrict__ src, const i64* __restrict__ dst,
      const i64* __restrict__ order)
      : colT1(colT1_), colT2(colT2_), b0(0), db(0), c0(0), dc(0) {
    e = order ? order[slot] : slot;
    i = src[e]; j = dst[e];
    a0 = rowptrA[i]; da = rowptrA[i + 1] - a0;
    bm1_row = bmT1 ? bmT1 + j * bm1_stride : nullptr;
    bm2_row = bmT2 ? bmT2 + j * bm2_stride : nullptr;
    if (!bmT1) { b0 = rowptrT1[j]; db = rowptrT1[j + 1] - b0; }
    if (!bmT2) { c0 = rowptrT2[j]; dc = rowptrT2[j + 1] - c0; }
  }

  // the flag byte of column k (a column of N(i)); the member counts take it too
  __device__ __forceinline__ unsigned probe(int32_t k, int& c1, int& c2) const {
    const bool f1 = bm1_row ? ((bm1_row[k >> 5] >> (k & 31)) & 1u) : sorted_has(colT1 + b0, db, k);
    const bool f2 = bm2_row ? ((bm2_row[k >> 5] >> (k & 31)) & 1u) : sorted_has(colT2 + c0, dc, k);
    const unsigned f = (f1 ? OCN_F_CN1 : 0u) | (f2 ? OCN_F_CN2 : 0u);
    c1 += f1;
    c2 += f2;
    return f;
  }
};

// ---- output
// One float4 of a candidate's three output rows: the pooled pair (where the heads read them) and x_i * x_j from the endpoint
// rows' quads a, b.
__device__ __forceinline__ void pool_emit(float4* __restrict__ o1, float4* __restrict__ o2, float4* __restrict__ o3,
                                          const float4& acc1, const float4& acc2, const float4& a, const float4& b, bool st1,
                                          bool st2) {
  if (st1) *o1 = acc1;
  if (st2) *o2 = acc2;
  *o3 = make_float4(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y), __fmul_rn(a.z, b.z), __fmul_rn(a.w, b.w));
}

// ... all of a lane's: output row e, endpoints i and j
template <int LPE, int NV>
__device__ __forceinline__ void pool_store(i64 e, i64 i, i64 j, int gl, const float4* __restrict__ h4, i64 rowq,
                                           const float4 (&acc1)[NV], const float4 (&acc2)[NV], float* __restrict__ xcn1,
                                           float* __restrict__ xcn2, float* __restrict__ xij, bool st1 = true, bool st2 = true) {
  const float4* hi = h4 + i * rowq + gl;
  const float4* hj = h4 + j * rowq + gl;
  float4* o1 = reinterpret_cast<float4*>(xcn1) + e * rowq + gl;
  float4* o2 = reinterpret_cast<float4*>(xcn2) + e * rowq + gl;
  float4* o3 = reinterpret_cast<float4*>(xij) + e * rowq + gl;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const float4 a = hi[v * LPE], b = hj[v * LPE];
    pool_emit(o1 + v * LPE, o2 + v * LPE, o3 + v * LPE, acc1[v], acc2[v], a, b, st1, st2);
  }
}
