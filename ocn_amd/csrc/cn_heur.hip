// Link heuristics (common neighbours, Adamic-Adar, resource allocation, ... — the training-free baselines of the OCN / NCN
// tables): per candidate (i, j) the sum of a per-node weight row over N(i) ∩ T1(j) and over N(i) ∩ T2(j), in ONE pass.
// The shape of cn8_pool.hip with a 16-byte node row in place of an embedding row: nothing of a candidate depends on the
// rest of the batch, so there are no flag bytes, no histogram, no atomics and no workspace.
// See include/ocn_hip.h (ocn_cn_node_sums).
#include "lane_group.h"

constexpr int HEUR_LPE = 16;                     // lanes per candidate: four candidates per wave, sixteen per workgroup
constexpr int HEUR_PT = 4;                       // positions per lane and round: a round tests 64 positions of N(i)

// membership of key in the sorted row a[0..n): the largest q with a[q] <= key is found in a number of steps that depends
// on n alone — the lanes of a group search the same row, so they stay together — and every load is unconditional and in
// bounds for any key (a key of -1, a lane without a position, is simply not found)
// (not common.h's sorted_has: that one's trip count and branches depend on the key, and it has no load for an empty lane)
__device__ __forceinline__ bool heur_row_has(const int32_t* __restrict__ a, i64 n, int32_t key) {
  if (n <= 0) return false;
  i64 base = 0;
  for (i64 len = n; len > 1;) {
    const i64 half = len >> 1;
    base += (a[base + half] <= key) ? half : 0;
    len -= half;
  }
  return a[base] == key;
}

__device__ __forceinline__ bool heur_bit(const unsigned* __restrict__ row, int32_t k) {
  const int32_t kc = k < 0 ? 0 : k;             // clamped index, predicated use: the load itself is unconditional
  return (k >= 0) & ((row[kc >> 5] >> (kc & 31)) & 1u);
}

// HEUR_LPE lanes cooperate on one candidate.  A round takes HEUR_LPE * HEUR_PT positions of the source row N(i): every
// lane loads its column ids, tests them against row j of T1 (and of T2), and the lanes that hit fetch their node's weight
// row (one 16-byte load).  The group then walks the ballot of the hits in ascending position and broadcasts each row, so
// that every lane performs the same adds: one fp32 add per member and weight column, in ascending column order, whatever
// the row's length (a hub row only takes more rounds).
template <bool HAS2>
__global__ __launch_bounds__(OCN_BLOCK) void cn_node_sums_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrT1, const int32_t* __restrict__ colT1,
    const i64* __restrict__ rowptrT2, const int32_t* __restrict__ colT2,
    const unsigned* __restrict__ bmT1, i64 bm1_stride, const unsigned* __restrict__ bmT2, i64 bm2_stride,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const float* __restrict__ w, float* __restrict__ sum1, float* __restrict__ sum2,
    int32_t* __restrict__ cnt1, int32_t* __restrict__ cnt2, float* __restrict__ deg) {
  const lane_group<HEUR_LPE> g;
  const int gl = g.gl, gbase = g.gbase;
  const i64 slot = g.slot(xcd_block());     // an XCD's eighth of the processing order, as cn8_pool_kernel takes
  if (slot >= B) return;                    // whole group leaves together
  const i64 e = order ? order[slot] : slot;
  const i64 i = src[e], j = dst[e];
  const i64 a0 = rowptrA[i], da = rowptrA[i + 1] - a0;
  const unsigned* bm1_row = bmT1 ? bmT1 + j * bm1_stride : nullptr;
  const unsigned* bm2_row = (HAS2 && bmT2) ? bmT2 + j * bm2_stride : nullptr;
  i64 b0 = 0, db = 0, c0 = 0, dc = 0;
  if (!bmT1 || deg) { b0 = rowptrT1[j]; db = rowptrT1[j + 1] - b0; }      // (the host refuses `deg` without T1's row pointers)
  if (HAS2 && !bmT2) { c0 = rowptrT2[j]; dc = rowptrT2[j + 1] - c0; }
  const float4* w4 = reinterpret_cast<const float4*>(w);
  f32x4 acc1 = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
  int c1 = 0, c2 = 0;
  for (i64 p0 = 0; p0 < da; p0 += HEUR_LPE * HEUR_PT) {
    int32_t k[HEUR_PT];
    unsigned f[HEUR_PT];
    f32x4 wv[HEUR_PT];
#pragma unroll
    for (int t = 0; t < HEUR_PT; ++t) {
      const i64 p = p0 + t * HEUR_LPE + gl;
      const int32_t kv = colA[a0 + (p < da ? p : da - 1)];
      k[t] = p < da ? kv : -1;
    }
#pragma unroll
    for (int t = 0; t < HEUR_PT; ++t) {
      const bool f1 = bm1_row ? heur_bit(bm1_row, k[t]) : heur_row_has(colT1 + b0, db, k[t]);
      bool f2 = false;
      if (HAS2) f2 = bm2_row ? heur_bit(bm2_row, k[t]) : heur_row_has(colT2 + c0, dc, k[t]);
      f[t] = (f1 ? OCN_F_CN1 : 0u) | (f2 ? OCN_F_CN2 : 0u);
      c1 += f1;
      c2 += f2;
    }
#pragma unroll
    for (int t = 0; t < HEUR_PT; ++t) {             // the lanes without a hit all read row 0: one cache line
      const float4 x = w4[f[t] ? k[t] : 0];
      wv[t] = f32x4{x.x, x.y, x.z, x.w};
    }
#pragma unroll
    for (int t = 0; t < HEUR_PT; ++t) {             // ascending position order: tile t, then lane
      unsigned long long m = lane_group_mask<HEUR_LPE>(f[t] != 0, gbase);
      while (m) {                                   // (the same trip count in every lane of the group)
        const int sl = gbase + __ffsll((long long)m) - 1;
        m &= m - 1;
        const unsigned ff = (unsigned)__shfl((int)f[t], sl, OCN_WAVE);
        const f32x4 xv = {__shfl(wv[t].x, sl, OCN_WAVE), __shfl(wv[t].y, sl, OCN_WAVE), __shfl(wv[t].z, sl, OCN_WAVE),
                          __shfl(wv[t].w, sl, OCN_WAVE)};
        if (ff & OCN_F_CN1) acc1 = acc1 + xv;
        if (ff & OCN_F_CN2) acc2 = acc2 + xv;
      }
    }
  }
#pragma unroll
  for (int o = HEUR_LPE / 2; o > 0; o >>= 1) {
    c1 += __shfl_xor(c1, o, OCN_WAVE);
    c2 += __shfl_xor(c2, o, OCN_WAVE);
  }
  // every lane of the group holds the same sums: four of them store one output each (vector stores)
  if (gl == 0) reinterpret_cast<float4*>(sum1)[e] = make_float4(acc1.x, acc1.y, acc1.z, acc1.w);
  if (gl == 1) reinterpret_cast<float4*>(sum2)[e] = make_float4(acc2.x, acc2.y, acc2.z, acc2.w);
  if (gl == 2) { cnt1[e] = c1; cnt2[e] = c2; }
  if (gl == 3 && deg) reinterpret_cast<float2*>(deg)[e] = make_float2((float)da, (float)db);
}

extern "C" {

int ocn_cn_node_sums(const int64_t* rowptrA, const int32_t* colA,
                     const int64_t* rowptrT1, const int32_t* colT1,
                     const int64_t* rowptrT2, const int32_t* colT2,
                     const uint32_t* bitmapT1, int64_t bm1_stride_words,
                     const uint32_t* bitmapT2, int64_t bm2_stride_words,
                     const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B, int64_t n_cols,
                     const float* w, float* sum1, float* sum2, int32_t* cnt1, int32_t* cnt2, float* deg, void* stream) {
  if (B < 0 || n_cols < 0) return OCN_EINVAL;
  if (!rowptrA || !colA || !src || !dst || !w || !sum1 || !sum2 || !cnt1 || !cnt2) return OCN_EINVAL;
  const bool has2 = bitmapT2 || rowptrT2 || colT2;                        // T2 is optional here
  if (!set_operand_ok(bitmapT1, bm1_stride_words, rowptrT1, colT1, n_cols)) return OCN_EINVAL;
  if (has2 && !set_operand_ok(bitmapT2, bm2_stride_words, rowptrT2, colT2, n_cols)) return OCN_EINVAL;
  if ((bitmapT1 && bm1_stride_words < 0) || (bitmapT2 && bm2_stride_words < 0)) return OCN_EINVAL;
  if (deg && !rowptrT1) return OCN_EINVAL;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(lane_group_blocks(B, HEUR_LPE));
#define LAUNCH_HEUR(HAS2)                                                                                              \
  hipLaunchKernelGGL((cn_node_sums_kernel<HAS2>), grid, dim3(OCN_BLOCK), 0, st, (const i64*)rowptrA, colA,             \
                     (const i64*)rowptrT1, colT1, (const i64*)rowptrT2, colT2, (const unsigned*)bitmapT1,              \
                     (i64)bm1_stride_words, (const unsigned*)bitmapT2, (i64)bm2_stride_words, (const i64*)src,         \
                     (const i64*)dst, (const i64*)order, (i64)B, w, sum1, sum2, cnt1, cnt2, deg)
  if (has2) LAUNCH_HEUR(true); else LAUNCH_HEUR(false);
#undef LAUNCH_HEUR
  return launch_status();
}

}  // extern "C"
