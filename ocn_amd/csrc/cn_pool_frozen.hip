// cn5 / cn7 with FROZEN column weights: intersection and weighted pooling of a candidate batch in ONE pass.
// The column weights {w1, t, inv2, 0} are the table a reference batch left (ocn_cn_weights_cn5 / _cn7, kept by
// ocn_amd/frozen.py) instead of the statistics of the batch at hand, so nothing of a candidate's pooled vectors depends
// on the rest of its batch: no flag bytes, no histogram atomics, no column statistics, no weights pass, no workspace.
// The arithmetic per candidate is that of ocn_cn_gather on the pattern route (entry_weights with c = 1, the fetch rule
// wa != 0 || wb != 0, product and sum rounded separately, ascending column order).  See include/ocn_hip.h
// (ocn_cn_pool_frozen).
#include "lane_group.h"

constexpr int FROZEN_UNR = 4;   // embedding rows in flight per lane group

// The lane-group walk of lane_group.h.  A round tests LPE * PT positions of the source row N(i) — one membership probe pair
// per lane and position — and the lane that holds a member's column id loads that column's weight row with it (one 16-byte
// load) and forms the entry's (wa, wb).  The entries with a non-zero weight are then walked in ascending position, each
// adding to BOTH accumulators.  A hub row is walked by the same group in the same order (it only takes more rounds).
template <int LPE, int NV>
__global__ __launch_bounds__(OCN_BLOCK) void cn_pool_frozen_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrT1, const int32_t* __restrict__ colT1,
    const i64* __restrict__ rowptrT2, const int32_t* __restrict__ colT2,
    const unsigned* __restrict__ bmT1, i64 bm1_stride, const unsigned* __restrict__ bmT2, i64 bm2_stride,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const float4* __restrict__ weights, const float* __restrict__ h, int H,
    float* __restrict__ xcn1, float* __restrict__ xcn2, float* __restrict__ xij,
    int32_t* __restrict__ cnt1, int32_t* __restrict__ cnt2) {
  constexpr int PT = lane_group<LPE>::PT;
  const lane_group<LPE> g;
  const int gl = g.gl, gbase = g.gbase;
  const i64 slot = g.slot(xcd_block());     // an XCD's eighth of the processing order, as the pooling of the chain takes
  if (slot >= B) return;                    // whole group leaves together
  const lane_group_pair c(slot, rowptrA, rowptrT1, colT1, rowptrT2, colT2, bmT1, bm1_stride, bmT2, bm2_stride, src, dst, order);
  const i64 e = c.e, i = c.i, j = c.j, a0 = c.a0, da = c.da;
  const float4* h4 = reinterpret_cast<const float4*>(h);
  const i64 rowq = H >> 2;                  // float4 per row
  f32x4 acc1[NV], acc2[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc1[v] = acc2[v] = f32x4{0.f, 0.f, 0.f, 0.f};
  int c1 = 0, c2 = 0;
  for (i64 p0 = 0; p0 < da; p0 += LPE * PT) {
    int32_t k[PT];
    unsigned f[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      const i64 p = p0 + t * LPE + gl;
      k[t] = p < da ? colA[a0 + p] : -1;
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      f[t] = 0;
      if (k[t] >= 0) f[t] = c.probe(k[t], c1, c2);      // (the member counts: whatever the weights are)
    }
    float wa[PT], wb[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      wa[t] = wb[t] = 0.f;
      if (f[t]) entry_weights(f[t], weights[k[t]], 1.0f, wa[t], wb[t]);
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {             // ascending position order: tile t, then lane
      const bool need = (wa[t] != 0.f) | (wb[t] != 0.f);
      unsigned long long m = lane_group_mask<LPE>(need, gbase);
      while (m) {
        int bsel[FROZEN_UNR];
        lane_group_take(m, bsel);
        float wwa[FROZEN_UNR], wwb[FROZEN_UNR];
        float4 x[FROZEN_UNR][NV];
#pragma unroll
        for (int u = 0; u < FROZEN_UNR; ++u) {
          const int sl = lane_group_src(gbase, bsel[u]);
          const int32_t kk = __shfl(k[t], sl, OCN_WAVE);
          wwa[u] = __shfl(wa[t], sl, OCN_WAVE);
          wwb[u] = __shfl(wb[t], sl, OCN_WAVE);
          lane_group_row<LPE>(bsel[u], kk, h4, rowq, gl, x[u]);
        }
#pragma unroll
        for (int u = 0; u < FROZEN_UNR; ++u) {
          if (bsel[u] >= 0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {       // two scalar chains: one multiply and one add per feature, entry and accumulator
              acc1[v].x = __fadd_rn(acc1[v].x, __fmul_rn(wwa[u], x[u][v].x));
              acc1[v].y = __fadd_rn(acc1[v].y, __fmul_rn(wwa[u], x[u][v].y));
              acc1[v].z = __fadd_rn(acc1[v].z, __fmul_rn(wwa[u], x[u][v].z));
              acc1[v].w = __fadd_rn(acc1[v].w, __fmul_rn(wwa[u], x[u][v].w));
              acc2[v].x = __fadd_rn(acc2[v].x, __fmul_rn(wwb[u], x[u][v].x));
              acc2[v].y = __fadd_rn(acc2[v].y, __fmul_rn(wwb[u], x[u][v].y));
              acc2[v].z = __fadd_rn(acc2[v].z, __fmul_rn(wwb[u], x[u][v].z));
              acc2[v].w = __fadd_rn(acc2[v].w, __fmul_rn(wwb[u], x[u][v].w));
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int o = LPE / 2; o > 0; o >>= 1) {
    c1 += __shfl_xor(c1, o, OCN_WAVE);
    c2 += __shfl_xor(c2, o, OCN_WAVE);
  }
  if (gl == 0) { cnt1[e] = c1; cnt2[e] = c2; }
  // (pool_store's loop, written out: through the call one instance in six gains an s_waitcnt)
  const float4* hi = h4 + i * rowq + gl;
  const float4* hj = h4 + j * rowq + gl;
  float4* o1 = reinterpret_cast<float4*>(xcn1) + e * rowq + gl;
  float4* o2 = reinterpret_cast<float4*>(xcn2) + e * rowq + gl;
  float4* o3 = reinterpret_cast<float4*>(xij) + e * rowq + gl;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const float4 a = hi[v * LPE], b = hj[v * LPE];
    pool_emit(o1 + v * LPE, o2 + v * LPE, o3 + v * LPE, make_float4(acc1[v].x, acc1[v].y, acc1[v].z, acc1[v].w),
              make_float4(acc2[v].x, acc2[v].y, acc2[v].z, acc2[v].w), a, b, true, true);
  }
}

extern "C" {

int ocn_cn_pool_frozen(const int64_t* rowptrA, const int32_t* colA,
                       const int64_t* rowptrT1, const int32_t* colT1,
                       const int64_t* rowptrT2, const int32_t* colT2,
                       const uint32_t* bitmapT1, int64_t bm1_stride_words,
                       const uint32_t* bitmapT2, int64_t bm2_stride_words,
                       const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B, int64_t n_cols,
                       const float* weights, const float* h, int32_t H, float* xcn1, float* xcn2, float* xij,
                       int32_t* cnt1, int32_t* cnt2, void* stream) {
  if (B < 0 || n_cols < 0) return OCN_EINVAL;
  if (!lane_group_width(H)) return OCN_EINVAL;
  if (!rowptrA || !colA || !src || !dst || !weights || !h || !xcn1 || !xcn2 || !xij || !cnt1 || !cnt2) return OCN_EINVAL;
  if (((uintptr_t)weights & 15u) != 0) return OCN_EINVAL;
  if (!set_operand_ok(bitmapT1, bm1_stride_words, rowptrT1, colT1, n_cols)) return OCN_EINVAL;
  if (!set_operand_ok(bitmapT2, bm2_stride_words, rowptrT2, colT2, n_cols)) return OCN_EINVAL;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_FROZEN(LPE, NV)                                                                                  \
  hipLaunchKernelGGL((cn_pool_frozen_kernel<LPE, NV>), dim3(lane_group_blocks(B, LPE)), dim3(OCN_BLOCK), 0, st, \
                     (const i64*)rowptrA, colA, (const i64*)rowptrT1, colT1, (const i64*)rowptrT2, colT2,       \
                     (const unsigned*)bitmapT1, (i64)bm1_stride_words, (const unsigned*)bitmapT2,               \
                     (i64)bm2_stride_words, (const i64*)src, (const i64*)dst, (const i64*)order, (i64)B,        \
                     reinterpret_cast<const float4*>(weights), h, (int)H, xcn1, xcn2, xij, cnt1, cnt2)
  OCN_SWITCH_WIDTH(H, LAUNCH_FROZEN)
#undef LAUNCH_FROZEN
  return launch_status();
}

}  // extern "C"
