// cn8 (CNLinkPredictorbaselearnablation, model.py:3233-3449): intersection and pooling of a candidate batch in ONE pass.
// cn8's pooled vectors carry no column weight — xcn1 = sum of h[k] over N(i) ∩ N(j), xcn2 = the same over N(i) ∩ T2(j) —
// so nothing of a candidate's score depends on the rest of the batch: no flag bytes, no histogram, no weights buffer.
// See include/ocn_hip.h (ocn_cn8_pool).
#include "lane_group.h"

constexpr int CN8_UNR = 4;      // embedding rows in flight per lane group

// The lane-group walk of lane_group.h.  A round tests LPE * PT positions of the source row N(i) — one membership probe pair
// per lane and position — and then adds the rows of the members, position by position in ascending order, into the two
// accumulators: one fp32 add per feature and entry, the order of a sequential spmm over the sorted row.  A hub row is walked
// by the same group in the same order (it only takes more rounds).
template <int LPE, int NV>
__global__ __launch_bounds__(OCN_BLOCK) void cn8_pool_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ rowptrT1, const int32_t* __restrict__ colT1,
    const i64* __restrict__ rowptrT2, const int32_t* __restrict__ colT2,
    const unsigned* __restrict__ bmT1, i64 bm1_stride, const unsigned* __restrict__ bmT2, i64 bm2_stride,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const float* __restrict__ h, int H, float* __restrict__ xcn1, float* __restrict__ xcn2, float* __restrict__ xij,
    int32_t* __restrict__ cnt1, int32_t* __restrict__ cnt2) {
  constexpr int PT = lane_group<LPE>::PT;
  const lane_group<LPE> g;
  const int gl = g.gl, gbase = g.gbase;
  const i64 slot = g.slot(xcd_block());     // an XCD's eighth of the processing order, as the pooling of cn5 / cn7 takes
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
      if (k[t] >= 0) f[t] = c.probe(k[t], c1, c2);
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {             // ascending position order: tile t, then lane
      unsigned long long m = lane_group_mask<LPE>(f[t] != 0, gbase);
      while (m) {
        int bsel[CN8_UNR];
        lane_group_take(m, bsel);
        unsigned ff[CN8_UNR];
        float4 x[CN8_UNR][NV];
#pragma unroll
        for (int u = 0; u < CN8_UNR; ++u) {
          const int sl = lane_group_src(gbase, bsel[u]);
          const int32_t kk = __shfl(k[t], sl, OCN_WAVE);
          ff[u] = bsel[u] < 0 ? 0u : (unsigned)__shfl((int)f[t], sl, OCN_WAVE);
          lane_group_row<LPE>(bsel[u], kk, h4, rowq, gl, x[u]);
        }
#pragma unroll
        for (int u = 0; u < CN8_UNR; ++u) {
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const f32x4 xv = {x[u][v].x, x[u][v].y, x[u][v].z, x[u][v].w};
            if (ff[u] & OCN_F_CN1) acc1[v] = acc1[v] + xv;
            if (ff[u] & OCN_F_CN2) acc2[v] = acc2[v] + xv;
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
  float4 out1[NV], out2[NV];                // (pool_store takes the float4 struct)
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    out1[v] = make_float4(acc1[v].x, acc1[v].y, acc1[v].z, acc1[v].w);
    out2[v] = make_float4(acc2[v].x, acc2[v].y, acc2[v].z, acc2[v].w);
  }
  pool_store<LPE, NV>(e, i, j, gl, h4, rowq, out1, out2, xcn1, xcn2, xij);
}

extern "C" {

int ocn_cn8_pool(const int64_t* rowptrA, const int32_t* colA,
                 const int64_t* rowptrT1, const int32_t* colT1,
                 const int64_t* rowptrT2, const int32_t* colT2,
                 const uint32_t* bitmapT1, int64_t bm1_stride_words,
                 const uint32_t* bitmapT2, int64_t bm2_stride_words,
                 const int64_t* src, const int64_t* dst, const int64_t* order, int64_t B, int64_t n_cols,
                 const float* h, int32_t H, float* xcn1, float* xcn2, float* xij,
                 int32_t* cnt1, int32_t* cnt2, void* stream) {
  if (B < 0 || n_cols < 0) return OCN_EINVAL;
  if (!lane_group_width(H)) return OCN_EINVAL;
  if (!rowptrA || !colA || !src || !dst || !h || !xcn1 || !xcn2 || !xij || !cnt1 || !cnt2) return OCN_EINVAL;
  if (!set_operand_ok(bitmapT1, bm1_stride_words, rowptrT1, colT1, n_cols)) return OCN_EINVAL;
  if (!set_operand_ok(bitmapT2, bm2_stride_words, rowptrT2, colT2, n_cols)) return OCN_EINVAL;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_CN8(LPE, NV)                                                                                 \
  hipLaunchKernelGGL((cn8_pool_kernel<LPE, NV>), dim3(lane_group_blocks(B, LPE)), dim3(OCN_BLOCK), 0, st,   \
                     (const i64*)rowptrA, colA, (const i64*)rowptrT1, colT1, (const i64*)rowptrT2, colT2,   \
                     (const unsigned*)bitmapT1, (i64)bm1_stride_words, (const unsigned*)bitmapT2,           \
                     (i64)bm2_stride_words, (const i64*)src, (const i64*)dst, (const i64*)order, (i64)B, h, \
                     (int)H, xcn1, xcn2, xij, cnt1, cnt2)
  OCN_SWITCH_WIDTH(H, LAUNCH_CN8)
#undef LAUNCH_CN8
  return launch_status();
}

}  // extern "C"
