// Per-common-neighbour attribution of a candidate batch: the sampled dense-dense product on the CN pattern.
// For every flagged entry (e, k) of the intersection pass — neighbour k of src[e] with a non-zero flag byte — the two inner
// products <h[k], g1[e]> and <h[k], g2[e]>, scaled by the entry's pooling weights (wa, wb): the share of member k in
// <g1[e], xcn1[e]> and <g2[e], xcn2[e]>, where xcn1 / xcn2 are what ocn_cn_gather pools with the same flags and table.
// The entry weights are entry_weights() of common.h and the fetch rule is the pooling's (h[k] is read exactly when wa != 0 or
// wb != 0).  No atomics, no workspace, no LDS.  See include/ocn_hip.h (ocn_cn_attribution).
#include "lane_group.h"

constexpr int ATTR_UNR = 4;   // embedding rows in flight per lane group

// The lane-group walk of lane_group.h; a lane keeps its part of g1[e] and g2[e] in registers for the whole row.  A round covers
// LPE * PT positions of the source row: every lane reads the flag byte, the column id and the walk count of its own positions
// and forms their (wa, wb).  For every entry that is fetched, every lane forms its partial dots over its own features (ascending,
// one fused multiply-add each), the group sums them with an xor butterfly — every lane ends with the same bits, and the order
// of the additions depends on (LPE, NV), that is on H, only — and the lane that owns the position keeps the result.  After the
// round every lane stores its own positions.  A hub row only takes more rounds.
template <int LPE, int NV>
__global__ __launch_bounds__(OCN_BLOCK) void cn_attr_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA, const i64* __restrict__ src,
    const i64* __restrict__ order, i64 B, const i64* __restrict__ off, const uint8_t* __restrict__ flags,
    const int32_t* __restrict__ wc, i64 flags_cap, const float4* __restrict__ weights, const float* __restrict__ h, int H,
    const float* __restrict__ g1, const float* __restrict__ g2, float2* __restrict__ attr, float* __restrict__ rank) {
  constexpr int PT = lane_group<LPE>::PT;
  const lane_group<LPE> g;
  const int gl = g.gl, gbase = g.gbase;
  const i64 slot = g.slot(xcd_block());
  if (slot >= B) return;                    // whole group leaves together
  const i64 e = order ? order[slot] : slot;
  const i64 i = src[e];
  const i64 a0 = rowptrA[i], da = rowptrA[i + 1] - a0;
  const i64 q0 = off[e];
  if (q0 < 0) return;                       // offsets of a scan that gave up (OCN_SCAN_POISON): nothing to write
  const float4* h4 = reinterpret_cast<const float4*>(h);
  const i64 rowq = H >> 2;                  // float4 per row
  f32x4 ga[NV], gb[NV];
  {
    const float4* p1 = reinterpret_cast<const float4*>(g1) + e * rowq + gl;
    const float4* p2 = reinterpret_cast<const float4*>(g2) + e * rowq + gl;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float4 a = p1[v * LPE], b = p2[v * LPE];
      ga[v] = f32x4{a.x, a.y, a.z, a.w};
      gb[v] = f32x4{b.x, b.y, b.z, b.w};
    }
  }
  for (i64 p0 = 0; p0 < da; p0 += LPE * PT) {
    int32_t k[PT];
    unsigned f[PT];
    float cv[PT];
    bool own[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      const i64 p = p0 + t * LPE + gl;
      own[t] = p < da && q0 + p < flags_cap;
      f[t] = own[t] ? (unsigned)flags[q0 + p] : 0u;
      k[t] = own[t] ? colA[a0 + p] : 0;
      cv[t] = (own[t] && wc) ? (float)wc[q0 + p] : 1.0f;
    }
    float wa[PT], wb[PT], r1[PT], r2[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      wa[t] = wb[t] = r1[t] = r2[t] = 0.f;
      if (f[t]) entry_weights(f[t], weights[k[t]], cv[t], wa[t], wb[t]);
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      const bool need = (wa[t] != 0.f) | (wb[t] != 0.f);
      unsigned long long m = lane_group_mask<LPE>(need, gbase);
      while (m) {
        int bsel[ATTR_UNR];
        lane_group_take(m, bsel);
        float4 x[ATTR_UNR][NV];
#pragma unroll
        for (int u = 0; u < ATTR_UNR; ++u) {
          const int sl = lane_group_src(gbase, bsel[u]);
          const int32_t kk = __shfl(k[t], sl, OCN_WAVE);
          lane_group_row<LPE>(bsel[u], kk, h4, rowq, gl, x[u]);
        }
#pragma unroll
        for (int u = 0; u < ATTR_UNR; ++u) {
          if (bsel[u] >= 0) {
            float d1 = 0.f, d2 = 0.f;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
              d1 = __fmaf_rn(x[u][v].x, ga[v].x, d1);
              d1 = __fmaf_rn(x[u][v].y, ga[v].y, d1);
              d1 = __fmaf_rn(x[u][v].z, ga[v].z, d1);
              d1 = __fmaf_rn(x[u][v].w, ga[v].w, d1);
              d2 = __fmaf_rn(x[u][v].x, gb[v].x, d2);
              d2 = __fmaf_rn(x[u][v].y, gb[v].y, d2);
              d2 = __fmaf_rn(x[u][v].z, gb[v].z, d2);
              d2 = __fmaf_rn(x[u][v].w, gb[v].w, d2);
            }
#pragma unroll
            for (int o = LPE / 2; o > 0; o >>= 1) {   // the group is converged here: m is the same in all of its lanes
              d1 = __fadd_rn(d1, __shfl_xor(d1, o, OCN_WAVE));
              d2 = __fadd_rn(d2, __shfl_xor(d2, o, OCN_WAVE));
            }
            if (gl == bsel[u]) {
              r1[t] = wa[t] != 0.f ? __fmul_rn(wa[t], d1) : 0.f;
              r2[t] = wb[t] != 0.f ? __fmul_rn(wb[t], d2) : 0.f;
            }
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      if (own[t]) {
        const i64 q = q0 + p0 + t * LPE + gl;
        attr[q] = make_float2(r1[t], r2[t]);
        rank[q] = f[t] ? __fadd_rn(r1[t], r2[t]) : -__builtin_inff();
      }
    }
  }
}

extern "C" {

int ocn_cn_attribution(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* order, int64_t B,
                       const int64_t* off, const uint8_t* flags, const int32_t* wc, int64_t flags_cap, const float* weights,
                       const float* h, int32_t H, const float* g1, const float* g2, float* attr, float* rank, void* stream) {
  if (B < 0 || flags_cap < 0) return OCN_EINVAL;
  if (!lane_group_width(H)) return OCN_EINVAL;
  if (!rowptrA || !colA || !src || !off || !flags || !weights || !h || !g1 || !g2 || !attr || !rank) return OCN_EINVAL;
  if ((((uintptr_t)weights | (uintptr_t)h | (uintptr_t)g1 | (uintptr_t)g2) & 15u) != 0) return OCN_EINVAL;
  if (((uintptr_t)attr & 7u) != 0) return OCN_EINVAL;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_ATTR(LPE, NV)                                                                                            \
  hipLaunchKernelGGL((cn_attr_kernel<LPE, NV>), dim3(lane_group_blocks(B, LPE)), dim3(OCN_BLOCK), 0, st,                \
                     (const i64*)rowptrA, colA, (const i64*)src, (const i64*)order, (i64)B, (const i64*)off, flags, wc, \
                     (i64)flags_cap, reinterpret_cast<const float4*>(weights), h, (int)H, g1, g2,                       \
                     reinterpret_cast<float2*>(attr), rank)
  OCN_SWITCH_WIDTH(H, LAUNCH_ATTR)
#undef LAUNCH_ATTR
  return launch_status();
}

}  // extern "C"
