// The pooling of cn5 / cn7 / cn8 from a half-precision embedding table (bf16 or f16 rows, fp32 sums): ocn_cn_gather_h16.
// What changes against cn_pool.hip is what a row costs — H * 2 bytes instead of H * 4, and half the resident table — and
// nothing else: bf16 -> fp32 and f16 -> fp32 are exact, the entry weights, the accumulators and the outputs are fp32, and every
// term is one separately rounded multiply and one add in ascending column order.  So the three output rows of a candidate
// are, bit for bit, what ocn_cn_gather leaves for the same table widened to fp32.  See include/ocn_hip.h.
//
// ONE form serves every row length: the lane-group walk of lane_group.h, the geometry of cn_gather_kernel (LPE lanes per
// candidate, NV * 4 features per lane, OCN_SWITCH_WIDTH).  A hub row (more than 1 024 entries) is walked by its lane group
// like any other row, only in more rounds — the order is the strictly sequential one by construction, and no second launch,
// LDS slab or workgroup-per-row pass exists here.  (The fp32 pooling's hub forms buy memory parallelism for such rows; what they
// would buy a half table has not been measured: DESIGN.md section 4, half-precision tables.)
#include "lane_group.h"
#include "slot_rec.h"

constexpr int H16_UNR = 4;                   // embedding rows in flight per lane group (eight where a wave has one candidate)

// A lane's piece of a row: its NV * 4 consecutive features as NV * 2 words of two elements each — one 8-byte (H <= 256) or
// 16-byte (H = 512) load.  Word c holds features 2c (low half) and 2c + 1 (high half).
template <int NV>
struct h16_piece { typedef unsigned type __attribute__((ext_vector_type(2 * NV))); };

// both elements of a word, widened exactly (bf16 is the high half of an fp32; f16 goes through v_cvt_f32_f16, which keeps
// subnormals: they are normal numbers in fp32)
template <int FMT>
__device__ __forceinline__ void h16_widen(unsigned w, float& lo, float& hi) {
  if constexpr (FMT == 0) {
    lo = __builtin_bit_cast(float, w << 16);
    hi = __builtin_bit_cast(float, w & 0xffff0000u);
  } else {
    lo = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
    hi = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
  }
}

// The arguments are ocn_cn_gather's (cn_gather_kernel, cn_pool.hip) without `rowsum`.  h16: [N][H] 2-byte elements.
template <int LPE, int NV, int FMT, int UNR = (LPE >= 64 ? 2 * H16_UNR : H16_UNR)>
__global__ __launch_bounds__(OCN_BLOCK) void cn_gather_h16_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const i64* __restrict__ off, const uint8_t* __restrict__ flags, const int32_t* __restrict__ wc,
    const float4* __restrict__ weights, const void* __restrict__ h16,
    float* __restrict__ xcn1, float* __restrict__ xcn2, float* __restrict__ xij,
    const i64* __restrict__ out_row, const int32_t* __restrict__ cnt1, const int32_t* __restrict__ cnt2,
    const u64* __restrict__ rec, const int32_t* __restrict__ perm) {
  typedef typename h16_piece<NV>::type piece;
  constexpr int PT = lane_group<LPE>::PT;
  constexpr int NQ = NV * 4;                 // features per lane
  const lane_group<LPE> g;
  const int gl = g.gl, gbase = g.gbase;
  i64 bid = xcd_block();                     // an XCD's eighth of the source order ...
  if (perm && (gridDim.x & 7) == 0) bid = perm[bid];      // ... and inside it the schedule's order (longest groups first)
  const i64 slot = g.slot(bid);
  if (slot >= B) return;                     // whole group leaves together
  i64 e, i, j, a0, da, base;
  bool has1, has2;
  if (rec) {                                 // the intersection pass's 32-byte slot record (slot_rec.h)
    const slot_rec r = rec_read_finished(rec, slot);
    e = r.e; i = r.i; j = r.j; a0 = r.a0; da = r.da;
    base = r.base; has1 = r.has1; has2 = r.has2;
  } else {
    e = order ? order[slot] : slot;
    i = src[e]; j = dst[e];
    a0 = rowptrA[i]; da = rowptrA[i + 1] - a0;
    base = off[e];
    has1 = !cnt1 || cnt1[e] > 0; has2 = !cnt2 || cnt2[e] > 0;
  }
  const piece* hp = reinterpret_cast<const piece*>(h16) + gl;      // this lane's piece of row 0; a row is LPE pieces
  f32x2 acc[NQ];                             // {xcn1, xcn2} pairs of the lane's features
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = f32x2{0.f, 0.f};
  if (has1 | has2) {                         // a candidate with neither kind of entry is not walked
    for (i64 p0 = 0; p0 < da; p0 += LPE * PT) {
      int32_t k[PT];
      unsigned f[PT];
      int32_t cv[PT];
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        const i64 p = p0 + t * LPE + gl;
        k[t] = 0; f[t] = 0; cv[t] = 1;
        if (p < da) {
          k[t] = colA[a0 + p]; f[t] = flags[base + p];
          if (wc) cv[t] = wc[base + p];
        }
      }
      float wa[PT], wb[PT];
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        wa[t] = wb[t] = 0.f;
        if (f[t]) entry_weights(f[t], weights[k[t]], (float)cv[t], wa[t], wb[t]);
      }
#pragma unroll
      for (int t = 0; t < PT; ++t) {           // ascending position order: tile t, then lane
        const bool need = (wa[t] != 0.f) | (wb[t] != 0.f);
        unsigned long long m = lane_group_mask<LPE>(need, gbase);
        while (m) {
          int bsel[UNR];
          lane_group_take(m, bsel);
          float wwa[UNR], wwb[UNR];
          piece x[UNR];
#pragma unroll
          for (int u = 0; u < UNR; ++u) {
            const int sl = lane_group_src(gbase, bsel[u]);
            const int32_t kk = __shfl(k[t], sl, OCN_WAVE);
            wwa[u] = __shfl(wa[t], sl, OCN_WAVE);
            wwb[u] = __shfl(wb[t], sl, OCN_WAVE);
            if (bsel[u] >= 0) x[u] = hp[(i64)kk * LPE];
          }
#pragma unroll
          for (int u = 0; u < UNR; ++u) {
            if (bsel[u] >= 0) {
              const f32x2 w = {wwa[u], wwb[u]};
#pragma unroll
              for (int c = 0; c < 2 * NV; ++c) {
                float lo, hi;
                h16_widen<FMT>(x[u][c], lo, hi);
                // (a widened element is a lone register, like chain_rows' LDS reads: the form of common.h that makes both
                // halves of the multiplicand pair real registers)
                axpy_pair_lds(acc[2 * c], w, lo);
                axpy_pair_lds(acc[2 * c + 1], w, hi);
              }
            }
          }
        }
      }
    }
  }
  const i64 oe = out_row ? out_row[e] : e;
  const bool st1 = !out_row || has1, st2 = !out_row || has1 || has2;      // rows the class-major heads never read stay unwritten
  const piece xi = hp[i * LPE], xj = hp[j * LPE];
  float4* o1 = reinterpret_cast<float4*>(xcn1) + (oe * LPE + gl) * NV;
  float4* o2 = reinterpret_cast<float4*>(xcn2) + (oe * LPE + gl) * NV;
  float4* o3 = reinterpret_cast<float4*>(xij) + (oe * LPE + gl) * NV;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    float4 a, b;
    h16_widen<FMT>(xi[2 * v], a.x, a.y); h16_widen<FMT>(xi[2 * v + 1], a.z, a.w);
    h16_widen<FMT>(xj[2 * v], b.x, b.y); h16_widen<FMT>(xj[2 * v + 1], b.z, b.w);
    pool_emit(o1 + v, o2 + v, o3 + v, make_float4(acc[4 * v].x, acc[4 * v + 1].x, acc[4 * v + 2].x, acc[4 * v + 3].x),
              make_float4(acc[4 * v].y, acc[4 * v + 1].y, acc[4 * v + 2].y, acc[4 * v + 3].y), a, b, st1, st2);
  }
}

extern "C" {

int ocn_cn_gather_h16(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                      const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flags, const int32_t* wc,
                      const float* weights, const void* h16, int32_t fmt, int32_t H, int64_t max_row_len, float* xcn1,
                      float* xcn2, float* xij, const int64_t* out_row, const int32_t* cnt1, const int32_t* cnt2,
                      const uint64_t* rec, const int32_t* perm, void* stream) {
  (void)max_row_len;                         // one form for every row length
  if (B < 0 || !lane_group_width(H) || (fmt != 0 && fmt != 1)) return OCN_EINVAL;
  if (B == 0) return 0;                      // (as ocn_cn_gather: an empty batch's tensors have no storage, its pointers are NULL)
  if (!rowptrA || !src || !dst || !off || !weights || !h16 || !xcn1 || !xcn2 || !xij) return OCN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_H16_FMT(LPE, NV, FMT)                                                                                        \
  hipLaunchKernelGGL((cn_gather_h16_kernel<LPE, NV, FMT>), dim3(blocks), dim3(OCN_BLOCK), 0, st, (const i64*)rowptrA, colA,  \
                     (const i64*)src, (const i64*)dst, (const i64*)order, (i64)B, (const i64*)off, flags, wc,                \
                     (const float4*)weights, h16, xcn1, xcn2, xij, (const i64*)out_row, cnt1, cnt2, (const u64*)rec, sched)
#define LAUNCH_H16(LPE, NV)                                                                              \
  {                                                                                                      \
    const unsigned blocks = lane_group_blocks(B, LPE);                                                   \
    const int32_t* sched = sched_followed(perm, rec, B, LPE);      /* the schedule to follow, or nullptr (common.h) */ \
    if (fmt == 0) LAUNCH_H16_FMT(LPE, NV, 0); else LAUNCH_H16_FMT(LPE, NV, 1);                           \
  }
  OCN_SWITCH_WIDTH(H, LAUNCH_H16)
#undef LAUNCH_H16
#undef LAUNCH_H16_FMT
  return launch_status();
}

}  // extern "C"
