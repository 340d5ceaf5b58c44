// The pooling of cn5 / cn7 / cn8 from an int8 embedding table — the image a retrieval index already keeps (int8 rows of
// `row_stride` bytes and one fp32 scale per row, ops.quantize_rows_i8) — exact or capped: ocn_cn_gather_q8.  A row costs H
// bytes instead of H * 4: at H = 256 one 256-byte request per lane group where bf16 takes two and fp32 four.  An element is
// v = fl32(float(q) * scale[k]) — int8 -> fp32 is exact, the product is ONE rounded fp32 multiply, subnormal results kept —
// and from there the term is the fp32 pooling's: one separately rounded multiply by the entry weight and one add, in ascending
// position.  So with D = float(q[:, :H]) * scale[:, None] the three output rows are, bit for bit, those of ocn_cn_gather on D
// (cap == 0) and, with `mult`, those of ocn_cn_gather_cap on D (cap >= 1).  The scale is never folded into the weights: that
// would move a rounding.  See include/ocn_hip.h.
//
// ONE form serves every row length, the form of cn_gather_h16_kernel: the lane-group walk of lane_group.h, LPE lanes per
// candidate, NV * 4 consecutive features per lane (OCN_SWITCH_WIDTH) — NV dwords of a row, one load; a hub row is walked by
// its lane group in more rounds.  The lane that owns a position fetches its column's scale beside its weights, and the scale
// travels to the group with the column id: a row stays one vector-memory request per lane.  CAPPED adds the sample of
// cn_gather_cap_kernel (cap_multiplier, philox.h: one rule for both).  No atomics, no LDS, no workspace.
#include "lane_group.h"
#include "philox.h"
#include "slot_rec.h"

constexpr int Q8_UNR = 4;                    // embedding rows in flight per lane group (eight where a wave has one candidate)

// A lane's piece of a row: its NV * 4 consecutive features as NV dwords of four bytes each — one 4-byte (H <= 256) or 8-byte
// (H = 512) load.  Byte b of dword c is feature 4c + b.
template <int NV>
struct q8_piece { typedef unsigned type __attribute__((ext_vector_type(NV))); };
template <>
struct q8_piece<1> { typedef unsigned type; };

template <int NV>
__device__ __forceinline__ unsigned q8_word(const typename q8_piece<NV>::type& x, int c) {
  if constexpr (NV == 1) return x; else return x[c];
}

// byte b of w, sign-extended and widened exactly (v_bfe_i32 + v_cvt_f32_i32, or the byte-select form of the convert),
// times the row's scale: one IEEE multiply
__device__ __forceinline__ float q8_elem(unsigned w, int b, float scale) {
  const int q = ((int)(w << (24 - 8 * b))) >> 24;
  return __fmul_rn((float)q, scale);
}

// The arguments are ocn_cn_gather's (cn_gather_kernel, cn_pool.hip) without `rowsum`; q8: [N] rows of row_stride bytes, the
// first H of them the row; scale: [N].  CAPPED: then the sample's, as cn_gather_cap_kernel.
template <int LPE, int NV, bool CAPPED, int UNR = (LPE >= 64 ? 2 * Q8_UNR : Q8_UNR)>
__global__ __launch_bounds__(OCN_BLOCK) void cn_gather_q8_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const i64* __restrict__ off, const uint8_t* __restrict__ flags, const int32_t* __restrict__ wc,
    const float4* __restrict__ weights, const int8_t* __restrict__ q8, i64 row_stride, const float* __restrict__ scale,
    float* __restrict__ xcn1, float* __restrict__ xcn2, float* __restrict__ xij,
    const i64* __restrict__ out_row, const int32_t* __restrict__ cnt1, const int32_t* __restrict__ cnt2,
    const u64* __restrict__ rec, const int32_t* __restrict__ perm,
    int cap, u64 seed, int32_t* __restrict__ mult) {
  typedef typename q8_piece<NV>::type piece;
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
  const char* hp = reinterpret_cast<const char*>(q8) + gl * NQ;      // this lane's piece of row 0
  f32x2 acc[NQ];                             // {xcn1, xcn2} pairs of the lane's features
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = f32x2{0.f, 0.f};
  if (has1 | has2) {                         // a candidate with neither kind of entry is not walked
    // ---- CAPPED: the member count u, where the row is long enough for the cap to matter: the flag bytes alone
    i64 u = 0;
    if constexpr (CAPPED) {
      if (da > cap) {
        int c = 0;
        for (i64 p = gl; p < da; p += LPE) c += flags[base + p] != 0;
#pragma unroll
        for (int o = LPE >> 1; o > 0; o >>= 1) c += __shfl_xor(c, o, OCN_WAVE);      // (stays inside the aligned lane group)
        u = c;
      }
    }
    const bool sampled = CAPPED && u > cap;
    const bool narrow = ((u64)u + 1) * (u64)cap <= 0xffffffffull;      // the strata's products fit 32 bits (every real batch)
    i64 rank0 = 0;                           // members in front of the current tile
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
      float wa[PT], wb[PT], sc[PT];
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        wa[t] = wb[t] = 0.f; sc[t] = 0.f;
        if (f[t]) {
          entry_weights(f[t], weights[k[t]], (float)cv[t], wa[t], wb[t]);
          sc[t] = scale[k[t]];
        }
      }
#pragma unroll
      for (int t = 0; t < PT; ++t) {           // ascending position order: tile t, then lane
        if constexpr (CAPPED) {
          // ---- the entry's multiplier: 1 for a member of a candidate within the cap, else its stratum's size or 0
          const bool member = f[t] != 0;
          int32_t s = member ? 1 : 0;
          if (sampled) {                       // (a lane group's branch, like the walk itself: the ballot is cut to the group)
            const unsigned long long mm = lane_group_mask<LPE>(member, gbase);
            const i64 r = rank0 + __popcll(mm & ((1ull << gl) - 1ull));
            rank0 += __popcll(mm);
            if (member)
              s = narrow ? cap_multiplier<unsigned>((unsigned)r, (unsigned)u, (unsigned)cap, (unsigned)i, (unsigned)j, seed)
                         : cap_multiplier<u64>((u64)r, (u64)u, (u64)cap, (unsigned)i, (unsigned)j, seed);
          }
          if (mult) {
            const i64 p = p0 + t * LPE + gl;
            if (p < da) mult[base + p] = s;
          }
          wa[t] = __fmul_rn(wa[t], (float)s);
          wb[t] = __fmul_rn(wb[t], (float)s);
        }
        const bool need = (wa[t] != 0.f) | (wb[t] != 0.f);
        unsigned long long m = lane_group_mask<LPE>(need, gbase);
        while (m) {
          int bsel[UNR];
          lane_group_take(m, bsel);
          float wwa[UNR], wwb[UNR], ssc[UNR];
          piece x[UNR];
#pragma unroll
          for (int q = 0; q < UNR; ++q) {
            const int sl = lane_group_src(gbase, bsel[q]);
            const int32_t kk = __shfl(k[t], sl, OCN_WAVE);
            wwa[q] = __shfl(wa[t], sl, OCN_WAVE);
            wwb[q] = __shfl(wb[t], sl, OCN_WAVE);
            ssc[q] = __shfl(sc[t], sl, OCN_WAVE);
            if (bsel[q] >= 0) x[q] = *reinterpret_cast<const piece*>(hp + (i64)kk * row_stride);
          }
#pragma unroll
          for (int q = 0; q < UNR; ++q) {
            if (bsel[q] >= 0) {
              const f32x2 w = {wwa[q], wwb[q]};
#pragma unroll
              for (int c = 0; c < NV; ++c) {
                const unsigned word = q8_word<NV>(x[q], c);
#pragma unroll
                for (int b = 0; b < 4; ++b)
                  // (a dequantised element is a lone register, like chain_rows' LDS reads: the form of common.h that makes
                  // both halves of the multiplicand pair real registers)
                  axpy_pair_lds(acc[4 * c + b], w, q8_elem(word, b, ssc[q]));
              }
            }
          }
        }
      }
    }
  } else if (CAPPED && mult) {               // not walked: no members, and its positions are written all the same
    for (i64 p = gl; p < da; p += LPE) mult[base + p] = 0;
  }
  const i64 oe = out_row ? out_row[e] : e;
  const bool st1 = !out_row || has1, st2 = !out_row || has1 || has2;      // rows the class-major heads never read stay unwritten
  const piece xi = *reinterpret_cast<const piece*>(hp + i * row_stride);
  const piece xj = *reinterpret_cast<const piece*>(hp + j * row_stride);
  const float si = scale[i], sj = scale[j];
  float4* o1 = reinterpret_cast<float4*>(xcn1) + (oe * LPE + gl) * NV;
  float4* o2 = reinterpret_cast<float4*>(xcn2) + (oe * LPE + gl) * NV;
  float4* o3 = reinterpret_cast<float4*>(xij) + (oe * LPE + gl) * NV;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const unsigned wi = q8_word<NV>(xi, v), wj = q8_word<NV>(xj, v);
    const float4 a = make_float4(q8_elem(wi, 0, si), q8_elem(wi, 1, si), q8_elem(wi, 2, si), q8_elem(wi, 3, si));
    const float4 b = make_float4(q8_elem(wj, 0, sj), q8_elem(wj, 1, sj), q8_elem(wj, 2, sj), q8_elem(wj, 3, sj));
    pool_emit(o1 + v, o2 + v, o3 + v, make_float4(acc[4 * v].x, acc[4 * v + 1].x, acc[4 * v + 2].x, acc[4 * v + 3].x),
              make_float4(acc[4 * v].y, acc[4 * v + 1].y, acc[4 * v + 2].y, acc[4 * v + 3].y), a, b, st1, st2);
  }
}

extern "C" {

int ocn_cn_gather_q8(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                     const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flags, const int32_t* wc,
                     const float* weights, const int8_t* q8, int64_t row_stride, const float* scale, int32_t H,
                     int64_t max_row_len, float* xcn1, float* xcn2, float* xij, const int64_t* out_row, const int32_t* cnt1,
                     const int32_t* cnt2, const uint64_t* rec, const int32_t* perm, int32_t cap, uint64_t seed, int32_t* mult,
                     void* stream) {
  (void)max_row_len;                         // one form for every row length
  if (B < 0 || cap < 0 || (cap == 0 && mult) || !lane_group_width(H)) return OCN_EINVAL;
  if (row_stride < H || (row_stride & 15)) return OCN_EINVAL;
  if (B == 0) return 0;                      // (as ocn_cn_gather: an empty batch's tensors have no storage, its pointers are NULL)
  if (!rowptrA || !colA || !src || !dst || !off || !flags || !weights || !q8 || !scale || !xcn1 || !xcn2 || !xij)
    return OCN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_Q8_FORM(LPE, NV, CAPPED)                                                                                      \
  hipLaunchKernelGGL((cn_gather_q8_kernel<LPE, NV, CAPPED>), dim3(blocks), dim3(OCN_BLOCK), 0, st, (const i64*)rowptrA, colA, \
                     (const i64*)src, (const i64*)dst, (const i64*)order, (i64)B, (const i64*)off, flags, wc,                \
                     (const float4*)weights, q8, (i64)row_stride, scale, xcn1, xcn2, xij, (const i64*)out_row, cnt1, cnt2,   \
                     (const u64*)rec, sched, (int)cap, (u64)seed, mult)
#define LAUNCH_Q8(LPE, NV)                                                                               \
  {                                                                                                      \
    const unsigned blocks = lane_group_blocks(B, LPE);                                                   \
    const int32_t* sched = sched_followed(perm, rec, B, LPE);      /* the schedule to follow, or nullptr (common.h) */ \
    if (cap) LAUNCH_Q8_FORM(LPE, NV, true); else LAUNCH_Q8_FORM(LPE, NV, false);                         \
  }
  OCN_SWITCH_WIDTH(H, LAUNCH_Q8)
#undef LAUNCH_Q8
#undef LAUNCH_Q8_FORM
  return launch_status();
}

}  // extern "C"
