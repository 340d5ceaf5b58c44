// The capped pooling of cn5 / cn7 / cn8: ocn_cn_gather_cap.  A candidate pools at most `cap` embedding rows, chosen by a
// deterministic stratified sample of its common-neighbour entries and reweighted so that the pooled vectors are unbiased
// estimates of ocn_cn_gather's; what a heavy candidate costs the pooling is then bounded whatever its degree.  The sample
// (include/ocn_hip.h states it in full): the members — positions with a non-zero flag byte — are ranked r = 0 .. u - 1 in
// ascending position; for u > cap = d the ranks are cut into d strata [ceil(t u / d), ceil((t + 1) u / d)), one rank per
// stratum is drawn with Philox4x32-10 under the counter (i, j, t, SAMPLE_STREAM_CN_CAP), and the drawn member is pooled with
// its entry weights times the stratum's size.  It is fixed by (seed, i, j, the candidate's flags) and by nothing else of
// the batch.  A candidate with u <= d is pooled exactly: the multiplier is 1, x * 1.0f is exact, every bit is ocn_cn_gather's.
//
// ONE form serves every row length, the form of cn_gather_h16_kernel: the lane-group walk of lane_group.h, LPE lanes per
// candidate, NV float4 per lane (OCN_SWITCH_WIDTH); a hub row is walked by its lane group in more rounds.  A candidate
// whose source row has at most `cap` entries cannot exceed the cap and takes the walk at once.  Any other is first counted:
// one pass over its flag bytes alone.  The walk then carries the running member rank (the group ballot's bits below the
// lane) and turns (wa, wb) into (wa s, wb s) or (0, 0); order, arithmetic and fetch rule are those of ocn_cn_gather.  The
// picks are evaluated per member (a lane holds one position of a tile, so a tile costs one Philox evaluation per wave, not
// per entry).  No atomics, no workspace, no LDS.
#include "lane_group.h"
#include "philox.h"
#include "slot_rec.h"

constexpr int CAP_UNR = 4;                   // embedding rows in flight per lane group (eight where a wave has one candidate)

// The arguments are ocn_cn_gather's (cn_gather_kernel, cn_pool.hip) without `rowsum`, then the sample's.
template <int LPE, int NV, int UNR = (LPE >= 64 ? 2 * CAP_UNR : CAP_UNR)>
__global__ __launch_bounds__(OCN_BLOCK) void cn_gather_cap_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA,
    const i64* __restrict__ src, const i64* __restrict__ dst, const i64* __restrict__ order, i64 B,
    const i64* __restrict__ off, const uint8_t* __restrict__ flags, const int32_t* __restrict__ wc,
    const float4* __restrict__ weights, const float* __restrict__ h,
    float* __restrict__ xcn1, float* __restrict__ xcn2, float* __restrict__ xij,
    const i64* __restrict__ out_row, const int32_t* __restrict__ cnt1, const int32_t* __restrict__ cnt2,
    const u64* __restrict__ rec, const int32_t* __restrict__ perm,
    int cap, u64 seed, int32_t* __restrict__ mult) {
  constexpr int PT = lane_group<LPE>::PT;
  const lane_group<LPE> g;
  const int gl = g.gl, gbase = g.gbase;
  i64 bid = xcd_block();                     // an XCD's eighth of the source order ...
  if (perm && (gridDim.x & 7) == 0) bid = perm[bid];      // ... and inside it the schedule's order (an upper bound of the cost here)
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
  const float4* h4 = reinterpret_cast<const float4*>(h);
  constexpr i64 rowq = (i64)LPE * NV;        // float4 per row
  f32x2 acc[NV][4];                          // {xcn1, xcn2} pairs of the lane's features
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[v][c] = f32x2{0.f, 0.f};
  if (has1 | has2) {                         // a candidate with neither kind of entry is not walked
    // ---- the member count u, where the row is long enough for the cap to matter: the flag bytes alone
    i64 u = 0;
    if (da > cap) {
      int c = 0;
      for (i64 p = gl; p < da; p += LPE) c += flags[base + p] != 0;
#pragma unroll
      for (int o = LPE >> 1; o > 0; o >>= 1) c += __shfl_xor(c, o, OCN_WAVE);      // (stays inside the aligned lane group)
      u = c;
    }
    const bool sampled = u > cap;
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
      float wa[PT], wb[PT];
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        wa[t] = wb[t] = 0.f;
        if (f[t]) entry_weights(f[t], weights[k[t]], (float)cv[t], wa[t], wb[t]);
      }
#pragma unroll
      for (int t = 0; t < PT; ++t) {           // ascending position order: tile t, then lane
        // ---- the entry's multiplier: 1 for a member of a candidate within the cap, else its stratum's size or 0
        const bool member = f[t] != 0;
        int32_t s = member ? 1 : 0;
        if (sampled) {                         // (a lane group's branch, like the walk itself: the ballot is cut to the group)
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
        const bool need = (wa[t] != 0.f) | (wb[t] != 0.f);
        unsigned long long m = lane_group_mask<LPE>(need, gbase);
        while (m) {
          int bsel[UNR];
          lane_group_take(m, bsel);
          float wwa[UNR], wwb[UNR];
          float4 x[UNR][NV];
#pragma unroll
          for (int q = 0; q < UNR; ++q) {
            const int sl = lane_group_src(gbase, bsel[q]);
            const int32_t kk = __shfl(k[t], sl, OCN_WAVE);
            wwa[q] = __shfl(wa[t], sl, OCN_WAVE);
            wwb[q] = __shfl(wb[t], sl, OCN_WAVE);
            lane_group_row<LPE>(bsel[q], kk, h4, rowq, gl, x[q]);
          }
#pragma unroll
          for (int q = 0; q < UNR; ++q) {
            if (bsel[q] >= 0) {
              const f32x2 w = {wwa[q], wwb[q]};
#pragma unroll
              for (int v = 0; v < NV; ++v) {
                axpy_pair(acc[v][0], w, x[q][v].x);
                axpy_pair(acc[v][1], w, x[q][v].y);
                axpy_pair(acc[v][2], w, x[q][v].z);
                axpy_pair(acc[v][3], w, x[q][v].w);
              }
            }
          }
        }
      }
    }
  } else if (mult) {                         // not walked: no members, and its positions are written all the same
    for (i64 p = gl; p < da; p += LPE) mult[base + p] = 0;
  }
  float4 acc1[NV], acc2[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    acc1[v] = make_float4(acc[v][0].x, acc[v][1].x, acc[v][2].x, acc[v][3].x);
    acc2[v] = make_float4(acc[v][0].y, acc[v][1].y, acc[v][2].y, acc[v][3].y);
  }
  // rows the class-major heads never read stay unwritten: the counts are those of the full set, not of the sample
  pool_store<LPE, NV>(out_row ? out_row[e] : e, i, j, gl, h4, rowq, acc1, acc2, xcn1, xcn2, xij,
                      !out_row || has1, !out_row || has1 || has2);
}

extern "C" {

int ocn_cn_gather_cap(const int64_t* rowptrA, const int32_t* colA, const int64_t* src, const int64_t* dst,
                      const int64_t* order, int64_t B, const int64_t* off, const uint8_t* flags, const int32_t* wc,
                      const float* weights, const float* h, int32_t H, int64_t max_row_len, float* xcn1, float* xcn2,
                      float* xij, const int64_t* out_row, const int32_t* cnt1, const int32_t* cnt2, const uint64_t* rec,
                      const int32_t* perm, int32_t cap, uint64_t seed, int32_t* mult, void* stream) {
  (void)max_row_len;                         // one form for every row length
  if (B < 0 || cap < 1 || !lane_group_width(H)) return OCN_EINVAL;
  if (B == 0) return 0;                      // (as ocn_cn_gather: an empty batch's tensors have no storage, its pointers are NULL)
  if (!rowptrA || !colA || !src || !dst || !off || !flags || !weights || !h || !xcn1 || !xcn2 || !xij) return OCN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_CAP(LPE, NV)                                                                                                  \
  {                                                                                                                          \
    const unsigned blocks = lane_group_blocks(B, LPE);                                                                       \
    const int32_t* sched = sched_followed(perm, rec, B, LPE);      /* the schedule to follow, or nullptr (common.h) */       \
    hipLaunchKernelGGL((cn_gather_cap_kernel<LPE, NV>), dim3(blocks), dim3(OCN_BLOCK), 0, st, (const i64*)rowptrA, colA,     \
                       (const i64*)src, (const i64*)dst, (const i64*)order, (i64)B, (const i64*)off, flags, wc,              \
                       (const float4*)weights, h, xcn1, xcn2, xij, (const i64*)out_row, cnt1, cnt2, (const u64*)rec, sched,  \
                       (int)cap, (u64)seed, mult);                                                                           \
  }
  OCN_SWITCH_WIDTH(H, LAUNCH_CAP)
#undef LAUNCH_CAP
  return launch_status();
}

}  // extern "C"
