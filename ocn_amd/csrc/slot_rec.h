// The slot record: what the intersection pass (cn_flags.hip; scan.hip's scatter starts it) hands the pooling (cn_pool.hip,
// cn_pool_h16.hip) about a processing slot, in OCN_REC_WORDS 64-bit words.  include/ocn_hip.h (ocn_cn_flags `rec`) lays it out
// and names its shifts and bits; every pack, load and field of one is here.  Two kernels keep their decode statements in
// their own bodies, field by field — cn_flags_kernel's record-fed start and cn_gather_pair_kernel, which say why — and
// take the fields, or at least the constants, from here like everyone else.
#pragma once
#include "common.h"

static_assert(OCN_REC_WORDS == 4, "slot record: two 16-byte halves");
#define REC_LEN_MASK ((1ull << OCN_REC_LEN_SHIFT) - 1)      /* word 2: the row start */
#define REC_BASE_MASK ((1ull << OCN_REC_FULL2_BIT) - 1)     /* word 3: the flag offset */
typedef const u64 (&rec_words)[OCN_REC_WORDS];

// ---- packing
__device__ __forceinline__ u64 rec_word1(i64 i, i64 j) { return (u64)i | ((u64)j << 32); }
__device__ __forceinline__ u64 rec_word2(i64 a0, i64 da) { return (u64)a0 | ((u64)da << OCN_REC_LEN_SHIFT); }
// the finished word 3: full2 = (da > 0 && cnt2 == da), has1 = cnt1 > 0, has2 = cnt2 > 0.  (The caller forms the three from its
// counts: with the comparisons in here, cn_flags_kernel<true, false, false, 2> came out with two scalar registers swapped.)
__device__ __forceinline__ u64 rec_word3(i64 base, bool full2, bool has1, bool has2) {
  return (u64)base | ((u64)full2 << OCN_REC_FULL2_BIT) | ((u64)has1 << OCN_REC_HAS1_BIT) | ((u64)has2 << OCN_REC_HAS2_BIT);
}
// words 0 - 2 (the intersection pass without a prep pass in front of it)
__device__ __forceinline__ void rec_pack_head(u64* r, i64 e, i64 i, i64 j, i64 a0, i64 da) {
  r[0] = (u64)e;
  r[1] = rec_word1(i, j);
  r[2] = rec_word2(a0, da);
}
// the started record (the prep pass's scatter): words 0 - 2 and the bare flag offset, two 16-byte stores
__device__ __forceinline__ void rec_pack_started(u64* r, i64 e, i64 i, i64 j, i64 a0, i64 da, i64 base) {
  ulonglong2* r2 = reinterpret_cast<ulonglong2*>(r);
  r2[0] = make_ulonglong2((u64)e, rec_word1(i, j));
  r2[1] = make_ulonglong2(rec_word2(a0, da), (u64)base);
}

// ---- loading
__device__ __forceinline__ u64* rec_at(u64* rec, i64 slot) { return rec + OCN_REC_WORDS * slot; }
// one slot: two 16-byte loads
__device__ __forceinline__ void rec_load(const u64* rec, i64 slot, u64 (&w)[OCN_REC_WORDS]) {
  const ulonglong2* rp = reinterpret_cast<const ulonglong2*>(rec + OCN_REC_WORDS * slot);
  const ulonglong2 ra = rp[0], rb = rp[1];
  w[0] = ra.x; w[1] = ra.y; w[2] = rb.x; w[3] = rb.y;
}
// NS consecutive slots from slot0 on: lane l loads word l of them — ONE load for all slots, in two registers (a 32-byte load
// per slot would hold 8 NS) — zero for a slot past the batch's end ...
template <int NS>
__device__ __forceinline__ u64 rec_load_spread(const u64* rec, i64 slot0, i64 B, int lane) {
  u64 recw = 0;
  if (lane < OCN_REC_WORDS * NS && slot0 + lane / OCN_REC_WORDS < B) recw = rec[OCN_REC_WORDS * slot0 + lane];
  return recw;
}
// ... and slot s's words, read from their lanes into scalars
__device__ __forceinline__ void rec_spread_words(u64 recw, int s, u64 (&w)[OCN_REC_WORDS]) {
#pragma unroll
  for (int q = 0; q < OCN_REC_WORDS; ++q)
    w[q] = (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)recw, OCN_REC_WORDS * s + q) |
           ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(recw >> 32), OCN_REC_WORDS * s + q) << 32);
}

// ---- the fields
__device__ __forceinline__ i64 rec_row(rec_words w) { return (i64)w[0]; }                                  // batch row e
__device__ __forceinline__ i64 rec_src(rec_words w) { return (i64)(w[1] & 0xffffffffull); }                // endpoints i, j
__device__ __forceinline__ i64 rec_dst(rec_words w) { return (i64)(w[1] >> 32); }
__device__ __forceinline__ i64 rec_start(rec_words w) { return (i64)(w[2] & REC_LEN_MASK); }               // N(i) in colA: a0, da
__device__ __forceinline__ i64 rec_len(rec_words w) { return (i64)(w[2] >> OCN_REC_LEN_SHIFT); }
// the flag offset of a STARTED record: word 3 whole — the scatter sets no bit above the offset, and a mask would be one more
// instruction per slot ...
__device__ __forceinline__ i64 rec_base_started(rec_words w) { return (i64)w[3]; }
// ... and of a finished one, under its three bits
__device__ __forceinline__ i64 rec_base(rec_words w) { return (i64)(w[3] & REC_BASE_MASK); }
__device__ __forceinline__ bool rec_has1(rec_words w) { return (w[3] >> OCN_REC_HAS1_BIT) & 1ull; }
__device__ __forceinline__ bool rec_has2(rec_words w) { return w[3] >> OCN_REC_HAS2_BIT; }
__device__ __forceinline__ bool rec_full2(rec_words w) { return (w[3] >> OCN_REC_FULL2_BIT) & 1ull; }

// ---- a finished record, whole (the one-slot poolings).  Fields in the order the kernels were measured with: the machine
// code follows it.
struct slot_rec {
  i64 e, i, j, a0, da, base;                 // batch row, endpoints, start and length of N(i) in colA, flag offset
  bool has1, has2, full2;                    // cnt1 > 0, cnt2 > 0, cnt2 == da > 0
};
__device__ __forceinline__ slot_rec rec_unpack_finished(rec_words w) {
  slot_rec r;
  r.e = rec_row(w); r.i = rec_src(w); r.j = rec_dst(w);
  r.a0 = rec_start(w); r.da = rec_len(w);
  r.base = rec_base(w); r.has1 = rec_has1(w); r.has2 = rec_has2(w);
  r.full2 = rec_full2(w);
  return r;
}
// ... read from its slot
__device__ __forceinline__ slot_rec rec_read_finished(const u64* rec, i64 slot) {
  u64 w[OCN_REC_WORDS];
  rec_load(rec, slot, w);
  return rec_unpack_finished(w);
}
