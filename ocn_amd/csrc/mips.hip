// Embedding retrieval: for every query the m nodes with the largest int8 inner product against it, over ALL nodes — an exact
// brute-force short list that is not bound to the graph neighbourhood ("Embedding retrieval").  It is an
// int8 GEMM on v_mfma_i32_32x32x32_i8 whose epilogue keeps m keys per query instead of writing a [Q][N] matrix.
//
// The keys are the A operand (rows of the accumulator tile), the queries the B operand (its columns): a lane then holds ONE
// query's products with 16 keys, so the query's current m-th best is one register of that lane.  A wave owns 32 queries — their
// fragments stay in registers for H = 64, 128, 256 — and their sorted lists of m 64-bit keys (topk_key with the node id in the
// low word) in LDS; nothing is shared between waves, so the kernel has no barrier.  The four waves of a workgroup stream the
// same contiguous slice of the key range, 32 keys at a time, the next tile's fragments and scales loaded ahead of the current
// tile's tests.  An accumulator is converted (exact: |dot| < 2^24), scaled (the one rounding) and compared with the query's
// threshold: a tile in which nothing passes costs that compare per element and one ballot.  What passes is checked for
// eligibility by its own lane (the source itself, a binary search in the source's row of M: the lanes' searches overlap), then
// compared as a key with the query's m-th best — kept in a register of the query's lane — and inserted by the whole wave, two list
// slots per lane at the most: an insertion is one round trip to LDS.  The threshold only ever drops a key that m better ones of
// the same query precede, and keys are distinct: the list after the slice is the m best of the slice whatever the order of the
// insertions.  n_split slices leave
// partial lists in the workspace; mips_merge_kernel selects the m best of a query's n_split * m keys as segment_topk does.
// See include/ocn_hip.h (ocn_mips_topm_i8).
#include "common.h"
#include "topk_key.h"
#include "window_sweep.h"     // ws_raise_lds_once

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

constexpr int MIPS_H_ALIGN = 64;                             // two 32-deep MFMA steps
constexpr int MIPS_H_MAX = 1024;                             // |dot| <= 1024 * 127^2 < 2^24: the conversion to fp32 is exact
constexpr int MIPS_QW = 32;                                  // queries of a wave: the columns of one accumulator tile
constexpr int MIPS_QT = MIPS_QW * OCN_WPB;                   // ... of a workgroup
constexpr int MIPS_KT = 32;                                  // keys of a tile: the rows of one accumulator tile
constexpr int MIPS_TARGET_WG = 256;                          // workgroups the automatic split aims at per 128 KiB of lists: one per CU
constexpr int MIPS_MIN_TILES = 64;                           // ... with at least this many tiles per slice
constexpr int MIPS_MAX_SPLIT = 64;

// the value a key was made from (-0.0 comes back as +0.0, a NaN as a NaN); the key of an empty slot gives a NaN as well
__device__ __forceinline__ float mips_key_val(u64 key) {
  const unsigned u = (unsigned)(key >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// the row of the tile that accumulator register j of lane half hh holds
__device__ __forceinline__ int mips_acc_row(int j, int hh) { return (j & 3) + 8 * (j >> 2) + 4 * hh; }

// One key that beats the m-th best of the list L (LDS, NS * 64 slots, sorted, best first, 0 = empty) is inserted by the whole
// wave: every lane shifts its one or two slots.  Returns the list's m-th best afterwards, read from the lane that holds it.
template <int NS>
__device__ __forceinline__ u64 mips_insert(u64* L, int m, u64 nk, int lane) {
  u64 nv[NS];
#pragma unroll
  for (int r = 0; r < NS; ++r) {
    const int j = r * OCN_WAVE + lane;
    const u64 v = L[j], up = j ? L[j - 1] : ~0ull;
    nv[r] = v > nk ? v : (up > nk ? nk : up);
  }
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r < NS; ++r) L[r * OCN_WAVE + lane] = nv[r];
  wave_lds_sync();
  const u64 last = (NS == 2 && m > OCN_WAVE) ? nv[NS - 1] : nv[0];
  return wave_readlane64(last, (m - 1) & 63);
}

// KS > 0: H == 64 * KS and the query fragments stay in registers; KS == 0: any H, both operands are loaded per step.
// NS: list slots per lane (m <= 64 * NS).  Workgroup b serves query tile b / n_split and key slice b % n_split.
template <int KS, int NS>
__global__ __launch_bounds__(OCN_BLOCK) void mips_topm_kernel(
    const int8_t* __restrict__ query, const int8_t* __restrict__ keys, const float* __restrict__ kscale, i64 Q, i64 N, int H,
    const i64* __restrict__ rows, const i64* __restrict__ rowptrM, const int32_t* __restrict__ colM, int drop_self, int m,
    int n_split, i64 per, float* __restrict__ top_val, i64* __restrict__ top_node, u64* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) u64 mips_lds[];
  constexpr int LS = NS * OCN_WAVE;                          // slots of a list
  constexpr int NF = KS > 0 ? 2 * KS : 1;                    // fragments of an operand row kept in registers
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int rr = lane & 31, hh = lane >> 5;
  const i64 qt = (i64)blockIdx.x / n_split;
  const int slice = (int)((i64)blockIdx.x % n_split);
  const i64 q0 = qt * MIPS_QT + (i64)w * MIPS_QW;            // this wave's first query
  if (q0 >= Q) return;                                       // (no barrier below: waves are independent)
  u64* lists = mips_lds + (size_t)w * MIPS_QW * LS;
  for (int t = lane; t < MIPS_QW * LS; t += OCN_WAVE) lists[t] = 0ull;
  wave_lds_sync();
  const i64 n_beg = (i64)slice * per, n_end = n_beg + per < N ? n_beg + per : N;
  const bool qvalid = q0 + rr < Q;
  const int8_t* qp = query + (qvalid ? q0 + rr : Q - 1) * (i64)H + 16 * hh;
  i32x4 bq[NF];
  if (KS > 0) {
#pragma unroll
    for (int s = 0; s < NF; ++s) bq[s] = *reinterpret_cast<const i32x4*>(qp + 32 * s);
  }
  // this lane's query: its m-th best as a key and as a value (a NaN at first: nothing is below it, everything passes until the
  // list is full), its source and the source's row of M — the tests below touch no global memory but that row
  u64 thrk = 0ull;
  float thrf = mips_key_val(0ull);
  i64 my_s = -1, my_m0 = 0, my_dm = 0;
  if (rows && qvalid) {
    my_s = rows[q0 + rr];
    if (colM && my_s >= 0 && my_s < N) {
      my_m0 = rowptrM[my_s];
      my_dm = rowptrM[my_s + 1] - my_m0;
    }
  }
  i32x4 a[NF];
  float ks[16];
  // the operands of the tile at `base`: key row base + rr (clamped: a row past N is never offered), the 16 scales of this lane's rows
  auto load_tile = [&](i64 base) {
    const i64 krow = base + rr < N ? base + rr : N - 1;
    const int8_t* kp = keys + krow * (i64)H + 16 * hh;
    if (KS > 0) {
#pragma unroll
      for (int s = 0; s < NF; ++s) a[s] = *reinterpret_cast<const i32x4*>(kp + 32 * s);
    }
    if (base + MIPS_KT <= N) {                               // (base is a multiple of 32 and kscale 16-byte aligned)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(kscale + base + 8 * g + 4 * hh);
        ks[4 * g] = v.x; ks[4 * g + 1] = v.y; ks[4 * g + 2] = v.z; ks[4 * g + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const i64 node = base + mips_acc_row(j, hh);
        ks[j] = kscale[node < N ? node : N - 1];
      }
    }
  };
  if (n_beg < n_end) load_tile(n_beg);
  for (i64 base = n_beg; base < n_end; base += MIPS_KT) {
    i32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0;
    if (KS > 0) {
#pragma unroll
      for (int s = 0; s < NF; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bq[s], acc, 0, 0, 0);
    } else {
      const i64 krow = base + rr < N ? base + rr : N - 1;
      const int8_t* kp = keys + krow * (i64)H + 16 * hh;
      for (int k = 0; k < H; k += 32)
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*reinterpret_cast<const i32x4*>(kp + k), *reinterpret_cast<const i32x4*>(qp + k),
                                                    acc, 0, 0, 0);
    }
    float val[16];
    bool any = false;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      val[j] = __fmul_rn((float)acc[j], ks[j]);
      any |= !(val[j] < thrf);
    }
    if (base + MIPS_KT < n_end) load_tile(base + MIPS_KT);   // the next tile's loads fly during the tests below
    if (__ballot(any && qvalid) == 0ull) continue;
    unsigned pm = 0u;                                        // bit j: register j passes the value test
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (qvalid && base + mips_acc_row(j, hh) < n_end && !(val[j] < thrf)) pm |= 1u << j;
    if (rows) {                                              // eligibility, every lane for its own few: the searches overlap
      unsigned t = pm;
      while (t) {
        const int j = __ffs((int)t) - 1;
        t &= t - 1;
        const i64 node = base + mips_acc_row(j, hh);
        if ((drop_self && node == my_s) || (my_dm > 0 && sorted_has(colM + my_m0, my_dm, (int32_t)node))) pm &= ~(1u << j);
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const u64 key = topk_key(val[j], (unsigned)(base + mips_acc_row(j, hh)));
      u64 mb = __ballot((pm >> j) & 1u);
      while (mb) {                                           // (the same trips in every lane)
        const int sl = __ffsll((long long)mb) - 1;
        mb &= mb - 1;
        const int c = sl & 31;
        const u64 nk = wave_readlane64(key, sl);
        if (nk <= wave_readlane64(thrk, c)) continue;        // (an earlier key of this tile has raised the query's threshold)
        const u64 thr = mips_insert<NS>(lists + c * LS, m, nk, lane);
        if (rr == c) { thrk = thr; thrf = mips_key_val(thr); }
      }
    }
  }
  // the lists: straight to the output where there is one slice, else to this slice's place among the query's partial lists
  for (int c = 0; c < MIPS_QW && q0 + c < Q; ++c) {
    const i64 q = q0 + c;
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      const int j = r * OCN_WAVE + lane;
      if (j >= m) continue;
      const u64 key = lists[c * LS + j];
      if (n_split > 1) {
        part[(q * n_split + slice) * (i64)m + j] = key;
      } else {
        top_val[q * m + j] = key ? mips_key_val(key) : -__builtin_inff();
        top_node[q * m + j] = key ? (i64)(0xffffffffu - (unsigned)key) : -1;
      }
    }
  }
}

// The m best of a query's n_split partial lists (n_split * m keys, 0 = empty): a wave owns a query and keeps the running best
// sorted across its lanes, as segment_topk_kernel does with the keys it makes itself.
template <int NS>
__global__ __launch_bounds__(OCN_BLOCK) void mips_merge_kernel(const u64* __restrict__ part, i64 Q, int m, int n_split,
                                                               float* __restrict__ top_val, i64* __restrict__ top_node) {
  const int lane = threadIdx.x & 63;
  const int kl = (m - 1) & 63;
  const i64 total = (i64)n_split * m;
  for (i64 q = (i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6); q < Q; q += (i64)gridDim.x * OCN_WPB) {
    const u64* src = part + q * total;
    u64 v[NS];
#pragma unroll
    for (int r = 0; r < NS; ++r) v[r] = 0ull;
    u64 thr = 0ull;
    for (i64 c0 = 0; c0 < total; c0 += OCN_WAVE) {
      const i64 p = c0 + lane;
      const u64 key = p < total ? src[p] : 0ull;
      u64 mb = __ballot(key > thr);
      while (mb) {
        const int sl = __ffsll((long long)mb) - 1;
        mb &= mb - 1;
        const u64 nk = wave_readlane64(key, sl);
        if (nk <= thr) continue;
        u64 up[NS];
#pragma unroll
        for (int r = 0; r < NS; ++r) up[r] = topk_shfl_up1(v[r]);
        if (NS == 2) { const u64 carry = wave_readlane64(v[0], 63); if (lane == 0) up[NS - 1] = carry; }
        if (lane == 0) up[0] = ~0ull;
#pragma unroll
        for (int r = 0; r < NS; ++r) v[r] = v[r] > nk ? v[r] : (up[r] > nk ? nk : up[r]);
        thr = wave_readlane64(v[NS - 1], kl);
      }
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      const int j = r * OCN_WAVE + lane;
      if (j < m) {
        top_val[q * m + j] = v[r] ? mips_key_val(v[r]) : -__builtin_inff();
        top_node[q * m + j] = v[r] ? (i64)(0xffffffffu - (unsigned)v[r]) : -1;
      }
    }
  }
}

// (keys per slice, slices) of a call: the requested or automatic split, no more slices than 32-key tiles, none empty
static inline void mips_resolve_split(int64_t Q, int64_t N, int32_t m, int32_t n_split, int64_t* per, int32_t* slices) {
  const int64_t tiles = (N + MIPS_KT - 1) / MIPS_KT, qtiles = (Q + MIPS_QT - 1) / MIPS_QT;
  int64_t ns = n_split;
  if (ns == 0) {
    const int64_t target = MIPS_TARGET_WG * (m <= OCN_WAVE ? 2 : 1);     // (lists of 64 slots: two workgroups fit a CU's LDS)
    ns = (target + (qtiles > 0 ? qtiles : 1) - 1) / (qtiles > 0 ? qtiles : 1);
    const int64_t by_len = tiles / MIPS_MIN_TILES;
    if (ns > by_len) ns = by_len;
    if (ns > MIPS_MAX_SPLIT) ns = MIPS_MAX_SPLIT;
    if (ns < 1) ns = 1;
  }
  if (ns > tiles) ns = tiles;
  const int64_t tiles_per = (tiles + ns - 1) / ns;
  *per = tiles_per * MIPS_KT;
  *slices = (int32_t)((tiles + tiles_per - 1) / tiles_per);
}

static inline int mips_sizes_bad(int64_t Q, int64_t N, int32_t m, int32_t n_split) {
  return Q < 0 || N < 1 || N >= ((int64_t)1 << 31) || m < 1 || m > TOPK_MAX || n_split < 0;
}

template <int KS, int NS>
static int mips_launch(const int8_t* query, const int8_t* keys, const float* kscale, int64_t Q, int64_t N, int32_t H,
                       const int64_t* rows, const int64_t* rowptrM, const int32_t* colM, int32_t drop_self, int32_t m,
                       int32_t slices, int64_t per, float* top_val, int64_t* top_node, void* workspace, void* stream) {
  static std::atomic<unsigned long long> lds_raised{0ull};   // (one per instance)
  constexpr size_t lds = (size_t)MIPS_QT * NS * OCN_WAVE * sizeof(u64);
  if (const int rc = ws_raise_lds_once((const void*)mips_topm_kernel<KS, NS>, lds, lds_raised)) return rc;
  const int64_t grid = (Q + MIPS_QT - 1) / MIPS_QT * slices;
  hipLaunchKernelGGL((mips_topm_kernel<KS, NS>), dim3((unsigned)grid), dim3(OCN_BLOCK), lds, (hipStream_t)stream, query, keys,
                     kscale, (i64)Q, (i64)N, (int)H, (const i64*)rows, (const i64*)rowptrM, colM, (int)drop_self, (int)m,
                     (int)slices, (i64)per, top_val, (i64*)top_node, (u64*)workspace);
  int rc = launch_status();
  if (rc || slices == 1) return rc;
  hipLaunchKernelGGL((mips_merge_kernel<NS>), dim3((unsigned)grid_for((Q + OCN_WPB - 1) / OCN_WPB, 256 * 8)), dim3(OCN_BLOCK), 0,
                     (hipStream_t)stream, (const u64*)workspace, (i64)Q, (int)m, (int)slices, top_val, (i64*)top_node);
  return launch_status();
}

extern "C" {

int32_t ocn_mips_max_m(void) { return TOPK_MAX; }
int32_t ocn_mips_h_align(void) { return MIPS_H_ALIGN; }

int64_t ocn_mips_workspace_bytes(int64_t Q, int64_t N, int32_t m, int32_t n_split) {
  if (mips_sizes_bad(Q, N, m, n_split)) return OCN_EINVAL;
  int64_t per;
  int32_t slices;
  mips_resolve_split(Q, N, m, n_split, &per, &slices);
  const int64_t bytes = slices > 1 ? Q * slices * m * (int64_t)sizeof(u64) : 0;
  return bytes > 8 ? bytes : 8;
}

int ocn_mips_topm_i8(const int8_t* query, const int8_t* keys, const float* kscale, int64_t Q, int64_t N, int32_t H,
                     const int64_t* rows, const int64_t* rowptrM, const int32_t* colM, int32_t drop_self, int32_t m,
                     int32_t n_split, float* top_val, int64_t* top_node, void* workspace, void* stream) {
  if (!query || !keys || !kscale || !top_val || !top_node || !workspace) return OCN_EINVAL;
  if (mips_sizes_bad(Q, N, m, n_split)) return OCN_EINVAL;
  if (H < MIPS_H_ALIGN || H > MIPS_H_MAX || (H % MIPS_H_ALIGN)) return OCN_EINVAL;
  if ((rowptrM == nullptr) != (colM == nullptr) || (rowptrM && !rows)) return OCN_EINVAL;
  if ((((uintptr_t)query) & 15u) || (((uintptr_t)keys) & 15u) || (((uintptr_t)kscale) & 15u) || (((uintptr_t)workspace) & 7u))
    return OCN_EINVAL;                                       // (fragments and scales are read 16 bytes at a time)
  if (Q == 0) return 0;
  int64_t per;
  int32_t slices;
  mips_resolve_split(Q, N, m, n_split, &per, &slices);
  if ((Q + MIPS_QT - 1) / MIPS_QT * slices >= ((int64_t)1 << 31)) return OCN_EINVAL;
#define MIPS_GO(KS)                                                                                                          \
  return m <= OCN_WAVE ? mips_launch<KS, 1>(query, keys, kscale, Q, N, H, rows, rowptrM, colM, drop_self, m, slices, per,   \
                                            top_val, top_node, workspace, stream)                                           \
                       : mips_launch<KS, 2>(query, keys, kscale, Q, N, H, rows, rowptrM, colM, drop_self, m, slices, per,   \
                                            top_val, top_node, workspace, stream)
  switch (H) {
    case 64: MIPS_GO(1);
    case 128: MIPS_GO(2);
    case 256: MIPS_GO(4);
    default: MIPS_GO(0);
  }
#undef MIPS_GO
}

}  // extern "C"
