// Shared primitives of the libocn_hip.so translation units (gfx950, wave64, 256-thread workgroups).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ocn_hip.h"

#define OCN_WAVE 64
#define OCN_BLOCK 256
#define OCN_WPB (OCN_BLOCK / OCN_WAVE)

typedef long long i64;
typedef unsigned long long u64;

// hist[c] = {packed, walks}: packed = n1 | n2 << 21 | n_union << 42 (one 64-bit atomic per CN entry
// instead of three 32-bit ones), walks = sum of the walk counts of column c (valued cn2 only).
#define HF_BITS 21
#define HF_MASK ((1ull << HF_BITS) - 1ull)
__device__ __forceinline__ int hf_n1(u64 w) { return (int)(w & HF_MASK); }
__device__ __forceinline__ int hf_n2(u64 w) { return (int)((w >> HF_BITS) & HF_MASK); }
__device__ __forceinline__ int hf_nu(u64 w) { return (int)((w >> (2 * HF_BITS)) & HF_MASK); }

// ---------------------------------------------------------------------------------------------
// the contract between the intersection pass (cn_flags.hip; scan.hip starts the records) and the pooling (cn_pool.hip,
// cn_pool_h16.hip): the slot record — slot_rec.h, all of it — and the schedule: its cost unit, its groups, and when a
// visiting order exists and is followed (sched_followed, below lane_group_epb)
// ---------------------------------------------------------------------------------------------
// a group's cost: the largest entry count among its four candidates (a wave walks one candidate), in buckets of 32 —
// measured at the collab shape (pooling): sum / max and 4 .. 256-entry buckets all land within
// 0.184 - 0.200 ms against 0.206 unscheduled; coarse buckets keep more of the source order's L2 locality
#define SCHED_COST(t, c) ((t) > (c) ? (t) : (c))
constexpr int SCHED_SHIFT = 5;
constexpr int POOL_LPE = 64;    /* lanes per candidate of the H = 256 pooling (64: one candidate per wave) */
#define SCHED_GROUP OCN_SCHED_GROUP    /* slots per scheduling group: a workgroup of the intersection pass == one of the H = 256 pooling */
static_assert(SCHED_GROUP == OCN_WPB, "a schedule group is a workgroup's waves, one slot each");

// cn5 / cn6: nip = innerprod / scale from the column statistics word (cn5_column_stats: 0 = no union entry,
// -1 = union entries but no column with n1 >= 2, else min{n1 >= 2} - INT_MAX - 1); model.py:2370-2376
__device__ __forceinline__ float cn5_nip(int sc, float ip) {
  float scale;
  if (sc == 0) scale = 1.0f;                                        // empty union vector
  else if (sc == -1) scale = 0.0f;                                  // only singleton columns: every ncn1 value is 0
  else scale = 1.0f / (float)(sc + 0x7fffffff + 1);                 // largest 1/S1 among columns with S1 >= 2
  return scale > 0.0f ? ip / scale : ip;
}

static inline int launch_status() { return (int)hipGetLastError(); }

// status words of a candidate batch (ocn_hip.h): [0] = this batch's error bits, [3] = the same bits, sticky — the library
// only ever ORs into it, the caller clears it when it has read it (a scoring loop reads it once per split, not per batch)
__device__ __forceinline__ void status_raise(int32_t* status, i64 total, i64 cap) {
  const int bits = total < 0 ? OCN_ST_SCAN : (total > cap ? OCN_ST_CAP : 0);
  if (bits) { atomicOr(status, bits); atomicOr(status + 3, bits); }
}

static inline int grid_for(i64 items_per_block_units, i64 cap = (1 << 20)) {
  i64 g = items_per_block_units < 1 ? 1 : items_per_block_units;
  return (int)(g > cap ? cap : g);
}

// H -> (LPE lanes per row, NV float4 per lane) of the kernels whose lane groups own a row of H = LPE * NV * 4 features:
// M(LPE, NV) launches the instance; any other width is refused (host code)
#define OCN_SWITCH_WIDTH(H, M)           \
  switch (H) {                           \
    case 16:  M(4, 1); break;            \
    case 32:  M(8, 1); break;            \
    case 64:  M(16, 1); break;           \
    case 128: M(32, 1); break;           \
    case 256: M(64, 1); break;           \
    case 512: M(64, 2); break;           \
    default: return OCN_EINVAL;          \
  }

// ... and the host checks that the entries of those kernels share (lane_group.h has the device side)
static inline bool lane_group_width(int H) { return H == 16 || H == 32 || H == 64 || H == 128 || H == 256 || H == 512; }
// candidates per workgroup, and the workgroups of a batch of B
constexpr i64 lane_group_epb(int lpe) { return (i64)OCN_WPB * (OCN_WAVE / lpe); }
static inline unsigned lane_group_blocks(i64 B, int lpe) { return (unsigned)((B + lane_group_epb(lpe) - 1) / lane_group_epb(lpe)); }
// The schedule's rule.  A batch of B slots is sched_groups(B) groups; ocn_gather_schedule orders them where every XCD's
// eighth is the same whole number of groups, at most SCHED_MAX_EIGHTH (the counting sort's ranks are 16-bit) ...
constexpr i64 SCHED_EIGHTHS = OCN_SCHED_EIGHTHS, SCHED_MAX_EIGHTH = OCN_SCHED_MAX_EIGHTH;
static inline i64 sched_groups(i64 B) { return (B + SCHED_GROUP - 1) / SCHED_GROUP; }
// ... and a pooling launch with `lpe` lanes per candidate follows `perm` where it reads the slot records and its workgroups
// are those groups (the intersection pass's workgroups); else nullptr.  (The kernels test gridDim.x & 7 themselves.)
static inline const int32_t* sched_followed(const int32_t* perm, const void* rec, i64 B, int lpe) {
  return perm && rec && lane_group_epb(lpe) == SCHED_GROUP && sched_groups(B) % SCHED_EIGHTHS == 0 ? perm : nullptr;
}
// a T1 / T2 operand: bit rows that cover n_cols columns, or both CSR arrays
static inline bool set_operand_ok(const void* bitmap, i64 stride_words, const void* rowptr, const void* col, i64 n_cols) {
  return bitmap ? stride_words * 32 >= n_cols : (rowptr && col);
}

// ---------------------------------------------------------------------------------------------
// wave / block primitives
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, OCN_WAVE);
  return v;
}

// inclusive scan across the 64 lanes of a wave
__device__ __forceinline__ i64 wave_incl_scan(i64 v, int lane) {
#pragma unroll
  for (int o = 1; o < OCN_WAVE; o <<= 1) {
    i64 t = __shfl_up(v, o, OCN_WAVE);
    if (lane >= o) v += t;
  }
  return v;
}

// lane l's 64-bit value (i64 / u64) in every lane, as a scalar: two 32-bit readlanes
template <typename T>
__device__ __forceinline__ T wave_readlane64(T v, int l) {
  static_assert(sizeof(T) == 8, "wave_readlane64: a 64-bit integer");
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l), hi = __builtin_amdgcn_readlane((unsigned)((u64)v >> 32), l);
  return (T)(((u64)hi << 32) | lo);
}

// a value every lane of the wave holds alike, moved to scalar registers (the loads it addresses become scalar too)
__device__ __forceinline__ i64 wave_uniform(i64 v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(u64)v), hi = __builtin_amdgcn_readfirstlane((unsigned)((u64)v >> 32));
  return (i64)(((u64)hi << 32) | lo);
}

// exclusive scan of one value per thread over a 256-thread block; returns the thread's prefix and
// the block total.  `sh` is 2*OCN_WPB i64 of LDS.
__device__ __forceinline__ i64 block_excl_scan(i64 v, i64* sh, i64* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  i64 inc = wave_incl_scan(v, lane);
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  i64 base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < OCN_WPB; ++i) {
    i64 s = sh[i];
    if (i < w) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// orders a wave's own LDS writes before its own LDS reads (and the reverse, for the next item's writes): LDS executes a
// wave's instructions in order, so only the compiler has to be kept from moving them
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Workgroups are dealt round-robin over the 8 XCDs (each with its own L2).  The candidates are visited in source-node
// order, so give every XCD one contiguous eighth of that order: candidates with neighbouring sources then share an L2
// instead of being spread over all eight.  Returns the workgroup's place in that order (blockIdx.x where the grid is
// no multiple of eight).
__device__ __forceinline__ i64 xcd_block() {
  i64 bid = blockIdx.x;
  if ((gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);
  return bid;
}

// ---------------------------------------------------------------------------------------------
// sorted-list membership
// ---------------------------------------------------------------------------------------------
// Branch-uniform binary search over a[0..n) (global or LDS): every lane of a wave searches the same
// row, so the trip count is wave-uniform and the top levels of the tree are shared cache lines.
template <typename P>
__device__ __forceinline__ bool sorted_has(P a, i64 n, int32_t key) {
  i64 lo = 0, hi = n;
  bool found = false;
  while (lo < hi) {
    const i64 mid = (lo + hi) >> 1;
    const int32_t v = a[mid];
    found |= (v == key);
    if (v < key) lo = mid + 1; else hi = mid;
  }
  return found;
}

// ---------------------------------------------------------------------------------------------
// walk-count route: which endpoint enumerates the 2-walks of a candidate edge (i, j)
// ---------------------------------------------------------------------------------------------
// cn2[e,k] = |N(k) ∩ N(j)| for k in N(i) is the number of 2-walks j -> m -> k.  "Forward" sweeps the
// rows N(k), k in N(i) (nds[i] = Σ_{k∈N(i)} d_k probes against N(j)); "reverse" sweeps the rows N(m),
// m in N(j) (nds[j] probes against N(i); its hits land through global atomics, each 64-chunk of N(j)
// sets up N(i)'s bitmap again, and the row is finalised by the forward kernel's items afterwards).
// A hub source with a modest target is 10-100x cheaper from the target's side.
#define WALK_CHUNK 64        /* rows (neighbours of i) per forward work item */
#define WALK_REV_CHUNK 16    /* rows (neighbours of j) per reverse work item: few items, so finer ones */
// Forward work items take `walk_group()` consecutive 64-row chunks of the source row, so that an item
// sweeps about WALK_ITEM_ELEMS elements: a light row (most of a batch) is one item instead of one per
// 64 neighbours — the per-item set-up (ticket, slot search, row pointers, N(j) bitmap) is what such
// items cost — while a hub row still spreads over many workgroups.
constexpr int WALK_ITEM_ELEMS = 16384;
#define WALK_GROUP_MAX 8      /* chunks per forward item: one per wave of the 512-thread workgroup */
__device__ __forceinline__ i64 walk_group(const i64* __restrict__ nds, i64 i, i64 di) {
  const i64 chunks = (di + WALK_CHUNK - 1) / WALK_CHUNK;
  if (!nds || chunks <= 1) return 1;
  const i64 per_chunk = nds[i] / chunks + 1;
  i64 cg = WALK_ITEM_ELEMS / per_chunk;
  if (cg > WALK_GROUP_MAX) cg = WALK_GROUP_MAX;
  return cg < 1 ? 1 : (cg > chunks ? chunks : cg);
}

// bit of a node in the per-candidate sweeps' Bloom bitmap (cn_walk.hip; walk_group.hip hands it to the host: ocn_walk_hash)
constexpr int WALK_BM_BITS = 17;
__host__ __device__ __forceinline__ unsigned walk_bit(int32_t v) { return ((unsigned)v * 2654435761u) >> (32 - WALK_BM_BITS); }

// batch slot of a work item: last slot with item_off[slot] <= item (item_off[0] = 0 <= item <
// item_off[B]).  Called by one whole wave: 64 probes per round instead of a dependent chain of
// log2(B) single loads (2 rounds for B = 2048, 3 for 65 536).  (cn_walk.hip, cn3_flags.hip: the items of ocn_chunk_offsets)
__device__ __forceinline__ i64 walk_item_slot(const i64* __restrict__ item_off, i64 B, i64 item, int lane) {
  i64 lo = 0, hi = B;                        // item_off[lo] <= item < item_off[hi]
  while (hi - lo > 1) {
    const i64 step = (hi - lo + OCN_WAVE - 1) / OCN_WAVE;
    const i64 idx = lo + (i64)(lane + 1) * step;
    const bool le = idx < hi && item_off[idx] <= item;
    const int c = __popcll(__ballot(le));
    lo += (i64)c * step;
    hi = lo + step < hi ? lo + step : hi;
  }
  return lo;
}

__device__ __forceinline__ bool walk_reverse(const i64* __restrict__ nds, i64 i, i64 j, i64 di, i64 dj) {
  if (!nds || dj == 0 || di == 0) return false;
  const i64 chunks_j = (dj + WALK_REV_CHUNK - 1) / WALK_REV_CHUNK;
  const i64 rev = 2 * nds[j] + di * chunks_j + 2 * di;
  return rev < nds[i];
}

// Two accumulators that take the same x: (a.x, a.y) += (w.x, w.y) * x on the packed-f32 pipe (v_pk_mul_f32 +
// v_pk_add_f32: one issue slot for both) — product and sum rounded separately, component for component what the two
// scalar statements a1 = a1 + w1 * x; a2 = a2 + w2 * x compute.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));      // register arrays carried across loop iterations: the native
                                                              // vector type is kept in registers where an array of the
                                                              // float4 struct ends up in scratch
__device__ __forceinline__ void axpy_pair(f32x2& a, const f32x2 w, const float x) {
#pragma clang fp contract(off)
  const f32x2 xx = {x, x};
  const f32x2 p = w * xx;
  a = a + p;
}
// The same for sums whose x comes out of LDS one float at a time (chain_rows).  There the form above compiles to
// `v_pk_mul_f32 v[w:w+1], v[x:x+1] op_sel_hi:[1,0]` — the pair's high register is never written, the instruction only names it — and
// the H = 64 wave kernel (all 64 lanes summing) returned wrong .x sums in lanes 48..63 about once in a hundred batches whenever
// another kernel ran beside it (a scoring loop's heads on a second stream): DESIGN.md section 6, tools/loop_race_check.py.  The empty
// asm makes both halves of the pair real registers (one v_mov per entry): an in-kernel recheck of every sum found 0 disagreements in
// 3 600 batches where the form above had ~50; two scalar chains are as clean and 5 % slower on the ppa / citation2 steps.
__device__ __forceinline__ void axpy_pair_lds(f32x2& a, const f32x2 w, const float x) {
#pragma clang fp contract(off)
  f32x2 xx = {x, x};
  asm volatile("" : "+v"(xx));
  const f32x2 p = w * xx;
  a = a + p;
}

__device__ __forceinline__ void axpy4(float4& acc, float w, const float4& x) {
  acc.x = __fadd_rn(acc.x, __fmul_rn(w, x.x));
  acc.y = __fadd_rn(acc.y, __fmul_rn(w, x.y));
  acc.z = __fadd_rn(acc.z, __fmul_rn(w, x.z));
  acc.w = __fadd_rn(acc.w, __fmul_rn(w, x.w));
}

// per-entry pooling weights from the flag byte, the column's {w1, t, inv2} and the cn2 value c (model.py:2380-2427)
__device__ __forceinline__ void entry_weights(unsigned f, const float4& w, float c, float& wa, float& wb) {
  wa = (f & OCN_F_CN1) ? w.x : 0.f;
  const float v = __fsub_rn((f & OCN_F_CN2) ? c : 0.f, (f & OCN_F_CN1) ? w.y : 0.f);
  wb = __fmul_rn(v, w.z);
}

// ---------------------------------------------------------------------------------------------
// fp32 operands on the bf16 matrix pipe (linear.hip, wgrad.hip)
// ---------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ float bf16_to_f32(__bf16 v) {
  return __builtin_bit_cast(float, (unsigned)__builtin_bit_cast(unsigned short, v) << 16);
}

// x = p1 + p2 + p3 (+ O(2^-27 |x|)), each term a bf16 (round to nearest even)
__device__ __forceinline__ void split3(float x, __bf16& p1, __bf16& p2, __bf16& p3) {
  p1 = (__bf16)x;
  const float r1 = x - bf16_to_f32(p1);
  p2 = (__bf16)r1;
  const float r2 = r1 - bf16_to_f32(p2);
  p3 = (__bf16)r2;
}

