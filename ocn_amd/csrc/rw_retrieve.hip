// Random-walk retrieval: a source's short list from W uniform walks of 2 or 3 steps instead of its whole neighbourhood.
// c2[v] / c3[v] = the walks whose second / third step ends in v; E[c2[v]] / W = RA(s, v) / deg s and E[c3[v]] / W =
// P3_ra(s, v) / deg s, so ranking by c2 + decay * c3 estimates the ranking by the "ra" path index P2 + decay * P3
// ("Random-walk retrieval").  The cost is W * L dependent row reads per source whatever its degree: no
// candidate list of the neighbourhood, no window sweep, no hub tail.
//
// One workgroup owns a query.  Its threads run the walks w = tid, tid + 256, ..., RW_ILP of them at a time so that a step's
// three dependent loads (two row pointers, one column) of several walks are in flight together: a walk is a latency chain, not
// a stream.  Visits go into an open-addressing table in LDS — key = node id, claimed by compare-and-swap, value = c2 | c3 << 16
// added atomically — so the counts are sums of integers: they depend on neither the schedule nor the launch geometry.  The
// table has at least twice as many slots as there can be distinct visits, W * (L - 1): it cannot fill up, there is no overflow
// status.  Then the occupied slots that are neither s nor in row s of M are compacted into a list (its order is the schedule's,
// the sort below removes that), sorted by node id in LDS (rowsort.h) and written with their counts looked up in the table.
// Every walk is a function of (seed, s, w, A): Philox4x32-10 with the SOURCE id in the counter (philox.h: streams 5 and 6), so
// a source's segment does not depend on its place in the request, and the count pass and the fill pass walk the same walks.
// See include/ocn_hip.h (ocn_rw_max_walks, ocn_rw_visits_count, ocn_rw_visits_fill).
#include "common.h"
#include "philox.h"
#include "rowsort.h"
#include "window_sweep.h"     // ws_raise_lds_once

constexpr int RW_ILP = 4;                                    // walks a thread keeps in flight
constexpr int RW_MIN_SLOTS = 64, RW_MAX_SLOTS = 16384;       // table slots (a power of two): 8 bytes each, 128 KiB at the most
constexpr int RW_LDS_MAX = 160 * 1024 - 1024;                // the CU's LDS less the static words and a margin
// distinct visits a launch may have to hold: half the largest table, and what the list (4 bytes each) fits behind it
constexpr int RW_MAX_VISITS = (RW_MAX_SLOTS / 2) < ((RW_LDS_MAX - 8 * RW_MAX_SLOTS) / 4) ? (RW_MAX_SLOTS / 2)
                                                                                         : ((RW_LDS_MAX - 8 * RW_MAX_SLOTS) / 4);
constexpr int RW_MAX_WALKS = RW_MAX_VISITS / 2;              // at L = 3 a walk makes two counted visits
static_assert(RW_MAX_WALKS >= 1024 && RW_MAX_WALKS <= 65535, "the 16-bit count fields and the promised minimum");
constexpr int RW_EMPTY = -1;                                 // (node ids are non-negative int32)

// slots of the table for `visits` = W * (L - 1) possible distinct keys: the power of two at or above twice that
static inline int rw_slots(int visits) {
  int s = RW_MIN_SLOTS;
  while (s < 2 * visits) s <<= 1;
  return s;
}
static inline size_t rw_lds_bytes(int slots, int visits) { return (size_t)slots * 8 + (size_t)visits * 4; }

__device__ __forceinline__ unsigned rw_hash(int key, int shift) { return ((unsigned)key * 0x9E3779B1u) >> shift; }

// one visit: the key's slot is found or claimed (linear probing; a free slot always exists), its packed count grows by inc
__device__ __forceinline__ void rw_visit(int* keys, unsigned* vals, unsigned mask, int shift, int key, unsigned inc) {
  unsigned h = rw_hash(key, shift);
  for (;;) {
    const int old = atomicCAS(&keys[h], RW_EMPTY, key);
    if (old == RW_EMPTY || old == key) break;
    h = (h + 1) & mask;
  }
  atomicAdd(&vals[h], inc);
}

// the packed count of a key that is in the table
__device__ __forceinline__ unsigned rw_lookup(const int* keys, const unsigned* vals, unsigned mask, int shift, int key) {
  unsigned h = rw_hash(key, shift);
  while (keys[h] != key) h = (h + 1) & mask;
  return vals[h];
}

// p -> the node a step from p reaches with the word u, or -1 where the walk has ended (p < 0) or ends here (an empty row)
__device__ __forceinline__ int rw_step(const int32_t* __restrict__ col, i64 b0, i64 b1, u64 u) {
  const i64 d = b1 - b0;
  return d > 0 ? col[b0 + (i64)__umul64hi(u, (u64)d)] : -1;
}

// FILL = false: count[q] = the candidates of query q.  FILL = true: its segment is written from ptr[q] on.
// Every barrier is reached by the whole workgroup: the query loop runs on blockIdx and kernel arguments, the sort on a count
// every thread reads from LDS alike.
template <bool FILL>
__global__ __launch_bounds__(OCN_BLOCK) void rw_visits_kernel(
    const i64* __restrict__ rowptrA, const int32_t* __restrict__ colA, const i64* __restrict__ rowptrM,
    const int32_t* __restrict__ colM, i64 n_cols, const i64* __restrict__ sources, i64 Q, int walks, int length, u64 seed,
    int slots, int shift, const i64* __restrict__ ptr, float decay, int32_t* __restrict__ count, longlong2* __restrict__ edges,
    float* __restrict__ val, int2* __restrict__ visits) {
  extern __shared__ __attribute__((aligned(16))) unsigned rw_lds[];
  __shared__ int s_n;
  int* keys = reinterpret_cast<int*>(rw_lds);
  unsigned* vals = rw_lds + slots;
  int32_t* list = reinterpret_cast<int32_t*>(rw_lds + 2 * slots);
  const unsigned mask = (unsigned)slots - 1u;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  for (i64 q = blockIdx.x; q < Q; q += gridDim.x) {
    const i64 s = sources[q];
    const bool valid = s >= 0 && s < n_cols;                 // (an id out of range has no walks and no candidates)
    for (int t = threadIdx.x; t < slots; t += OCN_BLOCK) { keys[t] = RW_EMPTY; vals[t] = 0u; }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const i64 a0 = valid ? rowptrA[s] : 0, da = valid ? rowptrA[s + 1] - a0 : 0;
    if (da > 0) {
      const unsigned s_lo = (unsigned)(u64)s, s_hi = (unsigned)((u64)s >> 32);
      for (int w0 = threadIdx.x; w0 < walks; w0 += OCN_BLOCK * RW_ILP) {
        int p[RW_ILP];
        u64 u2[RW_ILP], u3[RW_ILP];
        i64 b0[RW_ILP], b1[RW_ILP];
#pragma unroll
        for (int j = 0; j < RW_ILP; ++j) {                   // step 1: every walk leaves s
          const int w = w0 + j * OCN_BLOCK;
          p[j] = -1; u2[j] = 0; u3[j] = 0;
          if (w < walks) {
            const uint4 a = philox4x32_10(make_uint4((unsigned)w, s_lo, s_hi, SAMPLE_STREAM_RW_A), k0, k1);
            u2[j] = (u64)a.z | ((u64)a.w << 32);
            if (length == 3) {
              const uint4 b = philox4x32_10(make_uint4((unsigned)w, s_lo, s_hi, SAMPLE_STREAM_RW_B), k0, k1);
              u3[j] = (u64)b.x | ((u64)b.y << 32);
            }
            p[j] = colA[a0 + (i64)__umul64hi((u64)a.x | ((u64)a.y << 32), (u64)da)];
          }
        }
#pragma unroll
        for (int j = 0; j < RW_ILP; ++j) { b0[j] = 0; b1[j] = 0; if (p[j] >= 0) { b0[j] = rowptrA[p[j]]; b1[j] = rowptrA[p[j] + 1]; } }
#pragma unroll
        for (int j = 0; j < RW_ILP; ++j) p[j] = rw_step(colA, b0[j], b1[j], u2[j]);       // step 2
        if (length == 3) {
#pragma unroll
          for (int j = 0; j < RW_ILP; ++j) { b0[j] = 0; b1[j] = 0; if (p[j] >= 0) { b0[j] = rowptrA[p[j]]; b1[j] = rowptrA[p[j] + 1]; } }
        }
#pragma unroll
        for (int j = 0; j < RW_ILP; ++j) if (p[j] >= 0) rw_visit(keys, vals, mask, shift, p[j], 1u);
        if (length == 3) {
#pragma unroll
          for (int j = 0; j < RW_ILP; ++j) p[j] = rw_step(colA, b0[j], b1[j], u3[j]);     // step 3
#pragma unroll
          for (int j = 0; j < RW_ILP; ++j) if (p[j] >= 0) rw_visit(keys, vals, mask, shift, p[j], 1u << 16);
        }
      }
    }
    __syncthreads();
    if (da > 0) {                                            // (the same in every thread; no barrier inside)
      const i64 m0 = rowptrM[s], dm = rowptrM[s + 1] - m0;
      for (int t = threadIdx.x; t < slots; t += OCN_BLOCK) {
        const int k = keys[t];
        if (k == RW_EMPTY || k == (int)s || sorted_has(colM + m0, dm, (int32_t)k)) continue;
        const int at = atomicAdd(&s_n, 1);
        if (FILL) list[at] = k;
      }
    }
    __syncthreads();
    const int n = s_n;
    if (!FILL) {
      if (threadIdx.x == 0) count[q] = n;
    } else {
      cc_wg_sort(list, n);                                   // (barriers inside; n is the same in every thread)
      const i64 at0 = ptr[q], end = ptr[q + 1];
      for (int i = threadIdx.x; i < n; i += OCN_BLOCK) {
        const int k = list[i];
        const unsigned c = rw_lookup(keys, vals, mask, shift, k);
        const int c2 = (int)(c & 0xffffu), c3 = (int)(c >> 16);
        const i64 at = at0 + i;
        if (at < end) {                                      // offsets of another input write nothing past their own segment
          edges[at] = make_longlong2(s, (i64)k);
          val[at] = __fadd_rn((float)c2, __fmul_rn(decay, (float)c3));
          visits[at] = make_int2(c2, c3);
        }
      }
    }
    __syncthreads();                                         // the next query's clear stays behind these reads
  }
}

static inline int rw_args_bad(const void* rowptrA, const void* colA, const void* rowptrM, const void* colM, int64_t n_cols,
                              const void* sources, int64_t Q, int32_t walks, int32_t length) {
  if (!rowptrA || !colA || !rowptrM || !colM || !sources) return 1;
  if (n_cols < 1 || n_cols >= ((int64_t)1 << 31) || Q < 0) return 1;
  if (walks < 1 || walks > RW_MAX_WALKS || (length != 2 && length != 3)) return 1;
  return 0;
}

template <bool FILL>
static int rw_launch(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM, int64_t n_cols,
                     const int64_t* sources, int64_t Q, int32_t walks, int32_t length, uint64_t seed, const int64_t* ptr,
                     float decay, int32_t* count, int64_t* edges, float* val, int32_t* visits, void* stream) {
  static std::atomic<unsigned long long> lds_raised{0ull};   // (one per instance)
  if (const int rc = ws_raise_lds_once((const void*)rw_visits_kernel<FILL>, (size_t)RW_LDS_MAX, lds_raised)) return rc;
  const int nv = walks * (length - 1), slots = rw_slots(nv);
  int log2 = 0;
  while ((1 << log2) < slots) ++log2;
  hipLaunchKernelGGL(rw_visits_kernel<FILL>, dim3((unsigned)grid_for(Q, 256 * 8)), dim3(OCN_BLOCK), rw_lds_bytes(slots, nv),
                     (hipStream_t)stream, (const i64*)rowptrA, colA, (const i64*)rowptrM, colM, (i64)n_cols, (const i64*)sources,
                     (i64)Q, (int)walks, (int)length, (u64)seed, slots, 32 - log2, (const i64*)ptr, decay, count,
                     (longlong2*)edges, val, (int2*)visits);
  return launch_status();
}

extern "C" {

int32_t ocn_rw_max_walks(void) { return RW_MAX_WALKS; }

int ocn_rw_visits_count(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM, int64_t n_cols,
                        const int64_t* sources, int64_t Q, int32_t walks, int32_t length, uint64_t seed, int32_t* count,
                        void* stream) {
  if (rw_args_bad(rowptrA, colA, rowptrM, colM, n_cols, sources, Q, walks, length) || !count) return OCN_EINVAL;
  if (Q == 0) return 0;
  return rw_launch<false>(rowptrA, colA, rowptrM, colM, n_cols, sources, Q, walks, length, seed, nullptr, 0.0f, count, nullptr,
                          nullptr, nullptr, stream);
}

int ocn_rw_visits_fill(const int64_t* rowptrA, const int32_t* colA, const int64_t* rowptrM, const int32_t* colM, int64_t n_cols,
                       const int64_t* sources, int64_t Q, int32_t walks, int32_t length, uint64_t seed, const int64_t* ptr,
                       float decay, int64_t* edges, float* val, int32_t* visits, void* stream) {
  if (rw_args_bad(rowptrA, colA, rowptrM, colM, n_cols, sources, Q, walks, length) || !ptr || !edges || !val || !visits)
    return OCN_EINVAL;
  if (!(decay >= 0.0f) || decay > 3.402823466e+38f) return OCN_EINVAL;                 // (NaN, negative, infinite)
  if ((((uintptr_t)edges) & 15u) || (((uintptr_t)visits) & 7u)) return OCN_EINVAL;     // (written as 16- and 8-byte pairs)
  if (Q == 0) return 0;
  return rw_launch<true>(rowptrA, colA, rowptrM, colM, n_cols, sources, Q, walks, length, seed, ptr, length == 3 ? decay : 0.0f,
                         nullptr, edges, val, visits, stream);
}

}  // extern "C"
