// The common-neighbour stage, between K1 and K3: the longest-first visiting order of the pooling's workgroups, from the group
// costs the intersection pass leaves (cn_flags.hip).  common.h fixes the cost unit.  See include/ocn_hip.h (ocn_gather_schedule).
#include "common.h"

extern "C" {

// The visiting order of the pooling's slot groups: each XCD's contiguous eighth of the groups, stable-sorted by
// descending cost (64 buckets) — one workgroup per eighth, a counting sort in LDS: thread t counts the
// buckets of its contiguous share, the bucket-major table of counts is scanned, and the second pass writes every group
// to its rank.  Stable: groups of one source (one cost) stay neighbours.
#define SCHED_BUCKETS 64
static_assert(SCHED_MAX_EIGHTH <= 0xffff, "gather_schedule_kernel: ranks inside an eighth are unsigned short");
// `per`: groups per sorted range — an XCD's whole eighth, or a SEGMENT of it (ocn_gather_schedule `segment`): longest first inside
// segments keeps the sources in flight on an XCD within a narrow id range (their rows then meet in its L2) and still starts
// every segment with its long jobs.
__global__ __launch_bounds__(OCN_BLOCK) void gather_schedule_kernel(const int32_t* __restrict__ gcost, i64 per,
                                                                    int32_t* __restrict__ perm) {
  __shared__ unsigned short tc[SCHED_BUCKETS * OCN_BLOCK];
  __shared__ i64 s_scan[2 * OCN_WPB];
  const int t = threadIdx.x;
  const i64 lo = (i64)blockIdx.x * per;
  const i64 ipt = (per + OCN_BLOCK - 1) / OCN_BLOCK;                          // groups per thread, contiguous
  for (int b = 0; b < SCHED_BUCKETS; ++b) tc[b * OCN_BLOCK + t] = 0;
  auto bucket = [&](i64 q) -> int {
    const int c = max(gcost[lo + q], 0) >> SCHED_SHIFT;
    return SCHED_BUCKETS - 1 - (c < SCHED_BUCKETS - 1 ? c : SCHED_BUCKETS - 1);
  };
  for (i64 k = 0; k < ipt; ++k) {
    const i64 q = (i64)t * ipt + k;
    if (q < per) tc[bucket(q) * OCN_BLOCK + t] += 1;
  }
  __syncthreads();
  // exclusive scan of the flattened table (bucket-major, then thread): thread t owns entries [64 t, 64 t + 64)
  i64 mine = 0;
  for (int q = 0; q < SCHED_BUCKETS; ++q) mine += tc[t * SCHED_BUCKETS + q];
  i64 tot;
  i64 run = block_excl_scan(mine, s_scan, &tot);
  for (int q = 0; q < SCHED_BUCKETS; ++q) {
    const int v = tc[t * SCHED_BUCKETS + q];
    tc[t * SCHED_BUCKETS + q] = (unsigned short)run;
    run += v;
  }
  __syncthreads();
  for (i64 k = 0; k < ipt; ++k) {
    const i64 q = (i64)t * ipt + k;
    if (q < per) {
      const int b = bucket(q);
      perm[lo + tc[b * OCN_BLOCK + t]++] = (int32_t)(lo + q);
    }
  }
}

int ocn_gather_schedule(const int32_t* gcost, int64_t n_groups, int64_t segment, int32_t* perm, void* stream) {
  if (n_groups < 0 || n_groups % SCHED_EIGHTHS || n_groups / SCHED_EIGHTHS > SCHED_MAX_EIGHTH || segment < 0) return OCN_EINVAL;      // (common.h)
  if (n_groups == 0) return 0;
  if (!gcost || !perm) return OCN_EINVAL;
  i64 per = n_groups / SCHED_EIGHTHS;
  if (segment > 0 && segment < per && per % segment == 0) per = segment;      // (a segment that does not divide the eighth: whole eighths)
  hipLaunchKernelGGL(gather_schedule_kernel, dim3((unsigned)(n_groups / per)), dim3(OCN_BLOCK), 0, (hipStream_t)stream, gcost, per, perm);
  return launch_status();
}

}  // extern "C"
