// The common-neighbour stage, K2: the per-column weights of cn5 / cn6 / cn7, written in place over the histogram the
// intersection pass leaves (common.h: HF_BITS).  See include/ocn_hip.h for the reference call sites.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// K2: per-column weights {w1, t, inv2, 0}, in place over the histogram
//   pooled xcn1 uses w1;  a union entry with cn2 value c (1, or the walk count) contributes
//   (c·[in cn2] − t·[in cn1]) · inv2 to xcn2.
// ---------------------------------------------------------------------------------------------
// scalars[0] (zero on entry) ends as: 0 = no union entry at all; -1 = union entries but no column
// with n1 >= 2; otherwise min{n1 : n1 >= 2} - INT_MAX - 1 (<= -2).  One atomicMin per workgroup,
// skipped when the word already holds something at least as small.
__global__ __launch_bounds__(OCN_BLOCK) void cn5_column_stats(const u64* __restrict__ hist, i64 N,
                                                              int32_t* __restrict__ scalars) {
  __shared__ int sh[OCN_WPB];
  int v = 0;
  for (i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (i64)gridDim.x * blockDim.x) {
    const u64 pk = hist[2 * c];
    int t = pk ? -1 : 0;
    const int n1 = hf_n1(pk);
    if (n1 >= 2) t = n1 - 0x7fffffff - 1;
    v = t < v ? t : v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(v, o, OCN_WAVE);
    v = t < v ? t : v;
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < OCN_WPB; ++i) v = sh[i] < v ? sh[i] : v;
    if (v < 0 && v < __hip_atomic_load(scalars, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(scalars, v);
  }
}

__global__ __launch_bounds__(OCN_BLOCK) void cn5_column_weights(u64* __restrict__ hist, i64 N,
                                                                const float* __restrict__ innerprod,
                                                                const int32_t* __restrict__ scalars,
                                                                int valued, const float* __restrict__ s2_exact) {
  // model.py:2370-2376: scale = max |ncn1| over the union-aligned vector (1.0 if it is empty)
  const float nip = cn5_nip(scalars[0], innerprod[0]);
  float4* wout = reinterpret_cast<float4*>(hist);
  for (i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (i64)gridDim.x * blockDim.x) {
    const u64 pk = hist[2 * c];
    if (pk == 0) continue;                               // untouched column: never read by the gather
    const u64 walks = hist[2 * c + 1];
    const int n1 = hf_n1(pk), n2 = hf_n2(pk), nb = n1 + n2 - hf_nu(pk);
    const float inv1 = n1 >= 2 ? 1.0f / (float)n1 : 0.0f;              // :2263-2266 (Q2)
    const float t = __fmul_rn(nip, inv1);                              // nip * ncn1 value
    // :2405-2406 column sum of v = cn2 − nip·ncn1 over the union pattern.  The reference adds the entries one by
    // one in fp32, in ascending batch-row order (index_add_ over the coalesced COO): s2_exact holds exactly that
    // sum (ocn_cn_colsum_exact) whenever nip != 0.  For nip == 0 every v is an integer (1.0, or the walk count),
    // the sequential fp32 sum is the integer count itself as long as it stays below 2^24, and the closed form
    // below is that same number.
    float S2;
    if (s2_exact) {
      S2 = s2_exact[c];
    } else {
      double s2d;
      if (!valued) {
        const float v_both = __fsub_rn(1.0f, t);                         // :2380-2384
        const float v_only2 = __fsub_rn(1.0f, __fmul_rn(nip, 0.0f));
        const float v_only1 = __fsub_rn(0.0f, t);
        s2d = (double)(n2 - nb) * (double)v_only2 + (double)nb * (double)v_both +
              (double)(n1 - nb) * (double)v_only1;
      } else {
        s2d = (double)walks - (double)n1 * (double)t;
      }
      S2 = (float)s2d;
    }
    if (S2 == 0.0f) S2 = 1.0f;                                         // :2409
    wout[c] = make_float4(inv1, t, 1.0f / S2, 0.0f);                   // :2410-2413
  }
}

// cn6 (model.py:2535-2951), pattern route: stage 1 is cn5's (histA = {n1, n2, n_union} of cn1 / cn2,
// rewritten in place as {inv1, t, inv2, 0}); stage 2 orthogonalises cn3 (histB: its n1 field counts the
// cn3 entries of the column) against both normalised matrices,
//   v3 = [in cn3] - nip*inv1*[in cn1] - nip*ncn2,     S3 = column sum of v3 (0 -> 1),
// and histB is rewritten as {1/S3, 0, 0, 0}.  The column sums are formed from the integer counts in
// fp64 (exact for nip == 0: S2 = n2, S3 = n3), as for cn5.  nip_out[0] receives nip for the gather.
__global__ __launch_bounds__(OCN_BLOCK) void cn6_column_weights(u64* __restrict__ histA, u64* __restrict__ histB,
                                                                i64 N, const float* __restrict__ innerprod,
                                                                const int32_t* __restrict__ scalars,
                                                                float* __restrict__ nip_out,
                                                                const float* __restrict__ s2_exact,
                                                                const float* __restrict__ s3_exact) {
  const float nip = cn5_nip(scalars[0], innerprod[0]);
  if (blockIdx.x == 0 && threadIdx.x == 0) nip_out[0] = nip;
  float4* wa = reinterpret_cast<float4*>(histA);
  float4* wb = reinterpret_cast<float4*>(histB);
  for (i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (i64)gridDim.x * blockDim.x) {
    const u64 pa = histA[2 * c], pb = histB[2 * c];
    if (pa == 0 && pb == 0) continue;
    const int n1 = hf_n1(pa), n2 = hf_n2(pa), nb = n1 + n2 - hf_nu(pa), n3 = hf_n1(pb);
    const float inv1 = n1 >= 2 ? 1.0f / (float)n1 : 0.0f;
    const float t = __fmul_rn(nip, inv1);
    const float v_both = __fsub_rn(1.0f, t), v_only2 = __fsub_rn(1.0f, __fmul_rn(nip, 0.0f)), v_only1 = __fsub_rn(0.0f, t);
    float S2 = s2_exact ? s2_exact[c]
                        : (float)((double)(n2 - nb) * (double)v_only2 + (double)nb * (double)v_both +
                                  (double)(n1 - nb) * (double)v_only1);
    if (S2 == 0.0f) S2 = 1.0f;
    const float inv2 = 1.0f / S2;
    float S3;
    if (s3_exact) {
      S3 = s3_exact[c];
    } else {
      // column sum of the normalised cn2' values (1 up to rounding, or 0)
      const double s2n = (double)(n2 - nb) * (double)__fmul_rn(v_only2, inv2) + (double)nb * (double)__fmul_rn(v_both, inv2) +
                         (double)(n1 - nb) * (double)__fmul_rn(v_only1, inv2);
      S3 = (float)((double)n3 - (double)n1 * (double)t - (double)nip * s2n);
    }
    if (S3 == 0.0f) S3 = 1.0f;
    wa[c] = make_float4(inv1, t, inv2, 0.0f);
    wb[c] = make_float4(1.0f / S3, 0.0f, 0.0f, 0.0f);
  }
}

// d1 / d2 (or NULL = all ones): the diagonals diag(T_k(linspace(-1, 1, N))) the reference multiplies the normalised cn1 and
// the raw cn2 by (evaluate_polynomial, model.py:2995-3019; spspmm with the diagonal at :3141-3165 and :3186-3209 — one fp32
// product per entry).  The drivers hard-wire k = 0 (T0 = 1, the --polyfirst / --polysecond flags are parsed and ignored, Q4).
__global__ __launch_bounds__(OCN_BLOCK) void cn7_column_weights(u64* __restrict__ hist, i64 N,
                                                                float sum_fill, const float* __restrict__ d1,
                                                                const float* __restrict__ d2) {
  float4* wout = reinterpret_cast<float4*>(hist);
  for (i64 c = (i64)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (i64)gridDim.x * blockDim.x) {
    const u64 pk = hist[2 * c];
    if (pk == 0) continue;
    const int n1 = hf_n1(pk);
    const float inv1 = n1 >= 2 ? 1.0f / (float)n1 : sum_fill;          // model.py:3116-3120
    // cn1: ncn1 x T_k1 (model.py:3141-3165); cn2 raw (Q5) x T_k2 (:3186-3209): t = 0, "inv2" = the diagonal's entry, so that
    // an entry's weight (c - 0) * inv2 is the one product c * T_k2 the reference forms
    wout[c] = make_float4(__fmul_rn(inv1, d1 ? d1[c] : 1.0f), 0.0f, d2 ? d2[c] : 1.0f, 0.0f);
  }
}

extern "C" {

int ocn_cn5_column_stats(const uint64_t* hist, int64_t N, int32_t* scalars, void* stream) {
  if (N < 0 || (N > 0 && (!hist || !scalars))) return OCN_EINVAL;
  if (N == 0) return 0;
  const int grid = grid_for((N + OCN_BLOCK - 1) / OCN_BLOCK, 512);
  hipLaunchKernelGGL(cn5_column_stats, dim3(grid), dim3(OCN_BLOCK), 0, (hipStream_t)stream, (const u64*)hist, (i64)N,
                     scalars);
  return launch_status();
}

int ocn_cn_weights_cn5(uint64_t* hist, int64_t N, const float* innerprod, int32_t* scalars,
                       int32_t valued, const float* s2_exact, void* stream) {
  if (N < 0 || (N > 0 && (!hist || !innerprod || !scalars))) return OCN_EINVAL;
  if (N == 0) return 0;
  const int grid = grid_for((N + OCN_BLOCK - 1) / OCN_BLOCK, 2048);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cn5_column_weights, dim3(grid), dim3(OCN_BLOCK), 0, st, (u64*)hist, (i64)N,
                     innerprod, (const int32_t*)scalars, (int)valued, s2_exact);
  return launch_status();
}

int ocn_cn_weights_cn6(uint64_t* histA, uint64_t* histB, int64_t N, const float* innerprod, int32_t* scalars,
                       float* nip_out, const float* s2_exact, const float* s3_exact, void* stream) {
  if (N < 0 || (N > 0 && (!histA || !histB || !innerprod || !scalars || !nip_out))) return OCN_EINVAL;
  if (N == 0) return 0;
  const int grid = grid_for((N + OCN_BLOCK - 1) / OCN_BLOCK, 2048);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cn6_column_weights, dim3(grid), dim3(OCN_BLOCK), 0, st, (u64*)histA, (u64*)histB, (i64)N,
                     innerprod, (const int32_t*)scalars, nip_out, s2_exact, s3_exact);
  return launch_status();
}

int ocn_cn_weights_cn7(uint64_t* hist, int64_t N, float sum_fill, const float* diag1, const float* diag2, void* stream) {
  if (N < 0 || (N > 0 && !hist)) return OCN_EINVAL;
  if (N == 0) return 0;
  const int grid = grid_for((N + OCN_BLOCK - 1) / OCN_BLOCK, 2048);
  hipLaunchKernelGGL(cn7_column_weights, dim3(grid), dim3(OCN_BLOCK), 0, (hipStream_t)stream,
                     (u64*)hist, (i64)N, sum_fill, diag1, diag2);
  return launch_status();
}

}  // extern "C"
