// Sampled dense-dense product on the pattern of a CSR operator: the gradient of an encoder layer with respect to its messages.
// For entry p of row r with column k:  out[p] = fl(c * <g[r], x[k]>), c the coefficient the forward (spmm.hip) gives the entry —
// the entry weight (1, pre[k] or fl(pre[r]*pre[k]); times val[p] for a valued adjacency), times post[r], over the row length for
// mean.  The self term is no entry; under self_mode 2 an explicit self loop, which the forward replaces by the self term, gets +0.
// No atomics, no workspace, no LDS.  See include/ocn_hip.h (ocn_sddmm_csr).
#include "common.h"

constexpr int SDDMM_UNR = 4;   // x rows in flight per lane group

// entries per work item: a fixed run of consecutive positions of the entry space, so a hub row is many items.  One round of the
// lane group at the wide instances: at the collab shape (H = 256) runs of 64 took 0.34 ms, of 128 0.39, of 256 0.44, of 512 0.40
// on grids large enough to give every item its own lane group (message saliency)
__host__ __device__ constexpr int sddmm_run(int lpe) { return lpe < 32 ? 32 : lpe; }

// The lane-group shape of cn_attr_kernel: LPE lanes own a row and a lane keeps its NV float4 of g[r] in registers.  The work
// items are runs of RUN consecutive entry positions, dealt to the lane groups of the launch round-robin (the grid is sized by
// the row count; the entry count is read from rowptr[n_rows] on the device).  An item finds the row of its first position by
// bisection of rowptr and then walks row by row: a row shorter than the run is taken whole by the item it starts in, a longer
// one is cut — but an entry's value is formed from (r, k, p) alone, the same way in whichever item it falls.  A round covers LPE
// positions of the row: every lane reads the column and forms the coefficient of its own position; the entries are walked four
// x rows in flight, every lane forms its partial dot over its own features (ascending, one fused multiply-add each), the group
// sums them with an xor butterfly — every lane ends with the same bits, and the order of the additions depends on (LPE, NV),
// that is on F, only — and the lane that owns the position stores fl(c * d).
template <int LPE, int NV>
__global__ __launch_bounds__(OCN_BLOCK) void sddmm_csr_kernel(
    const i64* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val, i64 n_rows,
    const float* __restrict__ g, const float* __restrict__ x, int F, const float* __restrict__ pre,
    const float* __restrict__ post, int mode, int edge_scale, int self_mode, float* __restrict__ out) {
  constexpr int GPW = OCN_WAVE / LPE;
  constexpr i64 RUN = sddmm_run(LPE);
  const int lane = threadIdx.x & 63;
  const int gl = lane % LPE;
  const int gbase = lane - gl;
  const i64 slots = (i64)gridDim.x * OCN_WPB * GPW;
  const i64 slot = ((i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6)) * GPW + lane / LPE;
  const i64 nnz = rowptr[n_rows];
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const i64 rowq = F >> 2;                  // float4 per row

  for (i64 start = slot * RUN; start < nnz; start += slots * RUN) {     // group-uniform: the whole group takes an item together
    const i64 end = start + RUN < nnz ? start + RUN : nnz;
    i64 r;
    {                                        // first row with rowptr[r + 1] > start (start < nnz = rowptr[n_rows]: there is one)
      i64 lo = 0, hi = n_rows - 1;
      while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (rowptr[mid + 1] <= start) lo = mid + 1; else hi = mid;
      }
      r = lo;
    }
    i64 pos = start;
    while (pos < end) {
      i64 re = rowptr[r + 1];
      while (re <= pos && r + 1 < n_rows) { ++r; re = rowptr[r + 1]; }  // rows without an entry at or after pos
      if (re <= pos) break;                  // (a rowptr that is not ascending: nothing is indexed past it)
      const i64 a0 = rowptr[r];
      const i64 seg_end = re < end ? re : end;
      f32x4 gr[NV];
      {
        const float4* pg = g4 + r * rowq + gl;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const float4 a = pg[v * LPE];
          gr[v] = f32x4{a.x, a.y, a.z, a.w};
        }
      }
      const float pr = (pre && edge_scale) ? pre[r] : 1.0f;
      const float po = post ? post[r] : 1.0f;
      const float len = (float)(re - a0);    // mean: the forward divides by the number of terms added (no self term with mean)

      for (i64 p0 = pos; p0 < seg_end; p0 += LPE) {
        const i64 p = p0 + gl;
        const bool own = p < seg_end;
        int32_t k = 0;
        float c = 1.0f;
        if (own) {
          k = col[p];
          if (pre) c = edge_scale ? __fmul_rn(pr, pre[k]) : pre[k];
          if (val) c = __fmul_rn(val[p], c);
          if (post) c = __fmul_rn(po, c);
          if (mode == 1) c = __fdiv_rn(c, len);
        }
        const int cnt = (int)((seg_end - p0) < LPE ? (seg_end - p0) : LPE);
        float d = 0.f;
        for (int b0 = 0; b0 < cnt; b0 += SDDMM_UNR) {
          float4 xv[SDDMM_UNR][NV];
#pragma unroll
          for (int u = 0; u < SDDMM_UNR; ++u) {
            const int b = b0 + u;
            const int32_t kk = __shfl(k, gbase + (b < cnt ? b : 0), OCN_WAVE);
            if (b < cnt) {
              const float4* row = x4 + (i64)kk * rowq + gl;
#pragma unroll
              for (int v = 0; v < NV; ++v) xv[u][v] = row[v * LPE];
            }
          }
#pragma unroll
          for (int u = 0; u < SDDMM_UNR; ++u) {
            if (b0 + u < cnt) {
              float s = 0.f;
#pragma unroll
              for (int v = 0; v < NV; ++v) {
                s = __fmaf_rn(xv[u][v].x, gr[v].x, s);
                s = __fmaf_rn(xv[u][v].y, gr[v].y, s);
                s = __fmaf_rn(xv[u][v].z, gr[v].z, s);
                s = __fmaf_rn(xv[u][v].w, gr[v].w, s);
              }
#pragma unroll
              for (int o = LPE / 2; o > 0; o >>= 1)     // the group is converged here: cnt is the same in all of its lanes
                s = __fadd_rn(s, __shfl_xor(s, o, OCN_WAVE));
              if (gl == b0 + u) d = s;
            }
          }
        }
        if (own) out[p] = (self_mode == 2 && (i64)k == r) ? 0.f : __fmul_rn(c, d);
      }
      pos = seg_end;
    }
  }
}

extern "C" {

int ocn_sddmm_csr(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, const float* g, const float* x,
                  int32_t F, const float* pre, const float* post, int32_t mode, int32_t edge_scale, int32_t self_mode,
                  float* out, void* stream) {
  if (n_rows < 0 || mode < 0 || mode > 1 || self_mode < 0 || self_mode > 2) return OCN_EINVAL;
  if (F != 16 && F != 32 && F != 64 && F != 128 && F != 256 && F != 512) return OCN_EINVAL;
  if (mode == 1 && (pre || post || self_mode)) return OCN_EINVAL;
  if (!rowptr || !col || !g || !x || !out) return OCN_EINVAL;
  if ((((uintptr_t)g | (uintptr_t)x) & 15u) != 0) return OCN_EINVAL;
  if (n_rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  // One lane group per row, at least one workgroup per CU and at most 65 536 workgroups: lane groups beyond the items leave at
  // once, the items of a graph with more entries than the grid covers are dealt round-robin, and the geometry never changes
  // what an entry gets.  (At the collab shape 8 192 workgroups and more all took 0.34 ms, 2 048 took 0.38.)
#define LAUNCH_SDDMM(LPE, NV)                                                                                             \
  do {                                                                                                                    \
    const i64 gpb = (i64)OCN_WPB * (OCN_WAVE / LPE);                                                                      \
    i64 blocks = (n_rows + gpb - 1) / gpb;                                                                                \
    blocks = blocks < 256 ? 256 : (blocks > 65536 ? 65536 : blocks);                                                       \
    hipLaunchKernelGGL((sddmm_csr_kernel<LPE, NV>), dim3((unsigned)blocks), dim3(OCN_BLOCK), 0, st, (const i64*)rowptr,   \
                       col, val, (i64)n_rows, g, x, (int)F, pre, post, (int)mode, (int)edge_scale, (int)self_mode, out);  \
  } while (0)
  OCN_SWITCH_WIDTH(F, LAUNCH_SDDMM)
#undef LAUNCH_SDDMM
  return launch_status();
}

}  // extern "C"
