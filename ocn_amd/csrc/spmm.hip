// Encoder SpMM: one lane group per output row, fused row scales / self term / sum-mean-max.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// encoder SpMM
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OCN_BLOCK) void deg_rsqrt_kernel(const i64* __restrict__ rowptr,
                                                              const float* __restrict__ val, i64 n,
                                                              float add, float* __restrict__ out) {
  for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (i64)gridDim.x * blockDim.x) {
    float deg;
    if (val) {                               // valued adjacency (DropAdj rescale): adj.sum(dim=-1)
      deg = 0.f;
      for (i64 p = rowptr[r]; p < rowptr[r + 1]; ++p) deg += val[p];
    } else {
      deg = (float)(rowptr[r + 1] - rowptr[r]);
    }
    const float d = add + deg;
    out[r] = d > 0.f ? 1.0f / sqrtf(d) : 0.f;
  }
}

enum { SPMM_SUM = 0, SPMM_MEAN = 1, SPMM_MAX = 2 };

template <int MODE>
__device__ __forceinline__ void red4(float4& acc, float w, bool weighted, const float4& x) {
  if (MODE == SPMM_MAX && weighted) {        // valued max (torch_sparse spmm_max): max_k fl(val_ik * x_k)
    acc.x = fmaxf(acc.x, __fmul_rn(w, x.x)); acc.y = fmaxf(acc.y, __fmul_rn(w, x.y));
    acc.z = fmaxf(acc.z, __fmul_rn(w, x.z)); acc.w = fmaxf(acc.w, __fmul_rn(w, x.w));
  } else if (MODE == SPMM_MAX) {
    acc.x = fmaxf(acc.x, x.x); acc.y = fmaxf(acc.y, x.y);
    acc.z = fmaxf(acc.z, x.z); acc.w = fmaxf(acc.w, x.w);
  } else if (weighted) {
    axpy4(acc, w, x);
  } else {
    acc.x = __fadd_rn(acc.x, x.x); acc.y = __fadd_rn(acc.y, x.y);
    acc.z = __fadd_rn(acc.z, x.z); acc.w = __fadd_rn(acc.w, x.w);
  }
}

// LIST == false: lane group g of the launch owns output row g.  LIST == true (ocn_spmm_csr_rows): it owns the row rows[g]
// of the operator and writes row g of a compact y [n_list][F] — pre, post and the self term keep the GLOBAL row id.  The row
// id is all that differs: one body, so the two entries add a row's terms in the same order and give the same bits.  A listed
// id outside [0, n_rows) gives a zero row (nothing is indexed with it).
template <int LPE, int NV, int MODE, bool LIST>
__global__ __launch_bounds__(OCN_BLOCK) void spmm_csr_kernel(
    const i64* __restrict__ rowptr, const int32_t* __restrict__ col, i64 n_rows,
    const float* __restrict__ val, const float* __restrict__ x, int F, const float* __restrict__ pre,
    const float* __restrict__ post, int edge_scale, int self_mode, float* __restrict__ y,
    const i64* __restrict__ rows, i64 n_list) {
  constexpr int GPW = OCN_WAVE / LPE;
  constexpr int UNR = 4;
  const int lane = threadIdx.x & 63;
  const int gl = lane % LPE;
  const int gbase = lane - gl;
  const i64 slot = ((i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6)) * GPW + lane / LPE;
  if (slot >= (LIST ? n_list : n_rows)) return;
  const i64 r = LIST ? rows[slot] : slot;
  if (LIST && (r < 0 || r >= n_rows)) {
    float4* z = reinterpret_cast<float4*>(y) + slot * (F >> 2) + gl;
#pragma unroll
    for (int v = 0; v < NV; ++v) z[v * LPE] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const i64 a0 = rowptr[r], da = rowptr[r + 1] - a0;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const i64 rowq = F >> 2;
  const bool weighted = pre != nullptr || val != nullptr;
  // pre lives in the operator's COLUMN space (one entry per row of x).  pre[r] is used by edge_scale and by the self term only —
  // both need r to be a column id too — so it is loaded only for them: a rectangular operator with more rows than columns
  // (the valued-mean backward over Aᵀ) never indexes pre with a row id.
  const float pr = (pre && (edge_scale || self_mode)) ? pre[r] : 1.0f;

  float4 acc[NV];
  const float init = MODE == SPMM_MAX ? -INFINITY : 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = make_float4(init, init, init, init);

  // the row's own term: weight pre[r] (edge_scale 0) or fl(pre[r]*pre[r]) (edge_scale 1)
  const float wself = pre ? (edge_scale ? __fmul_rn(pr, pr) : pr) : 1.0f;
  bool self_done = self_mode != 2;
  i64 seen = 0;

  for (i64 p0 = 0; p0 < da; p0 += LPE) {
    const i64 p = p0 + gl;
    int32_t k = 0;
    float wk = 1.0f;
    if (p < da) {
      k = col[a0 + p];
      if (pre) wk = edge_scale ? __fmul_rn(pr, pre[k]) : pre[k];
      if (val) wk = __fmul_rn(val[a0 + p], wk);
    }
    const int cnt = (int)((da - p0) < LPE ? (da - p0) : LPE);
    for (int b0 = 0; b0 < cnt; b0 += UNR) {
      int32_t kk[UNR];
      float ww[UNR];
      float4 xv[UNR][NV];
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        const int b = b0 + t;
        const int sl = gbase + (b < cnt ? b : 0);
        kk[t] = __shfl(k, sl, OCN_WAVE);
        ww[t] = __shfl(wk, sl, OCN_WAVE);
        if (b < cnt) {
          const float4* row = x4 + (i64)kk[t] * rowq + gl;
#pragma unroll
          for (int v = 0; v < NV; ++v) xv[t][v] = row[v * LPE];
        }
      }
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        if (b0 + t < cnt) {
          if (!self_done && (i64)kk[t] >= r) {
            // sorted position of the diagonal (fill_diag): add it before the first column >= r
            const float4* row = x4 + r * rowq + gl;
#pragma unroll
            for (int v = 0; v < NV; ++v) red4<MODE>(acc[v], wself, weighted, row[v * LPE]);
            self_done = true;
            ++seen;
            if ((i64)kk[t] == r) continue;   // an explicit self loop is replaced, not doubled
          }
#pragma unroll
          for (int v = 0; v < NV; ++v) red4<MODE>(acc[v], ww[t], weighted, xv[t][v]);
          ++seen;
        }
      }
    }
  }
  if (self_mode == 1 || !self_done) {
    const float4* row = x4 + r * rowq + gl;
#pragma unroll
    for (int v = 0; v < NV; ++v) red4<MODE>(acc[v], wself, weighted, row[v * LPE]);
    ++seen;
  }
  const float po = post ? post[r] : 1.0f;
  float4* o = reinterpret_cast<float4*>(y) + slot * rowq + gl;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    float4 a = acc[v];
    if (MODE == SPMM_MEAN) {
      const float d = (float)(seen > 0 ? seen : 1);
      a.x /= d; a.y /= d; a.z /= d; a.w /= d;
    }
    if (MODE == SPMM_MAX && seen == 0) a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (post) { a.x = __fmul_rn(po, a.x); a.y = __fmul_rn(po, a.y); a.z = __fmul_rn(po, a.z); a.w = __fmul_rn(po, a.w); }
    o[v * LPE] = a;
  }
}

// Max aggregation under autograd.  Forward: y[i,f] = max over row i of fl(v_ik * x[k,f]) (v = 1 unvalued) and
// arg[i,f] = the COLUMN id k of the winner — the backward walks Aᵀ (SparseTensor.t(): no map back to A's positions), and
// in a coalesced row (i, k) names one entry.  Ties go to the first maximum in row (ascending column) order: the row's
// first entry seeds the lane, later entries replace it only when strictly greater.  Empty row: y = 0, arg = -1 (the plain
// kernel's seen == 0 rule).  Without NaN and ±0 ties y is bit-equal to spmm_csr_kernel<.., SPMM_MAX>.
template <int LPE, int NV>
__global__ __launch_bounds__(OCN_BLOCK) void spmm_max_arg_kernel(
    const i64* __restrict__ rowptr, const int32_t* __restrict__ col, i64 n_rows, const float* __restrict__ val,
    const float* __restrict__ x, int F, float* __restrict__ y, int32_t* __restrict__ arg) {
  constexpr int GPW = OCN_WAVE / LPE;
  constexpr int UNR = 4;
  const int lane = threadIdx.x & 63;
  const int gl = lane % LPE;
  const int gbase = lane - gl;
  const i64 r = ((i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6)) * GPW + lane / LPE;
  if (r >= n_rows) return;
  const i64 a0 = rowptr[r], da = rowptr[r + 1] - a0;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const i64 rowq = F >> 2;

  float4 acc[NV];
  int4 am[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) { acc[v] = make_float4(0.f, 0.f, 0.f, 0.f); am[v] = make_int4(-1, -1, -1, -1); }

  for (i64 p0 = 0; p0 < da; p0 += LPE) {
    const i64 p = p0 + gl;
    int32_t k = 0;
    float wk = 1.0f;
    if (p < da) {
      k = col[a0 + p];
      if (val) wk = val[a0 + p];
    }
    const int cnt = (int)((da - p0) < LPE ? (da - p0) : LPE);
    for (int b0 = 0; b0 < cnt; b0 += UNR) {
      int32_t kk[UNR];
      float ww[UNR];
      float4 xv[UNR][NV];
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        const int b = b0 + t;
        const int sl = gbase + (b < cnt ? b : 0);
        kk[t] = __shfl(k, sl, OCN_WAVE);
        ww[t] = __shfl(wk, sl, OCN_WAVE);
        if (b < cnt) {
          const float4* row = x4 + (i64)kk[t] * rowq + gl;
#pragma unroll
          for (int v = 0; v < NV; ++v) xv[t][v] = row[v * LPE];
        }
      }
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        if (b0 + t < cnt) {
          const bool first = p0 + b0 + t == 0;          // the row's first entry seeds every feature
          const int32_t kc = kk[t];
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            float4 c = xv[t][v];
            if (val) { c.x = __fmul_rn(ww[t], c.x); c.y = __fmul_rn(ww[t], c.y); c.z = __fmul_rn(ww[t], c.z); c.w = __fmul_rn(ww[t], c.w); }
            if (first || c.x > acc[v].x) { acc[v].x = c.x; am[v].x = kc; }
            if (first || c.y > acc[v].y) { acc[v].y = c.y; am[v].y = kc; }
            if (first || c.z > acc[v].z) { acc[v].z = c.z; am[v].z = kc; }
            if (first || c.w > acc[v].w) { acc[v].w = c.w; am[v].w = kc; }
          }
        }
      }
    }
  }
  float4* o = reinterpret_cast<float4*>(y) + r * rowq + gl;
  int4* oa = reinterpret_cast<int4*>(arg) + r * rowq + gl;
#pragma unroll
  for (int v = 0; v < NV; ++v) { o[v * LPE] = acc[v]; oa[v * LPE] = am[v]; }
}

// Max backward: gx[k,f] = Σ_{i in row k of Aᵀ, arg[i,f] == k} v_ik * g[i,f].  One lane group per row k of Aᵀ, the
// entries added (__fadd_rn) in Aᵀ's row order: no atomics, two runs are bit-equal.  Every gx row is written (zeros
// included), so the output needs no memset.
template <int LPE, int NV>
__global__ __launch_bounds__(OCN_BLOCK) void spmm_max_backward_kernel(
    const i64* __restrict__ rowptrT, const int32_t* __restrict__ colT, i64 n_rows, const float* __restrict__ valT,
    const int32_t* __restrict__ arg, const float* __restrict__ g, int F, float* __restrict__ gx) {
  constexpr int GPW = OCN_WAVE / LPE;
  constexpr int UNR = 4;
  const int lane = threadIdx.x & 63;
  const int gl = lane % LPE;
  const int gbase = lane - gl;
  const i64 r = ((i64)blockIdx.x * OCN_WPB + (threadIdx.x >> 6)) * GPW + lane / LPE;
  if (r >= n_rows) return;
  const i64 a0 = rowptrT[r], da = rowptrT[r + 1] - a0;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const int4* arg4 = reinterpret_cast<const int4*>(arg);
  const i64 rowq = F >> 2;
  const int32_t me = (int32_t)r;

  float4 acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);

  for (i64 p0 = 0; p0 < da; p0 += LPE) {
    const i64 p = p0 + gl;
    int32_t i = 0;
    float wi = 1.0f;
    if (p < da) {
      i = colT[a0 + p];
      if (valT) wi = valT[a0 + p];
    }
    const int cnt = (int)((da - p0) < LPE ? (da - p0) : LPE);
    for (int b0 = 0; b0 < cnt; b0 += UNR) {
      float ww[UNR];
      float4 gv[UNR][NV];
      int4 av[UNR][NV];
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        const int b = b0 + t;
        const int sl = gbase + (b < cnt ? b : 0);
        const int32_t ii = __shfl(i, sl, OCN_WAVE);
        ww[t] = __shfl(wi, sl, OCN_WAVE);
        if (b < cnt) {
          const i64 off = (i64)ii * rowq + gl;
#pragma unroll
          for (int v = 0; v < NV; ++v) { av[t][v] = arg4[off + v * LPE]; gv[t][v] = g4[off + v * LPE]; }
        }
      }
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        if (b0 + t < cnt) {
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            float4 c = gv[t][v];
            if (valT) { c.x = __fmul_rn(ww[t], c.x); c.y = __fmul_rn(ww[t], c.y); c.z = __fmul_rn(ww[t], c.z); c.w = __fmul_rn(ww[t], c.w); }
            if (av[t][v].x == me) acc[v].x = __fadd_rn(acc[v].x, c.x);
            if (av[t][v].y == me) acc[v].y = __fadd_rn(acc[v].y, c.y);
            if (av[t][v].z == me) acc[v].z = __fadd_rn(acc[v].z, c.z);
            if (av[t][v].w == me) acc[v].w = __fadd_rn(acc[v].w, c.w);
          }
        }
      }
    }
  }
  float4* o = reinterpret_cast<float4*>(gx) + r * rowq + gl;
#pragma unroll
  for (int v = 0; v < NV; ++v) o[v * LPE] = acc[v];
}

extern "C" {

#define SPMM_ARGS (const i64*)rowptr, col, (i64)n_rows, val, x, (int)F, pre, post, (int)edge_scale, \
                  (int)self_mode, y
// n_out lane groups: the operator's rows, or (LIST) the listed ones
#define LAUNCH_SPMM(LPE, NV, MODE)                                                                  \
  do {                                                                                              \
    const i64 rpb = (i64)OCN_WPB * (OCN_WAVE / (LPE));                                              \
    const dim3 grid((unsigned)((n_out + rpb - 1) / rpb));                                           \
    if (rows) hipLaunchKernelGGL((spmm_csr_kernel<LPE, NV, MODE, true>), grid, dim3(OCN_BLOCK), 0, st, SPMM_ARGS, \
                                 (const i64*)rows, (i64)n_out);                                     \
    else hipLaunchKernelGGL((spmm_csr_kernel<LPE, NV, MODE, false>), grid, dim3(OCN_BLOCK), 0, st, SPMM_ARGS, \
                            (const i64*)nullptr, (i64)0);                                           \
  } while (0)
#define DISPATCH_SPMM(MODE)                                                                         \
  do {                                                                                              \
    if (F == 16) LAUNCH_SPMM(4, 1, MODE);                                                           \
    else if (F == 32) LAUNCH_SPMM(8, 1, MODE);                                                      \
    else if (F == 64) LAUNCH_SPMM(16, 1, MODE);                                                     \
    else if (F == 128) LAUNCH_SPMM(32, 1, MODE);                                                    \
    else if (F == 256) LAUNCH_SPMM(64, 1, MODE);                                                    \
    else if (F == 512) LAUNCH_SPMM(64, 2, MODE);                                                    \
    else return OCN_EINVAL; /* feature widths of the reference configs only (16..512, pow2) */      \
  } while (0)

// rows == NULL: every row of the operator (n_out = n_rows); else the n_out listed ones into a compact y
static int spmm_launch(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, const float* x,
                       int32_t F, const float* pre, const float* post, int32_t mode, int32_t edge_scale,
                       int32_t self_mode, float* y, const int64_t* rows, int64_t n_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (mode == SPMM_SUM) DISPATCH_SPMM(SPMM_SUM);
  else if (mode == SPMM_MEAN) DISPATCH_SPMM(SPMM_MEAN);
  else DISPATCH_SPMM(SPMM_MAX);
  return launch_status();
}

int ocn_spmm_csr(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, const float* x,
                 int32_t F, const float* pre, const float* post, int32_t mode, int32_t edge_scale,
                 int32_t self_mode, float* y, void* stream) {
  if (n_rows < 0 || F <= 0 || mode < 0 || mode > 2 || self_mode < 0 || self_mode > 2) return OCN_EINVAL;
  if (n_rows == 0) return 0;
  if (!rowptr || !x || !y) return OCN_EINVAL;
  return spmm_launch(rowptr, col, val, n_rows, x, F, pre, post, mode, edge_scale, self_mode, y, nullptr, n_rows, stream);
}

// F -> (lanes per row, float4 per lane) of the lane-group kernels above: the widths of DISPATCH_SPMM
#define DISPATCH_F(LAUNCH)                                                                          \
  do {                                                                                              \
    if (F == 16) LAUNCH(4, 1);                                                                      \
    else if (F == 32) LAUNCH(8, 1);                                                                 \
    else if (F == 64) LAUNCH(16, 1);                                                                \
    else if (F == 128) LAUNCH(32, 1);                                                               \
    else if (F == 256) LAUNCH(64, 1);                                                               \
    else LAUNCH(64, 2);                                                                             \
  } while (0)

static inline bool spmm_width_ok(int32_t F) {
  return F == 16 || F == 32 || F == 64 || F == 128 || F == 256 || F == 512;
}

int ocn_spmm_csr_rows(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, const float* x,
                      int32_t F, const float* pre, const float* post, int32_t mode, int32_t edge_scale,
                      int32_t self_mode, const int64_t* rows, int64_t n_list, float* y, void* stream) {
  if (n_rows < 0 || n_list < 0 || !spmm_width_ok(F) || mode < 0 || mode > 2 || self_mode < 0 || self_mode > 2) return OCN_EINVAL;
  if (!rowptr || !col || !x || !rows || !y) return OCN_EINVAL;
  if (n_list == 0 || n_rows == 0) return 0;
  return spmm_launch(rowptr, col, val, n_rows, x, F, pre, post, mode, edge_scale, self_mode, y, rows, n_list, stream);
}

int ocn_spmm_csr_max_arg(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, const float* x,
                         int32_t F, float* y, int32_t* arg, void* stream) {
  if (n_rows < 0 || !spmm_width_ok(F)) return OCN_EINVAL;
  if (!rowptr || !col || !x || !y || !arg) return OCN_EINVAL;
  if (n_rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_MAX_ARG(LPE, NV)                                                                           \
  do {                                                                                                    \
    const i64 rpb = (i64)OCN_WPB * (OCN_WAVE / (LPE));                                                    \
    hipLaunchKernelGGL((spmm_max_arg_kernel<LPE, NV>), dim3((unsigned)((n_rows + rpb - 1) / rpb)),        \
                       dim3(OCN_BLOCK), 0, st, (const i64*)rowptr, col, (i64)n_rows, val, x, (int)F, y, arg); \
  } while (0)
  DISPATCH_F(LAUNCH_MAX_ARG);
#undef LAUNCH_MAX_ARG
  return launch_status();
}

int ocn_spmm_max_backward(const int64_t* rowptrT, const int32_t* colT, const float* valT, int64_t n_rows,
                          const int32_t* arg, const float* g, int32_t F, float* gx, void* stream) {
  if (n_rows < 0 || !spmm_width_ok(F)) return OCN_EINVAL;
  if (!rowptrT || !colT || !arg || !g || !gx) return OCN_EINVAL;
  if (n_rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_MAX_BWD(LPE, NV)                                                                           \
  do {                                                                                                    \
    const i64 rpb = (i64)OCN_WPB * (OCN_WAVE / (LPE));                                                    \
    hipLaunchKernelGGL((spmm_max_backward_kernel<LPE, NV>), dim3((unsigned)((n_rows + rpb - 1) / rpb)),   \
                       dim3(OCN_BLOCK), 0, st, (const i64*)rowptrT, colT, (i64)n_rows, valT, arg, g, (int)F, gx); \
  } while (0)
  DISPATCH_F(LAUNCH_MAX_BWD);
#undef LAUNCH_MAX_BWD
  return launch_status();
}

int ocn_deg_rsqrt(const int64_t* rowptr, const float* val, int64_t n_rows, float add, float* out,
                  void* stream) {
  if (n_rows < 0 || (n_rows > 0 && (!rowptr || !out))) return OCN_EINVAL;
  if (n_rows == 0) return 0;
  const int grid = grid_for((n_rows + OCN_BLOCK - 1) / OCN_BLOCK, 2048);
  hipLaunchKernelGGL(deg_rsqrt_kernel, dim3(grid), dim3(OCN_BLOCK), 0, (hipStream_t)stream,
                     (const i64*)rowptr, val, (i64)n_rows, add, out);
  return launch_status();
}

}  // extern "C"
