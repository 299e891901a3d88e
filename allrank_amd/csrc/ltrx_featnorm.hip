// Feature normalisation of a resident item array x[n, F] (the reference: reproducibility/normalize_features.py): per-column
// minimum, per-column mean and population std of the transformed value t, and the in-place standardisation.  Contract: include/ltrx.h.
//
// ARITHMETIC.  featnorm_value is the ONE statement of t: the fp32 value widened to fp64, negated where the column's flag says so, and
// log(. + eps_log) where the column takes the logarithm.  The moments and the in-place pass call it, so they see the same t.
//
// SHAPE.  All three passes are streams over 4 n F bytes.  A thread owns V consecutive columns (V = 4: one 16-byte access per row, where
// ld % 4 == 0 and x is 16-byte aligned; V = 1 otherwise) and `tpr` = min(ceil(F / V), 256) threads cover a row, so consecutive threads
// read consecutive addresses of a row and the next row lane goes on where the row ends; R = 256 / tpr row lanes walk the workgroup's
// block of rows in steps of R.  blockIdx.y selects the column tile where a row needs more than 256 threads (F > 1024, or > 256 in the
// 4-byte form).  A column piece that would cross the end of its row (F % 4 != 0) is read and written float by float: nothing behind
// the F-th column is touched.
//
// REDUCTION (deterministic).  Thread partials (fp64, in registers) -> LDS, combined over the row lanes by a tree whose shape depends on R
// alone -> row `blockIdx.x` of the workspace [workgroups, F] -> featnorm_final_kernel: 16 lanes per column take the rows j, j + 16, ...
// in order and a 4-step tree combines the lanes.  The minimum goes the same way (fp64 holds every fp32 exactly).
#include "ltrx_device.h"

#define LTRX_FEATNORM_THREADS 256
#define LTRX_FEATNORM_MAX_WORKGROUPS 2048       // partial rows of a call: 8 workgroups of 256 threads per CU
#define LTRX_FEATNORM_FINAL_COLS 16
#define LTRX_FEATNORM_FINAL_LANES 16

enum { FEATNORM_MIN = 0, FEATNORM_SUM = 1, FEATNORM_SQDEV = 2 };

__device__ __forceinline__ double featnorm_value(float x, bool neg, bool lg, double eps_log) {
  double t = (double)x;
  if (neg) t = -t;
  if (lg) t = log(t + eps_log);
  return t;
}

template <int MODE>
__device__ __forceinline__ double featnorm_combine(double a, double b) {
  return MODE == FEATNORM_MIN ? fmin(a, b) : a + b;
}

// how a call's rows and columns are spread over threads and workgroups: host and kernels read the same record
struct FeatnormPlan {
  int V, tpr, R, tiles, rows_per_wg, nblk;
};

static inline FeatnormPlan featnorm_plan(const void* x, int n, int F, int ld) {
  FeatnormPlan p;
  p.V = (ld % 4 == 0 && ((uintptr_t)x & 15) == 0) ? 4 : 1;
  const int pieces = (F + p.V - 1) / p.V;
  p.tpr = pieces < LTRX_FEATNORM_THREADS ? pieces : LTRX_FEATNORM_THREADS;
  p.R = LTRX_FEATNORM_THREADS / p.tpr;
  p.tiles = (pieces + p.tpr - 1) / p.tpr;
  int want = LTRX_FEATNORM_MAX_WORKGROUPS / p.tiles;                 // workgroups along the rows
  if (want < 1) want = 1;
  const int groups = (n + p.R - 1) / p.R;                            // steps of R rows
  if (want > groups) want = groups;
  p.rows_per_wg = ((groups + want - 1) / want) * p.R;
  p.nblk = (n + p.rows_per_wg - 1) / p.rows_per_wg;                  // <= want <= min(n, LTRX_FEATNORM_MAX_WORKGROUPS)
  return p;
}

static inline size_t featnorm_workspace_bytes(int n, int F) {
  if (n <= 0 || F <= 0) return 0;
  return (size_t)(n < LTRX_FEATNORM_MAX_WORKGROUPS ? n : LTRX_FEATNORM_MAX_WORKGROUPS) * (size_t)F * sizeof(double);
}

// the V columns c0 .. c0 + V - 1 of a row: one 16-byte access where the piece lies inside the row, floats otherwise
template <int V>
__device__ __forceinline__ void featnorm_load(const float* p, int live, float (&v)[V]) {
  if (V == 4 && live == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = e < live ? p[e] : 0.0f;
  }
}

template <int V, int MODE>
__global__ void __launch_bounds__(LTRX_FEATNORM_THREADS) featnorm_reduce_kernel(const float* __restrict__ x, int n, int F, int ld,
                                                                               const uint8_t* __restrict__ negate,
                                                                               const uint8_t* __restrict__ take_log, double eps_log,
                                                                               const double* __restrict__ mean, int tpr, int R,
                                                                               int rows_per_wg, double* __restrict__ part) {
  __shared__ double red[LTRX_FEATNORM_THREADS * V];
  const int cg = threadIdx.x % tpr, rl = threadIdx.x / tpr;
  const int c0 = ((int)blockIdx.y * tpr + cg) * V;
  const int live = rl < R ? min(max(F - c0, 0), V) : 0;            // columns of this thread inside the row
  double acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = MODE == FEATNORM_MIN ? (double)INFINITY : 0.0;
  if (live > 0) {
    bool neg[V], lg[V];
    double mu[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      neg[e] = e < live && negate[c0 + e] != 0;
      lg[e] = MODE != FEATNORM_MIN && e < live && take_log[c0 + e] != 0;
      mu[e] = (MODE == FEATNORM_SQDEV && e < live) ? mean[c0 + e] : 0.0;
    }
    const int r0 = (int)blockIdx.x * rows_per_wg;
    const int r1 = min(n, r0 + rows_per_wg);
#pragma unroll 2
    for (int r = r0 + rl; r < r1; r += R) {
      float v[V];
      featnorm_load<V>(x + (size_t)r * ld + c0, live, v);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (e < live) {
          const double t = featnorm_value(v[e], neg[e], lg[e], eps_log);
          if (MODE == FEATNORM_SQDEV) {
            const double d = t - mu[e];
            acc[e] += d * d;
          } else {
            acc[e] = featnorm_combine<MODE>(acc[e], t);
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) red[threadIdx.x * V + e] = acc[e];
  __syncthreads();
  int top = 1;
  while (top < R) top <<= 1;
  for (int s = top >> 1; s > 0; s >>= 1) {                         // row lane rl takes lane rl + s: the shape depends on R alone
    if (rl < s && rl + s < R) {
#pragma unroll
      for (int e = 0; e < V; ++e)
        red[threadIdx.x * V + e] = featnorm_combine<MODE>(red[threadIdx.x * V + e], red[(threadIdx.x + s * tpr) * V + e]);
    }
    __syncthreads();
  }
  if (rl == 0) {
    for (int e = 0; e < live; ++e) part[(size_t)blockIdx.x * F + c0 + e] = red[threadIdx.x * V + e];
  }
}

// column c of the nblk partial rows -> its result: the minimum (fp32), the mean = sum / n, or the std = sqrt(sum / n)
template <int MODE>
__global__ void __launch_bounds__(LTRX_FEATNORM_FINAL_COLS* LTRX_FEATNORM_FINAL_LANES)
    featnorm_final_kernel(const double* __restrict__ part, int nblk, int F, int n, double* __restrict__ out_d, float* __restrict__ out_f) {
  __shared__ double red[LTRX_FEATNORM_FINAL_COLS * LTRX_FEATNORM_FINAL_LANES];
  const int c = (int)blockIdx.x * LTRX_FEATNORM_FINAL_COLS + ((int)threadIdx.x % LTRX_FEATNORM_FINAL_COLS);
  const int j = (int)threadIdx.x / LTRX_FEATNORM_FINAL_COLS;
  double acc = MODE == FEATNORM_MIN ? (double)INFINITY : 0.0;
  if (c < F)
    for (int b = j; b < nblk; b += LTRX_FEATNORM_FINAL_LANES) acc = featnorm_combine<MODE>(acc, part[(size_t)b * F + c]);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = LTRX_FEATNORM_FINAL_LANES / 2; s > 0; s >>= 1) {
    if (j < s) red[threadIdx.x] = featnorm_combine<MODE>(red[threadIdx.x], red[threadIdx.x + s * LTRX_FEATNORM_FINAL_COLS]);
    __syncthreads();
  }
  if (j == 0 && c < F) {
    const double tot = red[threadIdx.x];
    if (MODE == FEATNORM_MIN) out_f[c] = (float)tot;
    if (MODE == FEATNORM_SUM) out_d[c] = tot / (double)n;
    if (MODE == FEATNORM_SQDEV) out_d[c] = sqrt(tot / (double)n);
  }
}

template <int V>
__global__ void __launch_bounds__(LTRX_FEATNORM_THREADS) featnorm_apply_kernel(float* __restrict__ x, int n, int F, int ld,
                                                                              const uint8_t* __restrict__ negate,
                                                                              const uint8_t* __restrict__ take_log, double eps_log,
                                                                              const double* __restrict__ mean,
                                                                              const double* __restrict__ std, double eps, int tpr, int R,
                                                                              int rows_per_wg) {
  const int cg = threadIdx.x % tpr, rl = threadIdx.x / tpr;
  const int c0 = ((int)blockIdx.y * tpr + cg) * V;
  const int live = rl < R ? min(max(F - c0, 0), V) : 0;
  if (live == 0) return;
  bool neg[V], lg[V];
  double mu[V], den[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    neg[e] = e < live && negate[c0 + e] != 0;
    lg[e] = e < live && take_log[c0 + e] != 0;
    mu[e] = e < live ? mean[c0 + e] : 0.0;
    den[e] = e < live ? std[c0 + e] + eps : 1.0;
  }
  const int r0 = (int)blockIdx.x * rows_per_wg;
  const int r1 = min(n, r0 + rows_per_wg);
#pragma unroll 2
  for (int r = r0 + rl; r < r1; r += R) {
    float* p = x + (size_t)r * ld + c0;
    float v[V];
    featnorm_load<V>(p, live, v);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = (float)((featnorm_value(v[e], neg[e], lg[e], eps_log) - mu[e]) / den[e]);
    if (V == 4 && live == 4) {
      *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (e < live) p[e] = v[e];
    }
  }
}

template <int MODE>
static int featnorm_reduce(const float* x, int n, int F, int ld, const uint8_t* negate, const uint8_t* take_log, double eps_log,
                           const double* mean, double* out_d, float* out_f, double* ws, hipStream_t s) {
  const FeatnormPlan p = featnorm_plan(x, n, F, ld);
  const dim3 grid(p.nblk, p.tiles), block(LTRX_FEATNORM_THREADS);
  if (p.V == 4)
    hipLaunchKernelGGL((featnorm_reduce_kernel<4, MODE>), grid, block, 0, s, x, n, F, ld, negate, take_log, eps_log, mean, p.tpr, p.R,
                       p.rows_per_wg, ws);
  else
    hipLaunchKernelGGL((featnorm_reduce_kernel<1, MODE>), grid, block, 0, s, x, n, F, ld, negate, take_log, eps_log, mean, p.tpr, p.R,
                       p.rows_per_wg, ws);
  LTRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(featnorm_final_kernel<MODE>, dim3((F + LTRX_FEATNORM_FINAL_COLS - 1) / LTRX_FEATNORM_FINAL_COLS),
                     dim3(LTRX_FEATNORM_FINAL_COLS * LTRX_FEATNORM_FINAL_LANES), 0, s, (const double*)ws, p.nblk, F, n, out_d, out_f);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

static inline bool featnorm_bad_shape(const void* x, int n, int F, int ld) { return !x || n <= 0 || F <= 0 || ld < F; }

extern "C" size_t ltrx_feature_min_workspace_bytes(int n, int F) { return featnorm_workspace_bytes(n, F); }
extern "C" size_t ltrx_feature_moments_workspace_bytes(int n, int F) { return featnorm_workspace_bytes(n, F); }

extern "C" int ltrx_feature_min(const float* x, int n, int F, int ld, const uint8_t* negate, float* min_out, void* ws,
                                ltrx_stream_t stream) {
  if (featnorm_bad_shape(x, n, F, ld) || !negate || !min_out || !ws) return LTRX_EINVAL;
  return featnorm_reduce<FEATNORM_MIN>(x, n, F, ld, negate, nullptr, 0.0, nullptr, nullptr, min_out, (double*)ws, (hipStream_t)stream);
}

extern "C" int ltrx_feature_moments(const float* x, int n, int F, int ld, const uint8_t* negate, const uint8_t* take_log,
                                    const double* eps_log_host, double* mean_out, double* std_out, void* ws, ltrx_stream_t stream) {
  if (featnorm_bad_shape(x, n, F, ld) || !negate || !take_log || !eps_log_host || !mean_out || !std_out || !ws) return LTRX_EINVAL;
  const double eps_log = *eps_log_host;
  const int rc = featnorm_reduce<FEATNORM_SUM>(x, n, F, ld, negate, take_log, eps_log, nullptr, mean_out, nullptr, (double*)ws,
                                               (hipStream_t)stream);
  if (rc != LTRX_OK) return rc;
  return featnorm_reduce<FEATNORM_SQDEV>(x, n, F, ld, negate, take_log, eps_log, mean_out, std_out, nullptr, (double*)ws,
                                         (hipStream_t)stream);
}

extern "C" int ltrx_feature_normalize(float* x, int n, int F, int ld, const uint8_t* negate, const uint8_t* take_log,
                                      const double* eps_log_host, const double* mean, const double* std, const double* eps_host,
                                      ltrx_stream_t stream) {
  if (featnorm_bad_shape(x, n, F, ld) || !negate || !take_log || !eps_log_host || !mean || !std || !eps_host) return LTRX_EINVAL;
  const FeatnormPlan p = featnorm_plan(x, n, F, ld);
  const dim3 grid(p.nblk, p.tiles), block(LTRX_FEATNORM_THREADS);
  if (p.V == 4)
    hipLaunchKernelGGL(featnorm_apply_kernel<4>, grid, block, 0, (hipStream_t)stream, x, n, F, ld, negate, take_log, *eps_log_host, mean,
                       std, *eps_host, p.tpr, p.R, p.rows_per_wg);
  else
    hipLaunchKernelGGL(featnorm_apply_kernel<1>, grid, block, 0, (hipStream_t)stream, x, n, F, ld, negate, take_log, *eps_log_host, mean,
                       std, *eps_host, p.tpr, p.R, p.rows_per_wg);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}
