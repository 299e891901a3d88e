// Small HBM-bound kernels of the explicit training step (allrank_amd/engine.py FusedTrainer): everything between
// the library GEMMs that the reference leaves to dozens of separate ATen launches.
//   ltrx_adam_step        torch.optim.Adam.step over ONE flat fp32 buffer (allrank/main.py:82; Adam lr 1e-3 in every
//                         shipped config) -- 4 streams in, 3 out, 16-B accesses; bias correction on the device step count
//   ltrx_colsum           bias gradients: out[n] = sum_m dY[m][n]   (nn.Linear backward; deterministic two-stage)
//   ltrx_relu_bwd         dz = dr * (r > 0) in place                 (transformer.py:227 / FCModel activation)
//   ltrx_score_head_fwd/bwd  OutputLayer with d_output == 1 (model.py:111-117): s[m] = <x[m,:], w> + b, and its backward
#include "ltrx_rowreg.h"

using namespace ltrx;

// ---------------------------------------------------------------------------------------------------------------
// Adam (torch defaults: amsgrad off, weight_decay 0, maximize off).  `step` is the 1-based step count, read from
// device memory so that the launch is graph-replayable; the kernel of block 0 does NOT bump it (the host wrapper
// enqueues a separate 1-thread increment first).
// ---------------------------------------------------------------------------------------------------------------
__global__ void ltrx_bump_step_kernel(float* __restrict__ step) { step[0] += 1.0f; }

__global__ void __launch_bounds__(256) ltrx_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, size_t n,
                                                        float lr, float b1, float b2, float eps, float wd, int decoupled,
                                                        const float* __restrict__ step, float grad_scale,
                                                        const float* __restrict__ grad_scale_dev) {
  // wd: torch.optim.Adam(weight_decay=wd) adds wd * p to the gradient; decoupled != 0: torch.optim.AdamW multiplies p by
  // (1 - lr * wd) before the update instead
  const float l2 = decoupled ? 0.f : wd, shrink = decoupled ? 1.0f - lr * wd : 1.0f;
  if (grad_scale_dev) grad_scale *= grad_scale_dev[0];
  const float t = step[0];
  const float bc1 = 1.0f - powf(b1, t);
  const float bc2s = sqrtf(1.0f - powf(b2, t));
  const float step_size = lr / bc1;
  const size_t n4 = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
#define LTRX_ADAM1(c)                                                   \
  {                                                                     \
    const float gr = gg.c * grad_scale + l2 * pp.c;                     \
    mm.c = b1 * mm.c + (1.0f - b1) * gr;                                \
    vv.c = b2 * vv.c + (1.0f - b2) * gr * gr;                           \
    pp.c = pp.c * shrink - step_size * (mm.c / (sqrtf(vv.c) / bc2s + eps)); \
  }
    LTRX_ADAM1(x) LTRX_ADAM1(y) LTRX_ADAM1(z) LTRX_ADAM1(w)
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  // tail (n % 4 elements)
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gr = g[i] * grad_scale + l2 * p[i];
    const float mi = b1 * m[i] + (1.0f - b1) * gr;
    const float vi = b2 * v[i] + (1.0f - b2) * gr * gr;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] * shrink - step_size * (mi / (sqrtf(vi) / bc2s + eps));
  }
#undef LTRX_ADAM1
}

// torch.optim.SGD (dampening 0): g' = g (+ wd p); buf = momentum buf + g'; p -= lr (nesterov ? g' + momentum buf : buf)
__global__ void __launch_bounds__(256) ltrx_sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                       size_t n, float lr, float momentum, int nesterov, float wd, float grad_scale,
                                                       const float* __restrict__ grad_scale_dev) {
  if (grad_scale_dev) grad_scale *= grad_scale_dev[0];
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float gr = g[i] * grad_scale + wd * p[i];
    if (momentum != 0.f) {
      const float b = momentum * buf[i] + gr;
      buf[i] = b;
      gr = nesterov ? gr + momentum * b : b;
    }
    p[i] -= lr * gr;
  }
}

extern "C" int ltrx_sgd_step(float* params, const float* grads, float* momentum_buf, size_t n, float lr, float momentum,
                             int nesterov, float weight_decay, float grad_scale, const float* grad_scale_dev, ltrx_stream_t stream) {
  if (!params || !grads || n == 0 || (momentum != 0.f && !momentum_buf) || (nesterov && !(momentum > 0.f))) return LTRX_EINVAL;
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(ltrx_sgd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, params, grads, momentum_buf, n, lr,
                     momentum, nesterov, weight_decay, grad_scale, grad_scale_dev);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

extern "C" int ltrx_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int decoupled, float* step_count,
                              float grad_scale, const float* grad_scale_dev, ltrx_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !step_count || n == 0) return LTRX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ltrx_bump_step_kernel, dim3(1), dim3(1), 0, s, step_count);
  LTRX_LAUNCH_CHECK();
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(ltrx_adam_kernel, dim3((unsigned)blocks), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, n, lr,
                     beta1, beta2, eps, weight_decay, decoupled, step_count, grad_scale, grad_scale_dev);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// column sums of a row-major [M, N] matrix (row stride ld): out[n] = sum_m a[m][n]
// stage 1: grid (ceil(N/64), R) blocks; each block's 4 waves stride over its row range, lanes own consecutive columns;
// stage 2: fixed-order combine of the R partial rows.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ltrx_colsum_partial_kernel(const float* __restrict__ a, int M, int N, int ld,
                                                                  float* __restrict__ partial) {
  __shared__ float sh[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int R = gridDim.y;
  const int rows_per = (M + R - 1) / R;
  const int r0 = blockIdx.y * rows_per;
  const int r1 = min(M, r0 + rows_per);
  float acc = 0.f;
  if (c < N)
    for (int r = r0 + w; r < r1; r += 4) acc += a[(size_t)r * ld + c];
  sh[w][lane] = acc;
  __syncthreads();
  if (w == 0 && c < N) partial[(size_t)blockIdx.y * N + c] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

__global__ void __launch_bounds__(256) ltrx_colsum_final_kernel(const float* __restrict__ partial, int R, int N,
                                                                float* __restrict__ out, int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  float acc = 0.f;
  for (int r = 0; r < R; ++r) acc += partial[(size_t)r * N + c];
  out[c] = accumulate ? out[c] + acc : acc;
}

static int colsum_rows(int M) {
  int r = (M + 255) / 256;
  return r > 64 ? 64 : (r < 1 ? 1 : r);
}

extern "C" size_t ltrx_colsum_workspace_bytes(int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  return (size_t)colsum_rows(M) * N * sizeof(float);
}

extern "C" int ltrx_colsum(const float* a, int M, int N, int ld, float* out, int accumulate, void* ws,
                           ltrx_stream_t stream) {
  if (!a || !out || !ws || M <= 0 || N <= 0 || ld < N) return LTRX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int R = colsum_rows(M);
  hipLaunchKernelGGL(ltrx_colsum_partial_kernel, dim3((N + 63) / 64, R), dim3(256), 0, s, a, M, N, ld, (float*)ws);
  LTRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ltrx_colsum_final_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const float*)ws, R, N, out, accumulate);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// elementwise helpers
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ltrx_relu_bwd_kernel(float* __restrict__ dr, const float* __restrict__ r, size_t n4,
                                                            float scale) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 d = reinterpret_cast<float4*>(dr)[i];
    const float4 a = reinterpret_cast<const float4*>(r)[i];
    d.x = a.x > 0.f ? d.x * scale : 0.f;
    d.y = a.y > 0.f ? d.y * scale : 0.f;
    d.z = a.z > 0.f ? d.z * scale : 0.f;
    d.w = a.w > 0.f ? d.w * scale : 0.f;
    reinterpret_cast<float4*>(dr)[i] = d;
  }
}

extern "C" int ltrx_relu_bwd(float* dr_inout, const float* r_post_act, size_t n, float scale, ltrx_stream_t stream) {
  if (!dr_inout || !r_post_act || n == 0 || (n & 3)) return LTRX_EINVAL;
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(ltrx_relu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dr_inout, r_post_act, n / 4, scale);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// OutputLayer, d_output == 1:  s[m] = <x[m,:], w> + b     (wave per row)
// backward: dx[m][c] = ds[m] * w[c];  dw[c] = sum_m ds[m] x[m][c];  db = sum_m ds[m]   (dw/db two-stage like colsum)
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ltrx_score_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                  const float* __restrict__ b, int M, int D,
                                                                  float* __restrict__ s) {
  const int lane = lane_id(), wpb = blockDim.x >> 6;
  for (int row = blockIdx.x * wpb + wave_id(); row < M; row += gridDim.x * wpb) {
    const float* xr = x + (size_t)row * D;
    float acc = 0.f;
    for (int c = lane; c < D; c += 64) acc += xr[c] * w[c];
    acc = wave_sum(acc);
    if (lane == 0) s[row] = acc + b[0];
  }
}

__global__ void __launch_bounds__(256) ltrx_score_head_bwd_kernel(const float* __restrict__ ds, const float* __restrict__ x,
                                                                  const float* __restrict__ w, int M, int D,
                                                                  float* __restrict__ dx, float* __restrict__ partial) {
  extern __shared__ float lds[];   // [wpb][D] dw partials + [wpb] db partials
  const int lane = lane_id(), wv = wave_id(), wpb = blockDim.x >> 6;
  float* my = lds + (size_t)wv * D;
  for (int c = lane; c < D; c += 64) my[c] = 0.f;
  float dbacc = 0.f;
  for (int row = blockIdx.x * wpb + wv; row < M; row += gridDim.x * wpb) {
    const float g = ds[row];
    const float* xr = x + (size_t)row * D;
    float* dxr = dx + (size_t)row * D;
    for (int c = lane; c < D; c += 64) {
      dxr[c] = g * w[c];
      my[c] += g * xr[c];
    }
    dbacc += g;   // identical in every lane
  }
  float* dbs = lds + (size_t)wpb * D;
  if (lane == 0) dbs[wv] = dbacc;
  __syncthreads();
  float* pa = partial + (size_t)blockIdx.x * (D + 1);
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    float a = 0.f;
    for (int k = 0; k < wpb; ++k) a += lds[(size_t)k * D + c];
    pa[c] = a;
  }
  if (threadIdx.x == 0) {
    float a = 0.f;
    for (int k = 0; k < wpb; ++k) a += dbs[k];
    pa[D] = a;
  }
}

// vectorised variant for D % 256 == 0 (NV = D / 256): a lane owns float4 columns 4 * lane + 256 * t, keeps its dw partials in
// registers over all the rows of its wave, 16-byte accesses; one LDS combine per workgroup at the end
template <int NV>
__global__ void __launch_bounds__(256) ltrx_score_head_bwd_vec_kernel(const float* __restrict__ ds, const float* __restrict__ x,
                                                                      const float* __restrict__ w, int M,
                                                                      float* __restrict__ dx, float* __restrict__ partial) {
  constexpr int D = 256 * NV;
  __shared__ float lds[4][D + 4];
  const int lane = lane_id(), wv = wave_id(), wpb = blockDim.x >> 6;
  float4 wreg[NV], acc[NV];
#pragma unroll
  for (int t = 0; t < NV; ++t) {
    wreg[t] = reinterpret_cast<const float4*>(w)[lane + 64 * t];
    acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float dbacc = 0.f;
  for (int row = blockIdx.x * wpb + wv; row < M; row += gridDim.x * wpb) {
    const float g = ds[row];
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * D);
    float4* dxr = reinterpret_cast<float4*>(dx + (size_t)row * D);
#pragma unroll
    for (int t = 0; t < NV; ++t) {
      const float4 xv = xr[lane + 64 * t];
      dxr[lane + 64 * t] = make_float4(g * wreg[t].x, g * wreg[t].y, g * wreg[t].z, g * wreg[t].w);
      acc[t].x += g * xv.x;
      acc[t].y += g * xv.y;
      acc[t].z += g * xv.z;
      acc[t].w += g * xv.w;
    }
    dbacc += g;
  }
  LTRX_ROWREG_HEAD_COMBINE(NV, lds, lane, wv, acc, dbacc, partial + (size_t)blockIdx.x * (D + 1));
}

// The parameter gradients of the kernel above where the head's input is xf = LN(xsum) and only xsum and the statistics are kept (the
// fused final norm + head, csrc/ltrx_layernorm.hip): xf is recomputed by the forward's rowreg_affine, nothing is written but the
// partials.  Grid, row walk and accumulation are ltrx_score_head_bwd's, the combine is shared, so dw / db keep the bits of the stored xf.
template <int NV>
__global__ void __launch_bounds__(256) ltrx_norm_head_wgrad_kernel(const float* __restrict__ ds, const float* __restrict__ xsum,
                                                                   const float* __restrict__ a, const float* __restrict__ b,
                                                                   const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                                   int M, float* __restrict__ partial) {
  constexpr int D = 256 * NV;
  __shared__ float lds[4][D + 4];
  const int lane = lane_id(), wv = wave_id(), wpb = blockDim.x >> 6;
  float4 av[NV], bv[NV], acc[NV];
#pragma unroll
  for (int t = 0; t < NV; ++t) {
    av[t] = reinterpret_cast<const float4*>(a)[lane + 64 * t];
    bv[t] = reinterpret_cast<const float4*>(b)[lane + 64 * t];
    acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float dbacc = 0.f;
  for (int row = blockIdx.x * wpb + wv; row < M; row += gridDim.x * wpb) {
    const float g = ds[row], mean = mean_in[row], r = rstd_in[row];
    const float4* xr = reinterpret_cast<const float4*>(xsum + (size_t)row * D);
#pragma unroll
    for (int t = 0; t < NV; ++t) {
      const float4 v = xr[lane + 64 * t];
      const float4 y = rowreg_affine(av[t], v, mean, r, bv[t]);
      acc[t].x += g * y.x;
      acc[t].y += g * y.y;
      acc[t].z += g * y.z;
      acc[t].w += g * y.w;
    }
    dbacc += g;
  }
  LTRX_ROWREG_HEAD_COMBINE(NV, lds, lane, wv, acc, dbacc, partial + (size_t)blockIdx.x * (D + 1));
}

// dw[c] = sum_k partial[k][c] (c < D), db = column D; 64 columns x 16 row groups (waves) per workgroup, fixed combine order
// (16 waves: with 4 the 512 partial rows were 128 dependent-latency iterations per wave, 21 us for 1 MB)
__global__ void __launch_bounds__(1024) ltrx_score_head_reduce_kernel(const float* __restrict__ partial, int nblk, int D,
                                                                      float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float sh[16][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float a0 = 0.f, a1 = 0.f;
  if (c <= D) {
    int k = rg;
    for (; k + 16 < nblk; k += 32) {
      a0 += partial[(size_t)k * (D + 1) + c];
      a1 += partial[(size_t)(k + 16) * (D + 1) + c];
    }
    if (k < nblk) a0 += partial[(size_t)k * (D + 1) + c];
  }
  sh[rg][cl] = a0 + a1;
  __syncthreads();
  if (rg == 0 && c <= D) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) a += sh[w][cl];
    if (c < D) dw[c] = a; else db[0] = a;
  }
}

static int head_grid(int M) {
  int g = (M + 63) / 64;
  return g > 512 ? 512 : (g < 1 ? 1 : g);
}

extern "C" int ltrx_score_head_fwd(const float* x, const float* w, const float* b, int M, int D, float* scores,
                                   ltrx_stream_t stream) {
  if (!x || !w || !b || !scores || M <= 0 || D <= 0) return LTRX_EINVAL;
  int g = (M + 3) / 4;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(ltrx_score_head_fwd_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, x, w, b, M, D, scores);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

extern "C" size_t ltrx_score_head_bwd_workspace_bytes(int M, int D) {
  if (M <= 0 || D <= 0) return 0;
  return (size_t)head_grid(M) * (D + 1) * sizeof(float);
}

extern "C" int ltrx_score_head_bwd(const float* dscores, const float* x, const float* w, int M, int D, float* dx,
                                   float* dw, float* db, void* ws, ltrx_stream_t stream) {
  if (!dscores || !x || !w || !dx || !dw || !db || !ws || M <= 0 || D <= 0) return LTRX_EINVAL;
  if ((size_t)(4 * D + 4) * sizeof(float) > 64 * 1024) return LTRX_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int g = head_grid(M);
  const bool al16 = ((((uintptr_t)x) | ((uintptr_t)dx) | ((uintptr_t)w)) & 15) == 0;
  if (D == 256 && al16)
    hipLaunchKernelGGL(ltrx_score_head_bwd_vec_kernel<1>, dim3(g), dim3(256), 0, s, dscores, x, w, M, dx, (float*)ws);
  else if (D == 512 && al16)
    hipLaunchKernelGGL(ltrx_score_head_bwd_vec_kernel<2>, dim3(g), dim3(256), 0, s, dscores, x, w, M, dx, (float*)ws);
  else if (D == 1024 && al16)
    hipLaunchKernelGGL(ltrx_score_head_bwd_vec_kernel<4>, dim3(g), dim3(256), 0, s, dscores, x, w, M, dx, (float*)ws);
  else
    hipLaunchKernelGGL(ltrx_score_head_bwd_kernel, dim3(g), dim3(256), (size_t)(4 * D + 4) * sizeof(float), s, dscores, x, w, M,
                       D, dx, (float*)ws);
  LTRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ltrx_score_head_reduce_kernel, dim3((D + 1 + 63) / 64), dim3(1024), 0, s, (const float*)ws, g, D, dw, db);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// dw / db of ltrx_score_head_bwd for x = LN(xsum; a, b) given by xsum and the saved statistics, bit for bit (ws: the same bytes)
extern "C" int ltrx_norm_head_wgrad(const float* dscores, const float* xsum, const float* a, const float* b, const float* mean,
                                    const float* rstd, int M, int D, float* dw, float* db, void* ws, ltrx_stream_t stream) {
  if (!dscores || !xsum || !a || !b || !mean || !rstd || !dw || !db || !ws || M <= 0 || D < 2) return LTRX_EINVAL;
  if (D % 256 != 0 || D > 1024 || ((((uintptr_t)xsum) | ((uintptr_t)a) | ((uintptr_t)b)) & 15) != 0) return LTRX_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int g = head_grid(M);
  ltrx_rowreg_dispatch(D, [&](auto nv) {
    hipLaunchKernelGGL(ltrx_norm_head_wgrad_kernel<decltype(nv)::value>, dim3(g), dim3(256), 0, s, dscores, xsum, a, b, mean, rstd, M,
                       (float*)ws);
  });
  LTRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ltrx_score_head_reduce_kernel, dim3((D + 1 + 63) / 64), dim3(1024), 0, s, (const float*)ws, g, D, dw, db);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// dropout plumbing of the explicit step: dst[i] = src[i] * keep_scale(i)  (the backward of a dropped residual branch /
// identity-activation FC output), and the per-step word that re-keys every dropout site at each hipGraph replay.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ltrx_dropout_apply_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t n,
                                                                 DropSpec drop, const uint32_t* __restrict__ drop_step) {
  if (drop_step) drop.seed ^= drop_step[0] * 0x9E3779B9u;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i] * drop_keep_scale(drop, (uint64_t)i);
}

extern "C" int ltrx_dropout_apply(const float* src, float* dst, size_t n, float p, uint32_t seed, const uint32_t* drop_step,
                                  ltrx_stream_t stream) {
  if (!src || !dst || n == 0 || !(p >= 0.f) || p >= 1.f) return LTRX_EINVAL;
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(ltrx_dropout_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, n,
                     ltrx_make_drop(p, seed), drop_step);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

__global__ void ltrx_bump_u32_kernel(uint32_t* __restrict__ w) { w[0] += 1u; }

extern "C" int ltrx_bump_u32(uint32_t* word, ltrx_stream_t stream) {
  if (!word) return LTRX_EINVAL;
  hipLaunchKernelGGL(ltrx_bump_u32_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, word);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Batched transpose: every weight matrix the input-gradient GEMMs need in transposed (K-contiguous) form, refreshed after
// the optimizer step by ONE launch.  desc[m] = {src offset, dst offset, rows, cols} in floats relative to the two base
// pointers; tile_start[m] = first workgroup of matrix m (32 x 32 tiles, row-major), tile_start[n] = total.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ltrx_transpose_batch_kernel(const float* __restrict__ src_base, float* __restrict__ dst_base,
                                                                   const int64_t* __restrict__ desc,
                                                                   const int32_t* __restrict__ tile_start, int n) {
  __shared__ float tile[32][33];
  int m = 0;
  while (m + 1 < n && (int)blockIdx.x >= tile_start[m + 1]) ++m;
  const int64_t so = desc[4 * m + 0], dof = desc[4 * m + 1];
  const int rows = (int)desc[4 * m + 2], cols = (int)desc[4 * m + 3];
  const int t = blockIdx.x - tile_start[m];
  const int tiles_c = (cols + 31) / 32;
  const int r0 = (t / tiles_c) * 32, c0 = (t % tiles_c) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
  const float* src = src_base + so;
  float* dst = dst_base + dof;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + 8 * k, c = c0 + tx;
    if (r < rows && c < cols) tile[ty + 8 * k][tx] = src[(size_t)r * cols + c];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + 8 * k, r = r0 + tx;              // dst[c][r] = src[r][c]
    if (r < rows && c < cols) dst[(size_t)c * rows + r] = tile[tx][ty + 8 * k];
  }
}

extern "C" int ltrx_transpose_batch(const float* src_base, float* dst_base, const int64_t* desc, const int32_t* tile_start,
                                    int n, int total_tiles, ltrx_stream_t stream) {
  if (!src_base || !dst_base || !desc || !tile_start || n <= 0 || total_tiles <= 0) return LTRX_EINVAL;
  hipLaunchKernelGGL(ltrx_transpose_batch_kernel, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, src_base, dst_base, desc,
                     tile_start, n);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// The whole per-step weight-image refresh in ONE launch (it was a transpose launch and two image launches, the second re-reading
// the transposed copies): workgroups 0 .. total_tiles-1 transpose their 32 x 32 tile and write BOTH the fp32 transposed copy and its
// pre-split bf16 hi/lo image (each thread owns 4 consecutive elements of a transposed row = one 16-byte image group); the remaining
// workgroups split the untransposed flat parameter buffer.  Needs every transposed matrix to have rows % 4 == 0 (the image groups
// of 4 must not straddle a transposed row) -- the host checks and otherwise keeps the three-launch form.
struct LtrxPadJob {
  const float* src;
  float* dst;
  void* dst_image;
  int rows, cols, ld;
};
__global__ void __launch_bounds__(256) ltrx_weight_images_kernel(const float* __restrict__ src_base, float* __restrict__ dst_base,
                                                                 float4* __restrict__ dst_image, const int64_t* __restrict__ desc,
                                                                 const int32_t* __restrict__ tile_start, int n, int total_tiles,
                                                                 float4* __restrict__ src_image, size_t nflat4, int flat_blocks,
                                                                 LtrxPadJob pad) {
  if ((int)blockIdx.x >= total_tiles + flat_blocks) {
    // row-padded copy of one matrix (the first FC weight [rows][cols] -> [rows][ld], so that its K extent is a multiple of the
    // GEMM's 32-column step): fp32 copy and image; the padding columns keep the zeros they were allocated with
    // (cols % 4 != 0: the source rows are no longer 16-byte aligned -- scalar loads, and the last group of a row carries the row's tail
    //  followed by zeros, i.e. it rewrites pad columns with the zeros they hold)
    const int c4 = (pad.cols + 3) >> 2, l4 = pad.ld >> 2;
    const bool vec = (pad.cols & 3) == 0;
    const size_t tot = (size_t)pad.rows * c4, nb = gridDim.x - total_tiles - flat_blocks;
    for (size_t i = (size_t)(blockIdx.x - total_tiles - flat_blocks) * blockDim.x + threadIdx.x; i < tot; i += nb * blockDim.x) {
      const size_t r = i / c4;
      const int c = (int)(i - r * c4);
      float4 v;
      if (vec) {
        v = reinterpret_cast<const float4*>(pad.src)[i];
      } else {
        const float* sr = pad.src + r * pad.cols;
        const int c0 = 4 * c;
        v.x = sr[c0];                                            // (c0 < cols: c < ceil(cols / 4))
        v.y = c0 + 1 < pad.cols ? sr[c0 + 1] : 0.f;
        v.z = c0 + 2 < pad.cols ? sr[c0 + 2] : 0.f;
        v.w = c0 + 3 < pad.cols ? sr[c0 + 3] : 0.f;
      }
      reinterpret_cast<float4*>(pad.dst)[r * l4 + c] = v;
      reinterpret_cast<float4*>(pad.dst_image)[r * l4 + c] = ltrx_split_image4(v);
    }
    return;
  }
  if ((int)blockIdx.x >= total_tiles) {
    const size_t nb = flat_blocks;
    for (size_t i = (size_t)(blockIdx.x - total_tiles) * blockDim.x + threadIdx.x; i < nflat4; i += nb * blockDim.x)
      src_image[i] = ltrx_split_image4(reinterpret_cast<const float4*>(src_base)[i]);
    return;
  }
  __shared__ float tile[32][33];
  int m = 0;
  while (m + 1 < n && (int)blockIdx.x >= tile_start[m + 1]) ++m;
  const int64_t so = desc[4 * m + 0], dof = desc[4 * m + 1];
  const int rows = (int)desc[4 * m + 2], cols = (int)desc[4 * m + 3];
  const int t = blockIdx.x - tile_start[m];
  const int tiles_c = (cols + 31) / 32;
  const int r0 = (t / tiles_c) * 32, c0 = (t % tiles_c) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
  const float* src = src_base + so;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + 8 * k, c = c0 + tx;
    tile[ty + 8 * k][tx] = (r < rows && c < cols) ? src[(size_t)r * cols + c] : 0.f;
  }
  __syncthreads();
  const int cl = threadIdx.x >> 3, r4 = (threadIdx.x & 7) * 4;  // transposed row c0 + cl, its elements r0 + r4 .. + 3
  const int c = c0 + cl, r = r0 + r4;
  if (c < cols && r < rows) {                                   // (rows % 4 == 0: a group is inside the matrix or outside)
    const float4 v = make_float4(tile[r4][cl], tile[r4 + 1][cl], tile[r4 + 2][cl], tile[r4 + 3][cl]);
    const size_t o = (size_t)dof + (size_t)c * rows + r;        // multiple of 4: dof and rows are
    *reinterpret_cast<float4*>(dst_base + o) = v;
    dst_image[o >> 2] = ltrx_split_image4(v);
  }
}

extern "C" int ltrx_weight_images(const float* src_base, size_t nflat, void* src_image, float* dst_base, void* dst_image,
                                  const int64_t* desc, const int32_t* tile_start, int n, int total_tiles, const float* pad_src,
                                  int pad_rows, int pad_cols, int pad_ld, float* pad_dst, void* pad_dst_image, ltrx_stream_t stream) {
  LtrxPadJob pad = {pad_src, pad_dst, pad_dst_image, pad_rows, pad_cols, pad_ld};
  if (pad_src) {
    if (!pad_dst || !pad_dst_image || pad_rows <= 0 || pad_cols <= 0 || pad_ld < (pad_cols + 3) / 4 * 4 || (pad_ld & 3) ||
        (((uintptr_t)pad_src | (uintptr_t)pad_dst | (uintptr_t)pad_dst_image) & 15))
      return LTRX_EINVAL;
  }
  if (!src_base || !src_image || (nflat & 3) || (((uintptr_t)src_base | (uintptr_t)src_image) & 15)) return LTRX_EINVAL;
  if (n < 0 || total_tiles < 0 || (n > 0 && (!dst_base || !dst_image || !desc || !tile_start || total_tiles <= 0))) return LTRX_EINVAL;
  if (n > 0 && (((uintptr_t)dst_base | (uintptr_t)dst_image) & 15)) return LTRX_EINVAL;
  if (n == 0) total_tiles = 0;
  size_t blocks = (nflat / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  size_t pblocks = pad_src ? ((size_t)pad_rows * ((pad_cols + 3) / 4) + 255) / 256 : 0;
  if (pblocks > 256) pblocks = 256;
  if (blocks == 0 && total_tiles == 0 && pblocks == 0) return LTRX_OK;
  hipLaunchKernelGGL(ltrx_weight_images_kernel, dim3((unsigned)(total_tiles + blocks + pblocks)), dim3(256), 0, (hipStream_t)stream,
                     src_base, dst_base, reinterpret_cast<float4*>(dst_image), desc, tile_start, n, total_tiles,
                     reinterpret_cast<float4*>(src_image), nflat / 4, (int)blocks, pad);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// One launch that takes a batch into the step's static input buffers (they are what a captured hipGraph reads): x and y copied,
// the padding mask y == pad_value written next to them (it was four launches: two copies, a compare, a bool copy).
__global__ void __launch_bounds__(256) ltrx_ingest_batch_kernel(const float* __restrict__ x, const float* __restrict__ y, size_t nx,
                                                                size_t ny, float pad_value, float* __restrict__ x_dst,
                                                                float* __restrict__ y_dst, unsigned char* __restrict__ mask_dst,
                                                                int x_blocks, int vec, int F, int ld_dst) {
  if ((int)blockIdx.x >= x_blocks) {
    const size_t i = (size_t)(blockIdx.x - x_blocks) * blockDim.x + threadIdx.x;
    if (i < ny) {
      const float v = y[i];
      y_dst[i] = v;
      mask_dst[i] = (v == pad_value) ? 1 : 0;
    }
    return;
  }
  const size_t stride = (size_t)x_blocks * blockDim.x;
  if (vec && ld_dst != F) {            // rows of F floats into rows of ld_dst floats (the padding columns are never written)
    const size_t n4 = nx >> 2;
    const int f4 = F >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const size_t r = i / f4;
      const int c = (int)(i - r * f4);
      reinterpret_cast<float4*>(x_dst + r * ld_dst)[c] = reinterpret_cast<const float4*>(x)[i];
    }
  } else if (vec) {
    const size_t n4 = nx >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
      reinterpret_cast<float4*>(x_dst)[i] = reinterpret_cast<const float4*>(x)[i];
  } else if (ld_dst != F) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nx; i += stride) x_dst[(i / F) * ld_dst + (i % F)] = x[i];
  } else {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nx; i += stride) x_dst[i] = x[i];
  }
}

extern "C" int ltrx_ingest_batch(const float* x, const float* y, size_t nx, size_t ny, int F, int ld_dst, float pad_value, float* x_dst,
                                 float* y_dst, unsigned char* mask_dst, ltrx_stream_t stream) {
  if (!y || !y_dst || !mask_dst || ny == 0 || (nx > 0 && (!x || !x_dst))) return LTRX_EINVAL;
  if (nx > 0 && (F <= 0 || ld_dst < F || nx % (size_t)F)) return LTRX_EINVAL;
  if (nx == 0) F = ld_dst = 1;
  const int vec = ((nx & 3) == 0 && (F & 3) == 0 && (ld_dst & 3) == 0 && (((uintptr_t)x | (uintptr_t)x_dst) & 15) == 0) ? 1 : 0;
  size_t xb = ((vec ? nx / 4 : nx) + 255) / 256;
  if (xb > 4096) xb = 4096;
  const size_t yb = (ny + 255) / 256;
  hipLaunchKernelGGL(ltrx_ingest_batch_kernel, dim3((unsigned)(xb + yb)), dim3(256), 0, (hipStream_t)stream, x, y, nx, ny, pad_value,
                     x_dst, y_dst, mask_dst, (int)xb, vec, F, ld_dst);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Row gather / scatter for compacted (variable-length) batches: the valid items of a padded [B, L] batch are packed into
// consecutive rows before the row-wise part of the step (dataset.py:28-38 pads every slate to the batch's slate length;
// the padded rows carry no gradient and are masked out as attention keys, so the step never needs them).
//   gather : dst[i, :] = src[idx[i], :]  for i < n, and dst[i, :] = 0 for n <= i < n_pad (alignment rows)
//   scatter: dst[idx[i], :] = src[i, :]  for i < n
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ltrx_gather_rows_kernel(const float* __restrict__ src, int ld_src,
                                                               const int32_t* __restrict__ idx, int n, int n_pad, int cols,
                                                               float* __restrict__ dst, int ld_dst) {
  const size_t total = (size_t)n_pad * cols;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / cols), c = (int)(e % cols);
    dst[(size_t)r * ld_dst + c] = (r < n) ? src[(size_t)idx[r] * ld_src + c] : 0.f;
  }
}
__global__ void __launch_bounds__(256) ltrx_scatter_rows_kernel(const float* __restrict__ src, int ld_src,
                                                                const int32_t* __restrict__ idx, int n, int cols,
                                                                float* __restrict__ dst, int ld_dst) {
  const size_t total = (size_t)n * cols;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / cols), c = (int)(e % cols);
    dst[(size_t)idx[r] * ld_dst + c] = src[(size_t)r * ld_src + c];
  }
}

// packed row r of a cu_seqlens layout whose slates keep their valid items first (dataset.py:28-38 pads at the end):
// idx[r] = b * L + (r - cu[b]) with cu[b] <= r < cu[b+1]  (binary search over the B+1 prefix sums)
__global__ void __launch_bounds__(256) ltrx_packed_row_index_kernel(const int32_t* __restrict__ cu, int B, int L, int n,
                                                                    int32_t* __restrict__ idx) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  int lo = 0, hi = B;                 // invariant: cu[lo] <= r < cu[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= r) lo = mid; else hi = mid;
  }
  idx[r] = lo * L + (r - cu[lo]);
}

static inline int row_copy_grid(size_t total) {
  size_t g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

extern "C" int ltrx_gather_rows(const float* src, int ld_src, const int32_t* idx, int n, int n_pad, int cols, float* dst,
                                int ld_dst, ltrx_stream_t stream) {
  if (!src || !idx || !dst || n < 0 || n_pad < n || cols <= 0 || ld_src < cols || ld_dst < cols) return LTRX_EINVAL;
  if (n_pad == 0) return LTRX_OK;
  hipLaunchKernelGGL(ltrx_gather_rows_kernel, dim3(row_copy_grid((size_t)n_pad * cols)), dim3(256), 0, (hipStream_t)stream, src,
                     ld_src, idx, n, n_pad, cols, dst, ld_dst);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

extern "C" int ltrx_packed_row_index(const int32_t* cu_seqlens, int B, int L, int n, int32_t* idx, ltrx_stream_t stream) {
  if (!cu_seqlens || !idx || B <= 0 || L <= 0 || n < 0 || (size_t)n > (size_t)B * L) return LTRX_EINVAL;
  if (n == 0) return LTRX_OK;
  hipLaunchKernelGGL(ltrx_packed_row_index_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, cu_seqlens, B, L, n, idx);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

extern "C" int ltrx_scatter_rows(const float* src, int ld_src, const int32_t* idx, int n, int cols, float* dst, int ld_dst,
                                 ltrx_stream_t stream) {
  if (!src || !idx || !dst || n < 0 || cols <= 0 || ld_src < cols || ld_dst < cols) return LTRX_EINVAL;
  if (n == 0) return LTRX_OK;
  hipLaunchKernelGGL(ltrx_scatter_rows_kernel, dim3(row_copy_grid((size_t)n * cols)), dim3(256), 0, (hipStream_t)stream, src,
                     ld_src, idx, n, cols, dst, ld_dst);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Gradient clipping (torch.nn.utils.clip_grad_norm_, train_utils.py:24-25) for the flat gradient buffer:
// scale_out[0] = min(1, max_norm / (||g||_2 + 1e-6)); the Adam kernel multiplies the gradients by it on the fly.
// Two-stage deterministic sum of squares (grid-stride partials, then one block).
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ltrx_sumsq_partial_kernel(const float* __restrict__ g, size_t n, float* __restrict__ partial) {
  __shared__ float red[LTRX_MAX_WAVES];
  float acc = 0.f;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) acc += g[i] * g[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ void __launch_bounds__(256) ltrx_clip_scale_kernel(const float* __restrict__ partial, int nb, float max_norm,
                                                              float* __restrict__ scale_out, float* __restrict__ norm_out) {
  __shared__ float red[LTRX_MAX_WAVES];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) acc += partial[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(acc);
    const float c = max_norm / (norm + 1e-6f);            // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6)
    scale_out[0] = c < 1.0f ? c : 1.0f;
    if (norm_out) norm_out[0] = norm;
  }
}

extern "C" size_t ltrx_clip_workspace_bytes(size_t n) {
  (void)n;
  return 1024 * sizeof(float);
}

extern "C" int ltrx_clip_grad_norm_scale(const float* grads, size_t n, float max_norm, float* scale_out, float* norm_out, void* ws,
                                         ltrx_stream_t stream) {
  if (!grads || !scale_out || !ws || n == 0 || !(max_norm > 0.f)) return LTRX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  size_t nb = (n + 255) / 256;
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(ltrx_sumsq_partial_kernel, dim3((unsigned)nb), dim3(256), 0, s, grads, n, (float*)ws);
  LTRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ltrx_clip_scale_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, (int)nb, max_norm, scale_out, norm_out);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Finiteness check of the explicit step (round 6).  main.py:89 wraps fit() in torch.autograd.detect_anomaly() when
// config.detect_anomaly is set; the explicit step has no autograd graph for that mode to watch, so allrank_amd.fit checks the loss
// and the flat gradient buffer itself: ONE launch over the buffer, result = (index of the first segment -- parameter tensor, in
// flat-buffer order -- that holds a NaN / Inf, 0x7fffffff if none; number of non-finite elements), read back with one host sync.
// HBM-bound: 4 B per element read once with 16-byte loads (25.5 MB at config 3: ~5 us).
// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ltrx_first_nonfinite_kernel(const float* __restrict__ buf, size_t n,
                                                                   const int64_t* __restrict__ seg_start, int n_seg,
                                                                   int* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  int first = 0x7fffffff, count = 0;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (i + 4 <= n) {
      const float4 q = *reinterpret_cast<const float4*>(buf + i);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
      for (size_t k = 0; i + k < n; ++k) v[k] = buf[i + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // NaN / Inf: exponent field all ones
      if ((__float_as_uint(v[k]) & 0x7F800000u) == 0x7F800000u) {
        ++count;
        // the segment of element i + k: the last start <= i + k (binary search over the sorted starts)
        int lo = 0, hi = n_seg - 1;
        const int64_t e = (int64_t)(i + k);
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (seg_start[mid] <= e) lo = mid;
          else hi = mid - 1;
        }
        first = min(first, lo);
      }
    }
  }
  if (count) {
    atomicMin(&out[0], first);
    atomicAdd(&out[1], count);
  }
}

__global__ void ltrx_first_nonfinite_init_kernel(int* __restrict__ out) {
  out[0] = 0x7fffffff;
  out[1] = 0;
}

extern "C" int ltrx_first_nonfinite(const float* buf, size_t n, const int64_t* seg_start, int n_seg, int* out, ltrx_stream_t stream) {
  if (!buf || !seg_start || !out || n == 0 || n_seg <= 0) return LTRX_EINVAL;
  if ((uintptr_t)buf & 15) return LTRX_EINVAL;
  hipLaunchKernelGGL(ltrx_first_nonfinite_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, out);
  const size_t quads = (n + 3) / 4;
  const unsigned grid = (unsigned)((quads + 255) / 256 < 2048 ? (quads + 255) / 256 : 2048);
  hipLaunchKernelGGL(ltrx_first_nonfinite_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, buf, n, seg_start, n_seg, out);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}
