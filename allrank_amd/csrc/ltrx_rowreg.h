// The register-resident row, D = 256 * NV (NV = 1..4): lane l of a wave holds float4 columns 4 * (l + 64 * t), t < NV.  The LayerNorm
// row arithmetic and the two per-workgroup partial combines on that layout are stated here once, so the plain kernels
// (ltrx_layernorm.hip), the fused final norm + score head (same file) and the head's weight gradients (ltrx_train.hip) agree bit for
// bit by construction, as does their host-side NV dispatch.  Three steps are macros, not functions: see LTRX_ROWREG_BWD_ACC.
#pragma once
#include <type_traits>

#include "ltrx_device.h"

namespace ltrx {

// mean and r = 1 / (std + eps) (unbiased std) of the row in v[]; `sum` is the lane's sum of its columns, pairwise per float4
template <int NV>
__device__ __forceinline__ void rowreg_stats(const float4 (&v)[NV], float sum, float eps, float& mean, float& r) {
  constexpr int D = 256 * NV;
  mean = wave_sum(sum) / (float)D;
  float sq = 0.f;
#pragma unroll
  for (int t = 0; t < NV; ++t) {
    const float dx = v[t].x - mean, dy = v[t].y - mean, dz = v[t].z - mean, dw = v[t].w - mean;
    sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
  }
  const float stdv = sqrtf(wave_sum(sq) / (float)(D - 1));
  r = 1.0f / (stdv + eps);
}

// y = a * xhat + b.  One expression for every caller also means one fma contraction of a * t + b under the build's default
// -ffp-contract, which the bit comparisons of tests/test_gpu_norm_head.py (y, scores, head gradients) depend on.
__device__ __forceinline__ float4 rowreg_affine(const float4 a, const float4 v, float mean, float r, const float4 b) {
  float4 o;
  o.x = a.x * ((v.x - mean) * r) + b.x;
  o.y = a.y * ((v.y - mean) * r) + b.y;
  o.z = a.z * ((v.z - mean) * r) + b.z;
  o.w = a.w * ((v.w - mean) * r) + b.w;
  return o;
}

// Backward of one row, dx = r (g - mean(g)) - tc xc with g = dy * a, in three steps that the kernels wrap in their own loads and stores.
// Step 1, per float4: da / db accumulate on the raw dy in g, then g becomes dy * a and feeds the lane's gsum and dot.  A macro: with
// g, da and db passed by reference the optimiser orders some instantiations' instructions differently, and the ISA is held fixed.
// g, da, db, gsum and dot are read and written, the rest only read; every argument is a side-effect-free lvalue (evaluated many times).
#define LTRX_ROWREG_BWD_ACC(g, xc, av, r, da, db, gsum, dot)                                   \
  do {                                                                                         \
    da.x += g.x * (xc.x * r); da.y += g.y * (xc.y * r);                                        \
    da.z += g.z * (xc.z * r); da.w += g.w * (xc.w * r);                                        \
    db.x += g.x; db.y += g.y; db.z += g.z; db.w += g.w;                                        \
    g.x *= av.x; g.y *= av.y; g.z *= av.z; g.w *= av.w;                                        \
    gsum += (g.x + g.y) + (g.z + g.w);                                                         \
    dot += (g.x * xc.x + g.y * xc.y) + (g.z * xc.z + g.w * xc.w);                              \
  } while (0)
// Step 2, per row: gm = mean(g) and tc = r^2 <g, xc> / ((D - 1) std), 0 for a constant row (std = 1 / r - eps = 0)
template <int NV>
__device__ __forceinline__ void rowreg_bwd_coef(float gsum, float dot, float r, float eps, float& gm, float& tc) {
  constexpr int D = 256 * NV;
  gm = wave_sum(gsum) / (float)D;
  dot = wave_sum(dot);
  const float stdv = 1.0f / r - eps;
  tc = (stdv > 0.f) ? r * r * dot / ((float)(D - 1) * stdv) : 0.f;
}
// Step 3, per float4
__device__ __forceinline__ float4 rowreg_bwd_dx(const float4 g, const float4 xc, float r, float gm, float tc) {
  float4 o;
  o.x = r * (g.x - gm) - tc * xc.x;
  o.y = r * (g.y - gm) - tc * xc.y;
  o.z = r * (g.z - gm) - tc * xc.z;
  o.w = r * (g.w - gm) - tc * xc.w;
  return o;
}
// The workgroup's (da, db) partials: wave w spills its da / db to lds[WPB][2][D], then prow[c], c < 2 D (the workgroup's row of the
// partials) is their sum in wave order.  A macro for the reason above; the kernel's NV, WPB, lane and w, the rest are lvalues.
#define LTRX_ROWREG_LN_COMBINE(NV, WPB, lds, lane, w, da, db, prow)                                  \
  do {                                                                                             \
    _Pragma("unroll") for (int t = 0; t < NV; ++t) {                                               \
      reinterpret_cast<float4*>(lds + (size_t)w * 2 * (256 * NV))[lane + 64 * t] = da[t];          \
      reinterpret_cast<float4*>(lds + (size_t)w * 2 * (256 * NV) + 256 * NV)[lane + 64 * t] = db[t]; \
    }                                                                                              \
    __syncthreads();                                                                               \
    for (int c = threadIdx.x; c < 2 * (256 * NV); c += blockDim.x) {                               \
      float sacc = 0.f;                                                                            \
      for (int ww = 0; ww < WPB; ++ww) sacc += lds[(size_t)ww * 2 * (256 * NV) + c];               \
      (prow)[c] = sacc;                                                                            \
    }                                                                                              \
  } while (0)
// The score head's (dw, db) partials of a four-wave workgroup: acc / dbacc to lds[4][D + 4], prow[c], c <= D, their pairwise sum -- at
// NV = 3, the one width ltrx_score_head_bwd gives to its scalar kernel, that kernel's wave-by-wave sum.
#define LTRX_ROWREG_HEAD_COMBINE(NV, lds, lane, wv, acc, dbacc, prow)                                             \
  do {                                                                                                          \
    _Pragma("unroll") for (int t = 0; t < NV; ++t) *reinterpret_cast<float4*>(&lds[wv][4 * (lane + 64 * t)]) = acc[t]; \
    if (lane == 0) lds[wv][256 * NV] = dbacc;                                                                   \
    __syncthreads();                                                                                            \
    for (int c = threadIdx.x; c <= 256 * NV; c += blockDim.x) {                                                 \
      float s = 0.f;                                                                                            \
      if (NV == 3) for (int k = 0; k < 4; ++k) s += lds[k][c];                                                  \
      else s = (lds[0][c] + lds[1][c]) + (lds[2][c] + lds[3][c]);                                               \
      (prow)[c] = s;                                                                                            \
    }                                                                                                           \
  } while (0)

}  // namespace ltrx

// Host side: f(std::integral_constant<int, NV>) for the NV of a width D = 256 * NV <= 1024 (1, 2, 3 -> themselves, else 4)
template <typename F>
static inline void ltrx_rowreg_dispatch(int D, F&& f) {
  switch (D / 256) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
