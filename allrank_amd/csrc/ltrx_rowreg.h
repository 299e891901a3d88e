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
// The workgroup's (da, db) partials in two halves, so that a kernel whose waves stand in for another launch shape's (rowreg_ln_bwd_side
// below) states the same stores and the same sum.  Spill: wave w writes its da / db to lds[WPB][2][D].  Sum, after a workgroup barrier:
// prow[c], c < 2 D (the workgroup's row of the partials) is the sum of the WPB spilled rows in wave order, one thread per column --
// which thread takes which column does not enter the result.  Macros for the reason above; WPB may be a run-time value.
#define LTRX_ROWREG_LN_SPILL(NV, lds, lane, w, da, db)                                               \
  do {                                                                                             \
    _Pragma("unroll") for (int t = 0; t < NV; ++t) {                                               \
      reinterpret_cast<float4*>(lds + (size_t)w * 2 * (256 * NV))[lane + 64 * t] = da[t];          \
      reinterpret_cast<float4*>(lds + (size_t)w * 2 * (256 * NV) + 256 * NV)[lane + 64 * t] = db[t]; \
    }                                                                                              \
  } while (0)
#define LTRX_ROWREG_LN_SUM(NV, WPB, lds, prow)                                                       \
  do {                                                                                             \
    for (int c = threadIdx.x; c < 2 * (256 * NV); c += blockDim.x) {                               \
      float sacc = 0.f;                                                                            \
      for (int ww = 0; ww < WPB; ++ww) sacc += lds[(size_t)ww * 2 * (256 * NV) + c];               \
      (prow)[c] = sacc;                                                                            \
    }                                                                                              \
  } while (0)
// a launch whose workgroup IS the block of WPB waves: the kernel's NV, WPB, lane and w, the rest are lvalues
#define LTRX_ROWREG_LN_COMBINE(NV, WPB, lds, lane, w, da, db, prow)                                  \
  do {                                                                                             \
    LTRX_ROWREG_LN_SPILL(NV, lds, lane, w, da, db);                                                \
    __syncthreads();                                                                               \
    LTRX_ROWREG_LN_SUM(NV, WPB, lds, prow);                                                        \
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

// ---- the plain LayerNorm backward (ltrx_layernorm_bwd_vec_kernel<NV, WPB> on `grid` workgroups) as a SIDE JOB of another launch ----
// The grouped weight-gradient launch (ltrx_gemm_tn256_kernel, csrc/ltrx_gemm.hip) keeps one 8-wave workgroup per CU and leaves
// 256 - tiles x splits CUs without one; those run this instead.  Bit for bit what the stand-alone kernel writes: side workgroup s of
// `side` plays the virtual blocks s, s + side, ... of that launch, its 8 waves standing in for a block's wpb waves (wpb 16: two passes
// of 8; wpb 4: two blocks at once).  A virtual wave walks the rows of the real one (row = vb * wpb + vw; row += grid * wpb) and
// accumulates da / db in that order; the block's partial row is LTRX_ROWREG_LN_SUM over the spilled rows as in the kernel; a virtual
// block without rows writes its zero row.  Few CUs carry the stream, so a wave keeps two rows in flight: the loads of the next row are
// issued before the arithmetic of the current one (only WHEN a load is issued differs from the kernel, no expression does).
struct LnBwdJob {
  const float *dy, *xsum, *a, *mean, *rstd, *dres;
  float *dx, *partial;
  int rows, grid, wpb;               // the stand-alone launch shape (ln_bwd_shape): wpb is 4 or 16
  float eps;
};
// lds: side_lds_floats(NV, wpb) floats; s: this workgroup's index among the `side` side workgroups; blockDim.x = 512
__host__ __device__ constexpr int rowreg_ln_side_par(int wpb) { return wpb < 8 ? 8 / wpb : 1; }       // virtual blocks played at once
__host__ __device__ constexpr size_t rowreg_ln_side_lds_floats(int D, int wpb) { return (size_t)rowreg_ln_side_par(wpb) * wpb * 2 * D; }
template <int NV>
__device__ __forceinline__ void rowreg_ln_bwd_side(const LnBwdJob& j, int s, int side, float* __restrict__ lds) {
  constexpr int D = 256 * NV;
  const float* __restrict__ dy = j.dy;
  const float* __restrict__ xsum = j.xsum;
  const float* __restrict__ dres = j.dres;
  const float* __restrict__ mean_in = j.mean;
  const float* __restrict__ rstd_in = j.rstd;
  float* __restrict__ dx = j.dx;
  const int rows = j.rows, grid = j.grid, wpb = j.wpb;
  const float eps = j.eps;
  const int lane = lane_id(), w = wave_id();
  const int par = rowreg_ln_side_par(wpb), passes = wpb > 8 ? wpb / 8 : 1;
  const int vslot = wpb < 8 ? w / wpb : 0;                  // which of the blocks played at once this wave belongs to
  float* slot = lds + (size_t)vslot * wpb * 2 * D;
  const int row_step = grid * wpb;
  float4 av[NV];
#pragma unroll
  for (int t = 0; t < NV; ++t) av[t] = reinterpret_cast<const float4*>(j.a)[lane + 64 * t];
  for (int k0 = 0; s + k0 * side < grid; k0 += par) {       // (workgroup-uniform)
    const int vb = s + (k0 + vslot) * side;
    for (int ps = 0; ps < passes; ++ps) {
      const int vw = wpb < 8 ? w % wpb : w + 8 * ps;
      float4 da[NV], db[NV];
#pragma unroll
      for (int t = 0; t < NV; ++t) {
        da[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        db[t] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      // two row buffers, addressed by compile-time constants only (registers)
      float4 g[2][NV], xs[2][NV], dr[2][NV];
      float mean[2], r[2];
      auto load = [&](auto bc, int row) {
        constexpr int b = decltype(bc)::value;
        mean[b] = mean_in[row];
        r[b] = rstd_in[row];
#pragma unroll
        for (int t = 0; t < NV; ++t) {
          g[b][t] = reinterpret_cast<const float4*>(dy + (size_t)row * D)[lane + 64 * t];
          xs[b][t] = reinterpret_cast<const float4*>(xsum + (size_t)row * D)[lane + 64 * t];
          if (dres) dr[b][t] = reinterpret_cast<const float4*>(dres + (size_t)row * D)[lane + 64 * t];
        }
        __builtin_amdgcn_sched_barrier(0);                    // the loads stay ahead of the other row's arithmetic
      };
      auto work = [&](auto bc, int row) {
        constexpr int b = decltype(bc)::value;
        float gsum = 0.f, dot = 0.f;
#pragma unroll
        for (int t = 0; t < NV; ++t) {
          xs[b][t].x -= mean[b]; xs[b][t].y -= mean[b]; xs[b][t].z -= mean[b]; xs[b][t].w -= mean[b];
          LTRX_ROWREG_BWD_ACC(g[b][t], xs[b][t], av[t], r[b], da[t], db[t], gsum, dot);
        }
        float gm, tc;
        rowreg_bwd_coef<NV>(gsum, dot, r[b], eps, gm, tc);
#pragma unroll
        for (int t = 0; t < NV; ++t) {
          float4 o = rowreg_bwd_dx(g[b][t], xs[b][t], r[b], gm, tc);
          if (dres) {
            const float4 d = dr[b][t];
            o.x += d.x; o.y += d.y; o.z += d.z; o.w += d.w;
          }
          reinterpret_cast<float4*>(dx + (size_t)row * D)[lane + 64 * t] = o;
        }
      };
      const std::integral_constant<int, 0> b0{};
      const std::integral_constant<int, 1> b1{};
      int row = vb < grid ? vb * wpb + vw : rows;
      if (row < rows) load(b0, row);
      while (row < rows) {
        int nx = row + row_step;
        if (nx < rows) load(b1, nx);
        work(b0, row);
        row = nx;
        if (row >= rows) break;
        nx = row + row_step;
        if (nx < rows) load(b0, nx);
        work(b1, row);
        row = nx;
      }
      LTRX_ROWREG_LN_SPILL(NV, slot, lane, vw, da, db);
    }
    __syncthreads();
    for (int q = 0; q < par; ++q) {
      const int vbq = s + (k0 + q) * side;
      if (vbq < grid) LTRX_ROWREG_LN_SUM(NV, wpb, (lds + (size_t)q * wpb * 2 * D), j.partial + (size_t)vbq * 2 * D);
    }
    __syncthreads();                                          // the spill rows are reused by the next blocks
  }
}

}  // namespace ltrx

// Host side: launch shape of the register-resident LayerNorm backward kernels (plain, norm + head, and the side job above): the grid
// and the waves per workgroup, decided in csrc/ltrx_layernorm.hip (ln_bwd_shape)
struct LnBwdShape { int grid, wpb; };
LnBwdShape ltrx_ln_bwd_shape(int rows, int D);
// the register-resident row layout holds D and these pointers
static inline bool ln_vec_ok(int D, const void* p0, const void* p1, const void* p2) {
  return D % 256 == 0 && D <= 1024 && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 15) == 0;
}

// f(std::integral_constant<int, NV>) for the NV of a width D = 256 * NV <= 1024 (1, 2, 3 -> themselves, else 4)
template <typename F>
static inline void ltrx_rowreg_dispatch(int D, F&& f) {
  switch (D / 256) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
