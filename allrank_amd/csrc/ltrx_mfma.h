// The vocabulary the matrix-core (MFMA) kernels share: ltrx_gemm.hip, ltrx_mha.hip, ltrx_mha_res.hip, ltrx_fcstep.hip.
#pragma once
#include "ltrx_device.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef bf16x4 __attribute__((address_space(3))) * lds_bf16x4_ptr;

namespace ltrx {

// row (of a 32 x 32 MFMA result tile) that register r of a lane in half `half` (lane >> 5) of the wave holds
__device__ __forceinline__ int rowmap(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// barrier that orders LDS only: __syncthreads() also drains vmcnt(0), i.e. it would wait at every tile for the global loads of
// the NEXT tile that were issued just before it (and for the touch_line requests)
__device__ __forceinline__ void lds_only_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Dropout on the attention probabilities (transformer.py:154-155): counter-based, two-level -- a fully mixed 32-bit seed
// per (slate*head, query) row and a short 2-multiply mix per key, so the per-element cost is ~8 VALU operations with 32-bit
// arithmetic only.  The forward and both backward kernels regenerate the same mask from (seed, row, key) -- and so do the kernels
// of the two attention paths (ltrx_mha.hip, ltrx_mha_res.hip), whose forward and backward are interchangeable: this is the one draw.
typedef DropSpec DropCfg;
__device__ __forceinline__ uint32_t drop_row_seed(const DropCfg& d, uint32_t bh, int L, int qrow) {
  return fmix32(d.seed ^ ((bh * (uint32_t)L + (uint32_t)qrow) * 0x9E3779B9u));
}
__device__ __forceinline__ float drop_scale_rk(const DropCfg& d, uint32_t row_seed, int key) {
  uint32_t x = (row_seed ^ (uint32_t)key) * 0x9E3779B1u;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  return ((x >> 8) >= d.thresh) ? d.inv_keep : 0.f;
}

}  // namespace ltrx
