// Device-side helpers shared by the libltrx kernels (gfx950 / CDNA4, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <atomic>
#include <initializer_list>

#include "../../include/ltrx.h"

#define LTRX_WAVE 64
#define LTRX_MAX_WAVES 16  // 1024-thread workgroup

#define LTRX_LAUNCH_CHECK()                                   \
  do {                                                        \
    hipError_t e__ = hipGetLastError();                       \
    if (e__ != hipSuccess) return LTRX_EHIP - (int)e__;       \
  } while (0)

// One-time per-DEVICE setup (hipFuncSetAttribute applies to the current device's copy of a kernel): thread-safe, and the only
// process state the library keeps -- idempotent facts about loaded code, never a mode that changes results (ltrx.h: re-entrant).
template <typename F>
static inline int ltrx_once_per_device(std::atomic<uint64_t>& done, F&& setup) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return LTRX_EHIP;
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return LTRX_OK;
  const int rc = setup();            // two threads racing here both set the same attribute: harmless
  if (rc == LTRX_OK) done.fetch_or(bit, std::memory_order_release);
  return rc;
}

// Dynamic LDS beyond the default allowance.  hipFuncAttributeMaxDynamicSharedMemorySize is the opt-in of this API for a launch that asks
// for more dynamic LDS than a runtime grants by default.  What HIP requires on gfx950 was measured (ROCm 7.2, MI355X): nothing -- it reports
// the CU's whole 160 KB as sharedMemPerBlock, launches with 48 KB + 4 B, 64 KB + 4 B, 100 KB and 159 KB of dynamic LDS run without the
// attribute, and hip_runtime_api.h calls the attribute a hint that AMD devices may ignore.  So neither the "48 * 1024" nor the "default
// 64 KB" that the launchers used to quote is a limit of this runtime.  The opt-in stays because it costs one call per kernel and device and
// keeps the library independent of that default; its threshold is the smallest default behind this API, 48 KB (CUDA's), so no runtime sees
// a larger request unannounced.  A site whose kernels always need more opts in unconditionally, a site whose need depends on the shape
// only above the allowance; both go through this one function.  `done` is the site's per-device flag.
#define LTRX_DEFAULT_DYNAMIC_LDS_BYTES (48 * 1024)
struct LtrxDynLds {
  const void* kernel;
  size_t bytes;
  template <typename K>
  LtrxDynLds(K* k, size_t b) : kernel((const void*)k), bytes(b) {}
};
static inline int ltrx_allow_dynamic_lds(std::atomic<uint64_t>& done, std::initializer_list<LtrxDynLds> kernels) {
  return ltrx_once_per_device(done, [&]() {
    for (const LtrxDynLds& k : kernels)
      if (hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.bytes) != hipSuccess) return LTRX_EHIP;
    return LTRX_OK;
  });
}

// cut-off ranks of a metric call, passed to the kernel by value (ltrx_ndcg_at, ltrx_mrr_at)
#define LTRX_MAX_ATS 16

struct LtrxAts {
  int n;
  int at[LTRX_MAX_ATS];
};

namespace ltrx {

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

// ---- wave (64-lane) reductions on the DPP cross-lane network: four in-row steps (quad_perm x2, row_half_mirror,
// row_mirror: every lane of a 16-lane row holds the row total), two row broadcasts (row_bcast15 into rows 1 and 3,
// row_bcast31 into rows 2 and 3: lane 63 holds the wave total) and one v_readlane -- 7 VALU-rate instructions instead of
// six dependent ds_bpermute round trips through the LDS crossbar.  Every lane gets the result; the order is fixed.
#define LTRX_DPP_I(old, src, ctrl, rowmask, bound) __builtin_amdgcn_update_dpp((old), (src), (ctrl), (rowmask), 0xF, (bound))
#define LTRX_DPP_F(old, src, ctrl, rowmask, bound) \
  __builtin_bit_cast(float, LTRX_DPP_I(__builtin_bit_cast(int, (old)), __builtin_bit_cast(int, (src)), (ctrl), (rowmask), (bound)))
__device__ __forceinline__ float wave_sum(float v) {
  v += LTRX_DPP_F(0.f, v, 0xB1, 0xF, true);     // quad_perm [1,0,3,2]
  v += LTRX_DPP_F(0.f, v, 0x4E, 0xF, true);     // quad_perm [2,3,0,1]
  v += LTRX_DPP_F(0.f, v, 0x141, 0xF, true);    // row_half_mirror
  v += LTRX_DPP_F(0.f, v, 0x140, 0xF, true);    // row_mirror
  v += LTRX_DPP_F(0.f, v, 0x142, 0xA, false);   // row_bcast15 -> rows 1, 3
  v += LTRX_DPP_F(0.f, v, 0x143, 0xC, false);   // row_bcast31 -> rows 2, 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, LTRX_DPP_F(v, v, 0xB1, 0xF, false));
  v = fmaxf(v, LTRX_DPP_F(v, v, 0x4E, 0xF, false));
  v = fmaxf(v, LTRX_DPP_F(v, v, 0x141, 0xF, false));
  v = fmaxf(v, LTRX_DPP_F(v, v, 0x140, 0xF, false));
  v = fmaxf(v, LTRX_DPP_F(v, v, 0x142, 0xA, false));
  v = fmaxf(v, LTRX_DPP_F(v, v, 0x143, 0xC, false));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ int wave_sum_i(int v) {
  v += LTRX_DPP_I(0, v, 0xB1, 0xF, true);
  v += LTRX_DPP_I(0, v, 0x4E, 0xF, true);
  v += LTRX_DPP_I(0, v, 0x141, 0xF, true);
  v += LTRX_DPP_I(0, v, 0x140, 0xF, true);
  v += LTRX_DPP_I(0, v, 0x142, 0xA, false);
  v += LTRX_DPP_I(0, v, 0x143, 0xC, false);
  return __builtin_amdgcn_readlane(v, 63);
}

// ---- workgroup reductions: wave partials through LDS, summed in a fixed order (deterministic). ----
// `red` must hold LTRX_MAX_WAVES floats.  All threads of the block must call; all get the result.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();  // protect `red` from a previous use
  if (lane_id() == 0) red[wave_id()] = v;
  __syncthreads();
  const int nw = blockDim.x >> 6;
  float t = 0.f;
  for (int w = 0; w < nw; ++w) t += red[w];
  return t;
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if (lane_id() == 0) red[wave_id()] = v;
  __syncthreads();
  const int nw = blockDim.x >> 6;
  float t = red[0];
  for (int w = 1; w < nw; ++w) t = fmaxf(t, red[w]);
  return t;
}
__device__ __forceinline__ int block_sum_i(int v, int* red) {
  v = wave_sum_i(v);
  __syncthreads();
  if (lane_id() == 0) red[wave_id()] = v;
  __syncthreads();
  const int nw = blockDim.x >> 6;
  int t = 0;
  for (int w = 0; w < nw; ++w) t += red[w];
  return t;
}

// ---- in-place inclusive prefix sum of an LDS array a[0..n) by the whole workgroup. ----
// Each thread scans a contiguous chunk serially, the per-thread totals are scanned with wave shuffles and
// a fixed-order combine across waves.  `red` holds LTRX_MAX_WAVES floats.  Contains the needed barriers;
// a[] must be fully written (and barrier'd) by the caller before the call; it is valid for all threads after.
__device__ __forceinline__ void block_inclusive_scan(float* a, int n, float* red) {
  const int T = blockDim.x;
  const int chunk = (n + T - 1) / T;
  const int lo = threadIdx.x * chunk;
  const int hi = min(lo + chunk, n);
  float tot = 0.f;
  for (int i = lo; i < hi; ++i) {
    tot += a[i];
    a[i] = tot;
  }
  // inclusive scan of `tot` across the wave
  float inc = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    float up = __shfl_up(inc, o, 64);
    if (lane_id() >= o) inc += up;
  }
  __syncthreads();
  if (lane_id() == 63) red[wave_id()] = inc;
  __syncthreads();
  // exclusive prefix inside the wave: the lane below's inclusive one.  (Not `inc - tot`: that difference is rounded at the size of inc,
  // which reaches to the END of this thread's chunk -- with chunk >= 2 an entry far smaller than its chunk's end lost all precision.)
  float base = __shfl_up(inc, 1, 64);
  if (lane_id() == 0) base = 0.f;
  for (int w = 0; w < wave_id(); ++w) base += red[w];
  for (int i = lo; i < hi; ++i) a[i] += base;
  __syncthreads();
}

__device__ __forceinline__ float sigmoidf_acc(float x) { return 1.0f / (1.0f + expf(-x)); }

// the murmur3 32-bit finaliser: every counter-based draw of the library ends in it (counter_hash below, the attention dropout's row
// seed in ltrx_mfma.h, the FixLength sampling keys in ltrx_data.hip)
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// The split-bf16 split of one float: x ~= hi + lo (+ lo2), hi = bf16(x), lo = bf16(x - hi), lo2 = bf16((x - hi) - lo): each further
// term is what the previous one leaves of the rest.  Every operand image and every on-the-fly staging of the library is written with
// these macros, so an image written anywhere is bit-identical to the split a GEMM applies while staging.  `hi` and `lo` are __bf16
// lvalues: vector elements, or locals that the site stores afterwards.
// (Macros, not a function: the terms of an inlined by-value function reach the optimiser in one fixed order relative to the vector
//  inserts around them, the sites have two such orders, and kernels of ltrx_gemm.hip, ltrx_mha_res.hip and ltrx_fcstep.hip schedule
//  differently when theirs changes; see profiles/NOTES.md.)
#define LTRX_BF16_REST(rest, prev) ((__bf16)((rest) - (float)(prev)))
#define LTRX_SPLIT_BF16(x, hi, lo) ((hi) = (__bf16)(x), (lo) = LTRX_BF16_REST(x, hi))

// Counter-based dropout: the keep decision of element `idx` of a tensor is a pure function of (seed, idx), so forward and
// backward kernels regenerate the same mask without storing it (murmur3 finaliser over the folded 64-bit index).
// `seed` = per-site constant XOR a per-step word read from device memory (so a captured hipGraph draws a fresh mask at
// every replay).  Returns 1/(1-p) for kept elements, 0 for dropped ones.
struct DropSpec {
  uint32_t seed;
  uint32_t thresh;     // drop iff (hash >> 8) < thresh,  thresh = p * 2^24  (0 = dropout off)
  float inv_keep;
};
// the generator itself: 32 hashed bits of element `idx` under `seed` (its top 24 bits are what the sites consume: the dropout
// decision below, the uniform draw of the stochastic NeuralSort noise in ltrx_neuralsort_stoch.hip)
__device__ __forceinline__ uint32_t counter_hash(uint32_t seed, uint64_t idx) {
  return fmix32((uint32_t)idx ^ ((uint32_t)(idx >> 32) * 0x9E3779B9u) ^ seed);
}
__device__ __forceinline__ float drop_keep_scale(const DropSpec& d, uint64_t idx) {
  return ((counter_hash(d.seed, idx) >> 8) >= d.thresh) ? d.inv_keep : 0.f;
}

}  // namespace ltrx
inline ltrx::DropSpec ltrx_make_drop(float p, uint32_t seed) {
  ltrx::DropSpec d;
  d.seed = seed;
  d.thresh = (p > 0.f) ? (uint32_t)(p * 16777216.0f) : 0u;
  d.inv_keep = (p > 0.f) ? 1.0f / (1.0f - p) : 1.0f;
  return d;
}

// 4 floats -> the 16 bytes {hi0..hi3, lo0..lo3} (bf16) of a pre-split operand image, by the same macro (LTRX_SPLIT_BF16) the GEMM
// kernels apply while staging, so an image written anywhere is bit-identical to the on-the-fly split
typedef __bf16 ltrx_bf16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ltrx_split_image4(const float4 v) {
  const float x[4] = {v.x, v.y, v.z, v.w};
  ltrx_bf16x4_t hi, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    LTRX_SPLIT_BF16(x[e], hi[e], lo[e]);
  }
  float4 o;
  *reinterpret_cast<ltrx_bf16x4_t*>(&o.x) = hi;
  *reinterpret_cast<ltrx_bf16x4_t*>(&o.z) = lo;
  return o;
}

// Per-slate work arrays of the listwise loss kernels (`narr` floats per item): in LDS (extern __shared__) while they fit the CU's
// 160 KB, otherwise in a global workspace that the SAME kernel body addresses through a generic pointer (template flag GWS): the
// arrays of a slate stay in its CU's L1 / the XCD's L2, and __syncthreads() orders global accesses inside a workgroup exactly as it
// orders LDS.  Slates up to LTRX_MAX_SLATE_LEN take the LDS form (the tuned path); up to LTRX_MAX_LONG_SLATE_LEN the global form --
// the reference pads a validation set to its longest slate with no bound (allrank/data/dataset_loading.py:185-194).
// One description per loss states its working set -- `narr` arrays of L floats plus `extra_floats`, and the per-slate results
// (`per_floats(B)`, a multiple of 4) that lead the call's workspace -- and everything else derives from it: the exported
// *_workspace_bytes, the LDS byte count, where the work arrays start in the workspace and their per-slate stride.  The description sits
// directly above its kernel, whose carve spells the same counts out.
#define LTRX_LDS_ARRAY_BUDGET_BYTES (160 * 1024 - 1024)
struct LtrxSlateArrays {
  int narr, extra_floats;
  size_t (*per_floats)(int B);
  std::atomic<uint64_t> lds_allowed{0};        // ltrx_allow_dynamic_lds of the LDS-form kernel, per device

  size_t floats(int L) const { return (size_t)narr * (size_t)L + (size_t)extra_floats; }
  size_t lds_bytes(int L) const { return floats(L) * sizeof(float); }
  bool in_lds(int L) const { return lds_bytes(L) <= (size_t)LTRX_LDS_ARRAY_BUDGET_BYTES; }
  size_t ws_stride(int L) const { return (floats(L) + 3) & ~(size_t)3; }      // a slate's block keeps 16-byte alignment
  size_t workspace_bytes(int B, int L) const {                                 // non-positive B, L count as 0
    B = B > 0 ? B : 0;
    L = L > 0 ? L : 0;
    return (per_floats(B) + (in_lds(L) ? 0 : ws_stride(L) * (size_t)B)) * sizeof(float);
  }
};
// per-slate results of a loss that keeps one float per slate
static inline size_t ltrx_per_slate_floats(int B) { return ((size_t)B + 3) & ~(size_t)3; }

// Launches one workgroup per slate: `lds_kernel` (GWS = false) with the arrays as dynamic LDS, or `ws_kernel` (GWS = true) with the
// arrays in the workspace `ws` behind the per-slate results.  `args` are the kernel's parameters up to its last two, (gws, gws_stride).
template <typename K, typename... Args>
static inline int ltrx_launch_slate_arrays(LtrxSlateArrays& d, K* lds_kernel, K* ws_kernel, int B, int L, dim3 block, float* ws,
                                           hipStream_t s, Args... args) {
  if (d.in_lds(L)) {
    const size_t lds = d.lds_bytes(L);
    if (lds > LTRX_DEFAULT_DYNAMIC_LDS_BYTES) {
      const int rc = ltrx_allow_dynamic_lds(d.lds_allowed, {{lds_kernel, LTRX_LDS_ARRAY_BUDGET_BYTES}});
      if (rc != LTRX_OK) return rc;
    }
    hipLaunchKernelGGL(lds_kernel, dim3(B), block, lds, s, args..., (float*)nullptr, (size_t)0);
  } else {
    hipLaunchKernelGGL(ws_kernel, dim3(B), block, 0, s, args..., ws + d.per_floats(B), d.ws_stride(L));
  }
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// The two layouts of a listwise loss / metric call (ltrx.h, "Ragged layout"), resolved once per workgroup -- the counterpart of
// which_slate() in ltrx_mha_res.hip.  One kernel body serves both through the template flag RAGGED:
//   padded: slate b = blockIdx.x owns rows b*L .. b*L+L-1, `len` = L, and a slot is padding where its label equals `pad`;
//   ragged: slate b = slate_order[blockIdx.x] (or blockIdx.x) owns rows cu[b] .. cu[b+1]-1, every one of them valid; L is max_len, which
//           only sizes the carve of the work arrays.  A slate longer than max_len is cut to its first max_len items, a negative
//           extent counts as empty and an order entry outside [0, B) is clamped: whatever the tables hold, a workgroup stays inside
//           its carve and the rows its cu entries name.
// The padded instantiation sees len == L and ltrx_is_pad's label compare, i.e. the loop bounds and tests it had before the flag.
struct LtrxSlate {
  int b, len;
  size_t row0;
};
template <bool RAGGED>
__device__ __forceinline__ LtrxSlate ltrx_slate(int L, const int32_t* __restrict__ cu, const int32_t* __restrict__ order) {
  LtrxSlate s;
  if (RAGGED) {
    const int b = order ? order[blockIdx.x] : (int)blockIdx.x;
    s.b = min(max(b, 0), (int)gridDim.x - 1);
    const int lo = cu[s.b];
    s.row0 = (size_t)lo;
    s.len = min(max(cu[s.b + 1] - lo, 0), L);
  } else {
    s.b = blockIdx.x;
    s.row0 = (size_t)blockIdx.x * L;
    s.len = L;
  }
  return s;
}
template <bool RAGGED>
__device__ __forceinline__ bool ltrx_is_pad(float y, float pad) {
  return !RAGGED && y == pad;
}

// The library's sort (ltrx.h, "sort tie policy"): stable descending by counting.  Item j stands before item i when its key is
// larger, or equal with the lower index -- float compares, so -0.0 and +0.0 tie, +-inf order as floats, and a NaN key stands before
// nothing and has nothing before it (rank 0, shared with the true maximum: the order of a slate that holds NaNs is unspecified).
// ltrx_count_ranks: the ranks of item i under K keys at once (ltrx_ndcg.hip: prediction and label; ltrx_rank.hip: the score), one walk
// over the slate's n items in LDS; `skip(j)` leaves item j out of the count (the padded slots of the padded layout).
__device__ __forceinline__ bool ltrx_sorts_before(float vj, int j, float vi, int i) { return (vj > vi) || (vj == vi && j < i); }
template <int K, typename Skip>
__device__ __forceinline__ void ltrx_count_ranks(const float* const (&key)[K], int n, int i, int (&rank)[K], Skip skip) {
  float vi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    vi[k] = key[k][i];
    rank[k] = 0;
  }
  for (int j = 0; j < n; ++j) {
    if (skip(j)) continue;
#pragma unroll
    for (int k = 0; k < K; ++k) rank[k] += ltrx_sorts_before(key[k][j], j, vi[k], i);
  }
}

// Final cross-slate reduction: out[0] = scale * sum_b per[b]  (fixed order -> deterministic).  One block.
// (host launcher lives in ltrx_common.hip; kernels are never launched across translation units)
int ltrx_launch_finalize_sum(const float* per, int B, float scale, float* out, hipStream_t s);
// x[0] = (denom[0] != 0) ? x[0] / denom[0] : 0   (one thread; used for batch-global normalisers kept on the device)
int ltrx_launch_div_by_device_scalar(float* x, const float* denom, hipStream_t s);
