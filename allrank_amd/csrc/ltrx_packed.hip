// Packed batches whose valid-row count lives in DEVICE memory (the forward-only scorer of engine.FusedScorer).
//
// A captured hipGraph bakes in every host-side launch argument.  The pack / unpack kernels of compact training
// (ltrx_gather_rows / ltrx_scatter_rows, csrc/ltrx_train.hip) take the valid row count n as a host integer, so a graph
// captured for one batch would be wrong for the next.  The kernels below read every count from cu_seqlens (i32[B+1], device
// memory) and size their grids from a host row BUCKET (`rows`, a rung of the scorer's ladder) that only bounds the work:
//
//   ltrx_assemble_packed : packed rows straight from a resident CSR set (x_items, y_items, offsets, slate ids) -- the padding
//       branch of FixLength (dataset_loading.py:81-93) followed by packing, without the padded [B, L, F] feature tensor.
//       x_out[r, :F] = x_items[offsets[slate_b] + j] for packed row r = cu[b] + j < cu[B]; rows [cu[B], rows) are zeroed;
//       y_out[b, l] = label or -1; idx_out[r] = b * L + j (-1 beyond cu[B]); pos_out[r] = j (-1 beyond cu[B]).
//   ltrx_gather_rows_cu  : the same packing of a batch that arrives padded ([B', L, cols] words, valid items first in every slate).
//   ltrx_scatter_rows_cu : packed rows back to the padded grid, the padded slots set to 0.
//   ltrx_zero_rows_cu    : the alignment rows [cu[B], rows) of a row buffer set to 0 (the captured variable-length training step).
// Rows are moved as 32-bit words (bit-exact for any 4-byte type; an int64 column is two words), 16 bytes per access where the
// row length, strides and base addresses allow it.
#include "ltrx_device.h"

namespace {

constexpr int kMaxBlocks = 8192;

// slate of packed row r (0 <= r < cu[B]): the largest b with cu[b] <= r -- empty slates (cu[b] == cu[b+1]) are skipped
__device__ __forceinline__ int slate_of_row(const int32_t* __restrict__ cu, int B, int r) {
  int lo = 0, hi = B;                 // invariant: cu[lo] <= r < cu[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

inline int grid_for(size_t total) {
  const size_t g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : (g > (size_t)kMaxBlocks ? (size_t)kMaxBlocks : g));
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

template <bool VEC>
__global__ void __launch_bounds__(256) ltrx_assemble_packed_kernel(const float* __restrict__ x_items, const float* __restrict__ y_items,
                                                                   const int64_t* __restrict__ offsets, const int64_t* __restrict__ slates,
                                                                   const int32_t* __restrict__ cu, int B, int L, int F, int rows,
                                                                   float* __restrict__ x_out, int ld_x, float* __restrict__ y_out,
                                                                   int32_t* __restrict__ idx_out, int64_t* __restrict__ pos_out, int xblocks) {
  if ((int)blockIdx.x < xblocks) {                     // ---- packed feature rows (+ index and position of every row)
    const int per_row = VEC ? F / 4 : F;
    const int n = min(cu[B], rows);
    const size_t total = (size_t)rows * per_row;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)xblocks * blockDim.x) {
      const int r = (int)(e / per_row), c = (int)(e % per_row);
      int64_t item = -1;
      int b = 0, j = 0;
      if (r < n) {
        b = slate_of_row(cu, B, r);
        j = r - cu[b];
        const int64_t s = slates[b];
        const int64_t base = offsets[s];
        if (j < L && base + j < offsets[s + 1]) item = base + j;
      }
      if (VEC) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (item >= 0) v = reinterpret_cast<const float4*>(x_items + (size_t)item * F)[c];
        reinterpret_cast<float4*>(x_out + (size_t)r * ld_x)[c] = v;
      } else {
        x_out[(size_t)r * ld_x + c] = item >= 0 ? x_items[(size_t)item * F + c] : 0.f;
      }
      if (c == 0) {
        if (idx_out) idx_out[r] = item >= 0 ? b * L + j : -1;
        if (pos_out) pos_out[r] = item >= 0 ? (int64_t)j : (int64_t)-1;     // PADDED_INDEX_VALUE
      }
    }
    return;
  }
  // ---- the padded label grid y[B, L] (-1 = PADDED_Y_VALUE), one thread per slot
  const size_t e = (size_t)(blockIdx.x - xblocks) * blockDim.x + threadIdx.x;
  if (e >= (size_t)B * L) return;
  const int b = (int)(e / L), j = (int)(e % L);
  float y = -1.0f;
  if (j < cu[b + 1] - cu[b]) {
    const int64_t s = slates[b];
    const int64_t base = offsets[s];
    if (base + j < offsets[s + 1]) y = y_items[base + j];
  }
  y_out[e] = y;
}

extern "C" int ltrx_assemble_packed(const float* x_items, const float* y_items, const int64_t* offsets, const int64_t* slates,
                                    const int32_t* cu_seqlens, int B, int L, int F, int rows, float* x_out, int ld_x, float* y_out,
                                    int32_t* idx_out, int64_t* pos_out, ltrx_stream_t stream) {
  if (!x_items || !y_items || !offsets || !slates || !cu_seqlens || !x_out || !y_out) return LTRX_EINVAL;
  if (B <= 0 || L <= 0 || F <= 0 || rows < 0 || ld_x < F || (size_t)B * L > (size_t)INT32_MAX) return LTRX_EINVAL;
  const bool vec = (F % 4 == 0) && (ld_x % 4 == 0) && aligned16(x_items) && aligned16(x_out);
  const size_t xtotal = (size_t)rows * (vec ? F / 4 : F);
  const int xblocks = rows > 0 ? grid_for(xtotal) : 0;
  const size_t yblocks = ((size_t)B * L + 255) / 256;
  const dim3 grid((unsigned)(xblocks + yblocks));
  if (vec)
    hipLaunchKernelGGL(ltrx_assemble_packed_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x_items, y_items, offsets, slates,
                       cu_seqlens, B, L, F, rows, x_out, ld_x, y_out, idx_out, pos_out, xblocks);
  else
    hipLaunchKernelGGL(ltrx_assemble_packed_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x_items, y_items, offsets, slates,
                       cu_seqlens, B, L, F, rows, x_out, ld_x, y_out, idx_out, pos_out, xblocks);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

template <bool VEC>
__global__ void __launch_bounds__(256) ltrx_gather_rows_cu_kernel(const uint32_t* __restrict__ src, int ld_src,
                                                                  const int32_t* __restrict__ cu, int B, int L, int cols, int rows,
                                                                  uint32_t* __restrict__ dst, int ld_dst, int32_t* __restrict__ idx_out) {
  const int per_row = VEC ? cols / 4 : cols;
  const int n = min(cu[B], rows);
  const size_t total = (size_t)rows * per_row;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / per_row), c = (int)(e % per_row);
    int64_t row = -1;                                  // row of the padded batch, -1: alignment row
    if (r < n) {
      const int b = slate_of_row(cu, B, r);
      const int j = r - cu[b];
      if (j < L) row = (int64_t)b * L + j;
    }
    if (VEC) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (row >= 0) v = reinterpret_cast<const uint4*>(src + (size_t)row * ld_src)[c];
      reinterpret_cast<uint4*>(dst + (size_t)r * ld_dst)[c] = v;
    } else {
      dst[(size_t)r * ld_dst + c] = row >= 0 ? src[(size_t)row * ld_src + c] : 0u;
    }
    if (c == 0 && idx_out) idx_out[r] = (int32_t)row;
  }
}

extern "C" int ltrx_gather_rows_cu(const float* src, int ld_src, const int32_t* cu_seqlens, int B, int L, int cols, int rows, float* dst,
                                   int ld_dst, int32_t* idx_out, ltrx_stream_t stream) {
  if (!src || !cu_seqlens || !dst || B <= 0 || L <= 0 || cols <= 0 || rows < 0 || ld_src < cols || ld_dst < cols) return LTRX_EINVAL;
  if ((size_t)B * L > (size_t)INT32_MAX) return LTRX_EINVAL;
  if (rows == 0) return LTRX_OK;
  const bool vec = (cols % 4 == 0) && (ld_src % 4 == 0) && (ld_dst % 4 == 0) && aligned16(src) && aligned16(dst);
  const size_t total = (size_t)rows * (vec ? cols / 4 : cols);
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  if (vec)
    hipLaunchKernelGGL(ltrx_gather_rows_cu_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, s, ld_src, cu_seqlens,
                       B, L, cols, rows, d, ld_dst, idx_out);
  else
    hipLaunchKernelGGL(ltrx_gather_rows_cu_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, s, ld_src, cu_seqlens,
                       B, L, cols, rows, d, ld_dst, idx_out);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

__global__ void __launch_bounds__(256) ltrx_scatter_rows_cu_kernel(const uint32_t* __restrict__ src, int ld_src,
                                                                   const int32_t* __restrict__ cu, int B, int L, int cols, int rows,
                                                                   uint32_t* __restrict__ dst, int ld_dst) {
  const size_t total = (size_t)B * L * cols;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t slot = e / cols;                      // b * L + j
    const int c = (int)(e % cols);
    const int b = (int)(slot / L), j = (int)(slot % L);
    const int r = cu[b] + j;
    const bool valid = j < cu[b + 1] - cu[b] && r < rows;
    dst[slot * ld_dst + c] = valid ? src[(size_t)r * ld_src + c] : 0u;
  }
}

extern "C" int ltrx_scatter_rows_cu(const float* src, int ld_src, const int32_t* cu_seqlens, int B, int L, int cols, int rows, float* dst,
                                    int ld_dst, ltrx_stream_t stream) {
  if (!src || !cu_seqlens || !dst || B <= 0 || L <= 0 || cols <= 0 || rows < 0 || ld_src < cols || ld_dst < cols) return LTRX_EINVAL;
  if ((size_t)B * L > (size_t)INT32_MAX) return LTRX_EINVAL;
  hipLaunchKernelGGL(ltrx_scatter_rows_cu_kernel, dim3(grid_for((size_t)B * L * cols)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(src), ld_src, cu_seqlens, B, L, cols, rows, reinterpret_cast<uint32_t*>(dst), ld_dst);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// the alignment rows [cu[B], rows) of a row buffer, columns [0, cols): zero.  What a kernel that writes rows of slates only (the
// varlen attention forward and backward) leaves untouched there, inside a captured step: the count is read here, on the device,
// and the grid covers `rows` rows whatever it is.
template <bool VEC>
__global__ void __launch_bounds__(256) ltrx_zero_rows_cu_kernel(float* __restrict__ x, int ld, int cols, const int32_t* __restrict__ cu,
                                                                int B, int rows) {
  const int per_row = VEC ? cols / 4 : cols;
  const int first = min(max(cu[B], 0), rows);
  const size_t total = (size_t)(rows - first) * per_row;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int r = first + (int)(e / per_row), c = (int)(e % per_row);
    if (VEC)
      reinterpret_cast<float4*>(x + (size_t)r * ld)[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    else
      x[(size_t)r * ld + c] = 0.f;
  }
}

extern "C" int ltrx_zero_rows_cu(float* x, int ld, int cols, const int32_t* cu_seqlens, int B, int rows, ltrx_stream_t stream) {
  if (!x || !cu_seqlens || B <= 0 || rows <= 0 || cols <= 0 || ld < cols) return LTRX_EINVAL;
  const bool vec = (cols % 4 == 0) && (ld % 4 == 0) && aligned16(x);
  const size_t total = (size_t)rows * (vec ? cols / 4 : cols);
  if (vec)
    hipLaunchKernelGGL(ltrx_zero_rows_cu_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, ld, cols, cu_seqlens, B,
                       rows);
  else
    hipLaunchKernelGGL(ltrx_zero_rows_cu_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, ld, cols, cu_seqlens, B,
                       rows);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}
