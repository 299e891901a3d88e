// libsvm / SVMlight text written on the device: the inverse of ltrx_libsvm_parse (ltrx_data.hip).  The reference saves clicked slates
// with scikit-learn's dump_svmlight_file on the host (allrank/data/dataset_saving.py:32); these kernels write the same bytes.
// Contract: include/ltrx.h, "libsvm text written on the device".  The number format is ltrx_fmt_g16 (ltrx_fmt.h), exact.
//
//   line of row r:   <%.16g of y[r]> qid:<qid[r]>  then  " <f + index_base>:<%.16g of X[r][f]>"  for every f with X[r][f] != 0, rising,
//                    then "\n" -- or " \n" where the row holds no non-zero value (what the library the reference calls writes).
//
// SHAPE.  One wave per row, a workgroup IS one wave (64 threads), rows taken grid-stride.  Lane 0 formats the head; then the row's F
// values go by in rounds of 64, lane l formatting value f0 + l into its own 24-byte LDS slot.  An inclusive wave scan of the token
// lengths places every token; pass A (ltrx_libsvm_line_bytes) only adds the lengths up.  Pass B (ltrx_libsvm_format) copies each token
// from its slot to its place in the wave's staging buffer, and the 64 lanes then move the staged bytes to the text in aligned 4-byte
// words (the buffer starts at the destination's address modulo 4, so words of the buffer are words of the text; the ragged first and
// last bytes go one by one).  Each store is bounded by [0, n_bytes): a line_start that does not belong to these rows cannot make the
// kernel write outside the text.  Placement needs no atomics; the one atomic is the count of rows that hold a non-finite number.
// Both passes run the formatter: a token's length is known only once it is rounded (9.9999995e-5 has fewer digits than its neighbour).
#include "ltrx_device.h"
#include "ltrx_fmt.h"

#define LTRX_SVMW_THREADS 64
#define LTRX_SVMW_MAX_WORKGROUPS 16384           // 64 one-wave workgroups per CU; more rows are taken grid-stride
#define LTRX_SVMW_INDEX_DIGITS 10                // a feature index is a positive int
#define LTRX_SVMW_TOKEN_BYTES (1 + LTRX_SVMW_INDEX_DIGITS + 1 + 22)          // " index:value"
#define LTRX_SVMW_HEAD_BYTES (22 + 5 + 20)       // "label qid:" and an int64 with its sign
// a round's staging: up to 3 bytes of alignment, the head, 64 tokens, the line's end " \n"; a multiple of 16
#define LTRX_SVMW_STAGE_BYTES ((3 + LTRX_SVMW_HEAD_BYTES + LTRX_SVMW_THREADS * LTRX_SVMW_TOKEN_BYTES + 2 + 15) & ~15)

namespace {

__device__ __forceinline__ int svmw_digits(uint32_t v) {
  int d = 1;
  while (v >= 10u) {
    v /= 10u;
    ++d;
  }
  return d;
}

// the decimal digits of v (d of them) at p[0 .. d)
__device__ __forceinline__ void svmw_put_u64(uint8_t* p, uint64_t v, int d) {
  for (int i = d - 1; i >= 0; --i) {
    p[i] = (uint8_t)('0' + (uint32_t)(v % 10ull));
    v /= 10ull;
  }
}

// "<label> qid:<q>" at p; returns its length (<= LTRX_SVMW_HEAD_BYTES)
__device__ int svmw_head(uint8_t* p, float label, int64_t q) {
  int n = ltrx_fmt_g16(label, p);
  p[n] = ' ', p[n + 1] = 'q', p[n + 2] = 'i', p[n + 3] = 'd', p[n + 4] = ':';
  n += 5;
  uint64_t a = q < 0 ? 0ull - (uint64_t)q : (uint64_t)q;
  if (q < 0) p[n++] = '-';
  int d = 1;
  for (uint64_t t = a; t >= 10ull; t /= 10ull) ++d;
  svmw_put_u64(p + n, a, d);
  return n + d;
}

__device__ __forceinline__ bool svmw_nonfinite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) == 0x7F800000u; }

// WRITE = false: line_bytes[r] and the non-finite count.  WRITE = true: the text.
template <bool WRITE>
__global__ void __launch_bounds__(LTRX_SVMW_THREADS) svmwrite_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ y,
                                                                     const int64_t* __restrict__ qid, int64_t n_rows, int F, float pad,
                                                                     int index_base, int64_t* __restrict__ line_bytes,
                                                                     int* __restrict__ bad, const int64_t* __restrict__ line_start,
                                                                     int64_t n_bytes, uint8_t* __restrict__ text) {
  __shared__ __attribute__((aligned(16))) uint8_t slot[LTRX_SVMW_THREADS][LTRX_FMT_SLOT];
  __shared__ __attribute__((aligned(16))) uint8_t stage[LTRX_SVMW_STAGE_BYTES];
  const int lane = threadIdx.x;
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const float label = y[r];
    if (label == pad) {                                      // (a NaN pad keeps every row); the same for the whole wave
      if (!WRITE && lane == 0) line_bytes[r] = 0;
      continue;
    }
    const float* row = X + r * ldx;
    int64_t at = WRITE ? line_start[r] : 0;                  // where the staged bytes go / the bytes counted so far
    int base = WRITE ? (int)((uintptr_t)(text + at) & 3u) : 0;
    int staged = 0;
    if (lane == 0) staged = svmw_head(stage + base, label, qid[r]);
    staged = __shfl(staged, 0, 64);
    bool any = false, nonfinite = svmw_nonfinite(label);
    for (int f0 = 0; f0 < F; f0 += LTRX_SVMW_THREADS) {
      const int f = f0 + lane;
      const float v = f < F ? row[f] : 0.0f;
      int len = 0, vlen = 0, ilen = 0;
      if (v != 0.0f) {                                       // -0.0 is left out, a NaN is written (and counted)
        vlen = ltrx_fmt_g16(v, slot[lane]);
        ilen = svmw_digits((uint32_t)(f + index_base));
        len = 1 + ilen + 1 + vlen;
        nonfinite = nonfinite || svmw_nonfinite(v);
      }
      int inc = len;                                         // inclusive scan over the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
      }
      const int total = __shfl(inc, 63, 64);
      any = any || total > 0;
      const bool last = f0 + LTRX_SVMW_THREADS >= F;
      if (WRITE) {
        if (len > 0) {
          uint8_t* p = stage + base + staged + (inc - len);
          p[0] = ' ';
          svmw_put_u64(p + 1, (uint64_t)(uint32_t)(f + index_base), ilen);
          p[1 + ilen] = ':';
          for (int i = 0; i < vlen; ++i) p[2 + ilen + i] = slot[lane][i];
        }
        int end = staged + total;
        if (last && lane == 0) {
          if (!any) stage[base + end] = ' ';
          stage[base + end + (any ? 0 : 1)] = '\n';
        }
        if (last) end += any ? 1 : 2;
        __syncthreads();                                     // one wave: orders the LDS writes before the reads below
        // staged bytes [base, base + end) -> text[at, at + end); word w of the buffer is an aligned word of the text
        uint8_t* dst = text + at - base;
        for (int w = lane * 4; w < base + end; w += LTRX_SVMW_THREADS * 4) {
          const int64_t g = at - base + w;                   // text offset of the word's first byte
          if (w >= base && w + 4 <= base + end && g >= 0 && g + 4 <= n_bytes) {
            *reinterpret_cast<uint32_t*>(dst + w) = *reinterpret_cast<const uint32_t*>(stage + w);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (w + i >= base && w + i < base + end && g + i >= 0 && g + i < n_bytes) dst[w + i] = stage[w + i];
          }
        }
        __syncthreads();                                     // the buffer is free again
        at += end;
        base = (int)((uintptr_t)(text + at) & 3u);
        staged = 0;
      } else {
        staged += total;
      }
    }
    if (!WRITE && lane == 0) line_bytes[r] = (int64_t)staged + (any ? 1 : 2);
    nonfinite = __any(nonfinite);
    if (!WRITE && nonfinite && lane == 0) atomicAdd(bad, 1);
  }
}

bool svmw_bad_args(const float* X, int64_t ldx, const float* y, const int64_t* qid, int64_t n_rows, int F, int index_base) {
  return !X || !y || !qid || n_rows <= 0 || F <= 0 || ldx < F || index_base < 0 || (int64_t)F + index_base > 0x7fffffffll;
}

unsigned svmw_grid(int64_t n_rows) { return (unsigned)(n_rows < LTRX_SVMW_MAX_WORKGROUPS ? n_rows : LTRX_SVMW_MAX_WORKGROUPS); }

}  // namespace

extern "C" int ltrx_libsvm_line_bytes(const float* X, int64_t ldx, const float* y, const int64_t* qid, int64_t n_rows, int F,
                                      float pad_value, int index_base, int64_t* line_bytes, int* bad, ltrx_stream_t stream) {
  if (svmw_bad_args(X, ldx, y, qid, n_rows, F, index_base) || !line_bytes || !bad) return LTRX_EINVAL;
  hipLaunchKernelGGL(svmwrite_kernel<false>, dim3(svmw_grid(n_rows)), dim3(LTRX_SVMW_THREADS), 0, (hipStream_t)stream, X, ldx, y, qid, n_rows,
                     F, pad_value, index_base, line_bytes, bad, (const int64_t*)nullptr, (int64_t)0, (uint8_t*)nullptr);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

extern "C" int ltrx_libsvm_format(const float* X, int64_t ldx, const float* y, const int64_t* qid, int64_t n_rows, int F, float pad_value,
                                  int index_base, const int64_t* line_start, int64_t n_bytes, uint8_t* text, ltrx_stream_t stream) {
  if (svmw_bad_args(X, ldx, y, qid, n_rows, F, index_base) || !line_start || !text || n_bytes <= 0) return LTRX_EINVAL;
  hipLaunchKernelGGL(svmwrite_kernel<true>, dim3(svmw_grid(n_rows)), dim3(LTRX_SVMW_THREADS), 0, (hipStream_t)stream, X, ldx, y, qid, n_rows,
                     F, pad_value, index_base, (int64_t*)nullptr, (int*)nullptr, line_start, n_bytes, text);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

extern "C" int ltrx_debug_format_g16(const float* v, int64_t n, uint8_t* text, int32_t* len) {
  if (!v || !text || !len || n < 0) return LTRX_EINVAL;
  for (int64_t i = 0; i < n; ++i) len[i] = ltrx_fmt_g16(v[i], text + i * LTRX_FMT_SLOT);
  return LTRX_OK;
}
