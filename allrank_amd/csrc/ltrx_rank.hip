// Ranked slates: packed scores -> every slate's items (features and labels) in descending score order, padded to L.
// Reference: allrank/inference/inference_utils.py:51-56 -- padded scores to -inf, scores.sort(descending=True), torch.gather of X and y.
//
// ORDER.  rank of item i = #{ j : s_j > s_i, or s_j == s_i and j < i }: the stable descending policy of ltrx_ndcg_at_cu, counted by the
// same loop (ltrx_device.h: ltrx_count_ranks).  -0.0 == +0.0 is a tie, +-inf order as floats.  The reference's torch.sort(descending=
// True) is NOT stable: on exact ties its order is undefined, and this kernel defines it (lower index first).  A slate that holds NaN
// scores has an unspecified order: several items may claim one rank and some ranks stay without an item; every output element is still
// written (a rank without an item gets the tail values), and no access leaves the slate's rows or its carve.
//
// One workgroup per slate, launched in slate_order and resolved by ltrx_slate<true> (its clamping rules hold here).
//   phase 1  scores -> LDS, rank by counting, inverse permutation (rank -> item) in LDS: 2 x 4 B per item, 64 KB at
//            LTRX_MAX_METRIC_SLATE_LEN.
//   phase 2  waves stride over the ranked rows, lanes over the columns of a row (a row narrower than the wave: 64 / columns rows per
//            wave instruction); 16-byte accesses where F % 4 == 0 and both bases are 16-byte aligned (every row then is), else dwords.
//   tail     rows len .. L-1 of the slate are one contiguous range: 0.0f features, -1.0f labels.
// Time: the launch lasts as long as its longest slate's counting pass, n^2 compares on one CU (1,251 items: about 0.1 ms, whatever the
// tail's bytes: profiles/rank_slates.md).
// The source rows come from the padded grid the scorer was given (x[B, L, F], valid items first) or straight from the resident CSR set
// (row (offsets[ids[b]] + i) * F of x_items): the padded features are never materialised on the input side.
// HBM per slate: n F floats read, L F floats written (+ 4 B per item of scores, 4 B per slot of labels); at 10 % valid the tail is
// most of the bytes.  Outputs must not overlap the inputs.
#include "ltrx_device.h"

using namespace ltrx;

// T: the unit a lane moves, float4 (C = F / 4 units per row) or float (C = F)
template <typename T, bool RESIDENT>
__global__ void __launch_bounds__(1024) ltrx_rank_kernel(const float* __restrict__ scores, const float* __restrict__ xs,
                                                        const float* __restrict__ ys, const int64_t* __restrict__ offsets,
                                                        const int64_t* __restrict__ ids, const int32_t* __restrict__ cu,
                                                        const int32_t* __restrict__ order, int max_len, int C, int L,
                                                        int32_t* __restrict__ perm, float* __restrict__ x_out, float* __restrict__ y_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ss = lds;                                          // [max_len] scores
  int* inv = reinterpret_cast<int*>(lds + max_len);         // [max_len] rank -> item, -1 = no item landed (NaN scores only)
  const LtrxSlate sl = ltrx_slate<true>(max_len, cu, order);
  int n = sl.len;
  size_t src0;                                              // the slate's first source row
  if (RESIDENT) {
    const int64_t id = ids[sl.b], lo = offsets[id];
    const int64_t ext = offsets[id + 1] - lo;               // never more rows than the set holds for this slate
    n = ext < (int64_t)n ? (int)(ext < 0 ? 0 : ext) : n;
    src0 = (size_t)lo;
  } else {
    src0 = (size_t)sl.b * L;
  }
  T zero;
  __builtin_memset(&zero, 0, sizeof(T));
  T* xo = reinterpret_cast<T*>(x_out) + (size_t)sl.b * L * C;
  const float* sp = scores + sl.row0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    ss[i] = sp[i];
    inv[i] = -1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float* const key[1] = {ss};
    int r[1];
    ltrx_count_ranks(key, n, i, r, [](int) { return false; });
    inv[r[0]] = i;
  }
  __syncthreads();
  if (perm)
    for (int r = threadIdx.x; r < n; r += blockDim.x) perm[sl.row0 + r] = inv[r];

  const T* xin = reinterpret_cast<const T*>(xs) + src0 * C;
  const float* yin = ys + src0;
  float* yo = y_out + (size_t)sl.b * L;
  // a wave instruction covers rpw rows of C units (C < 64), or 64 units of one row
  const int rpw = C >= 64 ? 1 : 64 / C;
  const int lr = C >= 64 ? 0 : lane_id() / C, lc = C >= 64 ? lane_id() : lane_id() % C;
  const int cstep = C >= 64 ? 64 : C;
  const int nw = blockDim.x >> 6;
  if (lr < rpw) {
    for (int r = wave_id() * rpw + lr; r < n; r += nw * rpw) {
      const int src = inv[r];
      const T* row = xin + (size_t)(src < 0 ? 0 : src) * C;
      T* dst = xo + (size_t)r * C;
      for (int c = lc; c < C; c += cstep) dst[c] = src < 0 ? zero : row[c];
      if (lc == 0) yo[r] = src < 0 ? -1.0f : yin[src];
    }
  }
  T* tail = xo + (size_t)n * C;
  const size_t cnt = (size_t)(L - n) * C;
  for (size_t e = threadIdx.x; e < cnt; e += blockDim.x) tail[e] = zero;
  for (int r = n + threadIdx.x; r < L; r += blockDim.x) yo[r] = -1.0f;
}

template <typename T, bool RESIDENT>
static int rank_launch(const float* scores, const float* xs, const float* ys, const int64_t* offsets, const int64_t* ids, const int32_t* cu,
                       const int32_t* order, int B, int max_len, int C, int L, int32_t* perm, float* x_out, float* y_out, hipStream_t s) {
  const size_t lds = 2 * (size_t)max_len * sizeof(float);
  if (lds > LTRX_DEFAULT_DYNAMIC_LDS_BYTES) {
    static std::atomic<uint64_t> attr_done{0};
    const int arc = ltrx_allow_dynamic_lds(attr_done, {{ltrx_rank_kernel<T, RESIDENT>, 2 * LTRX_MAX_METRIC_SLATE_LEN * sizeof(float)}});
    if (arc != LTRX_OK) return arc;
  }
  // the thread with the most items of the longest slate walks all of that slate's partners: 16 waves as soon as 4 would give a thread
  // a second item (the ragged rule of ltrx_ndcg_at_cu); the row moves of phase 2 and the tail only gain from more waves in flight
  const dim3 block(max_len > 256 ? 1024 : 256);
  hipLaunchKernelGGL((ltrx_rank_kernel<T, RESIDENT>), dim3(B), block, lds, s, scores, xs, ys, offsets, ids, cu, order, max_len, C, L, perm,
                     x_out, y_out);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

extern "C" int ltrx_rank_slates_cu(const float* scores, const float* x, const float* y, const float* x_items, const float* y_items,
                                   const int64_t* offsets, const int64_t* ids, const int32_t* cu_seqlens, const int32_t* slate_order,
                                   int B, int max_len, int F, int L, int32_t* perm, float* x_out, float* y_out, ltrx_stream_t stream) {
  const bool grid = x && y, resident = x_items && y_items && offsets && ids;
  const bool any_grid = x || y, any_resident = x_items || y_items || offsets || ids;
  if (!scores || !cu_seqlens || !x_out || !y_out || B <= 0 || F <= 0 || max_len <= 0 || L < max_len) return LTRX_EINVAL;
  if (grid == resident || (any_grid && !grid) || (any_resident && !resident)) return LTRX_EINVAL;     // exactly one complete source form
  if (max_len > LTRX_MAX_METRIC_SLATE_LEN) return LTRX_EUNSUPPORTED;
  const float* xs = grid ? x : x_items;
  const float* ys = grid ? y : y_items;
  const bool vec = F % 4 == 0 && (((uintptr_t)xs | (uintptr_t)x_out) & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    return grid ? rank_launch<float4, false>(scores, xs, ys, nullptr, nullptr, cu_seqlens, slate_order, B, max_len, F / 4, L, perm, x_out, y_out, s)
                : rank_launch<float4, true>(scores, xs, ys, offsets, ids, cu_seqlens, slate_order, B, max_len, F / 4, L, perm, x_out, y_out, s);
  return grid ? rank_launch<float, false>(scores, xs, ys, nullptr, nullptr, cu_seqlens, slate_order, B, max_len, F, L, perm, x_out, y_out, s)
              : rank_launch<float, true>(scores, xs, ys, offsets, ids, cu_seqlens, slate_order, B, max_len, F, L, perm, x_out, y_out, s);
}
