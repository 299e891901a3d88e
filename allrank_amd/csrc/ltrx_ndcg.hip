// NDCG@k / DCG@k metric + stable argsort indices.  Reference: allrank/models/metrics.py:7-77.
//
//   padded preds -> -inf, padded labels -> 0 (metrics.py:32-35); sort preds descending (:37); gather labels;
//   gain 2^y - 1 (:67) * 1/log2(pos+2) (:64-65); cumulative sum (:71) picked at ats-1 (:73-75);
//   ndcg = dcg / idcg with idcg = dcg(y_true, y_true), idcg == 0 -> filler_value (:21-24).
//
// One workgroup per slate.  Sorting = counting rank out of LDS (stable descending, padded last in index order);
// discounted gains are scattered to their sorted position in LDS and summed with a workgroup prefix scan, so
// a single pass serves every cut-off in `ats`.  The int64 order tensor (bit-exact under the tie policy of
// SURVEY.md §9.2) is optional.  HBM: 8 B/item in, 4*n_ats B/slate out (+8 B/item with order_out).
#include "ltrx_device.h"

using namespace ltrx;


// RAGGED: the cu_seqlens layout (ltrx_device.h: ltrx_slate) -- L is then max_len and sizes the carve only; the rank loops and the scans
// run to the slate's own length n, the pad tests fold away, order_out holds indices inside the slate, and an empty slate gives
// (filler, 0) like an all-padded one.  `gains` is a padded-layout argument.
template <bool RAGGED>
__global__ void __launch_bounds__(1024) ltrx_ndcg_kernel(const float* __restrict__ y_pred,
                                                        const float* __restrict__ y_true, int L, float pad,
                                                        float filler, LtrxAts ats, float* __restrict__ ndcg_out,
                                                        float* __restrict__ dcg_out, int64_t* __restrict__ order_out,
                                                        const float* __restrict__ gains, const int32_t* __restrict__ cu,
                                                        const int32_t* __restrict__ order) {
  extern __shared__ float lds[];
  float* ss = lds;           // [L]
  float* ys = lds + L;       // [L]
  float* dg = lds + 2 * L;   // [L] discounted gains in predicted order -> prefix sums
  float* ig = lds + 3 * L;   // [L] discounted gains in ideal order -> prefix sums
  __shared__ float red[LTRX_MAX_WAVES];
  __shared__ int redi[LTRX_MAX_WAVES];
  const LtrxSlate sl = ltrx_slate<RAGGED>(L, cu, order);
  const int b = sl.b;
  const int n = RAGGED ? sl.len : L;     // items of this slate that the loops visit
  const float* sp = y_pred + sl.row0;
  const float* yp = y_true + sl.row0;
  // caller-supplied gains (metrics.py:67 with gain_function != 2^x - 1): gain_function evaluated per item on the masked labels
  // (padded -> label 0, metrics.py:35), so a padded item carries gain_function(0) at its tail position in BOTH rankings
  const float* gp = gains ? gains + sl.row0 : nullptr;
  int nv = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    ss[i] = sp[i];
    const float y = yp[i];
    ys[i] = y;
    dg[i] = 0.f;
    ig[i] = 0.f;
    nv += !ltrx_is_pad<RAGGED>(y, pad);
  }
  nv = block_sum_i(nv, redi);
  int64_t* op = order_out ? order_out + sl.row0 : nullptr;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float yi = ys[i];
    if (ltrx_is_pad<RAGGED>(yi, pad)) {
      if (op || gp) {
        int before = 0;
        for (int j = 0; j < i; ++j) before += ltrx_is_pad<RAGGED>(ys[j], pad);
        if (op) op[nv + before] = i;
        if (gp) dg[nv + before] = ig[nv + before] = gp[i] / log2f((float)(nv + before) + 2.0f);
      }
      continue;
    }
    const float* const keys[2] = {ss, ys};     // predicted order, ideal order
    int rk[2];
    ltrx_count_ranks(keys, n, i, rk, [&](int j) { return ltrx_is_pad<RAGGED>(ys[j], pad); });
    const int rs = rk[0], ry = rk[1];
    const float gain = gp ? gp[i] : exp2f(yi) - 1.0f;
    dg[rs] = gain / log2f((float)rs + 2.0f);
    ig[ry] = gain / log2f((float)ry + 2.0f);
    if (op) op[rs] = i;
  }
  __syncthreads();
  block_inclusive_scan(dg, n, red);
  block_inclusive_scan(ig, n, red);
  if (threadIdx.x < ats.n) {
    int at = ats.at[threadIdx.x];
    at = at > n ? n : at;
    const bool empty = RAGGED && at <= 0;       // a slate without items: DCG 0 at every cut-off
    const float d = empty ? 0.f : dg[at - 1], id = empty ? 0.f : ig[at - 1];
    ndcg_out[(size_t)b * ats.n + threadIdx.x] = (id == 0.f) ? filler : d / id;
    if (dcg_out) dcg_out[(size_t)b * ats.n + threadIdx.x] = d;
  }
}

extern "C" size_t ltrx_ndcg_workspace_bytes(int B, int L) { (void)B; (void)L; return 0; }

// one host path for both layouts: cu == NULL is the padded call, L the ragged call's max_len
static int ndcg_launch(const float* y_pred, const float* y_true, const float* gains, const int32_t* cu, const int32_t* order, int B, int L,
                       const int* ats, int n_ats, float pad_value, float filler_value, float* ndcg_out, float* dcg_out,
                       int64_t* order_out, void* ws, ltrx_stream_t stream) {
  (void)ws;
  if (!y_pred || !y_true || !ats || !ndcg_out || B <= 0 || L <= 0 || n_ats <= 0) return LTRX_EINVAL;
  if (n_ats > LTRX_MAX_ATS || L > LTRX_MAX_METRIC_SLATE_LEN) return LTRX_EUNSUPPORTED;
  if (4 * (size_t)L * sizeof(float) > LTRX_DEFAULT_DYNAMIC_LDS_BYTES) {
    static std::atomic<uint64_t> attr_done{0};
    const int arc = ltrx_allow_dynamic_lds(attr_done, {{ltrx_ndcg_kernel<false>, 4 * LTRX_MAX_METRIC_SLATE_LEN * sizeof(float)},
                                                       {ltrx_ndcg_kernel<true>, 4 * LTRX_MAX_METRIC_SLATE_LEN * sizeof(float)}});
    if (arc != LTRX_OK) return arc;
  }
  LtrxAts a;
  a.n = n_ats;
  for (int i = 0; i < n_ats; ++i) {
    if (ats[i] <= 0) return LTRX_EINVAL;
    a.at[i] = ats[i];
  }
  // long slates: 16 waves.  A thread owns items i, i + T, ... and walks all of the slate's partners, so the launch takes as long as
  // the thread with the most items of the longest slate.  The padded call keeps its rule (1024 threads above L = 512).  The ragged call
  // decides by max_len, the longest slate of ITS batch, and goes to 1024 threads as soon as 256 would give a thread a second item.
  // Measured (profiles/ragged_eval.md, batches of 64 and 256 WEB30K-like slates, mean length 120): longest slate 420 - 444: 1024
  // threads 24 - 25 us against 37 - 39 us with 256; longest slate 200: 256 threads 12.2 us against 12.9 us with 1024 (the barriers
  // and scan steps span 16 waves for nothing).
  const dim3 block(L > (cu ? 256 : 512) ? 1024 : 256);
  if (cu)
    hipLaunchKernelGGL(ltrx_ndcg_kernel<true>, dim3(B), block, 4 * (size_t)L * sizeof(float), (hipStream_t)stream, y_pred, y_true, L,
                       pad_value, filler_value, a, ndcg_out, dcg_out, order_out, gains, cu, order);
  else
    hipLaunchKernelGGL(ltrx_ndcg_kernel<false>, dim3(B), block, 4 * (size_t)L * sizeof(float), (hipStream_t)stream, y_pred, y_true, L,
                       pad_value, filler_value, a, ndcg_out, dcg_out, order_out, gains, cu, order);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

extern "C" int ltrx_ndcg_at(const float* y_pred, const float* y_true, int B, int L, const int* ats, int n_ats,
                            float pad_value, float filler_value, float* ndcg_out, float* dcg_out, int64_t* order_out,
                            void* ws, ltrx_stream_t stream) {
  return ndcg_launch(y_pred, y_true, nullptr, nullptr, nullptr, B, L, ats, n_ats, pad_value, filler_value, ndcg_out, dcg_out, order_out, ws, stream);
}

extern "C" int ltrx_ndcg_at_gains(const float* y_pred, const float* y_true, const float* gains, int B, int L, const int* ats,
                                  int n_ats, float pad_value, float filler_value, float* ndcg_out, float* dcg_out,
                                  int64_t* order_out, void* ws, ltrx_stream_t stream) {
  if (!gains) return LTRX_EINVAL;
  return ndcg_launch(y_pred, y_true, gains, nullptr, nullptr, B, L, ats, n_ats, pad_value, filler_value, ndcg_out, dcg_out, order_out, ws, stream);
}

extern "C" int ltrx_ndcg_at_cu(const float* y_pred, const float* y_true, const int32_t* cu_seqlens, const int32_t* slate_order, int B,
                               int max_len, const int* ats, int n_ats, float filler_value, float* ndcg_out, float* dcg_out,
                               int64_t* order_out, void* ws, ltrx_stream_t stream) {
  if (!cu_seqlens) return LTRX_EINVAL;
  return ndcg_launch(y_pred, y_true, nullptr, cu_seqlens, slate_order, B, max_len, ats, n_ats, 0.f, filler_value, ndcg_out, dcg_out,
                     order_out, ws, stream);
}
