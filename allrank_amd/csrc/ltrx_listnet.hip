// Fused ListNet forward + backward.  Reference: allrank/models/losses/listNet.py:8-30.
//
//   mask = y_true == pad; P = softmax(y_pred | mask -> -inf); T = softmax(y_true | mask -> -inf)
//   loss = mean_b( -sum_i T_i * log(P_i + eps) )
//   d loss / d s_k = (1/B) [ P_k * sum_i T_i P_i/(P_i+eps)  -  T_k P_k/(P_k+eps) ]        
//
// One workgroup (256 threads = 4 waves) per slate; scores/labels are read once from HBM (coalesced,
// lane-strided), kept in registers/LDS, all reductions are wave shuffles + a 4-entry LDS combine.
// Algorithmic HBM traffic: 8 B/item read + 4 B/item written; compute is negligible -> launch/latency bound.
#include "ltrx_device.h"

using namespace ltrx;

// the two work arrays of the kernel below (ltrx_device.h: LtrxSlateArrays).  Their workspace form cannot be reached today: at
// LTRX_MAX_LONG_SLATE_LEN = 16384 they are 2 * 16384 * 4 B = 128 KB, inside the LDS budget; the rule is kept uniform all the same.
static LtrxSlateArrays listnet_arrays{2, 0, ltrx_per_slate_floats};
// GWS: the two work arrays live in a global workspace (slates too long for LDS; ltrx_device.h)
// RAGGED: the cu_seqlens layout (ltrx_device.h: ltrx_slate) -- L is then max_len (the carve), the loops run to the slate's length n
template <bool GWS, bool RAGGED>
__global__ void __launch_bounds__(256) ltrx_listnet_kernel(const float* __restrict__ y_pred,
                                                           const float* __restrict__ y_true, int L, float eps,
                                                           float pad, float inv_div, float* __restrict__ per_ws,
                                                           float* __restrict__ per_out, float* __restrict__ grad,
                                                           const int32_t* __restrict__ cu, const int32_t* __restrict__ order,
                                                           float* gws, size_t gws_stride) {
  extern __shared__ float lds[];
  float* base = GWS ? gws + (size_t)blockIdx.x * gws_stride : lds;
  float* ps = base;      // [L] exp(s - max)  -> P
  float* ts = base + L;  // [L] exp(y - max)  -> T
  __shared__ float red[LTRX_MAX_WAVES];
  const LtrxSlate sl = ltrx_slate<RAGGED>(L, cu, order);
  const int b = sl.b;
  const int n = RAGGED ? sl.len : L;
  const float* sp = y_pred + sl.row0;
  const float* yp = y_true + sl.row0;

  float smax = -INFINITY, ymax = -INFINITY;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float y = yp[i];
    bool valid = !ltrx_is_pad<RAGGED>(y, pad);
    float s = valid ? sp[i] : -INFINITY;
    float t = valid ? y : -INFINITY;
    ps[i] = s;
    ts[i] = t;
    smax = fmaxf(smax, s);
    ymax = fmaxf(ymax, t);
  }
  smax = block_max(smax, red);
  ymax = block_max(ymax, red);
  float ssum = 0.f, ysum = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float e = (ps[i] == -INFINITY) ? 0.f : expf(ps[i] - smax);
    float f = (ts[i] == -INFINITY) ? 0.f : expf(ts[i] - ymax);
    ps[i] = e;
    ts[i] = f;
    ssum += e;
    ysum += f;
  }
  ssum = block_sum(ssum, red);
  ysum = block_sum(ysum, red);
  // a fully padded slate has ssum == 0: the reference yields NaN there; we define its contribution as 0.
  const float inv_s = ssum > 0.f ? 1.0f / ssum : 0.f;
  const float inv_y = ysum > 0.f ? 1.0f / ysum : 0.f;
  float lsum = 0.f, rsum = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float P = ps[i] * inv_s, T = ts[i] * inv_y;
    ps[i] = P;
    ts[i] = T;
    if (T > 0.f) lsum += T * logf(P + eps);
    rsum += T * (P / (P + eps));   // P == 0 -> 0 (eps > 0); eps == 0 and P == 0 only when T == 0 as well
  }
  lsum = block_sum(lsum, red);
  rsum = block_sum(rsum, red);
  if (threadIdx.x == 0) {
    per_ws[b] = -lsum;
    if (per_out) per_out[b] = -lsum;
  }
  if (grad) {
    float* gp = grad + sl.row0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      float P = ps[i], T = ts[i];
      float r = (P > 0.f) ? P / (P + eps) : 0.f;
      gp[i] = (P * rsum - T * r) * inv_div;   // padded: P = T = 0 -> exactly 0
    }
  }
}

extern "C" size_t ltrx_listnet_workspace_bytes(int B, int L) { return listnet_arrays.workspace_bytes(B, L); }

// one host path for both layouts: cu == NULL is the padded call
static int listnet_launch(const float* y_pred, const float* y_true, const int32_t* cu, const int32_t* order, int B, int L, float eps,
                          float pad_value, float batch_divisor, float* loss_out, float* per_slate_out, float* grad_out, void* ws,
                          ltrx_stream_t stream) {
  if (!y_pred || !y_true || !loss_out || !ws || B <= 0 || L <= 0 || !(batch_divisor > 0.f)) return LTRX_EINVAL;
  if (L > LTRX_MAX_LONG_SLATE_LEN) return LTRX_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  float* per = (float*)ws;
  const int rc = cu ? ltrx_launch_slate_arrays(listnet_arrays, ltrx_listnet_kernel<false, true>, ltrx_listnet_kernel<true, true>, B, L,
                                               dim3(256), per, s, y_pred, y_true, L, eps, pad_value, 1.0f / batch_divisor, per,
                                               per_slate_out, grad_out, cu, order)
                    : ltrx_launch_slate_arrays(listnet_arrays, ltrx_listnet_kernel<false, false>, ltrx_listnet_kernel<true, false>, B, L,
                                               dim3(256), per, s, y_pred, y_true, L, eps, pad_value, 1.0f / batch_divisor, per,
                                               per_slate_out, grad_out, cu, order);
  if (rc != LTRX_OK) return rc;
  return ltrx_launch_finalize_sum(per, B, 1.0f / batch_divisor, loss_out, s);
}

extern "C" int ltrx_listnet_fwd_bwd(const float* y_pred, const float* y_true, int B, int L, float eps, float pad_value,
                                    float batch_divisor, float* loss_out, float* per_slate_out, float* grad_out,
                                    void* ws, ltrx_stream_t stream) {
  return listnet_launch(y_pred, y_true, nullptr, nullptr, B, L, eps, pad_value, batch_divisor, loss_out, per_slate_out, grad_out, ws, stream);
}

extern "C" int ltrx_listnet_fwd_bwd_cu(const float* y_pred, const float* y_true, const int32_t* cu_seqlens, const int32_t* slate_order,
                                       int B, int max_len, float eps, float batch_divisor, float* loss_out, float* per_slate_out,
                                       float* grad_out, void* ws, ltrx_stream_t stream) {
  if (!cu_seqlens) return LTRX_EINVAL;
  return listnet_launch(y_pred, y_true, cu_seqlens, slate_order, B, max_len, eps, 0.f, batch_divisor, loss_out, per_slate_out, grad_out, ws,
                        stream);
}
