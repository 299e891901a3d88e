// OutputLayer with d_output > 1 in eval mode, forward only: Linear(D, n_out), the output activation and model.score's sum over the
// output units in one launch (reference: allrank/models/model.py:111-117 and :127).
//   z_k = <x[r, :], W[k, :]> + bias[k],   p_k = act(z_k),   out[r, k] = p_k,   score[r] = p_0 + ... + p_{n_out-1}
// It replaces, for the forward-only scorer, a d -> n_out GEMM through a transposed weight padded to four columns (three bf16 products
// per fp32 product), ltrx_out_act_fwd and a sum over the last axis: here the products are exact fp32 fused multiply-adds.
//
// WORK SPLIT.  One wave per row, 4 waves per workgroup, the workgroups stride over the rows.  A row is D / 4 float4 units; lane l owns
// units l, l + 64, l + 128, l + 192 (D <= 1024: at most four) and loads them all before the first multiply, so a wave has up to 4 KB of
// its row in flight.  The row is read from HBM ONCE for all n_out outputs: n_out independent accumulators live in registers (the kernel
// is a template over n_out), each taking the lane's columns in ascending order, and each is closed by wave_sum (ltrx_device.h: a fixed
// order).  Every lane then holds all n_out sums; lane k keeps p_k and stores it, lane 0 stores the score: one 4 n_out-byte and one
// 4-byte store per row.
// W IN LDS.  W[n_out, D] is staged once per workgroup, as it lies in memory (4 n_out D bytes, at most 32 KB: below the default
// dynamic-LDS allowance), and every row the workgroup walks reads it from there: lane l reads unit l of row k, consecutive lanes
// consecutive 16-byte words, no bank conflict.  The staging moves float4 where W is 16-byte aligned, dwords otherwise.
// DETERMINISM.  No atomics; a row's results depend on the row, W and bias only -- not on the row count, the grid or the workgroup that
// takes it.
// ROOFLINE: HBM.  4 D bytes in per row (+ 4 (n_out + 1) out); 8 n_out FLOP per float4 unit against 16 bytes is far below the
// machine's balance, and the LDS reads (n_out float4 per unit) stay under the LDS rate for n_out <= 8.  No time has been measured.
#include "ltrx_device.h"

using namespace ltrx;

#define LTRX_OUT_HEAD_MAX_OUT 8
#define LTRX_OUT_HEAD_MAX_D 1024
#define LTRX_OUT_HEAD_UNITS (LTRX_OUT_HEAD_MAX_D / 4 / LTRX_WAVE)      // float4 units of a row per lane

template <int NOUT>
__global__ void __launch_bounds__(256) ltrx_out_head_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ W,
                                                                const float* __restrict__ bias, int rows, int D, int act, bool w_vec,
                                                                float* __restrict__ out, float* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) float lds[];        // W [NOUT][D]
  const int Q = D >> 2;                                               // float4 units per row
  float4* w4 = reinterpret_cast<float4*>(lds);
  if (w_vec) {
    const float4* src = reinterpret_cast<const float4*>(W);
    for (int i = threadIdx.x; i < NOUT * Q; i += blockDim.x) w4[i] = src[i];
  } else {
    for (int i = threadIdx.x; i < NOUT * D; i += blockDim.x) lds[i] = W[i];
  }
  __syncthreads();
  const int lane = lane_id(), wpb = blockDim.x >> 6;
  for (int row = blockIdx.x * wpb + wave_id(); row < rows; row += gridDim.x * wpb) {
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * ldx);
    float4 v[LTRX_OUT_HEAD_UNITS];
#pragma unroll
    for (int i = 0; i < LTRX_OUT_HEAD_UNITS; ++i) {
      const int q = lane + LTRX_WAVE * i;
      v[i] = q < Q ? xr[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float acc[NOUT];
#pragma unroll
    for (int k = 0; k < NOUT; ++k) acc[k] = 0.f;
#pragma unroll
    for (int i = 0; i < LTRX_OUT_HEAD_UNITS; ++i) {
      const int q = lane + LTRX_WAVE * i;
      if (q < Q) {
#pragma unroll
        for (int k = 0; k < NOUT; ++k) {
          const float4 w = w4[k * Q + q];
          acc[k] = __builtin_fmaf(v[i].x, w.x, acc[k]);
          acc[k] = __builtin_fmaf(v[i].y, w.y, acc[k]);
          acc[k] = __builtin_fmaf(v[i].z, w.z, acc[k]);
          acc[k] = __builtin_fmaf(v[i].w, w.w, acc[k]);
        }
      }
    }
    float sum = 0.f, mine = 0.f;
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
      const float z = wave_sum(acc[k]) + bias[k];
      const float p = act == 1 ? 1.0f / (1.0f + expf(-z)) : (act == 2 ? tanhf(z) : z);   // ltrx_out_act_fwd's formulae
      sum += p;
      if (lane == k) mine = p;
    }
    if (out && lane < NOUT) out[(size_t)row * NOUT + lane] = mine;
    if (score && lane == 0) score[row] = sum;
  }
}

template <int NOUT>
static int out_head_launch(const float* x, int ldx, const float* W, const float* bias, int rows, int D, int act, float* out, float* score,
                           hipStream_t s) {
  int g = (rows + 3) / 4;                                             // a wave per row; the rest of the rows by striding
  if (g > 1024) g = 1024;
  const bool w_vec = ((uintptr_t)W & 15) == 0;
  hipLaunchKernelGGL(ltrx_out_head_fwd_kernel<NOUT>, dim3(g), dim3(256), (size_t)NOUT * D * sizeof(float), s, x, ldx, W, bias, rows, D, act,
                     w_vec, out, score);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

extern "C" int ltrx_out_head_fwd(const float* x, int ldx, const float* W, const float* bias, int rows, int D, int n_out, int act, float* out,
                                 float* score, ltrx_stream_t stream) {
  if (!x || !W || !bias || (!out && !score) || rows <= 0 || D <= 0 || n_out <= 0 || ldx < D || act < 0 || act > 2) return LTRX_EINVAL;
  if (n_out > LTRX_OUT_HEAD_MAX_OUT || (D & 3) || D > LTRX_OUT_HEAD_MAX_D || (ldx & 3) || ((uintptr_t)x & 15)) return LTRX_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  switch (n_out) {
    case 1: return out_head_launch<1>(x, ldx, W, bias, rows, D, act, out, score, s);
    case 2: return out_head_launch<2>(x, ldx, W, bias, rows, D, act, out, score, s);
    case 3: return out_head_launch<3>(x, ldx, W, bias, rows, D, act, out, score, s);
    case 4: return out_head_launch<4>(x, ldx, W, bias, rows, D, act, out, score, s);
    case 5: return out_head_launch<5>(x, ldx, W, bias, rows, D, act, out, score, s);
    case 6: return out_head_launch<6>(x, ldx, W, bias, rows, D, act, out, score, s);
    case 7: return out_head_launch<7>(x, ldx, W, bias, rows, D, act, out, score, s);
    default: return out_head_launch<8>(x, ldx, W, bias, rows, D, act, out, score, s);
  }
}
