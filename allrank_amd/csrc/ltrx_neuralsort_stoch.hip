// Stochastic NeuralSort around the NeuralNDCG kernels (ltrx_neuralndcg.hip): the batch-wide minimum, the Gumbel draw, the
// perturbed pseudo slates, and the fold-back of their gradient.
// Reference: allrank/models/losses/loss_utils.py:70-112, allrank/models/losses/neuralNDCG.py:35-47,69.
//
//   m        = min over ALL B * L scores, padded slots included                              (loss_utils.py:102)
//   s_pos    = s + |m|;  with log_scores: log(s_pos + 1e-10)                                  (:102,:104-105)
//   s_pert_i = s_pos[b] + beta * g[sample, b]        for pseudo slate i = sample * B + b     (:103,:107)
//   g        = -log(-log(U + 1e-10) + 1e-10),  U uniform on [0, 1)                            (:70-81)
// Pseudo slate i is sorted under the padding mask of slate i / n_samples (mask.repeat_interleave, :108, neuralNDCG.py:41) and read
// out with the labels of slate i % B (neuralNDCG.py:44-47); the labels handed on to ltrx_neuralndcg_fwd_bwd encode that pair.
// Backward: d s_pert / d s = w (1 or 1 / (s + |m| + 1e-10)) elementwise, plus the path through |m|: sign(m) times the sum of all
// elementwise gradients, spread evenly over the elements that attain the minimum (torch's min() backward).
//
// All kernels stream: lanes run along L (one wave per pseudo slate) or along the flat B * L grid, 16 bytes per lane where the row
// length and the pointers allow it; each of the [n_samples, B, L] arrays is written once and read once.  The two reductions are
// per-workgroup partials in the workspace followed by one reducing workgroup in a later launch of the same stream -- no atomics,
// no dependence on dispatch order: the same inputs and step word give the same bits on every call.
#include "ltrx_device.h"

// the reference materialises s + |m| and beta * g before adding them (loss_utils.py:102,107): keep the rounded products
#pragma clang fp contract(off)

using namespace ltrx;

namespace {
constexpr int kMaxPartials = 256;   // workgroups of a partial-reduction launch (one partial per thread of the reducing workgroup)
constexpr float kGumbelEps = 1e-10f;   // loss_utils.py:70
constexpr float kLogEps = 1e-10f;      // loss_utils.py:105

struct StochWs {
  float* pmin;   // [kMaxPartials] per-workgroup minimum
  int* pcnt;     // [kMaxPartials] elements of the workgroup equal to its minimum
  float* psum;   // [kMaxPartials] per-workgroup sum of gs
  float* tot;    // [1] sum of gs
};

inline StochWs carve(void* ws) {
  StochWs w;
  char* p = (char*)ws;
  w.pmin = (float*)p;  p += kMaxPartials * 4;
  w.pcnt = (int*)p;    p += kMaxPartials * 4;
  w.psum = (float*)p;  p += kMaxPartials * 4;
  w.tot = (float*)p;
  return w;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// workgroups of a flat pass over n elements, 256 threads of `per` elements each
inline int flat_grid(size_t n, int per) {
  const size_t g = (n + (size_t)256 * per - 1) / ((size_t)256 * per);
  return (int)(g < (size_t)kMaxPartials ? (g ? g : 1) : (size_t)kMaxPartials);
}

__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }
__device__ __forceinline__ float block_min(float v, float* red) { return -block_max(-v, red); }

__device__ __forceinline__ float gumbel_of(uint32_t key, uint64_t idx) {
  const float u = (float)(counter_hash(key, idx) >> 8) * (1.0f / 16777216.0f);
  return -logf(-logf(u + kGumbelEps) + kGumbelEps);
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------
// batch minimum with its tie count.  Stage 1: workgroup g reduces a fixed slice of the flat score array.
// ---------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256) ltrx_nsort_min_partial_kernel(const float* __restrict__ s, size_t n, float* __restrict__ pmin,
                                                                     int* __restrict__ pcnt) {
  __shared__ float red[LTRX_MAX_WAVES];
  __shared__ int redi[LTRX_MAX_WAVES];
  const size_t stride = (size_t)gridDim.x * 256;
  const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  float m = INFINITY;
  int c = 0;
  auto take = [&](float v) {
    if (v < m) { m = v; c = 1; }
    else if (v == m) ++c;
  };
  if (VEC) {
    const float4* s4 = reinterpret_cast<const float4*>(s);
    for (size_t i = t0; i < n / 4; i += stride) {
      const float4 v = s4[i];
      take(v.x); take(v.y); take(v.z); take(v.w);
    }
  } else {
    for (size_t i = t0; i < n; i += stride) take(s[i]);
  }
  const float bm = block_min(m, red);
  const int bc = block_sum_i(m == bm ? c : 0, redi);
  if (threadIdx.x == 0) {
    pmin[blockIdx.x] = bm;
    pcnt[blockIdx.x] = bc;
  }
}

// Stage 2, one workgroup: smin = (m, ties); also the pseudo batch's normaliser cnt_ps = nonzero_count * n_samples
__global__ void __launch_bounds__(kMaxPartials) ltrx_nsort_min_final_kernel(const float* __restrict__ pmin, const int* __restrict__ pcnt,
                                                                             int parts, const float* __restrict__ nonzero_count,
                                                                             float n_samples, float* __restrict__ smin,
                                                                             float* __restrict__ cnt_ps) {
  __shared__ float red[LTRX_MAX_WAVES];
  __shared__ int redi[LTRX_MAX_WAVES];
  const int t = threadIdx.x;
  const float v = t < parts ? pmin[t] : INFINITY;
  const float m = block_min(v, red);
  const int ties = block_sum_i((t < parts && v == m) ? pcnt[t] : 0, redi);
  if (t == 0) {
    smin[0] = m;
    smin[1] = (float)ties;
    cnt_ps[0] = nonzero_count[0] * n_samples;
  }
}

// ---------------------------------------------------------------------------------------------------------
// the pseudo slates: one wave per pseudo slate i = sample * B + b, lanes along L
// ---------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256) ltrx_nsort_perturb_kernel(const float* __restrict__ scores, const float* __restrict__ y_true,
                                                                 const float* __restrict__ idcg, const float* __restrict__ smin, int B,
                                                                 int L, int S, float pad, float beta, int log_scores, int transposed,
                                                                 uint32_t seed, const uint32_t* __restrict__ seed_step,
                                                                 const float* __restrict__ gumbel_in, float* __restrict__ s_pert,
                                                                 float* __restrict__ y_ps, int32_t* __restrict__ k_rows,
                                                                 float* __restrict__ idcg_ps, float* __restrict__ gumbel_out) {
  const int i = blockIdx.x * 4 + wave_id();
  if (i >= S * B) return;                     // (wave-uniform)
  if (seed_step) seed ^= seed_step[0] * 0x9E3779B9u;
  const int b = i % B;                        // scores, read-out labels, idcg: slate i % B
  const int sort_src = i / S;                 // padding mask of the sort: slate i / n_samples
  const float am = fabsf(smin[0]);
  const float* sr = scores + (size_t)b * L;
  const float* yt = y_true + (size_t)b * L;
  const float* ys = y_true + (size_t)sort_src * L;
  const size_t row = (size_t)i * L;
  int valid = 0;
  auto item = [&](float s, float t, float tsort, float g) {
    float sp = s + am;
    if (log_scores) sp = logf(sp + kLogEps);
    const float bg = beta * g;
    float y;
    if (transposed) y = (tsort == pad) ? LTRX_NEURALSORT_PAD : t;
    else y = (tsort == pad) ? pad : ((t == pad) ? 0.f : t);
    valid += (t != pad);
    return make_float2(sp + bg, y);
  };
  if (VEC) {
    for (int l = lane_id() * 4; l < L; l += 256) {
      const float4 s = *reinterpret_cast<const float4*>(sr + l);
      const float4 t = *reinterpret_cast<const float4*>(yt + l);
      const float4 ts = *reinterpret_cast<const float4*>(ys + l);
      float4 g;
      if (gumbel_in) g = *reinterpret_cast<const float4*>(gumbel_in + row + l);
      else g = make_float4(gumbel_of(seed, row + l), gumbel_of(seed, row + l + 1), gumbel_of(seed, row + l + 2),
                           gumbel_of(seed, row + l + 3));
      const float2 o0 = item(s.x, t.x, ts.x, g.x), o1 = item(s.y, t.y, ts.y, g.y), o2 = item(s.z, t.z, ts.z, g.z),
                   o3 = item(s.w, t.w, ts.w, g.w);
      *reinterpret_cast<float4*>(s_pert + row + l) = make_float4(o0.x, o1.x, o2.x, o3.x);
      *reinterpret_cast<float4*>(y_ps + row + l) = make_float4(o0.y, o1.y, o2.y, o3.y);
      if (gumbel_out) *reinterpret_cast<float4*>(gumbel_out + row + l) = g;
    }
  } else {
    for (int l = lane_id(); l < L; l += 64) {
      const float g = gumbel_in ? gumbel_in[row + l] : gumbel_of(seed, row + l);
      const float2 o = item(sr[l], yt[l], ys[l], g);
      s_pert[row + l] = o.x;
      y_ps[row + l] = o.y;
      if (gumbel_out) gumbel_out[row + l] = g;
    }
  }
  valid = wave_sum_i(valid);
  if (lane_id() == 0) {
    if (k_rows) k_rows[i] = valid;
    idcg_ps[i] = idcg[b];
  }
}

// ---------------------------------------------------------------------------------------------------------
// fold: gs = w * sum over the samples, flat over B * L; stage 1 of sum(gs)
// ---------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256) ltrx_nsort_fold_kernel(const float* __restrict__ grad_ps, const float* __restrict__ scores,
                                                              const float* __restrict__ smin, size_t n, int S, int log_scores,
                                                              float* __restrict__ grad_out, float* __restrict__ psum) {
  __shared__ float red[LTRX_MAX_WAVES];
  const size_t stride = (size_t)gridDim.x * 256;
  const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  const float am = fabsf(smin[0]);
  float acc = 0.f;
  auto weight = [&](float s) { return log_scores ? 1.0f / ((s + am) + kLogEps) : 1.0f; };
  if (VEC) {
    const float4* g4 = reinterpret_cast<const float4*>(grad_ps);
    for (size_t e = t0; e < n / 4; e += stride) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < S; ++k) {
        const float4 v = g4[(size_t)k * (n / 4) + e];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
      }
      const float4 s = reinterpret_cast<const float4*>(scores)[e];
      a.x *= weight(s.x); a.y *= weight(s.y); a.z *= weight(s.z); a.w *= weight(s.w);
      reinterpret_cast<float4*>(grad_out)[e] = a;
      acc += a.x; acc += a.y; acc += a.z; acc += a.w;
    }
  } else {
    for (size_t e = t0; e < n; e += stride) {
      float a = 0.f;
      for (int k = 0; k < S; ++k) a += grad_ps[(size_t)k * n + e];
      a *= weight(scores[e]);
      grad_out[e] = a;
      acc += a;
    }
  }
  const float tot = block_sum(acc, red);
  if (threadIdx.x == 0) psum[blockIdx.x] = tot;
}

// stage 2, one workgroup: tot = sum of the partials in thread order
__global__ void __launch_bounds__(kMaxPartials) ltrx_nsort_sum_final_kernel(const float* __restrict__ psum, int parts,
                                                                             float* __restrict__ tot) {
  __shared__ float red[LTRX_MAX_WAVES];
  const float t = block_sum((int)threadIdx.x < parts ? psum[threadIdx.x] : 0.f, red);
  if (threadIdx.x == 0) tot[0] = t;
}

// the path through |m|: every element that attains the minimum gets sign(m) * sum(gs) / ties
__global__ void __launch_bounds__(256) ltrx_nsort_min_grad_kernel(const float* __restrict__ scores, const float* __restrict__ smin,
                                                                  const float* __restrict__ tot, size_t n, float* __restrict__ grad_out) {
  const float m = smin[0];
  if (m == 0.f) return;                       // sign(0) = 0
  const float add = (m > 0.f ? tot[0] : -tot[0]) / smin[1];
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride)
    if (scores[e] == m) grad_out[e] += add;
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------

extern "C" size_t ltrx_neuralsort_stoch_workspace_bytes(int B, int L, int n_samples) {
  if (B <= 0 || L <= 0 || n_samples <= 0) return 0;
  return (size_t)3 * kMaxPartials * 4 + 64;
}

extern "C" int ltrx_neuralsort_perturb(const float* scores, const float* y_true, const float* idcg, const float* nonzero_count, int B,
                                       int L, int n_samples, float pad_value, float beta, int log_scores, int transposed, uint32_t seed,
                                       const uint32_t* seed_step, const float* gumbel_in, float* s_pert, float* y_ps, int32_t* k_rows,
                                       float* idcg_ps, float* cnt_ps, float* smin_out, float* gumbel_out, void* ws,
                                       ltrx_stream_t stream) {
  if (!scores || !y_true || !idcg || !nonzero_count || !s_pert || !y_ps || !idcg_ps || !cnt_ps || !smin_out || !ws) return LTRX_EINVAL;
  if (B <= 0 || L <= 0 || n_samples <= 0 || (!transposed && !k_rows)) return LTRX_EINVAL;
  if (L > LTRX_MAX_SLATE_LEN) return LTRX_EUNSUPPORTED;
  if ((size_t)n_samples * (size_t)B > (size_t)INT32_MAX / 4) return LTRX_EUNSUPPORTED;      // (pseudo slates are counted in int)
  hipStream_t s = (hipStream_t)stream;
  const StochWs w = carve(ws);
  const size_t n = (size_t)B * L;
  const bool vflat = n % 4 == 0 && aligned16(scores);
  const int parts = flat_grid(n, vflat ? 4 : 1);
  if (vflat) hipLaunchKernelGGL(ltrx_nsort_min_partial_kernel<true>, dim3(parts), dim3(256), 0, s, scores, n, w.pmin, w.pcnt);
  else hipLaunchKernelGGL(ltrx_nsort_min_partial_kernel<false>, dim3(parts), dim3(256), 0, s, scores, n, w.pmin, w.pcnt);
  LTRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ltrx_nsort_min_final_kernel, dim3(1), dim3(kMaxPartials), 0, s, w.pmin, w.pcnt, parts, nonzero_count,
                     (float)n_samples, smin_out, cnt_ps);
  LTRX_LAUNCH_CHECK();
  const int rows = n_samples * B;
  const bool vrow = L % 4 == 0 && aligned16(scores) && aligned16(y_true) && aligned16(s_pert) && aligned16(y_ps) &&
                    aligned16(gumbel_in) && aligned16(gumbel_out);
  int32_t* kr = transposed ? nullptr : k_rows;
#define LTRX_NSORT_PERTURB(VEC_)                                                                                                   \
  hipLaunchKernelGGL(ltrx_nsort_perturb_kernel<VEC_>, dim3((rows + 3) / 4), dim3(256), 0, s, scores, y_true, idcg, smin_out, B, L, \
                     n_samples, pad_value, beta, log_scores, transposed, seed, seed_step, gumbel_in, s_pert, y_ps, kr, idcg_ps,  \
                     gumbel_out)
  if (vrow) LTRX_NSORT_PERTURB(true);
  else LTRX_NSORT_PERTURB(false);
#undef LTRX_NSORT_PERTURB
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

extern "C" int ltrx_neuralsort_fold_grad(const float* grad_ps, const float* scores, const float* smin, int B, int L, int n_samples,
                                         int log_scores, float* grad_out, void* ws, ltrx_stream_t stream) {
  if (!grad_ps || !scores || !smin || !grad_out || !ws || B <= 0 || L <= 0 || n_samples <= 0) return LTRX_EINVAL;
  if (L > LTRX_MAX_SLATE_LEN) return LTRX_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const StochWs w = carve(ws);
  const size_t n = (size_t)B * L;
  const bool vec = n % 4 == 0 && aligned16(grad_ps) && aligned16(scores) && aligned16(grad_out);
  const int parts = flat_grid(n, vec ? 4 : 1);
  if (vec) hipLaunchKernelGGL(ltrx_nsort_fold_kernel<true>, dim3(parts), dim3(256), 0, s, grad_ps, scores, smin, n, n_samples,
                              log_scores, grad_out, w.psum);
  else hipLaunchKernelGGL(ltrx_nsort_fold_kernel<false>, dim3(parts), dim3(256), 0, s, grad_ps, scores, smin, n, n_samples, log_scores,
                          grad_out, w.psum);
  LTRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ltrx_nsort_sum_final_kernel, dim3(1), dim3(kMaxPartials), 0, s, w.psum, parts, w.tot);
  LTRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ltrx_nsort_min_grad_kernel, dim3(flat_grid(n, 1)), dim3(256), 0, s, scores, smin, w.tot, n, grad_out);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}
