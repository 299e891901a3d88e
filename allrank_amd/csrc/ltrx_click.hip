// Clicks on ranked slates: the click models of allrank/click_models behind rank_and_click.py:88, one workgroup per slate.
// Reference: BaseCascadeModel.click / OnlyRelevantClickModel.click (candidates), MaxClicksModel (cumsum <= max), DiverseClicksModel
// (cascade_models.py:57-90: the q quantile of all pairwise distances is the duplicate margin; candidates are visited in rank order and
// clicked iff farther than the margin from every item clicked so far -- duplicate_aware.py:27-34).
//
// ARITHMETIC (the contract of include/ltrx.h).  click_add_square / click_root are the ONE statement of a pair's distance: fp64, the
// squares of the differences added over k ascending, every operation rounded on its own (no contraction into an FMA: numpy and scipy do
// not fuse), a correctly rounded square root.  It is symmetric in the pair.  The quantile and the greedy comparisons read the SAME stored
// value of a pair, so for an odd number of pairs, where the margin is one of the distances, that pair compares equal to the margin.
//
// A workgroup walks slates s = blockIdx.x, blockIdx.x + gridDim.x, ... of slate_order.  Per slate:
//   1  candidate flags of the n items into LDS (all threads), compacted in rank order by wave 0 (ballot + popcount), cut to the first
//      max_candidates (and, without `diverse`, to the first max_clicks: the clicks ARE the candidates then);
//   2  (diverse, and a margin is asked for or at least two candidates: with fewer no comparison can change the result)
//      the n (n - 1) / 2 distances by 64 x 64 tiles of pairs on and above the diagonal: LTRX_CLICK_KC features of the tile's 64 + 64
//      rows are staged in LDS (coalesced reads of the rows, a row stride of KC + 1 floats: no bank conflict), wave w owns rows
//      4 w .. 4 w + 3 of the tile and lane c its column c, so a pair's sum lives in ONE thread and runs over k ascending across the
//      chunks.  They go into LDS while n <= LTRX_CLICK_LDS_SLATE_LEN, else into this workgroup's slab of the workspace (a generic
//      pointer serves both; __syncthreads orders global accesses inside a workgroup);
//   3  the two order statistics of numpy's linear quantile by a radix select on the bit patterns (non-negative doubles order as their
//      uint64 patterns): 8 passes of 8 bits, a 256-bin integer histogram in LDS (a wave first folds the lanes that share its two
//      commonest digits into one add each: the leading bytes of distances are all alike), then ONE pass for the next larger value;
//   4  the greedy scan by wave 0: lanes over the clicked items, a lookup of the stored distance each, a ballot; stops at max_clicks;
//   5  clicks_out: 0 on the valid items, -1 behind them, then 1 on the clicked.
// The only atomics are integer ones in LDS (histogram counts, a uint64 minimum): results do not depend on the order of execution.
#include "ltrx_device.h"

using namespace ltrx;

#define LTRX_CLICK_HIST_BINS 256
#define LTRX_CLICK_SCRATCH_WORDS 8      // uint64 words shared by the phases of one slate

static inline size_t click_pairs(int n) { return n > 1 ? (size_t)n * (size_t)(n - 1) / 2 : 0; }

#define LTRX_CLICK_TILE 64              // pairs are computed by tiles of 64 x 64 rows
#define LTRX_CLICK_KC 32                // features of a tile's rows staged in LDS at a time
#define LTRX_CLICK_STAGE_FLOATS (2 * LTRX_CLICK_TILE * (LTRX_CLICK_KC + 1))
#define LTRX_CLICK_THREADS 1024         // of a diverse launch: 16 waves x 4 rows = a tile's 64 rows

// a pair's distance: s = 0, then s = click_add_square(s, a_k, b_k) for k ascending, then click_root(s)
__device__ __forceinline__ double click_add_square(double s, float a, float b) {
  const double d = __dsub_rn((double)a, (double)b);
  return __dadd_rn(s, __dmul_rn(d, d));
}
__device__ __forceinline__ double click_root(double s) { return __dsqrt_rn(s); }

// index of the pair (i < j) of a slate of n items in the row-major upper triangle
__device__ __forceinline__ int click_pair(int i, int j, int n) { return i * (2 * n - i - 1) / 2 + (j - i - 1); }

// key of ascending rank r (0-based) among keys[0 .. N): all threads call, all get the result.  hist: LTRX_CLICK_HIST_BINS counters,
// sh: two uint64 words.
__device__ __forceinline__ uint64_t click_select(const uint64_t* keys, int N, int r, uint32_t* hist, uint64_t* sh) {
  uint64_t prefix = 0;
  int rank = r;
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int t = threadIdx.x; t < LTRX_CLICK_HIST_BINS; t += blockDim.x) hist[t] = 0;
    __syncthreads();
    const uint64_t himask = shift == 56 ? 0ull : (~0ull << (shift + 8));
    for (int p0 = 0; p0 < N; p0 += blockDim.x) {             // (whole waves walk the loop: the ballots below see every lane)
      const int p = p0 + threadIdx.x;
      bool live = false;
      uint32_t bin = 0;
      if (p < N) {
        const uint64_t k = keys[p];
        live = (k & himask) == prefix;
        bin = (uint32_t)(k >> shift) & 255u;
      }
      for (int round = 0; round < 2; ++round) {               // the wave's two commonest digits: one add each
        const uint64_t m = __ballot(live);
        if (m == 0ull) break;
        const int leader = __ffsll((unsigned long long)m) - 1;
        const uint32_t lb = __shfl(bin, leader, 64);
        const uint64_t same = __ballot(live && bin == lb);
        if (lane_id() == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
        if (bin == lb) live = false;
      }
      if (live) atomicAdd(&hist[bin], 1u);
    }
    __syncthreads();
    if (wave_id() == 0) {                                    // lane l owns bins 4l .. 4l+3
      uint32_t h[4];
      uint32_t tot = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h[e] = hist[4 * lane_id() + e];
        tot += h[e];
      }
      uint32_t inc = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane_id() >= o) inc += up;
      }
      const uint64_t over = __ballot(inc > (uint32_t)rank);  // never empty: the counted keys number more than rank
      const int first = __ffsll((unsigned long long)over) - 1;
      if (lane_id() == first) {
        uint32_t c = inc - tot;
        int e = 0;
        while (e < 3 && c + h[e] <= (uint32_t)rank) c += h[e++];
        sh[0] = (uint64_t)(4 * lane_id() + e);
        sh[1] = (uint64_t)((uint32_t)rank - c);
      }
    }
    __syncthreads();
    prefix |= sh[0] << shift;
    rank = (int)sh[1];
    __syncthreads();                                         // sh and hist are rewritten by the next pass
  }
  return prefix;
}

__global__ void __launch_bounds__(1024) ltrx_click_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const int32_t* __restrict__ cu, const int32_t* __restrict__ order, int B,
                                                         int max_len, int F, int L, const double* __restrict__ u,
                                                         const double* __restrict__ observe_p, float threshold, int max_candidates,
                                                         int diverse, double q, int max_clicks, float* __restrict__ clicks_out,
                                                         double* __restrict__ margin_out, double* __restrict__ slabs, size_t slab_pairs,
                                                         int lds_pairs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  double* lds_dist = reinterpret_cast<double*>(lds_raw);                               // [lds_pairs]
  uint64_t* sh = reinterpret_cast<uint64_t*>(lds_dist + lds_pairs);                    // [LTRX_CLICK_SCRATCH_WORDS]
  uint32_t* hist = reinterpret_cast<uint32_t*>(sh + LTRX_CLICK_SCRATCH_WORDS);         // [LTRX_CLICK_HIST_BINS]
  int* cl = reinterpret_cast<int*>(hist + LTRX_CLICK_HIST_BINS);                       // [max_len] flags, then the candidate list
  float* stage = reinterpret_cast<float*>(cl + max_len);                               // [LTRX_CLICK_STAGE_FLOATS] (diverse only)
  int cap = max_candidates < 0 ? max_len : min(max_candidates, max_len);
  if (!diverse && max_clicks >= 0) cap = min(cap, max_clicks);

  for (int s = blockIdx.x; s < B; s += gridDim.x) {
    int b = order ? order[s] : s;
    b = min(max(b, 0), B - 1);
    const int lo = cu[b];
    const int n = min(max(cu[b + 1] - lo, 0), max_len);
    const float* ys = y + (size_t)b * L;
    const float* xs = x + (size_t)b * L * F;
    float* out = clicks_out + (size_t)b * L;

    // 1: candidates
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const bool observed = !u || observe_p[i] >= u[(size_t)lo + i];
      cl[i] = (observed ? ys[i] : 0.0f) >= threshold;
    }
    for (int i = threadIdx.x; i < L; i += blockDim.x) out[i] = i < n ? 0.0f : -1.0f;
    __syncthreads();
    if (wave_id() == 0) {
      int nc = 0;
      for (int base = 0; base < n; base += 64) {
        const int i = base + lane_id();
        const bool c = i < n && cl[i] != 0;
        const uint64_t mask = __ballot(c);
        if (c) {
          const int pos = nc + __popcll(mask & ((1ull << lane_id()) - 1ull));
          if (pos < cap) cl[pos] = i;                         // pos <= i: the flags of later chunks are still unread and untouched
        }
        nc += __popcll(mask);
      }
      if (lane_id() == 0) sh[2] = (uint64_t)min(nc, cap);
    }
    __syncthreads();
    const int nc = (int)sh[2];
    int nclicked = nc;                                        // without a greedy scan the clicks are the candidates
    double margin = 0.0;

    if (diverse && n > 1 && (margin_out || nc >= 2)) {
      // 2: distances
      const int N = n * (n - 1) / 2;
      double* dist = n <= LTRX_CLICK_LDS_SLATE_LEN ? lds_dist : slabs + (size_t)blockIdx.x * slab_pairs;
      float* As = stage;                                                               // [TILE][KC + 1] rows i0 ..
      float* Bs = stage + LTRX_CLICK_TILE * (LTRX_CLICK_KC + 1);                       // [TILE][KC + 1] rows j0 ..
      const int ntile = (n + LTRX_CLICK_TILE - 1) / LTRX_CLICK_TILE;
      for (int ti = 0; ti < ntile; ++ti) {
        for (int tj = ti; tj < ntile; ++tj) {
          const int i0 = ti * LTRX_CLICK_TILE, j0 = tj * LTRX_CLICK_TILE;
          double acc[4] = {0.0, 0.0, 0.0, 0.0};
          for (int k0 = 0; k0 < F; k0 += LTRX_CLICK_KC) {
            const int kc = min(LTRX_CLICK_KC, F - k0);
            __syncthreads();                                  // the previous chunk is consumed
            for (int e = threadIdx.x; e < LTRX_CLICK_TILE * LTRX_CLICK_KC; e += blockDim.x) {
              const int r = e / LTRX_CLICK_KC, k = e % LTRX_CLICK_KC;
              if (k < kc) {
                As[r * (LTRX_CLICK_KC + 1) + k] = i0 + r < n ? xs[(size_t)(i0 + r) * F + k0 + k] : 0.0f;
                Bs[r * (LTRX_CLICK_KC + 1) + k] = j0 + r < n ? xs[(size_t)(j0 + r) * F + k0 + k] : 0.0f;
              }
            }
            __syncthreads();
            const float* brow = Bs + lane_id() * (LTRX_CLICK_KC + 1);
            const float* arow = As + wave_id() * 4 * (LTRX_CLICK_KC + 1);
            for (int k = 0; k < kc; ++k) {
              const float bj = brow[k];
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[r] = click_add_square(acc[r], arow[r * (LTRX_CLICK_KC + 1) + k], bj);
            }
          }
          const int j = j0 + lane_id();
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = i0 + wave_id() * 4 + r;
            if (i < j && j < n) dist[click_pair(i, j, n)] = click_root(acc[r]);
          }
        }
      }
      __syncthreads();
      // 3: numpy's linear quantile
      const double v = __dmul_rn(q, (double)(N - 1));
      const int klo = min((int)floor(v), N - 1);
      const int khi = min(klo + 1, N - 1);
      const double t = __dsub_rn(v, (double)klo);
      const uint64_t* keys = reinterpret_cast<const uint64_t*>(dist);
      const uint64_t ka = click_select(keys, N, klo, hist, sh);
      uint64_t kb = ka;
      if (khi != klo) {
        if (threadIdx.x == 0) {
          sh[3] = 0;
          sh[4] = ~0ull;
        }
        __syncthreads();
        uint32_t le = 0;
        uint64_t gt = ~0ull;
        for (int p = threadIdx.x; p < N; p += blockDim.x) {
          const uint64_t k = keys[p];
          if (k <= ka) ++le; else gt = k < gt ? k : gt;
        }
        if (le) atomicAdd(reinterpret_cast<unsigned long long*>(&sh[3]), (unsigned long long)le);
        if (gt != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(&sh[4]), (unsigned long long)gt);
        __syncthreads();
        kb = sh[3] > (uint64_t)(klo + 1) ? ka : sh[4];
      }
      const double da = __builtin_bit_cast(double, ka), db = __builtin_bit_cast(double, kb);
      const double diff = __dsub_rn(db, da);
      margin = t < 0.5 ? __dadd_rn(da, __dmul_rn(diff, t)) : __dsub_rn(db, __dmul_rn(diff, __dsub_rn(1.0, t)));
      // 4: greedy scan, clicked items kept in place at the head of cl (never more of them than candidates visited)
      if (wave_id() == 0) {
        const int stop = max_clicks < 0 ? nc : min(max_clicks, nc);
        int k = 0;
        for (int c = 0; c < nc && k < stop; ++c) {
          const int i = cl[c];
          bool near = false;
          for (int e = lane_id(); e < k; e += 64) near |= !(dist[click_pair(cl[e], i, n)] > margin);
          if (__ballot(near) == 0ull) {
            if (lane_id() == 0) cl[k] = i;
            ++k;
            __threadfence_block();
          }
        }
        if (lane_id() == 0) sh[5] = (uint64_t)k;
      }
      __syncthreads();
      nclicked = (int)sh[5];
    } else if (diverse && max_clicks >= 0) {
      nclicked = min(nc, max_clicks);
    }
    // 5
    if (margin_out && threadIdx.x == 0) margin_out[b] = margin;
    for (int e = threadIdx.x; e < nclicked; e += blockDim.x) out[cl[e]] = 1.0f;
    __syncthreads();                                          // cl and sh belong to the next slate from here
  }
}

static inline bool click_needs_slab(int max_len, int diverse) { return diverse && max_len > LTRX_CLICK_LDS_SLATE_LEN; }

extern "C" size_t ltrx_click_workspace_bytes(int B, int max_len, int diverse) {
  if (B <= 0 || max_len <= 0 || !click_needs_slab(max_len, diverse)) return 0;
  return (size_t)(B < LTRX_CLICK_SLAB_WORKGROUPS ? B : LTRX_CLICK_SLAB_WORKGROUPS) * click_pairs(max_len) * sizeof(double);
}

extern "C" int ltrx_click_slates_cu(const float* x, const float* y, const int32_t* cu_seqlens, const int32_t* slate_order, int B,
                                    int max_len, int F, int L, const double* u, const double* observe_p, float threshold,
                                    int max_candidates, int diverse, const double* q_host, int max_clicks, float* clicks_out,
                                    double* margin_out, void* ws, ltrx_stream_t stream) {
  if (!x || !y || !cu_seqlens || !clicks_out || B <= 0 || F <= 0 || max_len <= 0 || L < max_len) return LTRX_EINVAL;
  if ((u == nullptr) != (observe_p == nullptr)) return LTRX_EINVAL;
  if (diverse && !q_host) return LTRX_EINVAL;
  const double q = diverse ? *q_host : 0.0;
  if (!(q >= 0.0 && q <= 1.0)) return LTRX_EINVAL;
  if (max_len > (diverse ? LTRX_MAX_SLATE_LEN : LTRX_MAX_METRIC_SLATE_LEN)) return LTRX_EUNSUPPORTED;
  const bool slab = click_needs_slab(max_len, diverse);
  if (slab && !ws) return LTRX_EINVAL;

  const int lds_pairs = diverse ? (int)click_pairs(max_len < LTRX_CLICK_LDS_SLATE_LEN ? max_len : LTRX_CLICK_LDS_SLATE_LEN) : 0;
  const size_t lds = (size_t)lds_pairs * sizeof(double) + LTRX_CLICK_SCRATCH_WORDS * sizeof(uint64_t) +
                     LTRX_CLICK_HIST_BINS * sizeof(uint32_t) + (size_t)max_len * sizeof(int) +
                     (diverse ? LTRX_CLICK_STAGE_FLOATS * sizeof(float) : 0);
  if (lds > LTRX_DEFAULT_DYNAMIC_LDS_BYTES) {
    static std::atomic<uint64_t> attr_done{0};
    const int arc = ltrx_allow_dynamic_lds(attr_done, {{ltrx_click_kernel, LTRX_LDS_ARRAY_BUDGET_BYTES}});
    if (arc != LTRX_OK) return arc;
  }
  // a workgroup that may need a slab owns one; without slabs the grid covers the slates up to a few workgroups per CU
  const int cap = slab ? LTRX_CLICK_SLAB_WORKGROUPS : 4096;
  const dim3 grid(B < cap ? B : cap), block(diverse ? LTRX_CLICK_THREADS : (max_len > 128 ? 1024 : 256));
  hipLaunchKernelGGL(ltrx_click_kernel, grid, block, lds, (hipStream_t)stream, x, y, cu_seqlens, slate_order, B, max_len, F, L, u,
                     observe_p, threshold, max_candidates, diverse, q, max_clicks, clicks_out, margin_out, (double*)ws,
                     click_pairs(max_len), lds_pairs);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}
