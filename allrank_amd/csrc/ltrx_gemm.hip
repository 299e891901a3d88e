// fp32-accurate GEMMs on the bf16 matrix cores ("split-bf16"): the dense projections of the scoring model
// (allrank/models/model.py:35-44 FCModel, transformer.py:193-203 q/k/v/out projections, :221-227 feed-forward).
//
// Why: gfx950 has no TF32/xf32 path and its exact-fp32 MFMA runs at the fp32 vector rate (157 TF), 1/16 of the bf16
// MFMA rate (2.5 PF).  Every fp32 operand is therefore split ON THE FLY, while it is staged into LDS, into two bf16
// terms x = hi + lo (hi = bf16(x), lo = bf16(x - hi); bf16 keeps 8 significand bits, unit round-off u = 2^-8, so
// |x - hi| <= 2^-8 |x| and |x - hi - lo| <= 2^-16 |x|; 2^-9 and 2^-18 are the TYPICAL sizes) and the product is evaluated as
//        A B^T  ~=  Ahi Bhi^T + Ahi Blo^T + Alo Bhi^T            (three v_mfma_f32_32x32x16_bf16, fp32 accumulate)
// bf16 x bf16 products are exact in fp32; the dropped terms (lo*lo and the split residuals) are BOUNDED by
// 3 * 2^-16 (1 + 2^-7) = 4.6e-5 of |a||b| per product and are TYPICALLY 3 * 2^-18 with pseudo-random sign (worst entry seen
// on unnormalised operands: 1.2e-5 of sum_k |a||b|), i.e. the same order as the round-off an fp32 accumulation over K = 512
// carries anyway.  3 MFMAs at the bf16 rate = 833 TF "fp32-equivalent" ceiling, 5.3x the fp32-MFMA roof, and each pair of
// fragment loads feeds 3 MFMAs, so the LDS traffic per MFMA is a third of a plain bf16 GEMM's.
// (NTERMS = 3 adds lo2 and uses 6 MFMAs: product error bounded by 4 * 2^-24 (1 + 2^-7) = 2.4e-7, typically 2^-26 -- the strict
//  mode.  ONE product, hi*hi alone: bounded by 2 * 2^-8 (1 + 2^-8) = 7.8e-3, typically 2^-9.  The three bounds are derived and
//  proved entrywise in tests/test_split_bf16_cpu.py.)
//
//   ltrx_gemm_nt : C[M,N] = A[M,K] * B[N,K]^T (+ bias[N]) (+ ReLU)        both operands K-contiguous
//                  -> forward of nn.Linear (B = weight [out,in]) and its input gradient (B = weight^T, kept transposed)
//   ltrx_gemm_tn : C[N',K'] = A[M,N']^T * B[M,K']  (split-K over M, deterministic two-stage reduction)
//                  -> weight gradient dW = dY^T X; both operands are contraction-STRIDED in memory, they are transposed
//                     on the way into LDS (each lane converts a 4(m) x 1(n) register column into one 8-byte LDS write).
//
// Two kernel families (the host wrappers pick per shape):
//   * 128 x 128 x 32 tiles, 4 waves (2 x 2) of 64 x 64 wave tiles, one LDS stage (32 KB), two workgroups per CU -- every
//     shape, ragged edges, the strict 3-term mode; global loads of K-tile t+1 are issued into registers before the MFMAs of
//     tile t (register double buffering).
//   * 256 x 256 x 32 tiles, 8 waves (2 x 4) of 128 x 64 wave tiles, two LDS stages (128 KB, one workgroup per CU), LDS-only
//     barrier, nontemporal output -- the big projections and their weight gradients (ltrx_gemm_nt256_kernel,
//     ltrx_gemm_tn256_kernel below; 1.3-1.6x the small tile on those shapes, see DESIGN.md section 4 for the measurements).
// LDS operand images are [row][k] bf16 with k contiguous, UNPADDED 64-byte rows and an XOR swizzle of the 16-byte chunks
// (swz_off): every lane fetches its 8-element MFMA fragment with one ds_read_b128, conflict-free in both directions.
// Workgroup ids are remapped so that the column tiles of one A row-panel run on the same XCD (shared L2).
#include "ltrx_mfma.h"
#include "ltrx_rowreg.h"
#include <limits.h>

using ltrx::lds_only_barrier;
using ltrx::rowmap;

namespace {

constexpr int BN = 128;   // output-tile columns (rows of B); the row count BM_ and the K-tile depth BK_ are template parameters

// split 4 floats into hi / lo (/ lo2) bf16 quads (LTRX_SPLIT_BF16 per element)
template <int NTERMS>
__device__ __forceinline__ void split4(const float4 v, bf16x4& hi, bf16x4& lo, bf16x4& lo2) {
  const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    __bf16 h, l;
    LTRX_SPLIT_BF16(x[e], h, l);
    hi[e] = h;
    lo[e] = l;
    if (NTERMS == 3) lo2[e] = LTRX_BF16_REST(x[e] - (float)h, l);
  }
}

// LDS operand images: [term][row][k] bf16, k contiguous, UNPADDED rows of BK_ elements (64 B at BK_ = 32); the 16-byte
// chunk c of row r is stored at chunk position c ^ swz(r), swz(r) = (r >> 2) & (BK_/8 - 1).  With that swizzle the
// 16-lane groups of a fragment ds_read_b128 (rows {0-3,12-15,20-27}+..., same logical chunk) hit 16 distinct 4-bank
// slots, and the staging ds_write_b64 (8 lanes per row, 2 rows per 16-lane group, rows 64 B apart) covers all 32 write
// banks exactly once: both directions are conflict-free (SQ_LDS_BANK_CONFLICT was 33 % of LDS cycles with padded rows).
template <int NTERMS, int BM_, int BK_>
struct Smem {
  static constexpr int LDK = BK_;
  __bf16 a[NTERMS][BM_ * LDK];
  __bf16 b[NTERMS][BN * LDK];
};

template <int BK_>
__device__ __forceinline__ int swz_off(int row, int k) {       // element offset of (row, k) inside an operand image
  constexpr int CH = BK_ / 8;                                   // 16-byte chunks per row
  const int c = (k >> 3) ^ ((row >> 2) & (CH - 1));
  return row * BK_ + c * 8 + (k & 7);
}

// the MFMA phase over one staged K-tile: wave (wr, wc) owns a 64 x 64 sub-tile = 2 x 2 MFMA tiles
template <int NTERMS, int BM_, int BK_>
__device__ __forceinline__ void mma_tile(const Smem<NTERMS, BM_, BK_>& s, int wr, int wc, f32x16 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int ks = 0; ks < BK_ / 16; ++ks) {
    bf16x8 af[NTERMS][2], bfr[NTERMS][2];
#pragma unroll
    for (int t = 0; t < NTERMS; ++t)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[t][i] = *reinterpret_cast<const bf16x8*>(&s.a[t][swz_off<BK_>(wr * 64 + i * 32 + l31, ks * 16 + 8 * half)]);
        bfr[t][i] = *reinterpret_cast<const bf16x8*>(&s.b[t][swz_off<BK_>(wc * 64 + i * 32 + l31, ks * 16 + 8 * half)]);
      }
    // term-major order: consecutive MFMAs write DIFFERENT accumulators (no back-to-back dependent issue); the
    // smallest terms are accumulated first.
#define LTRX_MMA_TERM(TA, TB)                                                                                     \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                     \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[TA][i], bfr[TB][j], acc[i][j], 0, 0, 0);
    if (NTERMS == 3) {
      LTRX_MMA_TERM(NTERMS - 2, NTERMS - 2)
      LTRX_MMA_TERM(0, NTERMS - 1)
      LTRX_MMA_TERM(NTERMS - 1, 0)
    }
    if (NTERMS >= 2) {
      LTRX_MMA_TERM(0, NTERMS >= 2 ? 1 : 0)
      LTRX_MMA_TERM(NTERMS >= 2 ? 1 : 0, 0)
    }
    LTRX_MMA_TERM(0, 0)
#undef LTRX_MMA_TERM
  }
}

// XCD-aware bijective remap of a linear workgroup id (cdna_hip_programming.md §5): ids that are consecutive after
// the remap land on the same XCD, so tiles sharing an operand panel share an L2.
__device__ __forceinline__ int xcd_remap(int id, int n) {
  const int q = n / 8, r = n % 8, xcd = id % 8, k = id / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// NT:  C[M,N] = A[M,K] B[N,K]^T (+bias) (+ReLU | * mask)
// workgroup = 2 * BM_/64 waves: (BM_/64) x 2 grid of 64 x 64 wave tiles over a BM_ x 128 output tile
// ------------------------------------------------------------------------------------------------------------------
template <int NTERMS, int BM_, int BK_>
__global__ void __launch_bounds__(BM_ * 2) __attribute__((amdgpu_waves_per_eu(2, 3))) ltrx_gemm_nt_kernel(const float* __restrict__ A, int lda,
                                                                  const float* __restrict__ B, int ldb,
                                                                  float* __restrict__ C, int ldc, int M, int N, int K,
                                                                  const float* __restrict__ bias, int act,
                                                                  const float* __restrict__ aux, int ldaux, int tiles_n,
                                                                  ltrx::DropSpec drop, const uint32_t* __restrict__ drop_step) {
  constexpr int T = BM_ * 2;                    // threads
  constexpr int C4 = BK_ / 4;                   // float4 per tile row
  constexpr int PA = BM_ * C4 / T;              // float4 per thread for the A tile
  constexpr int PB = BN * C4 / T;               //                     ... B tile
  __shared__ __attribute__((aligned(16))) Smem<NTERMS, BM_, BK_> s;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (id / tiles_n) * BM_, n0 = (id % tiles_n) * BN;
  const int wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
  const int srow = threadIdx.x / C4;            // staging: thread -> (row, float4 column); passes step T / C4 rows
  const int sc4 = (threadIdx.x % C4) * 4;
  constexpr int RSTEP = T / C4;
  float4 ra[PA], rb[PB];

  auto gload = [&](int k0) {
    const int k = k0 + sc4;
#pragma unroll
    for (int p = 0; p < PA; ++p) {
      const int r = srow + RSTEP * p;
      ra[p] = (m0 + r < M && k < K) ? *reinterpret_cast<const float4*>(A + (size_t)(m0 + r) * lda + k)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int p = 0; p < PB; ++p) {
      const int r = srow + RSTEP * p;
      rb[p] = (n0 + r < N && k < K) ? *reinterpret_cast<const float4*>(B + (size_t)(n0 + r) * ldb + k)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto sstore = [&]() {
    bf16x4 h, l, l2;
#pragma unroll
    for (int p = 0; p < PA; ++p) {
      const int o = swz_off<BK_>(srow + RSTEP * p, sc4);
      split4<NTERMS>(ra[p], h, l, l2);
      *reinterpret_cast<bf16x4*>(&s.a[0][o]) = h;
      if (NTERMS >= 2) *reinterpret_cast<bf16x4*>(&s.a[NTERMS >= 2 ? 1 : 0][o]) = l;
      if (NTERMS == 3) *reinterpret_cast<bf16x4*>(&s.a[NTERMS - 1][o]) = l2;
    }
#pragma unroll
    for (int p = 0; p < PB; ++p) {
      const int o = swz_off<BK_>(srow + RSTEP * p, sc4);
      split4<NTERMS>(rb[p], h, l, l2);
      *reinterpret_cast<bf16x4*>(&s.b[0][o]) = h;
      if (NTERMS >= 2) *reinterpret_cast<bf16x4*>(&s.b[NTERMS >= 2 ? 1 : 0][o]) = l;
      if (NTERMS == 3) *reinterpret_cast<bf16x4*>(&s.b[NTERMS - 1][o]) = l2;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = (K + BK_ - 1) / BK_;
  gload(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                 // the previous tile's fragments are consumed
    sstore();
    __syncthreads();
    if (kt + 1 < nk) gload((kt + 1) * BK_);   // in flight during the MFMAs below
    mma_tile<NTERMS, BM_, BK_>(s, wr, wc, acc);
  }

  // epilogue: lane owns column n0 + wc*64 + j*32 + (lane&31); register r is row rowmap(r, half)
  const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
  ltrx::DropSpec dsp = drop;
  if (drop_step) dsp.seed ^= drop_step[0] * 0x9E3779B9u;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wc * 64 + j * 32 + l31;
    if (col >= N) continue;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wr * 64 + i * 32 + rowmap(r, half);
        if (row < M) {
          float v = acc[i][j][r] + bv;
          if (act == 1) v = fmaxf(v, 0.f);
          if (act == 2) v = (aux[(size_t)row * ldaux + col] > 0.f) ? v * drop.inv_keep : 0.f;   // ReLU(+dropout) backward
          else if (drop.thresh != 0u) v *= ltrx::drop_keep_scale(dsp, (uint64_t)row * (uint64_t)N + (uint64_t)col);
          if (act == 3) v += aux[(size_t)row * ldaux + col];                                    // residual stream + drop(branch)
          C[(size_t)row * ldc + col] = v;
        }
      }
  }
}


// ------------------------------------------------------------------------------------------------------------------
// NT, large-tile variant for the big projections: 256 x 256 x 32 tile, 8 waves (2 x 4), wave tile 128 x 64 (128
// accumulator VGPRs), two LDS stages (128 KB: one workgroup per CU) and ONE LDS-only barrier per K-step.
// Why (tools/lab/gemm_ablate.hip, gemm256.hip; MI355X, M 61440 x N 2048 x K 512): in the 128 x 128 kernel the memory side
// (global loads -> split -> LDS) alone takes 340 us and the MFMAs alone 185 us, and the two do not overlap (567 us):
//   * per MFMA the 256 x 256 tile needs half the global-load and LDS-write traffic and 3/4 of the LDS fragment reads;
//   * __syncthreads() drains vmcnt(0), i.e. it exposes the latency of the prefetch issued just before it on every K-step;
//     the barrier here orders LDS only (release/acquire fences on the "local" address space + s_barrier), so the global
//     loads of tile t+2 stay in flight across it -- the prologue's barrier included (the loads of K-tile 1 land behind the MFMAs of
//     tile 0); after the last K-tile there is no barrier at all, the epilogue touches no LDS;
//   * the steady-state loop is branch-free, which lets the scheduler interleave the split/ds_write VALU work of tile t+1
//     with the MFMAs of tile t;
//   * the output tile is streamed with nontemporal stores: C (0.5 GB for the FFN) no longer evicts the operand panels
//     that the other tiles of the same XCD are about to re-read from L2.
// Measured: 567 -> 365 us (FFN1), 560 -> 345 us (FFN2).  Used when N is a multiple of 256, K of 32, and the grid fills
// the chip (a ragged last row tile is handled by clamped loads and guarded stores); everything else (and the strict
// 3-term mode, whose LDS images do not fit twice) stays on the kernel above.
// ------------------------------------------------------------------------------------------------------------------
// BM = 256 (wave tile 128 x 64) or 128 (wave tile 64 x 64, 96 KB of LDS): the 128-row variant is for shapes whose 256-row
// tiling would leave half of the CUs without a tile (M 15360 x N 512: 120 tiles of 256 x 256, 240 of 128 x 256)
// NT = number of bf16 terms per operand: 2 = hi + lo (three products), 1 = hi only (ONE product: the plain-bf16
// throughput mode, precision code 2 of the host wrappers -- NOT the parity arithmetic)
template <int BM, int NT = 2>
struct SmemNT {
  __bf16 a[NT][BM * 32];
  __bf16 b[NT][256 * 32];
};

// BIMG: B points at a pre-split IMAGE of the operand instead of fp32 values -- per 4 consecutive k the 16 bytes {hi0..hi3, lo0..lo3}
// (bf16) in place of the 4 floats, same addressing (ltrx_split_image; the weights and their transposes, refreshed once per optimizer
// step).  The staging of B is then a plain copy: half of the kernel's split work (VALU, and the power it draws) is gone, the bits
// that reach LDS -- and the results -- are identical.
//
// EPI: the epilogue as a compile-time kind.  The dropout-free epilogues the default training step launches are straight-line code --
// no test of act / bias / drop per row quad, one basic block from the last K-step's MFMAs to the last store -- and issue their loads
// EARLY: both bias vectors and the mask word ahead of the last K-step's MFMAs (the staging registers are dead there), the residual tile
// rolled two accumulator blocks ahead of its use, its first two blocks also ahead of those MFMAs.  EPI_GENERIC is the runtime-tested
// epilogue (acts 1 / 2, every dropout form, the ragged last row tile, the one-product mode, B read as fp32): same arithmetic per
// element in the same order, so a launch's bits do not depend on which kind the host picked (nt_epilogue_kind).
// In <false, 256, 2, true> the code after the last MFMA went from ~6000 static instructions, 308 conditional branches and 66 vmcnt
// waits to 200-720 instructions, no branch and 0-14 counted waits (the epilogue's first blocks are scheduled between the last
// K-step's MFMAs).  Measured on the MI355X, 256 slates x 240: 8.48 -> 8.39 ms per step; FFN-1 forward 394 -> 376 us, the QKV
// launches 282 -> 274 and 307 -> 287 us, FFN-2 dgrad 381 -> 372 us; the residual launches keep their ~25 us over their
// residual-free twins -- that is the HBM time of the 126 MB they read, not latency (profiles/NOTES.md, "Straight-line epilogues").
enum : int {
  EPI_GENERIC = 0,
  EPI_PLAIN,        // act 0, no bias: C = acc                      (the input-gradient launches)
  EPI_BIAS,         // act 0: C = acc + bias                        (Q / K / V)
  EPI_RELU_BITS,    // act 4: C = relu(acc + bias), one-bit mask written   (FFN-1 forward)
  EPI_MASK_READ,    // act 5, no bias: C = bit ? acc * inv_keep : 0        (FFN-2 input gradient)
  EPI_RESIDUAL,     // act 3: C = acc + bias + aux                  (out-projection and FFN-2 forward)
  EPI_KINDS
};

// 4x4 transpose inside a lane quad (two DPP butterflies: quad_perm [1,0,3,2] then [2,3,0,1]): registers a0..a3 of the four lanes
// (4 rows of ONE column each) become 4 consecutive columns of one row per lane (row q of the quad); b0 / b1 = bits 0 / 1 of q
__device__ __forceinline__ f32x4 quad_transpose(float a0, float a1, float a2, float a3, bool b0, bool b1) {
  // stage 1: exchange across lane bit 0
  const float r_lo = LTRX_DPP_F(0.f, b0 ? a0 : a1, 0xB1, 0xF, true);
  const float r_hi = LTRX_DPP_F(0.f, b0 ? a2 : a3, 0xB1, 0xF, true);
  const float c0 = b0 ? r_lo : a0, c1 = b0 ? a1 : r_lo, c2 = b0 ? r_hi : a2, c3 = b0 ? a3 : r_hi;
  // stage 2: exchange across lane bit 1
  const float r_a = LTRX_DPP_F(0.f, b1 ? c0 : c2, 0x4E, 0xF, true);
  const float r_b = LTRX_DPP_F(0.f, b1 ? c1 : c3, 0x4E, 0xF, true);
  return f32x4{b1 ? r_a : c0, b1 ? r_b : c1, b1 ? c2 : r_a, b1 ? c3 : r_b};
}

template <bool TAIL, int BM, int NT, bool BIMG, int EPI>
__device__ __forceinline__ void nt256_body(const float* __restrict__ A, int lda, const float* __restrict__ B,
                                           int ldb, float* __restrict__ C, int ldc, int M, int N, int K,
                                           const float* __restrict__ bias, int act,
                                           const float* __restrict__ aux, int ldaux, int tiles_n,
                                           ltrx::DropSpec drop, const uint32_t* __restrict__ drop_step) {
  static_assert(EPI == EPI_GENERIC || (!TAIL && NT == 2), "the straight-line epilogues have no row guard and are built for the parity arithmetic");
  constexpr int BK_ = 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  typedef SmemNT<BM, NT> SmemT;
  constexpr int L1 = NT - 1;           // index of the lo image (aliases hi when there is none; never touched then)
  constexpr int RI = BM / 64;          // 32-row accumulator blocks per wave (two wave rows)
  SmemT* s = reinterpret_cast<SmemT*>(smem_raw);
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (id / tiles_n) * BM, n0 = (id % tiles_n) * 256;
  const int wave = threadIdx.x >> 6, wr = wave >> 2, wc = wave & 3;
  const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
  const int srow = threadIdx.x >> 3, sc4 = (threadIdx.x & 7) * 4;        // staging: 64 rows x 8 float4 per pass, 4 passes
  float4 ra[RI], rb[4];
  // rows of A beyond M (the last row tile of a batch whose size is not a multiple of 256) are clamped to row M-1: they
  // are read but their results are never stored
  // (TAIL: only instantiated for a batch whose row count is not a multiple of 256 -- the extra address registers cost the
  // exact-multiple kernel 20 % when they are always there)
  const int ar0 = TAIL ? min(m0 + srow, M - 1) : m0 + srow;
  const float* Ap = A + (size_t)ar0 * lda + sc4;
  const float* Bp = B + (size_t)(n0 + srow) * ldb + sc4;
  auto gload = [&](int k0) {
#pragma unroll
    for (int p = 0; p < RI; ++p) {
      if constexpr (TAIL)
        ra[p] = *reinterpret_cast<const float4*>(Ap + (size_t)min(64 * p, M - 1 - ar0) * lda + k0);
      else
        ra[p] = *reinterpret_cast<const float4*>(Ap + (size_t)(64 * p) * lda + k0);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) rb[p] = *reinterpret_cast<const float4*>(Bp + (size_t)(64 * p) * ldb + k0);
  };
  auto sstore = [&](SmemT& d) {
    bf16x4 h, l, l2;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int o = swz_off<BK_>(srow + 64 * p, sc4);
      if (p < RI) {
        split4<2>(ra[p < RI ? p : 0], h, l, l2);
        *reinterpret_cast<bf16x4*>(&d.a[0][o]) = h;
        if (NT == 2) *reinterpret_cast<bf16x4*>(&d.a[L1][o]) = l;
      }
      if constexpr (BIMG) {
        *reinterpret_cast<float2*>(&d.b[0][o]) = make_float2(rb[p].x, rb[p].y);
        if (NT == 2) *reinterpret_cast<float2*>(&d.b[L1][o]) = make_float2(rb[p].z, rb[p].w);
      } else {
        split4<2>(rb[p], h, l, l2);
        *reinterpret_cast<bf16x4*>(&d.b[0][o]) = h;
        if (NT == 2) *reinterpret_cast<bf16x4*>(&d.b[L1][o]) = l;
      }
    }
  };
  f32x16 acc[RI][2];
#pragma unroll
  for (int i = 0; i < RI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  auto mma = [&](const SmemT& t) {
#pragma unroll
    for (int ks = 0; ks < BK_ / 16; ++ks) {
      bf16x8 af[NT][RI], bfr[NT][2];
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
          bfr[tt][j] = *reinterpret_cast<const bf16x8*>(&t.b[tt][swz_off<BK_>(wc * 64 + j * 32 + l31, ks * 16 + 8 * half)]);
#pragma unroll
        for (int i = 0; i < RI; ++i)
          af[tt][i] = *reinterpret_cast<const bf16x8*>(&t.a[tt][swz_off<BK_>(wr * (BM / 2) + i * 32 + l31, ks * 16 + 8 * half)]);
      }
#define LTRX_MMA256(TA, TB)                                                                                       \
  _Pragma("unroll") for (int i = 0; i < RI; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                    \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[TA][i], bfr[TB][j], acc[i][j], 0, 0, 0);
      if (NT == 2) {
        LTRX_MMA256(0, L1)
        LTRX_MMA256(L1, 0)
      }
      LTRX_MMA256(0, 0)
#undef LTRX_MMA256
    }
  };

  const int nk = K / BK_;
  gload(0);
  sstore(s[0]);
  if (nk > 1) gload(BK_);
  lds_only_barrier();                         // orders LDS only: the loads of K-tile 1 stay in flight behind the MFMAs of tile 0
  int kt = 0;
  for (; kt + 2 < nk; ++kt) {                 // steady state, branch-free: MFMAs of tile kt | stage tile kt+1 | prefetch kt+2
    mma(s[kt & 1]);
    sstore(s[(kt + 1) & 1]);
    gload((kt + 2) * BK_);
    lds_only_barrier();
  }
  if (kt + 1 < nk) {                          // the second-to-last K-tile (nk >= 2): nothing left to prefetch
    mma(s[kt & 1]);
    sstore(s[(kt + 1) & 1]);
    lds_only_barrier();
    ++kt;
  }

  // Epilogue with 16-byte stores.  An accumulator block keeps one COLUMN per lane (16 rows down the registers); a 4x4
  // transpose inside each lane quad (quad_transpose) turns registers 4g..4g+3 of the four lanes of a quad into 4 consecutive
  // columns of ONE row per lane, so the tile leaves the CU as 32 dwordx4 stores per lane instead of 128 dword stores -- the
  // vector-memory issue path is what bounds this kernel, and the saved activation of the ReLU backward (act 2), the residual
  // (act 3) and the bias are read as float4 the same way.
  const int q = lane & 3;
  const bool b0 = q & 1, b1 = q & 2;
  const int cq = l31 & ~3;
  // act 4 / 5: the ReLU(+dropout) mask as ONE BIT per element instead of the saved fp32 activation.  The lane that produces an
  // element in the forward launch (act 4) is the lane that needs its mask in the input-gradient launch (act 5: same M, N, tiling),
  // so the 128 bits of a lane's 32 row-quads travel as one private 16-byte word per (tile, thread): 1/32 of the bytes act 2 reads.
  uint4* const mask_words = reinterpret_cast<uint4*>(const_cast<float*>(aux)) + (size_t)id * 512 + threadIdx.x;

  if constexpr (EPI != EPI_GENERIC) {
    // Straight-line epilogue (see EPI above).  Element arithmetic = the generic epilogue's expressions in its order: + bias (+ 0
    // without one), ReLU, * inv_keep under the mask, + residual.
    constexpr bool HAS_BIAS = EPI == EPI_BIAS || EPI == EPI_RELU_BITS || EPI == EPI_RESIDUAL;
    constexpr int NBLK = 2 * RI;               // 32 x 32 accumulator blocks of a lane, in epilogue order: block b = (j, i) = (b / RI, b % RI)
    // Addresses as (wave-uniform 64-bit base, in scalar registers) + (one 32-bit byte offset per lane and matrix): a row quad's
    // address then costs scalar arithmetic only, and two VGPRs hold every address of the tile.
    const int wru = __builtin_amdgcn_readfirstlane(wr), wcu = __builtin_amdgcn_readfirstlane(wc);
    const int rowu = m0 + wru * (BM / 2), colu = n0 + wcu * 64;           // the wave's first row / column
    const char* const aux_u = reinterpret_cast<const char*>(aux + (size_t)rowu * ldaux + colu);
    char* const c_u = reinterpret_cast<char*>(C + (size_t)rowu * ldc + colu);
    const uint32_t aux_lane = 4u * (uint32_t)((4 * half + q) * ldaux + cq), c_lane = 4u * (uint32_t)((4 * half + q) * ldc + cq);
    f32x4 bv[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    f32x4 ax[EPI == EPI_RESIDUAL ? NBLK : 1][4];
    unsigned int mbits[4] = {0u, 0u, 0u, 0u};
    auto aux_load = [&](int b) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        ax[b][g] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(
            aux_u + 4 * ((size_t)((b % RI) * 32 + 8 * g) * ldaux + (b / RI) * 32) + aux_lane));
    };
    // issued ahead of the last K-step's MFMAs, whose ~1.5 us cover the round trips
    if constexpr (HAS_BIAS) {
      bv[0] = *reinterpret_cast<const f32x4*>(bias + colu + cq);
      bv[1] = *reinterpret_cast<const f32x4*>(bias + colu + cq + 32);
    }
    if constexpr (EPI == EPI_MASK_READ) {
      const uint4 w = *mask_words;
      mbits[0] = w.x; mbits[1] = w.y; mbits[2] = w.z; mbits[3] = w.w;
    }
    if constexpr (EPI == EPI_RESIDUAL) {
      aux_load(0);
      aux_load(1);
    }
    mma(s[kt & 1]);                           // the last K-tile; the epilogue touches no LDS, so no barrier follows
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
      const int j = b / RI, i = b % RI;
      if constexpr (EPI == EPI_RESIDUAL)
        if (b + 2 < NBLK) aux_load(b + 2);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v = quad_transpose(acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3], b0, b1);
        v.x += bv[j].x; v.y += bv[j].y; v.z += bv[j].z; v.w += bv[j].w;
        if constexpr (EPI == EPI_RELU_BITS) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
          mbits[(b * 4 + g) >> 3] |= ((v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u))
                                     << (((b * 4 + g) & 7) * 4);
        }
        if constexpr (EPI == EPI_MASK_READ) {
          const unsigned int nb_ = mbits[(b * 4 + g) >> 3] >> (((b * 4 + g) & 7) * 4);
          v.x = (nb_ & 1u) ? v.x * drop.inv_keep : 0.f;
          v.y = (nb_ & 2u) ? v.y * drop.inv_keep : 0.f;
          v.z = (nb_ & 4u) ? v.z * drop.inv_keep : 0.f;
          v.w = (nb_ & 8u) ? v.w * drop.inv_keep : 0.f;
        }
        if constexpr (EPI == EPI_RESIDUAL) {
          v.x += ax[b][g].x; v.y += ax[b][g].y; v.z += ax[b][g].z; v.w += ax[b][g].w;
        }
        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(c_u + 4 * ((size_t)(i * 32 + 8 * g) * ldc + j * 32) + c_lane));
      }
    }
    if constexpr (EPI == EPI_RELU_BITS) *mask_words = make_uint4(mbits[0], mbits[1], mbits[2], mbits[3]);
  } else {
  mma(s[kt & 1]);                             // the last K-tile; the epilogue touches no LDS, so no barrier follows
  ltrx::DropSpec dsp = drop;
  if (drop_step) dsp.seed ^= drop_step[0] * 0x9E3779B9u;
  unsigned int mbits[4] = {0u, 0u, 0u, 0u};
  if (act == 5) {
    const uint4 w = *mask_words;
    mbits[0] = w.x; mbits[1] = w.y; mbits[2] = w.z; mbits[3] = w.w;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wc * 64 + j * 32 + cq;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + col);
#pragma unroll
    for (int i = 0; i < RI; ++i) {
      f32x4 ax[4];
      if (act == 2 || act == 3) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = m0 + wr * (BM / 2) + i * 32 + 8 * g + 4 * half + q;
          ax[g] = (!TAIL || row < M) ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(aux + (size_t)row * ldaux + col))
                                     : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v = quad_transpose(acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3], b0, b1);   // row q, columns col..col+3
        const int row = m0 + wr * (BM / 2) + i * 32 + 8 * g + 4 * half + q;
        if (TAIL && row >= M) continue;
        v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
        if (act == 1 || act == 4) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        if (act == 5) {
          const unsigned int nb_ = mbits[((j * RI + i) * 4 + g) >> 3] >> ((((j * RI + i) * 4 + g) & 7) * 4);
          v.x = (nb_ & 1u) ? v.x * drop.inv_keep : 0.f;
          v.y = (nb_ & 2u) ? v.y * drop.inv_keep : 0.f;
          v.z = (nb_ & 4u) ? v.z * drop.inv_keep : 0.f;
          v.w = (nb_ & 8u) ? v.w * drop.inv_keep : 0.f;
        } else if (act == 2) {
          v.x = (ax[g].x > 0.f) ? v.x * drop.inv_keep : 0.f;
          v.y = (ax[g].y > 0.f) ? v.y * drop.inv_keep : 0.f;
          v.z = (ax[g].z > 0.f) ? v.z * drop.inv_keep : 0.f;
          v.w = (ax[g].w > 0.f) ? v.w * drop.inv_keep : 0.f;
        } else if (drop.thresh != 0u) {
          const uint64_t e = (uint64_t)row * (uint64_t)N + (uint64_t)col;
          v.x *= ltrx::drop_keep_scale(dsp, e);
          v.y *= ltrx::drop_keep_scale(dsp, e + 1);
          v.z *= ltrx::drop_keep_scale(dsp, e + 2);
          v.w *= ltrx::drop_keep_scale(dsp, e + 3);
        }
        if (act == 3) {      // SublayerConnection: x + dropout(sublayer(norm(x))) (transformer.py:98-106), the stream read here
          v.x += ax[g].x; v.y += ax[g].y; v.z += ax[g].z; v.w += ax[g].w;
        }
        if (act == 4)        // (after the dropout scaling: a dropped unit is 0 in the saved activation and passes no gradient)
          mbits[((j * RI + i) * 4 + g) >> 3] |= ((v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u))
                                                << ((((j * RI + i) * 4 + g) & 7) * 4);
        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(C + (size_t)row * ldc + col));
      }
    }
  }
  if (act == 4) *mask_words = make_uint4(mbits[0], mbits[1], mbits[2], mbits[3]);
  }
}

template <bool TAIL, int BM, int NT, bool BIMG, int EPI>
__global__ void __launch_bounds__(512) ltrx_gemm_nt256_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B,
                                                              int ldb, float* __restrict__ C, int ldc, int M, int N, int K,
                                                              const float* __restrict__ bias, int act,
                                                              const float* __restrict__ aux, int ldaux, int tiles_n,
                                                              ltrx::DropSpec drop, const uint32_t* __restrict__ drop_step) {
  nt256_body<TAIL, BM, NT, BIMG, EPI>(A, lda, B, ldb, C, ldc, M, N, K, bias, act, aux, ldaux, tiles_n, drop, drop_step);
}
// 64-row tiles, TWO workgroups per CU (2 x 80 KB of LDS, 128 registers per lane): for the shapes whose 128-row tiling is a single,
// not even full round of workgroups (N = 512 projections at 64 slates per GPU: 240 tiles) -- twice the workgroups, four waves per
// SIMD to hide the staging latency that two waves leave exposed
template <bool TAIL, int NT, bool BIMG, int EPI>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4)))
ltrx_gemm_nt64_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, float* __restrict__ C, int ldc, int M,
                      int N, int K, const float* __restrict__ bias, int act, const float* __restrict__ aux, int ldaux, int tiles_n,
                      ltrx::DropSpec drop, const uint32_t* __restrict__ drop_step) {
  nt256_body<TAIL, 64, NT, BIMG, EPI>(A, lda, B, ldb, C, ldc, M, N, K, bias, act, aux, ldaux, tiles_n, drop, drop_step);
}

// ------------------------------------------------------------------------------------------------------------------
// TN (weight gradient):  C[N',K'] = sum_m A[m][n'] * B[m][k'],  split over m into `splits` slabs
// ------------------------------------------------------------------------------------------------------------------
template <int NTERMS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 3))) ltrx_gemm_tn_kernel(const float* __restrict__ A, int lda,
                                                              const float* __restrict__ B, int ldb,
                                                              float* __restrict__ slabs, float* __restrict__ bias_slabs,
                                                              int M, int NP, int KP, int tiles_k, int m_per_split) {
  constexpr int BM = 128, BK = 32;
  __shared__ __attribute__((aligned(16))) Smem<NTERMS, BM, BK> s;
  const int tile = blockIdx.x, split = blockIdx.y;
  const int n0 = (tile / tiles_k) * BM, k0 = (tile % tiles_k) * BN;     // output tile: rows n', cols k'
  const int wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
  const int lane = threadIdx.x & 63;
  const int mbeg = split * m_per_split, mend = min(M, mbeg + m_per_split);

  // staging map: the K-tile is 32 contraction rows (m) x 128 columns.  A wave covers 8 m-rows (two groups of 4) per
  // pass... each lane owns ONE column (c = lane + 64*cc) and 4 consecutive m rows -> after the split one 8-byte LDS
  // write lands at [c][m..m+3] (k contiguous).  4 waves x 2 column halves x 4 m-groups: thread -> (mg, cc).
  //   thread t: column c = (t & 127), m-group g = t >> 7 (0..1); passes p = 0..3 cover m = 8p + 4g .. +3
  const int scol = threadIdx.x & 127, sg = threadIdx.x >> 7;
  float ra[4][4], rb[4][4];     // [pass][m within group]
  const bool want_bias = (bias_slabs != nullptr) && (tile % tiles_k == 0);   // column sums of A = the bias gradient
  float bsum = 0.f;

  const bool cola = n0 + scol < NP, colb = k0 + scol < KP;
  const float* pA = A + (cola ? n0 + scol : NP - 1);
  const float* pB = B + (colb ? k0 + scol : KP - 1);
  int mt_held = 0;                   // first contraction row of the tile currently held in ra/rb
  auto gload = [&](int mt) {         // raw loads (clamped rows); zero-select deferred to sstore
    mt_held = mt;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = min(mt + 8 * p + 4 * sg + e, mend - 1);
        ra[p][e] = pA[(size_t)m * lda];
        rb[p][e] = pB[(size_t)m * ldb];
      }
  };
  auto sstore = [&]() {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool okm = mt_held + 8 * p + 4 * sg + e < mend;
        ra[p][e] = (okm && cola) ? ra[p][e] : 0.f;
        rb[p][e] = (okm && colb) ? rb[p][e] : 0.f;
      }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int o = swz_off<BK>(scol, 8 * p + 4 * sg);
      bf16x4 h, l, l2;
      split4<NTERMS>(make_float4(ra[p][0], ra[p][1], ra[p][2], ra[p][3]), h, l, l2);
      *reinterpret_cast<bf16x4*>(&s.a[0][o]) = h;
      if (NTERMS >= 2) *reinterpret_cast<bf16x4*>(&s.a[NTERMS >= 2 ? 1 : 0][o]) = l;
      if (NTERMS == 3) *reinterpret_cast<bf16x4*>(&s.a[NTERMS - 1][o]) = l2;
      split4<NTERMS>(make_float4(rb[p][0], rb[p][1], rb[p][2], rb[p][3]), h, l, l2);
      *reinterpret_cast<bf16x4*>(&s.b[0][o]) = h;
      if (NTERMS >= 2) *reinterpret_cast<bf16x4*>(&s.b[NTERMS >= 2 ? 1 : 0][o]) = l;
      if (NTERMS == 3) *reinterpret_cast<bf16x4*>(&s.b[NTERMS - 1][o]) = l2;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (mbeg < mend) {
    gload(mbeg);
    for (int mt = mbeg; mt < mend; mt += BK) {
      __syncthreads();
      sstore();
      if (want_bias) {
#pragma unroll
        for (int p = 0; p < 4; ++p) bsum += (ra[p][0] + ra[p][1]) + (ra[p][2] + ra[p][3]);
      }
      __syncthreads();
      if (mt + BK < mend) gload(mt + BK);
      mma_tile<NTERMS, BM, BK>(s, wr, wc, acc);
    }
  }
  if (want_bias && n0 + scol < NP) bias_slabs[((size_t)split * 2 + sg) * NP + n0 + scol] = bsum;
  float* slab = slabs + (size_t)split * NP * KP;
  const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = k0 + wc * 64 + j * 32 + l31;
    if (col >= KP) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = n0 + wr * 64 + i * 32 + rowmap(r, half);
        if (row < NP) slab[(size_t)row * KP + col] = acc[i][j][r];
      }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// TN, large-tile variant (weight gradients of the big projections): 256 x 256 output tile, 8 waves (wave tile 128 x 64),
// K-step = 32 contraction rows, two LDS stages + LDS-only barrier, split-K slabs as above.
// Staging: 8 consecutive lanes fetch 128 contiguous bytes of one contraction row (16-byte loads, 4x fewer VMEM
// instructions than the dword loads above); a thread owns a 4 (m) x 4 (column) block of A and of B, i.e. after the split
// one 8-byte LDS write per column lands at [column][m .. m+3].  Rows r and r + 16 of an image swap bank halves (swz_t) so
// that the 16 lanes of a store group (8 column groups x 2 m-groups) hit 16 distinct bank pairs; the fragment reads stay
// conflict-free under that row permutation.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int swz_t(int row, int k) {
  const int c = (k >> 3) ^ ((row >> 2) & 3);
  return (row ^ ((row >> 4) & 1)) * 32 + c * 8 + (k & 7);
}

// Up to LTRX_TN_GROUP weight gradients over the SAME rows (the four projections of an encoder layer: dW = dY^T X with their own dY, X
// and output shape) in ONE launch: the tiles of all problems form one grid, so the chip is filled with total_tiles x splits workgroups
// instead of tiles x splits per problem -- 4x fewer splits, i.e. 4x fewer partial slabs to write and to reduce (round 4: the slabs were
// 550 MB per step whatever the batch; ltrx_gemm_tn_group).
#define LTRX_TN_GROUP 4
struct TnGroup {
  const float* A[LTRX_TN_GROUP];
  const float* B[LTRX_TN_GROUP];
  float* slabs[LTRX_TN_GROUP];
  float* bias_slabs[LTRX_TN_GROUP];
  int lda[LTRX_TN_GROUP], ldb[LTRX_TN_GROUP], NP[LTRX_TN_GROUP], KP[LTRX_TN_GROUP], tiles_k[LTRX_TN_GROUP];
  int kv[LTRX_TN_GROUP];             // columns of B that exist (= row length of the slabs and of C); KP = kv rounded up to the tile
  int tile_start[LTRX_TN_GROUP + 1];
  int nprob;
  // grouped launches (nprob > 1, at most 256 workgroups): workgroup id -> (tile, split), built by the host so that the tiles of one
  // (problem, split) -- which share their two operand row slabs -- sit on ONE XCD (workgroup w is dispatched to XCD w % 8)
  unsigned char map_tile[256];
  unsigned char map_split[256];
};

// A grouped launch with a SIDE JOB (ltrx_gemm_tn_group_ln): a one-dimensional grid of gemm_wgs + side workgroups, one per CU; ids
// below gemm_wgs take their (tile, split) from the map and run the GEMM path as it stands, the `side` ids above run the first-sublayer
// LayerNorm backward of the same encoder layer (ltrx::rowreg_ln_bwd_side) on CUs the plan would leave without a workgroup.
struct TnGroupLn {
  TnGroup g;
  ltrx::LnBwdJob ln;
  int gemm_wgs, side;
};
__device__ __forceinline__ const TnGroup& tn_group_of(const TnGroup& a) { return a; }
__device__ __forceinline__ const TnGroup& tn_group_of(const TnGroupLn& a) { return a.g; }

// SNV = 0: no side job (every launch of ltrx_gemm_tn and ltrx_gemm_tn_group).  SNV = 1..4: the side path for rows of 256 * SNV floats.
template <int NT, int SNV = 0>
__global__ void __launch_bounds__(512) ltrx_gemm_tn256_kernel(const std::conditional_t<SNV == 0, TnGroup, TnGroupLn> arg, int M,
                                                              int m_per_split) {
  constexpr int BK_ = 32;
  constexpr int L1 = NT - 1;
  typedef SmemNT<256, NT> SmemT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  if constexpr (SNV > 0) {
    if ((int)blockIdx.x >= arg.gemm_wgs) {                               // (workgroup-uniform)
      ltrx::rowreg_ln_bwd_side<SNV>(arg.ln, (int)blockIdx.x - arg.gemm_wgs, arg.side, reinterpret_cast<float*>(smem_raw));
      return;
    }
  }
  const TnGroup& grp = tn_group_of(arg);
  SmemT* s = reinterpret_cast<SmemT*>(smem_raw);
  // Workgroup -> (split, tile) in split-major order through the XCD remap: all tiles of one m-slab run on ONE XCD, so the dY
  // slab (shared by the tiles of a tile row) and the X slab (shared by the tiles of a tile column) are fetched from HBM once
  // and served to the other tiles by that XCD's L2.  PMC at the FFN shape (profiles/r01_pmc_tn256_xcd.md): L2 hit rate
  // 27 % -> 68 %, HBM-side reads 1.5 GB -> 0.63 GB per launch (= the algorithmic bytes); the duration does not change (the
  // kernel is bound by its staging path, not by HBM), the freed bandwidth is what the overlapped all-reduce needs.
  const int n_tiles = gridDim.x;
  int gtile, split;
  if (SNV > 0 || grp.nprob > 1) {                                       // (a launch with a side job always carries the map)
    const int w = blockIdx.x + n_tiles * blockIdx.y;
    gtile = grp.map_tile[w];
    split = grp.map_split[w];
  } else {
    const int wg = xcd_remap(blockIdx.x + n_tiles * blockIdx.y, n_tiles * gridDim.y);
    gtile = wg % n_tiles;
    split = wg / n_tiles;
  }
  int pi = 0;                                                          // (workgroup-uniform)
  while (pi + 1 < grp.nprob && gtile >= grp.tile_start[pi + 1]) ++pi;
  const float* __restrict__ A = grp.A[pi];
  const float* __restrict__ B = grp.B[pi];
  float* __restrict__ slabs = grp.slabs[pi];
  float* __restrict__ bias_slabs = grp.bias_slabs[pi];
  const int lda = grp.lda[pi], ldb = grp.ldb[pi], NP = grp.NP[pi], tiles_k = grp.tiles_k[pi], kv = grp.kv[pi];
  const int tile = gtile - grp.tile_start[pi];
  const int n0 = (tile / tiles_k) * 256, k0 = (tile % tiles_k) * 256;
  const int wave = threadIdx.x >> 6, wr = wave >> 2, wc = wave & 3;
  const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
  const int mbeg = split * m_per_split, mend = min(M, mbeg + m_per_split);
  const int cg = (threadIdx.x & 7) + 8 * wave, mg = (threadIdx.x >> 3) & 7;
  const float* PA = A + n0 + (size_t)(4 * mg) * lda + 4 * cg;
  const float* PB = B + k0 + (size_t)(4 * mg) * ldb + 4 * cg;
  float4 r[2][4];                    // [operand][m row]
  auto gload1 = [&](int mt, int g) {          // operand g of the m-slab starting at row mt
#pragma unroll
    for (int e = 0; e < 4; ++e)
      r[g][e] = g ? *reinterpret_cast<const float4*>(PB + (size_t)(mt + e) * ldb)
                  : *reinterpret_cast<const float4*>(PA + (size_t)(mt + e) * lda);
  };
  auto gload = [&](int mt) {
    gload1(mt, 0);
    gload1(mt, 1);
  };
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool want_bias = bias_slabs != nullptr && (tile % tiles_k) == 0;      // column sums of A = the bias gradient
  auto sstore1 = [&](SmemT& d, int g) {
    __bf16* img0 = g ? d.b[0] : d.a[0];
    __bf16* img1 = g ? d.b[L1] : d.a[L1];
    const float cx[4][4] = {{r[g][0].x, r[g][1].x, r[g][2].x, r[g][3].x}, {r[g][0].y, r[g][1].y, r[g][2].y, r[g][3].y},
                            {r[g][0].z, r[g][1].z, r[g][2].z, r[g][3].z}, {r[g][0].w, r[g][1].w, r[g][2].w, r[g][3].w}};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      bf16x4 h, l, l2;
      split4<2>(make_float4(cx[c][0], cx[c][1], cx[c][2], cx[c][3]), h, l, l2);
      const int o = swz_t(4 * cg + c, 4 * mg);
      *reinterpret_cast<bf16x4*>(&img0[o]) = h;
      if (NT == 2) *reinterpret_cast<bf16x4*>(&img1[o]) = l;
      if (g == 0 && want_bias) bsum[c] += (cx[c][0] + cx[c][1]) + (cx[c][2] + cx[c][3]);
    }
  };
  auto sstore = [&](SmemT& d) {
    sstore1(d, 0);
    sstore1(d, 1);
  };
  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
  auto mma1 = [&](const SmemT& t, int ks) {
    {
      bf16x8 af[NT][4], bfr[NT][2];
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
          bfr[tt][j] = *reinterpret_cast<const bf16x8*>(&t.b[tt][swz_t(wc * 64 + j * 32 + l31, ks * 16 + 8 * half)]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          af[tt][i] = *reinterpret_cast<const bf16x8*>(&t.a[tt][swz_t(wr * 128 + i * 32 + l31, ks * 16 + 8 * half)]);
      }
#define LTRX_MMA256(TA, TB)                                                                                       \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                     \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[TA][i], bfr[TB][j], acc[i][j], 0, 0, 0);
      if (NT == 2) {
        LTRX_MMA256(0, L1)
        LTRX_MMA256(L1, 0)
      }
      LTRX_MMA256(0, 0)
#undef LTRX_MMA256
    }
  };
  auto mma = [&](const SmemT& t) {
    mma1(t, 0);
    mma1(t, 1);
  };
  const int nk = (mend - mbeg) / BK_;            // M and m_per_split are multiples of 32 (host)
  if (nk > 0) {
    gload(mbeg);
    sstore(s[0]);
    if (nk > 1) gload(mbeg + BK_);
    __syncthreads();
    int kt = 0;
    for (; kt + 2 < nk; ++kt) {
      sstore(s[(kt + 1) & 1]);
      // pinned: left to itself the scheduler sinks these loads below the MFMA block (shorter live ranges), i.e. to a few
      // hundred cycles before the wait at the top of the next iteration, and every K-step eats the full memory latency
      __builtin_amdgcn_sched_barrier(0);
      gload(mbeg + (kt + 2) * BK_);
      __builtin_amdgcn_sched_barrier(0);
      mma(s[kt & 1]);
      lds_only_barrier();
    }
    for (; kt < nk; ++kt) {
      mma(s[kt & 1]);
      if (kt + 1 < nk) sstore(s[(kt + 1) & 1]);
      __syncthreads();
    }
  }
  if (want_bias) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v = bsum[c];
      v += __shfl_xor(v, 8);
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (mg == 0) bias_slabs[(size_t)split * NP + n0 + 4 * cg + c] = v;
    }
  }
  // (kv < the tile's column range: B's row stride covers the whole tile -- the host checks -- but only kv columns exist; the
  //  others were read from the padding and their products are dropped here)
  float* slab = slabs + (size_t)split * NP * kv;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = k0 + wc * 64 + j * 32 + l31;
    if (col < kv) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = n0 + wr * 128 + i * 32 + rowmap(q, half);
          slab[(size_t)row * kv + col] = acc[i][j][q];
        }
    }
  }
}

// Fixed-order sums of partial slabs, as device functions shared by the per-GEMM launch and the grouped launch (same order of
// additions in both: a result does not depend on which launch produced it).
// columns kind: out[c] = sum_s src[s * row_stride + c] for 64 columns per workgroup; its 4 waves take every 4th slab with 8 loads in
// flight, partials combined through LDS in a fixed order (one thread per column looping over all slabs was up to 128
// dependent-latency iterations in a handful of workgroups: the critical path of the launch)
__device__ __forceinline__ void reduce_cols(const float* __restrict__ src, int splits, size_t n, size_t row_stride,
                                            float* __restrict__ out, int lb, float (*sh)[64]) {
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const size_t c = (size_t)lb * 64 + cl;
  float a = 0.f;
  if (c < n) {
    int sidx = rg;
    for (; sidx + 28 < splits; sidx += 32) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(sidx + 4 * u) * row_stride + c];
#pragma unroll
      for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; sidx < splits; sidx += 4) a += src[(size_t)sidx * row_stride + c];
  }
  sh[rg][cl] = a;
  __syncthreads();
  if (rg == 0 && c < n) out[c] = (sh[0][cl] + sh[1][cl]) + (sh[2][cl] + sh[3][cl]);
}
// wide kind: C[i] = sum_s slabs[s * n + i], grid-stride over `nb` workgroups (this one is `lb`)
__device__ __forceinline__ void reduce_wide(const float* __restrict__ slabs, int splits, size_t n, float* __restrict__ C, int lb, int nb) {
  const size_t stride = (size_t)nb * blockDim.x;
  if ((n & 3) == 0 && (((uintptr_t)slabs | (uintptr_t)C) & 15) == 0) {
    // 16-byte accesses, eight slabs in flight per thread; the additions keep the slab order (same bits as the scalar loop)
    const size_t n4 = n >> 2;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(slabs);
    for (size_t i = (size_t)lb * blockDim.x + threadIdx.x; i < n4; i += stride) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      int sidx = 0;
      for (; sidx + 8 <= splits; sidx += 8) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(s4 + (size_t)(sidx + u) * n4 + i);
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v[u];
      }
      for (; sidx < splits; ++sidx) a += __builtin_nontemporal_load(s4 + (size_t)sidx * n4 + i);
      reinterpret_cast<f32x4*>(C)[i] = a;
    }
    return;
  }
  for (size_t i = (size_t)lb * blockDim.x + threadIdx.x; i < n; i += stride) {
    float a = 0.f;
    for (int sidx = 0; sidx < splits; ++sidx) a += slabs[(size_t)sidx * n + i];
    C[i] = a;
  }
}

// One launch serves the weight gradient (workgroups 0 .. main_blocks-1) and, when given, the bias gradient's column-sum slabs
// (the remaining workgroups).
__global__ void __launch_bounds__(256) ltrx_gemm_slab_reduce_kernel(const float* __restrict__ slabs, int splits,
                                                                    size_t n, float* __restrict__ C, int main_blocks,
                                                                    const float* __restrict__ slabs2, int splits2, size_t n2,
                                                                    float* __restrict__ C2) {
  __shared__ float sh[4][64];
  if ((int)blockIdx.x >= main_blocks) {
    reduce_cols(slabs2, splits2, n2, n2, C2, (int)blockIdx.x - main_blocks, sh);
    return;
  }
  reduce_wide(slabs, splits, n, C, (int)blockIdx.x, main_blocks);
}

static size_t slab_reduce_blocks(size_t n) {
  size_t blocks = ((n & 3) == 0 ? n / 4 : n) / 256 + 1;
  return blocks > 2048 ? 2048 : blocks;
}
static void launch_slab_reduce(const float* slabs, int splits, size_t n, float* C, const float* bslabs, int bsplits, size_t nb,
                               float* bias_out, hipStream_t s) {
  const size_t blocks = slab_reduce_blocks(n);
  const size_t bblocks = bias_out ? (nb + 63) / 64 : 0;
  hipLaunchKernelGGL(ltrx_gemm_slab_reduce_kernel, dim3((unsigned)(blocks + bblocks)), dim3(256), 0, s, slabs, splits, n, C,
                     (int)blocks, bslabs, bsplits, nb, bias_out);
}

// Several independent fixed-order reductions in ONE launch (ltrx_reduce_group): the partial slabs of a grouped weight-gradient GEMM,
// their bias column sums, and the parameter-gradient partials of the LayerNorm backward kernels of the same encoder layer -- eleven
// launches of 5-12 us per layer become one.  Entry e owns workgroups blk_start[e] .. blk_start[e+1]-1.
#define LTRX_REDUCE_GROUP 16
struct RedGroup {
  const float* src[LTRX_REDUCE_GROUP];
  float* dst[LTRX_REDUCE_GROUP];
  unsigned long long n[LTRX_REDUCE_GROUP];
  unsigned long long row_stride[LTRX_REDUCE_GROUP];
  int splits[LTRX_REDUCE_GROUP];
  int wide[LTRX_REDUCE_GROUP];
  int blk_start[LTRX_REDUCE_GROUP + 1];
  int nent;
};
__global__ void __launch_bounds__(256) ltrx_reduce_group_kernel(const RedGroup g) {
  __shared__ float sh[4][64];
  int e = 0;                                                            // (workgroup-uniform)
  while (e + 1 < g.nent && (int)blockIdx.x >= g.blk_start[e + 1]) ++e;
  const int lb = (int)blockIdx.x - g.blk_start[e];
  if (g.wide[e])
    reduce_wide(g.src[e], g.splits[e], (size_t)g.n[e], g.dst[e], lb, g.blk_start[e + 1] - g.blk_start[e]);
  else
    reduce_cols(g.src[e], g.splits[e], (size_t)g.n[e], (size_t)g.row_stride[e], g.dst[e], lb, sh);
}

// dst[i][c] = sum_{s < splits[i]} src[i][s * row_stride[i] + c]  for c < cols[i], i < n: every sum in a fixed order (deterministic;
// an entry gives the same bits as ltrx_gemm_tn's own reduction of the same slabs).  Entries with splits[i] <= 0 are skipped.
extern "C" int ltrx_reduce_group(int n, const float* const* src, const int* splits, const size_t* row_stride, const size_t* cols,
                                 float* const* dst, ltrx_stream_t stream) {
  if (n < 0 || n > LTRX_REDUCE_GROUP || (n > 0 && (!src || !splits || !row_stride || !cols || !dst))) return LTRX_EINVAL;
  RedGroup g = {};
  int ne = 0, blk = 0;
  for (int i = 0; i < n; ++i) {
    if (splits[i] <= 0 || cols[i] == 0) continue;
    if (!src[i] || !dst[i] || row_stride[i] < cols[i]) return LTRX_EINVAL;
    g.src[ne] = src[i];
    g.dst[ne] = dst[i];
    g.n[ne] = cols[i];
    g.row_stride[ne] = row_stride[i];
    g.splits[ne] = splits[i];
    g.wide[ne] = (row_stride[i] == cols[i] && cols[i] >= 16384) ? 1 : 0;
    g.blk_start[ne] = blk;
    blk += (int)(g.wide[ne] ? slab_reduce_blocks(cols[i]) : (cols[i] + 63) / 64);
    ++ne;
  }
  g.blk_start[ne] = blk;
  g.nent = ne;
  if (ne == 0) return LTRX_OK;
  hipLaunchKernelGGL(ltrx_reduce_group_kernel, dim3((unsigned)blk), dim3(256), 0, (hipStream_t)stream, g);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// pre-split operand image: every 4 consecutive floats of src become the 16 bytes {hi0..hi3, lo0..lo3} (bf16) of dst -- the same
// split4 the kernels apply while staging, so a GEMM fed from the image is bit-identical to one fed from the fp32 values
__global__ void __launch_bounds__(256) ltrx_split_image_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    bf16x4 h, l, l2;
    split4<2>(src[i], h, l, l2);
    float4 o;
    *reinterpret_cast<bf16x4*>(&o.x) = h;
    *reinterpret_cast<bf16x4*>(&o.z) = l;
    dst[i] = o;
  }
}

extern "C" int ltrx_split_image(const float* src, void* dst, size_t n, ltrx_stream_t stream) {
  if (!src || !dst || (n & 3) || (((uintptr_t)src | (uintptr_t)dst) & 15)) return LTRX_EINVAL;
  if (n == 0) return LTRX_OK;
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(ltrx_split_image_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), n / 4);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------
// `tile` argument of ltrx_gemm_nt / ltrx_gemm_tn (a per-call tuning argument, no process state).  ltrx_gemm_nt, and the code a plan
// segment carries: 0 = auto; 1 = 128x128x32 (4 waves), 2 = 128x128x64, 3 = 256x128x32 (8 waves), 4 = 256x128x64 (six- and one-product
// precision: 128x128x32 whatever the code); the 256-column (large-tile) kernel: 6 = 256x256x32, 7 = its 128x256x32 form, 8 = its 64x256x32
// form with two workgroups per CU (small batches); else as 1.  ltrx_gemm_tn: 0 = auto, 1 = never the 256x256 kernel, 9 = see tn_plan.
// (a PERSISTENT form of the 256x256x32 kernel -- one workgroup per CU walking its tiles, next tile's first K-steps prefetched
//  behind the epilogue -- was built and measured in round 3: bit-identical results, 0 ... -13 % in speed; tools/lab/gemm_persist.inc,
//  profiles/r03_gemm_persist_ab.md)

// one launch of ltrx_gemm_nt (the rows and pointers of one plan segment); every NT kernel has the one signature and launch statement
struct NtArgs {
  const float* A; int lda; const float* B; int ldb; float* C; int ldc; int M, N, K;
  const float* bias; int act; const float* aux; int ldaux; ltrx::DropSpec drop; const uint32_t* drop_step;
};
typedef void (*NtFn)(const float*, int, const float*, int, float*, int, int, int, int, const float*, int, const float*, int, int,
                     ltrx::DropSpec, const uint32_t*);
static int nt_launch(NtFn f, int tiles_m, int tiles_n, int threads, size_t lds, const NtArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(f, dim3(tiles_m * tiles_n), dim3(threads), lds, s, a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.M, a.N, a.K, a.bias, a.act,
                     a.aux, a.ldaux, tiles_n, a.drop, a.drop_step);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// The epilogue kind of a launch, from (act, bias, dropout): the straight-line kinds are the dropout-free epilogues of the default
// training step, in its form of the launch (exact row tiles, three products, B as a pre-split image).  With drop.thresh == 0 the
// generic epilogue never reads drop_step, so the kind does not depend on it.  Everything else is EPI_GENERIC -- same bits either way.
static int nt_epilogue_kind(int act, bool has_bias, bool drop_on, bool tail, bool plain, bool bimg) {
  if (drop_on || tail || plain || !bimg) return EPI_GENERIC;
  switch (act) {
    case 0: return has_bias ? EPI_BIAS : EPI_PLAIN;
    case 3: return has_bias ? EPI_RESIDUAL : EPI_GENERIC;
    case 4: return has_bias ? EPI_RELU_BITS : EPI_GENERIC;
    case 5: return has_bias ? EPI_GENERIC : EPI_MASK_READ;
    default: return EPI_GENERIC;
  }
}

// ---- the launch plan of ltrx_gemm_nt: every decision of a call, made once on the host before anything is launched ----
struct NtSeg {
  int m0, rows;                       // the rows of A / C / aux this launch covers
  int tile, nterms;                   // tile code 1-4, 6, 7, 8 (the `tile` table above); bf16 terms per operand (1, 2, 3)
  int tail, bimg, epi;                // 256-column kernel only: a partial last row tile; B read from its image; epilogue kind
};
struct NtPlan { int rc, nseg; NtSeg seg[2]; };       // LTRX_OK and 1 segment (2 in the row-split window), or the refusal and none

// the automatic tile where the 256-column kernel applies: one workgroup per CU, a grid that fills 3/4 .. 1 round, or at least ~1.4
// rounds (measured, tools/gemm_variants.py: 240 tiles 53 vs 77 us, 360 tiles parity, 120 tiles parity, 480 tiles 102 vs 132 us)
static int nt_auto_tile(int rows, int N) {
  const size_t nn = (size_t)(N / 256), t = (size_t)((rows + 255) / 256) * nn, t128 = (size_t)((rows + 127) / 128) * nn;
  if (t >= 360 || (t >= 168 && t <= 256)) return 6;
  if (t >= 136 && t < 168 && t128 > 256) return 6;    // one partial round still beats two rounds of smaller tiles
  if (t128 >= 176 && t128 <= 256) return 7;          // 128-row tiles when they make exactly one well-filled round
  // small batches (32 slates x 240 per GPU: 120 tiles of 128 rows): 64-row tiles, two workgroups per CU -- 55 vs 77 (128-row) vs
  // 108 us (small-tile kernel) at M 7680 x N 512 x K 2048 (tools/gemm_nt64_ab.py); same bits as every other tile
  const size_t t64 = (size_t)((rows + 63) / 64) * nn;
  if (t128 < 176 && t64 >= 176 && t64 <= 512) return 8;
  return 1;
}

// bytes of the one-bit ReLU mask of an [M, N] activation (acts 4 / 5 of ltrx_gemm_nt), 0 where that form does not apply: the mask is
// kept in the 256 x 256 tile kernel's (tile, thread) order, so both launches must take that kernel whatever their K, dropout and
// epilogue -- N % 256 == 0, K % 32 == 0 (K of the launch asked about: forward and input-gradient launch of one mask may differ -- ask for
// both) and a tile count with this property: wherever the function is non-zero, nt_plan for act 4 and for act 5, dropout off or on, is ONE
// segment on the 256-row tile (tests/test_gemm_plan_cpu.py; asserted by ltrx_gemm_nt).  Callers use acts 1 / 2 where it returns 0.
extern "C" size_t ltrx_gemm_nt_relu_bits_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || (N % 256) || (K % 32)) return 0;
  const size_t t = (size_t)((M + 255) / 256) * (N / 256);
  if (!(t >= 380 || (t >= 168 && t <= 256))) return 0;
  return t * 512 * 16;
}

// Pure (no HIP call, no pointer): the caller has checked the pointers and M, N, K > 0, act 0..5, tile >= 0, and states vec_epi (16-byte
// accesses to C, bias and aux) and bimg_ok (a usable image of B).  prec: 0 = three products, 1 = six (strict), 2 = one (plain bf16).
static NtPlan nt_plan(int M, int N, int K, int lda, int ldb, int ldc, int act, bool has_bias, bool drop_on, int prec, int tile,
                      bool vec_epi, bool bimg_ok) {
  NtPlan pl = {LTRX_EUNSUPPORTED, 0, {}};
  const bool plain = prec == 2, strict = prec != 0 && !plain;
  // the one-bit mask lives in the large-tile kernel's own (tile, thread) order: only where it runs
  if ((act == 4 || act == 5) && (tile != 0 || strict || !vec_epi || ltrx_gemm_nt_relu_bits_bytes(M, N, K) == 0)) return pl;
  if ((K & 3) || (lda & 3) || (ldb & 3) || lda < K || ldb < K || ldc < N) return pl;
  const bool large_ok = !strict && (N % 256) == 0 && (K % 32) == 0 && vec_epi;
  if (tile >= 6 && tile <= 8 && !large_ok) return pl;
  auto segment = [&](int m0, int rows, int v) {
    const bool large = v >= 6 && v <= 8, tail = large && rows % (v == 6 ? 256 : (v == 7 ? 128 : 64)) != 0;
    const int nterms = strict ? 3 : (plain ? 1 : 2);
    pl.seg[pl.nseg++] = {m0, rows, (large || (nterms == 2 && v >= 2 && v <= 4)) ? v : 1, nterms, tail, large && bimg_ok,
                         large ? nt_epilogue_kind(act, has_bias, drop_on, tail, plain, bimg_ok) : EPI_GENERIC};
  };
  const int nn = N / 256, tiles_m = (M + 255) / 256;
  if (tile != 0 || !large_ok) {
    segment(0, M, tile);
  } else if (const size_t t = (size_t)tiles_m * nn; t > 256 && t < 380 && (!drop_on || act == 2) && nn <= 256) {
    // between one and ~1.5 rounds of 256-row tiles: a second round for a handful of tiles costs as much as the first
    // (M 33000 x N 512: 95 us against 54 us for M 30720).  One exact round of large tiles first, the remaining rows as
    // their own (smaller) problem with its own automatic tile: 5-25 % faster over that range (tools/gemm_split_probe.py).
    // Only without dropout generated in the epilogue -- its hash is indexed by the row of THIS launch.
    const int m1 = (256 / nn) * 256;
    segment(0, m1, nt_auto_tile(m1, N));
    segment(m1, M - m1, nt_auto_tile(M - m1, N));
  } else {
    segment(0, M, nt_auto_tile(M, N));
  }
  pl.rc = LTRX_OK;
  return pl;
}

template <int BM, bool TAIL, int NT, bool BIMG, int EPI>
static NtFn nt_large_fn() {
  if constexpr (BM == 64) return ltrx_gemm_nt64_kernel<TAIL, NT, BIMG, EPI>;
  else return ltrx_gemm_nt256_kernel<TAIL, BM, NT, BIMG, EPI>;
}
// nullptr: no such instantiation (the mask kinds exist for the 256-row tile only -- the mask is kept in its (tile, thread) order)
template <int BM>
static NtFn nt_large_kernel(bool tail, int nt, bool bimg, int epi) {
  switch (epi) {
    case EPI_GENERIC:
#define LTRX_NT_GENERIC(TAIL_) \
  (nt == 2 ? (bimg ? nt_large_fn<BM, TAIL_, 2, true, EPI_GENERIC>() : nt_large_fn<BM, TAIL_, 2, false, EPI_GENERIC>()) \
           : (bimg ? nt_large_fn<BM, TAIL_, 1, true, EPI_GENERIC>() : nt_large_fn<BM, TAIL_, 1, false, EPI_GENERIC>()))
      return tail ? LTRX_NT_GENERIC(true) : LTRX_NT_GENERIC(false);
#undef LTRX_NT_GENERIC
    case EPI_PLAIN: return nt_large_fn<BM, false, 2, true, EPI_PLAIN>();
    case EPI_BIAS: return nt_large_fn<BM, false, 2, true, EPI_BIAS>();
    case EPI_RESIDUAL: return nt_large_fn<BM, false, 2, true, EPI_RESIDUAL>();
    case EPI_RELU_BITS:
      if constexpr (BM == 256) return nt_large_fn<BM, false, 2, true, EPI_RELU_BITS>();
      return nullptr;
    case EPI_MASK_READ:
      if constexpr (BM == 256) return nt_large_fn<BM, false, 2, true, EPI_MASK_READ>();
      return nullptr;
  }
  return nullptr;
}

template <int BM>
static int launch_nt_large(const NtArgs& a, const NtSeg& sg, hipStream_t s) {
  static std::atomic<uint64_t> attr_done{0};
  const int arc = ltrx_once_per_device(attr_done, [&]() {
    for (int epi = 0; epi < EPI_KINDS; ++epi)
      for (int c = 0; c < (epi == EPI_GENERIC ? 8 : 1); ++c) {
        const int nt = epi == EPI_GENERIC ? 1 + (c & 1) : 2;
        const NtFn f = nt_large_kernel<BM>(epi == EPI_GENERIC && (c & 4), nt, epi != EPI_GENERIC || (c & 2), epi);
        const size_t bytes = 2 * (nt == 2 ? sizeof(SmemNT<BM, 2>) : sizeof(SmemNT<BM, 1>));
        if (f && hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return LTRX_EHIP;
      }
    return LTRX_OK;
  });
  if (arc != LTRX_OK) return arc;
  const NtFn f = nt_large_kernel<BM>(sg.tail != 0, sg.nterms, sg.bimg != 0, sg.epi);
  if (!f) return LTRX_EUNSUPPORTED;
  const size_t lds = 2 * (sg.nterms == 2 ? sizeof(SmemNT<BM, 2>) : sizeof(SmemNT<BM, 1>));
  return nt_launch(f, (a.M + BM - 1) / BM, a.N / 256, 512, lds, a, s);
}

static int launch_nt_small(const NtArgs& a, const NtSeg& sg, hipStream_t s) {
  const int bm = sg.tile >= 3 ? 256 : 128;            // (codes 3, 4: 256-row tiles, 8 waves; only with two terms, see nt_plan)
  const NtFn f = sg.nterms == 3   ? ltrx_gemm_nt_kernel<3, 128, 32>
                 : sg.nterms == 1 ? ltrx_gemm_nt_kernel<1, 128, 32>
                 : sg.tile == 2   ? ltrx_gemm_nt_kernel<2, 128, 64>
                 : sg.tile == 3   ? ltrx_gemm_nt_kernel<2, 256, 32>
                 : sg.tile == 4   ? ltrx_gemm_nt_kernel<2, 256, 64>
                                  : ltrx_gemm_nt_kernel<2, 128, 32>;
  return nt_launch(f, (a.M + bm - 1) / bm, (a.N + BN - 1) / BN, 2 * bm, 0, a, s);
}

extern "C" int ltrx_gemm_nt(const float* A, int lda, const float* B, int ldb, const void* B_image, float* C, int ldc, int M, int N, int K,
                            const float* bias, int act, const float* aux, int ldaux, float drop_p, uint32_t drop_seed,
                            const uint32_t* drop_step, int strict, int tile, ltrx_stream_t stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || act < 0 || act > 5 || tile < 0) return LTRX_EINVAL;
  if (!(drop_p >= 0.f) || drop_p >= 1.f) return LTRX_EINVAL;
  const ltrx::DropSpec drop = ltrx_make_drop(drop_p, drop_seed);
  if ((act == 2 || act == 3) && (!aux || ldaux < N)) return LTRX_EINVAL;
  const bool mask = act == 4 || act == 5;             // the one-bit mask: a 16-byte aligned buffer of its own, no row stride
  if (mask && (!aux || ((uintptr_t)aux & 15))) return LTRX_EUNSUPPORTED;
  if (mask) ldaux = 0;
  // the alignment facts of the plan: 16-byte epilogue accesses; the pre-split image of B (same addressing as B, 16-byte aligned)
  const bool vec_epi = (ldc & 3) == 0 && ((uintptr_t)C & 15) == 0 && (!bias || ((uintptr_t)bias & 15) == 0) &&
                       (!aux || ((ldaux & 3) == 0 && ((uintptr_t)aux & 15) == 0));
  const bool bimg = B_image != nullptr && (((uintptr_t)B_image) & 15) == 0;
  const NtPlan pl = nt_plan(M, N, K, lda, ldb, ldc, act, bias != nullptr, drop.thresh != 0u, strict, tile, vec_epi, bimg);
  if (pl.rc != LTRX_OK) return pl.rc;
  // (the mask's (tile, thread) order is the 256-row kernel's: refuse any other tiling if the predicate and the plan ever disagree)
  if (mask && !(pl.nseg == 1 && pl.seg[0].tile == 6)) return LTRX_EUNSUPPORTED;
  for (int i = 0; i < pl.nseg; ++i) {
    const NtSeg& sg = pl.seg[i];
    const NtArgs a = {A + (size_t)sg.m0 * lda, lda, sg.bimg ? reinterpret_cast<const float*>(B_image) : B, ldb, C + (size_t)sg.m0 * ldc, ldc,
                      sg.rows, N, K, bias, act, aux ? aux + (size_t)sg.m0 * ldaux : nullptr, ldaux, drop, drop_step};
    const int rc = sg.tile == 6   ? launch_nt_large<256>(a, sg, (hipStream_t)stream)
                   : sg.tile == 7 ? launch_nt_large<128>(a, sg, (hipStream_t)stream)
                   : sg.tile == 8 ? launch_nt_large<64>(a, sg, (hipStream_t)stream)
                                  : launch_nt_small(a, sg, (hipStream_t)stream);
    if (rc != LTRX_OK) return rc;
  }
  return LTRX_OK;
}

static int tn_splits(int M, int tiles) {
  int want = (512 + tiles - 1) / tiles;            // aim for >= 512 workgroups
  int maxs = (M + 4 * 32 - 1) / (4 * 32);          // at least 4 K-tiles per split
  if (want > maxs) want = maxs;
  if (want > 64) want = 64;
  return want < 1 ? 1 : want;
}

// large-tile wgrad kernel: exact multiples only
static bool tn256_ok(int M, int NP, int KP) { return (NP % 256) == 0 && (KP % 256) == 0 && (M % 32) == 0 && M >= 2048; }
static int tn256_tiles(int NP, int KP) { return (NP / 256) * (KP / 256); }
// THE row-split rule of the large-tile kernel, single problem or group: one workgroup per CU and ONE round (never more than 256
// workgroups over all `tiles`), at least 4 K-steps (128 rows) per split, at least one split
static int tn256_max_splits(int tiles, int M) {
  int sp = tiles > 0 ? 256 / tiles : 1;
  if (sp > M / 128) sp = M / 128;
  return sp < 1 ? 1 : sp;
}
// ... and the split it becomes: rows per split in whole 32-row K-steps, then only as many splits as have rows
static void tn256_split(int tiles, int M, int* splits, int* mps) {
  const int sp = tn256_max_splits(tiles, M);
  *mps = ((M + sp - 1) / sp + 31) / 32 * 32;
  *splits = (M + *mps - 1) / *mps;
}
// THE slab layout of a grouped launch: problem (NP, kv) at `s` splits takes s weight slabs [NP, kv] (w floats), then s bias rows [NP]
// (bias floats) padded to 4 floats (bias_pad): the pointer walk, the exact need and the sizing bound read it
struct TnSlab { size_t w, bias, bias_pad; };
static TnSlab tn_slab_floats(int s, int NP, int kv) {
  const size_t b = (size_t)s * NP;
  return {b * kv, b, (b + 3) & ~(size_t)3};
}

// ---- the launch plan of ltrx_gemm_tn (pure: no HIP call, no pointer) ----
struct TnPlan {
  bool large;                         // the 256 x 256 tile kernel (else the 128 x 128 one)
  int kv;                             // columns of B that exist (the large tile computes kv rounded up to 256 of them)
  int tiles, splits, mps;             // grid (tiles, splits); rows per split
  size_t bias_off;                    // float offset of the bias slabs in the workspace ...
  int bias_rows;                      // ... and their row count (the 128 x 128 kernel writes two per split)
};
static TnPlan tn_plan(int M, int NP, int KP, int lda, int ldb, int precision, int tile) {
  TnPlan pl = {};
  pl.kv = KP;
  // the large tile also serves a B whose column count is not a multiple of 256 when its ROW STRIDE covers the last tile (the
  // engine pads the input features to 256 floats per row): the surplus columns are computed from the padding and dropped
  // (opt-in, tile = 9: the kernel reads B[m][KP .. KPr) -- the caller states that every row, the last one included, is readable there)
  const int KPr = (KP + 255) / 256 * 256;
  if (tile == 9 && (KPr == KP || ldb < KPr)) tile = 0;
  pl.large = (precision == 0 || precision == 2) && tile != 1 && (KPr == KP || tile == 9) && tn256_ok(M, NP, KPr) && ldb >= KPr &&
             (lda & 3) == 0 && (ldb & 3) == 0;
  if (pl.large) {
    pl.tiles = tn256_tiles(NP, KPr);
    tn256_split(pl.tiles, M, &pl.splits, &pl.mps);
    pl.bias_off = ((size_t)pl.splits * NP * KP + 3) & ~(size_t)3;
    pl.bias_rows = pl.splits;
  } else {
    pl.tiles = ((NP + 127) / 128) * ((KP + BN - 1) / BN);
    pl.splits = tn_splits(M, pl.tiles);
    pl.mps = ((M + pl.splits - 1) / pl.splits + 31) / 32 * 32;
    pl.bias_off = (size_t)pl.splits * NP * KP;
    pl.bias_rows = 2 * pl.splits;
  }
  return pl;
}

// splits ltrx_gemm_tn will use for (M, NP, KP), dense operands, tile 0 (exported for the sizing test: the workspace must cover every
// row count <= the M it was sized for, because variable-length batches call ltrx_gemm_tn with a different M every step)
extern "C" int ltrx_gemm_tn_splits(int M, int NP, int KP) {
  if (M <= 0 || NP <= 0 || KP <= 0) return 0;
  return tn_plan(M, NP, KP, NP, KP, 0, 0).splits;
}

// Upper bound over ALL row counts m <= M (not only M itself): the small-tile plan is monotone in m (tn_splits), the
// large-tile plan never uses more than tn256_max_splits but is not monotone (m is rounded to 32-row
// slabs and the kernel switches on at m >= 2048, m % 32 == 0), so its bound is taken whenever the shape could select it.
extern "C" size_t ltrx_gemm_tn_workspace_bytes(int M, int NP, int KP) {
  if (M <= 0 || NP <= 0 || KP <= 0) return 0;
  const int tiles = ((NP + 127) / 128) * ((KP + BN - 1) / BN);
  size_t sp = (size_t)tn_splits(M, tiles);
  if ((NP % 256) == 0 && M >= 2048) {                 // (KP % 256 != 0: the large tile over a padded B, when ldb allows it)
    const size_t s2 = (size_t)tn256_max_splits(tn256_tiles(NP, (KP + 255) / 256 * 256), M);
    if (s2 > sp) sp = s2;
  }
  return (sp * NP * KP + 2 * sp * NP) * sizeof(float);
}

// problem p of a large-tile launch, set in the order p = 0, 1, ...: the one place that fills the kernel's table (kv: B's real columns)
static void tn_group_set(TnGroup& g, int p, const float* A, int lda, const float* B, int ldb, int NP, int kv, float* slabs,
                         float* bias_slabs) {
  g.A[p] = A;
  g.B[p] = B;
  g.lda[p] = lda;
  g.ldb[p] = ldb;
  g.NP[p] = NP;
  g.kv[p] = kv;
  g.KP[p] = (kv + 255) / 256 * 256;
  g.tiles_k[p] = g.KP[p] / 256;
  g.tile_start[p + 1] = g.tile_start[p] + tn256_tiles(NP, g.KP[p]);      // (tile_start[0] = 0: the table starts zeroed)
  g.slabs[p] = slabs;
  g.bias_slabs[p] = bias_slabs;
  g.nprob = p + 1;
}

// the large-tile kernel's two staging buffers exceed the default dynamic-LDS allowance (ltrx_gemm_tn and ltrx_gemm_tn_group launch it)
static int tn256_allow_lds() {
  static std::atomic<uint64_t> attr_done{0};
  return ltrx_allow_dynamic_lds(attr_done, {{ltrx_gemm_tn256_kernel<2>, 2 * sizeof(SmemNT<256, 2>)}, {ltrx_gemm_tn256_kernel<1>, 2 * sizeof(SmemNT<256, 1>)},
                                           {ltrx_gemm_tn256_kernel<2, 1>, 2 * sizeof(SmemNT<256, 2>)}, {ltrx_gemm_tn256_kernel<2, 2>, 2 * sizeof(SmemNT<256, 2>)},
                                           {ltrx_gemm_tn256_kernel<2, 3>, 2 * sizeof(SmemNT<256, 2>)}, {ltrx_gemm_tn256_kernel<2, 4>, 2 * sizeof(SmemNT<256, 2>)}});
}
static void tn256_launch(bool plain, dim3 grid, const TnGroup& g, int M, int mps, hipStream_t s) {
  const auto k = plain ? ltrx_gemm_tn256_kernel<1> : ltrx_gemm_tn256_kernel<2>;
  hipLaunchKernelGGL(k, grid, dim3(512), 2 * (plain ? sizeof(SmemNT<256, 1>) : sizeof(SmemNT<256, 2>)), s, g, M, mps);
}

extern "C" int ltrx_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, float* bias_out, int M, int NP,
                            int KP, int strict, int tile, void* ws, ltrx_stream_t stream) {
  if (!A || !B || !C || !ws || M <= 0 || NP <= 0 || KP <= 0 || tile < 0) return LTRX_EINVAL;
  if (lda < NP || ldb < KP) return LTRX_EUNSUPPORTED;
  const bool plain = strict == 2;                     // precision code as in ltrx_gemm_nt
  const TnPlan pl = tn_plan(M, NP, KP, lda, ldb, strict, tile);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(pl.tiles, pl.splits);
  float* bslabs = bias_out ? (float*)ws + pl.bias_off : nullptr;
  if (pl.large) {
    const int arc = tn256_allow_lds();
    if (arc != LTRX_OK) return arc;
    TnGroup g = {};
    tn_group_set(g, 0, A, lda, B, ldb, NP, KP, (float*)ws, bslabs);
    tn256_launch(plain, grid, g, M, pl.mps, s);
  } else {
    const auto k = plain ? ltrx_gemm_tn_kernel<1> : (strict ? ltrx_gemm_tn_kernel<3> : ltrx_gemm_tn_kernel<2>);
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, A, lda, B, ldb, (float*)ws, bslabs, M, NP, KP, (KP + BN - 1) / BN, pl.mps);
  }
  LTRX_LAUNCH_CHECK();
  launch_slab_reduce((const float*)ws, pl.splits, (size_t)NP * KP, C, bslabs, pl.bias_rows, (size_t)NP, bias_out, s);
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// ---- grouped weight gradients (see TnGroup) ----
// tiles of the group when the grouped kernel can run it (every problem on the large tile, one round of at most 256 tiles), else 0
static int tn_group_tiles(int nprob, int M, const int* NP, const int* KP, const int* lda, const int* ldb, int strict) {
  if (nprob < 1 || nprob > LTRX_TN_GROUP || strict == 1) return 0;
  int t = 0;
  for (int p = 0; p < nprob; ++p) {
    if (!tn256_ok(M, NP[p], KP[p]) || (lda && ((lda[p] & 3) || lda[p] < NP[p])) || (ldb && ((ldb[p] & 3) || ldb[p] < KP[p]))) return 0;
    t += tn256_tiles(NP[p], KP[p]);
  }
  return t <= 256 ? t : 0;
}

// (problem, split) groups -> XCDs: fills g.map_tile / g.map_split for the total * splits (<= 256) workgroups of a grouped launch
static void tn_group_map(TnGroup& g, int total, int splits) {
  const int nprob = g.nprob;
  // (problem, split) groups, largest first, into the 8 XCDs (first fit, capacity = an even share of the grid; a group that fits
  // nowhere whole is cut); XCD x owns the workgroup ids x, x + 8, x + 16, ...
  const int nwg = total * splits;                        // <= 256 (tn256_split)
  const int cap = (nwg + 7) / 8;
  int fill[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int order[LTRX_TN_GROUP];
  for (int p = 0; p < nprob; ++p) order[p] = p;
  for (int a = 0; a < nprob; ++a)
    for (int b = a + 1; b < nprob; ++b)
      if (g.tile_start[order[b] + 1] - g.tile_start[order[b]] > g.tile_start[order[a] + 1] - g.tile_start[order[a]]) {
        const int t_ = order[a];
        order[a] = order[b];
        order[b] = t_;
      }
  auto slot_count = [&](int x) { return (nwg - x + 7) / 8; };      // ids x, x+8, ... < nwg
  for (int oi = 0; oi < nprob; ++oi) {
    const int p = order[oi], nt = g.tile_start[p + 1] - g.tile_start[p];
    for (int sp_ = 0; sp_ < splits; ++sp_) {
      int left = nt, next = 0;
      while (left > 0) {
        int best = -1;
        for (int x = 0; x < 8; ++x)                      // an XCD that takes the rest whole, else the emptiest one
          if (fill[x] + left <= (cap < slot_count(x) ? cap : slot_count(x))) {
            best = x;
            break;
          }
        if (best < 0) {
          int room = -1;
          for (int x = 0; x < 8; ++x) {
            const int r_ = slot_count(x) - fill[x];
            if (r_ > room) {
              room = r_;
              best = x;
            }
          }
        }
        int take = slot_count(best) - fill[best];
        if (take > left) take = left;
        for (int q = 0; q < take; ++q) {
          const int w = best + 8 * (fill[best] + q);
          g.map_tile[w] = (unsigned char)(g.tile_start[p] + next + q);
          g.map_split[w] = (unsigned char)sp_;
        }
        fill[best] += take;
        next += take;
        left -= take;
      }
    }
  }
  }

// bytes for ltrx_gemm_tn_group: an upper bound over every row count m <= M (variable-length batches): per problem one split more than
// tn256_max_splits allows at any m, and never less than the single-problem calls need (the fall-back of shapes that do not qualify)
extern "C" size_t ltrx_gemm_tn_group_workspace_bytes(int nprob, int M, const int* NP, const int* KP) {
  if (nprob < 1 || nprob > LTRX_TN_GROUP || M <= 0 || !NP || !KP) return 0;
  size_t single = 0;
  int t = 0;
  for (int p = 0; p < nprob; ++p) {
    const size_t b = ltrx_gemm_tn_workspace_bytes(M, NP[p], KP[p]);
    if (b > single) single = b;
    t += ((NP[p] + 255) / 256) * ((KP[p] + 255) / 256);
  }
  const int sp = tn256_max_splits(t, INT_MAX) + 1;   // (no row clamp: the bound callers size by has never depended on M)
  size_t grouped = 0;
  for (int p = 0; p < nprob; ++p) {
    const TnSlab sl = tn_slab_floats(sp, NP[p], KP[p]);
    grouped += (sl.w + sl.bias + 4) * sizeof(float);  // (+ 4 floats where the layout pads by at most 3: the values callers size by)
  }
  return grouped > single ? grouped : single;
}

// ---- the side job of a grouped launch (TnGroupLn): host plan ----
// Two measured figures decide whether the LayerNorm backward rides in the launch (profiles/NOTES.md, "LayerNorm backward in the
// weight-gradient launch's idle CUs"; tables in profiles/ln_in_wgrad_kernel_stats.md):
//   R = 49 000 bytes per microsecond streamed by ONE side workgroup (8 waves, two rows in flight each): 503 MB of dy, x, residual
//       gradient and dx at 61440 x 512 in 642 us on 16 side workgroups, 1221 us on 8 (51 500 each), next to a one-tile GEMM part;
//   2.5 us per K-step (32 rows) of a three-product GEMM workgroup: the grouped launch without a side job runs 1030 us at 384 K-steps
//       per workgroup (256 slates) and 246 us at 96 (64 slates), i.e. 2.68 and 2.56; earlier traces had 922-972 us (2.40-2.53).
// T, the duration of the GEMM part, is K-steps per workgroup x that figure.  The side job is taken only when
// bytes / (side x R) <= 0.8 T: the margin keeps it off the critical path on a slower device (the bench layer: 642 <= 768 us).
#ifndef LTRX_TN_SIDE_BYTES_PER_US
#define LTRX_TN_SIDE_BYTES_PER_US 49000.0
#endif
#ifndef LTRX_TN_KSTEP_US
#define LTRX_TN_KSTEP_US 2.5
#endif
struct TnSidePlan {
  bool grouped;                       // the grouped kernel runs (else: one ltrx_gemm_tn per problem)
  int total, splits, mps;             // tiles of the group, row splits, rows per split (tn256_split)
  size_t need;                        // bytes of workspace the grouped launch writes (tn_slab_floats), exactly
  int gemm_wgs, side;                 // workgroups of the GEMM path; side workgroups (0: no side job)
  LnBwdShape sh;                      // the stand-alone LayerNorm backward launch whose blocks the side workgroups play
};
// side_wgs 0: the rule above; > 0: that many side workgroups (tests), clamped to the CUs the GEMM path leaves free
static TnSidePlan tn_group_side_plan(int nprob, int M, const int* NP, const int* KP, const int* lda, const int* ldb, int strict,
                                     size_t ws_bytes, int rows, int D, bool vec, bool has_dres, int side_wgs) {
  TnSidePlan pl = {};
  pl.sh = ltrx_ln_bwd_shape(rows, D);
  pl.total = tn_group_tiles(nprob, M, NP, KP, lda, ldb, strict);
  pl.grouped = pl.total > 0;
  if (!pl.grouped) return pl;
  tn256_split(pl.total, M, &pl.splits, &pl.mps);
  for (int p = 0; p < nprob; ++p) {
    const TnSlab sl = tn_slab_floats(pl.splits, NP[p], KP[p]);
    pl.need += (sl.w + sl.bias_pad) * sizeof(float);
  }
  if (pl.need > ws_bytes) {
    pl.grouped = false;
    return pl;
  }
  pl.gemm_wgs = pl.total * pl.splits;
  const int free_cus = 256 - pl.gemm_wgs;
  // (the side path exists in the three-product kernel only; its spill rows must fit the kernel's LDS)
  if (free_cus <= 0 || strict != 0 || !vec || rows <= 0 || (pl.sh.wpb != 4 && pl.sh.wpb != 16) ||
      ltrx::rowreg_ln_side_lds_floats(D, pl.sh.wpb) * sizeof(float) > 2 * sizeof(SmemNT<256, 2>))
    return pl;
  if (side_wgs > 0) {
    pl.side = side_wgs < free_cus ? side_wgs : free_cus;
    return pl;
  }
  const double bytes = (double)rows * D * sizeof(float) * (has_dres ? 4.0 : 3.0);
  const double t_gemm = (double)(pl.mps / 32) * LTRX_TN_KSTEP_US;
  if (bytes / ((double)free_cus * LTRX_TN_SIDE_BYTES_PER_US) <= 0.8 * t_gemm) pl.side = free_cus;
  return pl;
}

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// ltrx_gemm_tn_group, and with `ln` the same launch carrying the LayerNorm backward as its side job (pl.side > 0)
static int tn_group_run(int nprob, const float* const* A, const int* lda, const float* const* B, const int* ldb, float* const* C,
                        float* const* bias_out, int M, const int* NP, const int* KP, int strict, void* ws, const float** slabs_out,
                        const float** bias_slabs_out, int* splits_out, const TnSidePlan& pl, const ltrx::LnBwdJob* ln, int ln_D, hipStream_t s) {
  const int total = pl.total, splits = pl.splits, mps = pl.mps;
  const int arc = tn256_allow_lds();
  if (arc != LTRX_OK) return arc;
  TnGroupLn gl = {};
  TnGroup& g = gl.g;
  float* w = (float*)ws;
  for (int p = 0; p < nprob; ++p) {
    const TnSlab sl = tn_slab_floats(splits, NP[p], KP[p]);
    tn_group_set(g, p, A[p], lda[p], B[p], ldb[p], NP[p], KP[p], w, bias_out[p] ? w + sl.w : nullptr);
    w += sl.w + sl.bias_pad;
  }
  tn_group_map(g, total, splits);
  if (ln && pl.side > 0) {
    gl.ln = *ln;
    gl.gemm_wgs = pl.gemm_wgs;
    gl.side = pl.side;
    ltrx_rowreg_dispatch(ln_D, [&](auto nv) {
      hipLaunchKernelGGL((ltrx_gemm_tn256_kernel<2, decltype(nv)::value>), dim3(pl.gemm_wgs + pl.side), dim3(512), 2 * sizeof(SmemNT<256, 2>),
                         s, gl, M, mps);
    });
  } else {
    tn256_launch(strict == 2, dim3(total, splits), g, M, mps, s);
  }
  LTRX_LAUNCH_CHECK();
  if (slabs_out) {                                    // the reduction is left to the caller (tn_group_check: all three or none)
    for (int p = 0; p < nprob; ++p) {
      slabs_out[p] = g.slabs[p];
      bias_slabs_out[p] = g.bias_slabs[p];
    }
    *splits_out = splits;
    return LTRX_OK;
  }
  for (int p = 0; p < nprob; ++p) {
    launch_slab_reduce(g.slabs[p], splits, (size_t)NP[p] * KP[p], C[p], g.bias_slabs[p], splits, (size_t)NP[p], bias_out[p], s);
    LTRX_LAUNCH_CHECK();
  }
  return LTRX_OK;
}

static int tn_group_check(int nprob, const float* const* A, const int* lda, const float* const* B, const int* ldb, float* const* C,
                          float* const* bias_out, int M, const int* NP, const int* KP, void* ws, const float** slabs_out,
                          const float** bias_slabs_out, int* splits_out) {
  const bool defer = slabs_out && bias_slabs_out && splits_out;   // the caller sums the slabs (ltrx_reduce_group)
  if ((slabs_out || bias_slabs_out || splits_out) && !defer) return LTRX_EINVAL;
  if (defer) *splits_out = 0;
  if (nprob < 1 || nprob > LTRX_TN_GROUP || !A || !lda || !B || !ldb || !C || !bias_out || !NP || !KP || !ws || M <= 0) return LTRX_EINVAL;
  for (int p = 0; p < nprob; ++p)
    if (!A[p] || !B[p] || !C[p] || NP[p] <= 0 || KP[p] <= 0) return LTRX_EINVAL;
  return LTRX_OK;
}

extern "C" int ltrx_gemm_tn_group(int nprob, const float* const* A, const int* lda, const float* const* B, const int* ldb, float* const* C,
                                  float* const* bias_out, int M, const int* NP, const int* KP, int strict, void* ws, size_t ws_bytes,
                                  const float** slabs_out, const float** bias_slabs_out, int* splits_out, ltrx_stream_t stream) {
  const int crc = tn_group_check(nprob, A, lda, B, ldb, C, bias_out, M, NP, KP, ws, slabs_out, bias_slabs_out, splits_out);
  if (crc != LTRX_OK) return crc;
  const TnSidePlan pl = tn_group_side_plan(nprob, M, NP, KP, lda, ldb, strict, ws_bytes, 0, 0, false, false, 0);
  if (!pl.grouped) {                                  // shapes outside the large-tile kernel: one call per problem
    for (int p = 0; p < nprob; ++p) {
      if (ltrx_gemm_tn_workspace_bytes(M, NP[p], KP[p]) > ws_bytes) return LTRX_EINVAL;
      const int rc = ltrx_gemm_tn(A[p], lda[p], B[p], ldb[p], C[p], bias_out[p], M, NP[p], KP[p], strict, 0, ws, stream);
      if (rc != LTRX_OK) return rc;
    }
    return LTRX_OK;
  }
  return tn_group_run(nprob, A, lda, B, ldb, C, bias_out, M, NP, KP, strict, ws, slabs_out, bias_slabs_out, splits_out, pl, nullptr,
                      0, (hipStream_t)stream);
}

// ltrx_gemm_tn_group followed by ltrx_layernorm_bwd_partial, with the LayerNorm backward run by the workgroups of the grouped launch
// that would otherwise leave their CUs idle whenever tn_group_side_plan takes it; else the two launches one after the other.  Same
// bits either way.  dx_out / ln_ws must not overlap an operand of the group: the side workgroups write while the others read.
extern "C" int ltrx_gemm_tn_group_ln(int nprob, const float* const* A, const int* lda, const float* const* B, const int* ldb,
                                     float* const* C, float* const* bias_out, int M, const int* NP, const int* KP, int strict, void* ws,
                                     size_t ws_bytes, const float** slabs_out, const float** bias_slabs_out, int* splits_out,
                                     const float* dy, const float* xsum, const float* a, const float* mean, const float* rstd,
                                     const float* dres_in, int rows, int D, float eps, float* dx_out, void* ln_ws, int* partial_rows_out,
                                     int side_wgs, int* side_taken_out, ltrx_stream_t stream) {
  if (!side_taken_out || !partial_rows_out || side_wgs < 0) return LTRX_EINVAL;
  *side_taken_out = 0;
  const int crc = tn_group_check(nprob, A, lda, B, ldb, C, bias_out, M, NP, KP, ws, slabs_out, bias_slabs_out, splits_out);
  if (crc != LTRX_OK) return crc;
  if (!dy || !xsum || !a || !mean || !rstd || !dx_out || !ln_ws || rows <= 0 || D < 2) return LTRX_EINVAL;   // (ln_bwd_main's)
  const bool vec = ln_vec_ok(D, dy, xsum, dx_out) && ln_vec_ok(D, a, dres_in, ln_ws);
  const TnSidePlan pl = tn_group_side_plan(nprob, M, NP, KP, lda, ldb, strict, ws_bytes, rows, D, vec, dres_in != nullptr, side_wgs);
  // (the partial rows' extent: the workspace the LayerNorm call asks for)
  const size_t dx_bytes = (size_t)rows * D * sizeof(float), lnws_bytes = ltrx_layernorm_bwd_workspace_bytes(rows, D);
  for (int p = 0; p < nprob; ++p) {
    if (lda[p] < NP[p] || ldb[p] < KP[p]) continue;   // (refused below by the GEMM call itself)
    const size_t na = ((size_t)(M - 1) * lda[p] + NP[p]) * sizeof(float), nb = ((size_t)(M - 1) * ldb[p] + KP[p]) * sizeof(float);
    if (ranges_overlap(dx_out, dx_bytes, A[p], na) || ranges_overlap(dx_out, dx_bytes, B[p], nb) ||
        ranges_overlap(ln_ws, lnws_bytes, A[p], na) || ranges_overlap(ln_ws, lnws_bytes, B[p], nb))
      return LTRX_EINVAL;
  }
  if (!pl.grouped || pl.side == 0) {
    const int rc = ltrx_gemm_tn_group(nprob, A, lda, B, ldb, C, bias_out, M, NP, KP, strict, ws, ws_bytes, slabs_out, bias_slabs_out,
                                      splits_out, stream);
    if (rc != LTRX_OK) return rc;
    return ltrx_layernorm_bwd_partial(dy, xsum, a, mean, rstd, dres_in, rows, D, eps, dx_out, ln_ws, partial_rows_out, stream);
  }
  ltrx::LnBwdJob job = {dy, xsum, a, mean, rstd, dres_in, dx_out, (float*)ln_ws, rows, pl.sh.grid, pl.sh.wpb, eps};
  const int rc = tn_group_run(nprob, A, lda, B, ldb, C, bias_out, M, NP, KP, strict, ws, slabs_out, bias_slabs_out, splits_out, pl, &job,
                              D, (hipStream_t)stream);
  if (rc != LTRX_OK) return rc;
  *partial_rows_out = pl.sh.grid;
  *side_taken_out = pl.side;
  return LTRX_OK;
}

// ---- test hooks (no GPU needed; documented in include/ltrx.h): what the plans above decide, by the code the calls run ----
extern "C" int ltrx_debug_tn_group_map(int nprob, int M, const int* NP, const int* KP, unsigned char* tile_out, unsigned char* split_out) {
  if (nprob < 1 || nprob > LTRX_TN_GROUP || !NP || !KP || !tile_out || !split_out || M <= 0) return 0;
  const TnSidePlan pl = tn_group_side_plan(nprob, M, NP, KP, nullptr, nullptr, 0, ~(size_t)0, 0, 0, false, false, 0);
  if (!pl.grouped) return 0;
  TnGroup g = {};
  for (int p = 0; p < nprob; ++p) tn_group_set(g, p, nullptr, 0, nullptr, 0, NP[p], KP[p], nullptr, nullptr);
  tn_group_map(g, pl.total, pl.splits);
  for (int w = 0; w < pl.gemm_wgs; ++w) {
    tile_out[w] = g.map_tile[w];
    split_out[w] = g.map_split[w];
  }
  return pl.gemm_wgs;
}

extern "C" int ltrx_debug_tn_group_side_plan(int nprob, int M, const int* NP, const int* KP, int rows, int D, int has_dres, int side_wgs,
                                             int* gemm_wgs_out, int* vblocks_out, int* owner_out) {
  if (nprob < 1 || nprob > LTRX_TN_GROUP || !NP || !KP || M <= 0 || rows <= 0 || D <= 0 || side_wgs < 0 || !gemm_wgs_out || !vblocks_out ||
      !owner_out)
    return 0;
  const TnSidePlan pl = tn_group_side_plan(nprob, M, NP, KP, nullptr, nullptr, 0, ~(size_t)0, rows, D, ln_vec_ok(D, nullptr, nullptr, nullptr),
                                           has_dres != 0, side_wgs);
  *gemm_wgs_out = pl.grouped ? pl.gemm_wgs : 0;
  *vblocks_out = pl.sh.grid;
  for (int vb = 0; vb < 320; ++vb) owner_out[vb] = -1;
  if (!pl.grouped) return 0;
  for (int sw = 0; sw < pl.side; ++sw)                 // the kernel's walk (rowreg_ln_bwd_side)
    for (int vb = sw; vb < pl.sh.grid; vb += pl.side) owner_out[vb] = pl.gemm_wgs + sw;
  return pl.side;
}

// (the three plans themselves)
extern "C" int ltrx_debug_gemm_nt_plan(int M, int N, int K, int lda, int ldb, int ldc, int act, int has_bias, int drop_on, int strict,
                                       int tile, int vec_epi, int b_image, int* out) {
  if (!out) return 0;
  NtPlan pl = {LTRX_EINVAL, 0, {}};
  if (M > 0 && N > 0 && K > 0 && act >= 0 && act <= 5 && tile >= 0)
    pl = nt_plan(M, N, K, lda, ldb, ldc, act, has_bias != 0, drop_on != 0, strict, tile, vec_epi != 0, b_image != 0);
  out[0] = pl.rc;
  for (int i = 0; i < pl.nseg; ++i) {
    const NtSeg& sg = pl.seg[i];
    const int v[7] = {sg.m0, sg.rows, sg.tile, sg.nterms, sg.tail, sg.bimg, sg.epi};
    for (int j = 0; j < 7; ++j) out[7 * i + j] = v[j];
  }
  return pl.nseg;
}

extern "C" int ltrx_debug_gemm_tn_plan(int M, int NP, int KP, int lda, int ldb, int strict, int tile, int* splits_out, int* rows_per_split_out,
                                       int* kv_out) {
  if (M <= 0 || NP <= 0 || KP <= 0 || tile < 0 || lda < NP || ldb < KP || !splits_out || !rows_per_split_out || !kv_out) return -1;
  const TnPlan pl = tn_plan(M, NP, KP, lda, ldb, strict, tile);
  *splits_out = pl.splits;
  *rows_per_split_out = pl.mps;
  *kv_out = pl.kv;
  return pl.large ? 1 : 0;
}

extern "C" int ltrx_debug_tn_group_plan(int nprob, int M, const int* NP, const int* KP, const int* lda, const int* ldb, int strict,
                                        size_t ws_bytes, int* splits_out, size_t* need_bytes_out) {
  if (splits_out) *splits_out = 0;
  if (need_bytes_out) *need_bytes_out = 0;
  if (nprob < 1 || nprob > LTRX_TN_GROUP || !NP || !KP || M <= 0 || !splits_out || !need_bytes_out) return 0;
  const TnSidePlan pl = tn_group_side_plan(nprob, M, NP, KP, lda, ldb, strict, ws_bytes, 0, 0, false, false, 0);   // as ltrx_gemm_tn_group
  *need_bytes_out = pl.need;
  if (pl.grouped) *splits_out = pl.splits;
  return pl.grouped ? 1 : 0;
}
