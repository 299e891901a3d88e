// The vocabulary of the split-bf16 attention kernels: ltrx_mha_res.hip (32 < d_k <= 64, the slate's images resident in LDS),
// ltrx_mha_wide.hip (64 < d_k <= 128) and ltrx_mha_narrow.hip (d_k <= 32).  What makes their forward and backward kernels
// interchangeable with each other and with the exact kernels of ltrx_mha.hip is stated here once: both row layouts through
// which_slate(), the log2-domain online softmax with the lazy reference kLazyTau, the natural-log lse at [slate, head, row], the
// dropout draw from (seed, query row, key) (drop_row_seed / drop_scale_rk, ltrx_mfma.h), and the three-product contraction
// X Y ~= Xlo Yhi + Xhi Ylo + Xhi Yhi in that order of accumulation (PL: only the last; mode 2).  The files keep their geometry, their
// swizzle and the offset tables built from it, their ring and barriers, their kernels and launchers.
#pragma once
#include "ltrx_mfma.h"

// ---- host: the launchers and shape predicates ltrx_mha.hip's C entry points dispatch to (defined in the file the name says;
// ltrx_mha_xwide.hip, 128 < d_k <= 256, is the fourth user of this vocabulary) ----
bool ltrx_mha_res_fits(int L, int dk);
bool ltrx_mha_res_bwd_fits(int L, int dk);
size_t ltrx_mha_res_bwd_ws_bytes(int B, int L, int h);
int ltrx_mha_fwd_res_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, int B, int L, int h, int dk, int rs,
                            float* o, int ors, float* lse, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu,
                            const int* order, bool plain, hipStream_t s);
int ltrx_mha_fwd_wide_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, int B, int L, int h, int dk, int rs,
                             float* o, int ors, float* lse, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu,
                             const int* order, bool plain, hipStream_t s);
int ltrx_mha_fwd_narrow_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, int B, int L, int h, int dk, int rs,
                               float* o, int ors, float* lse, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu,
                               const int* order, bool plain, hipStream_t s);
int ltrx_mha_bwd_res_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, const float* o, const float* dout,
                            const float* lse, int B, int L, int h, int dk, int rs, int ors, float* dq, float* dkk, float* dv, int drs,
                            void* ws, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order,
                            bool plain, hipStream_t s);
int ltrx_mha_bwd_wide_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, const float* o, const float* dout,
                             const float* lse, int B, int L, int h, int dk, int rs, int ors, float* dq, float* dkk, float* dv, int drs,
                             float* delta, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order,
                             bool plain, hipStream_t s);
int ltrx_mha_bwd_narrow_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, const float* o, const float* dout,
                               const float* lse, int B, int L, int h, int dk, int rs, int ors, float* dq, float* dkk, float* dv, int drs,
                               float* delta, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order,
                               bool plain, hipStream_t s);
int ltrx_mha_fwd_xwide_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, int B, int L, int h, int dk, int rs,
                              float* o, int ors, float* lse, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu,
                              const int* order, bool plain, hipStream_t s);
int ltrx_mha_bwd_xwide_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, const float* o, const float* dout,
                              const float* lse, int B, int L, int h, int dk, int rs, int ors, float* dq, float* dkk, float* dv, int drs,
                              float* delta, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order,
                              bool plain, hipStream_t s);

#define LTRX_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)

namespace ltrx {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
// lazy rescaling: a query's reference maximum only moves when a tile exceeds it by 2^8 (P <= 256: no overflow anywhere in fp32, the
// bf16 hi / lo split keeps its relative precision; O / l and m + log2 l do not depend on the reference)
constexpr float kLazyTau = 8.0f;

// the (slate, head) of workgroup `wg` (blockIdx.x of a grid (B h, row blocks)), in either row layout: padded [B, L] rows, or
// cu_seqlens rows with slate b = rows cu[b] .. cu[b + 1] - 1, optionally visited in `order`
struct Slate {
  int b, head, bh, Lmax, len;
  size_t row0;
};
__device__ __forceinline__ Slate which_slate(unsigned wg, int L, int h, const int* __restrict__ cu, const int* __restrict__ order) {
  Slate s;
  s.head = wg % h;
  s.b = order ? order[wg / h] : (int)(wg / h);
  s.bh = s.b * h + s.head;
  s.Lmax = L;
  s.row0 = cu ? (size_t)cu[s.b] : (size_t)s.b * L;
  s.len = cu ? cu[s.b + 1] - cu[s.b] : L;
  return s;
}

__device__ __forceinline__ float max_across_halves(float x) {     // lane i <-> lane i ^ 32: {lo, lo} and {hi, hi} after the swap
  const unsigned u = __float_as_uint(x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float sum_across_halves(float x) {
  const unsigned u = __float_as_uint(x);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// two fp32 values -> one register of two bf16 hi parts and one of two bf16 lo parts (x = hi + lo to 2^-17 relative): ONE conversion
// per pair and part, the hi parts widened back with a shift / a mask.  The subtraction comes in two forms that are NOT
// interchangeable: _packed is one v_pk_add_f32 (ltrx_mha_res.hip), _scalar two subtractions (ltrx_mha_wide.hip and
// ltrx_mha_narrow.hip, which are built without the packed-fp32 instructions: allrank_amd/build.py).  Swapping them was tried and
// compared with tools/asm_compare.py: it changes the body of 2 of ltrx_mha_narrow.hip's 4 kernels and of 6 of ltrx_mha_res.hip's
// 12, three of those with different register descriptors.  So both stay, under names that say which is which.
template <bool PL>
__device__ __forceinline__ void split_pair_packed(float x0, float x1, uint32_t& h, uint32_t& l) {
  const bf16x2 hp = {(__bf16)x0, (__bf16)x1};
  h = __builtin_bit_cast(uint32_t, hp);
  if (!PL) {
    const f32x2 hf = {__uint_as_float(h << 16), __uint_as_float(h & 0xffff0000u)};
    const f32x2 d = f32x2{x0, x1} - hf;
    const bf16x2 lp = {(__bf16)d[0], (__bf16)d[1]};
    l = __builtin_bit_cast(uint32_t, lp);
  }
}
template <bool PL>
__device__ __forceinline__ void split_pair_scalar(float x0, float x1, uint32_t& h, uint32_t& l) {
  const bf16x2 hp = {(__bf16)x0, (__bf16)x1};
  h = __builtin_bit_cast(uint32_t, hp);
  if (!PL) {
    const float d0 = x0 - __uint_as_float(h << 16), d1 = x1 - __uint_as_float(h & 0xffff0000u);
    const bf16x2 lp = {(__bf16)d0, (__bf16)d1};
    l = __builtin_bit_cast(uint32_t, lp);
  }
}
template <int NCT>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[NCT]) {
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
}

// staging: the two float4 of one (row, 8-column) position as 8 hi and 8 lo parts
__device__ __forceinline__ void split8(const float4& a, const float4& b, bf16x8& h, bf16x8& l) {
  const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    LTRX_SPLIT_BF16(x[e], h[e], l[e]);
  }
}

// ---- the two contractions of a 32-row tile.  `tile` = LDS address the per-lane byte offsets are relative to; an offset addresses
// the hi plane, the lo plane lies planeb bytes behind it.
// Row-wise: acc[r] = sum_c IMG[rowmap(r, half)][c] * FIXED[l31][c] -- S^T[key][query] in ONE accumulator (a dependent MFMA chain costs
// nothing).  k[ks] = offset of chunk 2 ks + half of row l31.
template <int KS, bool PL>
__device__ __forceinline__ f32x16 score_chain(const unsigned char* tile, const int (&k)[KS], int planeb, const bf16x8 (&fh)[KS],
                                              const bf16x8 (&fl)[KS]) {
  bf16x8 xh[KS], xl[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    xh[ks] = *reinterpret_cast<const bf16x8*>(tile + k[ks]);
    if (!PL) xl[ks] = *reinterpret_cast<const bf16x8*>(tile + k[ks] + planeb);
  }
  f32x16 a;
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
  if (!PL) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a = LTRX_MFMA(xl[ks], fh[ks], a);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a = LTRX_MFMA(xh[ks], fl[ks], a);
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) a = LTRX_MFMA(xh[ks], fh[ks], a);
  return a;
}
// Column-wise: out[ct][r'] += sum_row IMG[row][32 ct + l31] * p[row] (p in D layout: register r <-> tile row rowmap(r, half)).  The A
// fragment of block ct -- rows {16 u + 4 half + 0..3, 16 u + 8 + 4 half + 0..3}, the rows a lane's registers 8 u .. 8 u + 7 of p hold --
// comes from two transposed reads of the row-major image at v[u][ct][0 / 1]: p never moves between lanes.
template <int NCT, bool PL>
__device__ __forceinline__ void value_chain(const unsigned char* tile, const int (&v)[2][NCT][2], int planeb, const f32x16& p,
                                            f32x16 (&out)[NCT]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    u32x4 hw, lw = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t hj, lj = 0u;
      split_pair_scalar<PL>(p[8 * u + 2 * j], p[8 * u + 2 * j + 1], hj, lj);
      hw[j] = hj;
      lw[j] = lj;
    }
    const bf16x8 ph = __builtin_bit_cast(bf16x8, hw), pl = __builtin_bit_cast(bf16x8, lw);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const bf16x4 h0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(tile + v[u][ct][0]));
      const bf16x4 h1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(tile + v[u][ct][1]));
      const bf16x8 vh = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
      if (!PL) {
        const bf16x4 l0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(tile + v[u][ct][0] + planeb));
        const bf16x4 l1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(tile + v[u][ct][1] + planeb));
        const bf16x8 vl = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
        out[ct] = LTRX_MFMA(vl, ph, out[ct]);
        out[ct] = LTRX_MFMA(vh, pl, out[ct]);
      }
      out[ct] = LTRX_MFMA(vh, ph, out[ct]);
    }
  }
}

// lane owns output row row0 + l31; register 4 g + e of out[ct] is column 32 ct + 8 g + 4 half + e.  Written through a wave-private
// 4-KB LDS scratch one [32 rows][32 columns] block at a time, so that a store instruction covers 8 rows x 128 contiguous bytes
// instead of 64 lanes x 16 bytes in 32 different rows (the texture-address unit pays per line: 64 instead of 512 line writes per
// wave and tensor).  Scratch layout: chunk c of row r at c ^ ((r >> 1) & 7).
template <int NCT>
__device__ __forceinline__ void store_rows(float* __restrict__ base, int row0, int nrows, int dk, size_t rs, const f32x16 (&out)[NCT], float scale,
                                           f32x4* scratch) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
      scratch[l31 * 8 + ((2 * g + half) ^ ((l31 >> 1) & 7))] =
          f32x4{out[ct][4 * g + 0] * scale, out[ct][4 * g + 1] * scale, out[ct][4 * g + 2] * scale, out[ct][4 * g + 3] * scale};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = (lane >> 3) + 8 * j, c = 32 * ct + 4 * (lane & 7);
      const f32x4 v = scratch[r * 8 + ((lane & 7) ^ ((r >> 1) & 7))];
      if (row0 + r < nrows && c < dk) *reinterpret_cast<f32x4*>(base + (size_t)(row0 + r) * rs + c) = v;
    }
  }
}

}  // namespace ltrx
