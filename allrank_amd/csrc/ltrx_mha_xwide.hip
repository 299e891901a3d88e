// Masked self-attention FORWARD and BACKWARD on the bf16 matrix cores with fp32-class accuracy for EXTRA-WIDE heads, 128 < d_k <= 256
// (d_k % 4 == 0, zero-padded to DKP = 160 / 192 / 224 / 256 columns): a single-head model of d_model 192 or 256, two heads at 512.
// No other kernel of the library takes these widths.  The arithmetic and every convention are those of ltrx_mha_split.h -- three
// v_mfma_f32_32x32x16_bf16 products per contraction (PL: one; mode 2), Q pre-scaled by scale * log2 e before its split, the log2-domain
// online softmax with the lazy reference, the natural-log lse at [slate, head, row], P recomputed from lse in the backward, the dropout
// draw from (seed, query row, key), both row layouts through which_slate() -- so forward and backward see the same mask and a fully
// padded slate gives exact zeros.  K and V (backward: K / V, or Q / dO) STREAM through a ring of two 32-row tile slots in LDS, split
// into hi / lo on their way in; the fixed operand (Q; backward: Q and dO, or K and V) stays in registers for the whole loop.
//
// How the work is split -- the design of this file.  A wave that owned 32 queries across all 256 columns would hold 128 registers of
// Q hi / lo fragments and 128 of O accumulators before S, P, the streamed fragments and the staging registers: the plan of
// ltrx_mha_wide.hip (330 registers at DKP 128) does not scale.  Here the COLUMNS are split across a pair of waves:
//   * workgroup = four waves = 2 row groups x 2 column halves, 64 rows of one slate-head; grid (B h, ceil(L / 64)).  Wave w: rows
//     32 (w >> 1) .. + 31, column half ch = w & 1.
//   * a contraction over d (S = Q K^T; backward also dP = dO V^T) is split by column half: wave ch multiplies columns
//     ch DKP / 2 .. + DKP / 2 - 1 (DKP / 32 sixteen-column steps each, an even split at every DKP) and the two waves of a pair EXCHANGE
//     their 32 x 32 fp32 partials through LDS (4 KB per wave and quantity, accumulator layout, b128 stores and loads of consecutive
//     lanes: conflict-free).  Both then hold S = own + other -- one commutative fp32 addition, so the same bits -- and run the softmax
//     redundantly (16 exp2 per lane and tile; their m, l, P agree bit for bit, no second exchange).
//   * a product whose OUTPUT has d columns (O += P V; dQ += dS K; dK += dS^T Q; dV += P^T dO) is split by 32-column block: of the
//     NCT = DKP / 32 blocks wave 0 owns the first NC0 = ceil(NCT / 2), wave 1 the rest.  At an odd NCT (DKP 160, 224) wave 1 owns one
//     block fewer; its spare accumulator recomputes the last block and is dropped at the store (the pair's time per tile is wave 0's
//     either way, and the code has one shape).
//   registers at DKP 256, fixed operands + accumulators per wave: forward 64 (Q hi / lo) + 64 (O) = 128; dQ kernel 64 (Q) + 64 (dO) +
//   64 (dQ) = 192; dK/dV kernel, whose workgroups compute EITHER dV or dK (grid.z; see the kernel): 64 (K) + 64 (dV) = 128, or 64 (K) +
//   64 (V) + 64 (dK) = 192 -- against the 512 registers of one wave per SIMD.  No instantiation uses scratch; what the compiler
//   reports: profiles/mha_xwide.md.
//   LDS against the CU's 160 KB (163840 B), one workgroup per CU: a slot is four bf16 planes of 32 rows = 256 DKP bytes; the ring is
//   2 x 64 KB = 128 KB at DKP 256 (80 / 96 / 112 KB at 160 / 192 / 224).  Forward: + 4 x 4 KB of S partials = 144 KB.  Backward: + 4 x 8 KB
//   of S and dP partials = 160 KB exactly at DKP 256 (112 / 128 / 144 KB below it) -- so nothing else lives in LDS: the key mask of a
//   tile is a wave ballot (32 bits in scalar registers) instead of the wide kernels' bias array, and the dK/dV kernel's per-query lse,
//   delta and dropout seed sit in lanes 0-31 of every wave and reach the accumulator layout by ds_bpermute.
//   * two barriers per tile, and the next tile staged one operand at a time.  Tile 0 is stored before the loop.  Iteration t:
//     barrier A(t); global loads of the FIRST operand of tile t + 1; partial products on slot t & 1, written to the exchange buffers;
//     barrier B(t); that operand split and stored into slot (t + 1) & 1, global loads of the SECOND operand into the same registers;
//     the other wave's partials, softmax / dS, the output products on slot t & 1; the second operand stored.  A thread holds the
//     registers of half a tile, each load has one phase of MFMAs to arrive in (staging the whole tile at once cost the dK/dV kernel
//     64 to 76 bytes of scratch at DKP 256).  Ring: a thread that stores into slot (t + 1) & 1 has passed A(t), so every wave has
//     arrived there and has finished tile t - 1, the slot's previous tenant; the stores precede the thread's arrival at A(t + 1),
//     behind which tile t + 1 is read.  Exchange: a wave overwrites its buffer after A(t + 1), which its partner reaches only after
//     reading the partials of tile t.  Every wave takes every barrier; waves whose rows lie beyond the slate keep staging (a pair is
//     active or inactive together); the only early return is workgroup-uniform, before any barrier.
//   * image layout: row r of a plane is CH = DKP / 8 sixteen-byte chunks, chunk c at position c ^ s(r); a bank row is 16 chunks.
//       CH 32 (DKP 256; two bank rows per row): s = (r & 3) << 2 | (r >> 2) & 3, the swizzle of the wide kernels at DKP 128 -- it moves
//              the four low bits only, and their argument is about those.
//       CH 24 (DKP 192; r CH mod 16 = 8 (r & 1)): s = ((r >> 1) & 1) << 2 | (r >> 2) & 3.  Row-wise fragment reads (16 lanes = rows
//              r .. r + 15, one chunk): r & 1 picks the half of the bank row, the other three row bits a different chunk of it.
//              Transposed reads (32 lanes = rows r0 .. r0 + 3, r0 % 4 = 0, chunks 4 ct .. + 3): j & 1 picks the half, j >> 1 the
//              4-chunk group, the chunk its place -- 16 different positions both times.
//       CH 20, 28 (DKP 160, 224; r CH mod 16 = +- 4 r): s = (r >> 2) & 3, the wide kernels' layout at DKP 96 and its argument.
//     Planes and slots start at multiples of 256 bytes.  The staging stores (16 lanes = 16 consecutive chunks) permute inside aligned
//     groups of 4 / 8 / 16 chunks: conflict-free.
//   * no atomics; every sum has a fixed order, so results are deterministic.  The backward's workspace is delta[B, h, L] and nothing more.
#include "ltrx_mha_split.h"

using namespace ltrx;

namespace {

constexpr int NWAVE = 4;
constexpr int NTHREAD = 64 * NWAVE;
constexpr int QBLK = 64;                  // rows of a workgroup: two row groups of 32
constexpr int NSLOT = 2;
constexpr int XCHB = 4096;                // one 32 x 32 fp32 partial in the accumulator layout

template <int DKP>
struct Geo {
  static_assert(DKP % 32 == 0 && DKP > 128 && DKP <= 256, "the image layouts below are built for 20, 24, 28 and 32 chunks per row");
  static constexpr int CH = DKP / 8;                      // 16-byte chunks (8 bf16 columns) per row
  static constexpr int HALF = DKP / 2;                    // columns of a wave's share of a contraction over d
  static constexpr int KSH = DKP / 32;                    // 16-column steps of that share
  static constexpr int NCT = DKP / 32;                    // 32-column output blocks of the pair
  static constexpr int NC0 = (NCT + 1) / 2;               // ... of wave 0 (and accumulators of either wave)
  static constexpr int TILEB = 32 * DKP * 2;              // one plane of a tile
  static constexpr int SLOTB = 4 * TILEB;                 // two operands, hi and lo
  static constexpr size_t FWD_SMEM = (size_t)NSLOT * SLOTB + NWAVE * XCHB;
  static constexpr size_t BWD_SMEM = (size_t)NSLOT * SLOTB + 2 * NWAVE * XCHB;
  static_assert(BWD_SMEM <= 160 * 1024, "one workgroup per CU");
};

// byte offset of 16-byte chunk `chunk` of row `row` inside one plane of a tile (header: image layout)
template <int DKP>
__device__ __forceinline__ int xw_off(int row, int chunk) {
  constexpr int CH = DKP / 8;
  const int s = (CH % 16 == 0) ? (((row & 3) << 2) | ((row >> 2) & 3)) : (CH % 8 == 0) ? ((((row >> 1) & 1) << 2) | ((row >> 2) & 3)) : ((row >> 2) & 3);
  return row * (DKP * 2) + ((chunk ^ s) << 4);
}

// staging of ONE streamed operand (a plane pair of a slot): position i = threadIdx.x + 256 j of the 32 CH (row, chunk) positions of a
// tile (the last j is partly idle where 32 CH is no multiple of 256).  The two operands of a tile go through the same registers one
// after the other (header: two barriers per tile).
template <int DKP>
struct Stager {
  static constexpr int NPOS = (32 * Geo<DKP>::CH + NTHREAD - 1) / NTHREAD;
  float4 a[NPOS], b[NPOS];
};
template <int DKP>
__device__ __forceinline__ void stager_gload(Stager<DKP>& st, const float* __restrict__ xb, int rs, int tile, int len, int dk) {
#pragma unroll
  for (int j = 0; j < Stager<DKP>::NPOS; ++j) {
    const int i = threadIdx.x + NTHREAD * j, row = tile * 32 + i / Geo<DKP>::CH, c = (i % Geo<DKP>::CH) * 8;
    const bool ok = i < 32 * Geo<DKP>::CH && row < len;
    const float* p = xb + (size_t)row * rs + c;
    st.a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    st.b[j] = st.a[j];
    if (ok && c < dk) st.a[j] = *reinterpret_cast<const float4*>(p);
    if (ok && c + 4 < dk) st.b[j] = *reinterpret_cast<const float4*>(p + 4);
  }
}
template <int DKP, bool PL>
__device__ __forceinline__ void stager_sstore(const Stager<DKP>& st, unsigned char* planes) {      // hi plane; lo: + TILEB
#pragma unroll
  for (int j = 0; j < Stager<DKP>::NPOS; ++j) {
    const int i = threadIdx.x + NTHREAD * j;
    if (i >= 32 * Geo<DKP>::CH) continue;
    const int dst = xw_off<DKP>(i / Geo<DKP>::CH, i % Geo<DKP>::CH);
    bf16x8 h, l;
    split8(st.a[j], st.b[j], h, l);
    *reinterpret_cast<bf16x8*>(planes + dst) = h;
    if (!PL) *reinterpret_cast<bf16x8*>(planes + dst + Geo<DKP>::TILEB) = l;
  }
}
// tile 0 into slot 0, before the loop
template <int DKP, bool PL>
__device__ __forceinline__ void stage_first(Stager<DKP>& st, unsigned char* slot, const float* __restrict__ xb, int xrs, const float* __restrict__ yb,
                                            int yrs, int len, int dk) {
  stager_gload<DKP>(st, xb, xrs, 0, len, dk);
  stager_sstore<DKP, PL>(st, slot);
  stager_gload<DKP>(st, yb, yrs, 0, len, dk);
  stager_sstore<DKP, PL>(st, slot + 2 * Geo<DKP>::TILEB);
}

// a wave's fixed-operand fragments read straight from memory: row r0 + l31, columns 16 ks + 8 half + 0..7 of the `ncols` columns that
// start at xb (the wave's column half), times `pre`, split.  With `ob` (the same columns of O; xb is then dO): also returns the
// wave's share of delta = <dO row, O row>, summed in fp32 over the unsplit values of both lane halves.
template <int KS>
__device__ __forceinline__ float row_fragments(bf16x8 (&fh)[KS], bf16x8 (&fl)[KS], const float* __restrict__ xb, const float* __restrict__ ob, int r0,
                                               int len, int ncols, int rs, float pre) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const bool rok = r0 + l31 < len;
  const size_t ro = (size_t)(rok ? r0 + l31 : 0) * rs;                         // (row 0 exists)
  float del = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int c = 16 * ks + 8 * half;
    const bool oa = rok && c < ncols, ob2 = rok && c + 4 < ncols;
    const f32x4 va = *reinterpret_cast<const f32x4*>(xb + ro + (oa ? c : 0)), vb = *reinterpret_cast<const f32x4*>(xb + ro + (ob2 ? c + 4 : 0));
    float x[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[e] = oa ? va[e] : 0.f;
      x[4 + e] = ob2 ? vb[e] : 0.f;
    }
    if (ob) {
      const f32x4 xa = *reinterpret_cast<const f32x4*>(ob + ro + (oa ? c : 0)), xc = *reinterpret_cast<const f32x4*>(ob + ro + (ob2 ? c + 4 : 0));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        del += x[e] * xa[e];
        del += x[4 + e] * xc[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float y = x[e] * pre;
      LTRX_SPLIT_BF16(y, fh[ks][e], fl[ks][e]);
    }
  }
  return ob ? sum_across_halves(del) : 0.f;
}

// per-lane byte offsets inside a plane pair that do not depend on the tile, for column half `ch`
template <int DKP>
struct TileOffsets {
  int k[Geo<DKP>::KSH];            // row-wise fragment i: chunk 2 (ch KSH + i) + half of row l31
  int v[2][Geo<DKP>::NC0][2];      // transposed reads [u][ct][rows r0 / r0 + 8] of output block ch NC0 + ct (clamped to the last block)
};
template <int DKP>
__device__ __forceinline__ TileOffsets<DKP> tile_offsets(int ch) {
  using G = Geo<DKP>;
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5, i16 = lane & 15, g16 = (lane >> 4) & 1;
  const int rsub = i16 >> 2, c8 = (i16 & 3) >> 1, b8 = (i16 & 1) * 8;
  TileOffsets<DKP> f;
#pragma unroll
  for (int i = 0; i < G::KSH; ++i) f.k[i] = xw_off<DKP>(l31, 2 * (ch * G::KSH + i) + half);
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int ct = 0; ct < G::NC0; ++ct) {
      const int blk = min(ch * G::NC0 + ct, G::NCT - 1);
      const int r0 = 16 * u + 4 * half + rsub, chunk = (2 * blk + g16) * 2 + c8;
      f.v[u][ct][0] = xw_off<DKP>(r0, chunk) + b8;
      f.v[u][ct][1] = xw_off<DKP>(r0 + 8, chunk) + b8;
    }
  return f;
}

// two score_chain()s at once, for the backward kernels, which have no registers to spare: X[row][fixed] of the plane pair at `xs`
// against (xfh, xfl) and of the pair at `ys` against (yfh, yfl).  The streamed fragments are fetched one 16-column step at a time --
// 16 registers in flight instead of score_chain's 4 KS per product -- and the two accumulator chains alternate.
template <int KS, bool PL>
__device__ __forceinline__ void score_pair(const unsigned char* xs, const unsigned char* ys, const int (&k)[KS], int planeb, const bf16x8 (&xfh)[KS],
                                           const bf16x8 (&xfl)[KS], const bf16x8 (&yfh)[KS], const bf16x8 (&yfl)[KS], f32x16& x, f32x16& y) {
#pragma unroll
  for (int r = 0; r < 16; ++r) x[r] = y[r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const bf16x8 xh = *reinterpret_cast<const bf16x8*>(xs + k[ks]), yh = *reinterpret_cast<const bf16x8*>(ys + k[ks]);
    if (!PL) {
      const bf16x8 xl = *reinterpret_cast<const bf16x8*>(xs + k[ks] + planeb), yl = *reinterpret_cast<const bf16x8*>(ys + k[ks] + planeb);
      x = LTRX_MFMA(xl, xfh[ks], x);
      y = LTRX_MFMA(yl, yfh[ks], y);
      x = LTRX_MFMA(xh, xfl[ks], x);
      y = LTRX_MFMA(yh, yfl[ks], y);
    }
    x = LTRX_MFMA(xh, xfh[ks], x);
    y = LTRX_MFMA(yh, yfh[ks], y);  }
}

// the exchange of a 32 x 32 partial between the two waves of a pair: [register group g][lane] f32x4
__device__ __forceinline__ void xch_put(unsigned char* buf, const f32x16& a) {
  f32x4* p = reinterpret_cast<f32x4*>(buf) + (threadIdx.x & 63);
#pragma unroll
  for (int g = 0; g < 4; ++g) p[64 * g] = f32x4{a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]};
}
__device__ __forceinline__ f32x16 xch_add(const unsigned char* buf, const f32x16& a) {
  const f32x4* p = reinterpret_cast<const f32x4*>(buf) + (threadIdx.x & 63);
  f32x16 s;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 o = p[64 * g];
#pragma unroll
    for (int e = 0; e < 4; ++e) s[4 * g + e] = a[4 * g + e] + o[e];
  }
  return s;
}

// the key mask of tile `kt` as 32 bits: lanes 0-31 of every wave look at key 32 kt + lane (`pad`: its padding-mask byte)
__device__ __forceinline__ uint32_t keys_off(int kt, int len, uint8_t pad) {
  const int lane = threadIdx.x & 63;
  return (uint32_t)__builtin_amdgcn_ballot_w64(lane < 32 && (kt * 32 + lane >= len || pad));
}
__device__ __forceinline__ uint8_t pad_byte(const uint8_t* __restrict__ kpm, size_t row0, int kt, int len) {
  const int lane = threadIdx.x & 63, key = kt * 32 + lane;
  return (kpm && lane < 32 && key < len) ? kpm[row0 + key] : (uint8_t)0;
}
// S^T[key = rowmap(r, half)][query]: -inf where the key is masked or out of range
__device__ __forceinline__ void mask_keys(f32x16& s, uint32_t off, int half) {
  if (off == 0u) return;                               // (wave-uniform)
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if ((off >> rowmap(r, half)) & 1u) s[r] = -INFINITY;
}

__device__ __forceinline__ float lane_bcast(float x, int src) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(x)));
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// forward: workgroup (slate * h + head, query block of 64); wave w owns queries 64 blockIdx.y + 32 (w >> 1) .. + 31, column half w & 1
// ------------------------------------------------------------------------------------------------------------------
template <int DKP, bool DROP, bool PL>
__global__ void __launch_bounds__(NTHREAD) __attribute__((amdgpu_waves_per_eu(1, 1))) ltrx_mha_fwd_xwide_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const uint8_t* __restrict__ kpm, int L, int h, int dk,
    int rs, float* __restrict__ o, int ors, float* __restrict__ lse, float scale, DropCfg drop, const uint32_t* __restrict__ drop_step,
    const int* __restrict__ cu, const int* __restrict__ order) {
  using G = Geo<DKP>;
  extern __shared__ __attribute__((aligned(256))) unsigned char smem[];      // slot: K hi, K lo, V hi, V lo
  if (DROP && drop_step) drop.seed ^= drop_step[0] * 0x9E3779B9u;
  const Slate sl = which_slate(blockIdx.x, L, h, cu, order);
  const int len = sl.len;
  if ((int)(blockIdx.y * QBLK) >= len) return;         // whole workgroup beyond this slate (uniform: before any barrier)
  const int lane = threadIdx.x & 63, half = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), ch = wave & 1;
  unsigned char* xmine = smem + NSLOT * G::SLOTB + wave * XCHB;
  const unsigned char* xother = smem + NSLOT * G::SLOTB + (wave ^ 1) * XCHB;
  const size_t head0 = sl.row0 * rs + (size_t)sl.head * dk;
  Stager<DKP> sg;
  stage_first<DKP, PL>(sg, smem, k + head0, rs, v + head0, rs, len, dk);
  uint8_t pad_n = pad_byte(kpm, sl.row0, 0, len);
  const int q0 = blockIdx.y * QBLK + (wave >> 1) * 32;
  const bool active = q0 < len;                        // (inactive waves still stage and take every barrier)
  bf16x8 qh[G::KSH], ql[G::KSH];
  row_fragments<G::KSH>(qh, ql, q + head0 + ch * G::HALF, nullptr, q0, len, dk - ch * G::HALF, rs, scale * kLog2e);
  const TileOffsets<DKP> fo = tile_offsets<DKP>(ch);
  f32x16 oacc[G::NC0];
  zero_acc<G::NC0>(oacc);
  float m = -INFINITY, l = 0.f;
  const uint32_t drow = DROP ? drop_row_seed(drop, sl.bh, sl.Lmax, q0 + (lane & 31)) : 0u;
  const int nkt = (len + 31) / 32;
  for (int kt = 0; kt < nkt; ++kt) {
    unsigned char* slot = smem + (kt & (NSLOT - 1)) * G::SLOTB;
    unsigned char* next = smem + ((kt + 1) & (NSLOT - 1)) * G::SLOTB;
    const bool more = kt + 1 < nkt;
    const uint32_t off = keys_off(kt, len, pad_n);
    lds_only_barrier();                                // A
    if (more) {
      stager_gload<DKP>(sg, k + head0, rs, kt + 1, len, dk);      // K of the next tile: in flight during the score products
      pad_n = pad_byte(kpm, sl.row0, kt + 1, len);
    }
    f32x16 s;
    if (active) {
      s = score_chain<G::KSH, PL>(slot, fo.k, G::TILEB, qh, ql);      // this half's share of S^T[key][query], log2 domain
      xch_put(xmine, s);
    }
    lds_only_barrier();                                // B
    if (more) {
      stager_sstore<DKP, PL>(sg, next);
      stager_gload<DKP>(sg, v + head0, rs, kt + 1, len, dk);      // V of the next tile: in flight during the value products
    }
    if (active) {
      s = xch_add(xother, s);
      mask_keys(s, off, half);
      float mt = fmaxf(s[0], s[1]);
#pragma unroll
      for (int r = 2; r < 16; ++r) mt = fmaxf(mt, s[r]);
      mt = max_across_halves(mt);
      const bool grow = mt > m + kLazyTau;               // (first tile: m = -inf; nothing but masked keys so far: mt = -inf -> no)
      const float mn = grow ? mt : m;
      const float mref = (mn == -INFINITY) ? 0.f : mn;
      if (__builtin_amdgcn_ballot_w64(grow) != 0) {      // some query's reference moves: rescale what was accumulated under the old one
        const float alpha = grow ? fast_exp2(m - mref) : 1.0f;
        l *= alpha;
#pragma unroll
        for (int ct = 0; ct < G::NC0; ++ct)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[ct][r] *= alpha;
      }
      m = mn;
      f32x16 p;
      float ps0 = 0.f, ps1 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        p[r] = fast_exp2(s[r] - mref);
        p[r + 1] = fast_exp2(s[r + 1] - mref);
        ps0 += p[r];
        ps1 += p[r + 1];
      }
      l += ps0 + ps1;
      if (DROP) {
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] *= drop_scale_rk(drop, drow, kt * 32 + rowmap(r, half));
      }
      value_chain<G::NC0, PL>(slot + 2 * G::TILEB, fo.v, G::TILEB, p, oacc);      // O^T[d][query] += V^T[d][key] P^T[key][query]
    }
    if (more) stager_sstore<DKP, PL>(sg, next + 2 * G::TILEB);
  }
  if (!active) return;
  const float lt = sum_across_halves(l);
  const float inv = (lt > 0.f) ? 1.0f / lt : 0.f;
  // scratch: the slot that does NOT hold the last tile -- its tenant, tile nkt - 2, lies behind barrier A(nkt - 1), which this wave has
  // passed; nothing is staged any more
  f32x4* scratch = reinterpret_cast<f32x4*>(smem + (((nkt - 1) & (NSLOT - 1)) ^ 1) * G::SLOTB + wave * 4096);
  const int c0 = 32 * ch * G::NC0;                     // the wave's first output column (a spare block lies at or beyond DKP: dropped)
  store_rows<G::NC0>(o + sl.row0 * ors + (size_t)sl.head * dk + c0, q0, len, dk - c0, ors, oacc, inv, scratch);
  const int qrow = q0 + (lane & 31);
  if (ch == 0 && half == 0 && qrow < len) lse[((size_t)sl.b * h + sl.head) * sl.Lmax + qrow] = (lt > 0.f) ? (m + log2f(lt)) * kLn2 : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------
// backward, dQ: the forward's workgroup.  A slot holds V hi, V lo, K hi, K lo.  In registers: the wave's column half of Q (pre-scaled)
// and dO, its blocks of dQ.  Per tile: the halves of S^T = K Q^T and dP^T = V dO^T, exchanged; dS = P (dP keep - delta) scale;
// dQ^T += K^T dS^T (transposed reads of K).  delta = <dO, O> is summed over the pair in the prologue and written for the dK/dV kernel.
// ------------------------------------------------------------------------------------------------------------------
template <int DKP, bool DROP, bool PL>
__global__ void __launch_bounds__(NTHREAD) __attribute__((amdgpu_waves_per_eu(1, 1))) ltrx_mha_bwd_xwide_dq_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const uint8_t* __restrict__ kpm,
    const float* __restrict__ o, const float* __restrict__ dout, const float* __restrict__ lse, float* __restrict__ delta, int L, int h, int dk,
    int rs, int ors, float* __restrict__ dq, int drs, float scale, DropCfg drop, const uint32_t* __restrict__ drop_step,
    const int* __restrict__ cu, const int* __restrict__ order) {
  using G = Geo<DKP>;
  extern __shared__ __attribute__((aligned(256))) unsigned char smem[];
  if (DROP && drop_step) drop.seed ^= drop_step[0] * 0x9E3779B9u;
  const Slate sl = which_slate(blockIdx.x, L, h, cu, order);
  const int len = sl.len;
  if ((int)(blockIdx.y * QBLK) >= len) return;         // whole workgroup beyond this slate (uniform: before any barrier)
  const int lane = threadIdx.x & 63, half = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), ch = wave & 1;
  unsigned char* xmine = smem + NSLOT * G::SLOTB + wave * 2 * XCHB;          // S partial, then dP partial
  const unsigned char* xother = smem + NSLOT * G::SLOTB + (wave ^ 1) * 2 * XCHB;
  const size_t head0 = sl.row0 * rs + (size_t)sl.head * dk, ohead0 = sl.row0 * ors + (size_t)sl.head * dk;
  Stager<DKP> sg;
  stage_first<DKP, PL>(sg, smem, v + head0, rs, k + head0, rs, len, dk);
  uint8_t pad_n = pad_byte(kpm, sl.row0, 0, len);
  const int q0 = blockIdx.y * QBLK + (wave >> 1) * 32;
  const bool active = q0 < len;                        // (inactive waves still stage and take every barrier)
  bf16x8 qh[G::KSH], ql[G::KSH], dh[G::KSH], dl[G::KSH];
  row_fragments<G::KSH>(qh, ql, q + head0 + ch * G::HALF, nullptr, q0, len, dk - ch * G::HALF, rs, scale * kLog2e);
  const float del_half = row_fragments<G::KSH>(dh, dl, dout + ohead0 + ch * G::HALF, o + ohead0 + ch * G::HALF, q0, len, dk - ch * G::HALF, ors, 1.0f);
  reinterpret_cast<float*>(xmine)[lane] = del_half;    // (overwritten after barrier A(0), which the partner reaches after this read)
  lds_only_barrier();
  const float del_q = del_half + reinterpret_cast<const float*>(xother)[lane];
  const int qrow = q0 + (lane & 31);
  const size_t stat = (size_t)sl.bh * sl.Lmax + qrow;
  const float lse_q = (qrow < len) ? lse[stat] * kLog2e : 0.f;
  if (ch == 0 && half == 0 && qrow < len) delta[stat] = del_q;
  const TileOffsets<DKP> fo = tile_offsets<DKP>(ch);
  f32x16 dqacc[G::NC0];
  zero_acc<G::NC0>(dqacc);
  const uint32_t drow = DROP ? drop_row_seed(drop, sl.bh, sl.Lmax, qrow) : 0u;
  const int nkt = (len + 31) / 32;
  for (int kt = 0; kt < nkt; ++kt) {
    unsigned char* slot = smem + (kt & (NSLOT - 1)) * G::SLOTB;
    unsigned char* next = smem + ((kt + 1) & (NSLOT - 1)) * G::SLOTB;
    const bool more = kt + 1 < nkt;
    const uint32_t off = keys_off(kt, len, pad_n);
    lds_only_barrier();                                // A
    if (more) {
      stager_gload<DKP>(sg, v + head0, rs, kt + 1, len, dk);      // V of the next tile: in flight during the row-wise products
      pad_n = pad_byte(kpm, sl.row0, kt + 1, len);
    }
    f32x16 s, dp;
    if (active) {
      // halves of S^T[key][query] (log2 domain) and of dP^T[key][query] (before the dropout mask)
      score_pair<G::KSH, PL>(slot + 2 * G::TILEB, slot, fo.k, G::TILEB, qh, ql, dh, dl, s, dp);
      xch_put(xmine, s);
      xch_put(xmine + XCHB, dp);
    }
    lds_only_barrier();                                // B
    if (more) {
      stager_sstore<DKP, PL>(sg, next);
      stager_gload<DKP>(sg, k + head0, rs, kt + 1, len, dk);      // K of the next tile: in flight during the transposed product
    }
    if (active) {
      s = xch_add(xother, s);
      dp = xch_add(xother + XCHB, dp);
      mask_keys(s, off, half);
      f32x16 ds;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = fast_exp2(s[r] - lse_q);
        const float keep = DROP ? drop_scale_rk(drop, drow, kt * 32 + rowmap(r, half)) : 1.0f;
        ds[r] = p * (dp[r] * keep - del_q) * scale;
      }
      value_chain<G::NC0, PL>(slot + 2 * G::TILEB, fo.v, G::TILEB, ds, dqacc);         // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
    }
    if (more) stager_sstore<DKP, PL>(sg, next + 2 * G::TILEB);
  }
  if (!active) return;
  f32x4* scratch = reinterpret_cast<f32x4*>(smem + (((nkt - 1) & (NSLOT - 1)) ^ 1) * G::SLOTB + wave * 4096);      // (as the forward)
  const int c0 = 32 * ch * G::NC0;
  store_rows<G::NC0>(dq + sl.row0 * drs + (size_t)sl.head * dk + c0, q0, len, dk - c0, drs, dqacc, 1.0f, scratch);
}

// ------------------------------------------------------------------------------------------------------------------
// backward, dK/dV: one launch, grid (B h, ceil(L / 64), 2) -- workgroups z = 0 compute dV, z = 1 compute dK.  With both in one wave the
// fixed operands and accumulators alone would be 256 registers at DKP 256 (the wide kernels' dK/dV at DKP 128, which is within 4
// registers of the file) next to twice their staging registers; split, the dV half holds 64 (K) + 64 (dV) and the dK half 64 (K) +
// 64 (V) + 64 (dK), the dQ kernel's plan.  The price is S computed twice and Q / dO streamed by both; the gain, besides fitting, is twice
// the workgroups (a 64 x 240 batch fills 512 instead of 256).
// Wave w owns keys 64 blockIdx.y + 32 (w >> 1) .. + 31, column half w & 1.  A slot holds Q hi, Q lo, dO hi, dO lo (unscaled).  In
// registers: the wave's column half of K (pre-scaled: K enters only S here) and, for dK, of V; its blocks of dV or dK; the key's bias
// (-inf: masked or >= len).  Lanes 0-31 of every wave hold lse log2 e (+inf for a row >= len: P = 0), delta and, under dropout, the row
// seed of query 32 qt + lane.  Per tile, dV: the halves of S = Q K^T, exchanged; dV^T += dO^T (P keep).  dK: the halves of S and of
// dP = dO V^T, exchanged; dS; dK^T += Q^T dS.  A masked key has P = 0 in every tile: its dK and dV rows are exact zeros.
// ------------------------------------------------------------------------------------------------------------------
template <int DKP, bool DROP, bool PL, bool DV>
__device__ __forceinline__ void xwide_dkdv_body(unsigned char* smem, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                const uint8_t* __restrict__ kpm, const float* __restrict__ dout, const float* __restrict__ lse,
                                                const float* __restrict__ delta, int h, int dk, int rs, int ors, float* __restrict__ out, int drs,
                                                float scale, const DropCfg& drop, const Slate& sl) {
  using G = Geo<DKP>;
  const int len = sl.len;
  const int lane = threadIdx.x & 63, half = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), ch = wave & 1;
  unsigned char* xmine = smem + NSLOT * G::SLOTB + wave * 2 * XCHB;
  const unsigned char* xother = smem + NSLOT * G::SLOTB + (wave ^ 1) * 2 * XCHB;
  const size_t head0 = sl.row0 * rs + (size_t)sl.head * dk, ohead0 = sl.row0 * ors + (size_t)sl.head * dk;
  const size_t stat0 = (size_t)sl.bh * sl.Lmax;
  Stager<DKP> sg;
  stage_first<DKP, PL>(sg, smem, q + head0, rs, dout + ohead0, ors, len, dk);
  float lse_n = INFINITY, del_n = 0.f;                 // lanes 0-31: statistics of query 32 qt + lane of the tile being staged
  if (lane < 32 && lane < len) {
    lse_n = lse[stat0 + lane] * kLog2e;
    if (!DV) del_n = delta[stat0 + lane];
  }
  const int k0 = blockIdx.y * QBLK + (wave >> 1) * 32;
  const bool active = k0 < len;                        // (inactive waves still stage and take every barrier)
  bf16x8 kh[G::KSH], kl[G::KSH], vh[DV ? 1 : G::KSH], vl[DV ? 1 : G::KSH];
  row_fragments<G::KSH>(kh, kl, k + head0 + ch * G::HALF, nullptr, k0, len, dk - ch * G::HALF, rs, scale * kLog2e);
  if constexpr (!DV) row_fragments<G::KSH>(vh, vl, v + head0 + ch * G::HALF, nullptr, k0, len, dk - ch * G::HALF, rs, 1.0f);
  const int key = k0 + (lane & 31);
  const float kbias = (key >= len || (kpm && kpm[sl.row0 + key])) ? -INFINITY : 0.f;
  const TileOffsets<DKP> fo = tile_offsets<DKP>(ch);
  f32x16 acc[G::NC0];
  zero_acc<G::NC0>(acc);
  const int nqt = (len + 31) / 32;
  for (int qt = 0; qt < nqt; ++qt) {
    unsigned char* slot = smem + (qt & (NSLOT - 1)) * G::SLOTB;
    unsigned char* next = smem + ((qt + 1) & (NSLOT - 1)) * G::SLOTB;
    const bool more = qt + 1 < nqt;
    const float lse_c = lse_n, del_c = del_n;
    lds_only_barrier();                                // A
    if (more) {
      stager_gload<DKP>(sg, q + head0, rs, qt + 1, len, dk);      // Q of the next tile: in flight during the row-wise products
      const int qn = (qt + 1) * 32 + lane;
      lse_n = INFINITY;
      del_n = 0.f;
      if (lane < 32 && qn < len) {
        lse_n = lse[stat0 + qn] * kLog2e;
        if (!DV) del_n = delta[stat0 + qn];
      }
    }
    f32x16 s, dp;
    if (active) {
      if constexpr (DV) {
        s = score_chain<G::KSH, PL>(slot, fo.k, G::TILEB, kh, kl);      // this half's share of S[query][key], log2 domain
      } else {                                                         // ... and of dP[query][key] (before the dropout mask)
        score_pair<G::KSH, PL>(slot, slot + 2 * G::TILEB, fo.k, G::TILEB, kh, kl, vh, vl, s, dp);
        xch_put(xmine + XCHB, dp);
      }
      xch_put(xmine, s);
    }
    lds_only_barrier();                                // B
    if (more) {
      stager_sstore<DKP, PL>(sg, next);
      stager_gload<DKP>(sg, dout + ohead0, ors, qt + 1, len, dk);      // dO of the next tile: in flight during the transposed product
    }
    if (active) {
      s = xch_add(xother, s);
      if constexpr (!DV) dp = xch_add(xother + XCHB, dp);
      const uint32_t seed_c = DROP ? drop_row_seed(drop, sl.bh, sl.Lmax, qt * 32 + (lane & 31)) : 0u;
      f32x16 w;                                          // P keep (dV) or dS (dK)
#pragma unroll
      for (int r = 0; r < 16; ++r) {                     // query rowmap(r, half) of the tile: its statistics come from that lane
        const int src = rowmap(r, half);
        const float p = fast_exp2(s[r] + kbias - lane_bcast(lse_c, src));
        const float keep = DROP ? drop_scale_rk(drop, (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)seed_c), key) : 1.0f;
        w[r] = DV ? p * keep : p * (dp[r] * keep - lane_bcast(del_c, src)) * scale;
      }
      // dV^T[d][key] += dO^T[d][query] (P keep)[query][key], or dK^T[d][key] += Q^T[d][query] dS[query][key]
      value_chain<G::NC0, PL>(slot + (DV ? 2 * G::TILEB : 0), fo.v, G::TILEB, w, acc);
    }
    if (more) stager_sstore<DKP, PL>(sg, next + 2 * G::TILEB);
  }
  if (!active) return;
  f32x4* scratch = reinterpret_cast<f32x4*>(smem + (((nqt - 1) & (NSLOT - 1)) ^ 1) * G::SLOTB + wave * 4096);      // (as the forward)
  const int c0 = 32 * ch * G::NC0;
  store_rows<G::NC0>(out + sl.row0 * drs + (size_t)sl.head * dk + c0, k0, len, dk - c0, drs, acc, 1.0f, scratch);
}

template <int DKP, bool DROP, bool PL>
__global__ void __launch_bounds__(NTHREAD) __attribute__((amdgpu_waves_per_eu(1, 1))) ltrx_mha_bwd_xwide_dkdv_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const uint8_t* __restrict__ kpm,
    const float* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta, int L, int h, int dk, int rs, int ors,
    float* __restrict__ dkout, float* __restrict__ dvout, int drs, float scale, DropCfg drop, const uint32_t* __restrict__ drop_step,
    const int* __restrict__ cu, const int* __restrict__ order) {
  extern __shared__ __attribute__((aligned(256))) unsigned char smem[];
  if (DROP && drop_step) drop.seed ^= drop_step[0] * 0x9E3779B9u;
  const Slate sl = which_slate(blockIdx.x, L, h, cu, order);
  if ((int)(blockIdx.y * QBLK) >= sl.len) return;      // whole workgroup beyond this slate (uniform: before any barrier)
  if (blockIdx.z == 0)
    xwide_dkdv_body<DKP, DROP, PL, true>(smem, q, k, v, kpm, dout, lse, delta, h, dk, rs, ors, dvout, drs, scale, drop, sl);
  else
    xwide_dkdv_body<DKP, DROP, PL, false>(smem, q, k, v, kpm, dout, lse, delta, h, dk, rs, ors, dkout, drs, scale, drop, sl);
}

// ------------------------------------------------------------------------------------------------------------------
// host side (the C entry points ltrx_mha_fwd_xwide / ltrx_mha_bwd_xwide live next to ltrx_mha_fwd in ltrx_mha.hip and share its checks)
// ------------------------------------------------------------------------------------------------------------------
extern "C" int ltrx_mha_xwide_fits(int L, int d_k) {
  return (L > 0 && (L + QBLK - 1) / QBLK <= 65535 && d_k > 128 && d_k <= 256 && d_k % 4 == 0) ? 1 : 0;
}

#define LTRX_XWIDE_DKP(dk, CALL)        \
  do {                                  \
    if ((dk) <= 160) return CALL(160);  \
    if ((dk) <= 192) return CALL(192);  \
    if ((dk) <= 224) return CALL(224);  \
    return CALL(256);                   \
  } while (0)

template <int DKP>
static int launch_xwide(const float* q, const float* k, const float* v, const uint8_t* kpm, int B, int L, int h, int dk, int rs, float* o, int ors,
                        float* lse, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order, bool plain,
                        hipStream_t s) {
  constexpr size_t SM = Geo<DKP>::FWD_SMEM;
  static std::atomic<uint64_t> attr_done{0};
  const int arc = ltrx_allow_dynamic_lds(attr_done, {{ltrx_mha_fwd_xwide_kernel<DKP, false, false>, SM}, {ltrx_mha_fwd_xwide_kernel<DKP, true, false>, SM},
                                                     {ltrx_mha_fwd_xwide_kernel<DKP, false, true>, SM}, {ltrx_mha_fwd_xwide_kernel<DKP, true, true>, SM}});
  if (arc != LTRX_OK) return arc;
  const DropCfg drop = ltrx_make_drop(p_drop, seed);
  const float scale = 1.0f / sqrtf((float)dk);
  const dim3 grid(B * h, (L + QBLK - 1) / QBLK);
#define LTRX_XWIDE(D_, P_)                                                                                                                \
  hipLaunchKernelGGL((ltrx_mha_fwd_xwide_kernel<DKP, D_, P_>), grid, dim3(NTHREAD), SM, s, q, k, v, kpm, L, h, dk, rs, o, ors, lse, scale, drop, \
                     seed_step, cu, order)
  if (drop.thresh != 0u) {
    if (plain) LTRX_XWIDE(true, true); else LTRX_XWIDE(true, false);
  } else {
    if (plain) LTRX_XWIDE(false, true); else LTRX_XWIDE(false, false);
  }
#undef LTRX_XWIDE
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

int ltrx_mha_fwd_xwide_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, int B, int L, int h, int dk, int rs, float* o,
                              int ors, float* lse, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order,
                              bool plain, hipStream_t s) {
#define CALL(DKP) launch_xwide<DKP>(q, k, v, kpm, B, L, h, dk, rs, o, ors, lse, p_drop, seed, seed_step, cu, order, plain, s)
  LTRX_XWIDE_DKP(dk, CALL);
#undef CALL
}

// the backward: the dQ kernel (which also writes delta[B, h, L] into `delta`), then the dK/dV kernel on the same stream
template <int DKP>
static int launch_xwide_bwd(const float* q, const float* k, const float* v, const uint8_t* kpm, const float* o, const float* dout, const float* lse,
                            int B, int L, int h, int dk, int rs, int ors, float* dq, float* dkk, float* dv, int drs, float* delta, float p_drop,
                            uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order, bool plain, hipStream_t s) {
  constexpr size_t SM = Geo<DKP>::BWD_SMEM;
  static std::atomic<uint64_t> attr_done{0};
  const int arc = ltrx_allow_dynamic_lds(
      attr_done, {{ltrx_mha_bwd_xwide_dq_kernel<DKP, false, false>, SM}, {ltrx_mha_bwd_xwide_dq_kernel<DKP, true, false>, SM},
                  {ltrx_mha_bwd_xwide_dq_kernel<DKP, false, true>, SM}, {ltrx_mha_bwd_xwide_dq_kernel<DKP, true, true>, SM},
                  {ltrx_mha_bwd_xwide_dkdv_kernel<DKP, false, false>, SM}, {ltrx_mha_bwd_xwide_dkdv_kernel<DKP, true, false>, SM},
                  {ltrx_mha_bwd_xwide_dkdv_kernel<DKP, false, true>, SM}, {ltrx_mha_bwd_xwide_dkdv_kernel<DKP, true, true>, SM}});
  if (arc != LTRX_OK) return arc;
  const DropCfg drop = ltrx_make_drop(p_drop, seed);
  const float scale = 1.0f / sqrtf((float)dk);
  const dim3 grid(B * h, (L + QBLK - 1) / QBLK);
#define LTRX_XWIDE_DQ(D_, P_)                                                                                                              \
  hipLaunchKernelGGL((ltrx_mha_bwd_xwide_dq_kernel<DKP, D_, P_>), grid, dim3(NTHREAD), SM, s, q, k, v, kpm, o, dout, lse, delta, L, h, dk, rs, ors, \
                     dq, drs, scale, drop, seed_step, cu, order)
#define LTRX_XWIDE_DKDV(D_, P_)                                                                                                            \
  hipLaunchKernelGGL((ltrx_mha_bwd_xwide_dkdv_kernel<DKP, D_, P_>), dim3(grid.x, grid.y, 2), dim3(NTHREAD), SM, s, q, k, v, kpm, dout, lse, delta, L, h, dk, rs, ors, \
                     dkk, dv, drs, scale, drop, seed_step, cu, order)
  if (drop.thresh != 0u) {
    if (plain) LTRX_XWIDE_DQ(true, true); else LTRX_XWIDE_DQ(true, false);
  } else {
    if (plain) LTRX_XWIDE_DQ(false, true); else LTRX_XWIDE_DQ(false, false);
  }
  LTRX_LAUNCH_CHECK();
  if (drop.thresh != 0u) {
    if (plain) LTRX_XWIDE_DKDV(true, true); else LTRX_XWIDE_DKDV(true, false);
  } else {
    if (plain) LTRX_XWIDE_DKDV(false, true); else LTRX_XWIDE_DKDV(false, false);
  }
#undef LTRX_XWIDE_DQ
#undef LTRX_XWIDE_DKDV
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

int ltrx_mha_bwd_xwide_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, const float* o, const float* dout,
                              const float* lse, int B, int L, int h, int dk, int rs, int ors, float* dq, float* dkk, float* dv, int drs,
                              float* delta, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order, bool plain,
                              hipStream_t s) {
#define CALL(DKP) \
  launch_xwide_bwd<DKP>(q, k, v, kpm, o, dout, lse, B, L, h, dk, rs, ors, dq, dkk, dv, drs, delta, p_drop, seed, seed_step, cu, order, plain, s)
  LTRX_XWIDE_DKP(dk, CALL);
#undef CALL
}
