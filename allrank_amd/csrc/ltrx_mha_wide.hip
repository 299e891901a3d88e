// Masked self-attention FORWARD on the bf16 matrix cores with fp32-class accuracy for WIDE heads, 64 < d_k <= 128
// (allrank/models/transformer.py:137-156; the shipped 96 / 1 and 144 / 2 transformer configs have head widths 96 and 72).
//
// ltrx_mha_res.hip stops at d_k 64; wider heads otherwise run the exact kernels of ltrx_mha.hip on v_mfma_f32_32x32x2_f32, 1/16 of the
// bf16 matrix rate.  This kernel has the arithmetic and every convention of ltrx_mha_fwd_res_kernel -- each contraction is three
// v_mfma_f32_32x32x16_bf16 products X Y ~= Xhi Yhi + Xhi Ylo + Xlo Yhi (PL: only the first; mode 2), Q pre-scaled by scale * log2 e
// before its split, a log2-domain online softmax with the lazy reference (kLazyTau), the natural-log lse at [slate, head, row],
// dropout on P regenerated from (seed, query row, key) by drop_row_seed / drop_scale_rk, both layouts through which_slate() -- so
// its o / lse feed ltrx_mha_bwd of the same mode, which runs the exact backward at these widths.  Opt-in (ltrx_mha_fwd_wide):
// it rounds differently from the exact arm that ltrx_mha_fwd keeps dispatching here.
//
// What is different is how the work is laid out, because nothing of the resident design fits at these row widths:
//   * LDS.  Four bf16 planes (K hi / lo, V hi / lo) cost 8 DKP bytes per key row: a 256-row image would be 192 / 256 KB of the CU's
//     160.  K and V therefore STREAM through a ring of TWO 32-row tile slots (2 x 4 planes x 32 x DKP bf16 = 48 KB at DKP 96, 64 KB at
//     DKP 128).  A tile is split into hi / lo once, by the staging threads on its way from registers into its slot; the loads of tile
//     t + 1 are in flight while the waves compute on tile t.
//   * write-after-read with a two-slot ring and ONE barrier per tile.  Iteration t is: store tile t into slot t & 1; barrier t;
//     compute on slot t & 1.  A thread that stores tile t has passed barrier t - 1, so every wave has ARRIVED at barrier t - 1, and a
//     wave's compute of tile t - 2 -- the previous tenant of slot t & 1 -- precedes its arrival there in program order.  The only tile
//     a slow wave can still be reading is t - 1, in the other slot.  Two slots are thus enough and a deeper ring buys nothing: the
//     store of tile t + 1 cannot be issued before barrier t anyway, its data sits in registers.  (The resident kernel needed the
//     argument "a slot is written once per 256 keys"; this one needs "once per 64 keys, and 32 of them lie behind a barrier".)
//     The per-slot mask bias and the tile flag follow the same rule.
//   * workgroup.  FOUR waves (256 threads), 32 queries each: 128 queries per workgroup, grid (B h, ceil(L / 128)).  One wave per SIMD
//     may use up to the whole 512-entry register file: the Q hi / lo fragments (DKP / 16 pairs of bf16x8 = 48 / 64 registers) and the O
//     accumulators (DKP / 32 f32x16 = 48 / 64) stay in registers across the key loop next to S, P, the K / V fragments and the
//     staging registers of the next tile (64 DKP / 256 (row, 8-column) positions of 8 floats per thread) -- no scratch (the figures per
//     instantiation: profiles/mha_wide.md).  At DKP 96 all of that fits 256 registers, so the kernel is built for two waves per SIMD
//     and two workgroups (2 x 48 KB) share a CU; at DKP 128 it takes 330 and one workgroup has the CU.  Every workgroup streams all keys
//     of its slate; a 240-item slate is two workgroups.
//   * Q is read straight from memory in the fragment layout (lane = query row, 2 x 16 bytes per 16-column step): the LDS exchange
//     of the resident kernel's prologue would need 16 KB per wave here, i.e. the whole ring and a barrier of its own.
//   * image layout.  Row r of a plane is DKP * 2 bytes = CH = 12 / 16 sixteen-byte chunks; an LDS bank row is 16 chunks (64 banks).
//       DKP 128 (a row IS a bank row): chunk c of row r at position c ^ s(r), s(r) = (r & 3) << 2 | ((r >> 2) & 3).
//       DKP  96 (12 r + c mod 16: four rows walk through the four 4-chunk groups of a bank row): chunk c of row r at position
//               c ^ ((r >> 2) & 3) -- only the two low bits move, so the position stays inside the row's 12 chunks.
//     Row-wise K fragments (ds_read_b128: 16 lanes = rows r .. r + 15 mod 16, one chunk c): at 128, s is a bijection of r & 15, so
//     the 16 positions c ^ s(r) are the 16 different chunks of a bank row.  At 96 the bank position is 4 ((c / 4 - r) & 3) +
//     ((c & 3) ^ ((r >> 2) & 3)): r & 3 picks the group, (r >> 2) & 3 the chunk inside it -- 16 different ones again.
//     Transposed V reads (ds_read_b64_tr_b16: 32 lanes = rows r0 .. r0 + 3, r0 a multiple of 4, chunks 4 ct .. 4 ct + 3): at 128 the
//     position is ((ct ^ j) << 2) | (cc ^ a) for row r0 + j and chunk 4 ct + cc (a = (r0 >> 2) & 3); at 96 it is
//     4 ((ct - r0 - j) & 3) + (cc ^ a): the row picks the 4-chunk group, the chunk the place in it -- 16 different 16-byte positions,
//     every bank once, both times.  Tile slots and planes start at multiples of 256 bytes, so the argument holds in every slot.
//     The staging stores (16 lanes = 16 consecutive chunks of one or two rows) permute inside groups of 4 chunks: conflict-free.
//   * barriers.  Every wave takes every barrier.  A wave whose queries lie beyond the slate (`active` false) keeps staging; the only
//     early return is the workgroup-uniform one before the first barrier.  No thread reads a row at or beyond the slate's length.
// Compiled without the packed-fp32 VALU instructions (allrank_amd/build.py), and the code uses no two-float vector arithmetic.
//
// ---- BACKWARD (ltrx_mha_bwd_wide: ltrx_mha_bwd_wide_dq_kernel, then ltrx_mha_bwd_wide_dkdv_kernel on the same stream) ------------
// The same workgroup (four waves, 128 rows of one slate-head, grid (B h, ceil(L / 128))), ring (two 32-row slots of four bf16
// planes, one barrier per tile, the write-after-read argument above), image layout, three-product arithmetic and log2 domain.  P is
// recomputed from the saved natural-log lse -- P = exp2(S + key bias - lse log2 e) -- so there is no running reference here.
//   dQ kernel.  A wave owns 32 queries.  In registers for the whole key loop: Q hi / lo (pre-scaled by scale log2 e before the split),
//     dO hi / lo, the dQ accumulators.  A slot holds V hi, V lo, K hi, K lo.  Per tile: S^T = K Q^T (row-wise reads of K),
//     dP^T = V dO^T (row-wise reads of V), dS = P (dP keep - delta) scale in the accumulator layout, dQ^T += K^T dS^T (transposed
//     reads of K: dS never moves between lanes).  delta_q = <dO_q, O_q> is summed in fp32 in the prologue from the unsplit rows the
//     lane loads for its dO fragments, and written to ws[slate-head][q] for the second kernel.
//   dK/dV kernel.  A wave owns 32 keys.  In registers: K hi / lo (pre-scaled: K enters only S here), V hi / lo, the dK and dV
//     accumulators, the key's bias (-inf: masked or >= len).  A slot holds Q hi, Q lo, dO hi, dO lo (unscaled) and 32 entries each of
//     lse log2 e (+inf for a row >= len: P = 0), delta and, under dropout, the row seed, written by threads 0-31 under the rule of the
//     forward's kbias.  Per tile: S = Q K^T (row-wise Q), dP = dO V^T (row-wise dO), P keep and dS in one pass,
//     dV^T += dO^T (P keep) (transposed dO), dK^T += Q^T dS (transposed Q).  A masked key has P = 0 in every tile: its dK and dV rows are exact zeros.
//   * operand layout: REGISTERS, not a wave-private LDS image of dO.  One wave per SIMD owns the 512-entry register file; the fixed
//     operands and accumulators are 192 (dQ) / 256 (dK/dV) of them at DKP 128 and the rest -- S, dP, dS, the streamed fragments, the
//     staging registers -- fits beside them without scratch (profiles/mha_wide.md has the table), so the extra LDS reads and the
//     12 / 16 KB per wave of an image are not spent.
//   * bank conflicts: wide_off() is the layout of EVERY plane, planes and slots start at multiples of 256 bytes, and both kernels read
//     with the forward's two lane assignments (TileOffsets): the row-wise reads of K, V, Q and dO are score_tile's (16 lanes = 16 rows,
//     one chunk), the transposed reads of K, dO and Q are value_tile's (32 lanes = 4 rows x 4 chunks of one 4-chunk group).  The
//     forward's argument is about row and chunk numbers inside a plane only, so it covers all of them; the staging stores are the
//     forward's as well.  The 32-entry statistics of a slot are read as the forward reads kbias (b128, two addresses per wave).
//   * barriers: every wave takes every barrier, a wave beyond the slate keeps staging, the only early return is the workgroup-uniform
//     one before the first barrier, and no thread reads a row at or beyond the slate's length (statistics included).
#include "ltrx_mha_split.h"

using namespace ltrx;

namespace {

constexpr int NWAVE = 4;                  // waves of a workgroup
constexpr int QBLK = 32 * NWAVE;          // queries of a workgroup
constexpr int NTHREAD = 64 * NWAVE;
constexpr int NSLOT = 2;                  // tile slots of the ring

template <int DKP>
struct Geo {
  static_assert(DKP == 96 || DKP == 128, "the image layouts below are built for 12 and 16 chunks per row");
  static constexpr int CH = DKP / 8;                      // 16-byte chunks (8 bf16 columns) per row
  static constexpr int KS = DKP / 16;                     // 16-column steps of Q K^T
  static constexpr int NCT = DKP / 32;                    // 32-column blocks of O
  static constexpr int ROWB = DKP * 2;                    // bytes of a row of one plane
  static constexpr int TILEB = 32 * ROWB;                 // one plane of a tile
  static constexpr int SLOTB = 4 * TILEB;                 // K hi, K lo, V hi, V lo
  static constexpr int NPOS = 64 * CH / NTHREAD;          // (row, chunk) positions of K and V a thread stages per tile
  static constexpr int WPE = DKP == 96 ? 2 : 1;           // waves per SIMD the register budget is set for (workgroups per CU)
  static constexpr size_t SMEM = (size_t)NSLOT * SLOTB + NSLOT * 32 * sizeof(float) + 16;      // + mask bias per slot + tile flags
};

// byte offset of 16-byte chunk `chunk` of row `row` inside one plane of a tile (see the header for why it is conflict-free)
template <int DKP>
__device__ __forceinline__ int wide_off(int row, int chunk) {
  const int s = (DKP == 128) ? (((row & 3) << 2) | ((row >> 2) & 3)) : ((row >> 2) & 3);
  return row * (DKP * 2) + ((chunk ^ s) << 4);
}

// the tile-invariant part of a thread's staging work: position i = threadIdx.x + 256 j of the 64 CH positions of a tile, K's
// 32 CH first, then V's
template <int DKP>
struct Stager {
  const float* src[Geo<DKP>::NPOS];     // first float of the position in tile 0
  int row[Geo<DKP>::NPOS];              // row inside a tile
  int dst[Geo<DKP>::NPOS];              // byte offset inside a slot (hi plane; lo: + TILEB)
  bool ca[Geo<DKP>::NPOS], cb[Geo<DKP>::NPOS];      // columns c .. c + 3, c + 4 .. c + 7 inside the head
  float4 a[Geo<DKP>::NPOS], b[Geo<DKP>::NPOS];
};
template <int DKP>
__device__ __forceinline__ void stager_init(Stager<DKP>& st, const float* __restrict__ kb, const float* __restrict__ vb, int dk, int rs) {
  using G = Geo<DKP>;
#pragma unroll
  for (int j = 0; j < G::NPOS; ++j) {
    const int i = threadIdx.x + NTHREAD * j;
    const bool isv = i >= 32 * G::CH;
    const int w = isv ? i - 32 * G::CH : i;
    const int row = w / G::CH, chunk = w % G::CH, c = chunk * 8;
    st.row[j] = row;
    st.ca[j] = c < dk;
    st.cb[j] = c + 4 < dk;
    st.src[j] = (isv ? vb : kb) + (size_t)row * rs + (st.ca[j] ? c : 0);
    st.dst[j] = (isv ? 2 * G::TILEB : 0) + wide_off<DKP>(row, chunk);
  }
}
template <int DKP>
__device__ __forceinline__ void stager_gload(Stager<DKP>& st, int tile, int len, int rs) {
#pragma unroll
  for (int j = 0; j < Geo<DKP>::NPOS; ++j) {
    const bool ok = tile * 32 + st.row[j] < len;
    const float* p = st.src[j] + (size_t)tile * 32 * rs;
    st.a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    st.b[j] = st.a[j];
    if (ok && st.ca[j]) st.a[j] = *reinterpret_cast<const float4*>(p);
    if (ok && st.cb[j]) st.b[j] = *reinterpret_cast<const float4*>(p + 4);
  }
}
template <int DKP, bool PL>
__device__ __forceinline__ void stager_sstore(const Stager<DKP>& st, unsigned char* slot) {
#pragma unroll
  for (int j = 0; j < Geo<DKP>::NPOS; ++j) {
    bf16x8 h, l;
    split8(st.a[j], st.b[j], h, l);
    *reinterpret_cast<bf16x8*>(slot + st.dst[j]) = h;
    if (!PL) *reinterpret_cast<bf16x8*>(slot + st.dst[j] + Geo<DKP>::TILEB) = l;
  }
}

// a wave's fixed-operand fragments read straight from memory: row r0 + l31, columns 16 ks + 8 half + 0..7, times `pre`, split.
// Every load is issued before the first split.
template <int KS>
__device__ __forceinline__ void q_fragments(bf16x8 (&qh)[KS], bf16x8 (&ql)[KS], const float* __restrict__ qb, int q0, int len, int dk, int rs,
                                            float pre) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const bool rok = q0 + l31 < len;
  const float* rowp = qb + (size_t)(rok ? q0 + l31 : 0) * rs;                  // (row 0 exists)
  f32x4 a[KS], b[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int c = 16 * ks + 8 * half;
    const bool oa = rok && c < dk, ob = rok && c + 4 < dk;
    const f32x4 va = *reinterpret_cast<const f32x4*>(rowp + (oa ? c : 0));
    const f32x4 vb = *reinterpret_cast<const f32x4*>(rowp + (ob ? c + 4 : 0));
    a[ks] = oa ? va : f32x4{0.f, 0.f, 0.f, 0.f};
    b[ks] = ob ? vb : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const float x[8] = {a[ks][0] * pre, a[ks][1] * pre, a[ks][2] * pre, a[ks][3] * pre, b[ks][0] * pre, b[ks][1] * pre, b[ks][2] * pre, b[ks][3] * pre};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      LTRX_SPLIT_BF16(x[e], qh[ks][e], ql[ks][e]);
    }
  }
}

// per-lane byte offsets inside a slot that do not depend on the tile
template <int DKP>
struct TileOffsets {
  int k[Geo<DKP>::KS];             // K fragment ks: chunk 2 ks + half of row l31 (K hi plane; lo: + TILEB)
  int v[2][Geo<DKP>::NCT][2];      // V transposed reads [u][ct][rows r0 / r0 + 8] (V hi plane; lo: + TILEB)
};
template <int DKP>
__device__ __forceinline__ TileOffsets<DKP> tile_offsets() {
  using G = Geo<DKP>;
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5, i16 = lane & 15, g16 = (lane >> 4) & 1;
  const int rsub = i16 >> 2, c8 = (i16 & 3) >> 1, b8 = (i16 & 1) * 8;
  TileOffsets<DKP> f;
#pragma unroll
  for (int ks = 0; ks < G::KS; ++ks) f.k[ks] = wide_off<DKP>(l31, 2 * ks + half);
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int ct = 0; ct < G::NCT; ++ct) {
      const int r0 = 16 * u + 4 * half + rsub, chunk = (2 * ct + g16) * 2 + c8;
      f.v[u][ct][0] = 2 * G::TILEB + wide_off<DKP>(r0, chunk) + b8;
      f.v[u][ct][1] = 2 * G::TILEB + wide_off<DKP>(r0 + 8, chunk) + b8;
    }
  return f;
}

// S^T[key = rowmap(r, half)][query = l31] of the tile in `slot`, in one accumulator
template <int DKP, bool PL>
__device__ __forceinline__ f32x16 score_tile(const unsigned char* slot, const TileOffsets<DKP>& fo, const bf16x8 (&qh)[Geo<DKP>::KS],
                                             const bf16x8 (&ql)[Geo<DKP>::KS]) {
  return score_chain<Geo<DKP>::KS, PL>(slot, fo.k, Geo<DKP>::TILEB, qh, ql);
}

// O^T[d][query] += V^T[d][key] P^T[key][query] of the tile in `slot` (p in D layout: register r <-> key rowmap(r, half)).  The A
// fragment of block ct -- column 32 ct + l31, keys {16 u + 4 half + 0..3, 16 u + 8 + 4 half + 0..3}, the keys a lane's P registers
// 8 u .. 8 u + 7 hold -- comes from two transposed reads of the row-major image: P never moves between lanes.
template <int DKP, bool PL>
__device__ __forceinline__ void value_tile(const unsigned char* slot, const TileOffsets<DKP>& fo, const f32x16& p, f32x16 (&out)[Geo<DKP>::NCT]) {
  value_chain<Geo<DKP>::NCT, PL>(slot, fo.v, Geo<DKP>::TILEB, p, out);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// forward: workgroup (slate * h + head, query block of 128); wave w owns queries 128 blockIdx.y + 32 w .. + 31
// ------------------------------------------------------------------------------------------------------------------
template <int DKP, bool DROP, bool PL>
__global__ void __launch_bounds__(NTHREAD) __attribute__((amdgpu_waves_per_eu(Geo<DKP>::WPE, Geo<DKP>::WPE))) ltrx_mha_fwd_wide_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                    const float* __restrict__ v, const uint8_t* __restrict__ kpm, int L, int h,
                                                                    int dk, int rs, float* __restrict__ o, int ors, float* __restrict__ lse,
                                                                    float scale, DropCfg drop, const uint32_t* __restrict__ drop_step,
                                                                    const int* __restrict__ cu, const int* __restrict__ order) {
  using G = Geo<DKP>;
  extern __shared__ __attribute__((aligned(256))) unsigned char smem[];
  float* kbias = reinterpret_cast<float*>(smem + NSLOT * G::SLOTB);      // [slot][32]: -inf for a masked or out-of-range key, else 0
  int* kflag = reinterpret_cast<int*>(kbias + NSLOT * 32);               // [slot]: does the tile hold such a key?
  if (DROP && drop_step) drop.seed ^= drop_step[0] * 0x9E3779B9u;
  const Slate sl = which_slate(blockIdx.x, L, h, cu, order);
  const int len = sl.len;
  if ((int)(blockIdx.y * QBLK) >= len) return;         // whole workgroup beyond this slate (uniform: before any barrier)
  const int lane = threadIdx.x & 63, half = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t head0 = sl.row0 * rs + (size_t)sl.head * dk;
  Stager<DKP> sg;
  stager_init<DKP>(sg, k + head0, v + head0, dk, rs);
  stager_gload<DKP>(sg, 0, len, rs);
  uint8_t km_n = 0;                                    // threads 0-31: padding-mask byte of key 32 kt + threadIdx.x of the tile being staged
  if (threadIdx.x < 32 && kpm && (int)threadIdx.x < len) km_n = kpm[sl.row0 + threadIdx.x];
  const int q0 = blockIdx.y * QBLK + wave * 32;
  const bool active = q0 < len;                        // (inactive waves still stage and take every barrier)
  bf16x8 qh[G::KS], ql[G::KS];
  q_fragments<G::KS>(qh, ql, q + head0, q0, len, dk, rs, scale * kLog2e);      // S comes out of the MFMAs in the softmax's log2 domain
  const TileOffsets<DKP> fo = tile_offsets<DKP>();
  f32x16 oacc[G::NCT];
#pragma unroll
  for (int ct = 0; ct < G::NCT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[ct][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const uint32_t drow = DROP ? drop_row_seed(drop, sl.bh, sl.Lmax, q0 + (lane & 31)) : 0u;
  const int nkt = (len + 31) / 32;
  for (int kt = 0; kt < nkt; ++kt) {
    const int sidx = kt & (NSLOT - 1);
    unsigned char* slot = smem + sidx * G::SLOTB;
    stager_sstore<DKP, PL>(sg, slot);
    if (threadIdx.x < 32) {
      const bool off = kt * 32 + (int)threadIdx.x >= len || km_n;
      kbias[sidx * 32 + threadIdx.x] = off ? -INFINITY : 0.f;
      const bool any_off = __builtin_amdgcn_ballot_w64(off) != 0;
      if (threadIdx.x == 0) kflag[sidx] = any_off ? 1 : 0;
    }
    if (kt + 1 < nkt) {
      stager_gload<DKP>(sg, kt + 1, len, rs);          // in flight during this tile's MFMAs
      if (threadIdx.x < 32 && kpm && (kt + 1) * 32 + (int)threadIdx.x < len) km_n = kpm[sl.row0 + (kt + 1) * 32 + threadIdx.x];
    }
    lds_only_barrier();
    if (!active) continue;
    f32x16 s = score_tile<DKP, PL>(slot, fo, qh, ql);
    if (__builtin_amdgcn_readfirstlane(kflag[sidx])) {          // (wave-uniform) a masked or out-of-range key in this tile
      const float* kb = kbias + sidx * 32 + 4 * half;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(kb + 8 * g);       // keys 8 g + 4 half + 0..3 = rowmap(4 g + e, half)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[4 * g + e] += b4[e];
      }
    }
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
      for (int ct = 0; ct < G::NCT; ++ct)
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
    value_tile<DKP, PL>(slot, fo, p, oacc);
  }
  if (!active) return;
  const float lt = sum_across_halves(l);
  const float inv = (lt > 0.f) ? 1.0f / lt : 0.f;
  // scratch: the slot that does NOT hold the last tile -- its tenant, tile nkt - 2, lies behind barrier nkt - 1, which this wave has
  // passed; nothing is staged any more
  f32x4* scratch = reinterpret_cast<f32x4*>(smem + (((nkt - 1) & (NSLOT - 1)) ^ 1) * G::SLOTB + wave * 4096);
  store_rows<G::NCT>(o + sl.row0 * ors + (size_t)sl.head * dk, q0, len, dk, ors, oacc, inv, scratch);
  const int qrow = q0 + (lane & 31);
  if (half == 0 && qrow < len) lse[((size_t)sl.b * h + sl.head) * sl.Lmax + qrow] = (lt > 0.f) ? (m + log2f(lt)) * kLn2 : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------
// backward (header: BACKWARD).  Both kernels: workgroup (slate * h + head, row block of 128); wave w owns rows 128 blockIdx.y + 32 w ..
// ------------------------------------------------------------------------------------------------------------------
namespace {

// the staging of two streamed operands with row strides of their own (Q: rs, dO: ors) -- stager_init / stager_gload otherwise
template <int DKP>
__device__ __forceinline__ void stager_init2(Stager<DKP>& st, const float* __restrict__ xb, int xrs, const float* __restrict__ yb, int yrs, int dk) {
  using G = Geo<DKP>;
#pragma unroll
  for (int j = 0; j < G::NPOS; ++j) {
    const int i = threadIdx.x + NTHREAD * j;
    const bool isy = i >= 32 * G::CH;
    const int w = isy ? i - 32 * G::CH : i;
    const int row = w / G::CH, chunk = w % G::CH, c = chunk * 8;
    st.row[j] = row;
    st.ca[j] = c < dk;
    st.cb[j] = c + 4 < dk;
    st.src[j] = (isy ? yb : xb) + (size_t)row * (isy ? yrs : xrs) + (st.ca[j] ? c : 0);
    st.dst[j] = (isy ? 2 * G::TILEB : 0) + wide_off<DKP>(row, chunk);
  }
}
template <int DKP>
__device__ __forceinline__ void stager_gload2(Stager<DKP>& st, int tile, int len, int xrs, int yrs) {
#pragma unroll
  for (int j = 0; j < Geo<DKP>::NPOS; ++j) {
    const bool isy = (int)threadIdx.x + NTHREAD * j >= 32 * Geo<DKP>::CH;
    const bool ok = tile * 32 + st.row[j] < len;
    const float* p = st.src[j] + (size_t)tile * 32 * (isy ? yrs : xrs);
    st.a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    st.b[j] = st.a[j];
    if (ok && st.ca[j]) st.a[j] = *reinterpret_cast<const float4*>(p);
    if (ok && st.cb[j]) st.b[j] = *reinterpret_cast<const float4*>(p + 4);
  }
}

// the wave's dO fragments (q_fragments, unscaled) and delta = <dO row, O row>, summed in fp32 over the unsplit values of both halves
template <int DKP>
__device__ __forceinline__ float do_fragments(bf16x8 (&dh)[Geo<DKP>::KS], bf16x8 (&dl)[Geo<DKP>::KS], const float* __restrict__ dob,
                                              const float* __restrict__ ob, int q0, int len, int dk, int ors) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const bool rok = q0 + l31 < len;
  const size_t ro = (size_t)(rok ? q0 + l31 : 0) * ors;                        // (row 0 exists)
  float del = 0.f;
#pragma unroll
  for (int ks = 0; ks < Geo<DKP>::KS; ++ks) {
    const int c = 16 * ks + 8 * half;
    const bool oa = rok && c < dk, ob2 = rok && c + 4 < dk;
    const f32x4 da = *reinterpret_cast<const f32x4*>(dob + ro + (oa ? c : 0)), db = *reinterpret_cast<const f32x4*>(dob + ro + (ob2 ? c + 4 : 0));
    const f32x4 xa = *reinterpret_cast<const f32x4*>(ob + ro + (oa ? c : 0)), xb = *reinterpret_cast<const f32x4*>(ob + ro + (ob2 ? c + 4 : 0));
    float x[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[e] = oa ? da[e] : 0.f;
      x[4 + e] = ob2 ? db[e] : 0.f;
      del += x[e] * xa[e];
      del += x[4 + e] * xb[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      LTRX_SPLIT_BF16(x[e], dh[ks][e], dl[ks][e]);
    }
  }
  return sum_across_halves(del);
}

// two score_tile()s at once, for the kernel that has no registers to spare: X[row][fixed] of the plane pair at `xs` against (xfh, xfl)
// and of the pair at `ys` against (yfh, yfl).  The streamed fragments are fetched one 16-column step at a time -- 16 registers in
// flight instead of score_tile's 4 KS per product -- and the two accumulator chains alternate.
template <int DKP, bool PL>
__device__ __forceinline__ void score_tiles2(const unsigned char* xs, const unsigned char* ys, const TileOffsets<DKP>& fo,
                                             const bf16x8 (&xfh)[Geo<DKP>::KS], const bf16x8 (&xfl)[Geo<DKP>::KS],
                                             const bf16x8 (&yfh)[Geo<DKP>::KS], const bf16x8 (&yfl)[Geo<DKP>::KS], f32x16& x, f32x16& y) {
  using G = Geo<DKP>;
#pragma unroll
  for (int r = 0; r < 16; ++r) x[r] = y[r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < G::KS; ++ks) {
    const bf16x8 xh = *reinterpret_cast<const bf16x8*>(xs + fo.k[ks]), yh = *reinterpret_cast<const bf16x8*>(ys + fo.k[ks]);
    if (!PL) {
      const bf16x8 xl = *reinterpret_cast<const bf16x8*>(xs + fo.k[ks] + G::TILEB), yl = *reinterpret_cast<const bf16x8*>(ys + fo.k[ks] + G::TILEB);
      x = LTRX_MFMA(xl, xfh[ks], x);
      y = LTRX_MFMA(yl, yfh[ks], y);
      x = LTRX_MFMA(xh, xfl[ks], x);
      y = LTRX_MFMA(yh, yfl[ks], y);
    }
    x = LTRX_MFMA(xh, xfh[ks], x);
    y = LTRX_MFMA(yh, yfh[ks], y);
  }
}

template <int DKP>
constexpr size_t kDkdvSmem = (size_t)NSLOT * Geo<DKP>::SLOTB + NSLOT * 3 * 32 * sizeof(float);      // + lse, delta, row seed per slot

}  // namespace

template <int DKP, bool DROP, bool PL>
__global__ void __launch_bounds__(NTHREAD) __attribute__((amdgpu_waves_per_eu(1, 1))) ltrx_mha_bwd_wide_dq_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const uint8_t* __restrict__ kpm,
    const float* __restrict__ o, const float* __restrict__ dout, const float* __restrict__ lse, float* __restrict__ delta, int L, int h, int dk,
    int rs, int ors, float* __restrict__ dq, int drs, float scale, DropCfg drop, const uint32_t* __restrict__ drop_step,
    const int* __restrict__ cu, const int* __restrict__ order) {
  using G = Geo<DKP>;
  extern __shared__ __attribute__((aligned(256))) unsigned char smem[];      // slot: V hi, V lo, K hi, K lo
  float* kbias = reinterpret_cast<float*>(smem + NSLOT * G::SLOTB);      // [slot][32]: -inf for a masked or out-of-range key, else 0
  int* kflag = reinterpret_cast<int*>(kbias + NSLOT * 32);               // [slot]: does the tile hold such a key?
  if (DROP && drop_step) drop.seed ^= drop_step[0] * 0x9E3779B9u;
  const Slate sl = which_slate(blockIdx.x, L, h, cu, order);
  const int len = sl.len;
  if ((int)(blockIdx.y * QBLK) >= len) return;         // whole workgroup beyond this slate (uniform: before any barrier)
  const int lane = threadIdx.x & 63, half = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t head0 = sl.row0 * rs + (size_t)sl.head * dk, ohead0 = sl.row0 * ors + (size_t)sl.head * dk;
  Stager<DKP> sg;
  stager_init<DKP>(sg, v + head0, k + head0, dk, rs);  // V in the first plane pair, K in the second: value_tile() then reads K^T
  stager_gload<DKP>(sg, 0, len, rs);
  uint8_t km_n = 0;
  if (threadIdx.x < 32 && kpm && (int)threadIdx.x < len) km_n = kpm[sl.row0 + threadIdx.x];
  const int q0 = blockIdx.y * QBLK + wave * 32;
  const bool active = q0 < len;                        // (inactive waves still stage and take every barrier)
  bf16x8 qh[G::KS], ql[G::KS], dh[G::KS], dl[G::KS];
  q_fragments<G::KS>(qh, ql, q + head0, q0, len, dk, rs, scale * kLog2e);
  const float del_q = do_fragments<DKP>(dh, dl, dout + ohead0, o + ohead0, q0, len, dk, ors);
  const int qrow = q0 + (lane & 31);
  const size_t stat = (size_t)sl.bh * sl.Lmax + qrow;
  const float lse_q = (qrow < len) ? lse[stat] * kLog2e : 0.f;
  if (half == 0 && qrow < len) delta[stat] = del_q;
  const TileOffsets<DKP> fo = tile_offsets<DKP>();
  f32x16 dqacc[G::NCT];
  zero_acc<G::NCT>(dqacc);
  const uint32_t drow = DROP ? drop_row_seed(drop, sl.bh, sl.Lmax, qrow) : 0u;
  const int nkt = (len + 31) / 32;
  for (int kt = 0; kt < nkt; ++kt) {
    const int sidx = kt & (NSLOT - 1);
    unsigned char* slot = smem + sidx * G::SLOTB;
    stager_sstore<DKP, PL>(sg, slot);
    if (threadIdx.x < 32) {
      const bool off = kt * 32 + (int)threadIdx.x >= len || km_n;
      kbias[sidx * 32 + threadIdx.x] = off ? -INFINITY : 0.f;
      const bool any_off = __builtin_amdgcn_ballot_w64(off) != 0;
      if (threadIdx.x == 0) kflag[sidx] = any_off ? 1 : 0;
    }
    if (kt + 1 < nkt) {
      stager_gload<DKP>(sg, kt + 1, len, rs);          // in flight during this tile's MFMAs
      if (threadIdx.x < 32 && kpm && (kt + 1) * 32 + (int)threadIdx.x < len) km_n = kpm[sl.row0 + (kt + 1) * 32 + threadIdx.x];
    }
    lds_only_barrier();
    if (!active) continue;
    f32x16 s = score_tile<DKP, PL>(slot + 2 * G::TILEB, fo, qh, ql);          // S^T[key][query], log2 domain
    if (__builtin_amdgcn_readfirstlane(kflag[sidx])) {
      const float* kb = kbias + sidx * 32 + 4 * half;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(kb + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[4 * g + e] += b4[e];
      }
    }
    const f32x16 dp = score_tile<DKP, PL>(slot, fo, dh, dl);                   // dP^T[key][query] (before the dropout mask)
    f32x16 ds;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = fast_exp2(s[r] - lse_q);
      const float keep = DROP ? drop_scale_rk(drop, drow, kt * 32 + rowmap(r, half)) : 1.0f;
      ds[r] = p * (dp[r] * keep - del_q) * scale;
    }
    value_tile<DKP, PL>(slot, fo, ds, dqacc);                                  // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
  }
  if (!active) return;
  f32x4* scratch = reinterpret_cast<f32x4*>(smem + (((nkt - 1) & (NSLOT - 1)) ^ 1) * G::SLOTB + wave * 4096);      // (as the forward)
  store_rows<G::NCT>(dq + sl.row0 * drs + (size_t)sl.head * dk, q0, len, dk, drs, dqacc, 1.0f, scratch);
}

template <int DKP, bool DROP, bool PL>
__global__ void __launch_bounds__(NTHREAD) __attribute__((amdgpu_waves_per_eu(1, 1))) ltrx_mha_bwd_wide_dkdv_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const uint8_t* __restrict__ kpm,
    const float* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta, int L, int h, int dk, int rs, int ors,
    float* __restrict__ dkout, float* __restrict__ dvout, int drs, float scale, DropCfg drop, const uint32_t* __restrict__ drop_step,
    const int* __restrict__ cu, const int* __restrict__ order) {
  using G = Geo<DKP>;
  extern __shared__ __attribute__((aligned(256))) unsigned char smem[];      // slot: Q hi, Q lo, dO hi, dO lo
  float* lse_t = reinterpret_cast<float*>(smem + NSLOT * G::SLOTB);      // [slot][32]: lse log2 e of the tile's queries, +inf beyond the slate
  float* del_t = lse_t + NSLOT * 32;                                     // [slot][32]: delta
  uint32_t* seed_t = reinterpret_cast<uint32_t*>(del_t + NSLOT * 32);    // [slot][32]: dropout row seed (DROP)
  if (DROP && drop_step) drop.seed ^= drop_step[0] * 0x9E3779B9u;
  const Slate sl = which_slate(blockIdx.x, L, h, cu, order);
  const int len = sl.len;
  if ((int)(blockIdx.y * QBLK) >= len) return;         // whole workgroup beyond this slate (uniform: before any barrier)
  const int lane = threadIdx.x & 63, half = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t head0 = sl.row0 * rs + (size_t)sl.head * dk, ohead0 = sl.row0 * ors + (size_t)sl.head * dk;
  const size_t stat0 = (size_t)sl.bh * sl.Lmax;
  Stager<DKP> sg;
  stager_init2<DKP>(sg, q + head0, rs, dout + ohead0, ors, dk);
  stager_gload2<DKP>(sg, 0, len, rs, ors);
  float lse_n = INFINITY, del_n = 0.f;                 // threads 0-31: statistics of query 32 qt + threadIdx.x of the tile being staged
  if (threadIdx.x < 32 && (int)threadIdx.x < len) {
    lse_n = lse[stat0 + threadIdx.x] * kLog2e;
    del_n = delta[stat0 + threadIdx.x];
  }
  const int k0 = blockIdx.y * QBLK + wave * 32;
  const bool active = k0 < len;                        // (inactive waves still stage and take every barrier)
  bf16x8 kh[G::KS], kl[G::KS], vh[G::KS], vl[G::KS];
  q_fragments<G::KS>(kh, kl, k + head0, k0, len, dk, rs, scale * kLog2e);
  q_fragments<G::KS>(vh, vl, v + head0, k0, len, dk, rs, 1.0f);
  const int key = k0 + (lane & 31);
  const float kbias = (key >= len || (kpm && kpm[sl.row0 + key])) ? -INFINITY : 0.f;
  const TileOffsets<DKP> fo = tile_offsets<DKP>();
  TileOffsets<DKP> fq = fo;                            // value_tile()'s transposed reads, moved from the second plane pair to the first
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int ct = 0; ct < G::NCT; ++ct) {
      fq.v[u][ct][0] -= 2 * G::TILEB;
      fq.v[u][ct][1] -= 2 * G::TILEB;
    }
  f32x16 dkacc[G::NCT], dvacc[G::NCT];
  zero_acc<G::NCT>(dkacc);
  zero_acc<G::NCT>(dvacc);
  const int nqt = (len + 31) / 32;
  for (int qt = 0; qt < nqt; ++qt) {
    const int sidx = qt & (NSLOT - 1);
    unsigned char* slot = smem + sidx * G::SLOTB;
    stager_sstore<DKP, PL>(sg, slot);
    if (threadIdx.x < 32) {
      lse_t[sidx * 32 + threadIdx.x] = lse_n;
      del_t[sidx * 32 + threadIdx.x] = del_n;
      if (DROP) seed_t[sidx * 32 + threadIdx.x] = drop_row_seed(drop, sl.bh, sl.Lmax, qt * 32 + threadIdx.x);
    }
    if (qt + 1 < nqt) {
      stager_gload2<DKP>(sg, qt + 1, len, rs, ors);    // in flight during this tile's MFMAs
      if (threadIdx.x < 32) {
        const int qn = (qt + 1) * 32 + threadIdx.x;
        lse_n = INFINITY;
        del_n = 0.f;
        if (qn < len) {
          lse_n = lse[stat0 + qn] * kLog2e;
          del_n = delta[stat0 + qn];
        }
      }
    }
    lds_only_barrier();
    if (!active) continue;
    // both row-wise products first, then P keep and dS in one pass: the two accumulators and their two results are all that lives
    // across the transposed products, next to the 256 registers of the fixed operands
    f32x16 s, dp, pd, ds;                              // S[query][key] (log2 domain), dP[query][key] (before the dropout mask)
    score_tiles2<DKP, PL>(slot, slot + 2 * G::TILEB, fo, kh, kl, vh, vl, s, dp);
#pragma unroll
    for (int g = 0; g < 4; ++g) {                                              // queries 8 g + 4 half + 0..3 = rowmap(4 g + e, half)
      const int at = sidx * 32 + 4 * half + 8 * g;
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_t + at), d4 = *reinterpret_cast<const f32x4*>(del_t + at);
      u32x4 s4 = {0u, 0u, 0u, 0u};
      if (DROP) s4 = *reinterpret_cast<const u32x4*>(seed_t + at);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = fast_exp2(s[4 * g + e] + kbias - l4[e]);
        const float keep = DROP ? drop_scale_rk(drop, s4[e], key) : 1.0f;
        pd[4 * g + e] = p * keep;
        ds[4 * g + e] = p * (dp[4 * g + e] * keep - d4[e]) * scale;
      }
    }
    value_tile<DKP, PL>(slot, fo, pd, dvacc);                                  // dV^T[d][key] += dO^T[d][query] (P keep)[query][key]
    value_tile<DKP, PL>(slot, fq, ds, dkacc);                                  // dK^T[d][key] += Q^T[d][query] dS[query][key]
  }
  if (!active) return;
  // the free slot, as in the forward; the wave's 4 KB are used twice, one store_rows after the other
  f32x4* scratch = reinterpret_cast<f32x4*>(smem + (((nqt - 1) & (NSLOT - 1)) ^ 1) * G::SLOTB + wave * 4096);
  store_rows<G::NCT>(dkout + sl.row0 * drs + (size_t)sl.head * dk, k0, len, dk, drs, dkacc, 1.0f, scratch);
  store_rows<G::NCT>(dvout + sl.row0 * drs + (size_t)sl.head * dk, k0, len, dk, drs, dvacc, 1.0f, scratch);
}

// ------------------------------------------------------------------------------------------------------------------
// host side (the C entry point ltrx_mha_fwd_wide lives next to ltrx_mha_fwd in ltrx_mha.hip and shares its argument checks)
// ------------------------------------------------------------------------------------------------------------------
extern "C" int ltrx_mha_wide_fits(int L, int d_k) {
  return (L > 0 && (L + QBLK - 1) / QBLK <= 65535 && d_k > 64 && d_k <= 128 && d_k % 4 == 0) ? 1 : 0;
}

template <int DKP>
static int launch_wide(const float* q, const float* k, const float* v, const uint8_t* kpm, int B, int L, int h, int dk, int rs, float* o, int ors,
                       float* lse, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order, bool plain,
                       hipStream_t s) {
  constexpr size_t SM = Geo<DKP>::SMEM;
  static std::atomic<uint64_t> attr_done{0};
  const int arc = ltrx_allow_dynamic_lds(attr_done, {{ltrx_mha_fwd_wide_kernel<DKP, false, false>, SM}, {ltrx_mha_fwd_wide_kernel<DKP, true, false>, SM},
                                                     {ltrx_mha_fwd_wide_kernel<DKP, false, true>, SM}, {ltrx_mha_fwd_wide_kernel<DKP, true, true>, SM}});
  if (arc != LTRX_OK) return arc;
  const DropCfg drop = ltrx_make_drop(p_drop, seed);
  const float scale = 1.0f / sqrtf((float)dk);
  const dim3 grid(B * h, (L + QBLK - 1) / QBLK);
#define LTRX_WIDE(D_, P_)                                                                                                                \
  hipLaunchKernelGGL((ltrx_mha_fwd_wide_kernel<DKP, D_, P_>), grid, dim3(NTHREAD), SM, s, q, k, v, kpm, L, h, dk, rs, o, ors, lse, scale, drop, \
                     seed_step, cu, order)
  if (drop.thresh != 0u) {
    if (plain) LTRX_WIDE(true, true); else LTRX_WIDE(true, false);
  } else {
    if (plain) LTRX_WIDE(false, true); else LTRX_WIDE(false, false);
  }
#undef LTRX_WIDE
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

int ltrx_mha_fwd_wide_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, int B, int L, int h, int dk, int rs, float* o,
                             int ors, float* lse, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order,
                             bool plain, hipStream_t s) {
  if (dk <= 96) return launch_wide<96>(q, k, v, kpm, B, L, h, dk, rs, o, ors, lse, p_drop, seed, seed_step, cu, order, plain, s);
  return launch_wide<128>(q, k, v, kpm, B, L, h, dk, rs, o, ors, lse, p_drop, seed, seed_step, cu, order, plain, s);
}

// the backward: the dQ kernel (which also writes delta[B, h, L] into `delta`), then the dK/dV kernel on the same stream
template <int DKP>
static int launch_wide_bwd(const float* q, const float* k, const float* v, const uint8_t* kpm, const float* o, const float* dout, const float* lse,
                           int B, int L, int h, int dk, int rs, int ors, float* dq, float* dkk, float* dv, int drs, float* delta, float p_drop,
                           uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order, bool plain, hipStream_t s) {
  constexpr size_t SQ = Geo<DKP>::SMEM, SK = kDkdvSmem<DKP>;
  static std::atomic<uint64_t> attr_done{0};
  const int arc = ltrx_allow_dynamic_lds(
      attr_done, {{ltrx_mha_bwd_wide_dq_kernel<DKP, false, false>, SQ}, {ltrx_mha_bwd_wide_dq_kernel<DKP, true, false>, SQ},
                  {ltrx_mha_bwd_wide_dq_kernel<DKP, false, true>, SQ}, {ltrx_mha_bwd_wide_dq_kernel<DKP, true, true>, SQ},
                  {ltrx_mha_bwd_wide_dkdv_kernel<DKP, false, false>, SK}, {ltrx_mha_bwd_wide_dkdv_kernel<DKP, true, false>, SK},
                  {ltrx_mha_bwd_wide_dkdv_kernel<DKP, false, true>, SK}, {ltrx_mha_bwd_wide_dkdv_kernel<DKP, true, true>, SK}});
  if (arc != LTRX_OK) return arc;
  const DropCfg drop = ltrx_make_drop(p_drop, seed);
  const float scale = 1.0f / sqrtf((float)dk);
  const dim3 grid(B * h, (L + QBLK - 1) / QBLK);
#define LTRX_WIDE_DQ(D_, P_)                                                                                                               \
  hipLaunchKernelGGL((ltrx_mha_bwd_wide_dq_kernel<DKP, D_, P_>), grid, dim3(NTHREAD), SQ, s, q, k, v, kpm, o, dout, lse, delta, L, h, dk, rs, ors, \
                     dq, drs, scale, drop, seed_step, cu, order)
#define LTRX_WIDE_DKDV(D_, P_)                                                                                                             \
  hipLaunchKernelGGL((ltrx_mha_bwd_wide_dkdv_kernel<DKP, D_, P_>), grid, dim3(NTHREAD), SK, s, q, k, v, kpm, dout, lse, delta, L, h, dk, rs, ors, \
                     dkk, dv, drs, scale, drop, seed_step, cu, order)
  if (drop.thresh != 0u) {
    if (plain) LTRX_WIDE_DQ(true, true); else LTRX_WIDE_DQ(true, false);
  } else {
    if (plain) LTRX_WIDE_DQ(false, true); else LTRX_WIDE_DQ(false, false);
  }
  LTRX_LAUNCH_CHECK();
  if (drop.thresh != 0u) {
    if (plain) LTRX_WIDE_DKDV(true, true); else LTRX_WIDE_DKDV(true, false);
  } else {
    if (plain) LTRX_WIDE_DKDV(false, true); else LTRX_WIDE_DKDV(false, false);
  }
#undef LTRX_WIDE_DQ
#undef LTRX_WIDE_DKDV
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

int ltrx_mha_bwd_wide_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, const float* o, const float* dout,
                             const float* lse, int B, int L, int h, int dk, int rs, int ors, float* dq, float* dkk, float* dv, int drs,
                             float* delta, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order, bool plain,
                             hipStream_t s) {
  if (dk <= 96)
    return launch_wide_bwd<96>(q, k, v, kpm, o, dout, lse, B, L, h, dk, rs, ors, dq, dkk, dv, drs, delta, p_drop, seed, seed_step, cu, order,
                               plain, s);
  return launch_wide_bwd<128>(q, k, v, kpm, o, dout, lse, B, L, h, dk, rs, ors, dq, dkk, dv, drs, delta, p_drop, seed, seed_step, cu, order,
                              plain, s);
}
