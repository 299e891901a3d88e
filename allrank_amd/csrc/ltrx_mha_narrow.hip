// Masked self-attention FORWARD (and, below, BACKWARD) on the bf16 matrix cores with fp32-class accuracy for NARROW heads, d_k <= 32
// (allrank/models/transformer.py:137-156; a 128 / 4 or 64 / 2 transformer has head width 32, 64 / 4 has 16).
//
// ltrx_mha_res.hip starts at d_k 33; narrower heads otherwise run the exact kernels of ltrx_mha.hip on v_mfma_f32_32x32x2_f32, 1/16 of
// the bf16 matrix rate.  This kernel has the arithmetic and every convention of ltrx_mha_fwd_res_kernel and ltrx_mha_fwd_wide_kernel --
// each contraction is three v_mfma_f32_32x32x16_bf16 products X Y ~= Xhi Yhi + Xhi Ylo + Xlo Yhi (PL: only the first; mode 2), Q
// pre-scaled by scale * log2 e before its split (scale from the true d_k), a log2-domain online softmax with the lazy reference
// (kLazyTau), the natural-log lse at [slate, head, row], dropout on P regenerated from (seed, query row, key) by drop_row_seed /
// drop_scale_rk, both layouts through which_slate() -- so its o / lse feed ltrx_mha_bwd of the same mode, which runs the exact backward
// at these widths.  Opt-in (ltrx_mha_fwd_narrow): it rounds differently from the exact arm that ltrx_mha_fwd keeps dispatching here.
// The head is padded to 32 columns by predicated loads (d_k = 4, 8, ..., 32).
//
// The layout is its own, because at 32 columns a 32 x 32 score tile is 6 + 6 MFMAs and the wide kernel's rhythm -- one barrier and one
// staging round per 32 keys -- would be all overhead:
//   * LDS.  A row of one bf16 plane is 64 bytes.  K and V stream through a ring of TWO slots of 128 key rows, each K hi / K lo /
//     V hi / V lo planes of [128][32] bf16 = 4 x 8 KB = 32 KB; the ring is 64 KB (+ 1 KB of key bias, 32 B of group flags), so two
//     workgroups share a CU.  Each of the 256 threads stages four (row, 8-column) positions per tile -- rows t / 4 and t / 4 + 64 of K
//     and of V, chunk t & 3 -- and splits them into hi / lo once, on the way from registers into the slot, while the loads of the next
//     tile are in flight.
//   * write-after-read with a two-slot ring and ONE barrier per 128-key tile: ltrx_mha_wide.hip's argument per tile.  Iteration t is:
//     store tile t into slot t & 1; barrier t; compute on slot t & 1.  A thread that stores tile t has passed barrier t - 1, so every
//     wave has arrived there, and its compute of tile t - 2 -- the slot's previous tenant -- precedes that arrival in program order.
//     A 240-item slate costs two barriers.  The key bias and the group flags of a slot follow the same rule.
//   * 32-key groups.  Inside a tile the waves walk four groups of 32 keys.  A group's flag says: no key off (no bias is read), some
//     key off (masked or at / beyond the slate's length: the bias, 0 or -inf, is added), every key off (the group is skipped: its P
//     would be exact zeros and the reference would not move).  So the tail groups of a slate's last tile cost nothing.
//   * registers: ONE 32-query block per wave, 128 queries per workgroup, grid (B h, ceil(L / 128)).  Q hi / lo fragments are 2 x 2
//     bf16x8 = 16 registers and the O accumulator 16, so a wave could hold TWO blocks within the 256 registers of two waves per SIMD,
//     and every K / V fragment read from LDS would feed two MFMA chains while a 240-item slate-head is staged once, not twice.  That
//     form was built and timed on the device against this one (profiles/mha_narrow.md): 6 to 10 % faster at 256 slates x 240, but
//     5 to 6 % slower at 64 x 240 (256 workgroups: one per CU, nothing to overlap its prologue with) and 47 % slower on the packed
//     validation shape, whose time is set by the longest slate's workgroups: two blocks per wave double the serial work of exactly
//     those waves.  One block per wave is kept: 117 to 153 registers, no scratch.
//   * P stays in the accumulator layout between the two contractions (transposed V reads, as the wide kernel); nothing moves between
//     lanes but the cross-half max and sum.
//   * Q is read straight from memory in the fragment layout (lane = query row, 2 x 16 bytes per 16-column step).
//   * image layout.  Chunk c (16 bytes) of row r sits at position c ^ ((r >> 2) & 3) of the row's four chunks, so its place in the
//     256-byte bank row is 64 (r & 3) + 16 (c ^ ((r >> 2) & 3)): r & 3 picks the 64-byte quarter, (r >> 2) & 3 the chunk inside it.
//     Row-wise K fragments (ds_read_b128: 16 lanes = rows r .. r + 15, one chunk c): r & 15 runs through all 16 (quarter, chunk)
//     pairs -- 16 different 16-byte positions.  Transposed V reads (ds_read_b64_tr_b16: 32 lanes = rows r0 .. r0 + 3, r0 a multiple
//     of 4, four chunks, two 8-byte halves each): the row picks the quarter, the chunk (xor a constant) the place in it -- 16
//     different positions again.  The staging stores (16 lanes = rows 4 i .. 4 i + 3 x four chunks) likewise.  Planes, slots and
//     32-row groups start at multiples of 256 bytes and of 4 rows x 4, so the argument holds in each of them.
//   * barriers.  Every wave takes every barrier.  A wave whose queries lie beyond the slate keeps staging; the only early return is
//     the workgroup-uniform one before the first barrier.  No thread reads a row at or beyond the slate's length.
// Compiled without the packed-fp32 VALU instructions (allrank_amd/build.py), and the code uses no two-float vector arithmetic.
//
// ---- BACKWARD (ltrx_mha_bwd_narrow: ltrx_mha_bwd_narrow_dq_kernel, then ltrx_mha_bwd_narrow_dkdv_kernel on the same stream) --------
// Opt-in as well (FusedTrainer(narrow_heads="both")).  The same workgroup (four waves, a 32-row block per wave, 128 rows of one
// slate-head, grid (B h, ceil(L / 128))), ring (two slots of 128 rows x four bf16 planes, one barrier per tile, the write-after-read
// argument above), narrow_off() image layout, 32-row groups, three-product chains and log2 domain.  The layout argument carries over
// because it is about the ring and not about the forward: at 32 columns a group is 6 + 6 + 6 (dQ) or 6 + 6 + 6 + 6 (dK/dV) MFMAs
// (mode 1), still too little to pay a barrier and a staging round per 32 rows.  P is recomputed from the saved natural-log lse --
// P = exp2(S + key bias - lse log2 e) -- so there is no running reference; accumulation order is fixed, no atomics.
//   dQ kernel.  A wave owns 32 queries.  In registers for the whole key loop: Q hi / lo (pre-scaled by scale log2 e before the split),
//     dO hi / lo, lse log2 e, delta, the dQ accumulator.  The slot is the forward's -- K hi, K lo, V hi, V lo, staged by the forward's
//     Stager, with the forward's key bias and group flags: a group whose keys are all masked or beyond the slate is skipped (dS = 0).
//     Per group: S^T = K Q^T (row-wise reads of K), dP^T = V dO^T (row-wise reads of V), dS = P (dP keep - delta) scale in the
//     accumulator layout, dQ^T += K^T dS^T (transposed reads of K).  delta_q = <dO_q, O_q> is summed in fp32 in the prologue from the
//     unsplit rows the lane loads for its dO fragments, and written to ws[slate-head][q] for the second kernel.
//   dK/dV kernel.  A wave owns 32 keys.  In registers: K hi / lo (pre-scaled: K enters only S here), V hi / lo, the dK and dV
//     accumulators, the key's bias.  A slot holds Q hi, Q lo, dO hi, dO lo (unscaled; two row strides, split on the way into the
//     slot) and 128 entries each of lse log2 e (+inf for a row >= len: P = 0), delta and, under dropout, the row seed, written by
//     threads 0-127 under the rule of the forward's kbias.  Per group: S = Q K^T, dP = dO V^T (row-wise), P keep and dS in one pass,
//     dV^T += dO^T (P keep) (transposed dO), dK^T += Q^T dS (transposed Q).  Queries are not masked, so this kernel's group flag is a
//     comparison: query groups at or beyond the slate's length are skipped.  A wave whose 32 keys are all off (P = 0 in every tile)
//     keeps staging and taking barriers, runs no product and stores its exact zeros; a masked key inside a live block gets them from
//     P = exp2(-inf).
//   * P / dS stay in the ACCUMULATOR layout for the transposed contractions -- no wave-private LDS round trip.  They are the B operand
//     (rows = the contracted index, which a lane's 16 registers already hold for its column), and the A operand, the transposed
//     image, comes from ds_read_b64_tr_b16 of the row-major planes exactly as the forward reads V: value_chain() with the offsets
//     moved to the plane pair wanted (first_pair()).
//   * bank conflicts: every plane has the forward's layout and is read with the forward's two lane assignments (row-wise: K, V, Q, dO;
//     transposed: K, dO, Q), so the forward's argument covers all of them; the 128-entry statistics are read as kbias is (b128).
//   * resources (gfx950, -O3): dQ 132-161 VGPRs, dK/dV 191-224, no AGPRs, no scratch in any of the eight instantiations, two waves
//     per SIMD; dynamic LDS 66,592 B (dQ: the forward's) and 68,608 B (dK/dV: ring + 3 KB of statistics), two workgroups per CU.
//   * barriers: as the forward.  No thread reads a row at or beyond the slate's length (statistics and delta included).
#include "ltrx_mha_split.h"

using namespace ltrx;

namespace {

constexpr int NWAVE = 4;                  // waves of a workgroup
constexpr int QBLK = 32 * NWAVE;          // queries of a workgroup: a 32-query block per wave
constexpr int NTHREAD = 64 * NWAVE;
constexpr int NSLOT = 2;                  // tile slots of the ring
constexpr int TKEYS = 128;                // key rows of a tile
constexpr int NGRP = TKEYS / 32;          // 32-key groups of a tile
constexpr int KS = 2;                     // 16-column steps of Q K^T
constexpr int ROWB = 64;                  // bytes of a row of one plane (32 bf16)
constexpr int PLANEB = TKEYS * ROWB;      // one plane of a tile
constexpr int SLOTB = 4 * PLANEB;         // K hi, K lo, V hi, V lo
constexpr int GRPB = 32 * ROWB;           // a 32-key group inside a plane
constexpr int NPOS = 4;                   // (row, chunk) positions a thread stages per tile: K rows r, r + 64, V rows r, r + 64
constexpr size_t SMEM = (size_t)NSLOT * SLOTB + NSLOT * TKEYS * sizeof(float) + NSLOT * NGRP * sizeof(int);
static_assert(NTHREAD * NPOS == 2 * TKEYS * 4, "a tile is 2 x 128 rows x 4 chunks");
static_assert(NWAVE * 4096 <= SLOTB, "the epilogue's wave-private scratch lives in one slot");

// byte offset of 16-byte chunk `chunk` of row `row` inside one plane of a tile (see the header for why it is conflict-free)
__device__ __forceinline__ int narrow_off(int row, int chunk) { return row * ROWB + ((chunk ^ ((row >> 2) & 3)) << 4); }

// A thread's staging work.  Position j of 4: rows `row` (j even) / `row + 64` (j odd) of K (j < 2) / V (j >= 2), chunk threadIdx.x & 3.
struct Stager {
  const float* kp;      // first float of the thread's position in row `row` of tile 0
  const float* vp;
  int row, dst;         // row inside a tile; byte offset of (row, chunk) inside a plane -- row + 64 has the same swizzle: + 64 ROWB
  bool ca, cb;          // columns c .. c + 3, c + 4 .. c + 7 lie inside the head
  float4 a[NPOS], b[NPOS];
};
__device__ __forceinline__ void stager_init(Stager& st, const float* __restrict__ kb, const float* __restrict__ vb, int dk, int rs) {
  const int chunk = threadIdx.x & 3, c = chunk * 8;
  st.row = threadIdx.x >> 2;
  st.ca = c < dk;
  st.cb = c + 4 < dk;
  st.kp = kb + (size_t)st.row * rs + (st.ca ? c : 0);
  st.vp = vb + (size_t)st.row * rs + (st.ca ? c : 0);
  st.dst = narrow_off(st.row, chunk);
}
__device__ __forceinline__ void stager_gload(Stager& st, int tile, int len, int rs) {
#pragma unroll
  for (int j = 0; j < NPOS; ++j) {
    const bool ok = tile * TKEYS + st.row + 64 * (j & 1) < len;
    const float* p = (j < 2 ? st.kp : st.vp) + ((size_t)tile * TKEYS + 64 * (j & 1)) * rs;
    st.a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    st.b[j] = st.a[j];
    if (ok && st.ca) st.a[j] = *reinterpret_cast<const float4*>(p);
    if (ok && st.cb) st.b[j] = *reinterpret_cast<const float4*>(p + 4);
  }
}
template <bool PL>
__device__ __forceinline__ void stager_sstore(const Stager& st, unsigned char* slot) {
#pragma unroll
  for (int j = 0; j < NPOS; ++j) {
    bf16x8 h, l;
    split8(st.a[j], st.b[j], h, l);
    unsigned char* at = slot + (j < 2 ? 0 : 2 * PLANEB) + (j & 1) * 64 * ROWB + st.dst;
    *reinterpret_cast<bf16x8*>(at) = h;
    if (!PL) *reinterpret_cast<bf16x8*>(at + PLANEB) = l;
  }
}

// per-lane byte offsets inside a 32-key group of a slot
struct GroupOffsets {
  int k[KS];         // K fragment ks: chunk 2 ks + half of row l31 (K hi plane; lo: + PLANEB)
  int v[2][1][2];    // V transposed reads [u][rows r0 / r0 + 8] (V hi plane; lo: + PLANEB)
};
__device__ __forceinline__ GroupOffsets group_offsets() {
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5, i16 = lane & 15, g16 = (lane >> 4) & 1;
  const int rsub = i16 >> 2, c8 = (i16 & 3) >> 1, b8 = (i16 & 1) * 8;
  GroupOffsets f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) f.k[ks] = narrow_off(l31, 2 * ks + half);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r0 = 16 * u + 4 * half + rsub, chunk = 2 * g16 + c8;
    f.v[u][0][0] = 2 * PLANEB + narrow_off(r0, chunk) + b8;
    f.v[u][0][1] = 2 * PLANEB + narrow_off(r0 + 8, chunk) + b8;
  }
  return f;
}

// the wave's Q fragments: row q0 + l31, columns 16 ks + 8 half + 0..7, times `pre`, split
__device__ __forceinline__ void q_fragments_stepwise(bf16x8 (&qh)[KS], bf16x8 (&ql)[KS], const float* __restrict__ qb, int q0, int len, int dk, int rs,
                                            float pre) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const bool rok = q0 + l31 < len;
  const float* rowp = qb + (size_t)(rok ? q0 + l31 : 0) * rs;                  // (row 0 exists)
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int c = 16 * ks + 8 * half;
    const bool oa = rok && c < dk, ob = rok && c + 4 < dk;
    const f32x4 va = *reinterpret_cast<const f32x4*>(rowp + (oa ? c : 0));
    const f32x4 vb = *reinterpret_cast<const f32x4*>(rowp + (ob ? c + 4 : 0));
    float x[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[e] = oa ? va[e] * pre : 0.f;
      x[4 + e] = ob ? vb[e] * pre : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      LTRX_SPLIT_BF16(x[e], qh[ks][e], ql[ks][e]);
    }
  }
}

// what a wave carries across the key loop for its query block
struct Block {
  bf16x8 qh[KS], ql[KS];
  f32x16 o[1];                             // O^T[d][query] in the accumulator layout
  float m, l;                             // log2-domain reference and (this half's part of) the denominator of query l31
  uint32_t drow;
};

// One 32-key group at `gs` (its K hi plane) against the wave's query block.  S^T[key = rowmap(r, half)][query = l31] comes out of
// the first contraction in one accumulator; P stays in that layout and is the B operand of
// O^T[d][query] += V^T[d][key] P^T[key][query], whose A fragments -- column l31, keys {16 u + 4 half + 0..3, 16 u + 8 + 4 half + 0..3},
// the keys a lane's P registers 8 u .. 8 u + 7 hold -- come from two transposed reads of the row-major image.
template <bool DROP, bool PL>
__device__ __forceinline__ void key_group(const unsigned char* gs, const float* kb, bool biased, const GroupOffsets& fo, Block& w,
                                          const DropCfg& drop, int key0, int half) {
  f32x16 s = score_chain<KS, PL>(gs, fo.k, PLANEB, w.qh, w.ql);
  if (biased) {                                     // (wave-uniform) a masked or out-of-range key in this group
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(kb + 4 * half + 8 * g);      // keys 8 g + 4 half + 0..3 = rowmap(4 g + e, half)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[4 * g + e] += b4[e];
    }
  }
  float mt = fmaxf(s[0], s[1]);
#pragma unroll
  for (int r = 2; r < 16; ++r) mt = fmaxf(mt, s[r]);
  mt = max_across_halves(mt);
  const bool grow = mt > w.m + kLazyTau;             // (first group: m = -inf; nothing but masked keys so far: mt = -inf -> no)
  const float mn = grow ? mt : w.m;
  const float mref = (mn == -INFINITY) ? 0.f : mn;
  if (__builtin_amdgcn_ballot_w64(grow) != 0) {      // some query's reference moves: rescale what was accumulated under the old one
    const float alpha = grow ? fast_exp2(w.m - mref) : 1.0f;
    w.l *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) w.o[0][r] *= alpha;
  }
  w.m = mn;
  f32x16 p;
  float ps0 = 0.f, ps1 = 0.f;
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    p[r] = fast_exp2(s[r] - mref);
    p[r + 1] = fast_exp2(s[r + 1] - mref);
    ps0 += p[r];
    ps1 += p[r + 1];
  }
  w.l += ps0 + ps1;
  if (DROP) {
#pragma unroll
    for (int r = 0; r < 16; ++r) p[r] *= drop_scale_rk(drop, w.drow, key0 + rowmap(r, half));
  }
  value_chain<1, PL>(gs, fo.v, PLANEB, p, w.o);
}

// lane owns output row row0 + l31; register 4 g + e of out is column 8 g + 4 half + e.  Written through a wave-private 4-KB LDS
// scratch: ltrx_mha_split.h's store_rows for one 32-column block, written without the block loop -- store_rows<1> compiles to a
// different instruction order in all four kernels here (profiles/NOTES.md)
__device__ __forceinline__ void store_rows1(float* __restrict__ base, int row0, int nrows, int dk, size_t rs, const f32x16& out, float scale,
                                            f32x4* scratch) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
#pragma unroll
  for (int g = 0; g < 4; ++g)
    scratch[l31 * 8 + ((2 * g + half) ^ ((l31 >> 1) & 7))] =
        f32x4{out[4 * g + 0] * scale, out[4 * g + 1] * scale, out[4 * g + 2] * scale, out[4 * g + 3] * scale};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (lane >> 3) + 8 * j, c = 4 * (lane & 7);
    const f32x4 v = scratch[r * 8 + ((lane & 7) ^ ((r >> 1) & 7))];
    if (row0 + r < nrows && c < dk) *reinterpret_cast<f32x4*>(base + (size_t)(row0 + r) * rs + c) = v;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// forward: workgroup (slate * h + head, query block of 128); wave w owns queries 128 blockIdx.y + 32 w .. + 31
// ------------------------------------------------------------------------------------------------------------------
template <bool DROP, bool PL>
__global__ void __launch_bounds__(NTHREAD) __attribute__((amdgpu_waves_per_eu(2, 2))) ltrx_mha_fwd_narrow_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const uint8_t* __restrict__ kpm, int L, int h, int dk,
    int rs, float* __restrict__ o, int ors, float* __restrict__ lse, float scale, DropCfg drop, const uint32_t* __restrict__ drop_step,
    const int* __restrict__ cu, const int* __restrict__ order) {
  extern __shared__ __attribute__((aligned(256))) unsigned char smem[];
  float* kbias = reinterpret_cast<float*>(smem + NSLOT * SLOTB);         // [slot][128]: -inf for a masked or out-of-range key, else 0
  int* kflag = reinterpret_cast<int*>(kbias + NSLOT * TKEYS);            // [slot][group]: 0 no such key, 1 some, 2 all 32
  if (DROP && drop_step) drop.seed ^= drop_step[0] * 0x9E3779B9u;
  const Slate sl = which_slate(blockIdx.x, L, h, cu, order);
  const int len = sl.len;
  if ((int)(blockIdx.y * QBLK) >= len) return;         // whole workgroup beyond this slate (uniform: before any barrier)
  const int lane = threadIdx.x & 63, half = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t head0 = sl.row0 * rs + (size_t)sl.head * dk;
  Stager sg;
  stager_init(sg, k + head0, v + head0, dk, rs);
  stager_gload(sg, 0, len, rs);
  uint8_t km_n = 0;                                    // threads 0-127: padding-mask byte of key 128 kt + threadIdx.x of the tile being staged
  if (threadIdx.x < TKEYS && kpm && (int)threadIdx.x < len) km_n = kpm[sl.row0 + threadIdx.x];
  const int q0 = blockIdx.y * QBLK + wave * 32;
  const bool active = q0 < len;                        // (inactive waves still stage and take every barrier)
  Block w;
  q_fragments_stepwise(w.qh, w.ql, q + head0, q0, len, dk, rs, scale * kLog2e);      // S comes out of the MFMAs in the softmax's log2 domain
#pragma unroll
  for (int r = 0; r < 16; ++r) w.o[0][r] = 0.f;
  w.m = -INFINITY;
  w.l = 0.f;
  w.drow = DROP ? drop_row_seed(drop, sl.bh, sl.Lmax, q0 + (lane & 31)) : 0u;
  const GroupOffsets fo = group_offsets();
  const int nkt = (len + TKEYS - 1) / TKEYS;
  for (int kt = 0; kt < nkt; ++kt) {
    const int sidx = kt & (NSLOT - 1);
    unsigned char* slot = smem + sidx * SLOTB;
    stager_sstore<PL>(sg, slot);
    if (threadIdx.x < TKEYS) {                         // waves 0 and 1: lane i of wave w holds key 64 w + i, groups 2 w and 2 w + 1
      const bool off = kt * TKEYS + (int)threadIdx.x >= len || km_n;
      kbias[sidx * TKEYS + threadIdx.x] = off ? -INFINITY : 0.f;
      const uint64_t offs = __builtin_amdgcn_ballot_w64(off);
      if (lane < 2) {
        const uint32_t g32 = (uint32_t)(offs >> (32 * lane));
        kflag[sidx * NGRP + 2 * wave + lane] = g32 == 0u ? 0 : (g32 == 0xffffffffu ? 2 : 1);
      }
    }
    if (kt + 1 < nkt) {
      stager_gload(sg, kt + 1, len, rs);               // in flight during this tile's MFMAs
      if (threadIdx.x < TKEYS && kpm && (kt + 1) * TKEYS + (int)threadIdx.x < len) km_n = kpm[sl.row0 + (kt + 1) * TKEYS + threadIdx.x];
    }
    lds_only_barrier();
    if (!active) continue;
#pragma unroll 1
    for (int g = 0; g < NGRP; ++g) {
      const int flag = __builtin_amdgcn_readfirstlane(kflag[sidx * NGRP + g]);
      if (flag == 2) continue;                         // every key masked or beyond the slate: P = 0, the reference stays
      key_group<DROP, PL>(slot + g * GRPB, kbias + sidx * TKEYS + 32 * g, flag != 0, fo, w, drop, kt * TKEYS + 32 * g, half);
    }
  }
  if (!active) return;
  // scratch: the slot that does NOT hold the last tile -- its tenant, tile nkt - 2, lies behind barrier nkt - 1, which this wave has
  // passed; nothing is staged any more
  f32x4* scratch = reinterpret_cast<f32x4*>(smem + (((nkt - 1) & (NSLOT - 1)) ^ 1) * SLOTB + wave * 4096);
  const float lt = sum_across_halves(w.l);
  const float inv = (lt > 0.f) ? 1.0f / lt : 0.f;
  store_rows1(o + sl.row0 * ors + (size_t)sl.head * dk, q0, len, dk, ors, w.o[0], inv, scratch);
  const int qrow = q0 + (lane & 31);
  if (half == 0 && qrow < len) lse[((size_t)sl.b * h + sl.head) * sl.Lmax + qrow] = (lt > 0.f) ? (w.m + log2f(lt)) * kLn2 : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------
// backward (header: BACKWARD).  Both kernels: workgroup (slate * h + head, row block of 128); wave w owns rows 128 blockIdx.y + 32 w ..
// ------------------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t SMEM_DKDV = (size_t)NSLOT * SLOTB + NSLOT * 3 * TKEYS * sizeof(float);      // + lse, delta, row seed per slot

// the staging of two streamed operands with row strides of their own (Q: rs, dO: ors) -- stager_init / stager_gload otherwise
__device__ __forceinline__ void stager_init2(Stager& st, const float* __restrict__ xb, int xrs, const float* __restrict__ yb, int yrs, int dk) {
  const int chunk = threadIdx.x & 3, c = chunk * 8;
  st.row = threadIdx.x >> 2;
  st.ca = c < dk;
  st.cb = c + 4 < dk;
  st.kp = xb + (size_t)st.row * xrs + (st.ca ? c : 0);
  st.vp = yb + (size_t)st.row * yrs + (st.ca ? c : 0);
  st.dst = narrow_off(st.row, chunk);
}
__device__ __forceinline__ void stager_gload2(Stager& st, int tile, int len, int xrs, int yrs) {
#pragma unroll
  for (int j = 0; j < NPOS; ++j) {
    const bool ok = tile * TKEYS + st.row + 64 * (j & 1) < len;
    const float* p = (j < 2 ? st.kp : st.vp) + ((size_t)tile * TKEYS + 64 * (j & 1)) * (j < 2 ? xrs : yrs);
    st.a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    st.b[j] = st.a[j];
    if (ok && st.ca) st.a[j] = *reinterpret_cast<const float4*>(p);
    if (ok && st.cb) st.b[j] = *reinterpret_cast<const float4*>(p + 4);
  }
}

// group_offsets() with the transposed reads moved from the second plane pair of a slot to the first
__device__ __forceinline__ GroupOffsets first_pair(GroupOffsets f) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    f.v[u][0][0] -= 2 * PLANEB;
    f.v[u][0][1] -= 2 * PLANEB;
  }
  return f;
}

// the wave's dO fragments (q_fragments_stepwise, unscaled) and delta = <dO row, O row>, summed in fp32 over the unsplit values of
// both halves
__device__ __forceinline__ float do_fragments(bf16x8 (&dh)[KS], bf16x8 (&dl)[KS], const float* __restrict__ dob, const float* __restrict__ ob,
                                              int q0, int len, int dk, int ors) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
  const bool rok = q0 + l31 < len;
  const size_t ro = (size_t)(rok ? q0 + l31 : 0) * ors;                        // (row 0 exists)
  float del = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
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

// what a wave of the dQ kernel carries across the key loop for its query block
struct DqBlock {
  bf16x8 qh[KS], ql[KS], dh[KS], dl[KS];
  f32x16 dq[1];                           // dQ^T[d][query] in the accumulator layout
  float lse, del;                         // lse log2 e and delta of query l31
  uint32_t drow;
};

// One 32-key group at `gs` (its K hi plane; V: + 2 PLANEB) against the wave's query block: S^T = K Q^T and dP^T = V dO^T come out of
// two row-wise contractions in the accumulator layout [key = rowmap(r, half)][query = l31], dS is formed there, and it is the B operand
// of dQ^T[d][query] += K^T[d][key] dS^T[key][query], whose A fragments are transposed reads of K (`fk`): dS never moves between lanes.
template <bool DROP, bool PL>
__device__ __forceinline__ void dq_group(const unsigned char* gs, const float* kb, bool biased, const GroupOffsets& fo, const GroupOffsets& fk,
                                         DqBlock& w, float scale, const DropCfg& drop, int key0, int half) {
  f32x16 s = score_chain<KS, PL>(gs, fo.k, PLANEB, w.qh, w.ql);
  if (biased) {                                     // (wave-uniform) a masked or out-of-range key in this group
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(kb + 4 * half + 8 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[4 * g + e] += b4[e];
    }
  }
  const f32x16 dp = score_chain<KS, PL>(gs + 2 * PLANEB, fo.k, PLANEB, w.dh, w.dl);      // (before the dropout mask)
  f32x16 ds;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float p = fast_exp2(s[r] - w.lse);
    const float keep = DROP ? drop_scale_rk(drop, w.drow, key0 + rowmap(r, half)) : 1.0f;
    ds[r] = p * (dp[r] * keep - w.del) * scale;
  }
  value_chain<1, PL>(gs, fk.v, PLANEB, ds, w.dq);
}

// what a wave of the dK/dV kernel carries across the query loop for its key block
struct DkvBlock {
  bf16x8 kh[KS], kl[KS], vh[KS], vl[KS];
  f32x16 dk[1], dv[1];                    // dK^T[d][key], dV^T[d][key] in the accumulator layout
  float kbias;                            // of key l31: -inf for a masked or out-of-range key, else 0
};

// One 32-query group at `gs` (its Q hi plane; dO: + 2 PLANEB) against the wave's key block: S = Q K^T and dP = dO V^T in the
// accumulator layout [query = rowmap(r, half)][key = l31], P keep and dS in one pass over the group's statistics at `lse_g`, `del_g`,
// `seed_g`, then dV^T += dO^T (P keep) (transposed reads of dO: `fo`) and dK^T += Q^T dS (transposed reads of Q: `fq`).
template <bool DROP, bool PL>
__device__ __forceinline__ void dkdv_group(const unsigned char* gs, const float* lse_g, const float* del_g, const uint32_t* seed_g,
                                           const GroupOffsets& fo, const GroupOffsets& fq, DkvBlock& w, float scale, const DropCfg& drop, int key,
                                           int half) {
  const f32x16 s = score_chain<KS, PL>(gs, fo.k, PLANEB, w.kh, w.kl);
  const f32x16 dp = score_chain<KS, PL>(gs + 2 * PLANEB, fo.k, PLANEB, w.vh, w.vl);
  f32x16 pd, ds;
#pragma unroll
  for (int g = 0; g < 4; ++g) {                                                // queries 8 g + 4 half + 0..3 = rowmap(4 g + e, half)
    const int at = 4 * half + 8 * g;
    const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_g + at), d4 = *reinterpret_cast<const f32x4*>(del_g + at);
    u32x4 s4 = {0u, 0u, 0u, 0u};
    if (DROP) s4 = *reinterpret_cast<const u32x4*>(seed_g + at);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p = fast_exp2(s[4 * g + e] + w.kbias - l4[e]);
      const float keep = DROP ? drop_scale_rk(drop, s4[e], key) : 1.0f;
      pd[4 * g + e] = p * keep;
      ds[4 * g + e] = p * (dp[4 * g + e] * keep - d4[e]) * scale;
    }
  }
  value_chain<1, PL>(gs, fo.v, PLANEB, pd, w.dv);
  value_chain<1, PL>(gs, fq.v, PLANEB, ds, w.dk);
}

}  // namespace

template <bool DROP, bool PL>
__global__ void __launch_bounds__(NTHREAD) __attribute__((amdgpu_waves_per_eu(2, 2))) ltrx_mha_bwd_narrow_dq_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const uint8_t* __restrict__ kpm,
    const float* __restrict__ o, const float* __restrict__ dout, const float* __restrict__ lse, float* __restrict__ delta, int L, int h, int dk,
    int rs, int ors, float* __restrict__ dq, int drs, float scale, DropCfg drop, const uint32_t* __restrict__ drop_step,
    const int* __restrict__ cu, const int* __restrict__ order) {
  extern __shared__ __attribute__((aligned(256))) unsigned char smem[];      // slot: K hi, K lo, V hi, V lo (the forward's)
  float* kbias = reinterpret_cast<float*>(smem + NSLOT * SLOTB);         // [slot][128]: -inf for a masked or out-of-range key, else 0
  int* kflag = reinterpret_cast<int*>(kbias + NSLOT * TKEYS);            // [slot][group]: 0 no such key, 1 some, 2 all 32
  if (DROP && drop_step) drop.seed ^= drop_step[0] * 0x9E3779B9u;
  const Slate sl = which_slate(blockIdx.x, L, h, cu, order);
  const int len = sl.len;
  if ((int)(blockIdx.y * QBLK) >= len) return;         // whole workgroup beyond this slate (uniform: before any barrier)
  const int lane = threadIdx.x & 63, half = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t head0 = sl.row0 * rs + (size_t)sl.head * dk, ohead0 = sl.row0 * ors + (size_t)sl.head * dk;
  Stager sg;
  stager_init(sg, k + head0, v + head0, dk, rs);
  stager_gload(sg, 0, len, rs);
  uint8_t km_n = 0;                                    // threads 0-127: padding-mask byte of key 128 kt + threadIdx.x of the tile being staged
  if (threadIdx.x < TKEYS && kpm && (int)threadIdx.x < len) km_n = kpm[sl.row0 + threadIdx.x];
  const int q0 = blockIdx.y * QBLK + wave * 32;
  const bool active = q0 < len;                        // (inactive waves still stage and take every barrier)
  DqBlock w;
  q_fragments_stepwise(w.qh, w.ql, q + head0, q0, len, dk, rs, scale * kLog2e);
  w.del = do_fragments(w.dh, w.dl, dout + ohead0, o + ohead0, q0, len, dk, ors);
  const int qrow = q0 + (lane & 31);
  const size_t stat = (size_t)sl.bh * sl.Lmax + qrow;
  w.lse = (qrow < len) ? lse[stat] * kLog2e : 0.f;
  if (half == 0 && qrow < len) delta[stat] = w.del;
  zero_acc<1>(w.dq);
  w.drow = DROP ? drop_row_seed(drop, sl.bh, sl.Lmax, qrow) : 0u;
  const GroupOffsets fo = group_offsets();
  const GroupOffsets fk = first_pair(fo);
  const int nkt = (len + TKEYS - 1) / TKEYS;
  for (int kt = 0; kt < nkt; ++kt) {
    const int sidx = kt & (NSLOT - 1);
    unsigned char* slot = smem + sidx * SLOTB;
    stager_sstore<PL>(sg, slot);
    if (threadIdx.x < TKEYS) {                         // waves 0 and 1: lane i of wave w holds key 64 w + i, groups 2 w and 2 w + 1
      const bool off = kt * TKEYS + (int)threadIdx.x >= len || km_n;
      kbias[sidx * TKEYS + threadIdx.x] = off ? -INFINITY : 0.f;
      const uint64_t offs = __builtin_amdgcn_ballot_w64(off);
      if (lane < 2) {
        const uint32_t g32 = (uint32_t)(offs >> (32 * lane));
        kflag[sidx * NGRP + 2 * wave + lane] = g32 == 0u ? 0 : (g32 == 0xffffffffu ? 2 : 1);
      }
    }
    if (kt + 1 < nkt) {
      stager_gload(sg, kt + 1, len, rs);               // in flight during this tile's MFMAs
      if (threadIdx.x < TKEYS && kpm && (kt + 1) * TKEYS + (int)threadIdx.x < len) km_n = kpm[sl.row0 + (kt + 1) * TKEYS + threadIdx.x];
    }
    lds_only_barrier();
    if (!active) continue;
#pragma unroll 1
    for (int g = 0; g < NGRP; ++g) {
      const int flag = __builtin_amdgcn_readfirstlane(kflag[sidx * NGRP + g]);
      if (flag == 2) continue;                         // every key masked or beyond the slate: P = 0, dS = 0
      dq_group<DROP, PL>(slot + g * GRPB, kbias + sidx * TKEYS + 32 * g, flag != 0, fo, fk, w, scale, drop, kt * TKEYS + 32 * g, half);
    }
  }
  if (!active) return;
  f32x4* scratch = reinterpret_cast<f32x4*>(smem + (((nkt - 1) & (NSLOT - 1)) ^ 1) * SLOTB + wave * 4096);      // (as the forward)
  store_rows1(dq + sl.row0 * drs + (size_t)sl.head * dk, q0, len, dk, drs, w.dq[0], 1.0f, scratch);
}

template <bool DROP, bool PL>
__global__ void __launch_bounds__(NTHREAD) __attribute__((amdgpu_waves_per_eu(2, 2))) ltrx_mha_bwd_narrow_dkdv_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const uint8_t* __restrict__ kpm,
    const float* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta, int L, int h, int dk, int rs, int ors,
    float* __restrict__ dkout, float* __restrict__ dvout, int drs, float scale, DropCfg drop, const uint32_t* __restrict__ drop_step,
    const int* __restrict__ cu, const int* __restrict__ order) {
  extern __shared__ __attribute__((aligned(256))) unsigned char smem[];      // slot: Q hi, Q lo, dO hi, dO lo
  float* lse_t = reinterpret_cast<float*>(smem + NSLOT * SLOTB);         // [slot][128]: lse log2 e of the tile's queries, +inf beyond the slate
  float* del_t = lse_t + NSLOT * TKEYS;                                  // [slot][128]: delta
  uint32_t* seed_t = reinterpret_cast<uint32_t*>(del_t + NSLOT * TKEYS); // [slot][128]: dropout row seed (DROP)
  if (DROP && drop_step) drop.seed ^= drop_step[0] * 0x9E3779B9u;
  const Slate sl = which_slate(blockIdx.x, L, h, cu, order);
  const int len = sl.len;
  if ((int)(blockIdx.y * QBLK) >= len) return;         // whole workgroup beyond this slate (uniform: before any barrier)
  const int lane = threadIdx.x & 63, half = lane >> 5, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t head0 = sl.row0 * rs + (size_t)sl.head * dk, ohead0 = sl.row0 * ors + (size_t)sl.head * dk;
  const size_t stat0 = (size_t)sl.bh * sl.Lmax;
  Stager sg;
  stager_init2(sg, q + head0, rs, dout + ohead0, ors, dk);
  stager_gload2(sg, 0, len, rs, ors);
  float lse_n = INFINITY, del_n = 0.f;                 // threads 0-127: statistics of query 128 qt + threadIdx.x of the tile being staged
  if (threadIdx.x < TKEYS && (int)threadIdx.x < len) {
    lse_n = lse[stat0 + threadIdx.x] * kLog2e;
    del_n = delta[stat0 + threadIdx.x];
  }
  const int k0 = blockIdx.y * QBLK + wave * 32;
  const bool active = k0 < len;                        // (inactive waves still stage and take every barrier)
  DkvBlock w;
  q_fragments_stepwise(w.kh, w.kl, k + head0, k0, len, dk, rs, scale * kLog2e);      // (K enters only S here)
  q_fragments_stepwise(w.vh, w.vl, v + head0, k0, len, dk, rs, 1.0f);
  const int key = k0 + (lane & 31);
  w.kbias = (key >= len || (kpm && kpm[sl.row0 + key])) ? -INFINITY : 0.f;
  // a wave whose 32 keys are all off has P = 0 everywhere: it stages, takes the barriers and stores its exact zeros without the products
  const bool live = active && __builtin_amdgcn_ballot_w64(w.kbias == 0.f) != 0;
  zero_acc<1>(w.dk);
  zero_acc<1>(w.dv);
  const GroupOffsets fo = group_offsets();             // row-wise reads of either pair; transposed reads of dO
  const GroupOffsets fq = first_pair(fo);              // transposed reads of Q
  const int nqt = (len + TKEYS - 1) / TKEYS;
  for (int qt = 0; qt < nqt; ++qt) {
    const int sidx = qt & (NSLOT - 1);
    unsigned char* slot = smem + sidx * SLOTB;
    stager_sstore<PL>(sg, slot);
    if (threadIdx.x < TKEYS) {
      lse_t[sidx * TKEYS + threadIdx.x] = lse_n;
      del_t[sidx * TKEYS + threadIdx.x] = del_n;
      if (DROP) seed_t[sidx * TKEYS + threadIdx.x] = drop_row_seed(drop, sl.bh, sl.Lmax, qt * TKEYS + threadIdx.x);
    }
    if (qt + 1 < nqt) {
      stager_gload2(sg, qt + 1, len, rs, ors);         // in flight during this tile's MFMAs
      if (threadIdx.x < TKEYS) {
        const int qn = (qt + 1) * TKEYS + threadIdx.x;
        lse_n = INFINITY;
        del_n = 0.f;
        if (qn < len) {
          lse_n = lse[stat0 + qn] * kLog2e;
          del_n = delta[stat0 + qn];
        }
      }
    }
    lds_only_barrier();
    if (!live) continue;
    // the group flag of this kernel is a comparison: a query group at or beyond the slate's length is skipped, and queries are not
    // masked, so no other group is
    const int ng = min(NGRP, (len - qt * TKEYS + 31) / 32);
#pragma unroll 1
    for (int g = 0; g < ng; ++g) {
      const int at = sidx * TKEYS + 32 * g;
      dkdv_group<DROP, PL>(slot + g * GRPB, lse_t + at, del_t + at, seed_t + at, fo, fq, w, scale, drop, key, half);
    }
  }
  if (!active) return;
  // the free slot, as in the forward; the wave's 4 KB are used twice, one store_rows1 after the other
  f32x4* scratch = reinterpret_cast<f32x4*>(smem + (((nqt - 1) & (NSLOT - 1)) ^ 1) * SLOTB + wave * 4096);
  store_rows1(dkout + sl.row0 * drs + (size_t)sl.head * dk, k0, len, dk, drs, w.dk[0], 1.0f, scratch);
  store_rows1(dvout + sl.row0 * drs + (size_t)sl.head * dk, k0, len, dk, drs, w.dv[0], 1.0f, scratch);
}

// ------------------------------------------------------------------------------------------------------------------
// host side (the C entry points ltrx_mha_fwd_narrow / ltrx_mha_bwd_narrow live next to ltrx_mha_fwd / ltrx_mha_bwd in ltrx_mha.hip
// and share their argument checks)
// ------------------------------------------------------------------------------------------------------------------
extern "C" int ltrx_mha_narrow_fits(int L, int d_k) {
  return (L > 0 && (L + QBLK - 1) / QBLK <= 65535 && d_k > 0 && d_k <= 32 && d_k % 4 == 0) ? 1 : 0;
}

int ltrx_mha_fwd_narrow_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, int B, int L, int h, int dk, int rs, float* o,
                               int ors, float* lse, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order,
                               bool plain, hipStream_t s) {
  static std::atomic<uint64_t> attr_done{0};
  const int arc = ltrx_allow_dynamic_lds(attr_done, {{ltrx_mha_fwd_narrow_kernel<false, false>, SMEM}, {ltrx_mha_fwd_narrow_kernel<true, false>, SMEM},
                                                     {ltrx_mha_fwd_narrow_kernel<false, true>, SMEM}, {ltrx_mha_fwd_narrow_kernel<true, true>, SMEM}});
  if (arc != LTRX_OK) return arc;
  const DropCfg drop = ltrx_make_drop(p_drop, seed);
  const float scale = 1.0f / sqrtf((float)dk);
  const dim3 grid(B * h, (L + QBLK - 1) / QBLK);
#define LTRX_NARROW(D_, P_)                                                                                                             \
  hipLaunchKernelGGL((ltrx_mha_fwd_narrow_kernel<D_, P_>), grid, dim3(NTHREAD), SMEM, s, q, k, v, kpm, L, h, dk, rs, o, ors, lse, scale, drop, \
                     seed_step, cu, order)
  if (drop.thresh != 0u) {
    if (plain) LTRX_NARROW(true, true); else LTRX_NARROW(true, false);
  } else {
    if (plain) LTRX_NARROW(false, true); else LTRX_NARROW(false, false);
  }
#undef LTRX_NARROW
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}

// the backward: the dQ kernel (which also writes delta[B, h, L] into `delta`), then the dK/dV kernel on the same stream
int ltrx_mha_bwd_narrow_launch(const float* q, const float* k, const float* v, const uint8_t* kpm, const float* o, const float* dout,
                               const float* lse, int B, int L, int h, int dk, int rs, int ors, float* dq, float* dkk, float* dv, int drs,
                               float* delta, float p_drop, uint32_t seed, const uint32_t* seed_step, const int* cu, const int* order, bool plain,
                               hipStream_t s) {
  static std::atomic<uint64_t> attr_done{0};
  const int arc = ltrx_allow_dynamic_lds(
      attr_done, {{ltrx_mha_bwd_narrow_dq_kernel<false, false>, SMEM}, {ltrx_mha_bwd_narrow_dq_kernel<true, false>, SMEM},
                  {ltrx_mha_bwd_narrow_dq_kernel<false, true>, SMEM}, {ltrx_mha_bwd_narrow_dq_kernel<true, true>, SMEM},
                  {ltrx_mha_bwd_narrow_dkdv_kernel<false, false>, SMEM_DKDV}, {ltrx_mha_bwd_narrow_dkdv_kernel<true, false>, SMEM_DKDV},
                  {ltrx_mha_bwd_narrow_dkdv_kernel<false, true>, SMEM_DKDV}, {ltrx_mha_bwd_narrow_dkdv_kernel<true, true>, SMEM_DKDV}});
  if (arc != LTRX_OK) return arc;
  const DropCfg drop = ltrx_make_drop(p_drop, seed);
  const float scale = 1.0f / sqrtf((float)dk);
  const dim3 grid(B * h, (L + QBLK - 1) / QBLK);
#define LTRX_NARROW_DQ(D_, P_)                                                                                                            \
  hipLaunchKernelGGL((ltrx_mha_bwd_narrow_dq_kernel<D_, P_>), grid, dim3(NTHREAD), SMEM, s, q, k, v, kpm, o, dout, lse, delta, L, h, dk, rs, ors, \
                     dq, drs, scale, drop, seed_step, cu, order)
#define LTRX_NARROW_DKDV(D_, P_)                                                                                                          \
  hipLaunchKernelGGL((ltrx_mha_bwd_narrow_dkdv_kernel<D_, P_>), grid, dim3(NTHREAD), SMEM_DKDV, s, q, k, v, kpm, dout, lse, delta, L, h, dk, rs, \
                     ors, dkk, dv, drs, scale, drop, seed_step, cu, order)
  if (drop.thresh != 0u) {
    if (plain) LTRX_NARROW_DQ(true, true); else LTRX_NARROW_DQ(true, false);
  } else {
    if (plain) LTRX_NARROW_DQ(false, true); else LTRX_NARROW_DQ(false, false);
  }
  LTRX_LAUNCH_CHECK();
  if (drop.thresh != 0u) {
    if (plain) LTRX_NARROW_DKDV(true, true); else LTRX_NARROW_DKDV(true, false);
  } else {
    if (plain) LTRX_NARROW_DKDV(false, true); else LTRX_NARROW_DKDV(false, false);
  }
#undef LTRX_NARROW_DQ
#undef LTRX_NARROW_DKDV
  LTRX_LAUNCH_CHECK();
  return LTRX_OK;
}
