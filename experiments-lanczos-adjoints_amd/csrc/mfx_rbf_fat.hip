// libmfx: the matrix-core Gram matvec (3 x f16 split) as ONE wave per SIMD -- "fat waves", gfx950.
//   W[i][b] = s * sum_j K(x_i, x_j) V[j][b] + noise V[i][b]   (util/gp_util.py:160-176,225-226,536-541 of the reference)
//
// Why (round-3 measurements): with two waves per SIMD -- the same-program kernel k_rbf_h3_packed as well as
// the producer / consumer split (round 3; tools/experiments/pc_matvec/) -- the matrix pipe idles a third of the time: a wave's MFMA and another wave's
// VALU instruction compete for the SIMD's one vector issue port, and neither wave can see the other's schedule.  ONE wave that
// owns the SIMD can: tools/valu_mix_bench.hip runs 14 MFMAs plus the whole exp / hi-lo split chain of a 32 x 32 block in 470
// cycles (452 for the MFMAs alone) when every VALU instruction is placed behind a chosen MFMA so that
//   * no MFMA gap carries more than ~24 issue cycles of VALU work (v_exp_f32 = 8, the others 4) and at most two v_exp,
//   * no instruction follows its producer within one gap (exp -> cvt hi -> fma_mix -> cvt lo, one gap apart each),
// against 532 for the "pair by pair" order of the h3 kernels.  That placement is the table kSplit below.
//
// Shapes: RBF, d <= 16 (two distance MFMAs per block for d <= 8, three for d = 9 .. 12 -- BASELINE config 2 has d = 9 --, four for d = 13 .. 16),
// any number of vectors.
// Geometry: 256-thread workgroups = 4 waves x 128 rows (four 32-row blocks mi) x 64 probes; 512 registers per lane: 128
// accumulators + 128 chain masters (kChainTiles) live in the accumulation registers, the rest in VGPRs.  A 64-column tile is
// 8 blocks (jb, mi); per block 12 contraction MFMAs, 2 distance MFMAs (for the block after next) and 48 VALU instructions.
// The block pipeline runs ACROSS tiles (no per-tile prologue): during block b the wave contracts K_b, splits K_{b+1} (its last
// two pairs finish in the first gaps of block b + 1, before the MFMAs that read them) and computes the distances of K_{b+2}.
// Tile images (pre-packed by k_pack_tiles, LDS-DMA): two buffers; everything a tile contributes is in registers after its
// fifth block, so ONE barrier per tile (behind block 4: "tile t + 1 has landed, tile t's buffer is free") is all the
// synchronisation there is, and the request for tile t + 2 (made in block 5) has a whole tile to land.
#include <type_traits>

#include "mfx_internal.h"
#include "mfx_rbf_common.h"

namespace mfx {

// MFMA slots of a block and the placement of the split chain behind them, by the number NB of 32-probe blocks of a chunk.
//   NB = 2 (33..64 vectors): 14 slots -- 0-9 contraction c0-c9, 10 distance d0, 11 c10, 12 d1, 13 c11;
//   NB = 1 (<= 32 vectors):   8 slots -- c0 c1 c2 d0 c3 d1 c4 c5 (the distances two contraction MFMAs before the block ends: their
//                             first reader, a v_exp behind slot 0 of the next block, then follows three more MFMAs).
// Table entry = slot + kSlots * lag: lag 1 = in the NEXT block (only pairs of the second k-step, whose consumers come later in
// that block).  Steps of the chain of a pair of entries (2p, 2p + 1):  e: v_exp_f32 of one entry;  h: hi pair = v_cvt_pk_f16_f32;
// m: lo half = f16(k - hi) written straight into its half of the packed lo register (v_fma_mixlo_f16 for the even entry, then
// v_fma_mixhi_f16 for the odd one: 40 VALU instructions per block instead of 48 with v_fma_mix_f32 x 2 + v_cvt_pk; bit-identical).
//   NB = 2: issue cycles per slot (exp 8, others 4) 16 12 16 12 16 20 16 16 16 16 20 16 16 16 -- under the ~24 that hide behind an
//           MFMA, and no step follows its producer within one slot;
//   NB = 1: the same 40 instructions behind 8 MFMAs: 28 issue cycles in EVERY slot (pair p: both exps behind slot p, hi p + 1,
//           mixlo p + 2, mixhi p + 3) -- the block is VALU-bound (~290 cycles against 256 of matrix pipe), evenly.
struct FatSplit {
  int e[16], h[8], m[16];
};
// The chain tables by chunk width; the slot ORDER by chunk width and by the number NKD of distance MFMAs of a block
// (NKD = 2: d <= 8; NKD = 3: d = 9 .. 12 -- BASELINE config 2 has d = 9; NKD = 4: d = 13 .. 16).  With every further distance MFMA a block has one more slot and the
// tables stay as they are: an entry >= kSlots still means "in the next block", one slot later than before -- every consumer
// (the contraction MFMAs of k-step 1) still comes later.
constexpr FatSplit kFatSplit2 = {{0, 1, 2, 3, 4, 5, 5, 6, 7, 8, 9, 10, 10, 11, 12, 13},
                                 {2, 4, 6, 7, 9, 11, 12, 14},
                                 {3, 4, 5, 6, 7, 8, 8, 9, 10, 11, 12, 13, 13, 14, 15, 16}};
constexpr FatSplit kFatSplit1 = {{0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7},
                                 {1, 2, 3, 4, 5, 6, 7, 8},
                                 {2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10}};
template <int NB, int NKD>
struct FatPlan;
template <>
struct FatPlan<2, 2> {
  static constexpr int kSlots = 14;
  static constexpr FatSplit kSplit = kFatSplit2;
  // slot -> distance step q (or -1), slot -> contraction MFMA m (or -1), contraction MFMA -> slot
  static constexpr int dist_q(int slot) { return slot == 10 ? 0 : (slot == 12 ? 1 : -1); }
  static constexpr int contr_m(int slot) { return slot < 10 ? slot : (slot == 11 ? 10 : (slot == 13 ? 11 : -1)); }
  static constexpr int slot_of(int m) { return m < 10 ? m : (m == 10 ? 11 : 13); }
};
template <>
struct FatPlan<1, 2> {
  static constexpr int kSlots = 8;
  static constexpr FatSplit kSplit = kFatSplit1;
  static constexpr int dist_q(int slot) { return slot == 3 ? 0 : (slot == 5 ? 1 : -1); }
  static constexpr int contr_m(int slot) { return slot < 3 ? slot : (slot == 4 ? 3 : (slot >= 6 ? slot - 2 : -1)); }
  static constexpr int slot_of(int m) { return m < 3 ? m : (m == 3 ? 4 : m + 2); }
};
// NKD = 3, 64 vectors: 15 slots -- c0-c8, d0, c9, d1, c10, d2, c11 (the last distance MFMA again two MFMAs before the first v_exp on its block)
template <>
struct FatPlan<2, 3> {
  static constexpr int kSlots = 15;
  static constexpr FatSplit kSplit = kFatSplit2;
  static constexpr int dist_q(int slot) { return slot == 9 ? 0 : (slot == 11 ? 1 : (slot == 13 ? 2 : -1)); }
  static constexpr int contr_m(int slot) { return slot < 9 ? slot : (slot == 10 ? 9 : (slot == 12 ? 10 : (slot == 14 ? 11 : -1))); }
  static constexpr int slot_of(int m) { return m < 9 ? m : (m == 9 ? 10 : (m == 10 ? 12 : 14)); }
};
// NKD = 3, <= 32 vectors: 9 slots -- c0 c1 d0 c2 d1 c3 d2 c4 c5
template <>
struct FatPlan<1, 3> {
  static constexpr int kSlots = 9;
  static constexpr FatSplit kSplit = kFatSplit1;
  static constexpr int dist_q(int slot) { return slot == 2 ? 0 : (slot == 4 ? 1 : (slot == 6 ? 2 : -1)); }
  static constexpr int contr_m(int slot) { return slot < 2 ? slot : (slot == 3 ? 2 : (slot == 5 ? 3 : (slot >= 7 ? slot - 3 : -1))); }
  static constexpr int slot_of(int m) { return m < 2 ? m : (m == 2 ? 3 : (m == 3 ? 5 : m + 3)); }
};

// NKD = 4 (d = 13 .. 16), 64 vectors: 16 slots -- c0-c7, d0, c8, d1, c9, d2, c10, d3, c11;  <= 32 vectors: 10 slots -- c0 d0 c1 d1 c2 d2 c3 d3 c4 c5
template <>
struct FatPlan<2, 4> {
  static constexpr int kSlots = 16;
  static constexpr FatSplit kSplit = kFatSplit2;
  static constexpr int dist_q(int slot) { return (slot >= 8 && slot <= 14 && (slot & 1) == 0) ? (slot - 8) / 2 : -1; }
  static constexpr int contr_m(int slot) { return slot < 8 ? slot : ((slot & 1) ? 8 + (slot - 9) / 2 : -1); }
  static constexpr int slot_of(int m) { return m < 8 ? m : 9 + 2 * (m - 8); }
};
template <>
struct FatPlan<1, 4> {
  static constexpr int kSlots = 10;
  static constexpr FatSplit kSplit = kFatSplit1;
  static constexpr int dist_q(int slot) { return (slot >= 1 && slot <= 7 && (slot & 1) == 1) ? (slot - 1) / 2 : -1; }
  static constexpr int contr_m(int slot) { return slot == 0 ? 0 : (slot <= 6 && (slot & 1) == 0 ? slot / 2 : (slot >= 8 ? slot - 4 : -1)); }
  static constexpr int slot_of(int m) { return m == 0 ? 0 : (m <= 3 ? 2 * m : m + 4); }
};

template <int DPAD, int NB>
struct FatSmem {
  static constexpr int KD = DPAD + 2;
  static constexpr int NKD = (3 * KD + 15) / 16;
  static constexpr int AROW = NKD * 16 + 8;
  static constexpr int kABytes = 64 * AROW * 2;  // column operand of a tile (k_pack_tiles' pka)
  static constexpr int kVRow = NB * 32 * 16;      // one image row: the 16-B packs of the chunk's NB * 32 probes
  static constexpr int kVBytes = 2 * 8 * kVRow;   // probe image of a tile: 8 hi rows, then 8 lo rows
  static constexpr int kTile = kABytes + kVBytes;
  static constexpr int kTotal = 2 * kTile;
  static_assert(kABytes % 1024 == 0, "tile images are whole 1-KiB DMA pieces");
};

template <int DPAD, bool VEC4, int NB>
__global__ __launch_bounds__(256, 1) void k_rbf_fat_apply(const float* __restrict__ xs, const float* __restrict__ sq, int64_t n,
                                                          const float* __restrict__ outputscale, const float* __restrict__ noise,
                                                          const float* __restrict__ vscale, const float* __restrict__ x,
                                                          int64_t ldx, float* __restrict__ y, int64_t ldy, int64_t p,
                                                          const uintx4* __restrict__ pkv, const uintx4* __restrict__ pka,
                                                          float* __restrict__ part, const int* __restrict__ rangeflag,
                                                          int64_t ldpart, int64_t row0, int64_t rend) {
  if (rangeflag && *rangeflag != 0) return;  // f16 range guard: the fp32-distance launch queued behind this one does the work
  using S = FatSmem<DPAD, NB>;
  constexpr int KD = S::KD, NKD = S::NKD, AROW = S::AROW;
  static_assert(NKD >= 2 && NKD <= 4, "two to four distance MFMAs per block (d <= 16)");
  using Plan = FatPlan<NB, NKD>;
  constexpr int kSlots = Plan::kSlots;
  extern __shared__ __attribute__((aligned(16))) char fat_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  const int64_t i_wave = row0 + (int64_t)blockIdx.x * 512 + wid * 128;
  const int64_t b0 = (int64_t)blockIdx.y * (NB * 32);
  const int64_t ntile_all = (n + 63) / 64;
  // gridDim.z > 1: column split (rbf_split_count): this workgroup sweeps tiles [t_first, t_first + ntl)
  const int64_t t_first = ntile_all * blockIdx.z / gridDim.z;
  const int ntl = (int)(ntile_all * (blockIdx.z + 1) / gridDim.z - t_first);

  // an "a"-constrained operand keeps the function from being marked amdgpu-no-agpr: the contraction MFMAs are then selected in
  // their AGPR form and the 256 accumulator / master registers do not compete with the VGPR working set
  float agpr_seed = 0.f;
  asm volatile("; accumulators in AGPRs" : "+a"(agpr_seed));

  // LDS-DMA of local tile tl into buffer tl & 1: wave w copies the 1-KiB pieces w, w + 4, ... ([A image | V image])
  auto issue_tile_dma = [&](int tl) {
    const char* asrc = reinterpret_cast<const char*>(pka) + (t_first + tl) * (int64_t)S::kABytes;
    const char* vsrc = reinterpret_cast<const char*>(pkv) + ((int64_t)blockIdx.y * ntile_all + t_first + tl) * S::kVBytes;
    char* dst = fat_smem + (tl & 1) * S::kTile;
#pragma unroll
    for (int c = 0; c < (S::kABytes / 1024 + 3) / 4; ++c) {
      const int piece = wid + 4 * c;
      if (piece < S::kABytes / 1024) glds16(asrc + piece * 1024 + lane * 16, dst + piece * 1024);
    }
#pragma unroll
    for (int c = 0; c < S::kVBytes / 4096; ++c) glds16(vsrc + (wid + 4 * c) * 1024 + lane * 16, dst + S::kABytes + (wid + 4 * c) * 1024);
    static_assert(S::kVBytes % 4096 == 0, "a whole number of probe-image pieces per wave");
  };
  if (0 < ntl) issue_tile_dma(0);
  if (1 < ntl) issue_tile_dma(1);

  // B operand of the distance product, resident: the f16 image [Bh | Bl | Bh | 0] of [x_i, 1, |x_i|^2], negated for the odd row
  // blocks (with the columns' sign -- odd column blocks are packed negated -- block (jb, mi) yields (-1)^(jb + mi) t: the f16 MFMA's
  // rounding bias enters K with alternating sign)
  half8 bih[4][NKD];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    int64_t i = i_wave + mi * 32 + l31;
    if (i >= rend) i = rend - 1;
    if (i < row0) i = row0;
#pragma unroll
    for (int q = 0; q < NKD; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int slot = q * 16 + lhi * 8 + e;
        const int comp = slot / KD, kk = slot % KD;
        float v = 0.f;
        if (comp < 3) v = (kk < DPAD) ? xs[i * DPAD + kk] : (kk == DPAD ? 1.f : sq[i]);
        float hi, lo;
        split_hi_lo(v, hi, lo);
        const float w = comp == 1 ? lo : hi;
        bih[mi][q][e] = (_Float16)((mi & 1) ? -w : w);
      }
  }
  // each fragment becomes ONE 128-bit accumulation-register tuple here, once: the distance MFMAs below take their operands as "a"
  // tuples, and a fragment the allocator keeps in four scattered registers is copied into place in front of every one of them
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int q = 0; q < NKD; ++q) asm volatile("" : "+a"(bih[mi][q]));
  floatx16 acc[4][NB], mst[4][NB];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc[mi][nb][r] = 0.f;
        mst[mi][nb][r] = 0.f;
      }
  acc[0][0][0] = agpr_seed;

  // ---- fragment reads ---------------------------------------------------------------------------------------------------------
  auto read_a = [&](half8 (&a)[NKD], int buf, int jb) {  // column operand of a 32-column block: the distance MFMAs' A fragments
    const _Float16* img = reinterpret_cast<const _Float16*>(fat_smem + buf * S::kTile);
#pragma unroll
    for (int q = 0; q < NKD; ++q) a[q] = *reinterpret_cast<const half8*>(img + (jb * 32 + l31) * AROW + q * 16 + lhi * 8);
  };
  auto read_v1 = [&](half8& v, int buf, int jb, int s, int nb, int hl) {  // one probe fragment (k-step s, probe block nb, hi / lo)
    const int row = (jb * 2 + s) * 2 + lhi;
    v = *reinterpret_cast<const half8*>(fat_smem + buf * S::kTile + S::kABytes + hl * (8 * S::kVRow) + row * S::kVRow + (nb * 32 + l31) * 16);
  };
  // ---- the distance MFMAs: asm, because their 16 results must land in VGPRs with a literal-zero addend while the function's
  //      intrinsic MFMAs are in AGPR form.  The compiler does not see an MFMA there, so the wait states between the MFMA's
  //      write and the first VALU read are kept by construction: the first v_exp on a distance block follows at least two more
  //      MFMAs of this wave (it owns the SIMD's matrix pipe: >= 64 cycles). -----------------------------------------------------
  auto dist_step = [&](floatx16& kd, const half8& a, const half8& b, const bool first) {
    // (A / B operands in accumulation registers: the row operand lives there for good and the column operand is read from LDS
    //  straight into them, so neither takes part in the VGPR working set)
    // No wait states are inserted for an MFMA the compiler cannot see: the operands must be IN PLACE, not copied there (v_accvgpr_mov)
    // in front of the asm -- measured as wrong K blocks when the allocator kept bih scattered.  bih is pinned as tuples above, the
    // column operand arrives by ds_read_b128 (s_waitcnt is data-flow, the compiler keeps that); tests/test_gpu_matvec_kernels.py
    // checks every block position of a tile against the oracle.
    if (first) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(kd) : "a"(a), "a"(b));
    else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(kd) : "a"(a), "a"(b));
  };
  // ---- one micro-step of the split chain of a distance block, in place: t = 0 exp2 of entry i; 1 hi = f16 of pair i; 2 entry i
  //      minus its hi; 3 lo = f16 of pair i.  Register r of the block <-> column (r & 3) + 8 (r >> 2) + 4 lhi; the pair (2p, 2p + 1)
  //      is one packed register of the A fragment of k-step p >> 2. --------------------------------------------------------------
  auto split_op = [&](floatx16& w, half8 (&ah)[2], half8 (&al)[2], unsigned (&lopk)[8], const int t, const int i, const bool neg) {
    if (t == 0) {
      w[i] = __builtin_amdgcn_exp2f(neg ? -w[i] : w[i]);
    } else if (t == 1) {
      const half2v h = {(_Float16)w[2 * i], (_Float16)w[2 * i + 1]};  // one v_cvt_pk_f16_f32, round to nearest
      ah[i >> 2][(i & 3) * 2] = h[0];
      ah[i >> 2][(i & 3) * 2 + 1] = h[1];
    } else {
      const int pr = i >> 1;
      const half2v h = {ah[pr >> 2][(pr & 3) * 2], ah[pr >> 2][(pr & 3) * 2 + 1]};
      const unsigned hb = __builtin_bit_cast(unsigned, h);
      if ((i & 1) == 0) {
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lopk[pr]) : "v"(hb), "v"(w[i]));
      } else {
        asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lopk[pr]) : "v"(hb), "v"(w[i]));
        const half2v l = __builtin_bit_cast(half2v, lopk[pr]);
        al[pr >> 2][(pr & 3) * 2] = l[0];
        al[pr >> 2][(pr & 3) * 2 + 1] = l[1];
      }
    }
  };
  // all micro-steps of the table that fall behind MFMA slot `slot` (lag 0: on the next block's data, lag 1: on this block's)
  auto split_slot = [&](const int slot, const int lag, floatx16& w, half8 (&ah)[2], half8 (&al)[2], unsigned (&lopk)[8], const bool neg) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (Plan::kSplit.e[i] == slot + kSlots * lag) split_op(w, ah, al, lopk, 0, i, neg);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (Plan::kSplit.h[i] == slot + kSlots * lag) split_op(w, ah, al, lopk, 1, i, neg);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (Plan::kSplit.m[i] == slot + kSlots * lag) split_op(w, ah, al, lopk, 2, i, neg);
  };

  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): my pieces of tiles 0 and 1
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // ---- pipeline state.  Blocks are numbered along the sweep: block = 8 tile + 4 jb + mi. --------------------------------------
  // distance blocks: current (its last pairs still being split), next (being split), next but one.  Three roles, eight blocks per tile:
  // with three buffers that change roles by moves, the tile loop's back edge carries a rotation by 8 mod 3 = 2 positions (~6 v_mov per
  // block, 12 % of the VALU instructions of the VALU-bound <= 32-vector form).  There (registers to spare: 304 of 512) the buffers are a ring
  // of FOUR indexed by the block number -- 4 divides 8, every index is static, no move; with 64 vectors (all 512 registers in use, VALU
  // hidden behind the MFMAs) the three buffers stay.
  constexpr bool kRing4 = NB == 1;
  floatx16 wr[kRing4 ? 4 : 3];
#define MFX_WC(blk) wr[kRing4 ? ((blk) & 3) : 0]
#define MFX_WN(blk) wr[kRing4 ? (((blk) + 1) & 3) : 1]
#define MFX_WD(blk) wr[kRing4 ? (((blk) + 2) & 3) : 2]
  half8 ahc[2], alc[2], ahn[2], aln[2];   // A fragments (hi, lo) x k-step of the current and of the next block
  unsigned lpc[8], lpn[8];                 // packed lo pairs in the making (between the mixlo and the mixhi step)
  half8 vf[2][NB][2];           // probe fragments of the current column block [k-step][probe block][hi / lo]
  half8 ajs[2][NKD];            // column operand of a column block, by parity
  // prologue (once per sweep, not per tile): blocks 0 and 1 by hand
  read_a(ajs[0], 0, 0);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int hl = 0; hl < 2; ++hl) read_v1(vf[s][nb][hl], 0, 0, s, nb, hl);
#pragma unroll
  for (int q = 0; q < NKD; ++q) dist_step(MFX_WC(0), ajs[0][q], bih[0][q], q == 0);
#pragma unroll
  for (int q = 0; q < NKD; ++q) dist_step(MFX_WN(0), ajs[0][q], bih[1][q], q == 0);
  asm volatile("" : "+v"(MFX_WC(0)));  // ties the first reader of wc behind the last of these MFMAs (two MFMAs after the one that wrote wc)
  // block 0's split as far as the table places it before a block boundary (its lag-1 steps run in the loop, like every block's)
#pragma unroll
  for (int slot = 0; slot < kSlots; ++slot) split_slot(slot, 0, MFX_WC(0), ahc, alc, lpc, false);

  const float sc = outputscale[0];
  int tl = 0;
  for (; tl < ntl; ++tl) {
    const int buf = tl & 1;
    if (tl > 0 && (tl % kChainTiles) == 0) {  // chain fold: masters += accumulators, accumulators restart from zero
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            mst[mi][nb][r] += acc[mi][nb][r];
            acc[mi][nb][r] = 0.f;
          }
    }
#pragma unroll
    for (int blk = 0; blk < 8; ++blk) {
      const int jb = blk >> 2, mi = blk & 3;
      // block blk + 1 (being split: wn -> ahn / aln) and block blk + 2 (distances: wd); both may lie in the next tile
      const int blk1 = (blk + 1) & 7, blk2 = (blk + 2) & 7;
      const int jb2 = blk2 >> 2, mi2 = blk2 & 3;
      const bool neg_c = ((jb + mi) & 1) != 0, neg_n = (((blk1 >> 2) + (blk1 & 3)) & 1) != 0;
      if (blk == 5 && tl + 2 < ntl) issue_tile_dma(tl + 2);  // (this tile's buffer has been dead since the barrier behind block 4)
      // Invariant at this point: (ahc, alc) hold K_blk except for the table's lag-1 steps (still to run on wc); wn holds the
      // distances of block blk + 1, untouched; ajs[jb2 & 1] holds the column operand that block blk + 2 needs from its first
      // distance slot on.
#pragma unroll
      for (int slot = 0; slot < kSlots; ++slot) {
        __builtin_amdgcn_sched_barrier(0);
        if (Plan::dist_q(slot) >= 0) {
          const int q = Plan::dist_q(slot);
          dist_step(MFX_WD(blk), ajs[jb2 & 1][q], bih[mi2][q], q == 0);
        } else {
          const int m = Plan::contr_m(slot);
          const int s = m / (3 * NB), nb = (m / 3) % NB, w = m % 3;
          acc[mi][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w == 2 ? alc[s] : ahc[s], w == 1 ? vf[s][nb][1] : vf[s][nb][0],
                                                               acc[mi][nb], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        split_slot(slot, 1, MFX_WC(blk), ahc, alc, lpc, neg_c);  // this block's late pairs first (their consumers are a few slots away)
        split_slot(slot, 0, MFX_WN(blk), ahn, aln, lpn, neg_n);
        // fragment reads, one per gap: the probe fragments of the NEXT column block during this one (blocks mi = 1, 2: sixteen
        // reads... eight per block), the column operand of the column block after that in block mi = 1
        if (mi == 1 && slot < NKD) {
          // ajs of column block c + 1 is needed by the distances of block (c + 1, mi 0), issued in block (c, mi 2)
          ajs[(jb + 1) & 1][slot] = *reinterpret_cast<const half8*>(reinterpret_cast<const _Float16*>(fat_smem + (jb == 1 ? buf ^ 1 : buf) * S::kTile) +
                                                                   (((jb + 1) & 1) * 32 + l31) * AROW + slot * 16 + lhi * 8);
        }
        if (mi == 3) {
          // the probe fragments of the next column block roll in behind the last MFMA of this column block that reads the
          // register they replace: fragment (s, nb, hi) is read by MFMAs 3 NB s + 3 nb and + 2, (s, nb, lo) by + 1
#pragma unroll
          for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
              for (int hl = 0; hl < 2; ++hl) {
                const int mlast = 3 * NB * s + 3 * nb + (hl ? 1 : 2);
                if (Plan::slot_of(mlast) == slot) read_v1(vf[s][nb][hl], jb == 1 ? buf ^ 1 : buf, (jb + 1) & 1, s, nb, hl);
              }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (blk == 4) {
        // tile tl + 1 (requested a tile ago) has landed for everybody, and everybody is done with this tile's buffer: its last reads
        // -- the probe fragments of column block 1, rolled in during block 3 -- were consumed by the MFMAs of this block
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      // rotate: next -> current, next-but-one -> next
      ahc[0] = ahn[0]; ahc[1] = ahn[1];
      alc[0] = aln[0]; alc[1] = aln[1];
      if constexpr (!kRing4) {
        wr[0] = wr[1];
        wr[1] = wr[2];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) lpc[q] = lpn[q];
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // no LDS-DMA of mine is left in flight
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][nb][r] += mst[mi][nb][r];
  const float nz = gridDim.z > 1 ? 0.f : noise[0];
  float* yout = gridDim.z > 1 ? part + (int64_t)blockIdx.z * p * ldpart : y;
  const int64_t ldo = gridDim.z > 1 ? ldpart : ldy;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int64_t b = b0 + nb * 32 + l31;
      if (b >= p) continue;
      const float sb = sc * vscale[2 * b + 1] * (1.f / 32768.f);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t i = i_wave + mi * 32 + 8 * g + 4 * lhi;
        if (VEC4 && i + 3 < rend) {
          const float4 xv = *reinterpret_cast<const float4*>(x + b * ldx + i);
          float4 o;
          o.x = fmaf(sb, acc[mi][nb][4 * g + 0], nz * xv.x);
          o.y = fmaf(sb, acc[mi][nb][4 * g + 1], nz * xv.y);
          o.z = fmaf(sb, acc[mi][nb][4 * g + 2], nz * xv.z);
          o.w = fmaf(sb, acc[mi][nb][4 * g + 3], nz * xv.w);
          *reinterpret_cast<float4*>(yout + b * ldo + (i - row0)) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (i + e < rend) yout[b * ldo + (i - row0) + e] = fmaf(sb, acc[mi][nb][4 * g + e], nz * x[b * ldx + i + e]);
        }
      }
    }
}

#undef MFX_WC
#undef MFX_WN
#undef MFX_WD

// ================================================================================================================================
// The same sweep on v_mfma_f32_16x16x32_f16: RBF, d <= 8 (3 (d + 2) <= 32: the whole distance product is ONE k-step), chunks of 64
// vectors.  Same flops per cycle as 32x32x16, but the dense 16x16x32 stream holds a higher clock (tools/unit16_bench.hip; the
// parameter-gradient GEMM made the same move).
//
// Unit of work = 16 rows x 32 columns (a column block jb of the tile) x 64 probes: 2 distance MFMAs, 8 kernel entries per lane
// (8 v_exp, 4 v_cvt_pk, 4 v_fma_mixlo + 4 v_fma_mixhi), 12 contraction MFMAs = 4 probe groups of 16 x {hi hi, hi lo, lo hi}.  An
// MFMA holds the vector issue for 8 of its 16 cycles.  kFat16Tab is the model's table T0: one v_exp behind each of slots 0-7, two
// short instructions behind each of slots 8-13.  At the nominal costs (v_exp 8, the others 4) that is 8 issue
// cycles per slot; tools/slot_cost_bench.hip prices v_fma_mixlo/hi at 8, by which slots 10-13 carry 16.  The alternative with ONE
// mix per slot (exps two per slot behind 0-3, hi pairs behind 4-5, the lo halves behind 6-13) was measured on the kernel and is
// slower: 5.49 against 5.38 ms per launch (profiles/r13a_matvec_16x16x32/kernel_ab.log), so T0 stays.  The table fixes the ORDER of
// the chain between the MFMAs, not every position: the compiler sinks the four v_cvt_pk behind slot 9 (they are not pinned).
// A tile = 16 units u = 8 jb + it (it: the wave's eight 16-row tiles).  During unit u the wave contracts K_u, runs the whole split
// chain of K_{u+1} and computes the distances of K_{u+2}; the pipeline runs across tiles like k_rbf_fat_apply's.
//
// Everything the accuracy rests on is k_rbf_fat_apply's: the tile images of k_pack_tiles (bit for bit), two LDS buffers and one
// barrier per tile, the chain folds, the alternating block signs (32-row block it >> 1 negated when odd; odd column blocks are
// packed negated), the column split, the range guard, row blocks and the epilogue.  What differs is the order of the sums inside a
// tile: one k-step of 32 columns where the 32x32x16 form has two of 16, and one k-step of the distance product instead of two.
//
// How the images map onto the 16x16x32 fragments (lane = 16 g + c, g = 0..3):
//   * a 16-B pack of the probe image holds, for image row (jb, s, h) and one probe, the columns 16 s + 8 (e >> 2) + 4 h + (e & 3),
//     e = 0..7.  The contraction's B fragment of lane (g, probe c) is the pack of row 4 jb + g, i.e. (s, h) = (g >> 1, g & 1).
//   * so lane g must hold the kernel entries of exactly those columns: distance MFMA c2 (c2 = 0, 1) takes as its 16 A rows the
//     columns 16 (m >> 3) + 8 c2 + (m & 7), m = 0..15 ({0..7, 16..23}, then {8..15, 24..31}); its results land on lane (g, row c) in
//     registers r = 0..3 as columns 16 (g >> 1) + 8 c2 + 4 (g & 1) + r: entry e = 4 c2 + r of the pack order, no lane movement.
//   * accumulator (it, pg): lane (g, c) holds rows 16 it + 4 g + r, r = 0..3, of probe 16 pg + c: one float4 of the output.
struct Fat16Tab {
  int e[8], h[4], m[8];
};
// slot (0..13 of the unit BEFORE) behind which each micro-step of a unit's chain runs: exps behind slots 0-7, the four hi pairs
// behind 8 and 9, the lo halves behind 10-13; no step follows its producer within one slot
constexpr Fat16Tab kFat16Tab = {{0, 1, 2, 3, 4, 5, 6, 7}, {8, 8, 9, 9}, {10, 11, 10, 11, 12, 13, 12, 13}};

template <int DPAD, bool VEC4>
__global__ __launch_bounds__(256, 1) void k_rbf_fat_apply16(const float* __restrict__ xs, const float* __restrict__ sq, int64_t n,
                                                            const float* __restrict__ outputscale, const float* __restrict__ noise,
                                                            const float* __restrict__ vscale, const float* __restrict__ x,
                                                            int64_t ldx, float* __restrict__ y, int64_t ldy, int64_t p,
                                                            const uintx4* __restrict__ pkv, const uintx4* __restrict__ pka,
                                                            float* __restrict__ part, const int* __restrict__ rangeflag,
                                                            int64_t ldpart, int64_t row0, int64_t rend) {
  if (rangeflag && *rangeflag != 0) return;  // f16 range guard: the fp32-distance launch queued behind this one does the work
  using S = FatSmem<DPAD, 2>;
  constexpr int KD = S::KD, AROW = S::AROW;
  static_assert(S::NKD == 2 && 3 * KD <= 32, "the distance product is one k-step of 32");
  constexpr Fat16Tab T = kFat16Tab;
  extern __shared__ __attribute__((aligned(16))) char fat_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lg = lane >> 4;
  const int64_t i_wave = row0 + (int64_t)blockIdx.x * 512 + wid * 128;
  const int64_t b0 = (int64_t)blockIdx.y * 64;
  const int64_t ntile_all = (n + 63) / 64;
  const int64_t t_first = ntile_all * blockIdx.z / gridDim.z;
  const int ntl = (int)(ntile_all * (blockIdx.z + 1) / gridDim.z - t_first);

  // (as in k_rbf_fat_apply: keeps the contraction MFMAs in their AGPR form)
  float agpr_seed = 0.f;
  asm volatile("; accumulators in AGPRs" : "+a"(agpr_seed));

  auto issue_tile_dma = [&](int tl, int b) {  // tile tl into LDS buffer b = tl & 1 (a constant at every call)
    const char* asrc = reinterpret_cast<const char*>(pka) + (t_first + tl) * (int64_t)S::kABytes;
    const char* vsrc = reinterpret_cast<const char*>(pkv) + ((int64_t)blockIdx.y * ntile_all + t_first + tl) * S::kVBytes;
    char* dst = fat_smem + b * S::kTile;
#pragma unroll
    for (int c = 0; c < (S::kABytes / 1024 + 3) / 4; ++c) {
      const int piece = wid + 4 * c;
      if (piece < S::kABytes / 1024) glds16(asrc + piece * 1024 + lane * 16, dst + piece * 1024);
    }
#pragma unroll
    for (int c = 0; c < S::kVBytes / 4096; ++c) glds16(vsrc + (wid + 4 * c) * 1024 + lane * 16, dst + S::kABytes + (wid + 4 * c) * 1024);
  };
  if (0 < ntl) issue_tile_dma(0, 0);
  if (1 < ntl) issue_tile_dma(1, 1);

  // row operand of the distance product, resident: [Bh | Bl | Bh | 0] of [x_i, 1, |x_i|^2] along k = 8 g + e, negated for odd 32-row blocks
  half8 bi[8];
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    int64_t i = i_wave + it * 16 + l15;
    if (i >= rend) i = rend - 1;
    if (i < row0) i = row0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int slot = lg * 8 + e;
      const int comp = slot / KD, kk = slot % KD;
      float v = 0.f;
      if (comp < 3) v = (kk < DPAD) ? xs[i * DPAD + kk] : (kk == DPAD ? 1.f : sq[i]);
      float hi, lo;
      split_hi_lo(v, hi, lo);
      const float w = comp == 1 ? lo : hi;
      bi[it][e] = (_Float16)(((it >> 1) & 1) ? -w : w);
    }
  }
  floatx4 acc[8][4], mst[8][4];
#pragma unroll
  for (int it = 0; it < 8; ++it)
#pragma unroll
    for (int pg = 0; pg < 4; ++pg)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[it][pg][r] = 0.f;
        mst[it][pg][r] = 0.f;
      }
  acc[0][0][0] = agpr_seed;

  // ---- fragment reads ---------------------------------------------------------------------------------------------------------
  auto read_a = [&](half8& a, int buf, int jb, int c2) {  // A rows of distance MFMA c2 of column block jb
    const _Float16* img = reinterpret_cast<const _Float16*>(fat_smem + buf * S::kTile);
    a = *reinterpret_cast<const half8*>(img + (jb * 32 + 16 * (l15 >> 3) + 8 * c2 + (l15 & 7)) * AROW + lg * 8);
  };
  auto read_v = [&](half8& v, int buf, int jb, int f) {  // probe fragment f = 2 pg + (lo ? 1 : 0) of column block jb
    v = *reinterpret_cast<const half8*>(fat_smem + buf * S::kTile + S::kABytes + (f & 1) * (8 * S::kVRow) + (jb * 4 + lg) * S::kVRow +
                                        ((f >> 1) * 16 + l15) * 16);
  };
  // ---- the distance MFMA: asm, because its four results must land in VGPRs (v_exp cannot read an accumulation register) while the
  //      function's intrinsic MFMAs are in AGPR form.  The compiler sees no MFMA here and pads nothing:
  //      * operands: the row operand is written once before the sweep; the column operand arrives by ds_read_b128, whose s_waitcnt is
  //        data flow and kept.  What is left is a register copy of either that the allocator might put in front of the statement
  //        (VALU write -> MFMA A/B read: 2 wait states).  PAD = true opens the statement with an s_nop 1 against it: the prologue and
  //        the peeled tile, which run once.  The two-tile loop body takes PAD = false: nothing is carried across its back edge by
  //        a copy, its code holds no v_mov / v_accvgpr_* at all (read from the code object of all four instances), and
  //        the instruction in front of the statement is then the chain step of the slot before it (a v_exp behind slot 7, the
  //        v_cvt_pk behind slot 9), which writes the ring entry or the hi fragment of unit u + 1 -- never an operand of this MFMA.
  //      * result: a v_mfma_f32_16x16x32_f16 is an 8-pass MFMA; a VALU instruction may read its VGPR result 12 wait states after
  //        issue at the earliest.  The first reader of distance MFMA c2 (slot 8 + 2 c2 of unit u) is the v_exp behind slot 4 c2 of unit
  //        u + 1: six (c2 = 0) or eight (c2 = 1) MFMAs of this wave -- which owns the SIMD's matrix pipe, 16 cycles each -- and the
  //        chain's VALU instructions behind them (one per slot 0-7, two per slot 8-13) lie between: >= 12 instructions by the
  //        MFMAs and the table alone, and >= 96 cycles, with or without the s_nop.  The prologue has no such schedule and pads by hand.
  auto dist16 = [&](floatx4& kd, const half8& a, const half8& b, auto pad) {
    if constexpr (decltype(pad)::value) asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(kd) : "v"(a), "v"(b));
    else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(kd) : "v"(a), "v"(b));
  };
  // ---- one micro-step of the split chain of a unit (entries w[c2][r], e = 4 c2 + r): t = 0 exp2 of entry i; 1 hi pair i; 2 lo half
  //      of entry i (v_fma_mixlo / mixhi straight into its half of the packed lo register, as k_rbf_fat_apply) -------------------------
  auto chain = [&](floatx4 (&w)[2], half8& ah, half8& al, unsigned (&lp)[4], const int t, const int i, const bool neg) {
    if (t == 0) {
      w[i >> 2][i & 3] = __builtin_amdgcn_exp2f(neg ? -w[i >> 2][i & 3] : w[i >> 2][i & 3]);
    } else if (t == 1) {
      const half2v h = {(_Float16)w[i >> 1][(2 * i) & 3], (_Float16)w[i >> 1][(2 * i + 1) & 3]};  // one v_cvt_pk_f16_f32
      ah[2 * i] = h[0];
      ah[2 * i + 1] = h[1];
    } else {
      const int pr = i >> 1;
      const half2v h = {ah[2 * pr], ah[2 * pr + 1]};
      const unsigned hb = __builtin_bit_cast(unsigned, h);
      if ((i & 1) == 0) {
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lp[pr]) : "v"(hb), "v"(w[i >> 2][i & 3]));
      } else {
        asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lp[pr]) : "v"(hb), "v"(w[i >> 2][i & 3]));
        const half2v l = __builtin_bit_cast(half2v, lp[pr]);
        al[2 * pr] = l[0];
        al[2 * pr + 1] = l[1];
      }
    }
  };
  auto chain_slot = [&](const int slot, floatx4 (&w)[2], half8& ah, half8& al, unsigned (&lp)[4], const bool neg) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (T.e[i] == slot) chain(w, ah, al, lp, 0, i, neg);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (T.h[i] == slot) chain(w, ah, al, lp, 1, i, neg);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (T.m[i] == slot) chain(w, ah, al, lp, 2, i, neg);
  };

  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): my pieces of tiles 0 and 1
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // ---- pipeline state.  Units are numbered along the sweep: 16 tile + 8 jb + it; everything below is indexed by the unit's number
  //      mod 2 or mod 4 (16 is a multiple of both: every index is static, nothing is moved). -------------------------------------------
  floatx4 wr[4][2];     // distances -> kernel entries of a unit: ring of four (contracting u, splitting u + 1, distances of u + 2)
  half8 ah[2], al[2];   // A fragments (hi, lo) of the unit being contracted and of the next
  unsigned lp[4];       // packed lo pairs between their mixlo and mixhi step
  half8 vf[2][8];       // probe fragments [column block][2 pg + lo]
  half8 aj[2][2];       // column operand [column block][distance MFMA]
  // prologue (once per sweep): the distances of units 0 and 1 and the whole chain of unit 0, by hand
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2) read_a(aj[0][c2], 0, 0, c2);
#pragma unroll
  for (int f = 0; f < 8; ++f) read_v(vf[0][f], 0, 0, f);
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2) dist16(wr[0][c2], aj[0][c2], bi[0], std::true_type{});
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2) dist16(wr[1][c2], aj[0][c2], bi[1], std::true_type{});
  // no MFMA follows here: the 12 wait states (and more) between the last distance MFMA and the first v_exp, by hand
  asm volatile("s_nop 15\n\ts_nop 15" : "+v"(wr[0][0]), "+v"(wr[0][1]), "+v"(wr[1][0]), "+v"(wr[1][1]));
#pragma unroll
  for (int slot = 0; slot < 14; ++slot) chain_slot(slot, wr[0], ah[0], al[0], lp, false);

  const float sc = outputscale[0];
  // One tile, in LDS buffer `buf`.  The tile loop below runs TWO tiles per iteration, the period of the buffer rotation: the buffer
  // is a constant of the code (every LDS offset an immediate) and the loop body ends with every accumulator, fragment and ring entry
  // in the register it started in -- nothing is carried across the back edge by a copy.
  auto tile = [&](auto bc, auto pad, const int tl) {  // pad: the peeled tile (dist16's PAD; the sweep ends behind it)
    constexpr int buf = decltype(bc)::value;
    constexpr bool kLast = decltype(pad)::value;
    auto unit = [&](auto uc) {
      constexpr int u = decltype(uc)::value;
      constexpr int jb = u >> 3, it = u & 7;
      constexpr int u1 = (u + 1) & 15, u2 = (u + 2) & 15;  // the unit being split and the one whose distances are computed (may lie in the next tile)
      constexpr bool neg_n = (((u1 >> 3) + ((u1 & 7) >> 1)) & 1) != 0;
      // the fragments of column block jb ^ 1 roll in during column block jb: this tile's block 1, or the NEXT tile's block 0 (behind the barrier)
      constexpr int nbuf = jb == 1 ? buf ^ 1 : buf;
      if (u == 9 && tl + 2 < ntl) issue_tile_dma(tl + 2, buf);  // (this tile's buffer has been dead since the barrier behind unit 7)
#pragma unroll
      for (int slot = 0; slot < 14; ++slot) {
        __builtin_amdgcn_sched_barrier(0);
        // slots: hi hi of the four probe groups (0-3), hi lo (4-7), distance 0 (8), lo hi 0 (9), distance 1 (10), lo hi 1-3 (11-13): four
        // other accumulators between two MFMAs on the same one, and the lo fragment -- finished last -- is read last
        if (slot == 8 || slot == 10) {
          const int c2 = (slot - 8) / 2;
          // (the peeled tile ends the sweep: no unit 16 or 17 follows.  Their distances must not even be issued: the result of an asm
          //  MFMA lands 8 passes after issue, unseen by the compiler, and a ring entry nobody reads is dead at the statement -- its
          //  registers are handed to the next chain step at once and the late result lands on top of it.  Measured so: the hi
          //  fragment of unit 15 overwritten, NaN in row tile 7 behind every odd tile count.  In the loop body every entry is read.)
          if constexpr (!(kLast && u >= 14)) dist16(wr[(u + 2) & 3][c2], aj[(u2 >> 3) & 1][c2], bi[u2 & 7], pad);
        } else {
          const int m = slot < 8 ? slot : (slot == 9 ? 8 : slot - 2);
          const int w = m / 4, pg = m % 4;
          acc[it][pg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w == 2 ? al[u & 1] : ah[u & 1], w == 1 ? vf[jb][pg * 2 + 1] : vf[jb][pg * 2],
                                                               acc[it][pg], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!(kLast && u == 15)) chain_slot(slot, wr[(u + 1) & 3], ah[(u + 1) & 1], al[(u + 1) & 1], lp, neg_n);
        // fragment reads: one probe fragment of the next column block per unit; its column operand in unit it = 3 (first needed by the
        // distances issued in unit it = 6)
        if (slot == 2) read_v(vf[jb ^ 1][it], nbuf, jb ^ 1, it);
        if (it == 3 && (slot == 4 || slot == 5)) read_a(aj[jb ^ 1][slot - 4], nbuf, jb ^ 1, slot - 4);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (u == 7) {
        // tile tl + 1 (requested a tile ago) has landed for everybody, and everybody is done with this tile's buffer: its last reads
        // -- probe fragment 7 of column block 1 -- were issued behind slot 2 of this unit.  Every read of the next tile comes later.
        __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
    };
    unit(std::integral_constant<int, 0>{});
    unit(std::integral_constant<int, 1>{});
    unit(std::integral_constant<int, 2>{});
    unit(std::integral_constant<int, 3>{});
    unit(std::integral_constant<int, 4>{});
    unit(std::integral_constant<int, 5>{});
    unit(std::integral_constant<int, 6>{});
    unit(std::integral_constant<int, 7>{});
    unit(std::integral_constant<int, 8>{});
    unit(std::integral_constant<int, 9>{});
    unit(std::integral_constant<int, 10>{});
    unit(std::integral_constant<int, 11>{});
    unit(std::integral_constant<int, 12>{});
    unit(std::integral_constant<int, 13>{});
    unit(std::integral_constant<int, 14>{});
    unit(std::integral_constant<int, 15>{});
  };
  // The sweep chain by chain: the fold stands in front of every tile tl > 0 with tl % kChainTiles == 0, between the chains and not in
  // the tile loop, whose only loop-carried values are then the ones a tile itself carries.  A chain is an even number of tiles, so
  // only the sweep's last tile can be left over: it is peeled (it is an even tile: buffer 0), behind its fold if it opens a chain.
  static_assert(kChainTiles % 2 == 0, "a chain is a whole number of two-tile loop bodies");
  for (int t0 = 0; t0 < ntl; t0 += kChainTiles) {
    if (t0 > 0) {  // chain fold: masters += accumulators, accumulators restart from zero
#pragma unroll
      for (int it = 0; it < 8; ++it)
#pragma unroll
        for (int pg = 0; pg < 4; ++pg)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            mst[it][pg][r] += acc[it][pg][r];
            acc[it][pg][r] = 0.f;
          }
    }
    const int t1 = t0 + kChainTiles < ntl ? t0 + kChainTiles : ntl;
    for (int tl = t0; tl + 1 < t1; tl += 2) {
      tile(std::integral_constant<int, 0>{}, std::false_type{}, tl);
      tile(std::integral_constant<int, 1>{}, std::false_type{}, tl + 1);
    }
  }
  if (ntl & 1) tile(std::integral_constant<int, 0>{}, std::true_type{}, ntl - 1);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // no LDS-DMA of mine is left in flight
#pragma unroll
  for (int it = 0; it < 8; ++it)
#pragma unroll
    for (int pg = 0; pg < 4; ++pg)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[it][pg][r] += mst[it][pg][r];
  const float nz = gridDim.z > 1 ? 0.f : noise[0];
  float* yout = gridDim.z > 1 ? part + (int64_t)blockIdx.z * p * ldpart : y;
  const int64_t ldo = gridDim.z > 1 ? ldpart : ldy;
#pragma unroll
  for (int pg = 0; pg < 4; ++pg) {
    const int64_t b = b0 + pg * 16 + l15;
    if (b >= p) continue;
    const float sb = sc * vscale[2 * b + 1] * (1.f / 32768.f);
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int64_t i = i_wave + it * 16 + 4 * lg;
      if (VEC4 && i + 3 < rend) {
        const float4 xv = *reinterpret_cast<const float4*>(x + b * ldx + i);
        float4 o;
        o.x = fmaf(sb, acc[it][pg][0], nz * xv.x);
        o.y = fmaf(sb, acc[it][pg][1], nz * xv.y);
        o.z = fmaf(sb, acc[it][pg][2], nz * xv.z);
        o.w = fmaf(sb, acc[it][pg][3], nz * xv.w);
        *reinterpret_cast<float4*>(yout + b * ldo + (i - row0)) = o;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < rend) yout[b * ldo + (i - row0) + e] = fmaf(sb, acc[it][pg][e], nz * x[b * ldx + i + e]);
      }
    }
  }
}

int rbf_fat_launch(int dpad, int nb, bool vec4, bool wide16, dim3 grid, hipStream_t stream, const RbfMatvecArgs& a) {
  const char* not_built = "fat-wave Gram matvec supports d <= 16 and chunks of 32 or 64 vectors";
  MFX_REQUIRE(nb == 1 || nb == 2, MFX_ERR_UNSUPPORTED, "%s", not_built);
  if (wide16 && nb == 2 && dpad <= 8) {  // the 16x16x32 form: d <= 8, 64-wide chunks
    return with_mfma_dpad<8>(dpad, not_built, [&](auto dc) -> int {
      return with_bool(vec4, [&](auto v4) -> int {
        constexpr int DPAD = decltype(dc)::value;
        k_rbf_fat_apply16<DPAD, decltype(v4)::value><<<grid, 256, FatSmem<DPAD, 2>::kTotal, stream>>>(
            a.xs, a.sq, a.n, a.outputscale, a.noise, a.vscale, a.x, a.ldx, a.y, a.ldy, a.p, static_cast<const uintx4*>(a.pkv),
            static_cast<const uintx4*>(a.pka), a.part, a.rangeflag, a.ldpart, a.row0, a.rend);
        MFX_CHECK_LAUNCH();
        return MFX_OK;
      });
    });
  }
  return with_mfma_dpad<16>(dpad, not_built, [&](auto dc) -> int {
    return with_bool(nb == 2, [&](auto two) -> int {
      return with_bool(vec4, [&](auto v4) -> int {
        constexpr int DPAD = decltype(dc)::value, NB = decltype(two)::value ? 2 : 1;
        k_rbf_fat_apply<DPAD, decltype(v4)::value, NB><<<grid, 256, FatSmem<DPAD, NB>::kTotal, stream>>>(
            a.xs, a.sq, a.n, a.outputscale, a.noise, a.vscale, a.x, a.ldx, a.y, a.ldy, a.p, static_cast<const uintx4*>(a.pkv),
            static_cast<const uintx4*>(a.pka), a.part, a.rangeflag, a.ldpart, a.row0, a.rend);
        MFX_CHECK_LAUNCH();
        return MFX_OK;
      });
    });
  });
}

}  // namespace mfx
