// libmfx: parameter-gradient sweeps of the RBF / Matern Gram operator on the CDNA4 matrix cores (gfx950).
//
//   d/dtheta sum_bt L_bt^T K(theta) R_bt = sum_ij S_ij dK_ij/dtheta,   S = L^T R  (n x n, rank <= batch)
//
// S is a GEMM over the batch of (probe, Lanczos-step) pairs and never leaves the accumulators: the epilogue evaluates K_ij and its
// lengthscale weight (grad_weights) and reduces the tile to (d + 2) numbers per workgroup.  Two GEMMs, in this order in the file:
//   * 3 x f16 split  (rbf_mfma_grad_h, k_rbf_mfma_grad_h): pre-pass k_row_amax / k_global_scale / k_order_rows / k_pack_f16 writes
//     sorted, signed, scaled hi / lo f16 packs; the 256-row GEMM runs on v_mfma_f32_16x16x32_f16;
//   * exact fp32     (rbf_mfma_grad, k_rbf_mfma_grad): 128 x 128 tiles on v_mfma_f32_32x32x2_f32 straight from the fp32 rows.
// rbf_grad_path says which one runs; rbf_grad_h_layout is the split GEMM's workspace.  The two GEMM bodies are separate on purpose
// (different tiles, staging and epilogues).  The Gram matvec lives in mfx_rbf_mfma.hip; the two files share mfx_rbf_common.h only.
#include <stdlib.h>

#include <type_traits>

#include "mfx_internal.h"
#include "mfx_rbf_common.h"

namespace mfx {

// geometry of the parameter-gradient GEMM (both the fp32 and the 3 x f16 variant)
constexpr int kGM = 128, kGN = 128, kGK = 32, kGSplit = 8;
// L2 sharing inside an XCD (split gradient GEMM): the 64 workgroups resident on an XCD form an 8 x 8 patch -- 8 row blocks
// x 8 column sub-ranges -- so every L and every R operand slice is read by 8 workgroups at about the same time (1 fabric
// read + 7 L2 hits).  With one row block per workgroup and a private 1.3 MB L panel re-read for each of its 128 tiles,
// the launch pulled 2.2 TB through the fabric (FETCH_SIZE, L2 hit rate 19 %): it was fabric-bound at 7 TB/s, not MFMA-bound.
constexpr int kGSub = 8;
constexpr int kGLd = kGM + 4;  // padded row of the transposed S tile: conflict-free ds_write_b128

// epilogue of the gradient GEMMs: K_ij / outputscale and the lengthscale weight from the clamped squared distance.
// M52: Matern-5/2 has instances of its own (a fourth runtime branch cost the 256 x 256 split tile 12 B of scratch and the
// padded-64 exact sweep 6 more parked registers); the other three families share one instance and branch on `kind`.
template <bool M52>
__device__ __forceinline__ void grad_weights(int kind, float dist, float& kv, float& wl) {
  if constexpr (M52) {
    const float r = __builtin_amdgcn_sqrtf(5.f * dist + kEpsF32);
    const float e = __builtin_amdgcn_exp2f(-kLog2e * r);
    kv = fmaf(r, fmaf(r, 1.f / 3.f, 1.f), 1.f) * e;
    wl = fmaf(r, 5.f / 3.f, 5.f / 3.f) * e;
  } else if (kind == MFX_KERNEL_RBF) {
    kv = __builtin_amdgcn_exp2f(-0.72134752044448170368f * dist);
    wl = kv;
  } else if (kind == MFX_KERNEL_MATERN32) {
    const float r = __builtin_amdgcn_sqrtf(3.f * dist + kEpsF32);
    const float e = __builtin_amdgcn_exp2f(-kLog2e * r);
    kv = (1.f + r) * e;
    wl = 3.f * e;
  } else {
    const float r = __builtin_amdgcn_sqrtf(dist + kEpsF32);
    const float e = __builtin_amdgcn_exp2f(-kLog2e * r);
    kv = e;
    wl = dist > 0.f ? e / r : 0.f;
  }
}

// ================================================================================================
// Parameter-gradient sweep, 3 x f16 split: S = L^T R on the f16 matrix pipe.
//   pre-pass  k_pack_f16: (batch, n) fp32 rows -> hi/lo f16 packs [kb][i][8] (8 consecutive batch rows of
//             column i = one 16-byte MFMA A/B fragment), scaled by one power of two per operand
//             (global |max| -> 2^14), zero padded to batch % 32 == 0 and n % 128 == 0: the GEMM main loop
//             has no conversions, no bounds checks, fragment loads are plain ds_read_b128;
//   GEMM      same 128 x 128 tiling / epilogue as k_rbf_mfma_grad, 24 f16 MFMAs per 32-row stage instead
//             of 64 fp32 MFMAs at twice the cycles.
// ================================================================================================
__global__ __launch_bounds__(256) void k_row_amax(const float* __restrict__ x, int64_t ldx, int64_t n,
                                                  float* __restrict__ amax) {
  __shared__ float sm[4];
  const int64_t b = blockIdx.x;
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(x[b * ldx + i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) amax[b] = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

// scale[0] = row_scale_of(max_b amax[b]), scale[1] = 1 / scale[0]
__global__ void k_global_scale(const float* __restrict__ amax, int64_t rows, float* __restrict__ scale) {
  __shared__ float sm[256];
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < rows; i += 256) m = fmaxf(m, amax[i]);
  sm[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] = fmaxf(sm[threadIdx.x], sm[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float s = row_scale_of(sm[0]);
    scale[0] = s;
    scale[1] = 1.f / s;
  }
}

// Pseudo-random sign of column i of a packed gradient-GEMM operand (salt: which operand).  Column i of L carries sigma_i,
// column j of R carries tau_j, so the accumulator of S_ij holds sigma_i tau_j S_ij and the epilogue undoes the sign.
// Why: the f16 MFMA's floor bias (see the note above k_rbf_mfma_grad_h) is the SAME sign in every accumulator; with the operands' columns signed
// at random it enters S_ij as -sigma_i tau_j beta ulp -- sign-random over (i, j), uncorrelated with dK_ij/dtheta -- and
// sums like noise (~ |dK|_F) instead of coherently (~ sum_ij dK_ij, n times larger).  Measured: profiles/r02a_*.
__host__ __device__ __forceinline__ bool grad_col_sign(int64_t i, uint32_t salt) {
  uint32_t h = (uint32_t)i * 0x9E3779B1u + salt;
  h ^= h >> 15;
  h *= 0x85EBCA77u;
  h ^= h >> 13;
  h *= 0xC2B2AE3Du;
  return (h >> 31) != 0;
}
constexpr uint32_t kSaltL = 0x51ED270Bu, kSaltR = 0xB5297A4Du;

// ONE product instead of three for the rows that cannot matter, and the rows ORDERED BY SIZE.
// S = sum_b L_b^T R_b does not care in which order the batch rows are summed, and the adjoint states of the last Krylov steps are
// orders of magnitude smaller than those of the first (config 4: row maxima 8.8e3 at step 0, ~2e2 at steps 1-13, < 8 from step 30 on,
// 2e-3 at step 39; the basis rows are unit vectors).  The pre-pass therefore sorts the rows by the bound m_b = |L_b|max |R_b|max,
// largest first (a bitonic sort of <= 8192 keys in LDS, ties by the (step, probe) index: deterministic), and packs them in that order:
//   * the 32 rows that meet in one K = 32 MFMA step have similar magnitudes (what the (step, probe) order of round 2 was for: the
//     f16 MFMA aligns its products to the largest of them and truncates the rest);
//   * the cross products hi lo + lo hi of a row are 2^-11 of its hi hi product.  The TAIL of the sorted order -- the longest run of
//     the smallest rows whose bounds add up to at most 2^-MFX_GRAD_ONE_PRODUCT_LOG2 (default 2^-10) of the sum of ALL bounds -- is
//     multiplied hi hi only: with |lo| <= 2^-11 |x| the two cross terms of a row are at most 2 x 2^-11 m_b = 2^-10 m_b, so what that drops from
//     any S_ij is at most 2^-(10 + 10) = 2^-20 of sum_b m_b even if it all had one sign -- a bound relative to the summed row bounds
//     sum_b |L_b|max |R_b|max, NOT to |S_ij|; what protects the gradient (which cancels to 1e-4 .. 1e-5 of its terms) is measured: the
//     16-probe-set table of profiles/r05b_*.  The three-product sum itself drops terms of that size (lo lo, the MFMA's truncation).  Those stages (from stage n3 on) stage and
//     multiply their hi images only: a third of the MFMAs, half of the L2 -> LDS bytes.  (A per-row cut relative to the largest row
//     would let MANY small rows through that together carry the gradient; measured at config 4: per-row cut 2^-6 -> 4e-4 off.)
// Decided on the device per launch; no row qualifies when the rows are of similar size, and then nothing changes but the order.
// On row shards every rank picks its n3 from the maxima of ITS rows of L: the ranks may run different arithmetic on their tails
// (harmless: each rank's partial sums obey the bound above; the ranks' results are added in fp64 by the estimator's all-reduce).
// Knob: MFX_GRAD_ONE_PRODUCT_LOG2 at build time sets the default (10); the environment variable of the same name, read once per process,
// overrides it at run time -- 0 switches the tail off (every stage three products): the A/B without a rebuild.
#ifndef MFX_GRAD_ONE_PRODUCT_LOG2
#define MFX_GRAD_ONE_PRODUCT_LOG2 10
#endif
static int grad_one_product_log2() {
  static const int v = [] {
    const char* e = getenv("MFX_GRAD_ONE_PRODUCT_LOG2");
    const int x = e ? atoi(e) : MFX_GRAD_ONE_PRODUCT_LOG2;
    return x < 0 ? 0 : (x > 60 ? 60 : x);
  }();
  return v;
}
constexpr int kSortMax = 8192;  // rows the LDS sort takes (64 KB of 64-bit keys); larger batches keep the (step, probe) order, three products
// perm[bt] = source row of packed row bt (-1: a zero row of the padding); tail[0] = n3, the first one-product stage
__global__ __launch_bounds__(1024) void k_order_rows(const float* __restrict__ amaxL, const float* __restrict__ amaxR, int64_t batch,
                                                     int64_t inner, int64_t bpad, int npow2, int one_log2, int* __restrict__ perm,
                                                     int* __restrict__ tail) {
  extern __shared__ unsigned long long keys[];  // (bound bits << 32) | (0xFFFFFFFF - default position): sorted DESCENDING
  const int64_t outer = batch / inner;
  for (int i = threadIdx.x; i < npow2; i += 1024) {
    unsigned long long kv = 0;  // padding: after every real row
    if (i < batch) {
      const int64_t src = inner > 1 ? ((int64_t)i % outer) * inner + (int64_t)i / outer : i;  // default order: (step, probe)
      float m = amaxL[src] * amaxR[src];
      if (!(m >= 0.f) || m > 3.0e38f) m = 3.0e38f;  // NaN / inf rows first: never in the one-product tail
      kv = ((unsigned long long)__float_as_uint(m) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    }
    keys[i] = kv;
  }
  __syncthreads();
  for (int size = 2; size <= npow2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < npow2 / 2; t += 1024) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = keys[lo], b = keys[hi];
        if (desc ? a < b : a > b) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
      __syncthreads();
    }
  for (int64_t bt = threadIdx.x; bt < bpad; bt += 1024) {
    int src = -1;
    if (bt < batch) {
      const int64_t i = 0xFFFFFFFFu - (unsigned)(keys[bt] & 0xFFFFFFFFull);
      src = (int)(inner > 1 ? (i % outer) * inner + i / outer : i);
    }
    perm[bt] = src;
  }
  // the one-product tail: the longest run of the SMALLEST rows whose bounds add up to at most 2^-one_log2 of the sum of all bounds
  // (a row with a NaN / inf bound makes the sum infinite: no tail).  Block-wide: thread t owns `per` consecutive sorted rows; a suffix
  // scan over the threads' partial sums (wave shuffles + 16 wave totals in LDS) gives every thread the mass of the rows behind its
  // own, and the smallest row index whose suffix mass stays within the cut is found with one LDS atomicMin.  (Round 4 had thread 0 sum
  // and scan all <= 8192 keys alone, in front of both pack launches of every sweep.)
  __shared__ double wave_sum[16];
  __shared__ int first_row;
  const int nstage = (int)(bpad / 32);
  if (one_log2 <= 0) {
    if (threadIdx.x == 0) tail[0] = nstage;
    return;
  }
  const int per = npow2 >= 1024 ? npow2 / 1024 : 1;
  const int64_t r0 = (int64_t)threadIdx.x * per, r1 = r0 + per < batch ? r0 + per : batch;
  double mine = 0.0;
  for (int64_t bt = r1 - 1; bt >= r0; --bt) mine += (double)__uint_as_float((unsigned)(keys[bt] >> 32));
  // inclusive suffix sum over the lanes of a wave, then over the waves
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double suf = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_down(suf, off, 64);
    if (lane + off < 64) suf += o;
  }
  if (lane == 0) wave_sum[wv] = suf;
  if (threadIdx.x == 0) first_row = (int)batch;
  __syncthreads();
  double behind = 0.0, total = 0.0;  // mass of the waves behind mine; mass of all rows
  for (int w = 0; w < 16; ++w) {
    total += wave_sum[w];
    if (w > wv) behind += wave_sum[w];
  }
  const double cut = total < 1.0e38 ? ldexp(total, -one_log2) : -1.0;
  double mass = behind + (suf - mine);  // everything behind this thread's rows
  int64_t first = r1;
  for (int64_t bt = r1 - 1; bt >= r0; --bt) {
    const double m = (double)__uint_as_float((unsigned)(keys[bt] >> 32));
    if (mass + m > cut) break;
    mass += m;
    first = bt;
  }
  // rows are sorted by decreasing bound, so "suffix mass <= cut" holds from some row on: the smallest such row over all threads
  if (first < r1) atomicMin(&first_row, (int)first);
  __syncthreads();
  if (threadIdx.x == 0) tail[0] = (int)(((int64_t)first_row + 31) / 32);  // whole stages only
}
__global__ void k_order_default(int64_t batch, int64_t inner, int64_t bpad, int* __restrict__ perm, int* __restrict__ tail) {
  const int64_t bt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t outer = batch / inner;
  if (bt < bpad) perm[bt] = bt < batch ? (int)(inner > 1 ? (bt % outer) * inner + bt / outer : bt) : -1;
  if (bt == 0) tail[0] = (int)(bpad / 32);
}

// hi/lo packs: out[(kb * npad + i) * 8 + q] = piece of (+-) scale * x[perm[8 kb + q]][i], sign per column i = grad_col_sign(i, salt).
// The packed row order is k_order_rows' (by decreasing size).  Why the order matters beyond the one-product tail: the f16 MFMA aligns
// the products of an output element to the largest of them and truncates the others TOWARDS ZERO (tools/mfma_f16_trunc.hip), and the
// adjoint states of different Krylov steps differ by orders of magnitude -- with the caller's (probe, step) order every small product
// lost bits, always in the direction that shrinks its contribution, a sign-symmetric bias that no sign alternation can cancel
// (1.6e-4 / 4.3e-4 gradient error at n = 65536; round 2 packed (step, probe) for that reason, round 4 sorts outright).
__global__ __launch_bounds__(256) void k_pack_f16(const float* __restrict__ x, int64_t ldx, int64_t batch, int64_t n,
                                                  int64_t npad, const float* __restrict__ scale, uint32_t salt,
                                                  const int* __restrict__ perm, _Float16* __restrict__ hi, _Float16* __restrict__ lo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t kb = blockIdx.y;
  if (i >= npad) return;
  float s = scale[0];
  if (grad_col_sign(i, salt)) s = -s;
  half8 h, l;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int64_t src = perm[kb * 8 + q];  // k_order_rows: rows by decreasing size; -1 = a zero row of the padding
    const float v = (src >= 0 && i < n) ? x[src * ldx + i] * s : 0.f;
    float fh, fl;
    split_hi_lo(v, fh, fl);
    h[q] = (_Float16)fh;
    l[q] = (_Float16)fl;
  }
  *reinterpret_cast<half8*>(hi + (kb * npad + i) * 8) = h;
  *reinterpret_cast<half8*>(lo + (kb * npad + i) * 8) = l;
}

// rows per workgroup tile of the split gradient GEMM: 8 waves (4 x 2 of 64 x 64) on ONE staged tile pair -- the same two waves per
// SIMD as two 128 x 128 workgroups, but (256 + 128) instead of 2 x (128 + 128) operand columns through L2 -> LDS per stage
constexpr int kHM = 256;
constexpr int kHLd = kHM + 4;

// NBW = 32-column groups per wave: the workgroup tile is 256 rows x (2 NBW 32) columns, 8 waves as 4 x 2 of 64 x (NBW 32).
//   NBW = 2: 256 x 128 (round 1);  NBW = 4: 256 x 256 -- (256 + 256) instead of 2 x (256 + 128) operand columns through L2 -> LDS
//   per stage and per 256 x 256 of S, i.e. a third less of that traffic.  Its 128 accumulator registers
//   fit since the fp32 master accumulators are gone (see the note on the floor bias below).
// Round 4: the contraction runs on v_mfma_f32_16x16x32_f16 (a wave's 64 x (NBW 32) sub-tile = 4 x 2 NBW blocks of 16 x 16, the same 32 NBW
// accumulator registers): same flops and the same matrix-pipe cycles as on 32x32x16, but the chip holds a HIGHER CLOCK under this shape
// (tools/gradk_bench.hip, the K-loop alone on one box, alternating: 49.1 ms / 1.45 GHz on 32x32x16, 44.6 ms / 1.61 GHz on 16x16x32, both 90 %
// matrix pipe; MI355X_MICROARCH.md 'DVFS give-back' item 7).  One wave per SIMD on 128 x 128 (the round-3 plan) was measured there too and
// is SLOWER (51.9 ms: 88 % pipe with LDS-DMA issued by the computing wave, 82 % with register staging) -- a third fewer fragment bytes from LDS
// buy no clock.  A stage is now 32 batch rows (one K = 32 MFMA step): two 64-KB LDS images instead of a ring of four 16-row ones.
template <int DPAD, int NBW, bool REGEPI = false>
struct GradSmemH {
  static constexpr int TN = 2 * NBW * 32;  // columns of the workgroup tile
  // columns per pass of the LDS epilogue: 128; 64 for DPAD = 32 (16 < d <= 32, round 5), where x_i and x_j of the tile are twice as wide and a
  // 128-column S^T overlay would push the workgroup over the 160 KB of LDS
  static constexpr int GN = DPAD > 16 ? 64 : kGN;
  static constexpr int KQ = (DPAD + 2 + 3) / 4;  // k-steps of the epilogue's distance product (v_mfma_f32_16x16x4_f32)
  union {
    struct {
      _Float16 a_hi[2][4][kHM][8];  // [slot][kb-group within the 32-row stage][i][8]
      _Float16 a_lo[2][4][kHM][8];
      _Float16 b_hi[2][4][TN][8];
      _Float16 b_lo[2][4][TN][8];
    } st;
    float s_t[GN][kHLd];  // S^T of ONE pass of the epilogue
  } u;
  float xi[kHM][DPAD];
  float sqi[kHM];
  float xj[GN][DPAD];
  float sqj[GN];
  float sgj[GN];  // tau_j of the staged columns (+-1)
  float bq[REGEPI ? 4 * KQ : 1][REGEPI ? TN : 1];  // register epilogue: B' = [x_j, 1, |x_j|^2, 0..] of the tile's columns, k-major
  double red[8][DPAD + 2];
};


// The f16 MFMA truncates its internal sum towards -infinity: a bias of a fraction of an ulp per MFMA, invisible in
// any single accumulator but COHERENT across all n^2 accumulators of S, and the gradient sum_ij S_ij dK_ij/dtheta
// cancels to ~1e-4..1e-5 of its terms -- measured as a 0.1-1 % gradient error.  Round 1 cured it with alternating-sign
// K-chunks folded into fp32 master accumulators (64 more registers, 128 VALU instructions per chunk).  The pseudo-random
// column signs of the packed operands (grad_col_sign) do the same job for free: with them and WITHOUT the chunks the C4
// gradient is 9.8e-6 / 3.0e-5 off fp64, without either 2.2e-2 / 5.6e-2 (profiles/r02h_*) -- so the chunks and the master
// accumulators are gone, which is what makes room for the 256 x 256 tile.

template <int DPAD, int NBW, bool REGEPI, bool M52>
__device__ __forceinline__ void rbf_mfma_grad_h_body(const float* __restrict__ xs, const float* __restrict__ sq,
                                                            int64_t n, int64_t npad_l, int64_t npad_r, int ard, int kind,
                                                            const _Float16* __restrict__ Lh, const _Float16* __restrict__ Ll,
                                                            const _Float16* __restrict__ Rh, const _Float16* __restrict__ Rl,
                                                            int64_t nkb /* batch_pad / 8 */, int tiles_per_block,
                                                            uint32_t salt_l, uint32_t salt_r, double* __restrict__ partial,
                                                            int64_t row0, int64_t nrow, const int* __restrict__ one_product) {
  // rows: the nrow points row0 .. of X that the L operand covers (a row shard, or all n); columns: all n points
  using Smem = GradSmemH<DPAD, NBW, REGEPI>;
  constexpr int TN = Smem::TN;
  constexpr int NB16 = 2 * NBW;  // 16-column blocks of a wave's sub-tile
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  Smem& sm = *reinterpret_cast<Smem*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int wm = wid >> 1, wn = wid & 1;
  // blockIdx.x = XCD label (workgroups are dealt to XCDs round-robin in linear order); within an XCD, blockIdx.y
  // enumerates (row block, column sub-range) with the sub-range fastest, see kGSub
  const int64_t i0 = (int64_t)(blockIdx.y / kGSub) * kHM;
  const int64_t ntj = (n + TN - 1) / TN;
  const int64_t tj_begin = ((int64_t)blockIdx.x * kGSub + blockIdx.y % kGSub) * tiles_per_block;
  int64_t tj_end = tj_begin + tiles_per_block;
  if (tj_end > ntj) tj_end = ntj;

  for (int t = tid; t < kHM * DPAD; t += 512) {
    const int64_t g = i0 * DPAD + t;
    (&sm.xi[0][0])[t] = g < nrow * DPAD ? xs[row0 * DPAD + g] : 0.f;
  }
  if (tid < kHM) sm.sqi[tid] = (i0 + tid < nrow) ? sq[row0 + i0 + tid] : 0.f;

  constexpr int NG = REGEPI ? 3 : DPAD + 2;  // register epilogue: (lengthscale, outputscale, noise)
  double gsum[NG];
#pragma unroll
  for (int c = 0; c < NG; ++c) gsum[c] = 0.0;

  // Staging by LDS-DMA, no staging registers: a stage = 4 kb-groups (32 batch rows) x (256 | TN) columns x 16 B per operand image,
  // 1-KiB pieces (one wave-instruction = 64 columns of one kb-group).  Wave w moves, per stage:
  //   L hi and lo: columns 64 (w & 3) .., kb-groups (w >> 2) and (w >> 2) + 2                                  -> 4 pieces
  //   R hi and lo: TN = 256 the same -> 4 pieces;  TN = 128: columns 64 (w & 1) .., kb-group w >> 1             -> 2 pieces
  // Addresses are 32-bit byte offsets from the (scalar) image bases, advanced by one constant per stage.  TWO slots: the stage
  // being read and the next one in flight (requested when the last readers of its slot are done, a whole stage = 3072 matrix-pipe
  // cycles of the SIMD earlier for the lower half of the workgroup, half that for the upper half).
  const int nstage = (int)(nkb / 4);
  const uint32_t stage_bytes_l = (uint32_t)(4 * npad_l * 16), stage_bytes_r = (uint32_t)(4 * npad_r * 16);
  const int lcol = (wid & 3) * 64, lkb = wid >> 2;                          // wave-uniform
  const int rcol = TN == 256 ? (wid & 3) * 64 : (wid & 1) * 64, rkb = TN == 256 ? (wid >> 2) : (wid >> 1);
  const uint32_t offL = (uint32_t)(((int64_t)lkb * npad_l + i0 + lcol + lane) * 16);
  const uint32_t offR0 = (uint32_t)(((int64_t)rkb * npad_r + rcol + lane) * 16);
  const uint32_t kb2_l = (uint32_t)(2 * npad_l * 16), kb2_r = (uint32_t)(2 * npad_r * 16);
  const char* Lhb = reinterpret_cast<const char*>(Lh);
  const char* Llb = reinterpret_cast<const char*>(Ll);
  const char* Rhb = reinterpret_cast<const char*>(Rh);
  const char* Rlb = reinterpret_cast<const char*>(Rl);
  auto issue_stage = [&](uint32_t l_off, uint32_t r_off, int slot, int hi_only) {  // hi_only: a one-product stage (from n3 on: k_order_rows)
    glds16(Lhb + l_off, &sm.u.st.a_hi[slot][lkb][lcol][0]);
    glds16(Lhb + l_off + kb2_l, &sm.u.st.a_hi[slot][lkb + 2][lcol][0]);
    glds16(Rhb + r_off, &sm.u.st.b_hi[slot][rkb][rcol][0]);
    if constexpr (TN == 256) glds16(Rhb + r_off + kb2_r, &sm.u.st.b_hi[slot][rkb + 2][rcol][0]);
    if (!hi_only) {
      glds16(Llb + l_off, &sm.u.st.a_lo[slot][lkb][lcol][0]);
      glds16(Llb + l_off + kb2_l, &sm.u.st.a_lo[slot][lkb + 2][lcol][0]);
      glds16(Rlb + r_off, &sm.u.st.b_lo[slot][rkb][rcol][0]);
      if constexpr (TN == 256) glds16(Rlb + r_off + kb2_r, &sm.u.st.b_lo[slot][rkb + 2][rcol][0]);
    }
  };
  // stages from n3 on are one-product stages (a scalar of the pre-pass, k_order_rows; the same for every workgroup)
  int n3 = one_product[0];
  n3 = n3 < 0 ? 0 : (n3 > nstage ? nstage : n3);
  const int one_first = n3 == 0 ? 1 : 0;

  for (int64_t tj = tj_begin; tj < tj_end; ++tj) {
    const int64_t j0 = tj * TN;
    floatx4 acc[4][NB16];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < NB16; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;

    uint32_t ol = offL, orr = offR0 + (uint32_t)(j0 * 16);
    // (opaque per tile: otherwise the four 64-bit L addresses of a stage, which do not depend on the tile, are hoisted out of the
    //  tile loop and sit in -- or spill from -- registers the K-loop needs)
    asm volatile("" : "+v"(ol));
    if (!REGEPI || tj == tj_begin) {
      __syncthreads();  // previous tile's epilogue reads of the overlaid S^T tile are done
      issue_stage(ol, orr, 0, one_first);
    }  // (REGEPI: stage 0 of this tile was requested before the previous tile's epilogue)
    ol += stage_bytes_l;
    orr += stage_bytes_r;
    // PING-PONG: waves w and w + 4 share a SIMD.  With one barrier per stage all eight waves read their fragments from LDS
    // together (192 KB per stage with the matrix pipe idle) and then queue their MFMAs together.  Here the two
    // halves of the workgroup run half a stage apart: two barriers per stage -- B1 before the fragment reads, B2 before the
    // MFMAs -- and the upper half takes one extra barrier first, so that while one wave of a SIMD is in its MFMA cluster
    // the other one is in its read cluster.  Who needs what by when (A = waves 0-3, B = waves 4-7; barrier
    // numbers in A's count: A.B1(st) = 2 st, A.B2(st) = B.B1(st) = 2 st + 1, B.B2(st) = 2 st + 2):
    //   * A reads stage st between barriers 2 st and 2 st + 1, B between 2 st + 1 and 2 st + 2 (each waits for its reads,
    //     lgkmcnt(0), before its B2);
    //   * the slot of stage st - 1 is therefore free after barrier 2 st: every wave requests stage st + 1 into it after its
    //     B1(st) (A behind barrier 2 st, B behind 2 st + 1);
    //   * stage st + 1 is first read behind barrier 2 st + 2: every wave waits for ITS pieces (vmcnt(0): nothing younger is in
    //     flight) before it ARRIVES there -- A before its B1(st + 1), B before its B2(st);  stage 0 before the first barrier.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    if (wid >= 4) __builtin_amdgcn_s_barrier();  // the half-stage offset of the upper half
    // stages [0, n3): three products; stages [n3, nstage): hi hi only (n3 from k_order_rows).  TWO loops, each with its own straight-line
    // body: with the choice as a branch inside one loop the allocator spilled 140-190 registers around the joins
    auto run_stages = [&](auto one_c, int st_begin, int st_end) {
      constexpr bool ONE = decltype(one_c)::value;
      for (int st = st_begin; st < st_end; ++st) {
        const int slot = st & 1;
        if (wid < 4) __builtin_amdgcn_s_waitcnt(0x0F70);  // (A) my pieces of this stage, requested a stage ago
        __builtin_amdgcn_s_barrier();  // B1
        if (st + 1 < nstage) issue_stage(ol, orr, slot ^ 1, ONE ? 1 : (st + 1 >= n3 ? 1 : 0));
        ol += stage_bytes_l;
        orr += stage_bytes_r;
        half8 ah[4], al[ONE ? 1 : 4], bh[NB16], bl[ONE ? 1 : NB16];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          ah[a] = *reinterpret_cast<const half8*>(&sm.u.st.a_hi[slot][lq][wm * 64 + a * 16 + l15][0]);
          if constexpr (!ONE) al[a] = *reinterpret_cast<const half8*>(&sm.u.st.a_lo[slot][lq][wm * 64 + a * 16 + l15][0]);
        }
#pragma unroll
        for (int b = 0; b < NB16; ++b) {
          bh[b] = *reinterpret_cast<const half8*>(&sm.u.st.b_hi[slot][lq][wn * (NBW * 32) + b * 16 + l15][0]);
          if constexpr (!ONE) bl[b] = *reinterpret_cast<const half8*>(&sm.u.st.b_lo[slot][lq][wn * (NBW * 32) + b * 16 + l15][0]);
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the fragments are in registers
        if (wid >= 4) __builtin_amdgcn_s_waitcnt(0x0F70);  // (B) my pieces of stage st + 1
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();  // B2  (no s_setprio around the MFMA cluster: measured 0.5 % faster without, tools/gradk_bench.hip)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < NB16; ++b) {
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[a], bh[b], acc[a][b], 0, 0, 0);
            if constexpr (!ONE) {
              acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[a], bl[b], acc[a][b], 0, 0, 0);
              acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[a], bh[b], acc[a][b], 0, 0, 0);
            }
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    run_stages(std::false_type{}, 0, n3);
    run_stages(std::true_type{}, n3, nstage);
    if (wid < 4) __builtin_amdgcn_s_barrier();  // the lower half catches up: both halves have taken 2 nstage + 1 barriers
    if constexpr (REGEPI) {
      // Everything below that depends only on the workgroup's rows is invariant over the tile loop; hoisted out of it, it
      // would sit in registers through the K-loop, which has none to spare (measured: 380 B of spills, one reload per stage,
      // +14 % run time; adding an opaque zero does not help -- the compiler hoists the rest of the sum).  The row index itself goes
      // through opaque per-tile copies of the two lane coordinates: nothing that depends on them can leave the tile loop, and
      // only the coordinates themselves (which the K-loop needs anyway) stay live across it.
      int l15_t = l15, lq4_t = 4 * lq;
      asm volatile("" : "+v"(l15_t), "+v"(lq4_t));
      // ---- register epilogue (one lengthscale): the kernel entries are formed IN THE ACCUMULATOR LAYOUT -- the distance block
      //      D = A' B'^T with A' = [-2 x_i, |x_i|^2, 1], B' = [x_j, 1, |x_j|^2] on the fp32 MFMA (v_mfma_f32_16x16x4_f32: lane =
      //      column j, register r <-> row 4 (lane >> 4) + r, exactly like acc) -- so S o dK is 4 elementwise products per block:
      //      no S^T through LDS, no barriers, and the slots are free, so the next tile's first stage is in flight while this runs.
      constexpr int KQ = Smem::KQ;
      // (bq of the previous tile: every wave has passed at least one K-loop barrier since it read it)
      uint32_t taub[NB16];  // tau_j as a sign-bit mask
#pragma unroll
      for (int b = 0; b < NB16; ++b) taub[b] = grad_col_sign(j0 + wn * (NBW * 32) + b * 16 + l15, salt_r) ? 0x80000000u : 0u;
      for (int t = tid; t < TN * 4 * KQ; t += 512) {  // B' of the tile's columns (xs is a few MB: L2), BEFORE the prefetch
        const int col = t % TN, c = t / TN;
        const int64_t j = j0 + col;
        float v = 0.f;
        if (c < DPAD) v = j < n ? xs[j * DPAD + c] : 0.f;
        else if (c == DPAD) v = 1.f;
        else if (c == DPAD + 1) v = j < n ? sq[j] : 0.f;
        sm.bq[c][col] = v;
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): my bq writes have landed (the DMA counter is left alone)
      __builtin_amdgcn_s_barrier();        // every wave is done reading the last stage of this tile, and bq is complete
      if (tj + 1 < tj_end) issue_stage(ol - (uint32_t)(nstage + 1) * stage_bytes_l, offR0 + (uint32_t)((j0 + TN) * 16), 0, one_first);
      const bool diag_tile = (row0 + i0 < j0 + TN) && (j0 < row0 + i0 + kHM);
      float gl = 0.f, gs = 0.f, gn = 0.f;
      // one straight-line copy of the body per (tile meets the diagonal or not): with the diagonal test as a run-time branch inside
      // the 128 unrolled entries the compiler spills.  Per entry FIVE VALU instructions (the two waves of a SIMD run their epilogues
      // side by side, VALU-bound): the distance block comes out of the MFMA already scaled, t = c dist with c = -log2(e) / 2 folded
      // into A'; k = v_exp_f32(t) with the clamp modifier (k <= 1: the reference's max(dist, 0), util/gp_util.py:173, where it matters);
      // sigma_i tau_j undone by ONE v_xor3 with two sign masks; u = s k; sum u; sum u t (= c sum s k dist, unscaled at the end --
      // a distance that is negative by round-off enters as it is, ~1e-7 of one entry).
      auto body = [&](auto diag_c) {
        constexpr bool DIAG = decltype(diag_c)::value;
        int dj[NB16];  // column of block b's lane, relative to the first row of the workgroup's tile
#pragma unroll
        for (int b = 0; b < NB16; ++b) dj[b] = (int)(j0 - (row0 + i0)) + wn * (NBW * 32) + b * 16 + l15_t;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int il = wm * 64 + a * 16 + l15_t;
          float ai[KQ];
#pragma unroll
          for (int sI = 0; sI < KQ; ++sI) {
            const int c = 4 * sI + lq;
            const float v = c < DPAD ? -2.f * sm.xi[il][c < DPAD ? c : 0] : (c == DPAD ? sm.sqi[il] : (c == DPAD + 1 ? 1.f : 0.f));
            ai[sI] = kNegHalfLog2e * v;
          }
          uint32_t sgm[4];  // sigma of the row of register r as a sign-bit mask
          const int row_r0 = (int)i0 + wm * 64 + a * 16 + lq4_t;  // (local rows: < 2^31)
#pragma unroll
          for (int r = 0; r < 4; ++r) sgm[r] = grad_col_sign(row_r0 + r, salt_l) ? 0x80000000u : 0u;
#pragma unroll
          for (int b = 0; b < NB16; ++b) {
            floatx4 D = {0.f, 0.f, 0.f, 0.f};
            // a few distance blocks in flight, not all of them: the first operand of every other block waits (through an opaque
            // move) for the sums of the previous ones -- otherwise the optimiser gathers the MFMAs of all blocks up front
            float a0 = ai[0];
            if ((b & 1) == 0) asm volatile("" : "+v"(a0), "+v"(gs), "+v"(gl));
#pragma unroll
            for (int sI = 0; sI < KQ; ++sI)
              D = __builtin_amdgcn_mfma_f32_16x16x4f32(sI == 0 ? a0 : ai[sI], sm.bq[4 * sI + lq][wn * (NBW * 32) + b * 16 + l15], D, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float t = D[r];
              // sigma_i tau_j S_ij -> S_ij: flip the sign bit
              const float s_ij = __uint_as_float(__float_as_uint(acc[a][b][r]) ^ sgm[r] ^ taub[b]);
              if constexpr (DIAG) {
                const bool on = dj[b] == wm * 64 + a * 16 + lq4_t + r;
                t = on ? 0.f : t;
                gn += on ? s_ij : 0.f;
              }
              // exp2 with the clamp modifier, as an instruction the COMPILER emits (fmed3(x, 0, 1) folds into v_exp_f32 ... clamp): t comes
              // straight out of an MFMA, and the wait states between an MFMA's write and a VALU read are inserted by the compiler's hazard
              // recogniser -- which does not look inside inline asm.  Round 4 had this as asm("v_exp_f32_e64 ... clamp"): with the
              // 2-MFMA distance chain of d <= 4 it read the accumulator before the MFMA had written it (S o dK off by O(1) for every
              // non-ARD RBF operator with d = 2 .. 4; found by tools/fuzz_matvec.py in round 5), with the 3-MFMA chain of d = 5 .. 8
              // the same read happened to land late enough.
              const float kv = __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(t), 0.f, 1.f);
              const float u = s_ij * kv;
              gs += u;
              gl = fmaf(u, t, gl);
            }
          }
        }
      };
      if (diag_tile) body(std::true_type{}); else body(std::false_type{});
      gsum[0] += (double)gl * (1.0 / (double)kNegHalfLog2e);
      gsum[1] += (double)gs;
      gsum[2] += (double)gn;
    } else
    // ---- epilogue, in passes of 128 columns (the S^T overlay holds one pass): the waves whose blocks lie in the pass
    //      dump them, then thread = row i walks 64 of the pass's columns (as in k_rbf_mfma_grad) -------------------------
#pragma unroll
    for (int pass = 0; pass < TN / Smem::GN; ++pass) {
      __syncthreads();  // all waves are done with the stage images (pass 0) / with the previous pass's S^T
#pragma unroll
      for (int b = 0; b < NB16; ++b) {
        const int cb = wn * (NBW * 32) + b * 16;  // first column of the block within the tile
        if (cb / Smem::GN != pass) continue;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          float4 q;
          q.x = acc[a][b][0]; q.y = acc[a][b][1]; q.z = acc[a][b][2]; q.w = acc[a][b][3];
          *reinterpret_cast<float4*>(&sm.u.s_t[(cb % Smem::GN) + l15][wm * 64 + a * 16 + 4 * lq]) = q;
        }
      }
      const int64_t jp = j0 + pass * Smem::GN;
      for (int t = tid; t < Smem::GN * DPAD; t += 512) {
        const int64_t g = jp * DPAD + t;
        (&sm.xj[0][0])[t] = g < n * DPAD ? xs[g] : 0.f;
      }
      if (tid < Smem::GN) {
        sm.sqj[tid] = (jp + tid < n) ? sq[jp + tid] : 0.f;
        sm.sgj[tid] = grad_col_sign(jp + tid, salt_r) ? -1.f : 1.f;
      }
      __syncthreads();
      // (an opaque copy of the thread index per pass: the row quantities below are invariant over the tile loop, and hoisted out of
      //  it they spill around the K-loop, which has no register to spare)
      int tid_t = tid;
      asm volatile("" : "+v"(tid_t));
      const int il = tid_t & (kHM - 1), jh = (tid_t >> 8) * (Smem::GN / 2);
      const int64_t i = row0 + i0 + il;  // the point; L / the packs are indexed by the local row i0 + il
      const float sgi = grad_col_sign(i0 + il, salt_l) ? -1.f : 1.f;  // sigma_i: the accumulators hold sigma_i tau_j S_ij
      float xiv[DPAD];
#pragma unroll
      for (int c = 0; c < DPAD; c += 4) {
        const float4 q = *reinterpret_cast<const float4*>(&sm.xi[il][c]);
        xiv[c] = q.x; xiv[c + 1] = q.y; xiv[c + 2] = q.z; xiv[c + 3] = q.w;
      }
      const float si = sm.sqi[il];
      float gt[DPAD + 2];
#pragma unroll
      for (int c = 0; c < DPAD + 2; ++c) gt[c] = 0.f;
#pragma unroll(DPAD > 16 ? 1 : 2)  // (DPAD 32: x_j of two columns in flight is 64 registers -- with one, no spills)
      for (int jj = 0; jj < Smem::GN / 2; ++jj) {
        const int jl = jh + jj;
        const int64_t j = jp + jl;
        float xjv[DPAD];
#pragma unroll
        for (int c = 0; c < DPAD; c += 4) {
          const float4 q = *reinterpret_cast<const float4*>(&sm.xj[jl][c]);
          xjv[c] = q.x; xjv[c + 1] = q.y; xjv[c + 2] = q.z; xjv[c + 3] = q.w;
        }
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < DPAD; ++c) dot = fmaf(xiv[c], xjv[c], dot);
        float dist = fmaf(-2.f, dot, si + sm.sqj[jl]);
        dist = fmaxf(dist, 0.f);
        const bool live = (i0 + il < nrow) && (j < n);
        const float s_ij = live ? sm.u.s_t[jl][il] * (sgi * sm.sgj[jl]) : 0.f;
        float kv, wl;
        grad_weights<M52>(kind, i == j ? 0.f : dist, kv, wl);
        gt[DPAD] = fmaf(s_ij, kv, gt[DPAD]);
        const float w = s_ij * wl;
        if (ard) {
#pragma unroll
          for (int c = 0; c < DPAD; c += 2) {  // packed fp32 (v_pk_add / v_pk_mul / v_pk_fma): two dimensions per instruction
            const floatx2 xi2 = {xiv[c], xiv[c + 1]}, xj2 = {xjv[c], xjv[c + 1]};
            const floatx2 df = xi2 - xj2;
            floatx2 g2 = {gt[c], gt[c + 1]};
            g2 = __builtin_elementwise_fma(df * w, df, g2);
            gt[c] = g2[0];
            gt[c + 1] = g2[1];
          }
        } else {
          gt[0] = fmaf(w, dist, gt[0]);
        }
        if (i == j) gt[DPAD + 1] += s_ij;
      }
#pragma unroll
      for (int c = 0; c < DPAD + 2; ++c) gsum[c] += (double)gt[c];
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // no LDS-DMA of mine is left in flight
  if (tid < 8 * (DPAD + 2)) (&sm.red[0][0])[tid] = 0.0;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NG; ++c) {
    const double v = wave_sum(gsum[c]);
    // register epilogue: slots (0, DPAD, DPAD + 1) of the (DPAD + 2)-wide partial row, as the LDS epilogue fills them
    const int slot = REGEPI ? (c == 0 ? 0 : DPAD - 1 + c) : c;
    if (lane == 0) sm.red[wid][slot] = v;
  }
  __syncthreads();
  if (tid < DPAD + 2) {
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    partial[blk * (DPAD + 2) + tid] = ((sm.red[0][tid] + sm.red[1][tid]) + (sm.red[2][tid] + sm.red[3][tid])) +
                                      ((sm.red[4][tid] + sm.red[5][tid]) + (sm.red[6][tid] + sm.red[7][tid]));
  }
}

// M52 = false: RBF / Matern-1/2 / Matern-3/2 (runtime `kind`); true: the Matern-5/2 instance
template <int DPAD, int NBW, bool REGEPI, bool M52>
__global__ __launch_bounds__(512, 1) void k_rbf_mfma_grad_h(const float* __restrict__ xs, const float* __restrict__ sq,
                                                            int64_t n, int64_t npad_l, int64_t npad_r, int ard, int kind,
                                                            const _Float16* __restrict__ Lh, const _Float16* __restrict__ Ll,
                                                            const _Float16* __restrict__ Rh, const _Float16* __restrict__ Rl,
                                                            int64_t nkb /* batch_pad / 8 */, int tiles_per_block,
                                                            uint32_t salt_l, uint32_t salt_r, double* __restrict__ partial,
                                                            int64_t row0, int64_t nrow, const int* __restrict__ one_product) {
  static_assert(!(M52 && REGEPI), "the register epilogue is RBF only");
  rbf_mfma_grad_h_body<DPAD, NBW, REGEPI, M52>(xs, sq, n, npad_l, npad_r, ard, kind, Lh, Ll, Rh, Rl, nkb, tiles_per_block, salt_l, salt_r, partial, row0, nrow, one_product);
}

RbfGradHLayout rbf_grad_h_layout(int64_t n, int64_t nrow, int64_t batch) {
  RbfGradHLayout h;
  h.bpad = (batch + 31) / 32 * 32;
  h.npad = (n + kHM - 1) / kHM * kHM;
  h.npad_l = (nrow + kHM - 1) / kHM * kHM;
  const int64_t f16 = sizeof(_Float16);
  h.amaxL = 0;
  h.amaxR = h.bpad * 4;
  h.scl = 2 * h.bpad * 4;  // [sL, 1/sL, sR, 1/sR]
  h.tail = h.scl + 64;     // n3: the first one-product stage (k_order_rows)
  h.perm = h.tail + 64;    // packed row -> source row, bpad ints
  h.Lh = align_up(h.perm + h.bpad * 4, 256);
  h.Ll = h.Lh + h.bpad * h.npad_l * f16;
  h.Rh = h.Ll + h.bpad * h.npad_l * f16;
  h.Rl = h.Rh + h.bpad * h.npad * f16;
  // The total is sized for a whole operator (npad_l = npad).  The header needs align_up(12 bpad + 128, 256) <= 12 bpad + 383 bytes;
  // the 1536 the size has always carried covers that with 1153 to spare.
  h.bytes = 4 * h.bpad * h.npad * f16 + 3 * h.bpad * 4 + 1536;
  return h;
}

// the one launch site of k_rbf_mfma_grad_h
template <int DPAD, int NBW, bool REGEPI, bool M52>
static int launch_grad_h_k(const mfx_operator* op, const float* xs, const float* sq, const RbfGradHLayout& h, char* base, double* partial,
                           int64_t* nblocks_out, hipStream_t stream) {
  constexpr int TN = GradSmemH<DPAD, NBW>::TN;
  const int64_t n = op->n, row0 = op_row0(op), nrow = op_nrows(op);
  const int64_t nti = (nrow + kHM - 1) / kHM, ntj = (n + TN - 1) / TN;
  const int tiles_per_block = (int)((ntj + kGSplit * kGSub - 1) / (kGSplit * kGSub));
  const dim3 grid(kGSplit, (unsigned)(nti * kGSub));
  auto pack = [&](int64_t off) { return reinterpret_cast<const _Float16*>(base + off); };
  const size_t sh = sizeof(GradSmemH<DPAD, NBW, REGEPI>);
  const auto kernel = k_rbf_mfma_grad_h<DPAD, NBW, REGEPI, M52>;
  MFX_TRY(allow_big_lds(kernel, sh));
  kernel<<<grid, 512, sh, stream>>>(xs, sq, n, h.npad_l, h.npad, op->ard, op->kernel_fn, pack(h.Lh), pack(h.Ll), pack(h.Rh), pack(h.Rl),
                                    h.bpad / 8, tiles_per_block, kSaltL, kSaltR, partial, row0, nrow,
                                    reinterpret_cast<const int*>(base + h.tail));
  MFX_CHECK_LAUNCH();
  *nblocks_out = nti * kGSub * kGSplit;
  return MFX_OK;
}

template <int DPAD>
static int launch_grad_h(const mfx_operator* op, const float* xs, const float* sq, const float* L, int64_t ldl,
                         const float* R, int64_t ldr, int64_t batch, int64_t inner, double* partial, int64_t* nblocks_out,
                         void* hws, const RbfGradHLayout& h, hipStream_t stream) {
  const int64_t n = op->n, nrow = op_nrows(op), bpad = h.bpad;
  if (inner < 1 || batch % inner != 0) inner = 1;
  char* base = static_cast<char*>(hws);
  float* amaxL = reinterpret_cast<float*>(base + h.amaxL);
  float* amaxR = reinterpret_cast<float*>(base + h.amaxR);
  float* scl = reinterpret_cast<float*>(base + h.scl);
  int* tail = reinterpret_cast<int*>(base + h.tail);
  int* perm = reinterpret_cast<int*>(base + h.perm);
  auto pack = [&](int64_t off) { return reinterpret_cast<_Float16*>(base + off); };
  k_row_amax<<<(unsigned)batch, 256, 0, stream>>>(L, ldl, nrow, amaxL);
  k_row_amax<<<(unsigned)batch, 256, 0, stream>>>(R, ldr, n, amaxR);
  k_global_scale<<<1, 256, 0, stream>>>(amaxL, batch, scl);
  k_global_scale<<<1, 256, 0, stream>>>(amaxR, batch, scl + 2);
  if (bpad <= kSortMax) {
    int npow2 = 64;
    while (npow2 < bpad) npow2 <<= 1;
    // (the keys of kSortMax rows are the 64 KiB a kernel gets by default: its static LDS then needs the attribute)
    MFX_TRY(allow_big_lds(k_order_rows, (size_t)npow2 * 8 + 16 * sizeof(double) + sizeof(int)));
    k_order_rows<<<1, 1024, (size_t)npow2 * 8, stream>>>(amaxL, amaxR, batch, inner, bpad, npow2, grad_one_product_log2(), perm, tail);
  } else {
    k_order_default<<<(unsigned)((bpad + 255) / 256), 256, 0, stream>>>(batch, inner, bpad, perm, tail);
  }
  const dim3 pgrid((unsigned)((h.npad + 255) / 256), (unsigned)(bpad / 8));
  const dim3 pgrid_l((unsigned)((h.npad_l + 255) / 256), (unsigned)(bpad / 8));
  k_pack_f16<<<pgrid_l, 256, 0, stream>>>(L, ldl, batch, nrow, h.npad_l, scl, kSaltL, perm, pack(h.Lh), pack(h.Ll));
  k_pack_f16<<<pgrid, 256, 0, stream>>>(R, ldr, batch, n, h.npad, scl + 2, kSaltR, perm, pack(h.Rh), pack(h.Rl));
  MFX_CHECK_LAUNCH();
  // 256 x 256 workgroup tile (NBW = 4) for d <= 8; d = 9..16 keeps the 256 x 128 tile (the epilogue registers on top of 128
  // accumulators spill there)
  auto gemm = [&](auto nbw) -> int {
    constexpr int NBW = decltype(nbw)::value;
    // RBF kernel, one lengthscale, d <= 8: the register epilogue; Matern / ARD / d > 8: the LDS epilogue
    if constexpr (DPAD <= 8) {
      if (!op->ard && op->kernel_fn == MFX_KERNEL_RBF)
        return launch_grad_h_k<DPAD, NBW, true, false>(op, xs, sq, h, base, partial, nblocks_out, stream);
    }
    return with_bool(op->kernel_fn == MFX_KERNEL_MATERN52, [&](auto m52) -> int {
      return launch_grad_h_k<DPAD, NBW, false, decltype(m52)::value>(op, xs, sq, h, base, partial, nblocks_out, stream);
    });
  };
  if constexpr (DPAD <= 8) return gemm(Const<4>{});
  return gemm(Const<2>{});  // (d <= 8 never gets here, but its 256 x 128 instances have always been part of the code object)
}

// returns the device pointer holding [sL, 1/sL, sR, 1/sR] through scales_out
int rbf_mfma_grad_h(const mfx_operator* op, const float* xs, const float* sq, int dpad, const float* L, int64_t ldl,
                    const float* R, int64_t ldr, int64_t batch, int64_t inner, double* partial, int64_t* nblocks_out, void* hws,
                    const float** scales_out, hipStream_t stream) {
  const RbfGradHLayout h = rbf_grad_h_layout(op->n, op_nrows(op), batch);
  *scales_out = reinterpret_cast<const float*>(static_cast<const char*>(hws) + h.scl);
  return with_mfma_dpad<32>(dpad, "split parameter sweep supports d <= 32", [&](auto dc) -> int {
    return launch_grad_h<decltype(dc)::value>(op, xs, sq, L, ldl, R, ldr, batch, inner, partial, nblocks_out, hws, h, stream);
  });
}

// ================================================================================================
// Parameter-gradient sweep on the matrix cores.
//
//   d/dtheta sum_bt L_bt^T K(theta) R_bt = sum_ij S_ij dK_ij/dtheta,   S = L^T R  (n x n, rank <= batch)
//
// GEMM view: M = n (i), N = n (j), K = batch (all (probe, Lanczos-step) pairs of the adjoint at once:
// 2560 for BASELINE config 4).  Both operands are K-major in HBM ((batch, n) rows, n contiguous), which
// is exactly the A[i][k] / B[k][j] lane layout of v_mfma_f32_32x32x2_f32 -- LDS tiles are straight row
// copies (ds_write_b128), fragments are conflict-free ds_read_b32.  S never leaves the accumulators:
// the epilogue evaluates K_ij (distance from LDS-broadcast x_i and register x_j, v_exp_f32), multiplies
// and reduces to (d + 2) numbers per workgroup.  128 x 128 tile per workgroup (4 waves, 64 x 64 each),
// BK = 32 batch rows per stage, register-prefetched double buffering.
// grid = (8 column ranges, n/128 row tiles): blockIdx.x is the XCD label (round-robin dispatch), so the
// 64 resident workgroups of one XCD walk the SAME R panel (1.3 MB, L2-resident) while their L panels
// come from the Infinity Cache.
// ================================================================================================


template <int DPAD>
struct GradSmem {
  union {
    struct {
      float a[2][kGK][kGM];
      float b[2][kGK][kGN];
    } st;
    float s_t[kGN][kGLd];  // S^T tile (column j major) for the epilogue
  } u;
  float xi[kGM][DPAD];
  float sqi[kGM];
  float xj[kGN][DPAD];
  float sqj[kGN];
  double red[4][DPAD + 2];
};

template <int DPAD, bool VEC4>
__device__ __forceinline__ void grad_load_stage(float4 (&ra)[4], float4 (&rb)[4], const float* __restrict__ L,
                                                int64_t ldl, const float* __restrict__ R, int64_t ldr,
                                                int64_t batch, int64_t nrow, int64_t n, int64_t bt0, int64_t i0, int64_t j0,
                                                int tid) {
  // 32 rows x 128 floats = 1024 float4 per operand; thread t takes float4 (row = f / 32, col4 = f % 32)
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int f = tid + 256 * u;
    const int row = f >> 5, c4 = (f & 31) * 4;
    const int64_t bt = bt0 + row;
    float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
    if (bt < batch) {
      const float* pa = L + bt * ldl + i0 + c4;
      const float* pb = R + bt * ldr + j0 + c4;
      if (VEC4 && i0 + c4 + 3 < nrow) {
        va = *reinterpret_cast<const float4*>(pa);
      } else {
        if (i0 + c4 + 0 < nrow) va.x = pa[0];
        if (i0 + c4 + 1 < nrow) va.y = pa[1];
        if (i0 + c4 + 2 < nrow) va.z = pa[2];
        if (i0 + c4 + 3 < nrow) va.w = pa[3];
      }
      if (VEC4 && j0 + c4 + 3 < n) {
        vb = *reinterpret_cast<const float4*>(pb);
      } else {
        if (j0 + c4 + 0 < n) vb.x = pb[0];
        if (j0 + c4 + 1 < n) vb.y = pb[1];
        if (j0 + c4 + 2 < n) vb.z = pb[2];
        if (j0 + c4 + 3 < n) vb.w = pb[3];
      }
    }
    ra[u] = va;
    rb[u] = vb;
  }
}

template <int DPAD, bool VEC4, bool M52>
__device__ __forceinline__ void rbf_mfma_grad_body(const float* __restrict__ xs, const float* __restrict__ sq,
                                                          int64_t n, int ard, int kind, const float* __restrict__ L,
                                                          int64_t ldl, const float* __restrict__ R, int64_t ldr,
                                                          int64_t batch, int tiles_per_block,
                                                          double* __restrict__ partial, int64_t row0, int64_t nrow) {
  // rows: the nrow points row0 .. of X that L covers (a row shard, or all n), L indexed locally; columns: all n points
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  GradSmem<DPAD>& sm = *reinterpret_cast<GradSmem<DPAD>*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int wm = wid >> 1, wn = wid & 1;  // wave -> 64 x 64 quadrant of the 128 x 128 tile
  const int64_t i0 = (int64_t)(blockIdx.y / kGSub) * kGM;  // 8 x 8 L2-sharing patches per XCD, see kGSub
  const int64_t ntj = (n + kGN - 1) / kGN;
  const int64_t tj_begin = ((int64_t)blockIdx.x * kGSub + blockIdx.y % kGSub) * tiles_per_block;
  int64_t tj_end = tj_begin + tiles_per_block;
  if (tj_end > ntj) tj_end = ntj;

  // x_i, |x_i|^2 of this row tile (fixed for the workgroup)
  for (int t = tid; t < kGM * DPAD; t += 256) {
    const int64_t g = i0 * DPAD + t;
    (&sm.xi[0][0])[t] = g < nrow * DPAD ? xs[row0 * DPAD + g] : 0.f;
  }
  if (tid < kGM) sm.sqi[tid] = (i0 + tid < nrow) ? sq[row0 + i0 + tid] : 0.f;

  double gsum[DPAD + 2];
#pragma unroll
  for (int c = 0; c < DPAD + 2; ++c) gsum[c] = 0.0;

  const int64_t nstage = (batch + kGK - 1) / kGK;
  for (int64_t tj = tj_begin; tj < tj_end; ++tj) {
    const int64_t j0 = tj * kGN;
    floatx16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    float4 ra[4], rb[4];
    grad_load_stage<DPAD, VEC4>(ra, rb, L, ldl, R, ldr, batch, nrow, n, 0, i0, j0, tid);
    __syncthreads();  // previous tile's epilogue / LDS reads are done
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int f = tid + 256 * u;
      *reinterpret_cast<float4*>(&sm.u.st.a[0][f >> 5][(f & 31) * 4]) = ra[u];
      *reinterpret_cast<float4*>(&sm.u.st.b[0][f >> 5][(f & 31) * 4]) = rb[u];
    }
    __syncthreads();
    for (int64_t st = 0; st < nstage; ++st) {
      const int cur = (int)(st & 1);
      if (st + 1 < nstage) grad_load_stage<DPAD, VEC4>(ra, rb, L, ldl, R, ldr, batch, nrow, n, (st + 1) * kGK, i0, j0, tid);
#pragma unroll
      for (int kk = 0; kk < kGK; kk += 2) {
        float av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) av[a] = sm.u.st.a[cur][kk + lhi][wm * 64 + a * 32 + l31];
#pragma unroll
        for (int b = 0; b < 2; ++b) bv[b] = sm.u.st.b[cur][kk + lhi][wn * 64 + b * 32 + l31];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
      if (st + 1 < nstage) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int f = tid + 256 * u;
          *reinterpret_cast<float4*>(&sm.u.st.a[cur ^ 1][f >> 5][(f & 31) * 4]) = ra[u];
          *reinterpret_cast<float4*>(&sm.u.st.b[cur ^ 1][f >> 5][(f & 31) * 4]) = rb[u];
        }
      }
      __syncthreads();
    }
    // ---- epilogue: S^T tile -> LDS (overlays the staging buffers; the K-loop's last barrier has
    //      passed), then thread = row i walks 64 columns j: W_ij = S_ij exp(-dist_ij / 2) ------------
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float4 q;
          q.x = acc[a][b][4 * g + 0]; q.y = acc[a][b][4 * g + 1]; q.z = acc[a][b][4 * g + 2]; q.w = acc[a][b][4 * g + 3];
          *reinterpret_cast<float4*>(&sm.u.s_t[wn * 64 + b * 32 + l31][wm * 64 + a * 32 + 8 * g + 4 * lhi]) = q;
        }
    for (int t = tid; t < kGN * DPAD; t += 256) {
      const int64_t g = j0 * DPAD + t;
      (&sm.xj[0][0])[t] = g < n * DPAD ? xs[g] : 0.f;
    }
    if (tid < kGN) sm.sqj[tid] = (j0 + tid < n) ? sq[j0 + tid] : 0.f;
    __syncthreads();
    {
      const int il = tid & (kGM - 1), jh = (tid >> 7) * 64;
      const int64_t i = row0 + i0 + il;  // the point; L is indexed by the local row i0 + il
      float xiv[DPAD];
#pragma unroll
      for (int c = 0; c < DPAD; c += 4) {
        const float4 q = *reinterpret_cast<const float4*>(&sm.xi[il][c]);
        xiv[c] = q.x; xiv[c + 1] = q.y; xiv[c + 2] = q.z; xiv[c + 3] = q.w;
      }
      const float si = sm.sqi[il];
      float gt[DPAD + 2];
#pragma unroll
      for (int c = 0; c < DPAD + 2; ++c) gt[c] = 0.f;
#pragma unroll 2
      for (int jj = 0; jj < 64; ++jj) {
        const int jl = jh + jj;
        const int64_t j = j0 + jl;
        float xjv[DPAD];
#pragma unroll
        for (int c = 0; c < DPAD; c += 4) {
          const float4 q = *reinterpret_cast<const float4*>(&sm.xj[jl][c]);
          xjv[c] = q.x; xjv[c + 1] = q.y; xjv[c + 2] = q.z; xjv[c + 3] = q.w;
        }
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < DPAD; ++c) dot = fmaf(xiv[c], xjv[c], dot);
        float dist = fmaf(-2.f, dot, si + sm.sqj[jl]);
        dist = fmaxf(dist, 0.f);
        const bool live = (i0 + il < nrow) && (j < n);
        const float s_ij = live ? sm.u.s_t[jl][il] : 0.f;
        float kv, wl;
        grad_weights<M52>(kind, i == j ? 0.f : dist, kv, wl);
        gt[DPAD] = fmaf(s_ij, kv, gt[DPAD]);
        const float w = s_ij * wl;
        if (ard) {
#pragma unroll
          for (int c = 0; c < DPAD; c += 2) {  // packed fp32 (v_pk_add / v_pk_mul / v_pk_fma): two dimensions per instruction
            const floatx2 xi2 = {xiv[c], xiv[c + 1]}, xj2 = {xjv[c], xjv[c + 1]};
            const floatx2 df = xi2 - xj2;
            floatx2 g2 = {gt[c], gt[c + 1]};
            g2 = __builtin_elementwise_fma(df * w, df, g2);
            gt[c] = g2[0];
            gt[c + 1] = g2[1];
          }
        } else {
          gt[0] = fmaf(w, dist, gt[0]);
        }
        if (i == j) gt[DPAD + 1] += s_ij;
      }
#pragma unroll
      for (int c = 0; c < DPAD + 2; ++c) gsum[c] += (double)gt[c];
    }
  }
  // ---- workgroup reduction -> one partial row per workgroup ------------------------------------
#pragma unroll
  for (int c = 0; c < DPAD + 2; ++c) {
    const double v = wave_sum(gsum[c]);
    if (lane == 0) sm.red[wid][c] = v;
  }
  __syncthreads();
  if (tid < DPAD + 2) {
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    partial[blk * (DPAD + 2) + tid] = sm.red[0][tid] + sm.red[1][tid] + sm.red[2][tid] + sm.red[3][tid];
  }
}

// as for the split GEMM: M52 = false is the instance of the three runtime families, true the Matern-5/2 one
template <int DPAD, bool VEC4, bool M52>
__global__ __launch_bounds__(256, DPAD > 16 ? 1 : 2) /* DPAD = 32: 97 KB of LDS, one workgroup per CU anyway */ void k_rbf_mfma_grad(const float* __restrict__ xs, const float* __restrict__ sq,
                                                          int64_t n, int ard, int kind, const float* __restrict__ L,
                                                          int64_t ldl, const float* __restrict__ R, int64_t ldr,
                                                          int64_t batch, int tiles_per_block,
                                                          double* __restrict__ partial, int64_t row0, int64_t nrow) {
  rbf_mfma_grad_body<DPAD, VEC4, M52>(xs, sq, n, ard, kind, L, ldl, R, ldr, batch, tiles_per_block, partial, row0, nrow);
}

// Which parameter sweep runs.  The matrix-core GEMMs need n >= 256 and 16 rows -- or n >= 2048: from there on even ONE (lambda, x)
// pair (the PCG backward of the log-marginal likelihood) is cheaper here: the cost is the n^2 epilogue, which the VALU sweep pays at a
// quarter of the rate (16.8 vs ~4 ms at n = 36 584).
//   exact fp32, d <= 64 (beyond: x_i and x_j of a 128 x 128 tile, 2 x 128 x DPAD floats, no longer fit the LDS next to the operand stages);
//   3 x f16 split, d <= 32 (16 < d <= 32: its 256 x 128 form with 64-column epilogue passes -- 249 registers, 140 KB of LDS), in
//     rbf_mode MFX_RBF_F16X3 when the split-gradient region was carved and the packs fit the GEMM's 32-bit byte offsets:
//     2 B x padded batch x padded n < 4 GiB.
RbfGradPath rbf_grad_path(const mfx_operator* op, int64_t batch, bool have_hws) {
  if (op->dtype != MFX_F32 || op->d > 64 || op->n < 256 || !(batch >= 16 || op->n >= 2048)) return RbfGradPath::valu;
  const RbfGradHLayout h = rbf_grad_h_layout(op->n, op_nrows(op), batch);
  const bool fits32 = h.bpad * h.npad * 2 < ((int64_t)1 << 32);
  return op->d <= 32 && op->rbf_mode == MFX_RBF_F16X3 && have_hws && fits32 ? RbfGradPath::split : RbfGradPath::exact;
}

int64_t rbf_mfma_grad_partial_rows(int64_t n) { return ((n + kGM - 1) / kGM) * kGSplit * kGSub; }

int rbf_mfma_grad(const mfx_operator* op, const float* xs, const float* sq, int dpad, const float* L, int64_t ldl,
                  const float* R, int64_t ldr, int64_t batch, double* partial, int64_t* nblocks_out,
                  hipStream_t stream) {
  const int64_t n = op->n, row0 = op_row0(op), nrow = op_nrows(op);
  const int64_t nti = (nrow + kGM - 1) / kGM, ntj = (n + kGN - 1) / kGN;
  const int tiles_per_block = (int)((ntj + kGSplit * kGSub - 1) / (kGSplit * kGSub));
  const dim3 grid(kGSplit, (unsigned)(nti * kGSub));
  *nblocks_out = nti * kGSub * kGSplit;
  return with_mfma_dpad<64>(dpad, "exact-fp32 matrix-core parameter sweep supports d <= 64", [&](auto dc) -> int {
    return with_bool(vec4_ok(L, ldl, R, ldr, n, nrow), [&](auto v4) -> int {
      return with_bool(op->kernel_fn == MFX_KERNEL_MATERN52, [&](auto m52) -> int {
        constexpr int DPAD = decltype(dc)::value;
        const size_t sh = sizeof(GradSmem<DPAD>);
        const auto kernel = k_rbf_mfma_grad<DPAD, decltype(v4)::value, decltype(m52)::value>;
        MFX_TRY(allow_big_lds(kernel, sh));
        kernel<<<grid, 256, sh, stream>>>(xs, sq, n, op->ard, op->kernel_fn, L, ldl, R, ldr, batch, tiles_per_block, partial, row0, nrow);
        MFX_CHECK_LAUNCH();
        return MFX_OK;
      });
    });
  });
}

}  // namespace mfx
