// libmfx: matrix-free RBF / Matern Gram matvec on the CDNA4 matrix cores (gfx950).
//
// What is in this file, in order (rbf_apply_path, at the end, says which of them runs):
//   * k_rbf_mfma_apply          the fp32-exact matvec on v_mfma_f32_32x32x2_f32 (d <= 128), described right below;
//   * the vector scales         k_row_amax_bits / k_row_scale_from_bits / k_row_amax_part and their workspace (rbf_vscale_layout);
//   * the h3 pair               k_rbf_h3_packed and k_rbf_h3_split: the 3 x f16 split matvec (d <= 32), one kernel per staging;
//   * k_split_reduce            sums the partial results of a column-split launch;
//   * k_pack_tiles              the pre-pass that writes the packed kernel's (and the fat-wave kernels') tile images, and the
//                               pack workspace (rbf_pack_layout);
//   * the launch layer          launch_apply_h3k (pre-pass, packed or fat-wave kernel, split kernel, reduce) and launch_apply.
// The fat-wave kernels are in mfx_rbf_fat.hip, the parameter-gradient GEMMs in mfx_rbf_mfma_grad.hip.
//
// The fp32-exact kernel:
//
//   W[i][b] = s * sum_j exp(-max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) / 2) V[j][b] + noise V[i][b]
//   (x already divided by the lengthscale; util/gp_util.py:160-176,225-226,536-541)
//
// The Gram matrix is never materialised (the reference materialises (n/num x n) tiles,
// util/gp_util.py:496-509).  GEMM view: M = n rows i, N = probes, K = n columns j.
//   * v_mfma_f32_32x32x2_f32: A = K-tile (32 i x 2 j), B = V-tile (2 j x 32 probes), D = 32 i x 32 probes.
//   * The squared distances are themselves a small MFMA product (inner dimension d + 2, augmented
//     vectors), computed TRANSPOSED so that its accumulator registers, after v_min + v_exp in place,
//     are exactly the A operand of the contraction MFMA (lane = row i, register = column j) -- no
//     shuffle, no LDS round trip for K, ~2 VALU instructions per kernel entry.
//   * B comes from an LDS image Vt[j][probe] (probe-contiguous, conflict-free ds_read_b32), filled
//     from the (p, n) probe-major global layout with 256-B coalesced segments and a transposing store
//     (row pad 1 -> at most 2-way ds_write conflicts, which are free on gfx950).
//   * one wave owns MI x 32 rows and all NB x 32 probes of its chunk: MI*NB*16 accumulator registers.
// Bound: fp32 MFMA (2 n^2 p flop per matvec) -- the exp/distance VALU work co-issues underneath.
#include <stdlib.h>

#include <type_traits>

#include "mfx_internal.h"
#include "mfx_rbf_common.h"

namespace mfx {


__device__ __forceinline__ float dist_factor(int kind) {  // multiplies the squared distance inside the MFMA product
  return kind == MFX_KERNEL_RBF ? -0.72134752044448170368f
                                : (kind == MFX_KERNEL_MATERN52 ? 5.f : (kind == MFX_KERNEL_MATERN32 ? 3.f : 1.f)) * kLog2e * kLog2e;
}

// exp2(min(x, 0)) in ONE VALU instruction: v_exp_f32 with the clamp output modifier ([0, 1]); exp2 is
// monotone, so clamping the result equals clamping the argument (the reference clamps the squared
// distance at 0, util/gp_util.py:173).  fp32 MFMA shares the FP32 lanes with the VALU on gfx950
// (measured: removing the min/exp shortens the kernel by exactly their issue cycles), so every VALU
// instruction per kernel entry is paid in full.  Written so that the COMPILER emits the instruction (fmed3(x, 0, 1) folds into the
// clamp modifier of v_exp_f32): x is an MFMA result and the result feeds an MFMA operand, and the wait states on both sides are the
// hazard recogniser's job -- it does not look inside inline asm (rounds 1-4 had asm("v_exp_f32_e64 ... clamp; s_nop 1") here, which
// covered the second hazard by hand and the first one not at all; see the register epilogue of k_rbf_mfma_grad_h for what that cost).
__device__ __forceinline__ float exp2_clamped(float x) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(x), 0.f, 1.f); }

template <int DPAD, int NB, int kTJ>
struct RbfTile {
  static constexpr int KD = DPAD + 2;        // augmented inner dimension of the distance product
  static constexpr int LDV = NB * 32 + 1;    // padded probe row
  float aj[KD][kTJ];   // A operand of the distance MFMA, k-major: c * [-2 x_j, |x_j|^2, 1]
  float vt[kTJ][LDV];  // V^T tile [j][probe]
};

// One workgroup = 4 waves x 64 rows; grid.y = chunks of NB*32 probes.  Per 64-column tile and per
// (32-row, 32-column) block the wave runs
//   (1) KD/2 distance MFMAs  D^T[j][i] = sum_k A_j[k] B_i[k] = c (|x_i|^2 + |x_j|^2 - 2 x_i.x_j)   (c = -log2(e)/2)
//       A_j from LDS (k-major, conflict-free), B_i = [x_i, 1, |x_i|^2] resident in registers;
//   (2) 16 x { v_min(., 0), v_exp }  in place: the accumulator registers ARE the A operand of step (3):
//       register r of lane (i = lane & 31, h = lane >> 5) holds column j_r(h) = (r & 3) + 8 (r >> 2) + 4 h;
//   (3) 16 x NB contraction MFMAs  W[i][probe] += K[i][j_r(h)] V[j_r(h)][probe]  with B = Vt rows j_r(h).
// K never exists outside VGPRs.  Global -> LDS staging is register-prefetched and double-buffered: one
// barrier per tile.
template <int DPAD, int NB, bool VEC4, int kMI, int kTJ>
__global__ __launch_bounds__(256, 2) void k_rbf_mfma_apply(const float* __restrict__ xs, const float* __restrict__ sq,
                                                           int64_t n, const float* __restrict__ outputscale,
                                                           const float* __restrict__ noise,
                                                           const float* __restrict__ x, int64_t ldx,
                                                           float* __restrict__ y, int64_t ldy, int64_t p, int kind,
                                                           int64_t row0, int64_t rend) {
  // rows [row0, rend) of the operator (a row shard, or all of it): x has the full length n, y is indexed from row0
  using Tile = RbfTile<DPAD, NB, kTJ>;
  const float cfac = dist_factor(kind);
  constexpr int KD = Tile::KD, KS = KD / 2;
  __shared__ __attribute__((aligned(16))) Tile tile[2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int64_t i_wave = row0 + (int64_t)blockIdx.x * (4 * kMI * 32) + (int64_t)wid * (kMI * 32);
  const int64_t b0 = (int64_t)blockIdx.y * (NB * 32);

  // B operand of the distance product: B_i[k], k = 2 s + lhi
  float bi[kMI][KS];
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi) {
    int64_t i = i_wave + mi * 32 + l31;
    if (i >= rend) i = rend - 1;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 2 * s + lhi;
      bi[mi][s] = (k < DPAD) ? xs[i * DPAD + k] : (k == DPAD ? 1.f : sq[i]);
    }
  }
  floatx16 acc[kMI][NB];
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][nb][r] = 0.f;

  // ---- staging: registers <- global, LDS <- registers -----------------------------------------
  constexpr int kF4 = NB * 32 * (kTJ / 4);   // float4 chunks of the V tile
  constexpr int kVPT = (kF4 + 255) / 256;    // per thread
  constexpr int kXPT = (kTJ * DPAD + 255) / 256;
  float4 rv[kVPT];
  float rx[kXPT], rsq = 0.f;

  auto load_tile = [&](int64_t j0) {
#pragma unroll
    for (int u = 0; u < kVPT; ++u) {
      const int f = tid + 256 * u;
      const int bq = f / (kTJ / 4), j4 = (f % (kTJ / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (f < kF4 && b0 + bq < p) {
        const float* src = x + (b0 + bq) * ldx + j0 + j4;
        if (VEC4 && j0 + j4 + 3 < n) {
          v = *reinterpret_cast<const float4*>(src);
        } else {
          if (j0 + j4 + 0 < n) v.x = src[0];
          if (j0 + j4 + 1 < n) v.y = src[1];
          if (j0 + j4 + 2 < n) v.z = src[2];
          if (j0 + j4 + 3 < n) v.w = src[3];
        }
      }
      rv[u] = v;
    }
#pragma unroll
    for (int u = 0; u < kXPT; ++u) {
      const int t = tid + 256 * u;
      const int64_t g = j0 * DPAD + t;
      rx[u] = (t < kTJ * DPAD && g < n * DPAD) ? xs[g] : 0.f;
    }
    if (tid < kTJ) rsq = (j0 + tid < n) ? sq[j0 + tid] : 0.f;
  };
  auto store_tile = [&](Tile& tl) {
#pragma unroll
    for (int u = 0; u < kVPT; ++u) {
      const int f = tid + 256 * u;
      if (f < kF4) {
        const int bq = f / (kTJ / 4), j4 = (f % (kTJ / 4)) * 4;
        tl.vt[j4 + 0][bq] = rv[u].x;
        tl.vt[j4 + 1][bq] = rv[u].y;
        tl.vt[j4 + 2][bq] = rv[u].z;
        tl.vt[j4 + 3][bq] = rv[u].w;
      }
    }
#pragma unroll
    for (int u = 0; u < kXPT; ++u) {
      const int t = tid + 256 * u;
      if (t < kTJ * DPAD) tl.aj[t % DPAD][t / DPAD] = -2.f * cfac * rx[u];
    }
    if (tid < kTJ) {
      tl.aj[DPAD][tid] = cfac * rsq;
      tl.aj[DPAD + 1][tid] = cfac;
    }
  };

  load_tile(0);
  store_tile(tile[0]);
  __syncthreads();
  const int64_t ntile = (n + kTJ - 1) / kTJ;
  for (int64_t t = 0; t < ntile; ++t) {
    const Tile& tl = tile[t & 1];
    if (t + 1 < ntile) load_tile((t + 1) * kTJ);
#pragma unroll
    for (int jb = 0; jb < kTJ / 32; ++jb) {
      float aj[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) aj[s] = tl.aj[2 * s + lhi][jb * 32 + l31];
#pragma unroll
      for (int mi = 0; mi < kMI; ++mi) {
        floatx16 kd;
#pragma unroll
        for (int r = 0; r < 16; ++r) kd[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) kd = __builtin_amdgcn_mfma_f32_32x32x2f32(aj[s], bi[mi][s], kd, 0, 0, 0);
        if (kind == MFX_KERNEL_RBF) {
#pragma unroll
          for (int r = 0; r < 16; ++r) kd[r] = exp2_clamped(kd[r]);
        } else {
          // the diagonal 32 x 32 block: a point's distance to itself is exactly 0
          const bool diag_blk = (t * kTJ + jb * 32) == (i_wave + mi * 32);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float tv = kd[r];
            if (diag_blk && l31 == (r & 3) + 8 * (r >> 2) + 4 * lhi) tv = 0.f;
            kd[r] = kind == MFX_KERNEL_MATERN52   ? matern_from_t<MFX_KERNEL_MATERN52>(tv, 0.f)
                    : kind == MFX_KERNEL_MATERN32 ? matern_from_t<MFX_KERNEL_MATERN32>(tv, 0.f)
                                                  : matern_from_t<MFX_KERNEL_MATERN12>(tv, 0.f);
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int jr = jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
            acc[mi][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kd[r], tl.vt[jr][nb * 32 + l31], acc[mi][nb], 0, 0, 0);
        }
      }
    }
    if (t + 1 < ntile) store_tile(tile[(t + 1) & 1]);
    __syncthreads();
  }
  // ---- epilogue: y[b][i] = s * acc + noise * x[b][i];  D layout: col = lane & 31 (probe),
  //      row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)  -> 4 consecutive rows per register quad
  const float s = outputscale[0], nz = noise[0];
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int64_t b = b0 + nb * 32 + l31;
      if (b >= p) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t i = i_wave + mi * 32 + 8 * g + 4 * lhi;
        if (VEC4 && i + 3 < rend) {
          const float4 xv = *reinterpret_cast<const float4*>(x + b * ldx + i);
          float4 o;
          o.x = fmaf(s, acc[mi][nb][4 * g + 0], nz * xv.x);
          o.y = fmaf(s, acc[mi][nb][4 * g + 1], nz * xv.y);
          o.z = fmaf(s, acc[mi][nb][4 * g + 2], nz * xv.z);
          o.w = fmaf(s, acc[mi][nb][4 * g + 3], nz * xv.w);
          *reinterpret_cast<float4*>(y + b * ldy + (i - row0)) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (i + e < rend) y[b * ldy + (i - row0) + e] = fmaf(s, acc[mi][nb][4 * g + e], nz * x[b * ldx + i + e]);
        }
      }
    }
}

// ================================================================================================
// 3 x f16 split path ("fp32 emulation on the f16 matrix pipe").
//
// Why: on gfx950 the fp32-input MFMA runs at the fp32 VALU rate and does not co-execute with VALU
// work (ablation in DESIGN.md §3.2), so the fp32-exact kernel above is capped at ~70 % of 157 TFLOP/s.
// The f16 MFMA (v_mfma_f32_32x32x16_f16) is a separate pipe with 16x the rate.  Every fp32 operand is
// split into hi + lo with hi = top 11 significant bits (exactly an f16), lo = the remainder rounded to
// f16 (11 more bits), and the product is accumulated in fp32 as  hi*hi + hi*lo + lo*hi  (the dropped
// lo*lo term is 2^-24 relative, random sign).  K in [0, 1] needs no scaling; each probe vector is scaled by a
// power of two so that its largest entry is ~2^14 (scale undone, exactly, in the epilogue).
// Accuracy: |error| <= ~4 eps_fp32 per product, fp32 accumulation -- validated against the fp64 oracle
// at the same tolerances as the fp32-exact path (tests/test_gpu_parity.py).
// ================================================================================================
// per-row power-of-two scale (row_scale_of).  (The 256-thread |max| reduction is written out here, in k_row_amax_part and in the
// gradient file's k_row_amax: as one shared helper, by return value or by callback, it changed the instruction order of all three.)
//  Two tiny kernels instead of one workgroup per row (98 us at n = 131072): slice
// maxima (grid.x slices of a row) -> atomicMax on the bit pattern of the non-negative float (monotone as an integer), then the scales.
__global__ __launch_bounds__(256) void k_row_amax_bits(const float* __restrict__ x, int64_t ldx, int64_t n,
                                                       unsigned* __restrict__ amax_bits) {
  __shared__ float sm[4];
  const int64_t b = blockIdx.y;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    m = fmaxf(m, fabsf(x[b * ldx + i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(amax_bits + b, __float_as_uint(fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]))));
}

__global__ void k_row_scale_from_bits(const unsigned* __restrict__ amax_bits, int64_t rows, float* __restrict__ scale) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= rows) return;
  const float s = row_scale_of(__uint_as_float(amax_bits[b]));
  scale[2 * b] = s;
  scale[2 * b + 1] = 1.f / s;
}

// Pre-packed path: ONE launch in front of k_pack_tiles instead of three (zero + atomic maxima + scales).  Slice maxima of |x| per
// row, no atomics: part[b gx + slice]; k_pack_tiles folds a row's <= 64 slice maxima into its scale itself.  Block (0, 0) also
// clears the f16 range flag, which k_pack_tiles (behind this launch in stream order) raises.
__global__ __launch_bounds__(256) void k_row_amax_part(const float* __restrict__ x, int64_t ldx, int64_t n, float* __restrict__ part,
                                                       int* __restrict__ flag) {
  __shared__ float sm[4];
  const int64_t b = blockIdx.y;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    m = fmaxf(m, fabsf(x[b * ldx + i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    part[b * gridDim.x + blockIdx.x] = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    if (blockIdx.x == 0 && blockIdx.y == 0) *flag = 0;
  }
}

// slices of a vector for the row-maximum kernels
static int64_t amax_slices(int64_t n) { return (n + 8191) / 8192 < 64 ? (n + 8191) / 8192 : 64; }

RbfVscaleLayout rbf_vscale_layout(int64_t n, int64_t p) {
  RbfVscaleLayout v;
  v.scales = 0;
  v.amax_bits = 2 * p;
  v.rangeflag = 3 * p;
  v.amax_part = 3 * p + 64;
  v.gx = amax_slices(n);
  while (v.gx > 1 && v.amax_part + p * v.gx > kRbfVscaleFloats) --v.gx;
  v.ok = v.amax_part + p * v.gx <= kRbfVscaleFloats;  // p <= kRbfVscaleMaxP -- far beyond any probe count
  return v;
}

// in-kernel-split path: scale (rows, 2) = [s, 1/s] from the |max| bit patterns behind it
static int row_scales(const float* x, int64_t ldx, int64_t n, int64_t rows, float* vscale, const RbfVscaleLayout& v, hipStream_t stream) {
  unsigned* bits = reinterpret_cast<unsigned*>(vscale + v.amax_bits);
  static_assert(sizeof(unsigned) == sizeof(float), "the range flag sits one element behind the bit patterns");
  MFX_TRY(zero_async(bits, sizeof(unsigned) * (v.rangeflag + 1 - v.amax_bits), stream));  // + the f16 range flag behind them
  k_row_amax_bits<<<dim3((unsigned)amax_slices(n), (unsigned)rows), 256, 0, stream>>>(x, ldx, n, bits);
  k_row_scale_from_bits<<<(unsigned)((rows + 255) / 256), 256, 0, stream>>>(bits, rows, vscale + v.scales);
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

// ================================================================================================
// Pipelined 3 x f16 kernels ("h3"): the production fp32 Gram matvec, as a PAIR of kernels.
//
// Measured on gfx950 (ablations): in the un-pipelined split kernel the distance MFMAs, the exp/split VALU work and
// the f16 contraction MFMAs simply ADD UP -- the two waves of a SIMD run the same program between the same barriers and fall into
// lock-step, and the fp32 MFMA shares the FP32 lanes with the VALU.  So the overlap is built into ONE wave's instruction stream,
// pinned with sched_barrier.  Both kernels sweep 64-column tiles, a wave owns 2 x 32 rows and all NB x 32 probes of its chunk, and
// gridDim.z > 1 is a column split for small n (too few row blocks to fill 256 CUs): workgroup z sweeps its share of the tiles and
// writes a partial result to part[z][probe][row]; k_split_reduce adds them in a fixed order.
//
//   k_rbf_h3_packed  8 waves, 512 rows, one workgroup per CU.  Both LDS images of a tile come pre-packed from k_pack_tiles and are
//                    staged by LDS-DMA; the distances run on the f16 MFMA (operand image bih, sign alternation); "wide" schedule;
//                    chain folds into LDS / register masters.  Needs the pack workspace; built for DPAD <= 16, or DPAD 32 with NB 1.
//   k_rbf_h3_split   4 waves, 256 rows, two workgroups per CU.  Staging through registers with the hi / lo split of the probe tile in
//                    the kernel; the distances stay on the fp32 MFMA (a round-to-nearest fmaf chain; the f16 MFMA truncates its
//                    internal sum, tools/mfma_f16_rounding.hip); two-phase schedule.  All the work without the pack workspace.
//
// f16 range guard, the hand-over between the two: when a scaled input is too large for the f16 image of the distance operands
// (|x/l|^2 beyond ~6e4 / |c|), k_pack_tiles raises the range flag.  With a pack workspace both kernels are launched, one behind
// the other: the packed kernel returns at once if the flag is SET, the split kernel returns at once if it is CLEAR -- correct for
// any input, no host round trip, one empty launch per matvec.  Without a workspace rangeflag is null and the split kernel runs.
//
// Both take the same argument list (RbfMatvecArgs): rows [row0, rend) of the operator (a row shard, or all of it; row0 % 64 == 0),
// x and the packed tile images cover all n columns, y / part are indexed from row0.  The split kernel ignores pkv / pka.
// ================================================================================================
constexpr int kH3MI = 2, kH3TJ = 64;                  // 32-row blocks per wave; columns per staged tile
// waves per workgroup: the packed kernel runs 8 waves (512 rows) on ONE staged tile -- the same two waves per SIMD as two 4-wave
// workgroups, but half the L2 -> LDS traffic and half the LDS tile copies
constexpr int kH3WavesPacked = 8, kH3WavesSplit = 4;

// ---- packed: pre-packed tile images by LDS-DMA, f16 distances, wide schedule, chain folds -------------------------------------
template <int DPAD, int NB, bool VEC4, int KIND>
__global__ __launch_bounds__(64 * kH3WavesPacked, 1) void k_rbf_h3_packed(const float* __restrict__ xs, const float* __restrict__ sq,
                                                              int64_t n, const float* __restrict__ outputscale,
                                                              const float* __restrict__ noise,
                                                              const float* __restrict__ vscale,
                                                              const float* __restrict__ x, int64_t ldx,
                                                              float* __restrict__ y, int64_t ldy, int64_t p,
                                                              const uintx4* __restrict__ pkv, const uintx4* __restrict__ pka,
                                                              float* __restrict__ part, const int* __restrict__ rangeflag,
                                                              int64_t ldpart, int64_t row0, int64_t rend) {
  if (rangeflag && *rangeflag != 0) return;  // f16 range guard: the split kernel behind this launch does the work
  constexpr int kMI = kH3MI, kTJ = kH3TJ, WV = kH3WavesPacked;
  using Tile = RbfTileH3<DPAD, NB, kTJ, false>;
  constexpr int KD = Tile::KD, NKD = Tile::NKD;
  extern __shared__ __attribute__((aligned(16))) char h3_smem[];
  Tile* const tile = reinterpret_cast<Tile*>(h3_smem);  // [2]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  // master accumulators of the chain folds: blocks 0 .. kMI NB - 2 in LDS behind the tiles, the last one in registers
  constexpr int kBlocks = kMI * NB;
  float* const master = reinterpret_cast<float*>(h3_smem + 2 * sizeof(Tile)) + ((size_t)wid * (kBlocks - 1) * 16) * 64 + lane;
  float mreg[16];
  const int64_t i_wave = row0 + (int64_t)blockIdx.x * (WV * kMI * 32) + (int64_t)wid * (kMI * 32);
  const int64_t b0 = (int64_t)blockIdx.y * (NB * 32);

  // B operand of the distance product, resident in registers: the f16 image [Bh | Bl | Bh | 0] of the 3-product split of
  //   [x_i, 1, |x_i|^2] (slot c*KD + k pairs with [Ah | Ah | Al] of the column operand), NEGATED for the odd row block: together
  //   with the columns' sign (odd column block negated by k_pack_tiles) the distance comes out as (-1)^(jb+mi) t, so the f16 MFMA's
  //   round-toward-minus-infinity bias enters K with alternating sign over the 32x32 blocks instead of coherently.
  half8 bih[kMI][NKD];
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi) {
    int64_t i = i_wave + mi * 32 + l31;
    if (i >= rend) i = rend - 1;
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
  floatx16 acc[kMI][NB];
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][nb][r] = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) mreg[r] = 0.f;
#pragma unroll
  for (int q = 0; q < (kBlocks - 1) * 16; ++q) master[q * 64] = 0.f;
  auto fold_chain = [&]() {  // masters += accumulators; accumulators restart from zero
#pragma unroll
    for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int idx = mi * NB + nb;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (idx < kBlocks - 1) {
            float* m = master + (idx * 16 + r) * 64;
            *m += acc[mi][nb][r];
          } else {
            mreg[r] += acc[mi][nb][r];
          }
          acc[mi][nb][r] = 0.f;
        }
      }
  };

  // ---- both LDS images come PRE-PACKED from k_pack_tiles (once per matvec instead of once per workgroup and tile: the hi/lo
  //      split of the probe tile was 40 of the ~93 VALU instructions per 32x32 block, and VALU time adds to MFMA time).
  //      A tile's probe image is 2 x 8 rows x P packs of 16 B (hi rows, then lo rows), its column operand 64 x AROW halves.
  constexpr int kVPK = 2 * 8 * Tile::P;                 // 16-B packs of the probe image per tile
  constexpr int kAPK = kTJ * Tile::AROW * 2 / 16;       // 16-B packs of the column operand per tile
  static_assert(kVPK % 64 == 0 && kAPK % 64 == 0, "tile images are whole 1-KiB DMA pieces");
  const int64_t ntile_all = (n + kTJ - 1) / kTJ;
  // LDS-DMA of tile t's two images straight into the tile buffer: wave w copies the 1-KiB pieces w, w + WV, ...; no staging
  // registers, no ds_write (less data movement is what still buys time on this power-limited kernel)
  auto issue_tile_dma = [&](int64_t t, Tile& tl) {
    const char* vsrc = reinterpret_cast<const char*>(pkv + ((int64_t)blockIdx.y * ntile_all + t) * kVPK);
    const char* asrc = reinterpret_cast<const char*>(pka + t * kAPK);
    char* vdst = reinterpret_cast<char*>(&tl.vhi[0][0]);  // vhi and vlo are contiguous (no row pad in this layout)
    char* adst = reinterpret_cast<char*>(&tl.ajh[0][0]);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int c = 0; c < (kVPK / 64 + WV - 1) / WV; ++c) {
      const int piece = w + WV * c;
      if (piece < kVPK / 64) glds16(vsrc + piece * 1024 + lane * 16, vdst + piece * 1024);
    }
#pragma unroll
    for (int c = 0; c < (kAPK / 64 + WV - 1) / WV; ++c) {
      const int piece = w + WV * c;
      if (piece < kAPK / 64) glds16(asrc + piece * 1024 + lane * 16, adst + piece * 1024);
    }
  };

  // entries (2 pr, 2 pr + 1) of a distance block: K' = exp2(min(arg, 15)) and its hi/lo f16 pieces.  min as ONE compiler-visible
  // v_med3_f32 (fminf adds a canonicalising v_max; inline asm would hide the MFMA-result hazard from hipcc).
  // `neg`: this block's distances were produced negated (sign alternation); the sign is a free source modifier.
  // The same text in both kernels of the pair: as a shared helper it changed the register allocation of Matern-5/2 instances
  auto exp_split_pair = [&](const floatx16& kd, int pr, const bool diag_blk, const bool neg, half8 (&ah)[2], half8 (&al)[2]) {
    const int s = pr >> 2, q = (pr & 3) * 2;
    float k0, k1;
    const float d0 = neg ? -kd[8 * s + q] : kd[8 * s + q];
    const float d1 = neg ? -kd[8 * s + q + 1] : kd[8 * s + q + 1];
    if constexpr (KIND == MFX_KERNEL_RBF) {
      if constexpr (kClampRbf) {
        k0 = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(d0, -3.0e38f, kKShift));
        k1 = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(d1, -3.0e38f, kKShift));
      } else {
        k0 = __builtin_amdgcn_exp2f(d0);
        k1 = __builtin_amdgcn_exp2f(d1);
      }
    } else {
      // register r <-> column (r & 3) + 8 (r >> 2) + 4 lhi of the block: zero self-distance on the diagonal block
      const int r0 = 8 * s + q, r1 = r0 + 1;
      const float t0 = (diag_blk && l31 == (r0 & 3) + 8 * (r0 >> 2) + 4 * lhi) ? kEpsC : d0;
      const float t1 = (diag_blk && l31 == (r1 & 3) + 8 * (r1 >> 2) + 4 * lhi) ? kEpsC : d1;
      k0 = matern_from_te<KIND>(t0, 32768.f);
      k1 = matern_from_te<KIND>(t1, 32768.f);
    }
    const half2v h = {(_Float16)k0, (_Float16)k1};  // one v_cvt_pk_f16_f32 (round to nearest)
    // lo = k - hi in ONE instruction each: v_fma_mix_f32 reads the f16 half directly (no v_cvt_f32_f16 + v_sub).
    // Inputs/outputs are VALU values only, so no MFMA hazard hides inside the asm.
    float l0, l1;
    const unsigned hb = __builtin_bit_cast(unsigned, h);
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hb), "v"(k0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hb), "v"(k1));
    const half2v l = {(_Float16)l0, (_Float16)l1};
    ah[s][q] = h[0]; ah[s][q + 1] = h[1];
    al[s][q] = l[0]; al[s][q + 1] = l[1];
  };

  const int64_t ntile_tot = (n + kTJ - 1) / kTJ;
  const int64_t t_first = ntile_tot * blockIdx.z / gridDim.z, ntile = ntile_tot * (blockIdx.z + 1) / gridDim.z;
  issue_tile_dma(t_first, tile[t_first & 1]);
  __syncthreads();
  for (int64_t t = t_first; t < ntile; ++t) {
    const Tile& tl = tile[t & 1];
    if (t > t_first && ((t - t_first) % kChainTiles) == 0) fold_chain();
    // the other buffer was last read during tile t - 1, and every wave has passed the barrier that ended it
    if (t + 1 < ntile) issue_tile_dma(t + 1, tile[(t + 1) & 1]);
    // the one tile whose 64 columns are this wave's 64 rows holds the diagonal: only there (and only for the Matern
    // kernels) the per-entry self-distance fix is compiled in -- two copies of the tile body, chosen wave-uniformly
    auto do_tile = [&](auto diag_tag) {
      constexpr bool kDiag = decltype(diag_tag)::value;
      // ---- wide schedule: the exp / split of block b+1 is spread over ALL contraction MFMAs of block b (its distances were
      //      issued during block b-1), so the VALU stream runs beside the matrix pipe for the whole block instead of half of it
      //      (PMC: 29 % of the MFMA-busy cycles co-executed with VALU under the two-phase schedule) ----------------------
      half8 ah[2], al[2];
      floatx16 kdn;
      // column-operand fragments of one 32-column block (shared by its two row blocks: one LDS read per column block)
      half8 ajs[NKD];
      auto load_a = [&](int jbx) {
#pragma unroll
        for (int q = 0; q < NKD; ++q) ajs[q] = *reinterpret_cast<const half8*>(&tl.ajh[jbx * 32 + l31][q * 16 + lhi * 8]);
      };
      auto dist = [&](floatx16& kd, int mix) {
#pragma unroll
        for (int r = 0; r < 16; ++r) kd[r] = 0.f;
#pragma unroll
        for (int q = 0; q < NKD; ++q) kd = __builtin_amdgcn_mfma_f32_32x32x16_f16(ajs[q], bih[mix][q], kd, 0, 0, 0);
      };
      // B fragments (probe tile) of a block are fetched from LDS one block ahead: the ds_read latency in front of the first MFMA
      // of every block was ~10 % of the tile
      half8 bhb[2][2][NB], blb[2][2][NB];
      auto load_b = [&](int buf, int jbx) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const int row = (jbx * 2 + s) * 2 + lhi;
            bhb[buf][s][nb] = *reinterpret_cast<const half8*>(&tl.vhi[row][(nb * 32 + l31) * 8]);
            blb[buf][s][nb] = *reinterpret_cast<const half8*>(&tl.vlo[row][(nb * 32 + l31) * 8]);
          }
      };
      constexpr bool kPrefB = DPAD <= 16 && (NB == 1 || DPAD <= 8);  // elsewhere the second fragment set does not fit in 256 VGPRs
      if (kPrefB) load_b(0, 0);
      {
        static_assert(kMI == 2, "block order (jb, mi) = (0,0), (0,1), (1,0), (1,1)");
        floatx16 kd;
        load_a(0);
        dist(kd, 0);
        dist(kdn, 1);
#pragma unroll
        for (int pr = 0; pr < 8; ++pr) exp_split_pair(kd, pr, kDiag, false, ah, al);
      }
#pragma unroll
      for (int blk = 0; blk < 2 * kMI; ++blk) {
        const int jb = blk / kMI, mi = blk % kMI;
        constexpr int NM = 6 * NB;
        constexpr int MD = NM - NKD - 1;  // the distance MFMAs of block b+2 go behind contraction MFMAs MD .. MD+NKD-1
        const bool has_next = blk + 1 < 2 * kMI, has_next2 = blk + 2 < 2 * kMI;
        const int jbn = (blk + 1) / kMI, min_ = (blk + 1) % kMI;
        const int jb2 = (blk + 2) / kMI, mi2 = (blk + 2) % kMI;
        // the two row blocks of a column block share its probe fragments: one LDS read per column block, not per block
        const int cur = kPrefB ? (jb & 1) : 0;
        if (!kPrefB && mi == 0) load_b(0, jb);
        if (has_next2 && mi2 == 0) load_a(jb2);  // blocks (jb2, 0) and (jb2, 1) are issued from blocks blk and blk + 1
        const bool negn = ((jbn + min_) & 1) != 0;
        floatx16 kdn2;
#pragma unroll
        for (int r = 0; r < 16; ++r) kdn2[r] = 0.f;
        half8 ahn[2], aln[2];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const int s = m / (3 * NB), nb = (m / 3) % NB, w = m % 3;
          __builtin_amdgcn_sched_barrier(0);
          acc[mi][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w == 2 ? al[s] : ah[s], w == 1 ? blb[cur][s][nb] : bhb[cur][s][nb],
                                                               acc[mi][nb], 0, 0, 0);
          if constexpr (MD >= 0) {
            if (has_next2 && m >= MD && m - MD < NKD)
              kdn2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ajs[m - MD], bih[mi2][m - MD], kdn2, 0, 0, 0);
          } else {  // more distance MFMAs than contraction slots behind which to hide them (DPAD 32, one probe block: 7 against 6): spread evenly
            if (has_next2) {
#pragma unroll
              for (int q = 0; q < NKD; ++q)
                if (q >= NKD * m / NM && q < NKD * (m + 1) / NM)
                  kdn2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ajs[q], bih[mi2][q], kdn2, 0, 0, 0);
            }
          }
          if (kPrefB && m == 0 && blk == 0 && 2 * kMI > kMI) load_b(1, 1);  // the second column block's fragments, two blocks ahead
          __builtin_amdgcn_sched_barrier(0);
          if (has_next) {
#pragma unroll
            for (int pr = 0; pr < 8; ++pr)
              if (pr >= 8 * m / NM && pr < 8 * (m + 1) / NM)
                exp_split_pair(kdn, pr, kDiag && jbn == min_, negn, ahn, aln);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (has_next) {
          ah[0] = ahn[0]; ah[1] = ahn[1];
          al[0] = aln[0]; al[1] = aln[1];
          kdn = kdn2;
        }
      }
    };
    if (KIND != MFX_KERNEL_RBF && t * kTJ == i_wave) {
      do_tile(std::true_type{});
    } else {
      do_tile(std::false_type{});
    }
    __syncthreads();  // (also drains the LDS-DMA: vmcnt(0))
  }
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int idx = mi * NB + nb;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][nb][r] += idx < kBlocks - 1 ? master[(idx * 16 + r) * 64] : mreg[r];
    }
  // epilogue: out[b][i] = s / (vscale_b 2^15) * acc + noise * x[b][i], to y or (column split: no noise term) to this split's slab of
  // part.  D layout: col = lane & 31 (probe), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  The same text in both kernels of the pair:
  // as a shared helper it compiled to different code in the two-probe-block instances ("h3 pair")
  const float s = outputscale[0], nz = gridDim.z > 1 ? 0.f : noise[0];
  float* yout = gridDim.z > 1 ? part + (int64_t)blockIdx.z * p * ldpart : y;
  const int64_t ldo = gridDim.z > 1 ? ldpart : ldy;
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int64_t b = b0 + nb * 32 + l31;
      if (b >= p) continue;
      const float sb = s * vscale[2 * b + 1] * (1.f / 32768.f);
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

// ---- in-kernel split: staging through registers, fp32 distances, two-phase schedule ------------------------------------------
//   phase 1:  the fp32 distance MFMAs of block b+1 (FP32 lanes)  ||  the first half of block b's f16 contraction MFMAs (matrix pipe)
//   phase 2:  the exp / hi-lo split of block b+1 (VALU, FP32 lanes)  ||  the second half of block b's MFMAs
template <int DPAD, int NB, bool VEC4, int KIND>
__global__ __launch_bounds__(64 * kH3WavesSplit, 2) void k_rbf_h3_split(const float* __restrict__ xs, const float* __restrict__ sq,
                                                              int64_t n, const float* __restrict__ outputscale,
                                                              const float* __restrict__ noise,
                                                              const float* __restrict__ vscale,
                                                              const float* __restrict__ x, int64_t ldx,
                                                              float* __restrict__ y, int64_t ldy, int64_t p,
                                                              const uintx4* __restrict__ pkv, const uintx4* __restrict__ pka,
                                                              float* __restrict__ part, const int* __restrict__ rangeflag,
                                                              int64_t ldpart, int64_t row0, int64_t rend) {
  if (rangeflag && *rangeflag == 0) return;  // f16 range guard: the packed kernel in front of this launch did the work
  constexpr int kMI = kH3MI, kTJ = kH3TJ, WV = kH3WavesSplit;
  using Tile = RbfTileH3<DPAD, NB, kTJ, true>;
  constexpr int KD = Tile::KD, KS = KD / 2;
  constexpr float cfac = KIND == MFX_KERNEL_RBF ? kNegHalfLog2e : matern_nu2<KIND>() * kLog2e * kLog2e;
  extern __shared__ __attribute__((aligned(16))) char h3_smem[];
  Tile* const tile = reinterpret_cast<Tile*>(h3_smem);  // [2]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int64_t i_wave = row0 + (int64_t)blockIdx.x * (WV * kMI * 32) + (int64_t)wid * (kMI * 32);
  const int64_t b0 = (int64_t)blockIdx.y * (NB * 32);

  // B operand of the distance product, resident in registers: [x_i, 1, |x_i|^2], one float per k-step (k = 2 s + lhi)
  float bi[kMI][KS];
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi) {
    int64_t i = i_wave + mi * 32 + l31;
    if (i >= rend) i = rend - 1;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 2 * s + lhi;
      bi[mi][s] = (k < DPAD) ? xs[i * DPAD + k] : (k == DPAD ? 1.f : sq[i]);
    }
  }
  floatx16 acc[kMI][NB];
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][nb][r] = 0.f;

  // ---- staging: registers <- global, LDS <- registers (scaled, split into hi / lo f16 on the way) ----------------------------
  constexpr int kF4 = NB * 32 * (kTJ / 4);
  constexpr int kVPT = (kF4 + 255) / 256;
  constexpr int kXPT = (kTJ * DPAD + 255) / 256;
  float4 rv[kVPT];
  float rx[kXPT], rsq = 0.f;
  float vs[kVPT];
#pragma unroll
  for (int u = 0; u < kVPT; ++u) {
    const int f = tid + 256 * u;
    const int64_t b = b0 + f / (kTJ / 4);
    vs[u] = (f < kF4 && b < p) ? vscale[2 * b] : 0.f;
  }

  auto load_tile = [&](int64_t j0) {
#pragma unroll
    for (int u = 0; u < kVPT; ++u) {
      const int f = tid + 256 * u;
      const int bq = f / (kTJ / 4), j4 = (f % (kTJ / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (f < kF4 && b0 + bq < p) {
        const float* src = x + (b0 + bq) * ldx + j0 + j4;
        if (VEC4 && j0 + j4 + 3 < n) {
          v = *reinterpret_cast<const float4*>(src);
        } else {
          if (j0 + j4 + 0 < n) v.x = src[0];
          if (j0 + j4 + 1 < n) v.y = src[1];
          if (j0 + j4 + 2 < n) v.z = src[2];
          if (j0 + j4 + 3 < n) v.w = src[3];
        }
      }
      rv[u] = v;
    }
#pragma unroll
    for (int u = 0; u < kXPT; ++u) {
      const int t = tid + 256 * u;
      const int64_t g = j0 * DPAD + t;
      rx[u] = (t < kTJ * DPAD && g < n * DPAD) ? xs[g] : 0.f;
    }
    if (tid < kTJ) rsq = (j0 + tid < n) ? sq[j0 + tid] : 0.f;
  };
  auto store_tile = [&](Tile& tl) {
#pragma unroll
    for (int u = 0; u < kVPT; ++u) {
      const int f = tid + 256 * u;
      if (f < kF4) {
        const int bq = f / (kTJ / 4), j4 = (f % (kTJ / 4)) * 4;
        const int row = ((j4 >> 5) * 2 + ((j4 >> 4) & 1)) * 2 + ((j4 >> 2) & 1);
        const int col = bq * 8 + 4 * ((j4 >> 3) & 1);
        float h0, h1, h2, h3, l0, l1, l2, l3;
        split_hi_lo(rv[u].x * vs[u], h0, l0);
        split_hi_lo(rv[u].y * vs[u], h1, l1);
        split_hi_lo(rv[u].z * vs[u], h2, l2);
        split_hi_lo(rv[u].w * vs[u], h3, l3);
        half4 hh = {(_Float16)h0, (_Float16)h1, (_Float16)h2, (_Float16)h3};
        half4 ll = {(_Float16)l0, (_Float16)l1, (_Float16)l2, (_Float16)l3};
        *reinterpret_cast<half4*>(&tl.vhi[row][col]) = hh;
        *reinterpret_cast<half4*>(&tl.vlo[row][col]) = ll;
      }
    }
#pragma unroll
    for (int u = 0; u < kXPT; ++u) {
      const int t = tid + 256 * u;
      if (t < kTJ * DPAD) tl.aj[t % DPAD][t / DPAD] = -2.f * cfac * rx[u];
    }
    if (tid < kTJ) {
      // K' = 2^15 K: lo(K') stays a NORMAL f16 for K >= 4e-6 (RBF: shift folded into the product; Matern: into exp2)
      tl.aj[DPAD][tid] = cfac * rsq + (KIND == MFX_KERNEL_RBF ? kKShift : kEpsC);
      tl.aj[DPAD + 1][tid] = cfac;
    }
  };

  // entries (2 pr, 2 pr + 1) of a distance block: K' = exp2(min(arg, 15)) and its hi/lo f16 pieces.  min as ONE compiler-visible
  // v_med3_f32 (fminf adds a canonicalising v_max; inline asm would hide the MFMA-result hazard from hipcc).
  // The same text in both kernels of the pair: as a shared helper it changed the register allocation of Matern-5/2 instances
  auto exp_split_pair = [&](const floatx16& kd, int pr, const bool diag_blk, half8 (&ah)[2], half8 (&al)[2]) {
    const int s = pr >> 2, q = (pr & 3) * 2;
    float k0, k1;
    const float d0 = kd[8 * s + q], d1 = kd[8 * s + q + 1];
    if constexpr (KIND == MFX_KERNEL_RBF) {
      if constexpr (kClampRbf) {
        k0 = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(d0, -3.0e38f, kKShift));
        k1 = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(d1, -3.0e38f, kKShift));
      } else {
        k0 = __builtin_amdgcn_exp2f(d0);
        k1 = __builtin_amdgcn_exp2f(d1);
      }
    } else {
      // register r <-> column (r & 3) + 8 (r >> 2) + 4 lhi of the block: zero self-distance on the diagonal block
      const int r0 = 8 * s + q, r1 = r0 + 1;
      const float t0 = (diag_blk && l31 == (r0 & 3) + 8 * (r0 >> 2) + 4 * lhi) ? kEpsC : d0;
      const float t1 = (diag_blk && l31 == (r1 & 3) + 8 * (r1 >> 2) + 4 * lhi) ? kEpsC : d1;
      k0 = matern_from_te<KIND>(t0, 32768.f);
      k1 = matern_from_te<KIND>(t1, 32768.f);
    }
    const half2v h = {(_Float16)k0, (_Float16)k1};  // one v_cvt_pk_f16_f32 (round to nearest)
    // lo = k - hi in ONE instruction each: v_fma_mix_f32 reads the f16 half directly (no v_cvt_f32_f16 + v_sub).
    // Inputs/outputs are VALU values only, so no MFMA hazard hides inside the asm.
    float l0, l1;
    const unsigned hb = __builtin_bit_cast(unsigned, h);
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hb), "v"(k0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hb), "v"(k1));
    const half2v l = {(_Float16)l0, (_Float16)l1};
    ah[s][q] = h[0]; ah[s][q + 1] = h[1];
    al[s][q] = l[0]; al[s][q + 1] = l[1];
  };

  const int64_t ntile_tot = (n + kTJ - 1) / kTJ;
  const int64_t t_first = ntile_tot * blockIdx.z / gridDim.z, ntile = ntile_tot * (blockIdx.z + 1) / gridDim.z;
  load_tile(t_first * kTJ);
  store_tile(tile[t_first & 1]);
  __syncthreads();
  for (int64_t t = t_first; t < ntile; ++t) {
    const Tile& tl = tile[t & 1];
    if (t + 1 < ntile) load_tile((t + 1) * kTJ);
    // the one tile whose 64 columns are this wave's 64 rows holds the diagonal: only there (and only for the Matern
    // kernels) the per-entry self-distance fix is compiled in -- two copies of the tile body, chosen wave-uniformly
    auto do_tile = [&](auto diag_tag) {
      constexpr bool kDiag = decltype(diag_tag)::value;
      half8 ah[2], al[2];
      {  // pipeline prologue: fragments of block 0 of this tile
        floatx16 kd;
#pragma unroll
        for (int r = 0; r < 16; ++r) kd[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) kd = __builtin_amdgcn_mfma_f32_32x32x2f32(tl.aj[2 * s + lhi][l31], bi[0][s], kd, 0, 0, 0);
#pragma unroll
        for (int pr = 0; pr < 8; ++pr) exp_split_pair(kd, pr, kDiag, ah, al);  // block (jb 0, mi 0): the diagonal one in that tile
      }
#pragma unroll
      for (int blk = 0; blk < 2 * kMI; ++blk) {
        const int jb = blk / kMI, mi = blk % kMI;
        constexpr int NM = 6 * NB;       // contraction MFMAs of this block
        constexpr int NM1 = NM / 2;      // issued in phase 1, next to the distance MFMAs
        const bool has_next = blk + 1 < 2 * kMI;
        const int jbn = (blk + 1) / kMI, min_ = (blk + 1) % kMI;
        half8 bh[2][NB], bl[2][NB];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const int row = (jb * 2 + s) * 2 + lhi;
            bh[s][nb] = *reinterpret_cast<const half8*>(&tl.vhi[row][(nb * 32 + l31) * 8]);
            bl[s][nb] = *reinterpret_cast<const half8*>(&tl.vlo[row][(nb * 32 + l31) * 8]);
          }
        float ajn[KS];
        if (has_next) {
#pragma unroll
          for (int s = 0; s < KS; ++s) ajn[s] = tl.aj[2 * s + lhi][jbn * 32 + l31];
        }
        floatx16 kdn;
#pragma unroll
        for (int r = 0; r < 16; ++r) kdn[r] = 0.f;
        half8 ahn[2], aln[2];
        auto contraction = [&](int m) {
          const int s = m / (3 * NB), nb = (m / 3) % NB, w = m % 3;
          acc[mi][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w == 2 ? al[s] : ah[s], w == 1 ? bl[s][nb] : bh[s][nb],
                                                               acc[mi][nb], 0, 0, 0);
        };
        // ---- phase 1: the distance MFMAs of the next block, issued as early as possible (two per
        //      contraction MFMA) so that their result latency is covered by the rest of phase 1 -------
#pragma unroll
        for (int m = 0; m < NM1; ++m) {
          __builtin_amdgcn_sched_barrier(0);
          contraction(m);
          if (has_next) {
#pragma unroll
            for (int s = 0; s < KS; ++s)
              if (s >= 2 * m && s < 2 * (m + 1))
                kdn = __builtin_amdgcn_mfma_f32_32x32x2f32(ajn[s], bi[min_][s], kdn, 0, 0, 0);
          }
        }
        if (has_next) {  // distance steps that did not fit next to the NM1 contraction MFMAs (d > 8 with one probe block)
#pragma unroll
          for (int s = 2 * NM1; s < KS; ++s) kdn = __builtin_amdgcn_mfma_f32_32x32x2f32(ajn[s], bi[min_][s], kdn, 0, 0, 0);
        }
        // ---- phase 2: exp / split of the next block between the remaining contraction MFMAs -------
#pragma unroll
        for (int m = NM1; m < NM; ++m) {
          __builtin_amdgcn_sched_barrier(0);
          contraction(m);
          __builtin_amdgcn_sched_barrier(0);
          if (has_next) {
#pragma unroll
            for (int pr = 0; pr < 8; ++pr)
              if (pr >= 8 * (m - NM1) / (NM - NM1) && pr < 8 * (m - NM1 + 1) / (NM - NM1))
                exp_split_pair(kdn, pr, kDiag && jbn == min_, ahn, aln);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (has_next) {
          ah[0] = ahn[0]; ah[1] = ahn[1];
          al[0] = aln[0]; al[1] = aln[1];
        }
      }
    };
    if (KIND != MFX_KERNEL_RBF && t * kTJ == i_wave) {
      do_tile(std::true_type{});
    } else {
      do_tile(std::false_type{});
    }
    if (t + 1 < ntile) store_tile(tile[(t + 1) & 1]);
    __syncthreads();
  }
  // epilogue: out[b][i] = s / (vscale_b 2^15) * acc + noise * x[b][i], to y or (column split: no noise term) to this split's slab of
  // part.  D layout: col = lane & 31 (probe), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  The same text in both kernels of the pair:
  // as a shared helper it compiled to different code in the two-probe-block instances ("h3 pair")
  const float s = outputscale[0], nz = gridDim.z > 1 ? 0.f : noise[0];
  float* yout = gridDim.z > 1 ? part + (int64_t)blockIdx.z * p * ldpart : y;
  const int64_t ldo = gridDim.z > 1 ? ldpart : ldy;
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int64_t b = b0 + nb * 32 + l31;
      if (b >= p) continue;
      const float sb = s * vscale[2 * b + 1] * (1.f / 32768.f);
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

// y = sum_z part[z] + noise x   (fixed summation order: deterministic)
__global__ __launch_bounds__(256) void k_split_reduce(const float* __restrict__ part, int64_t ldpart, int nsplit, int64_t p,
                                                      int64_t nrow, int64_t ldy, const float* __restrict__ noise,
                                                      const float* __restrict__ x, int64_t ldx, float* __restrict__ y,
                                                      int64_t row0) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;  // local row: the point is row0 + i
  if (i >= nrow) return;
  float acc = 0.f;
  for (int z = 0; z < nsplit; ++z) acc += part[((int64_t)z * p + b) * ldpart + i];
  y[b * ldy + i] = fmaf(noise[0], x[b * ldx + row0 + i], acc);
}

// ------------------------------------------------------------------------------------------------
// Pre-pass of the pipelined matvec: the LDS images of every 64-column tile, written ONCE per matvec.
//   probe image   pkv[chunk][tile][lo?][row (jb, s, h)][probe][8]  : 16-B packs = the MFMA B fragments (hi / lo f16 of the scaled
//                 probe values of columns j = 32 jb + 16 s + 8 (e >> 2) + 4 h + (e & 3), e = 0..7)
//   column operand pka[tile][j][AROW] : [Ah | Ah | Al | 0] of c [-2 x_j, |x_j|^2 (+ shift or eps), 1], odd 32-column block negated
// grid (ntile, chunks + 1): blockIdx.y < chunks packs that probe chunk, the last one the column operand.
// ------------------------------------------------------------------------------------------------
template <int DPAD, int NB, int KIND>
__global__ __launch_bounds__(256) void k_pack_tiles(const float* __restrict__ xs, const float* __restrict__ sq, int64_t n,
                                                    float* __restrict__ vscale, const float* __restrict__ amax_part, int gx,
                                                    const float* __restrict__ x, int64_t ldx, int64_t p,
                                                    uintx4* __restrict__ pkv, uintx4* __restrict__ pka, int* __restrict__ rangeflag) {
  constexpr int kTJ = 64;
  using Tile = RbfTileH3<DPAD, NB, kTJ>;
  constexpr int KD = Tile::KD, P = Tile::P, AROW = Tile::AROW;
  constexpr float cfac = KIND == MFX_KERNEL_RBF ? kNegHalfLog2e : matern_nu2<KIND>() * kLog2e * kLog2e;
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x, j0 = t * kTJ, ntile = gridDim.x;
  if ((int)blockIdx.y < (int)gridDim.y - 1) {
    const int64_t b0 = (int64_t)blockIdx.y * P;
    uintx4* dst = pkv + ((int64_t)blockIdx.y * ntile + t) * (2 * 8 * P);
    // the power-of-two scales of this chunk's vectors from their slice maxima (k_row_amax_part); tile 0 publishes [s, 1/s] for the
    // epilogue of the matvec kernel
    __shared__ float svs[P];
    if (tid < P) {
      const int64_t b = b0 + tid;
      float sc = 0.f;
      if (b < p) {
        float m = 0.f;
        for (int g = 0; g < gx; ++g) m = fmaxf(m, amax_part[b * gx + g]);
        sc = row_scale_of(m);
        if (t == 0) {
          vscale[2 * b] = sc;
          vscale[2 * b + 1] = 1.f / sc;
        }
      }
      svs[tid] = sc;
    }
    __syncthreads();
    for (int f0 = tid; f0 < 8 * P; f0 += 256) {
      // 8 consecutive lanes read the 64 consecutive columns (256 B) of ONE probe row; the 16-B stores of a lane group land in
      // 8 different image rows, 8 consecutive probes each (a first version with lanes along the probes read 4 B per 512-KB
      // stride and cost a millisecond)
      const int row = f0 & 7, bq = f0 >> 3, f = row * P + bq;
      const int jb = row >> 2, s = (row >> 1) & 1, h = row & 1;
      const int64_t b = b0 + bq;
      half8 hh, ll;
      const float vs = svs[bq];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t j = j0 + 32 * jb + 16 * s + 8 * (e >> 2) + 4 * h + (e & 3);
        const float v = (b < p && j < n) ? x[b * ldx + j] * vs : 0.f;
        float fh, fl;
        split_hi_lo(v, fh, fl);
        hh[e] = (_Float16)fh;
        ll[e] = (_Float16)fl;
      }
      dst[f] = __builtin_bit_cast(uintx4, hh);
      dst[8 * P + f] = __builtin_bit_cast(uintx4, ll);
    }
  } else {
    __shared__ __attribute__((aligned(16))) _Float16 img[kTJ][AROW];
    for (int e = tid; e < kTJ * AROW; e += 256) (&img[0][0])[e] = (_Float16)0.f;
    __syncthreads();
    for (int e = tid; e < kTJ * KD; e += 256) {
      const int j = e / KD, kk = e % KD;
      const int64_t jg = j0 + j;
      float v;
      if (kk < DPAD) v = jg < n ? -2.f * cfac * xs[jg * DPAD + kk] : 0.f;
      else if (kk == DPAD) v = cfac * (jg < n ? sq[jg] : 0.f) + (KIND == MFX_KERNEL_RBF ? kKShift : kEpsC);
      else v = cfac;
      // largest magnitudes of the f16 images: this column-operand entry, and |x_j|^2 itself as a row-operand entry
      if (fabsf(v) > 6.0e4f || (kk == DPAD && jg < n && sq[jg] > 6.0e4f)) atomicOr(rangeflag, 1);
      float hi, lo;
      split_hi_lo(((j >> 5) & 1) ? -v : v, hi, lo);
      img[j][kk] = (_Float16)hi;
      img[j][KD + kk] = (_Float16)hi;
      img[j][2 * KD + kk] = (_Float16)lo;
    }
    __syncthreads();
    uintx4* dst = pka + t * (kTJ * AROW * 2 / 16);
    for (int f = tid; f < kTJ * AROW * 2 / 16; f += 256) dst[f] = reinterpret_cast<const uintx4*>(&img[0][0])[f];
  }
}

// Which kernel runs the chunks (of 64 vectors, or one of at most 32) of an RBF operator with d <= 16 (BASELINE config 4's matvec,
// config 2's): the fat-wave kernels (mfx_rbf_fat.hip: one wave per SIMD; the 32x32x16 form at 64 vectors: 82 % matrix-pipe share,
// -16 % cycles against h3; the 16x16x32 form: DESIGN.md §3.2).  The one A/B switch kept, MFX_RBF_FAT:
//   0  the same-program kernel k_rbf_h3_packed (two waves per SIMD) for every shape -- reproduces the comparison of DESIGN.md
//      §3.2 and the bit-identity test of the two kernels; h3 also takes every other shape;
//   1  k_rbf_fat_apply (v_mfma_f32_32x32x16_f16) for every shape the fat-wave form takes;
//   2  as 1, but d <= 8 with 64-wide chunks on k_rbf_fat_apply16 (v_mfma_f32_16x16x32_f16).
constexpr int kRbfFatDefault = 2;
static int rbf_fat() {
  static const int v = [] {
    const char* e = getenv("MFX_RBF_FAT");
    const int m = e ? atoi(e) : kRbfFatDefault;
    return m == 0 || m == 1 ? m : 2;
  }();
  return v;
}

// vectors per chunk of the pre-packed matvec: 64 from 33 vectors on; DPAD = 32 is built with one probe block per chunk only (the
// tile images and the chain masters of two blocks do not fit the 160 KB of LDS)
static int64_t chunk_width(int64_t p, int dpad) { return (p <= 32 || dpad > 16) ? 32 : 64; }

// column splits of the pipelined matvec (grid.z), for OCCUPANCY: too few 512-row workgroups to fill 256 CUs (small n, or a row
// shard of a large n).  512-row workgroups of 8 waves, one per CU and round: with s column splits the launch takes
// ceil(wgs s / 256) rounds of 1/s of the columns each; pick the s (at most 16, at least 8 tiles per split) that minimises
// rounds / s, plus a small charge per split for the prologue and the partial sums.  (n = 45 730: 90 row blocks -> s = 8, 720
// workgroups in 3 rounds = 0.375 of an unsplit launch, where "fill one round" (s = 2) gives 0.5.)
static int rbf_split_count(int64_t nrow, int64_t n, int64_t p, int dpad) {
  static const int forced = [] {
    const char* e = getenv("MFX_RBF_SPLIT");  // A/B: force the split count
    return e ? atoi(e) : 0;
  }();
  const int64_t pw = chunk_width(p, dpad);
  const int64_t wgs = ((nrow + 511) / 512) * ((p + pw - 1) / pw);
  const int64_t ntile = (n + 63) / 64;
  int64_t smax = ntile / 8;
  if (forced > 0) return forced <= 16 && forced <= ntile ? forced : 1;
  if (smax > 16) smax = 16;
  if (smax < 1 || wgs >= 2048) return 1;
  int best = 1;
  double best_cost = 1e30;
  for (int s = 1; s <= (int)smax; ++s) {
    const double rounds = (double)((wgs * s + 255) / 256);
    const double cost = rounds / s + 0.004 * s;
    if (cost < best_cost - 1e-12) {
      best_cost = cost;
      best = s;
    }
  }
  return best;
}

RbfPackLayout rbf_pack_layout(int64_t n, int64_t nrow, int64_t p, int dpad) {
  RbfPackLayout k;
  k.P = chunk_width(p, dpad);
  k.chunks = (p + k.P - 1) / k.P;
  k.ntile = (n + 63) / 64;
  const int64_t arow = ((3 * (dpad + 2) + 15) / 16) * 16 + 8;  // RbfTileH3::AROW
  k.off_a = align_up(k.chunks * k.ntile * 2 * 8 * k.P * 16, 256);
  k.off_part = k.off_a + align_up(k.ntile * 64 * arow * 2, 256);
  k.nsplit = rbf_split_count(nrow, n, p, dpad);
  k.ldpart = align_up(nrow, 4);  // the partials have their own stride (any n, any ldy)
  k.bytes = k.off_part + align_up((int64_t)k.nsplit * p * k.ldpart * 4, 256);
  return k;
}
int64_t rbf_pack_ws_bytes(const mfx_operator* op, int64_t p) {
  if (op->dtype != MFX_F32 || op->d > 32 || p < 1) return 0;
  return rbf_pack_layout(op->n, op_nrows(op), p, rbf_dpad(op->d)).bytes;
}

// the one launch site of the h3 pair: `kernel` = an instance of k_rbf_h3_packed or k_rbf_h3_split, with its wave count and LDS bytes
template <class Kernel>
static int launch_h3(Kernel kernel, int waves, size_t lds, dim3 grid, hipStream_t stream, const RbfMatvecArgs& a) {
  MFX_TRY(allow_big_lds(kernel, lds));
  kernel<<<grid, 64 * waves, lds, stream>>>(a.xs, a.sq, a.n, a.outputscale, a.noise, a.vscale, a.x, a.ldx, a.y, a.ldy, a.p,
                                            static_cast<const uintx4*>(a.pkv), static_cast<const uintx4*>(a.pka), a.part, a.rangeflag,
                                            a.ldpart, a.row0, a.rend);
  return MFX_OK;
}
// LDS: the two tile buffers + the chain masters of 8 waves x (2 NB - 1) blocks x 16 registers x 64 lanes
template <int DPAD, int NB, int KIND>
static int launch_h3_packed(bool vec4, dim3 grid, hipStream_t stream, const RbfMatvecArgs& a) {
  constexpr size_t kSm = 2 * sizeof(RbfTileH3<DPAD, NB, kH3TJ, false>) + (size_t)kH3WavesPacked * (kH3MI * NB - 1) * 16 * 64 * 4;
  return with_bool(vec4, [&](auto v4) -> int {
    return launch_h3(k_rbf_h3_packed<DPAD, NB, decltype(v4)::value, KIND>, kH3WavesPacked, kSm, grid, stream, a);
  });
}
// LDS: the two tile buffers
template <int DPAD, int NB, int KIND>
static int launch_h3_split(bool vec4, dim3 grid, hipStream_t stream, const RbfMatvecArgs& a) {
  constexpr size_t kSm = 2 * sizeof(RbfTileH3<DPAD, NB, kH3TJ, true>);
  return with_bool(vec4, [&](auto v4) -> int {
    return launch_h3(k_rbf_h3_split<DPAD, NB, decltype(v4)::value, KIND>, kH3WavesSplit, kSm, grid, stream, a);
  });
}

template <int DPAD, int NB, int KIND>
static int launch_apply_h3k(const mfx_operator* op, const float* xs, const float* sq, const float* x, int64_t ldx,
                            float* y, int64_t ldy, int64_t p, float* vscale, void* pk, hipStream_t stream) {
  const int64_t n = op->n;
  const int64_t row0 = op_row0(op), nrow = op_nrows(op), rend = row0 + nrow;
  MFX_REQUIRE(row0 % 64 == 0, MFX_ERR_INVALID, "matrix-core Gram matvec: row0 = %lld must be a multiple of 64", (long long)row0);
  // the pre-packed tile images need the caller's pack workspace (mfx_workspace_bytes sizes it); DPAD = 32 (16 < d <= 32, round 5): only the
  // in-kernel-split form with fp32-MFMA distances is built -- the packed images and the fat-wave kernel keep 3 KD / 16 f16 distance operands
  // per block resident or in the 160 KB of LDS next to the chain masters, which stops at DPAD = 16
  constexpr bool kPackBuilt = DPAD <= 16 || NB == 1;
  const bool pack = pk != nullptr && kPackBuilt;
  const RbfVscaleLayout vl = rbf_vscale_layout(n, p);
  MFX_REQUIRE(vl.ok, MFX_ERR_UNSUPPORTED, "matrix-core Gram matvec: %lld vectors exceed the scale / slice-maximum region of the workspace (at most %lld)", (long long)p, (long long)kRbfVscaleMaxP);
  int* rangeflag = reinterpret_cast<int*>(vscale + vl.rangeflag);
  float* amax_part = vscale + vl.amax_part;
  if (pack) {
    k_row_amax_part<<<dim3((unsigned)vl.gx, (unsigned)p), 256, 0, stream>>>(x, ldx, n, amax_part, rangeflag);
    MFX_CHECK_LAUNCH();
  } else {
    MFX_TRY(row_scales(x, ldx, n, p, vscale, vl, stream));
  }
  const unsigned chunks = (unsigned)((p + NB * 32 - 1) / (NB * 32));  // (pack: NB * 32 = chunk_width, so this is pl.chunks)
  const bool vec4 = vec4_ok(x, ldx, y, ldy, n, nrow);
  const RbfPackLayout pl = rbf_pack_layout(n, nrow, p, DPAD);
  char* pkb = static_cast<char*>(pk);
  const int nsplit = pk ? pl.nsplit : 1;
  RbfMatvecArgs a{xs, sq, n, (const float*)op->outputscale, (const float*)op->noise, vscale, x, ldx, y, ldy, p, nullptr, nullptr,
                  pk ? reinterpret_cast<float*>(pkb + pl.off_part) : nullptr, nullptr, pl.ldpart, row0, rend};
  // split kernel: 4-wave workgroups (256 rows); packed and fat-wave kernels: 512 rows
  const dim3 grid((unsigned)((nrow + 255) / 256), chunks, (unsigned)nsplit);
  const dim3 grid_pk((unsigned)((nrow + 511) / 512), chunks, (unsigned)nsplit);
  if constexpr (kPackBuilt) {
    if (pack) {
      a.pkv = pkb;
      a.pka = pkb + pl.off_a;
      a.rangeflag = rangeflag;
      k_pack_tiles<DPAD, NB, KIND><<<dim3((unsigned)pl.ntile, chunks + 1), 256, 0, stream>>>(
          xs, sq, n, vscale, amax_part, (int)vl.gx, x, ldx, p, static_cast<uintx4*>(pk), reinterpret_cast<uintx4*>(pkb + pl.off_a), rangeflag);
      MFX_CHECK_LAUNCH();
      int fat = 0;  // fat waves (mfx_rbf_fat.hip): four waves of 128 rows, one per SIMD
      if constexpr (KIND == MFX_KERNEL_RBF && DPAD <= 16) fat = rbf_fat();
      if (fat) MFX_TRY(rbf_fat_launch(DPAD, NB, vec4, fat == 2, grid_pk, stream, a));
      else MFX_TRY((launch_h3_packed<DPAD, NB, KIND>(vec4, grid_pk, stream, a)));
      // (the split launch below follows in every case: the f16 range guard, stated above the h3 pair)
    }
  }
  // fp32-MFMA distances, in-kernel split of the probe tiles: all the work without the pack workspace
  MFX_TRY((launch_h3_split<DPAD, NB, KIND>(vec4, grid, stream, a)));
  MFX_CHECK_LAUNCH();
  if (nsplit > 1) {
    k_split_reduce<<<dim3((unsigned)((nrow + 255) / 256), (unsigned)p), 256, 0, stream>>>(a.part, a.ldpart, nsplit, p, nrow, ldy,
                                                                                        (const float*)op->noise, x, ldx, y, row0);
    MFX_CHECK_LAUNCH();
  }
  return MFX_OK;
}

int rbf_mfma_apply_h3(const mfx_operator* op, const float* xs, const float* sq, int dpad, const float* x, int64_t ldx,
                      float* y, int64_t ldy, int64_t p, float* vscale, void* pk, hipStream_t stream) {
  // chunks of 64 vectors from 33 on; DPAD = 32 with the pack workspace: chunk_width's one block; without it: in-kernel split, two
  const bool two_blocks = pk ? chunk_width(p, dpad) == 64 : p > 32;
  return with_mfma_dpad<32>(dpad, "split matrix-core Gram matvec supports d <= 32", [&](auto dc) -> int {
    return with_bool(two_blocks, [&](auto two) -> int {
      return with_kind(op->kernel_fn, [&](auto kind) -> int {
        return launch_apply_h3k<decltype(dc)::value, decltype(two)::value ? 2 : 1, decltype(kind)::value>(op, xs, sq, x, ldx, y, ldy, p,
                                                                                                         vscale, pk, stream);
      });
    });
  });
}

// Which matvec runs.  rbf_mode 0: exact fp32 MFMA, 1: 3 x f16 matvec (fat-wave / pipelined kernels), 2: also the gradient GEMM split.
//   d <= 16: from 4 probes on, padding the probe dimension to 32 already beats the VALU kernel (C2-like: 12 ms -> ~1 ms).  1-3 vectors
//     (the CG solves of the log-marginal likelihood) in the split modes at n >= 2048: the VALU kernel costs 2-2.7x a matrix-core sweep
//     over one 32-probe block (measured, n = 131072: 12.9 vs 5.9 ms), whose probe guards handle any p >= 1.
//   16 < d <= 128 (round 5): the split kernels keep their distance operands resident and stop at d = 16, the exact-fp32 kernels of this
//     file are generic in the padded dimension (the distance product is KD / 2 = 17 or 33 fp32 MFMAs per block) -- every arithmetic mode
//     runs them there.  About half of the datasets the reference's UCI loaders fetch have 17 .. 27 input columns
//     (util/uci_util.py:68-316); the VALU kernel they fell to is 18 x slower per matvec than d = 16 on the matrix cores (profiles/r05k_*).
//   16 < d <= 32 in the split modes: the h3 kernel's in-kernel-split form -- fp32-MFMA distances (17 per block), the CONTRACTION on the
//     f16 pipe.
//   Everything else (fp64, d > 128, 1-3 vectors below n = 2048 or in the exact mode at d <= 16): the VALU kernel.
RbfApplyPath rbf_apply_path(const mfx_operator* op, int64_t p) {
  if (op->dtype != MFX_F32 || op->d > 128) return RbfApplyPath::valu;
  const bool split = op->rbf_mode >= MFX_RBF_F16X3_MATVEC;
  const bool few_ok = p >= 4 || op->n >= 2048;
  if (op->d <= 16) {
    if (p >= 4) return split ? RbfApplyPath::h3 : RbfApplyPath::exact;
    return split && few_ok ? RbfApplyPath::h3 : RbfApplyPath::valu;
  }
  if (!few_ok) return RbfApplyPath::valu;
  return split && op->d <= 32 ? RbfApplyPath::h3 : RbfApplyPath::exact;
}

// the one launch site of k_rbf_mfma_apply; MI: 32-row blocks per wave
template <int DPAD, int NB, int MI>
static int launch_apply(const mfx_operator* op, const float* xs, const float* sq, const float* x, int64_t ldx,
                        float* y, int64_t ldy, int64_t p, hipStream_t stream) {
  const int64_t n = op->n;
  const int64_t row0 = op_row0(op), nrow = op_nrows(op), rend = row0 + nrow;
  MFX_REQUIRE(row0 % 64 == 0, MFX_ERR_INVALID, "matrix-core Gram matvec: row0 = %lld must be a multiple of 64", (long long)row0);
  const dim3 grid((unsigned)((nrow + 4 * MI * 32 - 1) / (4 * MI * 32)), (unsigned)((p + NB * 32 - 1) / (NB * 32)));
  return with_bool(vec4_ok(x, ldx, y, ldy, n, nrow), [&](auto v4) -> int {
    k_rbf_mfma_apply<DPAD, NB, decltype(v4)::value, MI, 64><<<grid, 256, 0, stream>>>(
        xs, sq, n, (const float*)op->outputscale, (const float*)op->noise, x, ldx, y, ldy, p, op->kernel_fn, row0, rend);
    MFX_CHECK_LAUNCH();
    return MFX_OK;
  });
}

int rbf_mfma_apply(const mfx_operator* op, const float* xs, const float* sq, int dpad, const float* x, int64_t ldx,
                   float* y, int64_t ldy, int64_t p, hipStream_t stream) {
  // 64 rows per wave (2 workgroups per CU at n = 131072) unless the problem is too small to fill the chip
  // (DPAD >= 64: the resident row operand of the distance product is 33 registers per 32 rows -- one row block per wave)
  const bool small = (op_nrows(op) + 255) / 256 < 512;
  return with_mfma_dpad<128>(dpad, "exact-fp32 matrix-core Gram matvec supports d <= 128", [&](auto dc) -> int {
    return with_bool(p > 32, [&](auto two) -> int {  // chunks of 64 probes in grid.y
      constexpr int DPAD = decltype(dc)::value, NB = decltype(two)::value ? 2 : 1;
      if constexpr (DPAD <= 32) {
        if (!small) return launch_apply<DPAD, NB, 2>(op, xs, sq, x, ldx, y, ldy, p, stream);
      }
      return launch_apply<DPAD, NB, 1>(op, xs, sq, x, ldx, y, ldy, p, stream);
    });
  });
}

}  // namespace mfx
