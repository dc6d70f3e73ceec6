// libmfx: the matrix-free generalised Gauss-Newton operator of an MLP (MFX_OP_GGN) -- the linearised-Laplace calibration of the
// reference (util/bnn_util.py:263-293 ggn_vp_parallel, :477-499 callibration_loss) with theta and the data fixed:
//
//   y = sum_i J_i^T H_i J_i v + alpha v        J_i = d f(theta; x_i) / d theta,  H_i = loss Hessian in the logits
//
// Everything that depends on theta and the data is a tape (layer inputs a_l, activation slopes dact_l, softmax p) that the caller
// computes once; include/mfx.h (struct mfx_ggn_net) has the formulas and the theta layout.  One application is two kernels:
//
//   k_ggn_tiles   a workgroup takes tiles of kGgnTS = 32 samples and a GROUP of probes (4 in fp32, 2 in fp64): one wave per probe,
//                 lane j = unit j of the layer at hand.  A chunk of a tape matrix (64 units x 32 samples) is staged ONCE in LDS,
//                 transposed, and read by every wave of the group -- the reads are wave-uniform, so they broadcast (the slopes
//                 dact_l and the softmax go through the same buffer: every tape matrix is fetched once per group).  A thread keeps
//                 its unit's 32 tangents (forward) / cotangents (backward) in registers; between layers they pass through LDS.
//                 The first layer (d_in up to 65536) streams x in chunks of 64 columns, once forward against V_W_1 and once
//                 backward into y_W_1; the other layers (<= 64 units) are one chunk each.  Per-workgroup sums over its samples
//                 go to the workspace: part[workgroup][probe][P], every entry written (first tile) before it is added to.
//   k_ggn_reduce  y = sum over workgroups, in index order, + alpha v.
//
// No atomics and a fixed summation order: bit-identical from run to run; the arithmetic of a probe does not involve its group,
// so its bits do not depend on how many probes share the call.  The shift gradient (mfx_op_grads.noise += sum_b L_b . R_b) is a
// two-stage dot product with fp64 partial sums in the workspace.
//
// The two halves of that pass are also entry points of their own, the network Jacobian at the samples of a tape as a pair of linear
// maps (mfx_mlp_jac_apply, mfx_mlp_jac_t_apply: what the linearised-Laplace predictive needs at the test points):
//
//   k_jac_tiles     out[b][i][:] = J_i v_b: the forward tangent of k_ggn_tiles, written per sample; no workspace, no sum
//   k_jac_t_tiles   the backward accumulation started at g_L = U[b][i][:], per-workgroup partial sums as above
//   k_jac_t_reduce  y = sum over workgroups, in index order: ggn_reduce without the shift, k_ggn_reduce is the same sum with it
//
// The exact diagonal sum_i diag(J_i^T H_i J_i) (mfx_ggn_diag: the diagonal-Laplace baseline) is a fourth pass over the same tape:
//
//   k_ggn_diag_tiles   the backward sweep once per class, squared where it is produced; the waves of a workgroup share the classes
//                      instead of holding probes; partial sums as above, added by k_jac_t_reduce
//
// Shared: ggn_stage, ggn_accumulate, ggn_reduce, the host code.  The sweeps stay spelled out per kernel: DESIGN.md section 3.11.
#include "mfx_internal.h"

namespace mfx {

constexpr int kGgnTS = 32;           // samples per tile
constexpr int kGgnW = 64;            // widest layer past the input = lanes of a wave; also the chunk of d_in staged at a time
constexpr int kGgnMaxIn = 65536;     // widest input
constexpr int kGgnMaxBlocks = 64;    // workgroups along the samples: bounds the partial sums (nblk x p x P values)
constexpr int kGgnDotBlocks = 256;   // workgroups of the shift-gradient dot product

template <typename T>
struct GgnGroup {  // probes per workgroup: LDS holds (1 + group) x 64 x 32 values (46 KiB in fp32, 52 KiB in fp64)
  static constexpr int value = sizeof(T) == 4 ? 4 : 2;
};

template <typename T>
struct GgnArgs {
  int L, loss;
  int64_t N, P, ntiles;
  int w[MFX_GGN_MAX_LAYERS + 1];
  int64_t off[MFX_GGN_MAX_LAYERS + 1];  // off[l], l = 1..L: bias of layer l in theta; its kernel follows at off[l] + w[l]
  const T* theta;
  const T* act[MFX_GGN_MAX_LAYERS];
  const T* dact[MFX_GGN_MAX_LAYERS];
  const T* prob;
};

template <typename T>
struct GgnLds {
  static constexpr int TSP = kGgnTS + 16 / (int)sizeof(T);  // row padded by 16 bytes: the column writes of a wave spread over banks
  T aT[kGgnW][TSP];                                         // chunk of a tape matrix, [unit][sample]
  T tb[GgnGroup<T>::value][kGgnW][TSP];                     // per probe: tangents t_l / cotangents g_l, [unit][sample]
};

// aT[kk][i] = M[i0 + i][k0 + kk] (its square where Square) for the nv samples of the tile and the units of the chunk, 0 elsewhere
// (M: (N, width) row-major)
template <bool Square, typename T>
__device__ __forceinline__ void ggn_stage(GgnLds<T>& sm, const T* __restrict__ M, int width, int k0, int64_t i0, int nv) {
  for (int e = threadIdx.x; e < kGgnW * kGgnTS; e += blockDim.x) {
    const int kk = e & (kGgnW - 1), i = e / kGgnW;
    const int k = k0 + kk;
    const T m = (i < nv && k < width) ? M[(i0 + i) * width + k] : T(0);
    sm.aT[kk][i] = Square ? m * m : m;
  }
}

// part[idx] = val on a workgroup's first tile, += afterwards: the workspace is never read before it is written
template <typename T>
__device__ __forceinline__ void ggn_accumulate(T* __restrict__ out, int64_t idx, T val, bool first) {
  out[idx] = first ? val : out[idx] + val;
}

template <typename T>
__global__ __launch_bounds__(64 * GgnGroup<T>::value) void k_ggn_tiles(GgnArgs<T> a, const T* __restrict__ x, int64_t ldx, int64_t p,
                                                                       T* __restrict__ part) {
  constexpr int G = GgnGroup<T>::value, TS = kGgnTS, W = kGgnW;
  __shared__ __attribute__((aligned(16))) GgnLds<T> sm;
  const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.y * G + g;
  const bool live = b < p;  // wave-uniform; a wave without a probe still stages and meets the barriers
  const T* __restrict__ v = x + (live ? b : 0) * ldx;
  T* __restrict__ out = part + ((int64_t)blockIdx.x * p + (live ? b : 0)) * a.P;
  const int L = a.L, c = a.w[L];
  T s[TS];  // this unit's tangents, then cotangents, for the samples of the tile

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const bool first = tile == (int64_t)blockIdx.x;
    const int64_t i0 = tile * TS;
    const int nv = a.N - i0 < TS ? (int)(a.N - i0) : TS;

    // ---- forward tangent: s_l = V_W_l^T a_{l-1} + v_b_l + W_l^T t_{l-1} ----
    for (int l = 1; l <= L; ++l) {
      const int wi = a.w[l - 1], wo = a.w[l];
      const bool on = live && j < wo;
      const T* __restrict__ vW = v + a.off[l] + wo;
      const T* __restrict__ Wl = a.theta + a.off[l] + wo;
      const T vb = on ? v[a.off[l] + j] : T(0);
#pragma unroll
      for (int i = 0; i < TS; ++i) s[i] = vb;
      for (int k0 = 0; k0 < wi; k0 += W) {
        __syncthreads();  // the chunk before this one has been consumed
        ggn_stage<false>(sm, a.act[l - 1], wi, k0, i0, nv);
        __syncthreads();
        if (on) {
          const int kc = wi - k0 < W ? wi - k0 : W;
          if (l == 1) {
#pragma unroll 2
            for (int kk = 0; kk < kc; ++kk) {
              const T vw = vW[(int64_t)(k0 + kk) * wo + j];
#pragma unroll
              for (int i = 0; i < TS; ++i) s[i] += sm.aT[kk][i] * vw;
            }
          } else {  // wi <= 64: one chunk, kk is the unit of layer l - 1
#pragma unroll 2
            for (int kk = 0; kk < kc; ++kk) {
              const T vw = vW[kk * wo + j], wt = Wl[kk * wo + j];
#pragma unroll
              for (int i = 0; i < TS; ++i) s[i] += sm.aT[kk][i] * vw + sm.tb[g][kk][i] * wt;
            }
          }
        }
      }
      __syncthreads();  // every wave is done with t_{l-1} and with the last chunk
      if (l < L) {      // the slopes of the tile, staged once for the whole group (0 past the end of the tape)
        ggn_stage<false>(sm, a.dact[l], wo, 0, i0, nv);
        __syncthreads();
      }
      if (on) {
        if (l < L) {
#pragma unroll
          for (int i = 0; i < TS; ++i) sm.tb[g][j][i] = sm.aT[j][i] * s[i];
        } else {
#pragma unroll
          for (int i = 0; i < TS; ++i) sm.tb[g][j][i] = s[i];
        }
      }
    }

    // ---- H product: u = p o t_L - p (p . t_L), or u = t_L; samples past the end of the tape contribute nothing ----
    if (a.loss == MFX_GGN_CROSS_ENTROPY) ggn_stage<false>(sm, a.prob, c, 0, i0, nv);  // aT is free: the barrier above
    __syncthreads();
    if (live && j < c) {
      if (a.loss == MFX_GGN_CROSS_ENTROPY) {
#pragma unroll
        for (int i = 0; i < TS; ++i) s[i] = T(0);
        for (int m = 0; m < c; ++m) {
#pragma unroll
          for (int i = 0; i < TS; ++i) s[i] += sm.aT[m][i] * sm.tb[g][m][i];
        }
#pragma unroll
        for (int i = 0; i < TS; ++i) {
          const T pj = sm.aT[j][i];
          s[i] = pj * sm.tb[g][j][i] - pj * s[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < TS; ++i) s[i] = i < nv ? sm.tb[g][j][i] : T(0);
      }
    }

    // ---- backward: y_b_l += g_l, y_W_l += a_{l-1} g_l^T, g_{l-1} = dact_{l-1} o (W_l g_l) ----
    for (int l = L; l >= 1; --l) {
      const int wi = a.w[l - 1], wo = a.w[l];
      const bool on = live && j < wo;
      if (on) {
        T sb = T(0);
#pragma unroll
        for (int i = 0; i < TS; ++i) sb += s[i];
        ggn_accumulate<T>(out, a.off[l] + j, sb, first);
      }
      for (int k0 = 0; k0 < wi; k0 += W) {
        __syncthreads();
        ggn_stage<false>(sm, a.act[l - 1], wi, k0, i0, nv);
        __syncthreads();
        if (on) {
          const int kc = wi - k0 < W ? wi - k0 : W;
          const int64_t base = a.off[l] + wo + (int64_t)k0 * wo + j;
#pragma unroll 2
          for (int kk = 0; kk < kc; ++kk) {
            T acc = T(0);
#pragma unroll
            for (int i = 0; i < TS; ++i) acc += sm.aT[kk][i] * s[i];
            ggn_accumulate<T>(out, base + (int64_t)kk * wo, acc, first);
          }
        }
      }
      if (l > 1) {
        __syncthreads();  // tb is free (t_L, or the cotangents of the layer above, have been read)
        if (on) {
#pragma unroll
          for (int i = 0; i < TS; ++i) sm.tb[g][j][i] = s[i];
        }
        ggn_stage<false>(sm, a.dact[l - 1], wi, 0, i0, nv);  // aT is free as well: the slopes of layer l - 1, staged once for the group
        __syncthreads();
        if (live && j < wi) {
          const T* __restrict__ Wrow = a.theta + a.off[l] + wo + (int64_t)j * wo;
#pragma unroll
          for (int i = 0; i < TS; ++i) s[i] = T(0);
          for (int m = 0; m < wo; ++m) {
            const T wt = Wrow[m];
#pragma unroll
            for (int i = 0; i < TS; ++i) s[i] += sm.tb[g][m][i] * wt;
          }
#pragma unroll
          for (int i = 0; i < TS; ++i) s[i] = sm.aT[j][i] * s[i];
        }
      }
    }
    __syncthreads();  // the next tile stages into aT and writes tb
  }
}

// out[b][i][:] = J_i v_b for every probe b and sample i < N (out: (p, N, c) contiguous): the forward tangent of k_ggn_tiles with the
// same geometry -- a tile of 32 samples and a group of probes per workgroup, every tape chunk staged once per group -- ending in a
// store of t_L instead of the H product.  Samples past N in the last tile write nothing.
template <typename T>
__global__ __launch_bounds__(64 * GgnGroup<T>::value) void k_jac_tiles(GgnArgs<T> a, const T* __restrict__ x, int64_t ldx, int64_t p,
                                                                       T* __restrict__ out) {
  constexpr int G = GgnGroup<T>::value, TS = kGgnTS, W = kGgnW;
  __shared__ __attribute__((aligned(16))) GgnLds<T> sm;
  const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.y * G + g;
  const bool live = b < p;  // wave-uniform; a wave without a probe still stages and meets the barriers
  const T* __restrict__ v = x + (live ? b : 0) * ldx;
  const int L = a.L, c = a.w[L];
  T s[TS];  // this unit's tangents for the samples of the tile

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t i0 = tile * TS;
    const int nv = a.N - i0 < TS ? (int)(a.N - i0) : TS;
    for (int l = 1; l <= L; ++l) {
      const int wi = a.w[l - 1], wo = a.w[l];
      const bool on = live && j < wo;
      const T* __restrict__ vW = v + a.off[l] + wo;
      const T* __restrict__ Wl = a.theta + a.off[l] + wo;
      const T vb = on ? v[a.off[l] + j] : T(0);
#pragma unroll
      for (int i = 0; i < TS; ++i) s[i] = vb;
      for (int k0 = 0; k0 < wi; k0 += W) {
        __syncthreads();  // the chunk before this one has been consumed
        ggn_stage<false>(sm, a.act[l - 1], wi, k0, i0, nv);
        __syncthreads();
        if (on) {
          const int kc = wi - k0 < W ? wi - k0 : W;
          if (l == 1) {
#pragma unroll 2
            for (int kk = 0; kk < kc; ++kk) {
              const T vw = vW[(int64_t)(k0 + kk) * wo + j];
#pragma unroll
              for (int i = 0; i < TS; ++i) s[i] += sm.aT[kk][i] * vw;
            }
          } else {  // wi <= 64: one chunk, kk is the unit of layer l - 1
#pragma unroll 2
            for (int kk = 0; kk < kc; ++kk) {
              const T vw = vW[kk * wo + j], wt = Wl[kk * wo + j];
#pragma unroll
              for (int i = 0; i < TS; ++i) s[i] += sm.aT[kk][i] * vw + sm.tb[g][kk][i] * wt;
            }
          }
        }
      }
      __syncthreads();  // every wave is done with t_{l-1} and with the last chunk
      if (l < L) {      // the slopes of the tile, staged once for the whole group
        ggn_stage<false>(sm, a.dact[l], wo, 0, i0, nv);
        __syncthreads();
        if (on) {
#pragma unroll
          for (int i = 0; i < TS; ++i) sm.tb[g][j][i] = sm.aT[j][i] * s[i];
        }
      } else if (on) {  // j < c: lane j writes logit j, consecutive lanes consecutive addresses
        T* __restrict__ o = out + ((int64_t)b * a.N + i0) * c + j;
#pragma unroll
        for (int i = 0; i < TS; ++i) {
          if (i < nv) o[(int64_t)i * c] = s[i];
        }
      }
    }
    __syncthreads();  // the next tile stages into aT and writes tb
  }
}

// part[workgroup][b][:] = sum over the workgroup's samples of J_i^T u_bi, u (p, N, c) contiguous: the backward accumulation of
// k_ggn_tiles started at g_L = u_bi (0 past the end of the tape), the same geometry and the same partial sums.
template <typename T>
__global__ __launch_bounds__(64 * GgnGroup<T>::value) void k_jac_t_tiles(GgnArgs<T> a, const T* __restrict__ u, int64_t p,
                                                                         T* __restrict__ part) {
  constexpr int G = GgnGroup<T>::value, TS = kGgnTS, W = kGgnW;
  __shared__ __attribute__((aligned(16))) GgnLds<T> sm;
  const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.y * G + g;
  const bool live = b < p;  // wave-uniform; a wave without a probe still stages and meets the barriers
  T* __restrict__ out = part + ((int64_t)blockIdx.x * p + (live ? b : 0)) * a.P;
  const int L = a.L, c = a.w[L];
  T s[TS];  // this unit's cotangents for the samples of the tile

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const bool first = tile == (int64_t)blockIdx.x;
    const int64_t i0 = tile * TS;
    const int nv = a.N - i0 < TS ? (int)(a.N - i0) : TS;
    {
      const bool on = live && j < c;
      const T* __restrict__ ub = u + ((int64_t)(live ? b : 0) * a.N + i0) * c + j;
#pragma unroll
      for (int i = 0; i < TS; ++i) s[i] = (on && i < nv) ? ub[(int64_t)i * c] : T(0);
    }
    for (int l = L; l >= 1; --l) {
      const int wi = a.w[l - 1], wo = a.w[l];
      const bool on = live && j < wo;
      if (on) {
        T sb = T(0);
#pragma unroll
        for (int i = 0; i < TS; ++i) sb += s[i];
        ggn_accumulate<T>(out, a.off[l] + j, sb, first);
      }
      for (int k0 = 0; k0 < wi; k0 += W) {
        __syncthreads();
        ggn_stage<false>(sm, a.act[l - 1], wi, k0, i0, nv);
        __syncthreads();
        if (on) {
          const int kc = wi - k0 < W ? wi - k0 : W;
          const int64_t base = a.off[l] + wo + (int64_t)k0 * wo + j;
#pragma unroll 2
          for (int kk = 0; kk < kc; ++kk) {
            T acc = T(0);
#pragma unroll
            for (int i = 0; i < TS; ++i) acc += sm.aT[kk][i] * s[i];
            ggn_accumulate<T>(out, base + (int64_t)kk * wo, acc, first);
          }
        }
      }
      if (l > 1) {
        __syncthreads();  // tb is free (the cotangents of the layer above have been read)
        if (on) {
#pragma unroll
          for (int i = 0; i < TS; ++i) sm.tb[g][j][i] = s[i];
        }
        ggn_stage<false>(sm, a.dact[l - 1], wi, 0, i0, nv);  // aT is free as well: the slopes of layer l - 1, staged once for the group
        __syncthreads();
        if (live && j < wi) {
          const T* __restrict__ Wrow = a.theta + a.off[l] + wo + (int64_t)j * wo;
#pragma unroll
          for (int i = 0; i < TS; ++i) s[i] = T(0);
          for (int m = 0; m < wo; ++m) {
            const T wt = Wrow[m];
#pragma unroll
            for (int i = 0; i < TS; ++i) s[i] += sm.tb[g][m][i] * wt;
          }
#pragma unroll
          for (int i = 0; i < TS; ++i) s[i] = sm.aT[j][i] * s[i];
        }
      }
    }
    __syncthreads();  // the next tile stages into aT and writes tb
  }
}

// y_b[i] = sum_blk part[blk][b][i], the workgroups in index order, + alpha x_b[i] where Shift: k_ggn_reduce with, k_jac_t_reduce without
template <bool Shift, typename T>
__device__ __forceinline__ void ggn_reduce(const T* __restrict__ part, int64_t nblk, int64_t P, const T* __restrict__ alpha,
                                           const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, p = gridDim.y;
  if (i >= P) return;
  T acc = T(0);
  for (int64_t blk = 0; blk < nblk; ++blk) acc += part[(blk * p + b) * P + i];
  y[b * ldy + i] = Shift ? acc + alpha[0] * x[b * ldx + i] : acc;
}

template <typename T>
__global__ __launch_bounds__(256) void k_ggn_reduce(const T* __restrict__ part, int64_t nblk, int64_t P, const T* __restrict__ alpha,
                                                    const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy) {
  ggn_reduce<true, T>(part, nblk, P, alpha, x, ldx, y, ldy);
}
template <typename T>
__global__ __launch_bounds__(256) void k_jac_t_reduce(const T* __restrict__ part, int64_t nblk, int64_t P, T* __restrict__ y,
                                                      int64_t ldy) {
  ggn_reduce<false, T>(part, nblk, P, nullptr, nullptr, 0, y, ldy);
}

// ---- the exact diagonal sum_i diag(J_i^T H_i J_i) (mfx_ggn_diag); include/mfx.h has the formulas ----

// D = max(m1 - m2^2, 0), the product rounded on its own: contracted to fma(-m2, m2, m1) it is not 0 where m1 = round(m2 * m2) (c = 1),
// and hipcc contracts across statements (and through __fmul_rn) unless the expression says otherwise
template <typename T>
__device__ __forceinline__ T ggn_variance(T m1, T m2) {
#pragma clang fp contract(off)
  const T d = m1 - m2 * m2;
  return d > T(0) ? d : T(0);  // a variance under p: round-off below 0 is cut off
}

// One layer down, for the cotangents s of wave g (lane j = unit j of layer l on entry, of layer l - 1 on return):
// s <- dact_{l-1} o (W_l s).  The cotangents pass through the wave's own tb, the slopes of layer l - 1 are staged once for the
// workgroup (0 past the end of the tape).  Every wave of the workgroup calls it, with the same l: it holds two barriers.
template <typename T>
__device__ __forceinline__ void ggn_down(GgnLds<T>& sm, const GgnArgs<T>& a, int l, int g, int j, int64_t i0, int nv, T (&s)[kGgnTS]) {
  constexpr int TS = kGgnTS;
  const int wi = a.w[l - 1], wo = a.w[l];
  __syncthreads();  // tb and aT are free
  if (j < wo) {
#pragma unroll
    for (int i = 0; i < TS; ++i) sm.tb[g][j][i] = s[i];
  }
  ggn_stage<false>(sm, a.dact[l - 1], wi, 0, i0, nv);
  __syncthreads();
  if (j < wi) {
    const T* __restrict__ Wrow = a.theta + a.off[l] + wo + (int64_t)j * wo;
#pragma unroll
    for (int i = 0; i < TS; ++i) s[i] = T(0);
    for (int m = 0; m < wo; ++m) {
      const T wt = Wrow[m];
#pragma unroll
      for (int i = 0; i < TS; ++i) s[i] += sm.tb[g][m][i] * wt;
    }
#pragma unroll
    for (int i = 0; i < TS; ++i) s[i] = sm.aT[j][i] * s[i];
  }
}

// v[i] <- sum over the waves h = 0, 1, ... of the workgroup of lane j's v[i], in that order: every wave ends with the same bits
template <typename T>
__device__ __forceinline__ void ggn_sum_waves(GgnLds<T>& sm, int g, int j, T (&v)[kGgnTS]) {
  constexpr int G = GgnGroup<T>::value, TS = kGgnTS;
  __syncthreads();  // tb is free
#pragma unroll
  for (int i = 0; i < TS; ++i) sm.tb[g][j][i] = v[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < TS; ++i) {
    T acc = sm.tb[0][j][i];
#pragma unroll
    for (int h = 1; h < G; ++h) acc += sm.tb[h][j][i];
    v[i] = acc;
  }
}

// part[workgroup][:] = sum over the workgroup's samples of diag(J_i^T H_i J_i).  The geometry of k_ggn_tiles: tiles of 32 samples,
// lane j = unit j of the layer at hand, the waves of the workgroup (4 in fp32, 2 in fp64) in the place of its probes.  Row o of J_i
// is the backward sweep started at g_L = e_o; the classes are dealt to the waves round robin (wave g takes o = g, g + G, ...).
// Layer-outer: for the layer l whose entries are being produced every class is swept from L down to l again, so that only the two
// moments of that layer live in registers (m1 = sum_o p_o g^2, m2 = sum_o p_o g, 2 x 32 values) -- L (L - 1) / 2 layer steps per
// class instead of L - 1, at widths <= 64.  Then the moments are added over the waves in wave order, D = max(m1 - m2^2, 0) (m1 for
// MSE), and y_b_l += D, y_W_l += a_{l-1}^2 D^T with the squared inputs staged chunk by chunk; the rows of a chunk are dealt to the
// waves, which all hold the same D.
template <typename T>
__global__ __launch_bounds__(64 * GgnGroup<T>::value) void k_ggn_diag_tiles(GgnArgs<T> a, T* __restrict__ part) {
  constexpr int G = GgnGroup<T>::value, TS = kGgnTS, W = kGgnW;
  __shared__ __attribute__((aligned(16))) GgnLds<T> sm;
  __shared__ T po[G][TS];  // per wave: p_o of the class it is sweeping, for the samples of the tile
  const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
  T* __restrict__ out = part + (int64_t)blockIdx.x * a.P;
  const int L = a.L, c = a.w[L];
  const bool ce = a.loss == MFX_GGN_CROSS_ENTROPY;
  T s[TS];   // this unit's cotangents of the class at hand
  T m1[TS];  // sum_o p_o g^2 over this wave's classes, then over all; then D
  T m2[TS];  // sum_o p_o g (cross-entropy)

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const bool first = tile == (int64_t)blockIdx.x;
    const int64_t i0 = tile * TS;
    const int nv = a.N - i0 < TS ? (int)(a.N - i0) : TS;
    for (int l = L; l >= 1; --l) {
      const int wi = a.w[l - 1], wo = a.w[l];
#pragma unroll
      for (int i = 0; i < TS; ++i) m1[i] = m2[i] = T(0);
      for (int o0 = 0; o0 < c; o0 += G) {  // every wave makes every round, with or without a class: ggn_down holds barriers
        const int o = o0 + g;
        const bool has = o < c;  // wave-uniform
        if (j < TS) {  // p_o of the tile's samples (1 for MSE); 0 past the end of the tape: such samples contribute nothing
          const bool in = has && j < nv;
          po[g][j] = in ? (ce ? a.prob[(i0 + j) * c + o] : T(1)) : T(0);
        }
        const T e = (has && j == o) ? T(1) : T(0);
#pragma unroll
        for (int i = 0; i < TS; ++i) s[i] = e;
        for (int lp = L; lp > l; --lp) ggn_down<T>(sm, a, lp, g, j, i0, nv, s);
        __syncthreads();  // po of this round is written (a wave reads its own row, after its own reads of the round before)
        if (has && j < wo) {
#pragma unroll
          for (int i = 0; i < TS; ++i) {
            const T ps = po[g][i] * s[i];
            m2[i] += ps;
            m1[i] += ps * s[i];
          }
        }
      }
      ggn_sum_waves<T>(sm, g, j, m1);
      if (ce) {
        ggn_sum_waves<T>(sm, g, j, m2);
#pragma unroll
        for (int i = 0; i < TS; ++i) m1[i] = ggn_variance(m1[i], m2[i]);
      }
      if (g == 0 && j < wo) {
        T sb = T(0);
#pragma unroll
        for (int i = 0; i < TS; ++i) sb += m1[i];
        ggn_accumulate<T>(out, a.off[l] + j, sb, first);
      }
      for (int k0 = 0; k0 < wi; k0 += W) {
        __syncthreads();  // the chunk before this one (or the sums over the waves) has been consumed
        ggn_stage<true>(sm, a.act[l - 1], wi, k0, i0, nv);
        __syncthreads();
        if (j < wo) {
          const int kc = wi - k0 < W ? wi - k0 : W;
          const int64_t base = a.off[l] + wo + (int64_t)k0 * wo + j;
          for (int kk = g; kk < kc; kk += G) {
            T acc = T(0);
#pragma unroll
            for (int i = 0; i < TS; ++i) acc += sm.aT[kk][i] * m1[i];
            ggn_accumulate<T>(out, base + (int64_t)kk * wo, acc, first);
          }
        }
      }
    }
    __syncthreads();  // the next tile stages into aT and writes tb
  }
}

// partial[blockIdx.x] = this workgroup's share of sum_b L_b . R_b (fp64 sums, fixed order)
template <typename T>
__global__ __launch_bounds__(256) void k_ggn_dot(const T* __restrict__ L, int64_t ldl, const T* __restrict__ R, int64_t ldr, int64_t batch,
                                                 int64_t n, double* __restrict__ partial) {
  __shared__ double wsum[4];
  double acc = 0.0;
  for (int64_t b = 0; b < batch; ++b) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
      acc += (double)L[b * ldl + i] * (double)R[b * ldr + i];
    }
  }
  acc = wave_sum_all<double>(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

template <typename T>
__global__ __launch_bounds__(64) void k_ggn_dot_final(const double* __restrict__ partial, int nblk, T* __restrict__ g) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) acc += partial[i];
  acc = wave_sum_all<double>(acc);
  if (threadIdx.x == 0) g[0] += (T)acc;
}

static int64_t ggn_params(const mfx_ggn_net* net) {
  int64_t P = 0;
  for (int l = 1; l <= net->nlayers; ++l) P += ((int64_t)net->width[l - 1] + 1) * net->width[l];
  return P;
}

static int64_t ggn_blocks(int64_t N) {
  const int64_t tiles = (N + kGgnTS - 1) / kGgnTS;
  return tiles < kGgnMaxBlocks ? tiles : kGgnMaxBlocks;
}

static int64_t ggn_dot_blocks(int64_t n) {
  const int64_t blocks = (n + 255) / 256;
  return blocks < kGgnDotBlocks ? blocks : kGgnDotBlocks;
}

static int64_t ggn_part_bytes(const mfx_ggn_net* net, int dtype, int64_t p) {  // bytes of the partial sums part[workgroup][p][P]
  return ggn_blocks(net->nsamples) * p * ggn_params(net) * (int64_t)dtype_size(dtype);
}

// the checks of a net that the operator and the Jacobian maps share; `who` opens the message
static int ggn_check_net(const mfx_ggn_net* net, const char* who) {
  MFX_REQUIRE(net->nlayers >= 1 && net->nlayers <= MFX_GGN_MAX_LAYERS, MFX_ERR_INVALID, "%s: nlayers = %d is outside 1..%d", who,
              net->nlayers, MFX_GGN_MAX_LAYERS);
  MFX_REQUIRE(net->nsamples >= 1, MFX_ERR_INVALID, "%s: nsamples = %lld must be at least 1", who, (long long)net->nsamples);
  const int L = net->nlayers;
  for (int l = 0; l <= L; ++l) {
    MFX_REQUIRE(net->width[l] >= 1, MFX_ERR_INVALID, "%s: width[%d] = %d must be at least 1", who, l, net->width[l]);
  }
  MFX_REQUIRE(net->theta, MFX_ERR_INVALID, "%s: theta is NULL", who);
  for (int l = 0; l < L; ++l) {
    MFX_REQUIRE(net->act[l], MFX_ERR_INVALID, "%s: act[%d] is NULL", who, l);
    MFX_REQUIRE(l == 0 || net->dact[l], MFX_ERR_INVALID, "%s: dact[%d] is NULL", who, l);
  }
  return MFX_OK;
}

static int ggn_check_limits(const mfx_ggn_net* net, const char* who) {
  MFX_REQUIRE(net->width[0] <= kGgnMaxIn, MFX_ERR_UNSUPPORTED, "%s: width[0] = %d exceeds the input limit %d", who, net->width[0],
              kGgnMaxIn);
  for (int l = 1; l <= net->nlayers; ++l) {
    MFX_REQUIRE(net->width[l] <= kGgnW, MFX_ERR_UNSUPPORTED, "%s: width[%d] = %d exceeds the layer limit %d", who, l, net->width[l],
                kGgnW);
  }
  return MFX_OK;
}

// the loss of the operator and of the diagonal (the maps read neither loss nor prob), in two steps: the operator checks its shift between
static int ggn_check_loss(const mfx_ggn_net* net, const char* who) {
  MFX_REQUIRE(net->loss == MFX_GGN_CROSS_ENTROPY || net->loss == MFX_GGN_MSE, MFX_ERR_INVALID, "%s: unknown loss %d", who, net->loss);
  return MFX_OK;
}
static int ggn_check_prob(const mfx_ggn_net* net, const char* who) {
  MFX_REQUIRE(net->loss != MFX_GGN_CROSS_ENTROPY || net->prob, MFX_ERR_INVALID, "%s: prob is NULL (cross-entropy)", who);
  return MFX_OK;
}

static int ggn_check(const mfx_operator* op) {
  static const char* who = "GGN operator";
  const mfx_ggn_net* net = (const mfx_ggn_net*)op->ctx;
  MFX_REQUIRE(net, MFX_ERR_INVALID, "GGN operator: ctx (the mfx_ggn_net) is NULL");
  MFX_TRY(ggn_check_net(net, who));
  MFX_TRY(ggn_check_loss(net, who));
  MFX_REQUIRE(op->noise, MFX_ERR_INVALID, "GGN operator: noise (the shift alpha) is NULL");
  MFX_TRY(ggn_check_prob(net, who));
  const int64_t P = ggn_params(net);
  MFX_REQUIRE(op->n == P, MFX_ERR_INVALID, "GGN operator: n = %lld, but the widths give P = %lld parameters", (long long)op->n,
              (long long)P);
  MFX_TRY(ggn_check_limits(net, who));
  MFX_REQUIRE(op->nrows == 0, MFX_ERR_UNSUPPORTED, "GGN operator: no row block (nrows > 0): every output row sums over all samples");
  return MFX_OK;
}

static int ggn_check_grads(const mfx_operator*, const mfx_op_grads* grads, bool) {
  MFX_REQUIRE(!grads->x && !grads->dense_a && !grads->val, MFX_ERR_UNSUPPORTED,
              "GGN operator: only the shift gradient (grads->noise) exists; x, dense_a and val must be NULL (gradients with respect "
              "to theta or the inputs need third derivatives)");
  return MFX_OK;
}

static int64_t ggn_workspace_bytes(const mfx_operator* op, int64_t, int64_t p_apply) {
  const mfx_ggn_net* net = (const mfx_ggn_net*)op->ctx;
  if (!net || net->nlayers < 1 || net->nlayers > MFX_GGN_MAX_LAYERS || net->nsamples < 1) return 256;  // refused before any use
  const int64_t apply = ggn_part_bytes(net, op->dtype, p_apply > 0 ? p_apply : 1);
  const int64_t dot = kGgnDotBlocks * (int64_t)sizeof(double);
  return align_up(apply > dot ? apply : dot, 256);
}

// the kernel arguments of a checked net
template <typename T>
static GgnArgs<T> ggn_args(const mfx_ggn_net* net) {
  GgnArgs<T> a{};
  a.L = net->nlayers;
  a.loss = net->loss;
  a.N = net->nsamples;
  a.ntiles = (a.N + kGgnTS - 1) / kGgnTS;
  int64_t off = 0;
  for (int l = 0; l <= a.L; ++l) {
    a.w[l] = net->width[l];
    if (l >= 1) {
      a.off[l] = off;
      off += ((int64_t)a.w[l - 1] + 1) * a.w[l];
    }
    if (l < a.L) {
      a.act[l] = (const T*)net->act[l];
      a.dact[l] = (const T*)net->dact[l];
    }
  }
  a.P = off;
  a.theta = (const T*)net->theta;
  a.prob = (const T*)net->prob;
  return a;
}

// the launch of a tile kernel: nblk workgroups along the samples, one per group of G vectors across, a wave per vector
template <typename T, typename Tiles>
static int ggn_launch(int64_t nblk, int64_t p, Tiles tiles) {
  constexpr int G = GgnGroup<T>::value;
  tiles(dim3((unsigned)nblk, (unsigned)((p + G - 1) / G)), 64 * G);
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

// tile kernel, then reduce: part[workgroup][p][P] from at most 64 workgroups along the samples, y_b = their sum, + alpha x_b where Shift
template <typename T, bool Shift = false, typename Tiles>
static int ggn_pass(const GgnArgs<T>& a, int64_t p, Tiles tiles, const T* part, T* y, int64_t ldy, hipStream_t stream,
                    const T* alpha = nullptr, const T* x = nullptr, int64_t ldx = 0) {
  const int64_t nblk = ggn_blocks(a.N);
  MFX_TRY(ggn_launch<T>(nblk, p, tiles));
  const dim3 grid((unsigned)((a.P + 255) / 256), (unsigned)p);
  if constexpr (Shift) k_ggn_reduce<T><<<grid, 256, 0, stream>>>(part, nblk, a.P, alpha, x, ldx, y, ldy);
  else k_jac_t_reduce<T><<<grid, 256, 0, stream>>>(part, nblk, a.P, y, ldy);
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

template <typename T>
static int ggn_apply(const mfx_operator* op, int, const void* xv, int64_t ldx, const void*, int64_t, void* y, int64_t ldy, int64_t p,
                     void* ws, int64_t ws_bytes, hipStream_t stream) {  // symmetric: the mode is ignored
  const T* x = (const T*)xv;
  const mfx_ggn_net* net = (const mfx_ggn_net*)op->ctx;
  const GgnArgs<T> a = ggn_args<T>(net);
  const int64_t need = ggn_part_bytes(net, op->dtype, p);
  MFX_REQUIRE(ws && need <= ws_bytes, MFX_ERR_WORKSPACE, "GGN operator: workspace too small: need %lld bytes", (long long)need);
  const auto tiles = [&](dim3 grid, int block) { k_ggn_tiles<T><<<grid, block, 0, stream>>>(a, x, ldx, p, (T*)ws); };
  return ggn_pass<T, true>(a, p, tiles, (const T*)ws, (T*)y, ldy, stream, (const T*)op->noise, x, ldx);
}

// adds sum_b L_b . R_b to grads->noise (NULL: no launch)
template <typename T>
static int ggn_grad(const mfx_operator* op, const void* L, int64_t ldl, const void* R, int64_t ldr, int64_t batch, int64_t,
                    const mfx_op_grads* grads, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (!grads->noise) return MFX_OK;
  const int nblk = (int)ggn_dot_blocks(op->n);
  MFX_REQUIRE(ws && nblk * (int64_t)sizeof(double) <= ws_bytes, MFX_ERR_WORKSPACE, "GGN operator: workspace too small: need %lld bytes",
              (long long)(nblk * sizeof(double)));
  k_ggn_dot<T><<<nblk, 256, 0, stream>>>((const T*)L, ldl, (const T*)R, ldr, batch, op->n, (double*)ws);
  MFX_CHECK_LAUNCH();
  k_ggn_dot_final<T><<<1, 64, 0, stream>>>((const double*)ws, nblk, (T*)grads->noise);
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

// the launches of a captured driver call hold what ctx points at, not ctx
static void ggn_graph_key(const mfx_operator* op, GraphKey& key) { key.add(*(const mfx_ggn_net*)op->ctx); }

static const OpKind kGgnKind = {ggn_check, ggn_check_grads, ggn_workspace_bytes, {ggn_apply<float>, ggn_apply<double>},
                                {ggn_grad<float>, ggn_grad<double>},
                                "row sharding a GGN operator is not implemented: every output row sums over all samples", true,
                                ggn_graph_key};
const OpKind* ggn_kind() { return &kGgnKind; }  // for the table of kinds in mfx_ops.hip

// ---- the Jacobian maps of the net (mfx_mlp_jac_*): rectangular, so not an operator kind ----
static const char* const kJacWho = "MLP Jacobian";
constexpr int kJacMaxBlocks = 1024;  // workgroups along the samples of J V (no partial sums: bounded only to keep the tile loop short)

static int jac_check(const mfx_ggn_net* net, int dtype, int64_t p) {
  MFX_REQUIRE(net, MFX_ERR_INVALID, "MLP Jacobian: net is NULL");
  MFX_TRY(ggn_check_net(net, kJacWho));
  MFX_TRY(ggn_check_limits(net, kJacWho));
  MFX_REQUIRE(dtype == MFX_F32 || dtype == MFX_F64, MFX_ERR_UNSUPPORTED, "MLP Jacobian: unsupported dtype %d", dtype);
  MFX_REQUIRE(p >= 1, MFX_ERR_INVALID, "MLP Jacobian: p = %lld must be at least 1", (long long)p);
  MFX_REQUIRE(p <= 65535, MFX_ERR_UNSUPPORTED, "MLP Jacobian: p too large (at most 65535 vectors per call)");
  return MFX_OK;
}

template <typename T>
static int jac_apply_t(const mfx_ggn_net* net, const T* V, int64_t ldv, int64_t p, T* out, hipStream_t stream) {
  const GgnArgs<T> a = ggn_args<T>(net);
  const int64_t nblk = a.ntiles < kJacMaxBlocks ? a.ntiles : kJacMaxBlocks;
  return ggn_launch<T>(nblk, p, [&](dim3 grid, int block) { k_jac_tiles<T><<<grid, block, 0, stream>>>(a, V, ldv, p, out); });
}

template <typename T>
static int jac_t_apply_t(const mfx_ggn_net* net, const T* U, int64_t p, T* Y, int64_t ldy, T* ws, hipStream_t stream) {
  const GgnArgs<T> a = ggn_args<T>(net);
  return ggn_pass<T>(a, p, [&](dim3 grid, int block) { k_jac_t_tiles<T><<<grid, block, 0, stream>>>(a, U, p, ws); }, ws, Y, ldy, stream);
}

// ---- the exact diagonal of the GGN (mfx_ggn_diag): one value per parameter, so not an operator application ----
static const char* const kDiagWho = "GGN diagonal";

static int diag_check(const mfx_ggn_net* net, int dtype) {
  MFX_REQUIRE(net, MFX_ERR_INVALID, "GGN diagonal: net is NULL");
  MFX_TRY(ggn_check_net(net, kDiagWho));
  MFX_TRY(ggn_check_loss(net, kDiagWho));
  MFX_TRY(ggn_check_prob(net, kDiagWho));
  MFX_TRY(ggn_check_limits(net, kDiagWho));
  MFX_REQUIRE(dtype == MFX_F32 || dtype == MFX_F64, MFX_ERR_UNSUPPORTED, "GGN diagonal: unsupported dtype %d", dtype);
  return MFX_OK;
}

template <typename T>
static int diag_t(const mfx_ggn_net* net, T* diag, T* ws, hipStream_t stream) {  // part[workgroup][P]: one "vector"
  const GgnArgs<T> a = ggn_args<T>(net);
  return ggn_pass<T>(a, 1, [&](dim3 grid, int block) { k_ggn_diag_tiles<T><<<grid, block, 0, stream>>>(a, ws); }, ws, diag, a.P, stream);
}

}  // namespace mfx

using namespace mfx;

extern "C" {

int64_t mfx_ggn_diag_workspace_bytes(const mfx_ggn_net* net, int dtype) {
  if (diag_check(net, dtype) != MFX_OK) return -1;
  return align_up(ggn_part_bytes(net, dtype, 1), 256);
}

int mfx_ggn_diag(const mfx_ggn_net* net, int dtype, void* diag, void* ws, int64_t ws_bytes, void* stream) {
  MFX_TRY(diag_check(net, dtype));
  MFX_REQUIRE(diag, MFX_ERR_INVALID, "GGN diagonal: diag is NULL");
  const int64_t need = ggn_part_bytes(net, dtype, 1);
  MFX_REQUIRE(ws && need <= ws_bytes, MFX_ERR_WORKSPACE, "GGN diagonal: workspace too small: need %lld bytes", (long long)need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_dtype(dtype, [&](auto t) { return diag_t(net, (decltype(t)*)diag, (decltype(t)*)ws, s); });
}

int64_t mfx_mlp_jac_workspace_bytes(const mfx_ggn_net* net, int dtype, int64_t p) {
  if (jac_check(net, dtype, p) != MFX_OK) return -1;
  return align_up(ggn_part_bytes(net, dtype, p), 256);
}

int mfx_mlp_jac_apply(const mfx_ggn_net* net, int dtype, const void* V, int64_t ldv, int64_t p, void* out, void* stream) {
  MFX_TRY(jac_check(net, dtype, p));
  MFX_REQUIRE(V && out, MFX_ERR_INVALID, "MLP Jacobian: V or out is NULL");
  MFX_REQUIRE(ldv >= ggn_params(net), MFX_ERR_INVALID, "MLP Jacobian: ldv = %lld is less than the P = %lld parameters", (long long)ldv,
              (long long)ggn_params(net));
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_dtype(dtype, [&](auto t) { return jac_apply_t(net, (const decltype(t)*)V, ldv, p, (decltype(t)*)out, s); });
}

int mfx_mlp_jac_t_apply(const mfx_ggn_net* net, int dtype, const void* U, int64_t p, void* Y, int64_t ldy, void* ws, int64_t ws_bytes,
                        void* stream) {
  MFX_TRY(jac_check(net, dtype, p));
  MFX_REQUIRE(U && Y, MFX_ERR_INVALID, "MLP Jacobian: U or Y is NULL");
  MFX_REQUIRE(ldy >= ggn_params(net), MFX_ERR_INVALID, "MLP Jacobian: ldy = %lld is less than the P = %lld parameters", (long long)ldy,
              (long long)ggn_params(net));
  const int64_t need = ggn_part_bytes(net, dtype, p);
  MFX_REQUIRE(ws && need <= ws_bytes, MFX_ERR_WORKSPACE, "MLP Jacobian: workspace too small: need %lld bytes", (long long)need);
  return with_dtype(dtype, [&](auto t) {
    return jac_t_apply_t(net, (const decltype(t)*)U, p, (decltype(t)*)Y, ldy, (decltype(t)*)ws, static_cast<hipStream_t>(stream));
  });
}

}  // extern "C"
