// libmfx: the kernel-Gram operator on the VALU -- the generic path of every entry point (any dtype, any number of vectors, d <= 1024):
// matvec, parameter and input sweeps, the cross-covariance matvec and its VJP, the dense Gram block; with them the workspace carve,
// the k_rbf_prep cache, the switch to the matrix-core paths (mfx_rbf_mfma.hip: matvec; mfx_rbf_mfma_grad.hip: parameter sweeps)
// and the operator kind.
#include <utility>
#include <vector>

#include "mfx_internal.h"
#include "mfx_kernel_fn.h"
#include "mfx_rbf.h"

namespace mfx {

// ================================================================================================
// RBF Gram  K_ij = s exp(-max(0, |x_i/l|^2 + |x_j/l|^2 - 2 (x_i/l).(x_j/l)) / 2) + noise delta_ij
//   (util/gp_util.py:160-176 kernel, :225-226 noise inside the lazy kernel, :525-549 gram matvec)
// ================================================================================================

// xs[i][c] = X[i][c] / l_c (zero padded to DPAD), sq[i] = |xs_i|^2
template <typename T>
__global__ void k_rbf_prep(const T* __restrict__ X, int64_t n, int d, int dpad, const T* __restrict__ ls, int ard,
                           T* __restrict__ xs, T* __restrict__ sq) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T s = T(0);
  for (int c = 0; c < dpad; ++c) {
    T v = T(0);
    if (c < d) v = X[i * d + c] / ls[ard ? c : 0];
    xs[i * dpad + c] = v;
    s += v * v;
  }
  sq[i] = s;
}

// ---- tile steps that the matvec kernels and the Gram block share (every thread of the 256-thread workgroup calls them; no
// barrier inside).  The sweeps keep theirs written out: DESIGN.md section 3.3f ---------------------------------------------------

// sqj[TJ] = the squared norms of the points j0 .. j0 + TJ (points >= end as 0)
template <int TJ, typename T>
__device__ __forceinline__ void stage_sq(const T* __restrict__ sq, int64_t j0, int64_t end, T* sqj) {
  const int tid = threadIdx.x;
  if (tid < TJ) sqj[tid] = (j0 + tid < end) ? sq[j0 + tid] : T(0);
}

// column-point tile of the register kernels: xj[TJ][DPAD] = the points j0 .. j0 + TJ of xs (n, DPAD), with stage_sq
template <int TJ, int DPAD, typename T>
__device__ __forceinline__ void stage_points(const T* __restrict__ xs, const T* __restrict__ sq, int64_t j0, int64_t end,
                                             T (*xj)[DPAD], T* sqj) {
  for (int t = threadIdx.x; t < TJ * DPAD; t += 256) {
    const int64_t g = j0 * DPAD + t;
    (&xj[0][0])[t] = g < end * DPAD ? xs[g] : T(0);
  }
  stage_sq<TJ>(sq, j0, end, sqj);
}

// y = s acc (+ noise x on the rows of the square operator: self) for the PB vectors b0 .. of a matvec workgroup's row i < m
template <typename T, int PB>
__device__ __forceinline__ void store_matvec(const T (&acc)[PB], bool self, int64_t i, int64_t m, int64_t row0, int64_t b0, int64_t p,
                                             const T* __restrict__ outputscale, const T* __restrict__ noise, const T* __restrict__ x,
                                             int64_t ldx, T* __restrict__ y, int64_t ldy) {
  if (i >= m) return;
  const T s = outputscale[0], nz = noise[0];
#pragma unroll
  for (int q = 0; q < PB; ++q)
    if (b0 + q < p) y[(b0 + q) * ldy + i] = self ? s * acc[q] + nz * x[(b0 + q) * ldx + row0 + i] : s * acc[q];
}

constexpr int kRbfTJ = 128;

template <typename T, int DPAD, int PB>
__global__ __launch_bounds__(256) void k_rbf_apply(const T* __restrict__ xs, const T* __restrict__ sq, int64_t n,
                                                   const T* __restrict__ outputscale, const T* __restrict__ noise,
                                                   const T* __restrict__ x, int64_t ldx, T* __restrict__ y,
                                                   int64_t ldy, int64_t p, int kind,
                                                   const T* __restrict__ xrow, const T* __restrict__ sqrow, int64_t m,
                                                   int64_t row0) {
  // rows i < m come from (xrow, sqrow).  row0 >= 0: they are the points row0 .. row0 + m of X itself -- the square Gram
  // operator (or a row block of it): self distances exactly 0, noise on the diagonal; row0 < 0: another point set, the
  // cross-covariance K(X_new, X) of the posterior mean (util/gp_util.py:299-301)
  const bool self = row0 >= 0;
  __shared__ __attribute__((aligned(16))) T xj[kRbfTJ][DPAD];
  __shared__ T sqj[kRbfTJ];
  __shared__ T vj[PB][kRbfTJ];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const int64_t b0 = (int64_t)blockIdx.y * PB;
  const int64_t ic = i < m ? i : m - 1;
  T xi[DPAD];
#pragma unroll
  for (int c = 0; c < DPAD; ++c) xi[c] = xrow[ic * DPAD + c];
  const T sqi = sqrow[ic];
  T acc[PB];
#pragma unroll
  for (int q = 0; q < PB; ++q) acc[q] = T(0);
  for (int64_t j0 = 0; j0 < n; j0 += kRbfTJ) {
    stage_points<kRbfTJ, DPAD>(xs, sq, j0, n, xj, sqj);
    for (int t = tid; t < PB * kRbfTJ; t += 256) {
      const int q = t / kRbfTJ, jj = t % kRbfTJ;
      vj[q][jj] = (b0 + q < p && j0 + jj < n) ? x[(b0 + q) * ldx + j0 + jj] : T(0);
    }
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < kRbfTJ; ++jj) {
      T dot = T(0);
#pragma unroll
      for (int c = 0; c < DPAD; ++c) dot += xi[c] * xj[jj][c];
      T dist = sqi + sqj[jj] - T(2) * dot;
      dist = dist > T(0) ? dist : T(0);
      T kv, wl;
      if (kind == MFX_KERNEL_RBF) {
        kv = exp_neg_half(dist);
      } else {
        if (self && j0 + jj == row0 + i) dist = T(0);  // a point's distance to itself is exactly 0 (sqrt amplifies round-off)
        kernel_eval<T>(kind, dist, kv, wl);
      }
#pragma unroll
      for (int q = 0; q < PB; ++q) acc[q] += kv * vj[q][jj];
    }
    __syncthreads();
  }
  store_matvec(acc, self, i, m, row0, b0, p, outputscale, noise, x, ldx, y, ldy);
}

// tiles of the gradient sweeps: columns per tile, batch entries staged at a time
constexpr int kGradTJ = 16;
constexpr int kGradBC = 32;

// Weight sources of the cross sweeps (k_rbf_cross_grad[_wide]'s Src, further down): tile() gives S of one owner row i against
// the columns j0 .. j0 + TJ (columns >= je as 0), called by every thread of the workgroup at the top of a column tile.  rj is the
// caller's LDS staging tile; only the factored source uses it.
//
// Factored, S_ij = sum_b L_b[i] R_b[j] with L (batch, owners), R (batch, columns): the R slices of kGradBC batch entries at a
// time through rj, S accumulated in registers.  Waves without a live row (wave_live false) only stage.
template <typename T>
struct FactoredSrc {
  const T* L;
  int64_t ldl;
  const T* R;
  int64_t ldr, batch;
  static constexpr int kDotsTag = 1;
  template <int TJ>
  __device__ __forceinline__ void tile(bool live, bool wave_live, int64_t i, int64_t j0, int64_t je, T (*rj)[TJ], T (&S)[TJ]) const {
    const int tid = threadIdx.x;
#pragma unroll
    for (int jj = 0; jj < TJ; ++jj) S[jj] = T(0);
    for (int64_t bt0 = 0; bt0 < batch; bt0 += kGradBC) {
      __syncthreads();
      for (int t = tid; t < kGradBC * TJ; t += 256) {
        const int q = t / TJ, jj = t % TJ;
        rj[q][jj] = (bt0 + q < batch && j0 + jj < je) ? R[(bt0 + q) * ldr + j0 + jj] : T(0);
      }
      __syncthreads();
      if (!wave_live) continue;
      const int qmax = (int)((batch - bt0) < kGradBC ? (batch - bt0) : kGradBC);
      for (int q = 0; q < qmax; ++q) {
        const T l = live ? L[(bt0 + q) * ldl + i] : T(0);
#pragma unroll
        for (int jj = 0; jj < TJ; ++jj) S[jj] += l * rj[q][jj];
      }
    }
  }
};

// Dense, S (m, n) with leading dimension lds given as it is (the predictive variance's S_aj = -2 vbar_a W_aj is diagonal in any
// batch, so the factored form would need batch = m and an m-long inner loop per entry).  TRANS = false, owner = a row of S: the
// thread's own TJ consecutive entries, no other thread reads them, so they go straight to registers as 16-byte vector loads (vec:
// S and lds keep every row's tile 16-byte aligned; the tile is whole) -- an LDS round trip would only add a write, a barrier and a
// read.  Otherwise, and for the tail tile, scalar loads.  TRANS = true, owner = a column of S: entry (j, i), consecutive owners in
// consecutive lanes, coalesced.  No barrier: the loads are in flight while the caller stages the column points.
template <typename T, bool TRANS>
struct DenseSrc {
  const T* S;
  int64_t lds;
  int vec;
  static constexpr int kDotsTag = 2;
  template <int TJ>
  __device__ __forceinline__ void tile(bool live, bool, int64_t i, int64_t j0, int64_t je, T (*)[TJ], T (&s)[TJ]) const {
#pragma unroll
    for (int jj = 0; jj < TJ; ++jj) s[jj] = T(0);
    if (!live) return;
    if (TRANS) {
#pragma unroll
      for (int jj = 0; jj < TJ; ++jj)
        if (j0 + jj < je) s[jj] = S[(j0 + jj) * lds + i];
    } else {
      const T* row = S + i * lds + j0;
      if (vec && j0 + TJ <= je) {
        constexpr int V = 16 / (int)sizeof(T);
#pragma unroll
        for (int u = 0; u < TJ / V; ++u) {
          const Pack<T, V> p = load_pack<T, V>(row + u * V);
#pragma unroll
          for (int e = 0; e < V; ++e) s[u * V + e] = p.v[e];
        }
      } else {
#pragma unroll
        for (int jj = 0; jj < TJ; ++jj)
          if (j0 + jj < je) s[jj] = row[jj];
      }
    }
  }
};

// Parameter-gradient sweep (generic VALU path): workgroup = 256 rows i, walks all j in tiles of 16,
// S_ij = sum_bt L[bt][i] R[bt][j] accumulated in registers, then W = S o K and the per-parameter
// reductions.  Per-workgroup partials (double) -> k_rbf_grad_final (deterministic).
template <typename T, int DPAD>
__global__ __launch_bounds__(256) void k_rbf_grad(const T* __restrict__ xs, const T* __restrict__ sq, int64_t n,
                                                  int ard, int kind, const T* __restrict__ L, int64_t ldl,
                                                  const T* __restrict__ R, int64_t ldr, int64_t batch,
                                                  double* __restrict__ partial /* (nblocks, DPAD + 2) */,
                                                  int64_t row0, int64_t nrow) {
  __shared__ __attribute__((aligned(16))) T xj[kGradTJ][DPAD];
  __shared__ T sqj[kGradTJ];
  __shared__ T rj[kGradBC][kGradTJ];
  __shared__ double red[4][DPAD + 2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t il = (int64_t)blockIdx.x * 256 + tid;  // local row: L is indexed by il, the point is row0 + il
  const bool live = il < nrow;
  const int64_t i = row0 + il;
  const int64_t ic = live ? i : row0 + nrow - 1;
  T xi[DPAD];
#pragma unroll
  for (int c = 0; c < DPAD; ++c) xi[c] = xs[ic * DPAD + c];
  const T sqi = sq[ic];
  double g[DPAD + 2];  // [0..DPAD): lengthscale dims (ARD) or [0] scalar; [DPAD]: outputscale; [DPAD+1]: noise
#pragma unroll
  for (int c = 0; c < DPAD + 2; ++c) g[c] = 0.0;
  for (int64_t j0 = 0; j0 < n; j0 += kGradTJ) {
    T S[kGradTJ];
#pragma unroll
    for (int jj = 0; jj < kGradTJ; ++jj) S[jj] = T(0);
    for (int64_t bt0 = 0; bt0 < batch; bt0 += kGradBC) {
      __syncthreads();
      for (int t = tid; t < kGradBC * kGradTJ; t += 256) {
        const int q = t / kGradTJ, jj = t % kGradTJ;
        rj[q][jj] = (bt0 + q < batch && j0 + jj < n) ? R[(bt0 + q) * ldr + j0 + jj] : T(0);
      }
      __syncthreads();
      const int qmax = (int)((batch - bt0) < kGradBC ? (batch - bt0) : kGradBC);
      for (int q = 0; q < qmax; ++q) {
        const T l = live ? L[(bt0 + q) * ldl + il] : T(0);
#pragma unroll
        for (int jj = 0; jj < kGradTJ; ++jj) S[jj] += l * rj[q][jj];
      }
    }
    __syncthreads();
    for (int t = tid; t < kGradTJ * DPAD; t += 256) {
      const int64_t gi = j0 * DPAD + t;
      (&xj[0][0])[t] = gi < n * DPAD ? xs[gi] : T(0);
    }
    if (tid < kGradTJ) sqj[tid] = (j0 + tid < n) ? sq[j0 + tid] : T(0);
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < kGradTJ; ++jj) {
      if (j0 + jj >= n) continue;
      T dot = T(0);
#pragma unroll
      for (int c = 0; c < DPAD; ++c) dot += xi[c] * xj[jj][c];
      T dist = sqi + sqj[jj] - T(2) * dot;
      dist = dist > T(0) ? dist : T(0);
      if (kind != MFX_KERNEL_RBF && j0 + jj == i) dist = T(0);
      T kv, wl;
      kernel_eval<T>(kind, dist, kv, wl);
      g[DPAD] += (double)(S[jj] * kv);
      const T w = S[jj] * wl;
      if (ard) {
#pragma unroll
        for (int c = 0; c < DPAD; ++c) {
          const T df = xi[c] - xj[jj][c];
          g[c] += (double)(w * df * df);
        }
      } else {
        g[0] += (double)(w * dist);
      }
      if (j0 + jj == i) g[DPAD + 1] += (double)S[jj];
    }
  }
#pragma unroll
  for (int c = 0; c < DPAD + 2; ++c) {
    const double v = wave_sum(live ? g[c] : 0.0);
    if (lane == 0) red[wid][c] = v;
  }
  __syncthreads();
  if (tid < DPAD + 2) partial[(int64_t)blockIdx.x * (DPAD + 2) + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// ------------------------------------------------------------------------------------------------
// Wide inputs, d > 32 (round 5).  The reference's kernel functions take any input dimension (util/gp_util.py:151-184) and its UCI
// loaders go to d = 90 (song) and 385 (slice) (util/uci_util.py:85-99,303-310): refusing them is not an option for a drop-in.  The
// kernels above keep a point in registers (xi[DPAD]); here the scaled points are padded to a multiple of 32 and the distance is a
// small GEMM: a workgroup = 256 rows i x a tile of columns j, the d axis in chunks staged TRANSPOSED through LDS (xiT[c][row],
// xjT[c][col]), each thread accumulating <x_i, x_j> for its row and every column of the tile.  VALU arithmetic in the operator's
// dtype, every mode: correctness and the API first -- these shapes are not on the matrix cores.
// ------------------------------------------------------------------------------------------------
template <typename T> struct Wide { static constexpr int CH = sizeof(T) == 4 ? 32 : 16; };  // d-chunk: 32 KB of LDS for xiT
constexpr int kWideTJ = 32;   // columns per tile, matvec
constexpr int kWideGJ = 16;   // columns per tile, parameter sweep
constexpr int kWideGC = 32;   // ARD dimensions a workgroup of the sweep accumulates (blockIdx.y selects them)

// dot[jj] += <x_i, x_j> over all chunks of the padded d axis; TJ columns j0 .. j0 + TJ.  TAG only separates instantiations: the
// cross sweep takes its own per weight source, Src::kDotsTag (sharing k_rbf_grad_wide's <double, 16> reordered two registers of
// that kernel's code)
template <typename T, int TJ, int TAG = 0>
__device__ __forceinline__ void wide_dots(const T* __restrict__ xs, int64_t n, int dpad, const T* __restrict__ xrow, int64_t ic,
                                          int64_t j0, T (*xiT)[256], T (*xjT)[TJ], T (&dot)[TJ]) {
  constexpr int CH = Wide<T>::CH;
  const int tid = threadIdx.x;
#pragma unroll
  for (int jj = 0; jj < TJ; ++jj) dot[jj] = T(0);
  for (int c0 = 0; c0 < dpad; c0 += CH) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CH; ++c) xiT[c][tid] = xrow[ic * dpad + c0 + c];
    for (int t = tid; t < TJ * CH; t += 256) {
      const int jj = t / CH, c = t % CH;
      xjT[c][jj] = (j0 + jj < n) ? xs[(j0 + jj) * dpad + c0 + c] : T(0);
    }
    __syncthreads();
#pragma unroll 2
    for (int c = 0; c < CH; ++c) {
      const T xic = xiT[c][tid];
#pragma unroll
      for (int jj = 0; jj < TJ; ++jj) dot[jj] += xic * xjT[c][jj];
    }
  }
}

template <typename T, int PB>
__global__ __launch_bounds__(256) void k_rbf_apply_wide(const T* __restrict__ xs, const T* __restrict__ sq, int64_t n, int dpad,
                                                        const T* __restrict__ outputscale, const T* __restrict__ noise,
                                                        const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy,
                                                        int64_t p, int kind, const T* __restrict__ xrow,
                                                        const T* __restrict__ sqrow, int64_t m, int64_t row0) {
  // rows, row0: as k_rbf_apply
  constexpr int CH = Wide<T>::CH;
  const bool self = row0 >= 0;
  __shared__ __attribute__((aligned(16))) T xiT[CH][256];
  __shared__ __attribute__((aligned(16))) T xjT[CH][kWideTJ];
  __shared__ T sqj[kWideTJ];
  __shared__ T vj[PB][kWideTJ];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const int64_t b0 = (int64_t)blockIdx.y * PB;
  const int64_t ic = i < m ? i : m - 1;
  const T sqi = sqrow[ic];
  T acc[PB];
#pragma unroll
  for (int q = 0; q < PB; ++q) acc[q] = T(0);
  for (int64_t j0 = 0; j0 < n; j0 += kWideTJ) {
    __syncthreads();  // the previous tile's vj / sqj are read no more
    stage_sq<kWideTJ>(sq, j0, n, sqj);
    for (int t = tid; t < PB * kWideTJ; t += 256) {
      const int q = t / kWideTJ, jj = t % kWideTJ;
      vj[q][jj] = (b0 + q < p && j0 + jj < n) ? x[(b0 + q) * ldx + j0 + jj] : T(0);
    }
    T dot[kWideTJ];
    wide_dots<T, kWideTJ>(xs, n, dpad, xrow, ic, j0, xiT, xjT, dot);  // (its barriers publish vj / sqj too)
#pragma unroll
    for (int jj = 0; jj < kWideTJ; ++jj) {
      T dist = sqi + sqj[jj] - T(2) * dot[jj];
      dist = dist > T(0) ? dist : T(0);
      T kv, wl;
      if (kind == MFX_KERNEL_RBF) {
        kv = exp_neg_half(dist);
      } else {
        if (self && j0 + jj == row0 + i) dist = T(0);
        kernel_eval<T>(kind, dist, kv, wl);
      }
#pragma unroll
      for (int q = 0; q < PB; ++q) acc[q] += kv * vj[q][jj];  // (columns j >= n carry v = 0)
    }
  }
  store_matvec(acc, self, i, m, row0, b0, p, outputscale, noise, x, ldx, y, ldy);
}

// Parameter sweep for wide inputs: as k_rbf_grad; with ARD the d lengthscale derivatives do not fit a thread's registers, so the
// grid's second axis selects kWideGC of them (S_ij and the kernel weights are re-evaluated per selection: d / 32 times the work of
// a scalar lengthscale -- the price of keeping the direct, cancellation-free form sum_ij w_ij (x_ic - x_jc)^2).
template <typename T>
__global__ __launch_bounds__(256) void k_rbf_grad_wide(const T* __restrict__ xs, const T* __restrict__ sq, int64_t n, int dpad,
                                                       int ard, int kind, const T* __restrict__ L, int64_t ldl,
                                                       const T* __restrict__ R, int64_t ldr, int64_t batch,
                                                       double* __restrict__ partial /* (nblocks, dpad + 2) */, int64_t row0,
                                                       int64_t nrow) {
  constexpr int CH = Wide<T>::CH;
  __shared__ __attribute__((aligned(16))) T xiT[CH][256];
  __shared__ __attribute__((aligned(16))) T xjT[CH][kWideGJ];
  __shared__ __attribute__((aligned(16))) T xjg[kWideGJ][kWideGC];
  __shared__ T sqj[kWideGJ];
  __shared__ T rj[kGradBC][kWideGJ];
  __shared__ double red[4][kWideGC + 2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int gc = (int)blockIdx.y;  // ARD: dimensions gc * 32 .. gc * 32 + 31; scalar lengthscale: one selection
  const int64_t il = (int64_t)blockIdx.x * 256 + tid;
  const bool live = il < nrow;
  const int64_t i = row0 + il;
  const int64_t ic = live ? i : row0 + nrow - 1;
  const T sqi = sq[ic];
  T xig[kWideGC];
#pragma unroll
  for (int c = 0; c < kWideGC; ++c) xig[c] = ard ? xs[ic * dpad + gc * kWideGC + c] : T(0);
  double g[kWideGC + 2];  // [0 .. 32): this selection's lengthscale dims (scalar: [0]); [32]: outputscale; [33]: noise (selection 0 only)
#pragma unroll
  for (int c = 0; c < kWideGC + 2; ++c) g[c] = 0.0;
  for (int64_t j0 = 0; j0 < n; j0 += kWideGJ) {
    T S[kWideGJ];
#pragma unroll
    for (int jj = 0; jj < kWideGJ; ++jj) S[jj] = T(0);
    for (int64_t bt0 = 0; bt0 < batch; bt0 += kGradBC) {
      __syncthreads();
      for (int t = tid; t < kGradBC * kWideGJ; t += 256) {
        const int q = t / kWideGJ, jj = t % kWideGJ;
        rj[q][jj] = (bt0 + q < batch && j0 + jj < n) ? R[(bt0 + q) * ldr + j0 + jj] : T(0);
      }
      __syncthreads();
      const int qmax = (int)((batch - bt0) < kGradBC ? (batch - bt0) : kGradBC);
      for (int q = 0; q < qmax; ++q) {
        const T l = live ? L[(bt0 + q) * ldl + il] : T(0);
#pragma unroll
        for (int jj = 0; jj < kWideGJ; ++jj) S[jj] += l * rj[q][jj];
      }
    }
    __syncthreads();
    if (tid < kWideGJ) sqj[tid] = (j0 + tid < n) ? sq[j0 + tid] : T(0);
    if (ard)
      for (int t = tid; t < kWideGJ * kWideGC; t += 256) {
        const int jj = t / kWideGC, c = t % kWideGC;
        xjg[jj][c] = (j0 + jj < n) ? xs[(j0 + jj) * dpad + gc * kWideGC + c] : T(0);
      }
    T dot[kWideGJ];
    wide_dots<T, kWideGJ>(xs, n, dpad, xs, ic, j0, xiT, xjT, dot);
#pragma unroll
    for (int jj = 0; jj < kWideGJ; ++jj) {
      if (j0 + jj >= n) continue;
      T dist = sqi + sqj[jj] - T(2) * dot[jj];
      dist = dist > T(0) ? dist : T(0);
      if (kind != MFX_KERNEL_RBF && j0 + jj == i) dist = T(0);
      T kv, wl;
      kernel_eval<T>(kind, dist, kv, wl);
      const T w = S[jj] * wl;
      if (gc == 0) {
        g[kWideGC] += (double)(S[jj] * kv);
        if (j0 + jj == i) g[kWideGC + 1] += (double)S[jj];
      }
      if (ard) {
#pragma unroll
        for (int c = 0; c < kWideGC; ++c) {
          const T df = xig[c] - xjg[jj][c];
          g[c] += (double)(w * df * df);
        }
      } else {
        g[0] += (double)(w * dist);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kWideGC + 2; ++c) {
    const double v = wave_sum(live ? g[c] : 0.0);
    if (lane == 0) red[wid][c] = v;
  }
  __syncthreads();
  double* out = partial + (int64_t)blockIdx.x * (dpad + 2);
  if (tid < kWideGC && (ard || tid == 0)) out[gc * kWideGC + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  if (!ard)  // (the columns k_rbf_grad_final sums and drops)
    for (int c = 1 + tid; c < dpad; c += 256) out[c] = 0.0;
  if (gc == 0 && tid >= kWideGC && tid < kWideGC + 2)
    out[dpad + tid - kWideGC] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// ------------------------------------------------------------------------------------------------
// Input sweep: the gradient of G = sum_b L_b^T K R_b = sum_ij S_ij K_ij with respect to the raw inputs X.  With xs = X / l,
// dist_aj = |xs_a - xs_j|^2 and dK/d dist = -s wl / 2 (kernel_eval's weight, all three kernels):
//   dG/dX_ac = -(s / l_c) sum_j (S_aj + S_ja) wl_aj (xs_ac - xs_jc)
// Where the distance is clamped (dist <= 0: the diagonal, duplicated points) the term is 0 -- the reference's max(0, .) passes no
// gradient there.  One row a per thread: S_aj and S_ja of a tile of kGradTJ columns in two register accumulators, the row's d sums
// in registers (double), written once.  Every output row depends only on its own row of S + S^T: no cross-workgroup reduction,
// deterministic.  gx (n, d) row-major is accumulated into.
// ------------------------------------------------------------------------------------------------
template <typename T, int DPAD>
__global__ __launch_bounds__(256) void k_rbf_grad_x(const T* __restrict__ xs, const T* __restrict__ sq, int64_t n, int d,
                                                    int ard, int kind, const T* __restrict__ L, int64_t ldl,
                                                    const T* __restrict__ R, int64_t ldr, int64_t batch,
                                                    const T* __restrict__ ls, const T* __restrict__ outputscale,
                                                    T* __restrict__ gx) {
  __shared__ __attribute__((aligned(16))) T xj[kGradTJ][DPAD];
  __shared__ T sqj[kGradTJ];
  __shared__ T rj[kGradBC][kGradTJ];
  __shared__ T lj[kGradBC][kGradTJ];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const bool live = i < n;
  const int64_t ic = live ? i : n - 1;
  T xi[DPAD];
#pragma unroll
  for (int c = 0; c < DPAD; ++c) xi[c] = xs[ic * DPAD + c];
  const T sqi = sq[ic];
  double g[DPAD];
#pragma unroll
  for (int c = 0; c < DPAD; ++c) g[c] = 0.0;
  for (int64_t j0 = 0; j0 < n; j0 += kGradTJ) {
    T Sa[kGradTJ], St[kGradTJ];  // S_ij and S_ji of this row i and the tile's columns j
#pragma unroll
    for (int jj = 0; jj < kGradTJ; ++jj) Sa[jj] = St[jj] = T(0);
    for (int64_t bt0 = 0; bt0 < batch; bt0 += kGradBC) {
      __syncthreads();
      for (int t = tid; t < kGradBC * kGradTJ; t += 256) {
        const int q = t / kGradTJ, jj = t % kGradTJ;
        const bool in = bt0 + q < batch && j0 + jj < n;
        rj[q][jj] = in ? R[(bt0 + q) * ldr + j0 + jj] : T(0);
        lj[q][jj] = in ? L[(bt0 + q) * ldl + j0 + jj] : T(0);
      }
      __syncthreads();
      const int qmax = (int)((batch - bt0) < kGradBC ? (batch - bt0) : kGradBC);
      for (int q = 0; q < qmax; ++q) {
        const T l = live ? L[(bt0 + q) * ldl + i] : T(0);
        const T r = live ? R[(bt0 + q) * ldr + i] : T(0);
#pragma unroll
        for (int jj = 0; jj < kGradTJ; ++jj) {
          Sa[jj] += l * rj[q][jj];
          St[jj] += r * lj[q][jj];
        }
      }
    }
    __syncthreads();
    for (int t = tid; t < kGradTJ * DPAD; t += 256) {
      const int64_t gi = j0 * DPAD + t;
      (&xj[0][0])[t] = gi < n * DPAD ? xs[gi] : T(0);
    }
    if (tid < kGradTJ) sqj[tid] = (j0 + tid < n) ? sq[j0 + tid] : T(0);
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < kGradTJ; ++jj) {
      if (j0 + jj >= n || j0 + jj == i) continue;
      T dot = T(0);
#pragma unroll
      for (int c = 0; c < DPAD; ++c) dot += xi[c] * xj[jj][c];
      const T dist = sqi + sqj[jj] - T(2) * dot;
      if (!(dist > T(0))) continue;  // clamped: no gradient
      T kv, wl;
      kernel_eval<T>(kind, dist, kv, wl);
      const T w = (Sa[jj] + St[jj]) * wl;
#pragma unroll
      for (int c = 0; c < DPAD; ++c) g[c] += (double)(w * (xi[c] - xj[jj][c]));
    }
  }
  if (!live) return;
  const double s = (double)outputscale[0];
#pragma unroll
  for (int c = 0; c < DPAD; ++c)
    if (c < d) gx[i * d + c] += (T)(-s / (double)ls[ard ? c : 0] * g[c]);
}

constexpr int kWideXJ = 8;  // columns per tile, input sweep (S_ij and S_ji: twice the accumulators of the parameter sweep)

// the input sweep for wide inputs (d > 32): as k_rbf_grad_x with the distances of wide_dots; the row's d sums do not fit a thread's
// registers, so the grid's second axis selects kWideGC of them (S and the distances are re-evaluated per selection, as in
// k_rbf_grad_wide)
template <typename T>
__global__ __launch_bounds__(256) void k_rbf_grad_x_wide(const T* __restrict__ xs, const T* __restrict__ sq, int64_t n, int dpad,
                                                         int d, int ard, int kind, const T* __restrict__ L, int64_t ldl,
                                                         const T* __restrict__ R, int64_t ldr, int64_t batch,
                                                         const T* __restrict__ ls, const T* __restrict__ outputscale,
                                                         T* __restrict__ gx) {
  constexpr int CH = Wide<T>::CH;
  __shared__ __attribute__((aligned(16))) T xiT[CH][256];
  __shared__ __attribute__((aligned(16))) T xjT[CH][kWideXJ];
  __shared__ __attribute__((aligned(16))) T xjg[kWideXJ][kWideGC];
  __shared__ T sqj[kWideXJ];
  __shared__ T rj[kGradBC][kWideXJ];
  __shared__ T lj[kGradBC][kWideXJ];
  const int tid = threadIdx.x;
  const int gc = (int)blockIdx.y;  // dimensions gc * 32 .. gc * 32 + 31
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const bool live = i < n;
  const int64_t ic = live ? i : n - 1;
  const T sqi = sq[ic];
  T xig[kWideGC];
#pragma unroll
  for (int c = 0; c < kWideGC; ++c) xig[c] = xs[ic * dpad + gc * kWideGC + c];
  double g[kWideGC];
#pragma unroll
  for (int c = 0; c < kWideGC; ++c) g[c] = 0.0;
  for (int64_t j0 = 0; j0 < n; j0 += kWideXJ) {
    T Sa[kWideXJ], St[kWideXJ];
#pragma unroll
    for (int jj = 0; jj < kWideXJ; ++jj) Sa[jj] = St[jj] = T(0);
    for (int64_t bt0 = 0; bt0 < batch; bt0 += kGradBC) {
      __syncthreads();
      for (int t = tid; t < kGradBC * kWideXJ; t += 256) {
        const int q = t / kWideXJ, jj = t % kWideXJ;
        const bool in = bt0 + q < batch && j0 + jj < n;
        rj[q][jj] = in ? R[(bt0 + q) * ldr + j0 + jj] : T(0);
        lj[q][jj] = in ? L[(bt0 + q) * ldl + j0 + jj] : T(0);
      }
      __syncthreads();
      const int qmax = (int)((batch - bt0) < kGradBC ? (batch - bt0) : kGradBC);
      for (int q = 0; q < qmax; ++q) {
        const T l = live ? L[(bt0 + q) * ldl + i] : T(0);
        const T r = live ? R[(bt0 + q) * ldr + i] : T(0);
#pragma unroll
        for (int jj = 0; jj < kWideXJ; ++jj) {
          Sa[jj] += l * rj[q][jj];
          St[jj] += r * lj[q][jj];
        }
      }
    }
    __syncthreads();
    if (tid < kWideXJ) sqj[tid] = (j0 + tid < n) ? sq[j0 + tid] : T(0);
    for (int t = tid; t < kWideXJ * kWideGC; t += 256) {
      const int jj = t / kWideGC, c = t % kWideGC;
      xjg[jj][c] = (j0 + jj < n) ? xs[(j0 + jj) * dpad + gc * kWideGC + c] : T(0);
    }
    T dot[kWideXJ];
    wide_dots<T, kWideXJ>(xs, n, dpad, xs, ic, j0, xiT, xjT, dot);  // (its barriers publish sqj / xjg too)
#pragma unroll
    for (int jj = 0; jj < kWideXJ; ++jj) {
      if (j0 + jj >= n || j0 + jj == i) continue;
      const T dist = sqi + sqj[jj] - T(2) * dot[jj];
      if (!(dist > T(0))) continue;
      T kv, wl;
      kernel_eval<T>(kind, dist, kv, wl);
      const T w = (Sa[jj] + St[jj]) * wl;
#pragma unroll
      for (int c = 0; c < kWideGC; ++c) g[c] += (double)(w * (xig[c] - xjg[jj][c]));
    }
  }
  if (!live) return;
  const double s = (double)outputscale[0];
#pragma unroll
  for (int c = 0; c < kWideGC; ++c) {
    const int col = gc * kWideGC + c;
    if (col < d) gx[i * d + col] += (T)(-s / (double)ls[ard ? col : 0] * g[c]);
  }
}

// grads += factors * sum_blocks partial  (chain to the constrained parameters l, s, noise)
template <typename T>
__global__ __launch_bounds__(256) void k_rbf_grad_final(const double* __restrict__ partial, int64_t nblocks, int dpad, int d,
                                                        int ard, const T* __restrict__ ls, const T* __restrict__ outputscale,
                                                        T* __restrict__ g_ls, T* __restrict__ g_s, T* __restrict__ g_noise,
                                                        const float* __restrict__ scales) {
  __shared__ double sm[4];
  const int c = blockIdx.x;  // one workgroup per output column, fixed summation order (deterministic)
  double acc = 0.0;
  for (int64_t q = threadIdx.x; q < nblocks; q += 256) acc += partial[q * (dpad + 2) + c];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  acc = sm[0] + sm[1] + sm[2] + sm[3];
  if (scales) acc *= (double)scales[1] * (double)scales[3];  // undo the power-of-two operand scales of the split GEMM
  const double s = (double)outputscale[0];
  if (c < dpad) {
    if (ard ? (c < d) : (c == 0)) {
      if (g_ls) g_ls[c] += (T)(s * acc / (double)ls[ard ? c : 0]);
    }
  } else if (c == dpad) {
    if (g_s) g_s[0] += (T)acc;
  } else {
    if (g_noise) g_noise[0] += (T)acc;
  }
}

// ------------------------------------------------------------------------------------------------
// Cross-covariance VJP: the gradient of G = sum_b L_b^T K(P, Q) R_b = sum_oj S_oj K_oj (S_oj = sum_b L_b[o] R_b[j], never
// materialised) for two DIFFERENT point sets, the OWNER rows P (mo) and the columns Q (nc).  The posterior mean's
// y = K(X_new, X) v with cotangent ybar is owner = X_new (L = ybar, R = v); its X gradient is the same sum with owner = X
// (L = v, R = ybar).  With xs = x / l, dist = |xs_o - xs_j|^2 as k_rbf_apply computes it and dK/d dist = -s wl / 2:
//   d/ds   = sum S_oj K_oj / s                      d/dl_c = (s / l_c) sum S_oj wl_oj (xs_oc - xs_jc)^2 (scalar l: w dist)
//   d/dP_oc = -(s / l_c) sum_j S_oj wl_oj (xs_oc - xs_jc)
// No noise term.  Pairs with dist <= 0 (a test point equal to a training point) add nothing to the l and P terms (the
// reference's max(0, .), as in k_rbf_grad_x).  One owner row per thread, the other set's columns streamed through LDS in
// tiles; the column range is split over the grid's y axis (z for the wide form) so that a small owner set (a handful of
// acquisition points) still fills the chip.  go != null (a single split): go (mo, d) += the row's sums directly; else
// gpart (splits, mo, DPAD) gets the per-split fp64 sums and k_rbf_cross_gx_final adds them up in split order.  THETA: the
// workgroup's l / s sums go to partial (splits x blocks, DPAD + 2) in k_rbf_grad_final's layout (noise slot 0).  No atomics
// anywhere: bitwise reproducible.
// ------------------------------------------------------------------------------------------------
template <typename T, int DPAD, bool THETA, bool GX, typename Src>
__global__ __launch_bounds__(256) void k_rbf_cross_grad(const T* __restrict__ xo, const T* __restrict__ sqo, int64_t mo,
                                                        const T* __restrict__ xc, const T* __restrict__ sqc, int64_t nc,
                                                        int64_t chunk, int d, int ard, int kind, const Src src,
                                                        const T* __restrict__ ls, const T* __restrict__ outputscale,
                                                        T* __restrict__ go, double* __restrict__ gpart,
                                                        double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) T xj[kGradTJ][DPAD];
  __shared__ T sqj[kGradTJ];
  __shared__ T rj[kGradBC][kGradTJ];  // (the factored source's staging; unused, and not allocated, with a dense source)
  __shared__ double red[4][DPAD + 2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const bool live = i < mo;
  const bool wave_live = (int64_t)blockIdx.x * 256 + wid * 64 < mo;  // (uniform per wave: dead waves only stage tiles)
  const int64_t ic = live ? i : mo - 1;
  const int64_t jb = (int64_t)blockIdx.y * chunk;
  const int64_t je = jb + chunk < nc ? jb + chunk : nc;
  T xi[DPAD];
#pragma unroll
  for (int c = 0; c < DPAD; ++c) xi[c] = xo[ic * DPAD + c];
  const T sqi = sqo[ic];
  double gt[DPAD + 2];  // THETA: [0..DPAD) lengthscale dims (scalar: [0]), [DPAD] outputscale, [DPAD + 1] noise (stays 0)
  double gx[DPAD];
#pragma unroll
  for (int c = 0; c < DPAD + 2; ++c) gt[c] = 0.0;
#pragma unroll
  for (int c = 0; c < DPAD; ++c) gx[c] = 0.0;
  for (int64_t j0 = jb; j0 < je; j0 += kGradTJ) {
    T S[kGradTJ];
    src.template tile<kGradTJ>(live, wave_live, i, j0, je, rj, S);
    __syncthreads();
    for (int t = tid; t < kGradTJ * DPAD; t += 256) {
      const int64_t gi = j0 * DPAD + t;
      (&xj[0][0])[t] = gi < je * DPAD ? xc[gi] : T(0);
    }
    if (tid < kGradTJ) sqj[tid] = (j0 + tid < je) ? sqc[j0 + tid] : T(0);
    __syncthreads();
    if (!wave_live) continue;
#pragma unroll
    for (int jj = 0; jj < kGradTJ; ++jj) {
      if (j0 + jj >= je) continue;
      T dot = T(0);
#pragma unroll
      for (int c = 0; c < DPAD; ++c) dot += xi[c] * xj[jj][c];
      const T raw = sqi + sqj[jj] - T(2) * dot;
      const T dist = raw > T(0) ? raw : T(0);
      T kv, wl;
      kernel_eval<T>(kind, dist, kv, wl);
      if (THETA) gt[DPAD] += (double)(S[jj] * kv);
      if (!(raw > T(0))) continue;  // clamped: no l or input gradient
      const T w = S[jj] * wl;
      if (THETA) {
        if (ard) {
#pragma unroll
          for (int c = 0; c < DPAD; ++c) {
            const T df = xi[c] - xj[jj][c];
            gt[c] += (double)(w * df * df);
          }
        } else {
          gt[0] += (double)(w * dist);
        }
      }
      if (GX) {
#pragma unroll
        for (int c = 0; c < DPAD; ++c) gx[c] += (double)(w * (xi[c] - xj[jj][c]));
      }
    }
  }
  if (THETA) {
#pragma unroll
    for (int c = 0; c < DPAD + 2; ++c) {
      const double v = wave_sum(live ? gt[c] : 0.0);
      if (lane == 0) red[wid][c] = v;
    }
    __syncthreads();
    if (tid < DPAD + 2)
      partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (DPAD + 2) + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  }
  if (!GX || !live) return;
  if (go) {
    const double s = (double)outputscale[0];
#pragma unroll
    for (int c = 0; c < DPAD; ++c)
      if (c < d) go[i * d + c] += (T)(-s / (double)ls[ard ? c : 0] * gx[c]);
  } else if (gpart) {
#pragma unroll
    for (int c = 0; c < DPAD; ++c) gpart[((int64_t)blockIdx.y * mo + i) * DPAD + c] = gx[c];
  }
}

// the cross sweep for wide inputs (d > 32): as k_rbf_cross_grad with the distances of wide_dots; blockIdx.y selects kWideGC of
// the row's d sums (ARD lengthscale and input gradient; a scalar lengthscale without input gradient has one selection, as in
// k_rbf_grad_wide), blockIdx.z is the column split
template <typename T, bool THETA, bool GX, typename Src>
__global__ __launch_bounds__(256) void k_rbf_cross_grad_wide(const T* __restrict__ xo, const T* __restrict__ sqo, int64_t mo,
                                                             const T* __restrict__ xc, const T* __restrict__ sqc, int64_t nc,
                                                             int64_t chunk, int dpad, int d, int ard, int kind, const Src src,
                                                             const T* __restrict__ ls, const T* __restrict__ outputscale,
                                                             T* __restrict__ go, double* __restrict__ gpart,
                                                             double* __restrict__ partial) {
  constexpr int CH = Wide<T>::CH;
  __shared__ __attribute__((aligned(16))) T xiT[CH][256];
  __shared__ __attribute__((aligned(16))) T xjT[CH][kWideGJ];
  __shared__ __attribute__((aligned(16))) T xjg[kWideGJ][kWideGC];
  __shared__ T sqj[kWideGJ];
  __shared__ T rj[kGradBC][kWideGJ];  // (as in k_rbf_cross_grad)
  __shared__ double red[4][kWideGC + 2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int gc = (int)blockIdx.y;  // dimensions gc * 32 .. gc * 32 + 31
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const bool live = i < mo;
  const bool wave_live = (int64_t)blockIdx.x * 256 + wid * 64 < mo;
  const int64_t ic = live ? i : mo - 1;
  const int64_t jb = (int64_t)blockIdx.z * chunk;
  const int64_t je = jb + chunk < nc ? jb + chunk : nc;
  const bool sel = ard || GX;  // this selection's 32 dimensions are needed
  const T sqi = sqo[ic];
  T xig[kWideGC];
#pragma unroll
  for (int c = 0; c < kWideGC; ++c) xig[c] = sel ? xo[ic * dpad + gc * kWideGC + c] : T(0);
  double gt[kWideGC + 2];  // THETA: [0 .. 32) this selection's lengthscale dims (scalar: [0]); [32] outputscale; [33] noise
  double gx[kWideGC];
#pragma unroll
  for (int c = 0; c < kWideGC + 2; ++c) gt[c] = 0.0;
#pragma unroll
  for (int c = 0; c < kWideGC; ++c) gx[c] = 0.0;
  for (int64_t j0 = jb; j0 < je; j0 += kWideGJ) {
    T S[kWideGJ];
    src.template tile<kWideGJ>(live, wave_live, i, j0, je, rj, S);
    __syncthreads();
    if (tid < kWideGJ) sqj[tid] = (j0 + tid < je) ? sqc[j0 + tid] : T(0);
    if (sel)
      for (int t = tid; t < kWideGJ * kWideGC; t += 256) {
        const int jj = t / kWideGC, c = t % kWideGC;
        xjg[jj][c] = (j0 + jj < je) ? xc[(j0 + jj) * dpad + gc * kWideGC + c] : T(0);
      }
    T dot[kWideGJ];
    wide_dots<T, kWideGJ, Src::kDotsTag>(xc, je, dpad, xo, ic, j0, xiT, xjT, dot);  // (its barriers publish sqj / xjg too)
    if (!wave_live) continue;
#pragma unroll
    for (int jj = 0; jj < kWideGJ; ++jj) {
      if (j0 + jj >= je) continue;
      const T raw = sqi + sqj[jj] - T(2) * dot[jj];
      const T dist = raw > T(0) ? raw : T(0);
      T kv, wl;
      kernel_eval<T>(kind, dist, kv, wl);
      if (THETA && gc == 0) gt[kWideGC] += (double)(S[jj] * kv);
      if (!(raw > T(0))) continue;
      const T w = S[jj] * wl;
      if (THETA) {
        if (ard) {
#pragma unroll
          for (int c = 0; c < kWideGC; ++c) {
            const T df = xig[c] - xjg[jj][c];
            gt[c] += (double)(w * df * df);
          }
        } else if (gc == 0) {
          gt[0] += (double)(w * dist);
        }
      }
      if (GX) {
#pragma unroll
        for (int c = 0; c < kWideGC; ++c) gx[c] += (double)(w * (xig[c] - xjg[jj][c]));
      }
    }
  }
  if (THETA) {
#pragma unroll
    for (int c = 0; c < kWideGC + 2; ++c) {
      const double v = wave_sum(live ? gt[c] : 0.0);
      if (lane == 0) red[wid][c] = v;
    }
    __syncthreads();
    double* out = partial + ((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * (dpad + 2);
    if (ard) {
      if (tid < kWideGC) out[gc * kWideGC + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    } else if (gc == 0) {
      if (tid == 0) out[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
      for (int c = 1 + tid; c < dpad; c += 256) out[c] = 0.0;  // (the columns k_rbf_grad_final sums and drops)
    }
    if (gc == 0 && tid >= kWideGC && tid < kWideGC + 2)
      out[dpad + tid - kWideGC] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  }
  if (!GX || !live) return;
  if (go) {
    const double s = (double)outputscale[0];
#pragma unroll
    for (int c = 0; c < kWideGC; ++c) {
      const int col = gc * kWideGC + c;
      if (col < d) go[i * d + col] += (T)(-s / (double)ls[ard ? col : 0] * gx[c]);
    }
  } else if (gpart) {
#pragma unroll
    for (int c = 0; c < kWideGC; ++c) gpart[((int64_t)blockIdx.z * mo + i) * dpad + gc * kWideGC + c] = gx[c];
  }
}

// go (mo, d) += -(s / l_c) * sum over the splits of gpart (splits, mo, dpad), in split order
template <typename T>
__global__ __launch_bounds__(256) void k_rbf_cross_gx_final(const double* __restrict__ gpart, int64_t nsplit, int64_t mo, int dpad,
                                                            int d, int ard, const T* __restrict__ ls,
                                                            const T* __restrict__ outputscale, T* __restrict__ go) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= mo * d) return;
  const int64_t o = e / d;
  const int c = (int)(e % d);
  double acc = 0.0;
  for (int64_t q = 0; q < nsplit; ++q) acc += gpart[(q * mo + o) * dpad + c];
  go[e] += (T)(-(double)outputscale[0] / (double)ls[ard ? c : 0] * acc);
}

// The launch layer of the VALU kernel-Gram kernels.  Every launch site goes through with_dpad (mfx_rbf.h, with rbf_dpad and Const);
// the matvec sites also through one of the two vectors-per-workgroup choosers.

// vectors per workgroup (PB) of k_rbf_apply: launch(Const<PB>)
template <typename Launch>
static void with_apply_pb(int64_t p, Launch&& launch) {
  if (p == 1) launch(Const<1>{});
  else if (p == 2) launch(Const<2>{});
  else if (p <= 4) launch(Const<4>{});
  else launch(Const<8>{});
}

// ... and of k_rbf_apply_wide
template <typename T, typename Launch>
static void with_apply_wide_pb(int64_t p, Launch&& launch) {
  if (p == 1) launch(Const<1>{});
  else if (p <= 4 || sizeof(T) == 8) launch(Const<4>{});  // (8 fp64 vectors next to the 32 fp64 dot products of a tile would spill)
  else if constexpr (sizeof(T) == 4) launch(Const<8>{});
}

// A prepared point set (k_rbf_prep's output): x (m, dpad) = the points over the lengthscale, zero padded; sq (m) = their squared norms
template <typename T>
struct Points {
  const T *x, *sq;
  int64_t m;
};

struct RbfWs {
  void *xs, *sq;
  double* partial;
  float* vscale;  // (rows, 2) power-of-two scales of the f16-split path
  void* hws;      // f16 hi/lo packs of the split gradient sweep (sized for `batch_hint` rows)
  int64_t hws_bytes;
  void* pk;       // pre-packed f16 tile images of the pipelined matvec (sized for `p_apply` vectors)
  int64_t pk_bytes;
};

static int64_t rbf_carve(const mfx_operator* op, void* ws, int64_t ws_bytes, RbfWs* out, int64_t batch_hint = 0,
                         int64_t p_apply = 0) {
  const size_t es = dtype_size(op->dtype);
  const int dpad = rbf_dpad(op->d);
  Carver cv(ws, ws_bytes);
  RbfWs r;
  r.xs = cv.take(op->n * (dpad > 0 ? dpad : 1) * es);
  r.sq = cv.take(op->n * es);
  // per-workgroup gradient partials: VALU sweep n/256 rows, MFMA sweep 8 * n/128 rows, <= 34 doubles each
  r.partial = static_cast<double*>(cv.take(rbf_mfma_grad_partial_rows(op->n) * (dpad > 32 && dpad <= 64 ? dpad + 2 : 34) * sizeof(double)));  // 8 XCDs x 8 sub-ranges (DPAD 64: the matrix-core sweep writes 66 per workgroup; wider: the VALU sweep, dpad + 2 per 256 rows)
  r.vscale = static_cast<float*>(cv.take(kRbfVscaleFloats * sizeof(float)));  // RbfVscaleLayout
  r.hws_bytes = (op->dtype == MFX_F32 && op->rbf_mode == MFX_RBF_F16X3 && batch_hint > 0) ? rbf_grad_h_ws_bytes(op->n, batch_hint) : 0;
  r.hws = r.hws_bytes ? cv.take(r.hws_bytes) : nullptr;
  r.pk_bytes = (op->dtype == MFX_F32 && p_apply > 0) ? rbf_pack_ws_bytes(op, p_apply) : 0;
  r.pk = r.pk_bytes ? cv.take(r.pk_bytes) : nullptr;
  if (out) *out = r;
  return cv.off;
}

// what the last k_rbf_prep inside the current PrepScope of this thread prepared (null: nothing yet)
struct PrepKey {
  const void *x = nullptr, *ls = nullptr, *xs = nullptr;
  int64_t n = 0;
  int d = 0, ard = 0, dtype = 0;
  hipStream_t stream = nullptr;
  bool operator==(const PrepKey& o) const {
    return x == o.x && ls == o.ls && xs == o.xs && n == o.n && d == o.d && ard == o.ard && dtype == o.dtype && stream == o.stream;
  }
};
static thread_local int t_prep_depth = 0;
static thread_local PrepKey t_prep_done;

template <typename T>
static int rbf_prep(const mfx_operator* op, const RbfWs& w, int dpad, hipStream_t stream) {
  PrepKey key;
  key.x = op->x; key.ls = op->lengthscale; key.xs = w.xs; key.n = op->n; key.d = op->d; key.ard = op->ard; key.dtype = op->dtype;
  key.stream = stream;
  if (t_prep_depth > 0 && t_prep_done.xs != nullptr && t_prep_done == key) return MFX_OK;  // same driver call, same operator, same workspace
  k_rbf_prep<T><<<(unsigned)((op->n + 255) / 256), 256, 0, stream>>>(
      (const T*)op->x, op->n, op->d, dpad, (const T*)op->lengthscale, op->ard, (T*)w.xs, (T*)w.sq);
  MFX_CHECK_LAUNCH();
  if (t_prep_depth > 0) t_prep_done = key;
  return MFX_OK;
}

// the operator's own prepared X (rbf_prep's output in the carved workspace)
template <typename T>
static Points<T> own_points(const mfx_operator* op, const RbfWs& w) {
  return {(const T*)w.xs, (const T*)w.sq, op->n};
}

// Another point set (X_new of the cross-covariance, the two sets of a Gram block) is prepared in the caller's workspace:
// points_carve takes its x (m, dpad) and sq (m), es bytes per element, from cv; points_ws_bytes is the size of that; points_prep
// fills it.  On every call: the PrepScope cache of rbf_prep is for the operator's own X alone.
struct PointsWs {
  void *x, *sq;
};
static PointsWs points_carve(Carver& cv, const mfx_operator* op, int64_t m, size_t es) {
  const int dpad = rbf_dpad(op->d) > 0 ? rbf_dpad(op->d) : 1;  // (a size query answers for a d that the entry points refuse)
  PointsWs w;
  w.x = cv.take(m * dpad * es);
  w.sq = cv.take(m * es);
  return w;
}
static int64_t points_ws_bytes(const mfx_operator* op, int64_t m) {
  Carver cv(nullptr, 0);
  points_carve(cv, op, m, dtype_size(op->dtype));
  return cv.off;
}
template <typename T>
static int points_prep(const mfx_operator* op, const T* raw, int64_t m, const PointsWs& w, hipStream_t stream, Points<T>* out) {
  k_rbf_prep<T><<<(unsigned)((m + 255) / 256), 256, 0, stream>>>(raw, m, op->d, rbf_dpad(op->d), (const T*)op->lengthscale, op->ard,
                                                                (T*)w.x, (T*)w.sq);
  MFX_CHECK_LAUNCH();
  *out = {(const T*)w.x, (const T*)w.sq, m};
  return MFX_OK;
}

// y (p, rows.m) = s K(rows, cols) x with x (p, cols.m): the VALU matvec of every entry point.  row0 >= 0: rows are the points
// row0 .. row0 + rows.m of cols -- the square Gram operator or a row block of it, noise on the diagonal; row0 = -1: two different
// point sets (K(X_new, X) v, K(X, X_new) u), noise not read.
template <typename T>
static int rbf_apply_valu(int dpad, const Points<T>& rows, const Points<T>& cols, const T* outputscale, const T* noise, int64_t row0,
                          int kind, const T* x, int64_t ldx, T* y, int64_t ldy, int64_t p, hipStream_t stream) {
  auto grid = [&](int pb) { return dim3((unsigned)((rows.m + 255) / 256), (unsigned)((p + pb - 1) / pb)); };
  with_dpad(
      dpad,
      [&](auto dc) {
        with_apply_pb(p, [&](auto pb) {
          k_rbf_apply<T, decltype(dc)::value, decltype(pb)::value><<<grid(pb), 256, 0, stream>>>(
              cols.x, cols.sq, cols.m, outputscale, noise, x, ldx, y, ldy, p, kind, rows.x, rows.sq, rows.m, row0);
        });
      },
      [&] {
        with_apply_wide_pb<T>(p, [&](auto pb) {
          k_rbf_apply_wide<T, decltype(pb)::value><<<grid(pb), 256, 0, stream>>>(
              cols.x, cols.sq, cols.m, dpad, outputscale, noise, x, ldx, y, ldy, p, kind, rows.x, rows.sq, rows.m, row0);
        });
      });
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

template <typename T>
static int rbf_apply(const mfx_operator* op, const T* x, int64_t ldx, T* y, int64_t ldy, int64_t p, void* ws,
                     int64_t ws_bytes, hipStream_t stream) {
  const int dpad = rbf_dpad(op->d);
  MFX_REQUIRE(dpad > 0, MFX_ERR_UNSUPPORTED, "RBF operator supports d <= 1024 (got %d)", op->d);
  RbfWs w;
  MFX_REQUIRE(rbf_carve(op, ws, ws_bytes, &w, 0, p) <= ws_bytes && ws, MFX_ERR_WORKSPACE, "RBF workspace too small");
  MFX_TRY(rbf_prep<T>(op, w, dpad, stream));
  if constexpr (sizeof(T) == 4) {
    switch (rbf_apply_path(op, p)) {
      case RbfApplyPath::h3:
        return rbf_mfma_apply_h3(op, (const float*)w.xs, (const float*)w.sq, dpad, x, ldx, y, ldy, p, w.vscale, w.pk, stream);
      case RbfApplyPath::exact:
        return rbf_mfma_apply(op, (const float*)w.xs, (const float*)w.sq, dpad, x, ldx, y, ldy, p, stream);
      case RbfApplyPath::valu: break;
    }
  }
  const Points<T> X = own_points<T>(op, w);
  const int64_t row0 = op_row0(op);
  const Points<T> rows{X.x + row0 * dpad, X.sq + row0, op_nrows(op)};  // the operator's row block: a view into its own points
  return rbf_apply_valu<T>(dpad, rows, X, (const T*)op->outputscale, (const T*)op->noise, row0, op->kernel_fn, x, ldx, y, ldy, p,
                           stream);
}

// y (p, m) = K(X_new, X) v: the cross-covariance matvec of the posterior mean (util/gp_util.py:299-305), no noise term
template <typename T>
static int rbf_cross_apply(const mfx_operator* op, const T* xnew, int64_t m, const T* v, int64_t ldv, T* y, int64_t ldy,
                           int64_t p, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const int dpad = rbf_dpad(op->d);
  MFX_REQUIRE(dpad > 0, MFX_ERR_UNSUPPORTED, "RBF operator supports d <= 1024 (got %d)", op->d);
  RbfWs w;
  const int64_t base = rbf_carve(op, ws, ws_bytes, &w);
  Carver cv(ws ? (char*)ws + base : nullptr, ws_bytes - base);
  const PointsWs nw = points_carve(cv, op, m, sizeof(T));
  MFX_REQUIRE(ws && base + cv.off <= ws_bytes, MFX_ERR_WORKSPACE, "cross-Gram workspace too small");
  MFX_TRY(rbf_prep<T>(op, w, dpad, stream));
  Points<T> Xnew;
  MFX_TRY(points_prep<T>(op, xnew, m, nw, stream, &Xnew));
  return rbf_apply_valu<T>(dpad, Xnew, own_points<T>(op, w), (const T*)op->outputscale, (const T*)op->noise, -1, op->kernel_fn, v,
                           ldv, y, ldy, p, stream);
}

int64_t rbf_cross_ws_bytes(const mfx_operator* op, int64_t m) { return rbf_carve(op, nullptr, 0, nullptr) + points_ws_bytes(op, m); }

int op_cross_apply(const mfx_operator* op, const void* xnew, int64_t m, const void* v, int64_t ldv, void* y, int64_t ldy,
                   int64_t p, void* ws, int64_t ws_bytes, hipStream_t stream) {
  MFX_REQUIRE(op->kind == MFX_OP_RBF, MFX_ERR_UNSUPPORTED, "cross-covariance matvec needs a kernel-Gram operator");
  MFX_TRY(check_kernel_fn(op));
  ScopedTimer t(0, stream);
  return with_dtype(op->dtype, [&](auto t) -> int {
    using T = decltype(t);
    return rbf_cross_apply<T>(op, as<T>(xnew), m, as<T>(v), ldv, as<T>(y), ldy, p, ws, ws_bytes, stream);
  });
}

template <typename T>
static int rbf_grad(const mfx_operator* op, const T* L, int64_t ldl, const T* R, int64_t ldr, int64_t batch, int64_t inner,
                    const mfx_op_grads* grads, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const int dpad = rbf_dpad(op->d);
  MFX_REQUIRE(dpad > 0, MFX_ERR_UNSUPPORTED, "RBF operator supports d <= 1024 (got %d)", op->d);
  RbfWs w;
  MFX_REQUIRE(rbf_carve(op, ws, ws_bytes, &w, batch) <= ws_bytes && ws, MFX_ERR_WORKSPACE, "RBF workspace too small");
  MFX_TRY(rbf_prep<T>(op, w, dpad, stream));
  const int64_t row0 = op_row0(op), nrow = op_nrows(op);
  int64_t nblocks = (nrow + 255) / 256;
  bool done = false;
  const float* scales = nullptr;
  if constexpr (sizeof(T) == 4) {
    switch (rbf_grad_path(op, batch, w.hws != nullptr)) {
      case RbfGradPath::split:
        MFX_TRY(rbf_mfma_grad_h(op, (const float*)w.xs, (const float*)w.sq, dpad, L, ldl, R, ldr, batch, inner, w.partial, &nblocks,
                                w.hws, &scales, stream));
        done = true;
        break;
      case RbfGradPath::exact:
        MFX_TRY(rbf_mfma_grad(op, (const float*)w.xs, (const float*)w.sq, dpad, L, ldl, R, ldr, batch, w.partial,
                              &nblocks, stream));
        done = true;
        break;
      case RbfGradPath::valu: break;
    }
  }
  if (!done) {
    with_dpad(
        dpad,
        [&](auto dc) {
          k_rbf_grad<T, decltype(dc)::value><<<(unsigned)nblocks, 256, 0, stream>>>(
              (const T*)w.xs, (const T*)w.sq, op->n, op->ard, op->kernel_fn, L, ldl, R, ldr, batch, w.partial, row0, nrow);
        },
        [&] {
          k_rbf_grad_wide<T><<<dim3((unsigned)nblocks, op->ard ? (unsigned)(dpad / kWideGC) : 1u), 256, 0, stream>>>(
              (const T*)w.xs, (const T*)w.sq, op->n, dpad, op->ard, op->kernel_fn, L, ldl, R, ldr, batch, w.partial, row0, nrow);
        });
    MFX_CHECK_LAUNCH();
  }
  k_rbf_grad_final<T><<<dpad + 2, 256, 0, stream>>>(w.partial, nblocks, dpad, op->d, op->ard, (const T*)op->lengthscale,
                                            (const T*)op->outputscale, (T*)grads->lengthscale,
                                            (T*)grads->outputscale, (T*)grads->noise, scales);
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

// grads->x += dG/dX (the input sweep above).  VALU kernels for every dtype, mode and d: k_rbf_grad_x up to d = 32, k_rbf_grad_x_wide
// beyond.  Whole operator only (the caller refuses row blocks).
template <typename T>
static int rbf_grad_x(const mfx_operator* op, const T* L, int64_t ldl, const T* R, int64_t ldr, int64_t batch,
                      const mfx_op_grads* grads, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const int dpad = rbf_dpad(op->d);
  MFX_REQUIRE(dpad > 0, MFX_ERR_UNSUPPORTED, "RBF operator supports d <= 1024 (got %d)", op->d);
  RbfWs w;
  MFX_REQUIRE(rbf_carve(op, ws, ws_bytes, &w, batch) <= ws_bytes && ws, MFX_ERR_WORKSPACE, "RBF workspace too small");
  MFX_TRY(rbf_prep<T>(op, w, dpad, stream));
  const unsigned nblocks = (unsigned)((op->n + 255) / 256);
  with_dpad(
      dpad,
      [&](auto dc) {
        k_rbf_grad_x<T, decltype(dc)::value><<<nblocks, 256, 0, stream>>>(
            (const T*)w.xs, (const T*)w.sq, op->n, op->d, op->ard, op->kernel_fn, L, ldl, R, ldr, batch, (const T*)op->lengthscale,
            (const T*)op->outputscale, (T*)grads->x);
      },
      [&] {
        k_rbf_grad_x_wide<T><<<dim3(nblocks, (unsigned)(dpad / kWideGC)), 256, 0, stream>>>(
            (const T*)w.xs, (const T*)w.sq, op->n, dpad, op->d, op->ard, op->kernel_fn, L, ldl, R, ldr, batch,
            (const T*)op->lengthscale, (const T*)op->outputscale, (T*)grads->x);
      });
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

// the refusals shared by the transposed cross matvec and the cross VJP (before any launch)
static int check_cross_op(const mfx_operator* op) {
  MFX_REQUIRE(op->kind == MFX_OP_RBF, MFX_ERR_UNSUPPORTED, "cross-covariance matvec needs a kernel-Gram operator");
  MFX_REQUIRE(op->dtype == MFX_F32 || op->dtype == MFX_F64, MFX_ERR_INVALID, "unsupported dtype %d", op->dtype);
  MFX_REQUIRE(op->x && op->lengthscale && op->outputscale, MFX_ERR_INVALID, "RBF operator with null pointers");
  MFX_TRY(check_kernel_fn(op));
  MFX_REQUIRE(op->nrows == 0, MFX_ERR_UNSUPPORTED, "the cross-covariance transpose and VJP need the whole operator (no row block)");
  MFX_REQUIRE(rbf_dpad(op->d) > 0, MFX_ERR_UNSUPPORTED, "RBF operator supports d <= 1024 (got %d)", op->d);
  return MFX_OK;
}

// y (p, n) = K(X, X_new) u, u (p, m): the forward kernels with the roles swapped -- rows from the prepared X, columns from the
// prepared X_new, row0 = -1 (no self distances, no noise).  The noise argument of the kernels is not read in that mode.
template <typename T>
static int rbf_cross_apply_t(const mfx_operator* op, const T* xnew, int64_t m, const T* u, int64_t ldu, T* y, int64_t ldy,
                             int64_t p, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const int dpad = rbf_dpad(op->d);
  RbfWs w;
  const int64_t base = rbf_carve(op, ws, ws_bytes, &w);
  Carver cv(ws ? (char*)ws + base : nullptr, ws_bytes - base);
  const PointsWs nw = points_carve(cv, op, m, sizeof(T));
  MFX_REQUIRE(ws && base + cv.off <= ws_bytes, MFX_ERR_WORKSPACE, "cross-Gram workspace too small");
  MFX_TRY(rbf_prep<T>(op, w, dpad, stream));
  Points<T> Xnew;
  MFX_TRY(points_prep<T>(op, xnew, m, nw, stream, &Xnew));
  const T* s = (const T*)op->outputscale;
  return rbf_apply_valu<T>(dpad, own_points<T>(op, w), Xnew, s, /* noise, not read: */ s, -1, op->kernel_fn, u, ldu, y, ldy, p, stream);
}

int op_cross_apply_t(const mfx_operator* op, const void* xnew, int64_t m, const void* u, int64_t ldu, void* y, int64_t ldy,
                     int64_t p, void* ws, int64_t ws_bytes, hipStream_t stream) {
  MFX_TRY(check_cross_op(op));
  ScopedTimer t(0, stream);
  return with_dtype(op->dtype, [&](auto t) -> int {
    using T = decltype(t);
    return rbf_cross_apply_t<T>(op, as<T>(xnew), m, as<T>(u), ldu, as<T>(y), ldy, p, ws, ws_bytes, stream);
  });
}

// Column split of the cross sweep: enough workgroups (owner blocks x selections x splits) to fill the chip, every split at
// least kCrossMinCols columns, whole tiles of 16 columns (kGradTJ == kWideGJ).  A split count >= 2 routes the owner gradient
// through per-split fp64 partials.
constexpr int64_t kCrossFill = 1024;    // 4 workgroups per CU of the 256
constexpr int64_t kCrossMinCols = 128;
struct CrossPlan {
  int64_t gx, gy, chunk;
};
static CrossPlan cross_plan(int64_t mo, int64_t nc, int64_t sel) {
  CrossPlan c;
  c.gx = (mo + 255) / 256;
  int64_t gy = (kCrossFill + c.gx * sel - 1) / (c.gx * sel);
  const int64_t maxy = (nc + kCrossMinCols - 1) / kCrossMinCols;
  gy = gy < maxy ? gy : maxy;
  gy = gy > 1 ? gy : 1;
  c.chunk = ((nc + gy - 1) / gy + kGradTJ - 1) / kGradTJ * kGradTJ;
  c.gy = (nc + c.chunk - 1) / c.chunk;
  return c;
}

// bytes past rbf_carve: X_new prepared, the l / s partials, the per-split owner partials.  Sized with one selection, the most
// splits any launch of rbf_cross_vjp makes (more selections only lower the split count).
static int64_t cross_vjp_extra(const mfx_operator* op, int64_t m, int64_t* theta_bytes, int64_t* gpart_bytes) {
  const int dpad = rbf_dpad(op->d) > 0 ? rbf_dpad(op->d) : 1;
  int64_t tb = 0, gb = 0;
  const int64_t owners[2][2] = {{m, op->n}, {op->n, m}};
  for (const auto& oc : owners) {
    const CrossPlan pl = cross_plan(oc[0], oc[1], 1);
    const int64_t t = pl.gx * pl.gy * (dpad + 2) * (int64_t)sizeof(double);
    const int64_t g = pl.gy > 1 ? pl.gy * oc[0] * dpad * (int64_t)sizeof(double) : 0;
    tb = t > tb ? t : tb;
    gb = g > gb ? g : gb;
  }
  if (theta_bytes) *theta_bytes = tb;
  if (gpart_bytes) *gpart_bytes = gb;
  return points_ws_bytes(op, m) + align_up(tb, 256) + align_up(gb, 256);
}

int64_t rbf_cross_vjp_ws_bytes(const mfx_operator* op, int64_t m) {
  return rbf_carve(op, nullptr, 0, nullptr) + cross_vjp_extra(op, m, nullptr, nullptr);
}

// one sweep with the owner rows `own` against the columns `col`; src gives S (owners x columns): FactoredSrc with
// L (batch, own.m), R (batch, col.m), or DenseSrc.  The l / s sums and the owner gradient share one sweep where both sets of fp64 sums
// fit the registers (d <= 16); at padded d = 32 and for wide inputs the shared form spills (34 registers at DPAD 32 in fp32), so
// there they are two sweeps.
template <typename T, typename Src>
static int cross_sweep(const mfx_operator* op, int dpad, const Points<T>& own, const Points<T>& col, const Src& src, bool theta, T* go,
                       double* gpart, double* partial, int64_t* nblocks, hipStream_t stream) {
  const bool shared = dpad < 32;
  if (theta && go && !shared) {
    MFX_TRY(cross_sweep<T>(op, dpad, own, col, src, true, nullptr, gpart, partial, nblocks, stream));
    return cross_sweep<T>(op, dpad, own, col, src, false, go, gpart, partial, nblocks, stream);
  }
  const int64_t mo = own.m;
  const int64_t sel = dpad > 32 && (op->ard || go) ? dpad / kWideGC : 1;
  const CrossPlan pl = cross_plan(mo, col.m, sel);
  T* gdirect = pl.gy == 1 ? go : nullptr;
  double* gp = go && pl.gy > 1 ? gpart : nullptr;
  if (theta) *nblocks = pl.gx * pl.gy;
  const T *ls = (const T*)op->lengthscale, *s = (const T*)op->outputscale;
  with_dpad(
      dpad,
      [&](auto dc) {
        constexpr int D = decltype(dc)::value;
        const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
        auto launch = [&](auto th, auto gx) {
          k_rbf_cross_grad<T, D, decltype(th)::value, decltype(gx)::value, Src><<<grid, 256, 0, stream>>>(
              own.x, own.sq, mo, col.x, col.sq, col.m, pl.chunk, op->d, op->ard, op->kernel_fn, src, ls, s, gdirect, gp, partial);
        };
        if (!go) {
          launch(std::true_type{}, std::false_type{});
        } else if (!theta) {
          launch(std::false_type{}, std::true_type{});
        } else {
          if constexpr (D < 32) launch(std::true_type{}, std::true_type{});
        }
      },
      [&] {
        const dim3 grid((unsigned)pl.gx, (unsigned)sel, (unsigned)pl.gy);
        auto launch = [&](auto th, auto gx) {
          k_rbf_cross_grad_wide<T, decltype(th)::value, decltype(gx)::value, Src><<<grid, 256, 0, stream>>>(
              own.x, own.sq, mo, col.x, col.sq, col.m, pl.chunk, dpad, op->d, op->ard, op->kernel_fn, src, ls, s, gdirect, gp, partial);
        };
        if (!go) {
          launch(std::true_type{}, std::false_type{});
        } else {
          launch(std::false_type{}, std::true_type{});
        }
      });
  MFX_CHECK_LAUNCH();
  if (gp) {
    k_rbf_cross_gx_final<T><<<(unsigned)((mo * op->d + 255) / 256), 256, 0, stream>>>(gp, pl.gy, mo, dpad, op->d, op->ard, ls, s, go);
    MFX_CHECK_LAUNCH();
  }
  return MFX_OK;
}

// grads->lengthscale / outputscale += d/dtheta sum_aj S_aj K(X_new_a, X_j), grads->x += d/dX, gxnew += d/dX_new (each if non-null);
// by_new gives S with owner X_new, by_x the same S with owner X (what: the prefix of the workspace message).  Owner X_new carries
// its own gradient and the l / s partials; owner X runs only for grads->x (and then carries the partials when X_new's gradient is
// not asked for, so that a (theta, X) request is two sweeps, not three).
template <typename T, typename SrcNew, typename SrcX>
static int rbf_cross_vjp(const mfx_operator* op, const T* xnew, int64_t m, const SrcNew& by_new, const SrcX& by_x, const char* what,
                         const mfx_op_grads* grads, T* gxnew, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const int dpad = rbf_dpad(op->d);
  RbfWs w;
  const int64_t base = rbf_carve(op, ws, ws_bytes, &w);
  int64_t tb = 0, gb = 0;
  cross_vjp_extra(op, m, &tb, &gb);
  Carver cv(ws ? (char*)ws + base : nullptr, ws_bytes - base);
  const PointsWs nw = points_carve(cv, op, m, sizeof(T));
  double* partial = (double*)cv.take(tb);
  double* gpart = (double*)cv.take(gb);
  MFX_REQUIRE(ws && base + cv.off <= ws_bytes, MFX_ERR_WORKSPACE, "%scross-covariance VJP workspace too small", what);
  const bool theta = grads->lengthscale || grads->outputscale;
  T* gx = (T*)grads->x;
  if (!theta && !gx && !gxnew) return MFX_OK;
  MFX_TRY(rbf_prep<T>(op, w, dpad, stream));
  Points<T> Xnew;
  MFX_TRY(points_prep<T>(op, xnew, m, nw, stream, &Xnew));
  const Points<T> X = own_points<T>(op, w);
  int64_t nblocks = 0;
  if (gxnew || (theta && !gx)) MFX_TRY(cross_sweep<T>(op, dpad, Xnew, X, by_new, theta, gxnew, gpart, partial, &nblocks, stream));
  if (gx) MFX_TRY(cross_sweep<T>(op, dpad, X, Xnew, by_x, theta && !gxnew, gx, gpart, partial, &nblocks, stream));
  if (theta) {
    k_rbf_grad_final<T><<<dpad + 2, 256, 0, stream>>>(partial, nblocks, dpad, op->d, op->ard, (const T*)op->lengthscale,
                                                      (const T*)op->outputscale, (T*)grads->lengthscale, (T*)grads->outputscale,
                                                      nullptr, nullptr);
    MFX_CHECK_LAUNCH();
  }
  return MFX_OK;
}

// S = sum_b L_b^T R_b, L (batch, m), R (batch, n): owner X swaps the two factors
template <typename T>
static int cross_vjp_factored(const mfx_operator* op, const void* xnew, int64_t m, const void* L, int64_t ldl, const void* R,
                              int64_t ldr, int64_t batch, const mfx_op_grads* grads, void* gxnew, void* ws, int64_t ws_bytes,
                              hipStream_t stream) {
  const FactoredSrc<T> by_new{(const T*)L, ldl, (const T*)R, ldr, batch}, by_x{(const T*)R, ldr, (const T*)L, ldl, batch};
  return rbf_cross_vjp<T>(op, (const T*)xnew, m, by_new, by_x, "", grads, (T*)gxnew, ws, ws_bytes, stream);
}

int op_cross_vjp(const mfx_operator* op, const void* xnew, int64_t m, const void* L, int64_t ldl, const void* R, int64_t ldr,
                 int64_t batch, const mfx_op_grads* grads, void* gxnew, void* ws, int64_t ws_bytes, hipStream_t stream) {
  MFX_TRY(check_cross_op(op));
  MFX_REQUIRE(!grads->dense_a && !grads->val, MFX_ERR_INVALID,
              "the cross-covariance VJP fills the kernel-Gram fields only (dense_a / val must be NULL)");
  ScopedTimer t(1, stream);
  return with_dtype(op->dtype,
                    [&](auto t) { return cross_vjp_factored<decltype(t)>(op, xnew, m, L, ldl, R, ldr, batch, grads, gxnew, ws, ws_bytes, stream); });
}

// S (m, n) dense, leading dimension lds: owner X_new reads its rows, owner X its columns.  The row form's 16-byte loads: every
// tile starts at a multiple of 16 columns, so an aligned S and lds keep each tile aligned.
template <typename T>
static int cross_vjp_dense(const mfx_operator* op, const void* xnew, int64_t m, const void* S, int64_t lds, const mfx_op_grads* grads,
                           void* gxnew, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const int vec = (uintptr_t)S % 16 == 0 && (lds * (int64_t)sizeof(T)) % 16 == 0;
  const DenseSrc<T, false> by_new{(const T*)S, lds, vec};
  const DenseSrc<T, true> by_x{(const T*)S, lds, 0};
  return rbf_cross_vjp<T>(op, (const T*)xnew, m, by_new, by_x, "dense ", grads, (T*)gxnew, ws, ws_bytes, stream);
}

int op_cross_vjp_dense(const mfx_operator* op, const void* xnew, int64_t m, const void* S, int64_t lds, const mfx_op_grads* grads,
                       void* gxnew, void* ws, int64_t ws_bytes, hipStream_t stream) {
  MFX_TRY(check_cross_op(op));
  MFX_REQUIRE(!grads->dense_a && !grads->val, MFX_ERR_INVALID,
              "the cross-covariance VJP fills the kernel-Gram fields only (dense_a / val must be NULL)");
  ScopedTimer t(1, stream);
  return with_dtype(op->dtype, [&](auto t) { return cross_vjp_dense<decltype(t)>(op, xnew, m, S, lds, grads, gxnew, ws, ws_bytes, stream); });
}

PrepScope::PrepScope() {
  if (t_prep_depth++ == 0) t_prep_done = PrepKey{};
}
PrepScope::~PrepScope() {
  if (--t_prep_depth == 0) t_prep_done = PrepKey{};
}
// (suspensions nest as calls do: a stack per thread)
static thread_local std::vector<std::pair<int, PrepKey>> t_prep_suspended;
PrepSuspend::PrepSuspend() {
  t_prep_suspended.emplace_back(t_prep_depth, t_prep_done);
  t_prep_depth = 0;
  t_prep_done = PrepKey{};
}
PrepSuspend::~PrepSuspend() {
  t_prep_depth = t_prep_suspended.back().first;
  t_prep_done = t_prep_suspended.back().second;
  t_prep_suspended.pop_back();
}

int check_kernel_fn(const mfx_operator* op) {
  MFX_REQUIRE(op->kernel_fn >= MFX_KERNEL_RBF && op->kernel_fn <= MFX_KERNEL_MATERN52, MFX_ERR_INVALID, "unknown kernel_fn %d",
              op->kernel_fn);
  return MFX_OK;
}

static int gram_check(const mfx_operator* op) {
  MFX_TRY(check_kernel_fn(op));
  MFX_REQUIRE(op->x && op->lengthscale && op->outputscale && op->noise, MFX_ERR_INVALID, "RBF operator with null pointers");
  return MFX_OK;
}

static int gram_check_grads(const mfx_operator* op, const mfx_op_grads* grads, bool sharded) {
  MFX_REQUIRE(!grads->x || (!sharded && op->nrows == 0), MFX_ERR_UNSUPPORTED,
              "the input gradient (grads->x) is not available on row blocks or row-sharded drivers");
  return MFX_OK;
}

static int64_t gram_workspace_bytes(const mfx_operator* op, int64_t batch_hint, int64_t p_apply) {
  return rbf_carve(op, nullptr, 0, nullptr, batch_hint, p_apply);
}

template <typename T>
static int gram_apply(const mfx_operator* op, int, const void* x, int64_t ldx, const void*, int64_t, void* y, int64_t ldy, int64_t p,
                      void* ws, int64_t ws_bytes, hipStream_t stream) {
  return rbf_apply<T>(op, (const T*)x, ldx, (T*)y, ldy, p, ws, ws_bytes, stream);  // symmetric: transpose ignored
}

template <typename T>
static int gram_vjp(const mfx_operator* op, const void* Lv, int64_t ldl, const void* Rv, int64_t ldr, int64_t batch, int64_t inner,
                    const mfx_op_grads* grads, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const T* L = (const T*)Lv;
  const T* R = (const T*)Rv;
  const bool params = grads->lengthscale || grads->outputscale || grads->noise;
  if (!grads->x) {
    if (!params) return MFX_OK;
    return rbf_grad<T>(op, L, ldl, R, ldr, batch, inner, grads, ws, ws_bytes, stream);
  }
  PrepScope prep_scope;  // one k_rbf_prep for both sweeps
  if (params) MFX_TRY(rbf_grad<T>(op, L, ldl, R, ldr, batch, inner, grads, ws, ws_bytes, stream));
  return rbf_grad_x<T>(op, L, ldl, R, ldr, batch, grads, ws, ws_bytes, stream);
}

static const OpKind kGramKind = {gram_check, gram_check_grads, gram_workspace_bytes, {gram_apply<float>, gram_apply<double>},
                                 {gram_vjp<float>, gram_vjp<double>}, nullptr, true, nullptr};
const OpKind* gram_kind() { return &kGramKind; }  // for the table of kinds in mfx_ops.hip

// ================================================================================================
// Dense Gram block: out[a][b] = s kappa(|xa_a / l - xb_b / l|^2) written to memory (mfx_gram_block)
//
// A workgroup owns a 64 x 64 tile of the block.  The 64 points of xb (scaled, with their squared norms) are staged once in LDS;
// a thread keeps ONE scaled point of xa in registers (lane = row of the tile) and evaluates the 16 columns of its wave against it
// -- the LDS reads of a column are wave-uniform, so they broadcast.  The 64 x 64 results go through an LDS tile with a padded
// row (65: the column writes and the row reads are both conflict-free) so that every store instruction of a wave covers 64
// consecutive entries of one output row.  The arithmetic is k_rbf_apply's, in its order: dot product over c, |a|^2 + |b|^2 - 2 a.b,
// clamp at 0, kernel_eval.  Entry (a, b) and entry (b, a) of a symmetric block run the same instructions on the same two numbers
// per step (products and the sum of the two norms commute), so the block comes out bitwise symmetric without a mirror pass; its
// diagonal takes the distance 0 itself.  No atomics, no cross-workgroup state: deterministic.
// ================================================================================================
constexpr int kBlkT = 64;  // tile edge
constexpr int kBlkC = 16;  // columns per thread = kBlkT / 4 waves

// tile[row][col] -> out, a wave per row at a time (256-thread workgroup: rows w, w + 4, ...)
template <typename T>
__device__ __forceinline__ void gram_block_store(const T (*tile)[kBlkT + 1], int64_t a0, int64_t ma, int64_t b0, int64_t mb,
                                                 T* __restrict__ out, int64_t ldo) {
  const int col = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t b = b0 + col;
  if (b >= mb) return;
#pragma unroll 4
  for (int row = w; row < kBlkT; row += 4) {
    const int64_t a = a0 + row;
    if (a < ma) out[a * ldo + b] = tile[row][col];
  }
}

template <typename T>
__device__ __forceinline__ T gram_block_value(int kind, T s, T sqi, T sqj, T dot, bool diag) {
  T dist = sqi + sqj - T(2) * dot;
  dist = dist > T(0) ? dist : T(0);
  if (diag) dist = T(0);  // a point against itself: exactly 0, as the Gram operator takes it
  T kv, wl;
  kernel_eval<T>(kind, dist, kv, wl);
  return s * kv;
}

template <typename T, int DPAD>
__global__ __launch_bounds__(256) void k_gram_block(const T* __restrict__ xa, const T* __restrict__ sqa, int64_t ma,
                                                    const T* __restrict__ xb, const T* __restrict__ sqb, int64_t mb,
                                                    const T* __restrict__ outputscale, int kind, int sym, T* __restrict__ out,
                                                    int64_t ldo) {
  __shared__ __attribute__((aligned(16))) T xj[kBlkT][DPAD];
  __shared__ T sqj[kBlkT];
  __shared__ T tile[kBlkT][kBlkT + 1];
  const int tid = threadIdx.x, r = tid & 63, w = tid >> 6;
  const int64_t a0 = (int64_t)blockIdx.y * kBlkT, b0 = (int64_t)blockIdx.x * kBlkT;
  stage_points<kBlkT, DPAD>(xb, sqb, b0, mb, xj, sqj);
  const int64_t a = a0 + r;
  const int64_t ac = a < ma ? a : ma - 1;
  T xi[DPAD];
#pragma unroll
  for (int c = 0; c < DPAD; ++c) xi[c] = xa[ac * DPAD + c];
  const T sqi = sqa[ac];
  const T s = outputscale[0];
  __syncthreads();
#pragma unroll 4
  for (int jj = 0; jj < kBlkC; ++jj) {
    const int col = w * kBlkC + jj;
    T dot = T(0);
#pragma unroll
    for (int c = 0; c < DPAD; ++c) dot += xi[c] * xj[col][c];
    tile[r][col] = gram_block_value<T>(kind, s, sqi, sqj[col], dot, sym && a == b0 + col);
  }
  __syncthreads();
  gram_block_store<T>(tile, a0, ma, b0, mb, out, ldo);
}

// d > 32: the d axis in chunks of Wide<T>::CH staged transposed through LDS for both point sets ([c][point], the row padded by
// one so that the staging writes -- c fastest, as the global reads -- spread over the banks); 16 running dot products per thread.
template <typename T>
__global__ __launch_bounds__(256) void k_gram_block_wide(const T* __restrict__ xa, const T* __restrict__ sqa, int64_t ma,
                                                         const T* __restrict__ xb, const T* __restrict__ sqb, int64_t mb, int dpad,
                                                         const T* __restrict__ outputscale, int kind, int sym,
                                                         T* __restrict__ out, int64_t ldo) {
  constexpr int CH = Wide<T>::CH;
  __shared__ T xaT[CH][kBlkT + 1];
  __shared__ T xbT[CH][kBlkT + 1];
  __shared__ T sqj[kBlkT];
  __shared__ T tile[kBlkT][kBlkT + 1];
  const int tid = threadIdx.x, r = tid & 63, w = tid >> 6;
  const int64_t a0 = (int64_t)blockIdx.y * kBlkT, b0 = (int64_t)blockIdx.x * kBlkT;
  if (tid < kBlkT) sqj[tid] = (b0 + tid < mb) ? sqb[b0 + tid] : T(0);
  const int64_t a = a0 + r;
  const T sqi = sqa[a < ma ? a : ma - 1];
  const T s = outputscale[0];
  T dot[kBlkC];
#pragma unroll
  for (int jj = 0; jj < kBlkC; ++jj) dot[jj] = T(0);
  for (int c0 = 0; c0 < dpad; c0 += CH) {
    __syncthreads();  // the previous chunk is read no more
    for (int t = tid; t < kBlkT * CH; t += 256) {
      const int pt = t / CH, c = t % CH;
      xaT[c][pt] = (a0 + pt < ma) ? xa[(a0 + pt) * dpad + c0 + c] : T(0);
      xbT[c][pt] = (b0 + pt < mb) ? xb[(b0 + pt) * dpad + c0 + c] : T(0);
    }
    __syncthreads();  // (publishes sqj too)
#pragma unroll 2
    for (int c = 0; c < CH; ++c) {
      const T xic = xaT[c][r];
#pragma unroll
      for (int jj = 0; jj < kBlkC; ++jj) dot[jj] += xic * xbT[c][w * kBlkC + jj];
    }
  }
#pragma unroll
  for (int jj = 0; jj < kBlkC; ++jj) {
    const int col = w * kBlkC + jj;
    tile[r][col] = gram_block_value<T>(kind, s, sqi, sqj[col], dot[jj], sym && a == b0 + col);
  }
  __syncthreads();
  gram_block_store<T>(tile, a0, ma, b0, mb, out, ldo);
}

// workspace: the prepared forms of xa and xb (the symmetric block leaves the second unused)
struct BlockWs {
  PointsWs a, b;
};
static int64_t gram_block_carve(const mfx_operator* op, int64_t ma, int64_t mb, void* ws, int64_t ws_bytes, BlockWs* out) {
  const size_t es = dtype_size(op->dtype);
  Carver cv(ws, ws_bytes);
  BlockWs w;
  w.a = points_carve(cv, op, ma, es);
  w.b = points_carve(cv, op, mb, es);
  if (out) *out = w;
  return cv.off;
}

template <typename T>
static int gram_block_t(const mfx_operator* op, const T* xa, int64_t ma, const T* xb, int64_t mb, T* out, int64_t ldo,
                        const BlockWs& w, hipStream_t stream) {
  const int dpad = rbf_dpad(op->d);
  const int sym = xb == nullptr;
  Points<T> A, B;
  MFX_TRY(points_prep<T>(op, xa, ma, w.a, stream, &A));
  B = A;
  if (!sym) MFX_TRY(points_prep<T>(op, xb, mb, w.b, stream, &B));
  const dim3 grid((unsigned)((mb + kBlkT - 1) / kBlkT), (unsigned)((ma + kBlkT - 1) / kBlkT));
  const T* s = (const T*)op->outputscale;
  with_dpad(
      dpad,
      [&](auto dc) {
        k_gram_block<T, decltype(dc)::value><<<grid, 256, 0, stream>>>(A.x, A.sq, ma, B.x, B.sq, mb, s, op->kernel_fn, sym, out, ldo);
      },
      [&] { k_gram_block_wide<T><<<grid, 256, 0, stream>>>(A.x, A.sq, ma, B.x, B.sq, mb, dpad, s, op->kernel_fn, sym, out, ldo); });
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

// every refusal of mfx_gram_block, before any launch (op->x and op->noise are not looked at: the block has no noise term and its
// point sets are arguments)
static int check_gram_block(const mfx_operator* op, const void* xa, int64_t ma, const void* xb, int64_t mb, const void* out,
                            int64_t ldo) {
  MFX_REQUIRE(op && xa && out, MFX_ERR_INVALID, "mfx_gram_block: null argument");
  MFX_REQUIRE(op->kind == MFX_OP_RBF, MFX_ERR_UNSUPPORTED, "mfx_gram_block needs a kernel-Gram operator");
  MFX_REQUIRE(op->nrows == 0, MFX_ERR_UNSUPPORTED, "mfx_gram_block needs the whole operator (no row block)");
  MFX_REQUIRE(op->lengthscale && op->outputscale, MFX_ERR_INVALID, "mfx_gram_block: RBF operator with null pointers");
  MFX_REQUIRE(ma >= 1 && mb >= 1 && ldo >= mb, MFX_ERR_INVALID, "mfx_gram_block: bad sizes (ma %lld, mb %lld, ldo %lld)",
              (long long)ma, (long long)mb, (long long)ldo);
  MFX_REQUIRE(xb || mb == ma, MFX_ERR_INVALID, "mfx_gram_block: the symmetric block (xb == NULL) needs mb == ma (%lld != %lld)",
              (long long)mb, (long long)ma);
  MFX_TRY(check_kernel_fn(op));
  MFX_REQUIRE(op->dtype == MFX_F32 || op->dtype == MFX_F64, MFX_ERR_INVALID, "unsupported dtype %d", op->dtype);
  MFX_REQUIRE(op->d >= 1, MFX_ERR_INVALID, "mfx_gram_block: d must be >= 1 (got %d)", op->d);
  MFX_REQUIRE(rbf_dpad(op->d) > 0, MFX_ERR_UNSUPPORTED, "RBF operator supports d <= 1024 (got %d)", op->d);
  MFX_REQUIRE((ma + kBlkT - 1) / kBlkT <= 65535 && (mb + kBlkT - 1) / kBlkT <= 2147483647LL, MFX_ERR_UNSUPPORTED,
              "mfx_gram_block: at most %d rows per call", 65535 * kBlkT);
  return MFX_OK;
}

}  // namespace mfx

using namespace mfx;

extern "C" {

int64_t mfx_gram_block_workspace_bytes(const mfx_operator* op, int64_t ma, int64_t mb) {
  if (!op || op->kind != MFX_OP_RBF || ma <= 0 || mb <= 0) return -1;
  return gram_block_carve(op, ma, mb, nullptr, 0, nullptr) + 256;
}

int mfx_gram_block(const mfx_operator* op, const void* xa, int64_t ma, const void* xb, int64_t mb, void* out, int64_t ldo,
                   void* ws, int64_t ws_bytes, void* stream) {
  MFX_TRY(check_gram_block(op, xa, ma, xb, mb, out, ldo));
  BlockWs w;
  MFX_REQUIRE(ws && gram_block_carve(op, ma, mb, ws, ws_bytes, &w) <= ws_bytes, MFX_ERR_WORKSPACE,
              "mfx_gram_block: workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ScopedTimer t(0, s);
  return with_dtype(op->dtype, [&](auto t) -> int {
    using T = decltype(t);
    return gram_block_t<T>(op, as<T>(xa), ma, as<T>(xb), mb, as<T>(out), ldo, w, s);
  });
}

}  // extern "C"
