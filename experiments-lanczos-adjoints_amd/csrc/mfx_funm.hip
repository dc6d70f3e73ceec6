// libmfx: matrix-function--vector products on the Lanczos path,  f(A) v ~ |v| Q f(T) e1  (DESIGN.md section 3.5b).
//   - coefficients c = scale U (f(lam) o U[0]) of the k x k eigen-problem and their Daleckii-Krein VJP w.r.t. the tridiagonal
//   - the basis combination y = sum_j c_j q_j over the (p, k, n) storage of the basis and its VJP (dQ = c dy^T, dc = Q dy)
// The basis passes run on the vector geometry of mfx_vec.h: the combination IS the update kernel's sweep (y = 0 - sum_j (-c_j) q_j,
// an exact sign flip), the projection Q dy is the dots kernel with its fixed-order fp64 re-reduction; only the rank-one dQ is new.
#include <math.h>

#include "mfx_vec.h"

namespace mfx {

constexpr int kFunmBlock = 256;  // depth regimes: kSmallLdsDepth / kSmallMaxDepth of mfx_internal.h, shared with mfx_small.hip

// coeffs[b][j] = scale[b] sum_a U[j][a] f[a] U[0][a]: one workgroup per vector, one wave per row j, fp64 inside
template <typename T>
__global__ __launch_bounds__(kFunmBlock) void k_funm_coeffs(const T* __restrict__ evecs, const T* __restrict__ fvals,
                                                             const T* __restrict__ scale, int k, T* __restrict__ coeffs) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* g = reinterpret_cast<double*>(smem_raw);  // [k]: f(lam_a) U[0][a]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t b = blockIdx.x;
  const T* U = evecs + b * k * k;
  for (int a = tid; a < k; a += kFunmBlock) g[a] = (double)fvals[b * k + a] * (double)U[a];
  __syncthreads();
  const double sc = (double)scale[b];
  for (int j = wid; j < k; j += kFunmBlock / 64) {
    double acc = 0.0;
    for (int a = lane; a < k; a += 64) acc += (double)U[(int64_t)j * k + a] * g[a];
    acc = wave_sum(acc);
    if (lane == 0) coeffs[b * k + j] = (T)(sc * acc);
  }
}

// VJP of the coefficients w.r.t. (alpha, beta, scale).  With w = U^T dc, u0 = U[0], M_ac = F_ac w_a u0_c (F the divided differences of
// f at the eigenvalues, F_aa = f') and G = U M U^T:  dalpha_i = scale G_ii,  dbeta_i = scale (G_{i,i+1} + G_{i+1,i}),
// dscale = sum_a w_a f_a u0_a.  M is not symmetric (k_quadform_bwd's F o u0 u0^T is): both off-diagonals of G are formed.
// The rule for equal Ritz values is k_quadform_bwd's.  DEEP (k > 120): M is evaluated where it is used; LDS holds lam, f, f', u0, w.
template <typename T, bool DEEP>
__global__ __launch_bounds__(64) void k_funm_coeffs_bwd(const T* __restrict__ evals, const T* __restrict__ evecs,
                                                        const T* __restrict__ fvals, const T* __restrict__ dfvals,
                                                        const T* __restrict__ dcoeffs, const T* __restrict__ scale, int k,
                                                        T* __restrict__ dalpha, T* __restrict__ dbeta, int64_t lddbeta,
                                                        T* __restrict__ dscale) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* sw = reinterpret_cast<double*>(smem_raw);  // [k]
  double* M = sw + k;                                // [k][k], or lam, f, f', u0 (DEEP)
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const T* lam = evals + b * k;
  const T* U = evecs + b * k * k;
  const T* f = fvals + b * k;
  const T* df = dfvals + b * k;
  const T* dc = dcoeffs + b * k;
  double lmax = 0.0;
  for (int a = 0; a < k; ++a) lmax = fmax(lmax, fabs((double)lam[a]));
  const double tol = (sizeof(T) == 4 ? 1e-6 : 1e-13) * lmax;
  double ds = 0.0;
  for (int a = lane; a < k; a += 64) {
    double w = 0.0;
    for (int j = 0; j < k; ++j) w += (double)U[(int64_t)j * k + a] * (double)dc[j];
    sw[a] = w;
    ds += w * (double)f[a] * (double)U[a];
  }
  ds = wave_sum(ds);
  if (dscale && lane == 0) dscale[b] = (T)ds;
  __syncthreads();
  auto entry = [&](int a, int c, double la, double lc, double fa, double fc, double dfa, double dfc, double wa, double uc) {
    const double dl = la - lc;
    const double F = (a == c || fabs(dl) <= tol) ? 0.5 * (dfa + dfc) : (fa - fc) / dl;
    return F * wa * uc;
  };
  double *sl = M, *sf = M + k, *sd = M + 2 * k, *su = M + 3 * k;  // DEEP only
  if (DEEP) {
    for (int a = lane; a < k; a += 64) {
      sl[a] = (double)lam[a];
      sf[a] = (double)f[a];
      sd[a] = (double)df[a];
      su[a] = (double)U[a];
    }
  } else {
    for (int t = lane; t < k * k; t += 64) {
      const int a = t / k, c = t % k;
      M[t] = entry(a, c, (double)lam[a], (double)lam[c], (double)f[a], (double)f[c], (double)df[a], (double)df[c], sw[a], (double)U[c]);
    }
  }
  __syncthreads();
  const double sc = (double)scale[b];
  for (int i = lane; i < k; i += 64) {
    const bool nxt = i + 1 < k;
    const T* Ui = U + (int64_t)i * k;
    const T* Un = U + (int64_t)(nxt ? i + 1 : i) * k;
    double gii = 0.0, gup = 0.0, glo = 0.0;
    for (int a = 0; a < k; ++a) {
      double ti = 0.0, tn = 0.0;  // (M U_i)_a, (M U_{i+1})_a
      for (int c = 0; c < k; ++c) {
        const double m = DEEP ? entry(a, c, sl[a], sl[c], sf[a], sf[c], sd[a], sd[c], sw[a], su[c]) : M[a * k + c];
        ti += m * (double)Ui[c];
        tn += m * (double)Un[c];
      }
      gii += (double)Ui[a] * ti;  // G_ij = sum_a U_ia (M U_j)_a
      gup += (double)Ui[a] * tn;  // G_{i,i+1}
      glo += (double)Un[a] * ti;  // G_{i+1,i}
    }
    dalpha[b * k + i] = (T)(sc * gii);
    if (nxt) dbeta[b * lddbeta + i] = (T)(sc * (gup + glo));
  }
}

// dQ[b][j][:] = coeffs[b][j] dy[b][:]: the slice of dy is loaded once and stored k times
template <typename T, int VEC, int EPT>
__global__ __launch_bounds__(kBlock) void k_basis_outer(const T* __restrict__ coeffs, const T* __restrict__ dy, int64_t n, int k,
                                                        T* __restrict__ dQ) {
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int64_t slice0 = (int64_t)blockIdx.x * ((int64_t)blockDim.x * EPT);
  T dyr[EPT];
  load_own<T, VEC>(dyr, dy + b * n, slice0, n, tid);
  for (int j = 0; j < k; ++j) {
    const T c = coeffs[b * k + j];
    T out[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) out[e] = c * dyr[e];
    store_own<T, VEC>(out, dQ + (b * k + j) * n, slice0, n, tid);
  }
}

// slices of the finest geometry Ctx may choose (one 16-byte load per thread and row, or one wave): what the size query counts
static int64_t combine_max_slices(int64_t n) { return (n + 64 * kEpt - 1) / (64 * kEpt); }

template <typename T>
static Ctx<T> combine_ctx(int64_t n, int64_t k, int64_t p, int vec, hipStream_t s) {
  Ctx<T> c(n, k, p, vec, s);
  c.fine();
  c.kmax = (int)k;  // partial layout (p, k, slices): no remainder row here
  return c;
}

template <typename T>
static int basis_combine_t(const T* Q, const T* coeffs, int64_t n, int64_t k, int64_t p, T* y, hipStream_t s) {
  const Ctx<T> c = combine_ctx<T>(n, k, p, pick_vec<T>(n, {Q, y}), s);
  UpdateArgs<T> a{};
  a.rows = Q;
  a.rows_ldb = k * n;
  a.row_stride = n;
  a.m = (int)k;
  a.extra = coeffs;  // coef_j = s2 extra[b][j]; y = 0 - sum_j coef_j q_j
  a.extra_ldb = k;
  a.extra_stride = 1;
  a.s2 = T(-1);
  a.y = y;
  a.ldy = n;
  return launch_update(c, a, false, false);
}

template <typename T>
static int basis_combine_bwd_t(const T* Q, const T* coeffs, const T* dy, int64_t n, int64_t k, int64_t p, T* dQ, T* dcoeffs,
                               T* partial, hipStream_t s) {
  // each half on a geometry of its own pointers: neither output depends on whether the other is asked for
  if (dQ) {
    const Ctx<T> c = combine_ctx<T>(n, k, p, pick_vec<T>(n, {dy, dQ}), s);
    MFX_VEC_EPT_SWITCH(c, (k_basis_outer<T, VEC, EPT><<<c.grid(), c.wg, 0, s>>>(coeffs, dy, n, (int)k, dQ)));
    MFX_CHECK_LAUNCH();
  }
  if (dcoeffs) {
    const Ctx<T> c = combine_ctx<T>(n, k, p, pick_vec<T>(n, {Q, dy}), s);
    MFX_TRY(launch_dots(c, Q, k * n, n, (int)k, dy, n, partial));
    k_compact_partials<T><<<(unsigned)p, 256, 0, s>>>(partial, (int)k, c.nblk, (int)k, dcoeffs);
    MFX_CHECK_LAUNCH();
  }
  return MFX_OK;
}

static int check_combine_shape(int64_t n, int64_t k, int64_t p, int dtype) {
  MFX_REQUIRE(n >= 1 && k >= 1 && p >= 1, MFX_ERR_INVALID, "n, k, p must be positive (got %lld, %lld, %lld)", (long long)n, (long long)k,
              (long long)p);
  MFX_REQUIRE(dtype == MFX_F32 || dtype == MFX_F64, MFX_ERR_UNSUPPORTED, "unsupported dtype %d", dtype);
  MFX_REQUIRE(k <= kSmallMaxDepth, MFX_ERR_UNSUPPORTED, "basis combination supports k <= %d (got %lld)", kSmallMaxDepth, (long long)k);
  MFX_REQUIRE(p <= 65535, MFX_ERR_UNSUPPORTED, "basis combination supports p <= 65535 vectors per call (got %lld)", (long long)p);
  MFX_REQUIRE(combine_max_slices(n) <= INT32_MAX, MFX_ERR_UNSUPPORTED, "n = %lld is too long", (long long)n);
  return MFX_OK;
}

}  // namespace mfx

using namespace mfx;

extern "C" {

int mfx_funm_coeffs(const void* evals, const void* evecs, const void* fvals, const void* scale, int64_t p, int64_t k, int dtype,
                    void* coeffs, void* stream) {
  MFX_REQUIRE(evals && evecs && fvals && scale && coeffs, MFX_ERR_INVALID, "null argument");
  MFX_REQUIRE(p >= 1 && k >= 1, MFX_ERR_INVALID, "p, k must be positive");
  MFX_REQUIRE(p <= INT32_MAX, MFX_ERR_UNSUPPORTED, "one workgroup per vector: p <= 2^31 - 1 (got %lld)", (long long)p);
  MFX_REQUIRE(dtype == MFX_F32 || dtype == MFX_F64, MFX_ERR_UNSUPPORTED, "unsupported dtype %d", dtype);
  MFX_REQUIRE(k <= kSmallMaxDepth, MFX_ERR_UNSUPPORTED, "funm coefficients support k <= %d (got %lld)", kSmallMaxDepth, (long long)k);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t sh = (size_t)k * sizeof(double);
  return with_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    k_funm_coeffs<T><<<(unsigned)p, kFunmBlock, sh, s>>>(as<T>(evecs), as<T>(fvals), as<T>(scale), (int)k, as<T>(coeffs));
    MFX_CHECK_LAUNCH();
    return MFX_OK;
  });
}

int mfx_funm_coeffs_bwd(const void* evals, const void* evecs, const void* fvals, const void* dfvals, const void* dcoeffs,
                        const void* scale, int64_t p, int64_t k, int dtype, void* dalpha, void* dbeta, int64_t lddbeta, void* dscale,
                        void* stream) {
  MFX_REQUIRE(evals && evecs && fvals && dfvals && dcoeffs && scale && dalpha && (dbeta || k == 1), MFX_ERR_INVALID, "null argument");
  MFX_REQUIRE(p >= 1 && k >= 1, MFX_ERR_INVALID, "p, k must be positive");
  MFX_REQUIRE(k == 1 || lddbeta >= k - 1, MFX_ERR_INVALID, "lddbeta = %lld is shorter than the k - 1 = %lld off-diagonal entries",
              (long long)lddbeta, (long long)(k - 1));
  MFX_REQUIRE(p <= INT32_MAX, MFX_ERR_UNSUPPORTED, "one workgroup per vector: p <= 2^31 - 1 (got %lld)", (long long)p);
  MFX_REQUIRE(dtype == MFX_F32 || dtype == MFX_F64, MFX_ERR_UNSUPPORTED, "unsupported dtype %d", dtype);
  MFX_REQUIRE(k <= kSmallMaxDepth, MFX_ERR_UNSUPPORTED, "funm coefficient backward supports k <= %d (got %lld)", kSmallMaxDepth, (long long)k);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool deep = k > kSmallLdsDepth;
  const size_t sh = (size_t)(k + (deep ? 4 * k : k * k)) * sizeof(double);
  return with_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    return with_flag(deep, [&](auto deep_tag) -> int {
      constexpr bool DEEP = decltype(deep_tag)::value;
      MFX_TRY(allow_big_lds(k_funm_coeffs_bwd<T, DEEP>, sh));
      k_funm_coeffs_bwd<T, DEEP><<<(unsigned)p, 64, sh, s>>>(as<T>(evals), as<T>(evecs), as<T>(fvals), as<T>(dfvals), as<T>(dcoeffs),
                                                             as<T>(scale), (int)k, as<T>(dalpha), as<T>(dbeta), lddbeta, as<T>(dscale));
      MFX_CHECK_LAUNCH();
      return MFX_OK;
    });
  });
}

int mfx_basis_combine(const void* Q, const void* coeffs, int64_t n, int64_t k, int64_t p, int dtype, void* y, void* stream) {
  MFX_REQUIRE(Q && coeffs && y, MFX_ERR_INVALID, "null argument");
  MFX_TRY(check_combine_shape(n, k, p, dtype));
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    return basis_combine_t<T>(as<T>(Q), as<T>(coeffs), n, k, p, as<T>(y), s);
  });
}

int64_t mfx_basis_combine_workspace_bytes(int64_t n, int64_t k, int64_t p, int dtype) {
  if (check_combine_shape(n, k, p, dtype) != MFX_OK) return -1;
  Carver cv(nullptr, 0);
  cv.take(p * k * combine_max_slices(n) * (int64_t)dtype_size(dtype));  // per-slice partials of <q_j, dy>
  return cv.off;
}

int mfx_basis_combine_bwd(const void* Q, const void* coeffs, const void* dy, int64_t n, int64_t k, int64_t p, int dtype, void* dQ,
                          void* dcoeffs, void* ws, int64_t ws_bytes, void* stream) {
  MFX_REQUIRE(dy && (dQ || dcoeffs), MFX_ERR_INVALID, "null argument");
  MFX_REQUIRE(!dQ || coeffs, MFX_ERR_INVALID, "dQ needs the coefficients");
  MFX_REQUIRE(!dcoeffs || Q, MFX_ERR_INVALID, "dcoeffs needs the basis");
  MFX_TRY(check_combine_shape(n, k, p, dtype));
  void* partial = nullptr;
  if (dcoeffs) {
    const int64_t need = mfx_basis_combine_workspace_bytes(n, k, p, dtype);
    MFX_REQUIRE(ws && ws_bytes >= need, MFX_ERR_WORKSPACE, "workspace too small: %lld bytes given, %lld needed", (long long)ws_bytes,
                (long long)need);
    partial = ws;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    return basis_combine_bwd_t<T>(as<T>(Q), as<T>(coeffs), as<T>(dy), n, k, p, as<T>(dQ), as<T>(dcoeffs), as<T>(partial), s);
  });
}

}  // extern "C"
