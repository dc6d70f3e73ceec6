// libmfx: the random-Fourier-feature prior path of a pathwise GP posterior sample (Matheron's rule).
//
//   out[s][i] = c sum_{j<m} cos(2 pi (sum_t O[j][t] x[i][t] / l_t + b[j])) W[s][j]          c = sqrt(2 sigma_f / m)      mfx_rff_apply
//   dx[i][t]  = -2 pi c / l_t sum_s g[s][i] sum_j sin(2 pi (...)_ij) W[s][j] O[j][t]                                     mfx_rff_grad_x
//
// O (m, d) and b (m) come in REVOLUTIONS (frequencies and phases over 2 pi): the phase is accumulated in the compute dtype, reduced
// with fract() -- exact -- and handed to the hardware cosine, whose argument is in revolutions (fp64: cospi / sinpi of 2 fract).
// Matern-1/2 frequencies are Cauchy, so phases of 10^4 and more are ordinary inputs, not an edge case.
//
// GEMM view: M = n rows, N = S samples, K = m features, the K-operand (the (n, m) feature matrix) generated in registers and never
// stored.  A 256-thread workgroup owns 64 R rows (lane = row, R rows per lane) and sweeps the features in tiles of 32 staged in LDS:
// the O tile already divided by the lengthscale, the b tile and the W tile transposed to [feature][sample].  The four waves split
// the 32 features of a tile (8 each), so an entry's phase and cosine are computed exactly once; a lane keeps its rows' sums for all
// SC samples of the chunk in registers, and the four partial sums of a row are added in wave order through LDS at the end.
// Every LDS read of the tile loop is wave-uniform (one address per instruction: a broadcast, no bank conflict whatever d is); the
// O and b staging writes are consecutive per lane; the W tile is read coalesced along the features and written transposed (stride
// SC + pad per feature), which leaves a bank conflict on those few writes per thread and tile.  No atomics, no workspace, a fixed
// summation order: bit-identical from run to run.
// d beyond DC columns is swept in chunks of DC (the x chunk re-read per feature tile; d <= DC keeps the row in registers).
#include "mfx_internal.h"

namespace mfx {

constexpr int kRffFeat = 32;                    // features per staged tile
constexpr int kRffFw = kRffFeat / 4;            // features of a tile per wave
constexpr int kRffRed = 8;                      // samples per pass of the forward's cross-wave sum

template <typename T>
struct RffArgs {
  const T* x;
  int64_t ldx, n;
  int d;
  const T *omega, *phase;
  int64_t m;
  const T* ls;
  int ard;
  const T* os;
  const T* W;
  int64_t ldw;
  int sact;  // samples of this chunk (<= SC)
  const T* g;
  int64_t ldg;
  T* out;  // forward: (S, n) chunk; gradient: dx (n, d)
  int64_t ldout;
  int accumulate;  // gradient: add to dx (every sample chunk after the first)
  int xvec, wvec;  // 16-byte loads of x / W are aligned
};

__device__ __forceinline__ float rff_cos(float p) { return __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(p)); }
__device__ __forceinline__ float rff_sin(float p) { return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(p)); }
__device__ __forceinline__ double rff_cos(double p) { return cospi(2.0 * __builtin_amdgcn_fract(p)); }
__device__ __forceinline__ double rff_sin(double p) { return sinpi(2.0 * __builtin_amdgcn_fract(p)); }

// Om[jj][tt] = O[j0 + jj][t0 + tt] / l_t, zero beyond m and d
template <typename T, int DC>
__device__ __forceinline__ void rff_stage_omega(const RffArgs<T>& a, T* Om, int64_t j0, int t0) {
  for (int idx = threadIdx.x; idx < kRffFeat * DC; idx += 256) {
    const int jj = idx / DC, tt = idx % DC;
    const int64_t j = j0 + jj;
    const int t = t0 + tt;
    T v = T(0);
    if (j < a.m && t < a.d) v = a.omega[j * a.d + t] / a.ls[a.ard ? t : 0];
    Om[idx] = v;
  }
}

// Bs[jj] = b[j0 + jj];  Wt[jj][s] = W[s][j0 + jj], zero beyond m and the chunk's samples
template <typename T, int SC>
__device__ __forceinline__ void rff_stage_bw(const RffArgs<T>& a, T* Bs, T* Wt, int64_t j0) {
  constexpr int VEC = VecWidth<T>::value, SCP = SC + VEC, PK = kRffFeat / VEC;
  if (threadIdx.x < kRffFeat) Bs[threadIdx.x] = j0 + threadIdx.x < a.m ? a.phase[j0 + threadIdx.x] : T(0);
  for (int idx = threadIdx.x; idx < SC * PK; idx += 256) {
    const int s = idx / PK, q = idx % PK;
    const int64_t j = j0 + q * VEC;
    Pack<T, VEC> v;
#pragma unroll
    for (int e = 0; e < VEC; ++e) v.v[e] = T(0);
    if (s < a.sact) {
      const T* wp = a.W + (int64_t)s * a.ldw + j;
      if (a.wvec && j + VEC <= a.m) {
        v = load_pack<T, VEC>(wp);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if (j + e < a.m) v.v[e] = wp[e];
        }
      }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) Wt[(q * VEC + e) * SCP + s] = v.v[e];
  }
}

// xs[r][tt] = x[rows[r]][t0 + tt], zero beyond d
template <typename T, int R, int DC>
__device__ __forceinline__ void rff_load_x(const RffArgs<T>& a, const int64_t (&rows)[R], int t0, T (&xs)[R][DC]) {
  constexpr int VEC = VecWidth<T>::value;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const T* xp = a.x + rows[r] * a.ldx + t0;
#pragma unroll
    for (int q = 0; q < DC / VEC; ++q) {
      if (a.xvec && t0 + (q + 1) * VEC <= a.d) {
        const Pack<T, VEC> v = load_pack<T, VEC>(xp + q * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) xs[r][q * VEC + e] = v.v[e];
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) xs[r][q * VEC + e] = t0 + q * VEC + e < a.d ? xp[q * VEC + e] : T(0);
      }
    }
  }
}

// p[r][f] = b[j] + sum_t Om[j][t] x[r][t] for the FW features j of this wave in the tile at j0 (revolutions); leaves the b / W
// tiles of that tile staged.  nchunk == 1: xs holds the whole row already and only the tiles are staged.
template <typename T, int R, int SC, int DC>
__device__ __forceinline__ void rff_phases(const RffArgs<T>& a, const int64_t (&rows)[R], int wave, int64_t j0, int nchunk, T* Om, T* Bs,
                                           T* Wt, T* OmT, int tc, T (&xs)[R][DC], T (&p)[R][kRffFw]) {
  for (int c = 0; c < nchunk; ++c) {
    __syncthreads();  // the readers of the previous tiles are done
    rff_stage_omega<T, DC>(a, Om, j0, c * DC);
    if (c == 0) {
      rff_stage_bw<T, SC>(a, Bs, Wt, j0);
      if (OmT != Om) rff_stage_omega<T, DC>(a, OmT, j0, tc * DC);
    }
    if (nchunk > 1) rff_load_x<T, R, DC>(a, rows, c * DC, xs);
    __syncthreads();
#pragma unroll
    for (int f = 0; f < kRffFw; ++f) {
      const int jj = wave * kRffFw + f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        T acc = c == 0 ? Bs[jj] : p[r][f];
#pragma unroll
        for (int tt = 0; tt < DC; ++tt) acc += Om[jj * DC + tt] * xs[r][tt];
        p[r][f] = acc;
      }
    }
  }
}

template <typename T, int R, int SC, int DC>
__global__ __launch_bounds__(256) void k_rff_apply(RffArgs<T> a) {
  constexpr int VEC = VecWidth<T>::value, SCP = SC + VEC, ROWS = 64 * R;
  __shared__ __attribute__((aligned(16))) T Om[kRffFeat * DC];
  __shared__ __attribute__((aligned(16))) T Bs[kRffFeat];
  __shared__ __attribute__((aligned(16))) T Wt[kRffFeat * SCP];
  __shared__ __attribute__((aligned(16))) T red[3 * kRffRed * ROWS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * ROWS;
  int64_t rows[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r * 64 + lane;
    rows[r] = row < a.n ? row : a.n - 1;  // loads stay inside x; the store is masked
  }
  const int nchunk = (a.d + DC - 1) / DC;
  T xs[R][DC];
  if (nchunk == 1) rff_load_x<T, R, DC>(a, rows, 0, xs);
  T acc[R][SC];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int s = 0; s < SC; ++s) acc[r][s] = T(0);
  }
  for (int64_t j0 = 0; j0 < a.m; j0 += kRffFeat) {
    T p[R][kRffFw];
    rff_phases<T, R, SC, DC>(a, rows, wave, j0, nchunk, Om, Bs, Wt, Om, 0, xs, p);
#pragma unroll
    for (int f = 0; f < kRffFw; ++f) {
      const int jj = wave * kRffFw + f;
      T phi[R];
#pragma unroll
      for (int r = 0; r < R; ++r) phi[r] = rff_cos(p[r][f]);
#pragma unroll
      for (int s = 0; s < SC; ++s) {
        const T w = Wt[jj * SCP + s];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][s] += phi[r] * w;
      }
    }
  }
  // a row's four partial sums, added in wave order
  const T cscale = sqrt(T(2) * a.os[0] / T(a.m));
#pragma unroll
  for (int s0 = 0; s0 < SC; s0 += kRffRed) {
    __syncthreads();
    if (wave > 0) {
#pragma unroll
      for (int k = 0; k < kRffRed; ++k) {
#pragma unroll
        for (int r = 0; r < R; ++r) red[((wave - 1) * kRffRed + k) * ROWS + r * 64 + lane] = acc[r][s0 + k];
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int k = 0; k < kRffRed; ++k) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          T v = acc[r][s0 + k];
#pragma unroll
          for (int w = 0; w < 3; ++w) v += red[(w * kRffRed + k) * ROWS + r * 64 + lane];
          const int64_t row = row0 + r * 64 + lane;
          if (s0 + k < a.sact && row < a.n) a.out[(int64_t)(s0 + k) * a.ldout + row] = cscale * v;
        }
      }
    }
  }
}

// The VJP onto the points: the phase is recomputed, the sum over the features is local to a row.  Per output chunk of DC columns
// (one chunk when d <= DC) the whole feature sweep runs again, since a phase needs every column of the row.
template <typename T, int R, int SC, int DC>
__global__ __launch_bounds__(256) void k_rff_grad_x(RffArgs<T> a) {
  constexpr int VEC = VecWidth<T>::value, SCP = SC + VEC, ROWS = 64 * R;
  __shared__ __attribute__((aligned(16))) T OmP[kRffFeat * DC];
  __shared__ __attribute__((aligned(16))) T OmO[kRffFeat * DC];
  __shared__ __attribute__((aligned(16))) T Bs[kRffFeat];
  __shared__ __attribute__((aligned(16))) T Wt[kRffFeat * SCP];
  __shared__ __attribute__((aligned(16))) T red[3 * DC * ROWS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * ROWS;
  int64_t rows[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r * 64 + lane;
    rows[r] = row < a.n ? row : a.n - 1;
  }
  const int nchunk = (a.d + DC - 1) / DC;
  T* const OmT = nchunk == 1 ? OmP : OmO;  // the chunk of O the output columns multiply
  T xs[R][DC];
  if (nchunk == 1) rff_load_x<T, R, DC>(a, rows, 0, xs);
  T gi[R][SC];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int s = 0; s < SC; ++s) gi[r][s] = s < a.sact ? a.g[(int64_t)s * a.ldg + rows[r]] : T(0);
  }
  const T scale = T(-6.283185307179586476925286766559) * sqrt(T(2) * a.os[0] / T(a.m));
  for (int tc = 0; tc < nchunk; ++tc) {
    T dxa[R][DC];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int tt = 0; tt < DC; ++tt) dxa[r][tt] = T(0);
    }
    for (int64_t j0 = 0; j0 < a.m; j0 += kRffFeat) {
      T p[R][kRffFw];
      rff_phases<T, R, SC, DC>(a, rows, wave, j0, nchunk, OmP, Bs, Wt, OmT, tc, xs, p);
#pragma unroll
      for (int f = 0; f < kRffFw; ++f) {
        const int jj = wave * kRffFw + f;
        T q[R];
#pragma unroll
        for (int r = 0; r < R; ++r) q[r] = T(0);
#pragma unroll
        for (int s = 0; s < SC; ++s) {
          const T w = Wt[jj * SCP + s];
#pragma unroll
          for (int r = 0; r < R; ++r) q[r] += gi[r][s] * w;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) q[r] *= rff_sin(p[r][f]);
#pragma unroll
        for (int tt = 0; tt < DC; ++tt) {
          const T om = OmT[jj * DC + tt];
#pragma unroll
          for (int r = 0; r < R; ++r) dxa[r][tt] += q[r] * om;
        }
      }
    }
    __syncthreads();
    if (wave > 0) {
#pragma unroll
      for (int tt = 0; tt < DC; ++tt) {
#pragma unroll
        for (int r = 0; r < R; ++r) red[((wave - 1) * DC + tt) * ROWS + r * 64 + lane] = dxa[r][tt];
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t row = row0 + r * 64 + lane;
#pragma unroll
        for (int tt = 0; tt < DC; ++tt) {
          T v = dxa[r][tt];
#pragma unroll
          for (int w = 0; w < 3; ++w) v += red[(w * DC + tt) * ROWS + r * 64 + lane];
          const int t = tc * DC + tt;
          if (row < a.n && t < a.d) {
            T* dst = a.out + row * a.ldout + t;
            *dst = a.accumulate ? *dst + scale * v : scale * v;
          }
        }
      }
    }
  }
}

template <typename T>
struct RffGeom {  // rows per lane, samples per chunk (wide / narrow)
  static constexpr int R = sizeof(T) == 4 ? 2 : 1;
  static constexpr int SC = sizeof(T) == 4 ? 64 : 32;
  static constexpr int SCS = sizeof(T) == 4 ? 16 : 8;
};

template <typename T, int SC, int DC>
static int rff_launch(bool grad, const RffArgs<T>& a, hipStream_t stream) {
  constexpr int R = RffGeom<T>::R;
  const int64_t blocks = (a.n + 64 * R - 1) / (64 * R);
  if (grad) {
    k_rff_grad_x<T, R, SC, DC><<<(unsigned)blocks, 256, 0, stream>>>(a);
  } else {
    k_rff_apply<T, R, SC, DC><<<(unsigned)blocks, 256, 0, stream>>>(a);
  }
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

template <typename T>
static int rff_run(bool grad, const char* who, const void* x, int64_t ldx, int64_t n, int64_t d, const void* omega, const void* phase,
                   int64_t m, const void* ls, int ard, const void* os, const void* W, int64_t ldw, int64_t S, const void* g, int64_t ldg,
                   void* out, int64_t ldout, hipStream_t stream) {
  constexpr int R = RffGeom<T>::R, SC = RffGeom<T>::SC, SCS = RffGeom<T>::SCS, VEC = VecWidth<T>::value;
  MFX_REQUIRE((n + 64 * R - 1) / (64 * R) <= 2147483647LL, MFX_ERR_UNSUPPORTED, "%s: n = %lld needs more than 2^31 - 1 workgroups", who,
              (long long)n);
  RffArgs<T> a;
  a.x = (const T*)x;
  a.ldx = ldx;
  a.n = n;
  a.d = (int)d;
  a.omega = (const T*)omega;
  a.phase = (const T*)phase;
  a.m = m;
  a.ls = (const T*)ls;
  a.ard = ard;
  a.os = (const T*)os;
  a.ldw = ldw;
  a.ldg = ldg;
  a.ldout = ldout;
  a.xvec = ldx % VEC == 0 && (uintptr_t)x % 16 == 0;
  a.wvec = ldw % VEC == 0 && (uintptr_t)W % 16 == 0;  // a chunk starts SC rows further: ldw % VEC keeps it aligned
  // probe chunks, as the Gram launch layer walks them: wide chunks while more than two narrow ones are left, then narrow ones (a
  // narrow launch regenerates the features, d FMAs and a cosine per entry, for SCS sample FMAs: two of them cost less than one wide
  // chunk's SC sample FMAs, three cost more)
  for (int64_t s0 = 0, sc = 0; s0 < S; s0 += sc) {
    sc = S - s0 <= 2 * SCS ? SCS : SC;
    a.W = (const T*)W + s0 * ldw;
    a.sact = (int)(S - s0 < sc ? S - s0 : sc);
    a.g = grad ? (const T*)g + s0 * ldg : nullptr;
    a.out = grad ? (T*)out : (T*)out + s0 * ldout;
    a.accumulate = s0 > 0;
    if (sc == SCS) {
      MFX_TRY(d <= 8 ? (rff_launch<T, SCS, 8>(grad, a, stream)) : (rff_launch<T, SCS, 16>(grad, a, stream)));
    } else {
      MFX_TRY(d <= 8 ? (rff_launch<T, SC, 8>(grad, a, stream)) : (rff_launch<T, SC, 16>(grad, a, stream)));
    }
  }
  return MFX_OK;
}

static int rff_check(const char* who, int dtype, const void* x, int64_t ldx, int64_t n, int64_t d, const void* omega, const void* phase,
                     int64_t m, const void* ls, int ard, const void* os, const void* W, int64_t ldw, int64_t S) {
  MFX_REQUIRE(dtype == MFX_F32 || dtype == MFX_F64, MFX_ERR_INVALID, "%s: unknown dtype %d", who, dtype);
  MFX_REQUIRE(x && omega && phase && ls && os && W, MFX_ERR_INVALID,
              "%s: x, omega, phase, lengthscale, outputscale and W must not be NULL", who);
  MFX_REQUIRE(n >= 1 && m >= 1 && S >= 1, MFX_ERR_INVALID, "%s: n = %lld, m = %lld, S = %lld must all be >= 1", who, (long long)n,
              (long long)m, (long long)S);
  MFX_REQUIRE(d >= 1 && d <= 1024, MFX_ERR_INVALID, "%s: d = %lld must be in 1..1024", who, (long long)d);
  MFX_REQUIRE(ard == 0 || ard == 1, MFX_ERR_INVALID, "%s: ard = %d must be 0 (scalar lengthscale) or 1 (d lengthscales)", who, ard);
  MFX_REQUIRE(ldx >= d, MFX_ERR_INVALID, "%s: ldx = %lld is shorter than a row of x (d = %lld)", who, (long long)ldx, (long long)d);
  MFX_REQUIRE(ldw >= m, MFX_ERR_INVALID, "%s: ldw = %lld is shorter than a row of W (m = %lld)", who, (long long)ldw, (long long)m);
  return MFX_OK;
}

}  // namespace mfx

extern "C" int mfx_rff_apply(int dtype, const void* x, int64_t ldx, int64_t n, int64_t d, const void* omega, const void* phase,
                             int64_t m, const void* lengthscale, int ard, const void* outputscale, const void* W, int64_t ldw,
                             int64_t S, void* out, int64_t ldout, void* stream) {
  using namespace mfx;
  const char* who = "mfx_rff_apply";
  MFX_TRY(rff_check(who, dtype, x, ldx, n, d, omega, phase, m, lengthscale, ard, outputscale, W, ldw, S));
  MFX_REQUIRE(out, MFX_ERR_INVALID, "%s: out must not be NULL", who);
  MFX_REQUIRE(ldout >= n, MFX_ERR_INVALID, "%s: ldout = %lld is shorter than a row of out (n = %lld)", who, (long long)ldout,
              (long long)n);
  return with_dtype(dtype, [&](auto t) -> int {
    return rff_run<decltype(t)>(false, who, x, ldx, n, d, omega, phase, m, lengthscale, ard, outputscale, W, ldw, S, nullptr, 0, out,
                                ldout, (hipStream_t)stream);
  });
}

extern "C" int mfx_rff_grad_x(int dtype, const void* x, int64_t ldx, int64_t n, int64_t d, const void* omega, const void* phase,
                              int64_t m, const void* lengthscale, int ard, const void* outputscale, const void* W, int64_t ldw,
                              int64_t S, const void* g, int64_t ldg, void* dx, int64_t lddx, void* stream) {
  using namespace mfx;
  const char* who = "mfx_rff_grad_x";
  MFX_TRY(rff_check(who, dtype, x, ldx, n, d, omega, phase, m, lengthscale, ard, outputscale, W, ldw, S));
  MFX_REQUIRE(g && dx, MFX_ERR_INVALID, "%s: g and dx must not be NULL", who);
  MFX_REQUIRE(ldg >= n, MFX_ERR_INVALID, "%s: ldg = %lld is shorter than a row of g (n = %lld)", who, (long long)ldg, (long long)n);
  MFX_REQUIRE(lddx >= d, MFX_ERR_INVALID, "%s: lddx = %lld is shorter than a row of dx (d = %lld)", who, (long long)lddx, (long long)d);
  return with_dtype(dtype, [&](auto t) -> int {
    return rff_run<decltype(t)>(true, who, x, ldx, n, d, omega, phase, m, lengthscale, ard, outputscale, W, ldw, S, g, ldg, dx, lddx,
                                (hipStream_t)stream);
  });
}
