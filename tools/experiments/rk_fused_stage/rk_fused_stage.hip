// EXPERIMENT, not built into libmfx: the fused Runge-Kutta stencil stage, K_i = A (y + dt sum_j a_ij K_j) in one launch, with the
// combination of a 64 x 16 tile and its one-cell ring formed once in LDS.  Measured against the unfused route (k_rk_combine followed
// by k_stencil_apply) at res = 1000, wave form, Neumann, dopri5 with 9 steps, alternating windows (bench_rk_fused_vs_unfused.log in
// this directory, entry "fuse_dopri5_ms"): fp64 3 % faster, which is below three times the window-to-window spread; fp32 13 % (forward)
// and 7-8 % (forward + backward) SLOWER.  DESIGN.md section 3.4b has the table and the reading.  Bit-identical to the unfused route
// on every grid, form, boundary and dtype tested while it was in the library (both routes went through rk_combine_at and
// stencil_sum / stencil_emit below).  18-22 VGPRs, no scratch, 4752 B (fp32) / 9504 B (fp64) of LDS.
// To try it again: include this file from csrc/mfx_rk.hip, have k_stencil_apply call stencil_sum / stencil_emit, and launch it in
// rk_stage for MFX_OP_STENCIL with grid = (min(tiles, 2^20), p), 256 threads.
#include "../../../experiments-lanczos-adjoints_amd/csrc/mfx_internal.h"

namespace mfx {

constexpr int kStX = 64;       // columns of a workgroup's tile (one wave per row)
constexpr int kStRows = 4;     // rows per wave
constexpr int kStY = 4 * kStRows;  // rows of a workgroup's tile
constexpr int64_t kStMaxGrid = 1 << 20;  // workgroups per launch along x; larger grids walk their tiles in a loop

template <typename T>
struct StencilArgs {
  int ny, nx, form, neumann;
  unsigned mask;  // bit t set: w[t] != 0
  T w[9];
  const T* coef;  // (ny, nx) or null = ones
  int64_t tiles;  // tiles_x * tiles_y
  int tiles_x;
};

template <typename T>
static StencilArgs<T> stencil_args(const mfx_operator* op) {
  StencilArgs<T> a;
  a.ny = op->st_ny;
  a.nx = op->st_nx;
  a.form = op->st_form;
  a.neumann = op->st_boundary == MFX_BOUNDARY_NEUMANN;
  a.mask = 0;
  for (int t = 0; t < 9; ++t) {
    a.w[t] = (T)op->st_w[t];
    if (op->st_w[t] != 0.0) a.mask |= 1u << t;
  }
  a.coef = (const T*)op->val;
  a.tiles_x = (a.nx + kStX - 1) / kStX;
  a.tiles = (int64_t)a.tiles_x * ((a.ny + kStY - 1) / kStY);
  return a;
}

// u_pad[rr, cc] for a cell or a cell of the padding ring
template <typename T>
__device__ __forceinline__ T padded(const T* __restrict__ u, int rr, int cc, int ny, int nx, int neumann) {
  if (neumann) {
    rr = rr < 0 ? 0 : (rr >= ny ? ny - 1 : rr);
    cc = cc < 0 ? 0 : (cc >= nx ? nx - 1 : cc);
    return u[(int64_t)rr * nx + cc];
  }
  return (rr >= 0 && rr < ny && cc >= 0 && cc < nx) ? u[(int64_t)rr * nx + cc] : T(0);
}

// sum_t w[t] at(r + dr_t, c + dc_t), the terms in the order of the weights, one fused multiply-add per term.  `at` returns
// u_pad at a cell or a cell of the padding ring: from memory (stencil_at) or from a tile in LDS (the fused Runge-Kutta stage) --
// the same operands through the same instructions, so the two agree bit for bit.
template <typename T, typename F>
__device__ __forceinline__ T stencil_sum(const StencilArgs<T>& a, int r, int c, F&& at) {
  T s = T(0);
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    if (a.mask >> t & 1u) s = fma(a.w[t], at(r + t / 3 - 1, c + t % 3 - 1), s);
  }
  return s;
}

// (S u)[r, c]
template <typename T>
__device__ __forceinline__ T stencil_at(const StencilArgs<T>& a, const T* __restrict__ u, int r, int c) {
  return stencil_sum<T>(a, r, c, [&](int rr, int cc) { return padded<T>(u, rr, cc, a.ny, a.nx, a.neumann); });
}

// cell i of y = A x from v = (S x.u)[i] and, for the two-block forms, pass = x[m + i]: the field, the sign and the pass-through block
template <typename T>
__device__ __forceinline__ void stencil_emit(const StencilArgs<T>& a, T v, T pass, T* __restrict__ y, int64_t i, int64_t m) {
  if (a.coef) v *= a.coef[i];
  if (a.form == MFX_STENCIL_HEAT) {
    y[i] = v;
  } else if (a.form == MFX_STENCIL_HEAT2) {
    y[i] = -v;
    y[m + i] = pass;
  } else {
    y[i] = pass;
    y[m + i] = v;
  }
}

constexpr int kRkBaseBit = MFX_RK_MAX_STAGES;  // bit of RkCoef::mask that says "the base term is present"

template <typename T>
struct RkCoef {
  unsigned mask;  // bit j < 16: c[j] != 0; bit 16: c0 != 0
  T c0;
  T c[MFX_RK_MAX_STAGES];
};

// the two steps of one element of a combination: every kernel goes through them, in the order base, row 0, row 1, ...
template <typename T>
__device__ __forceinline__ T rk_scale(T c0, T base) {
  return c0 * base;
}
template <typename T>
__device__ __forceinline__ T rk_axpy(T c, T v, T acc) {
  return fma(c, v, acc);
}

// element i of c0 base + sum_j c_j rows[j]
template <typename T>
__device__ __forceinline__ T rk_combine_at(const RkCoef<T>& k, const T* __restrict__ base, const T* __restrict__ rows, int64_t row_stride,
                                           int64_t i) {
  T acc = (k.mask >> kRkBaseBit & 1u) ? rk_scale<T>(k.c0, base[i]) : T(0);
#pragma unroll
  for (int j = 0; j < MFX_RK_MAX_STAGES; ++j) {
    if (k.mask >> j & 1u) acc = rk_axpy<T>(k.c[j], rows[(int64_t)j * row_stride + i], acc);
  }
  return acc;
}

// K = A Y with Y = c0 base + sum_j c_j rows[j] for a stencil operator, Y never leaving the chip unless asked for (yout != null:
// the adjoint drivers need the stage values as the right factor of the parameter sweep).  A workgroup takes 64 x 16 tiles as
// k_stencil_apply does (wave w: rows 4 w .. 4 w + 3, lane = column); per tile it forms Y on the 66 x 18 cells of the tile and its
// ring -- a ring cell outside the grid is the clamped cell's Y (Neumann) or 0 (Dirichlet), which is what `padded` returns -- and
// applies the nine-term sum from LDS.  The second block of the two-block forms is combined where it is passed through.
constexpr int kRkTileX = kStX + 2, kRkTileY = kStY + 2;
template <typename T, bool WRITE_Y>
__global__ __launch_bounds__(256) void k_rk_stencil_stage(StencilArgs<T> a, RkCoef<T> k, const T* __restrict__ base, int64_t ldbase,
                                                          const T* __restrict__ rows, int64_t rows_ldb, int64_t row_stride,
                                                          T* __restrict__ yout, int64_t ldyout, T* __restrict__ kout, int64_t ldk) {
  __shared__ T tile[kRkTileY][kRkTileX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = (int64_t)a.ny * a.nx;
  base += (int64_t)blockIdx.y * ldbase;
  rows += (int64_t)blockIdx.y * rows_ldb;
  kout += (int64_t)blockIdx.y * ldk;
  if (WRITE_Y) yout += (int64_t)blockIdx.y * ldyout;
  for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
    const int c0 = (int)(t % a.tiles_x) * kStX, r0 = (int)(t / a.tiles_x) * kStY;
    for (int idx = tid; idx < kRkTileX * kRkTileY; idx += 256) {
      const int lr = idx / kRkTileX, lc = idx - lr * kRkTileX;
      int rr = r0 + lr - 1, cc = c0 + lc - 1;
      bool cell = rr >= 0 && rr < a.ny && cc >= 0 && cc < a.nx;
      if (a.neumann) {
        rr = rr < 0 ? 0 : (rr >= a.ny ? a.ny - 1 : rr);
        cc = cc < 0 ? 0 : (cc >= a.nx ? a.nx - 1 : cc);
        cell = true;
      }
      tile[lr][lc] = cell ? rk_combine_at<T>(k, base, rows, row_stride, (int64_t)rr * a.nx + cc) : T(0);
    }
    __syncthreads();
    const int c = c0 + lane;
    if (c < a.nx) {
#pragma unroll
      for (int q = 0; q < kStRows; ++q) {
        const int r = r0 + wave * kStRows + q;
        if (r >= a.ny) continue;
        const int64_t i = (int64_t)r * a.nx + c;
        const T v = stencil_sum<T>(a, r, c, [&](int rr, int cc) { return tile[rr - r0 + 1][cc - c0 + 1]; });
        const T pass = a.form == MFX_STENCIL_HEAT ? T(0) : rk_combine_at<T>(k, base, rows, row_stride, m + i);
        if (WRITE_Y) {
          yout[i] = tile[r - r0 + 1][lane + 1];
          if (a.form != MFX_STENCIL_HEAT) yout[m + i] = pass;
        }
        stencil_emit<T>(a, v, pass, kout, i, m);
      }
    }
    __syncthreads();
  }
}

}  // namespace mfx
