// libmfx: fixed-step explicit Runge-Kutta solves of y' = A y with their discrete and continuous (backsolve) adjoints -- the
// baselines of the reference's PDE work-precision study (util/pde_util.py:177-237) as native drivers.
//
//   Y_i = y + dt sum_{j<i} a_ij K_j,   K_i = A Y_i,   y+ = y + dt sum_i b_i K_i
//
// One kernel, k_rk_combine: out = c0 base + sum_j c_j V_j over up to 16 rows of a panel, the coefficients kernel arguments, zero
// coefficients skipped through a wave-uniform mask; it forms the stage values, the update, the adjoint's Kbar_i, the scaled L rows
// and the lambda accumulation.  (k_update of mfx_vec.h, behind mfx_basis_combine, reads its coefficients from device memory through an
// LDS prologue and has no factor on its base term: serving host coefficients through it would add an upload per launch, so the
// body is not shared; the thread-owned loads and stores are.)  The operator is applied through op_apply only.  A stage kernel that
// fuses the combination into the stencil apply was measured and is slower or within the noise: tools/experiments/rk_fused_stage,
// DESIGN.md section 3.4b.  No atomics anywhere.
//
// mfx_rk_solve_adaptive runs the same scheme on an embedded pair with the step size on the device: a
// control block in the workspace, k_rk_combine_dev (k_rk_combine with h read from the block), k_rk_err_partials, k_rk_control and
// k_rk_commit; the host polls the block once per chunk of attempts.
#include <math.h>

#include "mfx_vec.h"

namespace mfx {

constexpr int kRkBaseBit = MFX_RK_MAX_STAGES;  // bit of RkCoef::mask that says "the base term is present"

template <typename T>
struct RkCoef {
  unsigned mask;  // bit j < 16: c[j] != 0; bit 16: c0 != 0
  T c0;
  T c[MFX_RK_MAX_STAGES];
};

// the two steps of one element of a combination, in the order base, row 0, row 1, ...
template <typename T>
__device__ __forceinline__ T rk_scale(T c0, T base) {
  return c0 * base;
}
template <typename T>
__device__ __forceinline__ T rk_axpy(T c, T v, T acc) {
  return fma(c, v, acc);
}

// out[b] = c0 base[b] + sum_j c_j rows[b][j]: grid = (slices, p), EPT elements per thread held in registers across the rows.
// out may be base (every thread reads its own elements before it writes them).
template <typename T, int VEC, int EPT>
__global__ __launch_bounds__(kBlock) void k_rk_combine(RkCoef<T> k, const T* base, int64_t ldbase, const T* __restrict__ rows,
                                                       int64_t rows_ldb, int64_t row_stride, T* out, int64_t ldout, int64_t n) {
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int64_t slice0 = (int64_t)blockIdx.x * ((int64_t)blockDim.x * EPT);
  T acc[EPT];
  if (k.mask >> kRkBaseBit & 1u) {
    load_own<T, VEC>(acc, base + b * ldbase, slice0, n, tid);
#pragma unroll
    for (int e = 0; e < EPT; ++e) acc[e] = rk_scale<T>(k.c0, acc[e]);
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e) acc[e] = T(0);
  }
  const T* rb = rows + b * rows_ldb;
#pragma unroll
  for (int j = 0; j < MFX_RK_MAX_STAGES; ++j) {
    if (k.mask >> j & 1u) {
      T v[EPT];
      load_own<T, VEC>(v, rb + (int64_t)j * row_stride, slice0, n, tid);
#pragma unroll
      for (int e = 0; e < EPT; ++e) acc[e] = rk_axpy<T>(k.c[j], v[e], acc[e]);
    }
  }
  store_own<T, VEC>(acc, out + b * ldout, slice0, n, tid);
}

// ------------------------------------------------------------------------------------------------
// adaptive steps (mfx_rk_solve_adaptive): the step size lives on the device
// ------------------------------------------------------------------------------------------------
// The control block, at the start of the workspace.  h is the step of the attempt in flight (already clipped to t1 - t), h_abs the
// controller's unclipped proposal; `commit` and `row` are what k_rk_control hands to k_rk_commit.
struct RkCtl {
  double t, t_new, h, h_abs, t1;
  int64_t n_accepted, n_rejected, n_attempts, max_attempts, row;
  int32_t done, status, rejected, commit;
};

// the tableau numbers of one combination; the kernel multiplies them by the block's h.  mask as RkCoef::mask (c0 = 1 when present)
struct RkCoefDev {
  unsigned mask;
  double a[MFX_RK_MAX_STAGES];
};

// What every attempt starts with (scipy's _step_impl): refuse a proposal below 10 ulp(t), clip to t1, take h as the difference.
__device__ __forceinline__ void rk_ctl_propose(RkCtl* c) {
  const double t = c->t;
  if (c->h_abs < 10.0 * (nextafter(t, INFINITY) - t)) {
    c->status = MFX_RK_STEP_TOO_SMALL;
    c->done = 1;
    return;
  }
  double t_new = t + c->h_abs;
  if (t_new > c->t1) t_new = c->t1;
  c->t_new = t_new;
  c->h = t_new - t;
}

__global__ void k_rk_ctl_init(RkCtl* c, double t0, double t1, double dt0, int64_t max_attempts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  c->t = t0, c->t_new = t0, c->h = 0.0, c->h_abs = dt0, c->t1 = t1;
  c->n_accepted = c->n_rejected = c->n_attempts = 0;
  c->max_attempts = max_attempts;
  c->row = 0;
  c->done = 0, c->status = MFX_RK_OK, c->rejected = 0, c->commit = 0;
  rk_ctl_propose(c);
}

// k_rk_combine with c_j = T(h a_j), the fp64 product rounded once as rk_coef rounds the host's: the same bits as k_rk_combine
// launched with the step size the block holds.  Returns at once when the solve is over.
template <typename T, int VEC, int EPT>
__global__ __launch_bounds__(kBlock) void k_rk_combine_dev(const RkCtl* __restrict__ ctl, RkCoefDev k, const T* base, int64_t ldbase,
                                                           const T* __restrict__ rows, int64_t rows_ldb, int64_t row_stride, T* out,
                                                           int64_t ldout, int64_t n) {
  if (ctl->done) return;
  const double h = ctl->h;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int64_t slice0 = (int64_t)blockIdx.x * ((int64_t)blockDim.x * EPT);
  T acc[EPT];
  if (k.mask >> kRkBaseBit & 1u) {
    load_own<T, VEC>(acc, base + b * ldbase, slice0, n, tid);
#pragma unroll
    for (int e = 0; e < EPT; ++e) acc[e] = rk_scale<T>(T(1), acc[e]);
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e) acc[e] = T(0);
  }
  const T* rb = rows + b * rows_ldb;
#pragma unroll
  for (int j = 0; j < MFX_RK_MAX_STAGES; ++j) {
    const double cj = h * k.a[j];
    if ((k.mask >> j & 1u) && cj != 0.0) {
      T v[EPT];
      load_own<T, VEC>(v, rb + (int64_t)j * row_stride, slice0, n, tid);
#pragma unroll
      for (int e = 0; e < EPT; ++e) acc[e] = rk_axpy<T>((T)cj, v[e], acc[e]);
    }
  }
  store_own<T, VEC>(acc, out + b * ldout, slice0, n, tid);
}

// partial[b][blk] = sum over the block's elements of (err_i / scale_i)^2 in fp64, err = h sum_j e_j K_j over the rows with e_j != 0,
// scale_i = atol + rtol max(|y_i|, |y+_i|): one pass over y, y+ and those rows.  Fixed order inside the block, no atomics.
template <typename T, int VEC, int EPT>
__global__ __launch_bounds__(kBlock) void k_rk_err_partials(const RkCtl* __restrict__ ctl, RkCoefDev k, const T* __restrict__ y,
                                                            const T* __restrict__ ynew, int64_t ldy, const T* __restrict__ rows,
                                                            int64_t rows_ldb, int64_t row_stride, double rtol, double atol, int64_t n,
                                                            double* __restrict__ partial, int nblk) {
  __shared__ double sm[kBlock / 64];
  if (ctl->done) return;
  const double h = ctl->h;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t b = blockIdx.y;
  const int64_t slice0 = (int64_t)blockIdx.x * ((int64_t)blockDim.x * EPT);
  double err[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) err[e] = 0.0;
  const T* rb = rows + b * rows_ldb;
#pragma unroll
  for (int j = 0; j < MFX_RK_MAX_STAGES; ++j) {
    if (k.mask >> j & 1u) {
      const double cj = h * k.a[j];
      T v[EPT];
      load_own<T, VEC>(v, rb + (int64_t)j * row_stride, slice0, n, tid);
#pragma unroll
      for (int e = 0; e < EPT; ++e) err[e] = fma(cj, (double)v[e], err[e]);
    }
  }
  T ya[EPT], yb[EPT];
  load_own<T, VEC>(ya, y + b * ldy, slice0, n, tid);
  load_own<T, VEC>(yb, ynew + b * ldy, slice0, n, tid);
  double sum = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int64_t off = slice0 + (int64_t)((e / VEC) * (int)blockDim.x + tid) * VEC + (e % VEC);
    if (off < n) {  // an element past the end has no scale (atol may be 0)
      const double r = err[e] / (atol + rtol * fmax(fabs((double)ya[e]), fabs((double)yb[e])));
      sum = fma(r, r, sum);
    }
  }
  sum = wave_sum(sum);
  if (lane == 0) sm[wid] = sum;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += sm[w];
    partial[b * (int64_t)nblk + blockIdx.x] = tot;
  }
}

// One workgroup: the per-state sums of the partials in a fixed order (a wave per state, lanes strided over the blocks), their
// maximum, then thread 0 applies the controller to the block and appends the step size of an accepted attempt to dts.
__global__ __launch_bounds__(kBlock) void k_rk_control(RkCtl* ctl, const double* __restrict__ partial, int nblk, int64_t p, int64_t n,
                                                       double expo, double* __restrict__ dts, int64_t max_steps) {
  __shared__ double smax[kBlock / 64];
  __shared__ int sbad[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (ctl->done) {  // nothing reads `commit` before this kernel of the next attempt
    if (tid == 0) ctl->commit = 0;
    return;
  }
  double vmax = 0.0;
  int bad = 0;
  for (int64_t b = wid; b < p; b += kBlock / 64) {
    double s = 0.0;
    for (int q = lane; q < nblk; q += 64) s += partial[b * (int64_t)nblk + q];
    s = wave_sum_all(s);
    if (!isfinite(s)) bad = 1;
    else if (s > vmax) vmax = s;
  }
  if (lane == 0) smax[wid] = vmax, sbad[wid] = bad;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 0; w < kBlock / 64; ++w) {
    bad |= sbad[w];
    if (smax[w] > vmax) vmax = smax[w];
  }
  RkCtl c = *ctl;
  c.n_attempts += 1;
  c.commit = 0;
  if (bad) {
    c.status = MFX_RK_NONFINITE;
    c.done = 1;
    *ctl = c;
    return;
  }
  const double norm = sqrt(vmax / (double)n);
  if (norm < 1.0) {
    double factor = norm == 0.0 ? 10.0 : fmin(10.0, 0.9 * pow(norm, expo));
    if (c.rejected) factor = fmin(1.0, factor);
    dts[c.n_accepted] = c.h;
    c.n_accepted += 1;
    c.row = c.n_accepted;
    c.commit = 1;
    c.rejected = 0;
    c.t = c.t_new;
    c.h_abs = c.h * factor;
    if (c.t >= c.t1) c.done = 1;  // status stays MFX_RK_OK
  } else {
    c.h_abs = c.h * fmax(0.2, 0.9 * pow(norm, expo));
    c.rejected = 1;
    c.n_rejected += 1;
  }
  if (!c.done) {
    if (c.n_attempts >= c.max_attempts || c.n_accepted >= max_steps) {
      c.status = MFX_RK_MAX_ATTEMPTS;
      c.done = 1;
    } else {
      rk_ctl_propose(&c);
    }
  }
  *ctl = c;
}

// an accepted attempt: y <- y+, and row `row` of the kept iterates
template <typename T, int VEC, int EPT>
__global__ __launch_bounds__(kBlock) void k_rk_commit(const RkCtl* __restrict__ ctl, const T* __restrict__ ynew, T* __restrict__ y,
                                                      int64_t ldy, T* __restrict__ ys, int64_t ldys, int64_t n) {
  if (!ctl->commit) return;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int64_t slice0 = (int64_t)blockIdx.x * ((int64_t)blockDim.x * EPT);
  T v[EPT];
  load_own<T, VEC>(v, ynew + b * ldy, slice0, n, tid);
  store_own<T, VEC>(v, y + b * ldy, slice0, n, tid);
  if (ys) store_own<T, VEC>(v, ys + b * ldys + ctl->row * n, slice0, n, tid);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct RkGeom {  // what MFX_VEC_EPT_SWITCH reads
  int vec, ept, wg, nblk;
};

template <typename T>
struct RkCtx {
  const mfx_operator* op;
  const mfx_rk_tableau* tab;
  int64_t n, p;
  int s;
  void* opws;
  int64_t opws_bytes;
  hipStream_t stream;
};

template <typename T>
static RkCoef<T> rk_coef(double c0, bool has_base, const double* coef, int nrows) {
  RkCoef<T> k{};
  k.c0 = (T)c0;
  if (has_base && c0 != 0.0) k.mask |= 1u << kRkBaseBit;
  for (int j = 0; j < nrows; ++j) {
    k.c[j] = (T)coef[j];
    if (coef[j] != 0.0) k.mask |= 1u << j;
  }
  return k;
}

// launch geometry of a pass over (p, n) vectors and panel rows: 16-byte access when every pointer, leading dimension and the row
// stride allow it; Ctx::fine slicing when the coarse one leaves most CUs idle
template <typename T>
static RkGeom rk_geom(int64_t n, int64_t p, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds, int64_t row_stride) {
  constexpr int V = VecWidth<T>::value;
  RkGeom g;
  g.vec = pick_vec<T>(n, ptrs);
  if (p > 1)
    for (int64_t ld : lds)
      if (ld % V) g.vec = 1;
  if (row_stride % V) g.vec = 1;
  g.wg = pick_wg(n, p);
  g.ept = kEpt;
  g.nblk = (int)((n + (int64_t)g.wg * kEpt - 1) / ((int64_t)g.wg * kEpt));
  if (g.vec > 1 && g.wg == kBlock && (int64_t)g.nblk * p < 128) {  // Ctx::fine: one 16-byte load per thread and row
    g.ept = V;
    g.nblk = (int)((n + (int64_t)g.wg * V - 1) / ((int64_t)g.wg * V));
  }
  return g;
}

// out = c0 base + sum_{j < nrows} coef[j] rows[:, j, :]   (base NULL: no base term; nrows 0: no rows)
template <typename T>
static int rk_combine(const RkCtx<T>& c, double c0, const T* base, int64_t ldbase, const double* coef, int nrows, const T* rows,
                      int64_t rows_ldb, int64_t row_stride, T* out, int64_t ldout) {
  const RkCoef<T> k = rk_coef<T>(c0, base != nullptr, coef, nrows);
  const RkGeom g = rk_geom<T>(c.n, c.p, {base, rows, out}, {ldbase, rows_ldb, ldout}, row_stride);
  const dim3 grid((unsigned)g.nblk, (unsigned)c.p);
  if (!base) base = out;  // never read (the base bit is clear)
  if (!rows) rows = out;  // never read (no row bit is set)
  MFX_VEC_EPT_SWITCH(g, (k_rk_combine<T, VEC, EPT><<<grid, g.wg, 0, c.stream>>>(k, base, ldbase, rows, rows_ldb, row_stride, out, ldout, c.n)));
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

// stage i of a step of size h from `base`: K[:, i, :] = A (base + h sum_{j<i} a_ij K[:, j, :]); the stage value goes to yrow when
// that is asked for, else to ytmp
template <typename T>
static int rk_stage(const RkCtx<T>& c, int i, double h, const T* base, int64_t ldbase, T* K, T* yrow, int64_t ldyrow, T* ytmp) {
  const int64_t ldk = (int64_t)c.s * c.n;
  double coef[MFX_RK_MAX_STAGES] = {};
  bool any = false;
  for (int j = 0; j < i; ++j) {
    coef[j] = h * c.tab->a[i][j];
    any = any || coef[j] != 0.0;
  }
  T* Ki = K + (int64_t)i * c.n;
  const T* x = base;
  int64_t ldx = ldbase;
  if (any || yrow) {  // Y_1 = y needs no combination unless the stage value itself is wanted
    T* dst = yrow ? yrow : ytmp;
    const int64_t lddst = yrow ? ldyrow : c.n;
    MFX_TRY(rk_combine<T>(c, 1.0, base, ldbase, coef, i, K, ldk, c.n, dst, lddst));
    x = dst;
    ldx = lddst;
  }
  return op_apply(c.op, 0, x, ldx, nullptr, 0, Ki, ldk, c.p, c.opws, c.opws_bytes, c.stream);
}

// the update of a step of size h: out = base + h sum_i b_i K[:, i, :]
template <typename T>
static int rk_advance(const RkCtx<T>& c, double h, const T* base, int64_t ldbase, const T* K, T* out, int64_t ldout) {
  double coef[MFX_RK_MAX_STAGES] = {};
  for (int i = 0; i < c.s; ++i) coef[i] = h * c.tab->b[i];
  return rk_combine<T>(c, 1.0, base, ldbase, coef, c.s, K, (int64_t)c.s * c.n, c.n, out, ldout);
}

struct RkWs {
  void *y, *ytmp, *lam, *K, *Y, *Kbar, *Ybar, *opws;  // Kbar / Ybar: the backsolve's lambda stages and their images under A^T
  int64_t opws_bytes;
};

// mode 0: solve, 1: discrete adjoint, 2: backsolve
static int64_t rk_carve(const mfx_operator* op, int s, int64_t n, int64_t p, int mode, void* ws, int64_t ws_bytes, RkWs* out) {
  const int64_t es = (int64_t)dtype_size(op->dtype), vec = p * n * es, panel = p * s * n * es;
  Carver cv(ws, ws_bytes);
  RkWs w{};
  if (mode != 1) w.y = cv.take(vec);
  w.ytmp = cv.take(vec);
  if (mode != 0) w.lam = cv.take(vec);
  w.K = cv.take(panel);
  if (mode != 0) {
    w.Y = cv.take(panel);
    w.Kbar = cv.take(panel);
    w.Ybar = cv.take(panel);
  }
  w.opws_bytes = op_workspace_bytes(op, mode == 0 ? 1 : p * s, p);
  w.opws = cv.take(w.opws_bytes);
  if (out) *out = w;
  return cv.off;
}

template <typename T>
static int rk_solve_t(const RkCtx<T>& c, const double* dts, int64_t nsteps, const T* y0, int64_t ldy0, T* y1, int64_t ldy1, T* ys,
                      const RkWs& w) {
  const int64_t n = c.n, ldys = (nsteps + 1) * n;
  if (ys) MFX_TRY(copy_rows_async(ys, ldys * sizeof(T), y0, ldy0 * sizeof(T), n * sizeof(T), c.p, c.stream));
  for (int64_t step = 0; step < nsteps; ++step) {
    const T* cur;
    T* nxt;
    int64_t ldcur, ldnxt;
    if (ys) {
      cur = ys + step * n, nxt = ys + (step + 1) * n, ldcur = ldnxt = ldys;
    } else {
      cur = step == 0 ? y0 : (const T*)w.y, ldcur = step == 0 ? ldy0 : n;
      nxt = step == nsteps - 1 ? y1 : (T*)w.y, ldnxt = step == nsteps - 1 ? ldy1 : n;
    }
    for (int i = 0; i < c.s; ++i) MFX_TRY(rk_stage<T>(c, i, dts[step], cur, ldcur, (T*)w.K, nullptr, 0, (T*)w.ytmp));
    MFX_TRY(rk_advance<T>(c, dts[step], cur, ldcur, (const T*)w.K, nxt, ldnxt));
  }
  if (ys) MFX_TRY(copy_rows_async(y1, ldy1 * sizeof(T), ys + nsteps * n, ldys * sizeof(T), n * sizeof(T), c.p, c.stream));
  return MFX_OK;
}

template <typename T>
static int rk_adjoint_t(const RkCtx<T>& c, const double* dts, int64_t nsteps, const T* ys, const T* dy1, int64_t lddy1, T* dy0,
                        int64_t lddy0, const mfx_op_grads* grads, const RkWs& w) {
  const int64_t n = c.n, ldys = (nsteps + 1) * n, ldp = (int64_t)c.s * n;
  const int s = c.s;
  const bool native = op_kind(c.op)->native;
  T *lam = (T*)w.lam, *K = (T*)w.K, *Y = (T*)w.Y, *Kbar = (T*)w.Kbar, *Ybar = (T*)w.Ybar;
  MFX_TRY(copy_rows_async(lam, n * sizeof(T), dy1, lddy1 * sizeof(T), n * sizeof(T), c.p, c.stream));
  double ones[MFX_RK_MAX_STAGES];
  for (int i = 0; i < MFX_RK_MAX_STAGES; ++i) ones[i] = 1.0;
  for (int64_t step = nsteps - 1; step >= 0; --step) {
    const double dt = dts[step];
    const T* cur = ys + step * n;
    for (int i = 0; i < s; ++i) MFX_TRY(rk_stage<T>(c, i, dt, cur, ldys, K, Y + (int64_t)i * n, ldp, (T*)w.ytmp));
    for (int i = s - 1; i >= 0; --i) {
      double coef[MFX_RK_MAX_STAGES] = {};
      for (int j = i + 1; j < s; ++j) coef[j] = dt * c.tab->a[j][i];
      MFX_TRY(rk_combine<T>(c, dt * c.tab->b[i], lam, n, coef, s, Ybar, ldp, n, Kbar + (int64_t)i * n, ldp));
      MFX_TRY(op_apply(c.op, 1, Kbar + (int64_t)i * n, ldp, Y + (int64_t)i * n, ldp, Ybar + (int64_t)i * n, ldp, c.p, c.opws, c.opws_bytes,
                       c.stream));
    }
    if (native && grads) MFX_TRY(op_vjp_params(c.op, Kbar, n, Y, n, c.p * s, grads, c.opws, c.opws_bytes, c.stream));
    if (step > 0) {
      MFX_TRY(rk_combine<T>(c, 1.0, lam, n, ones, s, Ybar, ldp, n, lam, n));
    } else if (dy0) {
      MFX_TRY(rk_combine<T>(c, 1.0, lam, n, ones, s, Ybar, ldp, n, dy0, lddy0));
    }
  }
  return MFX_OK;
}

template <typename T>
static int rk_backsolve_t(const RkCtx<T>& c, const double* dts, int64_t nsteps, const T* y1, int64_t ldy1, const T* dy1, int64_t lddy1,
                          T* dy0, int64_t lddy0, const mfx_op_grads* grads, const RkWs& w) {
  const int64_t n = c.n, ldp = (int64_t)c.s * n;
  const int s = c.s;
  const bool native = op_kind(c.op)->native;
  T *y = (T*)w.y, *lam = (T*)w.lam, *Ky = (T*)w.K, *Y = (T*)w.Y, *Lam = (T*)w.Kbar, *Kl = (T*)w.Ybar, *tmp = (T*)w.ytmp;
  MFX_TRY(copy_rows_async(y, n * sizeof(T), y1, ldy1 * sizeof(T), n * sizeof(T), c.p, c.stream));
  MFX_TRY(copy_rows_async(lam, n * sizeof(T), dy1, lddy1 * sizeof(T), n * sizeof(T), c.p, c.stream));
  for (int64_t step = nsteps - 1; step >= 0; --step) {
    const double dt = dts[step], h = -dt;
    for (int i = 0; i < s; ++i) MFX_TRY(rk_stage<T>(c, i, h, y, n, Ky, Y + (int64_t)i * n, ldp, tmp));
    // lam' = -A^T lam with step h: Lam_i = lam + dt sum_{j<i} a_ij (A^T Lam_j), lam+ = lam + dt sum_i b_i (A^T Lam_i)
    for (int i = 0; i < s; ++i) {
      double coef[MFX_RK_MAX_STAGES] = {};
      for (int j = 0; j < i; ++j) coef[j] = dt * c.tab->a[i][j];
      T* Li = Lam + (int64_t)i * n;
      MFX_TRY(rk_combine<T>(c, 1.0, lam, n, coef, i, Kl, ldp, n, Li, ldp));
      const T* aux = Y + (int64_t)i * n;
      int64_t ldaux = ldp;
      if (!native) {  // a callback accumulates x^T dA aux inside the application: the quadrature weight -h b_i goes onto aux
        MFX_TRY(rk_combine<T>(c, dt * c.tab->b[i], aux, ldp, nullptr, 0, nullptr, 0, 0, tmp, n));
        aux = tmp;
        ldaux = n;
      }
      MFX_TRY(op_apply(c.op, 1, Li, ldp, aux, ldaux, Kl + (int64_t)i * n, ldp, c.p, c.opws, c.opws_bytes, c.stream));
    }
    if (native && grads) {  // thetabar += sum_i (-h b_i Lam_i)^T dA Y_i
      for (int i = 0; i < s; ++i) {
        T* Li = Lam + (int64_t)i * n;
        MFX_TRY(rk_combine<T>(c, dt * c.tab->b[i], Li, ldp, nullptr, 0, nullptr, 0, 0, Li, ldp));
      }
      MFX_TRY(op_vjp_params(c.op, Lam, n, Y, n, c.p * s, grads, c.opws, c.opws_bytes, c.stream));
    }
    MFX_TRY(rk_advance<T>(c, h, y, n, Ky, y, n));
    if (step > 0) {
      MFX_TRY(rk_advance<T>(c, dt, lam, n, Kl, lam, n));
    } else if (dy0) {
      MFX_TRY(rk_advance<T>(c, dt, lam, n, Kl, dy0, lddy0));
    }
  }
  return MFX_OK;
}

static int rk_check_tableau(const mfx_rk_tableau* tab) {
  MFX_REQUIRE(tab != nullptr, MFX_ERR_INVALID, "Runge-Kutta tableau is NULL");
  MFX_REQUIRE(tab->stages >= 1 && tab->stages <= MFX_RK_MAX_STAGES, MFX_ERR_INVALID, "Runge-Kutta tableau: %d stages, 1..%d expected",
              tab->stages, MFX_RK_MAX_STAGES);
  for (int i = 0; i < tab->stages; ++i) {
    MFX_REQUIRE(std::isfinite(tab->b[i]), MFX_ERR_INVALID, "Runge-Kutta tableau: b[%d] is not finite", i);
    for (int j = 0; j < tab->stages; ++j) {
      MFX_REQUIRE(std::isfinite(tab->a[i][j]), MFX_ERR_INVALID, "Runge-Kutta tableau: a[%d][%d] is not finite", i, j);
      MFX_REQUIRE(j < i || tab->a[i][j] == 0.0, MFX_ERR_INVALID,
                  "Runge-Kutta tableau: a[%d][%d] = %g on or above the diagonal (explicit methods only)", i, j, tab->a[i][j]);
    }
  }
  return MFX_OK;
}

// every refusal that the three drivers share, in the order of include/mfx.h
static int rk_check(const mfx_operator* op, const mfx_rk_tableau* tab, const double* dts, int64_t nsteps, int64_t n, int64_t p,
                    const mfx_op_grads* grads, int flags) {
  MFX_TRY(check_op(op));
  MFX_REQUIRE(op->nrows == 0, MFX_ERR_UNSUPPORTED, "the Runge-Kutta drivers take the whole operator (nrows = 0): there is no row-sharded form");
  MFX_TRY(rk_check_tableau(tab));
  MFX_REQUIRE(nsteps >= 1, MFX_ERR_INVALID, "nsteps = %lld must be at least 1", (long long)nsteps);
  MFX_REQUIRE(p >= 1, MFX_ERR_INVALID, "p = %lld must be at least 1", (long long)p);
  MFX_REQUIRE(n >= 1 && op->n == n, MFX_ERR_INVALID, "operator size %lld != n = %lld", (long long)op->n, (long long)n);
  MFX_REQUIRE(p <= 65535, MFX_ERR_UNSUPPORTED, "p = %lld exceeds the grid limit 65535", (long long)p);
  MFX_REQUIRE(dts != nullptr, MFX_ERR_INVALID, "dts is NULL");
  for (int64_t i = 0; i < nsteps; ++i) MFX_REQUIRE(std::isfinite(dts[i]), MFX_ERR_INVALID, "dts[%lld] is not finite", (long long)i);
  MFX_REQUIRE(flags == 0, MFX_ERR_INVALID, "unknown flag bits 0x%x (no flag is defined)", flags);
  if (grads) {
    MFX_REQUIRE(grads->x == nullptr, MFX_ERR_UNSUPPORTED,
                "the Runge-Kutta adjoints do not sweep the input gradient of a kernel-Gram operator (grads->x)");
    MFX_TRY(check_op_grads(op, grads, false));
  }
  return MFX_OK;
}

// the drivers' common key (depth = the number of steps) and what a captured solve depends on beyond it
static GraphKey rk_key(DriverId id, const mfx_operator* op, const mfx_rk_tableau* tab, const double* dts, int64_t nsteps, int64_t n,
                       int64_t p, const mfx_op_grads* grads, int flags, const void* ws, int64_t ws_bytes, const void* stream) {
  GraphKey key = driver_key(id, op, n, nsteps, p, grads, ws, ws_bytes, stream);
  key.add(flags).add(tab->stages);
  for (int i = 0; i < tab->stages; ++i) {
    key.add(tab->b[i]);
    for (int j = 0; j < i; ++j) key.add(tab->a[i][j]);
  }
  for (int64_t i = 0; i < nsteps; ++i) key.add(dts[i]);  // a step size is baked into the kernel arguments of its launches
  return key;
}

// What a Runge-Kutta entry point holds once nothing is left to refuse.  mode: see rk_carve
struct RkCall { RkWs ws; hipStream_t stream; };
static int rk_prologue(const char* fn, const mfx_operator* op, const mfx_rk_tableau* tab, int64_t n, int64_t p, int mode, void* ws,
                       int64_t ws_bytes, void* stream, RkCall* call) {
  const int64_t need = rk_carve(op, tab->stages, n, p, mode, ws, ws_bytes, &call->ws);
  MFX_REQUIRE(ws && need <= ws_bytes, MFX_ERR_WORKSPACE, "%s: workspace too small: %lld bytes given, %lld needed", fn,
              (long long)ws_bytes, (long long)need);
  call->stream = static_cast<hipStream_t>(stream);
  return MFX_OK;
}

template <typename T>
static RkCtx<T> rk_ctx(const mfx_operator* op, const mfx_rk_tableau* tab, int64_t n, int64_t p, const RkWs& w, hipStream_t st) {
  RkCtx<T> c;
  c.op = op, c.tab = tab, c.n = n, c.p = p, c.s = tab->stages;
  c.opws = w.opws, c.opws_bytes = w.opws_bytes, c.stream = st;
  return c;
}

// ---- adaptive steps ------------------------------------------------------------------------------------------------------------------
struct RkAdaptiveWs {
  RkCtl* ctl;
  double *dts, *partial;
  void *y, *ynew, *ytmp, *K, *opws;
  int64_t opws_bytes;
};

// an upper bound of rk_geom's nblk: 512 elements per workgroup is the finest slicing it picks
static int64_t rk_partial_slots(int64_t n) { return (n + 511) / 512; }

static int64_t rk_adaptive_carve(const mfx_operator* op, int s, int64_t n, int64_t p, int64_t max_steps, void* ws, int64_t ws_bytes,
                                 RkAdaptiveWs* out) {
  const int64_t es = (int64_t)dtype_size(op->dtype), vec = p * n * es;
  Carver cv(ws, ws_bytes);
  RkAdaptiveWs w{};
  w.ctl = static_cast<RkCtl*>(cv.take((int64_t)sizeof(RkCtl)));
  w.dts = static_cast<double*>(cv.take(max_steps * (int64_t)sizeof(double)));
  w.partial = static_cast<double*>(cv.take(p * rk_partial_slots(n) * (int64_t)sizeof(double)));
  w.y = cv.take(vec);
  w.ynew = cv.take(vec);
  w.ytmp = cv.take(vec);
  w.K = cv.take(vec * s);
  w.opws_bytes = op_workspace_bytes(op, 1, p);
  w.opws = cv.take(w.opws_bytes);
  if (out) *out = w;
  return cv.off;
}

static RkCoefDev rk_coef_dev(bool has_base, const double* coef, int nrows) {
  RkCoefDev k{};
  if (has_base) k.mask |= 1u << kRkBaseBit;
  for (int j = 0; j < nrows; ++j) {
    k.a[j] = coef[j];
    if (coef[j] != 0.0) k.mask |= 1u << j;
  }
  return k;
}

// out = base + h sum_{j < nrows} coef[j] K[:, j, :] with the block's h; every vector is a (p, n) workspace buffer
template <typename T>
static int rk_combine_dev(const RkCtx<T>& c, const RkCtl* ctl, const double* coef, int nrows, const T* base, const T* K, T* out) {
  const int64_t ldk = (int64_t)c.s * c.n;
  const RkCoefDev k = rk_coef_dev(true, coef, nrows);
  const RkGeom g = rk_geom<T>(c.n, c.p, {base, K, out}, {c.n, ldk, c.n}, c.n);
  const dim3 grid((unsigned)g.nblk, (unsigned)c.p);
  MFX_VEC_EPT_SWITCH(g, (k_rk_combine_dev<T, VEC, EPT><<<grid, g.wg, 0, c.stream>>>(ctl, k, base, c.n, K, ldk, c.n, out, c.n, c.n)));
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

// ONE attempt: the stages and the update of rk_solve_t's step with the block's h, the error partials, the controller, the commit
template <typename T>
static int rk_attempt(const RkCtx<T>& c, const mfx_rk_pair* pair, double rtol, double atol, int64_t max_steps, T* ys, const RkAdaptiveWs& w) {
  const int64_t n = c.n, ldk = (int64_t)c.s * n;
  T *y = (T*)w.y, *ynew = (T*)w.ynew, *ytmp = (T*)w.ytmp, *K = (T*)w.K;
  for (int i = 0; i < c.s; ++i) {
    bool any = false;
    for (int j = 0; j < i; ++j) any = any || c.tab->a[i][j] != 0.0;
    const T* x = y;
    if (any) {  // as rk_stage: Y_i = y needs no combination
      MFX_TRY(rk_combine_dev<T>(c, w.ctl, c.tab->a[i], i, y, K, ytmp));
      x = ytmp;
    }
    MFX_TRY(op_apply(c.op, 0, x, n, nullptr, 0, K + (int64_t)i * n, ldk, c.p, c.opws, c.opws_bytes, c.stream));
  }
  MFX_TRY(rk_combine_dev<T>(c, w.ctl, c.tab->b, c.s, y, K, ynew));
  const RkCoefDev ke = rk_coef_dev(false, pair->e, c.s);
  const RkGeom g = rk_geom<T>(n, c.p, {y, ynew, K}, {n, ldk}, n);
  MFX_REQUIRE(g.nblk <= rk_partial_slots(n), MFX_ERR_INVALID, "mfx_rk_solve_adaptive: %d slices exceed the partial sums' %lld slots", g.nblk,
              (long long)rk_partial_slots(n));
  const dim3 grid((unsigned)g.nblk, (unsigned)c.p);
  MFX_VEC_EPT_SWITCH(g, (k_rk_err_partials<T, VEC, EPT><<<grid, g.wg, 0, c.stream>>>(w.ctl, ke, y, ynew, n, K, ldk, n, rtol, atol, n, w.partial,
                                                                                   g.nblk)));
  MFX_CHECK_LAUNCH();
  k_rk_control<<<1, kBlock, 0, c.stream>>>(w.ctl, w.partial, g.nblk, c.p, n, -1.0 / (double)pair->order, w.dts, max_steps);
  MFX_CHECK_LAUNCH();
  const int64_t ldys = (max_steps + 1) * n;
  const RkGeom gc = rk_geom<T>(n, c.p, {y, ynew, ys}, {n, ldys}, n);
  MFX_VEC_EPT_SWITCH(gc, (k_rk_commit<T, VEC, EPT><<<dim3((unsigned)gc.nblk, (unsigned)c.p), gc.wg, 0, c.stream>>>(w.ctl, ynew, y, n, ys, ldys, n)));
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

static const char* rk_status_text(int status) {
  switch (status) {
    case MFX_RK_OK: return "ok";
    case MFX_RK_MAX_ATTEMPTS: return "max_attempts exhausted before t1";
    case MFX_RK_STEP_TOO_SMALL: return "step size below 10 ulp(t)";
    case MFX_RK_NONFINITE: return "non-finite error norm";
  }
  return "unknown status";
}

static int rk_check_adaptive(const mfx_operator* op, const mfx_rk_pair* pair, double t0, double t1, double dt0, double rtol, double atol,
                             int64_t max_steps, int64_t max_attempts, int64_t chunk, int64_t n, int64_t p, int flags) {
  MFX_REQUIRE(pair != nullptr, MFX_ERR_INVALID, "Runge-Kutta pair is NULL");
  MFX_TRY(rk_check(op, &pair->tab, &dt0, 1, n, p, nullptr, flags));
  for (int i = 0; i < pair->tab.stages; ++i) MFX_REQUIRE(std::isfinite(pair->e[i]), MFX_ERR_INVALID, "Runge-Kutta pair: e[%d] is not finite", i);
  MFX_REQUIRE(pair->order >= 1, MFX_ERR_INVALID, "Runge-Kutta pair: order = %d must be at least 1", pair->order);
  MFX_REQUIRE(rtol >= 0.0 && atol >= 0.0 && std::isfinite(rtol + atol) && rtol + atol > 0.0, MFX_ERR_INVALID,
              "rtol = %g, atol = %g: both must be non-negative and their sum finite and positive", rtol, atol);
  MFX_REQUIRE(dt0 > 0.0, MFX_ERR_INVALID, "dt0 = %g must be positive", dt0);
  MFX_REQUIRE(std::isfinite(t0) && std::isfinite(t1) && t1 > t0, MFX_ERR_INVALID, "t1 = %g must be finite and greater than t0 = %g", t1, t0);
  MFX_REQUIRE(max_steps >= 1, MFX_ERR_INVALID, "max_steps = %lld must be at least 1", (long long)max_steps);
  MFX_REQUIRE(max_attempts >= 1, MFX_ERR_INVALID, "max_attempts = %lld must be at least 1", (long long)max_attempts);
  MFX_REQUIRE(chunk >= 1, MFX_ERR_INVALID, "chunk = %lld must be at least 1", (long long)chunk);
  return MFX_OK;
}

}  // namespace mfx

using namespace mfx;

extern "C" {

int64_t mfx_rk_workspace_bytes(const mfx_operator* op, const mfx_rk_tableau* tab, int64_t n, int64_t p, int adjoint) {
  if (!op || adjoint < 0 || adjoint > 2 || !tab || tab->stages < 1 || tab->stages > MFX_RK_MAX_STAGES || n < 1 || p < 1) return -1;
  if (check_op(op) != MFX_OK || op->n != n) return -1;
  return rk_carve(op, tab->stages, n, p, adjoint, nullptr, 0, nullptr);
}

int mfx_rk_solve(const mfx_operator* op, const mfx_rk_tableau* tab, const double* dts, int64_t nsteps, const void* y0, int64_t ldy0,
                 int64_t n, int64_t p, void* y1, int64_t ldy1, void* ys, int flags, void* ws, int64_t ws_bytes, void* stream) {
  MFX_TRY(rk_check(op, tab, dts, nsteps, n, p, nullptr, flags));
  MFX_REQUIRE(y0 && y1, MFX_ERR_INVALID, "null argument");
  MFX_REQUIRE(ldy0 >= n && ldy1 >= n, MFX_ERR_INVALID, "leading dimensions %lld, %lld are shorter than n = %lld", (long long)ldy0,
              (long long)ldy1, (long long)n);
  RkCall call;
  MFX_TRY(rk_prologue("mfx_rk_solve", op, tab, n, p, 0, ws, ws_bytes, stream, &call));
  PrepScope prep_scope;
  GraphKey key = rk_key(kIdRkSolve, op, tab, dts, nsteps, n, p, nullptr, flags, ws, ws_bytes, stream);
  key.add(y0).add(ldy0).add(y1).add(ldy1).add(ys);
  return run_graphed(op_kind(op)->native, key, call.stream, [&](hipStream_t st) {
    return with_dtype(op->dtype, [&](auto t) -> int {
      using T = decltype(t);
      return rk_solve_t<T>(rk_ctx<T>(op, tab, n, p, call.ws, st), dts, nsteps, as<T>(y0), ldy0, as<T>(y1), ldy1, as<T>(ys), call.ws);
    });
  });
}

int mfx_rk_adjoint(const mfx_operator* op, const mfx_rk_tableau* tab, const double* dts, int64_t nsteps, const void* ys, int64_t n,
                   int64_t p, const void* dy1, int64_t lddy1, void* dy0, int64_t lddy0, const mfx_op_grads* grads, int flags, void* ws,
                   int64_t ws_bytes, void* stream) {
  MFX_TRY(rk_check(op, tab, dts, nsteps, n, p, grads, flags));
  MFX_REQUIRE(ys && dy1, MFX_ERR_INVALID, "null argument");
  MFX_REQUIRE(lddy1 >= n && (!dy0 || lddy0 >= n), MFX_ERR_INVALID, "leading dimensions %lld, %lld are shorter than n = %lld",
              (long long)lddy1, (long long)lddy0, (long long)n);
  RkCall call;
  MFX_TRY(rk_prologue("mfx_rk_adjoint", op, tab, n, p, 1, ws, ws_bytes, stream, &call));
  PrepScope prep_scope;
  GraphKey key = rk_key(kIdRkAdjoint, op, tab, dts, nsteps, n, p, grads, flags, ws, ws_bytes, stream);
  key.add(ys).add(dy1).add(lddy1).add(dy0).add(lddy0);
  return run_graphed(op_kind(op)->native, key, call.stream, [&](hipStream_t st) {
    return with_dtype(op->dtype, [&](auto t) -> int {
      using T = decltype(t);
      return rk_adjoint_t<T>(rk_ctx<T>(op, tab, n, p, call.ws, st), dts, nsteps, as<T>(ys), as<T>(dy1), lddy1, as<T>(dy0), lddy0, grads,
                             call.ws);
    });
  });
}

int mfx_rk_backsolve(const mfx_operator* op, const mfx_rk_tableau* tab, const double* dts, int64_t nsteps, const void* y1, int64_t ldy1,
                     int64_t n, int64_t p, const void* dy1, int64_t lddy1, void* dy0, int64_t lddy0, const mfx_op_grads* grads,
                     int flags, void* ws, int64_t ws_bytes, void* stream) {
  MFX_TRY(rk_check(op, tab, dts, nsteps, n, p, grads, flags));
  MFX_REQUIRE(y1 && dy1, MFX_ERR_INVALID, "null argument");
  MFX_REQUIRE(ldy1 >= n && lddy1 >= n && (!dy0 || lddy0 >= n), MFX_ERR_INVALID, "leading dimensions %lld, %lld, %lld are shorter than n = %lld",
              (long long)ldy1, (long long)lddy1, (long long)lddy0, (long long)n);
  RkCall call;
  MFX_TRY(rk_prologue("mfx_rk_backsolve", op, tab, n, p, 2, ws, ws_bytes, stream, &call));
  PrepScope prep_scope;
  GraphKey key = rk_key(kIdRkBacksolve, op, tab, dts, nsteps, n, p, grads, flags, ws, ws_bytes, stream);
  key.add(y1).add(ldy1).add(dy1).add(lddy1).add(dy0).add(lddy0);
  return run_graphed(op_kind(op)->native, key, call.stream, [&](hipStream_t st) {
    return with_dtype(op->dtype, [&](auto t) -> int {
      using T = decltype(t);
      return rk_backsolve_t<T>(rk_ctx<T>(op, tab, n, p, call.ws, st), dts, nsteps, as<T>(y1), ldy1, as<T>(dy1), lddy1, as<T>(dy0), lddy0,
                               grads, call.ws);
    });
  });
}

int64_t mfx_rk_adaptive_workspace_bytes(const mfx_operator* op, const mfx_rk_pair* pair, int64_t n, int64_t p, int64_t max_steps) {
  if (!op || !pair || pair->tab.stages < 1 || pair->tab.stages > MFX_RK_MAX_STAGES || n < 1 || p < 1 || max_steps < 1) return -1;
  if (check_op(op) != MFX_OK || op->n != n) return -1;
  return rk_adaptive_carve(op, pair->tab.stages, n, p, max_steps, nullptr, 0, nullptr);
}

int mfx_rk_solve_adaptive(const mfx_operator* op, const mfx_rk_pair* pair, double t0, double t1, double dt0, double rtol, double atol,
                          int64_t max_steps, int64_t max_attempts, int64_t chunk, const void* y0, int64_t ldy0, int64_t n, int64_t p,
                          void* y1, int64_t ldy1, void* ys, double* dts, mfx_rk_adaptive_info* info, int flags, void* ws,
                          int64_t ws_bytes, void* stream) {
  MFX_TRY(rk_check_adaptive(op, pair, t0, t1, dt0, rtol, atol, max_steps, max_attempts, chunk, n, p, flags));
  MFX_REQUIRE(y0 && y1 && info, MFX_ERR_INVALID, "null argument");
  MFX_REQUIRE(ldy0 >= n && ldy1 >= n, MFX_ERR_INVALID, "leading dimensions %lld, %lld are shorter than n = %lld", (long long)ldy0,
              (long long)ldy1, (long long)n);
  const mfx_rk_tableau* tab = &pair->tab;
  RkAdaptiveWs w;
  const int64_t need = rk_adaptive_carve(op, tab->stages, n, p, max_steps, ws, ws_bytes, &w);
  MFX_REQUIRE(ws && need <= ws_bytes, MFX_ERR_WORKSPACE, "mfx_rk_solve_adaptive: workspace too small: %lld bytes given, %lld needed",
              (long long)ws_bytes, (long long)need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (chunk > max_attempts) chunk = max_attempts;
  PrepScope prep_scope;
  // what a chunk's launches depend on: nothing of t0, t1, dt0, max_attempts (those are in the control block)
  GraphKey key = driver_key(kIdRkAdaptive, op, n, max_steps, p, nullptr, ws, ws_bytes, stream);
  key.add(flags).add(tab->stages).add(pair->order).add(rtol).add(atol).add(chunk).add(ys);
  for (int i = 0; i < tab->stages; ++i) {
    key.add(tab->b[i]).add(pair->e[i]);
    for (int j = 0; j < i; ++j) key.add(tab->a[i][j]);
  }
  RkWs shared{};
  shared.opws = w.opws, shared.opws_bytes = w.opws_bytes;
  RkCtl host{};
  const int rc = with_dtype(op->dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    const size_t row = (size_t)n * sizeof(T);
    k_rk_ctl_init<<<1, 1, 0, st>>>(w.ctl, t0, t1, dt0, max_attempts);
    MFX_CHECK_LAUNCH();
    MFX_TRY(copy_rows_async(w.y, row, y0, (size_t)ldy0 * sizeof(T), row, p, st));
    if (ys) MFX_TRY(copy_rows_async(ys, (size_t)(max_steps + 1) * row, y0, (size_t)ldy0 * sizeof(T), row, p, st));
    const int64_t max_chunks = (max_attempts + chunk - 1) / chunk;
    for (int64_t q = 0; q < max_chunks; ++q) {
      MFX_TRY(run_graphed(op_kind(op)->native, key, st, [&](hipStream_t s) -> int {
        const RkCtx<T> c = rk_ctx<T>(op, tab, n, p, shared, s);
        for (int64_t a = 0; a < chunk; ++a) MFX_TRY(rk_attempt<T>(c, pair, rtol, atol, max_steps, as<T>(ys), w));
        return MFX_OK;
      }));
      MFX_CHECK_HIP(hipMemcpyAsync(&host, w.ctl, sizeof(RkCtl), hipMemcpyDeviceToHost, st));
      MFX_CHECK_HIP(hipStreamSynchronize(st));
      if (host.done) break;
    }
    MFX_REQUIRE(host.done, MFX_ERR_HIP, "mfx_rk_solve_adaptive: the controller did not finish within max_attempts = %lld attempts",
                (long long)max_attempts);
    MFX_TRY(copy_rows_async(y1, (size_t)ldy1 * sizeof(T), w.y, row, row, p, st));
    if (dts && host.n_accepted > 0)
      MFX_CHECK_HIP(hipMemcpyAsync(dts, w.dts, (size_t)host.n_accepted * sizeof(double), hipMemcpyDeviceToHost, st));
    MFX_CHECK_HIP(hipStreamSynchronize(st));
    return MFX_OK;
  });
  MFX_TRY(rc);
  info->status = host.status;
  info->n_accepted = host.n_accepted, info->n_rejected = host.n_rejected, info->n_attempts = host.n_attempts;
  info->t_reached = host.t;
  if (host.status != MFX_RK_OK)
    set_error("mfx_rk_solve_adaptive: %s (t = %.17g of [%.17g, %.17g], %lld accepted, %lld rejected)", rk_status_text(host.status), host.t,
              t0, t1, (long long)host.n_accepted, (long long)host.n_rejected);
  return MFX_OK;
}

}  // extern "C"
