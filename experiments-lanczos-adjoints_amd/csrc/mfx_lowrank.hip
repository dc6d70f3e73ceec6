// Low-rank apply  Z_b = scale (V_b - L M L^T V_b)  on a batch of p vectors, and the operator kind built on it:
// MFX_OP_PRECOND, B = S A S with S = P^-1/2 = s^-1/2 (I - L C L^T) for the partial-Cholesky preconditioner P = s I + L L^T
// (DESIGN.md section 3.7c).
//
// mfx_precond_apply (mfx_cg.hip) evaluates the same expression one probe per workgroup row: its finishing kernel re-reads all of
// L^T (rank x n) for every probe.  Inside a Krylov step on S A S the map runs twice per matvec on all probes, so here a workgroup
// owns a slice of n AND a tile of kLrTile probes, and every element of L^T it loads is used for the whole tile: L^T traffic is
// ceil(p / kLrTile) * rank * n elements per pass instead of p * rank * n.
//
//   k_lr_project  part[b][j][slice] = sum_{i in slice} Lt[j][i] V[b][i]        grid (slices, probe tiles)
//   k_lr_small    U[b][j] = sum_i M[i][j] (sum_slices part[b][i][.])           grid (p); both sums in fp64, fixed order
//   k_lr_update   Z[b][i] = scale (V[b][i] - sum_j U[b][j] Lt[j][i])           grid (slices, probe tiles)
//
// A thread owns kLrEpt<T> elements of the slice (element e of thread t: slice0 + e * 256 + t, so every load of a wave covers 64
// consecutive elements) for all probes of the tile, in registers.  No atomics; the sums of a probe are formed by the same threads
// in the same order whatever p is and wherever the probe sits in the batch (the cross-lane tree of wave_sums pairs the same lanes
// for every value index, and a + b == b + a), so a probe's result is bit-identical for every batch (the convention of
// mfx_probe_group).  Arithmetic in the element type; no f16 split: S must be the same map on both sides of A.
#include "mfx_internal.h"

namespace mfx {

constexpr int kLrTile = 16;        // probes per workgroup
constexpr int kLrJg = 8;           // rows of Lt between two workgroup barriers of the projection
constexpr int kLrJc = 64;          // rows of U staged in LDS at a time by the update
constexpr int kLrMaxRank = 4096;   // k_lr_small keeps rank doubles in LDS
constexpr int64_t kPcChunk = 64;   // batch rows of one pass of the PRECOND parameter sweep
template <typename T>
struct LrEpt {
  static constexpr int value = 16 / sizeof(T);  // 4 (fp32) / 2 (fp64) elements per thread and probe
};
template <typename T>
constexpr int64_t lr_slice() { return (int64_t)kBlock * LrEpt<T>::value; }
template <typename T>
static int64_t lr_slices(int64_t n) { return (n + lr_slice<T>() - 1) / lr_slice<T>(); }

template <typename T>
__global__ __launch_bounds__(kBlock) void k_lr_project(const T* __restrict__ lt, int rank, const T* __restrict__ v, int64_t ldv,
                                                       int64_t n, int64_t p, T* __restrict__ part, int64_t nsl) {
  constexpr int E = LrEpt<T>::value;
  __shared__ T sm[kBlock / 64][kLrJg][kLrTile];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t sl = blockIdx.x, b0 = (int64_t)blockIdx.y * kLrTile;
  const int64_t i0 = sl * lr_slice<T>() + tid;
  T vr[kLrTile][E];
#pragma unroll
  for (int q = 0; q < kLrTile; ++q) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int64_t i = i0 + (int64_t)e * kBlock;
      vr[q][e] = (b0 + q < p && i < n) ? v[(b0 + q) * ldv + i] : T(0);
    }
  }
  for (int j0 = 0; j0 < rank; j0 += kLrJg) {
    const int nj = rank - j0 < kLrJg ? rank - j0 : kLrJg;
    for (int jj = 0; jj < nj; ++jj) {
      T lr[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int64_t i = i0 + (int64_t)e * kBlock;
        lr[e] = i < n ? lt[(int64_t)(j0 + jj) * n + i] : T(0);
      }
      T acc[kLrTile];
#pragma unroll
      for (int q = 0; q < kLrTile; ++q) {
        acc[q] = T(0);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[q] += lr[e] * vr[q][e];
      }
      const T wsum = wave_sums<kLrTile>(acc, lane);
      if (wave_sums_writer<kLrTile>(lane)) sm[wid][jj][row16_index<kLrTile>(lane)] = wsum;
    }
    __syncthreads();
    if (tid < nj * kLrTile) {
      const int jj = tid / kLrTile, q = tid % kLrTile;
      T sum = sm[0][jj][q];
#pragma unroll
      for (int w = 1; w < kBlock / 64; ++w) sum += sm[w][jj][q];
      if (b0 + q < p) part[((b0 + q) * rank + j0 + jj) * nsl + sl] = sum;
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_lr_small(const T* __restrict__ part, int64_t nsl, int rank, const T* __restrict__ mid,
                                                  T* __restrict__ u) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* t = reinterpret_cast<double*>(smem_raw);  // [rank]
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  for (int i = tid; i < rank; i += 256) {
    const T* row = part + (b * rank + i) * nsl;
    double acc = 0.0;
    for (int64_t s = 0; s < nsl; ++s) acc += (double)row[s];
    t[i] = acc;
  }
  __syncthreads();
  for (int j = tid; j < rank; j += 256) {
    double acc = 0.0;
    for (int i = 0; i < rank; ++i) acc += (double)mid[(int64_t)i * rank + j] * t[i];  // M is symmetric
    u[b * rank + j] = (T)acc;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_lr_update(const T* __restrict__ lt, int rank, const T* __restrict__ u,
                                                      const T* __restrict__ scale, const T* v, int64_t ldv, T* z, int64_t ldz,
                                                      int64_t n, int64_t p) {  // v and z may be the same buffer: no __restrict__
  constexpr int E = LrEpt<T>::value;
  __shared__ T su[kLrJc][kLrTile];
  const int tid = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.y * kLrTile;
  const int64_t i0 = (int64_t)blockIdx.x * lr_slice<T>() + tid;
  T acc[kLrTile][E];
#pragma unroll
  for (int q = 0; q < kLrTile; ++q) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int64_t i = i0 + (int64_t)e * kBlock;
      acc[q][e] = (b0 + q < p && i < n) ? v[(b0 + q) * ldv + i] : T(0);
    }
  }
  for (int j0 = 0; j0 < rank; j0 += kLrJc) {
    const int nj = rank - j0 < kLrJc ? rank - j0 : kLrJc;
    __syncthreads();  // the previous rows of U are read no more
    for (int t = tid; t < nj * kLrTile; t += kBlock) {
      const int jj = t / kLrTile, q = t % kLrTile;
      su[jj][q] = b0 + q < p ? u[(b0 + q) * rank + j0 + jj] : T(0);
    }
    __syncthreads();
    for (int jj = 0; jj < nj; ++jj) {
      T lr[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int64_t i = i0 + (int64_t)e * kBlock;
        lr[e] = i < n ? lt[(int64_t)(j0 + jj) * n + i] : T(0);
      }
#pragma unroll
      for (int q = 0; q < kLrTile; ++q) {
        const T c = su[jj][q];
#pragma unroll
        for (int e = 0; e < E; ++e) acc[q][e] -= c * lr[e];
      }
    }
  }
  const T sc = scale[0];
#pragma unroll
  for (int q = 0; q < kLrTile; ++q) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int64_t i = i0 + (int64_t)e * kBlock;
      if (b0 + q < p && i < n) z[(b0 + q) * ldz + i] = sc * acc[q][e];
    }
  }
}

// scratch of one low-rank apply on p vectors: the per-slice partials (p, rank, slices) and U (p, rank)
struct LrWs {
  void *part, *u;
};
template <typename T>
static LrWs lr_carve(Carver& cv, int64_t n, int64_t rank, int64_t p) {
  LrWs w;
  w.part = cv.take(p * rank * lr_slices<T>(n) * (int64_t)sizeof(T));
  w.u = cv.take(p * rank * (int64_t)sizeof(T));
  return w;
}
static LrWs lr_carve(Carver& cv, int dtype, int64_t n, int64_t rank, int64_t p) {
  return dtype == MFX_F64 ? lr_carve<double>(cv, n, rank, p) : lr_carve<float>(cv, n, rank, p);
}

// the three launches; every argument has been checked (lr_check)
template <typename T>
static int lr_apply(int64_t n, int64_t rank, const void* lt, const void* mid, const void* scale, const void* v, int64_t ldv, void* z,
                    int64_t ldz, int64_t p, const LrWs& w, hipStream_t stream) {
  const int64_t nsl = lr_slices<T>(n);
  const dim3 grid((unsigned)nsl, (unsigned)((p + kLrTile - 1) / kLrTile));
  k_lr_project<T><<<grid, kBlock, 0, stream>>>((const T*)lt, (int)rank, (const T*)v, ldv, n, p, (T*)w.part, nsl);
  MFX_CHECK_LAUNCH();
  k_lr_small<T><<<(unsigned)p, 256, (size_t)rank * sizeof(double), stream>>>((const T*)w.part, nsl, (int)rank, (const T*)mid, (T*)w.u);
  MFX_CHECK_LAUNCH();
  k_lr_update<T><<<grid, kBlock, 0, stream>>>((const T*)lt, (int)rank, (const T*)w.u, (const T*)scale, (const T*)v, ldv, (T*)z, ldz, n, p);
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

// what the factor of a low-rank apply must satisfy, for the entry point and the operator kind alike
static int lr_check_factor(const char* who, int dtype, int64_t n, int64_t rank, const void* lt, const void* mid, const void* scale) {
  MFX_REQUIRE(dtype == MFX_F32 || dtype == MFX_F64, MFX_ERR_UNSUPPORTED, "%s: unsupported dtype %d", who, dtype);
  MFX_REQUIRE(n >= 1 && rank >= 1 && rank <= n, MFX_ERR_INVALID, "%s: rank %lld outside [1, n = %lld]", who, (long long)rank,
              (long long)n);
  MFX_REQUIRE(lt && mid && scale, MFX_ERR_INVALID, "%s: null factor (lt, mid or scale)", who);
  MFX_REQUIRE(rank <= kLrMaxRank, MFX_ERR_UNSUPPORTED, "%s: rank %lld exceeds the limit %d", who, (long long)rank, kLrMaxRank);
  MFX_REQUIRE(n <= (int64_t)2147483647 * 512, MFX_ERR_UNSUPPORTED, "%s: n = %lld exceeds the grid limit", who, (long long)n);
  return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
// MFX_OP_PRECOND: B = S A S around a native inner operator A (op->ctx -> mfx_precond, its pc_inner)
// ------------------------------------------------------------------------------------------------
static const char* const kPcWho = "preconditioned operator";
static const mfx_precond* pc_of(const mfx_operator* op) { return (const mfx_precond*)op->ctx; }
static const mfx_operator* pc_inner(const mfx_operator* op) { return op->ctx ? pc_of(op)->pc_inner : nullptr; }

static int pc_check(const mfx_operator* op) {
  MFX_REQUIRE(op->ctx, MFX_ERR_INVALID, "%s: ctx (the mfx_precond) is NULL", kPcWho);
  const mfx_precond* pc = pc_of(op);
  const mfx_operator* in = pc->pc_inner;
  MFX_REQUIRE(in, MFX_ERR_INVALID, "%s: pc_inner is NULL", kPcWho);
  MFX_REQUIRE(in->kind != MFX_OP_PRECOND && in->kind != MFX_OP_CALLBACK, MFX_ERR_INVALID,
              "%s: the inner operator must be native and not itself preconditioned (kind %d)", kPcWho, in->kind);
  MFX_REQUIRE(in->kind != MFX_OP_AFFINE, MFX_ERR_INVALID,
              "%s: the inner operator must not be affine (its bordered matrix is not symmetric, and the drift gradient belongs to the "
              "affine kind alone)", kPcWho);
  MFX_TRY(check_op(in));
  MFX_REQUIRE(op_kind(in)->native, MFX_ERR_INVALID, "%s: the inner operator must be native", kPcWho);
  MFX_REQUIRE(in->dtype == op->dtype, MFX_ERR_INVALID, "%s: dtype %d, inner operator %d", kPcWho, op->dtype, in->dtype);
  MFX_REQUIRE(in->n == op->n, MFX_ERR_INVALID, "%s: n = %lld, inner operator %lld", kPcWho, (long long)op->n, (long long)in->n);
  MFX_REQUIRE(in->nrows == 0, MFX_ERR_INVALID, "%s: the inner operator must be whole (nrows = 0)", kPcWho);
  MFX_REQUIRE(op->nrows == 0, MFX_ERR_UNSUPPORTED, "%s: no row block (nrows > 0): S acts on whole vectors", kPcWho);
  return lr_check_factor(kPcWho, op->dtype, op->n, pc->pc_rank, pc->pc_lt, pc->pc_mid, pc->pc_scale);
}

static int pc_check_grads(const mfx_operator* op, const mfx_op_grads* grads, bool sharded) {
  const mfx_operator* in = pc_inner(op);
  if (!in || in->kind == MFX_OP_PRECOND) return MFX_OK;  // (pc_check refuses the descriptor)
  return check_op_grads(in, grads, sharded);             // S is a constant: the gradient fields are the inner kind's
}

// One layout for both calls, the inner operator's workspace FIRST: its per-call preparation (PrepScope) lives at the start of it,
// and the address must be the same for every application and for the parameter sweep of a driver call.
struct PcWs {
  void* inner;
  int64_t inner_bytes;
  void *t, *cl, *cr;  // apply: S x (p, n).  sweep: S L and S R of one chunk (rows, n) each
  LrWs lr;
};
static int64_t pc_carve_apply(const mfx_operator* op, int64_t p, void* ws, int64_t ws_bytes, PcWs* out) {
  const int64_t es = (int64_t)dtype_size(op->dtype);
  Carver cv(ws, ws_bytes);
  PcWs w{};
  w.inner_bytes = op_workspace_bytes(pc_inner(op), 0, p);
  w.inner = cv.take(w.inner_bytes);
  w.t = cv.take(p * op->n * es);
  w.lr = lr_carve(cv, op->dtype, op->n, pc_of(op)->pc_rank, p);
  if (out) *out = w;
  return cv.off;
}
static int64_t pc_carve_sweep(const mfx_operator* op, int64_t rows, void* ws, int64_t ws_bytes, PcWs* out) {
  const int64_t es = (int64_t)dtype_size(op->dtype);
  Carver cv(ws, ws_bytes);
  PcWs w{};
  w.inner_bytes = op_workspace_bytes(pc_inner(op), rows, 0);
  w.inner = cv.take(w.inner_bytes);
  w.cl = cv.take(rows * op->n * es);
  w.cr = cv.take(rows * op->n * es);
  w.lr = lr_carve(cv, op->dtype, op->n, pc_of(op)->pc_rank, rows);
  if (out) *out = w;
  return cv.off;
}
// rows of one pass of the sweep: at most kPcChunk, whole groups of `inner` rows when a group fits
static int64_t pc_chunk_rows(int64_t batch, int64_t inner) {
  int64_t rows = kPcChunk;
  if (inner > 1 && inner <= kPcChunk && batch % inner == 0) rows = kPcChunk / inner * inner;
  return rows < batch ? rows : batch;
}

static int64_t pc_workspace_bytes(const mfx_operator* op, int64_t batch_hint, int64_t p_apply) {
  const mfx_operator* in = pc_inner(op);
  if (!in || in->kind == MFX_OP_PRECOND || !op_kind(in) || pc_of(op)->pc_rank < 1 || op->n < 1) return 256;  // refused before any use
  const int64_t apply = pc_carve_apply(op, p_apply > 0 ? p_apply : 1, nullptr, 0, nullptr);
  const int64_t sweep = batch_hint > 0 ? pc_carve_sweep(op, batch_hint < kPcChunk ? batch_hint : kPcChunk, nullptr, 0, nullptr) : 0;
  return apply > sweep ? apply : sweep;
}

template <typename T>
static int pc_apply(const mfx_operator* op, int mode, const void* x, int64_t ldx, const void*, int64_t, void* y, int64_t ldy, int64_t p,
                    void* ws, int64_t ws_bytes, hipStream_t stream) {
  const mfx_precond* pc = pc_of(op);
  const mfx_operator* in = pc->pc_inner;
  PcWs w;
  const int64_t need = pc_carve_apply(op, p, ws, ws_bytes, &w);
  MFX_REQUIRE(ws && need <= ws_bytes, MFX_ERR_WORKSPACE, "%s: workspace too small: need %lld bytes", kPcWho, (long long)need);
  const int64_t n = op->n;
  MFX_TRY(lr_apply<T>(n, pc->pc_rank, pc->pc_lt, pc->pc_mid, pc->pc_scale, x, ldx, w.t, n, p, w.lr, stream));  // t = S x
  MFX_TRY(op_kind(in)->apply[sizeof(T) == 8](in, mode == 1 ? 1 : 0, w.t, n, nullptr, 0, y, ldy, p, w.inner, w.inner_bytes,
                                             stream));                                                        // u = A t (A^T t)
  return lr_apply<T>(n, pc->pc_rank, pc->pc_lt, pc->pc_mid, pc->pc_scale, y, ldy, y, ldy, p, w.lr, stream);  // y = S u, in place
}

// d/dtheta sum_b L_b^T S A(theta) S R_b = the inner kind's sweep on (S L_b, S R_b), kPcChunk rows at a time
template <typename T>
static int pc_vjp(const mfx_operator* op, const void* Lv, int64_t ldl, const void* Rv, int64_t ldr, int64_t batch, int64_t inner,
                  const mfx_op_grads* grads, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const mfx_precond* pc = pc_of(op);
  const mfx_operator* in = pc->pc_inner;
  const int64_t rows = pc_chunk_rows(batch, inner), n = op->n;
  PcWs w;
  const int64_t need = pc_carve_sweep(op, rows, ws, ws_bytes, &w);
  MFX_REQUIRE(ws && need <= ws_bytes, MFX_ERR_WORKSPACE, "%s: workspace too small: need %lld bytes", kPcWho, (long long)need);
  const int64_t group = (inner > 1 && rows % inner == 0) ? inner : 1;
  const T* L = (const T*)Lv;
  const T* R = (const T*)Rv;
  for (int64_t c0 = 0; c0 < batch; c0 += rows) {
    const int64_t cb = batch - c0 < rows ? batch - c0 : rows;
    MFX_TRY(lr_apply<T>(n, pc->pc_rank, pc->pc_lt, pc->pc_mid, pc->pc_scale, L + c0 * ldl, ldl, w.cl, n, cb, w.lr, stream));
    MFX_TRY(lr_apply<T>(n, pc->pc_rank, pc->pc_lt, pc->pc_mid, pc->pc_scale, R + c0 * ldr, ldr, w.cr, n, cb, w.lr, stream));
    MFX_TRY(op_kind(in)->vjp_params[sizeof(T) == 8](in, w.cl, n, w.cr, n, cb, cb % group == 0 ? group : 1, grads, w.inner,
                                                    w.inner_bytes, stream));
  }
  return MFX_OK;
}

// the launches of a captured call hold what ctx and pc_inner point at, not the pointers (the address in ctx is in the key through
// the bytes of *op, which the drivers add themselves)
static void pc_graph_key(const mfx_operator* op, GraphKey& key) {
  const mfx_operator* in = pc_inner(op);
  const mfx_precond* pc = pc_of(op);
  key.add(pc->pc_lt).add(pc->pc_mid).add(pc->pc_scale).add(pc->pc_rank).add(*in);  // (not the ADDRESS of the inner descriptor: its bytes)
  if (op_kind(in)->graph_key) op_kind(in)->graph_key(in, key);
}

static const OpKind kPrecondKind = {pc_check, pc_check_grads, pc_workspace_bytes, {pc_apply<float>, pc_apply<double>},
                                    {pc_vjp<float>, pc_vjp<double>},
                                    "row sharding a preconditioned operator is not implemented: L would need its rows sharded and "
                                    "L^T v all-reduced, as the row-sharded PCG does",
                                    true, pc_graph_key};
const OpKind* precond_kind() { return &kPrecondKind; }  // for the table of kinds in mfx_ops.hip

static int64_t lr_ws_bytes(int dtype, int64_t n, int64_t rank, int64_t p) {
  Carver cv(nullptr, 0);
  lr_carve(cv, dtype, n, rank, p);
  return cv.off;
}

}  // namespace mfx

using namespace mfx;

extern "C" {

int64_t mfx_lowrank_workspace_bytes(int dtype, int64_t n, int64_t rank, int64_t p) {
  if ((dtype != MFX_F32 && dtype != MFX_F64) || n < 1 || rank < 1 || rank > n || rank > kLrMaxRank || p < 1) return -1;
  return lr_ws_bytes(dtype, n, rank, p);
}

int mfx_lowrank_apply(int dtype, int64_t n, int64_t rank, const void* lt, const void* mid, const void* scale, const void* v,
                      int64_t ldv, void* z, int64_t ldz, int64_t p, void* ws, int64_t ws_bytes, void* stream) {
  static const char* who = "mfx_lowrank_apply";
  MFX_TRY(lr_check_factor(who, dtype, n, rank, lt, mid, scale));
  MFX_REQUIRE(v && z, MFX_ERR_INVALID, "%s: null vectors", who);
  MFX_REQUIRE(p >= 1 && ldv >= n && ldz >= n, MFX_ERR_INVALID, "%s: bad sizes (p %lld, ldv %lld, ldz %lld, n %lld)", who, (long long)p,
              (long long)ldv, (long long)ldz, (long long)n);
  MFX_REQUIRE((p + kLrTile - 1) / kLrTile <= 65535, MFX_ERR_UNSUPPORTED, "%s: at most %d vectors per call", who, 65535 * kLrTile);
  if (!(z == v && ldz == ldv)) {  // in place is allowed; any other overlap is not
    const int64_t es = (int64_t)dtype_size(dtype);
    const char *v0 = (const char*)v, *v1 = v0 + ((p - 1) * ldv + n) * es, *z0 = (const char*)z, *z1 = z0 + ((p - 1) * ldz + n) * es;
    MFX_REQUIRE(z1 <= v0 || v1 <= z0, MFX_ERR_INVALID, "%s: Z overlaps V (only Z == V with ldz == ldv is allowed)", who);
  }
  Carver cv(ws, ws_bytes);
  const LrWs w = lr_carve(cv, dtype, n, rank, p);
  MFX_REQUIRE(ws && cv.off <= ws_bytes, MFX_ERR_WORKSPACE, "%s: workspace too small: need %lld bytes", who, (long long)cv.off);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return with_dtype(dtype, [&](auto t) { return lr_apply<decltype(t)>(n, rank, lt, mid, scale, v, ldv, z, ldz, p, w, s); });
}

}  // extern "C"
