// libmfx: operators A(theta) -- apply, transpose-apply and the deferred parameter-gradient sweep
//   d/dtheta sum_b L_b^T A(theta) R_b        (arnoldi.py:207-209, lanczos.py:328-329)
// The table of operator kinds and the generic functions every driver goes through, with the DENSE and CSR kinds and the CALLBACK
// trampoline.  The other kinds stand next to their kernels: kernel-Gram in mfx_rbf_valu.hip, stencil, GGN, preconditioned, affine.
#include "mfx_internal.h"
#include "mfx_rbf.h"

namespace mfx {

// ================================================================================================
// DENSE   (tests/test_lanczos/test_tridiag_forward.py:18 `p @ s`)
// ================================================================================================
// y[b][i] = sum_j A[i][j] x[b][j] : one wave per row, PB probes per pass
template <typename T, int PB>
__global__ __launch_bounds__(256) void k_dense_apply(const T* __restrict__ A, int64_t lda, int64_t n,
                                                     const T* __restrict__ x, int64_t ldx, T* __restrict__ y,
                                                     int64_t ldy, int64_t p, int64_t row0, int64_t nrow) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + wid;  // local row: y[i] = (A x)[row0 + i]
  const int64_t b0 = (int64_t)blockIdx.y * PB;
  if (i >= nrow) return;
  T acc[PB];
#pragma unroll
  for (int q = 0; q < PB; ++q) acc[q] = T(0);
  const T* row = A + (row0 + i) * lda;
  for (int64_t j = lane; j < n; j += 64) {
    const T a = row[j];
#pragma unroll
    for (int q = 0; q < PB; ++q)
      if (b0 + q < p) acc[q] += a * x[(b0 + q) * ldx + j];
  }
#pragma unroll
  for (int q = 0; q < PB; ++q) {
    const T s = wave_sum(acc[q]);
    if (lane == 0 && b0 + q < p) y[(b0 + q) * ldy + i] = s;
  }
}

// y[b][j] = sum_i A[i][j] x[b][i] : lane = column, the 4 waves split the rows
template <typename T, int PB>
__global__ __launch_bounds__(256) void k_dense_apply_t(const T* __restrict__ A, int64_t lda, int64_t n,
                                                       const T* __restrict__ x, int64_t ldx, T* __restrict__ y,
                                                       int64_t ldy, int64_t p, int64_t row0, int64_t nrow) {
  __shared__ T sm[4][PB][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * 64 + lane;  // local row of A^T: y[j] = (A^T x)[row0 + j]
  const int64_t b0 = (int64_t)blockIdx.y * PB;
  T acc[PB];
#pragma unroll
  for (int q = 0; q < PB; ++q) acc[q] = T(0);
  if (j < nrow) {
    for (int64_t i = wid; i < n; i += 4) {
      const T a = A[i * lda + row0 + j];
#pragma unroll
      for (int q = 0; q < PB; ++q)
        if (b0 + q < p) acc[q] += a * x[(b0 + q) * ldx + i];
    }
  }
#pragma unroll
  for (int q = 0; q < PB; ++q) sm[wid][q][lane] = acc[q];
  __syncthreads();
  if (wid == 0 && j < nrow) {
#pragma unroll
    for (int q = 0; q < PB; ++q)
      if (b0 + q < p) y[(b0 + q) * ldy + j] = sm[0][q][lane] + sm[1][q][lane] + sm[2][q][lane] + sm[3][q][lane];
  }
}

// dA[row0 + i][j] += sum_bt L[bt][i] R[bt][j]   (i < nrow: the rows this call owns)
template <typename T>
__global__ __launch_bounds__(256) void k_dense_grad(const T* __restrict__ L, int64_t ldl, const T* __restrict__ R,
                                                    int64_t ldr, int64_t batch, int64_t n, T* __restrict__ dA,
                                                    int64_t row0, int64_t nrow) {
  const int tj = threadIdx.x & 15, ti = threadIdx.x >> 4;
  const int64_t i = (int64_t)blockIdx.y * 16 + ti, j = (int64_t)blockIdx.x * 16 + tj;
  if (i >= nrow || j >= n) return;
  double acc = 0.0;
  for (int64_t bt = 0; bt < batch; ++bt) acc += (double)L[bt * ldl + i] * (double)R[bt * ldr + j];
  dA[(row0 + i) * n + j] += (T)acc;
}

// ================================================================================================
// CSR   (experiments/benchmarks/.../suite_sparse/benchmark.py:64-68, exp_util.py:35-42)
// ================================================================================================
// 8 lanes per row; `perm` (optional) maps a stored position to its slot in val (transpose structure)
template <typename T>
__global__ __launch_bounds__(256) void k_csr_apply(const int32_t* __restrict__ crow, const int32_t* __restrict__ col,
                                                   const int32_t* __restrict__ perm, const T* __restrict__ val,
                                                   int64_t nrow, const T* __restrict__ x, int64_t ldx,
                                                   T* __restrict__ y, int64_t ldy, int64_t row0) {
  const int sub = threadIdx.x & 7;
  const int64_t row = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);  // local: y[row] = (A x)[row0 + row]
  const int64_t b = blockIdx.y;
  T acc = T(0);
  if (row < nrow) {
    const T* xb = x + b * ldx;
    for (int32_t e = crow[row0 + row] + sub; e < crow[row0 + row + 1]; e += 8) {
      const T v = perm ? val[perm[e]] : val[e];
      acc += v * xb[col[e]];
    }
  }
  acc += __shfl_down(acc, 4, 8);
  acc += __shfl_down(acc, 2, 8);
  acc += __shfl_down(acc, 1, 8);
  if (row < nrow && sub == 0) y[b * ldy + row] = acc;
}

// dval[e] += sum_bt L[bt][row_e - row0] R[bt][col_e]   (SDDMM on the sparsity pattern; only entries of the rows
// [row0, row0 + nrow) this call owns -- the others belong to other row shards)
template <typename T>
__global__ __launch_bounds__(256) void k_csr_grad(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                  int64_t nnz, const T* __restrict__ L, int64_t ldl,
                                                  const T* __restrict__ R, int64_t ldr, int64_t batch,
                                                  T* __restrict__ dval, int64_t row0, int64_t nrow) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const int64_t r = (int64_t)row[e] - row0, c = col[e];
  if (r < 0 || r >= nrow) return;
  double acc = 0.0;
  for (int64_t bt = 0; bt < batch; ++bt) acc += (double)L[bt * ldl + r] * (double)R[bt * ldr + c];
  dval[e] += (T)acc;
}

// ================================================================================================
// dispatch
// ================================================================================================
static int dense_check(const mfx_operator* op) {
  MFX_REQUIRE(op->dense_a, MFX_ERR_INVALID, "dense operator without matrix");
  return MFX_OK;
}

template <typename T>
static int dense_apply(const mfx_operator* op, int mode, const void* x, int64_t ldx, const void*, int64_t, void* y, int64_t ldy,
                       int64_t p, void*, int64_t, hipStream_t stream) {
  const int64_t n = op->n, row0 = op_row0(op), nrow = op_nrows(op);
  constexpr int PB = 4;
  if (mode != 1) {
    k_dense_apply<T, PB><<<dim3((unsigned)((nrow + 3) / 4), (unsigned)((p + PB - 1) / PB)), 256, 0, stream>>>(
        (const T*)op->dense_a, op->lda, n, (const T*)x, ldx, (T*)y, ldy, p, row0, nrow);
  } else {
    k_dense_apply_t<T, PB><<<dim3((unsigned)((nrow + 63) / 64), (unsigned)((p + PB - 1) / PB)), 256, 0, stream>>>(
        (const T*)op->dense_a, op->lda, n, (const T*)x, ldx, (T*)y, ldy, p, row0, nrow);
  }
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

template <typename T>
static int dense_vjp(const mfx_operator* op, const void* L, int64_t ldl, const void* R, int64_t ldr, int64_t batch, int64_t,
                     const mfx_op_grads* grads, void*, int64_t, hipStream_t stream) {
  if (!grads->dense_a) return MFX_OK;
  const int64_t n = op->n, row0 = op_row0(op), nrow = op_nrows(op);
  k_dense_grad<T><<<dim3((unsigned)((n + 15) / 16), (unsigned)((nrow + 15) / 16)), 256, 0, stream>>>(
      (const T*)L, ldl, (const T*)R, ldr, batch, n, (T*)grads->dense_a, row0, nrow);
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

static const OpKind kDenseKind = {dense_check, nullptr, nullptr, {dense_apply<float>, dense_apply<double>},
                                  {dense_vjp<float>, dense_vjp<double>}, nullptr, true, nullptr};

// an operator with no stored values (nnz == 0) is the zero matrix: only the row pointers exist, and the kernel, which
// finds every row empty, reads nothing else
static int csr_check(const mfx_operator* op) {
  MFX_REQUIRE(op->crow && (op->nnz <= 0 || (op->col && op->val)), MFX_ERR_INVALID, "CSR operator without structure");
  return MFX_OK;
}

template <typename T>
static int csr_apply(const mfx_operator* op, int mode, const void* x, int64_t ldx, const void*, int64_t, void* y, int64_t ldy,
                     int64_t p, void*, int64_t, hipStream_t stream) {
  const int64_t row0 = op_row0(op), nrow = op_nrows(op);
  const dim3 grid((unsigned)((nrow + 31) / 32), (unsigned)p);
  if (mode != 1) {
    k_csr_apply<T><<<grid, 256, 0, stream>>>(op->crow, op->col, nullptr, (const T*)op->val, nrow, (const T*)x, ldx, (T*)y, ldy, row0);
  } else {
    MFX_REQUIRE(op->t_crow && (op->nnz <= 0 || (op->t_col && op->t_perm)), MFX_ERR_INVALID,
                "CSR transpose structure required for the Arnoldi adjoint");
    k_csr_apply<T><<<grid, 256, 0, stream>>>(op->t_crow, op->t_col, op->t_perm, (const T*)op->val, nrow, (const T*)x, ldx, (T*)y, ldy, row0);
  }
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

template <typename T>
static int csr_vjp(const mfx_operator* op, const void* L, int64_t ldl, const void* R, int64_t ldr, int64_t batch, int64_t,
                   const mfx_op_grads* grads, void*, int64_t, hipStream_t stream) {
  if (!grads->val || op->nnz == 0) return MFX_OK;  // no stored values: nothing to accumulate (and a zero-sized grid is a launch error)
  MFX_REQUIRE(op->row && op->col, MFX_ERR_INVALID, "CSR gradient needs the COO row index");
  k_csr_grad<T><<<(unsigned)((op->nnz + 255) / 256), 256, 0, stream>>>(op->row, op->col, op->nnz, (const T*)L, ldl, (const T*)R, ldr,
                                                                     batch, (T*)grads->val, op_row0(op), op_nrows(op));
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

static const OpKind kCsrKind = {csr_check, nullptr, nullptr, {csr_apply<float>, csr_apply<double>},
                                {csr_vjp<float>, csr_vjp<double>}, nullptr, true, nullptr};

static int callback_check(const mfx_operator* op) {
  MFX_REQUIRE(op->callback, MFX_ERR_INVALID, "callback operator without function pointer");
  return MFX_OK;
}

static int op_apply_cb(const mfx_operator* op, int mode, const void* x, int64_t ldx, const void* aux, int64_t ldaux, void* y,
                       int64_t ldy, int64_t p, void*, int64_t, hipStream_t stream) {
  // A callback may call back into the library (a Python matvec around a native Gram operator).  Those are calls of their own, on a
  // workspace of the callee's whose contents the driver in progress knows nothing about: they must not inherit its PrepScope, or
  // the second nested application would skip k_rbf_prep and read whatever the caller left in its workspace since the first.
  // The price: every native Gram application inside a callback runs its own k_rbf_prep (one more launch per nested matvec).
  PrepSuspend suspend;
  const int rc = op->callback(op->ctx, mode, x, ldx, aux, ldaux, y, ldy, p, op->n, stream);
  MFX_REQUIRE(rc == 0, MFX_ERR_CALLBACK, "operator callback failed with code %d", rc);
  return MFX_OK;
}

static const OpKind kCallbackKind = {callback_check, nullptr, nullptr, {op_apply_cb, op_apply_cb}, {nullptr, nullptr},
                                     "row sharding needs a native operator", false, nullptr};

// ---- the table and the generic functions every driver goes through -----------------------------------
const OpKind *stencil_kind(), *ggn_kind(), *precond_kind(), *affine_kind();  // mfx_stencil.hip, mfx_ggn.hip, mfx_lowrank.hip, mfx_affine.hip

const OpKind* op_kind(const mfx_operator* op) {
  static const OpKind* const kinds[] = {&kDenseKind, &kCsrKind, gram_kind(), &kCallbackKind, stencil_kind(), ggn_kind(),
                                       precond_kind(), affine_kind()};  // by MFX_OP_*
  return op->kind >= 0 && op->kind < (int)(sizeof(kinds) / sizeof(kinds[0])) ? kinds[op->kind] : nullptr;
}

int check_op(const mfx_operator* op) {
  MFX_REQUIRE(op != nullptr, MFX_ERR_INVALID, "operator is NULL");
  MFX_REQUIRE(op->dtype == MFX_F32 || op->dtype == MFX_F64, MFX_ERR_UNSUPPORTED, "unsupported dtype %d", op->dtype);
  MFX_REQUIRE(op_kind(op), MFX_ERR_UNSUPPORTED, "unknown operator kind %d", op->kind);
  return op_kind(op)->check(op);
}

int check_op_sharded(const mfx_operator* op, const mfx_comm* cm, int64_t n) {
  const OpKind* kind = op_kind(op);
  MFX_REQUIRE(!kind || !kind->no_shard, MFX_ERR_UNSUPPORTED, "%s", kind->no_shard);
  MFX_REQUIRE(op->nrows == 0, MFX_ERR_INVALID, "pass the whole operator: the driver takes this rank's rows itself");
  MFX_REQUIRE(cm && cm->allreduce_sum && cm->allgather, MFX_ERR_INVALID, "communicator without callbacks");
  MFX_REQUIRE(cm->world >= 1 && cm->rank >= 0 && cm->rank < cm->world, MFX_ERR_INVALID, "bad rank %d of %d", cm->rank, cm->world);
  MFX_REQUIRE(cm->nloc >= 64 && cm->nloc % 64 == 0, MFX_ERR_INVALID, "rows per rank (%lld) must be a positive multiple of 64", (long long)cm->nloc);
  MFX_REQUIRE((int64_t)cm->world * cm->nloc >= n && (int64_t)(cm->world - 1) * cm->nloc < n, MFX_ERR_INVALID,
              "%d ranks x %lld rows do not tile n = %lld with a non-empty last shard", cm->world, (long long)cm->nloc, (long long)n);
  return MFX_OK;
}

int check_op_grads(const mfx_operator* op, const mfx_op_grads* grads, bool sharded) {
  if (!op || !grads) return MFX_OK;
  const OpKind* kind = op_kind(op);
  MFX_REQUIRE(!grads->drift || op->kind == MFX_OP_AFFINE, MFX_ERR_INVALID, "the drift gradient (grads->drift) needs an affine operator");
  if (kind && kind->check_grads) return kind->check_grads(op, grads, sharded);
  MFX_REQUIRE(!grads->x, MFX_ERR_INVALID, "the input gradient (grads->x) needs a kernel-Gram operator");
  return MFX_OK;
}

int64_t op_workspace_bytes(const mfx_operator* op, int64_t batch_hint, int64_t p_apply) {
  const OpKind* kind = op_kind(op);
  return kind && kind->workspace_bytes ? kind->workspace_bytes(op, batch_hint, p_apply) : 256;
}

// what op_apply and op_vjp_params refuse alike, before any launch
static int check_op_rows(const mfx_operator* op) {
  MFX_TRY(check_op(op));
  const int64_t n = op->n, row0 = op_row0(op), nrow = op_nrows(op);
  MFX_REQUIRE(row0 >= 0 && nrow >= 1 && row0 + nrow <= n, MFX_ERR_INVALID, "row block [%lld, +%lld) outside the operator (n = %lld)",
              (long long)row0, (long long)nrow, (long long)n);
  return MFX_OK;
}

int op_apply(const mfx_operator* op, int mode, const void* x, int64_t ldx, const void* aux, int64_t ldaux, void* y, int64_t ldy,
             int64_t p, void* ws, int64_t ws_bytes, hipStream_t stream) {
  MFX_TRY(check_op_rows(op));
  const OpKind* kind = op_kind(op);
  const auto apply = kind->apply[op->dtype == MFX_F64];
  if (!kind->native) return apply(op, mode, x, ldx, aux, ldaux, y, ldy, p, ws, ws_bytes, stream);
  MFX_REQUIRE(p <= 65535, MFX_ERR_UNSUPPORTED, "p too large");
  ScopedTimer t(0, stream);
  return apply(op, mode, x, ldx, aux, ldaux, y, ldy, p, ws, ws_bytes, stream);
}

int op_vjp_params(const mfx_operator* op, const void* L, int64_t ldl, const void* R, int64_t ldr, int64_t batch,
                  const mfx_op_grads* grads, void* ws, int64_t ws_bytes, hipStream_t stream, int64_t inner) {
  MFX_TRY(check_op_grads(op, grads, false));
  MFX_REQUIRE(!op_kind(op) || op_kind(op)->native, MFX_ERR_UNSUPPORTED, "callback operators own their parameter gradients");
  MFX_TRY(check_op_rows(op));
  return op_kind(op)->vjp_params[op->dtype == MFX_F64](op, L, ldl, R, ldr, batch, inner, grads, ws, ws_bytes, stream);
}

}  // namespace mfx

using namespace mfx;

extern "C" {

int mfx_op_apply(const mfx_operator* op, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t p,
                 int transpose, void* ws, int64_t ws_bytes, void* stream) {
  MFX_REQUIRE(op && x && y, MFX_ERR_INVALID, "null argument");
  return op_apply(op, transpose ? 1 : 0, x, ldx, nullptr, 0, y, ldy, p, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int mfx_op_vjp_params(const mfx_operator* op, const void* L, int64_t ldl, const void* R, int64_t ldr,
                      int64_t batch, const mfx_op_grads* grads, void* ws, int64_t ws_bytes, void* stream) {
  MFX_REQUIRE(op && L && R && grads, MFX_ERR_INVALID, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ScopedTimer t(1, s);
  return op_vjp_params(op, L, ldl, R, ldr, batch, grads, ws, ws_bytes, s);
}

}  // extern "C"
