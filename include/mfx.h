/*
 * mfx.h -- C-ABI of the MI355X-native Lanczos/Arnoldi-with-adjoint engine (libmfx.so).
 *
 * This is the drop-in boundary for the hot path of pnkraemer/experiments-lanczos-adjoints.  The
 * reference is pure-Python JAX and has no FFI; the entry points below are what a binding of its
 * functional API would call, and each one cites the reference function it replaces
 * (paths relative to /root/reference/src/matfree_extensions).
 *
 * Conventions
 *   - plain pointers + sizes only; all array pointers are DEVICE pointers unless stated otherwise;
 *   - every buffer is owned by the caller (outputs and workspace are pre-allocated; the library keeps
 *     no device allocations between calls);
 *   - every entry point is asynchronous on the given hipStream_t (passed as void*) and re-entrant
 *     across streams; no host synchronisation inside (except callback operators, see below);
 *   - return value 0 = ok, <0 = error (MFX_ERR_*); mfx_last_error() gives a thread-local message;
 *   - batched layout: a batch of p vectors of length n is row-major (p, n); the Krylov basis is
 *     (p, k, n) -- the layout lanczos.tridiag returns per probe (lanczos.py:165, `Q.T`), batched over
 *     probes in place of jax.vmap (hutchinson.py:14,53).
 */
#ifndef MFX_H
#define MFX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFX_VERSION 201 /* 201: + mfx_comm_rccl_count.  MFX_OP_STENCIL and the st_* fields at the end of mfx_operator are additive (no
                           bump, as for mfx_op_grads.x): callers that zero-fill the descriptor never select them.  MFX_OP_GGN is
                           additive too: its data travels through the existing `ctx` pointer, no struct grows.  So are the three
                           mfx_mlp_jac_* entry points: new symbols, no struct or existing signature changes.  So are
                           mfx_ggn_diag and mfx_ggn_diag_workspace_bytes: new symbols again, no bump.  MFX_OP_PRECOND is additive as
                           MFX_OP_GGN was (struct mfx_precond through `ctx`), and so are mfx_lowrank_apply / mfx_lowrank_workspace_bytes */

enum { MFX_F32 = 0, MFX_F64 = 1 };
enum { MFX_OP_DENSE = 0, MFX_OP_CSR = 1, MFX_OP_RBF = 2, MFX_OP_CALLBACK = 3, MFX_OP_STENCIL = 4, MFX_OP_GGN = 5 };
enum { MFX_OP_PRECOND = 6 }; /* S A S around a native operator, S = P^-1/2 of the partial-Cholesky preconditioner: struct mfx_precond */
enum { MFX_OP_AFFINE = 7 };  /* [[A, b], [0, 0]] around a native operator A: the affine field y' = A y + b as a linear one: struct mfx_affine */
/* Matrix-free 3x3 stencil operator (MFX_OP_STENCIL; util/pde_util.py:18-157).  With S the padded 3x3 correlation below and coef
 * the coefficient field:
 *   MFX_STENCIL_HEAT   state u,       n = ny nx:    y = coef o (S u)                  pde_heat                (:74-87)
 *   MFX_STENCIL_HEAT2  state (u, du), n = 2 ny nx:  y = (-coef o S u, du)             pde_heat_anisotropic    (:106-123)
 *   MFX_STENCIL_WAVE   state (u, du), n = 2 ny nx:  y = (du, coef o S u)              pde_wave_anisotropic    (:126-143)
 * MFX_BOUNDARY_DIRICHLET pads with zeros (:146-150); MFX_BOUNDARY_NEUMANN pads with the nearest cell, clamped on each axis
 * independently (jnp.pad mode="edge", :153-157). */
enum { MFX_STENCIL_HEAT = 0, MFX_STENCIL_HEAT2 = 1, MFX_STENCIL_WAVE = 2 };
enum { MFX_BOUNDARY_DIRICHLET = 0, MFX_BOUNDARY_NEUMANN = 1 };
enum { MFX_REORTHO_NONE = 0, MFX_REORTHO_FULL = 1 };
/* Arithmetic of the fp32 RBF Gram kernels (wide batches; fp64 operators ignore it):
 *   MFX_RBF_FP32          exact fp32 MFMA everywhere (v_mfma_f32_32x32x2_f32, a round-to-nearest fmaf chain)
 *   MFX_RBF_F16X3_MATVEC  Gram matvec emulated on the f16 matrix pipe: operands split hi + lo (2 x 11 bits),
 *                         hi*hi + hi*lo + lo*hi accumulated in fp32; the squared distances are the same 3-product
 *                         split on the f16 pipe, block signs alternating (falls back to fp32-MFMA distances when an
 *                         input exceeds the f16 range); parameter-gradient GEMM exact fp32.
 *   MFX_RBF_F16X3         additionally the parameter-gradient GEMM S = L^T R split the same way; the f16 MFMA's
 *                         truncation bias is decorrelated by pseudo-random column signs on both operands
 *                         (undone in the epilogue).  Fastest mode.
 * Accuracy of the three modes against the fp64 path at the C4 size: DESIGN.md section 3.2 / profiles/r02a_*. */
enum { MFX_RBF_FP32 = 0, MFX_RBF_F16X3_MATVEC = 1, MFX_RBF_F16X3 = 2 };
/* Kernel family of the Gram operator, with s = |x_i/l - x_j/l|^2 clamped at 0 (util/gp_util.py:69-184):
 *   MFX_KERNEL_RBF       sigma exp(-s/2)                                   kernel_scaled_rbf        :151-184
 *   MFX_KERNEL_MATERN12  sigma exp(-r),          r = sqrt(s + eps)         kernel_scaled_matern_12  :110-148
 *   MFX_KERNEL_MATERN32  sigma (1 + r) exp(-r),  r = sqrt(3 s + eps)       kernel_scaled_matern_32  :69-107
 *   MFX_KERNEL_MATERN52  sigma (1 + r + r^2/3) exp(-r), r = sqrt(5 s + eps) kernel_scaled_matern_52  (not in the reference)
 * eps = machine epsilon of the dtype (util/gp_util.py:99,140).  The distance of a point to itself is taken as
 * exactly 0 (the reference's expanded form leaves round-off there, which sqrt amplifies to 3e-4 in fp32). */
enum { MFX_KERNEL_RBF = 0, MFX_KERNEL_MATERN12 = 1, MFX_KERNEL_MATERN32 = 2, MFX_KERNEL_MATERN52 = 3 };
enum {
  MFX_OK = 0,
  MFX_ERR_INVALID = -1,     /* bad argument (shape, null pointer, depth out of range) */
  MFX_ERR_UNSUPPORTED = -2, /* dtype / operator kind / size not supported by this build */
  MFX_ERR_HIP = -3,         /* a HIP runtime call failed */
  MFX_ERR_WORKSPACE = -4,   /* workspace too small */
  MFX_ERR_CALLBACK = -5     /* a callback operator returned non-zero */
};

/* Callback operator (generic Python `matvec(v, *params)` of the reference, e.g. lanczos.py:28-33).
 * x, y are device pointers to p vectors of length n with leading dimensions ldx, ldy (elements).
 * The callee must enqueue its work on `stream` (or synchronise it itself).
 *   mode 0: y = A x                                            (arnoldi.py:84, lanczos.py:254)
 *   mode 1: y = A^T x, and accumulate d/dtheta [x^T A(theta) aux]   (arnoldi.py:207-209; aux = q_idx)
 *   mode 2: y = A x,   and accumulate d/dtheta [aux^T A(theta) x]   (lanczos.py:328-329; aux = x_j)
 * Parameter-gradient accumulation lives on the callee's side (it owns theta). */
typedef int (*mfx_callback_fn)(void* ctx, int mode, const void* x, int64_t ldx, const void* aux,
                               int64_t ldaux, void* y, int64_t ldy, int64_t p, int64_t n,
                               void* stream);

typedef double mfx_stencil_weights[9]; /* the 3 x 3 weights of a stencil operator, row-major (mfx_operator.st_w) */

/* Matrix-free generalised Gauss-Newton operator of an MLP (MFX_OP_GGN; util/bnn_util.py:263-293, 477-499):
 *   A(alpha) = sum_i J_i^T H_i J_i + alpha I,   J_i = d f(theta; x_i) / d theta (c x P),   H_i = loss Hessian in the logits (c x c)
 * with theta and the data FIXED: everything that depends on them is a tape the caller computes once (layer inputs, activation
 * slopes, softmax probabilities); the operator is one pass over that tape per application.  mfx_operator.ctx points at this HOST
 * struct (borrowed, valid for the call); its pointers are device pointers in the operator's dtype.  alpha is the device scalar
 * mfx_operator.noise; its gradient is mfx_op_grads.noise += sum_b L_b . R_b.
 * theta layout (also the layout of every vector the operator takes and returns): for each layer l = 1..L the bias (width[l]
 * values), then the kernel (width[l-1], width[l]) row-major -- flax's ravel_pytree order for the reference's model_mlp.
 * P = sum_l (width[l-1] + 1) width[l] must equal mfx_operator.n.  Per sample i and vector v, in that layout:
 *   t_0 = 0;  s_l = V_W_l^T a_{l-1} + v_b_l + W_l^T t_{l-1};  t_l = dact_l o s_l (l < L),  t_L = s_L
 *   u = p o t_L - p (p . t_L)  (MFX_GGN_CROSS_ENTROPY)   or   u = t_L  (MFX_GGN_MSE)
 *   g_L = u;  y_b_l += g_l;  y_W_l += a_{l-1} g_l^T;  g_{l-1} = dact_{l-1} o (W_l g_l);        y = sum_i (.) + alpha v
 * Symmetric: `transpose` is ignored.  The sum over samples runs in a fixed order (per-workgroup partial sums in the workspace,
 * then one pass that adds them and alpha v): no floating-point atomics, bit-identical from run to run, and the bits of a vector's
 * result do not depend on how many vectors share the call.
 * Refused before any launch.  MFX_ERR_INVALID: ctx, theta, noise, act[l] (l < L), dact[l] (1 <= l < L) or prob (cross-entropy)
 * NULL; nlayers outside 1..MFX_GGN_MAX_LAYERS; a width < 1; nsamples < 1; n != P; an unknown loss.  MFX_ERR_UNSUPPORTED:
 * width[0] > 65536 or width[l] > 64 for l >= 1 (the limits of the kernels); a row block (nrows > 0); the row-sharded drivers;
 * grads->x, grads->dense_a or grads->val non-NULL (gradients with respect to theta or the inputs need third derivatives; the
 * reference never takes them).  The element access of mfx_partial_cholesky refuses the kind, as for CSR. */
enum { MFX_GGN_CROSS_ENTROPY = 0, MFX_GGN_MSE = 1 };
#define MFX_GGN_MAX_LAYERS 8
typedef struct mfx_ggn_net {
  int32_t nlayers;                       /* L >= 1 dense layers */
  int32_t loss;                          /* MFX_GGN_* */
  int64_t nsamples;                      /* N >= 1 */
  int32_t width[MFX_GGN_MAX_LAYERS + 1]; /* width[0] = d_in ... width[L] = c */
  const void* theta;                     /* device, P values, layout above */
  const void* act[MFX_GGN_MAX_LAYERS];   /* act[l] = a_l, (N, width[l]) row-major, l = 0..L-1; a_0 = x */
  const void* dact[MFX_GGN_MAX_LAYERS];  /* dact[l] = phi'(z_l), (N, width[l]), l = 1..L-1; dact[0] unused */
  const void* prob;                      /* (N, c) softmax; NULL for MSE */
} mfx_ggn_net;

/* The Jacobian of the same MLP at the N samples of a tape, J = d f(theta; x_i) / d theta stacked over i ((N c) x P), as a pair of
 * linear maps: what the linearised-Laplace predictive N(f(x*), J* (GGN + alpha I)^-1 J*^T) needs at the test points
 * (util/bnn_util.py:206-215, 630-683).  They take the net directly -- J is rectangular, so it is not an operator kind -- and read
 * neither `loss` nor `prob` (any loss value and a NULL prob are accepted).  theta layout, tape and limits as above.
 *   mfx_mlp_jac_apply     out[b][i][:] = J_i v_b,  out (p, N, c) contiguous, V (p, P) with leading dimension ldv:
 *                           t_0 = 0;  s_l = V_W_l^T a_{l-1} + v_b_l + W_l^T t_{l-1};  t_l = dact_l o s_l (l < L);  out = t_L = s_L
 *                         No workspace and no sum over the samples.
 *   mfx_mlp_jac_t_apply   y_b = sum_i J_i^T u_bi,  U (p, N, c) contiguous, Y (p, P) with leading dimension ldy:
 *                           g_L = u_bi;  y_b_l += g_l;  y_W_l += a_{l-1} g_l^T;  g_{l-1} = dact_{l-1} o (W_l g_l)
 *                         The sum over samples as for the operator: per-workgroup partial sums in the workspace (written before
 *                         they are read), then one pass that adds them in index order; no atomics, bit-identical from run to run,
 *                         and the bits of a vector's result do not depend on how many vectors share the call.
 *   mfx_mlp_jac_workspace_bytes   bytes mfx_mlp_jac_t_apply needs for p vectors (host arithmetic); -1 for arguments it would refuse.
 * The two maps are each other's transpose: <U, J V> = <J^T U, V>.
 * Refused before any launch.  MFX_ERR_INVALID: net, theta, act[l] (l < L), dact[l] (1 <= l < L), V, U, out or Y NULL; nlayers
 * outside 1..MFX_GGN_MAX_LAYERS; a width < 1; nsamples < 1; p < 1; ldv or ldy less than P.  MFX_ERR_UNSUPPORTED: width[0] > 65536 or
 * width[l] > 64 for l >= 1; a dtype other than MFX_F32 / MFX_F64; p > 65535.  MFX_ERR_WORKSPACE: ws NULL or ws_bytes too small. */
int64_t mfx_mlp_jac_workspace_bytes(const mfx_ggn_net* net, int dtype, int64_t p);
int mfx_mlp_jac_apply(const mfx_ggn_net* net, int dtype, const void* V, int64_t ldv, int64_t p, void* out, void* stream);
int mfx_mlp_jac_t_apply(const mfx_ggn_net* net, int dtype, const void* U, int64_t p, void* Y, int64_t ldy, void* ws, int64_t ws_bytes,
                        void* stream);

/* The exact diagonal of the same GGN without the shift, diag = sum_i diag(J_i^T H_i J_i) (P values in the theta layout): the
 * diagonal-Laplace baseline the full-GGN calibration is compared against (util/bnn_baselines.py:10-82 exact_diagonal, which takes
 * N c^2 gradients; util/bnn_util.py:433-474 callibration_loss_diagonal).  It takes the net directly and reads `loss`, and `prob` for
 * cross-entropy only.  For sample i and class o let g_L = e_o and, going down, g_{l-1} = dact_{l-1} o (W_l g_l): row o of J_i has
 * the entry g_{l,m} at bias (l, m) and a_{l-1,k} g_{l,m} at kernel (l, k, m).  With
 *   D_il[m] = max(sum_o p_o g_{l,m}^2 - (sum_o p_o g_{l,m})^2, 0)   (MFX_GGN_CROSS_ENTROPY, H = diag(p) - p p^T)
 *   D_il[m] = sum_o g_{l,m}^2                                       (MFX_GGN_MSE, H = I)
 *   diag[bias (l, m)] = sum_i D_il[m]          diag[kernel (l, k, m)] = sum_i a_{i,l-1,k}^2 D_il[m]
 * The clamp is part of the contract: D is a variance under p, which round-off can push below 0 where the softmax is saturated;
 * the result is >= 0 entrywise (and exactly 0 for c = 1 with cross-entropy).  `diag` is written, not accumulated, and carries no
 * shift: the caller adds alpha.  Asynchronous on `stream`.  The sum over samples as for the operator: per-workgroup partial sums
 * in the workspace (written before they are read), then one pass that adds them in index order; no atomics, bit-identical from
 * run to run, independent of what the workspace held.
 *   mfx_ggn_diag_workspace_bytes   min(ceil(N / 32), 64) P values, rounded up to 256 bytes (host arithmetic); -1 for a net or a
 *                                  dtype the call would refuse.
 * Refused before any launch.  MFX_ERR_INVALID: net, diag, theta, act[l] (l < L), dact[l] (1 <= l < L) or prob (cross-entropy)
 * NULL; an unknown loss; nlayers outside 1..MFX_GGN_MAX_LAYERS; a width < 1; nsamples < 1.  MFX_ERR_UNSUPPORTED: width[0] > 65536
 * or width[l] > 64 for l >= 1; a dtype other than MFX_F32 / MFX_F64.  MFX_ERR_WORKSPACE: ws NULL or ws_bytes too small. */
int64_t mfx_ggn_diag_workspace_bytes(const mfx_ggn_net* net, int dtype);
int mfx_ggn_diag(const mfx_ggn_net* net, int dtype, void* diag, void* ws, int64_t ws_bytes, void* stream);

/* Operator descriptor: a POD of borrowed pointers, valid for the duration of one call.
 * Replaces the reference's `matvec(v, *params)` closures:
 *   DENSE    p @ x                          tests/test_lanczos/test_tridiag_forward.py:18
 *   CSR      BCOO((vals, idx)) @ x          experiments/benchmarks/.../suite_sparse/benchmark.py:64-68
 *   RBF      (K(X,X) + noise I) x           util/gp_util.py:69-184 (RBF / Matern kernels),225-226,525-549
 *   STENCIL  coef o conv3x3(pad(u))         util/pde_util.py:74-157 (heat / wave systems, both boundaries)
 *   GGN      (sum_i J_i^T H_i J_i + alpha I) x  util/bnn_util.py:263-293,477-499 (MLP, fixed theta; struct mfx_ggn_net above)
 *   PRECOND  S A S x, S = P^-1/2 held constant  (not in the reference) a native operator A between two low-rank applies (struct mfx_precond below)
 *   AFFINE   (A x + x_last b, 0)            util/pde_util.py:90-103 (pde_heat_affine): a native operator A in a rank-one border (struct mfx_affine below)
 *   CALLBACK any Python callable                                                              */
typedef struct mfx_operator {
  int32_t kind;  /* MFX_OP_* */
  int32_t dtype; /* MFX_F32 / MFX_F64: element type of vectors, matrix values and X */
  int64_t n;     /* operator is n x n */

  /* DENSE: row-major (n, n), leading dimension lda */
  const void* dense_a;
  int64_t lda;

  /* CSR (int32 indices).  `row` = COO row index per stored value (for the SDDMM gradient).  The
   * transpose structure (CSR of A^T: t_crow, t_col, and t_perm[e] = position of that value in `val`)
   * may be NULL for operators that are only applied forward. */
  const int32_t* crow;
  const int32_t* col;
  const int32_t* row;
  const void* val; /* CSR: the nnz stored values.  STENCIL: the coefficient field, (st_ny, st_nx) row-major, NULL = all ones */
  int64_t nnz;
  int64_t max_row_nnz; /* longest row of A (of A and A^T when the transpose structure is present); 0 = unknown */
  const int32_t* t_crow;
  const int32_t* t_col;
  const int32_t* t_perm;

  /* RBF Gram: X row-major (n, d); constrained hyper-parameters live on the device so that no host
   * synchronisation is needed: lengthscale (d values if ard else 1), outputscale (1), noise (1).
   * d <= 1024 (MFX_ERR_UNSUPPORTED beyond; the reference's kernels take any d, util/gp_util.py:151-184).  Which kernels run: fp32, d <= 32:
   * the f16-split matrix-core kernels (rbf_mode); fp32, up to d = 128 (parameter sweep: 64): the exact-fp32
   * matrix-core kernels in every rbf_mode; everything else (fp64, wider inputs, 1-3 vectors at n < 2048): VALU kernels. */
  const void* x;
  int32_t d;
  int32_t ard;
  int32_t rbf_mode;  /* MFX_RBF_* arithmetic of the fp32 Gram kernels (ignored for fp64) */
  int32_t kernel_fn; /* MFX_KERNEL_*: which stationary kernel the Gram operator evaluates; any other value is MFX_ERR_INVALID */
  const void* lengthscale;
  const void* outputscale;
  const void* noise; /* GGN: the shift alpha (1) */

  /* CALLBACK; GGN: ctx = const mfx_ggn_net* (host); PRECOND: ctx = const mfx_precond* (host); AFFINE: ctx = const mfx_affine* (host) */
  mfx_callback_fn callback;
  void* ctx;

  /* Row block (multi-GPU row sharding; the reference's own row partition of the Gram matvec is
   * util/gp_util.py:496-509).  nrows == 0: the whole operator.  nrows > 0: mfx_op_apply computes only rows
   * [row0, row0 + nrows) of A x (or of A^T x): x keeps length n, y has nrows entries per vector; and
   * mfx_op_vjp_params sums only those rows: L_b has nrows entries (rows row0.. of the full L_b), R_b length n.
   * The matrix-core Gram kernels need row0 % 64 == 0.  The single-device drivers require nrows == 0. */
  int64_t row0;
  int64_t nrows;

  /* STENCIL: a (st_ny, st_nx) row-major grid, both >= 1, cell (r, c) at index r st_nx + c; st_form = MFX_STENCIL_*, st_boundary =
   * MFX_BOUNDARY_*.  st_w are HOST values: st_w[(dr + 1) * 3 + (dc + 1)] multiplies u_pad[r + dr, c + dc], so
   * (S u)[r, c] = sum_{dr, dc} st_w[...] u_pad[r + dr, c + dc] -- a correlation; the reference's convolve2d(stencil, padded, "valid")
   * is this with the stencil flipped on both axes.  Weights that are exactly 0 are not read.  The coefficient field is `val` above
   * (a constant factor such as pde_heat's c is folded into st_w by the caller).  The transpose needs no extra structure.
   * Refused before any launch: MFX_ERR_INVALID for st_ny or st_nx < 1, n != st_ny st_nx (HEAT) or != 2 st_ny st_nx (HEAT2, WAVE), an
   * unknown st_form or st_boundary; MFX_ERR_UNSUPPORTED for more than 2^31 - 1 cells, a row block (nrows > 0) and the row-sharded
   * drivers (sharding a stencil needs a halo exchange).  The element access of mfx_partial_cholesky refuses the kind, as for CSR. */
  int32_t st_ny;
  int32_t st_nx;
  int32_t st_form;
  int32_t st_boundary;
  mfx_stencil_weights st_w;
} mfx_operator;

/* Preconditioned operator (MFX_OP_PRECOND; not in the reference): B = S A S with A = *pc_inner and S = pc_scale (I - L pc_mid L^T) the
 * inverse square root of the partial-Cholesky preconditioner P = s I + L L^T (pc_scale = s^-1/2; pc_mid = V diag(1 / ((s + g_i) +
 * sqrt(s (s + g_i)))) V^T for L^T L = V diag(g) V^T), so that log det A = log det P + tr log B and, S being a constant, the parameter
 * gradients of B are those of A on (S L_b, S R_b).  mfx_operator.ctx points at this HOST struct (borrowed, valid for the call), as
 * for MFX_OP_GGN: mfx_operator itself does not grow.
 *   pc_inner  HOST pointer to the descriptor of A (borrowed, valid for the call): any native kind except PRECOND itself, with the
 *             dtype and n of the outer descriptor and nrows == 0;
 *   pc_lt     L^T, (pc_rank, n) row-major;  pc_mid (pc_rank, pc_rank) symmetric;  pc_scale one value -- device pointers in the
 *             operator's dtype;  1 <= pc_rank <= n.
 * mode 0: y = S A S x;  transpose: y = S A^T S x.  mfx_op_grads means what it means for A (grads->x of a kernel-Gram inner
 * included); the sweep applies S to both factors 64 batch rows at a time, so its scratch is 2 * 64 * n elements.  A's per-call
 * preparation still runs once per driver call.
 * Refused before any launch: MFX_ERR_INVALID for a NULL ctx, a NULL, CALLBACK, PRECOND or AFFINE inner operator, an inner operator its own
 * kind refuses, a dtype or n that differs, an inner row block, pc_rank outside [1, n], a NULL pc_lt, pc_mid or pc_scale;
 * MFX_ERR_UNSUPPORTED for pc_rank > 4096, a row block (nrows > 0) and the row-sharded drivers (L would need its rows sharded and
 * L^T v all-reduced, as mfx_pcg_solve_sharded does).  The element access of mfx_partial_cholesky and the Gram-only entry points
 * refuse the kind, as they refuse every kind but their own. */
typedef struct mfx_precond {
  const mfx_operator* pc_inner;
  const void* pc_lt;
  const void* pc_mid;
  const void* pc_scale;
  int64_t pc_rank;
} mfx_precond;

/* Affine operator (MFX_OP_AFFINE; the reference's pde_heat_affine, util/pde_util.py:90-103, is the one field that needs it): the
 * bordered matrix B = [[A, b], [0, 0]] of the affine vector field y' = A y + b with A = *af_inner, so that d/dt (y, 1) = B (y, 1):
 * exp(t B) (y0, 1) = (e^{tA} y0 + t phi_1(tA) b, 1), and every explicit Runge-Kutta scheme on B is the same scheme on the affine
 * field.  mfx_operator.ctx points at this HOST struct (borrowed, valid for the call), as for MFX_OP_PRECOND; the operator has
 * n = af_inner->n + 1 unknowns.  With m = af_inner->n:
 *   mode 0:     y[:m] = A x[:m] + x[m] b,   y[m] = 0            (x[m] is read on the device: no host synchronisation)
 *   transpose:  y[:m] = A^T x[:m],          y[m] = b . x[:m]    (a two-stage sum in a fixed order, no atomics)
 *   gradients:  those of A on the first m entries of every L_b and R_b (same leading dimensions, no copies), and
 *               mfx_op_grads.drift[i] += sum_b R_b[m] L_b[i].
 *   af_inner  HOST pointer to the descriptor of A (borrowed, valid for the call): any native kind except PRECOND and AFFINE, with
 *             the dtype of the outer descriptor and nrows == 0;
 *   af_b      the drift b, m values in the operator's dtype (device pointer).
 * Workspace: A's own, then one double per probe and per 4096 entries of b for the partial sums of the transposed application.
 * Refused before any launch: MFX_ERR_INVALID for a NULL ctx, af_b or af_inner, a CALLBACK, PRECOND or AFFINE inner operator, an inner
 * operator its own kind refuses, a dtype that differs, n != af_inner->n + 1, an inner row block; MFX_ERR_UNSUPPORTED for a row block
 * (nrows > 0), the row-sharded drivers (the border row and column belong to no shard), grads->x of a kernel-Gram inner operator and
 * more than 65535 vectors in one application.  MFX_OP_PRECOND refuses an affine inner operator (MFX_ERR_INVALID). */
typedef struct mfx_affine {
  const mfx_operator* af_inner;
  const void* af_b;
} mfx_affine;

/* Parameter-gradient outputs (device pointers, ACCUMULATED into, caller zero-fills).  NULL = skip.
 *   dense_a (n, n) row-major, leading dimension = n;  val (CSR: nnz stored values; STENCIL: the (st_ny, st_nx) coefficient field,
 *     val[i] += sigma sum_b L_b[blk + i] (S R_b.u)[i] with (sigma, blk) = (+1, 0) HEAT, (-1, 0) HEAT2, (+1, st_ny st_nx) WAVE);
 *   lengthscale (d if ard else 1), outputscale (1), noise (1; GGN: the shift alpha, noise += sum_b L_b . R_b, the only field
 *     that kind fills);
 *   x (n, d) row-major in the operator's dtype: the gradient with respect to the raw kernel inputs X of a kernel-Gram operator
 *     (the reference differentiates the inputs its lazy kernel closes over, arnoldi.py:21-23, util/gp_util.py:221-231).
 *     Every entry point that takes grads honours it (mfx_op_vjp_params, mfx_arnoldi_adjoint, mfx_lanczos_adjoint; the PCG backward
 *     goes through mfx_op_vjp_params).  Refused before any launch: MFX_ERR_INVALID on any other operator kind, MFX_ERR_UNSUPPORTED
 *     on a row block (nrows > 0) and on the row-sharded drivers.  grads->x == NULL runs exactly the kernels of the other fields.
 *   drift (n - 1 values): the gradient with respect to af_b of an MFX_OP_AFFINE operator, drift[i] += sum_b R_b[n - 1] L_b[i]; the
 *     other fields then mean what they mean for its inner operator.  MFX_ERR_INVALID on every other kind.  It stands BEFORE x: the
 *     layout contract of this struct is that x is its LAST field (tests/test_input_grad_host.py holds the header and the ctypes
 *     mirror to it), so a new field cannot be appended after it.  The offset of x therefore moved by one pointer: callers that name
 *     the fields must be rebuilt against this header (the library, its ctypes mirror and the C programs of tests/cabi live and
 *     build in one tree; there is no other caller).  The offsets of the five fields before it are unchanged.
 * d/dtheta of  sum_b L_b^T A(theta) R_b   (arnoldi.py:207-209, lanczos.py:328-329).
 * The struct grew by `x` at the end, and later by `drift` before it, without a version bump (MFX_VERSION stays 201): C callers must
 * zero-fill it (mfx_op_grads g = {0}; or memset) so that fields they do not know are NULL. */
typedef struct mfx_op_grads {
  void* dense_a;
  void* val;
  void* lengthscale;
  void* outputscale;
  void* noise;
  void* drift;
  void* x;
} mfx_op_grads;

const char* mfx_last_error(void);
int mfx_version(void);

/* Probe groups of the Krylov vector kernels.  Between two operator applications the drivers below run their vector kernels
 * (dots, updates, combine) group by group -- the same kernels on g of the p probes at a time, every pass of a group before the
 * next group -- so that the later passes over a group's basis rows can be served by the Infinity Cache instead of HBM.  Results
 * are bit-identical for every g (a probe's sums are formed by the same workgroups in the same order).  This function is the rule:
 * the largest power of two g whose rows of one pass, g * k * n * elem_size bytes (twice that for adjoint != 0, which sweeps the
 * adjoint states beside the basis), fit a fixed budget; p when all probes fit -- then the launches are exactly the ungrouped
 * ones (every small problem).  1 <= g <= p always; -1 on a non-positive argument.  The row-sharded drivers do not group (each of
 * their vector kernels ends in an all-reduce over all probes).  The environment variable MFX_PROBE_GROUP=<g>, read once per
 * process, overrides the rule inside the drivers (0 = all probes in one launch); this function ignores it. */
int64_t mfx_probe_group(int64_t n, int64_t k, int64_t p, int64_t elem_size, int adjoint);

/* Workspace (bytes) needed by the drivers below for an (n, k, p) problem on this operator. */
int64_t mfx_workspace_bytes(const mfx_operator* op, int64_t n, int64_t k, int64_t p);

/* y_b = A x_b (transpose = 0) or A^T x_b (transpose = 1) for b < p.
 * Replaces one call of the user matvec, vmapped over probes (hutchinson.py:14). */
int mfx_op_apply(const mfx_operator* op, const void* x, int64_t ldx, void* y, int64_t ldy,
                 int64_t p, int transpose, void* ws, int64_t ws_bytes, void* stream);

/* grads += d/dtheta sum_{b<batch} L_b^T A(theta) R_b, with L_b = L + b*ldl, R_b = R + b*ldr.
 * Replaces the parameter half of jax.vjp(matvec) (arnoldi.py:207-209, lanczos.py:328-329), deferred
 * to ONE sweep over all (probe, step) pairs.  Not available for CALLBACK operators. */
int mfx_op_vjp_params(const mfx_operator* op, const void* L, int64_t ldl, const void* R,
                      int64_t ldr, int64_t batch, const mfx_op_grads* grads, void* ws,
                      int64_t ws_bytes, void* stream);

/* arnoldi._forward (arnoldi.py:57-101), batched over p start vectors, live columns only.
 *   v0 (p, n) -> Q (p, k, n) [= reference Q^T], H (p, k, k) row-major, r (p, n) un-normalised,
 *   c (p) = 1/|v0|.  second_pass != 0 runs the re-orthogonalisation pass (reference quirk Q1:
 *   the reference forward always does unless reortho_vjp="none", arnoldi.py:26,91). */
int mfx_arnoldi_forward(const mfx_operator* op, const void* v0, int64_t n, int64_t k, int64_t p,
                        int second_pass, void* Q, void* H, void* r, void* c, void* ws,
                        int64_t ws_bytes, void* stream);

/* arnoldi._forward for COMPLEX vectors (arnoldi.py:57-101 with its .conj() at :66,87,92,95; the case
 * tests/test_arnoldi/test_hessenberg_forward.py:10-37 runs with dtype=complex).  Forward only -- the reference's adjoint is not
 * exercised on complex input either.  All buffers are interleaved (re, im) pairs of the operator's REAL dtype:
 *   v0 (p, n) complex -> Q (p, k, n) complex [= reference Q^T, un-conjugated], H (p, k, k) complex row-major,
 *   r (p, n) complex, c (p) complex (= 1/|v0| + 0 i).
 * `op` is the complex-linear map in its real form: op->n = 2 n, acting on the interleaved vector (a dense complex A becomes the
 * (2 n, 2 n) matrix of 2 x 2 blocks [[Re, -Im], [Im, Re]]; a CALLBACK sees 2 n reals per vector).  The recurrence runs on the
 * real kernels of mfx_arnoldi_forward with two basis slots (q, i q) per complex Krylov vector.
 * Workspace: mfx_complex_workspace_bytes(op, n, k, p). */
int64_t mfx_complex_workspace_bytes(const mfx_operator* op, int64_t n, int64_t k, int64_t p);
int mfx_arnoldi_forward_complex(const mfx_operator* op, const void* v0, int64_t n, int64_t k, int64_t p,
                                int second_pass, void* Q, void* H, void* r, void* c, void* ws,
                                int64_t ws_bytes, void* stream);

/* arnoldi._adjoint (arnoldi.py:104-220).  Cotangents: dQ (p, k, n) or NULL (= 0), dH (p, k, k),
 * dr (p, n) or NULL, dc (p) or NULL.  Outputs dv (p, n); parameter gradients accumulated into
 * `grads` (native operators: one deferred sweep; CALLBACK: inside the callback, per step).
 * reortho = MFX_REORTHO_FULL re-projects lambda every step (arnoldi.py:200-204).
 * Lambda (p, k, n) is caller-provided scratch that holds the adjoint states on return.
 * dv == NULL: the cotangent of the start vector is not wanted (probes are constants in SLQ and in GP training).  The driver then
 * skips what produces only dv -- the last of the k operator applications with its dots, its combine step and the final scaling --
 * and leaves Lambda and `grads` bit for bit what they are with dv.  A CALLBACK operator is still applied k times (it accumulates
 * its parameter gradient inside the application); only the vector kernels behind the last one are skipped. */
int mfx_arnoldi_adjoint(const mfx_operator* op, int64_t n, int64_t k, int64_t p, const void* Q,
                        const void* H, const void* r, const void* c, const void* dQ,
                        const void* dH, const void* dr, const void* dc, int reortho, void* dv,
                        void* Lambda, const mfx_op_grads* grads, void* ws, int64_t ws_bytes,
                        void* stream);

/* lanczos._forward (lanczos.py:215-285): three-term recurrence, no re-orthogonalisation.
 *   v0 (p, n) -> xs (p, k+1, n), alpha (p, k), beta (p, k), vnorm (p) = |v0|. */
int mfx_lanczos_forward(const mfx_operator* op, const void* v0, int64_t n, int64_t k, int64_t p,
                        void* xs, void* alpha, void* beta, void* vnorm, void* ws,
                        int64_t ws_bytes, void* stream);

/* lanczos._adjoint (lanczos.py:288-335).  dxs (p, k+1, n) or NULL, dalpha (p, k), dbeta (p, k).
 * Outputs dv (p, n); Lambda (p, k, n) scratch (adjoint states).  Applies A (not A^T) as the
 * reference does (quirk Q4, lanczos.py:328).
 * dv == NULL as in mfx_arnoldi_adjoint: A lambda_0, the last xi and its dot with x_0 are skipped (a CALLBACK operator is still
 * applied to lambda_0); Lambda and `grads` are unchanged. */
int mfx_lanczos_adjoint(const mfx_operator* op, int64_t n, int64_t k, int64_t p, const void* xs,
                        const void* alpha, const void* beta, const void* vnorm, const void* dxs,
                        const void* dalpha, const void* dbeta, void* dv, void* Lambda,
                        const mfx_op_grads* grads, void* ws, int64_t ws_bytes, void* stream);

/* jnp.linalg.eigh of the k x k tridiagonal (lanczos.py:48-53), batched: alpha (p, k),
 * beta (p, k-1 values, leading dimension ldbeta) -> evals (p, k) (unordered), evecs (p, k, k) with
 * evecs[b][i][a] = component i of eigenvector a.  fp64 arithmetic inside.  k <= 120 in either dtype (work matrix in LDS);
 * 120 < k <= 2048 with fp64 buffers only (the rotations are accumulated in evecs itself; MFX_ERR_UNSUPPORTED in fp32 -- the Python
 * layer casts the k x k problem to fp64 there).  The call is asynchronous, so
 * a QL iteration that fails to converge (200 sweeps per eigenvalue) cannot be reported through the return code:
 * that probe's evals are set to NaN instead (never silently wrong numbers). */
int mfx_tridiag_eigh(const void* alpha, const void* beta, int64_t ldbeta, int64_t p, int64_t k,
                     int dtype, void* evals, void* evecs, void* stream);

/* VJP of  value_b = sum_a evecs[b][0][a]^2 f(evals[b][a])  w.r.t. (alpha, beta) -- what autodiff
 * through eigh + vmap(matfun) + dot yields in lanczos.py:53-59, in divided-difference form.
 * fvals = f(evals), dfvals = f'(evals) (p, k); gout (p) upstream cotangent.  k <= 2048 (beyond 120 the divided differences are
 * evaluated where they are used instead of stored in LDS). */
int mfx_slq_quadform_bwd(const void* evals, const void* evecs, const void* fvals,
                         const void* dfvals, const void* gout, int64_t p, int64_t k, int dtype,
                         void* dalpha, void* dbeta, int64_t lddbeta, void* stream);

/* ---- matrix-function--vector products on the Lanczos path:  f(A) v ~ |v| Q f(T) e1   ----------------
 * The thin layer between the tridiagonalisation and the user: the coefficient vector c = scale f(T) e1 from the eigen-problem
 * mfx_tridiag_eigh solved, the combination y = sum_j c_j q_j over the (p, k, n) basis, and the VJP of both.  No counterpart in
 * the reference (its vector-valued forms are jnp compositions, util/pde_util.py:257-268, :335-356).  All asynchronous, no atomics,
 * bit-reproducible from run to run; fp32 and fp64; every refusal below happens before any launch.
 *
 * coeffs[b][j] = scale[b] sum_a evecs[b][j][a] fvals[b][a] evecs[b][0][a]   (p, k);  fvals = f(evals) (p, k), scale (p).
 * fp64 arithmetic inside, one workgroup per vector, k <= 2048 (MFX_ERR_UNSUPPORTED beyond).  `evals` is not read (the caller
 * evaluated f); it is part of the signature so that forward and backward take the same eigen-problem.
 * MFX_ERR_INVALID: a null pointer, p < 1, k < 1; MFX_ERR_UNSUPPORTED: unknown dtype, k > 2048, p > 2^31 - 1. */
int mfx_funm_coeffs(const void* evals, const void* evecs, const void* fvals, const void* scale, int64_t p, int64_t k, int dtype,
                    void* coeffs, void* stream);

/* VJP of mfx_funm_coeffs w.r.t. the tridiagonal and the scale (Daleckii-Krein).  With U = evecs[b], w = U^T dcoeffs[b],
 * u0 = U[0][:], M_ac = F_ac w_a u0_c (F the divided differences of f at the eigenvalues, F_aa = f'(lam_a) = dfvals) and
 * G = U M U^T:   dalpha[b][i] = scale G_ii,   dbeta[b][i] = scale (G_{i,i+1} + G_{i+1,i})  (leading dimension lddbeta >= k - 1),
 * dscale[b] = <coeffs[b] / scale[b], dcoeffs[b]>  (dscale may be NULL).  M is not symmetric, unlike mfx_slq_quadform_bwd's.
 * Two Ritz values count as equal, and the mean of f' replaces the divided difference, exactly as in mfx_slq_quadform_bwd:
 * |lam_a - lam_c| <= (1e-6 in fp32, 1e-13 in fp64) max|lam|.  k <= 120: M in LDS; k <= 2048: evaluated where it is used.
 * MFX_ERR_INVALID: a null pointer other than dscale (dbeta may be NULL when k == 1), p < 1, k < 1, lddbeta < k - 1;
 * MFX_ERR_UNSUPPORTED: unknown dtype, k > 2048, p > 2^31 - 1. */
int mfx_funm_coeffs_bwd(const void* evals, const void* evecs, const void* fvals, const void* dfvals, const void* dcoeffs,
                        const void* scale, int64_t p, int64_t k, int dtype, void* dalpha, void* dbeta, int64_t lddbeta, void* dscale,
                        void* stream);

/* y[b][:] = sum_j coeffs[b][j] Q[b][j][:]   -- Q (p, k, n) contiguous, coeffs (p, k), y (p, n).  One pass over the basis on the
 * vector geometry of the Krylov drivers (grid = (slices, p), 16-byte loads when n and the pointers allow, double-buffered rows).
 * MFX_ERR_INVALID: a null pointer, n, k or p < 1; MFX_ERR_UNSUPPORTED: unknown dtype, k > 2048, p > 65535. */
int mfx_basis_combine(const void* Q, const void* coeffs, int64_t n, int64_t k, int64_t p, int dtype, void* y, void* stream);

/* VJP of mfx_basis_combine:  dQ[b][j][:] = coeffs[b][j] dy[b][:]  (p, k, n)  and  dcoeffs[b][j] = <Q[b][j], dy[b]>  (p, k): per-slice
 * partial sums in `ws`, re-reduced in fp64 in a fixed order.  dQ == NULL or dcoeffs == NULL skips that half (Q is not read without
 * dcoeffs, coeffs not without dQ; the other output is bit-identical to the full call's).  The workspace is needed for dcoeffs only:
 * mfx_basis_combine_workspace_bytes(n, k, p, dtype) bytes (-1 for arguments the call would refuse), MFX_ERR_WORKSPACE when short.
 * MFX_ERR_INVALID: null dy, both outputs NULL, a null input of a half that is asked for, n, k or p < 1; MFX_ERR_UNSUPPORTED as in
 * mfx_basis_combine. */
int64_t mfx_basis_combine_workspace_bytes(int64_t n, int64_t k, int64_t p, int dtype);
int mfx_basis_combine_bwd(const void* Q, const void* coeffs, const void* dy, int64_t n, int64_t k, int64_t p, int dtype, void* dQ,
                          void* dcoeffs, void* ws, int64_t ws_bytes, void* stream);

/* +-1 probes (matfree.hutchinson.sampler_rademacher call sites: util/gp_util.py:557,
 * optim_logml_adjoints_adaptive.py:109).  Counter-based: element (b, i) depends only on
 * (seed, first_probe + b, i), so probe shards on different GPUs form one global probe matrix. */
int mfx_rademacher(uint64_t seed, int64_t first_probe, int64_t p, int64_t n, int dtype, void* out,
                   void* stream);

/* ---- row-sharded Krylov drivers: one process per GPU, rows of every Krylov vector split over `world` ranks ---------
 *
 * Rank r owns rows [r nloc, min(n, (r+1) nloc)) of every vector (start vector, basis, remainder, adjoint states) and of
 * the operator; nloc is the same on every rank, a multiple of 64.  Per Krylov step the library needs
 *   - ONE all-gather of the (p, nloc) iterate (the operator's input is the full vector), and
 *   - sum-all-reduces of the (p, k+1) Gram-Schmidt coefficients / norms (the reference's `Q.T @ v`, arnoldi.py:87-92,
 *     becomes a partial sum per rank),
 * both enqueued on the caller's stream through the two function pointers below.  The host side supplies them:
 * matfree_extensions/distributed.py binds them to torch.distributed (backend "nccl" = RCCL over xGMI; "gloo" in tests).
 * Buffers handed to the callbacks lie inside the workspace `ws` or inside `Qfull` of the call in progress.
 * H, c and the coefficient buffers come out identical on every rank; parameter gradients are PARTIAL sums over this
 * rank's rows -- the caller adds them over the ranks (one small all-reduce, folded into the estimator's). */
typedef int (*mfx_allreduce_fn)(void* ctx, void* buf, int64_t count, int dtype, void* stream); /* in place, sum */
typedef int (*mfx_allgather_fn)(void* ctx, const void* in, void* out, int64_t count, int dtype,
                                void* stream); /* out[r * count + i] = in_of_rank_r[i] */
/* Optional neighbour exchange (sparse operators: a rank's rows read only a few entries owned by other ranks -- the halo of
 * a stencil -- so all-gathering the whole iterate moves far more than needed).  `full` holds p vectors of length n with leading
 * dimension ldfull; the library has already copied this rank's own rows (`local`, p rows with leading dimension ldlocal) into
 * their place [rank nloc, ...).  The callback must fill every entry of `full` that this rank's rows of A (transpose = 0) or of
 * A^T (transpose = 1) read and that another rank owns; it may leave the rest untouched (it is never read).  NULL: all-gather. */
typedef int (*mfx_exchange_fn)(void* ctx, const void* local, int64_t ldlocal, void* full, int64_t ldfull, int64_t p,
                               int dtype, int transpose, void* stream);
/* Optional: all p vectors of the iterate at once, straight from the row shards (`local`, leading dimension ldlocal) into the
 * operator input `full` (leading dimension ldfull): full[b][r count + i] = local_of_rank_r[b][i], count = nloc.  Used when every
 * rank owns exactly nloc rows (n == world nloc); saves the pack / unpack copies around `allgather`.  NULL: `allgather`. */
typedef int (*mfx_allgather_rows_fn)(void* ctx, const void* local, int64_t ldlocal, void* full, int64_t ldfull, int64_t p,
                                     int64_t count, int dtype, void* stream);
typedef struct mfx_comm {
  int32_t rank, world;
  int64_t nloc; /* rows per rank (last rank: n - rank * nloc >= 1) */
  mfx_allreduce_fn allreduce_sum;
  mfx_allgather_fn allgather;
  void* ctx;
  mfx_exchange_fn exchange;             /* optional, see above */
  mfx_allgather_rows_fn allgather_rows; /* optional, see above */
} mfx_comm;

/* Native communicator: the function pointers of an mfx_comm filled with C functions of libmfx that issue ncclAllReduce /
 * ncclAllGather (RCCL over xGMI) themselves, on the stream of the driver call -- no host-language callback on the path
 * (round 2 went libmfx -> ctypes -> torch.distributed, ~280 callbacks per SLQ step).  RCCL is loaded at run time
 * (dlopen "librccl.so.1"); MFX_ERR_UNSUPPORTED when it is not there.
 *   mfx_rccl_available   : 1 when librccl and the entry points used here could be bound in this process, else 0 (no GPU call;
 *                          lets every rank of a group agree on native vs. callback collectives BEFORE the collective creation);
 *   mfx_rccl_unique_id   : one rank makes the id (ncclGetUniqueId; id: >= 128 bytes of host memory) and hands it to the others
 *                          by any means (matfree_extensions/distributed.py broadcasts it with torch.distributed);
 *   mfx_comm_create_rccl : COLLECTIVE over the `world` ranks (ncclCommInitRank on the calling thread's current device);
 *   mfx_comm_destroy_rccl: releases the communicator (a no-op for an mfx_comm the caller filled in itself). */
int mfx_rccl_available(void);
int mfx_rccl_unique_id(void* id, int64_t bytes);
int mfx_comm_create_rccl(const void* id, int64_t bytes, int32_t rank, int32_t world, int64_t nloc, mfx_comm* out);
int mfx_comm_destroy_rccl(mfx_comm* comm);
/* How a native communicator moves the (p, nloc) iterate of a Krylov step into the (p, n) operator input -- two legs to measure on
 * an 8-GPU node (same results).  mfx_comm_create_rccl leaves the communicator in MFX_GATHER_GROUPED; the Python layer selects
 * MFX_GATHER_PACKED unless told otherwise (matfree_extensions/distributed.py, $MFX_GATHER):
 *   MFX_GATHER_GROUPED: ONE grouped launch of p ncclAllGather of nloc elements each, straight from the row shards into the
 *                       operator input (no pack / unpack copies; at config 4: 64 operations of 64 KB per rank);
 *   MFX_GATHER_PACKED : k_pack_shard, ONE ncclAllGather of p nloc elements (config 4: 4 MB per rank), k_unshard. */
#define MFX_GATHER_GROUPED 0
#define MFX_GATHER_PACKED 1
int mfx_comm_rccl_gather_mode(mfx_comm* comm, int mode);
/* What RCCL itself says about a native communicator: ncclCommCount -> *ranks, ncclCommUserRank -> *rank (the row group the drivers'
 * collectives really span -- reported by bench.py next to torch.distributed's world size, which is a different library's view).
 * MFX_ERR_INVALID for an mfx_comm the caller filled in itself.  No counterpart in the reference (no collective there). */
int mfx_comm_rccl_count(const mfx_comm* comm, int32_t* ranks, int32_t* rank);

int64_t mfx_sharded_workspace_bytes(const mfx_operator* op, const mfx_comm* comm, int64_t n, int64_t k, int64_t p);

/* mfx_arnoldi_forward on row shards.  v0, r: (p, nrows) packed; Q: (p, k, nrows); Qfull: (p, k, n) receives the
 * all-gathered basis (every rank holds all of it afterwards: it is the operator's input in the forward pass anyway, and
 * the R operand of the parameter-gradient sweep in the adjoint); H (p, k, k), c (p) replicated. */
int mfx_arnoldi_forward_sharded(const mfx_operator* op, const mfx_comm* comm, const void* v0, int64_t n, int64_t k,
                                int64_t p, int second_pass, void* Q, void* Qfull, void* H, void* r, void* c, void* ws,
                                int64_t ws_bytes, void* stream);

/* mfx_arnoldi_adjoint on row shards.  Q, dQ, Lambda: (p, k, nrows); r, dr, dv: (p, nrows); Qfull (p, k, n) from the
 * forward pass; H, dH, c, dc replicated.  grads: partial sums over this rank's rows (see above).  dv == NULL as in
 * mfx_arnoldi_adjoint (the last all-gather + operator application and what follows it are skipped). */
int mfx_arnoldi_adjoint_sharded(const mfx_operator* op, const mfx_comm* comm, int64_t n, int64_t k, int64_t p,
                                const void* Q, const void* Qfull, const void* H, const void* r, const void* c,
                                const void* dQ, const void* dH, const void* dr, const void* dc, int reortho, void* dv,
                                void* Lambda, const mfx_op_grads* grads, void* ws, int64_t ws_bytes, void* stream);

/* The three-term recurrence and its adjoint (mfx_lanczos_forward / mfx_lanczos_adjoint below; lanczos.py:231-335) on row
 * shards.  Vectors hold this rank's rows: v0, dv (p, nrows); xs, dxs (p, k + 1, nrows); Lambda (p, k, nrows).  alpha, beta,
 * vnorm and their cotangents are replicated.  Lambdafull (p, k, n) receives the gathered adjoint states -- the operator input
 * of every adjoint step and the right factor of the parameter-gradient sweep, whose result (`grads`) is this rank's PARTIAL sum
 * over its rows: the caller adds the ranks up.  Collectives per step: one all-gather of the iterate, the dots as small
 * all-reduces.  Workspace: mfx_sharded_workspace_bytes.  dv == NULL: the last xi and its dot with x_0 are skipped; lambda_0 is
 * still gathered (and the operator applied to it), because Lambdafull feeds the parameter sweep. */
int mfx_lanczos_forward_sharded(const mfx_operator* op, const mfx_comm* comm, const void* v0, int64_t n, int64_t k,
                                int64_t p, void* xs, void* alpha, void* beta, void* vnorm, void* ws, int64_t ws_bytes,
                                void* stream);
int mfx_lanczos_adjoint_sharded(const mfx_operator* op, const mfx_comm* comm, int64_t n, int64_t k, int64_t p,
                                const void* xs, const void* alpha, const void* beta, const void* vnorm, const void* dxs,
                                const void* dalpha, const void* dbeta, void* dv, void* Lambda, void* Lambdafull,
                                const mfx_op_grads* grads, void* ws, int64_t ws_bytes, void* stream);

/* ---- linear solves ("next" tier: the Mahalanobis half of the GP log-marginal likelihood) -------------------------
 *
 * (Preconditioned) conjugate gradients on a (p, n) batch of right-hand sides  (cg.py:19-60 pcg_fixed_step,
 * :74-137 pcg_adaptive; _safe_divide :222-241).  adaptive = 0: exactly `maxiter` iterations (num_matvecs);
 * adaptive = 1: per right-hand side, iterate while  rms(r / (atol + |x| rtol)) > 1  or steps < miniter, and
 * steps < maxiter; right-hand sides that stop are frozen, so a batch equals p independent solves.
 * Optional preconditioner: the Woodbury solve of  s I + L L^T  (low_rank.py:31-43) given Lt = L^T (rank, n)
 * row-major, minv = (s I + L^T L)^{-1} (rank, rank) and the device scalar s; precond_lt = NULL: none.
 * Outputs: x, r (p, n) packed (final iterate and residual, cg.py:39), num_steps int64 (p) or NULL.
 * Differentiation follows jax.lax.custom_linear_solve (cg.py:23-25): the caller solves again with the cotangent
 * and feeds (-lambda, x) to mfx_op_vjp_params. */
int64_t mfx_pcg_workspace_bytes(const mfx_operator* op, int64_t n, int64_t p, int64_t rank);
int mfx_pcg_solve(const mfx_operator* op, const void* b, int64_t ldb, int64_t n, int64_t p,
                  const void* precond_lt, int64_t rank, const void* precond_minv,
                  const void* precond_shift, int64_t maxiter, int64_t miniter, double atol, double rtol,
                  int adaptive, void* x, void* r, void* num_steps, void* ws, int64_t ws_bytes,
                  void* stream);

/* mfx_pcg_solve on row shards (cg.py:19-137, rows partitioned as util/gp_util.py:496-509): b, x, r hold this rank's rows
 * (p, nrows; ldb >= nrows); precond_lt holds this rank's COLUMNS of L^T, (rank, nrows) row-major; minv, shift replicated (built
 * from the whole L).  Per iteration: one all-gather of the search direction, and p.Ap, r.z, the adaptive error sum and L^T r as
 * small all-reduces -- every rank sees the same scalars, takes the same steps and stops at the same iteration.  num_steps is
 * replicated.  The re-orthogonalising variant is not sharded. */
int64_t mfx_pcg_sharded_workspace_bytes(const mfx_operator* op, const mfx_comm* comm, int64_t n, int64_t p, int64_t rank);
int mfx_pcg_solve_sharded(const mfx_operator* op, const mfx_comm* comm, const void* b, int64_t ldb, int64_t n, int64_t p,
                          const void* precond_lt, int64_t rank, const void* precond_minv, const void* precond_shift,
                          int64_t maxiter, int64_t miniter, double atol, double rtol, int adaptive, void* x, void* r,
                          void* num_steps, void* ws, int64_t ws_bytes, void* stream);

/* Fixed-step PCG that re-orthogonalises the residual against the stored, normalised earlier residuals each step
 * (cg.pcg_fixed_step_reortho, cg.py:140-219): q (p, num_matvecs, n) receives the rows r_i / sqrt(r_i . z_i), the
 * transpose of the reference's info["Q"].  Workspace: mfx_pcg_workspace_bytes with rank = max(rank, num_matvecs). */
int mfx_pcg_solve_reortho(const mfx_operator* op, const void* b, int64_t ldb, int64_t n, int64_t p,
                          const void* precond_lt, int64_t rank, const void* precond_minv,
                          const void* precond_shift, int64_t num_matvecs, void* x, void* r, void* q,
                          void* ws, int64_t ws_bytes, void* stream);

/* z = (v - L (s I + L^T L)^{-1} L^T v) / s on a (p, n) batch: the `solve(v, s)` of low_rank.py:31-43.
 * Workspace: mfx_pcg_workspace_bytes of any operator of this n and dtype. */
int mfx_precond_apply(int dtype, int64_t n, int64_t rank, const void* lt, const void* minv,
                      const void* shift, const void* v, int64_t ldv, void* z, int64_t ldz, int64_t p,
                      void* ws, int64_t ws_bytes, void* stream);

/* Z_b = scale (V_b - L M L^T V_b) for b < p: the shape of mfx_precond_apply's expression with the middle matrix and the factor
 * free -- M = mid (rank, rank) SYMMETRIC, scale a device scalar, lt = L^T (rank, n) row-major, all in `dtype` -- and L^T read once
 * per group of 16 vectors instead of once per vector: ceil(p / 16) * rank * n elements of L^T per pass (one projection pass, one
 * update pass).  With mid = (s I + L^T L)^-1 and scale = 1 / s it is mfx_precond_apply; with the mid and scale of
 * struct mfx_precond it is P^-1/2.  Three kernels: per-slice partial sums of L^T V; U = M (L^T V) with both sums in fp64 and the
 * slices in index order; the update.  No atomics, and no order that depends on p: a vector's result is bit-identical whatever p is
 * and wherever it sits in the batch (the convention of mfx_probe_group).  Arithmetic in `dtype` (no f16 split).
 * Z == V with ldz == ldv is allowed (in place).  Asynchronous on `stream`.
 *   mfx_lowrank_workspace_bytes   bytes for p vectors (host arithmetic); -1 for arguments the call would refuse.
 * Refused before any launch.  MFX_ERR_INVALID: rank < 1 or rank > n; lt, mid, scale, V or Z NULL; p < 1; ldv or ldz < n; Z
 * overlapping V in any other way than Z == V with ldz == ldv.  MFX_ERR_UNSUPPORTED: a dtype other than MFX_F32 / MFX_F64; rank >
 * 4096; p > 16 * 65535.  MFX_ERR_WORKSPACE: ws NULL or ws_bytes too small. */
int64_t mfx_lowrank_workspace_bytes(int dtype, int64_t n, int64_t rank, int64_t p);
int mfx_lowrank_apply(int dtype, int64_t n, int64_t rank, const void* lt, const void* mid, const void* scale, const void* v,
                      int64_t ldv, void* z, int64_t ldz, int64_t p, void* ws, int64_t ws_bytes, void* stream);

/* Modified batched CG (mBCG; Gardner et al. 2018, the estimator behind GPyTorch's marginal likelihood that
 * optim_logml_gpytorch_adaptive.py trains with): mfx_pcg_solve that keeps the scalars of its own iteration, so that ONE
 * preconditioned solve of [y - m, z_1 .. z_p] yields the Mahalanobis term (first column) and, from the probe columns, the Lanczos
 * tridiagonals T_b of M^-1/2 A M^-1/2 started at M^-1/2 b, M = s I + L L^T the preconditioner (M = I without one):
 *   b^T M^-1/2 log(M^-1/2 A M^-1/2) M^-1/2 b  ~  rz0_b e1^T log(T_b) e1,   logdet A = logdet M + E_z[that] for E[z z^T] = M.
 * Arguments up to num_steps, the iteration and the outputs x, r, num_steps are mfx_pcg_solve's bit for bit (the same kernels in the
 * same order; the two scalars are recorded by the thread that already holds them, no launch is added per iteration).  Then, with
 * alpha_j = (r.z)_j / (p.Ap)_j and beta_j = (r.z)_{j+1} / (r.z)_j:
 *   w0    (p, n) or NULL: M^-1 b, the first preconditioned residual (a copy of b without a preconditioner);
 *   rz0   (p): r_0 . z_0 = b^T M^-1 b;
 *   depth (p) int64: the number m_b of live steps.  Step j is live when j < num_steps[b], (r.z)_j > eps^2 and (p.Ap)_j > eps^2 (eps =
 *         machine epsilon of the dtype: the threshold below which the loop's own divisions are switched off, cg.py:222-241) and every
 *         earlier step is live;
 *   tdiag, toff (p, maxiter) in the operator's dtype:  tdiag[j] = 1 / alpha_j + (j > 0 ? beta_{j-1} / alpha_{j-1} : 0) for j < m_b,
 *         toff[j] = sqrt(beta_j) / alpha_j for j < m_b - 1; every other entry is exactly tdiag = 1, toff = 0 -- an identity block
 *         that decouples (log 1 = 0, no weight on e1), so e1^T log(T) e1 of the padded maxiter x maxiter matrix is that of the live
 *         block, and 0 for depth 0.  mfx_tridiag_eigh takes (tdiag, toff, ldbeta = maxiter) as they are.
 * One small kernel after the loop builds tdiag / toff / rz0 / depth.  The gradient of the log-determinant estimate is the trace
 * estimator tr(A^-1 dA) ~ mean_b x_b^T dA w0_b (x_b = A^-1 z_b): one mfx_op_vjp_params sweep over the solves.
 * Refused before any launch, with mfx_pcg_solve's codes: NULL tdiag, toff, rz0 or depth, maxiter < 1 (MFX_ERR_INVALID); a row
 * block, nrows > 0 (MFX_ERR_UNSUPPORTED: there is no sharded form); a short workspace (MFX_ERR_WORKSPACE).
 * Workspace: mfx_mbcg_workspace_bytes (mfx_pcg_workspace_bytes' vectors plus 2 p (maxiter + 1) scalars; -1 on a bad argument). */
int64_t mfx_mbcg_workspace_bytes(const mfx_operator* op, int64_t n, int64_t p, int64_t rank, int64_t maxiter);
int mfx_mbcg_solve(const mfx_operator* op, const void* b, int64_t ldb, int64_t n, int64_t p,
                   const void* precond_lt, int64_t rank, const void* precond_minv,
                   const void* precond_shift, int64_t maxiter, int64_t miniter, double atol, double rtol,
                   int adaptive, void* x, void* r, void* num_steps, void* w0, void* tdiag, void* toff,
                   void* rz0, void* depth, void* ws, int64_t ws_bytes, void* stream);

/* Probes with the preconditioner's covariance, for mfx_mbcg_solve:  out (p, n),
 *   out[b][i] = sqrt(s) eps(b, i) + sum_{c < rank} Lt[c][i] eps(b, n + c),
 * eps(b, j) = the element mfx_rademacher produces for (seed, first_probe + b, j) in a probe of length n + rank, so E[z z^T] =
 * s I + L L^T exactly and probe shards tile one global probe matrix.  lt (rank, n) row-major and the device scalar shift = s as in
 * mfx_precond_apply.  rank = 0 with shift = NULL: plain +-1 probes, bit for bit mfx_rademacher's (rank = 0 with a shift: scaled by
 * sqrt(s)).  One fused kernel generated from the counters: no (p, n + rank) buffer, no workspace.
 * MFX_ERR_INVALID: NULL out, n < 1, p < 1, rank < 0, rank > 0 without lt or shift, unknown dtype; MFX_ERR_UNSUPPORTED: rank > 1024. */
int mfx_precond_sample(int dtype, int64_t n, int64_t rank, const void* lt, const void* shift, uint64_t seed,
                       int64_t first_probe, int64_t p, void* out, void* stream);

/* Partial Cholesky factor of a dense or kernel-Gram operator, element access instead of the reference's
 * lazy_kernel(i, j) callable (low_rank.py:63-120 without pivoting, :123-228 with pivoting).  Output Lt (rank, n)
 * = the reference's factor transposed, already in the original row order (low_rank.py:227-228); pivots int64
 * (rank); success int32 (all pivots positive, :205).  with_noise adds the operator's noise to the diagonal
 * (likelihood_pdf, util/gp_util.py:225-226) or leaves it out (likelihood_pdf_p, :253-254). */
int mfx_partial_cholesky(const mfx_operator* op, int64_t rank, int pivot, int with_noise, void* lt,
                         void* pivots, void* success, void* ws, int64_t ws_bytes, void* stream);

/* y (p, m) = K(X_new, X) v for a kernel-Gram operator: the cross-covariance matvec of the posterior mean
 * (likelihood_condition[_p], util/gp_util.py:299-305,338-344: `matvec(kernel)(xs, inputs, weights)`), no noise
 * term.  xnew (m, d) row-major in the operator's dtype; v (p, n). */
int64_t mfx_gram_cross_workspace_bytes(const mfx_operator* op, int64_t m);
int mfx_gram_cross_apply(const mfx_operator* op, const void* xnew, int64_t m, const void* v, int64_t ldv,
                         void* y, int64_t ldy, int64_t p, void* ws, int64_t ws_bytes, void* stream);

/* The reverse mode of mfx_gram_cross_apply (the gradient of the posterior mean).
 * mfx_gram_cross_apply_t: y (p, n) = K(X, X_new) u with u (p, m), the transpose of mfx_gram_cross_apply (its VJP with
 *   respect to v); workspace: mfx_gram_cross_workspace_bytes.
 * mfx_gram_cross_vjp: with G = sum_b L_b^T K(X_new, X) R_b, L (batch, m), R (batch, n), ACCUMULATES
 *   grads->lengthscale, grads->outputscale += dG/dtheta;  grads->x (n, d) += dG/dX;  gxnew (m, d) += dG/dX_new
 *   (each if non-NULL; grads->noise is not touched: the cross-covariance has no noise term).  Pairs whose distance is
 *   <= 0 add nothing to the lengthscale and input terms.  Deterministic (no atomics).
 * Both refuse before any launch: a non-Gram operator (MFX_ERR_UNSUPPORTED, as mfx_gram_cross_apply), null or
 * inconsistent sizes / leading dimensions and grads->dense_a / grads->val set (MFX_ERR_INVALID), a row block
 * (nrows > 0: MFX_ERR_UNSUPPORTED), a short workspace (MFX_ERR_WORKSPACE). */
int mfx_gram_cross_apply_t(const mfx_operator* op, const void* xnew, int64_t m, const void* u, int64_t ldu,
                           void* y, int64_t ldy, int64_t p, void* ws, int64_t ws_bytes, void* stream);
int64_t mfx_gram_cross_vjp_workspace_bytes(const mfx_operator* op, int64_t m, int64_t batch);
int mfx_gram_cross_vjp(const mfx_operator* op, const void* xnew, int64_t m, const void* L, int64_t ldl,
                       const void* R, int64_t ldr, int64_t batch, const mfx_op_grads* grads, void* gxnew,
                       void* ws, int64_t ws_bytes, void* stream);

/* The cross-covariance VJP for a DENSE weight matrix (the gradient of the GP predictive variance, whose weights
 * S_aj = -2 vbar_a W_aj are diagonal in any batch of the factored form above).
 * mfx_gram_cross_vjp_dense: with G = sum_{a<m, j<n} S[a * lds + j] K(X_new_a, X_j), S (m, n) in the operator's dtype, ACCUMULATES
 *   grads->lengthscale, grads->outputscale += dG/dtheta;  grads->x (n, d) += dG/dX;  gxnew (m, d) += dG/dX_new
 *   (each if non-NULL; grads->noise is not touched).  The formulas, the distance <= 0 rule and the determinism of
 *   mfx_gram_cross_vjp.  Workspace: mfx_gram_cross_vjp_dense_workspace_bytes.
 * Refuses before any launch, with mfx_gram_cross_vjp's codes: a non-Gram operator or a row block (MFX_ERR_UNSUPPORTED), null
 * arguments, m < 1, lds < n, grads->dense_a / grads->val set (MFX_ERR_INVALID), a short workspace (MFX_ERR_WORKSPACE). */
int64_t mfx_gram_cross_vjp_dense_workspace_bytes(const mfx_operator* op, int64_t m);
int mfx_gram_cross_vjp_dense(const mfx_operator* op, const void* xnew, int64_t m, const void* S, int64_t lds,
                             const mfx_op_grads* grads, void* gxnew, void* ws, int64_t ws_bytes, void* stream);

/* A dense block of the kernel matrix written to memory: out[a * ldo + b] = k(xa_a, xb_b) for a < ma, b < mb -- the right-hand
 * sides K(xs, X) and the prior block K(xs, xs) of the joint GP predictive covariance K(xs, xs) - K(xs, X) A^-1 K(X, xs).
 *   op supplies the kernel family, dtype, d, ard, lengthscale and outputscale ONLY: there is no noise term, and op->x, op->n and
 *   op->noise are not read.  xa (ma, d), xb (mb, d) row-major in the operator's dtype; K(xs, X) is xb = op->x, mb = op->n.
 *   xb == NULL: the symmetric block K(xa, xa) (mb must equal ma).  Its diagonal takes the distance exactly 0, as the Gram operator
 *   does for a point against itself (value s kappa(0)), and out[a][b] == out[b][a] bitwise.
 * The formulas of the Gram operator (enum MFX_KERNEL_* above): inputs divided by the lengthscale, |a|^2 + |b|^2 - 2 a.b clamped
 * at 0, eps of the dtype inside Matern's square root; every family, scalar and ARD lengthscale, fp32 and fp64, d <= 1024.  Entries
 * of out beyond column mb of a row (ldo > mb) are not touched.  Deterministic (no atomics).  One 64 x 64 tile per workgroup,
 * stores coalesced along b: the kernel writes ma * mb elements and reads both point sets once per tile row / column.
 * Workspace: mfx_gram_block_workspace_bytes (the scaled copies and squared norms of both point sets; -1 for a non-Gram operator or
 * ma, mb < 1).
 * Refuses before any launch, with mfx_gram_cross_apply's codes: a non-Gram operator or a row block (MFX_ERR_UNSUPPORTED); null op,
 * xa, out, lengthscale or outputscale, ma < 1, mb < 1, ldo < mb, xb == NULL with mb != ma, an unknown kernel_fn or dtype
 * (MFX_ERR_INVALID); a short workspace (MFX_ERR_WORKSPACE).
 * Reverse mode: the gradient of sum_ab S_ab k(xa_a, xb_b) is mfx_gram_cross_vjp_dense on an operator whose x / n are xb / mb, with
 * xnew = xa (symmetric block: x = xa, and the xa gradient is gxnew + grads->x). */
int64_t mfx_gram_block_workspace_bytes(const mfx_operator* op, int64_t ma, int64_t mb);
int mfx_gram_block(const mfx_operator* op, const void* xa, int64_t ma, const void* xb, int64_t mb, void* out, int64_t ldo,
                   void* ws, int64_t ws_bytes, void* stream);

/* The random-Fourier-feature prior path of a pathwise GP posterior sample (Matheron's rule), the (n, m) feature matrix never stored:
 *   mfx_rff_apply   out[s * ldout + i] = c sum_{j<m} cos(2 pi (sum_{t<d} omega[j * d + t] x[i * ldx + t] / l_t + phase[j])) W[s * ldw + j]
 *   mfx_rff_grad_x  dx[i * lddx + t]   = -2 pi c / l_t sum_{s<S} g[s * ldg + i] sum_{j<m} sin(2 pi (...)_ij) W[s * ldw + j] omega[j * d + t]
 * with c = sqrt(2 outputscale / m).  x (n, d) row-major, leading dimension ldx; omega (m, d) contiguous and phase (m) in REVOLUTIONS
 * (the kernel's spectral frequencies at unit lengthscale and the phases, both divided by 2 pi: the phase is reduced with fract() and
 * goes to a cosine that takes revolutions, so phases of 10^4 and more lose nothing to the reduction); lengthscale: 1 (ard = 0) or d
 * (ard = 1) device values and outputscale: 1 device value, already constrained, as the Gram operator gets them; W (S, m), g (S, n)
 * and out (S, n) probe batches with leading dimensions ldw, ldg, ldout; dx (n, d), leading dimension lddx, is OVERWRITTEN.  All
 * arrays in `dtype` (MFX_F32 / MFX_F64).  mfx_rff_grad_x is the vector-Jacobian product of mfx_rff_apply onto x: it recomputes the
 * phases, keeps nothing from the forward, and sums within a row only.  Any n, m, S >= 1 and 1 <= d <= 1024; S beyond one chunk of
 * samples is looped inside.  No workspace, no atomics, a fixed summation order: bit-identical from run to run.  16-byte loads of x
 * and W are used when the pointer and the leading dimension allow them.
 * Refuse before any launch with MFX_ERR_INVALID: an unknown dtype, a NULL array, n, m or S < 1, d outside 1..1024, ard not 0 / 1,
 * ldx < d, ldw < m, ldout < n, ldg < n, lddx < d. */
int mfx_rff_apply(int dtype, const void* x, int64_t ldx, int64_t n, int64_t d, const void* omega, const void* phase, int64_t m,
                  const void* lengthscale, int ard, const void* outputscale, const void* W, int64_t ldw, int64_t S, void* out,
                  int64_t ldout, void* stream);
int mfx_rff_grad_x(int dtype, const void* x, int64_t ldx, int64_t n, int64_t d, const void* omega, const void* phase, int64_t m,
                   const void* lengthscale, int ard, const void* outputscale, const void* W, int64_t ldw, int64_t S, const void* g,
                   int64_t ldg, void* dx, int64_t lddx, void* stream);

/* ---- fixed-step explicit Runge-Kutta solves of y' = A y with native adjoints: the baselines of the PDE work-precision study ------
 * (util/pde_util.py:177-237 solver_euler / solver_diffrax; experiments/applications/partial_differential_equation/workprecision.py).
 * A is any operator the drivers above take.  Additive: new symbols, no struct or existing signature changes, MFX_VERSION stays 201.
 *
 * Tableau (HOST struct): `stages` in 1..MFX_RK_MAX_STAGES, `a` strictly lower triangular, nothing else assumed.  Per step of size dt:
 *   Y_i = y + dt sum_{j<i} a[i][j] K_j,   K_i = A Y_i,   y+ = y + dt sum_i b[i] K_i.
 * dts: nsteps HOST values (they may differ: solver_euler takes diff(ts)).  Vectors are (p, n) batches with the leading dimensions
 * given; ys, when not NULL, is (p, nsteps + 1, n) contiguous and receives every iterate: row 0 is y0, the last row is y1 bit for bit.
 *
 *   mfx_rk_solve      y1 = the nsteps-th iterate from y0.
 *   mfx_rk_adjoint    the DISCRETE adjoint (the exact gradient of the scheme): from ys and the cotangent dy1, per step from the last
 *                     to the first, the stages Y_i, K_i are recomputed from ys[step]; for i = s .. 1:
 *                     Kbar_i = dt b[i] lam + dt sum_{j>i} a[j][i] Ybar_j,  Ybar_i = A^T Kbar_i;  then lam += sum_i Ybar_i.  dy0 = lam after
 *                     the first step; dy0 == NULL skips that last store (grads are bit for bit those of the call that has it).
 *                     Parameter gradient: ONE mfx_op_vjp_params sweep per step, L = the Kbar rows, R = the Y rows, batch p s,
 *                     ACCUMULATED into `grads` (caller zero-fills) as in the Krylov adjoints; a CALLBACK operator accumulates inside
 *                     its transposed application (mode 1, aux = Y_i).
 *   mfx_rk_backsolve  the CONTINUOUS adjoint integrated backwards from y1 with the same tableau, no ys: steps h = -dt, dts reversed,
 *                     on y' = A y, lam' = -A^T lam, thetabar' = -(dA/dtheta)^T [lam, y]; the quadrature of a step is one
 *                     mfx_op_vjp_params sweep with L = the stage values of lam scaled by -h b[i], R = the stage values of y.
 *                     It differs from the discrete gradient by the discretisation error of the backward solve.
 *   mfx_rk_workspace_bytes   bytes for adjoint = 0 (solve), 1 (adjoint), 2 (backsolve); host arithmetic; -1 for arguments the
 *                     call would refuse.
 * flags: none is defined; pass 0.  (A stage kernel that fused the combination into the stencil apply was measured slower or within
 * the noise and is not in the library: DESIGN.md section 3.4b.)
 * Each driver is one fixed sequence of launches on `stream`, replayed from a hipGraph for a native operator; the graph's key
 * covers the tableau, every dts value, nsteps, flags, all pointers and sizes and the operator's own key.  No atomics: bit-identical
 * from run to run.
 * Refused before the workspace is carved and before any launch.  What the operator's kind refuses, first.  MFX_ERR_INVALID: a NULL
 * tableau, dts, or vector argument other than ys / dy0 / grads; stages outside 1..16; a non-zero entry of `a` on or above the
 * diagonal; a non-finite entry of `a`, `b` or dts; nsteps < 1; p < 1; n != op->n; a leading dimension < n; flags != 0.
 * MFX_ERR_UNSUPPORTED: a row block (nrows > 0; there is no row-sharded form), p > 65535, grads->x set (the input gradient of a
 * kernel-Gram operator is not swept here).  MFX_ERR_WORKSPACE: ws NULL or ws_bytes below the query. */
#define MFX_RK_MAX_STAGES 16
typedef struct mfx_rk_tableau {
  int32_t stages;
  double a[MFX_RK_MAX_STAGES][MFX_RK_MAX_STAGES];
  double b[MFX_RK_MAX_STAGES];
} mfx_rk_tableau;
int64_t mfx_rk_workspace_bytes(const mfx_operator* op, const mfx_rk_tableau* tab, int64_t n, int64_t p, int adjoint);
int mfx_rk_solve(const mfx_operator* op, const mfx_rk_tableau* tab, const double* dts, int64_t nsteps, const void* y0, int64_t ldy0,
                 int64_t n, int64_t p, void* y1, int64_t ldy1, void* ys, int flags, void* ws, int64_t ws_bytes, void* stream);
int mfx_rk_adjoint(const mfx_operator* op, const mfx_rk_tableau* tab, const double* dts, int64_t nsteps, const void* ys, int64_t n,
                   int64_t p, const void* dy1, int64_t lddy1, void* dy0, int64_t lddy0, const mfx_op_grads* grads, int flags, void* ws,
                   int64_t ws_bytes, void* stream);
int mfx_rk_backsolve(const mfx_operator* op, const mfx_rk_tableau* tab, const double* dts, int64_t nsteps, const void* y1, int64_t ldy1,
                     int64_t n, int64_t p, const void* dy1, int64_t lddy1, void* dy0, int64_t lddy0, const mfx_op_grads* grads,
                     int flags, void* ws, int64_t ws_bytes, void* stream);

/* ---- adaptive-step explicit Runge-Kutta solve of y' = A y on an embedded pair ----------------------------
 * Additive: new symbols, no struct or existing signature changes, MFX_VERSION stays 201.
 *
 * Pair (HOST struct): `tab` the propagated method, e = b - bhat the error weights (the local error estimate of a step of size h is
 * h sum_i e[i] K_i), `order` the exponent of the controller (error estimator order + 1: 5 for dopri5).
 *
 * Controller: the rule of scipy 1.15's scipy.integrate._ivp.rk.RungeKutta._step_impl.  An attempt from (t, y) with the proposal H:
 *   t+ = min(t + H, t1), h = t+ - t;  y+ = the step of size h;  scale_i = atol + rtol max(|y_i|, |y+_i|);
 *   norm = max over the p states of sqrt(mean_i (err_i / scale_i)^2)    (the batch shares ONE step sequence);
 *   norm < 1: accept (t, y) <- (t+, y+), H <- h f with f = 10 if norm == 0 else min(10, 0.9 norm^(-1/order)), capped at 1 when an
 *   attempt was rejected since the last accepted step;  otherwise reject: H <- h max(0.2, 0.9 norm^(-1/order)).
 * A clipped step that is accepted leaves t == t1 exactly.  The estimate, the scale and the norm are formed in fp64 from the stored
 * (fp32 or fp64) y, y+ and K rows.  Stage and update coefficients are the fp64 products h a[i][j], h b[i] rounded to the dtype once
 * and applied in the order of mfx_rk_solve: the accepted iterates are bit for bit those of mfx_rk_solve with the returned dts.
 *
 * t, h, the counters, the status and the accepted step sizes live in a control block in the workspace; the kernels of an attempt read
 * them there, so an attempt is one fixed launch sequence.  The host enqueues `chunk` attempts, copies the block back and synchronises
 * ONCE per chunk (THE CALL SYNCHRONISES `stream`); after completion inside a chunk the vector kernels return at once and the operator
 * applications run on unchanged data.  For a native operator a chunk is replayed from one hipGraph whose key holds the pair, rtol,
 * atol, chunk, max_steps, all pointers and sizes and the operator's key -- not t0, t1, dt0 or max_attempts.
 *
 * Outputs: y1 = the state at info->t_reached; ys, when not NULL, (p, max_steps + 1, n) contiguous: rows 0 .. n_accepted are the
 * accepted iterates (row 0 = y0), later rows are not written; dts (HOST, max_steps doubles, may be NULL): the n_accepted accepted step
 * sizes; info (HOST, required).  The return value is MFX_OK whenever the solve ran; how it ended is info->status, never silent:
 *   MFX_RK_OK; MFX_RK_MAX_ATTEMPTS (max_attempts attempts, or max_steps accepted steps, without reaching t1); MFX_RK_STEP_TOO_SMALL
 *   (a proposal below 10 ulp(t)); MFX_RK_NONFINITE (a non-finite error norm).  mfx_last_error() names a status other than MFX_RK_OK.
 * No atomics, fixed reduction orders: bit-identical from run to run and for every chunk.
 *   mfx_rk_adaptive_workspace_bytes   host arithmetic; -1 for arguments the call would refuse.
 * Refused before the workspace is carved and before any launch: everything mfx_rk_solve refuses; MFX_ERR_INVALID: a NULL pair or
 * info, a non-finite e, order < 1, rtol or atol negative or rtol + atol not finite or not positive, dt0 <= 0, t1 <= t0 (or either not
 * finite), max_steps < 1, max_attempts < 1, chunk < 1, flags != 0.  MFX_ERR_WORKSPACE: ws NULL or ws_bytes below the query. */
typedef struct mfx_rk_pair {
  mfx_rk_tableau tab;
  double e[MFX_RK_MAX_STAGES];
  int32_t order;
} mfx_rk_pair;
enum { MFX_RK_OK = 0, MFX_RK_MAX_ATTEMPTS = 1, MFX_RK_STEP_TOO_SMALL = 2, MFX_RK_NONFINITE = 3 };
typedef struct mfx_rk_adaptive_info {
  int32_t status;
  int64_t n_accepted, n_rejected, n_attempts;
  double t_reached;
} mfx_rk_adaptive_info;
int64_t mfx_rk_adaptive_workspace_bytes(const mfx_operator* op, const mfx_rk_pair* pair, int64_t n, int64_t p, int64_t max_steps);
int mfx_rk_solve_adaptive(const mfx_operator* op, const mfx_rk_pair* pair, double t0, double t1, double dt0, double rtol, double atol,
                          int64_t max_steps, int64_t max_attempts, int64_t chunk, const void* y0, int64_t ldy0, int64_t n, int64_t p,
                          void* y1, int64_t ldy1, void* ys, double* dts, mfx_rk_adaptive_info* info, int flags, void* ws,
                          int64_t ws_bytes, void* stream);

/* Per-kernel-class device timing with hipEvents recorded on the caller's stream (no host syncs
 * while enabled; events are read back in mfx_timing_read, which synchronises the events).
 * classes: 0 = operator apply, 1 = operator parameter-gradient sweep, 2 = Krylov vector kernels. */
int mfx_timing_enable(int enable);
int mfx_timing_reset(void);
int mfx_timing_read(int cls, double* total_ms, int64_t* launches);

/* hipGraph replay of launch-bound driver calls.  The Krylov drivers enqueue a fixed sequence of launches that
 * depends only on their arguments; for small problems (fewer than 256 vector-kernel workgroups, native operator,
 * timing off) the second call with identical arguments is captured into a hipGraph and later ones are one
 * hipGraphLaunch on the caller's stream.  The reference's counterpart is jax.jit's compiled executable
 * (experiments/benchmarks/wall_times_vjp_through_lanczos_arnoldi/suite_sparse/benchmark.py:91-121 times the
 * jitted function).  Environment MFX_GRAPHS=0 disables it.  Counters since load: calls captured, calls replayed. */
int mfx_graph_stats(int64_t* captured, int64_t* replayed);

#ifdef __cplusplus
}
#endif
#endif /* MFX_H */
