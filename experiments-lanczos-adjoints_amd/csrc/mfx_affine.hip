// libmfx: the affine operator (MFX_OP_AFFINE) -- a native operator A in a rank-one border,
//
//   B = [[A, b], [0, 0]]      d/dt (y, 1) = B (y, 1)   <=>   y' = A y + b      (the reference's pde_heat_affine, util/pde_util.py:90-103)
//
// so that every driver of linear fields (Arnoldi, expm_arnoldi, the Runge-Kutta solve and both of its adjoints) integrates the affine
// one unchanged.  The inner kind's own kernels write the first m = n - 1 entries; the kernels here do the border (DESIGN.md
// section 3.4c), all three HBM-bound streams over m-vectors:
//   k_affine_border   y[:m] += x[m] b, y[m] = 0          one read of b, one read-modify-write of y per probe
//   k_affine_dot      y[m] = b . x[:m]                    per-workgroup partial sums, then k_affine_dot_sum adds them in index order
//   k_affine_grad_b   db[i] += sum_b R_b[m] L_b[i]        the batch loop inside, one add per entry
// A thread owns 16-byte packs (4 floats, 2 doubles) of the vector it WRITES or streams (y, x, db), counted from that vector's own
// 16-byte boundary: a probe whose start is misaligned (n = m + 1 is odd whenever m is even, so every second probe of a dense batch
// is) still moves whole packs, and only the pack that holds the first and the one that holds the last element go entry by entry.
// The second operand (b, L_b) is loaded as a pack where its address is aligned too, entry by entry where not.  Lanes hold
// consecutive packs, so every wave instruction covers 1 KiB of consecutive entries.  No atomics, no cross-workgroup state, a fixed
// summation order: bit-identical from run to run.
#include "mfx_internal.h"

namespace mfx {

constexpr int64_t kAfSpan = 4096;  // entries of one vector per workgroup: 256 threads x 16 entries

static const char* const kAfWho = "affine operator";
static const mfx_affine* af_of(const mfx_operator* op) { return (const mfx_affine*)op->ctx; }
static const mfx_operator* af_inner(const mfx_operator* op) { return op->ctx ? af_of(op)->af_inner : nullptr; }

// position of element 0 of v inside its 16-byte pack
template <typename T>
__device__ __forceinline__ int pack_phase(const T* v) {
  return (int)((reinterpret_cast<uintptr_t>(v) / sizeof(T)) % VecWidth<T>::value);
}
// entries [lo, lo + VEC) of v, zero outside [0, n): one 16-byte load where all of them exist and the address is aligned
template <typename T>
__device__ __forceinline__ Pack<T, VecWidth<T>::value> load_entries(const T* __restrict__ v, int64_t lo, int64_t n) {
  constexpr int VEC = VecWidth<T>::value;
  if (lo >= 0 && lo + VEC <= n && reinterpret_cast<uintptr_t>(v + lo) % (sizeof(T) * VEC) == 0) return load_pack<T, VEC>(v + lo);
  Pack<T, VEC> r;
#pragma unroll
  for (int e = 0; e < VEC; ++e) r.v[e] = (lo + e >= 0 && lo + e < n) ? v[lo + e] : T(0);
  return r;
}
template <typename T>
__device__ __forceinline__ void store_entries(T* __restrict__ v, int64_t lo, int64_t n, const Pack<T, VecWidth<T>::value>& r) {
  constexpr int VEC = VecWidth<T>::value;
  if (lo >= 0 && lo + VEC <= n && reinterpret_cast<uintptr_t>(v + lo) % (sizeof(T) * VEC) == 0) {
    store_pack<T, VEC>(v + lo, r);
    return;
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e)
    if (lo + e >= 0 && lo + e < n) v[lo + e] = r.v[e];
}
// The packs of this workgroup's span of a vector whose element 0 stands at position `phase` of its pack: fn(j, lo), j < PacksPerThread,
// lo = first entry of the pack.  Unrolled: a kernel makes one pass that only loads (into registers indexed by j) and one that
// computes and stores, so all of a thread's 4 (fp32) or 8 (fp64) 16-byte loads per operand are in flight together.
template <typename T>
struct PacksPerThread {
  static constexpr int value = (int)(kAfSpan / VecWidth<T>::value / 256);
};
template <typename T, typename F>
__device__ __forceinline__ void for_packs(int phase, int64_t n, F fn) {
  constexpr int VEC = VecWidth<T>::value;
  const int64_t first = (int64_t)blockIdx.x * (kAfSpan / VEC);
#pragma unroll
  for (int j = 0; j < PacksPerThread<T>::value; ++j) {
    const int64_t lo = (first + j * 256 + threadIdx.x) * VEC - phase;
    if (lo < n) fn(j, lo);
  }
}
// workgroups that cover n entries at any phase
static int64_t af_blocks(int64_t n, int dtype) { return (n + 16 / (int64_t)dtype_size(dtype) - 1 + kAfSpan - 1) / kAfSpan; }

// y_q[:m] += x_q[m] b and y_q[m] = 0, q = blockIdx.y
template <typename T>
__global__ __launch_bounds__(256) void k_affine_border(const T* __restrict__ b, int64_t m, const T* __restrict__ x, int64_t ldx,
                                                       T* __restrict__ y, int64_t ldy) {
  constexpr int VEC = VecWidth<T>::value;
  const T s = x[(int64_t)blockIdx.y * ldx + m];
  y += (int64_t)blockIdx.y * ldy;
  const int phase = pack_phase(y);
  Pack<T, VEC> yv[PacksPerThread<T>::value], bv[PacksPerThread<T>::value];
  for_packs<T>(phase, m + 1, [&](int j, int64_t lo) {
    yv[j] = load_entries<T>(y, lo, m + 1);
    bv[j] = load_entries<T>(b, lo, m);
  });
  for_packs<T>(phase, m + 1, [&](int j, int64_t lo) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) yv[j].v[e] = lo + e == m ? T(0) : yv[j].v[e] + s * bv[j].v[e];
    store_entries<T>(y, lo, m + 1, yv[j]);
  });
}

// out[q ldo + blockIdx.x] = sum over this workgroup's span of b[i] x_q[i], in fp64: thread, wave, then the four waves in order
template <typename T>
__global__ __launch_bounds__(256) void k_affine_dot(const T* __restrict__ b, int64_t m, const T* __restrict__ x, int64_t ldx,
                                                    double* __restrict__ part, int64_t ldpart, T* __restrict__ y, int64_t ldy) {
  constexpr int VEC = VecWidth<T>::value;
  __shared__ double sm[4];
  x += (int64_t)blockIdx.y * ldx;
  double acc = 0.0;
  const int phase = pack_phase(x);
  Pack<T, VEC> xv[PacksPerThread<T>::value], bv[PacksPerThread<T>::value];
  for_packs<T>(phase, m, [&](int j, int64_t lo) {
    xv[j] = load_entries<T>(x, lo, m);
    bv[j] = load_entries<T>(b, lo, m);
  });
  for_packs<T>(phase, m, [&](int j, int64_t) {  // in the order of j: the sum of a thread does not depend on how the loads return
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc += (double)bv[j].v[e] * (double)xv[j].v[e];
  });
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    if (part) part[(int64_t)blockIdx.y * ldpart + blockIdx.x] = s;
    else y[(int64_t)blockIdx.y * ldy + m] = (T)s;  // one workgroup per probe: no second stage
  }
}
// y_q[m] = sum_g part[q][g]: one wave per probe, lane l takes g = l, l + 64, ...
template <typename T>
__global__ __launch_bounds__(64) void k_affine_dot_sum(const double* __restrict__ part, int64_t nblk, T* __restrict__ y, int64_t ldy,
                                                       int64_t m) {
  double acc = 0.0;
  for (int64_t g = threadIdx.x; g < nblk; g += 64) acc += part[(int64_t)blockIdx.x * nblk + g];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) y[(int64_t)blockIdx.x * ldy + m] = (T)acc;
}

// db[i] += sum_q R_q[m] L_q[i]
template <typename T>
__global__ __launch_bounds__(256) void k_affine_grad_b(const T* __restrict__ L, int64_t ldl, const T* __restrict__ R, int64_t ldr,
                                                       int64_t batch, int64_t m, T* __restrict__ db) {
  constexpr int VEC = VecWidth<T>::value;
  constexpr int NP = PacksPerThread<T>::value;
  const int phase = pack_phase(db);
  double acc[NP][VEC];
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[j][e] = 0.0;
  for (int64_t q = 0; q < batch; ++q) {  // one row of L at a time, all of this thread's packs of it in flight; q ascending per entry
    const double r = (double)R[q * ldr + m];
    Pack<T, VEC> lv[NP];
    for_packs<T>(phase, m, [&](int j, int64_t lo) { lv[j] = load_entries<T>(L + q * ldl, lo, m); });
    for_packs<T>(phase, m, [&](int j, int64_t) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[j][e] += r * (double)lv[j].v[e];
    });
  }
  for_packs<T>(phase, m, [&](int j, int64_t lo) {
    Pack<T, VEC> g = load_entries<T>(db, lo, m);
#pragma unroll
    for (int e = 0; e < VEC; ++e) g.v[e] += (T)acc[j][e];
    store_entries<T>(db, lo, m, g);
  });
}

static int af_check(const mfx_operator* op) {
  MFX_REQUIRE(op->ctx, MFX_ERR_INVALID, "%s: ctx (the mfx_affine) is NULL", kAfWho);
  const mfx_affine* af = af_of(op);
  MFX_REQUIRE(af->af_b, MFX_ERR_INVALID, "%s: af_b (the drift) is NULL", kAfWho);
  const mfx_operator* in = af->af_inner;
  MFX_REQUIRE(in, MFX_ERR_INVALID, "%s: af_inner is NULL", kAfWho);
  MFX_REQUIRE(in->kind != MFX_OP_CALLBACK && in->kind != MFX_OP_PRECOND && in->kind != MFX_OP_AFFINE, MFX_ERR_INVALID,
              "%s: the inner operator must be native and neither preconditioned nor affine itself (kind %d)", kAfWho, in->kind);
  MFX_TRY(check_op(in));
  MFX_REQUIRE(op_kind(in)->native, MFX_ERR_INVALID, "%s: the inner operator must be native", kAfWho);
  MFX_REQUIRE(in->dtype == op->dtype, MFX_ERR_INVALID, "%s: dtype %d, inner operator %d", kAfWho, op->dtype, in->dtype);
  MFX_REQUIRE(in->n >= 1, MFX_ERR_INVALID, "%s: the inner operator has no unknowns", kAfWho);
  MFX_REQUIRE(op->n == in->n + 1, MFX_ERR_INVALID, "%s: n = %lld, but the border of an inner operator of %lld unknowns has %lld", kAfWho,
              (long long)op->n, (long long)in->n, (long long)in->n + 1);
  MFX_REQUIRE(in->nrows == 0, MFX_ERR_INVALID, "%s: the inner operator must be whole (nrows = 0)", kAfWho);
  MFX_REQUIRE(op->nrows == 0, MFX_ERR_UNSUPPORTED, "%s: no row block (nrows > 0): the border row and column belong to no shard", kAfWho);
  return MFX_OK;
}

// the drift gradient is this kind's; every other field is the inner kind's
static int af_check_grads(const mfx_operator* op, const mfx_op_grads* grads, bool sharded) {
  const mfx_operator* in = af_inner(op);
  if (!in || in->kind == MFX_OP_AFFINE || in->kind == MFX_OP_PRECOND) return MFX_OK;  // (af_check refuses the descriptor)
  MFX_REQUIRE(!grads->x, MFX_ERR_UNSUPPORTED, "%s: the input gradient (grads->x) of a kernel-Gram inner operator is not swept", kAfWho);
  mfx_op_grads inner = *grads;
  inner.drift = nullptr;
  return check_op_grads(in, &inner, sharded);
}

// The inner operator's workspace FIRST, as in the preconditioned kind: its per-call preparation (PrepScope) lives at the start of it
// and must have one address for every application and for the parameter sweep of a driver call.  Then the partial sums.
struct AfWs {
  void* inner;
  int64_t inner_bytes;
  double* part;
  int64_t nblk;
};
static int64_t af_carve_apply(const mfx_operator* op, int64_t p, void* ws, int64_t ws_bytes, AfWs* out) {
  Carver cv(ws, ws_bytes);
  AfWs w{};
  w.inner_bytes = op_workspace_bytes(af_inner(op), 0, p);
  w.inner = cv.take(w.inner_bytes);
  w.nblk = af_blocks(op->n - 1, op->dtype);
  w.part = w.nblk > 1 ? (double*)cv.take(p * w.nblk * (int64_t)sizeof(double)) : nullptr;
  if (out) *out = w;
  return cv.off;
}

static int64_t af_workspace_bytes(const mfx_operator* op, int64_t batch_hint, int64_t p_apply) {
  const mfx_operator* in = af_inner(op);
  if (!in || in->kind == MFX_OP_AFFINE || in->kind == MFX_OP_PRECOND || !op_kind(in) || op->n < 1) return 256;  // refused before any use
  const int64_t apply = af_carve_apply(op, p_apply > 0 ? p_apply : 1, nullptr, 0, nullptr);
  const int64_t sweep = batch_hint > 0 ? op_workspace_bytes(in, batch_hint, p_apply) : 0;  // the sweep hands all of it to the inner kind
  return apply > sweep ? apply : sweep;
}

template <typename T>
static int af_apply(const mfx_operator* op, int mode, const void* x, int64_t ldx, const void*, int64_t, void* y, int64_t ldy, int64_t p,
                    void* ws, int64_t ws_bytes, hipStream_t stream) {
  const mfx_affine* af = af_of(op);
  const mfx_operator* in = af->af_inner;
  AfWs w;
  const int64_t need = af_carve_apply(op, p, ws, ws_bytes, &w);
  MFX_REQUIRE(ws && need <= ws_bytes, MFX_ERR_WORKSPACE, "%s: workspace too small: need %lld bytes", kAfWho, (long long)need);
  const int64_t m = in->n;
  MFX_REQUIRE(p >= 1 && p <= 65535, MFX_ERR_UNSUPPORTED, "%s: p = %lld outside 1..65535 (one grid row per probe)", kAfWho, (long long)p);
  MFX_TRY(op_kind(in)->apply[sizeof(T) == 8](in, mode == 1 ? 1 : 0, x, ldx, nullptr, 0, y, ldy, p, w.inner, w.inner_bytes, stream));
  if (mode != 1) {
    k_affine_border<T><<<dim3((unsigned)af_blocks(m + 1, op->dtype), (unsigned)p), 256, 0, stream>>>((const T*)af->af_b, m, (const T*)x,
                                                                                                     ldx, (T*)y, ldy);
    MFX_CHECK_LAUNCH();
    return MFX_OK;
  }
  k_affine_dot<T><<<dim3((unsigned)w.nblk, (unsigned)p), 256, 0, stream>>>((const T*)af->af_b, m, (const T*)x, ldx, w.part, w.nblk, (T*)y,
                                                                          ldy);
  MFX_CHECK_LAUNCH();
  if (w.part) {
    k_affine_dot_sum<T><<<(unsigned)p, 64, 0, stream>>>(w.part, w.nblk, (T*)y, ldy, m);
    MFX_CHECK_LAUNCH();
  }
  return MFX_OK;
}

// d/dtheta sum_q L_q^T B R_q: the inner kind's sweep on the first m entries of every row (pointer views), and the drift's own
template <typename T>
static int af_vjp(const mfx_operator* op, const void* L, int64_t ldl, const void* R, int64_t ldr, int64_t batch, int64_t inner,
                  const mfx_op_grads* grads, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const mfx_affine* af = af_of(op);
  const mfx_operator* in = af->af_inner;
  mfx_op_grads theirs = *grads;
  theirs.drift = nullptr;
  MFX_TRY(op_kind(in)->vjp_params[sizeof(T) == 8](in, L, ldl, R, ldr, batch, inner, &theirs, ws, ws_bytes, stream));
  if (!grads->drift || batch < 1) return MFX_OK;
  const int64_t m = in->n;
  k_affine_grad_b<T><<<(unsigned)af_blocks(m, op->dtype), 256, 0, stream>>>((const T*)L, ldl, (const T*)R, ldr, batch, m, (T*)grads->drift);
  MFX_CHECK_LAUNCH();
  return MFX_OK;
}

// the launches of a captured call hold what ctx and af_inner point at, not the pointers
static void af_graph_key(const mfx_operator* op, GraphKey& key) {
  const mfx_operator* in = af_inner(op);
  key.add(af_of(op)->af_b).add(*in);
  if (op_kind(in)->graph_key) op_kind(in)->graph_key(in, key);
}

static const OpKind kAffineKind = {af_check, af_check_grads, af_workspace_bytes, {af_apply<float>, af_apply<double>},
                                   {af_vjp<float>, af_vjp<double>},
                                   "row sharding an affine operator is not implemented: the border row and column belong to no shard",
                                   true, af_graph_key};
const OpKind* affine_kind() { return &kAffineKind; }  // for the table of kinds in mfx_ops.hip

}  // namespace mfx
