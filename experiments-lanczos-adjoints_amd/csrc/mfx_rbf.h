// Host-side interface of the kernel-Gram operator across its four translation units, and to the operator table: what
// mfx_rbf_valu.hip (carve, VALU kernels, path switch, the operator kind) calls in mfx_rbf_mfma.hip (matrix-core matvec) and
// mfx_rbf_mfma_grad.hip (matrix-core parameter sweeps), what the matvec file calls in mfx_rbf_fat.hip, what they share to get there --
// the padded-dimension dispatch, the run-time -> compile-time helpers of the launch sites and the layouts of the workspace regions --
// and what mfx_ops.hip takes from the VALU file: the kind for its table.
#pragma once
#include <type_traits>

#include "mfx_internal.h"

namespace mfx {

// ---- for the operator table (mfx_rbf_valu.hip) -----------------------------------------------------------------------------------
const OpKind* gram_kind();

// ---- padded dimension ----------------------------------------------------------------------------------------------------------
constexpr int kRbfMaxD = 1024;  // wide inputs (d > 32): padded to a multiple of 32, k_rbf_apply_wide / k_rbf_grad_wide
inline int rbf_dpad(int d) { return d <= 4 ? 4 : d <= 8 ? 8 : d <= 12 ? 12 : d <= 16 ? 16 : d <= kRbfMaxD ? (d + 31) / 32 * 32 : -1; }

// A compile-time value arrives at a launch site as a std::integral_constant argument of a generic lambda.
template <int V>
using Const = std::integral_constant<int, V>;

// rbf_dpad's value as a compile-time constant: narrow(Const<DPAD>) for the register kernels (a point in DPAD registers), wide() for
// d > 32 (the padded dimension stays a run-time argument of the *_wide kernels)
template <typename Narrow, typename WideFn>
static void with_dpad(int dpad, Narrow&& narrow, WideFn&& wide) {
  switch (dpad) {
    case 4: narrow(Const<4>{}); break;
    case 8: narrow(Const<8>{}); break;
    case 12: narrow(Const<12>{}); break;
    case 16: narrow(Const<16>{}); break;
    case 32: narrow(Const<32>{}); break;
    default: wide(); break;
  }
}

// The matrix-core set: with_dpad's five, then 64 / 96 / 128.  launch(Const<DPAD>) returns the status and is instantiated up to
// MAXD only, the widest form the entry point builds; beyond it (or off the set) `not_built` becomes the error message.
template <int MAXD, typename Launch>
static int with_mfma_dpad(int dpad, const char* not_built, Launch&& launch) {
  int rc = MFX_ERR_UNSUPPORTED;
  auto arm = [&](auto dc) {
    if constexpr (decltype(dc)::value <= MAXD) rc = launch(dc);
    else set_error("%s", not_built);
  };
  with_dpad(dpad, arm, [&] {
    if (dpad == 64) arm(Const<64>{});
    else if (dpad == 96) arm(Const<96>{});
    else if (dpad == 128) arm(Const<128>{});
    else set_error("%s", not_built);
  });
  return rc;
}

// f(std::true_type / std::false_type) for a run-time flag; f(Const<MFX_KERNEL_*>) for the operator's kernel family
template <typename F>
static auto with_bool(bool flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
static int with_kind(int kernel_fn, F&& f) {
  switch (kernel_fn) {
    case MFX_KERNEL_RBF: return f(Const<MFX_KERNEL_RBF>{});
    case MFX_KERNEL_MATERN12: return f(Const<MFX_KERNEL_MATERN12>{});
    case MFX_KERNEL_MATERN32: return f(Const<MFX_KERNEL_MATERN32>{});
    case MFX_KERNEL_MATERN52: return f(Const<MFX_KERNEL_MATERN52>{});
    default: set_error("unknown kernel_fn %d", kernel_fn); return MFX_ERR_INVALID;
  }
}

// 16-byte vector access to two fp32 operands: both extents and both leading dimensions multiples of 4, both bases 16-byte aligned
inline bool vec4_ok(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t n, int64_t nrow) {
  return (n % 4 == 0) && (nrow % 4 == 0) && (lda % 4 == 0) && (ldb % 4 == 0) && (reinterpret_cast<uintptr_t>(a) % 16 == 0) &&
         (reinterpret_cast<uintptr_t>(b) % 16 == 0);
}

// ---- which kernels run (mfx_rbf_mfma.hip / mfx_rbf_mfma_grad.hip, next to the kernels the answers describe) --------------------
enum class RbfApplyPath { valu, exact, h3 };    // VALU kernel | exact-fp32 MFMA | 3 x f16 split (fat-wave kernels or the h3 pair)
enum class RbfGradPath { valu, exact, split };  // VALU sweep | exact-fp32 MFMA GEMM | 3 x f16 split GEMM
RbfApplyPath rbf_apply_path(const mfx_operator* op, int64_t p);
RbfGradPath rbf_grad_path(const mfx_operator* op, int64_t batch, bool have_hws);  // have_hws: the split-gradient region was carved

// ---- workspace regions: one layout function each, used by the size query and by the launcher ---------------------------------
// vscale region of rbf_carve (floats): [0, 2p) the vectors' scales [s, 1/s]; [2p, 3p) |max| bit patterns (in-kernel-split path);
// [3p] the f16 range flag; [3p + 64, ...) gx slice maxima per vector (pre-packed path).  ok = false: p vectors do not fit.
constexpr int64_t kRbfVscaleFloats = 65536 * 3;
constexpr int64_t kRbfVscaleMaxP = (kRbfVscaleFloats - 64) / 4;  // one slice per vector behind the scales and the flag
static_assert(kRbfVscaleMaxP == 49136, "the limit the error message of the split matvec states");
struct RbfVscaleLayout {
  int64_t scales, amax_bits, rangeflag, amax_part;  // offsets in floats
  int64_t gx;                                       // slices per vector of k_row_amax_part
  bool ok;
};
RbfVscaleLayout rbf_vscale_layout(int64_t n, int64_t p);

// pack region: the pre-packed f16 tile images of the split matvec -- probe images [chunks][ntile] at 0, column operands [ntile] at
// off_a -- and the partial sums of its nsplit column splits (leading dimension ldpart) at off_part
struct RbfPackLayout {
  int64_t P, chunks, ntile;  // vectors per chunk (chunk_width), chunks of the p vectors, 64-column tiles
  int64_t off_a, off_part;   // bytes
  int nsplit;
  int64_t ldpart, bytes;
};
RbfPackLayout rbf_pack_layout(int64_t n, int64_t nrow, int64_t p, int dpad);
int64_t rbf_pack_ws_bytes(const mfx_operator* op, int64_t p);  // 0: no pre-packed form (fp64, d > 32)

// split-gradient region: row maxima of L and R, the two operands' scales [sL, 1/sL, sR, 1/sR], the first one-product stage, the
// packed row order, then the hi / lo f16 packs of L (bpad x npad_l each) and R (bpad x npad each).  Offsets in bytes.
struct RbfGradHLayout {
  int64_t bpad, npad, npad_l;
  int64_t amaxL, amaxR, scl, tail, perm, Lh, Ll, Rh, Rl, bytes;
};
RbfGradHLayout rbf_grad_h_layout(int64_t n, int64_t nrow, int64_t batch);
inline int64_t rbf_grad_h_ws_bytes(int64_t n, int64_t batch) { return rbf_grad_h_layout(n, n, batch).bytes; }

// rows of (dpad + 2) doubles the matrix-core sweeps write into rbf_carve's gradient partials: one per workgroup
int64_t rbf_mfma_grad_partial_rows(int64_t n);

// ---- entry points of the matrix-core kernels (matvec: mfx_rbf_mfma.hip; parameter sweeps: mfx_rbf_mfma_grad.hip) --------------
int rbf_mfma_apply(const mfx_operator* op, const float* xs, const float* sq, int dpad, const float* x, int64_t ldx,
                   float* y, int64_t ldy, int64_t p, hipStream_t stream);
int rbf_mfma_apply_h3(const mfx_operator* op, const float* xs, const float* sq, int dpad, const float* x, int64_t ldx,
                      float* y, int64_t ldy, int64_t p, float* vscale, void* pk, hipStream_t stream);
int rbf_mfma_grad(const mfx_operator* op, const float* xs, const float* sq, int dpad, const float* L, int64_t ldl,
                  const float* R, int64_t ldr, int64_t batch, double* partial, int64_t* nblocks_out,
                  hipStream_t stream);
// returns the device pointer holding [sL, 1/sL, sR, 1/sR] through scales_out
int rbf_mfma_grad_h(const mfx_operator* op, const float* xs, const float* sq, int dpad, const float* L, int64_t ldl,
                    const float* R, int64_t ldr, int64_t batch, int64_t inner, double* partial, int64_t* nblocks_out, void* hws,
                    const float** scales_out, hipStream_t stream);

// What one launch of the split matvec kernels (k_rbf_h3_packed, k_rbf_h3_split, k_rbf_fat_apply) takes, in the kernels' parameter order;
// pkv / pka are the uintx4 tile images of the pack region
struct RbfMatvecArgs {
  const float *xs, *sq;
  int64_t n;
  const float *outputscale, *noise, *vscale, *x;
  int64_t ldx;
  float* y;
  int64_t ldy, p;
  const void *pkv, *pka;
  float* part;
  const int* rangeflag;
  int64_t ldpart, row0, rend;
};
// launcher of the fat-wave matvec kernels (mfx_rbf_fat.hip): RBF, d <= 16, chunks of nb * 32 vectors (nb = 1, 2);
// wide16: k_rbf_fat_apply16 (v_mfma_f32_16x16x32_f16) where it is built -- d <= 8 and nb = 2 --, k_rbf_fat_apply for every other shape;
// grid = (ceil(rows / 512), chunks, splits)
int rbf_fat_launch(int dpad, int nb, bool vec4, bool wide16, dim3 grid, hipStream_t stream, const RbfMatvecArgs& a);

}  // namespace mfx
