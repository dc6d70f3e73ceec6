// Host-side refusals of the affine operator (MFX_OP_AFFINE, struct mfx_affine) for the sanitizer build
// (`make -C experiments-lanczos-adjoints_amd/csrc asan`): an affine descriptor around a dense 3 x 3 operator, and every fault of it
// refused with its MFX_ERR_* code BEFORE any launch, so the program needs no GPU (the pointers it passes are never dereferenced).
// Built with -fsanitize=address,undefined and linked against asan/libmfx_asan.so like cabi_host_checks.cpp.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "mfx.h"

static int failures = 0;
#define EXPECT(cond, what)                                                                          \
  do {                                                                                              \
    if (!(cond)) {                                                                                  \
      std::printf("FAIL %s:%d %s  [last error: %s]\n", __FILE__, __LINE__, what, mfx_last_error()); \
      ++failures;                                                                                   \
    }                                                                                               \
  } while (0)

static double d[64];
static void* const x = d;
static char ws[1 << 16];

static mfx_operator dense3() {
  mfx_operator op;
  std::memset(&op, 0, sizeof(op));
  op.kind = MFX_OP_DENSE;
  op.dtype = MFX_F64;
  op.n = 3;
  op.dense_a = x;
  op.lda = 3;
  return op;
}

static mfx_operator affine(const mfx_affine* af, int64_t n) {
  mfx_operator op;
  std::memset(&op, 0, sizeof(op));
  op.kind = MFX_OP_AFFINE;
  op.dtype = MFX_F64;
  op.n = n;
  op.ctx = const_cast<mfx_affine*>(af);
  return op;
}

// every entry the refusal has to come back from: both applications and the parameter sweep
static void refused(const mfx_operator& op, int code, const char* text, const char* what) {
  mfx_op_grads g;
  std::memset(&g, 0, sizeof(g));
  g.drift = x;
  EXPECT(mfx_op_apply(&op, x, op.n, x, op.n, 1, 0, ws, sizeof(ws), nullptr) == code && std::strstr(mfx_last_error(), text), what);
  EXPECT(mfx_op_apply(&op, x, op.n, x, op.n, 1, 1, ws, sizeof(ws), nullptr) == code && std::strstr(mfx_last_error(), text), what);
  EXPECT(mfx_op_vjp_params(&op, x, op.n, x, op.n, 1, &g, ws, sizeof(ws), nullptr) == code && std::strstr(mfx_last_error(), text), what);
  EXPECT(mfx_arnoldi_forward(&op, x, op.n, 2, 1, 1, x, x, x, x, ws, sizeof(ws), nullptr) == code && std::strstr(mfx_last_error(), text), what);
}

int main() {
  mfx_operator in = dense3();
  mfx_affine af = {&in, x};
  {
    mfx_operator op = affine(nullptr, 4);
    refused(op, MFX_ERR_INVALID, "ctx (the mfx_affine) is NULL", "null ctx");
  }
  {
    mfx_affine bad = {&in, nullptr};
    refused(affine(&bad, 4), MFX_ERR_INVALID, "af_b (the drift) is NULL", "null b");
    bad = {nullptr, x};
    refused(affine(&bad, 4), MFX_ERR_INVALID, "af_inner is NULL", "null inner");
  }
  for (int kind : {(int)MFX_OP_CALLBACK, (int)MFX_OP_PRECOND, (int)MFX_OP_AFFINE}) {
    mfx_operator other = dense3();
    other.kind = kind;
    mfx_affine bad = {&other, x};
    refused(affine(&bad, 4), MFX_ERR_INVALID, "neither preconditioned nor affine itself", "inner kind");
  }
  {
    mfx_operator broken = dense3();
    broken.dense_a = nullptr;
    mfx_affine bad = {&broken, x};
    refused(affine(&bad, 4), MFX_ERR_INVALID, "dense operator without matrix", "a fault of the inner operator");
    mfx_operator f32 = dense3();
    f32.dtype = MFX_F32;
    bad = {&f32, x};
    refused(affine(&bad, 4), MFX_ERR_INVALID, "inner operator 0", "inner dtype");
    mfx_operator block = dense3();
    block.nrows = 2;
    bad = {&block, x};
    refused(affine(&bad, 4), MFX_ERR_INVALID, "the inner operator must be whole", "inner row block");
  }
  for (int64_t n : {int64_t(3), int64_t(5)}) refused(affine(&af, n), MFX_ERR_INVALID, "the border of an inner operator of 3 unknowns has 4", "wrong n");
  {
    mfx_operator op = affine(&af, 4);
    op.nrows = 2;
    refused(op, MFX_ERR_UNSUPPORTED, "no row block (nrows > 0)", "row block");
  }
  {  // the drift gradient on another kind; the workspace of the valid descriptor is the inner operator's (no partial sums at m = 3)
    mfx_op_grads g;
    std::memset(&g, 0, sizeof(g));
    g.drift = x;
    EXPECT(mfx_op_vjp_params(&in, x, 3, x, 3, 1, &g, ws, sizeof(ws), nullptr) == MFX_ERR_INVALID, "drift gradient on a dense operator");
    mfx_operator op = affine(&af, 4);
    EXPECT(mfx_workspace_bytes(&op, 4, 1, 1) == mfx_workspace_bytes(&in, 4, 1, 1), "workspace of the valid descriptor");
  }
  if (failures) {
    std::printf("cabi_affine_checks: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("cabi_affine_checks ok\n");
  return 0;
}
