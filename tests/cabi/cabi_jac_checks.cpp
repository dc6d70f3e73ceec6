// Host-side argument checks of the MLP Jacobian entry points (mfx_mlp_jac_workspace_bytes, mfx_mlp_jac_apply, mfx_mlp_jac_t_apply) for
// the sanitizer build (`make -C experiments-lanczos-adjoints_amd/csrc asan`): every call below must be refused with its MFX_ERR_* code
// and a message BEFORE any launch, so the program needs no GPU (the pointers it passes are never dereferenced).  Built with
// -fsanitize=address,undefined and linked against asan/libmfx_asan.so like cabi_funm_checks.cpp; tests/test_mlp_jac_host.py runs it.
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

// widths (3, 7, 5, 3): P = 86; N = 65 is three tiles of 32 samples
static mfx_ggn_net good() {
  mfx_ggn_net net;
  std::memset(&net, 0, sizeof(net));
  net.nlayers = 3;
  net.loss = 77;  // not read: any value is accepted
  net.nsamples = 65;
  const int w[4] = {3, 7, 5, 3};
  for (int l = 0; l < 4; ++l) net.width[l] = w[l];
  net.theta = x;
  for (int l = 0; l < 3; ++l) net.act[l] = x;
  for (int l = 1; l < 3; ++l) net.dact[l] = x;
  net.prob = nullptr;  // not read either
  return net;
}

// all three entry points refuse `net` (with dtype and p) with `code`
static void refused(const mfx_ggn_net* net, int dtype, int64_t p, int code, const char* what) {
  EXPECT(mfx_mlp_jac_apply(net, dtype, x, 86, p, x, nullptr) == code, what);
  EXPECT(std::strlen(mfx_last_error()) > 0, what);
  EXPECT(mfx_mlp_jac_t_apply(net, dtype, x, p, x, 86, ws, sizeof(ws), nullptr) == code, what);
  EXPECT(std::strlen(mfx_last_error()) > 0, what);
  EXPECT(mfx_mlp_jac_workspace_bytes(net, dtype, p) == -1, what);
}

int main() {
  const int64_t P = 86;
  mfx_ggn_net net = good();

  // ---- the workspace query: host arithmetic; workgroups x p x P values, rounded up to 256 bytes ------------------------------------
  EXPECT(mfx_mlp_jac_workspace_bytes(&net, MFX_F64, 3) == (3 * 3 * P * 8 + 255) / 256 * 256, "query: three tiles, fp64");
  EXPECT(mfx_mlp_jac_workspace_bytes(&net, MFX_F32, 1) == (3 * 1 * P * 4 + 255) / 256 * 256, "query: three tiles, fp32");
  net.nsamples = 1000000;
  EXPECT(mfx_mlp_jac_workspace_bytes(&net, MFX_F64, 5) == (64 * 5 * P * 8 + 255) / 256 * 256, "query: at most 64 workgroups");
  net = good();

  // ---- the net ------------------------------------------------------------------------------------------------------------------
  refused(nullptr, MFX_F64, 1, MFX_ERR_INVALID, "null net");
  net.theta = nullptr;
  refused(&net, MFX_F64, 1, MFX_ERR_INVALID, "null theta");
  for (int l = 0; l < 3; ++l) {
    net = good();
    net.act[l] = nullptr;
    refused(&net, MFX_F32, 1, MFX_ERR_INVALID, "null act[l]");
  }
  for (int l = 1; l < 3; ++l) {
    net = good();
    net.dact[l] = nullptr;
    refused(&net, MFX_F64, 1, MFX_ERR_INVALID, "null dact[l]");
  }
  for (int nl : {0, -1, MFX_GGN_MAX_LAYERS + 1}) {
    net = good();
    net.nlayers = nl;
    refused(&net, MFX_F64, 1, MFX_ERR_INVALID, "nlayers out of range");
  }
  for (int l = 0; l < 4; ++l)
    for (int w : {0, -3}) {
      net = good();
      net.width[l] = w;
      refused(&net, MFX_F64, 1, MFX_ERR_INVALID, "a width below 1");
    }
  for (int64_t n : {int64_t(0), int64_t(-5)}) {
    net = good();
    net.nsamples = n;
    refused(&net, MFX_F32, 1, MFX_ERR_INVALID, "nsamples below 1");
  }
  // the limits of the kernels
  net = good();
  net.width[0] = 65537;
  EXPECT(mfx_mlp_jac_apply(&net, MFX_F64, x, int64_t(1) << 40, 1, x, nullptr) == MFX_ERR_UNSUPPORTED, "width[0] > 65536");
  EXPECT(std::strstr(mfx_last_error(), "limit 65536") != nullptr, "width[0] > 65536: the limit is named");
  EXPECT(mfx_mlp_jac_t_apply(&net, MFX_F64, x, 1, x, int64_t(1) << 40, ws, sizeof(ws), nullptr) == MFX_ERR_UNSUPPORTED, "width[0] > 65536");
  EXPECT(mfx_mlp_jac_workspace_bytes(&net, MFX_F64, 1) == -1, "width[0] > 65536");
  for (int l = 1; l < 4; ++l) {
    net = good();
    net.width[l] = 65;
    EXPECT(mfx_mlp_jac_apply(&net, MFX_F32, x, int64_t(1) << 40, 1, x, nullptr) == MFX_ERR_UNSUPPORTED, "width[l] > 64");
    EXPECT(std::strstr(mfx_last_error(), "limit 64") != nullptr, "width[l] > 64: the limit is named");
    EXPECT(mfx_mlp_jac_t_apply(&net, MFX_F32, x, 1, x, int64_t(1) << 40, ws, sizeof(ws), nullptr) == MFX_ERR_UNSUPPORTED, "width[l] > 64");
    EXPECT(mfx_mlp_jac_workspace_bytes(&net, MFX_F32, 1) == -1, "width[l] > 64");
  }
  net = good();

  // ---- dtype and p ----------------------------------------------------------------------------------------------------------------
  for (int dtype : {2, -1, 7}) refused(&net, dtype, 1, MFX_ERR_UNSUPPORTED, "unknown dtype");
  for (int64_t p : {int64_t(0), int64_t(-1)}) refused(&net, MFX_F64, p, MFX_ERR_INVALID, "p < 1");
  for (int64_t p : {int64_t(65536), int64_t(1) << 31}) refused(&net, MFX_F32, p, MFX_ERR_UNSUPPORTED, "p > 65535");

  // ---- the arguments of each call ----------------------------------------------------------------------------------------------------
  EXPECT(mfx_mlp_jac_apply(&net, MFX_F64, nullptr, P, 1, x, nullptr) == MFX_ERR_INVALID, "apply: null V");
  EXPECT(mfx_mlp_jac_apply(&net, MFX_F64, x, P, 1, nullptr, nullptr) == MFX_ERR_INVALID, "apply: null out");
  EXPECT(mfx_mlp_jac_apply(&net, MFX_F64, x, P - 1, 1, x, nullptr) == MFX_ERR_INVALID, "apply: ldv < P");
  EXPECT(std::strstr(mfx_last_error(), "ldv") != nullptr, "apply: ldv named");
  EXPECT(mfx_mlp_jac_t_apply(&net, MFX_F64, nullptr, 1, x, P, ws, sizeof(ws), nullptr) == MFX_ERR_INVALID, "t_apply: null U");
  EXPECT(mfx_mlp_jac_t_apply(&net, MFX_F64, x, 1, nullptr, P, ws, sizeof(ws), nullptr) == MFX_ERR_INVALID, "t_apply: null Y");
  EXPECT(mfx_mlp_jac_t_apply(&net, MFX_F64, x, 1, x, P - 1, ws, sizeof(ws), nullptr) == MFX_ERR_INVALID, "t_apply: ldy < P");
  EXPECT(std::strstr(mfx_last_error(), "ldy") != nullptr, "t_apply: ldy named");
  const int64_t need = 3 * 2 * P * 8;  // the partial sums of p = 2 in fp64: the call needs these, the query rounds up
  EXPECT(mfx_mlp_jac_t_apply(&net, MFX_F64, x, 2, x, P, ws, need - 1, nullptr) == MFX_ERR_WORKSPACE, "t_apply: workspace one byte short");
  EXPECT(mfx_mlp_jac_t_apply(&net, MFX_F64, x, 2, x, P, nullptr, sizeof(ws), nullptr) == MFX_ERR_WORKSPACE, "t_apply: null workspace");
  EXPECT(std::strlen(mfx_last_error()) > 0, "t_apply: message");
  EXPECT(mfx_mlp_jac_workspace_bytes(&net, MFX_F64, 2) >= need, "query covers the call");

  std::printf(failures ? "cabi_jac_checks: %d FAILED\n" : "cabi_jac_checks ok\n", failures);
  return failures ? 1 : 0;
}
