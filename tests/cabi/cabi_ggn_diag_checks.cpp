// Host-side argument checks of the exact GGN diagonal (mfx_ggn_diag_workspace_bytes, mfx_ggn_diag) for the sanitizer build
// (`make -C experiments-lanczos-adjoints_amd/csrc asan`): every call below must be refused with its MFX_ERR_* code and a message
// BEFORE any launch, so the program needs no GPU (the pointers it passes are never dereferenced).  Built with
// -fsanitize=address,undefined and linked against asan/libmfx_asan.so like cabi_jac_checks.cpp; tests/test_ggn_diag_host.py runs it.
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
static mfx_ggn_net good(int loss) {
  mfx_ggn_net net;
  std::memset(&net, 0, sizeof(net));
  net.nlayers = 3;
  net.loss = loss;
  net.nsamples = 65;
  const int w[4] = {3, 7, 5, 3};
  for (int l = 0; l < 4; ++l) net.width[l] = w[l];
  net.theta = x;
  for (int l = 0; l < 3; ++l) net.act[l] = x;
  for (int l = 1; l < 3; ++l) net.dact[l] = x;
  net.prob = loss == MFX_GGN_CROSS_ENTROPY ? x : nullptr;
  return net;
}

// the call refuses `net` with `dtype` with `code` and a message, and the query returns -1
static void refused(const mfx_ggn_net* net, int dtype, int code, const char* what) {
  EXPECT(mfx_ggn_diag(net, dtype, x, ws, sizeof(ws), nullptr) == code, what);
  EXPECT(std::strlen(mfx_last_error()) > 0, what);
  EXPECT(mfx_ggn_diag_workspace_bytes(net, dtype) == -1, what);
}

int main() {
  const int64_t P = 86;
  for (int loss : {MFX_GGN_CROSS_ENTROPY, MFX_GGN_MSE}) {
    mfx_ggn_net net = good(loss);

    // ---- the workspace query: host arithmetic; min(ceil(N / 32), 64) x P values, rounded up to 256 bytes ---------------------------
    EXPECT(mfx_ggn_diag_workspace_bytes(&net, MFX_F64) == (3 * P * 8 + 255) / 256 * 256, "query: three tiles, fp64");
    EXPECT(mfx_ggn_diag_workspace_bytes(&net, MFX_F32) == (3 * P * 4 + 255) / 256 * 256, "query: three tiles, fp32");
    net.nsamples = 1;
    EXPECT(mfx_ggn_diag_workspace_bytes(&net, MFX_F32) == (1 * P * 4 + 255) / 256 * 256, "query: one tile");
    net.nsamples = 64 * 32 + 1;
    EXPECT(mfx_ggn_diag_workspace_bytes(&net, MFX_F64) == (64 * P * 8 + 255) / 256 * 256, "query: 65 tiles, 64 workgroups");
    net.nsamples = 1000000;
    EXPECT(mfx_ggn_diag_workspace_bytes(&net, MFX_F64) == (64 * P * 8 + 255) / 256 * 256, "query: at most 64 workgroups");
    net = good(loss);

    // ---- the net ----------------------------------------------------------------------------------------------------------------
    refused(nullptr, MFX_F64, MFX_ERR_INVALID, "null net");
    net.theta = nullptr;
    refused(&net, MFX_F64, MFX_ERR_INVALID, "null theta");
    for (int l = 0; l < 3; ++l) {
      net = good(loss);
      net.act[l] = nullptr;
      refused(&net, MFX_F32, MFX_ERR_INVALID, "null act[l]");
    }
    for (int l = 1; l < 3; ++l) {
      net = good(loss);
      net.dact[l] = nullptr;
      refused(&net, MFX_F64, MFX_ERR_INVALID, "null dact[l]");
    }
    for (int nl : {0, -1, MFX_GGN_MAX_LAYERS + 1}) {
      net = good(loss);
      net.nlayers = nl;
      refused(&net, MFX_F64, MFX_ERR_INVALID, "nlayers out of range");
    }
    for (int l = 0; l < 4; ++l)
      for (int w : {0, -3}) {
        net = good(loss);
        net.width[l] = w;
        refused(&net, MFX_F64, MFX_ERR_INVALID, "a width below 1");
      }
    for (int64_t n : {int64_t(0), int64_t(-5)}) {
      net = good(loss);
      net.nsamples = n;
      refused(&net, MFX_F32, MFX_ERR_INVALID, "nsamples below 1");
    }
    for (int bad : {2, -1, 77}) {
      net = good(loss);
      net.loss = bad;
      refused(&net, MFX_F64, MFX_ERR_INVALID, "unknown loss");
      EXPECT(std::strstr(mfx_last_error(), "loss") != nullptr, "unknown loss: named");
    }
    // the limits of the kernel
    net = good(loss);
    net.width[0] = 65537;
    refused(&net, MFX_F64, MFX_ERR_UNSUPPORTED, "width[0] > 65536");
    EXPECT(mfx_ggn_diag(&net, MFX_F64, x, ws, sizeof(ws), nullptr) == MFX_ERR_UNSUPPORTED &&
               std::strstr(mfx_last_error(), "limit 65536") != nullptr,
           "width[0] > 65536: the limit is named");
    net.width[0] = 65536;  // the limit itself is taken: (65536 + 1) x 7 + 40 + 18 values per workgroup
    EXPECT(mfx_ggn_diag_workspace_bytes(&net, MFX_F32) == (3 * (int64_t(65537) * 7 + 58) * 4 + 255) / 256 * 256, "width[0] = 65536");
    for (int l = 1; l < 4; ++l) {
      net = good(loss);
      net.width[l] = 65;
      refused(&net, MFX_F32, MFX_ERR_UNSUPPORTED, "width[l] > 64");
      EXPECT(mfx_ggn_diag(&net, MFX_F32, x, ws, sizeof(ws), nullptr) == MFX_ERR_UNSUPPORTED &&
                 std::strstr(mfx_last_error(), "limit 64") != nullptr,
             "width[l] > 64: the limit is named");
    }
    net = good(loss);

    // ---- dtype ------------------------------------------------------------------------------------------------------------------
    for (int dtype : {2, -1, 7}) refused(&net, dtype, MFX_ERR_UNSUPPORTED, "unknown dtype");

    // ---- the arguments of the call ------------------------------------------------------------------------------------------------
    EXPECT(mfx_ggn_diag(&net, MFX_F64, nullptr, ws, sizeof(ws), nullptr) == MFX_ERR_INVALID, "null diag");
    EXPECT(std::strstr(mfx_last_error(), "diag is NULL") != nullptr, "null diag: named");
    const int64_t need = 3 * P * 8;  // the partial sums in fp64: the call needs these, the query rounds up
    EXPECT(mfx_ggn_diag(&net, MFX_F64, x, ws, need - 1, nullptr) == MFX_ERR_WORKSPACE, "workspace one byte short");
    EXPECT(mfx_ggn_diag(&net, MFX_F64, x, nullptr, sizeof(ws), nullptr) == MFX_ERR_WORKSPACE, "null workspace");
    EXPECT(std::strlen(mfx_last_error()) > 0, "workspace: message");
    EXPECT(mfx_ggn_diag_workspace_bytes(&net, MFX_F64) >= need, "query covers the call");
  }

  // ---- prob: read for cross-entropy only ---------------------------------------------------------------------------------------------
  mfx_ggn_net net = good(MFX_GGN_CROSS_ENTROPY);
  net.prob = nullptr;
  refused(&net, MFX_F64, MFX_ERR_INVALID, "null prob with cross-entropy");
  EXPECT(std::strstr(mfx_last_error(), "prob") != nullptr, "null prob: named");
  net = good(MFX_GGN_MSE);  // prob is NULL here
  EXPECT(mfx_ggn_diag_workspace_bytes(&net, MFX_F32) > 0, "mse: a NULL prob is accepted");
  EXPECT(mfx_ggn_diag(&net, MFX_F32, x, nullptr, 0, nullptr) == MFX_ERR_WORKSPACE, "mse: a NULL prob passes the checks of the net");

  std::printf(failures ? "cabi_ggn_diag_checks: %d FAILED\n" : "cabi_ggn_diag_checks ok\n", failures);
  return failures ? 1 : 0;
}
