// Host-side argument checks of the f(A) v entry points (mfx_funm_coeffs, mfx_funm_coeffs_bwd, mfx_basis_combine,
// mfx_basis_combine_workspace_bytes, mfx_basis_combine_bwd) for the sanitizer build (`make -C experiments-lanczos-adjoints_amd/csrc asan`):
// every call below must be refused with its MFX_ERR_* code and a message BEFORE any launch, so the program needs no GPU.  Built with
// -fsanitize=address,undefined and linked against asan/libmfx_asan.so like cabi_host_checks.cpp; tests/test_funm_host.py runs it.
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

int main() {
  static double d[64];
  void* const x = d;
  char ws[256];

  // ---- mfx_funm_coeffs -------------------------------------------------------------------------------------------------------
  EXPECT(mfx_funm_coeffs(nullptr, x, x, x, 1, 4, MFX_F64, x, nullptr) == MFX_ERR_INVALID, "coeffs: null evals");
  EXPECT(mfx_funm_coeffs(x, nullptr, x, x, 1, 4, MFX_F64, x, nullptr) == MFX_ERR_INVALID, "coeffs: null evecs");
  EXPECT(mfx_funm_coeffs(x, x, nullptr, x, 1, 4, MFX_F64, x, nullptr) == MFX_ERR_INVALID, "coeffs: null fvals");
  EXPECT(mfx_funm_coeffs(x, x, x, nullptr, 1, 4, MFX_F64, x, nullptr) == MFX_ERR_INVALID, "coeffs: null scale");
  EXPECT(mfx_funm_coeffs(x, x, x, x, 1, 4, MFX_F64, nullptr, nullptr) == MFX_ERR_INVALID, "coeffs: null output");
  EXPECT(std::strlen(mfx_last_error()) > 0, "coeffs: message");
  EXPECT(mfx_funm_coeffs(x, x, x, x, 0, 4, MFX_F64, x, nullptr) == MFX_ERR_INVALID, "coeffs: p = 0");
  EXPECT(mfx_funm_coeffs(x, x, x, x, 1, 0, MFX_F32, x, nullptr) == MFX_ERR_INVALID, "coeffs: k = 0");
  EXPECT(mfx_funm_coeffs(x, x, x, x, 1, 2049, MFX_F64, x, nullptr) == MFX_ERR_UNSUPPORTED, "coeffs: k > 2048");
  EXPECT(mfx_funm_coeffs(x, x, x, x, 1, 4, 7, x, nullptr) == MFX_ERR_UNSUPPORTED, "coeffs: dtype");
  EXPECT(mfx_funm_coeffs(x, x, x, x, int64_t(1) << 31, 4, MFX_F64, x, nullptr) == MFX_ERR_UNSUPPORTED, "coeffs: p beyond the grid");

  // ---- mfx_funm_coeffs_bwd ---------------------------------------------------------------------------------------------------
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, x, nullptr, x, 1, 4, MFX_F64, x, x, 3, x, nullptr) == MFX_ERR_INVALID, "coeffs_bwd: null dcoeffs");
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, nullptr, x, x, 1, 4, MFX_F64, x, x, 3, x, nullptr) == MFX_ERR_INVALID, "coeffs_bwd: null dfvals");
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, x, x, nullptr, 1, 4, MFX_F64, x, x, 3, x, nullptr) == MFX_ERR_INVALID, "coeffs_bwd: null scale");
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, x, x, x, 1, 4, MFX_F64, nullptr, x, 3, x, nullptr) == MFX_ERR_INVALID, "coeffs_bwd: null dalpha");
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, x, x, x, 1, 4, MFX_F64, x, nullptr, 3, x, nullptr) == MFX_ERR_INVALID, "coeffs_bwd: null dbeta, k > 1");
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, x, x, x, 1, 4, MFX_F64, x, x, 2, x, nullptr) == MFX_ERR_INVALID, "coeffs_bwd: lddbeta < k - 1");
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, x, x, x, 0, 4, MFX_F32, x, x, 3, x, nullptr) == MFX_ERR_INVALID, "coeffs_bwd: p = 0");
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, x, x, x, 1, -1, MFX_F32, x, x, 3, x, nullptr) == MFX_ERR_INVALID, "coeffs_bwd: k < 1");
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, x, x, x, 1, 2049, MFX_F64, x, x, 2048, x, nullptr) == MFX_ERR_UNSUPPORTED, "coeffs_bwd: k > 2048");
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, x, x, x, 1, 4, -2, x, x, 3, x, nullptr) == MFX_ERR_UNSUPPORTED, "coeffs_bwd: dtype");
  EXPECT(mfx_funm_coeffs_bwd(x, x, x, x, x, x, int64_t(1) << 31, 4, MFX_F64, x, x, 3, x, nullptr) == MFX_ERR_UNSUPPORTED, "coeffs_bwd: p beyond the grid");

  // ---- mfx_basis_combine -----------------------------------------------------------------------------------------------------
  EXPECT(mfx_basis_combine(nullptr, x, 8, 2, 1, MFX_F64, x, nullptr) == MFX_ERR_INVALID, "combine: null Q");
  EXPECT(mfx_basis_combine(x, nullptr, 8, 2, 1, MFX_F64, x, nullptr) == MFX_ERR_INVALID, "combine: null coeffs");
  EXPECT(mfx_basis_combine(x, x, 8, 2, 1, MFX_F64, nullptr, nullptr) == MFX_ERR_INVALID, "combine: null y");
  EXPECT(mfx_basis_combine(x, x, 0, 2, 1, MFX_F64, x, nullptr) == MFX_ERR_INVALID, "combine: n = 0");
  EXPECT(mfx_basis_combine(x, x, 8, 0, 1, MFX_F32, x, nullptr) == MFX_ERR_INVALID, "combine: k = 0");
  EXPECT(mfx_basis_combine(x, x, 8, 2, 0, MFX_F32, x, nullptr) == MFX_ERR_INVALID, "combine: p = 0");
  EXPECT(mfx_basis_combine(x, x, 8, 2049, 1, MFX_F32, x, nullptr) == MFX_ERR_UNSUPPORTED, "combine: k > 2048");
  EXPECT(mfx_basis_combine(x, x, 8, 2, 65536, MFX_F32, x, nullptr) == MFX_ERR_UNSUPPORTED, "combine: p > 65535");
  EXPECT(mfx_basis_combine(x, x, 8, 2, 1, 3, x, nullptr) == MFX_ERR_UNSUPPORTED, "combine: dtype");

  // ---- workspace query: host arithmetic; one 256-byte unit per started 256 bytes of (p, k, slices) partials -----------------------
  EXPECT(mfx_basis_combine_workspace_bytes(1, 1, 1, MFX_F32) == 256, "query: smallest problem");
  EXPECT(mfx_basis_combine_workspace_bytes(513, 3, 2, MFX_F64) == 256, "query: two slices, 3 x 2 x 2 doubles");
  EXPECT(mfx_basis_combine_workspace_bytes(2000000, 30, 1, MFX_F64) == (int64_t)30 * 3907 * 8 / 256 * 256 + 256, "query: n = 2e6, k = 30");
  EXPECT(mfx_basis_combine_workspace_bytes(131072, 40, 64, MFX_F32) == (int64_t)64 * 40 * 256 * 4, "query: n = 131072, k = 40, p = 64");
  for (int dtype : {MFX_F32, MFX_F64})
    for (int64_t n : {int64_t(1), int64_t(511), int64_t(4099), int64_t(1) << 33})
      for (int64_t k : {int64_t(1), int64_t(33), int64_t(2048)})
        for (int64_t p : {int64_t(1), int64_t(3)}) {
          const int64_t w = mfx_basis_combine_workspace_bytes(n, k, p, dtype);
          EXPECT(w >= p * k * ((n + 511) / 512) * (dtype == MFX_F64 ? 8 : 4) && w % 256 == 0, "query covers the partials");
        }
  EXPECT(mfx_basis_combine_workspace_bytes(0, 2, 1, MFX_F32) == -1, "query: n = 0");
  EXPECT(mfx_basis_combine_workspace_bytes(8, 2049, 1, MFX_F32) == -1, "query: k > 2048");
  EXPECT(mfx_basis_combine_workspace_bytes(8, 2, 1, 5) == -1, "query: dtype");

  // ---- mfx_basis_combine_bwd -------------------------------------------------------------------------------------------------
  EXPECT(mfx_basis_combine_bwd(x, x, nullptr, 8, 2, 1, MFX_F64, x, x, ws, sizeof(ws), nullptr) == MFX_ERR_INVALID, "combine_bwd: null dy");
  EXPECT(mfx_basis_combine_bwd(x, x, x, 8, 2, 1, MFX_F64, nullptr, nullptr, ws, sizeof(ws), nullptr) == MFX_ERR_INVALID, "combine_bwd: no output");
  EXPECT(mfx_basis_combine_bwd(x, nullptr, x, 8, 2, 1, MFX_F64, x, nullptr, ws, sizeof(ws), nullptr) == MFX_ERR_INVALID, "combine_bwd: dQ without coeffs");
  EXPECT(mfx_basis_combine_bwd(nullptr, x, x, 8, 2, 1, MFX_F64, nullptr, x, ws, sizeof(ws), nullptr) == MFX_ERR_INVALID, "combine_bwd: dcoeffs without Q");
  EXPECT(mfx_basis_combine_bwd(x, x, x, 8, 0, 1, MFX_F64, x, x, ws, sizeof(ws), nullptr) == MFX_ERR_INVALID, "combine_bwd: k = 0");
  EXPECT(mfx_basis_combine_bwd(x, x, x, 8, 2, 1, 9, x, x, ws, sizeof(ws), nullptr) == MFX_ERR_UNSUPPORTED, "combine_bwd: dtype");
  EXPECT(mfx_basis_combine_bwd(x, x, x, 8, 2, 1, MFX_F64, x, x, ws, 255, nullptr) == MFX_ERR_WORKSPACE, "combine_bwd: workspace one byte short");
  EXPECT(mfx_basis_combine_bwd(x, x, x, 8, 2, 1, MFX_F64, x, x, nullptr, 256, nullptr) == MFX_ERR_WORKSPACE, "combine_bwd: null workspace");
  EXPECT(std::strlen(mfx_last_error()) > 0, "combine_bwd: message");

  std::printf(failures ? "cabi_funm_checks: %d FAILED\n" : "cabi_funm_checks ok\n", failures);
  return failures ? 1 : 0;
}
