// Stand-alone host check of sdhip_sgd_step's argument validation (tests/test_sgd.py builds it together with
// csrc/optim_loss.hip and csrc/runtime.hip under AddressSanitizer + UBSan and runs it; no GPU is needed: every call below
// must be refused before anything is launched).  Exit status 0 and a last line "ok" mean every case was refused with
// SDHIP_ERR_ARG and a message.
#include <stdio.h>
#include <string.h>

#include "sdhip.h"

static int failures = 0;

static void expect_refused(const char* what, int rc, const char* needle) {
  const char* msg = sdhip_last_error();
  const bool ok = rc == SDHIP_ERR_ARG && msg && strstr(msg, "sgd_step") && strstr(msg, needle);
  printf("%-28s rc %d  \"%s\"%s\n", what, rc, msg ? msg : "(null)", ok ? "" : "   <-- FAILED");
  if (!ok) ++failures;
}

int main() {
  // host memory stands in for device memory: the checks look at the pointer values only
  alignas(16) static float p[8], g[8], m[8], lr[1];
  alignas(16) static long live[4] = {0, 4, 4, 8};
  expect_refused("params NULL", sdhip_sgd_step(nullptr, g, m, lr, 8, 0.9f, 1e-4f, 1.f, nullptr, 0, nullptr), "null");
  expect_refused("grads NULL", sdhip_sgd_step(p, nullptr, m, lr, 8, 0.9f, 1e-4f, 1.f, nullptr, 0, nullptr), "null");
  expect_refused("momentum_buf NULL", sdhip_sgd_step(p, g, nullptr, lr, 8, 0.9f, 1e-4f, 1.f, nullptr, 0, nullptr), "null");
  expect_refused("lr NULL", sdhip_sgd_step(p, g, m, nullptr, 8, 0.9f, 1e-4f, 1.f, nullptr, 0, nullptr), "null");
  expect_refused("n == 0", sdhip_sgd_step(p, g, m, lr, 0, 0.9f, 1e-4f, 1.f, nullptr, 0, nullptr), "sizes");
  expect_refused("n_live < 0", sdhip_sgd_step(p, g, m, lr, 8, 0.9f, 1e-4f, 1.f, live, -1, nullptr), "sizes");
  expect_refused("n_live < 0, no table", sdhip_sgd_step(p, g, m, lr, 8, 0.9f, 1e-4f, 1.f, nullptr, -3, nullptr), "sizes");
  expect_refused("params misaligned", sdhip_sgd_step(p + 1, g, m, lr, 4, 0.9f, 1e-4f, 1.f, nullptr, 0, nullptr), "aligned");
  expect_refused("grads misaligned", sdhip_sgd_step(p, g + 2, m, lr, 4, 0.9f, 1e-4f, 1.f, nullptr, 0, nullptr), "aligned");
  expect_refused("momentum_buf misaligned", sdhip_sgd_step(p, g, m + 3, lr, 4, 0.9f, 1e-4f, 1.f, nullptr, 0, nullptr), "aligned");
  expect_refused("live misaligned", sdhip_sgd_step(p, g, m, lr, 8, 0.9f, 1e-4f, 1.f, (const long*)((const char*)live + 4), 1, nullptr), "aligned");
  if (failures) {
    printf("%d case(s) were not refused as expected\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
