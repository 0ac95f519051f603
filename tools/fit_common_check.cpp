// Host-only check of csrc/fit_common.h's carving and argument checks, for a sanitizer build; no device is
// touched (ws_get and fail are stubs, and nothing here reaches a HIP call).
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tools/fit_common_check.cpp -o build/fit_common_check
//   build/fit_common_check        # prints "fit_common_check: N checks passed", exit status 0
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../mmla_audio_amd/csrc/fit_common.h"

namespace mmla {

// the slot is a host allocation of exactly the bytes asked for: a carve past it is an ASan report
static char* g_slot = nullptr;
static size_t g_slot_bytes = 0;
static int g_ws_fail = 0;

int ws_get(mmla_ctx* c, int slot, size_t bytes, void** out) {
  if (g_ws_fail) return fail(c, MMLA_E_OOM, "slot %d: no memory (stub)", slot);
  std::free(g_slot);
  g_slot = static_cast<char*>(std::malloc(bytes ? bytes : 1));
  g_slot_bytes = bytes;
  *out = g_slot;
  return MMLA_OK;
}

int fail(mmla_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

}  // namespace mmla

using namespace mmla;

static int g_checks = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    ++g_checks;                                                             \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

static bool has(const mmla_ctx& c, const char* text) { return c.err.find(text) != std::string::npos; }

int main() {
  mmla_ctx c;

  // ---- Carver: a null base measures; pieces are 256-byte multiples
  Carver m{nullptr};
  EXPECT(m.take<uint8_t>(1) == nullptr && m.total == 256);
  EXPECT(m.take<float>(64) == nullptr && m.total == 512);
  EXPECT(m.take<float>(65) == nullptr && m.total == 1024);
  EXPECT(m.take<double>(0) == nullptr && m.total == 1024);

  // ---- carve_slot: both passes agree; every piece is inside the slot and writable, none overlaps
  float* a = nullptr;
  int32_t* b = nullptr;
  uint8_t* z = nullptr;
  double* d = nullptr;
  int passes = 0;
  auto three = [&](Carver& cv) -> int {
    ++passes;
    a = cv.take<float>(100);
    b = cv.take<int32_t>(1);
    z = cv.take<uint8_t>(0);
    d = cv.take<double>(33);
    return MMLA_OK;
  };
  EXPECT(carve_slot(&c, 3, three) == MMLA_OK && passes == 2);
  EXPECT(g_slot_bytes == 512 + 256 + 512);
  EXPECT((char*)a == g_slot && (char*)b == g_slot + 512 && (char*)z == g_slot + 768 && (char*)d == g_slot + 768);
  std::memset(a, 1, 100 * sizeof(float));
  std::memset(b, 2, sizeof(int32_t));
  std::memset(d, 3, 33 * sizeof(double));
  EXPECT(((uint8_t*)a)[399] == 1 && ((uint8_t*)b)[0] == 2 && ((uint8_t*)d)[0] == 3);

  // ---- the mismatch check: a take in one pass only, either way round
  auto more_later = [&](Carver& cv) -> int {
    cv.take<float>(10);
    if (cv.base) cv.take<float>(10);
    return MMLA_OK;
  };
  c.err.clear();
  EXPECT(carve_slot(&c, 4, more_later) == MMLA_E_HIP && has(c, "carved 512 bytes of the 256 measured"));
  auto less_later = [&](Carver& cv) -> int {
    cv.take<float>(10);
    if (!cv.base) cv.take<float>(1000);
    return MMLA_OK;
  };
  c.err.clear();
  EXPECT(carve_slot(&c, 4, less_later) == MMLA_E_HIP && has(c, "workspace slot 4"));
  // an error of either pass, or of the allocation, comes back as it is
  auto failing = [&](Carver& cv) -> int { return cv.base ? fail(&c, MMLA_E_INVALID, "second pass") : MMLA_OK; };
  EXPECT(carve_slot(&c, 4, failing) == MMLA_E_INVALID && has(c, "second pass"));
  g_ws_fail = 1;
  passes = 0;
  EXPECT(carve_slot(&c, 4, three) == MMLA_E_OOM && passes == 1);
  g_ws_fail = 0;

  // ---- Stager: what passes through takes nothing (the copies would reach HIP: not here)
  {
    Stager dev{&c, true}, host{&c, false};
    Carver cv{nullptr};
    const int32_t user[4] = {0, 1, 2, 3};
    const int32_t* got = nullptr;
    EXPECT(dev.in(cv, user, 4, &got) == MMLA_OK && got == user && cv.total == 0);
    EXPECT(host.in(cv, (const int32_t*)nullptr, 4, &got) == MMLA_OK && got == nullptr && cv.total == 0);
    EXPECT(host.in(cv, user, 0, &got) == MMLA_OK && got == user && cv.total == 0);
    EXPECT(host.in(cv, user, 4, &got) == MMLA_OK && got == nullptr && cv.total == 256);   // measured, no copy yet
    float o[2];
    EXPECT(dev.out(cv, o, 2) == o && cv.total == 256);
    EXPECT(host.out(cv, (float*)nullptr, 2) == nullptr && cv.total == 256);
    EXPECT(host.out(cv, o, 2) == nullptr && cv.total == 512);
    EXPECT(dev.back(o, o, 2) == MMLA_OK && host.back((float*)nullptr, o, 2) == MMLA_OK && host.back(o, o, 0) == MMLA_OK);
  }

  // ---- check_perm
  const int32_t good[6] = {2, 0, 1, 0, 1, 2};
  EXPECT(check_perm(&c, "t", good, 2, 3) == MMLA_OK && bad_perm_row(good, 2, 3) == -1);
  const int32_t twice[6] = {2, 0, 1, 0, 1, 1};
  c.err.clear();
  EXPECT(check_perm(&c, "t", twice, 2, 3) == MMLA_E_INVALID && has(c, "t: perm row 1 is not a permutation of 0..2"));
  EXPECT(check_perm(&c, "t", twice, 1, 3) == MMLA_OK);
  const int32_t negative[3] = {0, -1, 2}, large[3] = {0, 3, 2}, huge[3] = {0, INT32_MAX, INT32_MIN};
  EXPECT(bad_perm_row(negative, 1, 3) == 0 && bad_perm_row(large, 1, 3) == 0 && bad_perm_row(huge, 1, 3) == 0);
  EXPECT(check_perm(&c, "t", nullptr, 0, 3) == MMLA_OK);    // rows = 0: perm is not read
  EXPECT(check_perm(&c, "t", nullptr, 5, 0) == MMLA_OK);    // n = 0: neither
  EXPECT(check_perm(&c, "t", nullptr, 0, 0) == MMLA_OK);
  const int32_t one[1] = {0}, not_one[1] = {1};
  EXPECT(check_perm(&c, "t", one, 1, 1) == MMLA_OK && check_perm(&c, "t", not_one, 1, 1) == MMLA_E_INVALID);

  // ---- check_labels
  const int32_t labels[4] = {0, 2, 1, 2};
  EXPECT(check_labels(&c, "labels", labels, 4, 3) == MMLA_OK);
  c.err.clear();
  EXPECT(check_labels(&c, "labels", labels, 4, 2) == MMLA_E_INVALID && has(c, "labels[1] = 2 outside [0, 2)"));
  c.err.clear();
  EXPECT(check_labels(&c, "val_labels", labels, 4, 2, "{0, 1}") == MMLA_E_INVALID &&
         has(c, "val_labels[1] = 2 outside {0, 1}"));
  EXPECT(check_labels(&c, "labels", negative, 3, 3) == MMLA_E_INVALID && has(c, "labels[1] = -1"));
  EXPECT(check_labels(&c, "labels", nullptr, 0, 3) == MMLA_OK);   // n = 0: l is not read
  EXPECT(check_labels(&c, "labels", labels, 1, 1) == MMLA_OK && check_labels(&c, "labels", labels, 2, 1) == MMLA_E_INVALID);

  std::free(g_slot);
  std::printf("fit_common_check: %d checks passed\n", g_checks);
  return 0;
}
