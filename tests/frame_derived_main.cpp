// frame_derived_main.cpp — a stand-alone program over csrc/frame_derived.h for a host sanitizer build (tests/test_uniform_refill_host.py
// compiles it with g++ -fsanitize=address,undefined and runs the result).  The values the host puts into a batched launch's frame table
// must be, as bit patterns, what include/urt_math.h gives per lane for the same inputs:
//   * a0, a1 = the seed-only half of rand_next for _Seed and _Seed + 0.5, and with them rand_draw(a, px, py) == rand_next(seed, px, py)
//     and the carried seed == (_Seed + 0.5) + 0.5 — over seeds on both sides of f_div_const's range, zeros, infinities and a NaN;
//   * origin = mul_m4(c2w, 0, 0, 0, 1), also for matrices with infinities and NaNs in the columns that 0 multiplies.
// Exit status 0: all equal and the sanitizers saw nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../unityraytracer_amd/csrc/frame_derived.h"

namespace {

int g_failures = 0;
#define EXPECT(cond, what)                                                        \
  do {                                                                            \
    if (!(cond)) { std::printf("FAILED %s: %s (line %d)\n", what, #cond, __LINE__); g_failures++; } \
  } while (0)

bool same_bits(float a, float b) { return urt::f_bits(a) == urt::f_bits(b); }

// (seed + seed / 17) / 100 with the IEEE divider: what rand_scale must return wherever f_div_const is documented to agree with it
float scale_by_division(float seed) { return (seed + seed / 17.0f) / 100.0f; }

void check_seed(float seed) {
  char what[64];
  std::snprintf(what, sizeof what, "seed %.9g", (double)seed);
  float c2w[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0.25f, 1.0f, -10.0f, 1};
  const urtd::FrameDerived d = urtd::frame_derived(c2w, seed);
  EXPECT(same_bits(d.a0, scale_by_division(seed)), what);        // (f_div_const equals the divider for every float: tests/test_oracle_math.py)
  EXPECT(same_bits(d.a1, scale_by_division(seed + 0.5f)), what);
  const float pixels[][2] = {{0, 0}, {1, 0}, {0, 1}, {7, 130}, {95, 63}, {1919, 1079}, {65535, 65535}};
  for (const auto& p : pixels) {
    float s = seed;
    const float r0 = urt::rand_next(s, p[0], p[1]);
    const float r1 = urt::rand_next(s, p[0], p[1]);
    EXPECT(same_bits(urt::rand_draw(d.a0, p[0], p[1]), r0), what);
    EXPECT(same_bits(urt::rand_draw(d.a1, p[0], p[1]), r1), what);
    EXPECT(same_bits((seed + 0.5f) + 0.5f, s), what);
  }
}

void check_origin(const float* c2w, const char* what) {
  const urtd::FrameDerived d = urtd::frame_derived(c2w, 0.5f);
  const urt::v3 o = urt::mul_m4(c2w, 0.0f, 0.0f, 0.0f, 1.0f);
  EXPECT(same_bits(d.origin[0], o.x) && same_bits(d.origin[1], o.y) && same_bits(d.origin[2], o.z), what);
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const float seeds[] = {0.0f, -0.0f, 0.5f, 1.0f, 100.25f, 1e-31f, -1e-31f, 9.9e-31f, 1e-30f, 1.1e-30f, 1e-38f, 1e-45f, 3e38f, -3e38f, 3.3e38f,
                         0.12345678f, 0.99999994f, 16777216.0f, 1e5f, inf, -inf, std::numeric_limits<float>::quiet_NaN()};
  for (float s : seeds) check_seed(s);
  uint32_t x = 0x5EEDu;                                           // a few thousand seeds in [0, 1): what RM:778 draws
  for (int k = 0; k < 4096; k++) {
    x = x * 1664525u + 1013904223u;
    check_seed((float)(x >> 8) / 16777216.0f);
  }
  float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0, 0.0f, 1.0f, -10.0f, 1};
  check_origin(m, "Scene1's camera");
  m[12] = -0.0f; m[13] = 1e-45f; m[14] = 3e38f;
  check_origin(m, "signed zero, denormal, huge");
  m[0] = inf; m[5] = -inf; m[10] = std::numeric_limits<float>::quiet_NaN();
  check_origin(m, "inf and NaN in the rotation");
  if (g_failures) { std::printf("frame table: %d failures\n", g_failures); return 1; }
  std::printf("frame table: ok\n");
  return 0;
}
