// Host check of sfrt_math::sqrt_select (sfrt_math.h), the selection that sfrt_device.h
// sqrt_cr_normal applies to v_sqrt_f32's result: for r set to the correctly rounded root
// (the host's sqrtf) and to each of its two neighbours, the selection returns the bits of the
// correctly rounded root, for
//   - every significand at one even and one odd exponent (x in [1, 2) and [2, 4)),
//   - the first and last 2^16 patterns of every binade from 2^-96 up to the largest finite,
//   - x = +0 with r = +0 (what v_sqrt_f32 returns) and with r = the least denormal: +0.
// Built and run by tests/test_sqrt_select.py:
//   g++ -O2 -std=c++17 -ffp-contract=off -I sfml-software-raytracer_amd/csrc sqrt_select_host_check.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "sfrt_math.h"

static unsigned long long g_cases = 0, g_bad = 0;

static void check(uint32_t xb) {
  const float x = sfrt_math::u2f(xb);
  const uint32_t want = sfrt_math::f2u(std::sqrt(x));
  for (int d = -1; d <= 1; d++) {
    const uint32_t got = sfrt_math::f2u(sfrt_math::sqrt_select(x, sfrt_math::u2f(want + (uint32_t)d)));
    g_cases++;
    if (got != want) {
      if (g_bad++ < 8) std::printf("x=0x%08x r=root%+d: 0x%08x, want 0x%08x\n", xb, d, got, want);
    }
  }
}

int main() {
  for (uint32_t m = 0; m < (1u << 23); m++) {
    check(0x3f800000u | m);  // 2^0: even exponent
    check(0x40000000u | m);  // 2^1: odd exponent
  }
  for (uint32_t e = 127u - 96u; e <= 254u; e++)
    for (uint32_t m = 0; m < (1u << 16); m++) {
      check((e << 23) | m);
      check((e << 23) | (0x007fffffu - m));
    }
  for (uint32_t rb : {0u, 1u}) {
    const uint32_t got = sfrt_math::f2u(sfrt_math::sqrt_select(0.0f, sfrt_math::u2f(rb)));
    g_cases++;
    if (got != 0u) {
      g_bad++;
      std::printf("x=+0 r=0x%08x: 0x%08x, want +0\n", rb, got);
    }
  }
  std::printf("cases=%llu mismatches=%llu\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
