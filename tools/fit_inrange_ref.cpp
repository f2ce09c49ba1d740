// fit_inrange_ref.cpp -- host restatement of the in-range fit's two chains (the-cooper-mapper_amd/csrc/lslam_device.hpp:
// div_inrange, sqrt_inrange) with fmaf, checked against `/` and sqrtf.  The device's v_rcp_f32 and v_sqrt_f32 are accurate to
// one ulp; here the seed is the correctly rounded value or either of its neighbours (`seed` = -1, 0, +1), and the chains must
// give the correctly rounded quotient and root for all three.  Build with -ffp-contract=off (tests/test_fit_inrange_ref.py does).
//
//   fit_inrange_ref random N SEED   N operand pairs inside the range, and N square-root operands    -> "mismatch <count>"
//   fit_inrange_ref edges           the range's edges and the zero numerators                        -> "checked <n> refused <m> mismatch <count>"
//   fit_inrange_ref guard           the guard predicate on operands at and just outside the limits   -> "guard <bits>"
//   fit_inrange_ref rcp5            the refined reciprocal of 5 for the three seeds, as hex words
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const float FIT_LO = 0x1p-30f, FIT_HI = 0x1p30f;

static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static float from_bits(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }
static float step(float x, int ulps) { return from_bits(bits(x) + (uint32_t)ulps); }  // x != 0, finite, same sign: |x| moves by ulps

static bool fit_inrange_ok(float a) { return std::fabs(a) >= FIT_LO && std::fabs(a) <= FIT_HI; }
// a denominator: in range, and its mantissa not all ones (over such a b a power of two's quotient lies 2^-25 above a tie, which
// the chain reaches from the correctly rounded seed only)
static bool fit_inrange_den_ok(float b) { return fit_inrange_ok(b) && (bits(b) | 0xff800000u) != 0xffffffffu; }

static float rcp_refined(float b, int seed) {
  const float r0 = step((float)(1.0 / (double)b), seed);  // (1 / b in double, rounded: the correctly rounded fp32 reciprocal)
  const float e = fmaf(-b, r0, 1.0f);
  return fmaf(e, r0, r0);
}
static float div_chain(float a, float b, float r) {
  float q = a * r;
  float e = fmaf(-b, q, a);
  q = fmaf(e, r, q);
  e = fmaf(-b, q, a);
  return fmaf(e, r, q);
}
static float sqrt_chain(float x, int seed) {
  float s = (float)std::sqrt((double)x);
  if (s != 0.0f) s = step(s, seed);
  const float sd = from_bits(bits(s) - 1u), su = from_bits(bits(s) + 1u);
  const float rd = fmaf(-sd, s, x), ru = fmaf(-su, s, x);
  float r = (0.0f >= rd) ? sd : s;
  r = (0.0f < ru) ? su : r;
  return r;
}

static uint64_t rng_state;
static uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}
// a float with a random sign and mantissa and an exponent uniform in [elo, ehi]; the top value of the range is FIT_HI itself
static float rnd_float(int elo, int ehi, bool sign) {
  const uint32_t e = (uint32_t)(elo + (int)(rnd() % (uint32_t)(ehi - elo + 1)) + 127);
  uint32_t m = rnd() & 0x7fffffu;
  return from_bits((sign && (rnd() & 1u) ? 0x80000000u : 0u) | (e << 23) | m);
}

static long check_div(float a, float b, bool verbose) {
  long bad = 0;
  const float want = a / b;
  for (int seed = -1; seed <= 1; ++seed) {
    const float got = div_chain(a, b, rcp_refined(b, seed));
    if (bits(got) != bits(want)) {
      ++bad;
      if (verbose) std::printf("div %a / %a seed %d: %a, want %a\n", a, b, seed, got, want);
    }
  }
  return bad;
}
static long check_sqrt(float x, bool verbose) {
  long bad = 0;
  const float want = sqrtf(x);
  for (int seed = -1; seed <= 1; ++seed) {
    const float got = sqrt_chain(x, seed);
    if (bits(got) != bits(want)) {
      ++bad;
      if (verbose) std::printf("sqrt %a seed %d: %a, want %a\n", x, seed, got, want);
    }
  }
  return bad;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "random") && argc == 4) {
    const long n = std::atol(argv[2]);
    rng_state = (uint64_t)std::atoll(argv[3]);
    long bad = 0;
    for (long i = 0; i < n; ++i) {
      float a = rnd_float(-30, 29, true), b = rnd_float(-30, 29, true);
      if (!fit_inrange_ok(a)) { ++bad; continue; }
      if (!fit_inrange_den_ok(b)) continue;  // (mantissa all ones: one draw in 2^23)
      bad += check_div(a, b, bad < 10);
      // the square root's range is its own: 2^-96 <= x < inf
      bad += check_sqrt(rnd_float(-96, 127, false), bad < 10);
    }
    std::printf("mismatch %ld\n", bad);
    return 0;
  }
  if (!std::strcmp(argv[1], "edges")) {
    // both limits' exponents and their neighbours inside, mantissas all zero and all ones (the top: FIT_HI itself, one value)
    std::vector<float> v;
    for (int e : {-30, -29, -1, 0, 1, 28, 29})
      for (uint32_t m : {0u, 1u, 0x400000u, 0x7ffffeu, 0x7fffffu})
        for (uint32_t s : {0u, 0x80000000u}) v.push_back(from_bits(s | ((uint32_t)(e + 127) << 23) | m));
    v.push_back(FIT_HI);
    v.push_back(-FIT_HI);
    long bad = 0, n = 0, refused = 0;
    for (float a : v)
      for (float b : v) {
        if (!fit_inrange_ok(a)) { ++bad; continue; }
        if (!fit_inrange_den_ok(b)) { ++refused; continue; }  // (the all-ones mantissas)
        bad += check_div(a, b, bad < 10); ++n;
      }
    for (float b : v) {  // zero numerators: +0 over either sign, -0 over a negative denominator
      if (!fit_inrange_den_ok(b)) continue;
      bad += check_div(0.0f, b, bad < 10); ++n;
      if (b < 0.0f) { bad += check_div(-0.0f, b, bad < 10); ++n; }
    }
    for (int e : {-96, -95, -31, -30, 0, 1, 59, 60, 126, 127})
      for (uint32_t m : {0u, 1u, 0x400000u, 0x7ffffeu, 0x7fffffu}) { bad += check_sqrt(from_bits(((uint32_t)(e + 127) << 23) | m), bad < 10); ++n; }
    bad += check_sqrt(0.0f, bad < 10); ++n;
    std::printf("checked %ld refused %ld mismatch %ld\n", n, refused, bad);
    return 0;
  }
  if (!std::strcmp(argv[1], "guard")) {
    // in: the limits themselves; out: one ulp outside, zero, -0, infinity, NaN, a denormal
    const float in[] = {FIT_LO, -FIT_LO, FIT_HI, -FIT_HI, 1.0f};
    const float out[] = {step(FIT_LO, -1), -step(FIT_LO, -1), step(FIT_HI, 1), -step(FIT_HI, 1), 0.0f, -0.0f, INFINITY, -INFINITY, NAN, 0x1p-140f};
    std::printf("guard");
    for (float x : in) std::printf(" %d", fit_inrange_ok(x) ? 1 : 0);
    std::printf(" |");
    for (float x : out) std::printf(" %d", fit_inrange_ok(x) ? 1 : 0);
    std::printf(" |");  // denominators: 1.5 passes, the all-ones mantissas do not
    for (float x : {1.5f, 0x1.fffffep0f, -0x1.fffffep-7f}) std::printf(" %d", fit_inrange_den_ok(x) ? 1 : 0);
    std::printf("\n");
    return 0;
  }
  if (!std::strcmp(argv[1], "rcp5")) {
    std::printf("rcp5");
    for (int seed = -1; seed <= 1; ++seed) std::printf(" %08x", bits(rcp_refined(5.0f, seed)));
    std::printf("\n");
    return 0;
  }
  return 2;
}
