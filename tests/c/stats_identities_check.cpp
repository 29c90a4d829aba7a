// Two identities the packed statistics pass (fognetsimpp_amd/csrc/replay_common.h,
// stats_accumulate_packed) relies on, restated in plain C++ and set against the formulas
// every other statistics pass keeps (simtime_to_int64, qtime_raw, hist_bin_raw).  Host only:
// build with -ffp-contract=off (each double operation separately rounded, as mul_rn / add_rn).
//
//  A. hist_bin_raw from the double at hand.  The pass has f = floor(x + 0.5), an integral
//     double with |f| < 2^63, and raw = (int64_t)f.  Then (double)raw == f, so the bin of
//     f * 1e-12 is the bin of (double)raw * 1e-12.
//  B. queueStartTime without the range test.  For a tick a in [0, kMaxTick = 2^61] the
//     round trip x = 1e12 * ((double)a * 1e-12) has |floor(x + 0.5)| < 2^63: simtime_to_int64
//     succeeds and the unchecked conversion returns the same value.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace {

constexpr int kHistBins = 64;  // FOGNET_HIST_BINS
constexpr int64_t kMaxTick = (int64_t)1 << 61;
constexpr double kTwo63 = 9223372036854775808.0;

// ---- the existing formulas
bool simtime_to_int64(double x, int64_t& out) {
  const double f = std::floor(x + 0.5);
  const bool ok = std::fabs(f) < kTwo63;
  out = ok ? (int64_t)f : 0;
  return ok;
}
double simtime_dbl(int64_t t) { return (double)t * 1e-12; }
int hist_bin_raw(int64_t raw) {
  const double v = simtime_dbl(raw);
  if (!(v >= 1.0)) return 0;
  int b;
  (void)std::frexp(v, &b);
  return b > kHistBins - 1 ? kHistBins - 1 : b;
}

// ---- the new helpers
int64_t simtime_to_int64_inrange(double x) { return (int64_t)std::floor(x + 0.5); }
int hist_bin_raw_f(double f) {
  const double v = f * 1e-12;
  if (!(v >= 1.0)) return 0;
  int b;
  (void)std::frexp(v, &b);
  return b > kHistBins - 1 ? kHistBins - 1 : b;
}

long failures = 0;
unsigned long long checked_a = 0, checked_b = 0;

void fail(const char* what, double f, int64_t a) {
  if (failures++ < 20) std::printf("FAIL %s: f=%a a=%" PRId64 "\n", what, f, a);
}

// A: f integral, |f| < 2^63
void check_f(double f) {
  if (!(std::fabs(f) < kTwo63) || f != std::floor(f)) return;  // not a value the pass can hold
  ++checked_a;
  const int64_t raw = (int64_t)f;
  if ((double)raw != f) fail("(double)(int64_t)f != f", f, raw);
  if (hist_bin_raw_f(f) != hist_bin_raw(raw)) fail("bin from f != bin from raw", f, raw);
}

// B: a in [0, kMaxTick]
void check_a(int64_t a) {
  if (a < 0 || a > kMaxTick) return;
  ++checked_b;
  const double x = 1e12 * simtime_dbl(a);
  int64_t want;
  const bool ok = simtime_to_int64(x, want);
  if (!ok) fail("simtime_to_int64 refuses an in-range tick", x, a);
  if (simtime_to_int64_inrange(x) != want) fail("unchecked conversion differs", x, a);
}

struct Rng {  // xorshift64*
  uint64_t s;
  uint64_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  }
};

}  // namespace

int main() {
  // every power of two and its neighbours (as integers where they are exact, and as the
  // adjacent doubles, which are integral from 2^52 on), both signs
  for (int k = 0; k <= 63; ++k) {
    const double p = std::ldexp(1.0, k);
    const double around[] = {p, p - 1.0, p + 1.0, p - 2.0, p + 2.0, std::nextafter(p, 0.0), std::nextafter(p, 2.0 * p)};
    for (double f : around) {
      check_f(f);
      check_f(-f);
    }
    if (k <= 61) {
      const int64_t a = (int64_t)1 << k;
      for (int64_t d = -2; d <= 2; ++d) check_a(a + d);
    }
  }
  check_f(0.0);
  for (int64_t d = -2; d <= 2; ++d) {
    check_f((double)(((int64_t)1 << 53) + d));
    check_f((double)(-((int64_t)1 << 53) + d));
  }
  // both ends of the tick range
  for (int64_t d = 0; d <= 4; ++d) {
    check_a(d);
    check_a(kMaxTick - d);
  }
  // 10^8 seeded random values each: every magnitude (a random shift), both signs
  Rng rng{0x5EED0009C0FFEEull};
  for (long i = 0; i < 100000000L; ++i) {
    const uint64_t u = rng.next();
    const int sh = (int)(rng.s >> 58);  // 0..63
    const int64_t m = (int64_t)(u >> 1) >> (sh % 63);
    check_f((double)((u & 1u) ? -m : m));
    check_a((int64_t)((u >> 3) >> (sh % 61)));  // (u >> 3 < 2^61: always inside the range)
  }
  std::printf("checked %llu integral doubles, %llu ticks\n", checked_a, checked_b);
  if (checked_a < 100000000ull || checked_b < 100000000ull) {
    std::printf("FAIL: too few values reached the checks\n");
    return 1;
  }
  if (failures) {
    std::printf("stats identities: %ld failures\n", failures);
    return 1;
  }
  std::printf("stats identities: all checks passed\n");
  return 0;
}
