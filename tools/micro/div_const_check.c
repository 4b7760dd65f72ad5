/* Host check of div_const (csrc/usv_device.hpp): for each compile-time divisor c of the f64 build,
 * q = RN(x y) with y = RN(1 / c), r = x - q c (one fma, exact), and RN(q + r y), or q itself where r is
 * zero or not a number, must equal the IEEE quotient x / c bit for bit:
 *   - random operands with random sign, mantissa and exponent in [-960, 960];
 *   - +-0, +-inf and NaN (the sign of a zero quotient and the special values are the quotient's).
 * Below 2^-960 the residual x - q c is itself subnormal and no longer exact: it is off by up to one
 * subnormal spacing (2^-1074), which the correction multiplies by y.  For subnormal and tiny operands
 * (exponent field 0 .. 62) the result is checked to lie within (1 + y) 2^-1074 plus one ulp of x / c,
 * with the sign of a zero result equal; how many differ at all is printed.
 *   gcc -O2 -ffp-contract=off -o div_const_check div_const_check.c -lm && ./div_const_check [samples per divisor]
 * Exit status 0 iff no mismatch. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t s = 88172645463325252ull;
static uint64_t xr(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

/* the device function, restated */
static double div_const(double x, double c) {
  const double y = 1.0 / c;
  const double q = x * y;
  const double r = fma(-q, c, x);
  return fabs(r) > 0.0 ? fma(r, y, q) : q;
}

static int same(double a, double b) { return (isnan(a) && isnan(b)) || memcmp(&a, &b, 8) == 0; }

static double operand(int exp_lo, int exp_span) {   /* random sign and mantissa, biased exponent in [lo, lo + span) */
  uint64_t bits = xr();
  bits = (bits & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(exp_lo + (int)(xr() % (uint64_t)exp_span)) << 52);
  double x;
  memcpy(&x, &bits, 8);
  return x;
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 10000000L;
  volatile double iz = 4.1, nrd = -2.79, m = 30.0, xud = -2.25, b = 0.41, cth = 0.78;
  const double cs[] = {0.01, m - xud, iz - nrd, b, 2 * cth, b * cth,            /* ASMC substep */
                       10.0, 3.14159265358979323846, 28.284271247461902, 0.075}; /* header, reward */
  const double special[] = {0.0, -0.0, INFINITY, -INFINITY, NAN};
  long bad_total = 0;
  for (unsigned k = 0; k < sizeof(cs) / sizeof(cs[0]); ++k) {
    const double c = cs[k], y = 1.0 / c;
    long bad = 0, plain = 0, bad_special = 0, bad_tiny = 0, inexact_tiny = 0;
    for (long i = 0; i < n; ++i) {
      const double x = operand(1023 - 960, 1921);
      bad += !same(div_const(x, c), x / c);
      plain += x * y != x / c;
    }
    for (unsigned j = 0; j < sizeof(special) / sizeof(special[0]); ++j)
      bad_special += !same(div_const(special[j], c), special[j] / c);
    for (long i = 0; i < n / 10; ++i) {
      const double x = operand(0, 63), got = div_const(x, c), want = x / c;
      inexact_tiny += !same(got, want);
      const double ulp = nextafter(fabs(want), INFINITY) - fabs(want);
      bad_tiny += !(fabs(got - want) <= 0x1p-1074 * (1.0 + fabs(y)) + ulp) || signbit(got) != signbit(want);
    }
    printf("c = %.17g: %ld mismatches of %ld (a plain multiply by 1/c: %ld); special values: %ld of 5; "
           "tiny operands: %ld of %ld beyond their bound (%ld not equal)\n",
           c, bad, n, plain, bad_special, bad_tiny, n / 10, inexact_tiny);
    bad_total += bad + bad_special + bad_tiny;
  }
  return bad_total != 0;
}
