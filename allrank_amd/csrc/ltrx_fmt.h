// "%.16g" of an fp32 value, exactly: the text Python's '%.16g' % float(numpy.float32(v)) gives (what scikit-learn's dump_svmlight_file
// prints for every label and value), for every fp32 bit pattern.  One function for host and device; contract: include/ltrx.h,
// "libsvm text written on the device".
//
// ARITHMETIC.  No floating point at all.  A finite non-zero fp32 is m * 2^e with 0 < m < 2^24 and -149 <= e <= 104, so its decimal
// expansion is finite (at most 39 integer digits, at most 149 fraction digits) and is produced here nine digits at a time:
//   e >= 0: the integer m << e (128 bits, four 32-bit words) divided by 10^9 until it is zero -- the remainders are the groups, least
//           significant first;
//   e <  0: the integer part m >> -e is one group; the fraction is a 160-bit fixed-point number (five 32-bit words) multiplied by 10^9
//           again and again -- the carry out of the top word is the next group, and the product stays exact.
// The three groups that start at the first non-zero one hold at least 19 significant digits.  Seventeen of them are taken: sixteen
// for the text, the seventeenth to round on, together with a sticky bit for everything behind it (the rest of the three groups, the
// lower groups of the integer, what is left of the fraction).  Round to nearest, ties to even on the sixteenth digit: exactly what a
// correctly rounding printf does.  Then %g's layout: trailing zeros stripped, no '.' without a fraction, fixed notation for decimal
// exponents -4 .. 15, d.ddde+XX (two exponent digits: |X| <= 45 for fp32) otherwise.
// Everything is kept in scalars (no array indexed at run time but the output slot), so on the device the state lives in registers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LTRX_FMT_HD __host__ __device__ inline
#else
#define LTRX_FMT_HD inline
#endif

#define LTRX_FMT_SLOT 24          // bytes of an output slot; the longest text has 22: -1.234567890123456e-05, -0.0001234567890123456

namespace ltrx_fmt {

LTRX_FMT_HD uint64_t pow10_u64(int k) {          // 10^k, 0 <= k <= 17
  uint64_t p = 1;
  for (int i = 0; i < k; ++i) p *= 10ull;
  return p;
}

LTRX_FMT_HD int digits_u32(uint32_t v) {         // decimal digits of v < 10^9 (1 for 0)
  return v >= 100000000u ? 9 : v >= 10000000u ? 8 : v >= 1000000u ? 7 : v >= 100000u ? 6 : v >= 10000u ? 5 : v >= 1000u ? 4 : v >= 100u ? 3
       : v >= 10u ? 2 : 1;
}

// (w3 w2 w1 w0) /= 10^9, returns the remainder: schoolbook division of four 32-bit words by a 32-bit divisor
LTRX_FMT_HD uint32_t div_1e9(uint32_t& w3, uint32_t& w2, uint32_t& w1, uint32_t& w0) {
  const uint64_t D = 1000000000ull;
  uint64_t t = w3;
  w3 = (uint32_t)(t / D), t = ((t % D) << 32) | w2;
  w2 = (uint32_t)(t / D), t = ((t % D) << 32) | w1;
  w1 = (uint32_t)(t / D), t = ((t % D) << 32) | w0;
  w0 = (uint32_t)(t / D);
  return (uint32_t)(t % D);
}

// the fraction 0.(f4 f3 f2 f1 f0) *= 10^9, returns the integer part (< 10^9)
LTRX_FMT_HD uint32_t mul_1e9(uint32_t& f4, uint32_t& f3, uint32_t& f2, uint32_t& f1, uint32_t& f0) {
  const uint64_t D = 1000000000ull;
  uint64_t t = (uint64_t)f0 * D;
  f0 = (uint32_t)t, t = (uint64_t)f1 * D + (t >> 32);
  f1 = (uint32_t)t, t = (uint64_t)f2 * D + (t >> 32);
  f2 = (uint32_t)t, t = (uint64_t)f3 * D + (t >> 32);
  f3 = (uint32_t)t, t = (uint64_t)f4 * D + (t >> 32);
  f4 = (uint32_t)t;
  return (uint32_t)(t >> 32);
}

}  // namespace ltrx_fmt

// writes the text of v to out[0 .. LTRX_FMT_SLOT) and returns its length (1 .. 22); no terminator
LTRX_FMT_HD int ltrx_fmt_g16(float v, uint8_t* out) {
  using namespace ltrx_fmt;
  const uint32_t bits = __builtin_bit_cast(uint32_t, v);
  const uint32_t ex = (bits >> 23) & 0xFFu, man = bits & 0x7FFFFFu;
  int n = 0;
  if (ex == 0xFFu && man != 0u) {                  // Python prints a NaN without its sign
    out[0] = 'n', out[1] = 'a', out[2] = 'n';
    return 3;
  }
  if (bits >> 31) out[n++] = '-';
  if (ex == 0xFFu) {
    out[n] = 'i', out[n + 1] = 'n', out[n + 2] = 'f';
    return n + 3;
  }
  if (ex == 0u && man == 0u) {
    out[n++] = '0';
    return n;
  }
  const uint32_t m = ex ? (man | 0x800000u) : man;
  const int e = ex ? (int)ex - 150 : -149;

  // ---- three nine-digit groups g0 g1 g2 from the first non-zero one; `top` = the decimal place of g0's leading digit ----
  uint32_t g0 = 0, g1 = 0, g2 = 0;
  int top;
  bool sticky = false;
  if (e >= 0) {
    uint64_t lo, hi;
    if (e < 64) {
      lo = (uint64_t)m << e;
      hi = e > 40 ? (uint64_t)m >> (64 - e) : 0ull;
    } else {
      lo = 0ull;
      hi = (uint64_t)m << (e - 64);
    }
    uint32_t w3 = (uint32_t)(hi >> 32), w2 = (uint32_t)hi, w1 = (uint32_t)(lo >> 32), w0 = (uint32_t)lo;
    int groups = 0;
    while ((w3 | w2 | w1 | w0) != 0u && groups < 5) {      // 2^128 < 10^45: five groups at most
      const uint32_t r = div_1e9(w3, w2, w1, w0);
      sticky = sticky || g2 != 0u;
      g2 = g1, g1 = g0, g0 = r;
      ++groups;
    }
    top = 9 * groups - 1;
  } else {
    const int s = -e;                                      // 1 .. 149
    const uint32_t ip = s < 24 ? m >> s : 0u;
    const uint32_t fm = s < 24 ? m & ((1u << s) - 1u) : m;  // fraction = fm / 2^s = (fm << (160 - s)) / 2^160
    const int sh = 160 - s, word = sh >> 5;                // fm < 2^min(s, 24): the shifted value spans two words, below 2^160
    const uint64_t two = (uint64_t)fm << (sh & 31);
    const uint32_t a = (uint32_t)two, b = (uint32_t)(two >> 32);
    uint32_t f0 = word == 0 ? a : 0u;
    uint32_t f1 = word == 1 ? a : word == 0 ? b : 0u;
    uint32_t f2 = word == 2 ? a : word == 1 ? b : 0u;
    uint32_t f3 = word == 3 ? a : word == 2 ? b : 0u;
    uint32_t f4 = word == 4 ? a : word == 3 ? b : 0u;
    if (ip != 0u) {
      g0 = ip;
      top = 8;
    } else {                                               // fm != 0: 2^-149 > 10^-45, so the fifth group at the latest is non-zero
      int k = 0;
      do {
        g0 = mul_1e9(f4, f3, f2, f1, f0);
        ++k;
      } while (g0 == 0u && k < 6);
      top = -1 - 9 * (k - 1);
    }
    g1 = mul_1e9(f4, f3, f2, f1, f0);
    g2 = mul_1e9(f4, f3, f2, f1, f0);
    sticky = (f4 | f3 | f2 | f1 | f0) != 0u;
  }

  // ---- seventeen significant digits V, the decimal exponent X of the first ----
  const int nd0 = digits_u32(g0);
  int X = top - (9 - nd0);
  const int k = 17 - nd0;                                  // digits still to take: 8 .. 16
  uint64_t V;
  if (k <= 9) {
    const uint32_t div = (uint32_t)pow10_u64(9 - k);
    V = (uint64_t)g0 * pow10_u64(k) + g1 / div;
    sticky = sticky || (g1 % div) != 0u || g2 != 0u;
  } else {
    const uint32_t div = (uint32_t)pow10_u64(18 - k);      // k - 9 digits of g2
    V = ((uint64_t)g0 * 1000000000ull + g1) * pow10_u64(k - 9) + g2 / div;
    sticky = sticky || (g2 % div) != 0u;
  }
  uint64_t S = V / 10ull;                                  // sixteen digits
  const uint32_t r = (uint32_t)(V % 10ull);
  if (r > 5u || (r == 5u && (sticky || (S & 1ull)))) ++S;
  if (S == 10000000000000000ull) {
    S = 1000000000000000ull;
    ++X;
  }
  int p = 16;                                              // significant digits left once the trailing zeros are gone
  while (p > 1 && S % 10ull == 0ull) {
    S /= 10ull;
    --p;
  }

  // ---- layout: digit i of S (0 = leading) goes to out[n + lead + i], one further where it stands behind the point ----
  const bool expo = X < -4 || X >= 16;
  const int lead = (!expo && X < 0) ? 1 - X : 0;           // "0." and -X - 1 zeros
  const int point = expo ? 0 : (X >= 0 ? X : -1);          // the point stands behind digit `point`
  if (lead) {
    out[n] = '0', out[n + 1] = '.';
    for (int i = 2; i < lead; ++i) out[n + i] = '0';
  }
  for (int i = p - 1; i >= 0; --i) {
    out[n + lead + i + ((lead == 0 && i > point) ? 1 : 0)] = (uint8_t)('0' + (uint32_t)(S % 10ull));
    S /= 10ull;
  }
  int len = n + lead + p;
  if (lead == 0) {
    if (p - 1 > point) {
      out[n + point + 1] = '.';
      ++len;
    } else {
      for (int i = p; i <= point; ++i) out[n + i] = '0';   // an integer with trailing zeros: 1e15 -> 1000000000000000
      len = n + point + 1;
    }
  }
  if (expo) {
    const int ax = X < 0 ? -X : X;
    out[len] = 'e', out[len + 1] = X < 0 ? '-' : '+';
    out[len + 2] = (uint8_t)('0' + ax / 10), out[len + 3] = (uint8_t)('0' + ax % 10);
    len += 4;
  }
  return len;
}
