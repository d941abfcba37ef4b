// shortest.h -- the shortest decimal digits that read back as the same float64 / float32, for host and device from one function:
// Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020), in integer arithmetic only.  Among the shortest
// decimals inside the value's rounding interval it takes the one closest to the value, which is what repr(float), numpy's
// format_float_scientific(unique=True) and scipy.io.mmwrite print.  A float32 is converted in float32: its interval is wider than that of
// the float64 of the same value, so its digits are fewer.
//
// The one table is 617 128-bit powers of ten, g(k) = ceil(10^k * 2^(127 - floor(log2 10^k))), written by tools/gen_pow10_table.py
// (pow10_table.h); float32 takes the upper word, rounded up.  The device reads it from global memory (9.6 KB, resident in L2 and in the
// vector L1 of a compute unit that formats): lanes index it by their own value's exponent, so the loads are vector loads whatever the
// address space, and a copy in LDS would cost every workgroup the whole table for at most 512 look-ups.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace cyto {

constexpr int POW10_MIN = -292, POW10_MAX = 324;
static const uint64_t POW10_HOST[POW10_MAX - POW10_MIN + 1][2] = {
#include "pow10_table.h"
};
static __device__ const uint64_t POW10_DEV[POW10_MAX - POW10_MIN + 1][2] = {
#include "pow10_table.h"
};

struct Pow10 {
    uint64_t hi, lo;
};
__host__ __device__ inline Pow10 pow10_entry(int k) {  // POW10_MIN <= k <= POW10_MAX
#if defined(__HIP_DEVICE_COMPILE__)
    return Pow10{POW10_DEV[k - POW10_MIN][0], POW10_DEV[k - POW10_MIN][1]};
#else
    return Pow10{POW10_HOST[k - POW10_MIN][0], POW10_HOST[k - POW10_MIN][1]};
#endif
}

struct Decimal {                                        // value = digits * 10^exp10; digits has no trailing zero
    uint64_t digits;
    int exp10;
};

// floor(log2(10^e)), |e| <= 1233
__host__ __device__ inline int floor_log2_pow10(int e) { return (e * 1741647) >> 19; }

// The upper 64 bits of cp * g / 2^64 with every lower bit that is set folded into bit 0 (the paper's rounding to odd).
__host__ __device__ inline uint64_t round_to_odd64(Pow10 g, uint64_t cp) {
    const unsigned __int128 x = (unsigned __int128)cp * g.lo;
    const unsigned __int128 y = (unsigned __int128)cp * g.hi + (uint64_t)(x >> 64);
    return (uint64_t)(y >> 64) | (uint64_t)((uint64_t)y > 1);
}
__host__ __device__ inline uint32_t round_to_odd32(uint64_t g, uint32_t cp) {
    const unsigned __int128 p = (unsigned __int128)g * cp;
    const uint64_t y = (uint64_t)(p >> 32);
    return (uint32_t)(y >> 32) | (uint32_t)((uint32_t)y > 1);
}

// The paper's figure 4 on the scaled boundaries vbl <= vb <= vbr (each 4 * value * 10^-k, rounded to odd): (digits, k) or (digits, k + 1).
template <typename U> __host__ __device__ inline Decimal schubfach_pick(U vbl, U vb, U vbr, bool even, int k) {
    const U lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
    const U s = vb / 4;
    if (s >= 10) {
        const U sp = s / 10;
        const bool up_inside = lower <= 40 * sp, wp_inside = 40 * sp + 40 <= upper;
        if (up_inside != wp_inside) return Decimal{(uint64_t)(sp + (wp_inside ? 1 : 0)), k + 1};
    }
    const bool u_inside = lower <= 4 * s, w_inside = 4 * s + 4 <= upper;
    if (u_inside != w_inside) return Decimal{(uint64_t)(s + (w_inside ? 1 : 0)), k};
    const U mid = 4 * s + 2;
    const bool up = vb > mid || (vb == mid && (s & 1) != 0);
    return Decimal{(uint64_t)(s + (up ? 1 : 0)), k};
}

__host__ __device__ inline Decimal strip_zeros(Decimal d) {
    if (d.digits <= 0xffffffffull) {
        uint32_t s = (uint32_t)d.digits;
        while (s % 10u == 0) s /= 10u, d.exp10++;
        d.digits = s;
    } else {
        while (d.digits % 10u == 0) d.digits /= 10u, d.exp10++;
    }
    return d;
}

// bits: a finite non-zero float64 (the sign bit is ignored).  digits < 10^17.
__host__ __device__ inline Decimal shortest_digits64(uint64_t bits) {
    const uint64_t frac = bits & 0x000fffffffffffffull;
    const int ex = (int)((bits >> 52) & 0x7ff);
    uint64_t c;
    int q;
    if (ex != 0) {
        c = frac | 0x0010000000000000ull;
        q = ex - 1075;
        if (q <= 0 && q > -53 && (c & ((uint64_t(1) << -q) - 1)) == 0) return strip_zeros(Decimal{c >> -q, 0});   // an integer below 2^53
    } else {
        c = frac;
        q = -1074;
    }
    const bool even = (c & 1) == 0;
    const bool closer = frac == 0 && ex > 1;           // a binade's first value: the lower neighbour is half as far away
    const uint64_t cbl = 4 * c - 2 + (closer ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
    const int k = (q * 1262611 - (closer ? 524031 : 0)) >> 22;       // floor(log10(2^q)), or floor(log10(3/4 * 2^q))
    const int h = q + floor_log2_pow10(-k) + 1;
    const Pow10 g = pow10_entry(-k);
    return strip_zeros(schubfach_pick<uint64_t>(round_to_odd64(g, cbl << h), round_to_odd64(g, cb << h), round_to_odd64(g, cbr << h), even, k));
}

// bits: a finite non-zero float32 (the sign bit is ignored).  digits < 10^9.
__host__ __device__ inline Decimal shortest_digits32(uint32_t bits) {
    const uint32_t frac = bits & 0x007fffffu;
    const int ex = (int)((bits >> 23) & 0xff);
    uint32_t c;
    int q;
    if (ex != 0) {
        c = frac | 0x00800000u;
        q = ex - 150;
        if (q <= 0 && q > -24 && (c & ((1u << -q) - 1)) == 0) return strip_zeros(Decimal{c >> -q, 0});   // an integer below 2^24
    } else {
        c = frac;
        q = -149;
    }
    const bool even = (c & 1) == 0;
    const bool closer = frac == 0 && ex > 1;
    const uint32_t cbl = 4 * c - 2 + (closer ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
    const int k = (q * 1262611 - (closer ? 524031 : 0)) >> 22;
    const int h = q + floor_log2_pow10(-k) + 1;
    const Pow10 g128 = pow10_entry(-k);
    const uint64_t g = g128.hi + (g128.lo != 0 ? 1 : 0);            // ceil(10^-k * 2^(63 - floor(log2 10^-k)))
    return strip_zeros(schubfach_pick<uint32_t>(round_to_odd32(g, cbl << h), round_to_odd32(g, cb << h), round_to_odd32(g, cbr << h), even, k));
}

}  // namespace cyto
