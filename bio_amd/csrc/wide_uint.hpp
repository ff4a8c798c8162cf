// wide_uint.hpp -- the integers behind a hit's measure (select.hip; include/biosketch.h "hits selected by a measure"): a fraction N/D of
// two 128-bit numbers, compared by cross products of 256 bits in four 64-bit limbs.  Host and device: the C++ test of the owners
// checks the device against this very header compiled by the host compiler.  Nothing here crosses the C ABI.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BSK_WIDE_FN __host__ __device__ inline
#else
#define BSK_WIDE_FN inline
#endif

typedef unsigned __int128 bsk_u128;

struct bsk_u256 {
    uint64_t w[4];  // little endian: w[0] the lowest limb
};

// a * b, every bit of it
BSK_WIDE_FN bsk_u256 wide_mul(bsk_u128 a, bsk_u128 b) {
    const uint64_t a0 = (uint64_t)a, a1 = (uint64_t)(a >> 64), b0 = (uint64_t)b, b1 = (uint64_t)(b >> 64);
    const bsk_u128 p00 = (bsk_u128)a0 * b0, p01 = (bsk_u128)a0 * b1, p10 = (bsk_u128)a1 * b0, p11 = (bsk_u128)a1 * b1;
    bsk_u256 r;
    r.w[0] = (uint64_t)p00;
    const bsk_u128 m1 = (p00 >> 64) + (uint64_t)p01 + (uint64_t)p10;            // three terms below 2^64
    r.w[1] = (uint64_t)m1;
    const bsk_u128 m2 = (m1 >> 64) + (p01 >> 64) + (p10 >> 64) + (uint64_t)p11;  // four terms below 2^64
    r.w[2] = (uint64_t)m2;
    r.w[3] = (uint64_t)(p11 >> 64) + (uint64_t)(m2 >> 64);  // (the product is below 2^256: no carry out)
    return r;
}

// -1, 0, 1 as x is below, equal to, above y
BSK_WIDE_FN int wide_cmp(const bsk_u256 &x, const bsk_u256 &y) {
    for (int i = 3; i >= 0; --i)
        if (x.w[i] != y.w[i]) return x.w[i] < y.w[i] ? -1 : 1;
    return 0;
}

// the sign of na / da - nb / db for positive denominators: that of na * db - nb * da
BSK_WIDE_FN int wide_frac_cmp(bsk_u128 na, bsk_u128 da, bsk_u128 nb, bsk_u128 db) {
    if (da == db) return na < nb ? -1 : na > nb ? 1 : 0;  // (the integer measures: D = 1)
    return wide_cmp(wide_mul(na, db), wide_mul(nb, da));
}
