/*
 * fe25519.h — X25519 (RFC 7748) over GF(2^255 - 19): field arithmetic, the
 * constant-time swap, the Montgomery ladder, the inversion and the freeze.
 * One source for both compilers: hipcc's device pass builds the kernels of
 * launch_dh.hip from it, plain g++ builds asan/dh_check.cpp from it, so the
 * CPU check under ASan/UBSan runs the code the GPU runs.  The only
 * device-only builtins are the 32-bit add-with-carry / subtract-with-borrow
 * (f25_addc / f25_subb), each with a plain C++ form beside it; the builtin
 * forms are checked on the device, one operation at a time and at the carry
 * edges, by tests/test_gpu_f25.py (noise_aead_debug_f25_op, debug_f25.hip).
 *
 * Layout: eight 32-bit limbs, radix 2^32, little endian — the 32 key bytes as
 * they lie in memory.  A value is any 256-bit number; it stands for its
 * residue mod p (2^256 == 38), so nothing is reduced between operations and
 * f25_freeze alone produces the canonical residue.  A product is eight rows
 * a_i * b of v_mad_u64_u32 chains (each step a_i * b_j + the step before's
 * high word, which fits 64 bits for any limbs), each row added into the
 * 16-word result by a 32-bit carry chain; the top eight words fold back
 * with x38.
 *
 * Secret handling: no branch, loop bound, address or table index depends on a
 * key bit or on an intermediate value.  The ladder runs its 255 steps
 * whatever the scalar, swaps by mask, and reads the scalar bit from the top
 * of a shifting register set (no indexed limb).  Every limb loop has constant
 * bounds and unrolls, so all state lives in registers: the kernels use no
 * scratch memory (tests/test_dh_host.py checks the compiler's report).
 */
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define F25_FN __host__ __device__ __forceinline__
#else
#define F25_FN static inline __attribute__((always_inline))
#endif
#if defined(__clang__)
#define F25_UNROLL _Pragma("unroll")
#define F25_NOUNROLL _Pragma("nounroll")
#else
#define F25_UNROLL
#define F25_NOUNROLL
#endif

namespace na {

struct F25 { uint32_t v[8]; };

/* a + b + cin -> sum, carry out (v_add_co / v_addc_co) */
F25_FN uint32_t f25_addc(uint32_t a, uint32_t b, uint32_t cin, uint32_t &cout)
{
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned int c;
    const uint32_t r = __builtin_addc(a, b, cin, &c);
    cout = c;
    return r;
#else
    const uint64_t t = (uint64_t)a + b + cin;
    cout = (uint32_t)(t >> 32);
    return (uint32_t)t;
#endif
}

/* a - b - bin -> difference, borrow out */
F25_FN uint32_t f25_subb(uint32_t a, uint32_t b, uint32_t bin, uint32_t &bout)
{
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned int c;
    const uint32_t r = __builtin_subc(a, b, bin, &c);
    bout = c;
    return r;
#else
    const uint64_t t = (uint64_t)a - b - bin;
    bout = (uint32_t)(t >> 63);
    return (uint32_t)t;
#endif
}

/* 32x32 -> 64 multiply-add: one v_mad_u64_u32.  With c < 2^32 it cannot
   overflow: (2^32 - 1)^2 + 2^32 - 1 < 2^64. */
F25_FN uint64_t f25_mad(uint32_t a, uint32_t b, uint64_t c) { return (uint64_t)a * b + c; }

F25_FN F25 f25_small(uint32_t x)
{
    F25 r;
    r.v[0] = x;
    F25_UNROLL
    for (int i = 1; i < 8; ++i) r.v[i] = 0;
    return r;
}

/* r + hi * 2^256 == r + 38 hi, for hi < 2^26.  When the first addition wraps,
   what is left is below 38 hi < 2^32, so the second x38 stays in limb 0. */
F25_FN void f25_fold(F25 &r, uint32_t hi)
{
    uint32_t c;
    r.v[0] = f25_addc(r.v[0], hi * 38u, 0u, c);
    F25_UNROLL
    for (int i = 1; i < 8; ++i) r.v[i] = f25_addc(r.v[i], 0u, c, c);
    r.v[0] += 38u * c;
}

F25_FN F25 f25_add(const F25 &a, const F25 &b)
{
    F25 r;
    uint32_t c = 0;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = f25_addc(a.v[i], b.v[i], c, c);
    f25_fold(r, c);
    return r;
}

/* a - b: a borrow out of limb 7 added 2^256 == 38, taken off again; if that
   borrows as well the value is at least 2^256 - 37 and the third step cannot. */
F25_FN F25 f25_sub(const F25 &a, const F25 &b)
{
    F25 r;
    uint32_t c = 0;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = f25_subb(a.v[i], b.v[i], c, c);
    r.v[0] = f25_subb(r.v[0], 38u * c, 0u, c);
    F25_UNROLL
    for (int i = 1; i < 8; ++i) r.v[i] = f25_subb(r.v[i], 0u, c, c);
    r.v[0] -= 38u * c;
    return r;
}

/* the 16-word value w folded to eight: low + 38 * high */
F25_FN F25 f25_reduce16(const uint32_t (&w)[16])
{
    F25 r;
    uint64_t t = 0;
    uint32_t c = 0;
    F25_UNROLL
    for (int j = 0; j < 8; ++j) {
        t = f25_mad(w[8 + j], 38u, t >> 32);
        r.v[j] = f25_addc(w[j], (uint32_t)t, c, c);
    }
    f25_fold(r, (uint32_t)(t >> 32) + c); /* at most 38 */
    return r;
}

F25_FN F25 f25_mul(const F25 &a, const F25 &b)
{
    uint32_t w[16];
    uint64_t t = 0;
    F25_UNROLL
    for (int j = 0; j < 8; ++j) {
        t = f25_mad(a.v[0], b.v[j], t >> 32);
        w[j] = (uint32_t)t;
    }
    w[8] = (uint32_t)(t >> 32);
    F25_UNROLL
    for (int i = 1; i < 8; ++i) {
        uint32_t c = 0;
        t = 0;
        F25_UNROLL
        for (int j = 0; j < 8; ++j) {
            t = f25_mad(a.v[i], b.v[j], t >> 32);
            w[i + j] = f25_addc(w[i + j], (uint32_t)t, c, c);
        }
        /* words i..i+7 so far plus a_i * b is below 2^288: no carry out */
        w[i + 8] = (uint32_t)(t >> 32) + c;
    }
    return f25_reduce16(w);
}

/* a^2: the 28 products a_i a_j (i < j) once, doubled, plus the squares */
F25_FN F25 f25_sq(const F25 &a)
{
    uint32_t w[16];
    uint64_t t = 0;
    w[0] = 0;
    F25_UNROLL
    for (int j = 1; j < 8; ++j) {
        t = f25_mad(a.v[0], a.v[j], t >> 32);
        w[j] = (uint32_t)t;
    }
    w[8] = (uint32_t)(t >> 32);
    F25_UNROLL
    for (int i = 1; i < 7; ++i) {
        uint32_t c = 0;
        t = 0;
        F25_UNROLL
        for (int j = i + 1; j < 8; ++j) {
            t = f25_mad(a.v[i], a.v[j], t >> 32);
            w[i + j] = f25_addc(w[i + j], (uint32_t)t, c, c);
        }
        /* the words above i + 7 are not written yet: this one starts here */
        w[i + 8] = (uint32_t)(t >> 32) + c;
    }
    w[15] = 0;
    /* twice the cross terms (below 2^512, so the top bit shifts out nothing),
       then a_i^2 into words 2i, 2i + 1 */
    F25_UNROLL
    for (int i = 15; i > 0; --i) w[i] = (w[i] << 1) | (w[i - 1] >> 31);
    w[0] = 0;
    uint32_t c = 0;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint64_t s = (uint64_t)a.v[i] * a.v[i];
        w[2 * i] = f25_addc(w[2 * i], (uint32_t)s, c, c);
        w[2 * i + 1] = f25_addc(w[2 * i + 1], (uint32_t)(s >> 32), c, c);
    }
    return f25_reduce16(w);
}

/* a * k for a constant k < 2^26 (121665, and the base point's u = 9) */
F25_FN F25 f25_mul_small(const F25 &a, uint32_t k)
{
    F25 r;
    uint64_t t = 0;
    F25_UNROLL
    for (int j = 0; j < 8; ++j) {
        t = f25_mad(a.v[j], k, t >> 32);
        r.v[j] = (uint32_t)t;
    }
    f25_fold(r, (uint32_t)(t >> 32));
    return r;
}

/* swap a and b where mask is all ones, keep them where it is zero */
F25_FN void f25_cswap(F25 &a, F25 &b, uint32_t mask)
{
    F25_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint32_t x = mask & (a.v[i] ^ b.v[i]);
        a.v[i] ^= x;
        b.v[i] ^= x;
    }
}

template <int N>
F25_FN F25 f25_sqn(F25 a)
{
    F25_NOUNROLL
    for (int i = 0; i < N; ++i) a = f25_sq(a);
    return a;
}

/* z^(p - 2) = z^(2^255 - 21): the fixed addition chain (254 squarings, 11
   multiplies); 0 gives 0. */
F25_FN F25 f25_invert(const F25 &z)
{
    const F25 z2 = f25_sq(z);
    const F25 z9 = f25_mul(f25_sqn<2>(z2), z);
    const F25 z11 = f25_mul(z9, z2);
    const F25 z_5_0 = f25_mul(f25_sq(z11), z9);              /* 2^5 - 1 */
    const F25 z_10_0 = f25_mul(f25_sqn<5>(z_5_0), z_5_0);    /* 2^10 - 1 */
    const F25 z_20_0 = f25_mul(f25_sqn<10>(z_10_0), z_10_0); /* 2^20 - 1 */
    const F25 z_40_0 = f25_mul(f25_sqn<20>(z_20_0), z_20_0); /* 2^40 - 1 */
    const F25 z_50_0 = f25_mul(f25_sqn<10>(z_40_0), z_10_0); /* 2^50 - 1 */
    const F25 z_100_0 = f25_mul(f25_sqn<50>(z_50_0), z_50_0);
    const F25 z_200_0 = f25_mul(f25_sqn<100>(z_100_0), z_100_0);
    const F25 z_250_0 = f25_mul(f25_sqn<50>(z_200_0), z_50_0);
    return f25_mul(f25_sqn<5>(z_250_0), z11);                /* 2^255 - 21 */
}

/* the canonical residue in [0, p) */
F25_FN F25 f25_freeze(F25 a)
{
    /* bit 255 is worth 19: now a < 2^255 + 19 */
    uint32_t c;
    const uint32_t top = a.v[7] >> 31;
    a.v[7] &= 0x7fffffffu;
    a.v[0] = f25_addc(a.v[0], 19u * top, 0u, c);
    F25_UNROLL
    for (int i = 1; i < 8; ++i) a.v[i] = f25_addc(a.v[i], 0u, c, c);
    /* a >= p exactly when a + 19 reaches 2^255, and then a - p is a + 19
       without that bit */
    F25 b;
    b.v[0] = f25_addc(a.v[0], 19u, 0u, c);
    F25_UNROLL
    for (int i = 1; i < 8; ++i) b.v[i] = f25_addc(a.v[i], 0u, c, c);
    const uint32_t mask = 0u - (b.v[7] >> 31);
    b.v[7] &= 0x7fffffffu;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) a.v[i] ^= mask & (a.v[i] ^ b.v[i]);
    return a;
}

/* 32 bytes at any alignment */
F25_FN F25 f25_load(const uint8_t *p)
{
    F25 r;
    F25_UNROLL
    for (int i = 0; i < 8; ++i)
        r.v[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
                 ((uint32_t)p[4 * i + 3] << 24);
    return r;
}

F25_FN void f25_store(uint8_t *p, const F25 &a)
{
    F25_UNROLL
    for (int i = 0; i < 8; ++i) {
        p[4 * i] = (uint8_t)a.v[i];
        p[4 * i + 1] = (uint8_t)(a.v[i] >> 8);
        p[4 * i + 2] = (uint8_t)(a.v[i] >> 16);
        p[4 * i + 3] = (uint8_t)(a.v[i] >> 24);
    }
}

/* X25519(k, u), RFC 7748 section 5: k is clamped here (as curve25519_donna
   and curved25519_scalarmult_basepoint do), bit 255 of u is ignored, a u of
   2^255 - 19 or more counts as its residue, and the result is canonical.
   u = 0 and the other points of small order give 0: z2 ends as 0 and
   f25_invert(0) is 0.  BASE: u is the base point 9 — the same ladder (no
   table indexed by the scalar), with the one multiply by u a small one. */
template <bool BASE>
F25_FN F25 x25519(F25 k, F25 u)
{
    k.v[0] &= ~7u;
    k.v[7] = (k.v[7] & 0x7fffffffu) | 0x40000000u;
    if (BASE) u = f25_small(9);
    u.v[7] &= 0x7fffffffu;
    /* bit 254 to the top: each step takes bit 31 of limb 7 and shifts */
    F25_UNROLL
    for (int i = 7; i > 0; --i) k.v[i] = (k.v[i] << 1) | (k.v[i - 1] >> 31);
    k.v[0] <<= 1;

    F25 x2 = f25_small(1), z2 = f25_small(0), x3 = u, z3 = f25_small(1);
    uint32_t swap = 0;
    F25_NOUNROLL
    for (int t = 0; t < 255; ++t) {
        const uint32_t bit = 0u - (k.v[7] >> 31);
        F25_UNROLL
        for (int i = 7; i > 0; --i) k.v[i] = (k.v[i] << 1) | (k.v[i - 1] >> 31);
        k.v[0] <<= 1;
        swap ^= bit;
        f25_cswap(x2, x3, swap);
        f25_cswap(z2, z3, swap);
        swap = bit;

        const F25 a = f25_add(x2, z2), b = f25_sub(x2, z2);
        const F25 aa = f25_sq(a), bb = f25_sq(b);
        const F25 e = f25_sub(aa, bb);
        const F25 da = f25_mul(f25_sub(x3, z3), a), cb = f25_mul(f25_add(x3, z3), b);
        x3 = f25_sq(f25_add(da, cb));
        const F25 d2 = f25_sq(f25_sub(da, cb));
        z3 = BASE ? f25_mul_small(d2, 9u) : f25_mul(d2, u);
        x2 = f25_mul(aa, bb);
        z2 = f25_mul(e, f25_add(aa, f25_mul_small(e, 121665u)));
    }
    f25_cswap(x2, x3, swap);
    f25_cswap(z2, z3, swap);
    return f25_freeze(f25_mul(x2, f25_invert(z2)));
}

} // namespace na
