/*
 * sc25519.h — scalars of Ed25519: integers mod the group order
 * L = 2^252 + 27742317777372353535851937790883648493, in eight 32-bit limbs,
 * radix 2^32, little endian — the 32 bytes of S as they lie in a signature.
 * One source for both compilers, as fe25519.h is: hipcc's device pass builds
 * the kernels of launch_sign.hip from it, plain g++ builds
 * asan/sign_check.cpp from it.
 *
 * An Sc is always canonical, in [0, L).  Everything here reduces a wider
 * value: the 512 bits of a SHA-512 digest (expand256_modm of 64 bytes), the
 * 256 bits of S or of the clamped secret scalar (expand256_modm of 32 bytes),
 * the 512 bits of a * b + c (mul256_modm then add256_modm).
 *
 * The reduction folds at bit 252, where 2^252 == -c (mod L) for the 125-bit
 * c = L - 2^252:
 *     x = lo + 2^252 hi                          hi below 2^260
 *       == lo - y,  y = c hi = ylo + 2^252 yhi   yhi below 2^133
 *       == lo - ylo + z,  z = c yhi = zlo + 2^252 zhi   zhi below 2^6
 *       == (lo + zlo + 2 L) - (ylo + c zhi)
 * The left bracket is below 2^252 + 2^252 + 2 L < 4 L, the right one below
 * 2^252 + 2^131 < 2 L, so the difference lies in (0, 4 L): it fits 255 bits
 * and cannot borrow, and subtracting 2 L and then L, each where it fits,
 * leaves [0, L).
 *
 * Branch-free: the sign path feeds it secrets (a, r, the digests).  Every loop
 * has constant bounds and unrolls; the conditional subtractions select by
 * mask; no limb is indexed by data.
 */
#pragma once
#include "fe25519.h"

namespace na {

struct Sc { uint32_t v[8]; };

/* L, and c = L - 2^252 */
#define SC_L_LIMBS {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0u, 0u, 0u, 0x10000000u}
#define SC_C_LIMBS {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu}

/* r = a * c: N limbs by four, N + 4 limbs out */
template <int N>
F25_FN void sc_mul_c(uint32_t (&r)[N + 4], const uint32_t (&a)[N])
{
    const uint32_t c[4] = SC_C_LIMBS;
    uint64_t t = 0;
    F25_UNROLL
    for (int i = 0; i < N; ++i) {
        t = f25_mad(a[i], c[0], t >> 32);
        r[i] = (uint32_t)t;
    }
    r[N] = (uint32_t)(t >> 32);
    F25_UNROLL
    for (int j = 1; j < 4; ++j) {
        uint32_t cy = 0;
        t = 0;
        F25_UNROLL
        for (int i = 0; i < N; ++i) {
            t = f25_mad(a[i], c[j], t >> 32);
            r[i + j] = f25_addc(r[i + j], (uint32_t)t, cy, cy);
        }
        /* limbs j.. so far plus a * c_j is below 2^(32 (N + 1)): no carry out */
        r[N + j] = (uint32_t)(t >> 32) + cy;
    }
}

/* x >> 252 of the limbs x[7..7 + N]: N limbs out */
template <int N, int M>
F25_FN void sc_high(uint32_t (&hi)[N], const uint32_t (&x)[M])
{
    F25_UNROLL
    for (int i = 0; i < N; ++i) {
        const uint32_t up = 8 + i < M ? x[8 + i] : 0u;
        hi[i] = (x[7 + i] >> 28) | (up << 4);
    }
}

/* a - k L where that is not negative, else a; a below 2^256 */
template <uint32_t K>
F25_FN void sc_sub_l_if_fits(uint32_t (&a)[8])
{
    const uint32_t l[8] = SC_L_LIMBS;
    uint32_t d[8], b = 0;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) {
        /* K L limb by limb: K is 1 or 2, and 2 L is L shifted by one */
        const uint32_t li = K == 1 ? l[i] : (l[i] << 1) | (i ? l[i - 1] >> 31 : 0u);
        d[i] = f25_subb(a[i], li, b, b);
    }
    const uint32_t keep = 0u - b; /* borrowed: a was smaller */
    F25_UNROLL
    for (int i = 0; i < 8; ++i) a[i] = d[i] ^ (keep & (d[i] ^ a[i]));
}

/* the 512-bit x mod L */
F25_FN Sc sc_reduce512(const uint32_t (&x)[16])
{
    const uint32_t l[8] = SC_L_LIMBS;
    uint32_t hi[9], y[13], yhi[5], z[9], zhi[1], w[5];
    sc_high<9>(hi, x);
    sc_mul_c<9>(y, hi);
    sc_high<5>(yhi, y);
    sc_mul_c<5>(z, yhi);
    sc_high<1>(zhi, z);
    sc_mul_c<1>(w, zhi);

    /* p = lo + zlo + 2 L */
    uint32_t p[8], q[8], cy = 0, cy2 = 0;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint32_t lo = i == 7 ? x[7] & 0x0fffffffu : x[i];
        const uint32_t zl = i == 7 ? z[7] & 0x0fffffffu : z[i];
        const uint32_t l2 = (l[i] << 1) | (i ? l[i - 1] >> 31 : 0u);
        p[i] = f25_addc(lo, zl, cy, cy);
        p[i] = f25_addc(p[i], l2, cy2, cy2);
    }
    /* q = ylo + c zhi */
    cy = 0;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) {
        const uint32_t yl = i == 7 ? y[7] & 0x0fffffffu : y[i];
        q[i] = f25_addc(yl, i < 5 ? w[i] : 0u, cy, cy);
    }
    uint32_t b = 0;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) p[i] = f25_subb(p[i], q[i], b, b);
    sc_sub_l_if_fits<2>(p);
    sc_sub_l_if_fits<1>(p);
    Sc r;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = p[i];
    return r;
}

/* the 256-bit x mod L: the same fold with nothing above limb 7 */
F25_FN Sc sc_reduce256(const uint32_t (&x)[8])
{
    uint32_t w[16];
    F25_UNROLL
    for (int i = 0; i < 16; ++i) w[i] = i < 8 ? x[i] : 0u;
    return sc_reduce512(w);
}

/* a b + c mod L, for canonical a, b, c: the product is below 2^506 */
F25_FN Sc sc_muladd(const Sc &a, const Sc &b, const Sc &c)
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
        uint32_t cy = 0;
        t = 0;
        F25_UNROLL
        for (int j = 0; j < 8; ++j) {
            t = f25_mad(a.v[i], b.v[j], t >> 32);
            w[i + j] = f25_addc(w[i + j], (uint32_t)t, cy, cy);
        }
        w[i + 8] = (uint32_t)(t >> 32) + cy;
    }
    uint32_t cy = 0;
    F25_UNROLL
    for (int i = 0; i < 16; ++i) w[i] = f25_addc(w[i], i < 8 ? c.v[i] : 0u, cy, cy);
    return sc_reduce512(w);
}

/* 64 little-endian bytes (a digest) mod L */
F25_FN Sc sc_from_bytes64(const uint8_t *p)
{
    uint32_t w[16];
    F25_UNROLL
    for (int i = 0; i < 16; ++i)
        w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
               ((uint32_t)p[4 * i + 3] << 24);
    return sc_reduce512(w);
}

/* 32 little-endian bytes mod L */
F25_FN Sc sc_from_bytes32(const uint8_t *p)
{
    const F25 x = f25_load(p);
    return sc_reduce256(x.v);
}

/* the canonical 32 bytes (contract256_modm) */
F25_FN void sc_store(uint8_t *p, const Sc &a)
{
    F25 x;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) x.v[i] = a.v[i];
    f25_store(p, x);
}

} // namespace na
