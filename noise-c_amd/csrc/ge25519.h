/*
 * ge25519.h — the group of Ed25519: the twisted Edwards curve
 * -x^2 + y^2 = 1 + d x^2 y^2 over GF(2^255 - 19), on the field arithmetic of
 * fe25519.h.  One source for both compilers, as fe25519.h is: the kernels of
 * launch_sign.hip and asan/sign_check.cpp compile the same functions.
 *
 * A point is extended coordinates (X : Y : Z : T), x = X/Z, y = Y/Z,
 * T = XY/Z (Hisil, Wong, Carter, Dawson 2008).  The operand of an addition is
 * kept precomputed as (Y + X, Y - X, 2 d T, Z).  With a = -1 a square and d
 * not one, the addition law is complete: it holds for equal points, for the
 * identity and for the points of small order, which is what lets the scalar
 * walks add an operand chosen by mask, the identity among the choices.
 *
 * Field elements are any 256-bit value standing for its residue, as
 * everywhere in fe25519.h; only ge_encode and the comparisons of ge_decode
 * freeze.
 *
 * The constants d, 2 d, sqrt(-1) and the base point are those
 * tests/ed25519_model.py derives from their definitions (d = -121665/121666,
 * sqrt(-1) = 2^((p-1)/4), B = (x, 4/5) with x even) and prints;
 * tests/test_sign_host.py compares the words below with the model's.
 *
 * Secret handling, for the callers that need it (ge_scalarmult_base): no
 * branch, address, table index or loop bound depends on a scalar bit or an
 * intermediate; the bit is read from the top of a shifting register set, the
 * operand is selected by mask.  ge_decode and ge_double_scalarmult work on
 * public data and say so.
 */
#pragma once
#include "fe25519.h"
#include "sc25519.h"

namespace na {

struct Ge { F25 x, y, z, t; };             /* extended coordinates */
struct GeCached { F25 ypx, ymx, t2d, z; }; /* an addition's second operand */

#define GE_D      {{0x135978a3u, 0x75eb4dcau, 0x4141d8abu, 0x00700a4du, 0x7779e898u, 0x8cc74079u, 0x2b6ffe73u, 0x52036ceeu}}
#define GE_D2     {{0x26b2f159u, 0xebd69b94u, 0x8283b156u, 0x00e0149au, 0xeef3d130u, 0x198e80f2u, 0x56dffce7u, 0x2406d9dcu}}
#define GE_SQRTM1 {{0x4a0ea0b0u, 0xc4ee1b27u, 0xad2fe478u, 0x2f431806u, 0x3dfbd7a7u, 0x2b4d0099u, 0x4fc1df0bu, 0x2b832480u}}
#define GE_BX     {{0x8f25d51au, 0xc9562d60u, 0x9525a7b2u, 0x692cc760u, 0xfdd6dc5cu, 0xc0a4e231u, 0xcd6e53feu, 0x216936d3u}}
#define GE_BY     {{0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u}}
#define GE_BT     {{0xa5b7dda3u, 0x6dde8ab3u, 0x775152f5u, 0x20f09f80u, 0x64abe37du, 0x66ea4e8eu, 0xd78b7665u, 0x67875f0fu}}
#define GE_B_YPX  {{0xf58c3b85u, 0x2fbc93c6u, 0xfb8c0e19u, 0xcf932dc6u, 0x643d42c2u, 0x270b4898u, 0x33d4ba65u, 0x07cf9d3au}}
#define GE_B_YMX  {{0xd740913eu, 0x9d103905u, 0xd140beb3u, 0xfd399f05u, 0x688f8a09u, 0xa5c18434u, 0x98f81267u, 0x44fd2f92u}}
#define GE_B_T2D  {{0x877aaa68u, 0xabc91205u, 0xccaac49eu, 0x26d9e823u, 0xdd43598cu, 0x5a1b7dcbu, 0x9f0c65a8u, 0x6f117b68u}}

F25_FN Ge ge_identity()
{
    Ge r;
    r.x = f25_small(0);
    r.y = f25_small(1);
    r.z = f25_small(1);
    r.t = f25_small(0);
    return r;
}

F25_FN Ge ge_base()
{
    Ge r;
    r.x = F25 GE_BX;
    r.y = F25 GE_BY;
    r.z = f25_small(1);
    r.t = F25 GE_BT;
    return r;
}

F25_FN GeCached ge_base_cached()
{
    GeCached r;
    r.ypx = F25 GE_B_YPX;
    r.ymx = F25 GE_B_YMX;
    r.t2d = F25 GE_B_T2D;
    r.z = f25_small(1);
    return r;
}

F25_FN GeCached ge_cache(const Ge &p)
{
    GeCached r;
    r.ypx = f25_add(p.y, p.x);
    r.ymx = f25_sub(p.y, p.x);
    r.t2d = f25_mul(p.t, F25 GE_D2);
    r.z = p.z;
    return r;
}

/* 2 p (dbl-2008-hwcd, a = -1): four squarings, four products.  T of p is
   not read. */
F25_FN Ge ge_double(const Ge &p)
{
    const F25 a = f25_sq(p.x), b = f25_sq(p.y);
    const F25 zz = f25_sq(p.z);
    const F25 c = f25_add(zz, zz);
    const F25 h = f25_add(a, b);                         /* -(D - B) with D = -A */
    const F25 e = f25_sub(h, f25_sq(f25_add(p.x, p.y))); /* -E */
    const F25 g = f25_sub(a, b);                         /* -G */
    const F25 f = f25_add(c, g);                         /* -F = C - G */
    Ge r;
    r.x = f25_mul(e, f);
    r.y = f25_mul(g, h);
    r.t = f25_mul(e, h);
    r.z = f25_mul(f, g);
    return r;
}

/* p + q (add-2008-hwcd-3, a = -1).  Z_ONE: q.z is 1 and is not read.
   WITH_T: the sum's T is wanted — a doubling that follows does not read it,
   and neither does ge_encode, so the walks leave that product out. */
template <bool Z_ONE, bool WITH_T>
F25_FN Ge ge_add(const Ge &p, const GeCached &q)
{
    const F25 a = f25_mul(f25_sub(p.y, p.x), q.ymx);
    const F25 b = f25_mul(f25_add(p.y, p.x), q.ypx);
    const F25 c = f25_mul(p.t, q.t2d);
    const F25 zz = Z_ONE ? p.z : f25_mul(p.z, q.z);
    const F25 d = f25_add(zz, zz);
    const F25 e = f25_sub(b, a), f = f25_sub(d, c), g = f25_add(d, c), h = f25_add(b, a);
    Ge r;
    r.x = f25_mul(e, f);
    r.y = f25_mul(g, h);
    r.z = f25_mul(f, g);
    r.t = WITH_T ? f25_mul(e, h) : f25_small(0);
    return r;
}

/* all ones where a is 0 mod p */
F25_FN uint32_t f25_is_zero_mask(const F25 &a)
{
    const F25 f = f25_freeze(a);
    uint32_t o = 0;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) o |= f.v[i];
    return 0u - (uint32_t)(o == 0);
}

F25_FN F25 f25_select(const F25 &a, const F25 &b, uint32_t mask_b)
{
    F25 r;
    F25_UNROLL
    for (int i = 0; i < 8; ++i) r.v[i] = a.v[i] ^ (mask_b & (a.v[i] ^ b.v[i]));
    return r;
}

/* z^(2^252 - 3) = z^((p - 5) / 8): the inversion's chain up to 2^250 - 1,
   two more squarings and z */
F25_FN F25 f25_pow22523(const F25 &z)
{
    const F25 z2 = f25_sq(z);
    const F25 z9 = f25_mul(f25_sqn<2>(z2), z);
    const F25 z11 = f25_mul(z9, z2);
    const F25 z_5_0 = f25_mul(f25_sq(z11), z9);
    const F25 z_10_0 = f25_mul(f25_sqn<5>(z_5_0), z_5_0);
    const F25 z_20_0 = f25_mul(f25_sqn<10>(z_10_0), z_10_0);
    const F25 z_40_0 = f25_mul(f25_sqn<20>(z_20_0), z_20_0);
    const F25 z_50_0 = f25_mul(f25_sqn<10>(z_40_0), z_10_0);
    const F25 z_100_0 = f25_mul(f25_sqn<50>(z_50_0), z_50_0);
    const F25 z_200_0 = f25_mul(f25_sqn<100>(z_100_0), z_100_0);
    const F25 z_250_0 = f25_mul(f25_sqn<50>(z_200_0), z_50_0);
    return f25_mul(f25_sqn<2>(z_250_0), z);
}

/* -A for the 32 bytes of a public key A, as ge25519_unpack_negative_vartime
   decodes them (ed25519-donna-impl-base.h:192-239); false where it refuses.
   y is the low 255 bits whatever their value (never compared with p);
   x = sqrt((y^2 - 1) / (d y^2 + 1)) is the candidate
   num den^3 (num den^7)^((p-5)/8), times sqrt(-1) where its square gives
   -num, refused where neither; x is then negated where its parity equals the
   sign bit, so that the parity of the result differs from it — also when x
   is 0, where nothing is checked.  Public data: the verdict is a plain bool. */
F25_FN bool ge_decode_negative(Ge &r, const uint8_t *pub)
{
    F25 y = f25_load(pub);
    const uint32_t sign = y.v[7] >> 31;
    y.v[7] &= 0x7fffffffu;
    const F25 yy = f25_sq(y);
    const F25 num = f25_sub(yy, f25_small(1));
    const F25 den = f25_add(f25_mul(yy, F25 GE_D), f25_small(1));
    const F25 d3 = f25_mul(f25_sq(den), den);
    F25 x = f25_mul(f25_mul(f25_sq(d3), den), num); /* num den^7 */
    x = f25_mul(f25_mul(f25_pow22523(x), d3), num);
    const F25 t = f25_mul(f25_sq(x), den);
    const uint32_t plus = f25_is_zero_mask(f25_sub(t, num));
    const uint32_t minus = f25_is_zero_mask(f25_add(t, num));
    x = f25_select(x, f25_mul(x, F25 GE_SQRTM1), ~plus);
    const F25 fx = f25_freeze(x);
    const uint32_t negate = 0u - (uint32_t)((fx.v[0] & 1u) == sign);
    r.x = f25_select(fx, f25_sub(f25_small(0), fx), negate);
    r.y = y;
    r.z = f25_small(1);
    r.t = f25_mul(r.x, y);
    return (plus | minus) != 0;
}

/* the 32 bytes of a point (ge25519_pack): canonical y, the parity of the
   canonical x in bit 255 */
F25_FN F25 ge_encode(const Ge &p)
{
    const F25 zi = f25_invert(p.z);
    const F25 x = f25_freeze(f25_mul(p.x, zi));
    F25 y = f25_freeze(f25_mul(p.y, zi));
    y.v[7] |= (x.v[0] & 1u) << 31;
    return y;
}

/* a scalar below 2^253 with bit 252 at the top of limb 7: the walks take
   bit 31 of limb 7 and shift, so no limb is indexed */
F25_FN void sc_walk_start(Sc &k)
{
    F25_UNROLL
    for (int i = 7; i > 0; --i) k.v[i] = (k.v[i] << 3) | (k.v[i - 1] >> 29);
    k.v[0] <<= 3;
}

F25_FN uint32_t sc_walk_bit(Sc &k)
{
    const uint32_t bit = 0u - (k.v[7] >> 31);
    F25_UNROLL
    for (int i = 7; i > 0; --i) k.v[i] = (k.v[i] << 1) | (k.v[i - 1] >> 31);
    k.v[0] <<= 1;
    return bit;
}

/* [k]B for a canonical k, in constant time: 253 doublings, an addition at
   every step whose operand is the identity or B by mask (for the identity,
   Y + X = Y - X = 1 and 2 d T = 0). */
F25_FN Ge ge_scalarmult_base(Sc k)
{
    const GeCached b = ge_base_cached();
    const F25 one = f25_small(1), zero = f25_small(0);
    sc_walk_start(k);
    Ge r = ge_identity();
    F25_NOUNROLL
    for (int t = 0; t < 253; ++t) {
        const uint32_t bit = sc_walk_bit(k);
        GeCached q;
        q.ypx = f25_select(one, b.ypx, bit);
        q.ymx = f25_select(one, b.ymx, bit);
        q.t2d = f25_select(zero, b.t2d, bit);
        q.z = one;
        r = ge_add<true, false>(ge_double(r), q);
    }
    return r;
}

/* [s]B + [h]Q for public s, h and a Q whose Z is 1 (verify: Q = -A as
   decoded): the joint bit-serial walk over the 253 bits.  Per bit one
   doubling and one addition of an operand selected by mask among {identity,
   Q, B, B + Q}: the 64 lanes of a wave hold different bits, so a branch would
   serialise all four arms. */
F25_FN Ge ge_double_scalarmult(Sc s, Sc h, const Ge &q)
{
    const GeCached cb = ge_base_cached();
    const GeCached cq = ge_cache(q);
    const GeCached cbq = ge_cache(ge_add<true, true>(ge_base(), cq));
    const F25 one = f25_small(1);
    sc_walk_start(s);
    sc_walk_start(h);
    Ge r = ge_identity();
    F25_NOUNROLL
    for (int t = 0; t < 253; ++t) {
        const uint32_t sb = sc_walk_bit(s), hb = sc_walk_bit(h);
        const uint32_t only_b = sb & ~hb, only_q = hb & ~sb, both = sb & hb, none = ~(sb | hb);
        GeCached o;
        F25_UNROLL
        for (int i = 0; i < 8; ++i) {
            const uint32_t id1 = none & one.v[i];
            o.ypx.v[i] = id1 | (only_b & cb.ypx.v[i]) | (only_q & cq.ypx.v[i]) | (both & cbq.ypx.v[i]);
            o.ymx.v[i] = id1 | (only_b & cb.ymx.v[i]) | (only_q & cq.ymx.v[i]) | (both & cbq.ymx.v[i]);
            o.t2d.v[i] = (only_b & cb.t2d.v[i]) | (only_q & cq.t2d.v[i]) | (both & cbq.t2d.v[i]);
            /* Z is 1 for the identity, for B and for Q */
            o.z.v[i] = (~both & one.v[i]) | (both & cbq.z.v[i]);
        }
        r = ge_add<false, false>(ge_double(r), o);
    }
    return r;
}

} // namespace na
