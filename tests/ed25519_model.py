"""Ed25519 as the reference computes it, in Python integers.

A model of the three functions behind NoiseSignState for Ed25519
(src/crypto/ed25519/ed25519.c:45-116): ed25519_publickey, ed25519_sign and
ed25519_sign_open, with the quirks of the last kept on purpose:

  - sig[63] & 0xE0 refuses; S is otherwise taken mod L, not range-checked;
  - the public key is decoded as ge25519_unpack_negative_vartime decodes it
    (ed25519-donna-impl-base.h:192-239): y is the low 255 bits whatever their
    value (never compared with p), the sign bit is not looked at when x = 0,
    a y whose x^2 has no root refuses;
  - the check is the byte comparison of encode([S]B - [h]A) with the 32 bytes
    of R: cofactorless, and R is never decoded.

Nothing but hashlib.  d, sqrt(-1) and the base point are derived from their
definitions (RFC 8032 section 5.1) and checked; limbs() prints a value as the
eight 32-bit words csrc/ge25519.h writes its constants in.
tests/test_sign_model_host.py holds the model against every record of
tests/golden/ed25519.json, which the reference itself wrote.
"""
import hashlib
import json
import os

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
D2 = 2 * D % P
SQRTM1 = pow(2, (P - 1) // 4, P)
assert SQRTM1 * SQRTM1 % P == P - 1

STATUS_REFUSED = 6  # section 8's status space: signature refused
SIGN_ED25519 = 0x5301
ERROR_INVALID_SIGNATURE = 0x4511

# the device's padding and block edges (64-byte prefix R || A for verify, 32-byte
# prefix for the r hash)
MESSAGE_LENGTHS = [0, 1, 31, 32, 47, 48, 63, 64, 65, 79, 80, 95, 96, 97, 175, 176, 191, 192, 193, 300]

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ed25519.json")


def sqrt_ratio(num, den):
    """x with den x^2 == num as the reference finds it, or None: the candidate
    num den^3 (num den^7)^((p-5)/8), times sqrt(-1) when it squares to -num."""
    x = num * pow(den, 3, P) * pow(num * pow(den, 7, P), (P - 5) // 8, P) % P
    t = den * x * x % P
    if (t - num) % P == 0:
        return x
    if (t + num) % P == 0:
        return x * SQRTM1 % P
    return None


# the base point: y = 4/5, x the even root
BY = 4 * pow(5, P - 2, P) % P
BX = sqrt_ratio((BY * BY - 1) % P, (D * BY * BY + 1) % P)
if BX & 1:
    BX = P - BX
B = (BX, BY, 1, BX * BY % P)
IDENTITY = (0, 1, 1, 0)


def add(p, q):
    """extended coordinates, a = -1: complete, so doubling is add(p, p)"""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = t1 * D2 * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def mul(k, p):
    r = IDENTITY
    for i in reversed(range(k.bit_length())):
        r = add(r, r)
        if (k >> i) & 1:
            r = add(r, p)
    return r


def encode(p):
    zi = pow(p[2], P - 2, P)
    x, y = p[0] * zi % P, p[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


assert encode(B) == bytes([0x58]) + bytes([0x66]) * 31
assert encode(mul(L, B)) == encode(IDENTITY)


def decode_negative(pub):
    """-A for the 32 bytes of a public key A, or None: the lenient decoding."""
    v = int.from_bytes(pub, "little")
    sign, y = v >> 255, v & (2**255 - 1)
    x = sqrt_ratio((y * y - 1) % P, (D * y * y + 1) % P)
    if x is None:
        return None
    if (x & 1) == sign:
        x = (P - x) % P
    return (x, y % P, 1, x * y % P)


def sha512_mod_l(*parts):
    return int.from_bytes(hashlib.sha512(b"".join(parts)).digest(), "little") % L


def secret_scalar(seed):
    h = bytearray(hashlib.sha512(seed).digest())
    h[0] &= 248
    h[31] &= 127
    h[31] |= 64
    return int.from_bytes(h[:32], "little"), bytes(h[32:])


def publickey(seed):
    return encode(mul(secret_scalar(seed)[0] % L, B))


def sign(msg, seed, pub):
    """pub is taken as given, as noise_signstate_sign takes the stored key"""
    a, prefix = secret_scalar(seed)
    r = sha512_mod_l(prefix, msg)
    rb = encode(mul(r, B))
    s = (sha512_mod_l(rb, pub, msg) * a + r) % L
    return rb + s.to_bytes(32, "little")


def check_point(msg, pub, sig):
    """encode([S]B - [h]A), or None where the reference refuses before it"""
    if sig[63] & 0xE0:
        return None
    na = decode_negative(pub)
    if na is None:
        return None
    h = sha512_mod_l(sig[:32], pub, msg)
    s = int.from_bytes(sig[32:], "little") % L
    return encode(add(mul(s, B), mul(h, na)))


def verify(msg, pub, sig):
    """True where ed25519_sign_open returns 0"""
    return check_point(msg, pub, sig) == sig[:32]


def status(msg, pub, sig):
    return 0 if verify(msg, pub, sig) else STATUS_REFUSED


def limbs(x):
    """x as csrc/ge25519.h writes a constant: eight 32-bit words, low first"""
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def header_constants():
    """name -> value of every field constant of csrc/ge25519.h"""
    return {"GE_D": D, "GE_D2": D2, "GE_SQRTM1": SQRTM1, "GE_BX": BX, "GE_BY": BY, "GE_BT": BX * BY % P,
            "GE_B_YPX": (BY + BX) % P, "GE_B_YMX": (BY - BX) % P, "GE_B_T2D": BX * BY * D2 % P}


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def fixture_verify_cases():
    """every record of the fixture that carries a verdict: (name, msg, pub, sig, ok)"""
    fx = fixture()
    out = []
    for c in fx["verify"]:
        out.append((c["name"], bytes.fromhex(c["msg"]), bytes.fromhex(c["pub"]), bytes.fromhex(c["sig"]),
                    c["rc"] == 0))
    return out


def fixture_sign_cases():
    """(name, seed, pub, msg, sig) of every record the reference signed"""
    fx = fixture()
    return [(c["name"], bytes.fromhex(c["seed"]), bytes.fromhex(c["pub"]), bytes.fromhex(c["msg"]),
             bytes.fromhex(c["sig"])) for c in fx["sign"]]


if __name__ == "__main__":
    for name, v in header_constants().items():
        print(name, ", ".join("0x%08xu" % w for w in limbs(v)))
