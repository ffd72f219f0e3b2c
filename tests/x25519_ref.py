"""A plain big-integer X25519 (RFC 7748 section 5) with the reference's rules:
the checker of tests/test_dh_host.py (which proves it against the reference's
own outputs, tests/golden/x25519.json) and of tests/test_gpu_dh.py.

curve25519_donna and curved25519_scalarmult_basepoint clamp the private key
themselves, ignore bit 255 of the public value, accept a public value of
2^255 - 19 or more as its residue, and return the fully reduced result; a
point of small order gives zeros."""
import json
import os

P = 2**255 - 19
A24 = 121665
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x25519.json")


def x25519(k: bytes, u: bytes) -> bytes:
    kn = int.from_bytes(k, "little")
    kn = (kn & ~7 & (2**255 - 1)) | 2**254
    x1 = (int.from_bytes(u, "little") & (2**255 - 1)) % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (kn >> t) & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % P, (x2 - z2) % P
        aa, bb = a * a % P, b * b % P
        e = (aa - bb) % P
        da, cb = (x3 - z3) * a % P, (x3 + z3) * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, z2 = x3, z3
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


def x25519_base(k: bytes) -> bytes:
    return x25519(k, (9).to_bytes(32, "little"))


def fixture_cases():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]
