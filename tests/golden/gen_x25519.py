"""Generate tests/golden/x25519.json from the reference noise-c itself.

Runs curve25519_donna (what noise_dhstate_calculate computes for Curve25519,
src/protocol/dhstate.c:685-717 through src/backend/ref/dh-curve25519.c:94-103)
and curved25519_scalarmult_basepoint (the public key of a private key,
dh-curve25519.c:49,73) of the reference library compiled from /root/reference
by oracle/Makefile (target `full`, oracle/_ref/libnoiseref_full.so).  Every
case holds a private key, a public value, shared = calculate(private, public
value) and public = the private key's own public key.  Build-container only;
the JSON is the committed fixture.

Usage: python tests/golden/gen_x25519.py
"""
import ctypes as C
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "..", "oracle", "_ref", "libnoiseref_full.so")
P = 2**255 - 19

# RFC 7748 section 5.2 (scalar, u, result) and section 6.1 (Alice, Bob, K)
RFC_5_2 = [
    ("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
     "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
     "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"),
    ("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
     "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
     "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"),
]
ALICE = ("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a",
         "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a")
BOB = ("5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb",
       "de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f")
SHARED_6_1 = "4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"
# public values at the edges: 0, 1, around p, all of 255 and of 256 bits, two
# points of order 8, and the base point
EDGE_U = [
    ("u=0", 0), ("u=1", 1), ("u=p-1", P - 1), ("u=p", P), ("u=p+1", P + 1),
    ("u=2^255-1", 2**255 - 1), ("u=0xff..ff", 2**256 - 1),
    ("u=order8a", 325606250916557431795983626356110631294008115727848805560023387167927233504),
    ("u=order8b", 39382357235489614581723060781553021112529911719440698176882885853963445705823),
    ("u=9", 9),
]


def main():
    L = C.CDLL(LIB)
    L.curve25519_donna.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.curved25519_scalarmult_basepoint.argtypes = [C.c_void_p, C.c_char_p]
    rnd = random.Random(0x58323535)
    cases = []

    def rand32():
        return bytes(rnd.getrandbits(8) for _ in range(32))

    def add(name, priv, pub):
        shared, public = C.create_string_buffer(32), C.create_string_buffer(32)
        L.curve25519_donna(shared, priv, pub)
        L.curved25519_scalarmult_basepoint(public, priv)
        cases.append({"name": name, "priv": priv.hex(), "pub": pub.hex(), "shared": shared.raw.hex(),
                      "public": public.raw.hex()})
        return cases[-1]

    for n, (k, u, out) in enumerate(RFC_5_2):
        assert add(f"rfc7748-5.2-{n + 1}", bytes.fromhex(k), bytes.fromhex(u))["shared"] == out
    a = add("rfc7748-6.1-alice", bytes.fromhex(ALICE[0]), bytes.fromhex(BOB[1]))
    b = add("rfc7748-6.1-bob", bytes.fromhex(BOB[0]), bytes.fromhex(ALICE[1]))
    assert a["shared"] == b["shared"] == SHARED_6_1
    assert a["public"] == ALICE[1] and b["public"] == BOB[1]
    for name, u in EDGE_U:
        add(name, rand32(), u.to_bytes(32, "little"))
    # scalars: all zero, all ones, and the bits the clamp clears set / the bit
    # it sets clear, each against the base point and a random point
    scalars = [("k=0", bytes(32)), ("k=0xff..ff", b"\xff" * 32),
               ("k=clamped-bits", bytes([0x07]) + bytes(30) + bytes([0x80])),
               ("k=clamped-bits-random", None)]
    for name, k in scalars:
        if k is None:
            r = rand32()
            k = bytes([r[0] | 7]) + r[1:31] + bytes([(r[31] | 0x80) & 0xBF])
        add(name + ",u=9", k, (9).to_bytes(32, "little"))
        add(name + ",u=random", k, rand32())
    for n in range(64):
        add(f"random-{n}", rand32(), rand32())
    with open(os.path.join(HERE, "x25519.json"), "w") as f:
        json.dump({"source": "reference curve25519_donna / curved25519_scalarmult_basepoint "
                             "(libnoiseref_full.so)", "cases": cases}, f, indent=1)
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
