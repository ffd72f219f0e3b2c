"""Generate tests/golden/ed25519.json from the reference noise-c itself.

Runs NoiseSignState for Ed25519 (src/protocol/signstate.c over
src/backend/ref/sign-ed25519.c and src/crypto/ed25519/ed25519.c) of the
reference library compiled by oracle/Makefile (target `full`,
oracle/_ref/libnoiseref_full.so) through noise_signstate_*.  Every byte and
every return code in the fixture is the reference's; tests/ed25519_model.py is
used only to build the unusual inputs (S + L, small-order keys, y + p), never
for an expected value.  Build-container only; the JSON is the committed
fixture.

  sign    seed, public key, message, signature: the five draft-irtf-cfrg-eddsa
          vectors of the reference's tests/unit/test-signstate.c (read from
          that file as data and checked against what the library computes),
          and 24 seeded random seeds over the device's message-length edges.
  verify  message, public key, signature, the reference's return code, in
          groups: the signed records as they are, their tampered variants, the
          S edge cases, the public-key edge cases, the small-order keys, a
          non-canonical R.

The generator fails unless the groups S + L, non-canonical y and small-order
keys each hold an accepted and a refused record: a device that refuses
everything unusual cannot pass.

Usage: python tests/golden/gen_ed25519.py [--check]
       --check: regenerate and compare with the committed file, write nothing.
"""
import ctypes as C
import json
import os
import random
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import ed25519_model as M  # noqa: E402

LIB = os.path.join(HERE, "..", "..", "oracle", "_ref", "libnoiseref_full.so")
VECTORS = "/root/reference/tests/unit/test-signstate.c"
OUT = os.path.join(HERE, "ed25519.json")
ID = M.SIGN_ED25519


class Ref:
    def __init__(self):
        self.L = L = C.CDLL(LIB)
        vp = C.c_void_p
        L.noise_signstate_new_by_id.argtypes = [C.POINTER(vp), C.c_int]
        L.noise_signstate_free.argtypes = [vp]
        L.noise_signstate_set_keypair_private.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.noise_signstate_set_public_key.argtypes = [vp, C.c_char_p, C.c_size_t]
        L.noise_signstate_get_public_key.argtypes = [vp, vp, C.c_size_t]
        L.noise_signstate_sign.argtypes = [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t]
        L.noise_signstate_verify.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]

    def new(self):
        st = C.c_void_p()
        assert self.L.noise_signstate_new_by_id(C.byref(st), ID) == 0
        return st

    def sign(self, seed, msg):
        """(public key, signature) of the keypair made from seed"""
        st = self.new()
        assert self.L.noise_signstate_set_keypair_private(st, seed, 32) == 0
        pub, sig = C.create_string_buffer(32), C.create_string_buffer(64)
        assert self.L.noise_signstate_get_public_key(st, pub, 32) == 0
        assert self.L.noise_signstate_sign(st, msg + b"\0", len(msg), sig, 64) == 0
        self.L.noise_signstate_free(st)
        return pub.raw, sig.raw

    def verify(self, msg, pub, sig):
        st = self.new()
        assert self.L.noise_signstate_set_public_key(st, pub, 32) == 0
        rc = self.L.noise_signstate_verify(st, msg + b"\0", len(msg), sig, 64)
        self.L.noise_signstate_free(st)
        assert rc in (0, M.ERROR_INVALID_SIGNATURE), hex(rc)
        return rc


def draft_vectors():
    """(seed, public key, message, signature) of every check_sign(...) call of
    the reference's unit test, as bytes"""
    text = open(VECTORS).read()
    out = []
    for call in re.findall(r"check_sign\s*\(NOISE_SIGN_ED25519,[^;]*;", text, re.S):
        args, cur = [], None
        # adjacent string literals make one argument; a comma ends it
        for tok in re.findall(r'"([^"]*)"|(,)', call.split('"Ed25519"', 1)[1]):
            if tok[1]:
                if cur is not None:
                    args.append(cur)
                cur = None
            else:
                cur = (cur or "") + tok[0]
        args.append(cur)
        assert len(args) == 4, args
        out.append(tuple(bytes.fromhex(a.replace("0x", "").replace(" ", "")) for a in args))
    assert len(out) == 5 and len(out[3][2]) == 1023
    return out


def flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def le(x):
    return x.to_bytes(32, "little")


def build():
    ref = Ref()
    rnd = random.Random(0x45443235)

    def rand(n):
        return bytes(rnd.getrandbits(8) for _ in range(n))

    sign, verify = [], []

    def add_sign(name, seed, msg):
        pub, sig = ref.sign(seed, msg)
        sign.append({"name": name, "seed": seed.hex(), "pub": pub.hex(), "msg": msg.hex(), "sig": sig.hex()})
        return pub, sig

    def add_verify(group, name, msg, pub, sig):
        rc = ref.verify(msg, pub, sig)
        verify.append({"group": group, "name": name, "msg": msg.hex(), "pub": pub.hex(), "sig": sig.hex(), "rc": rc})
        return rc

    for n, (seed, pub, msg, sig) in enumerate(draft_vectors()):
        assert add_sign(f"draft-{n + 1}", seed, msg) == (pub, sig)
        assert add_verify("valid", f"draft-{n + 1}", msg, pub, sig) == 0

    lengths = M.MESSAGE_LENGTHS + [rnd.choice(M.MESSAGE_LENGTHS) for _ in range(4)]
    assert len(lengths) == 24
    signed = []
    for n, ln in enumerate(lengths):
        seed, msg = rand(32), rand(ln)
        pub, sig = add_sign(f"random-{n}-len{ln}", seed, msg)
        signed.append((msg, pub, sig))
        assert add_verify("valid", f"random-{n}", msg, pub, sig) == 0
    for n, (msg, pub, sig) in enumerate(signed):
        add_verify("tampered", f"random-{n}-R-bit", msg, pub, flip(sig, rnd.randrange(256)))
        add_verify("tampered", f"random-{n}-S-bit", msg, pub, flip(sig, 256 + rnd.randrange(253)))
        if msg:
            add_verify("tampered", f"random-{n}-msg-bit", flip(msg, rnd.randrange(8 * len(msg))), pub, sig)
        add_verify("tampered", f"random-{n}-pub-bit", msg, flip(pub, rnd.randrange(256)), sig)
        add_verify("tampered", f"random-{n}-other-pub", msg, signed[(n + 1) % len(signed)][1], sig)

    # S edge cases
    for n, (msg, pub, sig) in enumerate(signed[:8]):
        s = int.from_bytes(sig[32:], "little")
        for bit in (253, 254, 255):
            add_verify("s_top_bits", f"random-{n}-S-bit{bit}", msg, pub, sig[:32] + le(s | 1 << bit))
        # S + L is below 2^253 (S < L < 2^252 + 2^125): it passes the top-bit
        # test and is reduced.  S + L + 1 passes it too and is another scalar;
        # S + 2 L reaches bit 253.
        assert s + M.L < 2**253 <= s + 2 * M.L
        add_verify("s_plus_l", f"random-{n}-S+L", msg, pub, sig[:32] + le(s + M.L))
        add_verify("s_plus_l", f"random-{n}-S+L+1", msg, pub, sig[:32] + le(s + M.L + 1))
        add_verify("s_plus_l", f"random-{n}-S+2L", msg, pub, sig[:32] + le(s + 2 * M.L))
        add_verify("s_edges", f"random-{n}-S=0", msg, pub, sig[:32] + le(0))
        add_verify("s_edges", f"random-{n}-S=L", msg, pub, sig[:32] + le(M.L))

    # public-key edge cases.  With S = 0 the check is encode(-[h]A) == R, so a
    # key of small order can be given a signature the reference accepts.
    ident = M.encode(M.IDENTITY)
    zero_sig = ident + le(0)
    msg = b"edge"
    for k in range(19):
        y = M.P + k
        if M.decode_negative(le(y)) is None:
            continue
        add_verify("noncanonical_y", f"y=p+{k}-identity-sig", msg, le(y), zero_sig)
        add_verify("noncanonical_y", f"y=p+{k}-random-sig", msg, le(y), rand(32) + le(rnd.randrange(M.L)))
    add_verify("noncanonical_y", "y=p+1-signbit-identity-sig", msg, le(M.P + 1 | 1 << 255), zero_sig)
    noroot = [y for y in range(2, 200) if M.decode_negative(le(y)) is None][:3]
    for y in noroot:
        add_verify("no_root", f"y={y}-identity-sig", msg, le(y), zero_sig)
        add_verify("no_root", f"y={y}-signbit-random-sig", msg, le(y | 1 << 255), rand(32) + le(rnd.randrange(M.L)))
    add_verify("y_edges", "y=1-identity-sig", msg, le(1), zero_sig)
    add_verify("y_edges", "y=1-signbit-identity-sig", msg, le(1 | 1 << 255), zero_sig)
    add_verify("y_edges", "y=p-1-identity-sig", msg, le(M.P - 1), zero_sig)
    add_verify("y_edges", "y=p-1-R=p-1", msg, le(M.P - 1), le(M.P - 1) + le(0))
    add_verify("y_edges", "y=p-1-signbit-identity-sig", msg, le(M.P - 1 | 1 << 255), zero_sig)

    # the eight points of small order: multiples of a point of order 8
    t = None
    for y in range(2, 1 << 16):  # [L] of a point of order 8 L has order 8
        p = M.decode_negative(le(y))
        if p is None:
            continue
        q = M.mul(M.L, p)
        if M.encode(M.mul(4, q)) != ident and M.encode(M.mul(8, q)) == ident:
            t = q
            break
    assert t is not None
    small = sorted({M.encode(M.mul(k, t)) for k in range(8)})
    assert len(small) == 8 and ident in small
    for enc in small:
        name = "order8-" + enc.hex()[:8] + ("-signbit" if enc[31] & 0x80 else "")
        add_verify("small_order", name + "-identity-sig", msg, enc, zero_sig)
        add_verify("small_order", name + "-random-sig", msg, enc, rand(32) + le(rnd.randrange(M.L)))
        # a message for which [h]A is the identity, and one for which it is not
        want = {0, M.ERROR_INVALID_SIGNATURE} if enc != ident else {0}
        for n in range(200):
            m = b"small-%d" % n
            rc = ref.verify(m, enc, zero_sig)
            if rc in want:
                want.discard(rc)
                add_verify("small_order", name + f"-msg{n}", m, enc, zero_sig)
            if not want:
                break
        assert not want, name

    # a non-canonical R for a signature that is otherwise valid: the identity
    # written as y = p + 1, under the identity key
    add_verify("noncanonical_r", "R=identity", msg, ident, zero_sig)
    add_verify("noncanonical_r", "R=p+1", msg, ident, le(M.P + 1) + le(0))
    m0, p0, s0 = signed[0]
    add_verify("noncanonical_r", "random-0-R-signbit", m0, p0, flip(s0, 255))

    for group in ("s_plus_l", "noncanonical_y", "small_order"):
        rcs = {c["rc"] for c in verify if c["group"] == group}
        assert rcs == {0, M.ERROR_INVALID_SIGNATURE}, (group, rcs)
    assert {c["rc"] for c in verify if c["name"] == "R=p+1"} == {M.ERROR_INVALID_SIGNATURE}
    return {"source": "reference NoiseSignState for Ed25519 (libnoiseref_full.so): noise_signstate_sign, "
                      "_verify, _get_public_key", "sign": sign, "verify": verify}


def main():
    fx = build()
    text = json.dumps(fx, indent=0)
    if "--check" in sys.argv[1:]:
        assert open(OUT).read() == text, "tests/golden/ed25519.json is not what the reference gives"
        print("ed25519.json: up to date")
        return
    with open(OUT, "w") as f:
        f.write(text)
    print(len(fx["sign"]), "signed,", len(fx["verify"]), "verify records,", len(text), "bytes")


if __name__ == "__main__":
    main()
