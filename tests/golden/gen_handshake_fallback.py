"""Generate tests/golden/handshake_fallback.json from the reference noise-c itself.

Runs noise_handshakestate_fallback and the noise_handshakestate_start after it
(src/protocol/handshakestate.c:888-1079, :800-885) of the reference library
compiled from its own sources by oracle/Makefile (target `full`,
oracle/_ref/libnoiseref_full.so), for what the 16 Curve25519 vectors of
tests/golden/vectors/noise-c-fallback.txt.gz do not reach: the originals XK,
KK and NK (the responder's side: the NK initiator has no static key) besides
IK; a fallback after a first message that verified; a fallback prologue that
differs from the original's, of another length, and an empty one; both
ciphers, BLAKE2s and SHA512, Noise and NoisePSK.

Per case: the keys, the original's first message, the fallback's messages
(both, or the first alone where only the responder can fall back), the
handshake hash and both split keys (ck read and proved through the public API
as tests/golden/gen_handshake_lengths.py does, whose reference wrapper this
script uses).  `refusals`: the return codes of the reference for a fallback
that cannot be: NN or XX as the original, before any message, after two
messages, and the start of the NK initiator.  Only recorded bytes and codes
go into the fixture.  Build-container only; the JSON is the committed fixture.

Usage: python tests/golden/gen_handshake_fallback.py
"""
import ctypes as C
import json
import os
import random

import gen_handshake_lengths as G

HERE = os.path.dirname(os.path.abspath(__file__))
SUITES = ["25519_ChaChaPoly_BLAKE2s", "25519_AESGCM_SHA512"]
ORIGINALS = ["IK", "XK", "KK", "NK"]
# (the first message verifies, the original's prologue length, the fallback's)
VARIANTS = [(False, 11, 11), (True, 5, 23), (False, 9, 0), (True, 0, 7)]
INITIATOR, RESPONDER, WRITE, READ, SPLIT = G.INITIATOR, G.RESPONDER, G.WRITE, G.READ, G.SPLIT


def load():
    L = G.load()
    L.noise_handshakestate_fallback.restype = C.c_int
    L.noise_handshakestate_fallback.argtypes = [C.c_void_p]
    return L


def pair(L, name, keys, stale):
    """both ends of the original after start; stale: the initiator holds an old responder key"""
    ini, res = G.Ref(L, name, INITIATOR, keys), G.Ref(L, name, RESPONDER, keys)
    if ini.needs_remote():
        ini.rs = keys["old_pub"] if stale else res.static_pub
        ini.set_remote(ini.rs)
    if res.needs_remote():
        res.set_remote(ini.static_pub)
        res.rs = ini.static_pub
    ini.start()
    res.start()
    return ini, res


def restart(L, ref, keys, fresh_e=None):
    """(rc of the fallback, rc of the start after it); the fallback's own prologue and ephemeral"""
    rc = L.noise_handshakestate_fallback(ref.st)
    if rc:
        return rc, None
    assert L.noise_handshakestate_set_prologue(ref.st, keys["fb_prologue"] or b"\0", len(keys["fb_prologue"])) == 0
    if fresh_e:
        dh = L.noise_handshakestate_get_fixed_ephemeral_dh(ref.st)
        assert L.noise_dhstate_set_keypair_private(dh, fresh_e, 32) == 0
    return rc, L.noise_handshakestate_start(ref.st)


def split_keys(L, ref, hid, hl, cid, rand):
    """(k1, k2) of a finished HandshakeState, proved through the public API; `ref` is the fallback's initiator"""
    ck = ref.chaining_key(hl)
    hs = C.c_void_p()
    assert L.noise_hashstate_new_by_id(C.byref(hs), hid) == 0
    o1, o2 = C.create_string_buffer(32), C.create_string_buffer(32)
    assert L.noise_hashstate_hkdf(hs, ck, hl, b"\0", 0, o1, 32, o2, 32) == 0
    L.noise_hashstate_free(hs)
    send, recv = ref.split()
    probe = rand(40)
    for key, cs in ((o1.raw, send), (o2.raw, recv)):
        mine = C.c_void_p()
        assert L.noise_cipherstate_new_by_id(C.byref(mine), cid) == 0
        assert L.noise_cipherstate_init_key(mine, key, 32) == 0
        assert G.encrypt_once(L, mine, probe) == G.encrypt_once(L, cs, probe)
        L.noise_cipherstate_free(mine)
        L.noise_cipherstate_free(cs)
    return o1.raw, o2.raw


def main():
    L = load()
    rnd = random.Random(0x46424B)

    def rand(n):
        return bytes(rnd.getrandbits(8) for _ in range(n))

    def new_keys(variant):
        verified, plen, fplen = VARIANTS[variant]
        keys = {"init_static": rand(32), "init_ephemeral": rand(32), "resp_static": rand(32),
                "resp_ephemeral": rand(32), "fresh": rand(32), "psk": rand(32), "prologue": rand(plen),
                "fb_prologue": rand(fplen), "old": rand(32)}
        pub = G.Ref(L, "Noise_NK_25519_ChaChaPoly_BLAKE2s", RESPONDER, dict(keys, resp_static=keys["old"], prologue=b""))
        keys["old_pub"] = pub.static_pub
        pub.free()
        return keys, verified

    cases, turn = [], 0
    for suite in SUITES:
        hid, hl = G.HASH_OF[suite.split("_")[2]]
        cid = G.CIPHER_OF[suite.split("_")[1]]
        for prefix in ("Noise", "NoisePSK"):
            for orig in ORIGINALS:
                for variant in range(len(VARIANTS)):
                    name = f"{prefix}_{orig}_{suite}"
                    keys, verified = new_keys(variant)
                    ini, res = pair(L, name, keys, stale=not verified)
                    both = ini.static_pub is not None  # the NK initiator cannot fall back
                    case = {"name": name, "pattern": orig, "first_verified": verified, "both_sides": both,
                            "resp_static": keys["resp_static"].hex(), "init_ephemeral": keys["init_ephemeral"].hex(),
                            "resp_ephemeral": keys["resp_ephemeral"].hex(), "fresh_ephemeral": keys["fresh"].hex(),
                            "init_remote_static": ini.rs.hex(), "prologue": keys["prologue"].hex(),
                            "fb_prologue": keys["fb_prologue"].hex(), "messages": []}
                    if both:
                        case["init_static"] = keys["init_static"].hex()
                    if res.needs_remote() or getattr(res, "rs", None):
                        case["resp_remote_static"] = res.rs.hex()
                    if prefix == "NoisePSK":
                        case["psk"] = keys["psk"].hex()
                    lens = [G.LENGTHS[(turn + 5 * j) % len(G.LENGTHS)] for j in range(3)]
                    turn += 1
                    payload = rand(lens[0])
                    rc, m = ini.write(payload)
                    assert rc == 0
                    rc, back = res.read(m)
                    assert (rc == 0 and back == payload) if verified else rc == 0x4504, (name, hex(rc))
                    case["messages"].append({"payload": payload.hex(), "ciphertext": m.hex()})
                    assert restart(L, res, keys, keys["fresh"]) == (0, 0), name
                    got = restart(L, ini, keys)
                    assert got == ((0, 0) if both else (0, 0x4508)), (name, got)
                    assert res.action == WRITE
                    payload = rand(lens[1])
                    rc, m = res.write(payload)
                    assert rc == 0 and len(m) == len(payload) + 96
                    case["messages"].append({"payload": payload.hex(), "ciphertext": m.hex()})
                    if both:
                        assert ini.action == READ and ini.read(m) == (0, payload)
                        payload = rand(lens[2])
                        rc, m = ini.write(payload)
                        assert rc == 0 and len(m) == len(payload) + 64 and res.read(m) == (0, payload)
                        case["messages"].append({"payload": payload.hex(), "ciphertext": m.hex()})
                        assert ini.action == res.action == SPLIT
                        hh = res.handshake_hash(hl)
                        assert hh == ini.handshake_hash(hl) and res.chaining_key(hl) == ini.chaining_key(hl)
                        k1, k2 = split_keys(L, res, hid, hl, cid, rand)
                        case["handshake_hash"], case["k1"], case["k2"] = hh.hex(), k1.hex(), k2.hex()
                    ini.free()
                    res.free()
                    cases.append(case)

    # the refusals: (name, messages done before the call)
    refusals = []
    suite = SUITES[0]
    for name, done in ((f"Noise_NN_{suite}", 1), (f"Noise_XX_{suite}", 1), (f"NoisePSK_XX_{suite}", 1),
                       (f"Noise_IK_{suite}", 0), (f"Noise_XK_{suite}", 0), (f"Noise_IK_{suite}", 2),
                       (f"Noise_XK_{suite}", 2), (f"Noise_KK_{suite}", 2), (f"Noise_NK_{suite}", 1),
                       (f"NoisePSK_NK_{suite}", 1)):
        for role in (INITIATOR, RESPONDER):
            keys, _ = new_keys(0)
            ini, res = pair(L, name, keys, stale=False)
            for _ in range(done):
                w, r = (ini, res) if ini.action == WRITE else (res, ini)
                rc, m = w.write(b"abc")
                assert rc == 0 and r.read(m) == (0, b"abc")
            me = ini if role == INITIATOR else res
            rc, rc_start = restart(L, me, keys, None if role == INITIATOR else keys["fresh"])
            refusals.append({"name": name, "role": role, "messages_done": done, "fallback_rc": rc, "start_rc": rc_start})
            ini.free()
            res.free()
    with open(os.path.join(HERE, "handshake_fallback.json"), "w") as f:
        json.dump({"source": "reference noise_handshakestate_fallback / _start (libnoiseref_full.so)",
                   "cases": cases, "refusals": refusals}, f, indent=1)
    print(len(cases), "cases,", sum(len(c["messages"]) for c in cases), "messages,", len(refusals), "refusals")


if __name__ == "__main__":
    main()
