"""Generate tests/golden/handshake_lengths.json from the reference noise-c itself.

Runs noise_handshakestate_write_message / _read_message
(src/protocol/handshakestate.c:1151-1340, 1419-1602) of the reference library
compiled from its own sources by oracle/Makefile (target `full`,
oracle/_ref/libnoiseref_full.so) with fixed keys and a different payload
length in every message, the lengths taken in turn from LENGTHS: the edges of
the 16-byte AEAD block and of the 64- and 128-byte hash blocks of h || data.

Per case (in the format of tests/golden/vectors, so that the model and the GPU
tests read it like a vector): the keys, every message with its payload, the
handshake hash and both split keys.  The reference has no accessor for the
split keys: ck is read from the SymmetricState just before the split (the 64
bytes in front of h, which noise_handshakestate_get_handshake_hash gives),
k1, k2 = the reference's own noise_hashstate_hkdf(ck, "") as in
symmetricstate.c:530-533, and both are then proved through the public API: a
CipherState keyed with them must encrypt as the CipherStates the reference's
split returned.

Also per case and message, `faults`: the return code of a read of the message
cut to 0, overhead - 1 and overhead bytes, and of a write into a buffer one
byte too small, each on fresh states run up to that message.  All ephemerals
are non-zero.  Build-container only; the JSON is the committed fixture.

Usage: python tests/golden/gen_handshake_lengths.py
"""
import ctypes as C
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "..", "oracle", "_ref", "libnoiseref_full.so")
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 111, 112, 127, 128, 129, 257]
SUITES = ["25519_ChaChaPoly_BLAKE2s", "25519_AESGCM_SHA512"]
PROTOCOLS = ["Noise_NN", "Noise_XX", "NoisePSK_IK", "Noise_N"]
INITIATOR, RESPONDER = 0x5201, 0x5202
WRITE, READ, SPLIT = 0x4101, 0x4102, 0x4104
HASH_OF = {"BLAKE2s": (0x4801, 32), "SHA512": (0x4804, 64)}
CIPHER_OF = {"ChaChaPoly": 0x4301, "AESGCM": 0x4302}
MAX_HASHLEN = 64


class Buffer(C.Structure):
    _fields_ = [("data", C.c_void_p), ("size", C.c_size_t), ("max_size", C.c_size_t)]


def load():
    L = C.CDLL(LIB)
    vp, sz = C.c_void_p, C.c_size_t
    sig = {
        "noise_handshakestate_new_by_name": (C.c_int, [C.POINTER(vp), C.c_char_p, C.c_int]),
        "noise_handshakestate_free": (C.c_int, [vp]),
        "noise_handshakestate_get_local_keypair_dh": (vp, [vp]),
        "noise_handshakestate_get_remote_public_key_dh": (vp, [vp]),
        "noise_handshakestate_get_fixed_ephemeral_dh": (vp, [vp]),
        "noise_handshakestate_needs_pre_shared_key": (C.c_int, [vp]),
        "noise_handshakestate_set_pre_shared_key": (C.c_int, [vp, C.c_char_p, sz]),
        "noise_handshakestate_set_prologue": (C.c_int, [vp, C.c_char_p, sz]),
        "noise_handshakestate_needs_local_keypair": (C.c_int, [vp]),
        "noise_handshakestate_needs_remote_public_key": (C.c_int, [vp]),
        "noise_handshakestate_start": (C.c_int, [vp]),
        "noise_handshakestate_get_action": (C.c_int, [vp]),
        "noise_handshakestate_write_message": (C.c_int, [vp, C.POINTER(Buffer), C.POINTER(Buffer)]),
        "noise_handshakestate_read_message": (C.c_int, [vp, C.POINTER(Buffer), C.POINTER(Buffer)]),
        "noise_handshakestate_split": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
        "noise_handshakestate_get_handshake_hash": (C.c_int, [vp, vp, sz]),
        "noise_dhstate_set_keypair_private": (C.c_int, [vp, C.c_char_p, sz]),
        "noise_dhstate_set_public_key": (C.c_int, [vp, C.c_char_p, sz]),
        "noise_dhstate_get_public_key": (C.c_int, [vp, vp, sz]),
        "noise_hashstate_new_by_id": (C.c_int, [C.POINTER(vp), C.c_int]),
        "noise_hashstate_hkdf": (C.c_int, [vp, C.c_char_p, sz, C.c_char_p, sz, vp, sz, vp, sz]),
        "noise_hashstate_free": (C.c_int, [vp]),
        "noise_cipherstate_new_by_id": (C.c_int, [C.POINTER(vp), C.c_int]),
        "noise_cipherstate_init_key": (C.c_int, [vp, C.c_char_p, sz]),
        "noise_cipherstate_encrypt": (C.c_int, [vp, C.POINTER(Buffer)]),
        "noise_cipherstate_free": (C.c_int, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


class Ref:
    """One HandshakeState of the reference with fixed keys."""

    def __init__(self, L, name, role, keys):
        self.L, self.keep = L, []
        st = C.c_void_p()
        assert L.noise_handshakestate_new_by_name(C.byref(st), name.encode(), role) == 0, name
        self.st = st
        me = "init" if role == INITIATOR else "resp"
        self.static_pub = None
        if L.noise_handshakestate_needs_local_keypair(st):
            dh = L.noise_handshakestate_get_local_keypair_dh(st)
            assert L.noise_dhstate_set_keypair_private(dh, keys[me + "_static"], 32) == 0
            pub = C.create_string_buffer(32)
            assert L.noise_dhstate_get_public_key(dh, pub, 32) == 0
            self.static_pub = pub.raw
        dh = L.noise_handshakestate_get_fixed_ephemeral_dh(st)
        if dh and keys.get(me + "_ephemeral"):
            assert L.noise_dhstate_set_keypair_private(dh, keys[me + "_ephemeral"], 32) == 0
        if L.noise_handshakestate_needs_pre_shared_key(st):
            assert L.noise_handshakestate_set_pre_shared_key(st, keys["psk"], 32) == 0
        if keys["prologue"]:
            assert L.noise_handshakestate_set_prologue(st, keys["prologue"], len(keys["prologue"])) == 0

    def needs_remote(self):
        return bool(self.L.noise_handshakestate_needs_remote_public_key(self.st))

    def set_remote(self, pub):
        dh = self.L.noise_handshakestate_get_remote_public_key_dh(self.st)
        assert self.L.noise_dhstate_set_public_key(dh, pub, 32) == 0

    def start(self):
        assert self.L.noise_handshakestate_start(self.st) == 0

    @property
    def action(self):
        return self.L.noise_handshakestate_get_action(self.st)

    def write(self, payload, room=65535):
        """(rc, message)"""
        out = C.create_string_buffer(max(room, 1))
        pay = C.create_string_buffer(payload, max(len(payload), 1))
        mb = Buffer(C.addressof(out), 0, room)
        pb = Buffer(C.addressof(pay), len(payload), len(payload))
        rc = self.L.noise_handshakestate_write_message(self.st, C.byref(mb), C.byref(pb))
        return rc, out.raw[:mb.size] if rc == 0 else None

    def read(self, msg):
        """(rc, payload)"""
        inp = C.create_string_buffer(msg, max(len(msg), 1))
        out = C.create_string_buffer(65535)
        mb = Buffer(C.addressof(inp), len(msg), len(msg))
        pb = Buffer(C.addressof(out), 0, 65535)
        rc = self.L.noise_handshakestate_read_message(self.st, C.byref(mb), C.byref(pb))
        return rc, out.raw[:pb.size] if rc == 0 else None

    def handshake_hash(self, hl):
        h = C.create_string_buffer(hl)
        assert self.L.noise_handshakestate_get_handshake_hash(self.st, h, hl) == 0
        return h.raw

    def chaining_key(self, hl):
        """ck of the SymmetricState: the NOISE_MAX_HASHLEN bytes in front of h"""
        words = C.cast(self.st, C.POINTER(C.c_size_t))
        sym = words[4]  # size, role/requirements/action, tokens, symmetric
        size = C.cast(sym, C.POINTER(C.c_size_t))[0]
        assert 2 * MAX_HASHLEN < size < 4096, size
        raw = C.string_at(sym, size)
        h = self.handshake_hash(hl)
        at = raw.rfind(h + bytes(MAX_HASHLEN - hl))
        assert at == size - MAX_HASHLEN, (at, size)
        return raw[at - MAX_HASHLEN: at - MAX_HASHLEN + hl]

    def split(self):
        send, recv = C.c_void_p(), C.c_void_p()
        assert self.L.noise_handshakestate_split(self.st, C.byref(send), C.byref(recv)) == 0
        return send, recv

    def free(self):
        self.L.noise_handshakestate_free(self.st)


def encrypt_once(L, cs, pt):
    buf = C.create_string_buffer(pt, len(pt) + 16)
    b = Buffer(C.addressof(buf), len(pt), len(pt) + 16)
    assert L.noise_cipherstate_encrypt(cs, C.byref(b)) == 0
    return buf.raw[:b.size]


def make_pair(L, name, keys):
    ini, res = Ref(L, name, INITIATOR, keys), Ref(L, name, RESPONDER, keys)
    # who needs the other's static key before the start: a pre-message
    ini.pre_remote, res.pre_remote = ini.needs_remote(), res.needs_remote()
    if ini.pre_remote:
        ini.set_remote(res.static_pub)
    if res.pre_remote:
        res.set_remote(ini.static_pub)
    ini.start()
    res.start()
    return ini, res


def run_to(L, name, keys, payloads, upto):
    """fresh states after `upto` messages: (writer, reader) of the next one"""
    ini, res = make_pair(L, name, keys)
    for j in range(upto):
        w, r = (ini, res) if ini.action == WRITE else (res, ini)
        rc, m = w.write(payloads[j])
        assert rc == 0
        assert r.read(m) == (0, payloads[j])
    return (ini, res) if ini.action == WRITE else (res, ini)


def main():
    L = load()
    rnd = random.Random(0x48534C4E)

    def rand(n):
        return bytes(rnd.getrandbits(8) for _ in range(n))

    cases, turn, used = [], 0, set()
    for variant in range(2):
        for suite in SUITES:
            for proto in PROTOCOLS:
                name = f"{proto}_{suite}"
                hid, hl = HASH_OF[suite.split("_")[2]]
                cid = CIPHER_OF[suite.split("_")[1]]
                keys = {"init_static": rand(32), "init_ephemeral": rand(32), "resp_static": rand(32),
                        "resp_ephemeral": rand(32), "psk": rand(32), "prologue": rand(11) if variant else b""}
                ini, res = make_pair(L, name, keys)
                case = {"name": name, "pattern": proto.split("_")[1], "messages": [], "faults": []}
                if ini.static_pub:
                    case["init_static"] = keys["init_static"].hex()
                if res.static_pub:
                    case["resp_static"] = keys["resp_static"].hex()
                case["init_ephemeral"] = keys["init_ephemeral"].hex()
                payloads = []
                if ini.pre_remote:
                    case["init_remote_static"] = res.static_pub.hex()
                if res.pre_remote:
                    case["resp_remote_static"] = ini.static_pub.hex()
                if proto.startswith("NoisePSK"):
                    case["init_psk"] = case["resp_psk"] = keys["psk"].hex()
                if keys["prologue"]:
                    case["init_prologue"] = case["resp_prologue"] = keys["prologue"].hex()
                while ini.action != SPLIT:
                    w, r = (ini, res) if ini.action == WRITE else (res, ini)
                    assert r.action == READ
                    plen = LENGTHS[turn % len(LENGTHS)]
                    turn += 5  # 5 and 17 are coprime: every length comes up
                    used.add(plen)
                    payload = rand(plen)
                    rc, m = w.write(payload)
                    assert rc == 0
                    assert r.read(m) == (0, payload)
                    if w is res:
                        case["resp_ephemeral"] = keys["resp_ephemeral"].hex()
                    payloads.append(payload)
                    case["messages"].append({"payload": payload.hex(), "ciphertext": m.hex()})
                assert res.action == SPLIT
                hh = ini.handshake_hash(hl)
                assert hh == res.handshake_hash(hl)
                ck = ini.chaining_key(hl)
                assert ck == res.chaining_key(hl)
                hs = C.c_void_p()
                assert L.noise_hashstate_new_by_id(C.byref(hs), hid) == 0
                o1, o2 = C.create_string_buffer(32), C.create_string_buffer(32)
                assert L.noise_hashstate_hkdf(hs, ck, hl, b"\0", 0, o1, 32, o2, 32) == 0
                L.noise_hashstate_free(hs)
                k1, k2 = o1.raw, o2.raw
                # the proof through the public API: the initiator sends under k1, receives under k2
                send, recv = ini.split()
                probe = rand(40)
                for key, cs in ((k1, send), (k2, recv)):
                    mine = C.c_void_p()
                    assert L.noise_cipherstate_new_by_id(C.byref(mine), cid) == 0
                    assert L.noise_cipherstate_init_key(mine, key, 32) == 0
                    assert encrypt_once(L, mine, probe) == encrypt_once(L, cs, probe), name
                    L.noise_cipherstate_free(mine)
                    L.noise_cipherstate_free(cs)
                case["handshake_hash"], case["k1"], case["k2"] = hh.hex(), k1.hex(), k2.hex()
                ini.free()
                res.free()
                # the length faults, each on fresh states
                for j, msg in enumerate(case["messages"]):
                    whole = bytes.fromhex(msg["ciphertext"])
                    over = len(whole) - len(payloads[j])
                    for cut in (0, over - 1, over):
                        w, r = run_to(L, name, keys, payloads, j)
                        rc, _ = r.read(whole[:cut])
                        case["faults"].append({"message": j, "kind": "read_cut", "length": cut, "rc": rc})
                        w.free()
                        r.free()
                    w, r = run_to(L, name, keys, payloads, j)
                    room = len(whole) - 1
                    rc, _ = w.write(payloads[j], room)
                    case["faults"].append({"message": j, "kind": "write_small", "room": room, "rc": rc})
                    w.free()
                    r.free()
                cases.append(case)
    assert used == set(LENGTHS), sorted(set(LENGTHS) - used)
    with open(os.path.join(HERE, "handshake_lengths.json"), "w") as f:
        json.dump({"source": "reference noise_handshakestate_write_message / _read_message (libnoiseref_full.so)",
                   "lengths": LENGTHS, "cases": cases}, f, indent=1)
    print(len(cases), "cases,", sum(len(c["messages"]) for c in cases), "messages,",
          sum(len(c["faults"]) for c in cases), "faults")


if __name__ == "__main__":
    main()
