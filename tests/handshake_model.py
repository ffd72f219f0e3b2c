"""A big-step model of one Noise handshake session, the checker of the batched
device handshakes (noise_aead_dev_handshake_*, include/noise_aead_hip.h
section 8).

Hash, HKDF and AEAD are the CPU oracle's, DH is tests/x25519_ref.py; the token
table is the Noise specification's and the start-up order the reference's
(handshakestate.c:800-885): name -> h, ck; MixHash(prologue); under NoisePSK
ck, temp = HKDF(ck, psk) and MixHash(temp); MixHash of the initiator's
pre-message static key, then the responder's.  Under NoisePSK every `e` token
is also MixKey(e.public).  tests/test_handshake_model_host.py proves the model
against every Curve25519 vector of tests/golden/vectors; the same table,
written out by plan_lines(), is what tests/test_handshake_host.py holds the
host plan of csrc/handshake_plan.h to."""
import functools
import gzip
import json
import os

import x25519_ref as X

# the big-integer ladder takes a millisecond or two: batches that differ only
# in cipher and hash share their keys, and so their ladder results
dh = functools.lru_cache(maxsize=None)(X.x25519)
dh_base = functools.lru_cache(maxsize=None)(X.x25519_base)

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vectors")

ERROR_NONE, ERROR_UNKNOWN_NAME, ERROR_NOT_APPLICABLE = 0, 0x4503, 0x4505
ROLE_INITIATOR, ROLE_RESPONDER = 0x5201, 0x5202
ACTION_WRITE, ACTION_READ, ACTION_SPLIT, ACTION_COMPLETE = 0x4101, 0x4102, 0x4104, 0x4105
STATUS_OK, STATUS_MAC, STATUS_NULL_KEY = 0, 1, 3

CIPHERS = {"ChaChaPoly": 0x4301, "AESGCM": 0x4302}
HASHES = {"BLAKE2s": 0x4801, "BLAKE2b": 0x4802, "SHA256": 0x4803, "SHA512": 0x4804}
HASH_LEN = {0x4801: 32, 0x4802: 64, 0x4803: 32, 0x4804: 64}

# initiator pre-message | responder pre-message | messages (Noise specification, section 7)
_TABLE = """
N  -|s| e es
K  s|s| e es ss
X  -|s| e es s ss
NN -|-| e / e ee
NK -|s| e es / e ee
NX -|-| e / e ee s es
XN -|-| e / e ee / s se
XK -|s| e es / e ee / s se
XX -|-| e / e ee s es / s se
KN s|-| e / e ee se
KK s|s| e es ss / e ee se
KX s|-| e / e ee se s es
IN -|-| e s / e ee se
IK -|s| e es s ss / e ee se
IX -|-| e s / e ee se s es
"""


def _parse_table():
    out = {}
    for line in _TABLE.strip().splitlines():
        name, rest = line.split(None, 1)
        pre_i, pre_r, msgs = rest.split("|")
        out[name] = (pre_i.strip() == "s", pre_r.strip() == "s", [m.split() for m in msgs.split("/")])
    return out


PATTERNS = _parse_table()
DH_NAMES = ("25519", "448", "NewHope")


def parse_name(name):
    """(rc, fields): prefix_pattern_dh_cipher_hash.  In scope: the fifteen
    patterns, 25519, both ciphers, the four hashes, Noise and NoisePSK.
    Well-formed but Curve448 / NewHope / hybrid / XXfallback: NOT_APPLICABLE."""
    f = name.split("_")
    if len(f) != 5 or f[0] not in ("Noise", "NoisePSK") or f[3] not in CIPHERS or f[4] not in HASHES:
        return ERROR_UNKNOWN_NAME, None
    pat, unsupported = f[1], False
    if pat.endswith("hfs") and len(pat) > 3:
        pat, unsupported = pat[:-3], True
        if pat.endswith("+"):
            if pat != "XXfallback+":
                return ERROR_UNKNOWN_NAME, None
            pat = pat[:-1]
    if pat == "XXfallback":
        unsupported = True
    elif pat not in PATTERNS:
        return ERROR_UNKNOWN_NAME, None
    dh = f[2].split("+")
    if len(dh) > 2 or any(d not in DH_NAMES for d in dh):
        return ERROR_UNKNOWN_NAME, None
    if dh != ["25519"]:
        unsupported = True
    if unsupported:
        return ERROR_NOT_APPLICABLE, None
    return ERROR_NONE, dict(psk=f[0] == "NoisePSK", pattern=pat, cipher=CIPHERS[f[3]], hash=HASHES[f[4]])


def message_plan(pattern, initiator, psk, index):
    """(steps, overhead, keyed_in, next action) of message `index` as the
    role sees it.  A step is "e" / "e+mk" (NoisePSK), "s" / "s+aead",
    "<dh>:<local>.<remote>" with each side e or s, "p" / "p+aead"."""
    msgs = PATTERNS[pattern][2]
    keyed = False
    for m in msgs[:index]:
        keyed = keyed or any(len(t) == 2 for t in m) or (psk and "e" in m)
    keyed_in, steps, overhead = keyed, [], 0
    for t in msgs[index]:
        if t == "e":
            steps.append("e+mk" if psk else "e")
            overhead += 32
            keyed = keyed or psk
        elif t == "s":
            steps.append("s+aead" if keyed else "s")
            overhead += 48 if keyed else 32
        else:
            # the first letter is the initiator's key, the second the responder's
            mine, theirs = (t[0], t[1]) if initiator else (t[1], t[0])
            steps.append(f"{t}:{mine}.{theirs}")
            keyed = True
    steps.append("p+aead" if keyed else "p")
    overhead += 16 if keyed else 0
    if index + 1 == len(msgs):
        nxt = "split"
    else:
        nxt = "write" if ((index + 1) % 2 == 0) == initiator else "read"
    return steps, overhead, keyed_in, nxt


def needs(pattern, initiator):
    """(local static, local ephemeral, remote static) the role must bring"""
    pre_i, pre_r, msgs = PATTERNS[pattern]
    mine = [t for m in msgs[0 if initiator else 1::2] for t in m]
    return ((pre_i if initiator else pre_r) or "s" in mine, "e" in mine, pre_r if initiator else pre_i)


def plan_lines():
    """The table as asan/handshake_check prints it."""
    out = []
    for pat in PATTERNS:
        for initiator in (True, False):
            for psk in (False, True):
                who = f"{pat} {'I' if initiator else 'R'} {'NoisePSK' if psk else 'Noise'}"
                ls, le, rs = needs(pat, initiator)
                out.append(f"req {who} local_s={int(ls)} local_e={int(le)} remote_s={int(rs)} psk={int(psk)}")
                for idx in range(len(PATTERNS[pat][2])):
                    steps, overhead, keyed_in, nxt = message_plan(pat, initiator, psk, idx)
                    way = "W" if (idx % 2 == 0) == initiator else "R"
                    out.append(f"plan {who} {idx} {way} keyed_in={int(keyed_in)} steps={','.join(steps)} "
                               f"overhead={overhead} next={nxt}")
    return out


class Session:
    """One HandshakeState.  s, e: private keys (bytes or None); rs: the remote
    static public key when it is a pre-message.  status is sticky: after a
    failure write() and read() return None and split() gives zero keys."""

    def __init__(self, orc, name, initiator, prologue=b"", psk=None, s=None, e=None, rs=None):
        rc, f = parse_name(name)
        assert rc == 0, (name, hex(rc))
        self.orc, self.f, self.initiator = orc, f, initiator
        self.hid, self.cid, self.psk = f["hash"], f["cipher"], f["psk"]
        self.hl = HASH_LEN[self.hid]
        self.s, self.e, self.rs, self.re = s, e, rs, None
        self.s_pub = dh_base(s) if s else None
        self.e_pub = dh_base(e) if e else None
        self.k, self.n, self.status, self.index = None, 0, STATUS_OK, 0
        nb = name.encode()
        self.h = nb + bytes(self.hl - len(nb)) if len(nb) <= self.hl else orc.hash(self.hid, nb)
        self.ck = self.h
        self.mix_hash(prologue)
        if self.psk:
            self.ck, temp = orc.hkdf(self.hid, self.ck, psk, self.hl, self.hl)
            self.mix_hash(temp)
        pre_i, pre_r, self.msgs = PATTERNS[f["pattern"]]
        if pre_i:
            self.mix_hash(self.s_pub if initiator else rs)
        if pre_r:
            self.mix_hash(rs if initiator else self.s_pub)

    # ---- SymmetricState
    def mix_hash(self, data):
        self.h = self.orc.hash(self.hid, self.h + data)

    def mix_key(self, ikm):
        self.ck, k = self.orc.hkdf(self.hid, self.ck, ikm, self.hl, self.hl)
        self.k, self.n = k[:32], 0

    def encrypt_and_hash(self, pt):
        if self.k is None:
            ct = pt
        else:
            ct = self.orc.encrypt(self.cid, self.k, self.n, pt, self.h)
            self.n += 1
        self.mix_hash(ct)
        return ct

    def decrypt_and_hash(self, ct):
        if self.k is None:
            pt = ct
        else:
            rc, pt = self.orc.decrypt(self.cid, self.k, self.n, ct, self.h)
            if rc:
                return None
            self.n += 1
        self.mix_hash(ct)
        return pt

    def dh(self, tok):
        mine, theirs = (tok[0], tok[1]) if self.initiator else (tok[1], tok[0])
        self.mix_key(dh(self.s if mine == "s" else self.e, self.rs if theirs == "s" else self.re))

    # ---- HandshakeState
    @property
    def action(self):
        if self.index >= len(self.msgs):
            return ACTION_SPLIT
        return ACTION_WRITE if (self.index % 2 == 0) == self.initiator else ACTION_READ

    def overhead(self):
        return message_plan(self.f["pattern"], self.initiator, self.psk, self.index)[1]

    def write(self, payload):
        assert self.action == ACTION_WRITE
        toks = self.msgs[self.index]
        self.index += 1
        if self.status:
            return None
        out = b""
        for t in toks:
            if t == "e":
                out += self.e_pub
                self.mix_hash(self.e_pub)
                if self.psk:
                    self.mix_key(self.e_pub)
            elif t == "s":
                out += self.encrypt_and_hash(self.s_pub)
            else:
                self.dh(t)
        return out + self.encrypt_and_hash(payload)

    def read(self, msg):
        assert self.action == ACTION_READ
        toks = self.msgs[self.index]
        self.index += 1
        if self.status:
            return None
        for t in toks:
            if t == "e":
                self.re, msg = msg[:32], msg[32:]
                self.mix_hash(self.re)
                if self.re == bytes(32):
                    self.status = STATUS_NULL_KEY
                    return None
                if self.psk:
                    self.mix_key(self.re)
            elif t == "s":
                take = 48 if self.k is not None else 32
                self.rs = self.decrypt_and_hash(msg[:take])
                msg = msg[take:]
                if self.rs is None:
                    self.status = STATUS_MAC
                    return None
            else:
                self.dh(t)
        payload = self.decrypt_and_hash(msg)
        if payload is None:
            self.status = STATUS_MAC
        return payload

    def split(self):
        """(k1, k2, handshake hash); the initiator sends under k1"""
        assert self.action == ACTION_SPLIT
        if self.status:
            return bytes(32), bytes(32), self.h
        k1, k2 = self.orc.hkdf(self.hid, self.ck, b"", 32, 32)
        return k1, k2, self.h


def load_vectors(fname):
    with gzip.open(os.path.join(VECTORS, fname), "rt") as f:
        return json.load(f)["vectors"]


def in_scope(v):
    return parse_name(v["name"])[0] == 0 and not v.get("fallback") and not v.get("hybrid")


def vector_sessions(orc, v):
    """The initiator and responder Sessions of a vector."""
    def hx(key):
        return bytes.fromhex(v[key]) if key in v else None
    ini = Session(orc, v["name"], True, hx("init_prologue") or b"", hx("init_psk"), hx("init_static"),
                  hx("init_ephemeral"), hx("init_remote_static"))
    res = Session(orc, v["name"], False, hx("resp_prologue") or b"", hx("resp_psk"), hx("resp_static"),
                  hx("resp_ephemeral"), hx("resp_remote_static"))
    return ini, res


def one_way(pattern):
    return len(PATTERNS[pattern][2]) == 1


def run_vector(orc, v):
    """Both sides of a vector through the model; every handshake message,
    every transport message and (when recorded) the handshake hash must equal
    the vector.  Returns True when a handshake hash was compared."""
    ini, res = vector_sessions(orc, v)
    msgs = v["messages"]
    j = 0
    while ini.action != ACTION_SPLIT:
        w, r = (ini, res) if ini.action == ACTION_WRITE else (res, ini)
        payload = bytes.fromhex(msgs[j]["payload"])
        assert w.overhead() == r.overhead()
        m = w.write(payload)
        assert m.hex() == msgs[j]["ciphertext"], (v["name"], j)
        assert len(m) == len(payload) + r.overhead()
        assert r.read(m) == payload, (v["name"], j)
        j += 1
    assert res.action == ACTION_SPLIT and ini.status == 0 and res.status == 0
    k1, k2, hh = ini.split()
    assert (k1, k2, hh) == res.split()
    nonce = [0, 0]
    for t, m in enumerate(msgs[j:]):
        d = 0 if one_way(ini.f["pattern"]) else (j + t) % 2  # the directions keep alternating; 0: the initiator sends
        ct = orc.encrypt(ini.cid, (k1, k2)[d], nonce[d], bytes.fromhex(m["payload"]))
        nonce[d] += 1
        assert ct.hex() == m["ciphertext"], (v["name"], "transport", t)
    if "handshake_hash" in v:
        assert hh.hex() == v["handshake_hash"], v["name"]
        return True
    return False
