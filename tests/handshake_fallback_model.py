"""The Noise Pipes fallback beside tests/handshake_model.py: what
noise_aead_dev_handshake_fallback and _fallback_merge (include/noise_aead_hip.h
section 15) do, for one session.

A fallback turns a handshake of NK, XK, KK or IK that has done exactly one
message into an XXfallback handshake with the roles swapped
(handshakestate.c:973-1079): the former responder becomes the initiator,
keeps the ephemeral it received and its static key pair and brings a fresh
ephemeral; the former initiator becomes the responder and keeps its ephemeral
and its static key pair.  Start-up (:822-877): the new name -> h, ck;
MixHash(prologue); the PSK step; then the pre-message, MixHash of the former
initiator's ephemeral and, under NoisePSK, MixKey of it.

handshake_model.Session is used as it is, by composition: Fallback builds a
Session without its constructor (whose name parser refuses XXfallback by
design), fills in the state above and hands every message, the split and the
status to it."""
import handshake_model as M

XXFALLBACK = [["e", "ee", "s", "se"], ["s", "es"]]  # after the pre-message <- e
FALLBACK_FROM = ("NK", "XK", "KK", "IK")  # interactive, the responder's static key known beforehand
FALLBACK_ONLY_FAILED = 1
STATUS_LENGTH, STATUS_ABSENT = 4, 5
ERROR_LOCAL_KEY_REQUIRED, ERROR_PSK_REQUIRED = 0x4508, 0x4509
ERROR_INVALID_PARAM, ERROR_INVALID_STATE = 0x450B, 0x450C


def fallback_name(name):
    f = name.split("_")
    f[1] = "XXfallback"
    return "_".join(f)


def eligible(status, was_initiator):
    """a former responder that verified (0) or failed (1) the first message, a
    former initiator that wrote it (0); 3 and 4 hold no usable ephemeral"""
    return status == M.STATUS_OK or (status == M.STATUS_MAC and not was_initiator)


def takes(status, selected, flags, was_initiator):
    if not eligible(status, was_initiator) or not selected:
        return False
    return status == M.STATUS_MAC if flags & FALLBACK_ONLY_FAILED else True


def message_plan(initiator, psk, index):
    """(steps, overhead, keyed_in, next action) of XXfallback's message
    `index`, in the words of handshake_model.message_plan"""
    keyed = psk or index > 0  # the pre-message e is a MixKey under NoisePSK
    keyed_in, steps, overhead = keyed, [], 0
    for t in XXFALLBACK[index]:
        if t == "e":
            steps.append("e+mk" if psk else "e")
            overhead += 32
            keyed = keyed or psk
        elif t == "s":
            steps.append("s+aead" if keyed else "s")
            overhead += 48 if keyed else 32
        else:
            mine, theirs = (t[0], t[1]) if initiator else (t[1], t[0])
            steps.append(f"{t}:{mine}.{theirs}")
            keyed = True
    steps.append("p+aead" if keyed else "p")
    overhead += 16 if keyed else 0
    nxt = "split" if index == 1 else ("read" if initiator else "write")
    return steps, overhead, keyed_in, nxt


def plan_lines():
    """the fallback plan as asan/handshake_fallback_check prints it"""
    out = []
    for initiator in (True, False):
        for psk in (False, True):
            who = f"XXfallback {'I' if initiator else 'R'} {'NoisePSK' if psk else 'Noise'}"
            out.append(f"req {who} local_s=1 local_e=1 remote_s=0 remote_e={int(initiator)} psk={int(psk)}")
            for idx in range(2):
                steps, overhead, keyed_in, nxt = message_plan(initiator, psk, idx)
                way = "W" if (idx % 2 == 0) == initiator else "R"
                out.append(f"plan {who} {idx} {way} keyed_in={int(keyed_in)} steps={','.join(steps)} "
                           f"overhead={overhead} next={nxt}")
    return out


def check(sess, psk=None, e=None):
    """the return code of a fallback of `sess` (a handshake_model.Session, or a
    Fallback, which never falls back again), in the order of the header"""
    if isinstance(sess, Fallback) or sess.f["pattern"] not in FALLBACK_FROM:
        return M.ERROR_NOT_APPLICABLE
    if sess.index != 1:
        return ERROR_INVALID_STATE
    if sess.s is None or (not sess.initiator and e is None):
        return ERROR_LOCAL_KEY_REQUIRED
    if sess.psk and psk is None:
        return ERROR_PSK_REQUIRED
    return M.ERROR_NONE


class Fallback:
    """One XXfallback HandshakeState made of `sess`; write, read, split,
    action, status and the keys are the inner Session's."""

    def __init__(self, orc, sess, prologue=b"", psk=None, e=None):
        assert check(sess, psk, e) == 0
        name = fallback_name("_".join(["NoisePSK" if sess.psk else "Noise", sess.f["pattern"], "25519",
                                       next(k for k, v in M.CIPHERS.items() if v == sess.cid),
                                       next(k for k, v in M.HASHES.items() if v == sess.hid)]))
        x = M.Session.__new__(M.Session)
        x.orc, x.initiator = orc, not sess.initiator
        x.f = dict(sess.f, pattern="XXfallback")
        x.hid, x.cid, x.psk, x.hl = sess.hid, sess.cid, sess.psk, sess.hl
        x.s, x.s_pub, x.rs = sess.s, sess.s_pub, None
        if x.initiator:  # the former responder: the received e stays, a fresh e of its own
            x.e, x.e_pub, x.re = e, M.dh_base(e), sess.re
        else:
            x.e, x.e_pub, x.re = sess.e, sess.e_pub, None
        x.k, x.n, x.status, x.index = None, 0, M.STATUS_OK, 0
        nb = name.encode()
        x.h = nb + bytes(x.hl - len(nb)) if len(nb) <= x.hl else orc.hash(x.hid, nb)
        x.ck = x.h
        x.mix_hash(prologue)
        if x.psk:
            x.ck, temp = orc.hkdf(x.hid, x.ck, psk, x.hl, x.hl)
            x.mix_hash(temp)
        pre = x.re if x.initiator else x.e_pub
        x.mix_hash(pre)
        if x.psk:
            x.mix_key(pre)
        x.msgs = XXFALLBACK
        self.name, self.x = name, x

    def overhead(self):
        return message_plan(self.x.initiator, self.x.psk, self.x.index)[1]

    def __getattr__(self, key):  # write, read, split, action, status, initiator, h, rs, ...
        return getattr(self.x, key)


def fallback(orc, sess, prologue=b"", psk=None, e=None, selected=True, flags=0):
    """One session of noise_aead_dev_handshake_fallback: (rc, fb).  fb is a
    Fallback when the session takes part — sess.status 0 then becomes 5 — and
    STATUS_ABSENT when it does not; None when the call is refused."""
    rc = check(sess, psk, e)
    if rc:
        return rc, None
    if not takes(sess.status, selected, flags, sess.initiator):
        return 0, STATUS_ABSENT
    fb = Fallback(orc, sess, prologue, psk, e)
    if sess.status == M.STATUS_OK:
        sess.status = STATUS_ABSENT
    return 0, fb


def merge(fb_status, fb_split, hs_status, hs_split):
    """One session of noise_aead_dev_handshake_fallback_merge: (k1, k2, h,
    status) from the two splits (k1, k2, h) — the fallback's keys swapped into
    the original role's orientation."""
    if fb_status == STATUS_ABSENT:
        return hs_split[0], hs_split[1], hs_split[2], hs_status
    if fb_status:
        return bytes(32), bytes(32), bytes(len(hs_split[2])), fb_status
    return fb_split[1], fb_split[0], fb_split[2], 0


def fallback_vectors():
    return [v for v in M.load_vectors("noise-c-fallback.txt.gz") if v["dh"] == "25519"]


def original_name(v):
    """the protocol the vector starts with: its name with the vector's pattern"""
    f = v["name"].split("_")
    f[1] = v["pattern"]
    return "_".join(f)


def vector_sessions(orc, v):
    """The two IK Sessions a fallback vector starts with."""
    return M.vector_sessions(orc, dict(v, name=original_name(v)))


def run_vector(orc, v):
    """A fallback vector through the model: the first message (which the
    responder must refuse), the fallback of both sides, the two fallback
    messages, the handshake hash and the transport messages equal the
    vector.  Returns the Fallback pair."""
    def hx(key):
        return bytes.fromhex(v[key]) if key in v else None
    ini, res = vector_sessions(orc, v)
    msgs = v["messages"]
    p0 = bytes.fromhex(msgs[0]["payload"])
    m0 = ini.write(p0)
    assert m0.hex() == msgs[0]["ciphertext"] and len(m0) == len(p0) + 96, (v["name"], 0)
    assert res.read(m0) is None and res.status == M.STATUS_MAC, (v["name"], "the first message verified")
    rc, fr = fallback(orc, res, hx("resp_prologue") or b"", hx("resp_psk"), hx("resp_ephemeral"))
    assert rc == 0 and res.status == M.STATUS_MAC
    rc, fi = fallback(orc, ini, hx("init_prologue") or b"", hx("init_psk"))
    assert rc == 0 and ini.status == STATUS_ABSENT
    assert fr.name == fi.name == v["name"]
    for j, (w, r) in ((1, (fr, fi)), (2, (fi, fr))):
        assert w.action == M.ACTION_WRITE and r.action == M.ACTION_READ
        payload = bytes.fromhex(msgs[j]["payload"])
        assert w.overhead() == r.overhead() == (96, 64)[j - 1]
        m = w.write(payload)
        assert m.hex() == msgs[j]["ciphertext"], (v["name"], j)
        assert r.read(m) == payload, (v["name"], j)
    assert fr.action == fi.action == M.ACTION_SPLIT and fr.status == fi.status == 0
    k1, k2, hh = fr.split()
    assert (k1, k2, hh) == fi.split()
    assert hh.hex() == v["handshake_hash"], v["name"]
    # the directions keep alternating: message 3 is the former responder's, the fallback's initiator, under k1
    nonce = [0, 0]
    for t, m in enumerate(msgs[3:]):
        d = t % 2
        ct = orc.encrypt(fr.cid, (k1, k2)[d], nonce[d], bytes.fromhex(m["payload"]))
        nonce[d] += 1
        assert ct.hex() == m["ciphertext"], (v["name"], "transport", t)
    return fr, fi
