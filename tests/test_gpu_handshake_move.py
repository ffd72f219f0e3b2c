"""Sessions that change their object, on the device:
noise_aead_dev_handshake_new_like, _move and _drop (include/noise_aead_hip.h
section 16) against the model of tests/handshake_move_model.py.

Sessions are independent, so what a session writes, reads and splits to is
what its tests/handshake_model.Session says — proved against the vectors —
whichever objects it passed through: every message, payload, split key,
handshake hash, status byte and result byte here is held to the models."""
import numpy as np
import pytest

import handshake_fallback_gpu as FG
import handshake_fallback_model as F
import handshake_model as M
import handshake_move_model as V
import transport_model as T
from gpu_support import dev_u32
from handshake_gpu import CANARY, Buf, Side, basic_vector, handshake, make_sessions, model_pair, payload_rows
from transport_gpu import Table, Wire

pytestmark = pytest.mark.gpu
XX = "Noise_XX_25519_ChaChaPoly_BLAKE2s"
XX_PSK = "NoisePSK_XX_25519_AESGCM_SHA512"


def rand_rows(seed, n, length):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, max(length, 1), dtype=np.uint8).tobytes()[:length] for _ in range(n)]


def tag(models):
    """session ids: what a message or a key is filed under while its session changes lanes"""
    for i, m in enumerate(models):
        m.sid = i
    return models


class Box:
    """One device handshake object (a handshake_gpu.Side) beside its model (a V.Obj)."""

    def __init__(self, side, sessions=None, model=None):
        self.side, self.A, self.torch = side, side.A, side.torch
        self.model = model if model is not None else V.Obj(side.n, sessions=sessions)

    @property
    def n(self):
        return self.side.n

    def like(self, capacity):
        """_new_like: an empty object at this one's position"""
        rc, hs = self.A.dev_handshake_new_like(self.side.hs, capacity, stream=self.side.sp)
        assert rc == 0 and hs, ("new_like", hex(rc))
        side = Side.__new__(Side)
        side.A, side.torch, side.name, side.n, side.hs = self.A, self.torch, self.side.name, capacity, hs
        side.keep, side.sp = self.side.keep, self.side.sp  # a key held once for all stays the caller's
        box = Box(side, model=V.Obj.like(self.model, capacity))
        assert side.action == self.side.action and side.overhead == self.side.overhead
        box.check()
        return box

    def check(self):
        assert self.side.status() == self.model.status()

    def lane_of(self, sid):
        return next(l for l, s in enumerate(self.model.lanes) if s is not None and s.sid == sid)

    def free(self):
        self.side.free()


def move(dst, src, m, dst_lanes=None, src_lanes=None, with_result=True):
    """_move on the device and in the model: the result bytes and both status arrays"""
    torch = dst.torch
    d = dev_u32(dst_lanes) if dst_lanes is not None else None
    s = dev_u32(src_lanes) if src_lanes is not None else None
    res = torch.full((m + 8,), CANARY, dtype=torch.uint8, device="cuda")
    rc = dst.A.dev_handshake_move(dst.side.hs, src.side.hs, m, dst_lanes=d.data_ptr() if d is not None else 0,
                                  src_lanes=s.data_ptr() if s is not None else 0,
                                  result=res.data_ptr() if with_result else 0, stream=dst.side.sp)
    assert rc == 0, ("move", hex(rc))
    want = V.move(dst.model, dst_lanes, src.model, src_lanes, m)
    torch.cuda.synchronize()
    got = res.cpu().tolist()
    assert got[:m] == (want if with_result else [CANARY] * m) and got[m:] == [CANARY] * 8
    dst.check()
    src.check()
    return want


def hop(box, lanes=None):
    """the whole object into a fresh one (lane j to lanes[j]); the old one is freed"""
    fresh, before = box.like(box.n), box.model.status()
    want = move(fresh, box, box.n, dst_lanes=lanes)
    assert want == [V.EMPTY if s == V.STATUS_ABSENT else V.MOVED for s in before]
    assert box.side.status() == [V.STATUS_ABSENT] * box.n
    box.free()
    return fresh


def write(box, payload_of, plen):
    """one write call; {sid: message}.  payload_of(sid): the session's payload.
    A lane that is empty or failed writes nothing at all."""
    side, lanes, torch = box.side, box.model.lanes, box.torch
    rows = [payload_of(s.sid) if s is not None else bytes(plen) for s in lanes]
    mlen = plen + side.overhead
    payload, msg = Buf(torch, box.n, max(plen, 1), [p or b"\0" for p in rows]), Buf(torch, box.n, mlen)
    rc = side.write(payload, plen, msg)
    assert rc == 0, ("write", hex(rc))
    sent, out = msg.read(), {}
    for l, s in enumerate(lanes):
        want = s.write(rows[l]) if s is not None else None
        if want is None:
            assert sent[l] == bytes([CANARY]) * mlen, ("lane", l, "wrote a message")
        else:
            assert sent[l] == want, ("message of session", s.sid, "in lane", l)
            out[s.sid] = want
    box.model.advanced()
    box.check()
    return out


def read(box, msgs, mlen):
    """one read call of msgs[sid]; {sid: payload} of the sessions that verified"""
    side, lanes, torch = box.side, box.model.lanes, box.torch
    plen = mlen - side.overhead
    rows = [msgs.get(s.sid, bytes(mlen)) if s is not None else bytes([0x5A]) * mlen for s in lanes]
    msg, got = Buf(torch, box.n, mlen, rows), Buf(torch, box.n, max(plen, 1))
    rc = side.read(msg, mlen, got)
    assert rc == 0, ("read", hex(rc))
    back, out = got.read(), {}
    for l, s in enumerate(lanes):
        if s is None:
            assert back[l] == bytes([CANARY]) * max(plen, 1), ("empty lane", l, "read a payload")
            continue
        pl = s.read(rows[l])
        if pl is not None:
            assert back[l][:plen] == pl, ("payload of session", s.sid, "in lane", l)
            out[s.sid] = pl
    box.model.advanced()
    box.check()
    return out


def split(box):
    """the split, held to the models: {sid: (k1, k2, h)}; an empty lane gives zeros"""
    k1, k2, hh = FG.split(box.side)
    out = {}
    for l, s in enumerate(box.model.lanes):
        if s is None:
            assert k1[l] == k2[l] == bytes(32) and hh[l] == bytes(box.side.hl), ("split of the empty lane", l)
            continue
        want = s.split()
        assert (k1[l], k2[l]) == want[:2], ("split keys of session", s.sid)
        if not s.status:
            assert hh[l] == want[2], ("handshake hash of session", s.sid)
        out[s.sid] = (k1[l], k2[l], hh[l])
    box.check()
    return out


def rotate(n, by):
    return [(j + by) % n for j in range(n)]


def run_to_split(boxes, payload, first=0, every=True):
    """Both sides (boxes: initiator-like first, the writer of message `first`)
    to the split, each side moved into a fresh object before every message but
    the first and before the split.  payload(j, sid): message j's payload.
    Returns the boxes, the messages {sid: bytes} of each step and the splits."""
    w, r = boxes
    msgs, j = [], first
    while w.side.action != w.A.ACTION_SPLIT:
        assert w.side.action == w.A.ACTION_WRITE_MESSAGE and r.side.action == w.A.ACTION_READ_MESSAGE
        assert w.side.overhead == r.side.overhead
        plen = len(payload(j, 0))
        sent = write(w, lambda sid: payload(j, sid), plen)
        got = read(r, sent, plen + r.side.overhead)
        assert got == {sid: payload(j, sid) for sid in sent}
        msgs.append(sent)
        j += 1
        if every:
            w, r = hop(w, rotate(w.n, j)), hop(r, rotate(r.n, 2 * j + 1))
        w, r = r, w
    assert r.side.action == w.A.ACTION_SPLIT
    if (j - first) % 2:
        w, r = r, w
    return (w, r), msgs, (split(w), split(r))


def check_transport(orc, v, first, keys, cid, one_way=False, turn=None):
    """the vector's transport messages under session 0's split keys; the
    directions go on alternating (turn: who sends message `first`, 0 the
    side that sends under k1)"""
    turn = first % 2 if turn is None else turn
    k1, k2 = keys
    nonce = [0, 0]
    for t, m in enumerate(v["messages"][first:]):
        d = 0 if one_way else (turn + t) % 2
        ct = orc.encrypt(cid, (k1, k2)[d], nonce[d], bytes.fromhex(m["payload"]))
        nonce[d] += 1
        assert ct.hex() == m["ciphertext"], (v["name"], "transport", t)


def one_per_pattern():
    """a Curve25519 vector of cacophony for each of the fifteen patterns, the
    prefix, cipher and hash changing from pattern to pattern"""
    vs = [v for v in M.load_vectors("cacophony.txt.gz") if M.in_scope(v)]
    out = []
    for i, p in enumerate(M.PATTERNS):
        mine = [v for v in vs if M.parse_name(v["name"])[1]["pattern"] == p]
        out.append(mine[(5 * i + 3) % len(mine)])
    return out


BASIC = one_per_pattern()
FALLBACK = F.fallback_vectors()


@pytest.mark.parametrize("v", BASIC, ids=[v["name"] for v in BASIC])
def test_vectors_through_a_move_at_every_step(aead, gpu, oracle, v):
    """n = 3, session 0 the vector: both sides change their object, and their
    lanes, between every two messages and before the split; the messages, the
    transport messages under the split keys and the handshake hash are the
    vector's."""
    import torch
    A, n = aead, 3
    sess = make_sessions(v, n, 7)
    pairs = [model_pair(oracle, v, s) for s in sess]
    ini = Box(Side(A, torch, v, sess, True), tag([p[0] for p in pairs]))
    res = Box(Side(A, torch, v, sess, False), tag([p[1] for p in pairs]))

    def payload(j, sid):
        p0 = bytes.fromhex(v["messages"][j]["payload"])
        return p0 if sid == 0 else rand_rows(100 * j + sid, 1, len(p0))[0]
    (ini, res), msgs, (si, sr) = run_to_split((ini, res), payload)
    for j, sent in enumerate(msgs):
        assert sent[0].hex() == v["messages"][j]["ciphertext"], (v["name"], "message", j)
    assert si == sr and set(si) == set(range(n))
    f = M.parse_name(v["name"])[1]
    check_transport(oracle, v, len(msgs), si[0][:2], f["cipher"], M.one_way(f["pattern"]))
    if "handshake_hash" in v:
        assert si[0][2].hex() == v["handshake_hash"]
    assert ini.side.status() == res.side.status() == [0] * n
    ini.free()
    res.free()


@pytest.mark.parametrize("v", FALLBACK, ids=[v["name"] for v in FALLBACK])
def test_fallback_vectors_through_a_move_at_every_step(aead, gpu, oracle, v):
    """The 16 fallback vectors at n = 3: the IK message fails, both sides fall
    back, and from there both fallback objects change their object before
    every message — the first too, which under NoisePSK starts with a key set
    — and before the split."""
    import torch
    A, n = aead, 3
    name = F.original_name(v)
    sess = FG.vector_sessions(v, n, 11)
    ini, res = FG.ik_side(A, torch, name, sess, True), FG.ik_side(A, torch, name, sess, False)
    pairs = [FG.model_pair(oracle, name, s) for s in sess]
    mi, mr = [p[0] for p in pairs], [p[1] for p in pairs]
    vm = v["messages"]
    FG.exchange(ini, res, mi, mr, [bytes.fromhex(vm[0]["payload"])] + rand_rows(1, n - 1, len(vm[0]["payload"]) // 2))
    fr, mfr = FG.fall_back(oracle, res, mr, sess)
    fi, mfi = FG.fall_back(oracle, ini, mi, sess)
    fr, fi = hop(Box(fr, tag(mfr)), [2, 0, 1]), hop(Box(fi, tag(mfi)), [1, 2, 0])

    def payload(j, sid):
        p0 = bytes.fromhex(vm[j]["payload"])
        return p0 if sid == 0 else rand_rows(100 * j + sid, 1, len(p0))[0]
    (fr, fi), msgs, (sr, si) = run_to_split((fr, fi), payload, first=1)
    assert [m[0].hex() for m in msgs] == [vm[1]["ciphertext"], vm[2]["ciphertext"]]
    assert sr == si and sr[0][2].hex() == v["handshake_hash"]
    check_transport(oracle, v, 3, sr[0][:2], mfr[0].cid, turn=0)  # message 3 is the fallback's initiator's
    for x in (ini, res, fr, fi):
        x.free()


# ------------------------------------------------------------------ the pool

def responder_cohort(A, torch, orc, name, n, seed, sid0):
    """n responders after `-> e` and `<- e, ee, s, es`, and the models of their
    clients (which never touch the device)"""
    v = basic_vector(name)
    sess = make_sessions(v, n, seed)
    pairs = [model_pair(orc, v, s) for s in sess]
    clients, servers = [p[0] for p in pairs], [p[1] for p in pairs]
    for i in range(n):
        clients[i].sid = servers[i].sid = sid0 + i
    box = Box(Side(A, torch, v, sess, False), servers)
    first = {c.sid: c.write(b"hello") for c in clients}
    assert read(box, first, 5 + box.side.overhead) == {c.sid: b"hello" for c in clients}
    second = write(box, lambda sid: b"answer %4d" % sid, 11)
    for c in clients:
        assert c.read(second[c.sid]) == b"answer %4d" % c.sid
    return box, clients


@pytest.mark.parametrize("name", [XX, XX_PSK])
def test_pool(aead, gpu, oracle, name):
    """Cohorts of 67, 5 and 64 responders are parked in a pool of 160 lanes;
    their third messages arrive over three ticks of 65, 1 and 64, in an order
    shuffled across the cohorts, one of them spoilt; six never arrive and are
    dropped.  One tick goes on into a session table and echoes a frame."""
    import torch
    A = aead
    PERM = [(7 * j + 3) % 160 for j in range(160)]
    low = sorted(PERM[72:136])
    places = [PERM[:67], sorted(PERM[67:72], reverse=True), low[0::2] + low[1::2]]  # scattered, descending, interleaved
    pool, clients, sid0 = None, [], 0
    for size, lanes, seed in zip((67, 5, 64), places, (3, 4, 5)):
        box, cs = responder_cohort(A, torch, oracle, name, size, seed, sid0)
        if pool is None:
            pool = box.like(160)
            assert pool.side.remote_static() == [bytes(32)] * 160
        assert move(pool, box, size, dst_lanes=lanes) == [V.MOVED] * size
        assert box.side.status() == [5] * size and box.side.remote_static() == [bytes(32)] * size
        box.free()
        for buf in box.side.keep:  # the cohort's key memory goes with it: the pool owns its rows
            buf.dev.fill_(0x33)
        clients += cs
        sid0 += size
    assert sorted(pool.model.status()) == [0] * 136 + [5] * 24
    third = {c.sid: c.write(b"third %3d" % c.sid) for c in clients}
    order = np.random.default_rng(9).permutation(136).tolist()
    ticks, late = [order[:65], order[65:66], order[66:130]], order[130:]
    spoilt = ticks[0][40]
    third[spoilt] = third[spoilt][:-1] + bytes([third[spoilt][-1] ^ 1])
    cipher = T.AESGCM if "AESGCM" in name else T.CHACHAPOLY
    for t, sids in enumerate(ticks):
        m = len(sids)
        lanes = [pool.lane_of(sid) for sid in sids]
        cohort = pool.like(m)
        assert move(cohort, pool, m, src_lanes=lanes) == [V.MOVED] * m
        got = read(cohort, third, 9 + cohort.side.overhead)
        assert got == {sid: b"third %3d" % sid for sid in sids if sid != spoilt}
        rs = cohort.side.remote_static()
        assert [rs[j] for j, sid in enumerate(sids)] == [clients[sid].s_pub for sid in sids]
        keys = split(cohort)
        status = cohort.model.status()
        assert status == [1 if sid == spoilt else 0 for sid in sids]
        for j, sid in enumerate(sids):
            if sid == spoilt:
                assert keys[sid][:2] == (bytes(32), bytes(32))
            else:
                assert keys[sid] == clients[sid].split() and keys[sid][0] != bytes(32)
        if t == 0:
            # the chain handshake -> _set_keys -> traffic: the slots are the pool lanes, the list is the tick's
            side = cohort.side
            server = Table(A, torch, oracle, cipher, False, 4 * m, n=160)
            server.set_keys(lanes, [keys[sid][:2] for sid in sids], status,
                            ptrs=(side.k1.data_ptr(), side.k2.data_ptr(), A.dev_handshake_status(side.hs)))
            assert server.has_key() == [int(l in lanes and pool_sid(cohort, lanes, l) != spoilt) for l in range(160)]
            client = Table(A, torch, oracle, cipher, True, 4 * m, n=160)
            client.set_keys(lanes, [clients[sid].split()[:2] for sid in sids])
            wire = Wire(torch, [T.frame(bytes([sid]) * 20 + bytes(16)) for sid in sids])
            assert client.run("seal", wire, slots=lanes) == [(1, 38, 0)] * m
            echoed = server.run("echo", wire, slots=lanes)
            assert [e == (1, 38, 0) for e in echoed] == [sid != spoilt for sid in sids]
            opened = client.run("open", wire, slots=lanes)
            assert [o == (1, 38, 0) for o in opened] == [sid != spoilt for sid in sids]
            server.free()
            client.free()
        cohort.free()
    # the six that never answered
    lanes = [pool.lane_of(sid) for sid in late]
    assert sorted(pool.side.status()) == [0] * 6 + [5] * 154
    d = dev_u32(lanes + [160, 0xFFFFFFFF])
    assert A.dev_handshake_drop(pool.side.hs, lanes=d.data_ptr(), m=8, stream=pool.side.sp) == 0
    V.drop(pool.model, lanes + [160, 0xFFFFFFFF])
    assert pool.side.status() == pool.model.status() == [5] * 160
    assert pool.side.remote_static() == [bytes(32)] * 160
    pool.free()


def pool_sid(cohort, lanes, pool_lane):
    """the session that came from that pool lane: entry j of the tick sits in the cohort's lane j"""
    return cohort.model.lanes[lanes.index(pool_lane)].sid


# ------------------------------------------------------------ result bytes

@pytest.mark.parametrize("with_result", [True, False])
def test_result_bytes(aead, gpu, oracle, with_result):
    """One call with entries of all four outcomes: a lane out of range on
    either side and on both, an empty source, a destination taken by a live
    and by a failed session, and one that moves.  Every lane of both objects
    then finishes where it is."""
    import torch
    A = aead
    v = basic_vector(XX)
    sess = make_sessions(v, 6, 13)
    pairs = [model_pair(oracle, v, s) for s in sess]
    clients, servers = tag([p[0] for p in pairs]), tag([p[1] for p in pairs])
    src = Box(Side(A, torch, v, sess, False), servers)
    first = {c.sid: c.write(b"") for c in clients}
    first[1] = bytes(32)  # an all-zero e: session 1 fails with status 3
    read(src, first, 32)
    assert src.side.status() == [0, 3, 0, 0, 0, 0]
    second = write(src, lambda sid: b"", 0)
    for c in clients:
        if c.sid != 1:
            assert c.read(second[c.sid]) == b""
    dst = src.like(6)
    assert move(dst, src, 2, dst_lanes=[1, 3]) == [V.MOVED, V.MOVED]  # a live and a failed session
    assert dst.side.status() == [5, 0, 5, 3, 5, 5] and src.side.status() == [5, 5, 0, 0, 0, 0]
    far = 0xFFFFFFFF
    got = move(dst, src, 7, dst_lanes=[0, 4, 7, 2, 1, 3, far], src_lanes=[2, 9, 3, 0, 4, 5, far], with_result=with_result)
    assert got == [V.MOVED, V.RANGE, V.RANGE, V.EMPTY, V.TAKEN, V.TAKEN, V.RANGE]
    assert dst.side.status() == [0, 0, 5, 3, 5, 5] and src.side.status() == [5, 5, 5, 0, 0, 0]
    third = {c.sid: c.write(b"last") for c in clients if c.sid != 1}
    done = {}
    for box in (src, dst):
        assert read(box, third, 4 + box.side.overhead) == {s.sid: b"last" for s in box.model.lanes if s and s.sid != 1}
        done.update(split(box))
    assert sorted(done) == list(range(6))
    for c in clients:
        assert done[c.sid][:2] == ((bytes(32), bytes(32)) if c.sid == 1 else c.split()[:2])
    src.free()
    dst.free()


# ------------------------------------------------- keys per session and shared

@pytest.mark.parametrize("name,shared", [("Noise_KK_25519_ChaChaPoly_SHA256", False), ("Noise_IK_25519_AESGCM_BLAKE2b", True)])
@pytest.mark.parametrize("initiator", [True, False])
def test_keys_per_session_and_shared(aead, gpu, oracle, name, shared, initiator):
    """KK with a static key per session, IK with one server key for all at
    stride 0.  One side changes its object after the first message and before
    the split; the key rows it was made with are overwritten after the move,
    so the moved sessions finish on the rows the new object owns."""
    import torch
    A, n = aead, 5
    v = basic_vector(name)
    sess = make_sessions(v, n, 17, shared=shared)
    pairs = [model_pair(oracle, v, s) for s in sess]
    ini = Box(Side(A, torch, v, sess, True, shared), tag([p[0] for p in pairs]))
    res = Box(Side(A, torch, v, sess, False, shared), tag([p[1] for p in pairs]))
    # another object at the same position whose server key lies elsewhere
    twin = Side(A, torch, v, sess, initiator, shared)
    mine = ini if initiator else res
    near = mine.like(n)
    rc = A.dev_handshake_move(near.side.hs, twin.hs, 0)
    once_for_all = shared and not initiator
    assert rc == (A.ERROR_INVALID_PARAM if once_for_all else 0), hex(rc)
    twin.free()
    near.free()
    sent = write(ini, lambda sid: b"one %d" % sid, 5)
    assert len(read(res, sent, 5 + res.side.overhead)) == n
    old = res if not initiator else ini
    fresh = old.like(n + 2)
    assert move(fresh, old, n, dst_lanes=[6, 1, 0, 4, 2]) == [V.MOVED] * n
    for buf in old.side.keep:
        if buf.stride:  # a key held once for all stays the caller's, and stays as it is
            buf.dev.fill_(0x33)
    if initiator:
        ini = fresh
    else:
        res = fresh
    sent = write(res, lambda sid: b"two %d" % sid, 5)
    assert len(sent) == n and len(read(ini, sent, 5 + ini.side.overhead)) == n
    fresh = hop(fresh, [3, 5, 0, 1, 2, 6, 4])
    if initiator:
        ini = fresh
    else:
        res = fresh
    si, sr = split(ini), split(res)
    assert si == sr and len(si) == n and all(k[0] != bytes(32) for k in si.values())
    for x in (ini, res, old):
        x.free()


# ------------------------------------------------------------------ fallback

def test_a_cohort_out_of_a_fallback_object(aead, gpu, oracle):
    """NoisePSK: the fallback starts with a key set.  After the fallback's
    first message the server takes two sessions out of its fallback object,
    reads their last message, and keys a table of its original role with the
    split's key pointers exchanged; it opens the client's frame."""
    import torch
    A, n = aead, 5
    name = "NoisePSK_IK_25519_AESGCM_SHA512"
    sess = FG.random_sessions(n, 71, stale=lambda i: True, psk=True, prologue=b"pipes", fb_prologue=b"fallback")
    ini, res = FG.ik_side(A, torch, name, sess, True), FG.ik_side(A, torch, name, sess, False)
    pairs = [FG.model_pair(oracle, name, s) for s in sess]
    mi, mr = [p[0] for p in pairs], [p[1] for p in pairs]
    FG.exchange(ini, res, mi, mr, rand_rows(72, n, 16))
    # an object made like one that may fall back may not
    near = Box(res, tag(list(mr))).like(n)
    assert A.dev_handshake_fallback(near.side.hs, local_ephemeral=near.side.keep[1].ptr, psk=near.side.keep[2].ptr) == \
        (A.ERROR_NOT_APPLICABLE, None)
    near.free()
    fr, mfr = FG.fall_back(oracle, res, mr, sess)
    fi, mfi = FG.fall_back(oracle, ini, mi, sess)
    server, client = Box(fr, tag(mfr)), Box(fi, tag(mfi))
    sent = write(server, lambda sid: b"again %d" % sid, 7)
    assert len(read(client, sent, 7 + client.side.overhead)) == n
    last = write(client, lambda sid: b"", 0)
    want = split(client)
    cohort = server.like(2)
    assert move(cohort, server, 2, src_lanes=[3, 1]) == [V.MOVED] * 2
    assert server.side.status() == [0, 5, 0, 5, 0]
    assert len(read(cohort, last, cohort.side.overhead)) == 2
    keys = split(cohort)
    assert keys == {3: want[3], 1: want[1]}
    # the original roles: the server was the responder.  k1 of the fallback is its own sending key.
    tab = Table(A, torch, oracle, T.AESGCM, False, 8, n=8)
    tab.set_keys([6, 2], [(keys[3][1], keys[3][0]), (keys[1][1], keys[1][0])], [0, 0],
                 ptrs=(cohort.side.k2.data_ptr(), cohort.side.k1.data_ptr(), A.dev_handshake_status(cohort.side.hs)))
    peer = Table(A, torch, oracle, T.AESGCM, True, 8, n=8)
    peer.set_keys([6, 2], [(want[3][1], want[3][0]), (want[1][1], want[1][0])])
    wire = Wire(torch, [T.frame(b"from the client " + bytes([i]) * 4 + bytes(16)) for i in (3, 1)])
    assert peer.run("seal", wire, slots=[6, 2]) == [(1, 38, 0)] * 2
    assert tab.run("open", wire, slots=[6, 2]) == [(1, 38, 0)] * 2
    assert wire.streams()[0][2:22] == b"from the client " + bytes([3]) * 4
    # the three that stayed finish in the fallback object
    assert len(read(server, last, server.side.overhead)) == 3
    rest = split(server)
    assert rest == {i: want[i] for i in (0, 2, 4)}
    for x in (ini, res, server, client, cohort, tab, peer):
        x.free()


# ---------------------------------------------------------------- neutrality

def test_a_move_at_every_step_changes_no_byte(aead, gpu, oracle):
    """67 sessions driven in one object per side, and the same sessions with
    both sides changing object and lanes at every step: device against
    device, every message, split key, hash and status."""
    import torch
    A, n = aead, 67
    name = "Noise_XX_25519_AESGCM_SHA256"
    v = basic_vector(name)
    sess = make_sessions(v, n, 23)
    plain = handshake(A, torch, oracle, v, sess, seed=5)
    pairs = [model_pair(oracle, v, s) for s in sess]
    ini = Box(Side(A, torch, v, sess, True), tag([p[0] for p in pairs]))
    res = Box(Side(A, torch, v, sess, False), tag([p[1] for p in pairs]))
    rows = {}

    def payload(j, sid):
        if j not in rows:
            rows[j] = payload_rows(v, j, n, 5)
        return rows[j][sid]
    (ini, res), msgs, (si, sr) = run_to_split((ini, res), payload)
    assert len(msgs) == plain["n_handshake"] == 3
    for j, sent in enumerate(msgs):
        assert [sent[i] for i in range(n)] == plain["msgs"][j], ("message", j)
    for mine, theirs in ((si, plain["ini_split"]), (sr, plain["res_split"])):
        assert [mine[i] for i in range(n)] == [(theirs[0][i], theirs[1][i], theirs[2][i]) for i in range(n)]
    assert sorted(ini.side.status()) == sorted(plain["ini_status"]) == [0] * n
    for x in (ini, res, plain["ini"], plain["res"]):
        x.free()
