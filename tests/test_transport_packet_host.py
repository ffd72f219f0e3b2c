"""Packet transport's host-only half without a GPU (header section 13).

The model (tests/transport_packet_model.py) against the section-11 model on
the same bytes, and by hand; noise-c_amd/asan/transport_packet_check.cpp, a
stand-alone program (`make -C noise-c_amd transport_packet_check`: g++
-fsanitize=address,undefined -fno-sanitize-recover=all) over
csrc/transport_plan.h, as a plain child process, on its own cases and on cases
fed from the model; then the argument order through the library itself, as far
as it goes without a reservation, on n == 0 objects and never-dereferenced
pointers.  No launch happens."""
import numpy as np

import transport_model as T
import transport_datagram_model as D
import transport_packet_model as P
from host_check import run_check

TOP64 = 2 ** 64 - 1
PAYLOADS = (0, 1, 15, 16, 17, 63, 64, 65, 300)


def keys_for(seed, n):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
            for _ in range(n)]


def table(oracle, cipher, initiator, keys, unkeyed=()):
    return [None if i in unkeyed else T.Session.of_role(oracle, cipher, initiator, *k) for i, k in enumerate(keys)]


def laid_out(streams, gap=3):
    """the streams one after another with guard bytes between: (wire, [offset of each])"""
    wire, offs = bytearray(b"\xEE" * gap), []
    for s in streams:
        offs.append(len(wire))
        wire += s + b"\xEE" * gap
    return bytes(wire), offs


def packets_of(streams, offs, slots):
    """the frames of the streams as packets at the frame bodies, grouped by entry"""
    return [(offs[j] + at, L, slots[j]) for j, s in enumerate(streams) for at, L in D.walk(s)[0]]


def state(sessions):
    return [(s.send, s.recv, D.window(s).words()) if s else None for s in sessions]


def interleave(groups):
    """round robin over the groups: every group's own order is kept"""
    out, k = [], 0
    while any(k < len(g) for g in groups):
        out += [g[k] for g in groups if k < len(g)]
        k += 1
    return out


def test_model_equals_the_datagram_model_on_the_same_bytes(oracle):
    for cipher in (T.CHACHAPOLY, T.AESGCM):
        rng = np.random.default_rng(cipher)
        keys = keys_for(cipher, 6)
        slots = [4, 0, 5, 2, 1]  # slot 3 has no traffic, slot 2 no key
        plain = [b"".join(D.seal_ready(rng.integers(0, 256, PAYLOADS[(3 * j + k) % 9], dtype=np.uint8).tobytes())
                          for k in range(2 + j)) for j in range(5)]
        # ---- seal: one slot's send is about to run out
        a1, a2 = (table(oracle, cipher, True, keys, unkeyed=(2,)) for _ in range(2))
        for a in (a1, a2):
            a[5].send = TOP64 - 1
        wire, offs = laid_out(plain)
        want = D.run_datagrams(a1, "seal", plain, 100, slots)
        sealed_wire, _ = laid_out([w[0] for w in want])
        packets = packets_of(plain, offs, slots)
        got_wire, statuses, either = P.run_packets(a2, "seal", wire, packets)
        assert got_wire == sealed_wire and not either and state(a1) == state(a2)
        sealed_frames = [w[1][0] for w in want]
        assert sealed_frames == [2, 3, 1, 0, 6] and a2[5].send == TOP64
        expect = []
        for j, s in enumerate(plain):
            count = len(D.walk(s)[0])
            expect += [P.NO_SESSION] * count if slots[j] == 2 else [P.OK] * sealed_frames[j] + [P.REPLAY] * (count - sealed_frames[j])
        assert statuses == expect
        # ---- open: reordered, duplicated and forged per entry
        sealed = [w[0] for w in want]
        delivered = []
        for j, s in enumerate(sealed):
            frames = D.walk(s)[0]
            parts = [bytearray(s[at - 2:at + L]) for at, L in frames]
            if j == 0:
                parts = parts[::-1]
            if j == 1:
                parts = [parts[2], parts[0], parts[0], parts[1]]  # a duplicate inside the call
            if j == 4:
                parts[1][12] ^= 0x20  # forged, between two good ones
                parts = parts[:3] + [parts[0]] + parts[3:]
            delivered.append(b"".join(bytes(x) for x in parts))
        b1, b2, b3 = (table(oracle, cipher, False, keys, unkeyed=(2,)) for _ in range(3))
        wire, offs = laid_out(delivered)
        want = D.run_datagrams(b1, "open", delivered, 100, slots)
        opened_wire, _ = laid_out([w[0] for w in want])
        packets = packets_of(delivered, offs, slots)
        got_wire, statuses, either = P.run_packets(b2, "open", wire, packets)
        assert got_wire == opened_wire and state(b1) == state(b2)
        per_entry = [[P.NO_SESSION] * len(D.walk(delivered[j])[0]) if slots[j] == 2 else w[2] for j, w in enumerate(want)]
        assert statuses == [x for e in per_entry for x in e]
        assert per_entry[1] == [0, 0, 5, 0] and per_entry[4][:4] == [0, 1, 0, 5] and P.FORGED in statuses
        # the status-5 frames that may hold either are the same frames, with the same two forms
        mine = {packets[p][0]: forms for p, forms in either.items()}
        theirs = {offs[j] + at: forms for j, w in enumerate(want) for at, forms in w[3].items()}
        assert mine == theirs and len(mine) == 2
        # ---- the same packets interleaved, each slot's own order kept: every slot sees what it saw
        groups, p = [], 0
        for j, s in enumerate(delivered):
            count = len(D.walk(s)[0])
            groups.append(list(range(p, p + count)))
            p += count
        mixed = interleave(groups)
        assert mixed != sorted(mixed) and sorted(mixed) == list(range(len(packets)))
        got_wire3, statuses3, either3 = P.run_packets(b3, "open", wire, [packets[p] for p in mixed])
        assert [statuses3[mixed.index(p)] for p in range(len(packets))] == statuses
        assert got_wire3 == got_wire and state(b3) == state(b2)
        assert {mixed[q] for q in either3} == set(either)


def test_model_by_hand(oracle):
    cipher = T.CHACHAPOLY
    keys = keys_for(7, 3)
    b = table(oracle, cipher, False, keys, unkeyed=(1,))
    rng = np.random.default_rng(7)

    def made(i, c, size=20):  # the responder receives under k1
        return c.to_bytes(8, "little") + oracle.encrypt(cipher, keys[i][0], c, rng.integers(0, 256, size, dtype=np.uint8).tobytes())

    def run(mode, sessions, parts):
        """parts: [(slot, bytes)] or [(slot, bytes, len)]"""
        wire, offs = laid_out([x[1] for x in parts], gap=5)
        packets = [(offs[k], x[2] if len(x) > 2 else len(x[1]), x[0]) for k, x in enumerate(parts)]
        return (wire, packets) + P.run_packets(sessions, mode, wire, packets)

    # an in-call duplicate (at another offset): 5, and it may hold either
    dup = made(0, 4)
    wire, packets, out, statuses, either = run("open", b, [(0, made(0, 3)), (0, dup), (2, made(2, 0)), (0, dup)])
    assert statuses == [0, 0, 0, 5] and list(either) == [3] and either[3][0] == dup and either[3][1] != dup
    assert either[3][1][:8] == dup[:8] and either[3][1][-16:] == dup[-16:]
    assert D.window(b[0]).top == 5 and D.window(b[2]).top == 1
    # a jump leaves a counter behind: fresh before the call, too old after the jump
    late = made(0, 6)
    wire, packets, out, statuses, either = run("open", b, [(0, made(0, 5 + 1024 + 2)), (0, late), (0, made(0, 8))])  # 8 is the window's oldest by then
    assert statuses == [0, 5, 0] and list(either) == [1] and D.window(b[0]).top == 5 + 1024 + 3
    assert out[packets[1][0]:packets[1][0] + packets[1][1]] == late  # the model keeps it as given
    # a forged packet between two good ones moves nothing and is untouched
    forged = bytearray(made(2, 2))
    forged[9] ^= 1
    before = D.window(b[2]).words()
    wire, packets, out, statuses, either = run("open", b, [(2, made(2, 1)), (2, bytes(forged)), (2, made(2, 3))])
    assert statuses == [0, 1, 0] and not either
    assert out[packets[1][0]:packets[1][0] + packets[1][1]] == bytes(forged)
    assert D.window(b[2]).top == 4 and D.window(b[2]).bits == 0b1011 and before == [1, 1] + [0] * 15
    # a replay of what an earlier call accepted: refused as the window stood, not in either, untouched
    again = made(2, 3)
    wire, packets, out, statuses, either = run("open", b, [(2, again), (2, TOP64.to_bytes(8, "little") + bytes(36))])
    assert statuses == [5, 5] and not either and out == wire
    assert b[0].recv == b[2].recv == 0  # the receive nonces are not in it
    # statuses 6 and 4 take no counter: the slot's next packet gets the next one
    a = table(oracle, cipher, True, keys, unkeyed=(1,))
    a[0].send = 10
    room = bytes(8) + b"payload" + bytes(16)
    parts = [(0, room), (1, room), (0, room, 23), (3, room), (0, room, 65536), (2 ** 32 - 1, room), (0, room), (2, room), (0, room)]
    wire, packets, out, statuses, either = run("seal", a, parts)
    assert statuses == [0, 6, 4, 6, 4, 6, 0, 0, 0] and not either
    counters = [int.from_bytes(out[off:off + 8], "little") for off, _, _ in packets]
    assert counters == [10, 0, 0, 0, 0, 0, 11, 0, 12] and a[0].send == 13 and a[2].send == 1
    for k, (off, ln, _) in enumerate(packets):
        if statuses[k]:
            assert out[off:off + len(room)] == room
    assert oracle.decrypt(cipher, keys[0][0], 12, out[packets[8][0] + 8:packets[8][0] + len(room)]) == (0, b"payload")
    # the same on an open: the refused ones meet no window
    wire, packets, out, statuses, either = run("open", b, [(1, made(0, 50)), (0, made(0, 2000), 23), (0, made(0, 2001)), (9, made(0, 2002))])
    assert statuses == [6, 4, 0, 6] and D.window(b[0]).top == 2002
    # seal exhaustion from send = 2^64 - 3: two are sealed, the rest get 5, the other slot goes on
    a[0].send = TOP64 - 2
    wire, packets, out, statuses, either = run("seal", a, [(0, room), (2, room), (0, room), (0, room), (2, room), (0, room)])
    assert statuses == [0, 0, 0, 5, 0, 5] and a[0].send == TOP64 and a[2].send == 3
    assert [int.from_bytes(out[off:off + 8], "little") for off, _, _ in packets] == [TOP64 - 2, 1, TOP64 - 1, 0, 2, 0]
    assert out[packets[3][0]:packets[3][0] + len(room)] == room
    wire, packets, out, statuses, either = run("seal", a, [(0, room)])
    assert statuses == [5] and out == wire and a[0].send == TOP64
    # n == 0: every packet has no session
    assert P.run_packets([], "open", wire, packets * 3)[1] == [6, 6, 6]


class Marked:
    """an AEAD for the feed: a record verifies unless its last byte says otherwise"""

    def encrypt(self, cipher, key, nonce, pt):
        return bytes(pt) + bytes(16)

    def decrypt(self, cipher, key, nonce, ct):
        return (1, b"") if ct[-1] else (0, bytes(ct[:-16]))


def feed_case(mode, n, keyed, windows, sends, packets):
    """One case of the program's feed with the model's statuses and state as
    its expectations.  windows: {slot: (top, [seen])}; sends: {slot: value};
    packets: [(slot, len, counter, forged)]."""
    sessions = [T.Session(Marked(), 0, b"", b"") if i in keyed else None for i in range(n)]
    lines = ["%s %d" % (mode, n), "keyed " + " ".join(str(i) for i in sorted(keyed))]
    for i, (top, seen) in windows.items():
        sessions[i].window = D.Window(top, sum(1 << (c % 1024) for c in seen))
        lines.append("window %d %d %s" % (i, top, " ".join(str(c) for c in seen)))
    for i, v in sends.items():
        sessions[i].send = v
        lines.append("send %d %d" % (i, v))
    wire, listed = bytearray(), []
    for slot, ln, counter, forged in packets:
        size = ln if 24 <= ln <= 65535 else 24
        listed.append((len(wire), ln, slot))
        wire += counter.to_bytes(8, "little") + bytes(size - 9) + bytes([forged])
    _, statuses, _ = P.run_packets(sessions, mode, bytes(wire), listed)
    for (slot, ln, counter, forged), st in zip(packets, statuses):
        lines.append("packet %d %d %d %d %d" % (slot, ln, counter, forged, st))
    for i, s in enumerate(sessions):
        if s:
            lines.append("after %d %d" % (i, D.window(s).top if mode == "open" else s.send))
    return "\n".join(lines + ["run"]) + "\n", statuses


def fed_cases():
    rng = np.random.default_rng(13)
    base = 5 * 1024
    cases = []
    # around a preset window's lower edge, duplicates, a jump, the ends, sentinels, three slots interleaved
    packets = []
    for c in (base - 1025, base - 1024, base - 1023, base - 1, base, base, base + 1, base - 1023, base + 1024 + 5, base + 2, base + 6,
              0, TOP64 - 1, TOP64, TOP64 - 1):
        packets += [(3, 24 + c % 50, c, 0), (0, 40, c, int(c % 3 == 0)), (4, 40, c, 0)]
    packets[5:5] = [(1, 40, 7, 0), (5, 40, 7, 0), (3, 23, 7, 0), (3, 65536, 7, 0), (2 ** 32 - 1, 0, 7, 0)]
    cases.append(feed_case("open", 5, {0, 3, 4}, {3: (base, [base - 1, base - 1024]), 4: (TOP64, [TOP64 - 1])}, {}, packets))
    # a random list over 67 slots
    packets = [(int(rng.integers(0, 70)), int(rng.choice([24, 25, 1424, 23, 65535])), int(rng.integers(0, 40)), int(rng.integers(0, 6) == 0))
               for _ in range(600)]
    cases.append(feed_case("open", 67, set(range(67)) - {13, 40}, {}, {}, packets))
    # seal ranks with exhaustion
    packets = [((0, 2, 0, 1, 0, 9, 2)[k % 7], (24, 100, 23, 24)[k % 4], 0, 0) for k in range(40)]
    cases.append(feed_case("seal", 4, {0, 2, 3}, {}, {0: TOP64 - 3, 2: 77}, packets))
    cases.append(feed_case("open", 0, set(), {}, {}, [(0, 40, 1, 0), (7, 40, 2, 0)]))
    return cases


def test_pipeline_equals_one_by_one_under_sanitizers():
    r = run_check("transport_packet_check", feed="")
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "transport_packet_check:" and last[2] == "checks" and last[4] == "failures"
    own = int(last[1])
    assert own > 900 and last[3] == "0", last
    # cases of ours with the model's statuses, window tops and sends: the program agrees
    cases = fed_cases()
    seen = {s for _, statuses in cases for s in statuses}
    assert seen == {0, 1, 4, 5, 6}
    assert cases[2][1].count(5) > 3 and cases[3][1] == [6, 6]
    feed = "".join(text for text, _ in cases)
    r = run_check("transport_packet_check", feed=feed)
    last = r.stdout.splitlines()[-1].split()
    assert int(last[1]) > own + sum(len(s) for _, s in cases) and last[3] == "0", last
    # and wrong ones: the program does compare
    text, statuses = cases[0]
    lines = text.splitlines()
    for flip in ({0: 5, 5: 0, 1: 0, 4: 0, 6: 4}, None):
        bad = list(lines)
        if flip:
            k = next(k for k, ln in enumerate(bad) if ln.startswith("packet ") and int(ln.split()[-1]) == 5)
            f = bad[k].split()
            bad[k] = " ".join(f[:-1] + [str(flip[int(f[-1])])])
        else:
            k = next(k for k, ln in enumerate(bad) if ln.startswith("after "))
            f = bad[k].split()
            bad[k] = " ".join(f[:-1] + [str(int(f[-1]) ^ 1)])
        r = run_check("transport_packet_check", feed="\n".join(bad) + "\n", checked=False)
        assert r.returncode == 1 and "FAIL expect" in r.stderr, r.stdout + r.stderr
        assert r.stdout.split()[-2] == "1"
    r = run_check("transport_packet_check", feed="open 3\nsomething else\n", checked=False)
    assert r.returncode == 1 and "FAIL feed" in r.stderr
    r = run_check("transport_packet_check", "an argument", feed="", checked=False)
    assert r.returncode == 1 and "FAIL argument" in r.stderr


def test_packet_argument_rules_through_the_library(aead):
    """Validation before any launch (no GPU work), in the stated order, as far
    as it goes on an object that has not reserved; the rules behind a
    reservation are asan/transport_packet_check's here and
    tests/test_gpu_transport_packet.py's on the device."""
    A = aead
    BAD, STATE, OK = A.ERROR_INVALID_PARAM, A.ERROR_INVALID_STATE, A.ERROR_NONE
    ok = dict(packets=0x1000, wire=0x90000, status=0x3000)
    calls = (A.dev_transport_seal_packets, A.dev_transport_open_packets)
    # a NULL object comes first, before count == 0
    for call in calls:
        for count in (0, 1):
            assert call(None, count=count, **ok) == BAD
    for max_packets in (0, 1, 2 ** 31, 2 ** 32 - 1):
        assert A.dev_transport_reserve_packets(None, max_packets) == BAD
    made = [A.dev_transport_new_unkeyed(A.CHACHAPOLY, A.ROLE_INITIATOR, 0, max_frames=0),
            A.dev_transport_new(A.AESGCM, A.ROLE_RESPONDER, 0, k1=0x10000, k2=0x20000, max_frames=0)]
    for rc, tr in made:
        assert rc == 0 and tr
        for max_packets in (0, 2 ** 31 + 1, 2 ** 32 - 1):
            assert A.dev_transport_reserve_packets(tr, max_packets) == BAD
        for call in calls:
            # count == 0 is fine whatever else is given, on an object that has not reserved too
            assert call(tr, count=0, **ok) == OK
            assert call(tr, count=0, packets=0, wire=0, status=0) == OK
            assert call(tr, count=0, **{**ok, "status": ok["packets"]}) == OK
            # count > 0 without a reservation, before the count, the pointers and the ranges
            assert call(tr, count=1, **ok) == STATE
            assert call(tr, count=2 ** 32 - 1, **ok) == STATE
            assert call(tr, count=1, packets=0, wire=0, status=0) == STATE
            assert call(tr, count=4, **{**ok, "status": ok["packets"] + 5}) == STATE
        # the calls of sections 9 to 11 on it are what they were
        assert A.dev_transport_seal_frames(tr, wire=0x90000, off=0x1000, length=0x2000, result=0x3000) == OK
        assert A.dev_transport_open_datagrams(tr, m=0, wire=0, off=0, length=0, result=0, frame_status=0) == OK
        assert A.dev_transport_free(tr) == OK


def test_packet_mirrors_have_the_layout_of_the_header(aead):
    import ctypes as C
    mirror, dt = np.dtype(aead.NoiseAeadPacket), np.dtype(aead.PACKET_DT)
    assert C.sizeof(aead.NoiseAeadPacket) == 16 == dt.itemsize
    assert dt.names == mirror.names == ("off", "len", "slot")
    assert [dt.fields[f][1] for f in dt.names] == [mirror.fields[f][1] for f in dt.names] == [0, 8, 12]
