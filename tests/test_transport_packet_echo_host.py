"""The packet echo's host-only half without a GPU (header section 14).

The model (tests/transport_packet_echo_model.py, the composition of the two
section-13 calls) against a loop written here by hand that takes the packets
one by one, opens each and seals it at once if it was accepted;
noise-c_amd/asan/transport_packet_echo_check.cpp, a stand-alone program
(`make -C noise-c_amd transport_packet_echo_check`: g++
-fsanitize=address,undefined -fno-sanitize-recover=all) over
csrc/transport_plan.h, as a plain child process; then the argument order
through the library itself, as far as it goes without a reservation, on n == 0
objects and never-dereferenced pointers.  No launch happens."""
import transport_model as T
import transport_datagram_model as D
import transport_packet_echo_model as E
import transport_packet_gpu as G
from host_check import run_check
from transport_gpu import keys_for

TOP64 = 2 ** 64 - 1


def sessions_for(oracle, cipher, keys):
    """a responder table of G.SLOTS slots, G.UNKEYED without a key, in the state echo_batch is made for"""
    sessions = [None if i == G.UNKEYED else T.Session.of_role(oracle, cipher, False, *k) for i, k in enumerate(keys)]
    G.preset_sessions(sessions)
    return sessions


def by_hand(sessions, wire, packets):
    """The packets one by one in list order, each opened and, if accepted,
    sealed at once: (wire, statuses).  A refused packet stays as given."""
    out, statuses = bytearray(wire), []
    for off, ln, slot in packets:
        if not 0 <= slot < len(sessions) or sessions[slot] is None:
            statuses.append(6)
            continue
        if ln < 24 or ln > 65535:
            statuses.append(4)
            continue
        s, w = sessions[slot], D.window(sessions[slot])
        c = int.from_bytes(wire[off:off + 8], "little")
        if not w.check(c):
            statuses.append(5)
            continue
        rc, pt = s.orc.decrypt(s.cipher, s.recv_key, c, bytes(wire[off + 8:off + ln]))
        if rc != 0:
            statuses.append(1)
            continue
        w.accept(c)
        if s.send == TOP64:  # opened, not echoed: the received counter, the plaintext, the tag bytes as they were
            out[off + 8:off + ln - 16] = pt
            statuses.append(5)
            continue
        out[off:off + 8] = s.send.to_bytes(8, "little")
        out[off + 8:off + ln] = s.orc.encrypt(s.cipher, s.send_key, s.send, pt)
        s.send += 1
        statuses.append(0)
    return bytes(out), statuses


def state(sessions):
    return [(s.send, s.recv, D.window(s).words()) if s else None for s in sessions]


def test_model_equals_the_loop_by_hand(oracle):
    for cipher in (T.CHACHAPOLY, T.AESGCM):
        keys = keys_for(500 + cipher, G.SLOTS)
        for count, exhausted in ((1, None), (64, None), (200, None), (200, 4), (65, 0)):
            a, b = sessions_for(oracle, cipher, keys), sessions_for(oracle, cipher, keys)
            for s in (a, b):
                if exhausted is not None:
                    s[exhausted].send = TOP64 - 3
            batch = G.echo_batch(oracle, cipher, keys, count, 510 + count)
            wire, packets = bytes(batch["wire"]), batch["packets"]
            got_wire, statuses, either = E.run_echo(a, wire, packets)
            want_wire, want = by_hand(b, wire, packets)
            assert statuses == want and state(a) == state(b)
            assert got_wire == want_wire  # the model keeps a packet that may hold either as given, as the loop does
            assert all(b[i].recv == 0 for i in G.KEYED)
            if count > 1:
                assert set(statuses) == {0, 1, 4, 5, 6} and either and 8 * len(either) <= count
                # a jump of slot 2's top by more than a window inside the call, and what it left behind
                assert D.window(a[2]).top > G.FIRST[2] + 1500
            for p in either:
                assert statuses[p] == 5 and either[p][0] == wire[packets[p][0]:packets[p][0] + packets[p][1]]
            # every echoed packet reads back under the send key and the counter in front; the counters
            # of a slot run from its send on in list order with no gap
            taken = {i: [] for i in G.KEYED}
            for p, (off, ln, slot) in enumerate(packets):
                if statuses[p] == 0:
                    c = int.from_bytes(got_wire[off:off + 8], "little")
                    taken[slot].append(c)
                    assert oracle.decrypt(cipher, a[slot].send_key, c, got_wire[off + 8:off + ln]) == (0, batch["sent"][p])
                elif statuses[p] in (1, 4, 6):
                    assert got_wire[off:off + len(batch["parts"][p])] == batch["parts"][p]
            for i in G.KEYED:
                first = TOP64 - 3 if i == exhausted else G.SENDS[i]
                assert taken[i] == list(range(first, first + len(taken[i]))) and a[i].send == first + len(taken[i])
            if exhausted is not None:
                assert a[exhausted].send == TOP64 and len(taken[exhausted]) == 3
                # the packets the open accepted after the send had run out: echoed where the send has room
                roomy = E.run_echo(sessions_for(oracle, cipher, keys), wire, packets)[1]
                late = [p for p in range(count) if statuses[p] == 5 and roomy[p] == 0]
                assert [p for p in range(count) if statuses[p] != roomy[p]] == late
                assert late, "no packet met the exhausted send"
                for p in late:  # opened: the received counter, the plaintext, the tag bytes as they were
                    off, ln, _ = packets[p]
                    assert got_wire[off:off + 8] == wire[off:off + 8] and got_wire[off + ln - 16:off + ln] == wire[off + ln - 16:off + ln]
                    assert got_wire[off + 8:off + ln - 16] == batch["sent"][p]


def test_model_by_hand_on_a_short_list(oracle):
    """seven packets whose every byte and status is written out here"""
    cipher = T.CHACHAPOLY
    keys = keys_for(77, 3)
    b = [T.Session.of_role(oracle, cipher, False, *k) for k in keys]
    b[1] = None
    b[0].send = TOP64 - 1

    def made(i, c, payload):  # the responder receives under k1
        return c.to_bytes(8, "little") + oracle.encrypt(cipher, keys[i][0], c, payload)

    forged = bytearray(made(2, 4, b"forged"))
    forged[-1] ^= 1
    parts = [made(0, 5, b"first"), made(2, 3, b"other slot"), bytes(forged), made(0, 5, b"first"), made(0, 6, b"second"),
             made(1, 0, b"unkeyed"), made(0, 9, b"")]
    wire, offs = G.lay(parts)
    packets = [(offs[k], len(x), (0, 2, 2, 0, 0, 1, 0)[k]) for k, x in enumerate(parts)]
    packets[6] = (offs[6], 23, 0)
    out, statuses, either = E.run_echo(b, bytes(wire), packets)
    assert statuses == [0, 0, 1, 5, 5, 6, 4]
    assert list(either) == [3]  # the duplicate; packet 4 was opened and met the exhausted send
    # packet 0: echoed under 2^64 - 2, the responder sends under k2
    assert out[offs[0]:offs[0] + 8] == (TOP64 - 1).to_bytes(8, "little")
    assert out[offs[0] + 8:offs[0] + len(parts[0])] == oracle.encrypt(cipher, keys[0][1], TOP64 - 1, b"first")
    assert out[offs[1]:offs[1] + len(parts[1])] == bytes(8) + oracle.encrypt(cipher, keys[2][1], 0, b"other slot")
    for k in (2, 3, 5, 6):
        assert out[offs[k]:offs[k] + len(parts[k])] == parts[k]
    assert out[offs[4]:offs[4] + len(parts[4])] == parts[4][:8] + b"second" + parts[4][-16:]
    assert b[0].send == TOP64 and b[2].send == 1 and b[0].recv == b[2].recv == 0
    assert D.window(b[0]).words()[:2] == [7, 0b1100000] and D.window(b[2]).words()[:2] == [4, 0b1000]
    mask = bytearray(out)
    for k, x in enumerate(parts):
        mask[offs[k]:offs[k] + len(x)] = bytes([G.CANARY]) * len(x)
    assert set(mask) == {G.CANARY}  # nothing between the packets moved
    assert E.run_echo([], bytes(wire), packets)[1] == [6] * 7


def test_echo_rule_equals_the_definition_under_sanitizers():
    r = run_check("transport_packet_echo_check")
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "transport_packet_echo_check:" and last[2] == "checks" and last[4] == "failures"
    assert int(last[1]) > 5000 and last[3] == "0", last
    r = run_check("transport_packet_echo_check", "an argument", checked=False)
    assert r.returncode == 1 and "FAIL argument" in r.stderr
    assert r.stdout.split()[-2] == "1"


def test_echo_argument_rules_through_the_library(aead):
    """Validation before any launch (no GPU work), in the stated order, as far
    as it goes on an object that has not reserved; the rules behind a
    reservation are asan/transport_packet_echo_check's here and
    tests/test_gpu_transport_packet_echo.py's on the device."""
    A = aead
    BAD, STATE, OK = A.ERROR_INVALID_PARAM, A.ERROR_INVALID_STATE, A.ERROR_NONE
    ok = dict(packets=0x1000, wire=0x90000, status=0x3000)
    call = A.dev_transport_echo_packets
    for count in (0, 1, 2 ** 32 - 1):  # a NULL object comes first, before count == 0
        assert call(None, count=count, **ok) == BAD
        assert call(None, count=count, packets=0, wire=0, status=0) == BAD
    made = [A.dev_transport_new_unkeyed(A.CHACHAPOLY, A.ROLE_RESPONDER, 0, max_frames=0),
            A.dev_transport_new(A.AESGCM, A.ROLE_INITIATOR, 0, k1=0x10000, k2=0x20000, max_frames=0)]
    for rc, tr in made:
        assert rc == 0 and tr
        # count == 0 is fine whatever else is given, on an object that has not reserved too
        assert call(tr, count=0, **ok) == OK
        assert call(tr, count=0, packets=0, wire=0, status=0) == OK
        assert call(tr, count=0, **{**ok, "status": ok["packets"]}) == OK
        # count > 0 without a reservation, before the count, the pointers and the ranges
        assert call(tr, count=1, **ok) == STATE
        assert call(tr, count=2 ** 32 - 1, **ok) == STATE
        assert call(tr, count=1, packets=0, wire=0, status=0) == STATE
        assert call(tr, count=4, **{**ok, "status": ok["packets"] + 5}) == STATE
        # its siblings on the same object are what they were
        assert A.dev_transport_open_packets(tr, count=1, **ok) == STATE
        assert A.dev_transport_seal_packets(tr, count=0, **ok) == OK
        assert A.dev_transport_free(tr) == OK
