"""The datagram model (tests/transport_datagram_model.py) against the reference
and against a set of seen counters.

Where the reference library is available (the `reflib` fixture), a session with
rising counters: each sealed frame equals noise_cipherstate_set_nonce(c) +
encrypt of the reference, each accepted frame's plaintext set_nonce(c) +
decrypt, for both ciphers; and the documented difference: for a counter behind
its state the reference answers NOISE_ERROR_INVALID_NONCE where the model says
"late but fresh".  Without it: the window's sequential statuses equal a
brute-force set-of-seen-counters model on random counter sequences around
every edge of the rule."""
import ctypes as C

import numpy as np
import pytest

import transport_model as T
import transport_datagram_model as D

PAYLOADS = (0, 1, 15, 16, 17, 63, 64, 65, 1400)
TOP64 = 2 ** 64 - 1


class RefState:
    """one reference CipherState under one key, moved by set_nonce"""

    def __init__(self, reflib, cipher, key):
        from oracle import NoiseBuffer
        self.L, self.NB = reflib.L, NoiseBuffer
        self.st = reflib._state(cipher, key, 0)

    def set_nonce(self, c):
        return self.L.noise_cipherstate_set_nonce(self.st, c)

    def encrypt(self, pt):
        buf = (C.c_uint8 * (len(pt) + 16)).from_buffer_copy(bytes(pt) + bytes(16))
        nb = self.NB(C.addressof(buf), len(pt), len(pt) + 16)
        rc = self.L.noise_cipherstate_encrypt_with_ad(self.st, None, 0, C.byref(nb))
        return rc, bytes(buf)[:nb.size]

    def decrypt(self, ct):
        buf = (C.c_uint8 * len(ct)).from_buffer_copy(bytes(ct))
        nb = self.NB(C.addressof(buf), len(ct), len(ct))
        rc = self.L.noise_cipherstate_decrypt_with_ad(self.st, None, 0, C.byref(nb))
        return rc, bytes(buf)[:nb.size]

    def free(self):
        self.L.noise_cipherstate_free(self.st)


@pytest.mark.parametrize("cipher", [T.CHACHAPOLY, T.AESGCM])
def test_model_equals_the_reference_under_set_nonce(oracle, reflib, cipher):
    rng = np.random.default_rng(cipher + 1)
    k1, k2 = rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    pts = [rng.integers(0, 256, p, dtype=np.uint8).tobytes() for p in PAYLOADS]
    ini = T.Session.of_role(oracle, cipher, True, k1, k2)
    res = T.Session.of_role(oracle, cipher, False, k1, k2)
    start = 2 ** 40 - 3
    ini.send = start
    plain = b"".join(D.seal_ready(pt) for pt in pts)
    (sealed, result, _, _), = D.run_datagrams([ini], "seal", [plain], 100)
    assert result == (len(pts), len(plain), 0) and ini.send == start + len(pts)
    frames = D.walk(sealed)[0]
    assert [L - D.MIN_L for _, L in frames] == list(PAYLOADS)
    # each sealed frame: its counter on the wire, then the reference's set_nonce + encrypt
    ref = RefState(reflib, cipher, k1)
    for k, ((at, L), pt) in enumerate(zip(frames, pts)):
        assert D.counter_of(sealed, at) == start + k
        assert ref.set_nonce(start + k) == 0
        rc, ct = ref.encrypt(pt)
        assert rc == 0 and sealed[at + 8:at + L] == ct
    ref.free()

    # the peer opens them with rising counters: each accepted frame is the reference's set_nonce + decrypt
    (opened, result, statuses, either), = D.run_datagrams([res], "open", [sealed], 100)
    assert result == (len(pts), len(sealed), 0, len(pts), 0) and statuses == [0] * len(pts) and not either
    assert res.recv == 0 and D.window(res).top == start + len(pts)
    ref = RefState(reflib, cipher, k1)
    for k, ((at, L), pt) in enumerate(zip(frames, pts)):
        assert ref.set_nonce(start + k) == 0
        rc, got = ref.decrypt(sealed[at + 8:at + L])
        assert rc == 0 and got == pt == opened[at + 8:at + L - 16]
        assert opened[at + L - 16:at + L] == sealed[at + L - 16:at + L] and opened[at:at + 8] == sealed[at:at + 8]
    # the documented difference: a counter behind the state.  The reference's set_nonce refuses to go backwards
    # (cipherstate.c:518-535); the model takes the frame once, late but fresh, and never again
    late = T.Session.of_role(oracle, cipher, False, k1, k2)
    order = [3, 0, 1, 0, 3]
    shuffled = b"".join(sealed[frames[k][0] - 2:frames[k][0] + frames[k][1]] for k in order)
    (_, result, statuses, either), = D.run_datagrams([late], "open", [shuffled], 100)
    assert statuses == [0, 0, 0, D.REPLAY, D.REPLAY] and result[3] == 3
    assert len(either) == 2  # in-call duplicates: each verified when it was opened
    assert ref.set_nonce(start + 0) == T.ERROR_INVALID_NONCE
    ref2 = RefState(reflib, cipher, k1)
    assert ref2.set_nonce(start + 3) == 0 and ref2.decrypt(sealed[frames[3][0] + 8:sum(frames[3])])[0] == 0
    assert ref2.set_nonce(start + 0) == T.ERROR_INVALID_NONCE  # where the model says status 0
    ref.free()
    ref2.free()


def _brute(counters):
    """statuses by a set of the counters accepted so far"""
    seen, out = set(), []
    for c in counters:
        top = max(seen) + 1 if seen else 0
        fresh = c != TOP64 and c not in seen and (c >= top or top - c <= 1024)
        out.append(fresh)
        if fresh:
            seen.add(c)
    return out, seen


def _window(counters, w=None):
    w = w or D.Window()
    out = []
    for c in counters:
        before = (w.top, w.bits)
        fresh = w.check(c)
        assert (w.top, w.bits) == before  # check reads only
        out.append(fresh)
        if fresh:
            w.accept(c)
    return out, w


EDGES = (-1025, -1024, -1023, -1, 0, 1, 1023, 1024, 1025, 2 ** 40)


def test_window_equals_a_set_of_seen_counters_around_every_edge():
    rng = np.random.default_rng(5)
    tops = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048 + 63, 2048 + 64, 2047, 5000, 2 ** 40, TOP64 - 1025, TOP64 - 1, TOP64]
    reached = set()
    for top in tops:
        for trial in range(12):
            seq = [top - 1] if top else []
            picks = [EDGES[int(x)] for x in rng.integers(0, len(EDGES), 6)]
            picks += [int(x) for x in rng.integers(-1100, 40, 6)]
            for d in picks:
                base = max(seq) + 1 if seq and trial % 2 else top  # around where top is by now, or where it started
                c = base + d
                if 0 <= c <= TOP64:
                    seq += [c, c] if trial % 3 == 0 else [c]
                    reached.add(d)
            seq += [0, TOP64 - 1, TOP64, 0, TOP64 - 1] if trial == 11 else []
            want, seen = _brute(seq)
            got, w = _window(seq)
            assert got == want, (top, seq)
            assert w.top == (max(seen) + 1 if seen else 0)
            for x in range(max(0, w.top - 1024), w.top):  # every bit of the window
                assert ((w.bits >> (x % 1024)) & 1) == (x in seen), (top, seq, x)
            assert D.Window.of_words(w.words()).__dict__ == w.__dict__ and len(w.words()) == 17
    assert reached >= set(EDGES)
    # the bit positions 63, 64 and 1023: a lap apart they are the same bit, and never confused
    for pos in (63, 64, 1023):
        for lap in (0, 1024, 77 * 1024):
            c = lap + pos
            seq = [c, c, c + 1023, c, c + 1024, c, c + 1, c + 2, c + 1024]
            assert _window(seq)[0] == _brute(seq)[0] == [True, False, True, False, True, False, True, True, False]
    # 2^64 - 1 is never fresh, 2^64 - 2 and 0 are, once
    assert _window([TOP64, 0, 0, TOP64 - 1, TOP64 - 1, TOP64, 0])[0] == [False, True, False, True, False, False, False]


def test_walk_is_the_stream_walk_with_24(oracle):
    for L in range(0, 40):
        s = T.frame(bytes(L))
        assert D.walk(s) == (([(2, L)], 2 + L, 0) if L >= 24 else ([], 0, T.ERROR_INVALID_LENGTH))
        assert T.walk(s, 0) == (([(2, L)], 2 + L, 0) if L >= 16 else ([], 0, T.ERROR_INVALID_LENGTH))
    s = b"".join(D.seal_ready(bytes(p)) for p in (0, 5, 9))
    assert D.walk(s) == T.walk(s, 0) and D.walk(s, 0, 2) == T.walk(s, 0, 2) and D.walk(s[:-1]) == T.walk(s[:-1], 0)
    assert D.walk(s, TOP64 - 2) == T.walk(s, TOP64 - 2) and D.walk(s, TOP64 - 2)[2] == T.ERROR_INVALID_NONCE


def test_model_call_over_entries(oracle):
    """unkeyed and out-of-range entries, the cap, first and accepted, a forged frame and a runt"""
    rng = np.random.default_rng(8)
    keys = [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
            for _ in range(4)]
    a = [T.Session.of_role(oracle, T.CHACHAPOLY, True, *k) for k in keys]
    b = [T.Session.of_role(oracle, T.CHACHAPOLY, False, *k) for k in keys]
    a[2] = b[2] = None
    plain = [b"".join(D.seal_ready(bytes([j]) * (3 + k)) for k in range(3)) for j in range(5)]
    slots = [3, 2, 0, 9, 1]
    sealed = D.run_datagrams(a, "seal", plain, 100, slots)
    assert [r[1] for r in sealed] == [(3, len(plain[0]), 0), (0, 0, D.ERROR_INVALID_STATE), (3, len(plain[2]), 0),
                                      (0, 0, D.ERROR_INVALID_PARAM), (3, len(plain[4]), 0)]
    assert sealed[1][0] == plain[1] and sealed[3][0] == plain[3] and [s.send for s in a if s] == [3, 3, 3]
    wire = [bytearray(r[0]) for r in sealed]
    frames = D.walk(bytes(wire[2]))[0]
    wire[2][frames[1][0] + 9] ^= 1  # forged, between two good frames
    wire[4] += T.frame(bytes(23)) + bytes(wire[4][:40])  # a runt stops the walk
    out = D.run_datagrams(b, "open", wire, 8, slots)
    assert [r[1] for r in out] == [(3, len(plain[0]), 0, 3, 0), (0, 0, D.ERROR_INVALID_STATE, 0, 0), (3, len(plain[2]), 0, 2, 3),
                                   (0, 0, D.ERROR_INVALID_PARAM, 0, 0), (2, T.walk(plain[4], 0, 2)[1], 0, 2, 6)]
    assert out[2][2] == [0, 1, 0] and out[2][0][:frames[1][0] + frames[1][1]][frames[1][0] - 2:] == bytes(wire[2])[frames[1][0] - 2:frames[1][0] + frames[1][1]]
    assert [s.recv for s in b if s] == [0, 0, 0] and D.window(b[0]).top == 3 and D.window(b[1]).top == 2
    # the rest of entry 4 in a second call: its third frame, then the runt
    rest = bytes(wire[4])[out[4][1][1]:]
    (after, result, statuses, _), = D.run_datagrams(b, "open", [rest], 8, [1])
    assert result == (1, len(plain[4]) - out[4][1][1], T.ERROR_INVALID_LENGTH, 1, 0) and statuses == [0]
    assert D.window(b[1]).words()[:2] == [3, 7]
