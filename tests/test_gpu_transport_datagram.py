"""Datagram transport: noise_aead_dev_transport_seal_datagrams / _open_datagrams
and the anti-replay windows (header section 11).

Every call is compared with the model of tests/transport_datagram_model.py
(proved against the reference by tests/test_transport_datagram_model_host.py):
every byte of the wire between canaries, every result, every frame status,
both nonce arrays and every word of the windows.  A status-5 frame that only an
earlier frame of the same call made a replay may hold its bytes as given or
its plaintext; the tests plant those cases and assert that the model names
exactly them before anything is compared.  The table and wire helpers are those
of tests/transport_gpu.py."""
import numpy as np
import pytest

import transport_gpu
import transport_model as T
import transport_datagram_model as D
from gpu_support import dev_u32, peek_u64, poke_u64
from transport_gpu import CIPHERS, N, PERM, Wire, keys_for, plain_streams

pytestmark = pytest.mark.gpu
IDS = ["ChaChaPoly", "AESGCM"]
TOP = 2 ** 32 - 1
TOP64 = 2 ** 64 - 1
PAYLOADS = (0, 1, 15, 16, 17, 63, 64, 65, 1400)
CANARY = 0xEE
UNKEYED = 13


class Table(transport_gpu.Table):
    """transport_gpu.Table with the datagram calls and the windows beside their model"""

    def windows(self):
        ptr, bits = self.A.dev_transport_replay(self.tr)
        assert ptr and bits == D.REPLAY_BITS
        flat = peek_u64(ptr, 17 * self.n)
        return [flat[17 * i:17 * i + 17] for i in range(self.n)]

    def want_windows(self):
        return [D.window(m).words() if m else [0] * 17 for m in self.model]

    def set_window(self, i, w):
        """through the object's own device array, and in the model"""
        ptr, _ = self.A.dev_transport_replay(self.tr)
        poke_u64(ptr + 136 * i, w.words())
        self.model[i].window = w.copy()

    def check_state(self):
        super().check_state()
        assert self.windows() == self.want_windows(), "windows"

    def datagrams(self, mode, wire, slots=None, max_frames=0):
        """One datagram call on the device and in the model; everything must
        equal the model's.  Returns the model's per-entry tuples."""
        A, torch = self.A, self.torch
        m = wire.n
        d_slots = dev_u32(slots) if slots is not None else None
        cap = max_frames or self.max_frames
        before = wire.rest()
        want = D.run_datagrams(self.model, mode, before, cap, slots)
        common = dict(slots=d_slots.data_ptr() if d_slots is not None else 0, m=m, max_frames=max_frames)
        if mode == "seal":
            def fn(tr, **kw):
                return A.dev_transport_seal_datagrams(tr, **common, **kw)
            results = wire.call(A, fn, self.tr)
        else:
            off = torch.tensor([o + p for o, p in zip(wire.offs, wire.pos)], dtype=torch.int64, device="cuda")
            ln = torch.tensor([l - p for l, p in zip(wire.lens, wire.pos)], dtype=torch.int32, device="cuda")
            res = torch.full((m + 1, 6), 0x55555555, dtype=torch.int32, device="cuda")
            fs = torch.full((cap + 16,), CANARY, dtype=torch.uint8, device="cuda")
            assert A.dev_transport_open_datagrams(self.tr, **common, wire=wire.dev.data_ptr(), off=off.data_ptr(),
                                                  length=ln.data_ptr(), result=res.data_ptr(), frame_status=fs.data_ptr(),
                                                  stream=self.sp) == 0
            torch.cuda.synchronize()
            r = res.cpu().numpy().view(np.uint32)
            assert (r[m] == 0x55555555).all(), "result rows"
            results = [(int(x[0]), int(x[1]), int(x[2]), int(x[3]), int(x[4]) | int(x[5]) << 32) for x in r[:m]]
            fs = fs.cpu().numpy()
        assert results == [w[1] for w in want], "results"
        if mode == "open":
            total = 0
            for j, w in enumerate(want):
                frames, first = w[1][0], w[1][4]
                assert not frames or first == total, ("first", j)
                assert list(fs[first:first + frames]) == w[2], ("statuses", j)
                total += frames
            assert total <= cap and (fs[total:] == CANARY).all(), "statuses past the call's total"
        got = wire.rest()
        for j, w in enumerate(want):
            image = bytearray(w[0])
            for at, (given, plain) in w[3].items():  # may hold either
                assert got[j][at:at + len(given)] in (given, plain), ("either", j, at)
                image[at:at + len(given)] = got[j][at:at + len(given)]
            assert got[j] == bytes(image), ("stream", j)
        self.check_state()
        return want


def payload_streams(seed, m):
    """seal-ready streams: entry j has 1 + j % 8 frames, payloads cycling through PAYLOADS"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(m):
        out.append(b"".join(D.seal_ready(rng.integers(0, 256, PAYLOADS[(j + 2 * k) % 9], dtype=np.uint8).tobytes())
                            for k in range(1 + j % 8)) + (b"\x00" if j % 5 == 3 else b""))
    return out


def reorder(stream, order):
    """the stream's frames in another order (what follows the last frame stays at the end)"""
    frames, consumed, _ = D.walk(stream)
    return b"".join(stream[frames[k][0] - 2:frames[k][0] + frames[k][1]] for k in order) + stream[consumed:]


def entries(m):
    """the slot list of a call of m entries: unsorted, with an unkeyed slot and two out of range"""
    if m == 1:
        return [PERM[2]]
    slots = PERM[:m]
    slots[7], slots[50] = TOP, N
    assert UNKEYED in slots
    return slots


def pair(aead, torch, oracle, cipher, max_frames, seed):
    keys = keys_for(seed)
    tabs = [Table(aead, torch, oracle, cipher, ini, max_frames, keys) for ini in (True, False)]
    for t in tabs:
        t.clear_keys([UNKEYED])
    return tabs


# ---------------------------------------------------------------- 1. seal, open, reorder, replay

@pytest.mark.parametrize("m", [1, 64, 65, 67])
@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_seal_open_reordered_and_replayed(aead, gpu, oracle, cipher, m):
    import torch
    a, b = pair(aead, torch, oracle, cipher, 400, 81)
    slots = entries(m)
    dead = [j for j, i in enumerate(slots) if i >= N or i == UNKEYED]
    assert m == 1 or len(dead) == 3
    for sender, receiver, seed in ((a, b, 82), (b, a, 83)):  # both roles seal and open
        plain = payload_streams(seed, m)
        assert m == 1 or {L - D.MIN_L for s in plain for _, L in D.walk(s)[0]} == set(PAYLOADS)
        wire = Wire(torch, plain)
        want = sender.datagrams("seal", wire, slots)
        assert [w[1][0] for j, w in enumerate(want) if j not in dead] == [1 + j % 8 for j in range(m) if j not in dead]
        sealed = wire.streams()
        for j in range(m):
            if j not in dead:
                assert [D.counter_of(sealed[j], at) for at, _ in D.walk(sealed[j])[0]] == list(range(1 + j % 8))
        # delivery: in order, reversed, shuffled in turn
        rng = np.random.default_rng(seed)
        delivered = []
        for j, s in enumerate(sealed):
            count = len(D.walk(s)[0])
            order = list(range(count)) if j % 3 == 0 or j in dead else list(range(count))[::-1] if j % 3 == 1 else list(rng.permutation(count))
            delivered.append(reorder(s, order))
        wire = Wire(torch, delivered)
        want = receiver.datagrams("open", wire, slots)
        opened = wire.streams()
        for j, w in enumerate(want):
            if j in dead:
                assert opened[j] == delivered[j] and w[1][2] != 0
                continue
            assert w[2] == [D.OK] * (1 + j % 8) and w[1][3] == 1 + j % 8 and not w[3]
            assert sorted(opened[j][at + 8:at + L - 16] for at, L in D.walk(opened[j])[0]) == \
                sorted(plain[j][at + 8:at + L - 16] for at, L in D.walk(plain[j])[0])
        assert receiver.nonces(1) == [0] * N  # the receive nonces are not in it
        # the same frames again: all replays, no byte and no window bit changes
        windows = receiver.windows()
        wire = Wire(torch, sealed)
        want = receiver.datagrams("open", wire, slots)
        for j, w in enumerate(want):
            assert j in dead or (w[2] == [D.REPLAY] * (1 + j % 8) and w[1][3] == 0 and not w[3])
        assert wire.streams() == sealed and receiver.windows() == windows
    a.free()
    b.free()


# ---------------------------------------------------------------- 2. one call, one entry each

def made(orc, cipher, key, counter, payload):
    """a datagram frame as the peer would have sealed it"""
    return D.datagram(counter, orc.encrypt(cipher, key, counter, bytes(payload)))


def flip(frame, at):
    f = bytearray(frame)
    f[at] ^= 0x04
    return bytes(f)


@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_in_call_cases(aead, gpu, oracle, cipher):
    """a duplicate inside the call; a forged tag between two good frames; a
    counter of 2^64 - 1; a jump of 2^40 followed by a frame that is now too
    old; a runt that stops the walk with the frames before it judged"""
    import torch
    keys = keys_for(91)
    b = Table(aead, torch, oracle, cipher, False, 64, keys)
    rng = np.random.default_rng(91)

    def f(i, c, size=33):
        return made(oracle, cipher, keys[i][0], c, rng.integers(0, 256, size, dtype=np.uint8).tobytes())  # the responder receives under k1
    dup = f(0, 1)
    never = D.datagram(TOP64, rng.integers(0, 256, 40, dtype=np.uint8).tobytes())
    streams = [
        f(0, 0) + dup + dup + f(0, 2, 0),
        f(1, 0, 17) + flip(f(1, 1, 64), -3) + f(1, 2, 1),
        f(2, 0) + never + f(2, 1) + D.datagram(TOP64, bytes(16)),
        f(3, 0) + f(3, 2 ** 40, 65) + f(3, 1) + f(3, 2 ** 40 + 1) + f(3, 2 ** 40 - 1022, 15) + f(3, 2 ** 40 - 1023, 16),
        f(4, 0) + f(4, 1, 1400) + T.frame(bytes(23)) + f(4, 2),
        b"",
        flip(f(6, 5), 2 + 8 + 4),  # the ciphertext forged
    ]
    wire = Wire(torch, streams)
    twin = [T.Session.of_role(oracle, cipher, False, *k) for k in keys]
    want = D.run_datagrams(twin, "open", streams, 64)
    at = [[fr[0] for fr in D.walk(s)[0]] for s in streams]
    # the model names exactly the planted in-call cases: the duplicate, and the two frames the jump left behind
    assert {(j, k) for j, w in enumerate(want) for k, x in enumerate(at[j]) if x in w[3]} == {(0, 2), (3, 2), (3, 5)}
    assert [w[2] for w in want] == [[0, 0, 5, 0], [0, 1, 0], [0, 5, 0, 5], [0, 0, 5, 0, 0, 5], [0, 0], [], [1]]
    assert want[4][1] == (2, at[4][1] + 24 + 1400, T.ERROR_INVALID_LENGTH, 2, 17) and want[3][1][3:] == (4, 11)
    got = b.datagrams("open", wire)  # entry j is slot j: no list
    assert [g[1] for g in got] == [w[1] for w in want]
    opened = wire.streams()
    assert opened[1][at[1][1] - 2:at[1][2] - 2] == streams[1][at[1][1] - 2:at[1][2] - 2]  # the forged frame, untouched
    assert opened[6] == streams[6] and opened[4][at[4][1] + 24 + 1400:] == streams[4][at[4][1] + 24 + 1400:]
    w = D.window(b.model[3])
    assert w.top == 2 ** 40 + 2 and bin(w.bits).count("1") == 3
    b.free()


# ---------------------------------------------------------------- 3. windows preset at their edges

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_preset_windows_at_the_edges(aead, gpu, oracle, cipher):
    import torch
    keys = keys_for(101)
    b = Table(aead, torch, oracle, cipher, True, 64, keys)  # the initiator receives under k2
    rng = np.random.default_rng(101)

    def f(i, c):
        body = rng.integers(0, 256, 1 + c % 70, dtype=np.uint8).tobytes()
        return made(oracle, cipher, keys[i][1], c, body) if c != TOP64 else D.datagram(c, body + bytes(16))  # no such nonce
    base = 5 * 1024  # top - 1024 is bit 0, top - 1 is bit 1023
    plans = {
        # slot: (top, seen counters, the counters delivered)
        3: (base, [base - 1024 + 64, base - 1], [base - 1025, base - 1024, base - 1024 + 63, base - 1024 + 64, base - 1, base - 2,
                                                 base - 1024 + 65, base, base - 1024, base - 1023]),
        64: (base + 63, [base + 62 - 1024, base], [base + 62 - 1024, base + 63 - 1024, base + 64 - 1024, base, base + 63 + 1023,
                                                   base + 63, base + 64, base + 62]),
        66: (TOP64, [TOP64 - 1, TOP64 - 1024], [TOP64, TOP64 - 1, TOP64 - 1024, TOP64 - 1025, TOP64 - 1023, TOP64 - 2]),
        0: (1, [0], [0, 1, 1025, 1, 2, 1026, 2]),
        9: (2000, [1999], [2000 + 1023, 1999, 2000, 3024 + 1024, 2001, 3025]),
    }
    slots = list(plans)
    for i, (top, seen, _) in plans.items():
        b.set_window(i, D.Window(top, sum(1 << (c % 1024) for c in seen)))
    b.check_state()
    streams = [b"".join(f(i, c) for c in plans[i][2]) for i in slots]
    # from the model, before the device runs: each edge is reached
    twin = [T.Session.of_role(oracle, cipher, True, *k) for k in keys]
    reached, bits, either = set(), set(), set()
    for i, (top, seen, counters) in plans.items():
        w = D.Window(top, sum(1 << (c % 1024) for c in seen))
        twin[i].window = w.copy()
        for c in counters:
            if c < w.top:
                reached.add((w.top - c, w.check(c)))
                bits.add((c % 1024, w.check(c)))
            elif c - w.top >= 1023:
                reached.add((w.top - c, w.check(c)))
            if w.check(c):
                w.accept(c)
    assert {(1025, False), (1024, True), (1024, False), (1, False), (-1023, True), (-1024, True)} <= reached
    assert {(63, True), (64, False), (64, True), (1023, False), (0, True), (0, False), (62, False)} <= bits
    want = D.run_datagrams(twin, "open", streams, 64, slots)
    planted = {(j, k) for j, w in enumerate(want) for k, fr in enumerate(D.walk(streams[j])[0]) if fr[0] in w[3]}
    # made replays inside the call: a counter the call's own advance of top left behind, or took twice
    assert planted == {(0, 8), (3, 3), (3, 6), (4, 4)}
    assert want[0][2] == [5, 0, 0, 5, 5, 0, 0, 0, 5, 0] and want[2][2] == [5, 5, 5, 5, 0, 0] and want[4][2] == [0, 5, 0, 0, 5, 0]
    wire = Wire(torch, streams)
    got = b.datagrams("open", wire, slots)
    assert [g[2] for g in got] == [w[2] for w in want]
    b.free()


# ---------------------------------------------------------------- 4. caps, unkeyed and out-of-range entries

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_caps_cut_before_inside_and_after_entries(aead, gpu, oracle, cipher):
    import torch
    keys = keys_for(111)
    a, b = pair(aead, torch, oracle, cipher, 40, 111)
    slots = [5, UNKEYED, 20, TOP, 7, N, 66, UNKEYED + 1]
    counts = [3, 0, 3, 0, 3, 0, 3, 3]
    live = [i for i in slots if i < N and i != UNKEYED]
    plain = [b"".join(D.seal_ready(bytes([j]) * (5 * j + k)) for k in range(3)) for j in range(len(slots))]
    for cap in (1, 3, 4, 6, 8, 9, 14, 15, 16, 0):  # before, inside and after entries, dead ones on both sides; the object's own
        for t in (a, b):
            t.set_keys(live, [keys[i] for i in live])  # and every window is new
        wire = Wire(torch, plain)
        want = a.datagrams("seal", wire, slots, cap)
        lim = cap or 40
        assert sum(w[1][0] for w in want) == min(lim, 15)
        assert [w[1][2] for w in want] == [0, D.ERROR_INVALID_STATE, 0, D.ERROR_INVALID_PARAM, 0, D.ERROR_INVALID_PARAM, 0, 0]
        want = b.datagrams("open", wire, slots, cap)
        assert [w[1][0] for w in want] == [w[1][3] for w in want]  # accepted: everything walked
        firsts = [sum(counts[:j]) if c else 0 for j, c in enumerate(counts)]
        assert [w[1][4] for w in want] == firsts and sum(w[1][0] for w in want) == min(lim, 15)
        assert [D.window(b.model[i]).top for i in live] == [w[1][0] for j, w in enumerate(want) if counts[j]]
    a.free()
    b.free()


# ---------------------------------------------------------------- 5. what resets a window and what leaves it alone

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_keys_reset_the_window_and_the_stream_calls_leave_it(aead, gpu, oracle, cipher):
    import torch
    keys = keys_for(121)
    a, b = (Table(aead, torch, oracle, cipher, ini, 400, keys) for ini in (True, False))
    b.set_nonces(1, {i: 7 for i in range(N)})
    plain = payload_streams(121, N)
    wire = Wire(torch, plain)
    a.datagrams("seal", wire)
    b.datagrams("open", wire)
    assert b.nonces(1) == [7] * N and [w[0] for w in b.windows()] == [1 + i % 8 for i in range(N)]
    assert a.windows() == [[0] * 17] * N  # a seal has no window
    # a stream tick on the same objects: sends go on from where the datagrams left them, the windows stay
    a.set_nonces(0, {i: 7 for i in range(N)})
    windows = b.windows()
    stream = Wire(torch, plain_streams(122, big=False))
    a.run("seal", stream)
    b.run("open", stream, list(range(N)))  # _open_frames_of
    assert b.windows() == windows and b.nonces(1) == [7 + i % 6 for i in range(N)]
    # re-keying and clearing reset the named slots' windows and no other
    fresh = keys_for(123, 2)
    b.set_keys([10, 40], fresh)
    b.clear_keys([3, 20, 99])
    now = b.windows()
    assert [now[i] for i in (10, 40, 3, 20)] == [[0] * 17] * 4
    assert all(now[i] == windows[i] for i in range(N) if i not in (10, 40, 3, 20))
    a.set_keys([10, 40], fresh)
    # the re-keyed slots take counter 0 again, the others refuse what they have seen
    wire = Wire(torch, payload_streams(124, N))
    for i in (10, 40):
        a.set_nonces(0, {i: 0})
    others = {i: 0 for i in range(N) if i not in (10, 40)}
    a.set_nonces(0, others)
    a.datagrams("seal", wire)
    want = b.datagrams("open", wire)
    for i in range(N):
        code = want[i][1][2]
        if i in (3, 20):
            assert code == D.ERROR_INVALID_STATE
        elif i in (10, 40):
            assert want[i][2] == [D.OK] * (1 + i % 8)
        else:  # counters 0 .. i % 8 once more, under the same keys: seen
            assert want[i][2] == [D.REPLAY] * (1 + i % 8)
    a.free()
    b.free()


# ---------------------------------------------------------------- 6. the seal's counter runs out

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_seal_stops_where_the_counter_runs_out(aead, gpu, oracle, cipher):
    """send + k == 2^64 - 1 stops the walk with NOISE_ERROR_INVALID_NONCE, as the stream seal; the peer takes
    2^64 - 2 and refuses a frame that claims 2^64 - 1"""
    import torch
    keys = keys_for(131, 4)
    a, b = (Table(aead, torch, oracle, cipher, ini, 16, keys, n=4) for ini in (True, False))
    a.set_nonces(0, {0: TOP64 - 2, 1: TOP64 - 1, 2: TOP64, 3: 2 ** 63})
    plain = [b"".join(D.seal_ready(bytes([k]) * (17 + k)) for k in range(3))] * 4
    wire = Wire(torch, plain)
    want = a.datagrams("seal", wire)
    two = D.walk(plain[0], 0, 2)[1]
    assert [w[1] for w in want] == [(2, two, T.ERROR_INVALID_NONCE), (1, D.walk(plain[0], 0, 1)[1], T.ERROR_INVALID_NONCE),
                                    (0, 0, T.ERROR_INVALID_NONCE), (3, len(plain[0]), 0)]
    assert a.nonces(0) == [TOP64, TOP64, TOP64, 2 ** 63 + 3]
    sealed = wire.streams()
    assert sealed[2] == plain[2] and sealed[0][two:] == plain[0][two:]  # the stopping frame and what follows: untouched
    # the peer: the unsealed frames claim counter 0, far behind a window at the top (5) or fresh and forged (1);
    # entry 2's first frame claims 2^64 - 1
    claim = bytearray(sealed[2])
    claim[2:10] = TOP64.to_bytes(8, "little")
    wire = Wire(torch, [sealed[0], sealed[1], bytes(claim), sealed[3]])
    want = b.datagrams("open", wire)
    assert [w[2] for w in want] == [[0, 0, 5], [0, 5, 5], [5, 1, 1], [0, 0, 0]]
    assert D.window(b.model[0]).top == TOP64 and D.window(b.model[3]).top == 2 ** 63 + 3
    a.free()
    b.free()


# ---------------------------------------------------------------- 7. the rules that need an object

def test_argument_rules_on_a_small_object(aead, gpu, oracle):
    """rules 3 to 6 of section 11 in order, each with everything after it wrong as well; nothing is launched"""
    import torch
    A = aead
    BAD = A.ERROR_INVALID_PARAM
    tab = Table(A, torch, oracle, T.CHACHAPOLY, True, 8, keys_for(141, 4), n=4)
    frames = [D.seal_ready(bytes(20))] * 4
    wire = Wire(torch, frames)
    slots = dev_u32([2, 0, 9, 3])
    off = torch.tensor(wire.offs, dtype=torch.int64, device="cuda")
    ln = torch.tensor(wire.lens, dtype=torch.int32, device="cuda")
    res = torch.zeros(4 * 24 + 64, dtype=torch.uint8, device="cuda")
    fs = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ok = dict(slots=slots.data_ptr(), wire=wire.dev.data_ptr(), off=off.data_ptr(), length=ln.data_ptr(),
              result=res.data_ptr(), stream=tab.sp)

    def seal(**kw):
        return A.dev_transport_seal_datagrams(tab.tr, **kw)

    def open_(frame_status=fs.data_ptr(), **kw):
        return A.dev_transport_open_datagrams(tab.tr, frame_status=frame_status, **kw)
    for call, width in ((seal, 16), (open_, 24)):
        assert call(m=5, max_frames=9, **{**ok, "wire": 0}) == BAD                         # m > n
        for k in ("wire", "off", "length", "result"):
            assert call(m=4, max_frames=9, **{**ok, k: 0}) == BAD, k                        # a NULL pointer
        assert call(m=4, max_frames=9, **ok) == BAD                                         # the cap
        for k, w in (("off", 8), ("length", 4), ("slots", 4)):
            for d in (0, w * 4 - 1, -width * 4 + 1):
                assert call(m=4, max_frames=8, **{**ok, "result": ok[k] + d}) == BAD, (k, d)
        assert call(m=0, max_frames=9, **{**ok, "result": ok["off"]}) == 0                  # m == 0 first
    assert open_(frame_status=0, m=4, **ok) == BAD
    for k, w in (("off", 8), ("length", 4), ("slots", 4), ("result", 24)):
        for d, cap, want in ((0, 0, BAD), (w * 4 - 1, 1, BAD), (w * 4, 1, 0), (-8, 0, 0), (-7, 0, BAD), (-7, 7, 0)):
            if want == 0:
                continue  # a call that passes would run: the passing side is asan/transport_datagram_check's
            assert open_(frame_status=ok[k] + d, m=4, max_frames=cap, **ok) == BAD, (k, d, cap)
    torch.cuda.synchronize()
    tab.check_state()  # nothing was launched: no send moved, no window bit, the wire as it was
    assert wire.streams() == frames and not res.any() and not fs.any()
    # without a list entry j is slot j, and a result where the list would be is fine
    assert seal(m=4, **{**ok, "slots": 0}) == 0
    torch.cuda.synchronize()
    assert tab.nonces(0) == [1, 1, 1, 1]
    tab.free()
