"""Rekey on the device: noise_aead_dev_rekey and
noise_aead_dev_transport_rekey (header section 12).

The raw keys' successors are compared with the model of
tests/transport_rekey_model.py (REKEY through the oracle's encrypt, held to the
known answers and the block formulas by tests/test_transport_rekey_host.py).
A table's contexts after a call are compared byte for byte, over the whole
context, with what noise_aead_dev_prepare builds from the model's key, and
everything a call must not touch (the other contexts, all nonces, all windows,
all state bytes) with what was there before.  Then traffic: frames sealed by a
rekeyed initiator equal the model's and open on a responder rekeyed the same
way, not on one that was not; and datagrams across a rekey, where the window
survives.  The table and wire helpers are those of tests/transport_gpu.py."""
import numpy as np
import pytest

import transport_gpu
import transport_model as T
import transport_datagram_model as D
import transport_rekey_model as R
from gpu_support import dev_bytes, dev_u32, peek_u64, poke_u64, prepared, stream, sync
from transport_gpu import CIPHERS, Wire, keys_for

pytestmark = pytest.mark.gpu
IDS = ["ChaChaPoly", "AESGCM"]
CANARY = 0xEE
K_COUNT = bytes(range(32))
FIXED = [K_COUNT, bytes(32), b"\xff" * 32]
# REKEY^3 of 00 01 .. 1f (the issue's table; tests/test_transport_rekey_host.py derives them on the CPU)
REKEY3 = {T.CHACHAPOLY: "83a272a70ec674e16167ca927f6556225f00403ccf784202ea421eec6250d359",
          T.AESGCM: "bf664a26ceb22d128912d93ac8e0cb34e835962120956ce111e1cd23000b7a08"}
REKEY1 = {T.CHACHAPOLY: ["50835543a205b22c9323f2022bc4f67d838f90e61d5ccf33c4513e01f85b5042",
                         "25ce5d37df19f3783185f2ffd5ab17fa3397c212f02d62fb1733e0b875b74c58",
                         "5bac2acd86a836c5dc98c116c1217ec31d3a63a9451319f097f3b4d6dab07787"],
          T.AESGCM: ["0201675c87335949b909793da5bb4d92fcf6d44b92a6e0792b6ae48b1881259d",
                     "f1573ed7ea59562387a25c24fabe25a3155fecd880e181089fe581c148cc6ba9",
                     "e686af6a1a45846d844a57057123da84529ec441d25c799cbaba1ffa30948e3f"]}
NMAX = 130

_reference = {}


def reference(orc, cipher):
    """(the NMAX raw keys of the primitive tests — the three fixed ones first —, their successors): computed once"""
    if cipher not in _reference:
        rng = np.random.default_rng(cipher + 1)
        keys = FIXED + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(NMAX - len(FIXED))]
        _reference[cipher] = (keys, [R.rekey(orc, cipher, k) for k in keys])
    return _reference[cipher]


# ---------------------------------------------------------------- 1. raw keys

def _canary(torch, nbytes):
    return torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_raw_keys(aead, gpu, oracle, cipher, n):
    """out of place and in place, the keys (and then the output too) at an odd
    address, a guard row behind the output and a byte in front of it"""
    import torch
    keys, want = reference(oracle, cipher)
    raw, want = b"".join(keys[:n]), b"".join(want[:n])
    src = _canary(torch, 1 + 32 * n + 32)
    src[1:1 + 32 * n] = dev_bytes(raw)
    image = src.cpu().numpy().copy()
    for out_at in (16, 1):  # an aligned output, an odd one
        out = _canary(torch, out_at + 32 * n + 32)
        rc = aead.dev_rekey(cipher, keys=src.data_ptr() + 1, n=n, out=out.data_ptr() + out_at, stream=stream())
        assert rc == 0, hex(rc)
        sync()
        got = out.cpu().numpy()
        assert got[out_at:out_at + 32 * n].tobytes() == want, ("successors", out_at, transport_gpu.differing(
            [got[out_at + 32 * i:out_at + 32 * i + 32].tobytes() for i in range(n)], [want[32 * i:32 * i + 32] for i in range(n)]))
        assert (got[:out_at] == CANARY).all() and (got[out_at + 32 * n:] == CANARY).all(), "wrote outside the output"
        assert (src.cpu().numpy() == image).all(), "the keys were written"
    # in place, at the odd address
    rc = aead.dev_rekey(cipher, keys=src.data_ptr() + 1, n=n, out=src.data_ptr() + 1, stream=stream())
    assert rc == 0, hex(rc)
    sync()
    got = src.cpu().numpy()
    assert got[1:1 + 32 * n].tobytes() == want, "in place"
    assert got[0] == CANARY and (got[1 + 32 * n:] == CANARY).all(), "wrote outside the keys"


@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_raw_keys_known_answers_and_three_calls(aead, gpu, oracle, cipher):
    """the three fixed keys against the written-out answers; then three calls
    in place, back to back on one stream with nothing between them"""
    import torch
    buf = dev_bytes(b"".join(FIXED))
    out = _canary(torch, 96 + 32)
    assert aead.dev_rekey(cipher, keys=buf.data_ptr(), n=3, out=out.data_ptr(), stream=stream()) == 0
    sync()
    got = out.cpu().numpy()
    assert [got[32 * i:32 * i + 32].tobytes().hex() for i in range(3)] == REKEY1[cipher]
    assert (got[96:] == CANARY).all()
    for _ in range(3):
        assert aead.dev_rekey(cipher, keys=buf.data_ptr(), n=3, out=buf.data_ptr(), stream=stream()) == 0
    sync()
    got = buf.cpu().numpy()
    assert got[:32].tobytes().hex() == REKEY3[cipher]
    assert [got[32 * i:32 * i + 32].tobytes() for i in range(3)] == [R.rekey_times(oracle, cipher, k, 3) for k in FIXED]
    # a refused call writes nothing
    assert aead.dev_rekey(cipher, keys=buf.data_ptr(), n=3, out=buf.data_ptr() + 32, stream=stream()) == aead.ERROR_INVALID_PARAM
    sync()
    assert (buf.cpu().numpy() == got).all()


# ---------------------------------------------------------------- 2. the table

class Table(transport_gpu.Table):
    """transport_gpu.Table with the rekey call beside its model, and the windows"""

    def windows(self):
        ptr, bits = self.A.dev_transport_replay(self.tr)
        assert ptr and bits == D.REPLAY_BITS
        return peek_u64(ptr, 17 * self.n)

    def poke_windows(self, words):
        ptr, _ = self.A.dev_transport_replay(self.tr)
        poke_u64(ptr, words)

    def snapshot(self):
        return dict(ctx=[self.ctx(0).copy(), self.ctx(1).copy()], nonces=[self.nonces(0), self.nonces(1)],
                    windows=self.windows(), state=self.has_key())

    def rekey(self, directions, slots=None, which=None, m=None, wait=True):
        """one call on the device and in the model; the (slot, direction bit) pairs the model rekeyed"""
        m = (len(slots) if slots is not None else self.n) if m is None else m
        d_slots = dev_u32(slots) if slots is not None else None
        d_which = dev_bytes(bytes(which)) if which is not None else None
        rc = self.A.dev_transport_rekey(self.tr, slots=d_slots.data_ptr() if d_slots is not None else 0, m=m,
                                        directions=directions, which=d_which.data_ptr() if d_which is not None else 0,
                                        stream=self.sp)
        assert rc == 0, ("dev_transport_rekey of %d entries" % m, hex(rc))
        if wait:
            self.torch.cuda.synchronize()
        return R.rekey_table(self.model, directions, m, slots, which)

    def check_rekeyed(self, before, done):
        """against the snapshot from before the call: the chosen contexts are
        prepare of the model's key over their whole length, every other context
        and everything else is as it was, byte for byte"""
        after = self.snapshot()
        for direction, attr in ((0, "send_key"), (1, "recv_key")):
            want = prepared(self.A, self.cipher, [getattr(s, attr) if s else None for s in self.model])
            assert want.shape == after["ctx"][direction].shape
            for i in range(self.n):
                got = after["ctx"][direction][i]
                if (i, 1 << direction) in done:
                    assert (got == want[i]).all(), ("rekeyed context", direction, i, int((got != want[i]).sum()), "bytes differ")
                    assert (got != before["ctx"][direction][i]).any(), ("context not rekeyed", direction, i)
                else:
                    assert (got == before["ctx"][direction][i]).all(), ("context touched", direction, i)
                    assert (got == want[i]).all(), ("the model's context", direction, i)
        assert after["nonces"] == before["nonces"], "nonces"
        assert after["windows"] == before["windows"], "windows"
        assert after["state"] == before["state"], "state bytes"
        self.check_state()


UNKEYED = (3, 9)
N_TABLE = 12


def table_of_12(aead, torch, oracle, cipher, initiator, keys=None):
    """12 slots, slots 3 and 9 unkeyed, every nonce distinct and non-zero, every window word non-zero"""
    keys = keys or keys_for(31, N_TABLE)
    t = Table(aead, torch, oracle, cipher, initiator, 64, keys, n=N_TABLE)
    t.clear_keys(list(UNKEYED))
    t.set_nonces(0, {i: 1000 + 3 * i for i in range(N_TABLE)})
    t.set_nonces(1, {i: 2 ** 40 + 7 * i for i in range(N_TABLE)})
    rng = np.random.default_rng(32)
    t.poke_windows([int(x) | 1 for x in rng.integers(1, 2 ** 63, 17 * N_TABLE)])
    t.check_state()
    return t, keys


# m = 9 entries, shuffled: an out-of-range slot, an unkeyed one, the bytes 0, 1, 2, 3 and 0xFF on live slots
SLOTS9 = [7, 99, 3, 0, 11, 5, 2, 10, 6]
WHICH9 = [3, 3, 3, 0, 1, 2, 3, 0xFF, 1]


@pytest.mark.parametrize("initiator", [True, False], ids=["initiator", "responder"])
@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_table_contexts(aead, gpu, oracle, cipher, initiator):
    import torch
    t, keys = table_of_12(aead, torch, oracle, cipher, initiator)
    chosen = {1: {(7, 1), (11, 1), (2, 1), (10, 1), (6, 1)}, 2: {(7, 2), (5, 2), (2, 2), (10, 2)}}
    chosen[3] = chosen[1] | chosen[2]
    cases = [
        ("list and bytes", dict(slots=SLOTS9, which=WHICH9), chosen),
        ("no list", dict(m=9, which=WHICH9), None),           # entries 0..8 are slots 0..8, slot 3 unkeyed
        ("no bytes", dict(slots=SLOTS9), None),
        ("neither", dict(m=9), None),
        ("one entry", dict(slots=[4], which=[0xFF]), {d: {(4, b) for b in (1, 2) if d & b} for d in (1, 2, 3)}),
        ("one entry, no list", dict(m=1), {d: {(0, b) for b in (1, 2) if d & b} for d in (1, 2, 3)}),
        ("one entry, unkeyed", dict(slots=[9]), {1: set(), 2: set(), 3: set()}),
        ("one entry, out of range", dict(slots=[N_TABLE], which=[3]), {1: set(), 2: set(), 3: set()}),
    ]
    for name, kw, expect in cases:
        for directions in (1, 2, 3):
            before = t.snapshot()
            done = t.rekey(directions, **kw)
            assert expect is None or set(done) == expect[directions], (name, directions, done)
            assert all(i not in UNKEYED and i < N_TABLE for i, _ in done)
            t.check_rekeyed(before, done)
    for direction in (0, 1):  # an unkeyed slot stays all-zero
        assert not t.ctx(direction)[list(UNKEYED)].any()
    # a refused call leaves the object as it was
    before = t.snapshot()
    d_slots = dev_u32(SLOTS9)
    for m, directions in ((9, 0), (9, 4), (9, 2 ** 32 - 1), (N_TABLE + 1, 3)):
        assert aead.dev_transport_rekey(t.tr, slots=d_slots.data_ptr(), m=m, directions=directions,
                                        stream=t.sp) == aead.ERROR_INVALID_PARAM
    assert aead.dev_transport_rekey(t.tr, slots=d_slots.data_ptr(), m=0, directions=0, stream=t.sp) == 0
    t.check_rekeyed(before, [])
    t.free()


@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_three_calls_back_to_back(aead, gpu, oracle, cipher):
    """REKEY^3: three calls on one stream with no synchronisation between them;
    each must read the round keys (the key) the call before it left"""
    import torch
    keys = keys_for(33, N_TABLE)
    keys[0] = (K_COUNT, K_COUNT)
    t, _ = table_of_12(aead, torch, oracle, cipher, True, keys)
    before = t.snapshot()
    done = []
    for _ in range(3):
        done = t.rekey(3, wait=False)
    torch.cuda.synchronize()
    assert len(done) == 2 * (N_TABLE - len(UNKEYED))
    assert t.model[0].send_key.hex() == t.model[0].recv_key.hex() == REKEY3[cipher]
    assert t.model[5].send_key == R.rekey_times(oracle, cipher, keys[5][0], 3)
    t.check_rekeyed(before, done)
    known = prepared(aead, cipher, [bytes.fromhex(REKEY3[cipher])])[0]
    for direction in (0, 1):
        assert (t.ctx(direction)[0] == known).all(), ("the known answer's context", direction)
    t.free()


# ---------------------------------------------------------------- 3. traffic

def frames_for(seed, n):
    """seal-ready streams: session i has 1 + i % 3 frames of unequal lengths"""
    rng = np.random.default_rng(seed)
    lens = (0, 1, 63, 64, 200, 17)
    return [b"".join(T.frame(rng.integers(0, 256, lens[(i + 2 * k) % 6], dtype=np.uint8).tobytes() + bytes(16))
                     for k in range(1 + i % 3)) for i in range(n)]


@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_traffic_across_a_rekey(aead, gpu, oracle, cipher):
    import torch
    n, picked = 8, [6, 1, 4]
    keys = keys_for(41, n)
    a = Table(aead, torch, oracle, cipher, True, 64, keys, n=n)
    b = Table(aead, torch, oracle, cipher, False, 64, keys, n=n)
    stale = Table(aead, torch, oracle, cipher, False, 64, keys, n=n)  # a responder that misses the rekey
    start = {i: 5 + 2 * i for i in range(n)}
    a.set_nonces(0, start)
    b.set_nonces(1, start)
    stale.set_nonces(1, start)
    assert set(a.rekey(R.SEND, picked)) == {(i, R.SEND) for i in picked}
    assert set(b.rekey(R.RECEIVE, picked)) == {(i, R.RECEIVE) for i in picked}
    everyone = list(range(n))
    plain = frames_for(42, n)
    counts = [1 + i % 3 for i in range(n)]
    wire = Wire(torch, plain)
    results = a.run("seal", wire, slots=everyone)  # every byte equals the rekey model's
    assert results == [(counts[i], len(plain[i]), 0) for i in range(n)]
    assert a.nonces(0) == [start[i] + counts[i] for i in range(n)]  # the nonces went on from where they were
    sealed = wire.streams()
    for i in range(n):  # and the model's bytes are the successor's for the picked slots, the old key's for the rest
        at, L = T.walk(sealed[i], 0)[0][0]
        key = R.rekey(oracle, cipher, keys[i][0]) if i in picked else keys[i][0]
        assert oracle.decrypt(cipher, key, start[i], sealed[i][at:at + L])[0] == 0, i
    wire = Wire(torch, sealed)
    results = b.run("open", wire, slots=everyone)
    assert results == [(counts[i], len(plain[i]), 0) for i in range(n)]
    opened = wire.streams()
    for i in range(n):
        assert [opened[i][at:at + L - 16] for at, L in T.walk(opened[i], 0)[0]] == \
            [plain[i][at:at + L - 16] for at, L in T.walk(plain[i], 0)[0]], i
    assert b.nonces(1) == [start[i] + counts[i] for i in range(n)]
    wire = Wire(torch, sealed)
    results = stale.run("open", wire, slots=everyone)
    assert results == [(0, 0, T.ERROR_MAC_FAILURE) if i in picked else (counts[i], len(plain[i]), 0) for i in range(n)]
    got = wire.streams()
    assert all(got[i] == sealed[i] for i in picked)
    for t in (a, b, stale):
        t.free()


# ---------------------------------------------------------------- 4. datagrams

def open_datagrams(t, streams, slots):
    """one _open_datagrams call over `streams`; (results, per-entry statuses, the streams after)"""
    torch, m = t.torch, len(streams)
    wire = Wire(torch, streams)
    off = torch.tensor(wire.offs, dtype=torch.int64, device="cuda")
    ln = torch.tensor(wire.lens, dtype=torch.int32, device="cuda")
    res = torch.full((m + 1, 6), 0x55555555, dtype=torch.int32, device="cuda")
    fs = torch.full((t.max_frames + 16,), CANARY, dtype=torch.uint8, device="cuda")
    d_slots = dev_u32(slots)
    rc = t.A.dev_transport_open_datagrams(t.tr, slots=d_slots.data_ptr(), m=m, wire=wire.dev.data_ptr(), off=off.data_ptr(),
                                          length=ln.data_ptr(), result=res.data_ptr(), frame_status=fs.data_ptr(), stream=t.sp)
    assert rc == 0, hex(rc)
    torch.cuda.synchronize()
    r, fs = res.cpu().numpy().view(np.uint32), fs.cpu().numpy()
    assert (r[m] == 0x55555555).all(), "result rows"
    results = [(int(x[0]), int(x[1]), int(x[2]), int(x[3]), int(x[4]) | int(x[5]) << 32) for x in r[:m]]
    statuses = [list(fs[x[4]:x[4] + x[0]]) for x in results]
    assert (fs[sum(x[0] for x in results):] == CANARY).all(), "statuses past the call's total"
    return results, statuses, wire.streams()


@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_datagrams_across_a_rekey(aead, gpu, oracle, cipher):
    """the receive window survives the rekey: a replay from before it is still
    a replay, the next counter opens under the new key and not under the old"""
    import torch
    n, slot = 4, 2
    keys = keys_for(51, n)
    a = Table(aead, torch, oracle, cipher, True, 32, keys, n=n)
    b = Table(aead, torch, oracle, cipher, False, 32, keys, n=n)
    old_key = keys[slot][0]  # the initiator sends under k1
    rng = np.random.default_rng(52)
    payloads = [rng.integers(0, 256, 20 + k, dtype=np.uint8).tobytes() for k in range(8)]

    def seal(count, first):
        """the initiator seals `count` datagrams of the slot; the sealed stream, held to the model"""
        wire = Wire(torch, [b"".join(D.seal_ready(payloads[first + k]) for k in range(count))])
        d_slots = dev_u32([slot])
        want = D.run_datagrams(a.model, "seal", wire.rest(), a.max_frames, [slot])

        def fn(tr, **kw):
            return aead.dev_transport_seal_datagrams(tr, slots=d_slots.data_ptr(), m=1, **kw)
        assert wire.call(aead, fn, a.tr) == [want[0][1]] and want[0][1][0] == count
        assert wire.streams()[0] == want[0][0]
        return want[0][0]

    first = seal(6, 0)
    want = D.run_datagrams(b.model, "open", [first], b.max_frames, [slot])
    results, statuses, _ = open_datagrams(b, [first], [slot])
    assert results == [want[0][1]] and statuses == [[D.OK] * 6] == [want[0][2]]
    assert D.window(b.model[slot]).top == 6
    # both peers rekey the same direction at the same counter
    assert a.rekey(R.SEND, [slot]) == [(slot, R.SEND)]
    assert b.rekey(R.RECEIVE, [slot]) == [(slot, R.RECEIVE)]
    assert a.nonces(0)[slot] == 6
    frames = D.walk(first)[0]
    at, L = frames[3]
    replay = first[at - 2:at + L]
    fresh = seal(1, 6)  # counter 6, under the new key
    assert D.counter_of(fresh, 2) == 6
    assert oracle.decrypt(cipher, R.rekey(oracle, cipher, old_key), 6, fresh[10:])[0] == 0
    late = D.datagram(7, oracle.encrypt(cipher, old_key, 7, payloads[7]))  # counter 7, under the old key
    stream_in = replay + fresh + late
    windows = b.windows()
    want = D.run_datagrams(b.model, "open", [stream_in], b.max_frames, [slot])
    results, statuses, after = open_datagrams(b, [stream_in], [slot])
    assert statuses == [[D.REPLAY, D.OK, D.FORGED]] == [want[0][2]]
    assert results == [want[0][1]] == [(3, len(stream_in), 0, 1, 0)]
    assert after[0] == want[0][0]
    assert after[0][:len(replay)] == replay and after[0][-len(late):] == late  # both untouched
    assert after[0][len(replay) + 10:len(replay) + 10 + len(payloads[6])] == payloads[6]
    got = b.windows()
    assert got[17 * slot:17 * slot + 17] == D.window(b.model[slot]).words() == [7, 0x7F] + [0] * 15
    assert got[:17 * slot] == windows[:17 * slot] and got[17 * slot + 17:] == windows[17 * slot + 17:]
    b.check_state()
    a.free()
    b.free()
