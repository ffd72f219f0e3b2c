"""Packet transport: noise_aead_dev_transport_reserve_packets / _seal_packets /
_open_packets (header section 13).

Every call is compared with the sequential model of
tests/transport_packet_model.py (held to the section-11 model by
tests/test_transport_packet_host.py): every byte of the wire with the guard
bytes between the packets, every status, both nonce arrays and every word of
the windows.  A status-5 packet that only an earlier packet of the same call
made a replay may hold its bytes as given or its plaintext; the tests plant
those and assert that the model names them before anything is compared.  The
table helpers are those of tests/transport_gpu.py."""
import numpy as np
import pytest

import noise_aead
import transport_gpu
import transport_model as T
import transport_datagram_model as D
import transport_packet_model as P
import transport_rekey_model as R
from gpu_support import dev, dev_u32, peek_u64, poke_u64
from transport_gpu import CIPHERS, N, PERM, Wire, differing, keys_for, plain_streams

pytestmark = pytest.mark.gpu
IDS = ["ChaChaPoly", "AESGCM"]
TOP64 = 2 ** 64 - 1
PAYLOADS = (0, 1, 15, 16, 17, 63, 64, 65, 300)
CANARY = 0xEE
UNTOUCHED = 0x77
UNKEYED = (13, 40)
BUSY = (0, 5, 13, 29, 30, 64, 66, 40)  # the slots of the scrambled traffic, two of them unkeyed


class Table(transport_gpu.Table):
    """transport_gpu.Table with the packet calls and the windows beside their model"""

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
        have, model = self.windows(), self.want_windows()
        assert have == model, ("windows", differing(have, model))

    def reserve(self, max_packets):
        rc = self.A.dev_transport_reserve_packets(self.tr, max_packets, self.sp)
        assert rc == 0, ("dev_transport_reserve_packets", max_packets, hex(rc))

    def launch(self, mode, d_wire, listed):
        """the call alone, on what `uploaded` made: nothing is copied, nothing waits"""
        d_packets, d_status, count = listed
        fn = self.A.dev_transport_seal_packets if mode == "seal" else self.A.dev_transport_open_packets
        rc = fn(self.tr, packets=d_packets.data_ptr(), count=count, wire=d_wire.data_ptr(), status=d_status.data_ptr(),
                stream=self.sp)
        assert rc == 0, ("dev_transport_%s_packets of %d" % (mode, count), hex(rc))

    def settle(self, mode, before, packets, d_wire, listed):
        """after a launch: the model's call on the bytes `before`; statuses, the
        whole wire, nonces, state bytes and windows must equal it.  Returns
        (the wire as it is now, the statuses, either)."""
        want_wire, want, either = P.run_packets(self.model, mode, bytes(before), packets)
        self.torch.cuda.synchronize()
        status, got = listed[1].cpu().numpy(), d_wire.cpu().numpy().tobytes()
        count = len(packets)
        assert status[:count].tolist() == want, (mode, "statuses", differing(status[:count].tolist(), want))
        assert (status[count:] == UNTOUCHED).all(), "a status past the last packet's"
        image = bytearray(want_wire)
        for p, (given, plain) in either.items():  # may hold either
            off, ln, _ = packets[p]
            assert got[off:off + ln] in (given, plain), ("either", p)
            image[off:off + ln] = got[off:off + ln]
        if got != bytes(image):
            at = next(k for k in range(len(got)) if got[k] != image[k])
            inside = [p for p, (off, ln, _) in enumerate(packets) if off <= at < off + ln and want[p] not in (4, 6)]
            assert False, (mode, "the wire differs from the model's at byte", at, "of packet", inside)
        self.check_state()
        return got, want, either

    def packets(self, mode, d_wire, packets):
        """one call on the device wire as it is, and in the model"""
        before = d_wire.cpu().numpy().tobytes()
        listed = uploaded(self.torch, packets)
        self.launch(mode, d_wire, listed)
        return self.settle(mode, before, packets, d_wire, listed)


def uploaded(torch, packets):
    """the list and its status bytes on the device: (d_packets, d_status, count)"""
    arr = np.array([(off, ln, slot) for off, ln, slot in packets], dtype=np.dtype(noise_aead.PACKET_DT))
    return dev(arr.view(np.uint8)), torch.full((len(packets) + 16,), UNTOUCHED, dtype=torch.uint8, device="cuda"), len(packets)


def lay(parts):
    """the parts one after another with 1 to 7 guard bytes between, so that they
    fall at odd and even offsets: (the wire, [offset of each part])"""
    wire, offs = bytearray([CANARY] * 5), []
    for k, s in enumerate(parts):
        offs.append(len(wire))
        wire += bytes(s) + bytes([CANARY]) * (1 + k % 7)
    return wire, offs


def on_device(torch, wire):
    return torch.from_numpy(np.frombuffer(bytes(wire), dtype=np.uint8).copy()).cuda()


def pair(aead, torch, oracle, cipher, seed, max_packets):
    keys = keys_for(seed)
    tabs = [Table(aead, torch, oracle, cipher, ini, 400, keys) for ini in (True, False)]
    for t in tabs:
        t.clear_keys(list(UNKEYED))
        t.reserve(max_packets)
    return tabs, keys


def room(payload):
    """a packet for the seal: 8 bytes of room, the payload, 16 bytes of room"""
    return bytes(8) + bytes(payload) + bytes(16)


def made(orc, cipher, key, counter, payload):
    """a packet as the peer would have sealed it"""
    if counter == TOP64:  # no such nonce
        return counter.to_bytes(8, "little") + bytes(payload) + bytes(16)
    return counter.to_bytes(8, "little") + orc.encrypt(cipher, key, counter, bytes(payload))


# ---------------------------------------------------------------- 1. scrambled traffic

def traffic(count, busy, payloads, seed):
    """`count` seal-ready packets in a scrambled arrival order with repeated
    slots, and their delivery: every packet once and a few twice, shuffled, at
    new offsets, a few of them forged.  The delivered wire is a gather of the
    sealed one: delivered = sealed[idx] ^ mask."""
    rng = np.random.default_rng(seed)
    slots = [busy[int(x)] for x in rng.integers(0, len(busy), count)] if count > 1 else [5]
    parts = [room(rng.integers(0, 256, payloads[(p + p // 9) % len(payloads)], dtype=np.uint8).tobytes()) for p in range(count)]
    wire, offs = lay(parts)
    sent = [(offs[p], len(parts[p]), slots[p]) for p in range(count)]
    arrive = list(range(count)) + [int(x) for x in rng.integers(0, count, min(7, count))]
    arrive = [arrive[int(q)] for q in rng.permutation(len(arrive))]
    wire_b, offs_b = lay([parts[p] for p in arrive])
    received = [(offs_b[q], len(parts[p]), slots[p]) for q, p in enumerate(arrive)]
    idx = np.zeros(len(wire_b), dtype=np.int64)  # byte 0 of the sealed wire is a guard byte
    mask = np.zeros(len(wire_b), dtype=np.uint8)
    forged = [q for q in range(len(arrive)) if q % 11 == 3 and count > 1]
    for q, p in enumerate(arrive):
        off, ln, _ = received[q]
        idx[off:off + ln] = np.arange(offs[p], offs[p] + ln)
        if q in forged:  # the tag, the ciphertext (or the tag's first byte), the counter's top byte, in turn
            mask[off + (ln - 1, 8, 7)[forged.index(q) % 3]] = 0x10
    return dict(parts=parts, wire=wire, sent=sent, arrive=arrive, received=received, idx=idx, mask=mask)


def scrambled(aead, torch, oracle, cipher, count, busy, payloads, seed, max_packets=None):
    """Seal the traffic on an initiator table, deliver it with a gather on the
    device, open it on the responder table: nothing between the calls waits
    for the device.  Then everything against the model."""
    (a, b), _ = pair(aead, torch, oracle, cipher, 200 + count, max_packets or 2 * count + 8)
    t = traffic(count, busy, payloads, seed)
    d_a, d_idx, d_mask = on_device(torch, t["wire"]), torch.from_numpy(t["idx"]).cuda(), torch.from_numpy(t["mask"]).cuda()
    listed_a, listed_b = uploaded(torch, t["sent"]), uploaded(torch, t["received"])
    torch.cuda.synchronize()
    a.launch("seal", d_a, listed_a)
    d_b = d_a[d_idx] ^ d_mask
    b.launch("open", d_b, listed_b)
    sealed, st_a, _ = a.settle("seal", t["wire"], t["sent"], d_a, listed_a)
    assert set(st_a) == ({0, 6} if count > 1 else {0})
    delivered = (np.frombuffer(sealed, dtype=np.uint8)[t["idx"]] ^ t["mask"]).tobytes()
    opened, st_b, either = b.settle("open", delivered, t["received"], d_b, listed_b)
    assert either and set(st_b) == ({0, 1, 5, 6} if count > 1 else {0, 5})
    assert b.nonces(1) == [0] * N  # the receive nonces are not in it
    # what was accepted is what was sent
    for q, p in enumerate(t["arrive"]):
        if st_b[q] == 0:
            off, ln, _ = t["received"][q]
            assert opened[off + 8:off + ln - 16] == t["parts"][p][8:-16]
    a.free()
    b.free()


@pytest.mark.parametrize("count", [1, 64, 65, 200])
@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_scrambled_traffic(aead, gpu, oracle, cipher, count):
    import torch
    # 64 packets on a reservation for 3000: the device sort takes another path for 64 items than for 3000
    scrambled(aead, torch, oracle, cipher, count, BUSY, PAYLOADS, count, max_packets=3000 if count == 64 else None)


@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_scrambled_traffic_past_one_sort_block(aead, gpu, oracle, cipher):
    """1500 packets over every slot: the device sort's path for more than one workgroup's worth"""
    import torch
    scrambled(aead, torch, oracle, cipher, 1500, PERM, (0, 1, 15, 16, 17), 1500)


# ---------------------------------------------------------------- 2. the same bytes through section 11

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_cross_check_with_the_datagram_call(aead, gpu, oracle, cipher):
    import torch
    A = aead
    keys = keys_for(301)
    b1, b2 = (Table(A, torch, oracle, cipher, False, 400, keys) for _ in range(2))
    for t in (b1, b2):
        t.clear_keys(list(UNKEYED))
    b2.reserve(400)
    m = 24
    slots = PERM[:m]
    assert set(UNKEYED) & set(slots)
    rng = np.random.default_rng(301)
    senders = [None if i in UNKEYED else T.Session.of_role(oracle, cipher, True, *keys[i]) for i in range(N)]
    plain = [b"".join(D.seal_ready(rng.integers(0, 256, PAYLOADS[(j + 2 * k) % 9], dtype=np.uint8).tobytes())
                      for k in range(1 + j % 6)) for j in range(m)]
    sealed = [w[0] for w in D.run_datagrams(senders, "seal", plain, 400, slots)]
    delivered = []
    for j, s in enumerate(sealed):
        frames = D.walk(s)[0]
        parts = [bytearray(s[at - 2:at + L]) for at, L in frames]
        if j % 4 == 1:
            parts = parts[::-1]
        if j % 4 == 2:
            parts = parts + [parts[0]]  # a duplicate inside the call
        if j % 4 == 3 and len(parts) > 1:
            parts[1][-1] ^= 0x01  # forged
        delivered.append(b"".join(bytes(x) for x in parts))
    wire1, wire2 = Wire(torch, delivered), Wire(torch, delivered)
    before = wire2.dev.cpu().numpy().tobytes()
    packets = [(wire2.offs[j] + at, L, slots[j]) for j, s in enumerate(delivered) for at, L in D.walk(s)[0]]
    # the datagram call on one table
    want1 = D.run_datagrams(b1.model, "open", delivered, 400, slots)
    d_slots = dev_u32(slots)
    off = torch.tensor(wire1.offs, dtype=torch.int64, device="cuda")
    ln = torch.tensor(wire1.lens, dtype=torch.int32, device="cuda")
    res = torch.zeros((m, 6), dtype=torch.int32, device="cuda")
    fs = torch.full((400,), CANARY, dtype=torch.uint8, device="cuda")
    assert A.dev_transport_open_datagrams(b1.tr, slots=d_slots.data_ptr(), m=m, wire=wire1.dev.data_ptr(), off=off.data_ptr(),
                                          length=ln.data_ptr(), result=res.data_ptr(), frame_status=fs.data_ptr(),
                                          stream=b1.sp) == 0
    # the packet call on the other, packets at the frame bodies
    listed = uploaded(torch, packets)
    b2.launch("open", wire2.dev, listed)
    opened2, statuses, either = b2.settle("open", before, packets, wire2.dev, listed)
    assert either and {0, 1, 5, 6} == set(statuses)
    # equal frame statuses
    r, fs = res.cpu().numpy().view(np.uint32), fs.cpu().numpy()
    per_frame = []
    for j in range(m):
        frames, first = int(r[j][0]), int(r[j][4])
        count = len(D.walk(delivered[j])[0])
        if slots[j] in UNKEYED:
            assert frames == 0 and int(r[j][2]) == D.ERROR_INVALID_STATE
            per_frame += [P.NO_SESSION] * count
        else:
            assert frames == count and fs[first:first + frames].tolist() == want1[j][2]
            per_frame += fs[first:first + frames].tolist()
    assert per_frame == statuses
    # equal windows, equal plaintext (a frame that may hold either holds one of its two forms in both)
    b1.check_state()
    assert b1.windows() == b2.windows() and b1.nonces(1) == b2.nonces(1) == [0] * N
    opened1 = bytearray(wire1.dev.cpu().numpy().tobytes())
    for p, (given, plain_form) in either.items():
        at, L, _ = packets[p]
        assert bytes(opened1[at:at + L]) in (given, plain_form)
        opened1[at:at + L] = opened2[at:at + L]
    assert bytes(opened1) == opened2
    b1.free()
    b2.free()


# ---------------------------------------------------------------- 3. every packet on one slot

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_skew_all_packets_on_one_slot(aead, gpu, oracle, cipher):
    import torch
    keys = keys_for(311)
    b = Table(aead, torch, oracle, cipher, False, 8, keys)
    b.reserve(200)
    slot, t0 = 29, 7 * 1024 + 5
    b.set_window(slot, D.Window(t0, sum(1 << (c % 1024) for c in (t0 - 1, t0 - 1024, t0 - 500))))
    b.check_state()
    rng = np.random.default_rng(311)
    rising = [t0 + int(x) for x in rng.permutation(60)]
    jump = t0 + 60 + 1500
    counters = [t0 - 1025, t0 - 1024, t0 - 1023, t0 - 1, t0 - 500, t0 - 499]      # the preset window's edges
    counters += rising + rising[5:15]                                             # reordered, then in-call duplicates
    counters += [jump, t0 + 10, t0 + 70, t0 + 600, jump, jump - 1024, jump - 1023]  # a jump of a window and more, what it left behind
    counters += [jump + 1 + int(x) for x in rng.permutation(200 - len(counters) - 1)] + [TOP64]
    assert len(counters) == 200
    parts = [made(oracle, cipher, keys[slot][0], c, rng.integers(0, 256, PAYLOADS[k % 9], dtype=np.uint8).tobytes())
             for k, c in enumerate(counters)]  # the responder receives under k1
    wire, offs = lay(parts)
    packets = [(offs[k], len(parts[k]), slot) for k in range(200)]
    d_wire = on_device(torch, wire)
    _, statuses, either = b.packets("open", d_wire, packets)
    assert statuses[:6] == [5, 5, 0, 5, 5, 0] and statuses[6:66] == [0] * 60 and statuses[66:76] == [5] * 10
    assert statuses[76:83] == [0, 5, 5, 0, 5, 5, 0] and statuses[83:199] == [0] * 116 and statuses[199] == 5
    # made replays inside the call: the ten duplicates, the three the jump left behind, the jump's own duplicate
    assert sorted(either) == list(range(66, 76)) + [77, 78, 80, 81]
    assert D.window(b.model[slot]).top == jump + 117
    b.free()


# ---------------------------------------------------------------- 4. refusals

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_refused_packets_touch_nothing_and_take_no_counter(aead, gpu, oracle, cipher):
    import torch
    (a, b), keys = pair(aead, torch, oracle, cipher, 321, 32)
    good = room(b"sixteen byte pay")
    bad = [(5, 0), (5, 23), (5, 65536), (N, len(good)), (2 ** 32 - 1, len(good)), (UNKEYED[0], len(good))]
    order = [(5, len(good))] + [x for pair_ in zip(bad, [(5, len(good)), (30, len(good))] * 3) for x in pair_]
    wire, offs = lay([good] * len(order))
    packets = [(offs[k], ln, slot) for k, (slot, ln) in enumerate(order)]
    want = [0, 4, 0, 4, 0, 4, 0, 6, 0, 6, 0, 6, 0]
    d_wire = on_device(torch, wire)
    sealed, statuses, _ = a.packets("seal", d_wire, packets)
    assert statuses == want
    counters = [int.from_bytes(sealed[off:off + 8], "little") for off, _, _ in packets]
    assert counters == [0, 0, 1, 0, 0, 0, 2, 0, 1, 0, 3, 0, 2]  # slots 5 and 30 count on past the refused ones
    for k, (off, _, _) in enumerate(packets):
        assert (sealed[off:off + len(good)] == good) == (want[k] != 0)
    assert a.nonces(0)[5] == 4 and a.nonces(0)[30] == 3
    # the open: the same list on the sealed bytes; the refused ones meet no window
    opened, statuses, either = b.packets("open", d_wire, packets)
    assert statuses == want and not either
    assert D.window(b.model[5]).words()[:2] == [4, 0b1111] and D.window(b.model[30]).words()[:2] == [3, 0b111]
    a.free()
    b.free()


# ---------------------------------------------------------------- 5. the seal's counter runs out

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_seal_stops_where_the_counter_runs_out(aead, gpu, oracle, cipher):
    import torch
    (a, b), keys = pair(aead, torch, oracle, cipher, 331, 32)
    a.set_nonces(0, {5: TOP64 - 2, 30: 2 ** 63})
    part = room(bytes(range(33)))
    slots = [5, 30, 5, 5, 30, 5, 0, 5]
    wire, offs = lay([part] * len(slots))
    packets = [(offs[k], len(part), s) for k, s in enumerate(slots)]
    d_wire = on_device(torch, wire)
    sealed, statuses, _ = a.packets("seal", d_wire, packets)
    assert statuses == [0, 0, 0, 5, 0, 5, 0, 5]
    assert a.nonces(0)[5] == TOP64 and a.nonces(0)[30] == 2 ** 63 + 2 and a.nonces(0)[0] == 1
    for k in (3, 5, 7):
        assert sealed[offs[k]:offs[k] + len(part)] == part
    # once more: the slot stays where it is
    _, statuses, _ = a.packets("seal", on_device(torch, wire), packets[:4])
    assert statuses == [5, 0, 5, 5] and a.nonces(0)[5] == TOP64
    # the peer takes 2^64 - 3 and 2^64 - 2; the unsealed packets claim counter 0, far behind by then
    _, statuses, either = b.packets("open", d_wire, packets)
    assert statuses == [0, 0, 0, 5, 0, 5, 0, 5] and not either and D.window(b.model[5]).top == TOP64
    a.free()
    b.free()


# ---------------------------------------------------------------- 6. composition in stream order

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_packet_calls_compose_with_the_other_calls(aead, gpu, oracle, cipher):
    import torch
    (a, b), keys = pair(aead, torch, oracle, cipher, 341, 32)
    rng = np.random.default_rng(341)
    slots = [5, 0, 5, 30, 0, 5, 66, 0, 5, 30]

    def round_trip(want_counters):
        parts = [room(rng.integers(0, 256, PAYLOADS[k % 9], dtype=np.uint8).tobytes()) for k in range(len(slots))]
        wire, offs = lay(parts)
        packets = [(offs[k], len(parts[k]), s) for k, s in enumerate(slots)]
        d_wire = on_device(torch, wire)
        sealed, statuses, _ = a.packets("seal", d_wire, packets)
        assert statuses == [0] * len(slots)
        assert [int.from_bytes(sealed[off:off + 8], "little") for off, _, _ in packets] == want_counters
        recv = b.nonces(1)
        opened, statuses, _ = b.packets("open", d_wire, packets)
        assert statuses == [0] * len(slots) and b.nonces(1) == recv  # a packet open leaves the receive nonces alone
        for k, (off, ln, _) in enumerate(packets):
            assert opened[off + 8:off + ln - 16] == parts[k][8:-16]

    round_trip([0, 0, 1, 0, 1, 2, 0, 2, 3, 1])
    # a rekey of slot 5 on both sides and new keys for slot 0, with no wait before the next packet calls
    for t, direction in ((a, R.SEND), (b, R.RECEIVE)):
        d_slots = dev_u32([5])
        assert aead.dev_transport_rekey(t.tr, slots=d_slots.data_ptr(), m=1, directions=direction, stream=t.sp) == 0
        assert R.rekey_table(t.model, direction, 1, [5]) == [(5, direction)]
    fresh = keys_for(342, 1)
    a.set_keys([0], fresh)
    b.set_keys([0], fresh)
    round_trip([4, 0, 5, 2, 1, 6, 1, 2, 7, 3])  # slot 5 goes on under its next key, slot 0 starts again
    # a stream tick in between leaves the windows alone
    keyed = {i: a.nonces(0)[i] for i in range(N) if i not in UNKEYED}
    b.set_nonces(1, keyed)
    windows = b.windows()
    stream = Wire(torch, plain_streams(343, big=False))
    a.run("seal", stream)
    b.run("open", stream)
    assert b.windows() == windows and a.windows() == [[0] * 17] * N
    assert b.nonces(1) == [0 if i in UNKEYED else keyed[i] + i % 6 for i in range(N)]
    sends = a.nonces(0)
    round_trip([sends[s] + slots[:k].count(s) for k, s in enumerate(slots)])  # the sends go on from where the stream left them
    a.free()
    b.free()


# ---------------------------------------------------------------- 7. the reservation and the rules behind it

def test_reservation_and_argument_rules_on_a_small_object(aead, gpu, oracle):
    """the rules of section 13 that need a reservation, in order, each with
    everything after it wrong as well; a refused call launches nothing"""
    import torch
    A = aead
    BAD, STATE = A.ERROR_INVALID_PARAM, A.ERROR_INVALID_STATE
    tab = Table(A, torch, oracle, T.CHACHAPOLY, True, 8, keys_for(351, 4), n=4)
    part = room(b"twenty bytes of load")
    wire, offs = lay([part] * 9)
    d_wire = on_device(torch, wire)
    packets = [(offs[k], len(part), k % 4) for k in range(9)]
    # one allocation: 8 status bytes, the list of 8 (8-byte aligned), 8 status bytes — touching it on both sides
    arr = np.array(packets[:8], dtype=np.dtype(A.PACKET_DT)).view(np.uint8)
    block = torch.full((8 + 128 + 8 + 16,), UNTOUCHED, dtype=torch.uint8, device="cuda")
    block[8:136] = torch.from_numpy(arr.copy()).cuda()
    base = block.data_ptr()
    assert base % 8 == 0
    ok = dict(packets=base + 8, wire=d_wire.data_ptr(), status=base + 136, stream=tab.sp)
    calls = (A.dev_transport_seal_packets, A.dev_transport_open_packets)
    for call in calls:
        assert call(tab.tr, count=8, **ok) == STATE and call(tab.tr, count=0, **ok) == 0  # not reserved yet
    assert A.dev_transport_reserve_packets(tab.tr, 0, tab.sp) == BAD
    assert A.dev_transport_reserve_packets(tab.tr, 2 ** 31 + 1, tab.sp) == BAD
    tab.reserve(8)
    assert A.dev_transport_reserve_packets(tab.tr, 8, tab.sp) == STATE
    assert A.dev_transport_reserve_packets(tab.tr, 0, tab.sp) == BAD  # the argument before the state
    for call in calls:
        assert call(tab.tr, count=9, **{**ok, "packets": 0}) == BAD                    # count > max_packets
        for k in ("packets", "wire", "status"):
            assert call(tab.tr, count=8, **{**ok, k: 0, **({} if k == "status" else {"status": base + 8})}) == BAD, k
        for status in (base + 8, base + 1, base + 135, base + 8 + 64):
            assert call(tab.tr, count=8, **{**ok, "status": status}) == BAD, status - base  # the statuses meet the list
        assert call(tab.tr, count=0, **{**ok, "status": base + 8}) == 0                # count == 0 first
    torch.cuda.synchronize()
    tab.check_state()  # nothing was launched: no send moved, the wire and the block as they were
    assert d_wire.cpu().numpy().tobytes() == bytes(wire)
    assert (block[:8] == UNTOUCHED).all() and (block[136:] == UNTOUCHED).all() and (block[8:136].cpu() == torch.from_numpy(arr)).all()
    # count == max_packets works, with the statuses touching the list from above, then from below
    want_wire, want, _ = P.run_packets(tab.model, "seal", bytes(wire), packets[:8])
    assert A.dev_transport_seal_packets(tab.tr, count=8, **ok) == 0
    torch.cuda.synchronize()
    assert block[136:144].tolist() == want == [0] * 8 and d_wire.cpu().numpy().tobytes() == want_wire
    assert (block[:8] == UNTOUCHED).all() and (block[144:] == UNTOUCHED).all() and (block[8:136].cpu() == torch.from_numpy(arr)).all()
    tab.check_state()
    d_wire = on_device(torch, wire)
    want_wire, want, _ = P.run_packets(tab.model, "seal", bytes(wire), packets[:8])
    assert A.dev_transport_seal_packets(tab.tr, count=8, **{**ok, "wire": d_wire.data_ptr(), "status": base}) == 0
    torch.cuda.synchronize()
    assert block[:8].tolist() == want == [0] * 8 and d_wire.cpu().numpy().tobytes() == want_wire
    assert tab.nonces(0) == [4, 4, 4, 4]
    tab.free()  # _free after a reservation
    # an object with n == 0: every packet has no session
    rc, tr = A.dev_transport_new_unkeyed(A.AESGCM, A.ROLE_RESPONDER, 0, max_frames=0, stream=tab.sp)
    assert rc == 0 and tr
    assert A.dev_transport_reserve_packets(tr, 4, tab.sp) == 0
    d_wire = on_device(torch, wire)
    for call in calls:
        listed = uploaded(torch, packets[:3] + [(0, 0, 2 ** 32 - 1)])
        assert call(tr, packets=listed[0].data_ptr(), count=4, wire=d_wire.data_ptr(), status=listed[1].data_ptr(), stream=tab.sp) == 0
        torch.cuda.synchronize()
        assert listed[1].tolist() == [6] * 4 + [UNTOUCHED] * 16
        assert call(tr, packets=listed[0].data_ptr(), count=5, wire=d_wire.data_ptr(), status=listed[1].data_ptr(), stream=tab.sp) == BAD
    assert d_wire.cpu().numpy().tobytes() == bytes(wire)
    assert A.dev_transport_free(tr) == 0
