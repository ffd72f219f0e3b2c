"""The packet calls beside their models (header sections 13 and 14): a table
of slots with its windows (Table, on tests/transport_gpu.py's), a list and its
status bytes on the device, packets laid out between guard bytes, and the
receive batch the echo tests share (echo_batch).  What
tests/test_gpu_transport_packet.py keeps inside itself, restated for the tests
of the echo.  Importable without pytest and without torch (the callers pass
torch in); echo_batch needs neither a device nor the library."""
import numpy as np

import noise_aead
import transport_gpu
import transport_datagram_model as D
import transport_packet_model as P
import transport_packet_echo_model as E
from gpu_support import dev, peek_u64, poke_u64
from transport_gpu import differing

TOP64 = 2 ** 64 - 1
PAYLOADS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 1400)
CANARY = 0xEE
UNTOUCHED = 0x77
SLOTS = 6
UNKEYED = 3
KEYED = (0, 1, 2, 4, 5)


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
        """the call alone ("seal", "open" or "echo"), on what `uploaded` made: nothing is copied, nothing waits"""
        d_packets, d_status, count = listed
        fn = getattr(self.A, "dev_transport_%s_packets" % mode)
        rc = fn(self.tr, packets=d_packets.data_ptr(), count=count, wire=d_wire.data_ptr(), status=d_status.data_ptr(),
                stream=self.sp)
        assert rc == 0, ("dev_transport_%s_packets of %d" % (mode, count), hex(rc))

    def modelled(self, mode, before, packets):
        """the model's call on the bytes `before`: (wire, statuses, either); the model's sessions advance"""
        if mode == "echo":
            return E.run_echo(self.model, bytes(before), packets)
        return P.run_packets(self.model, mode, bytes(before), packets)

    def compare(self, mode, want, packets, d_wire, listed, state=True):
        """after a launch, against what `modelled` gave: every status, the whole
        wire with the bytes between the packets, and (state) nonces, state bytes
        and windows.  Returns (the wire as it is now, the statuses, either)."""
        want_wire, statuses, either = want
        self.torch.cuda.synchronize()
        status, got = listed[1].cpu().numpy(), d_wire.cpu().numpy().tobytes()
        count = len(packets)
        assert status[:count].tolist() == statuses, (mode, "statuses", differing(status[:count].tolist(), statuses))
        assert (status[count:] == UNTOUCHED).all(), "a status past the last packet's"
        image = bytearray(want_wire)
        for p, (given, plain) in either.items():  # may hold either
            off, ln, _ = packets[p]
            assert got[off:off + ln] in (given, plain), ("either", p)
            image[off:off + ln] = got[off:off + ln]
        if got != bytes(image):
            at = next(k for k in range(len(got)) if got[k] != image[k])
            inside = [(p, statuses[p]) for p, (off, ln, _) in enumerate(packets) if off <= at < off + ln and statuses[p] not in (4, 6)]
            assert False, (mode, "the wire differs from the model's at byte", at, "of (packet, status)", inside)
        if state:
            self.check_state()
        return got, statuses, either

    def packets(self, mode, d_wire, packets):
        """one call on the device wire as it is, and in the model"""
        before = d_wire.cpu().numpy().tobytes()
        listed = uploaded(self.torch, packets)
        want = self.modelled(mode, before, packets)
        self.launch(mode, d_wire, listed)
        return self.compare(mode, want, packets, d_wire, listed)


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


def room(payload):
    """a packet for the seal: 8 bytes of room, the payload, 16 bytes of room"""
    return bytes(8) + bytes(payload) + bytes(16)


def made(orc, cipher, key, counter, payload):
    """a packet as the peer would have sealed it"""
    if counter == TOP64:  # no such nonce
        return counter.to_bytes(8, "little") + bytes(payload) + bytes(16)
    return counter.to_bytes(8, "little") + orc.encrypt(cipher, key, counter, bytes(payload))


# ---------------------------------------------------------------- the echo's receive batch

T0 = 3000                                  # slot 1's window before the call: top, and what it has seen
SEEN = (T0 - 1, T0 - 5, T0 - 1024)
REFUSED = (T0 - 1, T0 - 5, T0 - 1024, T0 - 1025, 17, TOP64)  # what that window refuses as it stands
SENDS = {0: 0, 1: 1000, 2: 2 ** 40, 4: 7, 5: 2 ** 63}
FIRST = {0: 0, 1: T0, 2: 50, 4: 2 ** 33, 5: 9}  # each slot's first counter of the call


def preset(table):
    """the state echo_batch is made for: slot 1's window, every send"""
    table.set_window(1, D.Window(T0, sum(1 << (c % 1024) for c in SEEN)))
    table.set_nonces(0, SENDS)


def preset_sessions(sessions):
    """the same on a list of model sessions"""
    sessions[1].window = D.Window(T0, sum(1 << (c % 1024) for c in SEEN))
    for i, v in SENDS.items():
        sessions[i].send = v


def echo_batch(orc, cipher, keys, count, seed, payloads=PAYLOADS, slots=KEYED):
    """A receive batch of `count` packets for a responder table of SLOTS slots
    (slot UNKEYED has no key) in the state of `preset`, the slots scrambled and
    interleaved, each slot's counters arriving in swapped pairs.  Among the
    valid packets, by position: forged ones (the tag, the ciphertext or the
    tag's first byte, the counter's top byte in turn), counters slot 1's window
    refuses as it stands, duplicates of an earlier packet at another offset,
    len 23 and len 65 536, a slot past the table, the unkeyed slot; and, from
    64 packets on, half way through the list a jump of slot 2's top by 1500
    and then the counter it left behind.  A list of one packet is one valid
    packet.  Returns dict(parts, wire, packets, sent): sent[p] is the payload of
    a packet that was made valid (forged and duplicated ones too), else None."""
    rng = np.random.default_rng(seed)
    nxt = {i: 0 for i in KEYED}
    parts, listed, sent, valid = [], [], [], []
    jumped = None

    def fresh(slot):
        k = nxt[slot]
        nxt[slot] += 1
        return FIRST[slot] + (k ^ 1)

    for p in range(count):
        slot = slots[(7 * p + p // 5) % len(slots)]
        payload = rng.integers(0, 256, payloads[(p + p // 9) % len(payloads)], dtype=np.uint8).tobytes()
        ln, body = None, None
        kind = p % 32 if count > 1 else 0
        if count >= 64 and p == count // 2:
            assert kind % 16 != 3, "the jump would be forged"
            slot = 2
            jumped = FIRST[2] + nxt[2] + 1         # never handed out: fresh before the call, too old after the jump
            counter = jumped + 1500
            nxt[2] += 1502 + nxt[2] % 2            # even: the swapped pairs go on above the jump
        elif jumped is not None and p == count // 2 + 1:
            slot, counter, jumped = 2, jumped, None
        elif kind % 16 == 7:
            slot, counter = 1, REFUSED[(p // 16) % len(REFUSED)]
        elif kind % 16 == 11 and valid:
            q = valid[int(rng.integers(0, len(valid)))]
            slot, body, payload = listed[q][1], parts[q], sent[q]
        elif kind == 5:
            slot, counter = (SLOTS, 2 ** 32 - 1)[(p // 32) % 2], 1
        elif kind == 21:
            slot, counter = UNKEYED, 1
        else:
            counter = fresh(slot)
        if body is None:
            key = keys[slot][0] if 0 <= slot < SLOTS else keys[0][0]  # the responder receives under k1
            body = made(orc, cipher, key, counter, payload)
        body = bytearray(body)
        if kind % 16 == 3:
            at = (len(body) - 1, 8, 7)[(p // 16) % 3]
            body[at] ^= 0x10
        elif kind == 13:
            ln = 23
        elif kind == 29:
            ln = 65536
        elif kind % 16 not in (7, 11) and 0 <= slot < SLOTS and slot != UNKEYED:
            valid.append(p)
        parts.append(bytes(body))
        listed.append((ln if ln is not None else len(body), slot))
        sent.append(payload)
    wire, offs = lay(parts)
    packets = [(offs[p], listed[p][0], listed[p][1]) for p in range(count)]
    return dict(parts=parts, wire=wire, packets=packets, sent=sent)
