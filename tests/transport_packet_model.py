"""A plain model of packet transport (noise_aead_dev_transport_seal_packets /
_open_packets, include/noise_aead_hip.h section 13): the packets of a list one
by one, in list order, over the windows of tests/transport_datagram_model.py
and the oracle's AEAD.  tests/test_transport_packet_host.py holds it to the
section-11 model on the same bytes; tests/test_gpu_transport_packet.py
compares the device with it."""
import transport_model as T
import transport_datagram_model as D

OK, FORGED, LENGTH, REPLAY, NO_SESSION = 0, 1, 4, 5, 6
MIN_LEN, MAX_LEN = D.MIN_L, 65535


def run_packets(sessions, mode, wire, packets):
    """One call ("seal" or "open") over packets = [(off, len, slot)] on the
    bytes `wire`; sessions[i] is the T.Session of slot i, or None for an
    unkeyed one.  Returns (the wire after the call, [status of each packet],
    either); either: {p: (as given, with its plaintext)}, the len bytes of the
    status-5 packets that may hold either.  Sends and windows advance."""
    assert mode in ("seal", "open")
    n, out = len(sessions), bytearray(wire)
    before = {i: D.window(s).copy() for i, s in enumerate(sessions) if s is not None}
    statuses, either = [], {}
    for p, (off, ln, slot) in enumerate(packets):
        if not 0 <= slot < n or sessions[slot] is None:
            statuses.append(NO_SESSION)
            continue
        if ln < MIN_LEN or ln > MAX_LEN:
            statuses.append(LENGTH)
            continue
        s = sessions[slot]
        assert off + ln <= len(wire), "a packet past the end of the wire"
        given = bytes(wire[off:off + ln])
        if mode == "seal":
            if s.send == T.NONCE_LIMIT:
                statuses.append(REPLAY)
                continue
            out[off:off + 8] = s.send.to_bytes(8, "little")
            out[off + 8:off + ln] = s.orc.encrypt(s.cipher, s.send_key, s.send, given[8:ln - 16])
            s.send += 1
            statuses.append(OK)
            continue
        c, w = int.from_bytes(given[:8], "little"), D.window(s)
        if not w.check(c):
            statuses.append(REPLAY)
            # only an earlier packet of this call made it a replay: it was opened before the window moved
            if before[slot].check(c):
                rc, pt = s.orc.decrypt(s.cipher, s.recv_key, c, given[8:])
                if rc == 0:
                    either[p] = (given, given[:8] + pt + given[ln - 16:])
            continue
        rc, pt = s.orc.decrypt(s.cipher, s.recv_key, c, given[8:])
        if rc != 0:
            statuses.append(FORGED)
            continue
        out[off + 8:off + ln - 16] = pt  # the tag bytes are left as they were
        w.accept(c)
        statuses.append(OK)
    return bytes(out), statuses, either
