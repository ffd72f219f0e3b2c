"""A plain model of datagram transport (noise_aead_dev_transport_seal_datagrams
/ _open_datagrams, include/noise_aead_hip.h section 11) on top of
tests/transport_model.py.

The anti-replay window in plain Python integers, the 24-byte frame walk, and
one call over a list of entries: the seal writes counter send + k in front of
each frame, the open judges every frame alone, in stream order, against the
window.  tests/test_transport_datagram_model_host.py proves it against the
reference's set_nonce + encrypt / decrypt and against a set-of-seen-counters
model; tests/test_gpu_transport_datagram.py compares the device with it."""
import transport_model as T

ERROR_INVALID_PARAM = 0x450B
ERROR_INVALID_STATE = 0x450C
COUNTER_LEN = 8
MIN_L = COUNTER_LEN + T.MAC_LEN
REPLAY_BITS = 1024
REPLAY_WORDS = REPLAY_BITS // 64
OK, FORGED, REPLAY = 0, 1, 5


class Window:
    """top: the highest accepted counter + 1; bits: bit c % 1024 for counter c"""

    def __init__(self, top=0, bits=0):
        self.top, self.bits = top, bits

    def check(self, c):
        """whether counter c is fresh; reads only"""
        if c == T.NONCE_LIMIT:
            return False
        if c >= self.top:
            return True
        if self.top - c > REPLAY_BITS:
            return False
        return not (self.bits >> (c % REPLAY_BITS)) & 1

    def accept(self, c):
        """a counter that check() found fresh"""
        if c >= self.top:
            if c - self.top >= REPLAY_BITS:
                self.bits = 0
            else:
                for x in range(self.top, c):
                    self.bits &= ~(1 << (x % REPLAY_BITS))
            self.top = c + 1
        self.bits |= 1 << (c % REPLAY_BITS)

    def words(self):
        """as the device holds it: [top, seen[0], .. seen[15]]"""
        return [self.top] + [(self.bits >> (64 * q)) & (2 ** 64 - 1) for q in range(REPLAY_WORDS)]

    @classmethod
    def of_words(cls, words):
        return cls(words[0], sum(w << (64 * q) for q, w in enumerate(words[1:])))

    def copy(self):
        return Window(self.top, self.bits)


def window(session) -> Window:
    """the session's window (a T.Session gets one the first time it is asked for)"""
    if not hasattr(session, "window"):
        session.window = Window()
    return session.window


def datagram(counter: int, body: bytes) -> bytes:
    """a frame around counter || body"""
    return T.frame(counter.to_bytes(8, "little") + bytes(body))


def seal_ready(payload: bytes) -> bytes:
    """a frame for the seal: 8 bytes of room, the payload, 16 bytes of room"""
    return T.frame(bytes(8) + bytes(payload) + bytes(16))


def walk(stream: bytes, nonce: int = 0, budget: int = T.NO_BUDGET):
    """T.walk with 24 as the smallest L"""
    frames, off, stop = [], 0, T.ERROR_NONE
    while off + 2 <= len(stream):
        L = (stream[off] << 8) | stream[off + 1]
        if off + 2 + L > len(stream):
            break
        if L < MIN_L:
            stop = T.ERROR_INVALID_LENGTH
            break
        if nonce + len(frames) == T.NONCE_LIMIT:
            stop = T.ERROR_INVALID_NONCE
            break
        if len(frames) == budget:
            break
        frames.append((off + 2, L))
        off += 2 + L
    return frames, off, stop


def counter_of(stream: bytes, at: int) -> int:
    return int.from_bytes(stream[at:at + 8], "little")


def _seal(s, stream, budget, cut):
    out = bytearray(stream)
    frames, consumed, stop = walk(stream, s.send, budget)
    for k, (at, L) in enumerate(frames):
        c = s.send + k
        out[at:at + 8] = c.to_bytes(8, "little")
        out[at + 8:at + L] = s.orc.encrypt(s.cipher, s.send_key, c, bytes(stream[at + 8:at + L - 16]))
    s.send += len(frames)
    return bytes(out), (len(frames), consumed, T.ERROR_NONE if cut else stop), [], {}


def _open(s, stream, budget, cut, first):
    out = bytearray(stream)
    frames, consumed, stop = walk(stream, 0, budget)
    w, before = window(s), window(s).copy()
    statuses, either = [], {}
    for at, L in frames:
        c = counter_of(stream, at)
        if not w.check(c):
            statuses.append(REPLAY)
            # only an earlier frame of this call made it a replay: it was opened before the window moved
            if before.check(c):
                rc, pt = s.orc.decrypt(s.cipher, s.recv_key, c, bytes(stream[at + 8:at + L]))
                if rc == 0:
                    either[at] = (bytes(stream[at:at + L]), bytes(stream[at:at + 8]) + pt + bytes(stream[at + L - 16:at + L]))
            continue
        rc, pt = s.orc.decrypt(s.cipher, s.recv_key, c, bytes(stream[at + 8:at + L]))
        if rc != 0:
            statuses.append(FORGED)
            continue
        out[at + 8:at + L - 16] = pt  # the tag bytes are left as they were
        w.accept(c)
        statuses.append(OK)
    result = (len(frames), consumed, T.ERROR_NONE if cut else stop, statuses.count(OK), first)
    return bytes(out), result, statuses, either


def run_datagrams(sessions, mode, streams, max_frames, slots=None):
    """One call ("seal" or "open") over entries 0 .. len(streams) - 1: entry j
    is slot slots[j] (slot j without a list); sessions[i] is the T.Session of
    slot i, or None for an unkeyed one.  Per entry: (stream after the call,
    result, [status of each walked frame], either).  The seal's result is
    (frames, consumed, error); the open's adds (accepted, first).  either:
    {body offset: (as given, with its plaintext)} of the status-5 frames that
    may hold either.  Sends and windows advance."""
    assert mode in ("seal", "open")
    n = len(sessions)
    slots = list(range(len(streams))) if slots is None else list(slots)
    assert len(slots) == len(streams)
    live = [j for j, i in enumerate(slots) if 0 <= i < n and sessions[i] is not None]
    assert len({slots[j] for j in live}) == len(live), "the listed slots must be distinct"
    fixed = (0, 0) if mode == "open" else ()
    out, base = [], 0
    for j, i in enumerate(slots):
        stream = bytes(streams[j])
        if j not in live:
            code = ERROR_INVALID_STATE if 0 <= i < n else ERROR_INVALID_PARAM
            out.append((stream, (0, 0, code) + fixed, [], {}))
            continue
        s = sessions[i]
        count = len(walk(stream, s.send if mode == "seal" else 0)[0])
        budget, cut = T.cap(base, count, max_frames)
        if mode == "seal":
            out.append(_seal(s, stream, budget, cut))
        else:
            out.append(_open(s, stream, budget, cut, base))
        base += count
    return out
