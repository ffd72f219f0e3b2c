"""A plain model of the device-resident transport sessions
(noise_aead_dev_transport_*, include/noise_aead_hip.h section 9).

One session: the frame walk over its stream, the per-frame seal and open
through the oracle's encrypt / decrypt, and the nonce and result rules.  A
batch: the cap across sessions.  tests/test_transport_model_host.py proves the
session against the reference's CipherState calls frame by frame;
tests/test_transport_host.py feeds the walk's cases to the C++ walk the
kernels compile; tests/test_gpu_transport.py compares the device with it."""
CHACHAPOLY, AESGCM = 0x4301, 0x4302
ERROR_NONE = 0
ERROR_MAC_FAILURE = 0x4504
ERROR_INVALID_LENGTH = 0x450A
ERROR_INVALID_NONCE = 0x450D
NONCE_LIMIT = 2 ** 64 - 1
MAC_LEN = 16
NO_BUDGET = 2 ** 64 - 1


def frame(body: bytes) -> bytes:
    """a frame around L = len(body) bytes"""
    assert len(body) <= 65535
    return bytes((len(body) >> 8, len(body) & 0xFF)) + bytes(body)


def walk(stream: bytes, nonce: int, budget: int = NO_BUDGET):
    """([(offset of the body, L)], consumed, stop): the frames taken from the
    start of the stream, frame k under nonce + k.  The checks of a frame, in
    the order of wire.c scan_frames: partial (stop with ERROR_NONE), L < 16,
    nonce + k exhausted; then the budget: a frame that would be taken as
    number `budget` is left for the next call with ERROR_NONE."""
    frames, off, stop = [], 0, ERROR_NONE
    while off + 2 <= len(stream):
        L = (stream[off] << 8) | stream[off + 1]
        if off + 2 + L > len(stream):
            break
        if L < MAC_LEN:
            stop = ERROR_INVALID_LENGTH
            break
        if nonce + len(frames) == NONCE_LIMIT:
            stop = ERROR_INVALID_NONCE
            break
        if len(frames) == budget:
            break
        frames.append((off + 2, L))
        off += 2 + L
    return frames, off, stop


def cap(base: int, count: int, max_frames: int):
    """(budget, cut) of a session whose uncapped walk takes `count` frames
    numbered from `base` in the batch: uncut when they all lie below
    max_frames; else the frames below max_frames, and the session reports
    ERROR_NONE whatever its walk met."""
    if base + count <= max_frames:
        return count, False
    return max(max_frames - base, 0), True


class Session:
    """The two CipherStates of one session: keys and nonces."""

    def __init__(self, orc, cipher, send_key, recv_key, send_nonce=0, recv_nonce=0):
        self.orc, self.cipher = orc, cipher
        self.send_key, self.recv_key = bytes(send_key), bytes(recv_key)
        self.send, self.recv = send_nonce, recv_nonce

    @classmethod
    def of_role(cls, orc, cipher, initiator, k1, k2):
        """the initiator sends under k1, the responder under k2"""
        return cls(orc, cipher, k1, k2) if initiator else cls(orc, cipher, k2, k1)

    def start_nonce(self, mode):
        return {"seal": self.send, "open": self.recv, "echo": max(self.send, self.recv)}[mode]

    def run(self, mode, stream: bytes, budget: int = NO_BUDGET, cut: bool = False):
        """(stream after the call, (frames, consumed, error), later): what
        seal_frames / open_frames / echo_frames do to this session's stream.
        later: {body offset: (as given, plaintext)} of the walked frames after
        a failed one whose own tag verified — each may hold either."""
        out = bytearray(stream)
        frames, consumed, stop = walk(stream, self.start_nonce(mode), budget)
        if cut:
            stop = ERROR_NONE
        if mode == "seal":
            for k, (at, L) in enumerate(frames):
                out[at:at + L] = self.orc.encrypt(self.cipher, self.send_key, self.send + k, bytes(stream[at:at + L - 16]))
            self.send += len(frames)
            return bytes(out), (len(frames), consumed, stop), {}
        prefix, later = len(frames), {}
        for k, (at, L) in enumerate(frames):
            rc, pt = self.orc.decrypt(self.cipher, self.recv_key, self.recv + k, bytes(stream[at:at + L]))
            if k < prefix and rc != 0:
                prefix = k
            elif k < prefix:  # the tag bytes are left as they were
                out[at:at + L - 16] = pt
                if mode == "echo":
                    out[at:at + L] = self.orc.encrypt(self.cipher, self.send_key, self.send + k, pt)
            elif rc == 0:
                later[at] = (bytes(stream[at:at + L]), pt + bytes(stream[at + L - 16:at + L]))
        result = (len(frames), consumed, stop)
        if prefix < len(frames):
            result = (prefix, frames[prefix][0] - 2, ERROR_MAC_FAILURE)
        self.recv += prefix
        if mode == "echo":
            self.send += prefix
        return bytes(out), result, later


def run_batch(sessions, mode, streams, max_frames):
    """One call over a batch: [(stream after, result, later)] per session.
    The walked frames are numbered in session order; the cap cuts there."""
    out, base = [], 0
    for s, stream in zip(sessions, streams):
        count = len(walk(stream, s.start_nonce(mode))[0])
        budget, cut = cap(base, count, max_frames)
        out.append(s.run(mode, stream, budget, cut) if (budget or not cut) else (bytes(stream), (0, 0, ERROR_NONE), {}))
        base += count
    return out


# ---- the cases of the walk for asan/transport_check (tests/test_transport_host.py)

def walk_cases():
    """[(name, stream, nonce, budget)]"""
    def f(L, fill=0x5A):
        return frame(bytes([fill]) * L)
    five = b"".join(f(16 + k, k) for k in range(5))
    return [
        ("empty", b"", 0, NO_BUDGET),
        ("one byte", b"\x00", 0, NO_BUDGET),
        ("header only", b"\x00\x10", 0, NO_BUDGET),
        ("header of an empty frame", b"\x00\x00", 0, NO_BUDGET),
        ("L=15", f(15), 0, NO_BUDGET),
        ("L=16", f(16), 0, NO_BUDGET),
        ("L=17", f(17), 0, NO_BUDGET),
        ("L=15 after two", f(16) + f(40) + f(15) + f(16), 7, NO_BUDGET),
        ("L=65535 fills the stream", f(65535), 0, NO_BUDGET),
        ("L=65535 short by one", f(65535)[:-1], 0, NO_BUDGET),
        ("partial last frame, short by one", f(16) + f(80) + f(33)[:-1], 0, NO_BUDGET),
        ("partial L<16 is partial", f(16) + f(15)[:-1], 0, NO_BUDGET),
        ("trailing byte", f(16) + b"\x00", 0, NO_BUDGET),
        ("nonce 3 below the limit, 5 frames", five, NONCE_LIMIT - 3, NO_BUDGET),
        ("nonce at the limit", five, NONCE_LIMIT, NO_BUDGET),
        ("nonce 1 below the limit", five, NONCE_LIMIT - 1, NO_BUDGET),
        ("nonce 5 below the limit, 5 frames", five, NONCE_LIMIT - 5, NO_BUDGET),
        ("L<16 before the nonce", f(16) + f(3), NONCE_LIMIT - 1, NO_BUDGET),
        ("budget cuts mid-way", five, 0, 3),
        ("budget 0", five, 0, 0),
        ("budget 0, empty stream", b"", 0, 0),
        ("budget equals the frames", five, 0, 5),
        ("budget larger", five, 0, 6),
        ("budget ends at a short frame", f(16) + f(16) + f(2), 0, 2),
        ("budget ends at the nonce limit", five, NONCE_LIMIT - 2, 2),
        ("budget before a short frame", f(16) + f(16) + f(2), 0, 1),
    ]


def walk_case_line(stream, nonce, budget, expect=None):
    """stream hex ('-' for the empty one), nonce, budget, frames, consumed, stop"""
    frames, consumed, stop = expect if expect is not None else walk(stream, nonce, budget)
    n = frames if isinstance(frames, int) else len(frames)
    return f"{stream.hex() or '-'} {nonce} {budget} {n} {consumed} {stop}\n"
