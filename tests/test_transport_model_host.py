"""The transport model (tests/transport_model.py) against the reference and
against the wire path's own frame parser.

Where the reference library is available (the `reflib` fixture; absent on the
GPU machine, where the conftest skips), the model's seal and open of a session
equal frame-by-frame noise_cipherstate_encrypt / _decrypt of the reference on
one CipherState per direction, for both ciphers — including the rule that a
MAC failure leaves the nonce where it was (cipherstate.c:400-405)."""
import ctypes as C

import numpy as np
import pytest

import noise_aead
import transport_model as T

LENS = (16, 17, 80, 1416, 65535)


def session_stream(rng, lens):
    """(seal-ready stream, plaintexts): frames of the given L"""
    pts = [rng.integers(0, 256, L - 16, dtype=np.uint8).tobytes() for L in lens]
    return b"".join(T.frame(pt + bytes(16)) for pt in pts), pts


class RefState:
    """one reference CipherState, called frame by frame"""

    def __init__(self, reflib, cipher, key, nonce):
        from oracle import NoiseBuffer
        self.L, self.NB = reflib.L, NoiseBuffer
        self.st = reflib._state(cipher, key, nonce)

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
def test_model_equals_the_reference_frame_by_frame(oracle, reflib, cipher):
    rng = np.random.default_rng(cipher)
    k1, k2 = rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    start = 5
    stream, pts = session_stream(rng, LENS + (40, 16))
    ini = T.Session.of_role(oracle, cipher, True, k1, k2)
    res = T.Session.of_role(oracle, cipher, False, k1, k2)
    ini.send = res.recv = start
    sealed, result, _ = ini.run("seal", stream)
    assert result == (len(pts), len(stream), 0) and ini.send == start + len(pts)
    # the reference's initiator: one state under k1, frame by frame
    ref = RefState(reflib, cipher, k1, start)
    for (at, L), pt in zip(T.walk(sealed, 0)[0], pts):
        rc, ct = ref.encrypt(pt)
        assert rc == 0 and sealed[at:at + L] == ct
    ref.free()

    # the responder opens it: frame 3 forged.  The reference's state refuses it, stays at its nonce (the untouched
    # frame still opens under it), and the model reports the prefix
    frames = T.walk(sealed, 0)[0]
    forged = bytearray(sealed)
    forged[frames[3][0] + 5] ^= 0x10
    opened, result, later = res.run("open", bytes(forged))
    assert result == (3, frames[3][0] - 2, T.ERROR_MAC_FAILURE) and res.recv == start + 3
    ref = RefState(reflib, cipher, k1, start)
    for k, (at, L) in enumerate(frames[:3]):
        rc, pt = ref.decrypt(forged[at:at + L])
        assert rc == 0 and pt == pts[k] and opened[at:at + L - 16] == pt
        assert opened[at + L - 16:at + L] == forged[at + L - 16:at + L]  # the tag bytes stay
    at, L = frames[3]
    rc, _ = ref.decrypt(forged[at:at + L])
    assert rc == T.ERROR_MAC_FAILURE and opened[at:at + L] == forged[at:at + L]
    rc, pt = ref.decrypt(sealed[at:at + L])  # nonce not advanced on the failure
    assert rc == 0 and pt == pts[3]
    ref.free()
    # frames after the failed one: each tag is good under nonce + k, so each may hold its plaintext
    assert sorted(later) == [f[0] for f in frames[4:]]
    for k, (at, L) in enumerate(frames[4:], 4):
        assert later[at] == (sealed[at:at + L], pts[k] + sealed[at + L - 16:at + L])
        assert opened[at:at + L] == sealed[at:at + L]  # the model's own image keeps them as given
    # the caller drops the forged frame's bytes for the true ones and calls again from `consumed`
    rest = sealed[result[1]:]
    opened2, result2, _ = res.run("open", rest)
    assert result2 == (len(pts) - 3, len(rest), 0) and res.recv == start + len(pts)
    assert [opened2[a:a + L - 16] for a, L in T.walk(rest, 0)[0]] == pts[3:]


def test_model_echo_is_open_then_seal_of_the_prefix(oracle):
    rng = np.random.default_rng(9)
    k1, k2 = bytes(range(32)), bytes(range(32, 64))
    stream, pts = session_stream(rng, (16, 80, 17, 40))
    client = T.Session.of_role(oracle, T.CHACHAPOLY, True, k1, k2)
    server = T.Session.of_role(oracle, T.CHACHAPOLY, False, k1, k2)
    server.send = 100
    sealed = client.run("seal", stream)[0]
    forged = bytearray(sealed)
    frames = T.walk(sealed, 0)[0]
    forged[frames[2][0]] ^= 1
    echoed, result, _ = server.run("echo", bytes(forged))
    assert result == (2, frames[2][0] - 2, T.ERROR_MAC_FAILURE) and (server.recv, server.send) == (2, 102)
    for k, (at, L) in enumerate(frames[:2]):
        assert echoed[at:at + L] == oracle.encrypt(T.CHACHAPOLY, k2, 100 + k, pts[k])
    assert echoed[frames[2][0] - 2:] == bytes(forged[frames[2][0] - 2:])


def test_model_walk_equals_parse_frames_on_well_formed_wires():
    rng = np.random.default_rng(3)
    for trial in range(40):
        lens = [int(rng.choice(LENS[:4] + (16, 300))) for _ in range(int(rng.integers(0, 7)))]
        wire = b"".join(T.frame(rng.integers(0, 256, L, dtype=np.uint8).tobytes()) for L in lens)
        for cut in (0, 1, 2, 5):  # and with a partial frame at the end
            w = wire[:len(wire) - cut] if cut <= len(wire) else wire
            frames, consumed, stop = T.walk(w, 0)
            assert frames == noise_aead.parse_frames(w) and stop == 0
            assert consumed == (frames[-1][0] + frames[-1][1] if frames else 0)
            for count in (0, 1, 3):
                assert T.walk(w, 0, count)[0] == noise_aead.parse_frames(w, count)


def test_model_batch_cap_continues_to_the_uncapped_result(oracle):
    """run_batch under a cap, continued from `consumed`, equals one uncapped call"""
    rng = np.random.default_rng(11)
    streams, keys = [], []
    for i in range(7):
        streams.append(session_stream(rng, [LENS[(i + k) % 4] for k in range(i % 4)])[0] + (b"\x00\x05abcde" if i == 4 else b""))
        keys.append((rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes()))
    total = sum(len(T.walk(s, 0)[0]) for s in streams)

    def fresh():
        return [T.Session.of_role(oracle, T.AESGCM, True, *k) for k in keys]
    whole = T.run_batch(fresh(), "seal", streams, total)
    assert [r[1][2] for r in whole] == [0, 0, 0, 0, T.ERROR_INVALID_LENGTH, 0, 0]
    for cap in (1, 2, total - 1, total, total + 5):
        sess, pos = fresh(), [0] * 7
        image = [bytearray(s) for s in streams]
        errors, calls = [0] * 7, 0
        while True:
            out = T.run_batch(sess, "seal", [bytes(image[i][pos[i]:]) for i in range(7)], cap)
            calls += 1
            assert sum(r[1][0] for r in out) <= cap
            for i, (after, (frames, consumed, error), _) in enumerate(out):
                image[i][pos[i]:] = after
                pos[i] += consumed
                errors[i] = error
            if sum(r[1][0] for r in out) == 0:
                break
        assert [bytes(b) for b in image] == [r[0] for r in whole], cap
        assert errors == [r[1][2] for r in whole] and pos == [r[1][1] for r in whole]
        assert calls == -(-total // cap) + 1
