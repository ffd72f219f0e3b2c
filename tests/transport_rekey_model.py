"""A plain model of rekey on the device (noise_aead_dev_rekey /
noise_aead_dev_transport_rekey, include/noise_aead_hip.h section 12) on top of
tests/transport_model.py.

REKEY(k) through the oracle's encrypt at nonce 2^64 - 1, as the Noise
specification writes it; the same function from single blocks, as the kernels
compute it; a session's rekey (keys replaced, nonces and window left alone);
and the entry rule of a call over a table.  tests/test_transport_rekey_host.py
holds the two forms of REKEY against each other and against the known answers;
tests/test_gpu_transport_rekey.py compares the device with this model."""
import transport_model as T

SEND, RECEIVE = 1, 2
REKEY_NONCE = 2 ** 64 - 1


def rekey(orc, cipher, key: bytes) -> bytes:
    """REKEY(k): the first 32 bytes of ENCRYPT(k, 2^64 - 1, "", 32 zero bytes)"""
    assert len(key) == 32
    return orc.encrypt(cipher, bytes(key), REKEY_NONCE, bytes(32))[:32]


def rekey_blocks(orc, cipher, key: bytes) -> bytes:
    """REKEY(k) block by block: ChaChaPoly, bytes 0..31 of the block under
    counter 1 and IV 2^64 - 1; AES-GCM, the CTR blocks 2 and 3 under
    J0 = 0^32 || BE64(2^64 - 1) || 00000001"""
    if cipher == T.CHACHAPOLY:
        return orc.chacha20_block(bytes(key), 1, REKEY_NONCE)[:32]
    assert cipher == T.AESGCM
    return b"".join(orc.aes256(bytes(key), bytes(4) + b"\xff" * 8 + c.to_bytes(4, "big")) for c in (2, 3))


def rekey_times(orc, cipher, key: bytes, times: int) -> bytes:
    for _ in range(times):
        key = rekey(orc, cipher, key)
    return key


def rekey_session(session, directions: int):
    """CipherState.Rekey() of the chosen directions of a T.Session: the key is
    replaced; the nonces (and a datagram window) stay as they are"""
    assert 0 <= directions <= 3
    if directions & SEND:
        session.send_key = rekey(session.orc, session.cipher, session.send_key)
    if directions & RECEIVE:
        session.recv_key = rekey(session.orc, session.cipher, session.recv_key)
    return session


def entry_directions(directions: int, which, j: int) -> int:
    """the directions a call rekeys for entry j: `which` is the call's bytes, or None"""
    return directions & (3 if which is None else which[j])


def rekey_table(sessions, directions: int, m: int, slots=None, which=None):
    """One call over entries 0 .. m - 1 of a table: sessions[i] is the
    T.Session of slot i, None for an unkeyed one.  Entry j is slot slots[j]
    (slot j without a list); an entry out of range or unkeyed is ignored.
    Returns the (slot, direction bit) pairs it rekeyed."""
    assert 1 <= directions <= 3
    done = []
    for j in range(m):
        i = j if slots is None else slots[j]
        if not 0 <= i < len(sessions) or sessions[i] is None:
            continue
        d = entry_directions(directions, which, j)
        rekey_session(sessions[i], d)
        done += [(i, bit) for bit in (SEND, RECEIVE) if d & bit]
    assert len(set(done)) == len(done), "the listed slots must be distinct"
    return done
