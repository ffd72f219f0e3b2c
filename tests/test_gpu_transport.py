"""Device-resident transport sessions: noise_aead_dev_transport_*.

Every call is compared with the model of tests/transport_model.py (proved
against the reference by tests/test_transport_model_host.py): every byte of
the wire, every result, both nonce arrays.  n = 67 sessions: one wave plus a
partial one.  The streams lie in one device buffer at odd, even and 16-byte
aligned offsets with unequal gaps, between 0xEE canaries that must read back
untouched; frame counts cycle through 0..5 and lengths through
{16, 17, 80, 1416, 65535}."""
import numpy as np
import pytest

import transport_model as T
from handshake_gpu import basic_vector, handshake, make_sessions
from transport_gpu import CIPHERS, LENS, N, Side, Wire, keys_for, plain_streams, total_frames

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("initiator", [True, False], ids=["initiator", "responder"])
@pytest.mark.parametrize("cipher", CIPHERS, ids=["ChaChaPoly", "AESGCM"])
def test_seal_equals_the_model_and_the_peer_opens_it(aead, gpu, oracle, cipher, initiator):
    import torch
    keys, plain = keys_for(1), plain_streams(1)
    lens = {L for s in plain for _, L in T.walk(s, 0)[0]}
    assert lens == set(LENS) and [len(T.walk(s, 0)[0]) for s in plain[:7]] == [0, 1, 2, 3, 4, 5, 0]
    assert any(T.walk(s, 0)[1] == len(s) > 0 for s in plain) and any(T.walk(s, 0)[1] == len(s) - 1 for s in plain)
    m = total_frames(plain)
    a = Side(aead, torch, oracle, cipher, initiator, keys, m)
    b = Side(aead, torch, oracle, cipher, not initiator, keys, m + 3)
    wire = Wire(torch, plain)
    sealed, results, _ = a.run("seal", wire)
    assert [r[0] for r in results] == [i % 6 for i in range(N)] and all(r[2] == 0 for r in results)
    assert a.nonces(0) == [i % 6 for i in range(N)] and a.nonces(1) == [0] * N
    opened, results, _ = b.run("open", wire)
    assert all(r[2] == 0 for r in results) and b.nonces(1) == [i % 6 for i in range(N)] and b.nonces(0) == [0] * N
    for i in range(N):  # the plaintext is back, each tag left as it was
        for at, L in T.walk(plain[i], 0)[0]:
            assert opened[i][at:at + L - 16] == plain[i][at:at + L - 16] and opened[i][at + L - 16:at + L] == sealed[i][at + L - 16:at + L]
    # a second tick on the same objects: the nonces carry over
    wire2 = Wire(torch, plain_streams(2, big=False))
    a.run("seal", wire2)
    b.run("open", wire2)
    assert a.nonces(0) == b.nonces(1) == [2 * (i % 6) for i in range(N)]
    a.free()
    b.free()


@pytest.mark.parametrize("cipher", CIPHERS, ids=["ChaChaPoly", "AESGCM"])
def test_stop_cases_among_clean_sessions(aead, gpu, oracle, cipher):
    """A partial frame, an L < 16 frame and an exhausted nonce (written
    through _nonces), each in a few sessions."""
    import torch
    keys, plain = keys_for(3), plain_streams(3, big=False)
    stops = {}
    for i in (4, 22, 64):  # the last frame short by one byte, by its body, and down to its header
        s = plain[i]
        at, L = T.walk(s, 0)[0][-1]
        plain[i] = s[:at - 2 + {4: 2 + L - 1, 22: 2 + 3, 64: 2}[i]]
        stops[i] = (i % 6 - 1, at - 2, 0)
    for i, tail in ((5, T.frame(bytes(15))), (23, T.frame(b"")), (65, T.frame(bytes(3)) + T.frame(bytes(40)))):
        at = T.walk(plain[i], 0)[1]
        plain[i] = plain[i][:at] + tail
        stops[i] = (i % 6, at, T.ERROR_INVALID_LENGTH)
    a = Side(aead, torch, oracle, cipher, True, keys, total_frames(plain) + 1)
    b = Side(aead, torch, oracle, cipher, False, keys, total_frames(plain) + 1)
    edge = {9: T.NONCE_LIMIT - 2, 10: T.NONCE_LIMIT, 66: T.NONCE_LIMIT - 1, 11: T.NONCE_LIMIT - 5, 16: 2 ** 32 - 1}
    for i, v in edge.items():
        frames = T.walk(plain[i], 0)[0]
        took = min(len(frames), T.NONCE_LIMIT - v)
        stops[i] = (took, frames[took][0] - 2 if took < len(frames) else T.walk(plain[i], 0)[1],
                    T.ERROR_INVALID_NONCE if took < len(frames) else 0)
    assert stops[9] == (2, stops[9][1], T.ERROR_INVALID_NONCE) and stops[10] == (0, 0, T.ERROR_INVALID_NONCE)
    assert stops[66] == (0, 0, 0) and stops[11][2] == 0  # session 66 has no frame: nothing to refuse
    a.set_nonces(0, edge)
    b.set_nonces(1, edge)
    wire = Wire(torch, plain)
    _, results, _ = a.run("seal", wire)
    for i, want in stops.items():
        assert results[i] == want, i
    assert sum(1 for r in results if r[2]) == 5
    _, results, _ = b.run("open", wire)
    for i, want in stops.items():
        assert results[i] == want, i
    assert b.nonces(1)[9] == T.NONCE_LIMIT and b.nonces(1)[16] == 2 ** 32 - 1 + 4
    a.free()
    b.free()


@pytest.mark.parametrize("cipher", CIPHERS, ids=["ChaChaPoly", "AESGCM"])
def test_forgeries_stop_their_session_alone(aead, gpu, oracle, cipher):
    """One flipped tag bit and one flipped body bit, in the first, a middle
    and the last frame of six sessions of five frames."""
    import torch
    keys, plain = keys_for(4), plain_streams(4)
    m = total_frames(plain)
    a, b = Side(aead, torch, oracle, cipher, True, keys, m), Side(aead, torch, oracle, cipher, False, keys, m)
    wire = Wire(torch, plain)
    sealed, _, _ = a.run("seal", wire)
    forged = {5: (0, "tag"), 11: (2, "tag"), 17: (4, "tag"), 23: (0, "body"), 29: (3, "body"), 65: (4, "body")}
    streams = [bytearray(s) for s in sealed]
    for i, (k, where) in forged.items():
        at, L = T.walk(sealed[i], 0)[0][k]
        streams[i][at + (L - 16 + 9 if where == "tag" else (L - 16) // 2)] ^= 0x04
    wire = Wire(torch, [bytes(s) for s in streams])
    got, results, want = b.run("open", wire, exact=False)
    recv = b.nonces(1)
    for i in range(N):
        if i not in forged:
            assert got[i] == want[i][0] and results[i][2] == 0, i  # byte for byte unaffected
            continue
        k = forged[i][0]
        frames = T.walk(sealed[i], 0)[0]
        assert results[i] == (k, frames[k][0] - 2, T.ERROR_MAC_FAILURE) and recv[i] == k
        end = frames[k][0] + frames[k][1]
        assert got[i][:end] == want[i][0][:end], i  # the verified prefix opened, the failed frame untouched
        assert got[i][frames[k][0] - 2:end] == bytes(streams[i][frames[k][0] - 2:end])
        later = want[i][2]
        assert sorted(later) == [f[0] for f in frames[k + 1:]]
        for at, L in frames[k + 1:]:  # as given, or the plaintext its own tag vouches for
            assert got[i][at - 2:at] == sealed[i][at - 2:at] and got[i][at:at + L] in later[at], (i, at)
        assert got[i][end:] == want[i][0][end:] or k < 4
    # the true frames arrive: each session goes on from its failed frame's nonce
    for i, (k, _) in forged.items():
        wire.pos[i] = results[i][1]
    for i in range(N):
        if i not in forged:
            wire.pos[i] = wire.lens[i]
    host = wire.dev.cpu().numpy()
    for i in forged:
        host[wire.offs[i] + wire.pos[i]:wire.offs[i] + wire.lens[i]] = np.frombuffer(sealed[i][wire.pos[i]:], dtype=np.uint8)
    wire.dev = torch.from_numpy(host).cuda()
    _, results, _ = b.run("open", wire)
    assert b.nonces(1) == [i % 6 for i in range(N)]
    final = wire.streams()
    for i in forged:
        for at, L in T.walk(plain[i], 0)[0]:
            assert final[i][at:at + L - 16] == plain[i][at:at + L - 16]
    a.free()
    b.free()


@pytest.mark.parametrize("which", ["total", "total-1", "one", "larger"])
@pytest.mark.parametrize("cipher", CIPHERS, ids=["ChaChaPoly", "AESGCM"])
def test_cap_continues_to_the_uncapped_result(aead, gpu, oracle, cipher, which):
    import torch
    n = 9 if which == "one" else N
    keys, plain = keys_for(5, n), plain_streams(5, n, big=False)
    plain[7] = plain[7] + T.frame(bytes(4))  # a stop that must survive the cuts
    total = total_frames(plain)
    cap = {"total": total, "total-1": total - 1, "one": 1, "larger": total + 7}[which]
    whole = T.run_batch([T.Session.of_role(oracle, cipher, True, *k) for k in keys], "seal", plain, total)
    a = Side(aead, torch, oracle, cipher, True, keys, cap)
    wire = Wire(torch, plain)
    calls, results = 0, None
    while True:
        _, results, _ = a.run("seal", wire)
        calls += 1
        if which == "total-1" and calls == 1:  # the cut lies inside the last session that has frames
            cutting = max(i for i in range(n) if i % 6)
            assert results[cutting][0] == cutting % 6 - 1 and results[cutting][2] == 0
        for i, r in enumerate(results):
            wire.pos[i] += r[1]
        if sum(r[0] for r in results) == 0:
            break
    assert calls == -(-total // cap) + 1
    assert wire.streams() == [w[0] for w in whole]
    assert wire.pos == [w[1][1] for w in whole] and [r[2] for r in results] == [w[1][2] for w in whole]
    assert results[7][2] == T.ERROR_INVALID_LENGTH and a.nonces(0) == [w[1][0] for w in whole]
    # and an open under the same cap, from the start
    b = Side(aead, torch, oracle, cipher, False, keys, cap)
    wire.pos = [0] * n
    while True:
        _, results, _ = b.run("open", wire)
        for i, r in enumerate(results):
            wire.pos[i] += r[1]
        if sum(r[0] for r in results) == 0:
            break
    opened = wire.streams()
    for i in range(n):
        for at, L in T.walk(plain[i], 0)[0]:
            assert opened[i][at:at + L - 16] == plain[i][at:at + L - 16]
    a.free()
    b.free()


@pytest.mark.parametrize("cipher", CIPHERS, ids=["ChaChaPoly", "AESGCM"])
def test_echo_is_open_then_seal_of_the_prefix(aead, gpu, oracle, cipher):
    import torch
    keys, plain = keys_for(6), plain_streams(6)
    m = total_frames(plain)
    client = Side(aead, torch, oracle, cipher, True, keys, m)
    server = Side(aead, torch, oracle, cipher, False, keys, m + 2)
    server.set_nonces(0, {i: 1000 + i for i in range(N)})  # the two directions count apart
    server.set_nonces(0, {14: T.NONCE_LIMIT - 1})          # and one send state runs out after a frame
    wire = Wire(torch, plain)
    sealed, _, _ = client.run("seal", wire)
    streams = [bytearray(s) for s in sealed]
    at, L = T.walk(sealed[29], 0)[0][2]
    streams[29][at + 1] ^= 0x80
    wire = Wire(torch, [bytes(s) for s in streams])
    got, results, want = server.run("echo", wire, exact=False)
    for i in range(N):
        if i != 29:
            assert got[i] == want[i][0], i
    assert results[29] == (2, at - 2, T.ERROR_MAC_FAILURE) and results[14] == (1, results[14][1], T.ERROR_INVALID_NONCE)
    assert server.nonces(1)[29] == 2 and server.nonces(0)[29] == 1000 + 29 + 2 and server.nonces(0)[14] == T.NONCE_LIMIT
    assert got[29][:at + L] == want[29][0][:at + L]  # the prefix echoed, the failed frame untouched
    for fa, fl in T.walk(sealed[29], 0)[0][3:]:      # later frames: as given or opened, never sealed again
        assert got[29][fa:fa + fl] in want[29][2][fa]
    # the client opens what came back: the prefix of every session, under the server's send nonces
    client.set_nonces(1, {i: 1000 + i for i in range(N)})
    client.set_nonces(1, {14: T.NONCE_LIMIT - 1})
    back = [g[:r[1]] for g, r in zip(got, results)]
    wire = Wire(torch, back)
    opened, results2, _ = client.run("open", wire)
    assert [r[0] for r in results2] == [r[0] for r in results] and all(r[2] == 0 for r in results2)
    for i in range(N):
        for fa, fl in T.walk(back[i], 0)[0]:
            assert opened[i][fa:fa + fl - 16] == plain[i][fa:fa + fl - 16]
    client.free()
    server.free()


@pytest.mark.parametrize("name", ["Noise_XX_25519_ChaChaPoly_BLAKE2s", "Noise_NK_25519_AESGCM_SHA256"])
def test_handshake_split_feeds_the_transport(aead, gpu, oracle, name):
    """Both roles through noise_aead_dev_handshake_* to the split; a transport
    object on each side straight from the split's device arrays; traffic both
    ways."""
    import torch
    n = 9
    v = basic_vector(name)
    sess = make_sessions(v, n, 7)
    r = handshake(aead, torch, oracle, v, sess, seed=7)
    assert r["ini_status"] == [0] * n and r["ini_split"][:2] == r["res_split"][:2]
    k1, k2, _ = r["ini_split"]
    keys = list(zip(k1, k2))
    cipher = r["models"][0][0].cid
    plain = plain_streams(8, n, big=False)
    m = total_frames(plain)
    ini = Side(aead, torch, oracle, cipher, True, keys, m, r["ini"].k1.data_ptr(), r["ini"].k2.data_ptr())
    res = Side(aead, torch, oracle, cipher, False, keys, m, r["res"].k1.data_ptr(), r["res"].k2.data_ptr())
    for w, rd in ((ini, res), (res, ini), (ini, res)):
        wire = Wire(torch, plain)
        w.run("seal", wire)
        opened, results, _ = rd.run("open", wire)
        assert [x[0] for x in results] == [i % 6 for i in range(n)] and all(x[2] == 0 for x in results)
        for i in range(n):
            for at, L in T.walk(plain[i], 0)[0]:
                assert opened[i][at:at + L - 16] == plain[i][at:at + L - 16]
    for side in (ini, res, r["ini"], r["res"]):
        side.free()


def test_free_mid_stream_and_the_empty_object(aead, gpu, oracle):
    import torch
    A = aead
    keys, plain = keys_for(9), plain_streams(9, big=False)
    a = Side(A, torch, oracle, T.AESGCM, True, keys, 64)
    wire = Wire(torch, plain)
    sp = torch.cuda.current_stream().cuda_stream
    off = torch.tensor(wire.offs, dtype=torch.int64, device="cuda")
    ln = torch.tensor(wire.lens, dtype=torch.int32, device="cuda")
    ok = dict(wire=wire.dev.data_ptr(), off=off.data_ptr(), length=ln.data_ptr(), result=wire.result.data_ptr(), stream=sp)
    # the ranges the host can see: the result array may touch the offsets and the lengths, not meet them
    for k, width in (("off", 8), ("length", 4)):
        for d in (0, width * N - 1, -16 * N + 1):
            assert A.dev_transport_seal_frames(a.tr, **{**ok, "result": ok[k] + d}) == A.ERROR_INVALID_PARAM
            assert A.dev_transport_echo_frames(a.tr, **{**ok, "result": ok[k] + d}) == A.ERROR_INVALID_PARAM
    for k in ("wire", "off", "length", "result"):
        assert A.dev_transport_open_frames(a.tr, **{**ok, k: 0}) == A.ERROR_INVALID_PARAM
    torch.cuda.synchronize()
    assert a.nonces(0) == [0] * N and wire.streams() == plain  # nothing was launched
    # calls in flight, then free: it waits, scrubs and frees
    for _ in range(3):
        assert A.dev_transport_seal_frames(a.tr, **ok) == 0
    assert A.dev_transport_free(a.tr) == A.ERROR_NONE
    torch.cuda.synchronize()
    wire.streams()
    # n == 0: a valid object whose calls launch nothing
    for cipher in CIPHERS:
        rc, tr = A.dev_transport_new(cipher, A.ROLE_RESPONDER, 0, k1=a.k1.data_ptr(), k2=a.k2.data_ptr(), max_frames=0, stream=sp)
        assert rc == 0 and tr
        for fn in (A.dev_transport_seal_frames, A.dev_transport_open_frames, A.dev_transport_echo_frames):
            assert fn(tr, **ok) == A.ERROR_NONE
        assert A.dev_transport_nonces(tr, 0) == 0 and A.dev_transport_free(tr) == A.ERROR_NONE
    torch.cuda.synchronize()
    assert wire.streams()[1] != plain[1] and (wire.result.cpu().numpy()[N] == 0x55555555).all()
