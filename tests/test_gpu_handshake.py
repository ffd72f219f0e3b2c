"""Batched Noise handshakes on the device: noise_aead_dev_handshake_*.

A device initiator batch talks to a device responder batch, message by
message; every byte either side writes is compared with the model of
tests/handshake_model.py (proved against the recorded vectors by
tests/test_handshake_model_host.py), and session 0 of every batch carries a
recorded vector of tests/golden/vectors/noise-c-basic.txt.gz whose bytes are
compared directly.  n = 67: one full workgroup plus three lanes.  Every device
buffer is laid out at an odd stride from an odd address between 0xEE canaries
that must read back untouched."""
import functools

import numpy as np
import pytest

import handshake_model as M
from handshake_gpu import CANARY, Buf, Side, basic_vector, handshake, make_sessions, model_pair

pytestmark = pytest.mark.gpu
N = 67


@functools.lru_cache(maxsize=None)
def basic_vectors():
    by_pattern = {}
    for v in M.load_vectors("noise-c-basic.txt.gz"):
        if M.in_scope(v):
            by_pattern.setdefault(v["pattern"], []).append(v)
    assert set(by_pattern) == set(M.PATTERNS) and all(len(x) == 16 for x in by_pattern.values())
    return by_pattern


def check_against_model_and_vector(A, torch, orc, v, r, n):
    assert r["ini_status"] == [0] * n and r["res_status"] == [0] * n
    assert r["ini_split"] == r["res_split"]
    k1, k2, hh = r["ini_split"]
    for i, (mi, mr) in enumerate(r["models"]):
        assert (k1[i], k2[i], hh[i]) == mi.split() == mr.split(), (v["name"], "split", i)
    # session 0 is the recorded vector
    for j in range(r["n_handshake"]):
        assert r["msgs"][j][0].hex() == v["messages"][j]["ciphertext"], (v["name"], j)
    assert hh[0].hex() == v["handshake_hash"], v["name"]
    # the vector's transport messages under the device's split keys: prepare + seal_uniform
    cipher = r["models"][0][0].cid
    sp = torch.cuda.current_stream().cuda_stream
    ctx = [torch.empty(n * A.dev_ctx_bytes(cipher), dtype=torch.uint8, device="cuda") for _ in range(2)]
    for c, keys in zip(ctx, (r["ini"].k1, r["ini"].k2)):
        assert A.dev_prepare(cipher, keys.data_ptr(), n, c.data_ptr(), sp) == 0
    nonce = [0, 0]
    pattern = v["pattern"]
    for t, m in enumerate(v["messages"][r["n_handshake"]:]):
        d = 0 if M.one_way(pattern) else (r["n_handshake"] + t) % 2
        pt = bytes.fromhex(m["payload"])
        L = len(pt)
        src = Buf(torch, n, max(L, 1), [pt or b"\0"] * n)
        dst = Buf(torch, n, L + 16)
        nb = torch.full((n,), nonce[d], dtype=torch.int64, device="cuda")
        assert A.dev_uniform(False, cipher, ctx=ctx[d].data_ptr(), nonce_base=nb.data_ptr(), inp=src.ptr, out=dst.ptr,
                             in_stride=src.stride, out_stride=dst.stride, length=L, n_records=n, recs_per_state=1,
                             stream=sp) == 0
        torch.cuda.synchronize()
        rows = dst.read()
        assert rows[0].hex() == m["ciphertext"], (v["name"], "transport", t)
        for i in {min(1, n - 1), n - 1}:
            assert rows[i] == orc.encrypt(cipher, (k1, k2)[d][i], nonce[d], pt), (v["name"], "transport", t, i)
        nonce[d] += 1


@pytest.mark.parametrize("pattern", list(M.PATTERNS))
def test_vectors_and_model_per_pattern(aead, gpu, oracle, pattern):
    """The pattern's 16 protocol names of noise-c-basic (2 prefixes x 2
    ciphers x 4 hashes), n = 67 each; the first name again with the
    responder's static key and the prologue at stride 0, and with n = 1."""
    import torch
    vs = basic_vectors()[pattern]
    seed = sorted(M.PATTERNS).index(pattern) + 1
    for v in vs:
        sess = make_sessions(v, N, seed)
        r = handshake(aead, torch, oracle, v, sess, seed=seed)
        check_against_model_and_vector(aead, torch, oracle, v, r, N)
        if "init_static" in v:  # the initiator's static key reached the responder (pre-message or `s` token)
            assert r["res"].remote_static() == [M.dh_base(s["ini_s"]) for s in sess]
        r["ini"].free()
        r["res"].free()
    v = vs[0]
    for n, shared in ((N, True), (1, False)):
        sess = make_sessions(v, n, seed, shared)
        r = handshake(aead, torch, oracle, v, sess, shared=shared, seed=seed)
        check_against_model_and_vector(aead, torch, oracle, v, r, n)
        r["ini"].free()
        r["res"].free()


@pytest.mark.parametrize("name", ["Noise_XX_25519_ChaChaPoly_BLAKE2s", "Noise_XX_25519_AESGCM_SHA256",
                                  "Noise_IK_25519_ChaChaPoly_SHA512", "NoisePSK_IK_25519_AESGCM_BLAKE2b"])
def test_failed_sessions_do_not_touch_the_others(aead, gpu, oracle, name):
    """What the responder reads is changed in flight: the ephemeral of
    session 66 zeroed (message 0), one tag bit of the `s` record of session 5
    and one of the payload tag of session 64 flipped (XX: message 2, IK:
    message 0).  Statuses 1, 1 and 3, sticky; zero split keys; nothing written
    to the failed sessions' payload slots from the failure on; every other
    session's every byte as in the untampered run."""
    import torch
    v = basic_vector(name)
    sess = make_sessions(v, N, 99)
    clean = handshake(aead, torch, oracle, v, sess, seed=99)
    assert clean["res_status"] == [0] * N
    s_msg = 2 if "_XX_" in name else 0  # the message whose `s` the responder opens
    seen = []

    def tamper(j, rows):
        rows = [bytearray(r) for r in rows]
        if j == 0:
            rows[66][:32] = bytes(32)
        if j == s_msg:
            at = 0 if s_msg == 2 else 32  # XX message 2: s first; IK message 0: e, then s
            rows[5][at + 32 + 7] ^= 0x10      # a bit of the 16-byte tag after the 32-byte key
            rows[64][-3] ^= 0x01              # a bit of the payload's tag
        seen.append(j)
        return [bytes(r) for r in rows] if j in (0, s_msg) else None
    bad = handshake(aead, torch, oracle, v, sess, tamper=tamper, seed=99)
    failed = {5: 1, 64: 1, 66: 3}
    assert bad["res_status"] == [failed.get(i, 0) for i in range(N)]
    k1, k2, hh = bad["res_split"]
    for i in range(N):
        if i in failed:
            assert k1[i] == bytes(32) and k2[i] == bytes(32), i
        else:
            assert (k1[i], k2[i], hh[i]) == tuple(x[i] for x in clean["res_split"]), i
    responder_reads = [j for j in range(bad["n_handshake"]) if j % 2 == 0]
    for j in range(bad["n_handshake"]):
        for i in range(N):
            if i not in failed:
                assert bad["msgs"][j][i] == clean["msgs"][j][i], (j, i)
                assert bad["payloads"][j][i] == clean["payloads"][j][i], (j, i)
    for j in responder_reads:
        plen = len(clean["payloads"][j][0])
        for i, since in ((66, 0), (5, s_msg), (64, s_msg)):
            if j >= since:
                assert bad["payloads"][j][i] == bytes([CANARY]) * plen, (j, i)
    assert sorted(seen) == list(range(bad["n_handshake"])), "every message went through tamper()"
    for r in (clean, bad):
        r["ini"].free()
        r["res"].free()


def test_null_ephemeral_status_is_sticky_from_the_first_message(aead, gpu, oracle):
    """XX: the zeroed ephemeral of message 0 gives status 3 at once, and the
    two later messages leave it."""
    import torch
    v = basic_vector("Noise_XX_25519_ChaChaPoly_SHA256")
    sess = make_sessions(v, 3, 5)
    ini, res = Side(aead, torch, v, sess, True), Side(aead, torch, v, sess, False)
    pay, msg = Buf(torch, 3, 4, [b"abcd"] * 3), Buf(torch, 3, 36)
    assert ini.write(pay, 4, msg) == 0
    rows = msg.read()
    rows[1] = bytes(32) + rows[1][32:]
    got = Buf(torch, 3, 4)
    assert res.read(Buf(torch, 3, 36, rows), 36, got) == 0
    assert res.status() == [0, 3, 0]
    assert got.read() == [b"abcd", bytes([CANARY]) * 4, b"abcd"]
    msg2 = Buf(torch, 3, 4 + res.overhead)
    assert res.write(pay, 4, msg2) == 0
    assert res.status() == [0, 3, 0]
    ini.free()
    res.free()


@pytest.mark.parametrize("first_long", [True, False])
def test_length_edges(aead, gpu, oracle, first_long):
    """NN, n = 2: an empty payload and the payload that makes a message
    exactly 65535 bytes, on the unkeyed message 0 (overhead 32) and on the
    keyed message 1 (overhead 48); one byte more is refused, and so is a
    read of overhead - 1 bytes; a refused call leaves the state as it was."""
    import torch
    A = aead
    v = basic_vector("Noise_NN_25519_ChaChaPoly_BLAKE2s")
    sess = make_sessions(v, 2, 11)
    ini, res = Side(A, torch, v, sess, True), Side(A, torch, v, sess, False)
    models = [model_pair(oracle, v, s) for s in sess]
    rng = np.random.default_rng(12)
    for j, (w, r) in enumerate(((ini, res), (res, ini))):
        over = w.overhead
        assert over == (32, 48)[j] == r.overhead
        plen = 65535 - over if (j == 0) == first_long else 0
        rows = [rng.integers(0, 256, max(plen, 1), dtype=np.uint8).tobytes()[:plen] for _ in range(2)]
        payload = Buf(torch, 2, max(plen, 1), [p or b"\0" for p in rows])
        msg = Buf(torch, 2, plen + over)
        if plen:
            big = Buf(torch, 2, plen + over + 1)
            assert A.dev_handshake_write_message(w.hs, payload=payload.ptr, payload_stride=payload.stride,
                                                 payload_len=plen + 1, msg=big.ptr, msg_stride=big.stride,
                                                 stream=w.sp) == A.ERROR_INVALID_LENGTH
        assert w.action == A.ACTION_WRITE_MESSAGE
        assert w.write(payload, plen, msg) == 0
        sent = msg.read()
        got = Buf(torch, 2, max(plen, 1))
        assert A.dev_handshake_read_message(r.hs, msg=msg.ptr, msg_stride=msg.stride, msg_len=over - 1, payload=got.ptr,
                                            payload_stride=got.stride, stream=r.sp) == A.ERROR_INVALID_LENGTH
        assert A.dev_handshake_read_message(r.hs, msg=msg.ptr, msg_stride=msg.stride, msg_len=65536, payload=got.ptr,
                                            payload_stride=got.stride, stream=r.sp) == A.ERROR_INVALID_LENGTH
        assert r.action == A.ACTION_READ_MESSAGE
        assert r.read(msg, plen + over, got) == 0
        back = got.read()
        for i, pair in enumerate(models):
            mw, mr = pair if j == 0 else pair[::-1]
            assert sent[i] == mw.write(rows[i]), (j, i)
            assert mr.read(sent[i]) == rows[i]
            assert back[i][:plen] == rows[i], (j, i)
            if not plen:
                assert back[i] == bytes([CANARY])
    ki, kr = ini.split(), res.split()
    assert ki == kr and ini.status() == res.status() == [0, 0]
    for i, (mi, _) in enumerate(models):
        assert (ki[0][i], ki[1][i], ki[2][i]) == mi.split()
    ini.free()
    res.free()


def test_host_rules(aead, gpu):
    """Everything the host refuses before a launch."""
    import torch
    A = aead
    key = Buf(torch, 4, 32, [bytes([i]) * 32 for i in range(4)])
    sp = torch.cuda.current_stream().cuda_stream
    I, R = A.ROLE_INITIATOR, A.ROLE_RESPONDER
    # names
    assert A.dev_handshake_new("Noise_XX_448_ChaChaPoly_SHA256", I, 4)[0] == A.ERROR_NOT_APPLICABLE
    assert A.dev_handshake_new("Noise_XXfallback_25519_AESGCM_SHA256", I, 4)[0] == A.ERROR_NOT_APPLICABLE
    assert A.dev_handshake_new("Noise_XY_25519_AESGCM_SHA256", I, 4)[0] == A.ERROR_UNKNOWN_NAME
    assert A.dev_handshake_new("Noise_XX_25519_AESGCM_SHA256", 7, 4, local_static=key.ptr,
                               local_ephemeral=key.ptr)[0] == A.ERROR_INVALID_PARAM
    # each missing key
    assert A.dev_handshake_new("Noise_XX_25519_AESGCM_SHA256", I, 4, local_ephemeral=key.ptr)[0] \
        == A.ERROR_LOCAL_KEY_REQUIRED
    assert A.dev_handshake_new("Noise_XX_25519_AESGCM_SHA256", I, 4, local_static=key.ptr)[0] \
        == A.ERROR_LOCAL_KEY_REQUIRED
    assert A.dev_handshake_new("Noise_NK_25519_AESGCM_SHA256", I, 4, local_ephemeral=key.ptr)[0] \
        == A.ERROR_REMOTE_KEY_REQUIRED
    assert A.dev_handshake_new("Noise_KN_25519_AESGCM_SHA256", R, 4, local_ephemeral=key.ptr)[0] \
        == A.ERROR_REMOTE_KEY_REQUIRED
    assert A.dev_handshake_new("NoisePSK_NN_25519_AESGCM_SHA256", I, 4, local_ephemeral=key.ptr)[0] \
        == A.ERROR_PSK_REQUIRED
    # strides in 1..31, a prologue without a pointer
    assert A.dev_handshake_new("Noise_NN_25519_AESGCM_SHA256", I, 4, local_ephemeral=key.ptr,
                               local_ephemeral_stride=31)[0] == A.ERROR_INVALID_PARAM
    assert A.dev_handshake_new("Noise_NN_25519_AESGCM_SHA256", I, 4, local_ephemeral=key.ptr,
                               prologue_len=3)[0] == A.ERROR_INVALID_PARAM
    # the wrong call for the action, bad strides, spans that meet
    rc, hs = A.dev_handshake_new("Noise_NN_25519_ChaChaPoly_SHA256", I, 4, local_ephemeral=key.ptr,
                                 local_ephemeral_stride=key.stride, stream=sp)
    assert rc == 0 and A.dev_handshake_get_action(hs) == A.ACTION_WRITE_MESSAGE
    assert A.dev_handshake_overhead(hs) == 32
    room = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = room.data_ptr()
    assert A.dev_handshake_read_message(hs, msg=p, msg_stride=64, msg_len=40, payload=p + 2048,
                                        payload_stride=8) == A.ERROR_INVALID_STATE
    assert A.dev_handshake_split(hs, k1=p, k2=p + 512) == A.ERROR_INVALID_STATE
    w = dict(payload=p, payload_stride=8, payload_len=8)
    assert A.dev_handshake_write_message(hs, msg=0, msg_stride=40, **w) == A.ERROR_INVALID_PARAM
    assert A.dev_handshake_write_message(hs, msg=p + 2048, msg_stride=39, **w) == A.ERROR_INVALID_PARAM
    assert A.dev_handshake_write_message(hs, msg=p + 2048, msg_stride=40, payload=0, payload_stride=8,
                                         payload_len=8) == A.ERROR_INVALID_PARAM
    assert A.dev_handshake_write_message(hs, msg=p + 2048, msg_stride=40, payload=p, payload_stride=7,
                                         payload_len=8) == A.ERROR_INVALID_PARAM
    assert A.dev_handshake_write_message(hs, msg=p + 31, msg_stride=40, **w) == A.ERROR_INVALID_PARAM  # meets byte 31
    assert A.dev_handshake_write_message(hs, msg=p + 32, msg_stride=40, stream=sp, **w) == 0  # touches, does not meet
    assert A.dev_handshake_get_action(hs) == A.ACTION_READ_MESSAGE
    assert A.dev_handshake_write_message(hs, msg=p + 2048, msg_stride=40, **w) == A.ERROR_INVALID_STATE
    # a read whose payload slots meet the message; then free a half-finished handshake
    assert A.dev_handshake_read_message(hs, msg=p, msg_stride=64, msg_len=56, payload=p + 3 * 64 + 55,
                                        payload_stride=8) == A.ERROR_INVALID_PARAM
    assert A.dev_handshake_read_message(hs, msg=p, msg_stride=64, msg_len=56, payload=p + 2048,
                                        payload_stride=7) == A.ERROR_INVALID_PARAM
    assert A.dev_handshake_free(hs) == 0
    assert A.dev_handshake_free(0) == A.ERROR_INVALID_PARAM
    torch.cuda.synchronize()


def test_an_empty_batch_launches_nothing(aead, gpu):
    """n = 0: a valid object; its calls check the state and the lengths,
    take NULL pointers, and walk the actions."""
    A = aead
    rc, hs = A.dev_handshake_new("Noise_NN_25519_AESGCM_SHA512", A.ROLE_RESPONDER, 0, local_ephemeral=8)
    assert rc == 0 and hs
    assert A.dev_handshake_status(hs) == 0
    assert A.dev_handshake_write_message(hs, msg=0, msg_stride=0) == A.ERROR_INVALID_STATE
    assert A.dev_handshake_read_message(hs, msg=0, msg_stride=0, msg_len=31) == A.ERROR_INVALID_LENGTH
    assert A.dev_handshake_read_message(hs, msg=0, msg_stride=0, msg_len=32) == 0
    assert A.dev_handshake_overhead(hs) == 48
    assert A.dev_handshake_write_message(hs, msg=0, msg_stride=0, payload_len=65535 - 47) == A.ERROR_INVALID_LENGTH
    assert A.dev_handshake_write_message(hs, msg=0, msg_stride=0, payload_len=65535 - 48) == 0
    assert A.dev_handshake_get_action(hs) == A.ACTION_SPLIT
    assert A.dev_handshake_split(hs, k1=0, k2=0) == 0
    assert A.dev_handshake_get_action(hs) == A.ACTION_COMPLETE and A.dev_handshake_overhead(hs) == 0
    assert A.dev_handshake_split(hs, k1=0, k2=0) == A.ERROR_INVALID_STATE
    assert A.dev_handshake_free(hs) == 0


def test_split_outputs_must_not_meet(aead, gpu):
    import torch
    A = aead
    v = basic_vector("Noise_N_25519_ChaChaPoly_BLAKE2s")
    sess = make_sessions(v, 2, 3)
    res = Side(A, torch, v, sess, False)
    ini = Side(A, torch, v, sess, True)
    msg = Buf(torch, 2, 48)
    assert ini.write(Buf(torch, 2, 1), 0, msg) == 0
    assert res.read(msg, 48, Buf(torch, 2, 1)) == 0
    room = torch.zeros(512, dtype=torch.uint8, device="cuda")
    p = room.data_ptr()
    assert A.dev_handshake_split(res.hs, k1=p, k2=p + 63) == A.ERROR_INVALID_PARAM
    assert A.dev_handshake_split(res.hs, k1=p, k2=p + 64, handshake_hash=p + 127) == A.ERROR_INVALID_PARAM
    assert A.dev_handshake_split(res.hs, k1=0, k2=p + 64) == A.ERROR_INVALID_PARAM
    assert res.action == A.ACTION_SPLIT
    assert A.dev_handshake_split(res.hs, k1=p, k2=p + 64, handshake_hash=p + 128, stream=res.sp) == 0
    torch.cuda.synchronize()
    ini.free()
    res.free()
