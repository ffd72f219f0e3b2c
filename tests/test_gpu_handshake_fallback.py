"""The Noise Pipes fallback on the device: noise_aead_dev_handshake_fallback
and _fallback_merge (include/noise_aead_hip.h section 15) against the model of
tests/handshake_fallback_model.py — which tests/test_handshake_fallback_host.py
proves against the recorded vectors and the reference's own fallback — byte
for byte: every message, every payload, the handshake hash, the split keys and
every status byte of both objects."""
import numpy as np
import pytest

import handshake_fallback_model as F
import handshake_model as M
import transport_model as T
from handshake_fallback_gpu import (exchange, fall_back, ik_side, merge, model_pair, model_split, model_status,
                                    random_sessions, split, vector_sessions)
from handshake_gpu import Buf
from transport_gpu import Table, Wire

pytestmark = pytest.mark.gpu
IK = "Noise_IK_25519_ChaChaPoly_BLAKE2s"


def rows_for(n, seed, length, first=None):
    rng = np.random.default_rng(seed)
    rows = [rng.integers(0, 256, max(length, 1), dtype=np.uint8).tobytes()[:length] for _ in range(n)]
    if first is not None:
        rows[0] = first
    return rows


def start(A, torch, orc, name, sess, shared=False, tamper=None):
    """both sides and their models after the original's first message"""
    ini, res = ik_side(A, torch, name, sess, True, shared), ik_side(A, torch, name, sess, False, shared)
    pairs = [model_pair(orc, name, s) for s in sess]
    mi, mr = [p[0] for p in pairs], [p[1] for p in pairs]
    assert ini.overhead == res.overhead == 96
    exchange(ini, res, mi, mr, rows_for(len(sess), 5, 16), tamper)
    assert ini.action == A.ACTION_READ_MESSAGE and res.action == A.ACTION_WRITE_MESSAGE
    return ini, res, mi, mr


def finish(w, r, mw, mrd, seed, tamper2=None):
    """the two fallback messages (w: fb's initiator), then both splits checked
    against the models; returns the device splits of (w, r)"""
    n = w.n
    A = w.A
    assert w.action == A.ACTION_WRITE_MESSAGE and r.action == A.ACTION_READ_MESSAGE
    assert w.overhead == 96
    exchange(w, r, mw, mrd, rows_for(n, seed, 15))
    assert r.overhead == 64
    exchange(r, w, mrd, mw, rows_for(n, seed + 1, 11), tamper2)
    assert w.action == r.action == A.ACTION_SPLIT
    out = []
    for side, models in ((w, mw), (r, mrd)):
        k1, k2, hh = split(side)
        assert side.action == A.ACTION_COMPLETE
        assert side.status() == model_status(models)
        for i, m in enumerate(models):
            want = model_split(m, side.hl)
            assert (k1[i], k2[i]) == want[:2], ("split keys of session", i)
            if m is not None and not m.status:
                assert hh[i] == want[2], ("handshake hash of session", i)
        out.append((k1, k2, hh))
    return out


VECTORS = F.fallback_vectors()


@pytest.mark.parametrize("v", VECTORS, ids=[v["name"] for v in VECTORS])
def test_fallback_vectors(aead, gpu, oracle, v):
    """Each of the 16 Curve25519 vectors of noise-c-fallback at n = 3: session
    0 holds the vector's keys.  The IK message fails at the responder, both
    sides fall back, and the two fallback messages, the handshake hash and the
    split keys equal the vector and the model."""
    import torch
    A, n = aead, 3
    name = F.original_name(v)
    sess = vector_sessions(v, n, 11)
    ini, res = ik_side(A, torch, name, sess, True), ik_side(A, torch, name, sess, False)
    pairs = [model_pair(oracle, name, s) for s in sess]
    mi, mr = [p[0] for p in pairs], [p[1] for p in pairs]
    msgs = v["messages"]
    sent = exchange(ini, res, mi, mr, rows_for(n, 1, 16, bytes.fromhex(msgs[0]["payload"])))
    assert sent[0].hex() == msgs[0]["ciphertext"]
    assert res.status() == [1] * n and ini.status() == [0] * n
    fr, mfr = fall_back(oracle, res, mr, sess)
    fi, mfi = fall_back(oracle, ini, mi, sess)
    assert res.status() == [1] * n and ini.status() == [5] * n and fr.status() == fi.status() == [0] * n
    assert fr.action == A.ACTION_WRITE_MESSAGE and fi.action == A.ACTION_READ_MESSAGE
    assert fr.overhead == fi.overhead == 96
    sent = exchange(fr, fi, mfr, mfi, rows_for(n, 2, 15, bytes.fromhex(msgs[1]["payload"])))
    assert sent[0].hex() == msgs[1]["ciphertext"]
    assert fr.overhead == fi.overhead == 64
    sent = exchange(fi, fr, mfi, mfr, rows_for(n, 3, 11, bytes.fromhex(msgs[2]["payload"])))
    assert sent[0].hex() == msgs[2]["ciphertext"]
    got = [split(fr), split(fi)]
    assert got[0] == got[1]
    assert fr.status() == fi.status() == [0] * n
    for i in range(n):
        assert (got[0][0][i], got[0][1][i], got[0][2][i]) == mfr[i].split() == mfi[i].split()
    assert got[0][2][0].hex() == v["handshake_hash"]
    # the transport messages of the vector: the fallback's initiator, the former responder, sends under k1
    ct = oracle.encrypt(mfr[0].cid, got[0][0][0], 0, bytes.fromhex(msgs[3]["payload"]))
    assert ct.hex() == msgs[3]["ciphertext"]
    ct = oracle.encrypt(mfr[0].cid, got[0][1][0], 0, bytes.fromhex(msgs[4]["payload"]))
    assert ct.hex() == msgs[4]["ciphertext"]
    for x in (ini, res, fr, fi):
        x.free()


@pytest.mark.parametrize("name,psk", [(IK, False), ("NoisePSK_IK_25519_AESGCM_SHA512", True)])
def test_mixed_batch(aead, gpu, oracle, name, psk):
    """n = 67: two 64-lane workgroups, the launch ending inside the second.  A
    stale static key at the sessions i % 3 == 0; the responder falls back with
    ONLY_FAILED, the initiator with the mask of the same sessions.  The
    others finish in hs, byte for byte as in a run with no fallback call; the
    stale ones finish in fb; the merge keys one table for all."""
    import torch
    A, n = aead, 67
    stale = [i % 3 == 0 for i in range(n)]
    sess = random_sessions(n, 21, stale=lambda i: stale[i], psk=psk, prologue=b"original", fb_prologue=b"fallback's")

    def second_and_split(ini, res, mi, mr):
        sent = exchange(res, ini, mr, mi, rows_for(n, 6, 9))
        return sent, split(ini), split(res)
    # the same run with no fallback call at all
    ini, res, mi, mr = start(A, torch, oracle, name, sess)
    plain_sent, plain_ini, plain_res = second_and_split(ini, res, mi, mr)
    assert res.status() == [int(s) for s in stale]
    ini.free()
    res.free()
    # and with it
    ini, res, mi, mr = start(A, torch, oracle, name, sess)
    assert res.status() == [int(s) for s in stale] and ini.status() == [0] * n
    fr, mfr = fall_back(oracle, res, mr, sess, flags=A.FALLBACK_ONLY_FAILED)
    fi, mfi = fall_back(oracle, ini, mi, sess, select=[int(s) for s in stale])
    assert res.status() == [1 if s else 0 for s in stale]
    assert ini.status() == [5 if s else 0 for s in stale]
    assert fr.status() == fi.status() == [0 if s else 5 for s in stale]
    sent, ini_split, res_split = second_and_split(ini, res, mi, mr)
    for i in range(n):
        if not stale[i]:
            assert sent[i] == plain_sent[i], ("the original's second message of session", i)
            assert [x[i] for x in ini_split] == [x[i] for x in plain_ini] == [x[i] for x in res_split], i
            assert ini_split[0][i] != bytes(32)
        else:
            assert ini_split[0][i] == ini_split[1][i] == res_split[0][i] == res_split[1][i] == bytes(32)
    assert res.status() == [1 if s else 0 for s in stale] and ini.status() == [5 if s else 0 for s in stale]
    fr_split, fi_split = finish(fr, fi, mfr, mfi, 30)
    assert fr.status() == fi.status() == [0 if s else 5 for s in stale]
    # the merge, on both ends, against the model's
    want = [F.merge(model_status(mfr)[i], model_split(mfr[i], res.hl), mr[i].status,
                    (res_split[0][i], res_split[1][i], res_split[2][i])) for i in range(n)]
    for hs_side, fb_side in ((res, fr), (ini, fi)):
        k1, k2, hh, st = merge(hs_side, fb_side)
        assert st == [0] * n
        for i in range(n):
            assert (k1[i], k2[i], hh[i]) == want[i][:3], ("merged session", i)
            if stale[i]:
                assert (k1[i], k2[i], hh[i]) == (fr_split[1][i], fr_split[0][i], fr_split[2][i])
    # one table per end, keyed on the device from the merged arrays; one echo tick
    cipher = T.AESGCM if "AESGCM" in name else T.CHACHAPOLY
    keys = [(w[0], w[1]) for w in want]
    tabs = []
    for hs_side, initiator in ((ini, True), (res, False)):
        tab = Table(A, torch, oracle, cipher, initiator, 8 * n)
        tab.set_keys(list(range(n)), keys, [0] * n,
                     ptrs=(hs_side.k1.data_ptr(), hs_side.k2.data_ptr(), hs_side.merged_status.data_ptr()))
        assert tab.has_key() == [1] * n
        tabs.append(tab)
    plain = [T.frame(bytes([i]) * 20 + bytes(16)) for i in range(n)]
    wire = Wire(torch, plain)
    assert tabs[0].run("seal", wire)[:2] == [(1, 38, 0)] * 2   # a stale session and a fresh one
    assert tabs[1].run("echo", wire)[:2] == [(1, 38, 0)] * 2
    assert tabs[0].run("open", wire)[:2] == [(1, 38, 0)] * 2
    assert wire.streams()[0][2:22] == bytes([0]) * 20 and wire.streams()[1][2:22] == bytes([1]) * 20
    for x in (ini, res, fr, fi, *tabs):
        x.free()


def test_select_and_the_eligible_set(aead, gpu, oracle):
    """Every first message verifies but two: session 1 arrives with an
    all-zero e (status 3 at the responder), session 2 is written and read
    through the ragged calls with a refused length (status 4 on both ends).
    The masks name them all the same; they stay out.  Session 4 verifies and
    is not selected: it stays in hs.  Sessions 0 and 3 verified and fall
    back: their status 0 becomes 5 in hs."""
    import torch
    A, n = aead, 5
    sess = random_sessions(n, 31)
    ini, res = ik_side(A, torch, IK, sess, True), ik_side(A, torch, IK, sess, False)
    pairs = [model_pair(oracle, IK, s) for s in sess]
    mi, mr = [p[0] for p in pairs], [p[1] for p in pairs]
    rows = rows_for(n, 32, 16)
    stride = 16 + 96 + 7
    payload, msg, got = Buf(torch, n, 16, rows), Buf(torch, n, 112, stride=stride), Buf(torch, n, 16)

    def u64(vals):
        return torch.tensor(vals, dtype=torch.int64, device="cuda")

    def u32(vals):
        return torch.tensor(vals, dtype=torch.int32, device="cuda")
    p_off, m_off, g_off = (u64([i * b.stride for i in range(n)]) for b in (payload, msg, got))
    p_len, m_len = u32([16, 16, 65535, 16, 16]), u32([0] * n)
    rc = A.dev_handshake_write_message_ragged(ini.hs, payload=payload.ptr, payload_off=p_off.data_ptr(),
                                              payload_len=p_len.data_ptr(), msg=msg.ptr, msg_off=m_off.data_ptr(),
                                              msg_len=m_len.data_ptr(), stream=ini.sp)
    assert rc == 0
    sent = msg.read()
    assert m_len.tolist() == [112, 112, 0, 112, 112] and ini.status() == [0, 0, 4, 0, 0]
    for i in (0, 1, 3, 4):
        assert sent[i] == mi[i].write(rows[i])
    mi[2].status, mi[2].index = F.STATUS_LENGTH, 1
    delivered = list(sent)
    delivered[1] = bytes(32) + sent[1][32:]
    msg = Buf(torch, n, 112, delivered, stride)
    in_len, out_len = u32([112, 112, 10, 112, 112]), u32([7] * n)
    rc = A.dev_handshake_read_message_ragged(res.hs, msg=msg.ptr, msg_off=m_off.data_ptr(), msg_len=in_len.data_ptr(),
                                             payload=got.ptr, payload_off=g_off.data_ptr(),
                                             payload_len=out_len.data_ptr(), stream=res.sp)
    assert rc == 0
    assert res.status() == [0, 3, 4, 0, 0] and out_len.tolist() == [16, 0, 0, 16, 16]
    for i in (0, 1, 3, 4):
        assert mr[i].read(delivered[i]) == (None if i == 1 else rows[i])
    mr[2].status, mr[2].index = F.STATUS_LENGTH, 1
    assert model_status(mr) == [0, 3, 4, 0, 0]
    fr, mfr = fall_back(oracle, res, mr, sess, select=[1, 1, 1, 1, 0])
    fi, mfi = fall_back(oracle, ini, mi, sess, select=[1, 0, 1, 1, 0])
    assert res.status() == model_status(mr) == [5, 3, 4, 5, 0]
    assert ini.status() == model_status(mi) == [5, 0, 4, 5, 0]
    assert fr.status() == fi.status() == model_status(mfr) == model_status(mfi) == [0, 5, 5, 0, 5]
    # session 4 finishes in hs, sessions 0 and 3 in fb
    exchange(res, ini, mr, mi, rows_for(n, 33, 9))
    k1, k2, hh = split(ini)
    assert (k1, k2) == split(res)[:2]
    assert (k1[4], k2[4], hh[4]) == mi[4].split() and k1[4] != bytes(32)
    assert [k1[i] for i in (0, 1, 2, 3)] == [bytes(32)] * 4
    assert ini.status() == [5, 1, 4, 5, 0] and res.status() == [5, 3, 4, 5, 0]
    finish(fr, fi, mfr, mfi, 40)
    for x in (ini, res, fr, fi):
        x.free()


def test_only_failed_without_failures(aead, gpu, oracle):
    """ONLY_FAILED and no failed session: fb has status 5 everywhere and its
    split writes zeros; hs is as it was."""
    import torch
    A, n = aead, 3
    sess = random_sessions(n, 41)
    ini, res, mi, mr = start(A, torch, oracle, IK, sess)
    fr, mfr = fall_back(oracle, res, mr, sess, flags=A.FALLBACK_ONLY_FAILED)
    assert mfr == [None] * n and fr.status() == [5] * n and res.status() == [0] * n
    room, back = Buf(torch, n, 96), Buf(torch, n, 64)
    assert fr.write(room, 0, room) == 0
    assert fr.read(back, 64, back) == 0
    k1, k2, hh = split(fr)
    assert k1 == k2 == [bytes(32)] * n and fr.status() == [5] * n
    room.read()  # nothing outside the slots
    # hs goes on
    exchange(res, ini, mr, mi, rows_for(n, 42, 4))
    assert split(ini)[:2] == split(res)[:2] and ini.status() == res.status() == [0] * n
    assert (ini.k1.cpu().numpy()[:32 * n] != 0).any()
    for x in (ini, res, fr):
        x.free()


def test_merge_overwrites_a_session_that_fails_in_the_fallback(aead, gpu, oracle):
    """All stale; the fallback's second message of session 1 is spoilt in
    flight, so session 1 fails inside fb at the former responder: the merge
    writes zeros over its keys and hash and gives fb's status."""
    import torch
    A, n = aead, 3
    sess = random_sessions(n, 51, stale=lambda i: True)
    ini, res, mi, mr = start(A, torch, oracle, IK, sess)
    fr, mfr = fall_back(oracle, res, mr, sess, flags=A.FALLBACK_ONLY_FAILED)
    fi, mfi = fall_back(oracle, ini, mi, sess)

    def spoil(rows):
        return [rows[0], rows[1][:-1] + bytes([rows[1][-1] ^ 0x80]), rows[2]]
    fr_split, fi_split = finish(fr, fi, mfr, mfi, 52, tamper2=spoil)
    assert fr.status() == [0, 1, 0] and fi.status() == [0, 0, 0]
    # hs's split as it lies: every session failed there, so zeros — marked, to see what the merge writes
    room = Buf(torch, n, 96)
    assert res.write(room, 0, room) == 0
    split(res)
    assert res.status() == [1, 1, 1]
    for t in (res.k1, res.k2, res.hh):
        t[:res.n * 32].fill_(0x77)
    k1, k2, hh, st = merge(res, fr)
    assert st == [0, 1, 0]
    for i in (0, 2):
        assert (k1[i], k2[i], hh[i]) == (fr_split[1][i], fr_split[0][i], fr_split[2][i])
        assert (k1[i], k2[i]) == (fi_split[1][i], fi_split[0][i]) and k1[i] != bytes(32)
    assert k1[1] == k2[1] == hh[1] == bytes(32)
    # an output that meets an array the call reads is refused before any launch
    ptrs = dict(hs_status=A.dev_handshake_status(res.hs), k1=res.k1.data_ptr(), k2=res.k2.data_ptr(),
                fb_k1=fr.k1.data_ptr(), fb_k2=fr.k2.data_ptr(), h=res.hh.data_ptr(), fb_h=fr.hh.data_ptr(),
                status=res.merged_status.data_ptr(), stream=res.sp)
    for change in (dict(k1=fr.k1.data_ptr() + 32 * n - 1), dict(k2=fr.k2.data_ptr()), dict(h=fr.hh.data_ptr() + 1),
                   dict(status=A.dev_handshake_status(res.hs) + n - 1), dict(status=A.dev_handshake_status(fr.hs)),
                   dict(status=fr.k2.data_ptr() + 5)):
        assert A.dev_handshake_fallback_merge(fr.hs, **{**ptrs, **change}) == A.ERROR_INVALID_PARAM, change
    assert A.dev_handshake_fallback_merge(fr.hs, **ptrs) == 0
    assert A.dev_handshake_fallback_merge(fi.hs, **{**ptrs, "k1": 0}) == A.ERROR_INVALID_PARAM
    torch.cuda.synchronize()
    for x in (ini, res, fr, fi):
        x.free()


def test_strides_and_the_free(aead, gpu, oracle):
    """One static key for the whole server and one prologue, of the original
    and of the fallback, at stride 0; hs is freed before fb is used; fb is
    freed half-way and after its split."""
    import torch
    A, n = aead, 67
    name = "NoisePSK_IK_25519_ChaChaPoly_SHA256"
    sess = random_sessions(n, 61, stale=lambda i: True, psk=True, prologue=b"one for all", fb_prologue=b"and one more", shared=True)
    ini, res, mi, mr = start(A, torch, oracle, name, sess, shared=True)
    assert res.status() == [1] * n
    fr, mfr = fall_back(oracle, res, mr, sess, shared=True)
    fi, mfi = fall_back(oracle, ini, mi, sess, shared=True)
    res.free()
    ini.free()
    finish(fr, fi, mfr, mfi, 62)
    assert fr.status() == fi.status() == [0] * n
    fr.free()
    fi.free()
    # a fallback object freed before its first message
    ini, res, mi, mr = start(A, torch, oracle, name, sess, shared=True)
    fr, _ = fall_back(oracle, res, mr, sess, shared=True)
    fr.free()
    assert A.dev_handshake_free(0) == A.ERROR_INVALID_PARAM
    ini.free()
    res.free()
