"""Batched handshakes with per-session offsets and lengths:
noise_aead_dev_handshake_write_message_ragged / _read_message_ragged.

A device initiator batch talks to a device responder batch through the ragged
calls; every byte, every out length, every status and every split output of
every session is compared with the model of tests/handshake_ragged_model.py
(proved against the reference's own bytes and return codes by
tests/test_handshake_ragged_host.py).  n = 67 unless stated.  Every buffer
starts at an odd address, the sessions' spans lie in a scrambled order — the
session order is not the wire order — at any alignment, with 0xEE canaries
between and around them that must read back untouched; the out-length arrays
lie between canary words."""
import functools
import json
import os

import numpy as np
import pytest

import handshake_model as M
import handshake_ragged_model as R
from gpu_support import peek
from handshake_gpu import CANARY, Buf, Side, basic_vector, make_sessions, model_pair

pytestmark = pytest.mark.gpu
N = 67
WORD = 0xEEEEEEEE
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handshake_lengths.json")


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


LENGTHS = fixture()["lengths"]


class Spans:
    """n spans, span i of widths[i] bytes, in a canary-filled tensor from its
    byte 1: in a scrambled order with gaps of 1..5 bytes, or (stride given)
    at i * stride."""

    def __init__(self, torch, widths, rows=None, seed=0, stride=None):
        self.torch, self.widths, n = torch, list(widths), len(widths)
        if stride is None:
            off, pos = [0] * n, 2
            for k in np.random.default_rng(1000 + seed).permutation(n):
                off[k] = pos
                pos += self.widths[k] + 1 + int(k) % 5
        else:
            assert stride >= max(self.widths)
            off, pos = [i * stride for i in range(n)], (n - 1) * stride + max(self.widths)
        host = np.full(1 + pos + 9, CANARY, dtype=np.uint8)
        if rows is not None:
            for i in range(n):
                assert len(rows[i]) == self.widths[i]
                host[1 + off[i]: 1 + off[i] + self.widths[i]] = np.frombuffer(rows[i], dtype=np.uint8)
        self.offsets = off
        self.dev = torch.from_numpy(host).cuda()
        self.ptr = self.dev.data_ptr() + 1
        self.off = torch.from_numpy(np.array(off, dtype=np.uint64).view(np.int64)).cuda()

    def read(self):
        """the spans; checks every byte between and around them"""
        h = self.dev.cpu().numpy()
        mask = np.ones(len(h), dtype=bool)
        rows = []
        for o, w in zip(self.offsets, self.widths):
            rows.append(h[1 + o: 1 + o + w].tobytes())
            mask[1 + o: 1 + o + w] = False
        assert (h[mask] == CANARY).all(), "wrote outside a span"
        return rows


class Lens:
    """n uint32 on the device between two canary words"""

    def __init__(self, torch, n, values=None):
        host = np.full(n + 2, WORD, dtype=np.uint32)
        if values is not None:
            host[1:n + 1] = np.array(values, dtype=np.uint32)
        self.dev = torch.from_numpy(host.view(np.int32)).cuda()
        self.ptr = self.dev.data_ptr() + 4

    def read(self):
        h = self.dev.cpu().numpy().view(np.uint32)
        assert h[0] == WORD and h[-1] == WORD, "wrote outside a length array"
        return [int(x) for x in h[1:-1]]


def rand_bytes(rng, n):
    return rng.integers(0, 256, max(n, 1), dtype=np.uint8).tobytes()[:n]


def blank(width):
    return bytes([CANARY]) * width


def write_ragged(A, side, pay: Spans, plens, msg: Spans, out: Lens):
    d_len = Lens(side.torch, len(plens), plens)
    rc = A.dev_handshake_write_message_ragged(side.hs, payload=pay.ptr, payload_off=pay.off.data_ptr(),
                                              payload_len=d_len.ptr, msg=msg.ptr, msg_off=msg.off.data_ptr(),
                                              msg_len=out.ptr, stream=side.sp)
    side.torch.cuda.synchronize()
    assert d_len.read() == list(plens), "the input lengths are read only"
    return rc


def read_ragged(A, side, msg: Spans, mlens, pay: Spans, out: Lens):
    d_len = Lens(side.torch, len(mlens), mlens)
    rc = A.dev_handshake_read_message_ragged(side.hs, msg=msg.ptr, msg_off=msg.off.data_ptr(), msg_len=d_len.ptr,
                                             payload=pay.ptr, payload_off=pay.off.data_ptr(), payload_len=out.ptr,
                                             stream=side.sp)
    side.torch.cuda.synchronize()
    assert d_len.read() == list(mlens), "the input lengths are read only"
    return rc


def exchange(A, torch, v, sess, payloads_of, deliver=None, kinds=None, seed=0, stride_of=None):
    """Both device sides through the whole handshake.  payloads_of(j, over):
    message j's payload per session.  deliver(j, rows): what the reader is
    handed instead of what was sent (rows of any length).  kinds[j]: "ragged"
    (default) or "uniform" (equal lengths).  stride_of(width): the ragged
    calls' spans at i * stride instead of scrambled.  Returns per message what
    was asked, written, reported, delivered and read back, and both sides'
    split rows and statuses."""
    n = len(sess)
    ini, res = Side(A, torch, v, sess, True), Side(A, torch, v, sess, False)
    out = dict(ini=ini, res=res, steps=[])
    j = 0
    while ini.action != A.ACTION_SPLIT:
        w, r = (ini, res) if ini.action == A.ACTION_WRITE_MESSAGE else (res, ini)
        assert r.action == A.ACTION_READ_MESSAGE and w.overhead == r.overhead
        over = w.overhead
        rows = payloads_of(j, over)
        plens = [len(p) for p in rows]
        kind = kinds[j] if kinds else "ragged"
        if kind == "uniform":
            plen = plens[0]
            assert plens == [plen] * n
            pay, msg = Buf(torch, n, max(plen, 1), [p or b"\0" for p in rows]), Buf(torch, n, plen + over)
            assert w.write(pay, plen, msg) == 0
            sent, sent_lens = msg.read(), [plen + over] * n
        else:
            # a refused session gets an 8-byte slot nothing may be written to
            widths = [p + over if p + over <= R.MAX_MESSAGE else 8 for p in plens]
            stride = stride_of(max(widths)) if stride_of else None
            pay = Spans(torch, plens, rows, seed=seed + 2 * j, stride=stride_of(max(plens + [1])) if stride_of else None)
            msg, lens = Spans(torch, widths, seed=seed + 2 * j + 1, stride=stride), Lens(torch, n)
            assert write_ragged(A, w, pay, plens, msg, lens) == 0
            sent, sent_lens = msg.read(), lens.read()
            assert pay.read() == rows, "the payloads are read only"
        assert w.action != A.ACTION_WRITE_MESSAGE, "the action advances for the batch"
        # what travels: the bytes the writer reported
        wire = [s[:l] if l else b"" for s, l in zip(sent, sent_lens)]
        given = deliver(j, list(wire)) if deliver else wire
        mlens = [len(m) for m in given]
        if kind == "uniform":
            mlen = mlens[0]
            assert mlens == [mlen] * n
            got = Buf(torch, n, max(mlen - over, 1))
            assert r.read(Buf(torch, n, mlen, given), mlen, got) == 0
            back, back_lens = [g[:mlen - over] for g in got.read()], [mlen - over] * n
            slots = back
        else:
            widths = [m - over if over <= m <= R.MAX_MESSAGE else 8 for m in mlens]
            stride = stride_of(max(widths + [1])) if stride_of else None
            src = Spans(torch, mlens, given, seed=seed + 2 * j + 50, stride=stride_of(max(mlens)) if stride_of else None)
            got, lens = Spans(torch, widths, seed=seed + 2 * j + 51, stride=stride), Lens(torch, n)
            assert read_ragged(A, r, src, mlens, got, lens) == 0
            slots, back_lens = got.read(), lens.read()
            assert src.read() == given, "the messages are read only"
            back = [s[:l] for s, l in zip(slots, back_lens)]
        out["steps"].append(dict(writer=w, over=over, asked=rows, sent=sent, sent_lens=sent_lens, given=given, back=back,
                                 back_lens=back_lens, slots=slots))
        j += 1
    assert res.action == A.ACTION_SPLIT
    out["ini_split"], out["res_split"] = ini.split(), res.split()
    out["ini_status"], out["res_status"] = ini.status(), res.status()
    return out


def ragged_models(orc, v, sess):
    """model_pair's sessions with the length rule"""
    pairs = [model_pair(orc, v, s) for s in sess]
    for pair in pairs:
        for m in pair:
            m.__class__ = R.RaggedSession
    return pairs


def check_against_model(orc, v, sess, r, uniform=()):
    """every session of every message, the statuses and the split outputs"""
    models = ragged_models(orc, v, sess)
    for j, st in enumerate(r["steps"]):
        wi = 0 if st["writer"] is r["ini"] else 1
        for i, pair in enumerate(models):
            mw, mr = pair[wi], pair[1 - wi]
            where = (v["name"], "message", j, "session", i)
            want = mw.write(st["asked"][i])
            if want is None:
                assert st["sent_lens"][i] == 0 and st["sent"][i] == blank(len(st["sent"][i])), where
            else:
                assert st["sent_lens"][i] == len(want) and st["sent"][i] == want, where
            pay = mr.read(st["given"][i])
            if pay is None:
                assert st["back_lens"][i] == 0, where
                if j not in uniform:
                    assert st["slots"][i] == blank(len(st["slots"][i])), where
            else:
                assert st["back_lens"][i] == len(pay) and st["back"][i] == pay, where
                assert st["slots"][i][len(pay):] == blank(len(st["slots"][i]) - len(pay)), where
    for side, split, status in ((0, r["ini_split"], r["ini_status"]), (1, r["res_split"], r["res_status"])):
        for i, pair in enumerate(models):
            assert status[i] == pair[side].status, (v["name"], "status", side, i)
            assert (split[0][i], split[1][i], split[2][i]) == pair[side].split(), (v["name"], "split", side, i)
    return models


def free(r):
    r["ini"].free()
    r["res"].free()


def rotated_payloads(n, seed, first=None):
    """session i's payload of message j has LENGTHS[(i + j) % 17] bytes;
    session 0 carries `first` (a fixture case's payloads) when given"""
    def of(j, over):
        rng = np.random.default_rng(seed * 131 + j)
        rows = [rand_bytes(rng, LENGTHS[(i + j) % len(LENGTHS)]) for i in range(n)]
        if first:
            rows[0] = first[j]
        return rows
    return of


# ---------------------------------------------------------------- 1. ragged equals uniform

@pytest.mark.parametrize("name", ["Noise_XX_25519_ChaChaPoly_BLAKE2s", "NoisePSK_IK_25519_AESGCM_SHA512"])
def test_ragged_equals_uniform(aead, gpu, oracle, name):
    """The same keys once through the uniform calls and once through the ragged
    calls with off[i] = i * stride and equal lengths: every message, payload,
    out length, status and split output byte for byte."""
    import torch
    v = basic_vector(name)
    sess = make_sessions(v, N, 21)
    n_msgs = len(M.PATTERNS[v["pattern"]][2])

    def payloads(j, over):
        rng = np.random.default_rng(2100 + j)
        return [rand_bytes(rng, (37, 0, 64)[j]) for _ in range(N)]
    uni = exchange(aead, torch, v, sess, payloads, kinds=["uniform"] * n_msgs)
    rag = exchange(aead, torch, v, sess, payloads, stride_of=lambda width: width + 5)
    assert len(uni["steps"]) == len(rag["steps"]) == n_msgs
    for a, b in zip(uni["steps"], rag["steps"]):
        assert a["sent"] == b["sent"] and a["back"] == b["back"] == a["asked"]
        assert b["sent_lens"] == a["sent_lens"] == [len(p) + a["over"] for p in a["asked"]]
        assert b["back_lens"] == a["back_lens"] == [len(p) for p in a["asked"]]
    for key in ("ini_split", "res_split", "ini_status", "res_status"):
        assert uni[key] == rag[key], key
    assert rag["ini_status"] == rag["res_status"] == [0] * N
    check_against_model(oracle, v, sess, rag)
    free(uni)
    free(rag)


# ---------------------------------------------------------------- 2. per-session lengths against the model

PREFIXES, CIPHERS, HASHES = ("Noise", "NoisePSK"), ("ChaChaPoly", "AESGCM"), ("BLAKE2s", "SHA512", "SHA256", "BLAKE2b")
FIXTURE_PATTERNS = {"NN": "Noise", "XX": "Noise", "IK": "NoisePSK", "N": "Noise"}


def names_of(pattern):
    """One name per pattern, rotated over prefix, cipher and hash; the
    fixture's patterns run under the fixture's names: both suites."""
    if pattern in FIXTURE_PATTERNS:
        return [f"{FIXTURE_PATTERNS[pattern]}_{pattern}_25519_{s}" for s in ("ChaChaPoly_BLAKE2s", "AESGCM_SHA512")]
    k = list(M.PATTERNS).index(pattern)
    return [f"{PREFIXES[k % 2]}_{pattern}_25519_{CIPHERS[(k // 2) % 2]}_{HASHES[k % 4]}"]


def test_the_rotation_covers_both_ciphers_all_hashes_both_prefixes():
    names = [n for p in M.PATTERNS for n in names_of(p)]
    fields = [n.split("_") for n in names]
    assert {f[1] for f in fields} == set(M.PATTERNS)
    assert {f[0] for f in fields} == set(PREFIXES) and {f[3] for f in fields} == set(CIPHERS)
    assert {f[4] for f in fields} == set(HASHES)
    assert {c["name"] for c in fixture()["cases"]} <= set(names)


@pytest.mark.parametrize("pattern", list(M.PATTERNS))
def test_per_session_lengths_against_the_model(aead, gpu, oracle, pattern):
    """Session i's payload of message j has LENGTHS[(i + j) % 17] bytes: 0 next
    to 257 in one wave, and the 64- and 128-byte block edges of h || data for
    both hash lengths.  The fixture's cases run as session 0 of batches under
    their names, with their own keys and lengths, and must give the
    reference's recorded bytes."""
    import torch
    for name in names_of(pattern):
        cases = [c for c in fixture()["cases"] if c["name"] == name] or [None]
        for k, case in enumerate(cases):
            v = case or basic_vector(name)
            seed = 300 + list(M.PATTERNS).index(pattern) + 40 * k
            sess = make_sessions(v, N, seed)
            first = [bytes.fromhex(m["payload"]) for m in case["messages"]] if case else None
            r = exchange(aead, torch, v, sess, rotated_payloads(N, seed, first), seed=seed)
            assert r["ini_status"] == r["res_status"] == [0] * N
            assert r["ini_split"] == r["res_split"]
            check_against_model(oracle, v, sess, r)
            for j, st in enumerate(r["steps"]):
                assert st["back"] == st["asked"]
                if case:
                    assert st["sent"][0].hex() == case["messages"][j]["ciphertext"], (name, j)
                else:
                    assert sorted({len(p) for p in st["asked"]}) == LENGTHS
            if case:
                k1, k2, hh = r["res_split"]
                assert (k1[0].hex(), k2[0].hex(), hh[0].hex()) == (case["k1"], case["k2"], case["handshake_hash"]), name
            free(r)


# ---------------------------------------------------------------- 3. length faults are per session

@pytest.mark.parametrize("name", ["Noise_NN_25519_ChaChaPoly_BLAKE2s", "Noise_XX_25519_ChaChaPoly_BLAKE2s"])
def test_length_faults_are_per_session(aead, gpu, oracle, name):
    """In the responder's read of message 0: messages of 0, overhead - 1 and
    65536 bytes (status 4), of exactly the overhead (an empty payload) and of
    65535 bytes (the largest; both status 0).  In the responder's write of
    message 1: payloads of 65535 - overhead + 1 bytes (status 4) and of
    65535 - overhead (status 0).  A refused session's slots stay untouched,
    its out length is 0, it is inert in the later messages, its 4 is sticky
    and its split keys are zeros; every other session matches, byte for byte,
    a run of the same batch with ordinary lengths in those places."""
    import torch
    v = basic_vector(name)
    sess = make_sessions(v, N, 31)
    EMPTY, SHORT, LONG, EXACT, LARGEST, W_OVER, W_MAX = 3, 17, 40, 41, 63, 64, 66
    read_faults, write_faults = {EMPTY, SHORT, LONG}, {W_OVER}

    def payloads(faults):
        def of(j, over):
            rows = rotated_payloads(N, 31)(j, over)
            rng = np.random.default_rng(3100 + j)
            if j == 0:
                rows[EXACT], rows[LARGEST] = b"", rand_bytes(rng, 65535 - over)
            if j == 1:
                rows[W_MAX] = rand_bytes(rng, 65535 - over)
                if faults:
                    rows[W_OVER] = rand_bytes(rng, 65535 - over + 1)
            return rows
        return of

    def deliver(j, rows):
        if j == 0:
            over = 32
            rows[EMPTY], rows[SHORT] = b"", rows[SHORT][:over - 1]
            rows[LONG] = rows[LONG] + bytes(65536 - len(rows[LONG]))
        return rows
    bad = exchange(aead, torch, v, sess, payloads(True), deliver=deliver, seed=31)
    clean = exchange(aead, torch, v, sess, payloads(False), seed=31)
    assert clean["ini_status"] == clean["res_status"] == [0] * N
    # the responder refuses the three reads and the one write; the initiator
    # is then handed nothing for those four sessions in message 1 and refuses that
    failed = read_faults | write_faults
    assert bad["res_status"] == [4 if i in failed else 0 for i in range(N)]
    assert bad["ini_status"] == [4 if i in failed else 0 for i in range(N)]
    check_against_model(oracle, v, sess, bad)
    check_against_model(oracle, v, sess, clean)
    first = bad["steps"][0]
    assert first["over"] == 32 and [len(m) for i, m in enumerate(first["given"]) if i in (EMPTY, SHORT, LONG, EXACT, LARGEST)] \
        == [0, 31, 65536, 32, 65535]
    assert first["back_lens"][EXACT] == 0 and first["back_lens"][LARGEST] == 65535 - 32
    second = bad["steps"][1]
    assert len(second["asked"][W_OVER]) + second["over"] == 65536 and second["sent_lens"][W_MAX] == 65535
    for st in bad["steps"][1:]:  # inert from the fault on, both ways
        for i in failed:
            assert st["sent_lens"][i] == 0 == st["back_lens"][i]
            assert st["sent"][i] == blank(len(st["sent"][i])) and st["slots"][i] == blank(len(st["slots"][i]))
    for i in read_faults:
        assert first["back_lens"][i] == 0 and first["slots"][i] == blank(8)
    for side in ("ini_split", "res_split"):
        for i in range(N):
            if i in failed:
                assert bad[side][0][i] == bytes(32) == bad[side][1][i], (side, i)
            else:
                assert [x[i] for x in bad[side]] == [x[i] for x in clean[side]], (side, i)
    for a, b in zip(bad["steps"], clean["steps"]):
        for i in range(N):
            if i not in failed:
                assert (a["sent"][i], a["sent_lens"][i], a["back"][i], a["back_lens"][i]) == \
                    (b["sent"][i], b["sent_lens"][i], b["back"][i], b["back_lens"][i]), i
    free(bad)
    free(clean)


# ---------------------------------------------------------------- 4. order of causes

def test_order_of_causes(aead, gpu, oracle):
    """NoisePSK_XX (message 0 is `e` and a sealed payload).  In the
    responder's one read of message 0: a session both short and tampered gets
    4, a tampered one 1, an all-zero `e` 3.  No pattern has a second read
    with an `e` in it, so the fourth rule takes the responder's next read,
    message 2: the sessions that already have 1, 3 and 4 are handed short
    messages there and keep what they have, and a fresh short one gets 4."""
    import torch
    v = basic_vector("NoisePSK_XX_25519_ChaChaPoly_SHA256")
    sess = make_sessions(v, N, 41)
    BOTH, TAMPERED, NULL_E, LATE = 2, 33, 64, 65

    def deliver(j, rows):
        if j == 0:
            t = bytearray(rows[BOTH][:47])  # overhead 48: one byte short, and a flipped bit
            t[40] ^= 0x04
            rows[BOTH] = bytes(t)
            t = bytearray(rows[TAMPERED])
            t[-1] ^= 0x80
            rows[TAMPERED] = bytes(t)
            rows[NULL_E] = bytes(32) + rows[NULL_E][32:]
        if j == 2:
            for i in (BOTH, TAMPERED, NULL_E, LATE):
                rows[i] = bytes(5)
        return rows
    r = exchange(aead, torch, v, sess, rotated_payloads(N, 41), deliver=deliver, seed=41)
    assert r["steps"][0]["over"] == 48
    want = {BOTH: 4, TAMPERED: 1, NULL_E: 3, LATE: 4}
    assert r["res_status"] == [want.get(i, 0) for i in range(N)]
    check_against_model(oracle, v, sess, r)
    free(r)
    # the statuses right after message 0, before anything later could change them
    ini, res = Side(aead, torch, v, sess, True), Side(aead, torch, v, sess, False)
    rows = rotated_payloads(N, 41)(0, 48)
    plens = [len(p) for p in rows]
    msg, lens = Spans(torch, [p + 48 for p in plens], seed=1), Lens(torch, N)
    assert write_ragged(aead, ini, Spans(torch, plens, rows, seed=2), plens, msg, lens) == 0
    given = deliver(0, msg.read())
    mlens = [len(m) for m in given]
    got, glens = Spans(torch, [max(m - 48, 0) or 8 for m in mlens], seed=3), Lens(torch, N)
    assert read_ragged(aead, res, Spans(torch, mlens, given, seed=4), mlens, got, glens) == 0
    assert res.status() == [{BOTH: 4, TAMPERED: 1, NULL_E: 3}.get(i, 0) for i in range(N)]
    out = glens.read()
    assert [out[i] for i in (BOTH, TAMPERED, NULL_E)] == [0, 0, 0] and out[LATE] == plens[LATE]
    ini.free()
    res.free()


# ---------------------------------------------------------------- 5. mixed calls

@pytest.mark.parametrize("kinds", [("uniform", "ragged", "uniform"), ("ragged", "uniform", "ragged")])
def test_uniform_and_ragged_calls_mix(aead, gpu, oracle, kinds):
    import torch
    v = basic_vector("Noise_XX_25519_AESGCM_BLAKE2b")
    sess = make_sessions(v, N, 51)

    def payloads(j, over):
        if kinds[j] == "uniform":
            rng = np.random.default_rng(5100 + j)
            return [rand_bytes(rng, 21) for _ in range(N)]
        return rotated_payloads(N, 51)(j, over)
    r = exchange(aead, torch, v, sess, payloads, kinds=kinds, seed=51)
    assert r["ini_status"] == r["res_status"] == [0] * N and r["ini_split"] == r["res_split"]
    check_against_model(oracle, v, sess, r, uniform={j for j in range(3) if kinds[j] == "uniform"})
    free(r)


# ---------------------------------------------------------------- 6. batch sizes

@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(aead, gpu, oracle, n):
    import torch
    v = basic_vector("Noise_NN_25519_ChaChaPoly_SHA256")
    sess = make_sessions(v, n, 60 + n)
    r = exchange(aead, torch, v, sess, rotated_payloads(n, 60 + n), seed=n)
    assert r["ini_status"] == r["res_status"] == [0] * n
    check_against_model(oracle, v, sess, r)
    free(r)


# ---------------------------------------------------------------- 7. host rules

def test_host_rules_through_the_library(aead, gpu):
    """The header's list line by line; a refused call leaves the action as
    it was; the all-NULL payload triple gives d_msg_len[i] = overhead."""
    import torch
    A = aead
    BAD, STATE = A.ERROR_INVALID_PARAM, A.ERROR_INVALID_STATE
    n = 4
    key = Buf(torch, n, 32, [bytes([i + 1]) * 32 for i in range(n)])
    sp = torch.cuda.current_stream().cuda_stream
    room = torch.full((8192,), CANARY, dtype=torch.uint8, device="cuda")
    p = room.data_ptr()
    offs = torch.tensor([i * 64 for i in range(n)], dtype=torch.int64, device="cuda")
    poffs = torch.tensor([4096 + i * 64 for i in range(n)], dtype=torch.int64, device="cuda")
    arr = torch.zeros(64, dtype=torch.int32, device="cuda")  # length arrays at arr, arr + 64, ...
    a = arr.data_ptr()
    good_w = dict(payload=p, payload_off=poffs.data_ptr(), payload_len=a, msg=p, msg_off=offs.data_ptr(), msg_len=a + 64)
    good_r = dict(msg=p, msg_off=offs.data_ptr(), msg_len=a + 64, payload=p, payload_off=poffs.data_ptr(),
                  payload_len=a + 128)
    W, Rd = A.dev_handshake_write_message_ragged, A.dev_handshake_read_message_ragged
    # 1. no object
    assert W(0, **good_w) == BAD and Rd(0, **good_r) == BAD
    rc, ini = A.dev_handshake_new("Noise_NN_25519_ChaChaPoly_SHA256", A.ROLE_INITIATOR, n, local_ephemeral=key.ptr,
                                  local_ephemeral_stride=key.stride, stream=sp)
    assert rc == 0
    rc, res = A.dev_handshake_new("Noise_NN_25519_ChaChaPoly_SHA256", A.ROLE_RESPONDER, n, local_ephemeral=key.ptr,
                                  local_ephemeral_stride=key.stride, stream=sp)
    assert rc == 0
    # 2. the wrong call for the action, before any pointer is looked at
    assert Rd(ini, **good_r) == STATE and W(res, **good_w) == STATE
    assert Rd(ini, msg=0, msg_off=0, msg_len=0, payload=0, payload_off=0, payload_len=0) == STATE
    # 4. NULL pointers; the payload triple of a write only all together
    for miss in ("msg", "msg_off", "msg_len"):
        assert W(ini, **{**good_w, miss: 0}) == BAD, miss
    for miss in (("payload",), ("payload_off",), ("payload_len",), ("payload", "payload_off"), ("payload_off", "payload_len"),
                 ("payload", "payload_len")):
        assert W(ini, **{**good_w, **{m: 0 for m in miss}}) == BAD, miss
    for miss in good_r:
        assert Rd(res, **{**good_r, miss: 0}) == BAD, miss
    # 5. the output lengths on an array the call reads: 4n = 16 and 8n = 32 bytes
    assert W(ini, **{**good_w, "msg_len": a + 12}) == BAD and W(ini, **{**good_w, "msg_len": a - 12}) == BAD
    assert W(ini, **{**good_w, "msg_len": offs.data_ptr() + 28}) == BAD
    assert W(ini, **{**good_w, "msg_len": poffs.data_ptr() - 12}) == BAD
    assert Rd(res, **{**good_r, "payload_len": a + 64 + 15}) == BAD
    assert Rd(res, **{**good_r, "payload_len": offs.data_ptr()}) == BAD
    assert Rd(res, **{**good_r, "payload_len": poffs.data_ptr() + 31}) == BAD
    # every refused call left the objects as they were
    assert A.dev_handshake_get_action(ini) == A.ACTION_WRITE_MESSAGE and A.dev_handshake_overhead(ini) == 32
    assert A.dev_handshake_get_action(res) == A.ACTION_READ_MESSAGE
    torch.cuda.synchronize()
    assert (room.cpu().numpy() == CANARY).all() and not arr.cpu().numpy().any(), "a refused call launches nothing"
    # arrays that touch are taken; the all-NULL payload triple: d_msg_len[i] = overhead
    out = Lens(torch, n)
    assert W(ini, msg=p, msg_off=offs.data_ptr(), msg_len=out.ptr, stream=sp) == 0
    assert out.read() == [32] * n and A.dev_handshake_get_action(ini) == A.ACTION_READ_MESSAGE
    assert W(ini, **good_w) == STATE
    got = Lens(torch, n)
    assert Rd(res, **{**good_r, "msg_len": out.ptr, "payload_len": got.ptr}, stream=sp) == 0
    assert got.read() == [0] * n and out.read() == [32] * n
    # message 1 the same way round: the keyed empty payload, overhead 48
    assert A.dev_handshake_overhead(res) == 48
    assert W(res, msg=p + 1024, msg_off=offs.data_ptr(), msg_len=out.ptr, stream=sp) == 0
    assert out.read() == [48] * n
    assert Rd(ini, **{**good_r, "msg": p + 1024, "msg_len": out.ptr, "payload_len": got.ptr}, stream=sp) == 0
    assert got.read() == [0] * n
    assert peek(A.dev_handshake_status(ini), n) == bytes(n) == peek(A.dev_handshake_status(res), n)
    assert A.dev_handshake_get_action(ini) == A.dev_handshake_get_action(res) == A.ACTION_SPLIT
    assert W(ini, **good_w) == STATE and Rd(res, **good_r) == STATE
    h = room.cpu().numpy()
    assert (h[4096:] == CANARY).all(), "an empty payload writes nothing"
    assert A.dev_handshake_free(ini) == 0 and A.dev_handshake_free(res) == 0


def test_an_empty_batch_walks_the_actions(aead, gpu):
    """n == 0: after the state, nothing else is looked at and nothing is launched"""
    A = aead
    rc, hs = A.dev_handshake_new("Noise_NN_25519_AESGCM_SHA512", A.ROLE_RESPONDER, 0, local_ephemeral=8)
    assert rc == 0 and hs
    none_r = dict(msg=0, msg_off=0, msg_len=0, payload=0, payload_off=0, payload_len=0)
    assert A.dev_handshake_write_message_ragged(hs, msg=0, msg_off=0, msg_len=0) == A.ERROR_INVALID_STATE
    assert A.dev_handshake_read_message_ragged(hs, **none_r) == 0
    assert A.dev_handshake_get_action(hs) == A.ACTION_WRITE_MESSAGE and A.dev_handshake_overhead(hs) == 48
    assert A.dev_handshake_read_message_ragged(hs, **none_r) == A.ERROR_INVALID_STATE
    assert A.dev_handshake_write_message_ragged(hs, payload=8, msg=0, msg_off=0, msg_len=0) == 0  # not even the triple
    assert A.dev_handshake_get_action(hs) == A.ACTION_SPLIT
    assert A.dev_handshake_split(hs, k1=0, k2=0) == 0
    assert A.dev_handshake_free(hs) == 0


# ---------------------------------------------------------------- 8. into the table

def test_a_refused_session_never_becomes_a_transport_session(aead, gpu, oracle):
    """A ragged XX batch with one status-4 session, _split, then _set_keys
    with the handshake's own status array: that slot stays unkeyed."""
    import torch
    A = aead
    v = basic_vector("Noise_XX_25519_ChaChaPoly_BLAKE2s")
    sess = make_sessions(v, N, 81)
    REFUSED = 29

    def deliver(j, rows):
        if j == 1:
            rows[REFUSED] = rows[REFUSED][:95]  # overhead 96
        return rows
    r = exchange(A, torch, v, sess, rotated_payloads(N, 81), deliver=deliver, seed=81)
    assert r["steps"][1]["over"] == 96
    assert r["ini_status"] == [4 if i == REFUSED else 0 for i in range(N)]
    ini = r["ini"]
    rc, tr = A.dev_transport_new_unkeyed(A.CHACHAPOLY, A.ROLE_INITIATOR, N, max_frames=64, stream=ini.sp)
    assert rc == 0
    slots = torch.arange(N, dtype=torch.int32, device="cuda")
    assert A.dev_transport_set_keys(tr, slots=slots.data_ptr(), m=N, k1=ini.k1.data_ptr(), k2=ini.k2.data_ptr(),
                                    status=A.dev_handshake_status(ini.hs), stream=ini.sp) == 0
    assert list(peek(A.dev_transport_has_key(tr), N)) == [0 if i == REFUSED else 1 for i in range(N)]
    assert A.dev_transport_free(tr) == 0
    free(r)
