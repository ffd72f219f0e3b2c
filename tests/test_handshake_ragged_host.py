"""The per-session half of the ragged handshake calls without a GPU.

tests/handshake_ragged_model.py (handshake_model.Session plus the length rule
and status 4) is proved against tests/golden/handshake_lengths.json — the
reference's own write_message / read_message with a different payload length
in every message, and its return codes for messages cut short and buffers one
byte too small — and must equal Session on every in-scope recorded vector.

noise-c_amd/asan/handshake_ragged_check.cpp, a stand-alone program (`make -C
noise-c_amd handshake_ragged_check`: g++ -fsanitize=address,undefined
-fno-sanitize-recover=all) over csrc/handshake_plan.h, prints hs_session_len —
the source the kernels run — over every (overhead, length) pair and checks
hs_check_write_ragged / hs_check_read_ragged against a byte-by-byte reading of
the header's list.  It runs here once, as a plain child process."""
import functools
import json
import os

import handshake_model as M
import handshake_ragged_model as R
import host_check
from host_check import ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "handshake_lengths.json")
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 111, 112, 127, 128, 129, 257]


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def ragged_pair(orc, v):
    def hx(key):
        return bytes.fromhex(v[key]) if key in v else None
    return (R.RaggedSession(orc, v["name"], True, hx("init_prologue") or b"", hx("init_psk"), hx("init_static"),
                            hx("init_ephemeral"), hx("init_remote_static")),
            R.RaggedSession(orc, v["name"], False, hx("resp_prologue") or b"", hx("resp_psk"), hx("resp_static"),
                            hx("resp_ephemeral"), hx("resp_remote_static")))


def run_to(orc, v, upto):
    """the model's (writer, reader) of message `upto`, after the messages before it"""
    ini, res = ragged_pair(orc, v)
    for j in range(upto):
        w, r = (ini, res) if ini.action == M.ACTION_WRITE else (res, ini)
        payload = bytes.fromhex(v["messages"][j]["payload"])
        assert r.read(w.write(payload)) == payload
    return (ini, res) if ini.action == M.ACTION_WRITE else (res, ini)


def test_the_fixture_is_what_the_issue_asks_for():
    fx = fixture()
    assert fx["lengths"] == LENGTHS
    names = {c["name"] for c in fx["cases"]}
    assert names == {f"{p}_25519_{s}" for p in ("Noise_NN", "Noise_XX", "NoisePSK_IK", "Noise_N")
                     for s in ("ChaChaPoly_BLAKE2s", "AESGCM_SHA512")}
    used = [len(m["payload"]) // 2 for c in fx["cases"] for m in c["messages"]]
    assert set(used) == set(LENGTHS)
    for c in fx["cases"]:
        lens = [len(m["payload"]) for m in c["messages"]]
        assert len(set(lens)) == len(lens), "a different payload length in every message"
        for key in ("init_ephemeral", "resp_ephemeral"):
            assert key not in c or any(bytes.fromhex(c[key])), "a non-zero ephemeral"
        kinds = sorted((f["message"], f["kind"]) for f in c["faults"])
        assert kinds == sorted((j, k) for j in range(len(c["messages"]))
                               for k in ("read_cut", "read_cut", "read_cut", "write_small"))
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_model_reproduces_the_reference_bytes(oracle):
    """every message, the handshake hash and both split keys of every case"""
    for c in fixture()["cases"]:
        ini, res = ragged_pair(oracle, c)
        for j, m in enumerate(c["messages"]):
            w, r = (ini, res) if ini.action == M.ACTION_WRITE else (res, ini)
            payload = bytes.fromhex(m["payload"])
            over = w.overhead()
            msg = w.write(payload)
            assert msg.hex() == m["ciphertext"], (c["name"], j)
            assert R.session_len(over, len(payload), True) == (False, len(msg))
            assert R.session_len(over, len(msg), False) == (False, len(payload))
            assert r.read(msg) == payload, (c["name"], j)
        assert ini.action == res.action == M.ACTION_SPLIT and ini.status == res.status == 0
        want = (bytes.fromhex(c["k1"]), bytes.fromhex(c["k2"]), bytes.fromhex(c["handshake_hash"]))
        assert ini.split() == want == res.split(), c["name"]


def test_model_reproduces_the_reference_return_codes(oracle):
    """The reference's code for every cut message and every buffer one byte too
    small is the code of the status the model ends with; a refused session
    is inert afterwards and splits to zero keys."""
    seen = {}
    for c in fixture()["cases"]:
        for f in c["faults"]:
            j = f["message"]
            w, r = run_to(oracle, c, j)
            whole = bytes.fromhex(c["messages"][j]["ciphertext"])
            payload = bytes.fromhex(c["messages"][j]["payload"])
            over = len(whole) - len(payload)
            assert w.overhead() == r.overhead() == over
            if f["kind"] == "read_cut":
                assert f["length"] in (0, over - 1, over)
                h_before = r.h
                got = r.read(whole[:f["length"]])
                rc = R.ERROR_OF_STATUS[r.status]
                assert rc == f["rc"], (c["name"], f)
                if f["length"] < over:
                    assert r.status == R.STATUS_LENGTH and got is None and r.h == h_before, (c["name"], f)
                elif not payload:
                    assert r.status == 0 and got == b"", "the whole message: an empty payload"
                s = r
            else:
                assert f["room"] == len(whole) - 1
                h_before = w.h
                assert w.write(payload, room=f["room"]) is None
                assert R.ERROR_OF_STATUS[w.status] == f["rc"] == R.ERROR_INVALID_LENGTH, (c["name"], f)
                assert w.h == h_before
                s = w
            seen[(f["kind"], f["rc"])] = seen.get((f["kind"], f["rc"]), 0) + 1
            if s.status:  # sticky and inert: the later calls do nothing, the split gives zeros
                first = s.status
                while s.action != M.ACTION_SPLIT:
                    assert (s.write(b"x") if s.action == M.ACTION_WRITE else s.read(bytes(200))) is None
                assert s.status == first and s.split()[:2] == (bytes(32), bytes(32))
    assert seen[("write_small", R.ERROR_INVALID_LENGTH)] == 32
    assert seen[("read_cut", R.ERROR_INVALID_LENGTH)] == 64, "0 and overhead - 1 bytes of all 32 messages"
    assert seen[("read_cut", R.ERROR_MAC_FAILURE)] + seen[("read_cut", 0)] == 32


def test_model_equals_session_on_every_in_scope_vector(oracle):
    """Within the lengths the uniform calls accept, the subclass changes
    nothing: all 480 in-scope vectors, every message, payload and split."""
    ran = 0
    for fname in ("cacophony.txt.gz", "noise-c-basic.txt.gz"):
        for v in M.load_vectors(fname):
            if not M.in_scope(v):
                continue
            base, mine = M.vector_sessions(oracle, v), ragged_pair(oracle, v)
            j = 0
            while base[0].action != M.ACTION_SPLIT:
                d = 0 if base[0].action == M.ACTION_WRITE else 1
                payload = bytes.fromhex(v["messages"][j]["payload"])
                m0, m1 = base[d].write(payload), mine[d].write(payload)
                assert m0 == m1 and m0.hex() == v["messages"][j]["ciphertext"], (v["name"], j)
                assert base[1 - d].read(m0) == mine[1 - d].read(m1) == payload
                j += 1
            for b, m in zip(base, mine):
                assert b.split() == m.split() and b.status == m.status == 0
            ran += 1
    assert ran == 480


# ---- the stand-alone program

@functools.lru_cache(maxsize=None)
def run_check():
    return host_check.run_check("handshake_ragged_check", timeout=300).stdout.splitlines()


def test_length_function_equals_the_model_rule():
    """hs_session_len, the source the kernels run, over every (overhead,
    length) pair, both directions"""
    got = [l for l in run_check() if l.startswith("len ")]
    want = []
    for write in (False, True):
        for over in (0, 16, 32, 48, 64, 96, 112):
            for length in list(range(0, 301)) + list(range(65400, 65601)):
                refused, other = R.session_len(over, length, write)
                want.append(f"len {'W' if write else 'R'} {over} {length} {int(refused)} {other}")
    assert len(want) == 2 * 7 * (301 + 201)
    assert got == want
    # a few rows spelled out, so that the rule is not only compared with itself
    assert "len R 48 47 1 0" in got and "len R 48 48 0 0" in got and "len R 48 65535 0 65487" in got
    assert "len R 48 65536 1 0" in got and "len R 0 0 0 0" in got
    assert "len W 48 65487 0 65535" in got and "len W 48 65488 1 0" in got and "len W 96 0 0 96" in got


def test_ragged_argument_checks_under_sanitizers():
    last = run_check()[-1].split()
    assert last[0] == "handshake_ragged_check:" and last[2] == "lens" and last[-1] == "failures"
    assert int(last[1]) == 2 * 7 * (301 + 201) and int(last[3]) > 5000 and last[5] == "0", last
