"""Rekey on the device without a GPU (header section 12).

(a) The model of tests/transport_rekey_model.py: REKEY(k) through the oracle's
    encrypt at nonce 2^64 - 1 equals the known answers, and equals the
    single-block formulas the kernels compute (one ChaCha20 block; two AES
    blocks) on random keys; a frame sealed under a rekeyed session opens under
    REKEY(k) and not under k.
(b) noise-c_amd/asan/transport_rekey_check.cpp, a stand-alone program (`make
    -C noise-c_amd transport_rekey_check`: g++ -fsanitize=address,undefined
    -fno-sanitize-recover=all) over csrc/transport_plan.h and csrc/dispatch.h,
    as a plain child process: both argument checks against a byte-by-byte
    reading of the header, the direction rule of an entry, the bytes of the
    counter blocks.
(c) The argument rules of both entry points through the library itself, on
    never-dereferenced pointers.  No launch happens.
(d) The compiler's resource report: the ChaChaPoly rekey kernels keep their
    state in registers (no scratch, no spills); the AES-GCM ones are printed.
"""
import os
import re
import subprocess

import numpy as np

import transport_model as T
import transport_rekey_model as R
from host_check import LIB, run_check

ROCM = os.environ.get("ROCM", "/opt/rocm")

K_COUNT = bytes(range(32))
KNOWN = {
    T.CHACHAPOLY: [
        (K_COUNT, 1, "50835543a205b22c9323f2022bc4f67d838f90e61d5ccf33c4513e01f85b5042"),
        (bytes(32), 1, "25ce5d37df19f3783185f2ffd5ab17fa3397c212f02d62fb1733e0b875b74c58"),
        (b"\xff" * 32, 1, "5bac2acd86a836c5dc98c116c1217ec31d3a63a9451319f097f3b4d6dab07787"),
        (K_COUNT, 3, "83a272a70ec674e16167ca927f6556225f00403ccf784202ea421eec6250d359"),
    ],
    T.AESGCM: [
        (K_COUNT, 1, "0201675c87335949b909793da5bb4d92fcf6d44b92a6e0792b6ae48b1881259d"),
        (bytes(32), 1, "f1573ed7ea59562387a25c24fabe25a3155fecd880e181089fe581c148cc6ba9"),
        (b"\xff" * 32, 1, "e686af6a1a45846d844a57057123da84529ec441d25c799cbaba1ffa30948e3f"),
        (K_COUNT, 3, "bf664a26ceb22d128912d93ac8e0cb34e835962120956ce111e1cd23000b7a08"),
    ],
}


def test_rekey_known_answers_and_block_formulas(oracle):
    for cipher, rows in KNOWN.items():
        for key, times, want in rows:
            assert R.rekey_times(oracle, cipher, key, times).hex() == want, (hex(cipher), key[:2].hex(), times)
            k = key
            for _ in range(times):
                k = R.rekey_blocks(oracle, cipher, k)
            assert k.hex() == want, ("block formula", hex(cipher), key[:2].hex(), times)
        rng = np.random.default_rng(cipher)
        for _ in range(64):
            key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
            got = R.rekey(oracle, cipher, key)
            assert len(got) == 32 and got == R.rekey_blocks(oracle, cipher, key), (hex(cipher), key.hex())
            assert got != key


def test_rekeyed_session_seals_under_the_successor(oracle):
    """rekey_session replaces the chosen keys and nothing else; what the model
    then seals opens under REKEY(k) at the nonce the session had reached."""
    rng = np.random.default_rng(5)
    for cipher in (T.CHACHAPOLY, T.AESGCM):
        k1, k2 = (rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(2))
        for directions in (1, 2, 3):
            s = T.Session.of_role(oracle, cipher, True, k1, k2)
            s.send, s.recv = 7, 11
            R.rekey_session(s, directions)
            assert (s.send, s.recv) == (7, 11)
            assert s.send_key == (R.rekey(oracle, cipher, k1) if directions & 1 else k1)
            assert s.recv_key == (R.rekey(oracle, cipher, k2) if directions & 2 else k2)
        s = R.rekey_session(T.Session.of_role(oracle, cipher, True, k1, k2), R.SEND)
        s.send = 7
        payload = bytes(range(40))
        out, result, _ = s.run("seal", T.frame(payload + bytes(16)))
        assert result == (1, 58, 0) and s.send == 8
        rc, pt = oracle.decrypt(cipher, R.rekey(oracle, cipher, k1), 7, out[2:])
        assert rc == 0 and pt == payload
        assert oracle.decrypt(cipher, k1, 7, out[2:])[0] != 0
        assert oracle.decrypt(cipher, R.rekey(oracle, cipher, k1), 0, out[2:])[0] != 0  # the nonce went on, not back to 0


def test_rekey_table_entry_rule(oracle):
    """ignored entries, the per-entry byte, the NULL list"""
    rng = np.random.default_rng(6)
    keys = [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
            for _ in range(6)]

    def table():
        return [None if i == 2 else T.Session.of_role(oracle, T.CHACHAPOLY, False, *keys[i]) for i in range(6)]

    sess = table()
    done = R.rekey_table(sess, 3, 5, slots=[4, 2, 99, 0, 5], which=[1, 3, 3, 0xFF, 0])
    assert done == [(4, 1), (0, 1), (0, 2)]
    nk = lambda k: R.rekey(oracle, T.CHACHAPOLY, k)  # noqa: E731
    assert sess[2] is None
    # the responder sends under k2
    assert (sess[4].send_key, sess[4].recv_key) == (nk(keys[4][1]), keys[4][0])
    assert (sess[0].send_key, sess[0].recv_key) == (nk(keys[0][1]), nk(keys[0][0]))
    for i in (1, 3, 5):
        assert (sess[i].send_key, sess[i].recv_key) == (keys[i][1], keys[i][0])
    sess = table()
    assert R.rekey_table(sess, 2, 4) == [(0, 2), (1, 2), (3, 2)]
    assert [R.entry_directions(d, None, 0) for d in range(4)] == [0, 1, 2, 3]
    assert [[R.entry_directions(d, [w], 0) for w in range(4)] for d in range(4)] == \
        [[0, 0, 0, 0], [0, 1, 0, 1], [0, 0, 2, 2], [0, 1, 2, 3]]


def test_argument_rules_direction_rule_and_blocks_under_sanitizers():
    r = run_check("transport_rekey_check")
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "transport_rekey_check:" and last[2] == "checks" and last[4] == "failures"
    assert int(last[1]) > 5000 and last[3] == "0", last
    # expectations of ours that hold, and wrong ones: the program does compare
    r = run_check("transport_rekey_check", "expect", "3", "-1", "3", "expect", "1", "2", "0", "expect", "2", "255", "2",
                  checked=False)
    assert r.returncode == 0 and r.stdout.split()[-2] == "0", r.stdout + r.stderr
    for wrong in (("3", "1", "3"), ("1", "-1", "3"), ("2", "1", "2"), ("3", "0", "1")):
        r = run_check("transport_rekey_check", "expect", *wrong, checked=False)
        assert r.returncode == 1 and "FAIL expect" in r.stderr, r.stdout + r.stderr
        assert r.stdout.split()[-2] != "0"
    r = run_check("transport_rekey_check", "something else", checked=False)
    assert r.returncode == 1 and "FAIL argument" in r.stderr


def test_rekey_argument_rules_through_the_library(aead):
    """Validation before any launch (no GPU work), in the stated order, on
    never-dereferenced pointers and n == 0 objects."""
    A = aead
    BAD, OK, UNKNOWN = A.ERROR_INVALID_PARAM, A.ERROR_NONE, A.ERROR_UNKNOWN_ID
    assert (A.REKEY_SEND, A.REKEY_RECEIVE) == (1, 2)
    ok = dict(keys=0x10000, n=4, out=0x20000)
    # 1. the cipher, also with n == 0 and whatever else is wrong
    for cipher in (0, 0x4300, 0x4303, A.DH_CURVE25519):
        assert A.dev_rekey(cipher, **ok) == UNKNOWN
        assert A.dev_rekey(cipher, keys=0, n=0, out=0) == UNKNOWN
        assert A.dev_rekey(cipher, keys=0x10000, n=4, out=0x10001) == UNKNOWN
    for cipher in (A.CHACHAPOLY, A.AESGCM):
        # 2. n == 0 before the pointers and the ranges
        assert A.dev_rekey(cipher, keys=0, n=0, out=0) == OK
        assert A.dev_rekey(cipher, keys=0x10000, n=0, out=0x10001) == OK
        # 3. a NULL pointer
        assert A.dev_rekey(cipher, **{**ok, "keys": 0}) == BAD
        assert A.dev_rekey(cipher, **{**ok, "out": 0}) == BAD
        assert A.dev_rekey(cipher, keys=0, n=1, out=0) == BAD
        # 4. the output may touch the keys but not meet them (exactly in place launches: the GPU tests)
        for out in (0x10000 + 1, 0x10000 - 1, 0x10000 + 32, 0x10000 + 4 * 32 - 1, 0x10000 - 4 * 32 + 1):
            assert A.dev_rekey(cipher, **{**ok, "out": out}) == BAD, hex(out)

    # the table call: a NULL object comes first, before m == 0
    for m in (0, 1):
        for directions in (0, 3):
            assert A.dev_transport_rekey(None, m=m, directions=directions) == BAD
    made = [A.dev_transport_new_unkeyed(A.CHACHAPOLY, A.ROLE_INITIATOR, 0, max_frames=0),
            A.dev_transport_new_unkeyed(A.AESGCM, A.ROLE_RESPONDER, 0, max_frames=8)]
    for rc, tr in made:
        assert rc == 0 and tr
        for directions in (0, 1, 2, 3, 4, 2 ** 32 - 1):
            assert A.dev_transport_rekey(tr, m=0, directions=directions) == OK  # m == 0 before the directions
            assert A.dev_transport_rekey(tr, m=0, directions=directions, slots=0x4000, which=0x5000) == OK
            assert A.dev_transport_rekey(tr, m=1, directions=directions) == BAD  # m > n
            assert A.dev_transport_rekey(tr, m=2 ** 32 - 1, directions=directions, slots=0x4000) == BAD
        assert A.dev_transport_free(tr) == OK


def _resource_report(unit):
    """{kernel: {row: value}} of hipcc's -Rpass-analysis=kernel-resource-usage for one device unit"""
    cmd = [f"{ROCM}/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-I../include", "-Icsrc",
           "--cuda-device-only", "-c", f"csrc/{unit}.hip", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, cwd=LIB, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    cur, rows = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*)", line)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].split(" [")[0].strip()
            rows[cur] = {}
        elif cur and ":" in t:
            k, v = t.split(":", 1)
            rows[cur][k.strip()] = v.split("[-R")[0].strip()
    return rows


def _report_line(name, row):
    return (f"{name}: VGPRs {row.get('VGPRs')}, SGPRs {row.get('TotalSGPRs')}, "
            f"occupancy {row.get('Occupancy [waves/SIMD]')} waves/SIMD, LDS {row.get('LDS Size [bytes/block]')} bytes, "
            f"scratch {row.get('ScratchSize [bytes/lane]')} bytes/lane, "
            f"spilled VGPRs {row.get('VGPRs Spill')}, spilled SGPRs {row.get('SGPRs Spill')}")


def test_chachapoly_rekey_kernels_use_no_scratch():
    """The compiler's own report for the transport unit, which holds both
    ChaChaPoly rekey kernels: a key's successor never leaves the registers."""
    rows = _resource_report("transport")
    kernels = {k: v for k, v in rows.items() if "tr_rekey_keys" in k or "tr_rekey_slots" in k}
    assert len(kernels) == 2, list(rows)  # the raw keys and the slots
    for name, row in kernels.items():
        report = _report_line(name, row)
        print(report)
        assert row.get("ScratchSize [bytes/lane]") == "0", report
        assert row.get("VGPRs Spill") == "0" and row.get("SGPRs Spill") == "0", report


def test_aesgcm_rekey_kernels_are_reported():
    """The AES-GCM rekey kernels of the AES unit: printed, not bounded."""
    rows = _resource_report("launch_aes")
    kernels = {k: v for k, v in rows.items() if "gcm_rekey_keys" in k or "gcm_rekey_slots" in k}
    assert len(kernels) == 2, [k for k in rows if "rekey" in k or "prepare" in k]
    for name, row in kernels.items():
        print(_report_line(name, row))
