"""Batched Ed25519 without a GPU: noise_aead_dev_sign_verify / _sign_public / _sign.

(a) noise-c_amd/asan/sign_check.cpp, a stand-alone program (`make -C
    noise-c_amd sign_check`: g++ -fsanitize=address,undefined
    -fno-sanitize-recover=all) over csrc/sc25519.h, csrc/ge25519.h and
    csrc/fe25519.h — the one source of the arithmetic, which the kernels
    compile too — computes every record of tests/golden/ed25519.json on the
    CPU, the SHA-512 digests supplied from hashlib, and checks the entry
    points' argument rules (csrc/dispatch.h check_sign_*) against a
    byte-by-byte reading of the header.  It runs here as a plain child process.
(b) The scalar arithmetic at its edges against Python integers.
(c) The constants of csrc/ge25519.h against the model's derivation.
(d) The argument rules through the library itself; no launch happens.
(e) The sign translation unit compiled for gfx950 spills no register in any
    kernel; VGPRs, occupancy and scratch are printed.
"""
import hashlib
import os
import random
import re
import subprocess

import ed25519_model as M
from host_check import LIB, run_check

ROCM = os.environ.get("ROCM", "/opt/rocm")
L = M.L


def le32(x):
    return x.to_bytes(32, "little").hex()


def answers(feed):
    """the answer lines of sign_check for `feed`, and its last line's numbers"""
    r = run_check("sign_check", feed=feed)
    lines = r.stdout.splitlines()
    last = lines[-1].split()
    assert last[0] == "sign_check:" and last[6] == "failures", lines[-1]
    cases, checks, failures = int(last[1]), int(last[3]), int(last[5])
    assert cases == len(lines) - 1 == feed.count("\n") and failures == 0, lines[-1]
    return [l.split(" ", 1) for l in lines[:-1]], checks


def test_fixture_through_the_shared_arithmetic_under_sanitizers():
    feed, want = [], []
    for name, msg, pub, sig, ok in M.fixture_verify_cases():
        hram = hashlib.sha512(sig[:32] + pub + msg).digest()
        feed.append(f"verify {pub.hex()} {sig.hex()} {hram.hex()}")
        point = M.check_point(msg, pub, sig)
        want.append((name, "verify", f"{0 if ok else 6} {point.hex() if point else '-'}"))
        assert (point == sig[:32]) == ok, name
        na = M.decode_negative(pub)
        feed.append(f"decode {pub.hex()}")
        want.append((name, "decode", "0" if na is None else "1 " + M.encode(na).hex()))
    for name, seed, pub, msg, sig in M.fixture_sign_cases():
        d = hashlib.sha512(seed).digest()
        dr = hashlib.sha512(M.secret_scalar(seed)[1] + msg).digest()
        hram = hashlib.sha512(sig[:32] + pub + msg).digest()
        feed.append(f"public {d.hex()}")
        want.append((name, "public", pub.hex()))
        feed.append(f"sign {d.hex()} {dr.hex()} {hram.hex()}")
        want.append((name, "sign", sig.hex()))
        r = int.from_bytes(dr, "little") % L
        feed.append(f"base {le32(r)}")
        want.append((name, "base", sig[:32].hex()))
    got, checks = answers("".join(l + "\n" for l in feed))
    assert checks > 50000
    verdicts = set()
    for (name, op, w), (gop, g) in zip(want, got):
        assert (gop, g) == (op, w), name
        if op == "verify":
            verdicts.add(w[0])
    assert verdicts == {"0", "6"}


def scalar_edges():
    e = [0, 1, L - 1, L, L + 1, 2**252, 2**253 - 1, 2**256 - 1, 2**512 - 1]
    for k in (2, 15, 2**252, 2**259):
        e += [k * L - 1, k * L + 1]
    assert all(0 <= v < 2**512 for v in e)
    rnd = random.Random(0x5C25519)
    return e + [rnd.getrandbits(512) for _ in range(256)]


def test_scalar_arithmetic_at_its_edges():
    feed, want = [], []
    for v in scalar_edges():
        feed.append("red512 " + v.to_bytes(64, "little").hex())
        want.append(le32(v % L))
        if v < 2**256:
            feed.append("red256 " + le32(v))
            want.append(le32(v % L))
    rnd = random.Random(0x5C25520)
    ops = [0, 1, 2, L - 2, L - 1, 2**252 - 1, 2**252, 2**128, 2**125 - 1]
    triples = [(a, b, c) for a in ops for b in ops for c in (0, 1, L - 1)]
    triples += [tuple(rnd.randrange(L) for _ in range(3)) for _ in range(256)]
    assert (L - 1, L - 1, L - 1) in triples
    for a, b, c in triples:
        feed.append(f"muladd {le32(a)} {le32(b)} {le32(c)}")
        want.append(le32((a * b + c) % L))
    # [k]B at the ends of the walk
    for k in (0, 1, 2, L - 1, 2**252, rnd.randrange(L)):
        feed.append("base " + le32(k))
        want.append(M.encode(M.mul(k, M.B)).hex())
    got, _ = answers("".join(l + "\n" for l in feed))
    for line, w, (_, g) in zip(feed, want, got):
        assert g == w, line
    # a line it cannot read is a failure, not a skipped case
    r = run_check("sign_check", feed="red512 00\n", checked=False)
    assert r.returncode == 1 and "FAIL input" in r.stderr, r.stdout + r.stderr


def test_header_constants_are_the_models():
    text = open(os.path.join(LIB, "csrc", "ge25519.h")).read()
    for name, value in M.header_constants().items():
        m = re.search(r"#define %s\s+\{\{([^}]*)\}\}" % name, text)
        assert m, name
        words = [int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")]
        assert words == M.limbs(value), name
    text = open(os.path.join(LIB, "csrc", "sc25519.h")).read()
    m = re.search(r"#define SC_L_LIMBS \{([^}]*)\}", text)
    assert [int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")] == M.limbs(L)
    m = re.search(r"#define SC_C_LIMBS \{([^}]*)\}", text)
    assert [int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")] == M.limbs(L - 2**252)[:4]


def test_dev_sign_argument_rules(aead):
    """Validation before any launch (no GPU work), on never-dereferenced pointers."""
    A = aead
    ID = A.SIGN_ED25519
    assert ID == 0x5301 and A.ERROR_INVALID_SIGNATURE == 0x4511
    buf = A.C.create_string_buffer(64)
    assert A.lib().noise_strerror(A.ERROR_INVALID_SIGNATURE, buf, 64) == 0 and buf.value == b"Invalid signature"
    vok = dict(pub=0x10000, pub_stride=32, sig=0x20000, sig_stride=64, msg=0x30000, msg_off=0x40000,
               msg_len=0x50000, n=4, status_in=0x60000, status=0x70000)
    sok = dict(priv=0x10000, priv_stride=32, pub=0x20000, pub_stride=32, msg=0x30000, msg_off=0x40000,
               msg_len=0x50000, n=4, sig_out=0x70000)

    def verify(**kw):
        a = {**vok, **kw}
        return A.dev_sign_verify(a.pop("sign_id", ID), **a)

    def sign(**kw):
        a = {**sok, **kw}
        return A.dev_sign(a.pop("sign_id", ID), **a)

    def public(**kw):
        a = {"priv": 0x10000, "priv_stride": 32, "n": 4, "pub_out": 0x30000, **kw}
        return A.dev_sign_public(a.pop("sign_id", ID), **a)

    for call in (verify, sign, public):
        assert call(sign_id=0x5302) == A.ERROR_UNKNOWN_ID
        assert call(sign_id=A.DH_CURVE25519, n=0) == A.ERROR_UNKNOWN_ID
    zeros = dict(pub=0, sig=0, msg=0, msg_off=0, msg_len=0, status_in=0, status=0)
    assert verify(n=0, pub_stride=5, sig_stride=3, **zeros) == A.ERROR_NONE
    assert sign(n=0, priv=0, pub=0, msg=0, msg_off=0, msg_len=0, sig_out=0, priv_stride=5) == A.ERROR_NONE
    assert public(n=0, priv=0, pub_out=0, priv_stride=7) == A.ERROR_NONE
    for k in ("pub", "sig", "msg", "msg_off", "msg_len", "status"):
        assert verify(**{k: 0}) == A.ERROR_INVALID_PARAM, k
    for k in ("priv", "pub", "msg", "msg_off", "msg_len", "sig_out"):
        assert sign(**{k: 0}) == A.ERROR_INVALID_PARAM, k
    for k in ("priv", "pub_out"):
        assert public(**{k: 0}) == A.ERROR_INVALID_PARAM, k
    for s in (1, 31):
        assert verify(pub_stride=s) == A.ERROR_INVALID_PARAM
        assert sign(priv_stride=s) == A.ERROR_INVALID_PARAM
        assert sign(pub_stride=s) == A.ERROR_INVALID_PARAM
        assert public(priv_stride=s) == A.ERROR_INVALID_PARAM
    for s in (1, 32, 63):
        assert verify(sig_stride=s) == A.ERROR_INVALID_PARAM
    assert verify(sig_stride=0) == A.ERROR_INVALID_PARAM
    # the output may touch an input span but not meet it; the message buffer
    # is the caller's guarantee
    for lo, span in ((0x10000, 4 * 32), (0x20000, 4 * 64), (0x40000, 4 * 8), (0x50000, 4 * 4), (0x60000, 4)):
        assert verify(status=lo + span - 1) == A.ERROR_INVALID_PARAM, hex(lo)
        assert verify(status=lo - 4 + 1) == A.ERROR_INVALID_PARAM, hex(lo)
    assert verify(pub_stride=0, status=0x10000 + 31) == A.ERROR_INVALID_PARAM
    assert verify(sig_stride=72, status=0x20000 + 3 * 72 + 63) == A.ERROR_INVALID_PARAM
    for lo, span in ((0x10000, 4 * 32), (0x20000, 4 * 32), (0x40000, 4 * 8), (0x50000, 4 * 4)):
        assert sign(sig_out=lo + span - 1) == A.ERROR_INVALID_PARAM, hex(lo)
        assert sign(sig_out=lo - 4 * 64 + 1) == A.ERROR_INVALID_PARAM, hex(lo)
    assert public(pub_out=0x10000 + 4 * 32 - 1) == A.ERROR_INVALID_PARAM
    assert public(pub_out=0x10000 - 4 * 32 + 1) == A.ERROR_INVALID_PARAM
    assert public(pub_out=0x10000) == A.ERROR_INVALID_PARAM
    assert sign(sig_out=0x10000) == A.ERROR_INVALID_PARAM


def test_sign_kernels_spill_nothing():
    """The compiler's own report for the sign unit.  The scratch it shows is
    the SHA-512 state and block buffer of the hash phases; a spilled register
    would be a limb of a point, or of a secret scalar, in device memory."""
    cmd = [f"{ROCM}/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-I../include", "-Icsrc",
           "--cuda-device-only", "-c", "csrc/launch_sign.hip", "-o", "/dev/null",
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, cwd=LIB, capture_output=True, text=True, timeout=600)
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
    kernels = {k: v for k, v in rows.items() if "_batch" in k}
    assert len(kernels) == 3, list(rows)  # verify, public, sign
    for name, row in rows.items():
        report = (f"{name}: VGPRs {row.get('VGPRs')}, AGPRs {row.get('AGPRs')}, "
                  f"occupancy {row.get('Occupancy [waves/SIMD]')} waves/SIMD, "
                  f"scratch {row.get('ScratchSize [bytes/lane]')} bytes/lane, "
                  f"spilled VGPRs {row.get('VGPRs Spill')}")
        print(report)
        assert row.get("VGPRs Spill") == "0" and row.get("SGPRs Spill") == "0", report
