"""Batched X25519 without a GPU: noise_aead_dev_dh_calculate / _dh_public.

(a) The big-integer ladder of tests/x25519_ref.py — the checker the GPU tests
    use — equals the reference's curve25519_donna and
    curved25519_scalarmult_basepoint on every case of tests/golden/x25519.json
    (gen_x25519.py): the RFC 7748 vectors, the edge public values, the small
    order points, the scalars that clamping changes, 64 random pairs.
(b) noise-c_amd/asan/dh_check.cpp, a stand-alone program (`make -C noise-c_amd
    dh_check`: g++ -fsanitize=address,undefined -fno-sanitize-recover=all)
    over csrc/fe25519.h — the one source of the field arithmetic, ladder,
    inversion and freeze, which the kernels compile too — computes every
    fixture case on the CPU and checks the entry points' argument rules
    (csrc/dispatch.h check_dh) against a byte-by-byte reading of the header.
    It runs here as a plain child process.
(c) The argument rules through the library itself; no launch happens.
(d) The DH translation unit compiled for gfx950 reports no scratch memory for
    any kernel: no limb of a private key is spilled to device memory.
(e) The field operations one at a time, on the operands of tests/f25_cases.py:
    the coverage condition (the edge set alone takes every named carry path
    of every operation, the random operands none of the rare ones), every
    vector through csrc/fe25519.h in dh_check under ASan/UBSan, and the
    argument rules of noise_aead_debug_f25_op, which tests/test_gpu_f25.py
    runs the same vectors through.
"""
import os
import re
import subprocess

import f25_cases as F
import x25519_ref as X
from host_check import LIB, run_check
ROCM = os.environ.get("ROCM", "/opt/rocm")


def test_checker_equals_the_reference_fixture():
    cases = X.fixture_cases()
    names = [c["name"] for c in cases]
    assert len(cases) >= 2 + 2 + 10 + 8 + 64 and len(set(names)) == len(names)
    assert cases[0]["shared"] == "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
    for c in cases:
        priv, pub = bytes.fromhex(c["priv"]), bytes.fromhex(c["pub"])
        assert X.x25519(priv, pub).hex() == c["shared"], c["name"]
        assert X.x25519_base(priv).hex() == c["public"], c["name"]
    by = {c["name"]: c for c in cases}
    # what the header promises about the edge values
    for n in ("u=0", "u=1", "u=p-1", "u=p", "u=p+1", "u=order8a", "u=order8b"):
        assert by[n]["shared"] == "00" * 32, n
    assert by["u=9"]["shared"] == by["u=9"]["public"]
    assert by["u=0xff..ff"]["shared"] == X.x25519(bytes.fromhex(by["u=0xff..ff"]["priv"]),
                                                  (18).to_bytes(32, "little")).hex()


def test_shared_ladder_and_argument_rules_under_sanitizers():
    cases = X.fixture_cases()
    feed = "".join(f"{c['priv']} {c['pub']} {c['shared']} {c['public']}\n" for c in cases)
    r = run_check("dh_check", feed=feed)
    line = [l for l in r.stdout.splitlines() if l.startswith("dh_check:")][-1].split()
    assert int(line[1]) == len(cases) and int(line[3]) > 50000 and line[5] == "0", line
    # a wrong expected value is noticed: the program does compare
    bad = cases[0]["shared"][:-1] + ("0" if cases[0]["shared"][-1] != "0" else "1")
    r = run_check("dh_check", feed=f"{cases[0]['priv']} {cases[0]['pub']} {bad} {cases[0]['public']}\n", checked=False)
    assert r.returncode == 1 and "FAIL calculate" in r.stderr, r.stdout + r.stderr


def test_f25_edge_set_takes_every_named_path():
    """The coverage condition of tests/f25_cases.py.  The restated steps must
    also give the right residue for every vector, or the path names mean
    nothing."""
    assert len(set(F.E)) == len(F.E) and all(0 <= v < F.M for v in F.E)
    assert set(F.PATHS) == set(F.OPS)
    for op in F.OPS:
        taken = {}
        for a, b in F.edge_vectors(op):
            raw, names = F.paths(op, a, b)
            assert raw % F.P == F.expected(op, a, b), (op, hex(a), hex(b))
            assert names <= set(F.PATHS[op]), (op, names)
            for name in names:
                taken[name] = taken.get(name, 0) + 1
        print(op, taken)
        assert all(taken.get(name, 0) >= 1 for name in F.PATHS[op]), (op, taken)
        assert len(F.random_vectors(op)) == F.RANDOM_PAIRS
        for a, b in F.random_vectors(op):
            raw, names = F.paths(op, a, b)
            assert raw % F.P == F.expected(op, a, b), (op, hex(a), hex(b))
            assert not names & set(F.RARE), (op, hex(a), hex(b), names)
        assert len(F.vectors(op)) % 64 != 0  # a launch ends inside a workgroup
    # freeze restated gives the canonical value itself, and the expectations
    # are what they say: in [0, p), a * a^-1 = 1
    for a in F.E:
        assert F.paths("freeze", a)[0] == a % F.P
        inv = F.expected("invert", a)
        assert 0 <= inv < F.P and a * inv % F.P == (0 if a % F.P == 0 else 1)


def test_f25_field_operations_under_sanitizers():
    """Every vector of every operation through the header on the CPU."""
    feed = "".join(F.check_lines(op) for op in F.OPS)
    total = sum(len(F.vectors(op)) for op in F.OPS)
    r = run_check("dh_check", feed=feed)
    lines = r.stdout.splitlines()
    f25 = [l for l in lines if l.startswith("dh_check f25:")][-1].split()
    assert int(f25[2]) == total and f25[4] == "0", f25
    last = [l for l in lines if l.startswith("dh_check:")][-1].split()
    assert last[1] == "0" and int(last[3]) > 50000 and last[5] == "0", last
    # a wrong expected value is noticed, for the operation that is frozen
    # here and for the one that freezes itself
    for op in ("sub", "freeze"):
        a, b = F.vectors(op)[5]
        wrong = (F.expected(op, a, b) + 1) % F.P
        r = run_check("dh_check", feed=f"f25 {op} {F.le32(a).hex()} {F.le32(b).hex()} {F.le32(wrong).hex()}\n", checked=False)
        assert r.returncode == 1 and f"FAIL f25 {op}" in r.stderr, r.stdout + r.stderr
        assert "dh_check f25: 1 vectors 1 failures" in r.stdout
    # and a line it cannot read is a failure, not a skipped vector
    r = run_check("dh_check", feed="f25 cube 00 00 00\n", checked=False)
    assert r.returncode == 1 and "FAIL input" in r.stderr, r.stdout + r.stderr


def test_debug_f25_op_argument_rules(aead):
    """Validation before any launch (no GPU work), on never-dereferenced pointers."""
    A = aead
    assert [A.F25_ADD, A.F25_SUB, A.F25_MUL, A.F25_SQ, A.F25_MUL_121665, A.F25_MUL_9, A.F25_FREEZE,
            A.F25_INVERT] == [F.OPS[op][0] for op in F.DEVICE_OPS] == list(range(8))
    ok = dict(a=0x10000, b=0x20000, n=4, out=0x30000)
    for op in (-1, 8, 0x4401):
        assert A.debug_f25_op(op, **ok) == A.ERROR_UNKNOWN_ID
        assert A.debug_f25_op(op, **{**ok, "n": 0}) == A.ERROR_UNKNOWN_ID
    for op in range(8):
        binary = op <= A.F25_MUL
        assert A.debug_f25_op(op, a=0, b=0, n=0, out=0) == A.ERROR_NONE
        assert A.debug_f25_op(op, **{**ok, "a": 0}) == A.ERROR_INVALID_PARAM
        assert A.debug_f25_op(op, **{**ok, "out": 0}) == A.ERROR_INVALID_PARAM
        if binary:
            assert A.debug_f25_op(op, **{**ok, "b": 0}) == A.ERROR_INVALID_PARAM
        # the output may touch an operand range but not meet it
        assert A.debug_f25_op(op, **{**ok, "out": 0x10000}) == A.ERROR_INVALID_PARAM
        assert A.debug_f25_op(op, **{**ok, "out": 0x10000 + 4 * 32 - 1}) == A.ERROR_INVALID_PARAM
        assert A.debug_f25_op(op, **{**ok, "out": 0x10000 - 4 * 32 + 1}) == A.ERROR_INVALID_PARAM
        if binary:
            assert A.debug_f25_op(op, **{**ok, "out": 0x20000 + 4 * 32 - 1}) == A.ERROR_INVALID_PARAM


def test_dev_dh_argument_rules(aead):
    """Validation before any launch (no GPU work), on never-dereferenced pointers."""
    A = aead
    ID = A.DH_CURVE25519
    assert ID == 0x4401
    ok = dict(priv=0x10000, priv_stride=32, pub=0x20000, pub_stride=32, n=4, shared=0x30000)

    def calc(**kw):
        return A.dev_dh_calculate(kw.pop("dh_id", ID), **{**ok, **kw})

    def public(**kw):
        a = {"priv": 0x10000, "priv_stride": 32, "n": 4, "pub_out": 0x30000, **kw}
        return A.dev_dh_public(a.pop("dh_id", ID), **a)

    assert calc(dh_id=0x4402) == A.ERROR_UNKNOWN_ID      # Curve448: not yet
    assert calc(dh_id=0x4801, n=0) == A.ERROR_UNKNOWN_ID
    assert public(dh_id=0) == A.ERROR_UNKNOWN_ID
    assert calc(n=0, priv=0, pub=0, shared=0, priv_stride=5) == A.ERROR_NONE
    assert public(n=0, priv=0, pub_out=0) == A.ERROR_NONE
    for k in ("priv", "pub", "shared"):
        assert calc(**{k: 0}) == A.ERROR_INVALID_PARAM, k
    for k in ("priv", "pub_out"):
        assert public(**{k: 0}) == A.ERROR_INVALID_PARAM, k
    for s in (1, 31):
        assert calc(priv_stride=s) == A.ERROR_INVALID_PARAM
        assert calc(pub_stride=s) == A.ERROR_INVALID_PARAM
        assert public(priv_stride=s) == A.ERROR_INVALID_PARAM
    # the output may touch an input span but not meet it
    assert calc(shared=0x10000) == A.ERROR_INVALID_PARAM
    assert calc(shared=0x10000 + 4 * 32 - 1) == A.ERROR_INVALID_PARAM
    assert calc(shared=0x20000 - 4 * 32 + 1) == A.ERROR_INVALID_PARAM
    assert calc(priv_stride=0, shared=0x10000 + 31) == A.ERROR_INVALID_PARAM
    assert calc(pub_stride=40, shared=0x20000 + 3 * 40 + 31) == A.ERROR_INVALID_PARAM
    assert public(pub_out=0x10000 + 4 * 32 - 1) == A.ERROR_INVALID_PARAM
    assert public(pub_out=0x10000 - 4 * 32 + 1) == A.ERROR_INVALID_PARAM
    assert public(n=1, pub_out=0x10000 + 31) == A.ERROR_INVALID_PARAM


def test_dh_kernels_use_no_scratch():
    """The compiler's own report for the DH unit (as tools/kres.py reads it)."""
    cmd = [f"{ROCM}/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-I../include", "-Icsrc",
           "--cuda-device-only", "-c", "csrc/launch_dh.hip", "-o", "/dev/null",
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
    kernels = {k: v for k, v in rows.items() if "x25519_batch" in k}
    assert len(kernels) == 2, list(rows)  # the base point and the per-session point
    for name, row in rows.items():
        report = (f"{name}: VGPRs {row.get('VGPRs')}, occupancy {row.get('Occupancy [waves/SIMD]')} waves/SIMD, "
                  f"scratch {row.get('ScratchSize [bytes/lane]')} bytes/lane, "
                  f"spilled VGPRs {row.get('VGPRs Spill')}")
        print(report)
        assert row.get("ScratchSize [bytes/lane]") == "0", report
        assert row.get("VGPRs Spill") == "0" and row.get("SGPRs Spill") == "0", report
