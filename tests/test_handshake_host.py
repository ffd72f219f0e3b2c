"""The host-only half of the batched handshakes without a GPU.

noise-c_amd/asan/handshake_check.cpp, a stand-alone program (`make -C
noise-c_amd handshake_check`: g++ -fsanitize=address,undefined
-fno-sanitize-recover=all) over csrc/handshake_plan.h, prints the steps and
the overhead of every message for every pattern x role x prefix, parses the
names it is fed, and runs the argument checks of write_message, read_message,
split and new against a byte-by-byte reading of the header comment.  It runs
here once, as a plain child process; the tests compare what it printed with
the table of tests/handshake_model.py — the table that
tests/test_handshake_model_host.py proves against the recorded vectors."""
import functools

import handshake_model as M
import host_check
FILES = ("cacophony.txt.gz", "noise-c-basic.txt.gz", "noise-c-fallback.txt.gz", "noise-c-hybrid.txt.gz")
MALFORMED = ["", "Noise", "Noise_XX_25519_ChaChaPoly", "Noise_XX_25519_ChaChaPoly_SHA256_", "noise_XX_25519_ChaChaPoly_SHA256",
             "NoisePSK2_XX_25519_ChaChaPoly_SHA256", "Noise_XY_25519_ChaChaPoly_SHA256", "Noise_XX_25518_AESGCM_SHA256",
             "Noise_XX_25519_AES_SHA256", "Noise_XX_25519_AESGCM_SHA384", "Noise_XX_25519_AESGCM_SHA256_extra",
             "Noise_hfs_25519_AESGCM_SHA256", "Noise_XX+hfs_25519+448_AESGCM_SHA256", "Noise_XX_25519+_AESGCM_SHA256",
             "Noise_XX_25519+448+448_AESGCM_SHA256", "Noise__25519_AESGCM_SHA256", "Noise_XX _25519_AESGCM_SHA256"]


def vector_names():
    names = []
    for f in FILES:
        names += [v["name"] for v in M.load_vectors(f)]
    return names


@functools.lru_cache(maxsize=None)
def run_check():
    names = vector_names() + MALFORMED
    r = host_check.run_check("handshake_check", feed="".join(n + "\n" for n in names), timeout=300)
    return r.stdout.splitlines(), names


def test_steps_and_overheads_equal_the_model_table():
    lines, _ = run_check()
    got = [l for l in lines if l.startswith(("req ", "plan "))]
    want = M.plan_lines()
    # 15 patterns x 2 roles x 2 prefixes, one line per message and one for the keys
    assert len(want) == 60 + 4 * sum(len(p[2]) for p in M.PATTERNS.values())
    assert got == want
    # a few rows spelled out, so that the table is not only compared with itself
    assert "plan XX I Noise 1 R keyed_in=0 steps=e,ee:e.e,s+aead,es:e.s,p+aead overhead=96 next=write" in got
    assert "plan IK R NoisePSK 0 R keyed_in=0 steps=e+mk,es:s.e,s+aead,ss:s.s,p+aead overhead=96 next=write" in got
    assert "plan NN I Noise 0 W keyed_in=0 steps=e,p overhead=32 next=read" in got
    assert "plan N R Noise 0 R keyed_in=0 steps=e,es:s.e,p+aead overhead=48 next=split" in got
    assert "req KX R Noise local_s=1 local_e=1 remote_s=1 psk=0" in got


def test_overheads_equal_the_recorded_messages():
    """ciphertext length - payload length of every handshake message of
    noise-c-basic is the overhead the plan gives."""
    seen = 0
    for v in M.load_vectors("noise-c-basic.txt.gz"):
        if not M.in_scope(v):
            continue
        rc, f = M.parse_name(v["name"])
        for idx in range(len(M.PATTERNS[f["pattern"]][2])):
            m = v["messages"][idx]
            over = (len(m["ciphertext"]) - len(m["payload"])) // 2
            assert M.message_plan(f["pattern"], True, f["psk"], idx)[1] == over, (v["name"], idx)
            assert M.message_plan(f["pattern"], False, f["psk"], idx)[1] == over
            seen += 1
    assert seen == 16 * sum(len(p[2]) for p in M.PATTERNS.values())


def test_parser_on_every_vector_name_and_on_malformed_ones():
    lines, names = run_check()
    answers = [l for l in lines if l.startswith("name ")]
    assert len(answers) == len(names) == 480 + 480 + 32 + 400 + len(MALFORMED)
    counts = {0: 0, M.ERROR_NOT_APPLICABLE: 0, M.ERROR_UNKNOWN_NAME: 0}
    for name, line in zip(names, answers):
        assert line.startswith(f"name {name} 0x"), line
        f = line[len(name) + 6:].split()
        rc = int(f[0], 16)
        want_rc, want = M.parse_name(name)
        assert rc == want_rc, line
        if rc == 0:
            assert f[1:] == [want["pattern"], f"0x{want['cipher']:04x}", f"0x{want['hash']:04x}", str(int(want["psk"]))], line
        counts[rc] += 1
        # and what the model's own answer must be, from the name alone
        if name in MALFORMED:
            assert rc == M.ERROR_UNKNOWN_NAME, line
        elif "448" in name or "NewHope" in name or "hfs" in name or "fallback" in name:
            assert rc == M.ERROR_NOT_APPLICABLE, line
        else:
            assert rc == 0 and "_25519_" in name, line
    assert counts == {0: 480, M.ERROR_NOT_APPLICABLE: 480 + 32 + 400, M.ERROR_UNKNOWN_NAME: len(MALFORMED)}


def test_argument_checks_under_sanitizers():
    lines, names = run_check()
    last = lines[-1].split()
    assert last[0] == "handshake_check:" and last[2] == "plans" and last[-1] == "failures"
    assert int(last[1]) == 4 * sum(len(p[2]) for p in M.PATTERNS.values())
    assert int(last[3]) == len(names) and int(last[5]) > 100000 and last[7] == "0", last
