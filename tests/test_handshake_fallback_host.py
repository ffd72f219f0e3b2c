"""The Noise Pipes fallback without a GPU (include/noise_aead_hip.h section 15).

The model of tests/handshake_fallback_model.py against the 16 Curve25519
vectors of noise-c-fallback and against tests/golden/handshake_fallback.json,
which tests/golden/gen_handshake_fallback.py recorded from the reference's own
noise_handshakestate_fallback; noise-c_amd/asan/handshake_fallback_check.cpp,
the host-only half of csrc/handshake_plan.h under ASan/UBSan, against the
model; and the argument rules of both calls through the library on n == 0
objects, which launch nothing."""
import functools
import json
import os

import handshake_fallback_model as F
import handshake_model as M
import host_check

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handshake_fallback.json")
STATUSES = list(range(8)) + [255]


# ------------------------------------------------------------ the model

def test_model_reproduces_every_25519_fallback_vector(oracle):
    vs = F.fallback_vectors()
    assert len(vs) == 16 and len(M.load_vectors("noise-c-fallback.txt.gz")) == 32
    seen = set()
    for v in vs:
        # the initiator's copy of the responder's static key is stale, so the first message fails
        assert bytes.fromhex(v["init_remote_static"]) != M.dh_base(bytes.fromhex(v["resp_static"]))
        over = [(len(m["ciphertext"]) - len(m["payload"])) // 2 for m in v["messages"][:3]]
        assert over == [96, 96, 64] and v["pattern"] == "IK"
        fr, fi = F.run_vector(oracle, v)
        assert fr.initiator and not fi.initiator and fr.rs == fi.s_pub and fi.rs == fr.s_pub
        seen.add((v["name"].split("_")[0], v["cipher"], v["hash"]))
    assert len(seen) == 16, "every prefix x cipher x hash, none skipped"


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def case_sessions(orc, c):
    def hx(key):
        return bytes.fromhex(c[key]) if key in c else None
    ini = M.Session(orc, c["name"], True, hx("prologue"), hx("psk"), hx("init_static"), hx("init_ephemeral"),
                    hx("init_remote_static"))
    res = M.Session(orc, c["name"], False, hx("prologue"), hx("psk"), hx("resp_static"), hx("resp_ephemeral"),
                    hx("resp_remote_static"))
    return ini, res


def test_model_reproduces_the_reference_fallback_fixture(oracle):
    """Originals IK, XK, KK and NK, a first message that verified or failed,
    fallback prologues of other lengths and empty, both ciphers, BLAKE2s and
    SHA512, both prefixes: every message, the hash and the split keys."""
    cases = fixture()["cases"]
    seen = set()
    for c in cases:
        def hx(key):
            return bytes.fromhex(c[key]) if key in c else None
        ini, res = case_sessions(oracle, c)
        msgs = [(bytes.fromhex(m["payload"]), bytes.fromhex(m["ciphertext"])) for m in c["messages"]]
        assert ini.write(msgs[0][0]) == msgs[0][1], (c["name"], 0)
        back = res.read(msgs[0][1])
        assert (back == msgs[0][0] and res.status == 0) if c["first_verified"] else (back is None and res.status == 1)
        rc, fr = F.fallback(oracle, res, hx("fb_prologue"), hx("psk"), hx("fresh_ephemeral"))
        assert rc == 0 and fr.name == F.fallback_name(c["name"])
        assert res.status == (F.STATUS_ABSENT if c["first_verified"] else M.STATUS_MAC)
        rc, fi = F.fallback(oracle, ini, hx("fb_prologue"), hx("psk"))
        assert (rc == 0) == c["both_sides"] and (rc == 0 or rc == F.ERROR_LOCAL_KEY_REQUIRED), (c["name"], hex(rc))
        assert fr.overhead() == 96 and fr.write(msgs[1][0]) == msgs[1][1], (c["name"], 1)
        assert len(msgs) == (3 if c["both_sides"] else 2)
        if c["both_sides"]:
            assert ini.status == F.STATUS_ABSENT
            assert fi.read(msgs[1][1]) == msgs[1][0]
            assert fi.overhead() == fr.overhead() == 64
            assert fi.write(msgs[2][0]) == msgs[2][1], (c["name"], 2)
            assert fr.read(msgs[2][1]) == msgs[2][0]
            assert fr.split() == fi.split() == (hx("k1"), hx("k2"), hx("handshake_hash"))
        seen.add((c["name"].split("_")[0], c["pattern"], c["name"].split("_", 3)[3], c["first_verified"],
                  len(hx("prologue")), len(hx("fb_prologue"))))
    assert len(seen) == len(cases) == 64
    assert {s[1] for s in seen} == {"IK", "XK", "KK", "NK"}
    assert {s[2] for s in seen} == {"ChaChaPoly_BLAKE2s", "AESGCM_SHA512"}
    assert {s[3:] for s in seen} == {(False, 11, 11), (True, 5, 23), (False, 9, 0), (True, 0, 7)}


def test_model_gives_the_reference_return_codes(oracle):
    """NN or XX as the original, a fallback before any message and after two,
    and the NK initiator, whose fallback the reference takes and whose start
    it refuses: the one call of this library gives that code."""
    refusals = fixture()["refusals"]
    keys = {k: bytes([i + 1]) * 32 for i, k in enumerate(("is", "ie", "rs", "re", "psk"))}
    codes = set()
    for r in refusals:
        rc, f = M.parse_name(r["name"])
        pre_i, pre_r, msgs = M.PATTERNS[f["pattern"]]
        ls_i, _, _ = M.needs(f["pattern"], True)
        psk = keys["psk"] if f["psk"] else None
        ini = M.Session(oracle, r["name"], True, b"", psk, keys["is"] if ls_i else None, keys["ie"],
                        M.dh_base(keys["rs"]) if pre_r else None)
        res = M.Session(oracle, r["name"], False, b"", psk, keys["rs"] if M.needs(f["pattern"], False)[0] else None, keys["re"],
                        M.dh_base(keys["is"]) if pre_i else None)
        for _ in range(r["messages_done"]):
            w, rd = (ini, res) if ini.action == M.ACTION_WRITE else (res, ini)
            assert rd.read(w.write(b"abc")) == b"abc"
        initiator = r["role"] == M.ROLE_INITIATOR
        got = F.check(ini if initiator else res, psk, None if initiator else keys["re"])
        want = r["fallback_rc"] or r["start_rc"]
        assert got == want, (r, hex(got))
        codes.add(want)
    assert codes == {0, M.ERROR_NOT_APPLICABLE, F.ERROR_INVALID_STATE, F.ERROR_LOCAL_KEY_REQUIRED}
    assert len(refusals) == 20


def test_take_part_rule_and_merge_of_the_model():
    assert [s for s in STATUSES if F.eligible(s, False)] == [0, 1] and [s for s in STATUSES if F.eligible(s, True)] == [0]
    assert F.takes(1, 1, F.FALLBACK_ONLY_FAILED, False) and not F.takes(0, 1, F.FALLBACK_ONLY_FAILED, False)
    assert F.takes(0, 1, 0, True) and not F.takes(0, 0, 0, True) and not F.takes(1, 1, 0, True)
    assert not F.takes(3, 1, 0, False) and not F.takes(4, 1, 0, False) and not F.takes(5, 1, 0, False)
    a, b, h = bytes([1]) * 32, bytes([2]) * 32, bytes([3]) * 32
    c, d, g = bytes([4]) * 32, bytes([5]) * 32, bytes([6]) * 32
    assert F.merge(0, (a, b, h), 1, (c, d, g)) == (b, a, h, 0)
    assert F.merge(5, (a, b, h), 0, (c, d, g)) == (c, d, g, 0) and F.merge(5, (a, b, h), 3, (c, d, g))[3] == 3
    assert F.merge(1, (a, b, h), 0, (c, d, g)) == (bytes(32), bytes(32), bytes(32), 1)


# ------------------------------------------------------------ the check program

def expectations():
    out = []
    for status in STATUSES:
        for selected in (0, 1):
            for flags in (0, 1):
                for init in (0, 1):
                    out.append((status, selected, flags, init, int(F.takes(status, selected, flags, bool(init)))))
    return out


@functools.lru_cache(maxsize=None)
def run_check():
    args = [str(x) for e in expectations() for x in ("expect", *e)]
    return host_check.run_check("handshake_fallback_check", *args, timeout=300).stdout.splitlines()


def test_check_program_names_and_plan_equal_the_model():
    lines = run_check()
    names = [l.split() for l in lines if l.startswith("fbname ")]
    assert len(names) == 16
    by_id = {v: k for k, v in {**M.CIPHERS, **M.HASHES}.items()}
    for _, psk, cipher, hash_, name, length in names:
        orig = "_".join(["NoisePSK" if psk == "1" else "Noise", "IK", "25519", by_id[int(cipher, 16)], by_id[int(hash_, 16)]])
        assert name == F.fallback_name(orig) and int(length) == len(name) <= 44
    assert {n[4] for n in names} == {v["name"] for v in F.fallback_vectors()}
    got = [l for l in lines if l.startswith(("req ", "plan "))]
    assert got == F.plan_lines()
    # spelled out, so that the table is not only compared with itself: keyed before message 0 under NoisePSK alone
    assert "plan XXfallback I Noise 0 W keyed_in=0 steps=e,ee:e.e,s+aead,se:s.e,p+aead overhead=96 next=read" in got
    assert "plan XXfallback R NoisePSK 0 R keyed_in=1 steps=e+mk,ee:e.e,s+aead,se:e.s,p+aead overhead=96 next=write" in got
    assert "plan XXfallback R Noise 1 W keyed_in=1 steps=s+aead,es:s.e,p+aead overhead=64 next=split" in got
    assert [l.split()[1] for l in lines if l.startswith("from ") and l.endswith(" 1")] == list(F.FALLBACK_FROM)
    assert len([l for l in lines if l.startswith("from ")]) == len(M.PATTERNS)
    merges = {int(l.split()[1]): l.split()[2] for l in lines if l.startswith("merge ")}
    assert merges == {s: ("take" if s == 0 else "keep" if s == 5 else "zero") for s in STATUSES}


def test_check_program_rules_under_sanitizers():
    last = run_check()[-1].split()
    assert last[0] == "handshake_fallback_check:" and last[-1] == "failures"
    assert int(last[1]) == len(expectations()) == 72 and int(last[3]) > 100000 and last[5] == "0", last


def test_check_program_reports_a_wrong_expectation():
    status, selected, flags, init, want = next(e for e in expectations() if e[:4] == (1, 1, 1, 0))
    assert want == 1
    r = host_check.run_check("handshake_fallback_check", "expect", "1", "1", "1", "0", "0", checked=False)
    assert r.returncode == 1 and "FAIL expect: 1 1 1 0" in r.stderr, r.stdout + r.stderr
    assert r.stdout.split()[-2] == "1"
    r = host_check.run_check("handshake_fallback_check", "something else", checked=False)
    assert r.returncode == 1 and "FAIL argument" in r.stderr


# ------------------------------------------------------------ through the library

P = 0x10000  # a device pointer that is never dereferenced: n == 0 launches nothing


def new(A, name, initiator, static=True):
    kw = dict(local_ephemeral=P, remote_static=P, psk=P)
    if static:
        kw["local_static"] = P
    rc, hs = A.dev_handshake_new(name, A.ROLE_INITIATOR if initiator else A.ROLE_RESPONDER, 0, **kw)
    assert rc == 0 and hs, (name, hex(rc))
    return hs


def advance(A, pair, count):
    """`count` messages between two n == 0 objects"""
    for _ in range(count):
        w, r = pair if A.dev_handshake_get_action(pair[0]) == A.ACTION_WRITE_MESSAGE else pair[::-1]
        over = A.dev_handshake_overhead(w)
        assert A.dev_handshake_write_message(w, payload_len=0, msg=0, msg_stride=0) == 0
        assert A.dev_handshake_read_message(r, msg=0, msg_stride=0, msg_len=over) == 0


def pair_after(A, name, count, static=True):
    pair = (new(A, name, True, static), new(A, name, False))
    advance(A, pair, count)
    return pair


def test_argument_rules_through_the_library(aead):
    """Every row of the header's list, in its order: each refusal with
    everything behind it wrong as well."""
    A = aead
    BAD, NA, STATE = A.ERROR_INVALID_PARAM, A.ERROR_NOT_APPLICABLE, A.ERROR_INVALID_STATE
    KEY, PSK = A.ERROR_LOCAL_KEY_REQUIRED, A.ERROR_PSK_REQUIRED
    worst = dict(prologue=0, prologue_len=9, prologue_stride=3, psk=0, psk_stride=7, local_ephemeral=0,
                 local_ephemeral_stride=7, flags=6)
    good = dict(prologue=P, prologue_len=9, prologue_stride=0, psk=P, psk_stride=32, local_ephemeral=P,
                local_ephemeral_stride=32, select=P, flags=A.FALLBACK_ONLY_FAILED)
    made = []
    # 1. NULL hs, cfg or fb, on objects that are wrong in every other way
    nn = pair_after(A, "NoisePSK_NN_25519_ChaChaPoly_BLAKE2s", 0)
    made += nn
    assert A.dev_handshake_fallback(0, **worst) == (BAD, None)
    assert A.dev_handshake_fallback(nn[1], no_cfg=True) == (BAD, None)
    assert A.dev_handshake_fallback(nn[1], no_out=True, **worst) == (BAD, None)
    # 2. the pattern, before the state and the keys
    for name in ("NoisePSK_NN_25519_ChaChaPoly_BLAKE2s", "Noise_XX_25519_AESGCM_SHA512", "Noise_IX_25519_AESGCM_SHA256",
                 "Noise_KN_25519_AESGCM_SHA256", "Noise_N_25519_AESGCM_SHA256", "Noise_K_25519_ChaChaPoly_BLAKE2b"):
        for count in (0, 1):
            pair = pair_after(A, name, count)
            made += pair
            for hs in pair:
                assert A.dev_handshake_fallback(hs, **worst) == (NA, None), (name, count)
                assert A.dev_handshake_fallback(hs, **good) == (NA, None), (name, count)
    # 3. exactly one message done, before the keys
    for name, counts in (("NoisePSK_IK_25519_ChaChaPoly_BLAKE2s", (0, 2)), ("NoisePSK_XK_25519_AESGCM_SHA512", (0, 2, 3)),
                         ("Noise_KK_25519_AESGCM_SHA512", (0, 2)), ("Noise_NK_25519_ChaChaPoly_SHA256", (0, 2))):
        for count in counts:
            pair = pair_after(A, name, count, static=False if "_NK_" in name else True)
            made += pair
            for hs in pair:
                assert A.dev_handshake_fallback(hs, **worst) == (STATE, None), (name, count)
                assert A.dev_handshake_fallback(hs, **good) == (STATE, None), (name, count)
    # and after the split
    ik = pair_after(A, "Noise_IK_25519_ChaChaPoly_BLAKE2s", 2)
    made += ik
    for hs in ik:
        assert A.dev_handshake_split(hs, k1=0, k2=0) == 0
        assert A.dev_handshake_fallback(hs, **good) == (STATE, None)
    # 4. the static key of the side that falls back, a former responder's fresh ephemeral; before the PSK
    nk = pair_after(A, "NoisePSK_NK_25519_ChaChaPoly_BLAKE2s", 1, static=False)
    made += nk
    assert A.dev_handshake_fallback(nk[0], **worst) == (KEY, None)
    assert A.dev_handshake_fallback(nk[0], **good) == (KEY, None)  # the NK initiator has no static key
    assert A.dev_handshake_fallback(nk[1], **worst) == (KEY, None)
    assert A.dev_handshake_fallback(nk[1], **{**good, "local_ephemeral": 0}) == (KEY, None)
    # 5. the PSK, before the prologue and the strides
    assert A.dev_handshake_fallback(nk[1], **{**worst, "local_ephemeral": P}) == (PSK, None)
    assert A.dev_handshake_fallback(nk[1], **{**good, "psk": 0}) == (PSK, None)
    ik = pair_after(A, "NoisePSK_IK_25519_AESGCM_SHA512", 1)
    made += ik
    assert A.dev_handshake_fallback(ik[0], **worst) == (PSK, None)  # a former initiator brings no ephemeral
    assert A.dev_handshake_fallback(ik[1], **{**worst, "local_ephemeral": P}) == (PSK, None)
    # 6. the prologue and stride rules of _new, and the flags
    for hs, initiator in ((ik[0], True), (ik[1], False)):
        for change in (dict(prologue=0), dict(prologue_stride=8), dict(psk_stride=31), dict(flags=2), dict(flags=3)):
            assert A.dev_handshake_fallback(hs, **{**good, **change}) == (BAD, None), change
        rc, fb = A.dev_handshake_fallback(hs, **{**good, "local_ephemeral_stride": 31})
        assert rc == (0 if initiator else BAD), "only a former responder's ephemeral is read"
        if fb:
            assert A.dev_handshake_free(fb) == 0
    # a refused call left hs as it was: the call now goes through, on both ends, with n == 0
    assert A.dev_handshake_get_action(ik[0]) == A.ACTION_READ_MESSAGE
    assert A.dev_handshake_get_action(ik[1]) == A.ACTION_WRITE_MESSAGE
    rc, fi = A.dev_handshake_fallback(ik[0], **{**good, "prologue": 0, "prologue_len": 0, "local_ephemeral": 0, "select": 0, "flags": 0})
    assert rc == 0 and fi
    rc, fr = A.dev_handshake_fallback(ik[1], **good)
    assert rc == 0 and fr
    made += [fi, fr]
    assert A.dev_handshake_get_action(fr) == A.ACTION_WRITE_MESSAGE and A.dev_handshake_get_action(fi) == A.ACTION_READ_MESSAGE
    assert A.dev_handshake_status(fr) == 0  # n == 0 owns nothing
    # a fallback never falls back again; hs goes on as it was
    assert A.dev_handshake_fallback(fr, **good) == (NA, None) and A.dev_handshake_fallback(fi, **good) == (NA, None)
    assert A.dev_handshake_get_action(ik[0]) == A.ACTION_READ_MESSAGE
    # the merge before fb's split, then fb's messages, split and merge
    merge = dict(hs_status=P, k1=P, k2=P, fb_k1=P, fb_k2=P, h=P, fb_h=P, status=P)
    assert A.dev_handshake_fallback_merge(fr, **merge) == STATE
    assert A.dev_handshake_fallback_merge(fr, **{**merge, "k1": 0}) == BAD  # a NULL pointer before the state
    assert [A.dev_handshake_overhead(x) for x in (fr, fi)] == [96, 96]
    advance(A, (fr, fi), 1)
    assert [A.dev_handshake_overhead(x) for x in (fr, fi)] == [64, 64]
    assert A.dev_handshake_fallback(fr, **good) == (NA, None)
    advance(A, (fr, fi), 1)
    for fb in (fr, fi):
        assert A.dev_handshake_get_action(fb) == A.ACTION_SPLIT
        assert A.dev_handshake_fallback_merge(fb, **merge) == STATE
        assert A.dev_handshake_split(fb, k1=0, k2=0) == 0
        assert A.dev_handshake_fallback_merge(fb, **merge) == 0
        assert A.dev_handshake_fallback_merge(fb, **{**merge, "h": 0, "fb_h": 0}) == 0
        for k in merge:
            assert A.dev_handshake_fallback_merge(fb, **{**merge, k: 0}) == BAD, k
    assert A.dev_handshake_fallback_merge(0, **merge) == BAD
    for hs in made:
        assert A.dev_handshake_free(hs) == 0


def test_xxfallback_names_are_still_refused(aead):
    A = aead
    for v in M.load_vectors("noise-c-fallback.txt.gz"):
        for role in (A.ROLE_INITIATOR, A.ROLE_RESPONDER):
            rc, hs = A.dev_handshake_new(v["name"], role, 0, local_static=P, local_ephemeral=P, remote_static=P, psk=P)
            assert (rc, hs) == (A.ERROR_NOT_APPLICABLE, None), v["name"]
    rc, hs = A.dev_handshake_new("Noise_XXfallback+hfs_25519+448_AESGCM_SHA256", A.ROLE_INITIATOR, 0, local_static=P,
                                 local_ephemeral=P)
    assert (rc, hs) == (A.ERROR_NOT_APPLICABLE, None)
    assert M.parse_name("Noise_XXfallback_25519_ChaChaPoly_BLAKE2s")[0] == M.ERROR_NOT_APPLICABLE
