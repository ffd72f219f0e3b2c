"""Sessions that change their object, without a GPU (include/noise_aead_hip.h
section 16).

The model of tests/handshake_move_model.py on its own;
noise-c_amd/asan/handshake_move_check.cpp, the host-only half of
csrc/handshake_plan.h under ASan/UBSan, against the model; and the argument
rules of _new_like, _move and _drop through the library on n == 0 objects,
which launch nothing."""
import functools

import handshake_model as M
import handshake_move_model as V
import host_check

STATUSES = list(range(6))


# ------------------------------------------------------------ the model

def test_rule_of_the_model_reads_as_the_table():
    assert V.move_rule(False, True, 0, 5) == V.RANGE and V.move_rule(True, False, 0, 5) == V.RANGE
    assert V.move_rule(False, False, 5, 0) == V.RANGE, "the range before the statuses"
    assert V.move_rule(True, True, 5, 0) == V.EMPTY, "an empty source before a taken destination"
    assert V.move_rule(True, True, 5, 5) == V.EMPTY
    assert [V.move_rule(True, True, 0, d) for d in STATUSES] == [V.TAKEN] * 5 + [V.MOVED]
    assert [V.move_rule(True, True, s, 5) for s in STATUSES] == [V.MOVED] * 5 + [V.EMPTY], "a failed session moves"
    assert (V.MOVED, V.EMPTY, V.TAKEN, V.RANGE) == (0, 1, 2, 3)


class Stub:
    """a session as far as move and drop look at it"""

    def __init__(self, tag, status=0):
        self.tag, self.status = tag, status


def test_move_and_drop_of_the_model():
    src = V.Obj(4, "here", [Stub("a"), Stub("b", 1), Stub("c")])
    dst = V.Obj(3, "here", [Stub("x", 3)])
    assert src.status() == [0, 1, 0, 5] and dst.status() == [3, 5, 5]
    got = V.move(dst, [0, 1, 2, 3, 1], src, [0, 1, 3, 2, 4], 5)
    assert got == [V.TAKEN, V.MOVED, V.EMPTY, V.RANGE, V.RANGE]
    assert [s and s.tag for s in src.lanes] == ["a", None, "c", None]
    assert [s and s.tag for s in dst.lanes] == ["x", "b", None] and dst.status() == [3, 1, 5]
    assert V.move(dst, None, src, [2, 0, 3], 3) == [V.TAKEN, V.TAKEN, V.EMPTY]
    V.drop(dst, [0, 7])
    assert dst.status() == [5, 1, 5]
    assert V.move(dst, None, src, None, 1) == [V.MOVED] and dst.lanes[0].tag == "a" and src.status() == [5, 5, 0, 5]
    like = V.Obj.like(dst, 2)
    assert like.position == "here" and like.status() == [5, 5]


def test_position_of_a_model_session(oracle):
    key = bytes(range(32))
    a = M.Session(oracle, "Noise_XX_25519_ChaChaPoly_BLAKE2s", False, b"", None, key, key)
    b = M.Session(oracle, "Noise_XX_25519_ChaChaPoly_BLAKE2s", False, b"p", None, key[::-1], key)
    assert V.position_of(a) == V.position_of(b), "keys and prologue are the session's, not the position's"
    c = M.Session(oracle, "Noise_XX_25519_ChaChaPoly_BLAKE2s", True, b"", None, key, key)
    assert V.position_of(a) != V.position_of(c)
    b.read(c.write(b""))
    assert V.position_of(a) != V.position_of(b) and V.position_of(b)[5:] == (1, False, 0)
    b.write(b"")
    assert V.position_of(b)[5:] == (2, True, 1), "after <- e, ee, s, es: the key of es, and one nonce of it spent"


# ------------------------------------------------------------ the check program

def expectations():
    return [(si, di, ss, ds, V.move_rule(bool(si), bool(di), ss, ds))
            for si in (0, 1) for di in (0, 1) for ss in STATUSES for ds in STATUSES]


@functools.lru_cache(maxsize=None)
def run_check():
    args = [str(x) for e in expectations() for x in ("expect", *e)]
    return host_check.run_check("handshake_move_check", *args, timeout=300).stdout.splitlines()


def test_check_program_rule_equals_the_model():
    rules = [tuple(int(x) for x in l.split()[1:]) for l in run_check() if l.startswith("rule ")]
    assert rules == expectations() and len(rules) == 144
    assert {r[4] for r in rules} == {0, 1, 2, 3}


def test_check_program_position_predicate():
    """two positions that differ in exactly one field are not the same, whichever field"""
    got = {l.split()[1]: int(l.split()[2]) for l in run_check() if l.startswith("position ")}
    fields = ("pattern", "cipher", "hash", "psk", "fallback", "role", "action", "index", "keyed", "nonce")
    assert got == {**{f: 0 for f in fields}, "none": 1}


def test_check_program_rules_under_sanitizers():
    last = run_check()[-1].split()
    assert last[0] == "handshake_move_check:" and last[-1] == "failures"
    assert int(last[1]) == len(expectations()) == 144 and int(last[3]) > 250000 and last[5] == "0", last


def test_check_program_reports_a_wrong_expectation():
    assert V.move_rule(True, True, 1, 5) == V.MOVED
    r = host_check.run_check("handshake_move_check", "expect", "1", "1", "1", "5", "2", checked=False)
    assert r.returncode == 1 and "FAIL expect: 1 1 1 5" in r.stderr, r.stdout + r.stderr
    assert r.stdout.split()[-2] == "1"
    r = host_check.run_check("handshake_move_check", "something else", checked=False)
    assert r.returncode == 1 and "FAIL argument" in r.stderr


# ------------------------------------------------------------ through the library

P = 0x10000  # a device pointer that is never dereferenced: n == 0 launches nothing


def new(A, name, initiator, made, **change):
    kw = dict(local_static=P, local_ephemeral=P, remote_static=P, psk=P)
    kw.update(change)
    rc, hs = A.dev_handshake_new(name, A.ROLE_INITIATOR if initiator else A.ROLE_RESPONDER, 0, **kw)
    assert rc == 0 and hs, (name, hex(rc))
    made.append(hs)
    return hs


def like(A, hs, made, capacity=0):
    rc, out = A.dev_handshake_new_like(hs, capacity)
    assert rc == 0 and out, hex(rc)
    made.append(out)
    return out


def step(A, w, r):
    """one message between two n == 0 objects"""
    over = A.dev_handshake_overhead(w)
    assert A.dev_handshake_write_message(w, payload_len=0, msg=0, msg_stride=0) == 0
    assert A.dev_handshake_read_message(r, msg=0, msg_stride=0, msg_len=over) == 0


def test_argument_rules_through_the_library(aead):
    """Every row of the header's lists, in their order: each refusal with
    everything behind it wrong as well."""
    A = aead
    BAD, STATE, NA = A.ERROR_INVALID_PARAM, A.ERROR_INVALID_STATE, A.ERROR_NOT_APPLICABLE
    XX = "Noise_XX_25519_ChaChaPoly_BLAKE2s"
    made = []
    ini, res = new(A, XX, True, made), new(A, XX, False, made)

    # ---- _new_like: NULL out or like, then the state
    assert A.dev_handshake_new_like(0, 4) == (BAD, None)
    assert A.dev_handshake_new_like(res, 4, no_out=True) == (BAD, None)
    pool = like(A, res, made)
    assert A.dev_handshake_get_action(pool) == A.ACTION_READ_MESSAGE and A.dev_handshake_overhead(pool) == 32
    assert A.dev_handshake_status(pool) == 0 and A.dev_handshake_remote_static(pool) == 0  # no lanes own nothing

    # ---- _move
    # 1. a NULL object, with everything behind it wrong
    assert A.dev_handshake_move(0, ini, 9, result=P, dst_lanes=P) == BAD
    assert A.dev_handshake_move(ini, 0, 9, result=P, dst_lanes=P) == BAD
    # 2. one object as both, at a position that is no position to move at
    assert A.dev_handshake_move(pool, pool, 0) == BAD
    # 3. the position, before the keys: the role, the index, the name
    assert A.dev_handshake_move(pool, ini, 0) == STATE
    other = new(A, "Noise_XX_25519_ChaChaPoly_SHA256", False, made)
    assert A.dev_handshake_move(pool, other, 0) == STATE
    psk = new(A, "NoisePSK_XX_25519_ChaChaPoly_BLAKE2s", False, made)
    assert A.dev_handshake_move(pool, psk, 0) == STATE
    shared = new(A, XX, False, made, local_static_stride=0)  # once for all: rule 4 alone would refuse it
    step(A, ini, shared)
    assert A.dev_handshake_move(pool, shared, 0) == STATE  # one message ahead
    # 4. the keys: dst from _new holds its per-session keys in the caller's rows
    assert A.dev_handshake_move(res, pool, 0) == BAD
    assert A.dev_handshake_move(pool, res, 0) == 0  # 5. m == 0, before the lists
    shared0 = new(A, XX, False, made, local_static_stride=0)
    assert A.dev_handshake_move(pool, shared0, 0) == BAD  # per session against once for all
    pool0 = like(A, shared0, made)
    assert A.dev_handshake_move(pool0, shared0, 0) == 0  # once for all through the same pointer
    elsewhere = new(A, XX, False, made, local_static=P + 64, local_static_stride=0)
    assert A.dev_handshake_move(pool0, elsewhere, 0) == BAD  # ... and through another
    assert A.dev_handshake_move(like(A, pool0, made), elsewhere, 0) == BAD  # the pointer is handed on
    nokey = new(A, "Noise_NN_25519_ChaChaPoly_BLAKE2s", False, made, local_static=0)
    withkey = new(A, "Noise_NN_25519_ChaChaPoly_BLAKE2s", False, made)
    assert A.dev_handshake_move(like(A, withkey, made), nokey, 0) == BAD  # held against never had
    assert A.dev_handshake_move(like(A, nokey, made), nokey, 0) == 0
    # 6. a NULL list with m above that object's n (here 0), before 7
    assert A.dev_handshake_move(pool, res, 1, result=P) == BAD
    assert A.dev_handshake_move(pool, res, 1, dst_lanes=P, result=P) == BAD
    assert A.dev_handshake_move(pool, res, 1, src_lanes=P, result=P) == BAD
    # 7. d_result meeting a list
    assert A.dev_handshake_move(pool, res, 2, dst_lanes=P, src_lanes=P + 64, result=P + 7) == BAD
    assert A.dev_handshake_move(pool, res, 2, dst_lanes=P, src_lanes=P + 64, result=P + 65) == BAD
    # two objects at the end of their messages may move; after the split nothing does
    a, b = new(A, "Noise_NN_25519_ChaChaPoly_BLAKE2s", True, made), new(A, "Noise_NN_25519_ChaChaPoly_BLAKE2s", False, made)
    step(A, a, b)
    step(A, b, a)
    cohort = like(A, b, made)
    assert A.dev_handshake_get_action(cohort) == A.ACTION_SPLIT and A.dev_handshake_move(cohort, b, 0) == 0
    assert A.dev_handshake_split(b, k1=0, k2=0) == 0
    assert A.dev_handshake_move(cohort, b, 0) == STATE and A.dev_handshake_new_like(b, 1) == (STATE, None)
    assert A.dev_handshake_split(cohort, k1=0, k2=0) == 0
    assert A.dev_handshake_move(cohort, b, 0) == STATE, "both complete: the same position, and none to move at"
    # a refused call left the objects as they were
    assert A.dev_handshake_get_action(pool) == A.ACTION_READ_MESSAGE and A.dev_handshake_get_action(res) == A.ACTION_READ_MESSAGE

    # ---- _drop: as _clear_keys
    assert A.dev_handshake_drop(0, lanes=0, m=3) == BAD
    assert A.dev_handshake_drop(pool, lanes=0, m=0) == 0 and A.dev_handshake_drop(res, lanes=0, m=0) == 0
    assert A.dev_handshake_drop(pool, lanes=P, m=1) == BAD  # m > n
    assert A.dev_handshake_drop(pool, lanes=0, m=1) == BAD

    # ---- _fallback of an object made by _new_like, where the object it was made like falls back
    IK = "Noise_IK_25519_ChaChaPoly_BLAKE2s"
    ii, ir = new(A, IK, True, made), new(A, IK, False, made)
    step(A, ii, ir)
    for hs in (ii, ir):
        assert A.dev_handshake_fallback(like(A, hs, made), local_ephemeral=P) == (NA, None)
        assert A.dev_handshake_fallback(like(A, hs, made), no_cfg=True) == (BAD, None)
        rc, fb = A.dev_handshake_fallback(hs, local_ephemeral=P)
        assert rc == 0 and fb
        made.append(fb)
        # a cohort of a fallback object: an ordinary object at the fallback's position
        cohort = like(A, fb, made)
        assert A.dev_handshake_overhead(cohort) == 96 and A.dev_handshake_move(cohort, fb, 0) == 0
        assert A.dev_handshake_move(cohort, like(A, hs, made), 0) == STATE
    for hs in made:
        assert A.dev_handshake_free(hs) == 0
