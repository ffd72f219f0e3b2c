"""The session table's host-only half without a GPU (header section 10).

The model of tests/transport_table_model.py against tests/transport_model.py;
noise-c_amd/asan/transport_table_check.cpp, a stand-alone program (`make -C
noise-c_amd transport_table_check`: g++ -fsanitize=address,undefined
-fno-sanitize-recover=all) over csrc/transport_plan.h, as a plain child
process: the slot of a call's entry on heap lists of exactly their length, and
the new argument checks against a byte-by-byte reading of the header; then the
same argument rules through the library itself, on never-dereferenced
pointers.  No launch happens."""
import numpy as np

import transport_model as T
import transport_table_model as M
from host_check import run_check


def _sessions(oracle, cipher, n, dead):
    rng = np.random.default_rng(11)
    keys = [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
            for _ in range(n)]
    return [None if i in dead else T.Session.of_role(oracle, cipher, True, *keys[i]) for i in range(n)], keys


def _streams(n):
    rng = np.random.default_rng(12)
    return [b"".join(T.frame(rng.integers(0, 256, 16 + 3 * k, dtype=np.uint8).tobytes() + bytes(16)) for k in range(1 + j % 3))
            for j in range(n)]


def test_splice_equals_a_batch_with_empty_streams(oracle):
    """An entry taken out (unkeyed, or out of range) is, for every other entry,
    an entry with an empty stream: it takes no frame numbers.  Caps that cut
    before, at and after a removed entry, and none."""
    n, dead = 9, {2, 5}
    slots = [7, 2, 0, 99, 5, 8, 3, 2 ** 32 - 1, 1]  # two unkeyed, two out of range, unsorted
    streams = _streams(len(slots))  # the removed entries' streams are full of frames
    removed = [j for j, i in enumerate(slots) if i >= n or i in dead]
    assert removed == [1, 3, 4, 7]
    counts = [0 if j in removed else 1 + j % 3 for j in range(len(slots))]
    total = sum(counts)
    # the frame numbers at which entries 1, 3/4 and 7 stand
    at = [sum(counts[:j]) for j in range(len(slots))]
    caps = sorted({1, at[1] - 1, at[1], at[1] + 1, at[3] - 1, at[3], at[3] + 1, at[7], at[7] + 1, total - 1, total, total + 5})
    assert at[1] == 1 and at[3] == 4 and at[3] == at[4]
    for cipher in (T.CHACHAPOLY, T.AESGCM):
        for mode in ("seal", "open", "echo"):
            for cap in caps:
                if cap < 1:
                    continue
                sess, keys = _sessions(oracle, cipher, n, dead)
                twin = [T.Session.of_role(oracle, cipher, True, *keys[i]) if i < n else
                        T.Session(oracle, cipher, bytes(32), bytes(32)) for i in slots]
                got = M.run_table(sess, mode, streams, cap, slots)
                want = T.run_batch(twin, mode, [b"" if j in removed else s for j, s in enumerate(streams)], cap)
                for j, i in enumerate(slots):
                    if j in removed:
                        code = M.ERROR_INVALID_PARAM if i >= n else M.ERROR_INVALID_STATE
                        assert got[j] == (streams[j], (0, 0, code), {}), (cipher, mode, cap, j)
                        assert want[j][1][0] == 0  # and the empty stream took no numbers either
                    else:
                        assert got[j] == want[j], (cipher, mode, cap, j)
                        assert (sess[i].send, sess[i].recv) == (twin[j].send, twin[j].recv)
    # without a list: entry j is slot j
    sess, keys = _sessions(oracle, T.CHACHAPOLY, n, dead)
    got = M.run_table(sess, "seal", _streams(n), 7)
    assert [g[1][2] for g in got] == [M.ERROR_INVALID_STATE if i in dead else 0 for i in range(n)]
    assert sum(g[1][0] for g in got) == 7


def test_slots_and_argument_rules_under_sanitizers():
    r = run_check("transport_table_check")
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "transport_table_check:" and last[2] == "checks" and last[4] == "failures"
    assert int(last[1]) > 10000 and last[3] == "0", last
    # an expectation of ours that holds, and wrong ones: the program does compare
    r = run_check("transport_table_check", "expect", "67", "66", "1", "expect", "67", "67", "0", "expect", "67", str(2 ** 32 - 1), "0",
                  checked=False)
    assert r.returncode == 0 and r.stdout.split()[-2] == "0", r.stdout + r.stderr
    for wrong in (("67", "67", "1"), ("67", "66", "0"), ("67", str(2 ** 32 - 1), "1")):
        r = run_check("transport_table_check", "expect", *wrong, checked=False)
        assert r.returncode == 1 and "FAIL expect" in r.stderr, r.stdout + r.stderr
        assert r.stdout.split()[-2] == "1"
    r = run_check("transport_table_check", "something else", checked=False)
    assert r.returncode == 1 and "FAIL argument" in r.stderr


def test_table_argument_rules_through_the_library(aead):
    """Validation before any launch (no GPU work), in the stated order, on n == 0
    objects from both constructors and never-dereferenced pointers."""
    A = aead
    BAD, OK = A.ERROR_INVALID_PARAM, A.ERROR_NONE

    def unkeyed(cipher=A.CHACHAPOLY, role=A.ROLE_INITIATOR, n=4, max_frames=64):
        rc, tr = A.dev_transport_new_unkeyed(cipher, role, n, max_frames=max_frames)
        assert rc != 0 and tr is None
        return rc

    # _new_unkeyed: the cipher, the role, the pointer, max_frames
    for cipher in (0, 0x4300, 0x4303):
        assert unkeyed(cipher=cipher) == A.ERROR_UNKNOWN_ID
        assert unkeyed(cipher=cipher, role=0, max_frames=0) == A.ERROR_UNKNOWN_ID
    for cipher in (A.CHACHAPOLY, A.AESGCM):
        for role in (0, 0x5203, 1):
            assert unkeyed(cipher=cipher, role=role) == BAD
            assert unkeyed(cipher=cipher, role=role, max_frames=0) == BAD
        for role in (A.ROLE_INITIATOR, A.ROLE_RESPONDER):
            assert unkeyed(cipher=cipher, role=role, max_frames=0) == BAD
            assert unkeyed(cipher=cipher, role=role, max_frames=2 ** 31 + 1) == BAD
            assert unkeyed(cipher=cipher, role=role, n=2 ** 32 - 1, max_frames=2 ** 32 - 1) == BAD
    L = A.lib()
    assert L.noise_aead_dev_transport_new_unkeyed(None, A.CHACHAPOLY, A.ROLE_INITIATOR, 4, 64, None) == BAD
    assert L.noise_aead_dev_transport_new_unkeyed(None, 0, A.ROLE_INITIATOR, 4, 64, None) == A.ERROR_UNKNOWN_ID
    assert L.noise_aead_dev_transport_new_unkeyed(None, A.AESGCM, 0, 0, 0, None) == BAD

    frame_calls = (A.dev_transport_seal_frames_of, A.dev_transport_open_frames_of, A.dev_transport_echo_frames_of)
    ok_of = dict(slots=0x4000, wire=0x90000, off=0x1000, length=0x2000, result=0x3000)
    ok_set = dict(slots=0x4000, k1=0x10000, k2=0x20000)

    # a NULL object comes first, before m == 0
    for m in (0, 1):
        assert A.dev_transport_set_keys(None, m=m, **ok_set) == BAD
        assert A.dev_transport_clear_keys(None, slots=0x4000, m=m) == BAD
        for call in frame_calls:
            assert call(None, m=m, **ok_of) == BAD
    assert A.dev_transport_has_key(None) == 0 and A.debug_transport_ctx(None, 0) == (0, 0)

    # n == 0 objects from both constructors: valid, own nothing; m == 0 is fine whatever else is given, m > 0 is m > n
    made = [A.dev_transport_new_unkeyed(A.CHACHAPOLY, A.ROLE_INITIATOR, 0, max_frames=0),
            A.dev_transport_new_unkeyed(A.AESGCM, A.ROLE_RESPONDER, 0, max_frames=2 ** 32 - 1),
            A.dev_transport_new(A.AESGCM, A.ROLE_INITIATOR, 0, k1=0x10000, k2=0x20000, max_frames=0)]
    for rc, tr in made:
        assert rc == 0 and tr
        assert A.dev_transport_has_key(tr) == 0 and A.dev_transport_nonces(tr, 0) == 0
        assert [A.debug_transport_ctx(tr, d)[0] for d in (0, 1, 2, -1)] == [0, 0, 0, 0]
        assert A.dev_transport_set_keys(tr, m=0, **ok_set) == OK
        assert A.dev_transport_set_keys(tr, m=0, slots=0, k1=0, k2=0) == OK  # m == 0 before the pointers
        assert A.dev_transport_set_keys(tr, m=1, **ok_set) == BAD            # m > n
        assert A.dev_transport_set_keys(tr, m=1, **ok_set, status=0x5000) == BAD
        assert A.dev_transport_clear_keys(tr, slots=0, m=0) == OK
        assert A.dev_transport_clear_keys(tr, slots=0x4000, m=1) == BAD
        for call in frame_calls:
            assert call(tr, m=0, **ok_of) == OK
            assert call(tr, m=0, max_frames=2 ** 32 - 1, slots=0, wire=0, off=0, length=0, result=0) == OK
            assert call(tr, m=0, **{**ok_of, "result": 0x1000}) == OK
            assert call(tr, m=1, **ok_of) == BAD
            assert call(tr, m=2 ** 32 - 1, **ok_of) == BAD
        # the calls of section 9 on it are what they were
        assert A.dev_transport_seal_frames(tr, wire=0x90000, off=0x1000, length=0x2000, result=0x3000) == OK
        assert A.dev_transport_seal_frames(tr, wire=0x90000, off=0x1000, length=0x2000, result=0) == BAD
        assert A.dev_transport_free(tr) == OK
