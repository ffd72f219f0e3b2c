"""The host-only half of the device-resident transport sessions without a GPU.

noise-c_amd/asan/transport_check.cpp, a stand-alone program (`make -C
noise-c_amd transport_check`: g++ -fsanitize=address,undefined
-fno-sanitize-recover=all) over csrc/transport_plan.h, runs the frame walk the
kernels compile on the cases of tests/transport_model.py (each stream on a
heap buffer of exactly its length), the cap across sessions against numbering
the frames one by one, and the argument checks of noise_aead_dev_transport_*
against a byte-by-byte reading of the header comment.  It runs here as a plain
child process.  The same argument rules then go through the library itself;
no launch happens."""
import transport_model as T
from host_check import run_check


def test_model_walk_on_the_cases_spelled_out():
    """what the model itself says about the cases, from the rules alone"""
    got = {name: (len(T.walk(s, n, b)[0]),) + T.walk(s, n, b)[1:] for name, s, n, b in T.walk_cases()}
    five = sum(2 + 16 + k for k in range(5))
    want = {
        "empty": (0, 0, 0), "one byte": (0, 0, 0), "header only": (0, 0, 0),
        "header of an empty frame": (0, 0, T.ERROR_INVALID_LENGTH),
        "L=15": (0, 0, T.ERROR_INVALID_LENGTH), "L=16": (1, 18, 0), "L=17": (1, 19, 0),
        "L=15 after two": (2, 18 + 42, T.ERROR_INVALID_LENGTH),
        "L=65535 fills the stream": (1, 65537, 0), "L=65535 short by one": (0, 0, 0),
        "partial last frame, short by one": (2, 18 + 82, 0), "partial L<16 is partial": (1, 18, 0),
        "trailing byte": (1, 18, 0),
        "nonce 3 below the limit, 5 frames": (3, 18 + 19 + 20, T.ERROR_INVALID_NONCE),
        "nonce at the limit": (0, 0, T.ERROR_INVALID_NONCE),
        "nonce 1 below the limit": (1, 18, T.ERROR_INVALID_NONCE),
        "nonce 5 below the limit, 5 frames": (5, five, 0),
        "L<16 before the nonce": (1, 18, T.ERROR_INVALID_LENGTH),
        "budget cuts mid-way": (3, 18 + 19 + 20, 0), "budget 0": (0, 0, 0), "budget 0, empty stream": (0, 0, 0),
        "budget equals the frames": (5, five, 0), "budget larger": (5, five, 0),
        "budget ends at a short frame": (2, 36, T.ERROR_INVALID_LENGTH),
        "budget ends at the nonce limit": (2, 18 + 19, T.ERROR_INVALID_NONCE),
        "budget before a short frame": (1, 18, 0),
    }
    assert got == want


def test_model_cap_rule():
    assert T.cap(0, 5, 5) == (5, False) and T.cap(0, 5, 4) == (4, True) and T.cap(3, 5, 5) == (2, True)
    assert T.cap(5, 2, 5) == (0, True) and T.cap(5, 0, 5) == (0, False) and T.cap(6, 0, 5) == (0, True)
    assert T.cap(7, 3, 5) == (0, True)


def test_walk_cap_and_argument_rules_under_sanitizers():
    cases = T.walk_cases()
    r = run_check("transport_check", feed="".join(T.walk_case_line(s, n, b) for _, s, n, b in cases))
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "transport_check:" and last[2] == "walks" and last[-1] == "failures"
    assert int(last[1]) == len(cases) >= 20 and int(last[3]) > 10000 and last[5] == "0", last
    # a wrong expected value is noticed: the program does compare
    name, s, n, b = cases[10]
    frames, consumed, stop = T.walk(s, n, b)
    for wrong, word in (((len(frames) + 1, consumed, stop), "FAIL walk"), ((len(frames), consumed - 1, stop), "FAIL walk"),
                        ((len(frames), consumed, T.ERROR_INVALID_LENGTH), "FAIL walk")):
        r = run_check("transport_check", feed=T.walk_case_line(s, n, b, wrong), checked=False)
        assert r.returncode == 1 and word in r.stderr, r.stdout + r.stderr
        assert "transport_check: 1 walks" in r.stdout and r.stdout.split()[-2] == "1"
    # and a line it cannot read is a failure, not a skipped case
    r = run_check("transport_check", feed="zz 0 0 0 0 0\n", checked=False)
    assert r.returncode == 1 and "FAIL input" in r.stderr, r.stdout + r.stderr


def test_transport_argument_rules_through_the_library(aead):
    """Validation before any launch (no GPU work), on never-dereferenced pointers."""
    A = aead
    ok_new = dict(k1=0x10000, k2=0x20000, max_frames=64)

    def new(cipher=A.CHACHAPOLY, role=A.ROLE_INITIATOR, n=4, **kw):
        rc, tr = A.dev_transport_new(cipher, role, n, **{**ok_new, **kw})
        assert rc != 0 and tr is None
        return rc

    # the order: the cipher, the role, the pointers, max_frames
    for cipher in (0, 0x4300, 0x4303, 0x4803):
        assert new(cipher=cipher) == A.ERROR_UNKNOWN_ID
        assert new(cipher=cipher, role=0, k1=0, max_frames=0) == A.ERROR_UNKNOWN_ID
    for cipher in (A.CHACHAPOLY, A.AESGCM):
        for role in (0, 0x5200, 0x5203, 1):
            assert new(cipher=cipher, role=role) == A.ERROR_INVALID_PARAM
        for role in (A.ROLE_INITIATOR, A.ROLE_RESPONDER):
            assert new(cipher=cipher, role=role, k1=0) == A.ERROR_INVALID_PARAM
            assert new(cipher=cipher, role=role, k2=0) == A.ERROR_INVALID_PARAM
            assert new(cipher=cipher, role=role, n=0, k1=0) == A.ERROR_INVALID_PARAM
            assert new(cipher=cipher, role=role, max_frames=0) == A.ERROR_INVALID_PARAM
            assert new(cipher=cipher, role=role, max_frames=2 ** 31 + 1) == A.ERROR_INVALID_PARAM
            assert new(cipher=cipher, role=role, n=2 ** 32 - 1, max_frames=2 ** 32 - 1) == A.ERROR_INVALID_PARAM
    assert A.lib().noise_aead_dev_transport_new(None, A.CHACHAPOLY, A.ROLE_INITIATOR, 4, 0x10000, 0x20000, 64,
                                                None) == A.ERROR_INVALID_PARAM
    assert A.lib().noise_aead_dev_transport_new(None, 0, A.ROLE_INITIATOR, 4, 0x10000, 0x20000, 64,
                                                None) == A.ERROR_UNKNOWN_ID
    assert A.dev_transport_free(None) == A.ERROR_INVALID_PARAM
    assert A.dev_transport_nonces(None, 0) == 0 and A.dev_transport_nonces(None, 1) == 0

    # an n == 0 object: valid (max_frames is not looked at), owns nothing, and its calls check their pointers
    for cipher, role, m in ((A.CHACHAPOLY, A.ROLE_INITIATOR, 0), (A.AESGCM, A.ROLE_RESPONDER, 2 ** 32 - 1)):
        rc, tr = A.dev_transport_new(cipher, role, 0, k1=0x10000, k2=0x20000, max_frames=m)
        assert rc == 0 and tr
        assert [A.dev_transport_nonces(tr, d) for d in (0, 1, 2, -1)] == [0, 0, 0, 0]
        ok = dict(wire=0x90000, off=0x1000, length=0x2000, result=0x3000)
        for call in (A.dev_transport_seal_frames, A.dev_transport_open_frames, A.dev_transport_echo_frames):
            assert call(tr, **ok) == A.ERROR_NONE
            assert call(tr, **{**ok, "result": 0x1000}) == A.ERROR_NONE  # empty ranges meet nothing
            for k in ok:
                assert call(tr, **{**ok, k: 0}) == A.ERROR_INVALID_PARAM, k
            assert call(None, **ok) == A.ERROR_INVALID_PARAM
        assert A.dev_transport_free(tr) == A.ERROR_NONE
