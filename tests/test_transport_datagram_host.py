"""Datagram transport's host-only half without a GPU (header section 11).

noise-c_amd/asan/transport_datagram_check.cpp, a stand-alone program (`make -C
noise-c_amd transport_datagram_check`: g++ -fsanitize=address,undefined
-fno-sanitize-recover=all) over csrc/transport_plan.h, as a plain child
process: the anti-replay window the kernels run against a set of counters, the
24-byte walk on heap buffers of exactly their length, and the argument checks
against a byte-by-byte reading of the header; then the same argument order
through the library itself, on n == 0 objects and never-dereferenced pointers.
No launch happens."""
import transport_datagram_model as D
from host_check import run_check


def test_window_walk_and_argument_rules_under_sanitizers():
    r = run_check("transport_datagram_check")
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "transport_datagram_check:" and last[2] == "checks" and last[4] == "failures"
    assert int(last[1]) > 100000 and last[3] == "0", last
    # expectations of ours from the model, around the window's lower edge and at the ends: the program agrees
    cases = []
    for accepted, counter in ((2000, 977), (2000, 976), (2000, 2000), (2000, 2001), (2000, 1999), (5, 0), (2 ** 64 - 2, 2 ** 64 - 1),
                              (2 ** 64 - 2, 2 ** 64 - 1026), (2 ** 64 - 2, 2 ** 64 - 1025), (0, 0), (2 ** 40, 2 ** 40 - 1023)):
        w = D.Window()
        w.accept(accepted)
        cases.append((str(accepted), str(counter), "1" if w.check(counter) else "0"))
    assert [c[2] for c in cases] == ["1", "0", "0", "1", "1", "1", "0", "0", "1", "0", "1"]
    r = run_check("transport_datagram_check", *(x for c in cases for x in ("expect", *c)), checked=False)
    assert r.returncode == 0 and r.stdout.split()[-2] == "0", r.stdout + r.stderr
    # and wrong ones: the program does compare
    for a, c, fresh in cases[:4] + cases[6:9]:
        r = run_check("transport_datagram_check", "expect", a, c, "0" if fresh == "1" else "1", checked=False)
        assert r.returncode == 1 and "FAIL expect" in r.stderr, r.stdout + r.stderr
        assert r.stdout.split()[-2] == "1"
    r = run_check("transport_datagram_check", "something else", checked=False)
    assert r.returncode == 1 and "FAIL argument" in r.stderr


def test_datagram_argument_rules_through_the_library(aead):
    """Validation before any launch (no GPU work), in the stated order, on
    n == 0 objects from both constructors and never-dereferenced pointers."""
    A = aead
    BAD, OK = A.ERROR_INVALID_PARAM, A.ERROR_NONE
    ok = dict(slots=0x4000, wire=0x90000, off=0x1000, length=0x2000, result=0x3000)

    def seal(tr, **kw):
        return A.dev_transport_seal_datagrams(tr, **kw)

    def open_(tr, frame_status=0x5000, **kw):
        return A.dev_transport_open_datagrams(tr, frame_status=frame_status, **kw)

    # a NULL object comes first, before m == 0
    for call in (seal, open_):
        for m in (0, 1):
            assert call(None, m=m, **ok) == BAD
    assert A.dev_transport_replay(None) == (0, 1024)

    made = [A.dev_transport_new_unkeyed(A.CHACHAPOLY, A.ROLE_INITIATOR, 0, max_frames=0),
            A.dev_transport_new_unkeyed(A.AESGCM, A.ROLE_RESPONDER, 0, max_frames=2 ** 32 - 1),
            A.dev_transport_new(A.AESGCM, A.ROLE_INITIATOR, 0, k1=0x10000, k2=0x20000, max_frames=0)]
    for rc, tr in made:
        assert rc == 0 and tr
        assert A.dev_transport_replay(tr) == (0, 1024)  # n == 0: it owns nothing
        assert A.lib().noise_aead_dev_transport_replay(tr, None) is None
        for call in (seal, open_):
            # m == 0 is fine whatever else is given
            assert call(tr, m=0, **ok) == OK
            assert call(tr, m=0, max_frames=2 ** 32 - 1, slots=0, wire=0, off=0, length=0, result=0) == OK
            assert call(tr, m=0, **{**ok, "result": 0x1000}) == OK
            # m > 0 is m > n, before the pointers, the cap and the ranges
            assert call(tr, m=1, **ok) == BAD
            assert call(tr, m=1, **{**ok, "slots": 0}) == BAD
            assert call(tr, m=2 ** 32 - 1, **ok) == BAD
        assert open_(tr, m=0, frame_status=0, **ok) == OK
        # the stream calls on it are what they were
        assert A.dev_transport_seal_frames(tr, wire=0x90000, off=0x1000, length=0x2000, result=0x3000) == OK
        assert A.dev_transport_open_frames_of(tr, m=0, **ok) == OK
        assert A.dev_transport_free(tr) == OK
