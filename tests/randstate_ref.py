"""The reference's own RandState, loaded from the built reference library
(oracle.REF_FULL_SO), beside a snapshot of its generator for the oracle."""
import ctypes as C

from oracle import RandSnapshot, REF_FULL_SO


def ref_randstate():
    """A reference RandState (OS-seeded) and a snapshot of its generator:
    struct NoiseRandState_s {size_t size; size_t left; chacha_ctx chacha;}
    (randstate.c:47-58), chacha input words 4..15 = key, counter, IV."""
    R = C.CDLL(REF_FULL_SO)
    R.noise_randstate_new.argtypes = [C.POINTER(C.c_void_p)]
    R.noise_randstate_pad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
    R.noise_randstate_free.argtypes = [C.c_void_p]
    st = C.c_void_p()
    rc = R.noise_randstate_new(C.byref(st))
    assert rc == 0, "noise_randstate_new: %#x" % rc
    return R, st


def snapshot_of(st):
    w = (C.c_uint32 * 16).from_address(st.value + 16)
    s = RandSnapshot()
    for i in range(8):
        s.key[i] = w[4 + i]
    s.counter = w[12] | (w[13] << 32)
    s.iv = w[14] | (w[15] << 32)
    s.left = C.c_size_t.from_address(st.value + 8).value
    return s
