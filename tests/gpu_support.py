"""What every GPU test needs: torch on demand, host <-> device copies, reads
and writes of device memory the library owns, and the library's ids and flags
under the short names the tests use.  Importable without pytest and without
torch (the child programs and tools/ import it too)."""
import ctypes

import numpy as np

import noise_aead

CHACHA, AES = noise_aead.CHACHAPOLY, noise_aead.AESGCM
# NOISE_AEAD_FLAG_*: verify-first is the default open order (round 6);
# ONE_PASS opts a ChaChaPoly FAST open into decrypt-while-authenticating
FLAG_FAST, FLAG_CT_GHASH = noise_aead.FLAG_FAST, noise_aead.FLAG_CT_GHASH
FLAG_VERIFY_FIRST, FLAG_ONE_PASS = noise_aead.FLAG_VERIFY_FIRST, noise_aead.FLAG_ONE_PASS
INVALID_PARAM, UNKNOWN_ID = noise_aead.ERROR_INVALID_PARAM, noise_aead.ERROR_UNKNOWN_ID

# NoiseAeadRecord as a numpy dtype (tests/test_support_host.py holds it to the ctypes mirror)
REC_DT = [("in_off", "<u8"), ("out_off", "<u8"), ("nonce", "<u8"), ("ctx_off", "<u8"),
          ("ad_off", "<u8"), ("len", "<u4"), ("ad_len", "<u4")]


def ru(x, m):
    return (x + m - 1) // m * m


def _torch():
    import torch
    return torch


def dev(arr):
    return _torch().from_numpy(np.ascontiguousarray(arr)).to("cuda")


def dev_u32(values):
    return dev(np.array(values, dtype=np.uint32).view(np.int32))


def dev_bytes(data: bytes):
    return dev(np.frombuffer(bytes(data), dtype=np.uint8).copy())


def stream():
    return _torch().cuda.current_stream().cuda_stream


def sync():
    _torch().cuda.synchronize()


# ------------------------------------------- device memory the library owns

def _memcpy(dst, src, nbytes, kind):
    hip = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)  # the HIP runtime torch already loaded
    sync()
    rc = hip.hipMemcpy(dst, src, ctypes.c_size_t(nbytes), kind)
    assert rc == 0, "hipMemcpy kind %d of %d bytes: error %d" % (kind, nbytes, rc)


def peek(ptr, nbytes) -> bytes:
    host = (ctypes.c_uint8 * nbytes)()
    _memcpy(host, ctypes.c_void_p(ptr), nbytes, 2)  # device to host
    return bytes(host)


def poke(ptr, data: bytes):
    host = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    _memcpy(ctypes.c_void_p(ptr), host, len(data), 1)  # host to device


def peek_u8(ptr, n):
    return np.frombuffer(peek(ptr, n), dtype=np.uint8)


def peek_u64(ptr, n):
    return np.frombuffer(peek(ptr, 8 * n), dtype="<u8").tolist()


def poke_u64(ptr, values):
    poke(ptr, np.array(values, dtype="<u8").tobytes())


# ------------------------------------------------------------- key contexts

def prepare(aead, cipher, keys):
    """noise_aead_dev_prepare of the keys: (the contexts, the keys) on the device"""
    keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 32)
    d_keys = dev(keys.reshape(-1))
    ctx = _torch().empty(keys.shape[0] * aead.dev_ctx_bytes(cipher), dtype=_torch().uint8, device="cuda")
    rc = aead.dev_prepare(cipher, d_keys.data_ptr(), keys.shape[0], ctx.data_ptr(), stream())
    assert rc == 0, "dev_prepare of %d keys: %#x" % (keys.shape[0], rc)
    return ctx, d_keys


def prepared(A, cipher, keys):
    """noise_aead_dev_prepare of each key (None: no key) into a zeroed buffer: [len(keys), ctx_bytes]"""
    cb = A.dev_ctx_bytes(cipher)
    raw = dev_bytes(b"".join(k or bytes(32) for k in keys))
    ctx = _torch().zeros(len(keys) * cb, dtype=_torch().uint8, device="cuda")
    rc = A.dev_prepare(cipher, raw.data_ptr(), len(keys), ctx.data_ptr(), stream())
    assert rc == 0, "dev_prepare of %d keys: %#x" % (len(keys), rc)
    sync()
    out = ctx.cpu().numpy().reshape(len(keys), cb).copy()
    for i, k in enumerate(keys):
        if k is None:
            out[i] = 0
    return out
