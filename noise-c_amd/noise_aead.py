"""Python mirror of the noise-c CipherState interface over the gfx950 engine.

Thin ctypes layer over ``lib/libnoise_aead_hip.so`` (include/noise_aead_hip.h).
Names, argument meaning and return codes follow the reference C API
(include/noise/protocol/cipherstate.h:34-53) so tests read like
tests/unit/test-cipherstate.c: calls return the raw NOISE_ERROR_* code.

There is no fallback of any kind: if the shared library is missing this
module raises on import of ``lib()``; if no GPU is usable the crypto calls
return NOISE_ERROR_SYSTEM.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# NOISE_AEAD_LIB: another build of the same ABI (A/B measurements only)
LIB_PATH = os.environ.get("NOISE_AEAD_LIB") or os.path.join(HERE, "lib", "libnoise_aead_hip.so")
HEADER = os.path.join(HERE, "..", "include", "noise_aead_hip.h")


def NOISE_ID(ch: str, num: int) -> int:  # constants.h:31
    return (ord(ch) << 8) | num


CIPHER_NONE = 0
CHACHAPOLY = NOISE_ID("C", 1)
AESGCM = NOISE_ID("C", 2)
ERROR_NONE = 0
ERROR_NO_MEMORY = NOISE_ID("E", 1)
ERROR_UNKNOWN_ID = NOISE_ID("E", 2)
ERROR_UNKNOWN_NAME = NOISE_ID("E", 3)
ERROR_MAC_FAILURE = NOISE_ID("E", 4)
ERROR_NOT_APPLICABLE = NOISE_ID("E", 5)
ERROR_SYSTEM = NOISE_ID("E", 6)
ERROR_REMOTE_KEY_REQUIRED = NOISE_ID("E", 7)
ERROR_LOCAL_KEY_REQUIRED = NOISE_ID("E", 8)
ERROR_PSK_REQUIRED = NOISE_ID("E", 9)
ERROR_INVALID_LENGTH = NOISE_ID("E", 10)
ERROR_INVALID_PARAM = NOISE_ID("E", 11)
ERROR_INVALID_STATE = NOISE_ID("E", 12)
ERROR_INVALID_NONCE = NOISE_ID("E", 13)
ERROR_INVALID_PUBLIC_KEY = NOISE_ID("E", 15)
ERROR_INVALID_SIGNATURE = NOISE_ID("E", 17)
ROLE_INITIATOR = NOISE_ID("R", 1)  # constants.h:111-112
ROLE_RESPONDER = NOISE_ID("R", 2)
ACTION_NONE = 0  # constants.h:115-120
ACTION_WRITE_MESSAGE = NOISE_ID("A", 1)
ACTION_READ_MESSAGE = NOISE_ID("A", 2)
ACTION_SPLIT = NOISE_ID("A", 4)
ACTION_COMPLETE = NOISE_ID("A", 5)
MAX_PAYLOAD_LEN = 65535
HASH_BLAKE2s = NOISE_ID("H", 1)  # constants.h:43-46
HASH_BLAKE2b = NOISE_ID("H", 2)
HASH_SHA256 = NOISE_ID("H", 3)
HASH_SHA512 = NOISE_ID("H", 4)
DH_CURVE25519 = NOISE_ID("D", 1)  # constants.h:51
SIGN_ED25519 = NOISE_ID("S", 1)  # constants.h:108
STATUS_SIGNATURE_REFUSED = 6  # section 8's status space, written by dev_sign_verify
HASH_LEN = {HASH_BLAKE2s: 32, HASH_BLAKE2b: 64, HASH_SHA256: 32, HASH_SHA512: 64}


class NoiseBuffer(C.Structure):
    """include/noise/protocol/buffer.h:33-40"""
    _fields_ = [("data", C.c_void_p), ("size", C.c_size_t), ("max_size", C.c_size_t)]

    @classmethod
    def inout(cls, mem, size, max_size):  # noise_buffer_set_inout
        return cls(C.addressof(mem) if mem is not None else None, size, max_size)

    @classmethod
    def input(cls, mem, size):  # noise_buffer_set_input
        return cls(C.addressof(mem) if mem is not None else None, size, size)


class NoiseAeadUniform(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("nonce_base", C.c_void_p), ("in_", C.c_void_p),
                ("out", C.c_void_p), ("ad", C.c_void_p), ("status", C.c_void_p),
                ("in_stride", C.c_uint64), ("out_stride", C.c_uint64),
                ("ad_stride", C.c_uint64), ("recs_per_state", C.c_uint32),
                ("n_records", C.c_uint32), ("len", C.c_uint32), ("ad_len", C.c_uint32),
                ("lanes_per_record", C.c_uint32), ("flags", C.c_uint32)]


class NoiseAeadRecord(C.Structure):
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("nonce", C.c_uint64),
                ("ctx_off", C.c_uint64), ("ad_off", C.c_uint64), ("len", C.c_uint32),
                ("ad_len", C.c_uint32)]


class NoiseAeadRagged(C.Structure):
    _fields_ = [("ctx_base", C.c_void_p), ("recs", C.c_void_p), ("in_", C.c_void_p),
                ("out", C.c_void_p), ("ad", C.c_void_p), ("status", C.c_void_p),
                ("n_records", C.c_uint32), ("lanes_per_record", C.c_uint32),
                ("flags", C.c_uint32), ("reserved_", C.c_uint32)]


class NoiseAeadHandshakeConfig(C.Structure):
    _fields_ = [("protocol_name", C.c_char_p), ("role", C.c_int), ("n", C.c_uint32),
                ("d_prologue", C.c_void_p), ("prologue_stride", C.c_uint64), ("prologue_len", C.c_uint32),
                ("d_psk", C.c_void_p), ("psk_stride", C.c_uint64),
                ("d_local_static_priv", C.c_void_p), ("local_static_stride", C.c_uint64),
                ("d_local_ephemeral_priv", C.c_void_p), ("local_ephemeral_stride", C.c_uint64),
                ("d_remote_static_pub", C.c_void_p), ("remote_static_stride", C.c_uint64)]


class NoiseAeadHandshakeFallbackConfig(C.Structure):
    _fields_ = [("d_prologue", C.c_void_p), ("prologue_stride", C.c_uint64), ("prologue_len", C.c_uint32),
                ("d_psk", C.c_void_p), ("psk_stride", C.c_uint64),
                ("d_local_ephemeral_priv", C.c_void_p), ("local_ephemeral_stride", C.c_uint64),
                ("d_select", C.c_void_p), ("flags", C.c_uint32)]


FALLBACK_ONLY_FAILED = 1


class NoiseAeadTransportResult(C.Structure):
    _fields_ = [("frames", C.c_uint32), ("consumed", C.c_uint32), ("error", C.c_int32),
                ("reserved_", C.c_uint32)]


class NoiseAeadPacket(C.Structure):
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint32), ("slot", C.c_uint32)]


# NoiseAeadPacket as a numpy dtype
PACKET_DT = [("off", "<u8"), ("len", "<u4"), ("slot", "<u4")]

FLAG_FAST = 1
FLAG_CT_GHASH = 2
FLAG_VERIFY_FIRST = 4  # the default open order since round 6 (accepted, overrides ONE_PASS)
FLAG_ONE_PASS = 8      # opt-in: ChaChaPoly FAST opens decrypt while authenticating
_LIB = None


def lib() -> C.CDLL:
    """Load the gfx950 library; raise loudly when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} missing: run `make -C noise-c_amd` "
                           "(or __graft_entry__.build()); there is no CPU fallback")
    # One HIP runtime per process: when PyTorch provides the device memory it
    # must be loaded first, so that our NEEDED libamdhip64.so.7 binds to the
    # copy torch already mapped (same SONAME) instead of a second runtime that
    # would not know torch's allocations.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    P = C.POINTER
    sigs = {
        "noise_cipherstate_new_by_id": (i, [P(vp), i]),
        "noise_cipherstate_new_by_name": (i, [P(vp), C.c_char_p]),
        "noise_cipherstate_free": (i, [vp]),
        "noise_cipherstate_get_cipher_id": (i, [vp]),
        "noise_cipherstate_get_key_length": (sz, [vp]),
        "noise_cipherstate_get_mac_length": (sz, [vp]),
        "noise_cipherstate_init_key": (i, [vp, vp, sz]),
        "noise_cipherstate_has_key": (i, [vp]),
        "noise_cipherstate_encrypt_with_ad": (i, [vp, vp, sz, P(NoiseBuffer)]),
        "noise_cipherstate_decrypt_with_ad": (i, [vp, vp, sz, P(NoiseBuffer)]),
        "noise_cipherstate_encrypt": (i, [vp, P(NoiseBuffer)]),
        "noise_cipherstate_decrypt": (i, [vp, P(NoiseBuffer)]),
        "noise_cipherstate_set_nonce": (i, [vp, C.c_uint64]),
        "noise_cipherstate_get_max_key_length": (i, []),
        "noise_cipherstate_get_max_mac_length": (i, []),
        "noise_chachapoly_new": (vp, []),
        "noise_aesgcm_new": (vp, []),
        "noise_cipherstate_encrypt_batch": (i, [P(vp), P(vp), P(sz), P(NoiseBuffer), sz, P(i)]),
        "noise_cipherstate_decrypt_batch": (i, [P(vp), P(vp), P(sz), P(NoiseBuffer), sz, P(i)]),
        "noise_wire_alloc": (vp, [sz]),
        "noise_wire_free": (None, [vp]),
        "noise_wire_seal": (i, [vp, vp, sz, P(sz), P(sz)]),
        "noise_wire_open": (i, [vp, vp, sz, P(sz), P(sz)]),
        "noise_wire_echo": (i, [vp, vp, vp, sz, P(sz), P(sz)]),
        "noise_aead_dev_hkdf": (i, [i, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp,
                                    C.c_uint32, vp, C.c_uint32, vp]),
        "noise_aead_dev_split": (i, [i, vp, C.c_uint32, vp, vp, vp]),
        "noise_aead_dev_encrypt_and_hash": (i, [i, i, vp, P(NoiseAeadRagged), vp]),
        "noise_aead_dev_decrypt_and_hash": (i, [i, i, vp, P(NoiseAeadRagged), vp]),
        "noise_aead_dev_ctx_bytes": (sz, [i]),
        "noise_aead_dev_prepare": (i, [i, vp, C.c_uint32, vp, vp]),
        "noise_aead_dev_seal_uniform": (i, [i, P(NoiseAeadUniform), vp]),
        "noise_aead_dev_open_uniform": (i, [i, P(NoiseAeadUniform), vp]),
        "noise_aead_dev_duplex_uniform": (i, [i, P(NoiseAeadUniform), P(NoiseAeadUniform), vp]),
        "noise_aead_dev_seal_ragged": (i, [i, P(NoiseAeadRagged), vp]),
        "noise_aead_dev_open_ragged": (i, [i, P(NoiseAeadRagged), vp]),
        "noise_aead_dev_duplex_ragged": (i, [i, P(NoiseAeadRagged), P(NoiseAeadRagged), vp]),
        "noise_aead_dev_default_lanes": (i, [i, C.c_uint32]),
        "noise_aead_dev_duplex_lanes": (i, [i, C.c_uint32]),
        "noise_aead_dev_pad": (i, [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, i, vp, vp]),
        "noise_aead_dev_dh_calculate": (i, [i, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp]),
        "noise_aead_dev_dh_public": (i, [i, vp, C.c_uint64, C.c_uint32, vp, vp]),
        "noise_aead_dev_sign_verify": (i, [i, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp, vp]),
        "noise_aead_dev_sign_public": (i, [i, vp, C.c_uint64, C.c_uint32, vp, vp]),
        "noise_aead_dev_sign": (i, [i, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, C.c_uint32, vp, vp]),
        "noise_aead_dev_handshake_new": (i, [P(vp), P(NoiseAeadHandshakeConfig), vp]),
        "noise_aead_dev_handshake_free": (i, [vp]),
        "noise_aead_dev_handshake_get_action": (i, [vp]),
        "noise_aead_dev_handshake_overhead": (sz, [vp]),
        "noise_aead_dev_handshake_write_message": (i, [vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp]),
        "noise_aead_dev_handshake_read_message": (i, [vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp]),
        "noise_aead_dev_handshake_write_message_ragged": (i, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "noise_aead_dev_handshake_read_message_ragged": (i, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "noise_aead_dev_handshake_split": (i, [vp, vp, vp, vp, vp]),
        "noise_aead_dev_handshake_status": (vp, [vp]),
        "noise_aead_dev_handshake_remote_static": (vp, [vp]),
        "noise_aead_dev_handshake_fallback": (i, [vp, P(NoiseAeadHandshakeFallbackConfig), P(vp), vp]),
        "noise_aead_dev_handshake_fallback_merge": (i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "noise_aead_dev_handshake_new_like": (i, [P(vp), vp, C.c_uint32, vp]),
        "noise_aead_dev_handshake_move": (i, [vp, vp, vp, vp, C.c_uint32, vp, vp]),
        "noise_aead_dev_handshake_drop": (i, [vp, vp, C.c_uint32, vp]),
        "noise_aead_dev_transport_new": (i, [P(vp), i, i, C.c_uint32, vp, vp, C.c_uint32, vp]),
        "noise_aead_dev_transport_free": (i, [vp]),
        "noise_aead_dev_transport_nonces": (vp, [vp, i]),
        "noise_aead_dev_transport_seal_frames": (i, [vp, vp, vp, vp, vp, vp]),
        "noise_aead_dev_transport_open_frames": (i, [vp, vp, vp, vp, vp, vp]),
        "noise_aead_dev_transport_echo_frames": (i, [vp, vp, vp, vp, vp, vp]),
        "noise_aead_dev_transport_new_unkeyed": (i, [P(vp), i, i, C.c_uint32, C.c_uint32, vp]),
        "noise_aead_dev_transport_set_keys": (i, [vp, vp, C.c_uint32, vp, vp, vp, vp]),
        "noise_aead_dev_transport_clear_keys": (i, [vp, vp, C.c_uint32, vp]),
        "noise_aead_dev_transport_has_key": (vp, [vp]),
        "noise_aead_dev_transport_seal_frames_of": (i, [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]),
        "noise_aead_dev_transport_open_frames_of": (i, [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]),
        "noise_aead_dev_transport_echo_frames_of": (i, [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]),
        "noise_aead_dev_transport_seal_datagrams": (i, [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]),
        "noise_aead_dev_transport_open_datagrams": (i, [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]),
        "noise_aead_dev_transport_replay": (vp, [vp, P(C.c_uint32)]),
        "noise_aead_dev_rekey": (i, [i, vp, C.c_uint32, vp, vp]),
        "noise_aead_dev_transport_rekey": (i, [vp, vp, C.c_uint32, C.c_uint32, vp, vp]),
        "noise_aead_dev_transport_reserve_packets": (i, [vp, C.c_uint32, vp]),
        "noise_aead_dev_transport_seal_packets": (i, [vp, vp, C.c_uint32, vp, vp, vp]),
        "noise_aead_dev_transport_open_packets": (i, [vp, vp, C.c_uint32, vp, vp, vp]),
        "noise_aead_dev_transport_echo_packets": (i, [vp, vp, C.c_uint32, vp, vp, vp]),
        "noise_aead_debug_transport_ctx": (vp, [vp, i, P(sz)]),
        "noise_strerror": (i, [i, C.c_char_p, sz]),
        "noise_perror": (None, [C.c_char_p, i]),
        "noise_aead_debug_batch_stats": (None, [P(C.c_uint64), P(C.c_uint64)]),
        "noise_aead_debug_last_freed_ctx": (vp, [P(sz)]),
        "noise_aead_debug_last_plan": (i, [C.c_char_p, sz]),
        "noise_aead_debug_f25_op": (i, [i, vp, vp, C.c_uint32, vp, vp]),
        "noise_aead_dev_fill_splitmix": (i, [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]),
    }
    for name, (res, args) in sigs.items():
        if os.environ.get("NOISE_AEAD_LIB") and not hasattr(L, name):
            continue  # an older build under A/B: only the entry points it has
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _LIB = L
    return L


# ---------------------------------------------------------------- wire path
# Frames of examples/echo (echo-common.c:643-688): 2-byte BE length || body.

def frame_for_seal(messages) -> bytes:
    """Seal-ready wire image: each message as one frame whose header is the
    final length (len + 16) followed by the plaintext and 16 bytes of room."""
    out = bytearray()
    for m in messages:
        L = len(m) + 16
        if L > MAX_PAYLOAD_LEN:
            raise ValueError("message too long for one frame")
        out += bytes((L >> 8, L & 0xFF)) + bytes(m) + bytes(16)
    return bytes(out)


def parse_frames(wire: bytes, count=None):
    """[(offset of the body, L)] of the complete frames at the start of wire."""
    out, off = [], 0
    while off + 2 <= len(wire) and (count is None or len(out) < count):
        L = (wire[off] << 8) | wire[off + 1]
        if off + 2 + L > len(wire):
            break
        out.append((off + 2, L))
        off += 2 + L
    return out


def _wire_call(fn, states, buf, length):
    consumed, frames = C.c_size_t(), C.c_size_t()
    rc = fn(*[s.ptr for s in states], buf, length, C.byref(consumed), C.byref(frames))
    return rc, consumed.value, frames.value


def wire_seal(state, buf, length):
    """noise_wire_seal over a ctypes buffer / address; (rc, consumed, frames)."""
    return _wire_call(lib().noise_wire_seal, [state], buf, length)


def wire_open(state, buf, length):
    return _wire_call(lib().noise_wire_open, [state], buf, length)


def wire_echo(recv, send, buf, length):
    return _wire_call(lib().noise_wire_echo, [recv, send], buf, length)


class PinnedWire:
    """A noise_wire_alloc() buffer (pinned host memory), freed on close()."""

    def __init__(self, nbytes: int):
        self.n = nbytes
        self.addr = lib().noise_wire_alloc(nbytes)
        if not self.addr:
            raise MemoryError("noise_wire_alloc failed")
        self.view = (C.c_uint8 * nbytes).from_address(self.addr)

    def close(self):
        if self.addr:
            lib().noise_wire_free(self.addr)
            self.addr = None


def _bytes_ptr(b):
    if b is None:
        return None
    if isinstance(b, (bytes, bytearray)) and len(b) == 0:
        return None
    buf = (C.c_uint8 * len(b)).from_buffer_copy(bytes(b))
    return buf


class CipherState:
    """Object wrapper over a NoiseCipherState* (cipherstate.h:32)."""

    def __init__(self, ptr: int):
        self.ptr = C.c_void_p(ptr)

    @classmethod
    def new_by_id(cls, cid: int):
        p = C.c_void_p()
        rc = lib().noise_cipherstate_new_by_id(C.byref(p), cid)
        return rc, (cls(p.value) if p.value else None)

    @classmethod
    def new_by_name(cls, name):
        p = C.c_void_p()
        rc = lib().noise_cipherstate_new_by_name(
            C.byref(p), name.encode() if isinstance(name, str) else name)
        return rc, (cls(p.value) if p.value else None)

    def free(self) -> int:
        rc = lib().noise_cipherstate_free(self.ptr)
        self.ptr = C.c_void_p(None)
        return rc

    @property
    def cipher_id(self) -> int:
        return lib().noise_cipherstate_get_cipher_id(self.ptr)

    @property
    def key_length(self) -> int:
        return lib().noise_cipherstate_get_key_length(self.ptr)

    @property
    def mac_length(self) -> int:
        return lib().noise_cipherstate_get_mac_length(self.ptr)

    @property
    def has_key(self) -> int:
        return lib().noise_cipherstate_has_key(self.ptr)

    def init_key(self, key, key_len=None) -> int:
        k = _bytes_ptr(key) if key is not None else None
        return lib().noise_cipherstate_init_key(
            self.ptr, k, len(key) if key_len is None else key_len)

    @property
    def nonce(self) -> int:
        """n of the state: the u64 at offset 16 of struct NoiseCipherState_s
        (internal.h:58-146; there is no getter in the reference API)."""
        return C.c_uint64.from_address(self.ptr.value + 16).value

    def set_nonce(self, n: int) -> int:
        return lib().noise_cipherstate_set_nonce(self.ptr, n)

    def encrypt_with_ad(self, ad, buf: NoiseBuffer) -> int:
        a = _bytes_ptr(ad)
        return lib().noise_cipherstate_encrypt_with_ad(self.ptr, a, len(ad or b""), C.byref(buf))

    def decrypt_with_ad(self, ad, buf: NoiseBuffer) -> int:
        a = _bytes_ptr(ad)
        return lib().noise_cipherstate_decrypt_with_ad(self.ptr, a, len(ad or b""), C.byref(buf))

    # convenience: bytes in, bytes out (raises on error)
    def seal(self, pt: bytes, ad: bytes = b"") -> bytes:
        mem = (C.c_uint8 * (len(pt) + 16)).from_buffer_copy(bytes(pt) + bytes(16))
        nb = NoiseBuffer.inout(mem, len(pt), len(pt) + 16)
        rc = self.encrypt_with_ad(ad, nb)
        if rc:
            raise RuntimeError(f"encrypt failed: {rc:#x}")
        return bytes(mem)[: nb.size]

    def open(self, ct: bytes, ad: bytes = b""):
        mem = (C.c_uint8 * max(1, len(ct))).from_buffer_copy(bytes(ct) or b"\0")
        nb = NoiseBuffer.input(mem, len(ct))
        rc = self.decrypt_with_ad(ad, nb)
        return rc, bytes(mem)[: nb.size]


def _batch(fn_name, states, buffers, ads=None):
    n = len(states)
    st_arr = (C.c_void_p * max(1, n))(*[s.ptr.value if s else None for s in states])
    buf_arr = (NoiseBuffer * max(1, n))(*buffers)
    res = (C.c_int * max(1, n))()
    keep = []
    if ads is not None:
        ad_ptrs = []
        for a in ads:
            m = _bytes_ptr(a)
            keep.append(m)
            ad_ptrs.append(C.addressof(m) if m is not None else None)
        ad_arr = (C.c_void_p * max(1, n))(*ad_ptrs)
        len_arr = (C.c_size_t * max(1, n))(*[len(a or b"") for a in ads])
    else:
        ad_arr, len_arr = None, None
    rc = getattr(lib(), fn_name)(st_arr, ad_arr, len_arr, buf_arr, n, res)
    for i in range(n):
        buffers[i].size = buf_arr[i].size
    return rc, list(res[:n])


def encrypt_batch(states, buffers, ads=None):
    """noise_cipherstate_encrypt_batch: same results as sequential calls."""
    return _batch("noise_cipherstate_encrypt_batch", states, buffers, ads)


def decrypt_batch(states, buffers, ads=None):
    """noise_cipherstate_decrypt_batch: same results as sequential calls."""
    return _batch("noise_cipherstate_decrypt_batch", states, buffers, ads)


# ------------------------------------------------------------ device API

def dev_ctx_bytes(cipher: int) -> int:
    return lib().noise_aead_dev_ctx_bytes(cipher)


def dev_prepare(cipher: int, d_raw_keys: int, n_states: int, d_ctx: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_prepare(cipher, d_raw_keys, n_states, d_ctx, stream or None)


def dev_uniform(open_: bool, cipher: int, *, ctx: int, nonce_base: int, inp: int, out: int,
                in_stride: int, out_stride: int, length: int, n_records: int,
                recs_per_state: int, status: int = 0, ad: int = 0, ad_stride: int = 0,
                ad_len: int = 0, lanes: int = 0, flags: int = 0, stream: int = 0) -> int:
    j = NoiseAeadUniform(ctx, nonce_base, inp, out, ad or None, status or None, in_stride,
                         out_stride, ad_stride, recs_per_state, n_records, length, ad_len,
                         lanes, flags)
    f = lib().noise_aead_dev_open_uniform if open_ else lib().noise_aead_dev_seal_uniform
    return f(cipher, C.byref(j), stream or None)


def uniform_job(*, ctx: int, nonce_base: int, inp: int, out: int, in_stride: int,
                out_stride: int, length: int, n_records: int, recs_per_state: int,
                status: int = 0, ad: int = 0, ad_stride: int = 0, ad_len: int = 0,
                lanes: int = 0, flags: int = 0) -> NoiseAeadUniform:
    return NoiseAeadUniform(ctx, nonce_base, inp, out, ad or None, status or None, in_stride,
                            out_stride, ad_stride, recs_per_state, n_records, length, ad_len,
                            lanes, flags)


def dev_duplex(cipher: int, seal_job: NoiseAeadUniform, open_job: NoiseAeadUniform,
               stream: int = 0) -> int:
    """noise_aead_dev_duplex_uniform: seal_job and open_job in one launch."""
    return lib().noise_aead_dev_duplex_uniform(cipher, C.byref(seal_job), C.byref(open_job),
                                               stream or None)


PADDING_ZERO, PADDING_RANDOM = NOISE_ID("G", 1), NOISE_ID("G", 2)


def dev_pad(*, rand: int, payloads: int, stride: int, orig_lens: int, padded_len: int, n: int,
            mode: int, done: int = 0, stream: int = 0) -> int:
    """noise_aead_dev_pad (device pointers; rand may be 0 = NULL state)."""
    return lib().noise_aead_dev_pad(rand or None, payloads, stride, orig_lens, padded_len, n, mode,
                                    done or None, stream or None)


def dev_ragged(open_: bool, cipher: int, *, ctx_base: int, recs: int, inp: int, out: int,
               n_records: int, status: int = 0, ad: int = 0, lanes: int = 0,
               flags: int = 0, stream: int = 0) -> int:
    j = NoiseAeadRagged(ctx_base or None, recs, inp, out, ad or None, status or None,
                        n_records, lanes, flags, 0)
    f = lib().noise_aead_dev_open_ragged if open_ else lib().noise_aead_dev_seal_ragged
    return f(cipher, C.byref(j), stream or None)


def ragged_job(*, ctx_base: int, recs: int, inp: int, out: int, n_records: int, status: int = 0,
               ad: int = 0, lanes: int = 0, flags: int = 0) -> NoiseAeadRagged:
    return NoiseAeadRagged(ctx_base or None, recs or None, inp or None, out or None, ad or None,
                           status or None, n_records, lanes, flags, 0)


def dev_duplex_ragged(cipher: int, seal_job: NoiseAeadRagged, open_job: NoiseAeadRagged,
                      stream: int = 0) -> int:
    """noise_aead_dev_duplex_ragged: seal_job and open_job in one launch where
    they can share a kernel (a job may be None: the NULL job)."""
    return lib().noise_aead_dev_duplex_ragged(cipher, C.byref(seal_job) if seal_job is not None else None,
                                              C.byref(open_job) if open_job is not None else None,
                                              stream or None)


def dev_hkdf(hash_id: int, *, keys: int, key_len: int, data: int = 0, data_len: int = 0,
             n: int, out1: int, out1_len: int, out2: int, out2_len: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_hkdf(hash_id, keys, key_len, data or None, data_len, n, out1,
                                     out1_len, out2, out2_len, stream or None)


def dev_and_hash(open_: bool, cipher: int, hash_id: int, *, ctx_base: int, h: int, recs: int,
                 inp: int, out: int, n_records: int, status: int = 0, flags: int = 0,
                 stream: int = 0) -> int:
    """noise_aead_dev_{en,de}crypt_and_hash: AD = the hashes at h; record
    ctx_off values are offsets from ctx_base (as dev_ragged)."""
    j = NoiseAeadRagged(ctx_base or None, recs, inp, out, h, status or None, n_records, 0,
                        flags, 0)
    f = (lib().noise_aead_dev_decrypt_and_hash if open_ else
         lib().noise_aead_dev_encrypt_and_hash)
    return f(cipher, hash_id, h, C.byref(j), stream or None)


def dev_split(hash_id: int, *, ck: int, n: int, k1: int, k2: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_split(hash_id, ck, n, k1, k2, stream or None)


def dev_dh_calculate(dh_id: int, *, priv: int, priv_stride: int = 32, pub: int, pub_stride: int = 32,
                     n: int, shared: int, stream: int = 0) -> int:
    """noise_aead_dev_dh_calculate: n shared keys, packed 32 bytes apart at
    `shared` (a stride of 0: one key for all n sessions)."""
    return lib().noise_aead_dev_dh_calculate(dh_id, priv or None, priv_stride, pub or None, pub_stride,
                                             n, shared or None, stream or None)


def dev_dh_public(dh_id: int, *, priv: int, priv_stride: int = 32, n: int, pub_out: int,
                  stream: int = 0) -> int:
    """noise_aead_dev_dh_public: the public key of each of n private keys."""
    return lib().noise_aead_dev_dh_public(dh_id, priv or None, priv_stride, n, pub_out or None,
                                          stream or None)


def dev_sign_verify(sign_id: int, *, pub: int, pub_stride: int = 32, sig: int, sig_stride: int = 64,
                    msg: int, msg_off: int, msg_len: int, n: int, status_in: int = 0, status: int,
                    stream: int = 0) -> int:
    """noise_aead_dev_sign_verify: n Ed25519 verdicts as status bytes (0, or 6:
    refused); message i is msg_len[i] bytes at msg + msg_off[i] (device arrays
    of u64 / u32).  A pub_stride of 0 is one signer for all; an entry whose
    status_in byte is non-zero keeps that byte and reads nothing."""
    return lib().noise_aead_dev_sign_verify(sign_id, pub or None, pub_stride, sig or None, sig_stride,
                                            msg or None, msg_off or None, msg_len or None, n,
                                            status_in or None, status or None, stream or None)


def dev_sign_public(sign_id: int, *, priv: int, priv_stride: int = 32, n: int, pub_out: int,
                    stream: int = 0) -> int:
    """noise_aead_dev_sign_public: the Ed25519 public key of each of n 32-byte seeds."""
    return lib().noise_aead_dev_sign_public(sign_id, priv or None, priv_stride, n, pub_out or None,
                                            stream or None)


def dev_sign(sign_id: int, *, priv: int, priv_stride: int = 32, pub: int, pub_stride: int = 32,
             msg: int, msg_off: int, msg_len: int, n: int, sig_out: int, stream: int = 0) -> int:
    """noise_aead_dev_sign: n signatures R || S, packed 64 bytes apart at
    sig_out; the public keys are taken as given."""
    return lib().noise_aead_dev_sign(sign_id, priv or None, priv_stride, pub or None, pub_stride,
                                     msg or None, msg_off or None, msg_len or None, n, sig_out or None,
                                     stream or None)


# ---- batched handshakes (include/noise_aead_hip.h section 8); `hs` is the
# NoiseAeadDevHandshake* as an integer, every data argument a device pointer

def dev_handshake_new(name, role: int, n: int, *, prologue: int = 0, prologue_stride: int = 0,
                      prologue_len: int = 0, psk: int = 0, psk_stride: int = 32, local_static: int = 0,
                      local_static_stride: int = 32, local_ephemeral: int = 0, local_ephemeral_stride: int = 32,
                      remote_static: int = 0, remote_static_stride: int = 32, stream: int = 0):
    """noise_aead_dev_handshake_new: (rc, hs); hs is None unless rc == 0."""
    if isinstance(name, str):
        name = name.encode()
    cfg = NoiseAeadHandshakeConfig(name, role, n, prologue or None, prologue_stride, prologue_len,
                                   psk or None, psk_stride, local_static or None, local_static_stride,
                                   local_ephemeral or None, local_ephemeral_stride,
                                   remote_static or None, remote_static_stride)
    hs = C.c_void_p()
    rc = lib().noise_aead_dev_handshake_new(C.byref(hs), C.byref(cfg), stream or None)
    return rc, hs.value


def dev_handshake_free(hs: int) -> int:
    return lib().noise_aead_dev_handshake_free(hs)


def dev_handshake_get_action(hs: int) -> int:
    return lib().noise_aead_dev_handshake_get_action(hs)


def dev_handshake_overhead(hs: int) -> int:
    return lib().noise_aead_dev_handshake_overhead(hs)


def dev_handshake_write_message(hs: int, *, payload: int = 0, payload_stride: int = 0, payload_len: int = 0,
                                msg: int, msg_stride: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_handshake_write_message(hs, payload or None, payload_stride, payload_len,
                                                        msg or None, msg_stride, stream or None)


def dev_handshake_read_message(hs: int, *, msg: int, msg_stride: int, msg_len: int, payload: int = 0,
                               payload_stride: int = 0, stream: int = 0) -> int:
    return lib().noise_aead_dev_handshake_read_message(hs, msg or None, msg_stride, msg_len, payload or None,
                                                       payload_stride, stream or None)


def dev_handshake_write_message_ragged(hs: int, *, payload: int = 0, payload_off: int = 0, payload_len: int = 0,
                                       msg: int, msg_off: int, msg_len: int, stream: int = 0) -> int:
    """payload_off / msg_off: n uint64 on the device; payload_len: n uint32;
    msg_len: n uint32 the call writes.  The payload triple may be 0 all three."""
    return lib().noise_aead_dev_handshake_write_message_ragged(hs, payload or None, payload_off or None,
                                                               payload_len or None, msg or None, msg_off or None,
                                                               msg_len or None, stream or None)


def dev_handshake_read_message_ragged(hs: int, *, msg: int, msg_off: int, msg_len: int, payload: int,
                                      payload_off: int, payload_len: int, stream: int = 0) -> int:
    """msg_off / payload_off: n uint64 on the device; msg_len: n uint32;
    payload_len: n uint32 the call writes."""
    return lib().noise_aead_dev_handshake_read_message_ragged(hs, msg or None, msg_off or None, msg_len or None,
                                                              payload or None, payload_off or None,
                                                              payload_len or None, stream or None)


def dev_handshake_split(hs: int, *, k1: int, k2: int, handshake_hash: int = 0, stream: int = 0) -> int:
    return lib().noise_aead_dev_handshake_split(hs, k1 or None, k2 or None, handshake_hash or None,
                                                stream or None)


def dev_handshake_status(hs: int) -> int:
    """device pointer of the n status bytes (0 ok, 1 MAC failure, 3 null ephemeral, 4 a refused length)"""
    return lib().noise_aead_dev_handshake_status(hs) or 0


def dev_handshake_remote_static(hs: int) -> int:
    """device pointer of the n x 32 remote static public keys"""
    return lib().noise_aead_dev_handshake_remote_static(hs) or 0


# ---- the Noise Pipes fallback (include/noise_aead_hip.h section 15)

def dev_handshake_fallback(hs: int, *, prologue: int = 0, prologue_stride: int = 0, prologue_len: int = 0,
                           psk: int = 0, psk_stride: int = 32, local_ephemeral: int = 0,
                           local_ephemeral_stride: int = 32, select: int = 0, flags: int = 0, stream: int = 0,
                           no_cfg: bool = False, no_out: bool = False):
    """noise_aead_dev_handshake_fallback: (rc, fb); fb is None unless rc == 0.
    no_cfg / no_out: a NULL cfg / a NULL fb pointer, for the argument tests."""
    cfg = NoiseAeadHandshakeFallbackConfig(prologue or None, prologue_stride, prologue_len, psk or None, psk_stride,
                                           local_ephemeral or None, local_ephemeral_stride, select or None, flags)
    fb = C.c_void_p()
    rc = lib().noise_aead_dev_handshake_fallback(hs, None if no_cfg else C.byref(cfg), None if no_out else C.byref(fb),
                                                 stream or None)
    return rc, fb.value


def dev_handshake_fallback_merge(fb: int, *, hs_status: int, k1: int, k2: int, fb_k1: int, fb_k2: int, h: int = 0,
                                 fb_h: int = 0, status: int, stream: int = 0) -> int:
    """noise_aead_dev_handshake_fallback_merge: fb's split folded into hs's
    (k1, k2, h as they lie) and the n status bytes for _set_keys."""
    return lib().noise_aead_dev_handshake_fallback_merge(fb, hs_status or None, k1 or None, k2 or None, fb_k1 or None,
                                                         fb_k2 or None, h or None, fb_h or None, status or None,
                                                         stream or None)


# ---- sessions that change their object (include/noise_aead_hip.h section 16)

MOVED, MOVE_EMPTY, MOVE_TAKEN, MOVE_RANGE = 0, 1, 2, 3


def dev_handshake_new_like(like: int, capacity: int, *, stream: int = 0, no_out: bool = False):
    """noise_aead_dev_handshake_new_like: (rc, hs); hs is None unless rc == 0.
    no_out: a NULL out pointer, for the argument tests."""
    hs = C.c_void_p()
    rc = lib().noise_aead_dev_handshake_new_like(None if no_out else C.byref(hs), like or None, capacity, stream or None)
    return rc, hs.value


def dev_handshake_move(dst: int, src: int, m: int, *, dst_lanes: int = 0, src_lanes: int = 0, result: int = 0,
                       stream: int = 0) -> int:
    """noise_aead_dev_handshake_move: dst_lanes / src_lanes: m uint32 on the
    device, or 0 for 0 .. m-1; result: m bytes the call writes, or 0."""
    return lib().noise_aead_dev_handshake_move(dst or None, dst_lanes or None, src or None, src_lanes or None, m,
                                               result or None, stream or None)


def dev_handshake_drop(hs: int, *, lanes: int, m: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_handshake_drop(hs or None, lanes or None, m, stream or None)


# ---- device-resident transport sessions (include/noise_aead_hip.h section 9);
# `tr` is the NoiseAeadDevTransport* as an integer, every data argument a device
# pointer; a result is n NoiseAeadTransportResult (frames, consumed, error, 0)

def dev_transport_new(cipher: int, role: int, n: int, *, k1: int, k2: int, max_frames: int, stream: int = 0):
    """noise_aead_dev_transport_new: (rc, tr); tr is None unless rc == 0."""
    tr = C.c_void_p()
    rc = lib().noise_aead_dev_transport_new(C.byref(tr), cipher, role, n, k1 or None, k2 or None, max_frames,
                                            stream or None)
    return rc, tr.value


def dev_transport_free(tr: int) -> int:
    return lib().noise_aead_dev_transport_free(tr)


def dev_transport_nonces(tr: int, direction: int) -> int:
    """device pointer of the n 64-bit nonces of one direction (0 send, 1 receive)"""
    return lib().noise_aead_dev_transport_nonces(tr, direction) or 0


def _transport_call(fn, tr, wire, off, length, result, stream):
    return fn(tr, wire or None, off or None, length or None, result or None, stream or None)


def dev_transport_seal_frames(tr: int, *, wire: int, off: int, length: int, result: int, stream: int = 0) -> int:
    return _transport_call(lib().noise_aead_dev_transport_seal_frames, tr, wire, off, length, result, stream)


def dev_transport_open_frames(tr: int, *, wire: int, off: int, length: int, result: int, stream: int = 0) -> int:
    return _transport_call(lib().noise_aead_dev_transport_open_frames, tr, wire, off, length, result, stream)


def dev_transport_echo_frames(tr: int, *, wire: int, off: int, length: int, result: int, stream: int = 0) -> int:
    return _transport_call(lib().noise_aead_dev_transport_echo_frames, tr, wire, off, length, result, stream)


# ---- the session table (section 10): slots keyed and un-keyed on the device,
# calls over a device list of m slot numbers (32-bit)

def dev_transport_new_unkeyed(cipher: int, role: int, n: int, *, max_frames: int, stream: int = 0):
    """noise_aead_dev_transport_new_unkeyed: (rc, tr); tr is None unless rc == 0."""
    tr = C.c_void_p()
    rc = lib().noise_aead_dev_transport_new_unkeyed(C.byref(tr), cipher, role, n, max_frames, stream or None)
    return rc, tr.value


def dev_transport_set_keys(tr: int, *, slots: int, m: int, k1: int, k2: int, status: int = 0, stream: int = 0) -> int:
    return lib().noise_aead_dev_transport_set_keys(tr, slots or None, m, k1 or None, k2 or None, status or None,
                                                   stream or None)


def dev_transport_clear_keys(tr: int, *, slots: int, m: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_transport_clear_keys(tr, slots or None, m, stream or None)


def dev_transport_has_key(tr: int) -> int:
    """device pointer of the n state bytes (1 keyed, 0 unkeyed)"""
    return lib().noise_aead_dev_transport_has_key(tr) or 0


def _transport_call_of(fn, tr, slots, m, max_frames, wire, off, length, result, stream):
    return fn(tr, slots or None, m, max_frames, wire or None, off or None, length or None, result or None, stream or None)


def dev_transport_seal_frames_of(tr: int, *, slots: int, m: int, max_frames: int = 0, wire: int, off: int, length: int,
                                 result: int, stream: int = 0) -> int:
    return _transport_call_of(lib().noise_aead_dev_transport_seal_frames_of, tr, slots, m, max_frames, wire, off, length,
                              result, stream)


def dev_transport_open_frames_of(tr: int, *, slots: int, m: int, max_frames: int = 0, wire: int, off: int, length: int,
                                 result: int, stream: int = 0) -> int:
    return _transport_call_of(lib().noise_aead_dev_transport_open_frames_of, tr, slots, m, max_frames, wire, off, length,
                              result, stream)


def dev_transport_echo_frames_of(tr: int, *, slots: int, m: int, max_frames: int = 0, wire: int, off: int, length: int,
                                 result: int, stream: int = 0) -> int:
    return _transport_call_of(lib().noise_aead_dev_transport_echo_frames_of, tr, slots, m, max_frames, wire, off, length,
                              result, stream)


# ---- datagram transport (section 11): every frame carries its counter; a
# slot list of 0 means entry j is slot j.  The open's result is m
# NoiseAeadDatagramResult (frames, consumed, error, accepted, 64-bit first)

def dev_transport_seal_datagrams(tr: int, *, slots: int = 0, m: int, max_frames: int = 0, wire: int, off: int, length: int,
                                 result: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_transport_seal_datagrams(tr, slots or None, m, max_frames, wire or None, off or None,
                                                         length or None, result or None, stream or None)


def dev_transport_open_datagrams(tr: int, *, slots: int = 0, m: int, max_frames: int = 0, wire: int, off: int, length: int,
                                 result: int, frame_status: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_transport_open_datagrams(tr, slots or None, m, max_frames, wire or None, off or None,
                                                         length or None, result or None, frame_status or None,
                                                         stream or None)


def dev_transport_replay(tr: int):
    """(device pointer of the n windows {uint64 top; uint64 seen[16]}, or 0; the window size in bits)"""
    bits = C.c_uint32(0)
    return lib().noise_aead_dev_transport_replay(tr, C.byref(bits)) or 0, bits.value


# ---- rekey on the device (section 12): k = REKEY(k), nonces untouched

REKEY_SEND, REKEY_RECEIVE = 1, 2


def dev_rekey(cipher: int, *, keys: int, n: int, out: int, stream: int = 0) -> int:
    """noise_aead_dev_rekey: the successor of each of n packed 32-byte keys, to
    `out` (which may be `keys`)."""
    return lib().noise_aead_dev_rekey(cipher, keys or None, n, out or None, stream or None)


def dev_transport_rekey(tr: int, *, slots: int = 0, m: int, directions: int, which: int = 0, stream: int = 0) -> int:
    """noise_aead_dev_transport_rekey: entry j rekeys the directions
    `directions` & (its byte of `which`, or 3 without one) of its slot."""
    return lib().noise_aead_dev_transport_rekey(tr, slots or None, m, directions, which or None, stream or None)


# ---- packet transport (section 13): a device list of count NoiseAeadPacket
# {off, len, slot} in arrival order, slots repeated; one status byte per packet
# (0 done, 1 the tag failed, 4 the length, 5 the counter refused, 6 no session)

PACKET_OK, PACKET_FORGED, PACKET_LENGTH, PACKET_REPLAY, PACKET_NO_SESSION = 0, 1, 4, 5, 6


def dev_transport_reserve_packets(tr: int, max_packets: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_transport_reserve_packets(tr, max_packets, stream or None)


def dev_transport_seal_packets(tr: int, *, packets: int, count: int, wire: int, status: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_transport_seal_packets(tr, packets or None, count, wire or None, status or None,
                                                       stream or None)


def dev_transport_open_packets(tr: int, *, packets: int, count: int, wire: int, status: int, stream: int = 0) -> int:
    return lib().noise_aead_dev_transport_open_packets(tr, packets or None, count, wire or None, status or None,
                                                       stream or None)


def dev_transport_echo_packets(tr: int, *, packets: int, count: int, wire: int, status: int, stream: int = 0) -> int:
    """section 14: the open of the list and the seal of what it accepted, in place, in one call"""
    return lib().noise_aead_dev_transport_echo_packets(tr, packets or None, count, wire or None, status or None,
                                                       stream or None)


def debug_transport_ctx(tr: int, direction: int):
    """(device pointer of the n contexts of one direction, bytes per context); (0, 0) when there is none"""
    size = C.c_size_t(0)
    return lib().noise_aead_debug_transport_ctx(tr, direction, C.byref(size)) or 0, size.value


def dev_fill_splitmix(d_out: int, nbytes: int, seed: int, word0: int = 0, stream: int = 0) -> int:
    return lib().noise_aead_dev_fill_splitmix(d_out, nbytes, seed, word0, stream or None)


def last_plan() -> str:
    """The batch kernel this thread launched last, with its template arguments,
    grid and kernel arguments (noise_aead_debug_last_plan)."""
    buf = C.create_string_buffer(256)
    lib().noise_aead_debug_last_plan(buf, len(buf))
    return buf.value.decode()


# the operations of noise_aead_debug_f25_op (NOISE_AEAD_F25_*)
F25_ADD, F25_SUB, F25_MUL, F25_SQ, F25_MUL_121665, F25_MUL_9, F25_FREEZE, F25_INVERT = range(8)


def debug_f25_op(op: int, *, a: int, b: int = 0, n: int, out: int, stream: int = 0) -> int:
    """noise_aead_debug_f25_op: one field operation of csrc/fe25519.h on each
    of n packed 32-byte elements; the raw result, 32 bytes each, at `out`."""
    return lib().noise_aead_debug_f25_op(op, a or None, b or None, n, out or None, stream or None)


def dev_default_lanes(cipher: int, n_records: int) -> int:
    return lib().noise_aead_dev_default_lanes(cipher, n_records)


def dev_duplex_lanes(cipher: int, n_records: int) -> int:
    return lib().noise_aead_dev_duplex_lanes(cipher, n_records)
