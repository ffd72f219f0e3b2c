"""The model of one session of the ragged handshake calls
(noise_aead_dev_handshake_write_message_ragged / _read_message_ragged,
include/noise_aead_hip.h section 8): handshake_model.Session plus the length
rule of one session and status 4.

The rule, checked before any token: a write whose message would not fit
(payload length + overhead over `room`, 65535 unless the caller's buffer is
smaller) and a read of a message longer than 65535 bytes or shorter than the
overhead are refused; the session takes status 4 and is from then on the
failed session of the base class — write() and read() return None, split()
gives zero keys, the first cause is sticky.  The reference gives the same
code, NOISE_ERROR_INVALID_LENGTH, at the token it reaches
(handshakestate.c:1454, :1489, :1320-1324; symmetricstate.c:419-422) and is
NOISE_ACTION_FAILED afterwards; tests/test_handshake_ragged_host.py proves
that against tests/golden/handshake_lengths.json."""
import handshake_model as M

STATUS_LENGTH = 4
MAX_MESSAGE = 65535
ERROR_MAC_FAILURE, ERROR_INVALID_LENGTH, ERROR_INVALID_PUBLIC_KEY = 0x4504, 0x450A, 0x450F
# what the reference returns for a session that ends with a status
ERROR_OF_STATUS = {M.STATUS_OK: 0, M.STATUS_MAC: ERROR_MAC_FAILURE, M.STATUS_NULL_KEY: ERROR_INVALID_PUBLIC_KEY,
                   STATUS_LENGTH: ERROR_INVALID_LENGTH}


def session_len(overhead, length, write, room=MAX_MESSAGE):
    """(refused, the other length): the message length of a write of `length`
    payload bytes, the payload length of a read of `length` message bytes; 0
    when refused"""
    if write:
        return (True, 0) if length + overhead > room else (False, length + overhead)
    return (True, 0) if length > MAX_MESSAGE or length < overhead else (False, length - overhead)


class RaggedSession(M.Session):
    def write(self, payload, room=MAX_MESSAGE):
        if not self.status and session_len(self.overhead(), len(payload), True, room)[0]:
            self.status = STATUS_LENGTH
        return super().write(payload)

    def read(self, msg):
        if not self.status and session_len(self.overhead(), len(msg), False)[0]:
            self.status = STATUS_LENGTH
        return super().read(msg)
