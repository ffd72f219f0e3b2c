"""A model of handshake sessions that change their object: the checker of
noise_aead_dev_handshake_new_like / _move / _drop (include/noise_aead_hip.h
section 16).

An object is a list of lanes, each a session of tests/handshake_model.py (or a
Fallback of tests/handshake_fallback_model.py) or None for an empty lane, and
a position that all its sessions share.  Sessions are independent, so a
session's expected bytes are its own model's, whichever objects it passed
through: move and drop only say which lane holds which session.  The rule of
one entry is written here from the header's table, not from
csrc/handshake_plan.h; tests/test_handshake_move_host.py holds the two
together.  Importable without pytest and without torch."""

STATUS_ABSENT = 5
MOVED, EMPTY, TAKEN, RANGE = 0, 1, 2, 3
OUTCOMES = {MOVED: "moved", EMPTY: "empty", TAKEN: "taken", RANGE: "range"}


def move_rule(src_in_range, dst_in_range, src_status, dst_status):
    """the result byte of one entry; the causes in the header's order"""
    causes = ((RANGE, not (src_in_range and dst_in_range)),
              (EMPTY, src_status == STATUS_ABSENT),
              (TAKEN, dst_status != STATUS_ABSENT))
    return next((code for code, holds in causes if holds), MOVED)


def position_of(sess):
    """what every session of an object shares: the handshake (a Fallback has
    the pattern XXfallback), the role, the messages done, whether a key is
    set and the nonce"""
    f = sess.f
    return (f["psk"], f["pattern"], f["cipher"], f["hash"], sess.initiator, sess.index, sess.k is not None, sess.n)


class Obj:
    """`capacity` lanes at a position (None: not yet known, taken from the
    first session that arrives)"""

    def __init__(self, capacity, position=None, sessions=None):
        self.lanes = [None] * capacity
        self.position = position
        for i, s in enumerate(sessions or []):
            self.lanes[i] = s
        if sessions and position is None:
            self.position = position_of(sessions[0])

    @classmethod
    def like(cls, other, capacity):
        return cls(capacity, other.position)

    @property
    def n(self):
        return len(self.lanes)

    def status(self):
        return [STATUS_ABSENT if s is None else s.status for s in self.lanes]

    def advanced(self):
        """after a message call of the object: the position of its sessions now"""
        live = [s for s in self.lanes if s is not None and s.status == 0]  # a failed one stopped in mid-message
        if live:
            self.position = position_of(live[0])


def move(dst, dst_lanes, src, src_lanes, m):
    """noise_aead_dev_handshake_move on the two models: the m result bytes.
    A list of None means 0 .. m-1."""
    assert dst is not src and dst.position == src.position, (dst.position, src.position)
    out = []
    for j in range(m):
        s = j if src_lanes is None else src_lanes[j]
        d = j if dst_lanes is None else dst_lanes[j]
        s_in, d_in = s < src.n, d < dst.n
        both = s_in and d_in
        r = move_rule(s_in, d_in, src.status()[s] if both else 0, dst.status()[d] if both else 0)
        if r == MOVED:
            dst.lanes[d], src.lanes[s] = src.lanes[s], None
        out.append(r)
    return out


def drop(obj, lanes):
    for i in lanes:
        if i < obj.n:
            obj.lanes[i] = None
