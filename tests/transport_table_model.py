"""A plain model of the session table (noise_aead_dev_transport_* over slots,
include/noise_aead_hip.h section 10) on top of tests/transport_model.py.

A call names the slots it is about.  An entry whose slot is out of range or
unkeyed has a fixed result, reads and writes nothing of its stream and takes
no frame numbers, so the other entries behave as a batch made of exactly them
in list order: the model takes the two kinds out, runs T.run_batch on the
rest and splices the fixed results back in."""
import transport_model as T

ERROR_INVALID_PARAM = 0x450B
ERROR_INVALID_STATE = 0x450C


def run_table(sessions, mode, streams, max_frames, slots=None):
    """One call over entries 0 .. len(streams) - 1: entry j is slot slots[j]
    (slot j without a list) with streams[j].  sessions[i] is the T.Session of
    slot i, or None for an unkeyed slot.  [(stream after, result, later)] per
    entry, as T.run_batch gives them; the sessions' nonces advance."""
    n = len(sessions)
    slots = list(range(len(streams))) if slots is None else list(slots)
    assert len(slots) == len(streams)
    live = [j for j, i in enumerate(slots) if 0 <= i < n and sessions[i] is not None]
    assert len({slots[j] for j in live}) == len(live), "the listed slots must be distinct"
    ran = T.run_batch([sessions[slots[j]] for j in live], mode, [streams[j] for j in live], max_frames)
    out = []
    for j, i in enumerate(slots):
        if not 0 <= i < n:
            out.append((bytes(streams[j]), (0, 0, ERROR_INVALID_PARAM), {}))
        elif sessions[i] is None:
            out.append((bytes(streams[j]), (0, 0, ERROR_INVALID_STATE), {}))
        else:
            out.append(ran[live.index(j)])
    return out
