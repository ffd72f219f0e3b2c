"""The session table: noise_aead_dev_transport_* over slots (header section 10).

One long-lived object whose slots are keyed (_set_keys, from packed key arrays
and an optional device status array) and un-keyed (_clear_keys) on the device,
and whose frame calls may name the slots they are about (_frames_of).  Every
call is compared with the model of tests/transport_table_model.py: every byte
of the wire between canaries, every result, both nonce arrays and the state
bytes; the key contexts with noise_aead_dev_prepare of the right key into a
zeroed buffer, byte for byte.  n = 67 slots: one wave plus a partial one.  The
wire and object helpers are those of tests/transport_gpu.py."""
import pytest

import transport_model as T
import transport_table_model as M
from gpu_support import dev_bytes, dev_u32
from handshake_gpu import basic_vector, handshake, make_sessions
from transport_gpu import CIPHERS, N, PERM, Table, Wire, keys_for, plain_streams

pytestmark = pytest.mark.gpu
IDS = ["ChaChaPoly", "AESGCM"]
TOP = 2 ** 32 - 1


# ---------------------------------------------------------------- 1. contexts

@pytest.mark.parametrize("initiator", [True, False], ids=["initiator", "responder"])
@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_set_keys_builds_the_contexts_prepare_builds(aead, gpu, oracle, cipher, initiator):
    import torch
    tab = Table(aead, torch, oracle, cipher, initiator, 8)
    tab.check_state()
    tab.check_contexts()  # all zero
    slots = PERM[:40]
    slots = slots[:10] + [N] + slots[10:30] + [TOP] + slots[30:]
    keys = keys_for(31, len(slots))
    status = [0] * len(slots)
    for j, v in ((0, 1), (4, 3), (17, 255), (33, 1), (41, 2)):
        status[j] = v
    assert slots[10] == N and slots[31] == TOP and len(set(slots)) == len(slots) == 42
    # non-zero nonces beforehand: in a slot that gets keys, in one whose entry failed, in one not named
    unnamed = next(i for i in range(N) if i not in slots)
    tab.set_nonces(0, {slots[1]: 77, slots[0]: 5, unnamed: 1234})
    tab.set_nonces(1, {slots[1]: 2 ** 40, slots[0]: 6, unnamed: T.NONCE_LIMIT})
    tab.set_keys(slots, keys, status)
    assert tab.model[slots[0]] is None and tab.model[slots[4]] is None and tab.model[slots[1]] is not None
    assert sum(1 for m in tab.model if m) == 40 - 5
    tab.check_state()
    assert tab.nonces(0)[slots[1]] == tab.nonces(1)[slots[1]] == tab.nonces(0)[slots[0]] == tab.nonces(1)[slots[0]] == 0
    assert tab.nonces(0)[unnamed] == 1234 and tab.nonces(1)[unnamed] == T.NONCE_LIMIT
    tab.check_contexts()
    # the role picked the directions
    s = tab.model[slots[1]]
    assert (s.send_key, s.recv_key) == (keys[1] if initiator else keys[1][::-1])
    # without a status array every in-range entry is keyed; slots not named keep every byte
    before = [tab.ctx(0).copy(), tab.ctx(1).copy()]
    again = [slots[0], TOP, slots[4]]
    tab.set_keys(again, keys[:3])
    tab.check_state()
    tab.check_contexts()
    for d in (0, 1):
        now = tab.ctx(d)
        for i in range(N):
            assert i in again or (now[i] == before[d][i]).all(), (d, i)
    tab.free()


# ---------------------------------------------------------------- 2. unkeyed slots in the full calls

def _dead(i):
    return i % 7 == 3


def _pair(aead, torch, oracle, cipher, max_frames, seed):
    """an initiator and a responder table, the slots with _dead(i) unkeyed"""
    keys = keys_for(seed)
    live = [i for i in PERM if not _dead(i)]
    pair = []
    for initiator in (True, False):
        tab = Table(aead, torch, oracle, cipher, initiator, max_frames)
        tab.set_keys(live, [keys[i] for i in live])
        pair.append(tab)
    return pair


@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_unkeyed_slots_in_the_full_calls(aead, gpu, oracle, cipher):
    """The cap is exactly the keyed sessions' frame total: the unkeyed slots'
    streams, full of frames, take no numbers."""
    import torch
    total = sum(i % 6 for i in range(N) if not _dead(i))
    a, b = _pair(aead, torch, oracle, cipher, total, 41)
    plain = plain_streams(41, big=False)
    assert sum(len(T.walk(plain[i], 0)[0]) for i in range(N) if _dead(i)) > 10
    wire = Wire(torch, plain)
    results = a.run("seal", wire)
    assert [r[2] for r in results] == [M.ERROR_INVALID_STATE if _dead(i) else 0 for i in range(N)]
    assert [r[0] for r in results] == [0 if _dead(i) else i % 6 for i in range(N)]  # nobody was cut
    results = b.run("open", wire)
    assert [r[0] for r in results] == [0 if _dead(i) else i % 6 for i in range(N)]
    wire = Wire(torch, plain_streams(42, big=False))
    a.run("seal", wire)
    results = b.run("echo", wire)
    assert [r[:1] + r[2:] for r in results] == [(0, M.ERROR_INVALID_STATE) if _dead(i) else (i % 6, 0) for i in range(N)]
    assert b.nonces(0) == [0 if _dead(i) else i % 6 for i in range(N)]
    a.free()
    b.free()


@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_unkeyed_slots_on_both_sides_of_a_cut(aead, gpu, oracle, cipher):
    import torch
    cutting = 34
    assert not _dead(cutting) and cutting % 6 == 4
    cap = sum(i % 6 for i in range(cutting) if not _dead(i)) + 2
    a, b = _pair(aead, torch, oracle, cipher, cap, 43)
    wire = Wire(torch, plain_streams(43, big=False))
    for tab, mode in ((a, "seal"), (b, "open")):
        results = tab.run(mode, wire)
        assert results[cutting] == (2, results[cutting][1], 0)
        for i in range(N):
            if _dead(i):
                assert results[i] == (0, 0, M.ERROR_INVALID_STATE), i
            elif i > cutting:
                assert results[i] == (0, 0, 0), i
        assert any(_dead(i) for i in range(cutting)) and any(_dead(i) for i in range(cutting + 1, N))
    a.free()
    b.free()


# ---------------------------------------------------------------- 3. re-key and clear

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_rekey_and_clear_after_traffic(aead, gpu, oracle, cipher):
    import torch
    keys = keys_for(51)
    total = sum(i % 6 for i in range(N))
    a, b = (Table(aead, torch, oracle, cipher, ini, total + 5, keys) for ini in (True, False))
    assert a.has_key() == [1] * N  # an object from _new starts with every slot keyed
    wire = Wire(torch, plain_streams(51, big=False))
    a.run("seal", wire)
    b.run("open", wire)
    assert a.nonces(0)[10] == b.nonces(1)[10] == 4
    fresh = keys_for(52, 2)
    cleared = [3, 20, 99, 66]
    for tab in (a, b):
        tab.set_keys([10, 40], fresh)
        tab.clear_keys(cleared)
        tab.check_state()
        tab.check_contexts()  # the named slots new or all zero, every other slot as it was
        assert [tab.has_key()[i] for i in (3, 20, 66, 10, 40, 11)] == [0, 0, 0, 1, 1, 1]
        assert tab.nonces(0)[10] == tab.nonces(1)[10] == tab.nonces(0)[20] == tab.nonces(1)[20] == 0
    plain = plain_streams(53, big=False)
    wire = Wire(torch, plain)
    results = a.run("seal", wire)
    for i in (3, 20, 66):
        assert results[i] == (0, 0, M.ERROR_INVALID_STATE)
    results = b.run("open", wire)
    opened = wire.streams()
    for at, L in T.walk(plain[10], 0)[0]:  # the peer opened the re-keyed slot, from nonce 0
        assert opened[10][at:at + L - 16] == plain[10][at:at + L - 16]
    assert results[10] == (4, results[10][1], 0) and b.nonces(1)[10] == 4 and a.nonces(0)[10] == 4
    assert b.nonces(1)[16] == a.nonces(0)[16] == 8  # a slot not named carried its nonces on
    a.free()
    b.free()


# ---------------------------------------------------------------- 4. subset calls

S_STOP, S_NONCE, S_FORGED, S_UNKEYED = 34, 5, 16, 13


def _entries(m):
    """the slot list of a call of m entries"""
    if m == N:
        return list(PERM)
    if m == 1:
        return [PERM[2]]
    slots = PERM[:m]
    slots[7], slots[50] = TOP, N
    assert S_UNKEYED in slots
    return slots


@pytest.mark.parametrize("m", [1, 64, 65, 67])
@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_subset_calls_equal_the_model_and_a_twin_full_call(aead, gpu, oracle, cipher, m):
    import torch
    keys = keys_for(61)
    plain = plain_streams(61, big=False)
    plain[S_STOP] = plain[S_STOP] + T.frame(bytes(4))  # an L < 16 stop after its frames
    slots = _entries(m)
    assert len(slots) == m and len(set(slots)) == m and slots != sorted(slots) or m == 1
    big = 400  # no object cap cuts
    tabs = {}
    for name, ini in (("a", True), ("a2", True), ("b", False), ("b2", False)):
        tab = tabs[name] = Table(aead, torch, oracle, cipher, ini, big, keys)
        tab.clear_keys([S_UNKEYED])
        tab.set_nonces(0 if ini else 1, {S_NONCE: T.NONCE_LIMIT - 1})  # one frame, then the nonce runs out
    a, a2, b, b2 = (tabs[k] for k in ("a", "a2", "b", "b2"))

    def entry_streams(per_slot):
        return [per_slot[i] if i < N else plain[5] for i in slots]

    def twin_streams(per_slot):
        return [per_slot[i] if i in slots else b"" for i in range(N)]

    # seal: a call whose cap cuts inside a listed session, then max_frames = 0 (the object's own) for the rest
    wire = Wire(torch, entry_streams(plain))
    cap, cutting = (3, 1) if m > 1 else (2, 0)
    first = a.run("seal", wire, slots, max_frames=cap)
    assert 0 < first[cutting][0] < len(T.walk(plain[slots[cutting]], 0)[0]) and first[cutting][2] == 0
    assert sum(r[0] for r in first) == cap
    for j, r in enumerate(first):
        wire.pos[j] += r[1]
    second = a.run("seal", wire, slots, max_frames=0)
    whole = [(f[0] + s[0], f[1] + s[1], s[2]) for f, s in zip(first, second)]
    wire2 = Wire(torch, twin_streams(plain))
    twin = a2.run("seal", wire2)
    sealed, sealed2 = wire.streams(), wire2.streams()
    for j, i in enumerate(slots):
        if i < N:
            assert sealed[j] == sealed2[i] and whole[j] == twin[i], (j, i)
        else:
            assert sealed[j] == plain[5] and whole[j] == (0, 0, M.ERROR_INVALID_PARAM)
    assert a.nonces(0) == a2.nonces(0) and a.nonces(1) == a2.nonces(1)
    if m > 1:
        assert whole[slots.index(S_STOP)][2] == T.ERROR_INVALID_LENGTH
        assert whole[slots.index(S_NONCE)] == (1, whole[slots.index(S_NONCE)][1], T.ERROR_INVALID_NONCE)
        assert whole[slots.index(S_UNKEYED)] == (0, 0, M.ERROR_INVALID_STATE)

    # open, with the last frame of one listed session forged; the cap given is the object's own
    per_slot = [bytearray(s) for s in sealed2]
    if m > 1:
        at, L = T.walk(sealed2[S_FORGED], 0)[0][-1]
        per_slot[S_FORGED][at + 3] ^= 0x20
    per_slot = [bytes(s) for s in per_slot]
    wire = Wire(torch, entry_streams(per_slot))
    got = b.run("open", wire, slots, max_frames=big)
    wire2 = Wire(torch, twin_streams(per_slot))
    twin = b2.run("open", wire2)
    opened, opened2 = wire.streams(), wire2.streams()
    for j, i in enumerate(slots):
        if i < N:
            assert opened[j] == opened2[i] and got[j] == twin[i], (j, i)
    assert b.nonces(0) == b2.nonces(0) and b.nonces(1) == b2.nonces(1)
    if m > 1:
        assert got[slots.index(S_FORGED)] == (3, at - 2, T.ERROR_MAC_FAILURE)
    else:  # alone: an unkeyed and an out-of-range entry
        for slot, code in ((S_UNKEYED, M.ERROR_INVALID_STATE), (TOP, M.ERROR_INVALID_PARAM), (N, M.ERROR_INVALID_PARAM)):
            for mode in ("seal", "open", "echo"):
                assert a.run(mode, Wire(torch, [plain[5]]), [slot]) == [(0, 0, code)]
    # an echo over the list: the server's two directions move together
    wire = Wire(torch, entry_streams(plain))
    a.run("seal", wire, slots)
    b.run("echo", wire, slots)
    for tab in tabs.values():
        tab.free()


# ---------------------------------------------------------------- 5. two handshake batches into one table

@pytest.mark.parametrize("name", ["Noise_XX_25519_ChaChaPoly_BLAKE2s", "Noise_NK_25519_AESGCM_SHA256"])
def test_two_handshake_batches_key_one_table(aead, gpu, oracle, name):
    """Batches of 5 and 7 sessions through noise_aead_dev_handshake_* to the
    split, then _set_keys with each handshake's own device status array into
    interleaved slots of an initiator and a responder table.  One session's
    messages are spoilt in flight: its slot stays unkeyed on both sides."""
    import torch
    A = aead
    v = basic_vector(name)
    cipher = T.CHACHAPOLY if "ChaChaPoly" in name else T.AESGCM
    ini_tab, res_tab = (Table(A, torch, oracle, cipher, ini, 64) for ini in (True, False))
    batches = [(5, [1, 3, 5, 7, 9], None), (7, [0, 2, 4, 6, 8, 66, 10], 2)]
    hands = []
    for n, slots, spoilt in batches:
        def tamper(j, rows, spoilt=spoilt):
            rows = [bytearray(r) for r in rows]
            rows[spoilt][-1] ^= 0x01
            return [bytes(r) for r in rows]
        sess = make_sessions(v, n, 70 + n)
        r = handshake(A, torch, oracle, v, sess, tamper=tamper if spoilt is not None else None, seed=70 + n)
        hands.append(r)
        want = [1 if i == spoilt else 0 for i in range(n)]
        assert [min(s, 1) for s in r["ini_status"]] == want and [min(s, 1) for s in r["res_status"]] == want
        assert spoilt is None or 1 in (r["ini_status"][spoilt], r["res_status"][spoilt])
        k1, k2, _ = r["ini_split"]
        for tab, side, status in ((ini_tab, r["ini"], r["ini_status"]), (res_tab, r["res"], r["res_status"])):
            tab.set_keys(slots, list(zip(k1, k2)), status,
                         ptrs=(side.k1.data_ptr(), side.k2.data_ptr(), A.dev_handshake_status(side.hs)))
            tab.check_state()
    keyed = [1, 3, 5, 7, 9, 0, 2, 6, 8, 66, 10]
    for tab in (ini_tab, res_tab):
        assert tab.has_key() == [1 if i in keyed else 0 for i in range(N)]
        tab.check_contexts()
    tick = [4, 66, 1, 0, 9, 10, 2]  # the failed session's slot among those with traffic
    plain = plain_streams(71, N, big=False)
    streams = [plain[i + 1] for i in range(len(tick))]
    for w, rd in ((ini_tab, res_tab), (res_tab, ini_tab), (ini_tab, res_tab)):
        wire = Wire(torch, streams)
        w.run("seal", wire, tick, max_frames=32)
        results = rd.run("open", wire, tick)
        opened = wire.streams()
        assert results[0] == (0, 0, M.ERROR_INVALID_STATE) and opened[0] == streams[0]
        for j in range(1, len(tick)):
            assert results[j] == ((j + 1) % 6, results[j][1], 0)
            for at, L in T.walk(streams[j], 0)[0]:
                assert opened[j][at:at + L - 16] == streams[j][at:at + L - 16]
    for x in (ini_tab, res_tab, *(r["ini"] for r in hands), *(r["res"] for r in hands)):
        x.free()


# ---------------------------------------------------------------- 6. small objects

def test_small_objects_and_the_rules_that_need_an_object(aead, gpu, oracle):
    import torch
    A = aead
    BAD = A.ERROR_INVALID_PARAM
    sp = torch.cuda.current_stream().cuda_stream
    calls = (A.dev_transport_seal_frames_of, A.dev_transport_open_frames_of, A.dev_transport_echo_frames_of)
    # n == 0: a valid object that owns nothing and launches nothing
    for cipher in CIPHERS:
        rc, tr = A.dev_transport_new_unkeyed(cipher, A.ROLE_RESPONDER, 0, max_frames=0, stream=sp)
        assert rc == 0 and tr and A.dev_transport_has_key(tr) == 0 and A.debug_transport_ctx(tr, 1) == (0, 0)
        assert A.dev_transport_clear_keys(tr, slots=0, m=0, stream=sp) == 0
        assert A.dev_transport_free(tr) == 0
    for cipher in CIPHERS:
        tab = Table(A, torch, oracle, cipher, True, 8, n=4)
        slots, keys = dev_u32([2, 0, 9, 3]), dev_bytes(bytes(range(128)) * 2)
        wire = Wire(torch, [T.frame(bytes(20))] * 4)
        off = torch.tensor(wire.offs, dtype=torch.int64, device="cuda")
        ln = torch.tensor(wire.lens, dtype=torch.int32, device="cuda")
        ok = dict(slots=slots.data_ptr(), wire=wire.dev.data_ptr(), off=off.data_ptr(), length=ln.data_ptr(),
                  result=wire.result.data_ptr(), stream=sp)
        # rules 3 to 6, in order, each with everything after it wrong as well
        for call in calls:
            assert call(tab.tr, m=5, max_frames=9, **{**ok, "wire": 0}) == BAD                      # m > n
            for k in ("slots", "wire", "off", "length", "result"):
                assert call(tab.tr, m=4, max_frames=9, **{**ok, k: 0}) == BAD, k                     # a NULL pointer
            assert call(tab.tr, m=4, max_frames=9, **ok) == BAD                                      # the cap
            for k, width in (("off", 8), ("length", 4), ("slots", 4)):
                for d in (0, width * 4 - 1, -16 * 4 + 1):
                    assert call(tab.tr, m=4, max_frames=8, **{**ok, "result": ok[k] + d}) == BAD, (k, d)
            assert call(tab.tr, m=0, max_frames=9, **{**ok, "result": ok["off"]}) == 0               # m == 0 first
        assert A.dev_transport_set_keys(tab.tr, slots=ok["slots"], m=5, k1=keys.data_ptr(), k2=keys.data_ptr()) == BAD
        assert A.dev_transport_set_keys(tab.tr, slots=ok["slots"], m=4, k1=0, k2=keys.data_ptr()) == BAD
        assert A.dev_transport_set_keys(tab.tr, slots=0, m=4, k1=keys.data_ptr(), k2=keys.data_ptr()) == BAD
        assert A.dev_transport_clear_keys(tab.tr, slots=ok["slots"], m=5) == BAD
        assert A.dev_transport_clear_keys(tab.tr, slots=0, m=4) == BAD
        tab.check_state()  # nothing was launched: every slot unkeyed, the wire as it was
        assert wire.streams() == [T.frame(bytes(20))] * 4
        # work in flight, then free: it waits, scrubs and frees
        assert A.dev_transport_set_keys(tab.tr, slots=ok["slots"], m=4, k1=keys.data_ptr(), k2=keys.data_ptr() + 128,
                                        stream=sp) == 0
        assert A.dev_transport_seal_frames_of(tab.tr, m=4, max_frames=0, **ok) == 0
        assert A.dev_transport_free(tab.tr) == 0
        torch.cuda.synchronize()
        after = wire.streams()
        assert after[2] == T.frame(bytes(20)) and after[0] != T.frame(bytes(20))  # entry 2 names slot 9 of 4
