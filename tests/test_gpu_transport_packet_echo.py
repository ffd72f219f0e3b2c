"""Packet echo: noise_aead_dev_transport_echo_packets (header section 14).

Every call is compared with tests/transport_packet_echo_model.py, the
composition of the two section-13 models that the header defines the call by
(held to a loop written by hand by tests/test_transport_packet_echo_host.py):
every byte of the wire with the guard bytes between the packets, every status,
both nonce arrays and every word of the windows.  A status-5 packet that only
an earlier packet of the same call made a replay may hold its bytes as given
or its plaintext; the batches plant those, at most one packet in eight.  The
tables have 6 slots, one of them unkeyed, and are reserved for 256 packets
unless the test is about another count.  The helpers are those of
tests/transport_packet_gpu.py."""
import numpy as np
import pytest

import transport_model as T
import transport_datagram_model as D
import transport_packet_echo_model as E
import transport_rekey_model as R
from gpu_support import dev_u32
from transport_gpu import CIPHERS, keys_for
from transport_packet_gpu import (CANARY, FIRST, KEYED, PAYLOADS, SENDS, SLOTS, TOP64, UNKEYED, UNTOUCHED, Table, echo_batch, lay,
                                  made, on_device, preset, room, uploaded)

pytestmark = pytest.mark.gpu
IDS = ["ChaChaPoly", "AESGCM"]
RESERVED = 256


def table(aead, torch, oracle, cipher, initiator, keys, reserved=RESERVED):
    t = Table(aead, torch, oracle, cipher, initiator, 8, keys, n=SLOTS)
    t.clear_keys([UNKEYED])
    t.reserve(reserved)
    return t


def responder(aead, torch, oracle, cipher, keys, reserved=RESERVED):
    """the echoing side in the state the batches are made for"""
    b = table(aead, torch, oracle, cipher, False, keys, reserved)
    preset(b)
    return b


def counters(wire, packets, statuses):
    """per slot, the counters in front of the echoed packets, in list order"""
    out = {}
    for (off, _, slot), st in zip(packets, statuses):
        if st == 0:
            out.setdefault(slot, []).append(int.from_bytes(wire[off:off + 8], "little"))
    return out


# ---------------------------------------------------------------- 1. scrambled lists against the model

def scrambled(aead, torch, oracle, cipher, count, payloads=PAYLOADS, reserved=RESERVED):
    keys = keys_for(600 + count, SLOTS)
    b = responder(aead, torch, oracle, cipher, keys, reserved)
    batch = echo_batch(oracle, cipher, keys, count, 610 + count, payloads)
    packets = batch["packets"]
    want = b.modelled("echo", batch["wire"], packets)
    # on the CPU, before any launch: the list holds every cause, and few packets that may hold either
    if count > 1:  # a list of one packet holds one status
        assert {0, 1, 4, 5, 6} == set(want[1]) and want[2]
        assert D.window(b.model[2]).top > FIRST[2] + 1500  # the jump of a window and more happened
    else:
        assert want[1] == [0]
    assert 8 * len(want[2]) <= count
    d_wire, listed = on_device(torch, batch["wire"]), uploaded(torch, packets)
    b.launch("echo", d_wire, listed)
    got, statuses, _ = b.compare("echo", want, packets, d_wire, listed)
    assert b.nonces(1) == [0] * SLOTS  # the receive nonces are not in it
    taken = counters(got, packets, statuses)
    for i in KEYED:  # send + k for the k-th echoed packet of the slot, with no gap for the refused ones between
        assert taken.get(i, []) == list(range(SENDS[i], SENDS[i] + statuses_of(packets, statuses, i).count(0)))
    b.free()
    return batch, got, statuses


def statuses_of(packets, statuses, slot):
    return [st for (_, _, s), st in zip(packets, statuses) if s == slot]


@pytest.mark.parametrize("count", [1, 64, 65, 200])
@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_scrambled_lists_against_the_model(aead, gpu, oracle, cipher, count):
    """64 and 65 put run heads on both sides of a workgroup's border"""
    import torch
    scrambled(aead, torch, oracle, cipher, count)


# ---------------------------------------------------------------- 2. against the two calls

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_echo_equals_open_then_seal_of_the_accepted(aead, gpu, oracle, cipher):
    import torch
    keys = keys_for(621, SLOTS)
    one, two = (responder(aead, torch, oracle, cipher, keys) for _ in range(2))
    batch = echo_batch(oracle, cipher, keys, 200, 622)
    packets = batch["packets"]
    wire1, wire2 = on_device(torch, batch["wire"]), on_device(torch, batch["wire"])
    listed1 = uploaded(torch, packets)
    one.launch("echo", wire1, listed1)
    # the other table: the open, the statuses read on the host, the seal over the sub-list built there
    listed2 = uploaded(torch, packets)
    two.launch("open", wire2, listed2)
    torch.cuda.synchronize()
    merged = listed2[1].clone()
    accepted = [p for p, st in enumerate(listed2[1][:len(packets)].tolist()) if st == 0]
    assert accepted and len(accepted) < len(packets)
    listed3 = uploaded(torch, [packets[p] for p in accepted])
    two.launch("seal", wire2, listed3)
    torch.cuda.synchronize()
    merged[torch.tensor(accepted, device="cuda")] = listed3[1][:len(accepted)]
    assert torch.equal(wire1, wire2)
    assert torch.equal(listed1[1], merged)
    assert {0, 1, 4, 5, 6} == set(merged[:len(packets)].tolist())
    def words(values):  # 64-bit words as a tensor
        return torch.from_numpy(np.array(values, dtype=np.uint64).view(np.int64))
    assert torch.equal(words(one.windows()), words(two.windows())) and any(w[0] for w in one.windows())
    assert torch.equal(words(one.nonces(0)), words(two.nonces(0))) and one.nonces(0) != [SENDS.get(i, 0) for i in range(SLOTS)]
    assert one.nonces(1) == two.nonces(1) == [0] * SLOTS
    one.free()
    two.free()


# ---------------------------------------------------------------- 3. the peer reads the replies

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_the_peer_opens_every_reply(aead, gpu, oracle, cipher):
    import torch
    keys = keys_for(631, SLOTS)
    a, b = table(aead, torch, oracle, cipher, True, keys), responder(aead, torch, oracle, cipher, keys)
    batch = echo_batch(oracle, cipher, keys, 200, 632)
    packets = batch["packets"]
    d_wire = on_device(torch, batch["wire"])
    _, statuses, _ = b.packets("echo", d_wire, packets)
    replies = [p for p, st in enumerate(statuses) if st == 0]
    assert len(replies) > 100
    opened, back, either = a.packets("open", d_wire, [packets[p] for p in replies])
    assert back == [0] * len(replies) and not either
    for p in replies:
        off, ln, _ = packets[p]
        assert opened[off + 8:off + ln - 16] == batch["sent"][p]
    # the initiator's windows hold exactly the counters send .. send + k - 1 of each slot
    have = a.windows()
    for i in range(SLOTS):
        w = D.Window()
        for c in range(SENDS.get(i, 0), SENDS.get(i, 0) + statuses_of(packets, statuses, i).count(0)):
            w.accept(c)
        assert have[i] == w.words(), i
    a.free()
    b.free()


# ---------------------------------------------------------------- 4. one slot, 200 packets

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_one_run_of_200_packets(aead, gpu, oracle, cipher):
    """one lane walks what four workgroups' lanes stand beside"""
    import torch
    keys = keys_for(641, SLOTS)
    b = responder(aead, torch, oracle, cipher, keys)
    batch = echo_batch(oracle, cipher, keys, 200, 642, slots=(4,))
    packets = batch["packets"]
    assert sum(1 for _, _, s in packets if s == 4) > 150
    d_wire = on_device(torch, batch["wire"])
    got, statuses, either = b.packets("echo", d_wire, packets)
    mine = statuses_of(packets, statuses, 4)
    assert {0, 1, 4, 5} == set(mine) and either
    assert counters(got, packets, statuses)[4] == list(range(SENDS[4], SENDS[4] + mine.count(0)))
    assert b.nonces(0)[4] == SENDS[4] + mine.count(0)
    b.free()


# ---------------------------------------------------------------- 5. the send counter runs out

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_echo_stops_where_the_send_counter_runs_out(aead, gpu, oracle, cipher):
    import torch
    keys = keys_for(651, SLOTS)
    b = table(aead, torch, oracle, cipher, False, keys)
    b.set_nonces(0, {5: TOP64 - 2, 0: 40})
    rng = np.random.default_rng(651)
    slots = [5, 0, 5, 5, 0, 5, 5]
    arrived = {5: iter((3, 1, 2, 0, 4)), 0: iter((7, 8))}
    payloads = [rng.integers(0, 256, PAYLOADS[2 + k], dtype=np.uint8).tobytes() for k in range(len(slots))]
    parts = [made(oracle, cipher, keys[s][0], next(arrived[s]), payloads[k]) for k, s in enumerate(slots)]
    wire, offs = lay(parts)
    packets = [(offs[k], len(parts[k]), s) for k, s in enumerate(slots)]
    d_wire = on_device(torch, wire)
    got, statuses, either = b.packets("echo", d_wire, packets)
    assert statuses == [0, 0, 0, 5, 0, 5, 5] and not either
    assert counters(got, packets, statuses) == {5: [TOP64 - 2, TOP64 - 1], 0: [40, 41]}
    for k in (3, 5, 6):  # opened, not echoed: the received counter in front, the plaintext, the tag bytes as they were
        assert got[offs[k]:offs[k] + len(parts[k])] == parts[k][:8] + payloads[k] + parts[k][-16:]
    assert b.windows()[5][:2] == [5, 0b11111] and b.windows()[0][:2] == [9, 0b110000000]
    assert b.nonces(0)[5] == TOP64 and b.nonces(0)[0] == 42
    # once more: the slot stays where it is, and its window goes on accepting
    again = [made(oracle, cipher, keys[5][0], 9, b"late")]
    wire, offs = lay(again)
    got, statuses, _ = b.packets("echo", on_device(torch, wire), [(offs[0], len(again[0]), 5)])
    assert statuses == [5] and b.nonces(0)[5] == TOP64 and b.windows()[5][0] == 10
    b.free()


# ---------------------------------------------------------------- 6. nothing refused is touched

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_refused_packets_are_as_given_and_take_no_counter(aead, gpu, oracle, cipher):
    import torch
    keys = keys_for(661, SLOTS)
    b = responder(aead, torch, oracle, cipher, keys)
    batch = echo_batch(oracle, cipher, keys, 128, 662)
    packets, parts = batch["packets"], batch["parts"]
    d_wire = on_device(torch, batch["wire"])
    got, statuses, either = b.packets("echo", d_wire, packets)
    mask = np.frombuffer(got, dtype=np.uint8).copy()
    seen = set()
    for p, (off, ln, slot) in enumerate(packets):
        if statuses[p] in (1, 4, 6) or (statuses[p] == 5 and p not in either):
            assert got[off:off + len(parts[p])] == parts[p], (p, statuses[p])  # forged, bad length, no session, refused as the window stood
            seen.add(statuses[p])
        mask[off:off + len(parts[p])] = CANARY
    assert seen == {1, 4, 5, 6}
    assert (mask == CANARY).all()  # the canaries around every packet
    sends = b.nonces(0)
    for i in range(SLOTS):  # the echoed packets of a slot are the advance of its send
        assert statuses_of(packets, statuses, i).count(0) == sends[i] - SENDS.get(i, 0)
    assert sends[UNKEYED] == 0
    b.free()


# ---------------------------------------------------------------- 7. composition in one stream

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_echo_composes_in_stream_order_without_a_wait(aead, gpu, oracle, cipher):
    """echo -> _seal_packets -> _rekey of the send direction -> echo: four calls launched back to back"""
    import torch
    keys = keys_for(671, SLOTS)
    b = responder(aead, torch, oracle, cipher, keys)
    first = echo_batch(oracle, cipher, keys, 64, 672)
    rng = np.random.default_rng(673)
    pushed = [room(rng.integers(0, 256, PAYLOADS[k % len(PAYLOADS)], dtype=np.uint8).tobytes()) for k in range(20)]
    wire2, offs2 = lay(pushed)
    packets2 = [(offs2[k], len(pushed[k]), (0, 1, UNKEYED, 4, 1)[k % 5]) for k in range(20)]
    # the second batch: counters above everything the first one brought, a replay of the first one's among them
    second = []
    for k in range(30):
        slot = KEYED[(3 * k) % len(KEYED)]
        second.append(made(oracle, cipher, keys[slot][0], FIRST[slot] + 5000 + k // 2, rng.integers(0, 256, PAYLOADS[k % 10], dtype=np.uint8).tobytes()))
    second.append(first["parts"][0])
    wire3, offs3 = lay(second)
    packets3 = [(offs3[k], len(second[k]), KEYED[(3 * k) % len(KEYED)]) for k in range(30)] + [(offs3[30], len(second[30]), first["packets"][0][2])]
    d1, d2, d3 = on_device(torch, first["wire"]), on_device(torch, wire2), on_device(torch, wire3)
    l1, l2, l3 = uploaded(torch, first["packets"]), uploaded(torch, packets2), uploaded(torch, packets3)
    d_slots = dev_u32(list(range(SLOTS)))
    torch.cuda.synchronize()
    b.launch("echo", d1, l1)
    b.launch("seal", d2, l2)
    assert aead.dev_transport_rekey(b.tr, slots=d_slots.data_ptr(), m=SLOTS, directions=R.SEND, stream=b.sp) == 0
    b.launch("echo", d3, l3)
    # the model, call by call; the device state is compared after the last
    want1 = b.modelled("echo", first["wire"], first["packets"])
    sends = [m.send if m else 0 for m in b.model]
    want2 = b.modelled("seal", wire2, packets2)
    assert len(R.rekey_table(b.model, R.SEND, SLOTS, list(range(SLOTS)))) == len(KEYED)
    want3 = b.modelled("echo", wire3, packets3)
    b.compare("echo", want1, first["packets"], d1, l1, state=False)
    sealed, st2, _ = b.compare("seal", want2, packets2, d2, l2, state=False)
    got3, st3, _ = b.compare("echo", want3, packets3, d3, l3)
    # the seal's counters go on from where the first echo left the sends
    taken = counters(sealed, packets2, st2)
    assert set(st2) == {0, 6} and all(taken[i] == list(range(sends[i], sends[i] + len(taken[i]))) for i in taken)
    assert st3[:30] == [0] * 30 and st3[30] == 5  # the first batch's packet again: its window has it
    # the second echo's replies are under the next key
    off, ln, slot = packets3[0]
    c = int.from_bytes(got3[off:off + 8], "little")
    old = T.Session.of_role(oracle, cipher, False, *keys[slot]).send_key
    assert oracle.decrypt(cipher, R.rekey(oracle, cipher, old), c, got3[off + 8:off + ln])[0] == 0
    assert oracle.decrypt(cipher, old, c, got3[off + 8:off + ln])[0] != 0
    b.free()


# ---------------------------------------------------------------- 8. past one sort block

@pytest.mark.parametrize("cipher", CIPHERS, ids=IDS)
def test_scrambled_list_past_one_sort_block(aead, gpu, oracle, cipher):
    """1500 packets: the device sort's path for more than one workgroup's worth"""
    import torch
    scrambled(aead, torch, oracle, cipher, 1500, payloads=(0, 1, 15, 16, 17), reserved=1500)


# ---------------------------------------------------------------- 9. small object rules

def test_echo_argument_rules_on_a_small_object(aead, gpu, oracle):
    """the rules that need a reservation; a refused call launches nothing"""
    import torch
    A = aead
    BAD, STATE = A.ERROR_INVALID_PARAM, A.ERROR_INVALID_STATE
    keys = keys_for(691, 4)
    tab = Table(A, torch, oracle, T.CHACHAPOLY, False, 8, keys, n=4)
    parts = [made(oracle, T.CHACHAPOLY, keys[k % 4][0], k // 4, b"twenty bytes of load") for k in range(9)]
    wire, offs = lay(parts)
    d_wire = on_device(torch, wire)
    packets = [(offs[k], len(parts[k]), k % 4) for k in range(9)]
    # one allocation: 8 status bytes, the list of 8 (8-byte aligned), 8 status bytes — touching it on both sides
    arr = np.array(packets[:8], dtype=np.dtype(A.PACKET_DT)).view(np.uint8)
    block = torch.full((8 + 128 + 8 + 16,), UNTOUCHED, dtype=torch.uint8, device="cuda")
    block[8:136] = torch.from_numpy(arr.copy()).cuda()
    base = block.data_ptr()
    assert base % 8 == 0
    ok = dict(packets=base + 8, wire=d_wire.data_ptr(), status=base + 136, stream=tab.sp)
    call = A.dev_transport_echo_packets
    assert call(tab.tr, count=8, **ok) == STATE and call(tab.tr, count=0, **ok) == 0  # not reserved yet
    tab.reserve(8)
    assert call(tab.tr, count=9, **{**ok, "packets": 0}) == BAD                        # count > max_packets
    for k in ("packets", "wire", "status"):
        assert call(tab.tr, count=8, **{**ok, k: 0, **({} if k == "status" else {"status": base + 8})}) == BAD, k
    for status in (base + 8, base + 1, base + 135, base + 8 + 64):
        assert call(tab.tr, count=8, **{**ok, "status": status}) == BAD, status - base  # the statuses meet the list
    assert call(tab.tr, count=0, **{**ok, "status": base + 8}) == 0                    # count == 0 first
    torch.cuda.synchronize()
    tab.check_state()  # nothing was launched: no window or send moved, the wire and the block as they were
    assert d_wire.cpu().numpy().tobytes() == bytes(wire)
    assert (block[:8] == UNTOUCHED).all() and (block[136:] == UNTOUCHED).all() and (block[8:136].cpu() == torch.from_numpy(arr)).all()
    # count == max_packets works, with the statuses touching the list from above
    want_wire, want, _ = E.run_echo(tab.model, bytes(wire), packets[:8])
    assert call(tab.tr, count=8, **ok) == 0
    torch.cuda.synchronize()
    assert block[136:144].tolist() == want == [0] * 8 and d_wire.cpu().numpy().tobytes() == want_wire
    assert (block[:8] == UNTOUCHED).all() and (block[144:] == UNTOUCHED).all() and (block[8:136].cpu() == torch.from_numpy(arr)).all()
    tab.check_state()
    assert tab.nonces(0) == [2, 2, 2, 2]
    tab.free()
    # an object with n == 0: every packet has no session
    rc, tr = A.dev_transport_new_unkeyed(A.AESGCM, A.ROLE_RESPONDER, 0, max_frames=0, stream=tab.sp)
    assert rc == 0 and tr
    assert A.dev_transport_reserve_packets(tr, 4, tab.sp) == 0
    d_wire = on_device(torch, wire)
    listed = uploaded(torch, packets[:3] + [(0, 0, 2 ** 32 - 1)])
    assert call(tr, packets=listed[0].data_ptr(), count=4, wire=d_wire.data_ptr(), status=listed[1].data_ptr(), stream=tab.sp) == 0
    torch.cuda.synchronize()
    assert listed[1].tolist() == [6] * 4 + [UNTOUCHED] * 16
    assert call(tr, packets=listed[0].data_ptr(), count=5, wire=d_wire.data_ptr(), status=listed[1].data_ptr(), stream=tab.sp) == BAD
    assert d_wire.cpu().numpy().tobytes() == bytes(wire)
    assert A.dev_transport_free(tr) == 0
