#!/usr/bin/env python3
"""What the packet calls (include/noise_aead_hip.h section 13) cost over the
datagram calls of section 11, on identical payloads.

One table of 65 536 slots per role, ChaChaPoly and AESGCM, 1400-B payloads.  A
shape is E active slots with F packets each; the wire is E framed streams of F
datagram frames, so both calls work on the same bytes: the datagram call takes
the streams grouped, one entry per slot (its code is unchanged from the parent
commit: the yardstick); the packet call takes the frame bodies as a list in
scrambled arrival order — the slots scrambled, a slot's packets interleaved
with every other slot's.
    one1024, one65536    one packet per slot, 1 024 and 65 536 active slots
    sixteen              16 packets per slot on 4 096 slots, interleaved
    skew1024, skew65536  every packet on one slot: the serial run walk
Arms per shape: pk_seal / dg_seal, pk_open / dg_open, and pk_replay /
dg_replay, the open of a flood of replays (every window has seen the call's
counters before).

One call is timed with a pair of device events; between calls, untimed, the
wire, the nonces and the windows are put back.  The arms alternate call by
call inside a round, `--rounds` rounds after `--warmup`.  A line gives per arm
the median, minimum and maximum microseconds, and the packet arms as ratios to
the datagram arms.  Before the timing the two seals must give the same bytes
with every status 0, both opens must give every payload back with every status
0 and equal windows, and both replayed opens must give every status 5 and
change no byte.  DESIGN.md 4.17 records the figures.

    python tools/transport_packet_bench.py --out profiles/transport_packet.jsonl

--echo: what the packet echo (section 14) costs beside the two calls it is
defined by.  The initiator seals the list; the responder then answers it, in
the same process, on the same object and lists, in two arms that alternate call
by call: `echo`, one _echo_packets call, and `pair`, _open_packets followed at
once by _seal_packets of the whole list — what a server does today if it
refuses to synchronise in the middle of its tick (every packet is accepted, so
the whole list is the sub-list of the accepted).  The shapes are 1 024 and
65 536 packets at 1 and at 16 interleaved packets per slot.  Before the timing
both arms must leave the same bytes, statuses, windows and send counters, every
status 0, and the initiator must open every reply to the payload it sent.
DESIGN.md 4.18 records the figures.

    python tools/transport_packet_bench.py --echo --out profiles/transport_packet_echo.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "noise-c_amd")]

N = 65536
PLAIN = 1400
WINDOW_BYTES = 136
ECHO_SHAPES = {"one1024": (1024, 1), "one65536": (N, 1), "sixteen1024": (64, 16), "sixteen65536": (4096, 16)}
SHAPES = {"one1024": (1024, 1), "one65536": (N, 1), "sixteen": (4096, 16), "skew1024": (1, 1024), "skew65536": (1, N)}


def stat(v):
    med = statistics.median(v)
    return dict(us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                spread=round((max(v) - min(v)) / med, 4))


def echo_arms(A, torch, hip, dev, sp, ini, res, pk, pk_seal, reset, windows, timed, wire, plain, rows, pstat):
    """--echo on one shape: (the line's own fields, whether both arms computed the same and the peer read it)"""
    count, stride = rows.shape
    send_ptr, ini_win = A.dev_transport_nonces(res, 0), A.dev_transport_replay(ini)[0]

    def echo():
        return A.dev_transport_echo_packets(res, **pk)

    def pair():
        return A.dev_transport_open_packets(res, **pk) or A.dev_transport_seal_packets(res, **pk)

    def rewind():
        reset()
        assert hip.hipMemsetAsync(send_ptr, 0, 8 * N, sp) == 0

    def sends():
        v = torch.empty(N, dtype=torch.int64, device=dev)
        assert hip.hipMemcpyAsync(v.data_ptr(), send_ptr, 8 * N, 3, sp) == 0
        return v

    # the receive batch: the list as the initiator seals it
    wire.copy_(plain)
    rewind()
    assert pk_seal() == 0
    torch.cuda.synchronize(dev)
    ok = not pstat.any()
    sealed = wire.clone()
    left = {}
    for name, fn in (("echo", echo), ("pair", pair)):
        wire.copy_(sealed)
        rewind()
        assert fn() == 0
        torch.cuda.synchronize(dev)
        ok = ok and not pstat.any()
        left[name] = (wire.clone(), pstat.clone(), windows(), sends())
    ok = ok and all(torch.equal(x, y) for x, y in zip(left["echo"], left["pair"]))
    ok = ok and int(left["echo"][3].sum()) == count  # every packet took a send counter
    # the initiator opens the replies: the payloads it sent
    wire.copy_(left["echo"][0])
    assert A.dev_transport_open_packets(ini, **pk) == 0
    torch.cuda.synchronize(dev)
    w = wire[:count * stride].view(count, stride)
    ok = ok and not pstat.any() and torch.equal(w[:, 10:10 + PLAIN], rows[:, 10:10 + PLAIN])
    assert hip.hipMemsetAsync(ini_win, 0, N * WINDOW_BYTES, sp) == 0

    def before(name):
        wire.copy_(sealed)
        rewind()
    times = timed({"echo": echo, "pair": pair}, before)
    ok = ok and not pstat.any()
    med = {a: statistics.median(v) for a, v in times.items()}
    line = dict(echo=stat(times["echo"]), pair=stat(times["pair"]), echo_over_pair=round(med["echo"] / med["pair"], 4),
                saved_us=round(med["pair"] - med["echo"], 1))
    return line, bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ciphers", default="ChaChaPoly,AESGCM")
    ap.add_argument("--echo", action="store_true", help="time _echo_packets against _open_packets + _seal_packets")
    ap.add_argument("--shapes", default=None, help="default: every shape of the mode")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = ECHO_SHAPES if args.echo else SHAPES

    import numpy as np
    import torch
    import noise_aead as A
    A.lib()
    assert torch.cuda.is_available(), "transport_packet_bench needs the GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_s = torch.cuda.current_stream(dev)
    sp = main_s.cuda_stream
    hip = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    lines, bad = [], 0
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(arms, before):
        """{arm: [µs]}: the arms alternate inside a round; before(name) runs untimed"""
        times = {k: [] for k in arms}
        for rnd in range(args.warmup + args.rounds):
            for name, fn in arms.items():
                before(name)
                t0.record(main_s)
                rc = fn()
                t1.record(main_s)
                torch.cuda.synchronize(dev)
                if rc:
                    raise RuntimeError(f"{name}: {rc:#x}")
                if rnd >= args.warmup:
                    times[name].append(t0.elapsed_time(t1) * 1000.0)
        return times

    k1 = torch.empty(N * 32, dtype=torch.uint8, device=dev)
    k2 = torch.empty(N * 32, dtype=torch.uint8, device=dev)
    assert A.dev_fill_splitmix(k1.data_ptr(), N * 32, 0x4B31, 0, sp) == 0
    assert A.dev_fill_splitmix(k2.data_ptr(), N * 32, 0x4B32, 0, sp) == 0
    device_name = torch.cuda.get_device_name(dev)
    body = 8 + PLAIN + 16
    stride = 2 + body

    for cname in args.ciphers.split(","):
        cipher = {"ChaChaPoly": A.CHACHAPOLY, "AESGCM": A.AESGCM}[cname]
        tabs = []
        for role in (A.ROLE_INITIATOR, A.ROLE_RESPONDER):
            rc, tr = A.dev_transport_new(cipher, role, N, k1=k1.data_ptr(), k2=k2.data_ptr(), max_frames=N, stream=sp)
            assert rc == 0, hex(rc)
            assert A.dev_transport_reserve_packets(tr, N, sp) == 0
            tabs.append(tr)
        ini, res = tabs
        win_ptr, bits = A.dev_transport_replay(res)
        assert win_ptr and bits == 1024
        seen = torch.empty(N * WINDOW_BYTES, dtype=torch.uint8, device=dev)  # the windows after the call's counters

        def windows():
            w = torch.empty(N * WINDOW_BYTES, dtype=torch.uint8, device=dev)
            assert hip.hipMemcpyAsync(w.data_ptr(), win_ptr, N * WINDOW_BYTES, 3, sp) == 0
            return w

        def reset(saved=None):
            for tr, d in ((ini, 0), (res, 1)):
                assert hip.hipMemsetAsync(A.dev_transport_nonces(tr, d), 0, 8 * N, sp) == 0
            if saved is None:
                assert hip.hipMemsetAsync(win_ptr, 0, N * WINDOW_BYTES, sp) == 0
            else:
                assert hip.hipMemcpyAsync(win_ptr, saved.data_ptr(), N * WINDOW_BYTES, 3, sp) == 0

        for shape in (args.shapes.split(",") if args.shapes else shapes):
            E, F = shapes[shape]
            count = E * F
            # E streams of F frames, random but for the headers and the counters' room
            plain = torch.empty(count * stride + 64, dtype=torch.uint8, device=dev)
            assert A.dev_fill_splitmix(plain.data_ptr(), count * stride + 64, 0x5452, 0, sp) == 0
            rows = plain[:count * stride].view(count, stride)
            rows[:, 0] = body >> 8
            rows[:, 1] = body & 0xFF
            rows[:, 2:10] = 0
            slots = ((np.arange(E, dtype=np.int64) * 40503 + 7) % N)  # E distinct slots, unsorted
            d_slots = torch.from_numpy(slots.astype(np.uint32).view(np.int32)).to(dev)
            d_off = torch.arange(E, device=dev, dtype=torch.int64) * (F * stride)
            d_len = torch.full((E,), F * stride, dtype=torch.int32, device=dev)
            # the list: packet p is frame p // E of entry perm[p % E] — arrival order scrambled, a slot's own order kept
            perm = (np.arange(E, dtype=np.int64) * 25173 + 11) % E if E > 1 else np.zeros(1, dtype=np.int64)
            assert len(set(perm.tolist())) == E
            p = np.arange(count, dtype=np.int64)
            entry, k = perm[p % E], p // E
            listed = np.zeros(count, dtype=np.dtype(A.PACKET_DT))
            listed["off"] = (entry * F + k) * stride + 2
            listed["len"] = body
            listed["slot"] = slots[entry]
            d_list = torch.from_numpy(listed.view(np.uint8).copy()).to(dev)
            frame_of = torch.from_numpy(entry * F + k).to(dev)  # the frame of the wire that packet p is
            wire = plain.clone()
            r16 = torch.zeros((E, 4), dtype=torch.int32, device=dev)
            r24 = torch.zeros((E, 6), dtype=torch.int32, device=dev)
            fstat = torch.full((count,), 0xEE, dtype=torch.uint8, device=dev)
            pstat = torch.full((count,), 0xEE, dtype=torch.uint8, device=dev)
            dg = dict(slots=d_slots.data_ptr(), m=E, max_frames=count, wire=wire.data_ptr(), off=d_off.data_ptr(),
                      length=d_len.data_ptr(), stream=sp)
            pk = dict(packets=d_list.data_ptr(), count=count, wire=wire.data_ptr(), status=pstat.data_ptr(), stream=sp)

            def dg_seal():
                return A.dev_transport_seal_datagrams(ini, result=r16.data_ptr(), **dg)

            def dg_open():
                return A.dev_transport_open_datagrams(res, result=r24.data_ptr(), frame_status=fstat.data_ptr(), **dg)

            def pk_seal():
                return A.dev_transport_seal_packets(ini, **pk)

            def pk_open():
                return A.dev_transport_open_packets(res, **pk)

            if args.echo:
                line, ok = echo_arms(A, torch, hip, dev, sp, ini, res, pk, pk_seal, reset, windows, timed, wire, plain, rows, pstat)
                bad += not ok
                lines.append(json.dumps(dict(
                    shape=shape, cipher=cname, slots=N, active=E, packets_per_slot=F, packets=count, payload=PLAIN,
                    rounds=args.rounds, warmup=args.warmup, device=device_name, **line, verified=bool(ok))))
                print(lines[-1], flush=True)
                del plain, rows, wire
                torch.cuda.empty_cache()
                continue

            # ---- the arms compute the same bytes
            reset()
            assert dg_seal() == 0
            torch.cuda.synchronize(dev)
            r = r16.cpu().numpy()
            ok = int(r[:, 0].sum()) == count and not r[:, 2].any()
            sealed = wire.clone()
            wire.copy_(plain)
            reset()
            assert pk_seal() == 0
            torch.cuda.synchronize(dev)
            ok = ok and torch.equal(wire, sealed) and not pstat.any()
            counters = sealed[:count * stride].view(count, stride)[:, 2:10].contiguous().view(torch.int64).view(count)
            ok = ok and torch.equal(counters[frame_of], torch.from_numpy(k).to(dev))  # send + k, k counted in list order
            opened = {}
            for name, fn, status in (("dg", dg_open, fstat), ("pk", pk_open, pstat)):
                wire.copy_(sealed)
                reset()
                assert fn() == 0
                torch.cuda.synchronize(dev)
                ok = ok and not status.any()
                w = wire[:count * stride].view(count, stride)  # the payloads back, the counters as sealed
                ok = ok and torch.equal(w[:, 10:10 + PLAIN], rows[:, 10:10 + PLAIN])
                ok = ok and torch.equal(w[:, :10], sealed[:count * stride].view(count, stride)[:, :10])
                opened[name] = windows()
                wire.copy_(sealed)
                assert fn() == 0  # every packet again
                torch.cuda.synchronize(dev)
                ok = ok and bool((status == 5).all()) and torch.equal(wire, sealed) and torch.equal(windows(), opened[name])
            ok = ok and torch.equal(opened["dg"], opened["pk"])
            seen.copy_(opened["pk"])
            bad += not ok

            arms = {"pk_seal": pk_seal, "dg_seal": dg_seal, "pk_open": pk_open, "dg_open": dg_open,
                    "pk_replay": pk_open, "dg_replay": dg_open}

            def before(name):
                wire.copy_(plain if name.endswith("seal") else sealed)
                reset(seen if name.endswith("replay") else None)
            times = timed(arms, before)
            bad += not (bool((fstat == 5).all()) and bool((pstat == 5).all()))  # the last arms were the replays
            med = {a: statistics.median(v) for a, v in times.items()}
            lines.append(json.dumps(dict(
                shape=shape, cipher=cname, slots=N, active=E, packets_per_slot=F, packets=count, payload=PLAIN,
                rounds=args.rounds, warmup=args.warmup, device=device_name, **{a: stat(v) for a, v in times.items()},
                seal_over_datagrams=round(med["pk_seal"] / med["dg_seal"], 4),
                open_over_datagrams=round(med["pk_open"] / med["dg_open"], 4),
                replay_over_datagrams=round(med["pk_replay"] / med["dg_replay"], 4), verified=bool(ok))))
            print(lines[-1], flush=True)
            del plain, rows, wire, sealed, opened, w
            torch.cuda.empty_cache()
        for tr in tabs:
            A.dev_transport_free(tr)
        del seen
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
