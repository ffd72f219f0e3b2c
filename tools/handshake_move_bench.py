#!/usr/bin/env python3
"""What taking a cohort out of a pool costs a server
(noise_aead_dev_handshake_new_like / _move, header section 16).

65 536 XX responders (ChaChaPoly/BLAKE2s, 16-byte payloads) have read the first
message and written the second; they are parked in a pool.  Arm 1 is a tick
that finishes m of them — _new_like(pool, m), _move of m scattered pool lanes
into it, read of message 3, split — at m = 64, 4096 and 65 536.  Arm 2 is the
read of message 3 and the split of an object of m sessions made by _new and
driven in lockstep to the same position: what the tick costs without the two
new calls.  Both alternate inside a round and are timed with device events over
`--reps` ticks per window; everything else (making the objects of arm 2,
putting the moved sessions back into the pool, the frees) lies outside the
window.  _move alone is timed the same way.

Before any timing the keys of the moved cohort are compared with those of the
same sessions finished in lockstep: equal and not zero.  DESIGN.md 4.20
records the figures.

    python tools/handshake_move_bench.py --out profiles/handshake_move.jsonl
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "noise-c_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

PAYLOAD = 16
XX = "Noise_XX_25519_ChaChaPoly_BLAKE2s"
X = (PAYLOAD + 32, PAYLOAD + 96, PAYLOAD + 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=65536)
    ap.add_argument("--m", default="64,4096,65536")
    ap.add_argument("--reps", type=int, default=4, help="ticks per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import noise_aead as A
    A.lib()
    assert torch.cuda.is_available(), "handshake_move_bench needs the GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_s = torch.cuda.current_stream(dev)
    sp = main_s.cuda_stream
    n = args.pool
    lines, bad = [], 0

    def filled(nbytes, word0):
        t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert A.dev_fill_splitmix(t.data_ptr(), nbytes, 0x4D56, word0, sp) == 0
        return t

    def zeros(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def ok(rc, what):
        if rc:
            raise RuntimeError(f"{what}: {rc:#x}")

    def new(initiator, count):
        s, e = (ini_s, ini_e) if initiator else (res_s, res_e)
        rc, hs = A.dev_handshake_new(XX, A.ROLE_INITIATOR if initiator else A.ROLE_RESPONDER, count, stream=sp,
                                     local_static=s.data_ptr(), local_ephemeral=e.data_ptr())
        ok(rc, "new")
        return hs

    def write(hs, msg, mlen, rows=None):
        rows = payload if rows is None else rows
        ok(A.dev_handshake_write_message(hs, payload=rows.data_ptr(), payload_stride=PAYLOAD, payload_len=PAYLOAD,
                                         msg=msg.data_ptr(), msg_stride=mlen, stream=sp), "write")

    def read(hs, msg, mlen):
        ok(A.dev_handshake_read_message(hs, msg=msg.data_ptr(), msg_stride=mlen, msg_len=mlen, payload=got.data_ptr(),
                                        payload_stride=PAYLOAD, stream=sp), "read")

    def split(hs, k1, k2, h):
        ok(A.dev_handshake_split(hs, k1=k1.data_ptr(), k2=k2.data_ptr(), handshake_hash=h.data_ptr(), stream=sp), "split")

    def like(hs, count):
        rc, out = A.dev_handshake_new_like(hs, count, stream=sp)
        ok(rc, "new_like")
        return out

    def move(dst, src, count, dst_lanes=None, src_lanes=None):
        ok(A.dev_handshake_move(dst, src, count, dst_lanes=dst_lanes.data_ptr() if dst_lanes is not None else 0,
                                src_lanes=src_lanes.data_ptr() if src_lanes is not None else 0, stream=sp), "move")

    def timed(fn, before=None, after=None):
        """us per tick over one window of --reps ticks; before / after run outside the events"""
        total = 0.0
        for _ in range(args.reps):
            state = before() if before else None
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            t0.record(main_s)
            state = fn(state)
            t1.record(main_s)
            torch.cuda.synchronize(dev)
            total += t0.elapsed_time(t1) * 1000.0
            if after:
                after(state)
        return total / args.reps

    ini_s, ini_e, res_s, res_e = (filled(n * 32, k << 40) for k in range(4))
    payload, got = filled(n * PAYLOAD, 6 << 40), zeros(n * PAYLOAD)
    msg = [zeros(n * m) for m in X]
    out = zeros(n * X[1])
    k = [zeros(n * 32) for _ in range(4)]
    hh = [zeros(n * 32) for _ in range(2)]

    # the clients' messages, and the pool: every responder after message 2
    ini, first = new(True, n), new(False, n)
    write(ini, msg[0], X[0])
    read(first, msg[0], X[0])
    write(first, msg[1], X[1])
    read(ini, msg[1], X[1])
    write(ini, msg[2], X[2])
    A.dev_handshake_free(ini)
    pool = like(first, n)
    move(pool, first, n)
    torch.cuda.synchronize(dev)
    A.dev_handshake_free(first)

    for m in [int(x) for x in args.m.split(",")]:
        assert m <= n
        # m pool lanes spread over the pool (the first m sessions' messages are read at stride X[2],
        # so the lanes are those of sessions 0 .. m-1 under a stride that scatters them)
        step = n // m
        lanes = (torch.arange(m, dtype=torch.int64, device=dev) * step).to(torch.int32)
        # message 3 of the sessions in those lanes, packed
        third = msg[2].view(n, X[2])[lanes.long()].contiguous().view(-1)
        pay_m = payload.view(n, PAYLOAD)[lanes.long()].contiguous()

        def lockstep():
            """an object of the same m sessions made by _new, at the position of the pool"""
            s, e = res_s.view(n, 32)[lanes.long()].contiguous(), res_e.view(n, 32)[lanes.long()].contiguous()
            rc, hs = A.dev_handshake_new(XX, A.ROLE_RESPONDER, m, stream=sp, local_static=s.data_ptr(),
                                         local_ephemeral=e.data_ptr())
            ok(rc, "new")
            first_m = msg[0].view(n, X[0])[lanes.long()].contiguous()
            ok(A.dev_handshake_read_message(hs, msg=first_m.data_ptr(), msg_stride=X[0], msg_len=X[0], payload=got.data_ptr(),
                                            payload_stride=PAYLOAD, stream=sp), "read")
            write(hs, out, X[1], pay_m)  # the payloads those sessions answered with: the same h, so message 3 verifies
            torch.cuda.synchronize(dev)
            return hs, (s, e, first_m)

        def arm2(state):
            hs = state[0]
            read(hs, third, X[2])
            split(hs, k[2], k[3], hh[1])
            return state

        def arm1(_):
            cohort = like(pool, m)
            move(cohort, pool, m, src_lanes=lanes)
            read(cohort, third, X[2])
            split(cohort, k[0], k[1], hh[0])
            return cohort

        def put_back(cohort):
            """outside the window: a cohort cannot go back once split, so the pool's lanes are refilled
            from a fresh object of the same sessions"""
            A.dev_handshake_free(cohort)
            hs, keep = lockstep()
            move(pool, hs, m, dst_lanes=lanes)
            torch.cuda.synchronize(dev)
            A.dev_handshake_free(hs)

        def free_lockstep(state):
            A.dev_handshake_free(state[0])

        def move_only(_):
            cohort = like(pool, m)
            torch.cuda.synchronize(dev)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(main_s)
            move(cohort, pool, m, src_lanes=lanes)
            t1.record(main_s)
            torch.cuda.synchronize(dev)
            us = t0.elapsed_time(t1) * 1000.0
            move(pool, cohort, m, dst_lanes=lanes)  # at the same position: back they go
            torch.cuda.synchronize(dev)
            A.dev_handshake_free(cohort)
            return us

        # once, untimed: the moved cohort and the lockstep object give the same keys
        put_back(arm1(None))
        st = arm2(lockstep())
        torch.cuda.synchronize(dev)
        same = torch.equal(k[0][:m * 32], k[2][:m * 32]) and torch.equal(k[1][:m * 32], k[3][:m * 32]) \
            and torch.equal(hh[0][:m * 32], hh[1][:m * 32]) and bool(k[0][:m * 32].view(m, 32).any(dim=1).all())
        bad += not same
        free_lockstep(st)

        for _ in range(args.warmup):
            timed(arm1, after=put_back)
            timed(arm2, before=lockstep, after=free_lockstep)
        t1s, t2s, tm = [], [], []
        for _ in range(args.rounds):  # the arms alternate inside a round
            t1s.append(timed(arm1, after=put_back))
            t2s.append(timed(arm2, before=lockstep, after=free_lockstep))
            tm.append(statistics.mean(move_only(None) for _ in range(args.reps)))
        med1, med2 = statistics.median(t1s), statistics.median(t2s)
        row = dict(name=XX, pool=n, m=m, payload=PAYLOAD, reps=args.reps, rounds=args.rounds, warmup=args.warmup,
                   device=torch.cuda.get_device_name(dev),
                   cohort_tick_us_median=round(med1, 1), cohort_tick_us_min=round(min(t1s), 1), cohort_tick_us_max=round(max(t1s), 1),
                   lockstep_us_median=round(med2, 1), lockstep_us_min=round(min(t2s), 1), lockstep_us_max=round(max(t2s), 1),
                   move_us_median=round(statistics.median(tm), 1), move_us_min=round(min(tm), 1), move_us_max=round(max(tm), 1),
                   cohort_over_lockstep=round(med1 / med2, 4), verified=bool(same))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    A.dev_handshake_free(pool)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
