#!/usr/bin/env python3
"""A/B of noise_aead_dev_duplex_ragged against the separate ragged launches.

The data is bench.py's C5 step with two ciphertext sets (--c5-sets 2): 128 Ki
records of 64 B-16 KiB over 512 states, ChaChaPoly for the even states and
AES-GCM for the odd ones (64 Ki records per cipher); step k seals the
plaintext into set k % 2 and opens set (k + 1) % 2, sealed by step k - 1, so
a step's seal and open are independent jobs.  Per cipher, three arms:

  separate_1s  noise_aead_dev_seal_ragged, then _open_ragged, one stream
  separate_2s  the same two launches on two streams (fork / join by events),
               as bench.py's C5 step issues them
  duplex       noise_aead_dev_duplex_ragged (NOISE_AEAD_RAGGED_DUPLEX=1, so
               the shared kernel runs whatever the default is; the plan the
               library printed is recorded)

then both ciphers together as C5 runs them: the four separate launches on
four streams against one duplex call per cipher on two streams.

Each arm is timed with device events over `--steps` steps, the arms
alternating inside each of `--rounds` interleaved rounds, after a warm-up of
every arm.  One JSON line per (group, arm, round) and one summary line per
(group, arm) — median, minimum, maximum in microseconds per step and the
spread (max - min) / median between the rounds of that arm — go to stdout and
to --out.  The decision rule: a family's shared launch is the
default only if its duplex arm is faster than the better separate arm by more
than the spread seen between repeats of one arm.

    python tools/duplex_ragged_ab.py --out profiles/duplex_ragged_ab.jsonl
"""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("NOISE_AEAD_RAGGED_DUPLEX", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "noise-c_amd")]

import numpy as np  # noqa: E402

import bench  # noqa: E402  (the C5 generators: mixed_layout, the seeds, the record layout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=131072, help="records per step, both ciphers together")
    ap.add_argument("--states", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--one-pass", action="store_true", help="ChaChaPoly opens with NOISE_AEAD_FLAG_ONE_PASS")
    ap.add_argument("--only", default=None, choices=("chacha", "aes", "both"))
    ap.add_argument("--arms", default=None, help="comma-separated arm names to run (default: all), "
                    "e.g. duplex,duplex_2s for a profiler run of the shared launches alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.steps >= 1 and args.rounds >= 1

    import torch
    import noise_aead as A
    A.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_s = torch.cuda.current_stream(dev)
    sp = main_s.cuda_stream
    R, S = args.records, args.states
    lay = bench.mixed_layout(R, S, 0)
    rec_dt = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("nonce", "<u8"), ("ctx_off", "<u8"),
                       ("ad_off", "<u8"), ("len", "<u4"), ("ad_len", "<u4")])
    pt = torch.empty(lay["total"], dtype=torch.uint8, device=dev)
    assert A.dev_fill_splitmix(pt.data_ptr(), pt.numel(), bench.SEED_PT, 0, sp) == 0
    cts = [torch.empty_like(pt), torch.empty_like(pt)]
    back = torch.empty_like(pt)
    groups = {}
    for name, cipher, parity in (("chacha", bench.CHACHA, 0), ("aes", bench.AES, 1)):
        states = [s for s in range(S) if s % 2 == parity]
        cb = A.dev_ctx_bytes(cipher)
        raw = torch.empty(len(states) * 32, dtype=torch.uint8, device=dev)
        for i, s in enumerate(states):
            assert A.dev_fill_splitmix(raw[32 * i:].data_ptr(), 32, bench.SEED_KEY, 4 * s, sp) == 0
        ctx = torch.empty(len(states) * cb, dtype=torch.uint8, device=dev)
        assert A.dev_prepare(cipher, raw.data_ptr(), len(states), ctx.data_ptr(), sp) == 0
        slot_of = {s: i for i, s in enumerate(states)}
        idx = np.nonzero((lay["st_global"] % 2) == parity)[0]
        recs = np.zeros(len(idx), dtype=rec_dt)
        recs["in_off"] = recs["out_off"] = lay["off"][idx]
        recs["nonce"] = lay["nonce"][idx]
        recs["ctx_off"] = np.array([slot_of[s] for s in lay["st_local"][idx]], dtype=np.uint64) * cb
        recs["len"] = lay["lens"][idx]
        d_recs = torch.from_numpy(recs.view(np.uint8)).to(dev)
        st = torch.empty(len(idx), dtype=torch.uint8, device=dev)
        oflags = A.FLAG_ONE_PASS if args.one_pass and cipher == bench.CHACHA else 0
        g = dict(name=name, cipher=cipher, ctx=ctx, raw=raw, recs=d_recs, n=len(idx), st=st,
                 bytes=int(lay["lens"][idx].sum()), oflags=oflags)

        def job(open_, inp, out, g=g):
            return A.ragged_job(ctx_base=g["ctx"].data_ptr(), recs=g["recs"].data_ptr(), inp=inp.data_ptr(),
                                out=out.data_ptr(), n_records=g["n"], status=g["st"].data_ptr() if open_ else 0,
                                flags=A.FLAG_FAST | (g["oflags"] if open_ else 0))
        # the two sets' jobs, built once: [k % 2] seals into cts[k % 2] and opens cts[(k + 1) % 2]
        g["seal"] = [job(False, pt, cts[k]) for k in range(2)]
        g["open"] = [job(True, cts[1 - k], back) for k in range(2)]
        groups[name] = g
    lib = A.lib()
    import ctypes as C

    def seal(g, k, stream):
        return lib.noise_aead_dev_seal_ragged(g["cipher"], C.byref(g["seal"][k]), stream)

    def open_(g, k, stream):
        return lib.noise_aead_dev_open_ragged(g["cipher"], C.byref(g["open"][k]), stream)

    def duplex(g, k, stream):
        return lib.noise_aead_dev_duplex_ragged(g["cipher"], C.byref(g["seal"][k]), C.byref(g["open"][k]), stream)

    for g in groups.values():  # set 1 sealed before step 0 opens it
        assert seal(g, 1, sp) == 0
    torch.cuda.synchronize(dev)
    side = [torch.cuda.Stream(dev) for _ in range(3)]

    def fork_join(calls):
        """calls: [(fn, group)] — the first on the main stream, the others on side streams"""
        def step(k):
            ev = torch.cuda.Event()
            ev.record(main_s)
            rc = 0
            for i, (fn, g) in enumerate(calls):
                s = main_s if i == 0 else side[i - 1]
                if i:
                    s.wait_event(ev)
                rc = rc or fn(g, k, s.cuda_stream)
            for i in range(1, len(calls)):
                done = torch.cuda.Event()
                done.record(side[i - 1])
                main_s.wait_event(done)
            return rc
        return step

    def in_order(calls):
        def step(k):
            rc = 0
            for fn, g in calls:
                rc = rc or fn(g, k, sp)
            return rc
        return step

    ch, ae = groups["chacha"], groups["aes"]
    plans = {}
    arms = {}
    for g in (ch, ae):
        arms[g["name"]] = {"separate_1s": in_order([(seal, g), (open_, g)]),
                           "separate_2s": fork_join([(seal, g), (open_, g)]),
                           "duplex": in_order([(duplex, g)])}
    arms["both"] = {"separate_4s": fork_join([(seal, ch), (seal, ae), (open_, ae), (open_, ch)]),
                    "duplex_2s": fork_join([(duplex, ch), (duplex, ae)])}
    if args.only:
        arms = {args.only: arms[args.only]}
    if args.arms:
        arms = {grp: {a: f for a, f in by.items() if a in args.arms.split(",")} for grp, by in arms.items()}
    kstep = [0]

    def run(step, n):
        for _ in range(n):
            if step(kstep[0] % 2):
                raise RuntimeError("launch failed")
            kstep[0] += 1

    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for group, by_arm in arms.items():
        nbytes = sum(g["bytes"] for g in groups.values() if group in (g["name"], "both")) * 2  # sealed + opened
        for arm, step in by_arm.items():  # warm-up of every arm (and the plan each prints)
            kstep[0] = 0
            run(step, args.warmup + (args.warmup % 2))  # an even count: every arm starts on set 0
            torch.cuda.synchronize(dev)
            plans[(group, arm)] = A.last_plan()
        times = {arm: [] for arm in by_arm}
        for rnd in range(args.rounds):
            for arm, step in by_arm.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(main_s)
                run(step, args.steps + (args.steps % 2))
                t1.record(main_s)
                torch.cuda.synchronize(dev)
                us = t0.elapsed_time(t1) * 1000.0 / (args.steps + (args.steps % 2))
                times[arm].append(us)
                emit(dict(group=group, arm=arm, round=rnd, us_per_step=round(us, 2)))
        for arm, t in times.items():
            med = statistics.median(t)
            emit(dict(group=group, arm=arm, summary=True, rounds=len(t), steps=args.steps,
                      us_median=round(med, 2), us_min=round(min(t), 2), us_max=round(max(t), 2),
                      spread=round((max(t) - min(t)) / med, 4), gib_s=round(nbytes / med * 1e6 / 2**30, 1),
                      records=sum(g["n"] for g in groups.values() if group in (g["name"], "both")),
                      one_pass=bool(args.one_pass), last_plan=plans[(group, arm)]))
    st_bad = sum(int((g["st"] != 0).sum()) for g in groups.values())
    emit(dict(verified=st_bad == 0, rejected=st_bad,
              what="statuses of the last opens (every record was sealed by a step before)"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if st_bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
