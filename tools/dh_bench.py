#!/usr/bin/env python3
"""Rate of the batched X25519 (noise_aead_dev_dh_calculate) on the device.

For n = 4096 (the session count of bench.py's C4/C5), 65 536 and 1 Mi
sessions: n random private keys against n random public values, packed
(stride 32), one launch per step.  Each n is warmed up, then timed with device
events over enough steps for a window of at least `--min-keys` shared keys, in
`--rounds` rounds; the line of an n gives the median, minimum and maximum
microseconds per launch, the spread between the rounds and the shared keys per
second at the median, and the same for noise_aead_dev_dh_public.  The first,
a middle and the last session of every n are checked against the big-integer
ladder of tests/x25519_ref.py.

The figure to set the rate against is the reference's own single-threaded
`Curve25519 calculate` line (perf_dh_calculate, tests/performance/
test-performance.c:211-240) on the host CPU; DESIGN.md 4.10 records both.

    python tools/dh_bench.py --out profiles/dh_x25519.jsonl
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "noise-c_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,65536,1048576", help="comma-separated session counts")
    ap.add_argument("--min-keys", type=int, default=4 << 20, help="shared keys per timed window, at least")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import noise_aead as A
    import x25519_ref as X
    A.lib()
    assert torch.cuda.is_available(), "dh_bench needs the GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_s = torch.cuda.current_stream(dev)
    sp = main_s.cuda_stream
    lines = []
    bad = 0
    for n in [int(x) for x in args.n.split(",")]:
        priv = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        pub = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        out = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        assert A.dev_fill_splitmix(priv.data_ptr(), priv.numel(), 0x25519, 0, sp) == 0
        assert A.dev_fill_splitmix(pub.data_ptr(), pub.numel(), 0x25519, 1 << 40, sp) == 0
        ops = {"calculate": lambda: A.dev_dh_calculate(A.DH_CURVE25519, priv=priv.data_ptr(), pub=pub.data_ptr(),
                                                       n=n, shared=out.data_ptr(), stream=sp),
               "public": lambda: A.dev_dh_public(A.DH_CURVE25519, priv=priv.data_ptr(), n=n,
                                                 pub_out=out.data_ptr(), stream=sp)}
        steps = max(5, -(-args.min_keys // n))
        row = dict(n=n, steps=steps, rounds=args.rounds, warmup=args.warmup, device=torch.cuda.get_device_name(dev))
        for _ in range(args.warmup):
            for op in ops.values():
                assert op() == 0
        torch.cuda.synchronize(dev)
        times = {name: [] for name in ops}
        for _ in range(args.rounds):  # the two entry points alternate inside a round
            for name, op in ops.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(main_s)
                for _ in range(steps):
                    if op():
                        raise RuntimeError("launch failed")
                t1.record(main_s)
                torch.cuda.synchronize(dev)
                times[name].append(t0.elapsed_time(t1) * 1000.0 / steps)
        for name, t in times.items():
            med = statistics.median(t)
            row[name] = dict(us_median=round(med, 2), us_min=round(min(t), 2), us_max=round(max(t), 2),
                             spread=round((max(t) - min(t)) / med, 4), keys_per_s=round(n / med * 1e6))
        # what the timed kernels computed: the calculate launch once more, three sessions against the ladder
        assert ops["calculate"]() == 0
        torch.cuda.synchronize(dev)
        ph, uh, oh = (t.cpu().numpy().reshape(n, 32) for t in (priv, pub, out))
        wrong = [i for i in sorted({0, n // 2, n - 1}) if bytes(oh[i]) != X.x25519(bytes(ph[i]), bytes(uh[i]))]
        bad += len(wrong)
        row["verified"] = not wrong
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        print(f"n = {n}: {row['calculate']['keys_per_s']} shared keys/s, "
              f"{row['public']['keys_per_s']} public keys/s", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
