#!/usr/bin/env python3
"""What a rekey of a session table's slots costs (include/noise_aead_hip.h
section 12), beside the call a caller had before it.

Per cipher one table as large as the largest m (ChaChaPoly 65 536 slots,
AESGCM 16 384), and for each m:
    rekey      noise_aead_dev_transport_rekey of m scrambled slots, both
               directions, no per-entry bytes;
    set_keys   noise_aead_dev_transport_set_keys of the same m slots from packed
               keys: what "rekeying by a fresh key" cost, given that somebody
               had derived the key, and the baseline that exists without rekey.
    m = 1, 1024, 65 536 (ChaChaPoly); 1, 1024, 16 384 (AESGCM).

One call is timed with a pair of device events.  The arms alternate call by
call inside a round, `--rounds` rounds after `--warmup`; set_keys runs first in
a round, so every rekey works on freshly keyed slots.  A line gives per arm the
median, minimum and maximum microseconds.  Before the timing, the contexts of a
sample of slots after set_keys + rekey must equal noise_aead_dev_prepare of
noise_aead_dev_rekey of the keys, and the nonces must be as they were.  A
library without the rekey entry points (NOISE_AEAD_LIB pointing at an older
build) is timed for set_keys alone.  DESIGN.md 4.16 records the figures.

    python tools/transport_rekey_bench.py --out profiles/transport_rekey.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "noise-c_amd")]

SIZES = {"ChaChaPoly": (1, 1024, 65536), "AESGCM": (1, 1024, 16384)}


def stat(v):
    med = statistics.median(v)
    return dict(us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ciphers", default="ChaChaPoly,AESGCM")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import noise_aead as A
    has_rekey = hasattr(A.lib(), "noise_aead_dev_transport_rekey")
    assert torch.cuda.is_available(), "transport_rekey_bench needs the GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_s = torch.cuda.current_stream(dev)
    sp = main_s.cuda_stream
    hip = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    lines, bad = [], 0
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(arms):
        """{arm: [µs]}: the arms alternate inside a round"""
        times = {k: [] for k in arms}
        for rnd in range(args.warmup + args.rounds):
            for name, fn in arms.items():
                t0.record(main_s)
                rc = fn()
                t1.record(main_s)
                torch.cuda.synchronize(dev)
                if rc:
                    raise RuntimeError(f"{name}: {rc:#x}")
                if rnd >= args.warmup:
                    times[name].append(t0.elapsed_time(t1) * 1000.0)
        return times

    device_name = torch.cuda.get_device_name(dev)
    for cname in args.ciphers.split(","):
        cipher = {"ChaChaPoly": A.CHACHAPOLY, "AESGCM": A.AESGCM}[cname]
        cb = A.dev_ctx_bytes(cipher)
        n = max(SIZES[cname])
        k1 = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        k2 = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        assert A.dev_fill_splitmix(k1.data_ptr(), n * 32, 0x4B31, 0, sp) == 0
        assert A.dev_fill_splitmix(k2.data_ptr(), n * 32, 0x4B32, 0, sp) == 0
        rc, tab = A.dev_transport_new_unkeyed(cipher, A.ROLE_INITIATOR, n, max_frames=64, stream=sp)
        assert rc == 0, hex(rc)
        for m in SIZES[cname]:
            # m distinct slots of the table, unsorted (an odd multiplier permutes 0 .. 2^k - 1)
            slots = ((np.arange(m, dtype=np.int64) * 40503 + 7) % n).astype(np.int64)
            d_slots = torch.from_numpy(slots.astype(np.uint32).view(np.int32)).to(dev)

            def set_keys():
                return A.dev_transport_set_keys(tab, slots=d_slots.data_ptr(), m=m, k1=k1.data_ptr(), k2=k2.data_ptr(),
                                                stream=sp)

            def rekey():
                return A.dev_transport_rekey(tab, slots=d_slots.data_ptr(), m=m, directions=3, stream=sp)

            ok = True
            if has_rekey:
                # ---- the successor's contexts: a sample of entries, both directions (the initiator sends under k1)
                sample = sorted(set(range(0, m, max(m // 16, 1))) | {m - 1})
                nonces = torch.arange(1, 2 * n + 1, dtype=torch.int64, device=dev)
                assert set_keys() == 0
                for d in (0, 1):
                    assert hip.hipMemcpyAsync(A.dev_transport_nonces(tab, d), nonces.data_ptr() + 8 * n * d, 8 * n, 3, sp) == 0
                assert rekey() == 0
                got = torch.empty(cb, dtype=torch.uint8, device=dev)
                want = torch.zeros(cb, dtype=torch.uint8, device=dev)  # prepare leaves the context's padding as it finds it
                nk = torch.empty(32, dtype=torch.uint8, device=dev)
                back = torch.empty(n, dtype=torch.int64, device=dev)
                for d, keys in ((0, k1), (1, k2)):
                    base, size = A.debug_transport_ctx(tab, d)
                    assert size == cb
                    for j in sample:
                        assert A.dev_rekey(cipher, keys=keys.data_ptr() + 32 * j, n=1, out=nk.data_ptr(), stream=sp) == 0
                        assert A.dev_prepare(cipher, nk.data_ptr(), 1, want.data_ptr(), sp) == 0
                        assert hip.hipMemcpyAsync(got.data_ptr(), base + int(slots[j]) * cb, cb, 3, sp) == 0
                        torch.cuda.synchronize(dev)
                        if not torch.equal(got, want):
                            ok = False
                            print(f"{cname} m={m}: context of entry {j} (slot {int(slots[j])}), direction {d}: "
                                  f"{int((got != want).sum())} bytes differ", file=sys.stderr)
                    assert hip.hipMemcpyAsync(back.data_ptr(), A.dev_transport_nonces(tab, d), 8 * n, 3, sp) == 0
                    torch.cuda.synchronize(dev)
                    if not torch.equal(back, nonces[n * d:n * d + n]):
                        ok = False
                        print(f"{cname} m={m}: {int((back != nonces[n * d:n * d + n]).sum())} nonces of direction {d} moved",
                              file=sys.stderr)
                bad += not ok
            arms = {"set_keys": set_keys}
            if has_rekey:
                arms["rekey"] = rekey
            times = timed(arms)
            med = {k: statistics.median(v) for k, v in times.items()}
            extra = dict(ratio=round(med["rekey"] / med["set_keys"], 4), verified=bool(ok)) if has_rekey else {}
            lines.append(json.dumps(dict(
                part="rekey", cipher=cname, slots=n, entries=m, directions=3, ctx_bytes=cb, rounds=args.rounds,
                warmup=args.warmup, device=device_name, **{k: stat(v) for k, v in times.items()}, **extra)))
            print(lines[-1], flush=True)
        A.dev_transport_free(tab)
        del k1, k2
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
