#!/usr/bin/env python3
"""What the session table's calls (include/noise_aead_hip.h section 10) buy
over what a caller had before, on identical data.

Both parts run on one table of 65 536 slots per role, ChaChaPoly and AESGCM:
    tick       m active slots of the table have one frame of 1400 B plaintext
               each, the others nothing.  noise_aead_dev_transport_seal_frames_of
               / _open_frames_of over the m slots (scrambled order, this call's
               cap m) against the existing full call on the same object with
               d_len = 0 for the idle slots, which walks all n sessions and
               launches the AEAD over the object's max_frames = n records.
               m = 1024 and m = n.
    set_keys   noise_aead_dev_transport_set_keys of m = 4096 and m = 65 536
               scrambled slots against two packed noise_aead_dev_prepare calls
               of m keys each (what _new does for a whole batch).

One call is timed with a pair of device events; between calls, untimed, the
wire is put back and the nonces go back to 0.  The arms of a part alternate
call by call inside a round, `--rounds` rounds after `--warmup`.  A line gives
per arm the median, minimum and maximum microseconds.  Before the timing the
_of seal must equal the full call's seal byte for byte, the _of open must give
every frame back, and the contexts _set_keys built must equal prepare's.
DESIGN.md 4.13 records the figures.

    python tools/transport_table_bench.py --out profiles/transport_table.jsonl
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


def stat(v):
    med = statistics.median(v)
    return dict(us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ciphers", default="ChaChaPoly,AESGCM")
    ap.add_argument("--parts", default="tick,set_keys")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import noise_aead as A
    A.lib()
    assert torch.cuda.is_available(), "transport_table_bench needs the GPU: there is no CPU path"
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

    def scrambled(m):
        """m distinct slots of the table, unsorted (an odd multiplier permutes 0 .. 2^16 - 1)"""
        return ((np.arange(m, dtype=np.int64) * 40503 + 7) % N).astype(np.int64)

    k1 = torch.empty(N * 32, dtype=torch.uint8, device=dev)
    k2 = torch.empty(N * 32, dtype=torch.uint8, device=dev)
    assert A.dev_fill_splitmix(k1.data_ptr(), N * 32, 0x4B31, 0, sp) == 0
    assert A.dev_fill_splitmix(k2.data_ptr(), N * 32, 0x4B32, 0, sp) == 0
    device_name = torch.cuda.get_device_name(dev)

    for cname in args.ciphers.split(","):
        cipher = {"ChaChaPoly": A.CHACHAPOLY, "AESGCM": A.AESGCM}[cname]
        cb = A.dev_ctx_bytes(cipher)

        if "tick" in args.parts.split(","):
            rc, ini = A.dev_transport_new(cipher, A.ROLE_INITIATOR, N, k1=k1.data_ptr(), k2=k2.data_ptr(), max_frames=N, stream=sp)
            assert rc == 0, hex(rc)
            rc, res = A.dev_transport_new(cipher, A.ROLE_RESPONDER, N, k1=k1.data_ptr(), k2=k2.data_ptr(), max_frames=N, stream=sp)
            assert rc == 0, hex(rc)

            def reset(_name=None):
                for tr, d in ((ini, 0), (res, 1)):
                    assert hip.hipMemsetAsync(A.dev_transport_nonces(tr, d), 0, 8 * N, sp) == 0

            for m in (1024, N):
                slots = scrambled(m)
                stride = 2 + PLAIN + 16
                nbytes = m * stride
                plain = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
                assert A.dev_fill_splitmix(plain.data_ptr(), nbytes + 64, 0x5452, 0, sp) == 0
                hdr = torch.arange(m, device=dev, dtype=torch.int64) * stride
                plain[hdr] = (PLAIN + 16) >> 8
                plain[hdr + 1] = (PLAIN + 16) & 0xFF
                wire, sealed = plain.clone(), torch.empty_like(plain)
                off = np.arange(m, dtype=np.int64) * stride
                off_full, len_full = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int32)
                off_full[slots], len_full[slots] = off, stride
                d_slots = torch.from_numpy(slots.astype(np.uint32).view(np.int32)).to(dev)
                d_off, d_len = torch.from_numpy(off).to(dev), torch.full((m,), stride, dtype=torch.int32, device=dev)
                d_off_full, d_len_full = torch.from_numpy(off_full).to(dev), torch.from_numpy(len_full).to(dev)
                r_of = torch.zeros((m, 4), dtype=torch.int32, device=dev)
                r_full = torch.zeros((N, 4), dtype=torch.int32, device=dev)
                of = dict(slots=d_slots.data_ptr(), m=m, max_frames=m, wire=wire.data_ptr(), off=d_off.data_ptr(),
                          length=d_len.data_ptr(), result=r_of.data_ptr(), stream=sp)
                full = dict(wire=wire.data_ptr(), off=d_off_full.data_ptr(), length=d_len_full.data_ptr(),
                            result=r_full.data_ptr(), stream=sp)
                # ---- the two forms compute the same bytes, and the open gives the frames back
                reset()
                assert A.dev_transport_seal_frames(ini, **full) == 0
                sealed.copy_(wire)
                wire.copy_(plain)
                reset()
                assert A.dev_transport_seal_frames_of(ini, **of) == 0
                torch.cuda.synchronize(dev)
                r = r_of.cpu().numpy()
                ok = torch.equal(wire, sealed) and int(r[:, 0].sum()) == m and not r[:, 2].any()
                assert A.dev_transport_open_frames_of(res, **of) == 0
                torch.cuda.synchronize(dev)
                r = r_of.cpu().numpy()
                body = (torch.arange(nbytes + 64, device=dev) % stride) < 2 + PLAIN  # the tags stay as sealed
                body[nbytes:] = True
                ok = ok and torch.equal(wire[body], plain[body]) and int(r[:, 0].sum()) == m and not r[:, 2].any()
                del body
                bad += not ok
                arms = {"of_seal": lambda: A.dev_transport_seal_frames_of(ini, **of),
                        "full_seal": lambda: A.dev_transport_seal_frames(ini, **full),
                        "of_open": lambda: A.dev_transport_open_frames_of(res, **of),
                        "full_open": lambda: A.dev_transport_open_frames(res, **full)}

                def before(name):
                    wire.copy_(plain if name.endswith("seal") else sealed)
                    reset()
                times = timed(arms, before)
                bad += int(r_full.cpu().numpy()[:, 0].sum()) != m or int(r_of.cpu().numpy()[:, 0].sum()) != m
                med = {k: statistics.median(v) for k, v in times.items()}
                lines.append(json.dumps(dict(
                    part="tick", cipher=cname, slots=N, active=m, object_max_frames=N, call_max_frames=m,
                    frame_plaintext=PLAIN, rounds=args.rounds, warmup=args.warmup, device=device_name,
                    **{k: stat(v) for k, v in times.items()},
                    seal_ratio=round(med["of_seal"] / med["full_seal"], 4), open_ratio=round(med["of_open"] / med["full_open"], 4),
                    verified=bool(ok))))
                print(lines[-1], flush=True)
                del plain, wire, sealed
            A.dev_transport_free(ini)
            A.dev_transport_free(res)
            torch.cuda.empty_cache()

        if "set_keys" in args.parts.split(","):
            rc, tab = A.dev_transport_new_unkeyed(cipher, A.ROLE_INITIATOR, N, max_frames=64, stream=sp)
            assert rc == 0, hex(rc)
            for m in (4096, N):
                slots = scrambled(m)
                d_slots = torch.from_numpy(slots.astype(np.uint32).view(np.int32)).to(dev)
                ctx = torch.zeros(2 * m * cb, dtype=torch.uint8, device=dev)

                def prepare_x2():
                    rc = A.dev_prepare(cipher, k1.data_ptr(), m, ctx.data_ptr(), sp)
                    return rc or A.dev_prepare(cipher, k2.data_ptr(), m, ctx.data_ptr() + m * cb, sp)

                def set_keys():
                    return A.dev_transport_set_keys(tab, slots=d_slots.data_ptr(), m=m, k1=k1.data_ptr(), k2=k2.data_ptr(),
                                                    stream=sp)
                # ---- the same contexts: a sample of entries, both directions
                assert prepare_x2() == 0 and set_keys() == 0
                got = torch.empty(cb, dtype=torch.uint8, device=dev)
                ok = True
                for j in range(0, m, max(m // 64, 1)):
                    for d in (0, 1):
                        base, size = A.debug_transport_ctx(tab, d)
                        assert size == cb and hip.hipMemcpyAsync(got.data_ptr(), base + int(slots[j]) * cb, cb, 3, sp) == 0
                        torch.cuda.synchronize(dev)
                        ok = ok and torch.equal(got, ctx[(d * m + j) * cb:(d * m + j + 1) * cb])
                bad += not ok
                times = timed({"set_keys": set_keys, "prepare_x2": prepare_x2}, lambda name: None)
                med = {k: statistics.median(v) for k, v in times.items()}
                lines.append(json.dumps(dict(
                    part="set_keys", cipher=cname, slots=N, keyed=m, ctx_bytes=cb, rounds=args.rounds, warmup=args.warmup,
                    device=device_name, **{k: stat(v) for k, v in times.items()},
                    ratio=round(med["set_keys"] / med["prepare_x2"], 4), verified=bool(ok))))
                print(lines[-1], flush=True)
                del ctx
                torch.cuda.empty_cache()
            A.dev_transport_free(tab)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
