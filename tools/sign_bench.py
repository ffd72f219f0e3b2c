#!/usr/bin/env python3
"""What batched Ed25519 costs (noise_aead_dev_sign_verify / _sign_public /
_sign, header section 17).

n signatures by n signers over messages of 32 bytes (a static key: the
certificate flow) and, for verify, of 300 bytes, at n = 64, 1024, 4096 and
65 536.  Everything is made on the device: seeds from the library's SplitMix
fill, the public keys by _sign_public, the signatures by _sign.  Each call is
timed with device events over `--reps` calls per window; the arms alternate
inside a round.  Next to verify it prints

  (a) noise_aead_dev_dh_calculate at the same n: the project's own yardstick
      for this field arithmetic (one 255-step Montgomery ladder);
  (b) the reference's noise_signstate_verify from
      oracle/_ref/libnoiseref_full.so on 16 CPU threads, where that library is
      present (the column is left out otherwise).

Before any timing every signature is verified on the device (all accepted)
and one flipped bit per signature is refused.  DESIGN.md 4.21 records the
figures.

    python tools/sign_bench.py --out profiles/sign.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "noise-c_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
REF = os.path.join(ROOT, "oracle", "_ref", "libnoiseref_full.so")
CPU_THREADS = 16


def reference_verifies_per_s(pubs, sigs, msgs, count):
    """noise_signstate_verify of `count` entries on CPU_THREADS threads (the
    calls release the interpreter lock); None without the reference build"""
    if not os.path.exists(REF):
        return None
    L = C.CDLL(REF)
    vp = C.c_void_p
    L.noise_signstate_new_by_id.argtypes = [C.POINTER(vp), C.c_int]
    L.noise_signstate_set_public_key.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.noise_signstate_verify.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.noise_signstate_free.argtypes = [vp]
    count = min(count, len(pubs))
    states = []
    for i in range(count):
        st = vp()
        assert L.noise_signstate_new_by_id(C.byref(st), 0x5301) == 0
        assert L.noise_signstate_set_public_key(st, pubs[i], 32) == 0
        states.append(st)
    bad = [0] * CPU_THREADS

    def work(t):
        for i in range(t, count, CPU_THREADS):
            bad[t] += L.noise_signstate_verify(states[i], msgs[i], len(msgs[i]), sigs[i], 64) != 0

    threads = [threading.Thread(target=work, args=(t,)) for t in range(CPU_THREADS)]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    dt = time.perf_counter() - t0
    for st in states:
        L.noise_signstate_free(st)
    assert sum(bad) == 0, "the reference refused a signature the device made"
    return count / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="64,1024,4096,65536")
    ap.add_argument("--lens", default="32,300", help="message lengths; sign and public use the first")
    ap.add_argument("--reps", type=int, default=4, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-count", type=int, default=4096, help="entries of the reference's CPU column")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import noise_aead as A
    A.lib()
    assert torch.cuda.is_available(), "sign_bench needs the GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_s = torch.cuda.current_stream(dev)
    sp = main_s.cuda_stream
    ID = A.SIGN_ED25519
    lines, bad = [], 0

    def filled(nbytes, word0):
        t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert A.dev_fill_splitmix(t.data_ptr(), nbytes, 0x5347, word0, sp) == 0
        return t

    def ok(rc, what):
        if rc:
            raise RuntimeError(f"{what}: {rc:#x}")

    def timed(fn):
        """us per call over one window of --reps calls"""
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0.record(main_s)
        for _ in range(args.reps):
            fn()
        t1.record(main_s)
        torch.cuda.synchronize(dev)
        return t0.elapsed_time(t1) * 1000.0 / args.reps

    lens = [int(x) for x in args.lens.split(",")]
    for n in [int(x) for x in args.n.split(",")]:
        seeds, peer = filled(n * 32, 1 << 40), filled(n * 32, 2 << 40)
        pubs = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        shared = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        ok(A.dev_sign_public(ID, priv=seeds.data_ptr(), n=n, pub_out=pubs.data_ptr(), stream=sp), "public")
        row = dict(n=n, reps=args.reps, rounds=args.rounds, warmup=args.warmup, device=torch.cuda.get_device_name(dev))
        arms = {}
        per_len = {}
        for ln in lens:
            msgs = filled(n * ln, (3 << 40) + ln)
            off = torch.arange(n, dtype=torch.int64, device=dev) * ln
            mlen = torch.full((n,), ln, dtype=torch.int32, device=dev)
            sigs = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
            kw = dict(msg=msgs.data_ptr(), msg_off=off.data_ptr(), msg_len=mlen.data_ptr(), n=n, stream=sp)
            ok(A.dev_sign(ID, priv=seeds.data_ptr(), pub=pubs.data_ptr(), sig_out=sigs.data_ptr(), **kw), "sign")
            per_len[ln] = (msgs, off, mlen, sigs, kw)

            def verify(kw=kw, sigs=sigs):
                ok(A.dev_sign_verify(ID, pub=pubs.data_ptr(), sig=sigs.data_ptr(), status=status.data_ptr(), **kw), "verify")

            # once, untimed: all accepted, and all refused with one bit of S flipped
            verify()
            torch.cuda.synchronize(dev)
            good = int(status.count_nonzero().item()) == 0
            forged = sigs.clone()
            forged.view(n, 64)[:, 40] ^= 1
            ok(A.dev_sign_verify(ID, pub=pubs.data_ptr(), sig=forged.data_ptr(), status=status.data_ptr(), **kw), "verify")
            torch.cuda.synchronize(dev)
            good = good and bool((status == 6).all().item())
            bad += not good
            row[f"verified_len{ln}"] = good
            arms[f"verify_len{ln}"] = verify
        ln0 = lens[0]
        kw0, sigs0 = per_len[ln0][4], per_len[ln0][3]
        arms[f"sign_len{ln0}"] = lambda: ok(A.dev_sign(ID, priv=seeds.data_ptr(), pub=pubs.data_ptr(),
                                                      sig_out=sigs0.data_ptr(), **kw0), "sign")
        arms["public"] = lambda: ok(A.dev_sign_public(ID, priv=seeds.data_ptr(), n=n, pub_out=pubs.data_ptr(),
                                                     stream=sp), "public")
        arms["dh_calculate"] = lambda: ok(A.dev_dh_calculate(A.DH_CURVE25519, priv=seeds.data_ptr(), pub=peer.data_ptr(),
                                                             n=n, shared=shared.data_ptr(), stream=sp), "dh")
        for _ in range(args.warmup):
            for fn in arms.values():
                timed(fn)
        times = {k: [] for k in arms}
        for _ in range(args.rounds):  # the arms alternate inside a round
            for k, fn in arms.items():
                times[k].append(timed(fn))
        for k, ts in times.items():
            med = statistics.median(ts)
            row[f"{k}_us_median"] = round(med, 1)
            row[f"{k}_us_min"] = round(min(ts), 1)
            row[f"{k}_us_max"] = round(max(ts), 1)
            row[f"{k}_per_s"] = round(n / med * 1e6)
        row[f"verify_len{ln0}_over_dh"] = round(row[f"verify_len{ln0}_us_median"] / row["dh_calculate_us_median"], 3)
        if n >= args.cpu_count:
            msgs, _, _, sigs, _ = per_len[ln0]
            c = args.cpu_count
            h_pub, h_sig, h_msg = pubs.cpu().numpy(), sigs.cpu().numpy(), msgs.cpu().numpy()
            rate = reference_verifies_per_s([h_pub[32 * i:32 * i + 32].tobytes() for i in range(c)],
                                            [h_sig[64 * i:64 * i + 64].tobytes() for i in range(c)],
                                            [h_msg[ln0 * i:ln0 * i + ln0].tobytes() for i in range(c)], c)
            if rate is not None:
                row[f"reference_cpu_{CPU_THREADS}_threads_verify_per_s"] = round(rate)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
