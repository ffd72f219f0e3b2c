#!/usr/bin/env python3
"""What a tick of the device-resident transport sessions costs
(noise_aead_dev_transport_seal_frames / _open_frames) beside the AEAD alone.

Three shapes, each for ChaChaPoly and AESGCM, the sessions' streams back to
back in one device buffer (frames at whatever alignment that gives):
    64ki_x1   65 536 sessions x 1 frame of 1400 B plaintext
    4ki_x16    4 096 sessions x 16 frames of 1400 B
    c5_mix       512 sessions x 256 frames, plaintext lengths 64 + SplitMix64 %
               16321 (bench.py's C5 mix: 128 Ki records, 256 per state)
The reference time is noise_aead_dev_{seal,open}_ragged on the same frames
through descriptors built on the host beforehand, with the same layout (not
FAST), automatic lanes and exactly the frames as records: those entry points
are what a caller had before, and the transport object calls them itself, so
the difference is the walk, scan, build and commit launches (and the refused
descriptors, none here: max_frames is the frame count).

One tick is timed with a pair of device events around the one call; between
ticks, untimed, the wire is put back (the open needs ciphertext again, both
arms alike) and the object's receive nonces go back to 0.  The arms alternate
tick by tick inside a round — transport seal, ragged seal, transport open,
ragged open — for `--rounds` rounds after `--warmup`.  A line gives, per arm,
the median, minimum and maximum microseconds and the spread, and the ratio of
the medians.  Before the timing the transport seal must equal the ragged seal
byte for byte and the transport open must give every frame back with no
error.  DESIGN.md 4.12 records the figures.

    python tools/transport_bench.py --out profiles/transport.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "noise-c_amd")]

SHAPES = {"64ki_x1": (65536, 1, None), "4ki_x16": (4096, 16, None), "c5_mix": (512, 256, "c5")}


def frame_lengths(np, sessions, per, mix):
    """L of every frame (plaintext + 16), session by session"""
    if mix is None:
        return np.full(sessions * per, 1400 + 16, dtype=np.int64)
    from bench import SEED_LEN, splitmix64_np
    gi = np.arange(sessions * per, dtype=np.uint64)
    return (np.uint64(64) + splitmix64_np(np.uint64(SEED_LEN) + gi) % np.uint64(16321)).astype(np.int64) + 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ciphers", default="ChaChaPoly,AESGCM")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import noise_aead as A
    A.lib()
    assert torch.cuda.is_available(), "transport_bench needs the GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_s = torch.cuda.current_stream(dev)
    sp = main_s.cuda_stream
    hip = ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    lines, bad = [], 0

    for shape in args.shapes.split(","):
        sessions, per, mix = SHAPES[shape]
        L = frame_lengths(np, sessions, per, mix)
        total = len(L)
        hdr = np.zeros(total, dtype=np.int64)
        hdr[1:] = np.cumsum(L + 2)[:-1]
        nbytes = int(hdr[-1] + L[-1] + 2)
        s_off = hdr[::per].copy()
        s_len = np.add.reduceat(L + 2, np.arange(0, total, per))
        assert s_len.max() < 2 ** 32 and (s_off + s_len)[-1] == nbytes

        plain = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
        assert A.dev_fill_splitmix(plain.data_ptr(), nbytes + 64, 0x5452, 0, sp) == 0
        d_hdr = torch.from_numpy(hdr).to(dev)
        d_L = torch.from_numpy(L).to(dev)
        plain[d_hdr] = (d_L >> 8).to(torch.uint8)
        plain[d_hdr + 1] = (d_L & 0xFF).to(torch.uint8)
        d_off = torch.from_numpy(s_off).to(dev)
        d_len = torch.from_numpy(s_len.astype(np.int32)).to(dev)
        result = torch.zeros((sessions, 4), dtype=torch.int32, device=dev)
        status = torch.zeros(total, dtype=torch.uint8, device=dev)
        k1 = torch.empty(sessions * 32, dtype=torch.uint8, device=dev)
        k2 = torch.empty(sessions * 32, dtype=torch.uint8, device=dev)
        assert A.dev_fill_splitmix(k1.data_ptr(), sessions * 32, 0x4B31, 0, sp) == 0
        assert A.dev_fill_splitmix(k2.data_ptr(), sessions * 32, 0x4B32, 0, sp) == 0
        wire = plain.clone()
        sealed = torch.empty_like(plain)

        for cname in args.ciphers.split(","):
            cipher = {"ChaChaPoly": A.CHACHAPOLY, "AESGCM": A.AESGCM}[cname]
            cb = A.dev_ctx_bytes(cipher)
            # the reference arm: the initiator's send contexts and one descriptor per frame, built here
            ctx = torch.empty(sessions * cb, dtype=torch.uint8, device=dev)
            assert A.dev_prepare(cipher, k1.data_ptr(), sessions, ctx.data_ptr(), sp) == 0
            recs = np.zeros(total, dtype=[("in_off", "<u8"), ("out_off", "<u8"), ("nonce", "<u8"), ("ctx_off", "<u8"),
                                          ("ad_off", "<u8"), ("len", "<u4"), ("ad_len", "<u4")])
            recs["in_off"] = recs["out_off"] = hdr + 2
            recs["nonce"] = np.arange(total) % per
            recs["ctx_off"] = (np.arange(total) // per) * cb
            recs["len"] = L - 16
            d_recs = torch.from_numpy(recs.view(np.uint8)).to(dev)

            def ragged(open_):
                return A.dev_ragged(open_, cipher, ctx_base=ctx.data_ptr(), recs=d_recs.data_ptr(), inp=wire.data_ptr(),
                                    out=wire.data_ptr(), n_records=total, status=status.data_ptr(), ad=wire.data_ptr(),
                                    stream=sp)

            rc, ini = A.dev_transport_new(cipher, A.ROLE_INITIATOR, sessions, k1=k1.data_ptr(), k2=k2.data_ptr(),
                                          max_frames=total, stream=sp)
            assert rc == 0, hex(rc)
            rc, res = A.dev_transport_new(cipher, A.ROLE_RESPONDER, sessions, k1=k1.data_ptr(), k2=k2.data_ptr(),
                                          max_frames=total, stream=sp)
            assert rc == 0, hex(rc)
            io = dict(wire=wire.data_ptr(), off=d_off.data_ptr(), length=d_len.data_ptr(), result=result.data_ptr(), stream=sp)

            def reset():
                """untimed, in stream order: every nonce back to 0"""
                for tr, d in ((ini, 0), (res, 1)):
                    assert hip.hipMemsetAsync(A.dev_transport_nonces(tr, d), 0, 8 * sessions, sp) == 0

            # ---- the two arms compute the same bytes
            wire.copy_(plain)
            assert ragged(False) == 0
            sealed.copy_(wire)
            wire.copy_(plain)
            assert A.dev_transport_seal_frames(ini, **io) == 0
            torch.cuda.synchronize(dev)
            r = result.cpu().numpy()
            ok = torch.equal(wire, sealed) and int(r[:, 0].sum()) == total and not r[:, 2].any() \
                and (r[:, 1].astype(np.int64) == s_len).all()
            assert A.dev_transport_open_frames(res, **io) == 0
            torch.cuda.synchronize(dev)
            r = result.cpu().numpy()
            body = torch.ones(nbytes + 64, dtype=torch.bool, device=dev)  # the tags stay as sealed
            tag0 = d_hdr + 2 + d_L - 16
            for j in range(16):
                body[tag0 + j] = False
            ok = ok and torch.equal(wire[body], plain[body]) and int(r[:, 0].sum()) == total and not r[:, 2].any()
            del body
            bad += not ok

            arms = {"transport_seal": (lambda: A.dev_transport_seal_frames(ini, **io), plain),
                    "ragged_seal": (lambda: ragged(False), plain),
                    "transport_open": (lambda: A.dev_transport_open_frames(res, **io), sealed),
                    "ragged_open": (lambda: ragged(True), sealed)}
            times = {k: [] for k in arms}
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for rnd in range(args.warmup + args.rounds):
                for name, (fn, image) in arms.items():  # the arms alternate inside a round
                    wire.copy_(image)
                    reset()
                    t0.record(main_s)
                    rc = fn()
                    t1.record(main_s)
                    torch.cuda.synchronize(dev)
                    if rc:
                        raise RuntimeError(f"{name}: {rc:#x}")
                    if rnd >= args.warmup:
                        times[name].append(t0.elapsed_time(t1) * 1000.0)
            # the last timed open verified everything
            r = result.cpu().numpy()
            bad += bool(status.any().item()) or int(r[:, 0].sum()) != total

            def stat(v):
                med = statistics.median(v)
                return dict(us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                            spread=round((max(v) - min(v)) / med, 4))
            row = dict(shape=shape, cipher=cname, sessions=sessions, frames_per_session=per, frames=total,
                       wire_bytes=nbytes, rounds=args.rounds, warmup=args.warmup, device=torch.cuda.get_device_name(dev),
                       layout="frames back to back, any alignment; records = frames; automatic lanes",
                       **{k: stat(v) for k, v in times.items()},
                       seal_ratio=round(statistics.median(times["transport_seal"]) / statistics.median(times["ragged_seal"]), 4),
                       open_ratio=round(statistics.median(times["transport_open"]) / statistics.median(times["ragged_open"]), 4),
                       seal_added_us=round(statistics.median(times["transport_seal"]) - statistics.median(times["ragged_seal"]), 1),
                       open_added_us=round(statistics.median(times["transport_open"]) - statistics.median(times["ragged_open"]), 1),
                       verified=bool(ok))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
            A.dev_transport_free(ini)
            A.dev_transport_free(res)
            del ctx, d_recs
        del plain, wire, sealed
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
