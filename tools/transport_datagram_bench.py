#!/usr/bin/env python3
"""What the datagram calls (include/noise_aead_hip.h section 11) cost over the
stream calls of the session table, on identical payloads.

Parts, on one table of 65 536 slots per role, ChaChaPoly and AESGCM:
    tick   m active slots have one frame of 1400 B payload each.  The open's
           arms: (a) dg_open, noise_aead_dev_transport_open_datagrams on
           in-order counters; (b) of_open, _open_frames_of on the same
           payloads as stream frames; (c) ragged_open, the bare
           noise_aead_dev_open_ragged of the same records (descriptors built
           beforehand); (d) dg_replay, (a) with every frame a replay, which
           shows what the pre-check saves.  The seal's arms: dg_seal, of_seal,
           ragged_seal.  m = 1024 and m = n, scrambled slots, the call's cap m.
    keys   noise_aead_dev_transport_set_keys and _clear_keys of m = 4096 and
           m = 65 536 scrambled slots, which now also zero 136 bytes of window
           per slot; with --parent-lib (a build of the parent commit) the two
           builds alternate call by call, first this build first, then the
           parent's first, so that an effect of the position shows.

One call is timed with a pair of device events; between calls, untimed, the
wire, the nonces and the windows are put back.  The arms of a part alternate
call by call inside a round, `--rounds` rounds after `--warmup`.  A line gives
per arm the median, minimum and maximum microseconds.  Before the timing the
three seals must give the same CT || tag, the datagram open must give every
payload back with every status 0, and the replayed open must give every status
5 and change no byte.  DESIGN.md 4.14 records the figures.

    python tools/transport_datagram_bench.py --out profiles/transport_datagram.jsonl
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


def stat(v):
    med = statistics.median(v)
    return dict(us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                spread=round((max(v) - min(v)) / med, 4))


def parent_library(path):
    """the table calls of another build of the library, side by side with this one"""
    L = ctypes.CDLL(path)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.noise_aead_dev_transport_new_unkeyed.argtypes = [ctypes.POINTER(vp), i, i, u32, u32, vp]
    L.noise_aead_dev_transport_set_keys.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.noise_aead_dev_transport_clear_keys.argtypes = [vp, vp, u32, vp]
    L.noise_aead_dev_transport_free.argtypes = [vp]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ciphers", default="ChaChaPoly,AESGCM")
    ap.add_argument("--parts", default="tick,keys")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libnoise_aead_hip.so built from the parent commit (the keys part)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import noise_aead as A
    A.lib()
    assert torch.cuda.is_available(), "transport_datagram_bench needs the GPU: there is no CPU path"
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

    def framed(m, body, seed):
        """m frames of `body` bytes each, random but for the headers: (tensor with 64 bytes of slack, stride)"""
        stride = 2 + body
        t = torch.empty(m * stride + 64, dtype=torch.uint8, device=dev)
        assert A.dev_fill_splitmix(t.data_ptr(), m * stride + 64, seed, 0, sp) == 0
        hdr = torch.arange(m, device=dev, dtype=torch.int64) * stride
        t[hdr] = body >> 8
        t[hdr + 1] = body & 0xFF
        return t, stride

    def rows(t, m, stride):
        return t[:m * stride].view(m, stride)

    k1 = torch.empty(N * 32, dtype=torch.uint8, device=dev)
    k2 = torch.empty(N * 32, dtype=torch.uint8, device=dev)
    assert A.dev_fill_splitmix(k1.data_ptr(), N * 32, 0x4B31, 0, sp) == 0
    assert A.dev_fill_splitmix(k2.data_ptr(), N * 32, 0x4B32, 0, sp) == 0
    device_name = torch.cuda.get_device_name(dev)
    rec_t = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("nonce", "<u8"), ("ctx_off", "<u8"), ("ad_off", "<u8"),
                      ("len", "<u4"), ("ad_len", "<u4")])

    for cname in args.ciphers.split(","):
        cipher = {"ChaChaPoly": A.CHACHAPOLY, "AESGCM": A.AESGCM}[cname]
        cb = A.dev_ctx_bytes(cipher)

        if "tick" in args.parts.split(","):
            rc, ini = A.dev_transport_new(cipher, A.ROLE_INITIATOR, N, k1=k1.data_ptr(), k2=k2.data_ptr(), max_frames=N, stream=sp)
            assert rc == 0, hex(rc)
            rc, res = A.dev_transport_new(cipher, A.ROLE_RESPONDER, N, k1=k1.data_ptr(), k2=k2.data_ptr(), max_frames=N, stream=sp)
            assert rc == 0, hex(rc)
            win_ptr, bits = A.dev_transport_replay(res)
            assert win_ptr and bits == 1024
            seen = torch.empty(N * WINDOW_BYTES, dtype=torch.uint8, device=dev)  # the windows after counter 0 of every slot

            def reset(windows=None):
                for tr, d in ((ini, 0), (res, 1)):
                    assert hip.hipMemsetAsync(A.dev_transport_nonces(tr, d), 0, 8 * N, sp) == 0
                if windows is None:
                    assert hip.hipMemsetAsync(win_ptr, 0, N * WINDOW_BYTES, sp) == 0
                else:
                    assert hip.hipMemcpyAsync(win_ptr, windows.data_ptr(), N * WINDOW_BYTES, 3, sp) == 0

            for m in (1024, N):
                slots = scrambled(m)
                d_slots = torch.from_numpy(slots.astype(np.uint32).view(np.int32)).to(dev)
                # the same payloads as datagram frames (counter room, payload, tag room) and as stream frames
                dg_plain, dg_stride = framed(m, 8 + PLAIN + 16, 0x5452)
                st_plain, st_stride = framed(m, PLAIN + 16, 0x5453)
                rows(dg_plain, m, dg_stride)[:, 2:10] = 0
                rows(st_plain, m, st_stride)[:, 2:2 + PLAIN] = rows(dg_plain, m, dg_stride)[:, 10:10 + PLAIN]
                dg_wire, st_wire, rg_wire = dg_plain.clone(), st_plain.clone(), dg_plain.clone()
                dg_off = torch.arange(m, device=dev, dtype=torch.int64) * dg_stride
                st_off = torch.arange(m, device=dev, dtype=torch.int64) * st_stride
                dg_len = torch.full((m,), dg_stride, dtype=torch.int32, device=dev)
                st_len = torch.full((m,), st_stride, dtype=torch.int32, device=dev)
                r16 = torch.zeros((m, 4), dtype=torch.int32, device=dev)
                r24 = torch.zeros((m, 6), dtype=torch.int32, device=dev)
                fstat = torch.full((m,), 0xEE, dtype=torch.uint8, device=dev)
                rstat = torch.full((m,), 0xEE, dtype=torch.uint8, device=dev)
                dg = dict(slots=d_slots.data_ptr(), m=m, max_frames=m, wire=dg_wire.data_ptr(), off=dg_off.data_ptr(),
                          length=dg_len.data_ptr(), stream=sp)
                st = dict(slots=d_slots.data_ptr(), m=m, max_frames=m, wire=st_wire.data_ptr(), off=st_off.data_ptr(),
                          length=st_len.data_ptr(), result=r16.data_ptr(), stream=sp)
                # the records of the bare ragged calls: what the datagram builder writes, made beforehand
                recs = {}
                for name, ctx0 in (("seal", 0), ("open", N)):
                    r = np.zeros(m, dtype=rec_t)
                    r["in_off"] = r["out_off"] = np.arange(m, dtype=np.uint64) * dg_stride + 10
                    r["ctx_off"] = (slots.astype(np.uint64) + ctx0) * cb
                    r["len"] = PLAIN
                    recs[name] = torch.from_numpy(r.view(np.uint8).copy()).to(dev)
                ctx = {"seal": A.debug_transport_ctx(ini, 0)[0], "open": A.debug_transport_ctx(res, 0)[0]}

                def ragged(name):
                    return A.dev_ragged(name == "open", cipher, ctx_base=ctx[name], recs=recs[name].data_ptr(),
                                        inp=rg_wire.data_ptr(), out=rg_wire.data_ptr(), ad=rg_wire.data_ptr(), n_records=m,
                                        status=rstat.data_ptr() if name == "open" else 0, stream=sp)

                def dg_open():
                    return A.dev_transport_open_datagrams(res, result=r24.data_ptr(), frame_status=fstat.data_ptr(), **dg)

                # ---- the arms compute the same bytes
                reset()
                assert A.dev_transport_seal_datagrams(ini, result=r16.data_ptr(), **dg) == 0
                torch.cuda.synchronize(dev)
                r = r16.cpu().numpy()
                ok = int(r[:, 0].sum()) == m and not r[:, 2].any()
                reset()
                assert A.dev_transport_seal_frames_of(ini, **st) == 0 and ragged("seal") == 0
                torch.cuda.synchronize(dev)
                dg_sealed, st_sealed = dg_wire.clone(), st_wire.clone()
                ok = ok and torch.equal(rows(dg_sealed, m, dg_stride)[:, 10:], rows(st_sealed, m, st_stride)[:, 2:])
                ok = ok and torch.equal(dg_sealed, rg_wire) and not rows(dg_sealed, m, dg_stride)[:, 2:10].any()  # counter 0
                reset()
                assert dg_open() == 0
                torch.cuda.synchronize(dev)
                r = r24.cpu().numpy()
                ok = ok and int(r[:, 3].sum()) == m and not fstat.any()
                ok = ok and torch.equal(rows(dg_wire, m, dg_stride)[:, :10 + PLAIN], rows(dg_plain, m, dg_stride)[:, :10 + PLAIN])
                assert hip.hipMemcpyAsync(seen.data_ptr(), win_ptr, N * WINDOW_BYTES, 3, sp) == 0
                dg_wire.copy_(dg_sealed)
                assert dg_open() == 0  # every frame again
                torch.cuda.synchronize(dev)
                ok = ok and bool((fstat == 5).all()) and torch.equal(dg_wire, dg_sealed) and int(r24.cpu().numpy()[:, 3].sum()) == 0
                assert A.dev_transport_open_frames_of(res, **st) == 0 and ragged("open") == 0
                torch.cuda.synchronize(dev)
                ok = ok and torch.equal(rows(st_wire, m, st_stride)[:, 2:2 + PLAIN], rows(dg_plain, m, dg_stride)[:, 10:10 + PLAIN])
                ok = ok and torch.equal(rows(rg_wire, m, dg_stride)[:, 10:10 + PLAIN], rows(dg_plain, m, dg_stride)[:, 10:10 + PLAIN])
                ok = ok and not rstat.any()
                bad += not ok

                arms = {"dg_seal": lambda: A.dev_transport_seal_datagrams(ini, result=r16.data_ptr(), **dg),
                        "of_seal": lambda: A.dev_transport_seal_frames_of(ini, **st),
                        "ragged_seal": lambda: ragged("seal"),
                        "dg_open": dg_open,
                        "of_open": lambda: A.dev_transport_open_frames_of(res, **st),
                        "ragged_open": lambda: ragged("open"),
                        "dg_replay": dg_open}

                def before(name):
                    sealing = name.endswith("seal")
                    dg_wire.copy_(dg_plain if sealing else dg_sealed)
                    st_wire.copy_(st_plain if sealing else st_sealed)
                    rg_wire.copy_(dg_plain if sealing else dg_sealed)
                    reset(seen if name == "dg_replay" else None)
                times = timed(arms, before)
                bad += not bool((fstat == 5).all())  # the last arm was the replay
                med = {k: statistics.median(v) for k, v in times.items()}
                lines.append(json.dumps(dict(
                    part="tick", cipher=cname, slots=N, active=m, object_max_frames=N, call_max_frames=m,
                    frame_payload=PLAIN, rounds=args.rounds, warmup=args.warmup, device=device_name,
                    **{k: stat(v) for k, v in times.items()},
                    seal_over_stream=round(med["dg_seal"] / med["of_seal"], 4),
                    open_over_stream=round(med["dg_open"] / med["of_open"], 4),
                    replay_over_open=round(med["dg_replay"] / med["dg_open"], 4), verified=bool(ok))))
                print(lines[-1], flush=True)
                del dg_plain, st_plain, dg_wire, st_wire, rg_wire, dg_sealed, st_sealed
            A.dev_transport_free(ini)
            A.dev_transport_free(res)
            del seen
            torch.cuda.empty_cache()

        if "keys" in args.parts.split(","):
            rc, tab = A.dev_transport_new_unkeyed(cipher, A.ROLE_INITIATOR, N, max_frames=64, stream=sp)
            assert rc == 0, hex(rc)
            P, ptab = None, ctypes.c_void_p()
            if args.parent_lib:
                P = parent_library(args.parent_lib)
                assert P.noise_aead_dev_transport_new_unkeyed(ctypes.byref(ptab), cipher, A.ROLE_INITIATOR, N, 64, sp) == 0
            for m in (4096, N):
                slots = scrambled(m)
                d_slots = torch.from_numpy(slots.astype(np.uint32).view(np.int32)).to(dev)
                this = {"set_keys": lambda: A.dev_transport_set_keys(tab, slots=d_slots.data_ptr(), m=m, k1=k1.data_ptr(),
                                                                     k2=k2.data_ptr(), stream=sp),
                        "clear_keys": lambda: A.dev_transport_clear_keys(tab, slots=d_slots.data_ptr(), m=m, stream=sp)}
                parent = {}
                if P:
                    parent = {"set_keys_parent": lambda: P.noise_aead_dev_transport_set_keys(
                                  ptab, d_slots.data_ptr(), m, k1.data_ptr(), k2.data_ptr(), None, sp),
                              "clear_keys_parent": lambda: P.noise_aead_dev_transport_clear_keys(ptab, d_slots.data_ptr(), m, sp)}
                for order, arms in (("this_first", {**this, **parent}), ("parent_first", {**parent, **this})):
                    if order == "parent_first" and not P:
                        continue
                    times = timed(arms, lambda name: None)
                    med = {k: statistics.median(v) for k, v in times.items()}
                    ratios = {}
                    if P:
                        ratios = dict(set_keys_over_parent=round(med["set_keys"] / med["set_keys_parent"], 4),
                                      clear_keys_over_parent=round(med["clear_keys"] / med["clear_keys_parent"], 4))
                    lines.append(json.dumps(dict(
                        part="keys", cipher=cname, slots=N, keyed=m, ctx_bytes=cb, order=order, rounds=args.rounds,
                        warmup=args.warmup, device=device_name, **{k: stat(v) for k, v in times.items()}, **ratios)))
                    print(lines[-1], flush=True)
            A.dev_transport_free(tab)
            if P:
                P.noise_aead_dev_transport_free(ptab)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
