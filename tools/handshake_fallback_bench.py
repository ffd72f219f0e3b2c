#!/usr/bin/env python3
"""What the Noise Pipes fallback costs a server
(noise_aead_dev_handshake_fallback / _fallback_merge, header section 15).

A server with one static key (stride 0) answers n IK clients of which a share
holds a stale copy of that key: 0 %, 1 %, 10 % and 100 %, at n = 4096 and
65 536, ChaChaPoly/BLAKE2s, 16-byte payloads.  The timed responder tick is
new, read IK message 1, fallback (ONLY_FAILED), write the fallback's first
message and read its second, write IK message 2 for the clients that stay (the
original has no split without it), both splits, merge.  The comparison is the
same n sessions as a fresh XX batch (new, read, write, read, split), which a
server without this call would have to run for the clients it could not
answer — after reading the statuses on the host.  Both alternate inside a round
and are timed with device events over `--reps` ticks per window; the objects
are freed outside the window.

Before any timing both ends run the whole exchange once: the messages the timed
responder reads come from it, and after the merge on both ends the two sides
must hold the same non-zero keys for every session with every status byte 0.
DESIGN.md 4.19 records the figures.

    python tools/handshake_fallback_bench.py --out profiles/handshake_fallback.jsonl
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "noise-c_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

PAYLOAD = 16
IK, XX = "Noise_IK_25519_ChaChaPoly_BLAKE2s", "Noise_XX_25519_ChaChaPoly_BLAKE2s"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,65536")
    ap.add_argument("--shares", default="0,0.01,0.1,1", help="the share of the clients whose copy of the static key is stale")
    ap.add_argument("--reps", type=int, default=4, help="ticks per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import noise_aead as A
    from gpu_support import peek_u8
    A.lib()
    assert torch.cuda.is_available(), "handshake_fallback_bench needs the GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_s = torch.cuda.current_stream(dev)
    sp = main_s.cuda_stream
    lines, bad = [], 0

    def filled(nbytes, word0):
        t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert A.dev_fill_splitmix(t.data_ptr(), nbytes, 0x4642, word0, sp) == 0
        return t

    def zeros(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def public(priv, n):
        pub = zeros(n * 32)
        assert A.dev_dh_public(A.DH_CURVE25519, priv=priv.data_ptr(), n=n, pub_out=pub.data_ptr(), stream=sp) == 0
        return pub

    def window(fn):
        held = []
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(main_s)
        for _ in range(args.reps):
            held += fn()
        t1.record(main_s)
        torch.cuda.synchronize(dev)
        for hs in held:
            A.dev_handshake_free(hs)
        return t0.elapsed_time(t1) * 1000.0 / args.reps

    def write(hs, msg, mlen, payload):
        rc = A.dev_handshake_write_message(hs, payload=payload.data_ptr(), payload_stride=PAYLOAD, payload_len=PAYLOAD,
                                           msg=msg.data_ptr(), msg_stride=mlen, stream=sp)
        if rc:
            raise RuntimeError(f"write: {rc:#x}")

    def read(hs, msg, mlen, got):
        rc = A.dev_handshake_read_message(hs, msg=msg.data_ptr(), msg_stride=mlen, msg_len=mlen, payload=got.data_ptr(),
                                          payload_stride=PAYLOAD, stream=sp)
        if rc:
            raise RuntimeError(f"read: {rc:#x}")

    for n in [int(x) for x in args.n.split(",")]:
        ini_s, ini_e, res_e, fresh_e = (filled(n * 32, k << 40) for k in range(4))
        res_s, old_s = filled(32, 4 << 40), filled(32, 5 << 40)
        res_s_pub, old_s_pub = public(res_s, 1), public(old_s, 1)
        payload, got = filled(n * PAYLOAD, 6 << 40), zeros(n * PAYLOAD)
        M1, FA, FB, M2 = PAYLOAD + 96, PAYLOAD + 96, PAYLOAD + 64, PAYLOAD + 48  # IK 1, fallback 1 and 2, IK 2
        X = (PAYLOAD + 32, PAYLOAD + 96, PAYLOAD + 64)
        out = zeros(n * (PAYLOAD + 96))
        k = [zeros(n * 32) for _ in range(8)]
        hh = [zeros(n * 32) for _ in range(4)]
        merged = [zeros(n), zeros(n)]

        def new(name, initiator, rs=None):
            kw = dict(local_ephemeral=(ini_e if initiator else res_e).data_ptr(),
                      local_static=(ini_s if initiator else res_s).data_ptr(), local_static_stride=32 if initiator else 0)
            if rs is not None:
                kw.update(remote_static=rs.data_ptr(), remote_static_stride=32)
            rc, hs = A.dev_handshake_new(name, A.ROLE_INITIATOR if initiator else A.ROLE_RESPONDER, n, stream=sp, **kw)
            assert rc == 0, hex(rc)
            return hs

        def merge(fb, hs, k1, k2, h, fb_k1, fb_k2, fb_h, status):
            rc = A.dev_handshake_fallback_merge(fb, hs_status=A.dev_handshake_status(hs), k1=k1.data_ptr(), k2=k2.data_ptr(),
                                                fb_k1=fb_k1.data_ptr(), fb_k2=fb_k2.data_ptr(), h=h.data_ptr(),
                                                fb_h=fb_h.data_ptr(), status=status.data_ptr(), stream=sp)
            if rc:
                raise RuntimeError(f"merge: {rc:#x}")

        def split(hs, k1, k2, h):
            if A.dev_handshake_split(hs, k1=k1.data_ptr(), k2=k2.data_ptr(), handshake_hash=h.data_ptr(), stream=sp):
                raise RuntimeError("split")

        # the XX messages the comparison's responder reads
        xi, xr = new(XX, True), new(XX, False)
        xmsg = [zeros(n * m) for m in X]
        for j in range(3):
            w, r = (xi, xr) if j % 2 == 0 else (xr, xi)
            write(w, xmsg[j], X[j], payload)
            read(r, xmsg[j], X[j], got)
        split(xi, k[0], k[1], hh[0])
        split(xr, k[2], k[3], hh[1])
        torch.cuda.synchronize(dev)
        bad += not (torch.equal(k[0], k[2]) and torch.equal(k[1], k[3]) and bool(k[0].any()))
        A.dev_handshake_free(xi)
        A.dev_handshake_free(xr)

        def xx_responder():
            hs = new(XX, False)
            read(hs, xmsg[0], X[0], got)
            write(hs, out, X[1], payload)
            read(hs, xmsg[2], X[2], got)
            split(hs, k[2], k[3], hh[1])
            return [hs]

        for share in [float(x) for x in args.shares.split(",")]:
            every = round(1 / share) if share else 0
            stale = torch.zeros(n, dtype=torch.bool, device=dev)
            if every:
                stale[::every] = True
            n_stale = int(stale.sum())
            rs = res_s_pub.repeat(n).view(n, 32).clone()
            rs[stale] = old_s_pub
            rs = rs.view(-1).contiguous()
            select = stale.to(torch.uint8)
            # the whole exchange once, untimed, on both ends
            ini, res = new(IK, True, rs), new(IK, False)
            m1, fa, fb_, m2 = zeros(n * M1), zeros(n * FA), zeros(n * FB), zeros(n * M2)
            write(ini, m1, M1, payload)
            read(res, m1, M1, got)
            rc, fr = A.dev_handshake_fallback(res, local_ephemeral=fresh_e.data_ptr(), flags=A.FALLBACK_ONLY_FAILED, stream=sp)
            assert rc == 0, hex(rc)
            rc, fi = A.dev_handshake_fallback(ini, select=select.data_ptr(), stream=sp)
            assert rc == 0, hex(rc)
            write(fr, fa, FA, payload)
            read(fi, fa, FA, got)
            write(fi, fb_, FB, payload)
            read(fr, fb_, FB, got)
            write(res, m2, M2, payload)
            read(ini, m2, M2, got)
            split(ini, k[0], k[1], hh[0])
            split(fi, k[4], k[5], hh[2])
            merge(fi, ini, k[0], k[1], hh[0], k[4], k[5], hh[2], merged[0])
            split(res, k[2], k[3], hh[1])
            split(fr, k[6], k[7], hh[3])
            merge(fr, res, k[2], k[3], hh[1], k[6], k[7], hh[3], merged[1])
            torch.cuda.synchronize(dev)
            failed = int((peek_u8(A.dev_handshake_status(res), n) == 1).sum())
            ok = (torch.equal(k[0], k[2]) and torch.equal(k[1], k[3]) and torch.equal(hh[0], hh[1])
                  and not bool(merged[0].any()) and not bool(merged[1].any())
                  and bool(k[0].view(n, 32).any(dim=1).all()) and failed == n_stale)
            bad += not ok
            first_keys = k[2].clone()
            for hs in (ini, res, fr, fi):
                A.dev_handshake_free(hs)

            def tick():
                hs = new(IK, False)
                read(hs, m1, M1, got)
                rc, fb = A.dev_handshake_fallback(hs, local_ephemeral=fresh_e.data_ptr(), flags=A.FALLBACK_ONLY_FAILED,
                                                  stream=sp)
                if rc:
                    raise RuntimeError(f"fallback: {rc:#x}")
                write(fb, out, FA, payload)
                read(fb, fb_, FB, got)
                write(hs, out, M2, payload)
                split(hs, k[2], k[3], hh[1])
                split(fb, k[6], k[7], hh[3])
                merge(fb, hs, k[2], k[3], hh[1], k[6], k[7], hh[3], merged[1])
                return [hs, fb]

            for _ in range(args.warmup):
                window(tick)
                window(xx_responder)
            t_fb, t_xx = [], []
            for _ in range(args.rounds):  # the two alternate inside a round
                t_fb.append(window(tick))
                t_xx.append(window(xx_responder))
            window(tick)  # the last writer of k[2]
            ok2 = torch.equal(k[2], first_keys) and not bool(merged[1].any())  # the timed ticks computed the same keys
            bad += not ok2
            med, med_xx = statistics.median(t_fb), statistics.median(t_xx)
            row = dict(name=IK, n=n, stale_share=share, stale=n_stale, payload=PAYLOAD, reps=args.reps, rounds=args.rounds,
                       warmup=args.warmup, device=torch.cuda.get_device_name(dev),
                       tick_us_median=round(med, 1), tick_us_min=round(min(t_fb), 1), tick_us_max=round(max(t_fb), 1),
                       xx_us_median=round(med_xx, 1), xx_us_min=round(min(t_xx), 1), xx_us_max=round(max(t_xx), 1),
                       tick_over_xx=round(med / med_xx, 4), sessions_per_s=round(n / med * 1e6), verified=bool(ok and ok2))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
