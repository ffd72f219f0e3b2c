#!/usr/bin/env python3
"""Rate of whole responder-side handshakes on the device
(noise_aead_dev_handshake_*), and the share of it that is not the ladders.

For NN, XX and IK over ChaChaPoly/BLAKE2s and AESGCM/SHA256, n = 4096 (the
session count of bench.py's C4/C5) and 65 536 sessions: a server with one
static key (stride 0) and n fresh ephemerals answers n clients.  A device
initiator batch and a responder batch first run the handshake once (untimed);
its messages are what the timed responder reads, and its two sides must agree
on every split key, with session 0 checked against tests/handshake_model.py.
Then the responder alone — new, every read and write, split — is timed with
device events over `--reps` handshakes per window in `--rounds` rounds after a
warm-up; the objects are freed outside the window.  In the same run the bare
ladder launches that handshake contains (noise_aead_dev_dh_calculate once per
DH token, noise_aead_dev_dh_public for the ephemerals and for the one static
key) are timed the same way.  A line gives the median, minimum and maximum
microseconds per handshake batch, the spread, handshakes per second at the
median, the ladders' microseconds and the share of the time outside them, the
launches per message (library calls that launch: ladder, MixKey, MixHash,
descriptor builder, AEAD, null check, AES-GCM prepare) and the device bytes
the object holds per session.  DESIGN.md 4.11 records the figures.

    python tools/handshake_bench.py --out profiles/handshake.jsonl
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "noise-c_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

PAYLOAD = 16


def launches(M, pattern, cipher_name, initiator=False):
    """library calls that launch, per message, as csrc/handshake.hip issues them"""
    out, stale = [], True
    for idx in range(len(M.PATTERNS[pattern][2])):
        steps = M.message_plan(pattern, initiator, False, idx)[0]
        writes = (idx % 2 == 0) == initiator
        k = 0
        for s in steps:
            if ":" in s:  # a DH token: ladder + MixKey
                k += 2
                stale = True
            elif s in ("e", "e+mk"):  # MixHash (+ null check on a read) (+ MixKey)
                k += (1 if writes else 2) + (s == "e+mk")
                stale = stale or s == "e+mk"
            elif s.endswith("+aead"):  # builder + AEAD + MixHash, after a prepare when k changed
                k += 3 + (1 if stale and cipher_name == "AESGCM" else 0)
                stale = False
            else:  # an unkeyed s or payload: MixHash with copy
                k += 1
        out.append(k)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,65536")
    ap.add_argument("--patterns", default="NN,XX,IK")
    ap.add_argument("--suites", default="ChaChaPoly_BLAKE2s,AESGCM_SHA256")
    ap.add_argument("--reps", type=int, default=6, help="handshake batches per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import noise_aead as A
    import handshake_model as M
    from oracle import Oracle
    A.lib()
    assert torch.cuda.is_available(), "handshake_bench needs the GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_s = torch.cuda.current_stream(dev)
    sp = main_s.cuda_stream
    orc = Oracle()
    lines, bad = [], 0

    def filled(nbytes, word0):
        t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert A.dev_fill_splitmix(t.data_ptr(), nbytes, 0x4853, word0, sp) == 0
        return t

    for n in [int(x) for x in args.n.split(",")]:
        ini_s, ini_e, res_e = filled(n * 32, 0), filled(n * 32, 1 << 40), filled(n * 32, 2 << 40)
        res_s = filled(32, 3 << 40)
        res_s_pub = torch.zeros(32, dtype=torch.uint8, device=dev)
        assert A.dev_dh_public(A.DH_CURVE25519, priv=res_s.data_ptr(), n=1, pub_out=res_s_pub.data_ptr(), stream=sp) == 0
        payload = filled(n * PAYLOAD, 4 << 40)
        scratch = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        for pattern in args.patterns.split(","):
            for suite in args.suites.split(","):
                name = f"Noise_{pattern}_25519_{suite}"
                n_msgs = len(M.PATTERNS[pattern][2])
                need_i, need_r = M.needs(pattern, True), M.needs(pattern, False)

                def new(initiator):
                    need = need_i if initiator else need_r
                    kw = dict(local_ephemeral=(ini_e if initiator else res_e).data_ptr())
                    if need[0]:
                        kw.update(local_static=(ini_s if initiator else res_s).data_ptr(),
                                  local_static_stride=32 if initiator else 0)
                    if need[2]:  # IK: the initiator knows the server's key
                        assert initiator
                        kw.update(remote_static=res_s_pub.data_ptr(), remote_static_stride=0)
                    rc, hs = A.dev_handshake_new(name, A.ROLE_INITIATOR if initiator else A.ROLE_RESPONDER, n,
                                                 stream=sp, **kw)
                    assert rc == 0, hex(rc)
                    return hs

                # the untimed full handshake: the messages the responder will read
                ini, res = new(True), new(False)
                msgs, lens = [], []
                for idx in range(n_msgs):
                    w, r = (ini, res) if idx % 2 == 0 else (res, ini)
                    mlen = PAYLOAD + A.dev_handshake_overhead(w)
                    m = torch.zeros(n * mlen, dtype=torch.uint8, device=dev)
                    got = torch.zeros(n * PAYLOAD, dtype=torch.uint8, device=dev)
                    assert A.dev_handshake_write_message(w, payload=payload.data_ptr(), payload_stride=PAYLOAD,
                                                         payload_len=PAYLOAD, msg=m.data_ptr(), msg_stride=mlen,
                                                         stream=sp) == 0
                    assert A.dev_handshake_read_message(r, msg=m.data_ptr(), msg_stride=mlen, msg_len=mlen,
                                                        payload=got.data_ptr(), payload_stride=PAYLOAD, stream=sp) == 0
                    msgs.append(m)
                    lens.append(mlen)
                keys = [torch.zeros(n * 32, dtype=torch.uint8, device=dev) for _ in range(4)]
                assert A.dev_handshake_split(ini, k1=keys[0].data_ptr(), k2=keys[1].data_ptr(), stream=sp) == 0
                assert A.dev_handshake_split(res, k1=keys[2].data_ptr(), k2=keys[3].data_ptr(), stream=sp) == 0
                torch.cuda.synchronize(dev)
                ok = torch.equal(keys[0], keys[2]) and torch.equal(keys[1], keys[3]) and bool(keys[0].any())
                # session 0 against the model
                s0 = lambda t: bytes(t[:32].cpu().numpy())
                mi = M.Session(orc, name, True, s=s0(ini_s) if need_i[0] else None, e=s0(ini_e),
                               rs=s0(res_s_pub) if need_i[2] else None)
                mr = M.Session(orc, name, False, s=s0(res_s) if need_r[0] else None, e=s0(res_e))
                p0 = bytes(payload[:PAYLOAD].cpu().numpy())
                for idx in range(n_msgs):
                    mw, mrd = (mi, mr) if idx % 2 == 0 else (mr, mi)
                    m = mw.write(p0)
                    ok = ok and m == bytes(msgs[idx][:lens[idx]].cpu().numpy()) and mrd.read(m) == p0
                ok = ok and mr.split()[0] == s0(keys[2])
                A.dev_handshake_free(ini)
                A.dev_handshake_free(res)
                bad += not ok

                out_msg = torch.zeros(n * (PAYLOAD + 128), dtype=torch.uint8, device=dev)
                got = torch.zeros(n * PAYLOAD, dtype=torch.uint8, device=dev)

                def responder():
                    hs = new(False)
                    for idx in range(n_msgs):
                        if idx % 2 == 0:
                            rc = A.dev_handshake_read_message(hs, msg=msgs[idx].data_ptr(), msg_stride=lens[idx],
                                                              msg_len=lens[idx], payload=got.data_ptr(),
                                                              payload_stride=PAYLOAD, stream=sp)
                        else:
                            rc = A.dev_handshake_write_message(hs, payload=payload.data_ptr(), payload_stride=PAYLOAD,
                                                               payload_len=PAYLOAD, msg=out_msg.data_ptr(),
                                                               msg_stride=lens[idx], stream=sp)
                        if rc:
                            raise RuntimeError(f"message {idx}: {rc:#x}")
                    if A.dev_handshake_split(hs, k1=keys[2].data_ptr(), k2=keys[3].data_ptr(), stream=sp):
                        raise RuntimeError("split")
                    return hs

                n_dh = sum(len(t) == 2 for m in M.PATTERNS[pattern][2] for t in m)

                def ladders():
                    """the bare ladder launches of one responder handshake"""
                    rc = A.dev_dh_public(A.DH_CURVE25519, priv=res_e.data_ptr(), n=n, pub_out=scratch.data_ptr(), stream=sp)
                    if need_r[0]:
                        rc |= A.dev_dh_public(A.DH_CURVE25519, priv=res_s.data_ptr(), priv_stride=0, n=1,
                                              pub_out=res_s_pub.data_ptr(), stream=sp)
                    for _ in range(n_dh):
                        rc |= A.dev_dh_calculate(A.DH_CURVE25519, priv=res_e.data_ptr(), pub=ini_e.data_ptr(), n=n,
                                                 shared=scratch.data_ptr(), stream=sp)
                    if rc:
                        raise RuntimeError("ladder launch failed")

                def window(fn):
                    held = []
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(main_s)
                    for _ in range(args.reps):
                        held.append(fn())
                    t1.record(main_s)
                    torch.cuda.synchronize(dev)
                    for hs in held:
                        if hs:
                            A.dev_handshake_free(hs)
                    return t0.elapsed_time(t1) * 1000.0 / args.reps

                for _ in range(args.warmup):
                    window(responder)
                    window(ladders)
                t_hs, t_dh = [], []
                for _ in range(args.rounds):  # the two alternate inside a round
                    t_hs.append(window(responder))
                    t_dh.append(window(ladders))
                torch.cuda.synchronize(dev)
                ok2 = torch.equal(keys[0], keys[2]) and torch.equal(keys[1], keys[3])  # the timed runs computed the same keys
                bad += not ok2
                med, med_dh = statistics.median(t_hs), statistics.median(t_dh)
                hl = M.HASH_LEN[M.HASHES[suite.split("_")[1]]]
                cipher = M.CIPHERS[suite.split("_")[0]]
                per_session = 2 * hl + 32 + (A.dev_ctx_bytes(cipher) if suite.startswith("AESGCM") else 0) + 32 + 2 \
                    + 4 * 32 + 48
                row = dict(name=name, n=n, payload=PAYLOAD, reps=args.reps, rounds=args.rounds, warmup=args.warmup,
                           device=torch.cuda.get_device_name(dev),
                           us_median=round(med, 1), us_min=round(min(t_hs), 1), us_max=round(max(t_hs), 1),
                           spread=round((max(t_hs) - min(t_hs)) / med, 4), handshakes_per_s=round(n / med * 1e6),
                           ladder_launches=dict(dh_calculate=n_dh, dh_public_n=1, dh_public_1=int(need_r[0])),
                           ladders_us_median=round(med_dh, 1), ladders_spread=round((max(t_dh) - min(t_dh)) / med_dh, 4),
                           share_outside_ladders=round(1 - med_dh / med, 4),
                           launches_per_message=launches(M, pattern, suite.split("_")[0]),
                           device_bytes_per_session=per_session, verified=bool(ok and ok2))
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
