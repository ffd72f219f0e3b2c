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

--ragged measures the per-session offsets and lengths of
_write_message_ragged / _read_message_ragged instead (ragged_main below):

    python tools/handshake_bench.py --ragged --parent-lib <a build of the parent commit> \\
        --rounds 9 --out profiles/handshake_ragged.jsonl
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


UNIFORM_CALLS = ("noise_aead_dev_handshake_new", "noise_aead_dev_handshake_free", "noise_aead_dev_handshake_overhead",
                 "noise_aead_dev_handshake_write_message", "noise_aead_dev_handshake_read_message",
                 "noise_aead_dev_handshake_split")


def ragged_main(args):
    """--ragged: what per-session offsets and lengths cost.  The XX
    ChaChaPoly/BLAKE2s responder (new, read, write, read, split) with 16-byte
    payloads in four arms that alternate inside a round: the uniform calls of
    the parent commit's build (--parent-lib, left out when it is not given),
    the uniform calls of this build, the ragged calls with equal lengths and
    strided offsets, and the ragged calls with payload lengths spread over
    0..1024 at scrambled offsets.  Before any timing the arms with 16-byte
    payloads must have written the same message and the same split keys."""
    import ctypes as C

    import numpy as np
    import torch
    import noise_aead as A
    this = A.lib()
    assert torch.cuda.is_available(), "handshake_bench needs the GPU: there is no CPU path"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    main_s = torch.cuda.current_stream(dev)
    sp = main_s.cuda_stream
    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        for fn in UNIFORM_CALLS:
            getattr(parent, fn).restype = getattr(this, fn).restype
            getattr(parent, fn).argtypes = getattr(this, fn).argtypes
    name = b"Noise_XX_25519_ChaChaPoly_BLAKE2s"
    OVER = (32, 96, 64)
    lines, bad = [], 0

    def filled(nbytes, word0):
        t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        assert A.dev_fill_splitmix(t.data_ptr(), nbytes, 0x4853, word0, sp) == 0
        return t

    def dev_array(values, dtype):
        return torch.from_numpy(np.asarray(values, dtype=dtype).view(np.int64 if dtype == np.uint64 else np.int32)).to(dev)

    for n in [int(x) for x in args.n.split(",")]:
        ini_s, ini_e, res_e, res_s = filled(n * 32, 0), filled(n * 32, 1 << 40), filled(n * 32, 2 << 40), filled(32, 3 << 40)

        def new(lib, initiator):
            cfg = A.NoiseAeadHandshakeConfig(name, A.ROLE_INITIATOR if initiator else A.ROLE_RESPONDER, n, None, 0, 0,
                                             None, 32, (ini_s if initiator else res_s).data_ptr(), 32 if initiator else 0,
                                             (ini_e if initiator else res_e).data_ptr(), 32, None, 32)
            hs = C.c_void_p()
            rc = lib.noise_aead_dev_handshake_new(C.byref(hs), C.byref(cfg), sp)
            assert rc == 0, hex(rc)
            return hs.value

        class Layout:
            """the payloads and the three messages of one arm: lengths, offsets, buffers"""

            def __init__(self, plens, scrambled, seed):
                rng = np.random.default_rng(seed)
                self.plens = [np.asarray(p, dtype=np.uint32) for p in plens]
                self.pay, self.pay_off, self.pay_len, self.msg, self.msg_off, self.msg_len, self.out_len = ([] for _ in range(7))
                for j in range(3):
                    for widths, bufs, offs in ((self.plens[j], self.pay, self.pay_off),
                                               (self.plens[j] + OVER[j], self.msg, self.msg_off)):
                        order = rng.permutation(n) if scrambled else np.arange(n)
                        off = np.zeros(n, dtype=np.uint64)
                        off[order] = np.concatenate((np.zeros(1, dtype=np.uint64), np.cumsum(widths[order].astype(np.uint64))[:-1]))
                        total = int(widths.astype(np.uint64).sum())
                        bufs.append(filled(total, (4 + j) << 40) if bufs is self.pay else
                                    torch.zeros(max(total, 1), dtype=torch.uint8, device=dev))
                        offs.append(dev_array(off, np.uint64))
                    self.pay_len.append(dev_array(self.plens[j], np.uint32))
                    self.msg_len.append(dev_array(self.plens[j] + OVER[j], np.uint32))
                    self.out_len.append(torch.zeros(n, dtype=torch.int32, device=dev))
                self.k1, self.k2 = (torch.zeros(n * 32, dtype=torch.uint8, device=dev) for _ in range(2))

        def write(lib, hs, lay, j, ragged):
            if ragged:
                return lib.noise_aead_dev_handshake_write_message_ragged(
                    hs, lay.pay[j].data_ptr(), lay.pay_off[j].data_ptr(), lay.pay_len[j].data_ptr(), lay.msg[j].data_ptr(),
                    lay.msg_off[j].data_ptr(), lay.out_len[j].data_ptr(), sp)
            return lib.noise_aead_dev_handshake_write_message(hs, lay.pay[j].data_ptr(), PAYLOAD, PAYLOAD,
                                                              lay.msg[j].data_ptr(), PAYLOAD + OVER[j], sp)

        def read(lib, hs, lay, j, ragged, into):
            if ragged:
                return lib.noise_aead_dev_handshake_read_message_ragged(
                    hs, lay.msg[j].data_ptr(), lay.msg_off[j].data_ptr(), lay.msg_len[j].data_ptr(), into.data_ptr(),
                    lay.pay_off[j].data_ptr(), lay.out_len[j].data_ptr(), sp)
            return lib.noise_aead_dev_handshake_read_message(hs, lay.msg[j].data_ptr(), PAYLOAD + OVER[j], PAYLOAD + OVER[j],
                                                             into.data_ptr(), PAYLOAD, sp)

        equal = [np.full(n, PAYLOAD)] * 3
        spread = [(np.arange(n, dtype=np.uint64) * 37 + 11 * j) % 1025 for j in range(3)]
        lays = dict(uniform=Layout(equal, False, 1), ragged_equal=Layout(equal, False, 1), ragged_spread=Layout(spread, True, 2))
        if parent:
            lays["parent_uniform"] = Layout(equal, False, 1)
        arms = {"uniform": (this, False), "ragged_equal": (this, True), "ragged_spread": (this, True),
                "parent_uniform": (parent, False)}
        got = torch.zeros(int(max(p.sum() for p in spread)) + 1, dtype=torch.uint8, device=dev)
        # the untimed full handshakes: the messages each arm's responder reads
        for arm, lay in lays.items():
            lib, ragged = arms[arm]
            ini, res = new(lib, True), new(lib, False)
            for j in range(3):
                w, r = (ini, res) if j % 2 == 0 else (res, ini)
                assert lib.noise_aead_dev_handshake_overhead(w) == OVER[j]
                assert write(lib, w, lay, j, ragged) == 0 and read(lib, r, lay, j, ragged, got) == 0
            keys = [torch.zeros(n * 32, dtype=torch.uint8, device=dev) for _ in range(2)]
            assert lib.noise_aead_dev_handshake_split(ini, keys[0].data_ptr(), keys[1].data_ptr(), None, sp) == 0
            assert lib.noise_aead_dev_handshake_split(res, lay.k1.data_ptr(), lay.k2.data_ptr(), None, sp) == 0
            torch.cuda.synchronize(dev)
            ok = torch.equal(keys[0], lay.k1) and torch.equal(keys[1], lay.k2) and bool(lay.k1.any())
            if ragged:  # the reader's out lengths (written last) are the payloads' own
                ok = ok and all(torch.equal(lay.out_len[j], lay.pay_len[j]) for j in range(3))
            bad += not ok
            lib.noise_aead_dev_handshake_free(ini)
            lib.noise_aead_dev_handshake_free(res)
            lay.msg1_first = lay.msg[1].clone()
        same = all(torch.equal(lays["uniform"].msg[j], lays[a].msg[j]) for a in lays if a != "ragged_spread" for j in range(3)) \
            and all(torch.equal(lays["uniform"].k1, lays[a].k1) for a in lays if a != "ragged_spread")
        bad += not same

        def responder(arm):
            lib, ragged = arms[arm]
            lay = lays[arm]

            def run():
                hs = new(lib, False)
                rc = read(lib, hs, lay, 0, ragged, got) or write(lib, hs, lay, 1, ragged) or read(lib, hs, lay, 2, ragged, got) \
                    or lib.noise_aead_dev_handshake_split(hs, lay.k1.data_ptr(), lay.k2.data_ptr(), None, sp)
                if rc:
                    raise RuntimeError(f"{arm}: {rc:#x}")
                return lib, hs
            return run

        def window(fn):
            held = []
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(main_s)
            for _ in range(args.reps):
                held.append(fn())
            t1.record(main_s)
            torch.cuda.synchronize(dev)
            for lib, hs in held:
                lib.noise_aead_dev_handshake_free(hs)
            return t0.elapsed_time(t1) * 1000.0 / args.reps

        order = [a for a in args.arm_order.split(",") if a in lays]
        assert sorted(order) == sorted(lays), "--arm-order names every arm once"
        for _ in range(args.warmup):
            for arm in order:
                window(responder(arm))
        times = {a: [] for a in order}
        for _ in range(args.rounds):  # the arms alternate inside a round
            for arm in order:
                times[arm].append(window(responder(arm)))
        torch.cuda.synchronize(dev)
        again = all(torch.equal(lays[a].msg[1], lays[a].msg1_first) for a in order)  # the timed runs wrote the same message
        bad += not again
        med = {a: statistics.median(t) for a, t in times.items()}
        row = dict(name=name.decode(), mode="ragged", n=n, payload=PAYLOAD, spread_payloads="0..1024, mean %.0f" %
                   float(np.mean([p.mean() for p in spread])), reps=args.reps, rounds=args.rounds, warmup=args.warmup,
                   device=torch.cuda.get_device_name(dev),
                   arms={a: dict(us_median=round(med[a], 1), us_min=round(min(times[a]), 1), us_max=round(max(times[a]), 1))
                         for a in order},
                   arms_not_run=[a for a in arms if a not in lays],
                   ragged_equal_over_uniform=round(med["ragged_equal"] / med["uniform"], 4),
                   ragged_spread_over_uniform=round(med["ragged_spread"] / med["uniform"], 4),
                   verified=bool(same and again and not bad))
        if parent:
            lo, hi = min(times["parent_uniform"]), max(times["parent_uniform"])
            row["uniform_median_inside_parent_min_max"] = bool(lo <= med["uniform"] <= hi)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ragged", action="store_true", help="the ragged message calls against the uniform ones (XX responder)")
    ap.add_argument("--parent-lib", default=None, help="--ragged: a build of the parent commit, for its uniform arm")
    ap.add_argument("--arm-order", default="parent_uniform,uniform,ragged_equal,ragged_spread",
                    help="--ragged: the order of the arms inside a round")
    ap.add_argument("--n", default="4096,65536")
    ap.add_argument("--patterns", default="NN,XX,IK")
    ap.add_argument("--suites", default="ChaChaPoly_BLAKE2s,AESGCM_SHA256")
    ap.add_argument("--reps", type=int, default=6, help="handshake batches per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.ragged:
        return ragged_main(args)

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
