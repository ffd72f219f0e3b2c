"""Child process of test_gpu_worker.py's placement test (not collected by
pytest): single-record seal/open through the resident worker, checked
against the oracle, under whatever NOISE_AEAD_WORKER_VRAM the parent set.
The worker picks its request placement once per process, hence the child.
Prints "placement N" (noise_aead_debug_worker_placement) and exits non-zero
on the first mismatch.  The other modes (--classes, --sequence, --threads,
--head-edges, ...) say what they run in their functions' docstrings."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "noise-c_amd")):
    sys.path.insert(0, p)

import noise_aead as aead  # noqa: E402
import oracle as O  # noqa: E402

# the hand-written lists of the placement test and of --head-edges
# (tests/test_length_classes_host.py counts what they reach)
MAIN_LENS = (0, 1, 17, 1024, 1400, 2100, 3100, 4033, 8000, 16384)
MAIN_ADS = (0, 32)
HEAD_EDGE_ADS = (0, 17)


def head_edge_lens(A):
    ad_pad = (A + 15) & ~15
    return sorted({head + d - 32 - ad_pad - tag
                   for head in (2048, 3072) for tag in (0, 16) for d in (-1, 0, 1, 15, 16, 17)})


def main():
    if not os.path.exists(O.ORACLE_SO):
        O.build(ref=False)
    orc = O.Oracle()
    aead.lib()
    for cipher in (0x4301, 0x4302):
        rnd = random.Random(cipher ^ 0x77)
        key = bytes(rnd.randrange(256) for _ in range(32))
        _, tx = aead.CipherState.new_by_id(cipher)
        _, rx = aead.CipherState.new_by_id(cipher)
        assert tx.init_key(key) == 0 and rx.init_key(key) == 0
        n = 0
        for L in MAIN_LENS:
            if cipher == 0x4302 and L > 4096:
                continue
            for A in MAIN_ADS:
                pt = bytes(rnd.randrange(256) for _ in range(L))
                ad = bytes(rnd.randrange(256) for _ in range(A))
                ct = tx.seal(pt, ad)
                if ct != orc.encrypt(cipher, key, n, pt, ad):
                    print("seal mismatch", hex(cipher), L, A)
                    return 1
                bad = bytearray(ct)
                bad[rnd.randrange(len(bad))] ^= 1
                rc, back = rx.open(bytes(bad), ad)
                if rc != aead.ERROR_MAC_FAILURE or back != bytes(bad) or rx.nonce != n:
                    print("tamper not rejected", hex(cipher), L, A)
                    return 1
                rc, back = rx.open(ct, ad)
                if rc != 0 or back != pt:
                    print("open mismatch", hex(cipher), L, A)
                    return 1
                n += 1
        tx.free()
        rx.free()
    print("placement", aead.lib().noise_aead_debug_worker_placement())
    return 0


def free_check():
    """--free-check (run with NOISE_AEAD_DEBUG_WORKER_IDLE_MS=10000, so no
    worker leaves by idling): an AES-GCM single call leaves the worker
    resident with the state's context cached in LDS; freeing the state must
    make it leave (it zeroes that cache on the way out) within 200 ms.
    Prints "left_ms X"."""
    import time
    lib = aead.lib()
    lib.noise_aead_debug_workers_resident.restype = int
    _, st = aead.CipherState.new_by_id(0x4302)
    assert st.init_key(bytes(range(32))) == 0
    st.seal(bytes(100))
    time.sleep(0.05)
    if lib.noise_aead_debug_workers_resident() < 1:
        print("no resident worker after the call")
        return 1
    t0 = time.time()
    st.free()
    while lib.noise_aead_debug_workers_resident() and time.time() - t0 < 0.2:
        time.sleep(0.001)
    left = lib.noise_aead_debug_workers_resident() == 0
    print("left_ms", round((time.time() - t0) * 1e3, 3) if left else -1)
    return 0 if left else 1


def free_concurrent():
    """--free-concurrent (run with NOISE_AEAD_WORKER_QUEUES=2,
    NOISE_AEAD_WORKER_SLOTS=1 and NOISE_AEAD_DEBUG_WORKER_IDLE_MS=10000:
    two groups of one slot each): thread A keeps making ChaChaPoly
    single calls (its worker stays resident, its request headers keep being
    written); the main thread's AES-GCM state S, used once from the main
    thread (the other worker caches its context), is freed.  The worker that
    was sent S's context must leave — its stop word is no longer part of the
    header A's calls rewrite — and A's worker, which never saw
    S's context, must stay (no relaunch of it).  Prints "parked_ok 1"."""
    import threading
    import time
    lib = aead.lib()
    lib.noise_aead_debug_workers_resident.restype = int
    lib.noise_aead_debug_worker_launches.restype = int
    stop = [False]
    errs = []
    started = threading.Event()

    def caller():
        _, cs = aead.CipherState.new_by_id(0x4301)
        cs.init_key(bytes(range(32)))
        n = 0
        while not stop[0]:
            if len(cs.seal(bytes(1400))) != 1416:
                errs.append("seal")
            n += 1
            if n == 50:
                started.set()
        cs.free()

    T0 = time.time()
    marks = []
    th = threading.Thread(target=caller)
    th.start()
    started.wait(30)
    marks.append(time.time())
    _, st = aead.CipherState.new_by_id(0x4302)
    assert st.init_key(bytes(range(1, 33))) == 0
    st.seal(bytes(100))
    marks.append(time.time())
    time.sleep(0.05)
    import ctypes as C

    def per_group():
        a = (C.c_uint * 12)()
        lib.noise_aead_debug_worker_group_launches(a, 12)
        return list(a)
    g0 = per_group()
    res0, l0 = lib.noise_aead_debug_workers_resident(), lib.noise_aead_debug_worker_launches()
    st.free()
    t0 = time.time()
    while lib.noise_aead_debug_workers_resident() >= res0 and time.time() - t0 < 0.5:
        time.sleep(0.001)
    res1 = lib.noise_aead_debug_workers_resident()
    marks.append(time.time())
    time.sleep(0.1)
    l1 = lib.noise_aead_debug_worker_launches()
    stop[0] = True
    th.join()
    ok = res0 == 2 and res1 == 1 and l1 == l0 and not errs
    print("resident", res0, res1, "launches", l0, l1, "errs", errs[:3])
    print("per group + ensure causes", g0, per_group())
    lib.noise_aead_debug_worker_leave_reason.restype = C.c_uint
    print("leave reasons g0 g1", lib.noise_aead_debug_worker_leave_reason(0, 0),
          lib.noise_aead_debug_worker_leave_reason(1, 0))
    for gi in (0, 1):
        a = (C.c_uint * 4)()
        lib.noise_aead_debug_worker_leave_info(gi, 0, a)
        print("leave info", gi, list(a), "age_s", ((a[1] - a[0]) & 0xffffffff) / 1e8)
    print("timeline", [round(x - T0, 3) for x in marks])
    print("parked_ok", 1 if ok else 0)
    return 0 if ok else 1


def relaunch_free():
    """--relaunch-free (run with NOISE_AEAD_DEBUG_WORKER_LEAVE=1 and
    NOISE_AEAD_DEBUG_WORKER_IDLE_MS=10000): every single call's group leaves
    after the call checked it was up and before the request is posted, so the
    call's wait loop relaunches the group and the new workgroup serves the
    request and caches the AES-GCM context.  Freeing the state must still park
    that group within 200 ms (the relaunch used to wipe the slot's
    context history).  The call's result is checked against the oracle.
    Prints "relaunch_free_ok 1"."""
    import time
    lib = aead.lib()
    lib.noise_aead_debug_workers_resident.restype = int
    orc = O.Oracle()
    key = bytes(range(7, 39))
    _, st = aead.CipherState.new_by_id(0x4302)
    assert st.init_key(key) == 0
    pt = bytes(range(200))
    ct = st.seal(pt)
    if ct != orc.encrypt(0x4302, key, 0, pt):
        print("seal mismatch")
        return 1
    time.sleep(0.05)
    res0 = lib.noise_aead_debug_workers_resident()
    t0 = time.time()
    st.free()
    while lib.noise_aead_debug_workers_resident() and time.time() - t0 < 0.2:
        time.sleep(0.001)
    res1 = lib.noise_aead_debug_workers_resident()
    ok = res0 >= 1 and res1 == 0
    print("resident", res0, res1)
    print("relaunch_free_ok", 1 if ok else 0)
    return 0 if ok else 1


def group_idle():
    """--group-idle (run with NOISE_AEAD_WORKER_QUEUES=1,
    NOISE_AEAD_WORKER_SLOTS=2, NOISE_AEAD_DEBUG_WORKER_IDLE_MS=20): one
    group of two slots.  The main thread makes one call (its slot then stays
    idle) while thread A keeps calling for 300 ms: the group must not leave
    for the idle slot's sake (a workgroup leaves for idleness only when every
    slot of its group is idle), so no relaunch happens; once both are quiet
    the group leaves by itself.  Prints "group_idle_ok 1"."""
    import threading
    import time
    lib = aead.lib()
    lib.noise_aead_debug_workers_resident.restype = int
    lib.noise_aead_debug_worker_launches.restype = int
    _, mine = aead.CipherState.new_by_id(0x4301)
    mine.init_key(bytes(range(32)))
    started = threading.Event()
    stop = [False]
    errs = []

    def caller():
        _, cs = aead.CipherState.new_by_id(0x4301)
        cs.init_key(bytes(range(3, 35)))
        started.set()
        while not stop[0]:
            if len(cs.seal(bytes(1400))) != 1416:
                errs.append("seal")
        cs.free()

    assert len(mine.seal(bytes(100))) == 116  # slot 0: launches the group
    th = threading.Thread(target=caller)
    th.start()
    started.wait(30)
    time.sleep(0.05)
    l0 = lib.noise_aead_debug_worker_launches()
    time.sleep(0.3)  # 15 idle timeouts of the main thread's slot
    l1 = lib.noise_aead_debug_worker_launches()
    stop[0] = True
    th.join()
    t0 = time.time()
    while lib.noise_aead_debug_workers_resident() and time.time() - t0 < 2.0:
        time.sleep(0.005)
    left = lib.noise_aead_debug_workers_resident() == 0
    mine.free()
    ok = l0 == l1 and left and not errs
    print("launches", l0, l1, "left", left, "errs", errs[:3])
    print("group_idle_ok", 1 if ok else 0)
    return 0 if ok else 1


def head_edges():
    """--head-edges: the transport edge of the request's input stream (key ||
    AD padded to 16 || record [|| tag]).  Its first `head` bytes travel as
    stamped chunks, the rest raw: head is 3072 stream bytes with the request
    in host memory and 2048 in device memory.  For both heads, both ciphers,
    AD 0 and 17 and both directions (open's stream carries the 16-byte tag),
    every record length whose stream total is head - 1, head, head + 1,
    head + 15, head + 16 or head + 17: seal against the oracle, tampered open
    rejected with buffer and nonce untouched, open back.  Prints
    "head_edges N" (cases run) and "placement P"."""
    if not os.path.exists(O.ORACLE_SO):
        O.build(ref=False)
    orc = O.Oracle()
    aead.lib()
    cases = 0
    for cipher in (0x4301, 0x4302):
        rnd = random.Random(cipher ^ 0x4EAD)
        key = bytes(rnd.randrange(256) for _ in range(32))
        _, tx = aead.CipherState.new_by_id(cipher)
        _, rx = aead.CipherState.new_by_id(cipher)
        assert tx.init_key(key) == 0 and rx.init_key(key) == 0
        n = 0
        for A in HEAD_EDGE_ADS:
            lens = head_edge_lens(A)
            assert len(lens) == 18 and max(lens) + 16 <= 3100
            ad = bytes(rnd.randrange(256) for _ in range(A))
            for L in lens:
                pt = rnd.getrandbits(8 * L).to_bytes(L, "little")
                ct = tx.seal(pt, ad)
                if ct != orc.encrypt(cipher, key, n, pt, ad):
                    print("seal mismatch", hex(cipher), L, A)
                    return 1
                bad = bytearray(ct)
                bad[rnd.randrange(len(bad))] ^= 1 << rnd.randrange(8)
                rc, back = rx.open(bytes(bad), ad)
                if rc != aead.ERROR_MAC_FAILURE or back != bytes(bad) or rx.nonce != n:
                    print("tamper not rejected", hex(cipher), L, A)
                    return 1
                rc, back = rx.open(ct, ad)
                if rc != 0 or back != pt:
                    print("open mismatch", hex(cipher), L, A)
                    return 1
                n += 1
                cases += 1
        tx.free()
        rx.free()
    print("head_edges", cases)
    print("placement", aead.lib().noise_aead_debug_worker_placement())
    return 0


CHACHA, AES = aead.CHACHAPOLY, aead.AESGCM
NONCE0 = (1 << 32) - 3  # both nonce words live: the counter crosses 2^32 inside every run


def _oracle():
    if not os.path.exists(O.ORACLE_SO):
        O.build(ref=False)
    return O.Oracle()


def _flip(rnd, ct, ad, where):
    """(ct, ad) with one random bit flipped in bytes [lo, hi) of `where` =
    (field, lo, hi), field "ct", "tag" or "ad"; an empty range falls to the
    tag."""
    field, lo, hi = where
    if hi <= lo:
        field, lo, hi = "tag", 0, 16
    ct, ad = bytearray(ct), bytearray(ad)
    pos, bit = rnd.randrange(lo, hi), 1 << rnd.randrange(8)
    if field == "ad":
        ad[pos] ^= bit
    else:
        ct[pos + (len(ct) - 16 if field == "tag" else 0)] ^= bit
    return bytes(ct), bytes(ad)


class _Pair:
    """a sealing and an opening state under one key, nonces from NONCE0"""

    def __init__(self, cipher, key):
        self.cipher, self.key, self.n = cipher, key, NONCE0
        _, self.tx = aead.CipherState.new_by_id(cipher)
        _, self.rx = aead.CipherState.new_by_id(cipher)
        for st in (self.tx, self.rx):
            assert st.init_key(key) == 0 and st.set_nonce(NONCE0) == 0

    def record(self, orc, rnd, seed, L, A, where):
        """Seal against the oracle, a tampered open rejected with buffer and
        nonce as given, open back: None, or what went wrong."""
        pt, ad = orc.fill(seed, L), orc.fill(seed ^ 0xAD, A)
        ct = self.tx.seal(pt, ad)
        if ct != orc.encrypt(self.cipher, self.key, self.n, pt, ad):
            return "seal mismatch"
        bad, bad_ad = _flip(rnd, ct, ad, where)
        rc, back = self.rx.open(bad, bad_ad)
        if rc != aead.ERROR_MAC_FAILURE or back != bad or self.rx.nonce != self.n:
            return "tamper in %s not rejected" % (where,)
        rc, back = self.rx.open(ct, ad)
        if rc != 0 or back != pt:
            return "open mismatch"
        self.n += 1
        if self.tx.nonce != self.n or self.rx.nonce != self.n:
            return "nonce"
        return None

    def free(self):
        self.tx.free()
        self.rx.free()


def classes(which):
    """--classes chacha | aes: every record length tests/length_classes.py
    derives for the resident worker, under the placement
    (NOISE_AEAD_WORKER_VRAM) and GHASH (NOISE_AEAD_CT_GHASH) the parent set.
    chacha: full("wfast"), wfast_border(), full("wmulti") and
    full("wtransport", placement in use); the tampered bit of case i lands in
    the ciphertext, the tag or the AD (i % 3), for the multi-path records in
    chunk 0, the last chunk or a block of the last ChaCha pass
    (wmulti_flips).  aes: full("gcm_wide", ct), lengths over 4096 included
    (gcm_wide_record in place in LDS).  Stops at the first mismatch, naming
    cipher, len, ad_len and the case.  Prints "classes N" and "placement P"."""
    import length_classes as LC
    orc = _oracle()
    lib = aead.lib()
    ct_ghash = os.environ.get("NOISE_AEAD_CT_GHASH", "0") == "1"
    rnd = random.Random(0xC1A55 + ct_ghash)
    cipher = CHACHA if which == "chacha" else AES
    pair = _Pair(cipher, orc.fill(0x1234 + cipher, 32))
    pair.tx.seal(b"")  # the first call sets the worker up: the placement is known
    pair.rx.set_nonce(NONCE0 + 1)
    pair.n += 1
    placement = lib.noise_aead_debug_worker_placement()
    vram = 1 if placement == 2 else 0
    simple = lambda i, L, A: (("ct", 0, L), ("tag", 0, 16), ("ad", 0, A))[i % 3]
    if which == "chacha":
        lists = [("wfast", LC.full("wfast"), lambda x: LC.wfast(*x), simple),
                 ("border", LC.wfast_border(), lambda x: (LC.worker_fast_fits(*x),), simple),
                 ("wmulti", LC.full("wmulti"), lambda x: LC.wmulti(*x), lambda i, L, A: LC.wmulti_flips(L, A)[i % 3]),
                 ("wtransport", sorted({x[1:] for x in LC.full("wtransport", vram)}),
                  lambda x: (LC.wtransport(vram, 0, *x), LC.wtransport(vram, 1, *x)), simple)]
    else:
        lists = [("gcm_wide", LC.full("gcm_wide", 0, ct_ghash), lambda x: LC.gcm_wide(x[0], x[1], ct_ghash), simple)]
    done = 0
    for name, items, case, where in lists:
        for i, (L, A) in enumerate(items):
            err = pair.record(orc, rnd, (done << 8) ^ cipher, L, A, where(i, L, A))
            if err:
                print(err, hex(cipher), "list", name, "len", L, "ad_len", A, "case", case((L, A)))
                return 1
            done += 1
    pair.free()
    print("classes", done)
    print("placement", placement)
    return 0


SEQ_LENS = (0, 16, 100, 1400, 3100, 4033, 20000)  # head only, head + tail, fast / multi
SEQ_ADS = (0, 17)


def sequence():
    """--sequence: one thread, so one slot, serving three AES-GCM and two
    ChaChaPoly states in a fixed pseudo-random order, every result against
    the oracle: a seal, an open of the oracle's record, or a tampered open
    (rejected, buffer and nonce as given).  The third AES-GCM state evicts
    the least recently used of the two contexts cached in LDS, long records
    are followed by short ones, rejected opens by seals (each counted, none
    may be 0).  Midway one AES-GCM state is keyed again (same state and
    context address, next generation) and one is freed and a new one made
    (ctx_take may hand it the freed address).  Last, per cipher, one call
    with 257 and one with 1000 bytes of AD (over WORKER_MAX_AD): the launch
    path serves them with the same nonce and result, and no worker kernel is
    launched for them.  Prints "sequence N evictions E long_short S
    reject_seal R big_ad B"."""
    orc = _oracle()
    lib = aead.lib()
    lib.noise_aead_debug_worker_launches.restype = int
    rnd = random.Random(0x5E9)
    states = {}

    def make(name, cipher, salt):
        key = orc.fill(salt, 32)
        _, st = aead.CipherState.new_by_id(cipher)
        assert st.init_key(key) == 0 and st.set_nonce(NONCE0) == 0
        states[name] = [cipher, key, st]

    for k, name in enumerate(("A0", "A1", "A2", "C0", "C1")):
        make(name, AES if name[0] == "A" else CHACHA, 100 + k)

    def call(name, kind, L, A, seed):
        cipher, key, st = states[name]
        n = st.nonce
        pt, ad = orc.fill(seed, L), orc.fill(seed ^ 0xAD, A)
        exp = orc.encrypt(cipher, key, n, pt, ad)
        if kind == "seal":
            ok = st.seal(pt, ad) == exp and st.nonce == n + 1
        elif kind == "open":
            rc, back = st.open(exp, ad)
            ok = rc == 0 and back == pt and st.nonce == n + 1
        else:
            bad, bad_ad = _flip(rnd, exp, ad, (("ct", 0, L), ("tag", 0, 16), ("ad", 0, A))[seed % 3])
            rc, back = st.open(bad, bad_ad)
            ok = rc == aead.ERROR_MAC_FAILURE and back == bad and st.nonce == n
        if not ok:
            print(kind, "mismatch", hex(cipher), "state", name, "len", L, "ad_len", A, "call", seed)
        return ok

    evictions = long_short = reject_seal = 0
    lru, prev = [], None  # the two AES-GCM states used last; the call before
    for i in range(200):
        if i == 100:
            # A0 keyed again in place, A1 freed and made anew: both under new keys
            key = orc.fill(777, 32)
            assert states["A0"][2].init_key(key) == 0 and states["A0"][2].set_nonce(NONCE0) == 0
            states["A0"][1] = key
            states["A1"][2].free()
            make("A1", AES, 778)
        name = rnd.choice(sorted(states))
        kind = rnd.choice(("seal", "seal", "open", "tamper"))
        L, A = rnd.choice(SEQ_LENS), rnd.choice(SEQ_ADS)
        if not call(name, kind, L, A, i):
            return 1
        if name[0] == "A":
            evictions += len(lru) == 2 and name not in lru
            lru = ([x for x in lru if x != name] + [name])[-2:]
        if prev:
            long_short += prev[1] >= 4033 and L <= 100
            reject_seal += prev[0] == "tamper" and kind == "seal"
        prev = (kind, L)
    big_ad = 0
    for name in ("C0", "A2"):
        for kind, A in (("seal", 257), ("open", 1000)):
            before = lib.noise_aead_debug_worker_launches()
            if not call(name, kind, 1400, A, 1000 + A):
                return 1
            if lib.noise_aead_debug_worker_launches() != before:
                print("a worker kernel was launched for ad_len", A)
                return 1
            big_ad += 1
    for _cipher, _key, st in states.values():
        st.free()
    print("sequence", 200, "evictions", evictions, "long_short", long_short, "reject_seal", reject_seal,
          "big_ad", big_ad)
    return 0 if evictions and long_short and reject_seal else 1


THREAD_LENS = (0, 100, 1400, 4032, 4033, 9000)  # both ChaChaPoly paths, head only and head + tail


def threads():
    """--threads: four threads at once (ctypes releases the GIL), each with a
    ChaChaPoly and an AES-GCM pair of states of its own, 150 seal-then-open
    calls each over THREAD_LENS and both ciphers, compared with what the
    oracle gave before the loops started.  Prints "mismatches M" (0),
    "served S" (threads whose last call a worker served) and "resident R"
    (request slots of the resident groups)."""
    import threading
    orc = _oracle()
    lib = aead.lib()
    lib.noise_aead_debug_workers_resident.restype = int
    T, CALLS = 4, 150
    plans = []
    for t in range(T):
        pairs = {c: _Pair(c, orc.fill(31 * t + c, 32)) for c in (CHACHA, AES)}
        plan, n = [], {CHACHA: NONCE0, AES: NONCE0}
        for i in range(CALLS):
            c = (CHACHA, AES)[(i + t) % 2]
            L, A = THREAD_LENS[(i // 2 + t) % len(THREAD_LENS)], (0, 17)[(i // 12) % 2]
            pt, ad = orc.fill((t << 16) | i, L), orc.fill((t << 16) | i | 0x8000, A)
            plan.append((c, pt, ad, orc.encrypt(c, pairs[c].key, n[c], pt, ad)))
            n[c] += 1
        plans.append((pairs, plan))
    bad = [[] for _ in range(T)]
    served = [0] * T
    go = threading.Barrier(T)

    def run(t):
        pairs, plan = plans[t]
        go.wait()
        for i, (c, pt, ad, exp) in enumerate(plan):
            ct = pairs[c].tx.seal(pt, ad)
            rc, back = pairs[c].rx.open(ct, ad)
            if ct != exp or rc != 0 or back != pt:
                bad[t].append((hex(c), i, len(pt), len(ad)))
        served[t] = 1 if lib.noise_aead_debug_worker_placement() else 0

    ths = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    resident = lib.noise_aead_debug_workers_resident()
    for pairs, _plan in plans:
        for pr in pairs.values():
            pr.free()
    wrong = [x for b in bad for x in b]
    if wrong:
        print("first mismatches (cipher, call, len, ad_len)", wrong[:5])
    print("calls", T * CALLS, "mismatches", len(wrong), "served", sum(served), "resident", resident)
    return 0 if not wrong and sum(served) == T else 1


if __name__ == "__main__":
    if "--classes" in sys.argv:
        sys.exit(classes(sys.argv[sys.argv.index("--classes") + 1]))
    if "--sequence" in sys.argv:
        sys.exit(sequence())
    if "--threads" in sys.argv:
        sys.exit(threads())
    if "--head-edges" in sys.argv:
        sys.exit(head_edges())
    if "--group-idle" in sys.argv:
        sys.exit(group_idle())
    if "--free-check" in sys.argv:
        sys.exit(free_check())
    if "--free-concurrent" in sys.argv:
        sys.exit(free_concurrent())
    if "--relaunch-free" in sys.argv:
        sys.exit(relaunch_free())
    sys.exit(main())
