"""AEAD batch helpers that more than one GPU test module uses: uniform and
duplex launches against the oracle, the shared length lists, the segmented
ragged batch, the edge-value check of a kernel family (tests/edge_records.py)
and the resident worker's hand-picked lengths.  Importable without pytest and
without torch."""
import os
import random

import numpy as np

import edge_records as E
from gpu_support import (AES, CHACHA, FLAG_CT_GHASH, FLAG_ONE_PASS, FLAG_VERIFY_FIRST, REC_DT, _torch, dev, prepare, ru,
                         stream, sync)

LENS = [0, 1, 15, 16, 17, 48, 56, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257,
        1023, 1400, 1401, 4096, 5000]
EDGE_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1400, 1983, 1984, 1985, 2047, 2048,
             4095, 4096, 4097, 8191, 8192, 16383, 16384, 16385, 30000, 40000, 65519]
REFUSED = [65520, 70000]


# ------------------------------------------------------------ uniform batches

def gpu_uniform(aead, open_, cipher, keys, nonce_base, rps, inp, in_stride, length, count,
                out_stride, lanes=0, ad=None, ad_stride=0, ad_len=0, out_init=0xA5, out=None,
                flags=0):
    ctx, _k = prepare(aead, cipher, keys)
    d_nb = dev(np.asarray(nonce_base, dtype=np.uint64).view(np.int64))
    d_in = dev(inp)
    if out is None:
        d_out = _torch().full((count * out_stride + 64,), out_init, dtype=_torch().uint8, device="cuda")
    else:
        d_out = out
    d_st = _torch().full((max(1, count),), 7, dtype=_torch().uint8, device="cuda")
    d_ad = dev(ad) if ad is not None else None
    rc = aead.dev_uniform(open_, cipher, ctx=ctx.data_ptr(), nonce_base=d_nb.data_ptr(),
                          inp=d_in.data_ptr(), out=d_out.data_ptr(), in_stride=in_stride,
                          out_stride=out_stride, length=length, n_records=count,
                          recs_per_state=rps, status=d_st.data_ptr(),
                          ad=d_ad.data_ptr() if d_ad is not None else 0, ad_stride=ad_stride,
                          ad_len=ad_len, lanes=lanes, flags=flags, stream=stream())
    assert rc == 0, hex(rc)
    sync()
    return d_out.cpu().numpy(), d_st.cpu().numpy()[:count]


def rejected_fill(cipher, out_init, flags=0):
    """What a rejected record's output holds after an out-of-place open:
    untouched (its prior fill) when the open verified first — every open by
    default since round 6 (dispatch.h open_vf; every AES-GCM open always)
    — and zeroed after a ChaChaPoly open that opted into
    NOISE_AEAD_FLAG_ONE_PASS (VERIFY_FIRST overrides it)."""
    return 0 if (cipher == CHACHA and flags & FLAG_ONE_PASS and not flags & FLAG_VERIFY_FIRST) else out_init


def oracle_seal_records(oracle, cipher, keys, nonce_base, rps, pt, in_stride, length, count,
                        out_stride, ad=None, ad_stride=0, ad_len=0):
    out = np.full(count * out_stride + 64, 0xA5, dtype=np.uint8)
    for i in range(count):
        s = i // rps
        p = bytes(pt[i * in_stride: i * in_stride + length])
        a = bytes(ad[i * ad_stride: i * ad_stride + ad_len]) if ad_len else b""
        ct = oracle.encrypt(cipher, bytes(keys[s]), int(nonce_base[s]) + i % rps, p, a)
        out[i * out_stride: i * out_stride + length + 16] = np.frombuffer(ct, dtype=np.uint8)
    return out


# --------------------------------------------------------------------- duplex

def duplex_kernel(aead, cipher, lanes, layout, flags, case):
    """The one-launch kernel that include/noise_aead_hip.h promises the two
    jobs of a duplex case, None where it promises two launches: an empty job,
    a layout that is not FAST, AES-GCM without one state per 256 records;
    ChaChaPoly jobs on different lane counts, on other than 1, 4 or 8 lanes,
    on 4 or 8 with a verify-first open, or of which only one has a state per
    wave."""
    (_La, na, rpsa), (_Lb, nb_, rpsb) = case
    tf = {False: "false", True: "true"}
    if not na or not nb_ or layout == "packed":
        return None
    if cipher == AES:
        if rpsa % 256 or rpsb % 256:
            return None
        staged = os.environ.get("NOISE_AEAD_GCM_DUPLEX") == "staged"
        return "gcm_duplex_%s<%s>" % ("staged" if staged else "fused", tf[bool(flags & FLAG_CT_GHASH)])
    ka, kb = (lanes or aead.dev_duplex_lanes(cipher, n) for n in (na, nb_))
    vf = bool(flags & FLAG_VERIFY_FIRST) or not flags & FLAG_ONE_PASS
    if ka != kb or ka not in (1, 4, 8) or (ka != 1 and vf):
        return None
    ua, ub = rpsa % (64 // ka) == 0, rpsb % (64 // ka) == 0
    if ua != ub:
        return None
    return "chachapoly_duplex_solo<%s>" % tf[ua] if ka == 1 else "chachapoly_duplex_staged<%d,%s>" % (ka, tf[ua])


def duplex_cases_check(aead, oracle, cipher, cases, layout, lanes, flags, rng):
    """One noise_aead_dev_duplex_uniform call per case, written ((len, records,
    records per state) of the seal job, the same of the open job), checked
    against the oracle (test_duplex_vs_oracle; tests/aes_shapes_check.py runs
    it under the AES-GCM environment switches); the kernel that ran
    (noise_aead_debug_last_plan) is the one duplex_kernel names.  Returns the
    last case's device buffers."""
    for case in cases:
        (La, na, rpsa), (Lb, nb_, rpsb) = case
        def strides(L):
            if layout == "packed":
                return L, L + 16
            if layout == "slot128":
                return (max(L, 1) + 127) // 128 * 128, (L + 16 + 127) // 128 * 128
            return (max(L, 1) + 63) // 64 * 64, (L + 16 + 63) // 64 * 64
        ia, oa = strides(La)
        ib, ob = strides(Lb)
        Sa, Sb = (na + rpsa - 1) // rpsa, max(1, (nb_ + rpsb - 1) // rpsb)
        ka = rng.integers(0, 256, (Sa, 32), dtype=np.uint8)
        kb = rng.integers(0, 256, (Sb, 32), dtype=np.uint8)
        nba = rng.integers(0, 2**62, Sa, dtype=np.uint64)
        nbb = rng.integers(0, 2**62, Sb, dtype=np.uint64)
        pta = rng.integers(0, 256, na * ia + 64, dtype=np.uint8)
        ptb = rng.integers(0, 256, max(1, nb_) * ib + 64, dtype=np.uint8)
        exp_a = oracle_seal_records(oracle, cipher, ka, nba, rpsa, pta, ia, La, na, oa)
        ctb = oracle_seal_records(oracle, cipher, kb, nbb, rpsb, ptb, ib, Lb, nb_, ob)
        bad = sorted(set(int(x) for x in rng.integers(0, max(1, nb_), 4))) if nb_ else []
        for b in bad:
            ctb[b * ob + int(rng.integers(0, Lb + 16))] ^= 0x10
        ctxa, _k1 = prepare(aead, cipher, ka)
        ctxb, _k2 = prepare(aead, cipher, kb)
        d_nba, d_nbb = dev(nba.view(np.int64)), dev(nbb.view(np.int64))
        d_pta, d_ctb = dev(pta), dev(ctb)
        d_outa = _torch().full((na * oa + 64,), 0xA5, dtype=_torch().uint8, device="cuda")
        d_outb = _torch().full((max(1, nb_) * ib + 64,), 0x5A, dtype=_torch().uint8, device="cuda")
        d_st = _torch().full((max(1, nb_),), 7, dtype=_torch().uint8, device="cuda")
        sj = aead.uniform_job(ctx=ctxa.data_ptr(), nonce_base=d_nba.data_ptr(), inp=d_pta.data_ptr(),
                              out=d_outa.data_ptr(), in_stride=ia, out_stride=oa, length=La,
                              n_records=na, recs_per_state=rpsa, lanes=lanes,
                              flags=flags & FLAG_CT_GHASH)
        oj = aead.uniform_job(ctx=ctxb.data_ptr(), nonce_base=d_nbb.data_ptr(), inp=d_ctb.data_ptr(),
                              out=d_outb.data_ptr(), in_stride=ob, out_stride=ib, length=Lb,
                              n_records=nb_, recs_per_state=rpsb, status=d_st.data_ptr(),
                              lanes=lanes, flags=flags)
        rc = aead.dev_duplex(cipher, sj, oj, stream())
        assert rc == 0, (case, hex(rc))
        want = duplex_kernel(aead, cipher, lanes, layout, flags, case)
        ran = aead.last_plan().split()[0]
        assert ran == want if want else "duplex" not in ran, (case, ran, want)
        sync()
        got_a, back, st = d_outa.cpu().numpy(), d_outb.cpu().numpy(), d_st.cpu().numpy()
        assert np.array_equal(got_a[:na * oa], exp_a[:na * oa]), f"duplex seal len={La}"
        for i in range(nb_):
            seg = back[i * ib: i * ib + Lb]
            if i in bad:
                fill = rejected_fill(cipher, 0x5A, flags)
                assert st[i] == 1 and np.all(seg == fill), f"duplex open len={Lb} rec={i}"
            else:
                assert st[i] == 0, f"duplex open len={Lb} rec={i}"
                assert np.array_equal(seg, ptb[i * ib: i * ib + Lb]), f"len={Lb} rec={i}"
    return ctxa, d_nba, d_pta, d_outa, d_outb, d_st


# ------------------------------------------------- the segmented ragged batch

def _fast_slot(L):
    """a FAST slot: 64-B aligned, readable to roundup64(max(len, 1)), room for the tag"""
    return ((max(int(L), 1) + 16 + 63) // 64) * 64 + 64


def _ragged_batch(rng, count, S):
    lens = rng.integers(0, 2600, count)
    big = rng.choice(count, count // 50, replace=False)
    lens[big] = rng.integers(2600, 16385, len(big))
    lens[:len(EDGE_LENS)] = EDGE_LENS
    lens[len(EDGE_LENS):len(EDGE_LENS) + len(REFUSED)] = REFUSED
    perm = rng.permutation(count)          # descriptors in no particular order
    lens = lens[perm]
    adls = np.where(rng.random(count) < 0.1, rng.integers(0, 48, count), 0)
    slots = np.array([_fast_slot(min(int(L), 65519)) for L in lens], dtype=np.int64)
    offs = np.zeros(count, dtype=np.int64)
    offs[1:] = np.cumsum(slots)[:-1]
    total = int(offs[-1] + slots[-1]) + 256
    recs = np.zeros(count, dtype=REC_DT)
    recs["in_off"] = recs["out_off"] = offs
    recs["nonce"] = rng.integers(0, 2**63, count, dtype=np.int64).astype(np.uint64)
    key_idx = rng.integers(0, S, count).astype(np.uint32)
    recs["ctx_off"] = key_idx.astype(np.uint64) * 32
    recs["ad_off"] = np.arange(count, dtype=np.uint64) * 64
    recs["len"] = lens
    recs["ad_len"] = adls
    return recs, key_idx, offs, lens, total


# -------------------------------------- edge values through a kernel family

FLIPS = [("tag", i) for i in range(128)] + [("ct", "first"), ("ct", "last"), ("ct", "partial")]


def flip_at(flip, L):
    """(byte, bit) of one flip of the matrix in a record of L bytes, or None
    where the record has no such bit: tag bit i; the first ciphertext bit; the
    last one; bit 0 of the last byte of a partial block."""
    kind, which = flip
    if kind == "tag":
        return L + which // 8, which % 8
    if L == 0 or (which == "partial" and L % 16 == 0):
        return None
    return (0, 0) if which == "first" else (L - 1, 7 if which == "last" else 0)


def flip_rounds(lens, odd, checked):
    """The matrix as rounds of {record: (byte, bit)}: every flip that some
    checked record has a bit for lands in a record of `odd`, chosen by its
    length (the ciphertext flips first, they fit fewer records); the records
    between stay as crafted."""
    pending = [f for f in reversed(FLIPS) if any(flip_at(f, lens[i]) for i in checked)]
    assert len(pending) >= 128, ("flips the checked records have a bit for", len(pending))
    n_flips, rounds = len(pending), []
    while pending:
        flipped = {}
        for i in odd:
            f = next((f for f in pending if flip_at(f, lens[i])), None)
            if f is not None:
                pending.remove(f)
                flipped[i] = flip_at(f, lens[i])
        assert flipped, ("no flipped record has a bit for", pending)
        rounds.append(flipped)
    assert sum(len(r) for r in rounds) == n_flips, ("flips placed", sum(len(r) for r in rounds), "of", n_flips)
    return rounds


def check_family(recs, run, ct_offs, pt_offs, ip_offs, sizes, rej, checked=None, what=""):
    """(a)-(c) of tests/test_gpu_edge_values.py's docstring over the records
    `checked` (default: all).  run(open_, inplace, buf, init) -> (out, status): one launch over a
    host image of the input (records at ct_offs for an open, pt_offs for a
    seal, ip_offs in place) whose out-of-place output starts filled with init.
    sizes = (bytes of a CT-side image, of a PT-side one, of an in-place one)."""
    checked = list(range(len(recs))) if checked is None else checked
    lens = [len(r["pt"]) for r in recs]
    ct_total, pt_total, ip_total = sizes

    def opened(out, st, offs, flipped, given, init, inplace):
        for i in checked:
            o, L, lab = int(offs[i]), lens[i], (what, i, lens[i], recs[i]["label"], flipped.get(i))
            if i in flipped:
                assert st[i] == 1, ("flipped record accepted",) + lab
                if inplace:
                    assert bytes(out[o:o + L + 16]) == bytes(given[o:o + L + 16]), ("rejected in place",) + lab
                else:
                    assert np.all(out[o:o + L] == init), ("rejected output",) + lab
            else:
                assert st[i] == 0, ("crafted record rejected",) + lab
                assert bytes(out[o:o + L]) == recs[i]["pt"], ("plaintext",) + lab

    def sealed(out, offs):
        for i in checked:
            o, L = int(offs[i]), lens[i]
            assert bytes(out[o:o + L + 16]) == recs[i]["sealed"], (what, "seal", i, L, recs[i]["label"])

    for inplace in (False, True):
        c_offs, p_offs = (ip_offs, ip_offs) if inplace else (ct_offs, pt_offs)
        c_total, p_total = (ip_total, ip_total) if inplace else (ct_total, pt_total)
        fill = rejected_fill(*rej)
        ct_img = E.layout(recs, "sealed", c_offs, c_total, 0x11)
        out, st = run(True, inplace, ct_img, 0x5A)                                   # (a)
        opened(out, st, p_offs if not inplace else c_offs, {}, ct_img, 0x5A, inplace)
        out, _ = run(False, inplace, E.layout(recs, "pt", c_offs if inplace else p_offs, p_total, 0x22), 0xA5)
        sealed(out, c_offs)                                                          # (b)
        if not inplace and len(checked) == len(recs):  # and not a byte outside the records
            assert np.array_equal(out[:c_total], E.layout(recs, "sealed", c_offs, c_total, 0xA5)), (what, "stray")
        odd = checked[1::2]                                                          # (c)
        for flipped in flip_rounds(lens, odd, checked):
            img = ct_img.copy()
            for i, (byte, bit) in flipped.items():
                img[int(c_offs[i]) + byte] ^= 1 << bit
            init = 0x5A if fill else 0xC3  # a fill of 0 must differ from the buffer's own start
            out, st = run(True, inplace, img, init)
            opened(out, st, p_offs if not inplace else c_offs, flipped, img, init if fill else 0, inplace)


def crafted_ragged(aead, cipher, recs, fast):
    """Crafted records (and unchecked filler), each with a context of its own,
    in slots of one buffer: 64-B aligned ones readable to roundup64(len) with
    room for the tag (FAST) or packed at odd offsets.  (the slots' offsets, the
    buffer's size, prepare() of the keys, the descriptors and the AD on the device)"""
    n = len(recs)
    lens = np.array([len(r["pt"]) for r in recs], dtype=np.int64)
    slots = np.array([ru(max(int(L), 1) + 16, 64) + 64 if fast else int(L) + 16 + 5 for L in lens])
    offs = np.zeros(n, dtype=np.int64)
    offs[1:] = np.cumsum(slots)[:-1]
    assert not fast or not (offs % 64).any(), "FAST: the caller guarantees 16-byte aligned records"
    keys = np.frombuffer(b"".join(r["key"] for r in recs), dtype=np.uint8).reshape(n, 32).copy()
    d = np.zeros(n, dtype=REC_DT)
    d["in_off"] = d["out_off"] = offs
    d["nonce"] = np.array([r["nonce"] for r in recs], dtype=np.uint64)
    d["ctx_off"] = np.arange(n, dtype=np.uint64) * aead.dev_ctx_bytes(cipher)
    d["ad_off"] = np.arange(n, dtype=np.uint64) * 64
    d["len"] = lens
    d["ad_len"] = [len(r["ad"]) for r in recs]
    d_ad = dev(E.layout(recs, "ad", [64 * i for i in range(n)], 64 * n + 64))
    return offs, int(offs[-1] + slots[-1]) + 256, prepare(aead, cipher, keys), dev(d.view(np.uint8)), d_ad


def _filler(n, seed):
    """n records of at most 64 bytes: random plaintext, random CT || tag (an
    open rejects them; nothing of theirs is checked)."""
    rng = np.random.default_rng(seed)
    out = []
    for L in rng.integers(0, 65, n):
        blob = rng.integers(0, 256, int(L) + 16 + 32 + 8, dtype=np.uint8).tobytes()
        out.append(dict(pt=blob[:L], sealed=blob[:L + 16], key=blob[-40:-8], ad=b"",
                        nonce=int.from_bytes(blob[-8:], "little") >> 1, label=None))
    return out


# ------------------------------------------------------ the resident worker

# hand-picked lengths: one unit, unit boundaries, 63 units (4032 B), the
# 256-block Poly limit with a 256-byte AD (3824 B), then some of the multi-pass
# path (worker_chacha_multi) up to the 65519-byte maximum.  They are a sample,
# not the paths' cases: tests/length_classes.py derives those (wfast, wmulti,
# wtransport) and tests/test_gpu_worker.py's test_worker_length_classes_* run them;
# tests/test_length_classes_host.py counts what this list reaches of them
WORKER_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 1023, 1024, 1025, 1400,
               2047, 2048, 3823, 3824, 3825, 4031, 4032, 4033, 4096, 8000, 16384, 16385, 20000,
               40001, 65519]
WORKER_ADS = [0, 1, 16, 17, 32, 255, 256]


def worker_cases():
    rnd = random.Random(0x5EED)
    out = []
    for L in WORKER_LENS:
        for A in WORKER_ADS:
            if rnd.random() < 0.5 and L not in (0, 3824, 4032, 4033, 65519) and A not in (0, 256):
                continue  # a sample of the grid, the edges always
            out.append((L, A))
    return out
