"""Child process of test_gpu_aes_shapes.py (not collected by pytest): the
AES-GCM kernels that only an environment switch reaches, against the oracle.
NOISE_AEAD_GCM_SHAPE and NOISE_AEAD_GCM_DUPLEX are read once per process,
hence the child; the parent sets them.  Each launch is asked which kernel it
ran (noise_aead_debug_last_plan): gcm_ragged_staged in the forced shape,
gcm_duplex_staged where the duplex switch asks for it.

  aes_shapes_check.py ragged   the windowed ragged kernel in the forced shape
  aes_shapes_check.py duplex   the same, then the duplex of two uniform jobs
  aes_shapes_check.py classes  the ragged kernel over the (len, ad_len) list of
                               tests/length_classes.py for its lanes per record

Prints "ok N" (N records checked) and exits non-zero on the first mismatch.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "noise-c_amd"),
          os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import noise_aead as aead  # noqa: E402
import oracle as O  # noqa: E402
from aead_gpu import duplex_cases_check  # noqa: E402
from gpu_support import AES, FLAG_CT_GHASH, REC_DT, dev, prepare, stream, sync  # noqa: E402

FIXED_LENS = [0, 15, 16, 17, 1400, 4096]
AD_SLOT = 32
# NOISE_AEAD_GCM_SHAPE: threads per workgroup, records per group, lanes per record
SHAPES = {"w1024r1": "1024,%s,1,4", "w1024r2": "1024,%s,2,4", "w1024r2k8": "1024,%s,2,8"}


def ran_forced_shape(open_, fast, ct):
    tf = {False: "false", True: "true"}
    shape = SHAPES[os.environ["NOISE_AEAD_GCM_SHAPE"]] % tf[bool(ct)]
    want = "gcm_ragged_staged<%s,%s,%s>" % (tf[open_], tf[bool(fast)], shape)
    assert aead.last_plan().split()[0] == want, (aead.last_plan(), want)


def drawn_lengths(rng, count):
    """lengths 0..600 with each of FIXED_LENS at 11 places (all window
    positions), AD of 1, 16, 21 or 32 bytes on every third record"""
    lens = rng.integers(0, 601, count)
    for j, L in enumerate(FIXED_LENS):
        lens[7 * j + 5::101] = L
    adls = np.where(np.arange(count) % 3 == 0, rng.choice([1, 16, 21, 32], count), 0)
    return lens, adls


def ragged(orc, fast, ct, pairs=None):
    """lanes_per_record = 4 (off gcm_wide; the forced shape decides the lanes
    that run).  Without pairs: 1100 records of drawn_lengths(): 256-record
    windows with a partial last one (512 at w1024r2).  With pairs: one record
    per (len, ad_len), AD slots of 64 bytes.  Per-state runs of 1..300 records,
    so windows hold one, two and three or more states (both LDS slots and the
    global-context path)."""
    rng = np.random.default_rng(9001 + 2 * fast + ct)
    count = len(pairs) if pairs else 1100
    ad_slot = 64 if pairs else AD_SLOT
    runs = []
    while sum(runs) < count:
        runs.append(int(rng.choice([1, 3, 40, 130, 300])))
    state_of = np.repeat(np.arange(len(runs)), runs)[:count]
    keys = rng.integers(0, 256, (len(runs), 32), dtype=np.uint8)
    ctx, _k = prepare(aead, AES, keys)
    cb = aead.dev_ctx_bytes(AES)
    if pairs:
        lens, adls = (np.array([p[i] for p in pairs], dtype=np.int64) for i in (0, 1))
    else:
        lens, adls = drawn_lengths(rng, count)
    slot = (lens + 16 + 63) // 64 * 64 if fast else lens + 16 + 5
    offs = np.zeros(count, dtype=np.int64)
    offs[1:] = np.cumsum(slot)[:-1]
    total = int(offs[-1] + slot[-1]) + 64
    pt = rng.integers(0, 256, total, dtype=np.uint8)
    ad = rng.integers(0, 256, count * ad_slot, dtype=np.uint8)
    nonces = rng.integers(0, 2**62, count, dtype=np.int64).astype(np.uint64)
    recs = np.zeros(count, dtype=REC_DT)
    recs["in_off"] = recs["out_off"] = offs
    recs["nonce"] = nonces
    recs["ctx_off"] = state_of.astype(np.uint64) * cb
    recs["ad_off"] = np.arange(count) * ad_slot
    recs["len"] = lens
    recs["ad_len"] = adls
    flags = (aead.FLAG_FAST if fast else 0) | (FLAG_CT_GHASH if ct else 0)
    d_recs, d_ad = dev(recs.view(np.uint8)), dev(ad)
    kw = dict(ctx_base=ctx.data_ptr(), recs=d_recs.data_ptr(), n_records=count,
              ad=d_ad.data_ptr(), flags=flags, lanes=4, stream=stream())
    what = "fast=%d ct=%d" % (fast, ct)

    # seal, out of place: every record is the oracle's, no byte between records written
    exp = np.full(total, 0xA5, dtype=np.uint8)
    for i in range(count):
        o, L = int(offs[i]), int(lens[i])
        a = bytes(ad[ad_slot * i: ad_slot * i + int(adls[i])])
        c = orc.encrypt(AES, bytes(keys[state_of[i]]), int(nonces[i]), bytes(pt[o:o + L]), a)
        exp[o:o + L + 16] = np.frombuffer(c, dtype=np.uint8)
    d_pt = dev(pt)
    d_ct = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    assert aead.dev_ragged(False, AES, inp=d_pt.data_ptr(), out=d_ct.data_ptr(), **kw) == 0
    ran_forced_shape(False, fast, ct)
    sync()
    sealed = d_ct.cpu().numpy()
    for i in range(count):
        o, L = int(offs[i]), int(lens[i])
        assert np.array_equal(sealed[o:o + L + 16], exp[o:o + L + 16]), (what, "seal", i, L)
    assert np.array_equal(sealed, exp), (what, "seal wrote between records")

    bad = np.arange(count) % 37 == 5
    tampered = sealed.copy()
    for i in np.nonzero(bad)[0]:
        tampered[int(offs[i]) + int(rng.integers(0, int(lens[i]) + 16))] ^= 0x40

    # open in place: a rejected record's bytes stay exactly as given
    exp_in = tampered.copy()
    # open out of place into 0x5A: a rejected record's output is never written
    exp_out = np.full(total, 0x5A, dtype=np.uint8)
    for i in np.nonzero(~bad)[0]:
        o, L = int(offs[i]), int(lens[i])
        exp_in[o:o + L] = exp_out[o:o + L] = pt[o:o + L]
    for in_place, want in ((True, exp_in), (False, exp_out)):
        d_in = dev(tampered)
        d_out = d_in if in_place else torch.full((total,), 0x5A, dtype=torch.uint8, device="cuda")
        d_st = torch.full((count,), 9, dtype=torch.uint8, device="cuda")
        assert aead.dev_ragged(True, AES, inp=d_in.data_ptr(), out=d_out.data_ptr(),
                               status=d_st.data_ptr(), **kw) == 0
        ran_forced_shape(True, fast, ct)
        sync()
        st, back = d_st.cpu().numpy(), d_out.cpu().numpy()
        assert np.array_equal(st, bad.astype(np.uint8)), (what, "status", in_place)
        for i in range(count):
            o, n = int(offs[i]), int(lens[i]) + 16
            assert np.array_equal(back[o:o + n], want[o:o + n]), (what, "open", in_place, i, bool(bad[i]))
        assert np.array_equal(back, want), (what, "open wrote between records", in_place)
    return 3 * count


DUPLEX_CASES = [((1400, 300, 256), (1401, 513, 256)), ((1, 256, 256), (4096, 256, 256))]


def duplex(orc, flags):
    """test_duplex_vs_oracle's check (128-B slots) on DUPLEX_CASES, written
    (len, records, records per state): unequal workgroup counts in both
    directions and a partial last workgroup."""
    duplex_cases_check(aead, orc, AES, DUPLEX_CASES, "slot128", 0, flags,
                       np.random.default_rng(3131 + flags))
    return sum(a[1] + b[1] for a, b in DUPLEX_CASES)


def main():
    if not os.path.exists(O.ORACLE_SO):
        O.build(ref=False)
    orc = O.Oracle()
    aead.lib()
    n = 0
    pairs = None
    if sys.argv[1:] == ["classes"]:
        import length_classes
        lanes = int(SHAPES[os.environ["NOISE_AEAD_GCM_SHAPE"]].rsplit(",", 1)[1])
        pairs = length_classes.full("gcm", lanes)
    for fast in (True, False):
        for ct in (False, True):
            n += ragged(orc, fast, ct, pairs)
    if sys.argv[1:] == ["duplex"]:
        for flags in (0, FLAG_CT_GHASH):
            n += duplex(orc, flags)
    print("ok", n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
