"""Record lengths swept through every AEAD kernel's lane and step geometry.

tests/length_classes.py restates each kernel family's partition arithmetic and
derives, per family, one length for every geometric case a record's length
can put it in (which lane starts the chain, absorbs the AD or holds the tail;
the tail's Poly1305 blocks; the power of r or H each lane is scaled by; the
tree levels and jumps that run).  Here each kernel runs those lists against
the CPU oracle: every sealed byte with its tag, every status, every verified
plaintext, every rejected record's bytes (out of place: untouched, or zeroed
by a NOISE_AEAD_FLAG_ONE_PASS ChaChaPoly open; in place: exactly as given),
and the bytes between records.  One record in eight of every open is
tampered, the last ciphertext byte and the first tag byte in turn.  Every
launch is asked which kernel it ran (noise_aead_debug_last_plan).  Each
ChaChaPoly length runs once without AD and once with 1, 16, 17 or 48 bytes of
it; the AES-GCM cases carry their AD length themselves.

The sweep_* functions take the length list as an argument, so the same
harness can be fed any other list.  Each case prints its wall time.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":  # the child process: what conftest.py does for pytest
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "noise-c_amd")]

import length_classes as C
from aead_gpu import duplex_kernel, oracle_seal_records, rejected_fill
from gpu_support import AES, CHACHA, FLAG_CT_GHASH, FLAG_ONE_PASS, REC_DT, _torch, dev, prepare, ru, stream, sync

pytestmark = pytest.mark.gpu

TF = {False: "false", True: "true"}
HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "aes_shapes_check.py")


@pytest.fixture(autouse=True)
def wall_time(request):
    t = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - t))


def tamper(ct, offs, lens, bad):
    """one flipped bit in each bad record: the last CT byte and the first tag
    byte in turn (a record of no bytes: the tag)"""
    for n, i in enumerate(np.nonzero(bad)[0]):
        o, L = int(offs[i]), int(lens[i])
        ct[o + (L - 1 if n % 2 == 0 and L else L)] ^= 0x01


def differing(got, want, offs, sizes, pairs, case):
    """the (len, ad_len, case) of the records whose bytes differ"""
    out = []
    for i, (o, n) in enumerate(zip(offs, sizes)):
        if not np.array_equal(got[o:o + n], want[o:o + n]):
            out.append((int(pairs[i][0]), int(pairs[i][1]), case(pairs[i]) if case else None))
    return out


def check_image(got, want, offs, sizes, pairs, case, what):
    if np.array_equal(got, want):
        return
    recs = differing(got, want, offs, sizes, pairs, case)
    assert not recs, "%s: %d records differ: %s" % (what, len(recs), recs[:12])
    assert False, "%s: bytes between records were written" % (what,)


# ------------------------------------------------------------ ragged batches

class RaggedBatch:
    """Every (len, ad_len) of `pairs` among `filler` 64-byte records, the
    descriptors permuted, on the host: descriptors, plaintext, AD, and what
    the oracle says of each pass.  FAST: 64-byte aligned slots with 64 canary
    bytes after the tag; else packed at odd offsets, odd records' input
    misaligned by 3 bytes.  The open's input `given` holds CT || tag where the
    seal read its plaintext, one record in eight tampered; `want_out` is the
    image of an out-of-place open into 0x5A, `want_in` of one in place."""

    def __init__(self, aead, oracle, cipher, pairs, fast, oflags=0, filler=0, seed=1):
        rng = np.random.default_rng(seed)
        pairs = list(pairs) + [(64, 0)] * filler
        if filler:
            pairs = [pairs[i] for i in rng.permutation(len(pairs))]
        self.pairs, self.n, self.cipher = pairs, len(pairs), cipher
        n = self.n
        self.lens = lens = np.array([p[0] for p in pairs], dtype=np.int64)
        S = 7
        self.keys = keys = rng.integers(0, 256, (S, 32), dtype=np.uint8)
        key_idx = rng.integers(0, S, n).astype(np.uint32)
        slots = ru(np.maximum(lens, 1) + 16, 64) + 64 if fast else lens + 16 + 5 + 3
        self.offs = offs = np.zeros(n, dtype=np.int64)
        offs[1:] = np.cumsum(slots)[:-1]
        self.total = total = int(offs[-1] + slots[-1]) + 64
        self.mis = mis = np.zeros(n, dtype=np.int64) if fast else 3 * (np.arange(n) % 2)
        self.recs = recs = np.zeros(n, dtype=REC_DT)
        recs["in_off"], recs["out_off"] = offs + mis, offs
        recs["nonce"] = rng.integers(0, 2**62, n, dtype=np.int64).astype(np.uint64)
        recs["ctx_off"] = key_idx.astype(np.uint64) * aead.dev_ctx_bytes(cipher)
        recs["ad_off"] = np.arange(n, dtype=np.uint64) * 64
        recs["len"], recs["ad_len"] = lens, [p[1] for p in pairs]
        self.irecs = recs.copy()  # the in-place open
        self.irecs["out_off"] = recs["in_off"]
        self.pt = pt = rng.integers(0, 256, total, dtype=np.uint8)
        self.ad = rng.integers(0, 256, n * 64 + 64, dtype=np.uint8)
        self.exp = exp = np.full(total, 0xA5, dtype=np.uint8)
        oracle.seal_ragged(cipher, np.ascontiguousarray(keys.reshape(-1)), key_idx, recs, pt, exp, self.ad)
        self.given = given = np.full(total, 0xA5, dtype=np.uint8)
        for i in range(n):
            o, L = int(offs[i]), int(lens[i]) + 16
            given[o + mis[i]:o + mis[i] + L] = exp[o:o + L]
        self.bad = bad = np.arange(n) % 8 == 3
        tamper(given, offs + mis, lens, bad)
        fill = rejected_fill(cipher, 0x5A, oflags)
        self.want_out = np.full(total, 0x5A, dtype=np.uint8)
        self.want_in = given.copy()
        for i in range(n):
            o, L, m = int(offs[i]), int(lens[i]), int(mis[i])
            if bad[i]:
                self.want_out[o:o + L] = fill
            else:
                self.want_out[o:o + L] = self.want_in[o + m:o + m + L] = pt[o + m:o + m + L]

    def job(self, aead, open_, inplace, lanes, flags):
        """Fresh device buffers for one pass: (NoiseAeadRagged, output, statuses, keep-alive)."""
        torch = _torch()
        ctx, k = prepare(aead, self.cipher, self.keys)
        recs = (self.irecs if inplace else self.recs) if open_ else self.recs
        d_recs, d_ad, d_in = dev(recs.view(np.uint8)), dev(self.ad), dev(self.given if open_ else self.pt)
        d_out = d_in if open_ and inplace else torch.full((self.total,), 0x5A if open_ else 0xA5, dtype=torch.uint8,
                                                          device="cuda")
        d_st = torch.full((self.n,), 9, dtype=torch.uint8, device="cuda")
        j = aead.ragged_job(ctx_base=ctx.data_ptr(), recs=d_recs.data_ptr(), inp=d_in.data_ptr(), out=d_out.data_ptr(),
                            n_records=self.n, status=d_st.data_ptr(), ad=d_ad.data_ptr(), lanes=lanes, flags=flags)
        return j, d_out, d_st, (ctx, k, d_recs, d_ad, d_in)

    def check(self, open_, inplace, out, st, case, what):
        """out, st: a pass's output image and statuses, on the host"""
        want_st = self.bad if open_ else np.zeros(self.n, dtype=bool)
        wrong = np.nonzero(st != want_st)[0]
        assert not len(wrong), "%s statuses: %s" % (what, [(self.pairs[i], int(st[i]), case(self.pairs[i]) if case else None)
                                                            for i in wrong[:12]])
        if not open_:
            check_image(out, self.exp, self.offs, self.lens + 16, self.pairs, case, what)
        elif inplace:
            check_image(out, self.want_in, self.offs + self.mis, self.lens + 16, self.pairs, case, what)
        else:
            check_image(out, self.want_out, self.offs, self.lens, self.pairs, case, what)


def run_ragged(aead, cipher, open_, j):
    rc = aead.dev_ragged(open_, cipher, ctx_base=j.ctx_base, recs=j.recs, inp=j.in_, out=j.out, n_records=j.n_records,
                         status=j.status, ad=j.ad, lanes=j.lanes_per_record, flags=j.flags, stream=stream())
    assert rc == 0, hex(rc)
    return aead.last_plan().split()


def sweep_ragged(aead, oracle, cipher, pairs, *, lanes, fast, flags=0, oflags=0, want, case=None,
                 filler=0, seed=1):
    """One seal launch and two open launches (out of place into 0x5A, in
    place) over a RaggedBatch of `pairs`.  want: (seal kernel, open kernel)
    as plan_print names them."""
    B = RaggedBatch(aead, oracle, cipher, pairs, fast, oflags, filler, seed)
    flags |= aead.FLAG_FAST if fast else 0
    for open_, inplace in ((False, False), (True, False), (True, True)):
        j, d_out, d_st, _keep = B.job(aead, open_, inplace, lanes, flags | (oflags if open_ else 0))
        plan = run_ragged(aead, cipher, open_, j)
        assert plan[0] == want[open_], plan
        if open_ and cipher == CHACHA:
            assert plan[-1] == "vf=%d" % (not oflags & FLAG_ONE_PASS), plan
        sync()
        B.check(open_, inplace, d_out.cpu().numpy(), d_st.cpu().numpy(), case,
                "%s %s in_place=%d" % ("open" if open_ else "seal", want[open_], inplace))
    return 3 * B.n


# ------------------------------------------------------------- uniform jobs

class UniformBatch:
    """`count` records of one (len, ad_len) on the host with what the oracle
    says of each pass, as RaggedBatch.  FAST: one stride of
    roundup64(len + 16) + 64 for both sides (canary bytes after every tag);
    else an odd stride of len + 21 or len + 22."""

    def __init__(self, oracle, cipher, rng, L, adl, rps, count, fast, oflags=0):
        self.cipher, self.L, self.adl, self.rps, self.count = cipher, L, adl, rps, count
        S = (count + rps - 1) // rps
        self.stride = stride = ru(max(L, 1) + 16, 64) + 64 if fast else (L + 16 + 5) | 1
        self.keys = rng.integers(0, 256, (S, 32), dtype=np.uint8)
        self.nb = rng.integers(0, 2**62, S, dtype=np.uint64)
        self.pt = pt = rng.integers(0, 256, count * stride + 64, dtype=np.uint8)
        self.ad = rng.integers(0, 256, count * 48 + 64, dtype=np.uint8)
        akw = dict(ad=self.ad, ad_stride=48, ad_len=adl) if adl else {}
        self.exp = oracle_seal_records(oracle, cipher, self.keys, self.nb, rps, pt, stride, L, count, stride, **akw)
        self.given = self.exp.copy()
        self.bad = bad = np.arange(count) % 8 == 3
        tamper(self.given, np.arange(count, dtype=np.int64) * stride, np.full(count, L), bad)
        fill = rejected_fill(cipher, 0x5A, oflags)
        self.want_out = np.full(count * stride + 64, 0x5A, dtype=np.uint8)
        self.want_in = self.given.copy()
        for i in range(count):
            o = i * stride
            if bad[i]:
                self.want_out[o:o + L] = fill
            else:
                self.want_out[o:o + L] = self.want_in[o:o + L] = pt[o:o + L]

    def job(self, aead, open_, inplace, lanes, flags):
        """Fresh device buffers for one pass: (NoiseAeadUniform, output, statuses, keep-alive)."""
        torch = _torch()
        ctx, k = prepare(aead, self.cipher, self.keys)
        d_nb, d_ad = dev(self.nb.view(np.int64)), dev(self.ad)
        d_in = dev(self.given if open_ else self.pt)
        d_out = d_in if open_ and inplace else torch.full((len(self.exp),), 0x5A if open_ else 0xA5, dtype=torch.uint8,
                                                          device="cuda")
        d_st = torch.full((self.count,), 7, dtype=torch.uint8, device="cuda")
        j = aead.uniform_job(ctx=ctx.data_ptr(), nonce_base=d_nb.data_ptr(), inp=d_in.data_ptr(), out=d_out.data_ptr(),
                             in_stride=self.stride, out_stride=self.stride, length=self.L, n_records=self.count,
                             recs_per_state=self.rps, status=d_st.data_ptr() if open_ else 0,
                             ad=d_ad.data_ptr() if self.adl else 0, ad_stride=48 if self.adl else 0, ad_len=self.adl,
                             lanes=lanes, flags=flags)
        return j, d_out, d_st, (ctx, k, d_nb, d_ad, d_in)

    def check(self, open_, inplace, out, st, what):
        if open_:
            assert np.array_equal(st != 0, self.bad) and st.max() <= 1, what + ": statuses"
        assert np.array_equal(out, self.want_in if inplace else (self.want_out if open_ else self.exp)), what


def sweep_uniform(aead, oracle, cipher, pairs, *, lanes, rps, count, fast, flags=0, oflags=0, want, case=None,
                  seed=2):
    """One seal launch and two open launches (out of place, in place) per
    (len, ad_len) of `pairs`, a UniformBatch of `count` records each."""
    import ctypes
    rng = np.random.default_rng(seed)
    for L, adl in pairs:
        B = UniformBatch(oracle, cipher, rng, L, adl, rps, count, fast, oflags)
        for open_, inplace in ((False, False), (True, False), (True, True)):
            what = "%s %s in_place=%d len=%d ad=%d case=%s" % ("open" if open_ else "seal", want[open_], inplace, L, adl,
                                                              case((L, adl)) if case else None)
            j, d_out, d_st, _keep = B.job(aead, open_, inplace, lanes, flags | (oflags if open_ else 0))
            f = aead.lib().noise_aead_dev_open_uniform if open_ else aead.lib().noise_aead_dev_seal_uniform
            assert f(cipher, ctypes.byref(j), stream()) == 0
            plan = aead.last_plan().split()
            assert plan[0] == want[open_], plan
            if open_ and cipher == CHACHA:
                assert plan[-1] == "vf=%d" % (not oflags & FLAG_ONE_PASS), plan
            sync()
            B.check(open_, inplace, d_out.cpu().numpy(), d_st.cpu().numpy(), what)
    return 3 * count * len(pairs)


def il_case(K):
    return lambda p: C.il(K, p[0])


# ----------------------------------- 1. windowed ragged ChaChaPoly, every K

def ragged_il_names(K, fast, oflags):
    vf = fast and not oflags & FLAG_ONE_PASS  # dispatch.h plan_ragged: vf_order
    return ("chachapoly_seal_ragged<%d,%s>" % (K, TF[fast]),
            "chachapoly_open_ragged<%d,%s,%s>" % (K, TF[fast], TF[vf]))


@pytest.mark.parametrize("K,fast,oflags", [(K, f, 0) for K in C.IL_LANES for f in (True, False)] +
                         [(4, True, FLAG_ONE_PASS), (8, True, FLAG_ONE_PASS)])
def test_ragged_windowed(aead, gpu, oracle, K, fast, oflags):
    """chachapoly_{seal,open}_ragged<K, FAST[, VF]>: the whole `full` list of
    the K-lane group, 24 K - 7 cases, with and without AD, in one launch."""
    sweep_ragged(aead, oracle, CHACHA, C.with_ad(C.full("il", K)), lanes=K, fast=fast, oflags=oflags,
                 want=ragged_il_names(K, fast, oflags), case=il_case(K), seed=100 + K + fast)


# -------------------------------- 2. uniform ChaChaPoly, a launch per length

def uniform_il_names(K, fast, ukey, oflags):
    if not fast or K > 8:
        return tuple("chachapoly_%s_uniform<%d,%s>" % (so, K, TF[fast]) for so in ("seal", "open"))
    seal = "chachapoly_seal_staged<%d,%s>" % (K, TF[ukey])
    if oflags & FLAG_ONE_PASS:
        return seal, "chachapoly_open_staged<%d,%s>" % (K, TF[ukey])
    return seal, "chachapoly_open_staged_vf<%d,%s>" % (K, TF[ukey])


# K, FAST layout, one state per wave (UKEY), open flags
UNIFORM_IL = ([(K, True, False, 0) for K in (16, 32, 64)] + [(K, False, False, 0) for K in (4, 8)] +
              [(K, True, u, f) for K in (4, 8) for u in (False, True) for f in (FLAG_ONE_PASS, 0)])


@pytest.mark.parametrize("K,fast,ukey,oflags", UNIFORM_IL)
def test_uniform_interleaved(aead, gpu, oracle, K, fast, ukey, oflags):
    """The generic kernel at 16, 32 and 64 lanes and, packed, at 4 and 8; the
    staged kernels (one-pass and verify-first opens) at 4 and 8: the `reduced`
    list, 256 / K + 1 records a launch (a full workgroup and a record), states
    of 3 records straddling waves, or one state per wave."""
    rps = 64 // K if ukey else 3
    sweep_uniform(aead, oracle, CHACHA, C.with_ad(C.reduced(K)), lanes=K, rps=rps, count=256 // K + 1,
                  fast=fast, oflags=oflags, want=uniform_il_names(K, fast, ukey, oflags), case=il_case(K),
                  seed=200 + K + 2 * fast + ukey)


# ------------------------------------------------- 3. one lane, two segments

@pytest.mark.parametrize("count", [65, 130])
@pytest.mark.parametrize("oflags", [0, FLAG_ONE_PASS])
def test_uniform_solo(aead, gpu, oracle, count, oflags):
    """chachapoly_{seal,open}_solo: the 49 cases of the two-unit steps."""
    sweep_uniform(aead, oracle, CHACHA, C.with_ad(C.full("solo")), lanes=1, rps=13, count=count, fast=True,
                  oflags=oflags, want=("chachapoly_seal_solo<false,false>", "chachapoly_open_solo<false,false>"),
                  case=lambda p: C.solo(p[0]), seed=300 + count)


@pytest.mark.parametrize("oflags", [0, FLAG_ONE_PASS])
def test_uniform_seg2(aead, gpu, oracle, oflags):
    """chachapoly_seg2_uniform: the 73 cases of the two-segment split."""
    sweep_uniform(aead, oracle, CHACHA, C.with_ad(C.full("seg", 2)), lanes=2, rps=13, count=37, fast=True,
                  oflags=oflags, want=("chachapoly_seg2_uniform<false,false>", "chachapoly_seg2_uniform<true,false>"),
                  case=lambda p: C.seg(2, p[0]), seed=310)


# ------------------------------------------------------- 4. segmented ragged

@pytest.mark.parametrize("oflags", [0, FLAG_ONE_PASS])
def test_ragged_segmented(aead, gpu, oracle, oflags):
    """chachapoly_seg_ragged: the 185 cases of K = 1 .. 16 segments, with and
    without AD, among 16 384 64-byte records (the kernel's threshold)."""
    sweep_ragged(aead, oracle, CHACHA, C.with_ad(C.full("seg_ragged")), lanes=0, fast=True, oflags=oflags,
                 want=("chachapoly_seg_ragged<false>", "chachapoly_seg_ragged<true>"),
                 case=lambda p: C.seg_ragged(p[0]), filler=16384, seed=400)


# ---------------------------------------------------------------- 5. AES-GCM

def gcm_case(K):
    return lambda p: C.gcm(K, *p)


@pytest.mark.parametrize("rps,count", [(13, 65), (256, 257)])
def test_gcm_uniform(aead, gpu, oracle, rps, count):
    """gcm_uniform (states of 13 records) and gcm_staged (one state per 256):
    a launch per (len, ad_len) of the 99 four-lane cases."""
    k = "gcm_staged" if rps == 256 else "gcm_uniform"
    sweep_uniform(aead, oracle, AES, C.full("gcm", 4), lanes=0, rps=rps, count=count, fast=True,
                  want=(k + "<false,false>", k + "<true,false>"), case=gcm_case(4), seed=500 + rps)


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("ct", [False, True])
def test_gcm_ragged(aead, gpu, oracle, fast, ct):
    """gcm_ragged_staged at four lanes: the 99 cases in one launch."""
    want = tuple("gcm_ragged_staged<%s,%s,256,%s,1,4>" % (TF[o], TF[fast], TF[ct]) for o in (False, True))
    sweep_ragged(aead, oracle, AES, C.full("gcm", 4), lanes=4, fast=fast, flags=FLAG_CT_GHASH if ct else 0,
                 want=want, case=gcm_case(4), seed=510 + 2 * fast + ct)


@pytest.mark.parametrize("ct", [False, True])
def test_gcm_wide(aead, gpu, oracle, ct):
    """gcm_wide (a workgroup per record): the 207 eight-chain cases and the
    lengths 16 M and 16 M - 9 at M = EARLY - 1, EARLY, EARLY + 1, 255, 256,
    257 blocks (the open's early key stream, the seal's second round)."""
    pairs = C.full("gcm_wide", 0, ct)
    assert len(pairs) <= 512
    sweep_ragged(aead, oracle, AES, pairs, lanes=0, fast=True, flags=FLAG_CT_GHASH if ct else 0,
                 want=("gcm_wide<false,%s>" % TF[ct], "gcm_wide<true,%s>" % TF[ct]),
                 case=lambda p: C.gcm_wide(p[0], p[1], ct), seed=520 + ct)


def test_gcm_eight_lane_windows(gpu):
    """gcm_ragged_staged<.., 2, 8>, reached by NOISE_AEAD_GCM_SHAPE=w1024r2k8
    in a child process (tests/aes_shapes_check.py): the 207 eight-lane cases,
    FAST and not, table and constant-time GHASH."""
    env = dict(os.environ, NOISE_AEAD_GCM_SHAPE="w1024r2k8")
    env.pop("NOISE_AEAD_GCM_DUPLEX", None)
    r = subprocess.run([sys.executable, HELPER, "classes"], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.split() == ["ok", str(4 * 3 * len(C.full("gcm", 8)))]


# ----------------------------------------------------------------- 6. duplex

def sweep_duplex_uniform(aead, oracle, cipher, pairs, *, lanes, rps, count, oflags, seed=6):
    """noise_aead_dev_duplex_uniform, one call per i: the seal job takes
    pairs[i], the open job pairs[-1-i] (a UniformBatch each, FAST, out of
    place): the shared kernel test_gpu_parity.duplex_kernel names, and both
    whole output images and the statuses as the separate calls leave them —
    what sweep_uniform holds those to."""
    rng = np.random.default_rng(seed)
    pairs = list(pairs)
    for i, (sp, op) in enumerate(zip(pairs, pairs[::-1])):
        X = UniformBatch(oracle, cipher, rng, sp[0], sp[1], rps, count, True)
        Y = UniformBatch(oracle, cipher, rng, op[0], op[1], rps, count, True, oflags)
        jx, x_out, _xs, _kx = X.job(aead, False, False, lanes, 0)
        jy, y_out, y_st, _ky = Y.job(aead, True, False, lanes, oflags)
        assert aead.dev_duplex(cipher, jx, jy, stream()) == 0
        want = duplex_kernel(aead, cipher, lanes, "fast", oflags, ((sp[0], count, rps), (op[0], count, rps)))
        assert want and aead.last_plan().split()[0] == want, (aead.last_plan(), want)
        sync()
        X.check(False, False, x_out.cpu().numpy(), None, "duplex seal %s len=%d ad=%d" % (want, sp[0], sp[1]))
        Y.check(True, False, y_out.cpu().numpy(), y_st.cpu().numpy(), "duplex open %s len=%d ad=%d" % (want, op[0], op[1]))
    return 2 * count * len(pairs)


@pytest.mark.parametrize("cipher,lanes,oflags", [(CHACHA, 1, 0), (CHACHA, 1, FLAG_ONE_PASS), (CHACHA, 4, FLAG_ONE_PASS),
                                                 (CHACHA, 8, FLAG_ONE_PASS), (AES, 0, 0)])
def test_duplex_uniform(aead, gpu, oracle, cipher, lanes, oflags):
    """chachapoly_duplex_solo over the 49 one-lane lengths and
    chachapoly_duplex_staged<4|8> over the `reduced` lists, each with and
    without AD; gcm_duplex_fused over the 99 (len, ad_len) cases."""
    if cipher == AES:
        pairs, n, rps = C.full("gcm", 4), 257, 256
    elif lanes == 1:
        pairs, n, rps = C.with_ad(C.full("solo")), 65, 13
    else:
        pairs, n, rps = C.with_ad(C.reduced(lanes)), 256 // lanes + 1, 3
    sweep_duplex_uniform(aead, oracle, cipher, pairs, lanes=lanes, rps=rps, count=n, oflags=oflags, seed=600 + lanes)


# noise_aead_dev_duplex_ragged's shared launches.  All but the segmented one
# beside a one-pass open are off by default (dispatch.h ragged_duplex_default)
# and the switch is read once per process, so the cases run this file as a
# script in a child process with NOISE_AEAD_RAGGED_DUPLEX=1, as
# tests/test_gpu_duplex_ragged.py runs its own.
# name -> (the shared kernel, cipher, (len, ad_len) pairs, 64-byte filler records, lanes per record,
#          both jobs' flags, the open job's flags, the case of a pair)
DUPLEX_RAGGED = {
    "k4": ("chachapoly_duplex_ragged<4,true,true>", CHACHA, lambda: C.with_ad(C.full("il", 4)), 0, 4, 0, 0, il_case(4)),
    "k64": ("chachapoly_duplex_ragged<64,true,true>", CHACHA, lambda: C.with_ad(C.full("il", 64)), 0, 64, 0, 0,
            il_case(64)),
    "seg": ("chachapoly_seg_duplex", CHACHA, lambda: C.with_ad(C.full("seg_ragged")), 16384, 0, 0, 0,
            lambda p: C.seg_ragged(p[0])),
    "seg-one-pass": ("chachapoly_seg_duplex", CHACHA, lambda: C.with_ad(C.full("seg_ragged")), 16384, 0, 0, FLAG_ONE_PASS,
                     lambda p: C.seg_ragged(p[0])),
    "aes": ("gcm_duplex_ragged<true,256,false,1,4>", AES, lambda: C.full("gcm", 4), 0, 4, 0, 0, gcm_case(4)),
    "aes-ct": ("gcm_duplex_ragged<true,256,true,1,4>", AES, lambda: C.full("gcm", 4), 0, 4, FLAG_CT_GHASH, 0, gcm_case(4)),
}


def duplex_ragged_case(aead, oracle, name):
    """The batch of the standalone sweep (item 1, item 4, the AES ragged one)
    as the seal job and, with other keys and bytes, as the open job of one
    call, in buffers of their own, the open out of place and then in place:
    the shared kernel's name; both whole output images and both status arrays
    equal to the two separate calls' on fresh buffers, and to the oracle's."""
    torch = _torch()
    expect, cipher, pairs, filler, lanes, flags, oflags, case = DUPLEX_RAGGED[name]
    seed = 700 + 2 * sorted(DUPLEX_RAGGED).index(name)
    X = RaggedBatch(aead, oracle, cipher, pairs(), True, 0, filler, seed)
    Y = RaggedBatch(aead, oracle, cipher, pairs(), True, oflags, filler, seed + 1)
    flags |= aead.FLAG_FAST
    for inplace in (False, True):
        jx, x_out, x_st, _kx = X.job(aead, False, False, lanes, flags)
        jy, y_out, y_st, _ky = Y.job(aead, True, inplace, lanes, flags | oflags)
        rc = aead.dev_duplex_ragged(cipher, jx, jy, stream())
        assert rc == 0, hex(rc)
        plan = aead.last_plan()
        assert plan.split()[0] == expect, (plan, expect)
        sync()
        sx, sx_out, sx_st, _ksx = X.job(aead, False, False, lanes, flags)
        sy, sy_out, sy_st, _ksy = Y.job(aead, True, inplace, lanes, flags | oflags)
        run_ragged(aead, cipher, False, sx)
        run_ragged(aead, cipher, True, sy)
        sync()
        assert torch.equal(x_out, sx_out) and torch.equal(x_st, sx_st), "duplex seal differs from the separate call"
        assert torch.equal(y_out, sy_out) and torch.equal(y_st, sy_st), "duplex open differs from the separate call"
        X.check(False, False, x_out.cpu().numpy(), x_st.cpu().numpy(), case, "duplex seal " + expect)
        Y.check(True, inplace, y_out.cpu().numpy(), y_st.cpu().numpy(), case, "duplex open %s in_place=%d" % (expect, inplace))
    return expect


def test_duplex_ragged(gpu):
    """Each case of DUPLEX_RAGGED (duplex_ragged_case) in one child process."""
    import json
    env = dict(os.environ, NOISE_AEAD_RAGGED_DUPLEX="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *DUPLEX_RAGGED], env=env, capture_output=True,
                       text=True, timeout=300)
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            got[d["case"]] = (d["ok"], d["detail"])
    for name, (ok, detail) in got.items():
        print(name, detail)
        assert ok, (name, detail)
    assert r.returncode == 0 and set(got) == set(DUPLEX_RAGGED), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def main(argv):
    """The child process: one line of JSON per case.  A failed comparison
    goes on to the next case; anything else (a HIP error among them) ends the
    process there, so nothing more starts on the GPU."""
    import json
    import noise_aead
    import oracle as O
    if not os.path.exists(O.ORACLE_SO):
        O.build(ref=False)
    orc = O.Oracle()
    for name in argv:
        t = time.perf_counter()
        try:
            detail, ok, stop = duplex_ragged_case(noise_aead, orc, name), True, False
        except AssertionError as e:  # its text goes to the parent
            detail, ok, stop = "AssertionError: %s" % str(e)[:1500], False, False
        except Exception as e:  # noqa: BLE001
            detail, ok, stop = "%s: %s" % (type(e).__name__, str(e)[:1500]), False, True
        print(json.dumps({"case": name, "ok": ok, "detail": "%s (%.2f s)" % (detail, time.perf_counter() - t)}),
              flush=True)
        if stop:
            return 3
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
