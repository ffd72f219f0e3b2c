"""GPU parity at the arithmetic edges: crafted records through every kernel family.

tests/edge_records.py builds records whose Poly1305 accumulator ends at 0, 1,
4, p - 1, ... (both sides of fe_finish's final subtraction), whose tag add
carries through every word or none, whose serial Horner prefix is 0 / 4 /
p - 1 before a block of sixteen 0xFF bytes, and whose GHASH inputs and final
values are 0, all ones or a single bit; nonce bases carry out of the low word
inside every state's run.  tests/test_edge_records_host.py pins those records
to the oracle (and the reference) on the CPU.  Here, for each kernel family:

(a) the crafted CT || tag opens: every status 0, the oracle's plaintext;
(b) that plaintext seals to the crafted CT || tag, byte for byte;
(c) the tag-bit matrix: each of the 128 tag bits flipped in a record of its
    own, then the first ciphertext bit, the last one and bit 0 of the last
    byte of a partial block; every flipped record is rejected with status 1
    and its output is the rejected fill (out of place) or the bytes as given
    (in place), every unflipped record between them is accepted.

Out of place and in place.  All comparisons are bit-exact.
"""
import ctypes as C

import numpy as np
import pytest

import edge_records as E
from aead_gpu import FLIPS, _filler, check_family, crafted_ragged, flip_at
from edge_records import AES, CHACHA
from gpu_support import FLAG_CT_GHASH, FLAG_FAST, FLAG_ONE_PASS, FLAG_VERIFY_FIRST, _torch, dev, prepare, ru, stream, sync

pytestmark = pytest.mark.gpu

AD_STRIDE = 48


# ------------------------------------------------------------------ uniform

def uniform_strides(kind, L):
    """(plaintext-side stride, CT-side stride, in-place stride)."""
    if kind == "packed":
        # packed; one byte of slack where packed strides would be 16-aligned
        # and so select the FAST kernels
        p = L + (L % 16 == 0)
        return p, p + 16, p + 16
    if kind == "seg":
        s = ru(max(L, 1), 64) + 64
        return s, s, s
    m = 128 if kind == "slot128" else 64
    return ru(max(L, 1), m), ru(L + 16, m), ru(L + 16, m)


class UniformJob:
    """One crafted batch on the device: its context, nonce bases and AD."""

    def __init__(self, aead, b, kind, lanes):
        self.aead, self.b, self.lanes = aead, b, lanes
        self.ps, self.cs, self.ips = uniform_strides(kind, b.L)
        self.ctx, self._k = prepare(aead, b.cipher, b.keys)
        self.d_nb = dev(b.nonce_base.view(np.int64))
        self.d_ad = dev(b.strided("ad", AD_STRIDE)) if b.ad_len else None
        n = b.count
        self.offs = ([i * self.cs for i in range(n)], [i * self.ps for i in range(n)],
                     [i * self.ips for i in range(n)])
        self.sizes = (n * self.cs + 64, n * self.ps + 64, n * self.ips + 64)

    def job(self, open_, inplace, buf, init, flags):
        torch = _torch()
        b = self.b
        ins = self.ips if inplace else (self.cs if open_ else self.ps)
        outs = self.ips if inplace else (self.ps if open_ else self.cs)
        d_in = dev(buf)
        d_out = d_in if inplace else torch.full((b.count * outs + 64,), init, dtype=torch.uint8, device="cuda")
        d_st = torch.full((b.count,), 7, dtype=torch.uint8, device="cuda")
        j = self.aead.uniform_job(ctx=self.ctx.data_ptr(), nonce_base=self.d_nb.data_ptr(), inp=d_in.data_ptr(),
                                  out=d_out.data_ptr(), in_stride=ins, out_stride=outs, length=b.L,
                                  n_records=b.count, recs_per_state=b.rps,
                                  status=d_st.data_ptr() if open_ else 0,
                                  ad=self.d_ad.data_ptr() if b.ad_len else 0,
                                  ad_stride=AD_STRIDE if b.ad_len else 0, ad_len=b.ad_len, lanes=self.lanes,
                                  flags=flags if open_ else flags & FLAG_CT_GHASH)
        return j, d_in, d_out, d_st

    def runner(self, flags):
        lib = self.aead.lib()

        def run(open_, inplace, buf, init):
            j, _d_in, d_out, d_st = self.job(open_, inplace, buf, init, flags)
            f = lib.noise_aead_dev_open_uniform if open_ else lib.noise_aead_dev_seal_uniform
            rc = f(self.b.cipher, C.byref(j), stream())
            assert rc == 0, hex(rc)
            sync()
            return d_out.cpu().numpy(), d_st.cpu().numpy()
        return run

    def check(self, flags, what):
        b = self.b
        check_family(b.records, self.runner(flags), *self.offs, self.sizes, (b.cipher, 0x5A, flags),
                     what=(what, b.L, b.ad_len))


@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32, 64])
def test_chacha_generic_uniform(aead, gpu, oracle, lanes):
    """chachapoly_{seal,open}_uniform<K, false>: unaligned strides, states of
    13 records straddling waves, default order and ONE_PASS (scrubbed)."""
    for shape in E.CHACHA_GENERIC:
        for flags in (0, FLAG_ONE_PASS):
            UniformJob(aead, E.shaped(oracle, shape), "packed", lanes).check(flags, ("generic", lanes, flags))


@pytest.mark.parametrize("lanes", [0, 1, 4, 8])
@pytest.mark.parametrize("oflags", [0, FLAG_ONE_PASS])
def test_chacha_staged_uniform_key(aead, gpu, oracle, lanes, oflags):
    """FAST layouts with a wave-uniform key: one state per 256 records, 300
    records (a partial last block), 64-B slots.  Lanes 1, 4 and 8 take the
    LDS-staged kernels; lanes 0 is the library's choice, which for a batch
    this small is 64 lanes: chachapoly_{seal,open}_uniform<64, true>."""
    for shape in E.CHACHA_STAGED:
        UniformJob(aead, E.shaped(oracle, shape), "fast", lanes).check(oflags, ("staged", lanes, oflags))


@pytest.mark.parametrize("lanes", [4, 8])
@pytest.mark.parametrize("oflags", [0, FLAG_ONE_PASS])
def test_chacha_staged_record_key(aead, gpu, oracle, lanes, oflags):
    """The staged FAST kernels with a key per record (13 records per state)."""
    for shape in E.CHACHA_GENERIC:
        UniformJob(aead, E.shaped(oracle, shape), "fast", lanes).check(oflags, ("staged-rk", lanes, oflags))


@pytest.mark.parametrize("shape", E.CHACHA_SEG2, ids=lambda s: "n%d-rps%d-L%d" % s[1:4])
def test_chacha_seg2_uniform(aead, gpu, oracle, shape):
    """chachapoly_seg2_uniform: two segments per record joined by r^e."""
    for flags in (FLAG_VERIFY_FIRST, FLAG_ONE_PASS):
        UniformJob(aead, E.shaped(oracle, shape), "seg", 2).check(flags, ("seg2", flags))


@pytest.mark.parametrize("rps", [13, 256])
@pytest.mark.parametrize("ct", [0, FLAG_CT_GHASH])
def test_aes_uniform(aead, gpu, oracle, rps, ct):
    """gcm_uniform (13 records per state, unaligned) and gcm_staged (one state
    per 256 records, FAST), 4-bit tables and the constant-time GHASH."""
    for shape in E.AES_UNIFORM:
        if shape[2] == rps:
            UniformJob(aead, E.shaped(oracle, shape), "fast" if rps == 256 else "packed", 0).check(
                ct, ("aes", rps, ct))


# ------------------------------------------------------------------- duplex

def duplex_check(aead, oracle, cipher, shape_x, shape_y, kind, lanes, flags):
    """Batch X through (a)-(c) as one job of noise_aead_dev_duplex_uniform
    while the other job of the same call is crafted batch Y (sealed when X is
    opened, opened when X is sealed), checked on every call."""
    X = UniformJob(aead, E.shaped(oracle, shape_x), kind, lanes)
    Y = UniformJob(aead, E.shaped(oracle, shape_y), kind, lanes)
    y = Y.b
    y_pt = E.layout(y.records, "pt", Y.offs[1], Y.sizes[1], 0x22)
    y_ct = E.layout(y.records, "sealed", Y.offs[0], Y.sizes[0], 0x11)

    def run(open_, inplace, buf, init):
        jx, _xi, x_out, x_st = X.job(open_, inplace, buf, init, flags)
        jy, _yi, y_out, y_st = Y.job(not open_, False, y_pt if open_ else y_ct, 0x77, flags)
        sj, oj = (jy, jx) if open_ else (jx, jy)
        rc = aead.dev_duplex(cipher, sj, oj, stream())
        assert rc == 0, hex(rc)
        sync()
        got = y_out.cpu().numpy()
        if open_:  # Y was sealed beside the open of X
            for i, r in enumerate(y.records):
                o = Y.offs[0][i]
                assert bytes(got[o:o + y.L + 16]) == r["sealed"], ("duplex partner seal", i, r["label"])
        else:
            assert not y_st.cpu().numpy().any()
            for i, r in enumerate(y.records):
                o = Y.offs[1][i]
                assert bytes(got[o:o + y.L]) == r["pt"], ("duplex partner open", i, r["label"])
        return x_out.cpu().numpy(), x_st.cpu().numpy()

    check_family(X.b.records, run, *X.offs, X.sizes, (cipher, 0x5A, flags), what=("duplex", kind, lanes, flags))


@pytest.mark.parametrize("lanes", [4, 8])
def test_duplex_chacha_staged(aead, gpu, oracle, lanes):
    """chachapoly_duplex_staged<4>, <8>: both jobs FAST, one state per 256
    records, one-pass open."""
    a, b = (CHACHA, 300, 256, 1400, 0), (CHACHA, 300, 256, 100, 32)
    duplex_check(aead, oracle, CHACHA, a, b, "fast", lanes, FLAG_ONE_PASS)
    duplex_check(aead, oracle, CHACHA, b, a, "fast", lanes, FLAG_ONE_PASS)


@pytest.mark.parametrize("flags", [FLAG_ONE_PASS, 0])
def test_duplex_chacha_solo(aead, gpu, oracle, flags):
    """chachapoly_duplex_solo: one lane per record, 128-B slots, about 600
    records a side, one-pass and verify-first open."""
    a, b = E.CHACHA_SOLO
    duplex_check(aead, oracle, CHACHA, a, b, "slot128", 1, flags)
    duplex_check(aead, oracle, CHACHA, b, a, "slot128", 1, flags)


@pytest.mark.parametrize("ct", [0, FLAG_CT_GHASH])
def test_duplex_aes(aead, gpu, oracle, ct):
    """gcm_duplex_fused, tables and constant-time GHASH."""
    a, b = (AES, 300, 256, 1400, 0), (AES, 300, 256, 100, 21)
    duplex_check(aead, oracle, AES, a, b, "slot128", 0, ct)
    duplex_check(aead, oracle, AES, b, a, "slot128", 0, ct)


# ------------------------------------------------------------------- ragged

def ragged_check(aead, cipher, recs, checked, fast, lanes, flags, what):
    """recs: crafted records (and unchecked filler), each with a context of
    its own, in slots of one buffer: 64-B aligned ones readable to
    roundup64(len) with room for the tag (FAST) or packed at odd offsets."""
    torch, n = _torch(), len(recs)
    offs, total, (ctx, _k), d_recs, d_ad = crafted_ragged(aead, cipher, recs, fast)
    seal_flags = (FLAG_FAST if fast else 0) | (flags & FLAG_CT_GHASH)

    def run(open_, inplace, buf, init):
        d_in = dev(buf)
        d_out = d_in if inplace else torch.full((total,), init, dtype=torch.uint8, device="cuda")
        d_st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        rc = aead.dev_ragged(open_, cipher, ctx_base=ctx.data_ptr(), recs=d_recs.data_ptr(), inp=d_in.data_ptr(),
                             out=d_out.data_ptr(), n_records=n, ad=d_ad.data_ptr(), status=d_st.data_ptr(),
                             lanes=lanes, flags=(FLAG_FAST if fast else 0) | flags if open_ else seal_flags,
                             stream=stream())
        assert rc == 0, hex(rc)
        sync()
        return d_out.cpu().numpy(), d_st.cpu().numpy()

    check_family(recs, run, offs, offs, offs, (total, total, total), (cipher, 0x5A, flags), checked=checked,
                 what=what)


@pytest.mark.parametrize("lanes", [0, 1, 4, 8, 16, 64])
@pytest.mark.parametrize("fast", [True, False])
def test_ragged_chacha(aead, gpu, oracle, lanes, fast):
    """chachapoly_{seal,open}_ragged<K, FAST>: records with a key and a nonce
    of their own, single-block and AD-only (L = 0) records among them.  Lanes
    0 is the library's choice, 64 lanes for a batch this small (the same
    kernel as lanes 64, reached through the default)."""
    b = E.ragged_shaped(oracle, "chacha")
    for flags in (0, FLAG_ONE_PASS):
        ragged_check(aead, CHACHA, b.records, None, fast, lanes, flags, ("ragged", lanes, fast, flags))


@pytest.mark.parametrize("flags", [0, FLAG_ONE_PASS])
def test_ragged_chacha_segmented(aead, gpu, oracle, flags):
    """chachapoly_seg_ragged (FAST batches of 16 384 records or more with
    automatic lanes): crafted records of 1400 B - 65519 B, every segment count
    and every target at each length, spread among 16 400 unchecked filler
    records of at most 64 B."""
    crafted = E.ragged_shaped(oracle, "seg").records
    recs = _filler(16400, 31)
    step = len(recs) // len(crafted)
    checked = []
    for k, r in enumerate(crafted):
        checked.append(k * (step + 1) + 7)
        recs.insert(checked[-1], r)
    assert len(recs) >= 16384 and all(recs[i] is c for i, c in zip(checked, crafted))
    ragged_check(aead, CHACHA, recs, checked, True, 0, flags, ("seg-ragged", flags))


@pytest.mark.parametrize("lanes", [0, 4])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("ct", [0, FLAG_CT_GHASH])
def test_ragged_aes(aead, gpu, oracle, lanes, fast, ct):
    """gcm_wide (lanes 0: a workgroup per record) and gcm_ragged_staged."""
    b = E.ragged_shaped(oracle, "aes")
    ragged_check(aead, AES, b.records, None, fast, lanes, ct, ("ragged-aes", lanes, fast, ct))


# -------------------------------------------------------- resident worker

@pytest.mark.parametrize("name", ["worker_chacha", "worker_aes"])
def test_worker_crafted_records(aead, gpu, oracle, name):
    """The CipherState API (resident worker): ChaChaPoly fast path (16, 1400,
    4032 B), multi-pass path (4033, 16384 B), AES-GCM gcm_wide_record."""
    b = E.ragged_shaped(oracle, name)
    _, st = aead.CipherState.new_by_id(b.cipher)
    for i, r in enumerate(b.records):
        lab = (name, i, len(r["pt"]), r["label"])
        assert st.init_key(r["key"]) == 0 and (r["nonce"] == 0 or st.set_nonce(r["nonce"]) == 0)
        rc, pt = st.open(r["sealed"], r["ad"])
        assert rc == 0 and pt == r["pt"], ("open",) + lab
        assert st.nonce == r["nonce"] + 1
        assert st.init_key(r["key"]) == 0 and (r["nonce"] == 0 or st.set_nonce(r["nonce"]) == 0)
        assert st.seal(r["pt"], r["ad"]) == r["sealed"], ("seal",) + lab
    st.free()


@pytest.mark.parametrize("name", ["worker_matrix", "worker_matrix_aes"])
def test_worker_tag_bit_matrix(aead, gpu, oracle, name):
    """128 opens of a crafted 64-byte record, one tag bit flipped in each:
    MAC failure, the buffer as given, the nonce where it was; then the
    record itself is accepted."""
    b = E.ragged_shaped(oracle, name)
    r = b.records[0]
    _, st = aead.CipherState.new_by_id(b.cipher)
    assert st.init_key(r["key"]) == 0 and st.set_nonce(r["nonce"]) == 0
    for byte, bit in filter(None, (flip_at(f, 64) for f in FLIPS)):
        bad = bytearray(r["sealed"])
        bad[byte] ^= 1 << bit
        rc, back = st.open(bytes(bad), r["ad"])
        assert rc == aead.ERROR_MAC_FAILURE and back == bytes(bad), (name, byte, bit)
        assert st.nonce == r["nonce"], (name, byte, bit)
    rc, pt = st.open(r["sealed"], r["ad"])
    assert rc == 0 and pt == r["pt"] and st.nonce == r["nonce"] + 1
    st.free()
