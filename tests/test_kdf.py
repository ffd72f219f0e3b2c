"""Session key fan-out: noise_aead_dev_hkdf / _split.

The device HKDF must equal the reference's noise_hashstate_hkdf
(hashstate.c:476-516) byte for byte: against the reference's own outputs
(tests/golden/hkdf.json, gen_hkdf.py) and against the oracle on a large
random batch for each of the four Noise hashes.  The split keys then drive
the transport ciphers: a record sealed under noise_aead_dev_split's k1 must
equal the oracle's seal under the oracle's split of the same ck.

The lengths: an HKDF written here with hashlib from hashstate.c's rules
(py_hkdf) pins the oracle's and the device's at every key length 1..256 (the
HMAC key path changes after the block length, 64 or 128) and every data length
0..256 (the padding of SHA-2's last block changes at 55/56 mod 64 and 111/112
mod 128, BLAKE2 holds back a last block that is full), three sessions per
launch so that keys + i * key_len runs at odd strides; and one and_hash job
whose record i is i bytes long puts the hashed length on every residue mod 128."""
import hashlib
import hmac
import json
import os

import numpy as np
import pytest

HASHES = [0x4801, 0x4802, 0x4803, 0x4804]
HLEN = {0x4801: 32, 0x4802: 64, 0x4803: 32, 0x4804: 64}


HASHLIB = {0x4801: hashlib.blake2s, 0x4802: hashlib.blake2b, 0x4803: hashlib.sha256, 0x4804: hashlib.sha512}
SESSIONS = 3


def py_hmac(hid, key, msg):
    """noise_hashstate_hmac (hashstate.c:406-449): a key longer than a block
    is hashed, the key is zero-padded to a block, ipad 0x36, opad 0x5c."""
    H = HASHLIB[hid]
    blen = H().block_size
    if len(key) > blen:
        key = H(key).digest()
    kb = key + bytes(blen - len(key))
    inner = H(bytes(x ^ 0x36 for x in kb) + msg).digest()
    return H(bytes(x ^ 0x5C for x in kb) + inner).digest()


def py_hkdf(hid, key, data, l1, l2):
    """noise_hashstate_hkdf (hashstate.c:476-516)"""
    temp = py_hmac(hid, key, data)
    o1 = py_hmac(hid, temp, b"\x01")
    o2 = py_hmac(hid, temp, o1 + b"\x02")
    return o1[:l1], o2[:l2]


def sweep_cases(hid):
    """[(key_len, data_len, out1_len, out2_len, keys, datas)] of the length
    sweep: every key length with data of 0, 1 and 32 bytes, then every data
    length under a key of hash_len bytes; SESSIONS distinct keys and data per
    case; the output lengths hash_len and hash_len - 1, in alternating order."""
    hl = HLEN[hid]
    pool = np.random.default_rng(hid).integers(0, 256, 8192, dtype=np.uint8).tobytes()
    lens = [(kl, dl) for kl in range(1, 257) for dl in (0, 1, 32)] + [(hl, dl) for dl in range(257)]
    cases = []
    for c, (kl, dl) in enumerate(lens):
        at, keys = [], []
        for i in range(SESSIONS):
            o = (c * 7 + i * 263) % 3000
            while pool[o:o + kl] in keys:  # a key of a byte or two can come twice
                o += 1
            at.append(o)
            keys.append(pool[o:o + kl])
        datas = [pool[4000 + o:4000 + o + dl] for o in at]
        cases.append((kl, dl, hl - c % 2, hl - 1 + c % 2, keys, datas))
    return cases


@pytest.mark.parametrize("hid", HASHES)
def test_oracle_hash_equals_hashlib(oracle, hid):
    msg = np.random.default_rng(hid + 1).integers(0, 256, 300, dtype=np.uint8).tobytes()
    assert HASHLIB[hid]().digest_size == HLEN[hid]
    for n in range(301):
        assert oracle.hash(hid, msg[:n]) == HASHLIB[hid](msg[:n]).digest(), n


@pytest.mark.parametrize("hid", HASHES)
def test_oracle_hkdf_equals_hashlib_at_every_length(oracle, hid):
    hl = HLEN[hid]
    cases = sweep_cases(hid)
    assert len(cases) == 256 * 3 + 257
    blen = HASHLIB[hid]().block_size
    assert {blen - 1, blen, blen + 1, 256} <= {c[0] for c in cases}
    for kl, dl, _, _, keys, datas in cases:
        for key, data in zip(keys, datas):
            assert len(key) == kl and len(data) == dl
            # a second witness of the HMAC written above
            assert py_hmac(hid, key, data) == hmac.new(key, data, HASHLIB[hid]).digest(), (kl, dl)
            for l1, l2 in ((hl, hl - 1), (hl - 1, hl)):
                assert oracle.hkdf(hid, key, data, l1, l2) == py_hkdf(hid, key, data, l1, l2), (kl, dl, l1, l2)


def test_dev_hkdf_argument_rules(aead):
    """Validation before any launch (no GPU work): hashstate.c:496-497."""
    A = aead
    assert A.dev_hkdf(0x4899, keys=8, key_len=32, n=1, out1=8, out1_len=32, out2=8,
                      out2_len=32) == A.ERROR_UNKNOWN_ID
    assert A.dev_hkdf(0x4803, keys=8, key_len=32, n=1, out1=8, out1_len=33, out2=8,
                      out2_len=32) == A.ERROR_INVALID_LENGTH
    assert A.dev_hkdf(0x4803, keys=0, key_len=32, n=1, out1=8, out1_len=32, out2=8,
                      out2_len=32) == A.ERROR_INVALID_PARAM
    assert A.dev_hkdf(0x4803, keys=8, key_len=32, data=0, data_len=5, n=1, out1=8,
                      out1_len=32, out2=8, out2_len=32) == A.ERROR_INVALID_PARAM
    assert A.dev_hkdf(0x4804, keys=8, key_len=300, n=1, out1=8, out1_len=32, out2=8,
                      out2_len=32) == A.ERROR_INVALID_LENGTH
    assert A.dev_hkdf(0x4804, keys=8, key_len=64, n=0, out1=8, out1_len=32, out2=8,
                      out2_len=32) == A.ERROR_NONE


def _run_hkdf(A, torch, hid, keys, data, l1, l2):
    n, kl = keys.shape
    dl = data.shape[1] if data is not None else 0
    d_keys = torch.from_numpy(keys.reshape(-1).copy()).cuda()
    d_data = torch.from_numpy(data.reshape(-1).copy()).cuda() if dl else None
    o1 = torch.zeros(n * max(l1, 1), dtype=torch.uint8, device="cuda")
    o2 = torch.zeros(n * max(l2, 1), dtype=torch.uint8, device="cuda")
    assert A.dev_hkdf(hid, keys=d_keys.data_ptr(), key_len=kl,
                      data=d_data.data_ptr() if dl else 0, data_len=dl, n=n,
                      out1=o1.data_ptr(), out1_len=l1, out2=o2.data_ptr(), out2_len=l2,
                      stream=torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return o1.cpu().numpy()[:n * l1].reshape(n, l1), o2.cpu().numpy()[:n * l2].reshape(n, l2)


@pytest.mark.gpu
def test_dev_hkdf_reference_golden(aead, gpu):
    import torch
    with open(os.path.join(os.path.dirname(__file__), "golden", "hkdf.json")) as f:
        cases = json.load(f)["cases"]
    for c in cases:
        key = np.frombuffer(bytes.fromhex(c["key"]), dtype=np.uint8)[None, :]
        data = bytes.fromhex(c["data"])
        dat = np.frombuffer(data, dtype=np.uint8)[None, :] if data else None
        l1, l2 = len(c["out1"]) // 2, len(c["out2"]) // 2
        o1, o2 = _run_hkdf(aead, torch, c["hash_id"], key, dat, l1, l2)
        assert bytes(o1[0]).hex() == c["out1"] and bytes(o2[0]).hex() == c["out2"], c


@pytest.mark.gpu
@pytest.mark.parametrize("hid", HASHES)
def test_dev_hkdf_at_every_length(aead, gpu, hid):
    """The sweep of sweep_cases through noise_aead_dev_hkdf, one launch of
    SESSIONS sessions per case, all into one output arena of 0xC3 that is read
    back once: the outputs must be py_hkdf's and every byte between them must
    still be 0xC3."""
    import time
    import torch
    cases = sweep_cases(hid)
    inp, want, where = bytearray(), bytearray(), []
    for kl, dl, l1, l2, keys, datas in cases:
        k_off = len(inp)
        inp += b"".join(keys)
        d_off = len(inp)
        inp += b"".join(datas)
        outs = [py_hkdf(hid, k, d, l1, l2) for k, d in zip(keys, datas)]
        want += b"\xc3" * 8
        o1_off = len(want)
        want += b"".join(o[0] for o in outs) + b"\xc3" * 8
        o2_off = len(want)
        want += b"".join(o[1] for o in outs)
        where.append((k_off, d_off, o1_off, o2_off))
    want += b"\xc3" * 8
    d_in = torch.from_numpy(np.frombuffer(bytes(inp), dtype=np.uint8).copy()).cuda()
    d_out = torch.full((len(want),), 0xC3, dtype=torch.uint8, device="cuda")
    # a launch is three lanes of serial hashing: independent, so they go round
    # four streams and overlap
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    streams = [torch.cuda.Stream() for _ in range(4)]
    for c, ((kl, dl, l1, l2, _, _), (k_off, d_off, o1_off, o2_off)) in enumerate(zip(cases, where)):
        sp = streams[c % len(streams)].cuda_stream
        assert aead.dev_hkdf(hid, keys=d_in.data_ptr() + k_off, key_len=kl,
                             data=d_in.data_ptr() + d_off if dl else 0, data_len=dl, n=SESSIONS,
                             out1=d_out.data_ptr() + o1_off, out1_len=l1,
                             out2=d_out.data_ptr() + o2_off, out2_len=l2, stream=sp) == 0
    torch.cuda.synchronize()
    print(f"hkdf sweep {hid:#x}: {len(cases)} launches in {time.perf_counter() - t0:.2f} s")
    got = d_out.cpu().numpy().tobytes()
    assert d_in.cpu().numpy().tobytes() == bytes(inp), "keys or data written"
    if got != bytes(want):
        for (kl, dl, l1, l2, _, _), (_, _, o1_off, o2_off) in zip(cases, where):
            end = o2_off + SESSIONS * l2 + 8
            assert got[o1_off - 8:end] == bytes(want[o1_off - 8:end]), (kl, dl, l1, l2)
    assert got == bytes(want)


def _hkdf_with_canaries(A, torch, hid, keys, datas, l1, l2):
    """One launch into two outputs with 64 canary bytes on each side (a zero
    output length leaves only canaries); the outputs of session i."""
    n = len(keys)
    d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).cuda()
    d_data = torch.from_numpy(np.frombuffer(b"".join(datas), dtype=np.uint8).copy()).cuda()
    outs = [torch.full((64 + n * l + 64,), 0xC3, dtype=torch.uint8, device="cuda") for l in (l1, l2)]
    assert A.dev_hkdf(hid, keys=d_keys.data_ptr(), key_len=len(keys[0]), data=d_data.data_ptr(),
                      data_len=len(datas[0]), n=n, out1=outs[0].data_ptr() + 64, out1_len=l1,
                      out2=outs[1].data_ptr() + 64, out2_len=l2,
                      stream=torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    rows = []
    for o, l in zip(outs, (l1, l2)):
        h = o.cpu().numpy()
        assert (h[:64] == 0xC3).all() and (h[64 + n * l:] == 0xC3).all(), "wrote outside an output"
        rows.append([h[64 + i * l:64 + (i + 1) * l].tobytes() for i in range(n)])
    return list(zip(*rows))


@pytest.mark.gpu
@pytest.mark.parametrize("hid", HASHES)
def test_dev_hkdf_length_limits(aead, gpu, hid):
    """The longest key and data the device HKDF takes, over two workgroups
    (65 sessions), with both outputs whole and with either one empty: nothing
    is written for an output length of 0."""
    import torch
    hl, n = HLEN[hid], 65
    pool = np.random.default_rng(hid + 2).integers(0, 256, 2 * n * 256, dtype=np.uint8).tobytes()
    keys = [pool[i * 256:(i + 1) * 256] for i in range(n)]
    datas = [pool[(n + i) * 256:(n + i + 1) * 256] for i in range(n)]
    for l1, l2 in ((hl, hl), (0, hl), (hl, 0)):
        got = _hkdf_with_canaries(aead, torch, hid, keys, datas, l1, l2)
        for i in range(n):
            assert got[i] == py_hkdf(hid, keys[i], datas[i], l1, l2), (l1, l2, i)


@pytest.mark.gpu
@pytest.mark.parametrize("hid", HASHES)
def test_dev_split_batch_matches_oracle(aead, gpu, oracle, hid):
    """4096 sessions (C4/C5's state count) through the split shape, plus a
    mix_key batch (HKDF(ck, 32-byte DH output) -> new ck and temp key)."""
    import torch
    rng = np.random.default_rng(hid)
    n, hl = 4096, HLEN[hid]
    ck = rng.integers(0, 256, (n, hl), dtype=np.uint8)
    d_ck = torch.from_numpy(ck.reshape(-1).copy()).cuda()
    k1 = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    k2 = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    assert aead.dev_split(hid, ck=d_ck.data_ptr(), n=n, k1=k1.data_ptr(), k2=k2.data_ptr()) == 0
    torch.cuda.synchronize()
    k1h, k2h = k1.cpu().numpy().reshape(n, 32), k2.cpu().numpy().reshape(n, 32)
    for i in list(range(0, n, 97)) + [n - 1]:
        e1, e2 = oracle.hkdf(hid, bytes(ck[i]), b"", 32, 32)
        assert bytes(k1h[i]) == e1 and bytes(k2h[i]) == e2, i
    dh = rng.integers(0, 256, (256, 32), dtype=np.uint8)
    o1, o2 = _run_hkdf(aead, torch, hid, ck[:256], dh, hl, hl)
    for i in range(0, 256, 17):
        e1, e2 = oracle.hkdf(hid, bytes(ck[i]), bytes(dh[i]), hl, hl)
        assert bytes(o1[i]) == e1 and bytes(o2[i]) == e2, i


@pytest.mark.gpu
@pytest.mark.parametrize("cipher", [0x4301, 0x4302])
def test_split_keys_drive_transport(aead, gpu, oracle, cipher):
    """split -> noise_aead_dev_prepare -> seal, all on the device; equal to
    the oracle's split + encrypt (the c1 direction, nonce 0..)."""
    import torch
    rng = np.random.default_rng(cipher)
    n, L = 64, 300
    ck = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d_ck = torch.from_numpy(ck.reshape(-1).copy()).cuda()
    k1 = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    k2 = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    assert aead.dev_split(0x4801, ck=d_ck.data_ptr(), n=n, k1=k1.data_ptr(), k2=k2.data_ptr(),
                          stream=sp) == 0
    ctx = torch.empty(n * aead.dev_ctx_bytes(cipher), dtype=torch.uint8, device="cuda")
    assert aead.dev_prepare(cipher, k1.data_ptr(), n, ctx.data_ptr(), sp) == 0
    pt = rng.integers(0, 256, (n, 320), dtype=np.uint8)
    d_pt = torch.from_numpy(pt.reshape(-1).copy()).cuda()
    d_ct = torch.zeros(n * 320, dtype=torch.uint8, device="cuda")
    nb = torch.zeros(n, dtype=torch.int64, device="cuda")
    assert aead.dev_uniform(False, cipher, ctx=ctx.data_ptr(), nonce_base=nb.data_ptr(),
                            inp=d_pt.data_ptr(), out=d_ct.data_ptr(), in_stride=320,
                            out_stride=320, length=L, n_records=n, recs_per_state=1,
                            stream=sp) == 0
    torch.cuda.synchronize()
    ct = d_ct.cpu().numpy().reshape(n, 320)
    for i in range(n):
        key1, _ = oracle.hkdf(0x4801, bytes(ck[i]), b"", 32, 32)
        assert bytes(ct[i, :L + 16]) == oracle.encrypt(cipher, key1, 0, bytes(pt[i, :L])), i


@pytest.mark.gpu
@pytest.mark.parametrize("cipher,hid", [(0x4301, 0x4801), (0x4302, 0x4803), (0x4301, 0x4804),
                                        (0x4302, 0x4802)])
def test_encrypt_and_hash_batch(aead, gpu, oracle, cipher, hid):
    """noise_symmetricstate_{encrypt,decrypt}_and_hash (symmetricstate.c
    :352-445) for 300 states at once: AD = h_i; h_i <- HASH(h_i || CT || tag);
    a record whose tag fails keeps its old h and its ciphertext."""
    import torch
    rng = np.random.default_rng(cipher + hid)
    n, hl = 300, HLEN[hid]
    keys = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d_keys = torch.from_numpy(keys.reshape(-1).copy()).cuda()
    cb = aead.dev_ctx_bytes(cipher)
    ctx = torch.empty(n * cb, dtype=torch.uint8, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    assert aead.dev_prepare(cipher, d_keys.data_ptr(), n, ctx.data_ptr(), sp) == 0
    h0 = rng.integers(0, 256, (n, hl), dtype=np.uint8)
    lens = rng.integers(0, 1500, n)
    offs = np.zeros(n, dtype=np.int64)
    offs[1:] = np.cumsum(lens + 16 + 7)[:-1]
    total = int(offs[-1] + lens[-1] + 16 + 64)
    pt = rng.integers(0, 256, total, dtype=np.uint8)
    nonces = rng.integers(0, 2**40, n).astype(np.uint64)
    dt = [("in_off", "<u8"), ("out_off", "<u8"), ("nonce", "<u8"), ("ctx_off", "<u8"),
          ("ad_off", "<u8"), ("len", "<u4"), ("ad_len", "<u4")]
    recs = np.zeros(n, dtype=dt)
    recs["in_off"] = recs["out_off"] = offs
    recs["nonce"] = nonces
    recs["ctx_off"] = np.arange(n, dtype=np.uint64) * cb
    recs["ad_off"] = np.arange(n, dtype=np.uint64) * hl
    recs["len"] = lens
    recs["ad_len"] = hl
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    d_buf = torch.from_numpy(pt.copy()).cuda()
    d_h = torch.from_numpy(h0.reshape(-1).copy()).cuda()
    kw = dict(ctx_base=ctx.data_ptr(), h=d_h.data_ptr(), recs=d_recs.data_ptr(), inp=d_buf.data_ptr(),
              out=d_buf.data_ptr(), n_records=n, stream=sp)
    # job->ad must be the hashes
    assert aead.dev_and_hash(False, cipher, hid, **kw) == 0
    torch.cuda.synchronize()
    ct = d_buf.cpu().numpy()
    h1 = d_h.cpu().numpy().reshape(n, hl)
    for i in range(n):
        o, L = int(offs[i]), int(lens[i])
        exp = oracle.encrypt(cipher, bytes(keys[i]), int(nonces[i]), bytes(pt[o:o + L]),
                             bytes(h0[i]))
        assert bytes(ct[o:o + L + 16]) == exp, i
        assert bytes(h1[i]) == oracle.hash(hid, bytes(h0[i]) + exp), i
    # the receiving side: same h0, tampered records fail and keep h0
    bad = np.arange(n) % 23 == 4
    tampered = ct.copy()
    for i in np.nonzero(bad)[0]:
        tampered[int(offs[i]) + int(lens[i]) + 3] ^= 1
    d_buf = torch.from_numpy(tampered.copy()).cuda()
    d_h = torch.from_numpy(h0.reshape(-1).copy()).cuda()
    d_st = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    kw.update(h=d_h.data_ptr(), inp=d_buf.data_ptr(), out=d_buf.data_ptr())
    assert aead.dev_and_hash(True, cipher, hid, status=d_st.data_ptr(), **kw) == 0
    torch.cuda.synchronize()
    st, back, h2 = d_st.cpu().numpy(), d_buf.cpu().numpy(), d_h.cpu().numpy().reshape(n, hl)
    assert np.array_equal(st != 0, bad)
    for i in range(n):
        o, L = int(offs[i]), int(lens[i])
        if bad[i]:
            assert bytes(h2[i]) == bytes(h0[i]) and np.array_equal(back[o:o + L + 16],
                                                                   tampered[o:o + L + 16]), i
        else:
            assert np.array_equal(back[o:o + L], pt[o:o + L]), i
            assert bytes(h2[i]) == oracle.hash(hid, bytes(h0[i]) + bytes(ct[o:o + L + 16])), i


@pytest.mark.gpu
@pytest.mark.parametrize("cipher,hid", [(0x4301, 0x4801), (0x4302, 0x4803), (0x4301, 0x4804),
                                        (0x4302, 0x4802)])
def test_encrypt_and_hash_every_length(aead, gpu, oracle, cipher, hid):
    """One job whose record i is i bytes long, i = 0..271: the hashed message
    h || CT || tag has hash_len + i + 16 bytes, so every residue mod 128 (and
    mod 64) comes up, each padding boundary of SHA-2's and BLAKE2's last block
    among them, on the sealing and on the opening side.  The hashes are
    hashlib's."""
    import torch
    rng = np.random.default_rng(cipher * 3 + hid)
    n, hl = 272, HLEN[hid]
    assert {(hl + i + 16) % 128 for i in range(n)} == set(range(128))
    keys = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d_keys = torch.from_numpy(keys.reshape(-1).copy()).cuda()
    cb = aead.dev_ctx_bytes(cipher)
    ctx = torch.empty(n * cb, dtype=torch.uint8, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    assert aead.dev_prepare(cipher, d_keys.data_ptr(), n, ctx.data_ptr(), sp) == 0
    h0 = rng.integers(0, 256, (n, hl), dtype=np.uint8)
    lens = np.arange(n)
    offs = np.zeros(n, dtype=np.int64)
    offs[1:] = np.cumsum(lens + 16 + 7)[:-1]
    total = int(offs[-1] + lens[-1] + 16 + 64)
    pt = rng.integers(0, 256, total, dtype=np.uint8)
    nonces = rng.integers(0, 2**40, n).astype(np.uint64)
    dt = [("in_off", "<u8"), ("out_off", "<u8"), ("nonce", "<u8"), ("ctx_off", "<u8"),
          ("ad_off", "<u8"), ("len", "<u4"), ("ad_len", "<u4")]
    recs = np.zeros(n, dtype=dt)
    recs["in_off"] = recs["out_off"] = offs
    recs["nonce"] = nonces
    recs["ctx_off"] = np.arange(n, dtype=np.uint64) * cb
    recs["ad_off"] = np.arange(n, dtype=np.uint64) * hl
    recs["len"] = lens
    recs["ad_len"] = hl
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    d_buf = torch.from_numpy(pt.copy()).cuda()
    d_h = torch.from_numpy(h0.reshape(-1).copy()).cuda()
    kw = dict(ctx_base=ctx.data_ptr(), h=d_h.data_ptr(), recs=d_recs.data_ptr(), inp=d_buf.data_ptr(),
              out=d_buf.data_ptr(), n_records=n, stream=sp)
    assert aead.dev_and_hash(False, cipher, hid, **kw) == 0
    torch.cuda.synchronize()
    ct = d_buf.cpu().numpy()
    h1 = d_h.cpu().numpy().reshape(n, hl)
    want_h = []
    for i in range(n):
        o = int(offs[i])
        exp = oracle.encrypt(cipher, bytes(keys[i]), int(nonces[i]), bytes(pt[o:o + i]), bytes(h0[i]))
        assert bytes(ct[o:o + i + 16]) == exp, i
        want_h.append(HASHLIB[hid](bytes(h0[i]) + exp).digest())
        assert bytes(h1[i]) == want_h[i], i
    # the receiving side from the same h0: every record opens and arrives at the same hash
    d_h = torch.from_numpy(h0.reshape(-1).copy()).cuda()
    d_st = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    kw.update(h=d_h.data_ptr())
    assert aead.dev_and_hash(True, cipher, hid, status=d_st.data_ptr(), **kw) == 0
    torch.cuda.synchronize()
    st, back, h2 = d_st.cpu().numpy(), d_buf.cpu().numpy(), d_h.cpu().numpy().reshape(n, hl)
    assert (st == 0).all()
    for i in range(n):
        o = int(offs[i])
        assert np.array_equal(back[o:o + i], pt[o:o + i]), i
        assert bytes(h2[i]) == want_h[i], i
