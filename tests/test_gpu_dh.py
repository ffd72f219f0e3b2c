"""Batched X25519 on the device: noise_aead_dev_dh_calculate / _dh_public.

Every shared key and public key the kernels write is compared with the
big-integer ladder of tests/x25519_ref.py, which tests/test_dh_host.py proves
against the reference's own outputs (tests/golden/x25519.json); the fixture
itself runs as one batch.  Sizes: one session, one wave less one, one wave,
one wave plus one, and several workgroups with a partial last one."""
import functools

import numpy as np
import pytest

import x25519_ref as X

pytestmark = pytest.mark.gpu
ID = 0x4401


@functools.lru_cache(maxsize=None)
def ref(k: bytes, u: bytes) -> bytes:
    return X.x25519(k, u)


def rows(a):
    return [bytes(r) for r in a]


def place(torch, keys, stride, lead):
    """The n keys `stride` bytes apart from byte `lead` of a 0xEE-filled device
    buffer (stride 0: the one key at `lead`); (tensor, pointer of key 0)."""
    n = len(keys)
    size = lead + (n - 1) * stride + 32 + 16
    h = np.full(size, 0xEE, dtype=np.uint8)
    for i, k in enumerate(keys if stride else keys[:1]):
        h[lead + i * stride: lead + i * stride + 32] = np.frombuffer(k, dtype=np.uint8)
    d = torch.from_numpy(h).cuda()
    assert d.data_ptr() % 16 == 0
    return d, d.data_ptr() + lead


def run(aead, torch, privs, pubs, n, *, priv_stride=32, pub_stride=32, lead=0):
    """calculate (pubs given) or public (pubs None) of n sessions into an
    output with 64 canary bytes on each side; the n outputs.  Checks that the
    canaries and the input buffers read back as they were."""
    d_priv, p_priv = place(torch, privs, priv_stride, lead)
    before = [d_priv.clone()]
    out = torch.full((64 + 32 * n + 64,), 0xC3, dtype=torch.uint8, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    if pubs is not None:
        d_pub, p_pub = place(torch, pubs, pub_stride, lead)
        before.append(d_pub.clone())
        rc = aead.dev_dh_calculate(ID, priv=p_priv, priv_stride=priv_stride, pub=p_pub, pub_stride=pub_stride,
                                   n=n, shared=out.data_ptr() + 64, stream=sp)
    else:
        rc = aead.dev_dh_public(ID, priv=p_priv, priv_stride=priv_stride, n=n, pub_out=out.data_ptr() + 64,
                                stream=sp)
    assert rc == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:64] == 0xC3).all() and (o[64 + 32 * n:] == 0xC3).all(), "wrote outside d_shared[32 n)"
    assert torch.equal(d_priv, before[0]), "private keys written"
    if pubs is not None:
        assert torch.equal(d_pub, before[1]), "public values written"
    return rows(o[64: 64 + 32 * n].reshape(n, 32))


def keys(rng, n):
    return rows(rng.integers(0, 256, (n, 32), dtype=np.uint8))


def test_reference_fixture_as_one_batch(aead, gpu):
    import torch
    cases = X.fixture_cases()
    privs = [bytes.fromhex(c["priv"]) for c in cases]
    pubs = [bytes.fromhex(c["pub"]) for c in cases]
    shared = run(aead, torch, privs, pubs, len(cases))
    public = run(aead, torch, privs, None, len(cases))
    for c, s, p in zip(cases, shared, public):
        assert s.hex() == c["shared"], c["name"]
        assert p.hex() == c["public"], c["name"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_every_session_matches_the_ladder(aead, gpu, n):
    import torch
    rng = np.random.default_rng(1000 + n)
    privs, pubs = keys(rng, n), keys(rng, n)
    shared = run(aead, torch, privs, pubs, n)
    public = run(aead, torch, privs, None, n)
    for i in range(n):
        assert shared[i] == ref(privs[i], pubs[i]), i
        assert public[i] == ref(privs[i], (9).to_bytes(32, "little")), i


@pytest.mark.parametrize("priv_stride,pub_stride,lead", [(0, 32, 0), (32, 0, 0), (40, 40, 1), (32, 32, 0),
                                                         (0, 40, 3), (72, 0, 2)])
def test_strides_and_unaligned_keys(aead, gpu, priv_stride, pub_stride, lead):
    """Stride 0 is one key for all sessions (a static key against n
    ephemerals); stride 40 from a pointer one byte past an aligned one makes
    every load unaligned.  70 sessions: two workgroups, the second partial."""
    import torch
    n = 70
    rng = np.random.default_rng(7)  # the same keys for every layout: one reference
    privs, pubs = keys(rng, n), keys(rng, n)
    shared = run(aead, torch, privs, pubs, n, priv_stride=priv_stride, pub_stride=pub_stride, lead=lead)
    public = run(aead, torch, privs, None, n, priv_stride=priv_stride, lead=lead)
    for i in range(n):
        k = privs[i if priv_stride else 0]
        assert shared[i] == ref(k, pubs[i if pub_stride else 0]), i
        assert public[i] == ref(k, (9).to_bytes(32, "little")), i


def test_both_sides_agree_on_the_device(aead, gpu):
    """calculate(a, public(b)) == calculate(b, public(a)) for 128 pairs, with
    nothing but the private keys coming from the host."""
    import torch
    n = 128
    rng = np.random.default_rng(25519)
    a = torch.from_numpy(rng.integers(0, 256, n * 32, dtype=np.uint8)).cuda()
    b = torch.from_numpy(rng.integers(0, 256, n * 32, dtype=np.uint8)).cuda()
    pa, pb, sa, sb = (torch.zeros(n * 32, dtype=torch.uint8, device="cuda") for _ in range(4))
    sp = torch.cuda.current_stream().cuda_stream
    assert aead.dev_dh_public(ID, priv=a.data_ptr(), n=n, pub_out=pa.data_ptr(), stream=sp) == 0
    assert aead.dev_dh_public(ID, priv=b.data_ptr(), n=n, pub_out=pb.data_ptr(), stream=sp) == 0
    assert aead.dev_dh_calculate(ID, priv=a.data_ptr(), pub=pb.data_ptr(), n=n, shared=sa.data_ptr(),
                                 stream=sp) == 0
    assert aead.dev_dh_calculate(ID, priv=b.data_ptr(), pub=pa.data_ptr(), n=n, shared=sb.data_ptr(),
                                 stream=sp) == 0
    torch.cuda.synchronize()
    assert torch.equal(sa, sb)
    sh = sa.cpu().numpy().reshape(n, 32)
    assert (sh != 0).any(axis=1).all() and len({bytes(r) for r in sh}) == n
    # and they are the right keys, not merely equal ones
    ah, bh = a.cpu().numpy().reshape(n, 32), b.cpu().numpy().reshape(n, 32)
    for i in (0, 63, 64, 127):
        assert bytes(sh[i]) == ref(bytes(ah[i]), ref(bytes(bh[i]), (9).to_bytes(32, "little"))), i


@pytest.mark.parametrize("cipher", [0x4301, 0x4302])
def test_dh_drives_mix_key_split_and_transport(aead, gpu, oracle, cipher):
    """DH -> mix_key -> split -> prepare -> seal for 64 sessions with no host
    round trip: dev_dh_calculate's packed output is dev_hkdf's data.  Equal to
    the ladder -> oracle.hkdf -> oracle.hkdf -> oracle.encrypt."""
    import torch
    H = 0x4801
    rng = np.random.default_rng(cipher)
    n, L = 64, 300
    privs, pubs = keys(rng, n), keys(rng, n)
    ck = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pt = rng.integers(0, 256, (n, 320), dtype=np.uint8)
    d_priv = torch.from_numpy(np.frombuffer(b"".join(privs), dtype=np.uint8).copy()).cuda()
    d_pub = torch.from_numpy(np.frombuffer(b"".join(pubs), dtype=np.uint8).copy()).cuda()
    d_ck = torch.from_numpy(ck.reshape(-1).copy()).cuda()
    dh, ck2, tk, k1, k2 = (torch.zeros(n * 32, dtype=torch.uint8, device="cuda") for _ in range(5))
    sp = torch.cuda.current_stream().cuda_stream
    assert aead.dev_dh_calculate(ID, priv=d_priv.data_ptr(), pub=d_pub.data_ptr(), n=n, shared=dh.data_ptr(),
                                 stream=sp) == 0
    assert aead.dev_hkdf(H, keys=d_ck.data_ptr(), key_len=32, data=dh.data_ptr(), data_len=32, n=n,
                         out1=ck2.data_ptr(), out1_len=32, out2=tk.data_ptr(), out2_len=32, stream=sp) == 0
    assert aead.dev_split(H, ck=ck2.data_ptr(), n=n, k1=k1.data_ptr(), k2=k2.data_ptr(), stream=sp) == 0
    ctx = torch.empty(n * aead.dev_ctx_bytes(cipher), dtype=torch.uint8, device="cuda")
    assert aead.dev_prepare(cipher, k1.data_ptr(), n, ctx.data_ptr(), sp) == 0
    d_pt = torch.from_numpy(pt.reshape(-1).copy()).cuda()
    d_ct = torch.zeros(n * 320, dtype=torch.uint8, device="cuda")
    nb = torch.zeros(n, dtype=torch.int64, device="cuda")
    assert aead.dev_uniform(False, cipher, ctx=ctx.data_ptr(), nonce_base=nb.data_ptr(), inp=d_pt.data_ptr(),
                            out=d_ct.data_ptr(), in_stride=320, out_stride=320, length=L, n_records=n,
                            recs_per_state=1, stream=sp) == 0
    torch.cuda.synchronize()
    ct = d_ct.cpu().numpy().reshape(n, 320)
    for i in range(n):
        new_ck, _ = oracle.hkdf(H, bytes(ck[i]), ref(privs[i], pubs[i]), 32, 32)
        key1, _ = oracle.hkdf(H, new_ck, b"", 32, 32)
        assert bytes(ct[i, :L + 16]) == oracle.encrypt(cipher, key1, 0, bytes(pt[i, :L])), i
