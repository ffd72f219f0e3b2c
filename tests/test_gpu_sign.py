"""Batched Ed25519 on the device: noise_aead_dev_sign_verify / _sign_public /
_sign (header section 17).

Every verdict, public key and signature the kernels write is compared with the
reference's own (tests/golden/ed25519.json, run as one batch) or with the model
of tests/ed25519_model.py, which tests/test_sign_model_host.py proves against
that fixture.  Sizes: one entry, one wave less one, one wave, one wave plus
one, and several workgroups with a partial last one.  The random entries are
made once and shared; message lengths are the device's padding and block
edges (ed25519_model.MESSAGE_LENGTHS)."""
import functools

import numpy as np
import pytest

import ed25519_model as M
import handshake_model as HM
import transport_model as T
from gpu_support import dev_bytes
from handshake_gpu import Buf, Side, basic_vector, make_sessions, packed, payload_rows
from transport_gpu import Table, Wire, plain_streams

pytestmark = pytest.mark.gpu
ID = M.SIGN_ED25519
CANARY = 0xEE
POOL = 130


def flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def pool(one_signer=False):
    """POOL entries (seed, msg, pub, sig, status, the seed's own public key):
    every third one tampered in R, S, the message or the key in turn;
    one_signer: the same key for all (then the key is never the tampered part)."""
    rng = np.random.default_rng(2519 + one_signer)
    ca = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    out = []
    for i in range(POOL):
        seed = ca if one_signer else rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        ln = M.MESSAGE_LENGTHS[int(rng.integers(len(M.MESSAGE_LENGTHS)))]
        msg = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        own = pub = M.publickey(seed)
        sig = M.sign(msg, seed, pub)
        if i % 3 == 1:
            what = (i // 3) % (3 if one_signer else 4)
            if what == 0:
                sig = flip(sig, int(rng.integers(256)))
            elif what == 1:
                sig = flip(sig, 256 + int(rng.integers(253)))
            elif what == 2 and msg:
                msg = flip(msg, int(rng.integers(8 * len(msg))))
            else:
                pub = flip(pub, int(rng.integers(255))) if not one_signer else pub
                sig = sig if not one_signer else flip(sig, 300)
        out.append((seed, msg, pub, sig, M.status(msg, pub, sig), own))
    assert {e[4] for e in out} == {0, 6} and sum(e[4] == 6 for e in out) >= POOL // 3 - 2
    return out


def place(torch, items, width, stride, lead):
    """The items `stride` bytes apart from byte `lead` of a canary-filled device
    buffer (stride 0: the one item at `lead`); (tensor, pointer of item 0)."""
    n = len(items)
    h = np.full(lead + (n - 1) * stride + width + 16, CANARY, dtype=np.uint8)
    for i, k in enumerate(items if stride else items[:1]):
        assert len(k) == width
        h[lead + i * stride: lead + i * stride + width] = np.frombuffer(k, dtype=np.uint8)
    d = torch.from_numpy(h).cuda()
    return d, d.data_ptr() + lead


class Messages:
    """The messages in one canary-filled device buffer, with their offset and
    length arrays; descending: the later a message, the lower it lies."""

    def __init__(self, torch, msgs, lead=0, descending=False):
        order = list(range(len(msgs)))
        if descending:
            order.reverse()
        offs, cur = [0] * len(msgs), 7 + lead
        for i in order:
            offs[i] = cur
            cur += len(msgs[i]) + (i % 3)  # unequal gaps; a gap of 0 lets neighbours touch
        h = np.full(cur + 16, CANARY, dtype=np.uint8)
        for o, m in zip(offs, msgs):
            h[o:o + len(m)] = np.frombuffer(m, dtype=np.uint8)
        self.buf = torch.from_numpy(h).cuda()
        self.off = torch.tensor(offs, dtype=torch.int64, device="cuda")
        self.len = torch.tensor([len(m) for m in msgs], dtype=torch.int32, device="cuda")
        self.kw = dict(msg=self.buf.data_ptr(), msg_off=self.off.data_ptr(), msg_len=self.len.data_ptr())
        self.inputs = [self.buf, self.off, self.len]


def verify(aead, torch, entries, *, pub_stride=32, sig_stride=64, lead=0, descending=False, status_in=None,
           in_place=False):
    """the n status bytes of one call over entries (msg, pub, sig), written
    between canaries; checks that no input changed"""
    n = len(entries)
    m = Messages(torch, [e[0] for e in entries], lead, descending)
    d_pub, p_pub = place(torch, [e[1] for e in entries], 32, pub_stride, lead)
    d_sig, p_sig = place(torch, [e[2] for e in entries], 64, sig_stride, lead)
    out = torch.full((64 + n + 64,), 0xC3, dtype=torch.uint8, device="cuda")
    p_in = 0
    if status_in is not None:
        if in_place:
            out[64:64 + n] = torch.tensor(list(status_in), dtype=torch.uint8, device="cuda")
            p_in = out.data_ptr() + 64
        else:
            d_in = dev_bytes(bytes(status_in))
            p_in = d_in.data_ptr()
    inputs = [d_pub, d_sig, *m.inputs]
    before = [t.clone() for t in inputs]
    rc = aead.dev_sign_verify(ID, pub=p_pub, pub_stride=pub_stride, sig=p_sig, sig_stride=sig_stride, n=n,
                              status_in=p_in, status=out.data_ptr() + 64,
                              stream=torch.cuda.current_stream().cuda_stream, **m.kw)
    assert rc == 0, hex(rc)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:64] == 0xC3).all() and (o[64 + n:] == 0xC3).all(), "wrote outside d_status[n)"
    assert all(torch.equal(a, b) for a, b in zip(inputs, before)), "an input was written"
    if status_in is not None and not in_place:
        assert bytes(d_in.cpu().numpy()) == bytes(status_in), "d_status_in was written"
    return o[64:64 + n].tolist()


def sign(aead, torch, seeds, pubs, msgs, *, priv_stride=32, pub_stride=32, lead=0, descending=False):
    """(public keys, signatures) of one _sign_public and one _sign call"""
    n = len(seeds)
    m = Messages(torch, msgs, lead, descending)
    d_priv, p_priv = place(torch, seeds, 32, priv_stride, lead)
    d_pub, p_pub = place(torch, pubs, 32, pub_stride, lead)
    inputs = [d_priv, d_pub, *m.inputs]
    before = [t.clone() for t in inputs]
    pk, sg = packed(torch, n, 32), packed(torch, n, 64)
    sp = torch.cuda.current_stream().cuda_stream
    assert aead.dev_sign_public(ID, priv=p_priv, priv_stride=priv_stride, n=n, pub_out=pk.data_ptr(), stream=sp) == 0
    assert aead.dev_sign(ID, priv=p_priv, priv_stride=priv_stride, pub=p_pub, pub_stride=pub_stride, n=n,
                         sig_out=sg.data_ptr(), stream=sp, **m.kw) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(inputs, before)), "an input was written"
    h_pk, h_sg = pk.cpu().numpy(), sg.cpu().numpy()
    assert (h_pk[32 * n:] == CANARY).all() and (h_sg[64 * n:] == CANARY).all(), "wrote past a packed output"
    return ([h_pk[32 * i:32 * i + 32].tobytes() for i in range(n)],
            [h_sg[64 * i:64 * i + 64].tobytes() for i in range(n)])


def test_reference_fixture_as_one_batch(aead, gpu):
    import torch
    cases = M.fixture_verify_cases()
    got = verify(aead, torch, [(msg, pub, sig) for _, msg, pub, sig, _ in cases])
    for (name, _, _, _, ok), st in zip(cases, got):
        assert st == (0 if ok else 6), name
    signed = M.fixture_sign_cases()
    pks, sigs = sign(aead, torch, [c[1] for c in signed], [c[2] for c in signed], [c[3] for c in signed])
    for (name, _, pub, _, sig), pk, sg in zip(signed, pks, sigs):
        assert pk == pub, name
        assert sg == sig, name


@pytest.mark.parametrize("n", [1, 63, 64, 65, POOL])
def test_every_entry_matches_the_model(aead, gpu, n):
    import torch
    e = pool()[:n]
    assert verify(aead, torch, [x[1:4] for x in e]) == [x[4] for x in e]
    # the seeds' own keys sign the (possibly tampered) messages
    pubs = [x[5] for x in e]
    pks, sigs = sign(aead, torch, [x[0] for x in e], pubs, [x[1] for x in e])
    assert pks == pubs
    for i in (0, n // 2, n - 1):
        assert sigs[i] == M.sign(e[i][1], e[i][0], pubs[i]), i


@pytest.mark.parametrize("pub_stride,sig_stride,lead,descending", [(0, 64, 0, False), (32, 72, 1, False),
                                                                   (40, 64, 3, True), (0, 72, 3, True),
                                                                   (40, 72, 1, False)])
def test_strides_and_placement(aead, gpu, pub_stride, sig_stride, lead, descending):
    """pub_stride 0 is one signer for all entries (a CA); a lead of 1 or 3
    bytes makes every load unaligned; descending offsets put message i + 1
    below message i.  70 entries: two workgroups, the second partial."""
    import torch
    e = pool(one_signer=pub_stride == 0)[:70]
    got = verify(aead, torch, [x[1:4] for x in e], pub_stride=pub_stride, sig_stride=sig_stride, lead=lead,
                 descending=descending)
    assert got == [x[4] for x in e]
    # signing with the same layout of keys: the public keys are taken as given
    seeds, msgs = [x[0] for x in e], [x[1] for x in e]
    pubs = [x[2] for x in e]
    pks, sigs = sign(aead, torch, seeds, pubs, msgs, priv_stride=pub_stride, pub_stride=pub_stride, lead=lead,
                     descending=descending)
    for i in (0, 1, 63, 64, 69):
        k = i if pub_stride else 0
        assert pks[i] == e[k][5], i
        assert sigs[i] == M.sign(msgs[i], seeds[k], pubs[k]), i


@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
def test_status_pass_through(aead, gpu, in_place):
    """An entry whose input status is non-zero keeps it: those entries carry
    forged signatures, which would read 6 had they been looked at, and the good
    entries beside them read 0."""
    import torch
    e = [list(x[1:5]) for x in pool()]
    status_in = [0] * POOL
    for i, v in ((0, 1), (63, 3), (64, 5), (POOL - 1, 200)):
        status_in[i] = v
        msg, pub, sig, _ = e[i]
        e[i] = [msg, pub, flip(sig, 7), None]
        assert M.status(msg, pub, e[i][2]) == 6
    want = [status_in[i] or e[i][3] for i in range(POOL)]
    assert want[1] == 6 and want[2] == 0 and want[0] == 1 and want[POOL - 1] == 200
    got = verify(aead, torch, [x[:3] for x in e], status_in=status_in, in_place=in_place)
    assert got == want


def test_sign_then_verify_on_the_device(aead, gpu):
    """_sign_public -> _sign -> _sign_verify for 130 seeds with nothing but the
    seeds and the messages coming from the host."""
    import torch
    e = pool()
    n = POOL
    seeds, msgs = [x[0] for x in e], [x[1] for x in e]
    m = Messages(torch, msgs)
    d_seed = dev_bytes(b"".join(seeds))
    pk, sg = packed(torch, n, 32), packed(torch, n, 64)
    st = torch.full((n,), 0xC3, dtype=torch.uint8, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    assert aead.dev_sign_public(ID, priv=d_seed.data_ptr(), n=n, pub_out=pk.data_ptr(), stream=sp) == 0
    assert aead.dev_sign(ID, priv=d_seed.data_ptr(), pub=pk.data_ptr(), n=n, sig_out=sg.data_ptr(), stream=sp,
                         **m.kw) == 0
    assert aead.dev_sign_verify(ID, pub=pk.data_ptr(), sig=sg.data_ptr(), n=n, status=st.data_ptr(), stream=sp,
                                **m.kw) == 0
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n
    h_pk, h_sg = pk.cpu().numpy(), sg.cpu().numpy()
    for i in range(n):
        assert h_pk[32 * i:32 * i + 32].tobytes() == e[i][5], i
        assert h_sg[64 * i:64 * i + 64].tobytes() == M.sign(msgs[i], seeds[i], e[i][5]), i


def test_certificates_gate_the_session_table(aead, gpu, oracle):
    """The flow this is for.  Eight XX handshakes whose third message carries
    sig_CA(client static key) as its payload.  The responder reads the message,
    splits, verifies the payloads against the remote static keys the handshake
    stored — one CA key, the handshake's status as the input status — and keys
    its table with the merged status, all on one stream with nothing read on the
    host in between.  Two certificates are forged and one message has a spoilt
    tag: exactly the five good slots are keyed, and carry traffic."""
    import torch
    A = aead
    name = "Noise_XX_25519_ChaChaPoly_BLAKE2s"
    v = basic_vector(name)
    n, forged, spoilt = 8, (1, 6), 4
    sess = make_sessions(v, n, 517)
    ca_seed = bytes(range(32))
    ca_pub = M.publickey(ca_seed)
    certs = []
    for i, s in enumerate(sess):
        static_pub = HM.dh_base(s["ini_s"])
        c = M.sign(static_pub, ca_seed, ca_pub)
        certs.append(flip(c, 300 + i) if i in forged else c)
    ini, res = Side(A, torch, v, sess, True), Side(A, torch, v, sess, False)
    for j in range(2):  # e; e, ee, s, es
        w, r = (ini, res) if j == 0 else (res, ini)
        rows = payload_rows(v, j, n, 517)
        plen = len(rows[0])
        mlen = plen + w.overhead
        payload, msg = Buf(torch, n, max(plen, 1), [p or b"\0" for p in rows]), Buf(torch, n, mlen)
        assert w.write(payload, plen, msg) == 0
        assert r.read(msg, mlen, Buf(torch, n, max(plen, 1))) == 0
    mlen = 64 + ini.overhead
    msg = Buf(torch, n, mlen)
    assert ini.write(Buf(torch, n, 64, certs), 64, msg) == 0
    sent = [bytearray(r) for r in msg.read()]
    sent[spoilt][-1] ^= 0x01
    msg = Buf(torch, n, mlen, [bytes(r) for r in sent])
    k1i, k2i, _ = ini.split()
    assert ini.status() == [0] * n

    # the responder's tick: no host read from here to the end of _set_keys
    sp = res.sp
    slots = [3, 0, 5, 1, 7, 2, 6, 4]
    tab = Table(A, torch, oracle, T.CHACHAPOLY, False, 64, n=n)
    ca = dev_bytes(ca_pub)
    off = torch.tensor([32 * i for i in range(n)], dtype=torch.int64, device="cuda")
    ln = torch.full((n,), 32, dtype=torch.int32, device="cuda")
    merged = torch.full((n + 1,), 0xC3, dtype=torch.uint8, device="cuda")
    payload = Buf(torch, n, 64)
    k1, k2, hh = packed(torch, n, 32), packed(torch, n, 32), packed(torch, n, 32)
    torch.cuda.synchronize()
    assert res.read(msg, mlen, payload) == 0
    assert A.dev_handshake_split(res.hs, k1=k1.data_ptr(), k2=k2.data_ptr(), handshake_hash=hh.data_ptr(),
                                 stream=sp) == 0
    assert A.dev_sign_verify(ID, pub=ca.data_ptr(), pub_stride=0, sig=payload.ptr, sig_stride=payload.stride,
                             msg=A.dev_handshake_remote_static(res.hs), msg_off=off.data_ptr(),
                             msg_len=ln.data_ptr(), n=n, status_in=A.dev_handshake_status(res.hs),
                             status=merged.data_ptr(), stream=sp) == 0
    want = [6 if i in forged else 1 if i == spoilt else 0 for i in range(n)]
    tab.set_keys(slots, list(zip(k1i, k2i)), want, ptrs=(k1.data_ptr(), k2.data_ptr(), merged.data_ptr()))

    assert merged.cpu().tolist() == want + [0xC3]
    assert res.status() == [1 if i == spoilt else 0 for i in range(n)]  # the handshake's own bytes are not written
    good = [i for i in range(n) if want[i] == 0]
    assert len(good) == 5
    assert tab.has_key() == [1 if slots.index(s) in good else 0 for s in range(n)]
    tab.check_contexts()
    ini_tab = Table(A, torch, oracle, T.CHACHAPOLY, True, 64, n=n)
    ini_tab.set_keys(slots, list(zip(k1i, k2i)), [0] * n, ptrs=(ini.k1.data_ptr(), ini.k2.data_ptr(), 0))
    plain = plain_streams(72, n + 1, big=False)
    streams = [plain[j + 1] for j in range(n)]
    for w, rd, senders in ((ini_tab, tab, slots), (tab, ini_tab, [slots[i] for i in good])):
        wire = Wire(torch, streams[:len(senders)])
        w.run("seal", wire, senders, max_frames=32)
        results = rd.run("open", wire, senders)
        opened = wire.streams()
        for j, s in enumerate(senders):
            if slots.index(s) in good:
                assert results[j][2] == 0 and results[j][0] == (j + 1) % 6, (j, results[j])
                for at, L in T.walk(streams[j], 0)[0]:
                    assert opened[j][at:at + L - 16] == streams[j][at:at + L - 16]
            else:
                assert results[j] == (0, 0, A.ERROR_INVALID_STATE), (j, results[j])
    for x in (tab, ini_tab, ini, res):
        x.free()

