"""Device fallbacks beside the model of tests/handshake_fallback_model.py:
noise_aead_dev_handshake_fallback / _fallback_merge (include/noise_aead_hip.h
section 15) on the objects of tests/handshake_gpu.py.  A session here is a
dict of ini_s, ini_e, res_s, res_e0 (the responder's ephemeral of the original
handshake), res_e (its fresh one of the fallback), rs (the responder static
public key the initiator holds: stale or not), psk, prologue and fb_prologue.  Importable without pytest and without
torch (the callers pass torch in)."""
import numpy as np

import handshake_fallback_model as F
import handshake_model as M
from handshake_gpu import Buf, Side, packed, packed_rows


def rand32(rng):
    return rng.integers(0, 256, 32, dtype=np.uint8).tobytes()


def random_sessions(n, seed, stale=lambda i: False, psk=False, prologue=b"", fb_prologue=b"", shared=False):
    """shared: one responder static key, one prologue and one fallback
    prologue for all (the device side then passes them at stride 0)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = dict(ini_s=rand32(rng), ini_e=rand32(rng), res_s=rand32(rng), res_e=rand32(rng), old=rand32(rng), res_e0=rand32(rng),
                 psk=rand32(rng) if psk else None,
                 prologue=rng.integers(0, 256, 64, dtype=np.uint8).tobytes()[:len(prologue)],
                 fb_prologue=rng.integers(0, 256, 64, dtype=np.uint8).tobytes()[:len(fb_prologue)])
        if shared or i == 0:
            s["prologue"], s["fb_prologue"] = prologue, fb_prologue
        if shared and i:
            s["res_s"], s["old"] = out[0]["res_s"], out[0]["old"]
        s["rs"] = M.dh_base(s["old"] if stale(i) else s["res_s"])
        out.append(s)
    return out


def vector_sessions(v, n, seed):
    """session 0: the fallback vector's keys; the others random, stale too"""
    def hx(key):
        return bytes.fromhex(v[key]) if key in v else None
    prologue = hx("init_prologue") or b""
    assert prologue == (hx("resp_prologue") or b"")
    out = random_sessions(n, seed, stale=lambda i: True, psk="init_psk" in v, prologue=prologue, fb_prologue=prologue)
    out[0].update(ini_s=hx("init_static"), ini_e=hx("init_ephemeral"), res_s=hx("resp_static"),
                  res_e=hx("resp_ephemeral"), rs=hx("init_remote_static"), psk=hx("init_psk"))
    return out


def model_pair(orc, name, s):
    return (M.Session(orc, name, True, s["prologue"], s["psk"], s["ini_s"], s["ini_e"], s["rs"]),
            M.Session(orc, name, False, s["prologue"], s["psk"], s["res_s"], s["res_e0"], None))


def _side(A, torch, name, n, hs, keep):
    side = Side.__new__(Side)
    side.A, side.torch, side.name, side.n, side.hs, side.keep = A, torch, name, n, hs, keep
    side.sp = torch.cuda.current_stream().cuda_stream
    return side


def ik_side(A, torch, name, sess, initiator, shared=False):
    """One side of the original handshake (an IK-like pattern: the initiator
    holds rs).  shared: the responder's static key, the initiator's copy of it
    and the prologue at stride 0."""
    n, kw, keep = len(sess), {}, []

    def give(key, rows, stride=None):
        b = Buf(torch, n, len(rows[0]), rows, stride)
        keep.append(b)
        kw[key], kw[key + "_stride"] = b.ptr, b.stride
    zero = 0 if shared else None
    if initiator:
        give("local_static", [s["ini_s"] for s in sess])
        give("local_ephemeral", [s["ini_e"] for s in sess])
        give("remote_static", [s["rs"] for s in sess], zero)
    else:
        give("local_static", [s["res_s"] for s in sess], zero)
        give("local_ephemeral", [s["res_e0"] for s in sess])
    if sess[0]["psk"] is not None:
        give("psk", [s["psk"] for s in sess])
    if sess[0]["prologue"]:
        give("prologue", [s["prologue"] for s in sess], zero)
        kw["prologue_len"] = len(sess[0]["prologue"])
    sp = torch.cuda.current_stream().cuda_stream
    rc, hs = A.dev_handshake_new(name, A.ROLE_INITIATOR if initiator else A.ROLE_RESPONDER, n, stream=sp, **kw)
    assert rc == 0, (name, hex(rc))
    return _side(A, torch, name, n, hs, keep)


def fall_back(orc, side, models, sess, select=None, flags=0, shared=False):
    """noise_aead_dev_handshake_fallback on `side` and F.fallback on its
    models: (the Side over fb, the models: a Fallback, or None for a session
    that does not take part).  The models of `side` get their status 5."""
    A, torch, n = side.A, side.torch, side.n
    was_initiator = models[0].initiator
    kw, keep = {}, []

    def give(key, rows, stride=None):
        b = Buf(torch, n, len(rows[0]), rows, stride)
        keep.append(b)
        kw[key], kw[key + "_stride"] = b.ptr, b.stride
    if not was_initiator:
        give("local_ephemeral", [s["res_e"] for s in sess])
    if sess[0]["psk"] is not None:
        give("psk", [s["psk"] for s in sess])
    if sess[0]["fb_prologue"]:
        give("prologue", [s["fb_prologue"] for s in sess], 0 if shared else None)
        kw["prologue_len"] = len(sess[0]["fb_prologue"])
    if select is not None:
        keep.append(torch.tensor(list(select), dtype=torch.uint8, device="cuda"))
        kw["select"] = keep[-1].data_ptr()
    rc, fb = A.dev_handshake_fallback(side.hs, flags=flags, stream=side.sp, **kw)
    assert rc == 0 and fb, ("fallback", hex(rc))
    out = []
    for i, (m, s) in enumerate(zip(models, sess)):
        rc, f = F.fallback(orc, m, s["fb_prologue"], s["psk"], None if was_initiator else s["res_e"],
                           select is None or select[i], flags)
        assert rc == 0
        out.append(None if f == F.STATUS_ABSENT else f)
    return _side(A, torch, side.name, n, fb, keep), out


def exchange(w, r, mws, mrs, rows, tamper=None):
    """One message on the device and in the models: w writes rows[i], r reads
    what arrives (tamper(sent rows) may change it in flight).  Where a model
    writes, the device wrote the same bytes; where a model reads a payload,
    the device read the same.  A model of None is a session not in the
    object.  Returns the rows sent."""
    torch, n = w.torch, w.n
    plen = len(rows[0])
    assert w.overhead == r.overhead, ("overheads", w.overhead, r.overhead)
    mlen = plen + w.overhead
    payload = Buf(torch, n, max(plen, 1), [p or b"\0" for p in rows])
    msg = Buf(torch, n, mlen)
    rc = w.write(payload, plen, msg)
    assert rc == 0, ("write", hex(rc))
    sent = msg.read()
    delivered = sent
    if tamper:
        delivered = tamper(sent)
        msg = Buf(torch, n, mlen, delivered)
    got = Buf(torch, n, max(plen, 1))
    rc = r.read(msg, mlen, got)
    assert rc == 0, ("read", hex(rc))
    back = [g[:plen] for g in got.read()]
    for i in range(n):
        want = mws[i].write(rows[i]) if mws[i] is not None else None
        if want is not None:
            assert sent[i] == want, ("message of session", i)
        if mrs[i] is not None:
            pl = mrs[i].read(delivered[i])
            if pl is not None:
                assert pl == rows[i] and back[i] == pl, ("payload of session", i)
    return sent


def split(side):
    """Side.split that also keeps the hash tensor: (k1, k2, h rows)"""
    hl = M.HASH_LEN[M.parse_name(side.name)[1]["hash"]]
    side.hl, side.hh = hl, packed(side.torch, side.n, hl)
    side.k1, side.k2 = packed(side.torch, side.n, 32), packed(side.torch, side.n, 32)
    rc = side.A.dev_handshake_split(side.hs, k1=side.k1.data_ptr(), k2=side.k2.data_ptr(),
                                    handshake_hash=side.hh.data_ptr(), stream=side.sp)
    assert rc == 0, ("split", hex(rc))
    side.torch.cuda.synchronize()
    return packed_rows(side.k1, side.n, 32), packed_rows(side.k2, side.n, 32), packed_rows(side.hh, side.n, hl)


def model_status(models):
    return [F.STATUS_ABSENT if m is None else m.status for m in models]


def model_split(m, hl):
    return m.split() if m is not None else (bytes(32), bytes(32), None)


def merge(hs_side, fb_side):
    """_fallback_merge into hs_side's split, as it lies: (k1, k2, h rows, the
    status bytes); hs_side.merged_status is the device array for _set_keys"""
    torch, n = hs_side.torch, hs_side.n
    st = packed(torch, n, 1)
    rc = hs_side.A.dev_handshake_fallback_merge(
        fb_side.hs, hs_status=hs_side.A.dev_handshake_status(hs_side.hs), k1=hs_side.k1.data_ptr(),
        k2=hs_side.k2.data_ptr(), fb_k1=fb_side.k1.data_ptr(), fb_k2=fb_side.k2.data_ptr(), h=hs_side.hh.data_ptr(),
        fb_h=fb_side.hh.data_ptr(), status=st.data_ptr(), stream=hs_side.sp)
    assert rc == 0, ("merge", hex(rc))
    torch.cuda.synchronize()
    hs_side.merged_status = st
    return (packed_rows(hs_side.k1, n, 32), packed_rows(hs_side.k2, n, 32), packed_rows(hs_side.hh, n, hs_side.hl),
            [r[0] for r in packed_rows(st, n, 1)])
