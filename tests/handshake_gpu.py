"""Device handshake batches beside the model of tests/handshake_model.py: the
canary-guarded device buffers, one noise_aead_dev_handshake_* object per side,
and a whole handshake of both sides checked message by message.  Importable
without pytest and without torch (the callers pass torch in)."""
import numpy as np

import handshake_model as M
from gpu_support import peek

CANARY = 0xEE


def basic_vector(name):
    return next(v for v in M.load_vectors("noise-c-basic.txt.gz") if v["name"] == name)


class Buf:
    """n rows of `width` bytes on the device, `stride` apart (0: one row for
    all) from byte 1 of a canary-filled tensor."""

    def __init__(self, torch, n, width, rows=None, stride=None):
        self.torch, self.n, self.width = torch, n, width
        self.stride = width + 5 if stride is None else stride
        self.count = n if self.stride else 1
        host = np.full(1 + (self.count - 1) * self.stride + width + 9, CANARY, dtype=np.uint8)
        if rows is not None:
            for i in range(self.count):
                assert len(rows[i]) == width, ("row", i, "has", len(rows[i]), "bytes, the slot", width)
                host[1 + i * self.stride: 1 + i * self.stride + width] = np.frombuffer(rows[i], dtype=np.uint8)
        self.dev = torch.from_numpy(host).cuda()
        self.ptr = self.dev.data_ptr() + 1

    def read(self):
        """the rows; checks every byte between and around them"""
        h = self.dev.cpu().numpy()
        mask = np.ones(len(h), dtype=bool)
        rows = []
        for i in range(self.count):
            lo = 1 + i * self.stride
            rows.append(h[lo:lo + self.width].tobytes())
            mask[lo:lo + self.width] = False
        assert (h[mask] == CANARY).all(), "wrote outside a slot"
        return rows


def packed(torch, n, width):
    return torch.full((n * width + 64,), CANARY, dtype=torch.uint8, device="cuda")


def packed_rows(t, n, width):
    h = t.cpu().numpy()
    assert (h[n * width:] == CANARY).all(), "wrote past a packed output"
    return [h[i * width:(i + 1) * width].tobytes() for i in range(n)]


def make_sessions(v, n, seed, shared=False):
    """Session 0: the vector's keys, prologue and PSK; the others seeded
    random ones (the same for every name of a seed, so the ladder results are
    shared).  shared: one responder static key and one prologue for all."""
    def hx(key):
        return bytes.fromhex(v[key]) if key in v else None
    rng = np.random.default_rng(seed)
    prologue = hx("init_prologue") or b""
    assert prologue == (hx("resp_prologue") or b""), (v["name"], "the two prologues differ")
    out = [dict(ini_s=hx("init_static"), ini_e=hx("init_ephemeral"), res_s=hx("resp_static"),
                res_e=hx("resp_ephemeral"), psk=hx("init_psk"), prologue=prologue)]
    for _ in range(1, n):
        draw = {k: rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for k in ("ini_s", "ini_e", "res_s", "res_e", "psk")}
        draw["prologue"] = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()[:len(prologue)]
        s = {k: (draw[k] if out[0][k] is not None else None) for k in draw}
        if shared:
            s["res_s"], s["prologue"] = out[0]["res_s"], prologue
        out.append(s)
    return out


def model_pair(orc, v, s):
    ini_rs = M.dh_base(s["res_s"]) if "init_remote_static" in v else None
    res_rs = M.dh_base(s["ini_s"]) if "resp_remote_static" in v else None
    return (M.Session(orc, v["name"], True, s["prologue"], s["psk"], s["ini_s"], s["ini_e"], ini_rs),
            M.Session(orc, v["name"], False, s["prologue"], s["psk"], s["res_s"], s["res_e"], res_rs))


class Side:
    """One device handshake object with the device copies of its inputs."""

    def __init__(self, A, torch, v, sess, initiator, shared=False, n=None):
        self.A, self.torch, self.name = A, torch, v["name"]
        n = len(sess) if n is None else n
        me, other = ("ini", "res") if initiator else ("res", "ini")
        kw, self.keep = {}, []

        def give(name, rows, stride=None):
            b = Buf(torch, n, len(rows[0]), rows, stride)
            self.keep.append(b)
            kw[name], kw[name + "_stride"] = b.ptr, b.stride
        rs_key = "init_remote_static" if initiator else "resp_remote_static"
        if sess[0][me + "_s"] is not None:
            give("local_static", [s[me + "_s"] for s in sess], 0 if shared and not initiator else None)
        if sess[0][me + "_e"] is not None:
            give("local_ephemeral", [s[me + "_e"] for s in sess])
        if rs_key in v:
            give("remote_static", [M.dh_base(s[other + "_s"]) for s in sess], 0 if shared and initiator else None)
        if sess[0]["psk"] is not None:
            give("psk", [s["psk"] for s in sess])
        if sess[0]["prologue"]:
            give("prologue", [s["prologue"] for s in sess], 0 if shared else None)
            kw["prologue_len"] = len(sess[0]["prologue"])
        self.sp = torch.cuda.current_stream().cuda_stream
        rc, self.hs = A.dev_handshake_new(v["name"], A.ROLE_INITIATOR if initiator else A.ROLE_RESPONDER, n,
                                          stream=self.sp, **kw)
        assert rc == 0, hex(rc)
        self.n = n

    @property
    def action(self):
        return self.A.dev_handshake_get_action(self.hs)

    @property
    def overhead(self):
        return self.A.dev_handshake_overhead(self.hs)

    def write(self, payload: Buf, plen, msg: Buf):
        return self.A.dev_handshake_write_message(self.hs, payload=payload.ptr if plen else 0,
                                                  payload_stride=payload.stride, payload_len=plen, msg=msg.ptr,
                                                  msg_stride=msg.stride, stream=self.sp)

    def read(self, msg: Buf, mlen, payload: Buf):
        return self.A.dev_handshake_read_message(self.hs, msg=msg.ptr, msg_stride=msg.stride, msg_len=mlen,
                                                 payload=payload.ptr if mlen > self.overhead else 0,
                                                 payload_stride=payload.stride, stream=self.sp)

    def split(self):
        """(k1 rows, k2 rows, handshake hash rows)"""
        hl = M.HASH_LEN[M.parse_name(self.name)[1]["hash"]]
        k1, k2, hh = packed(self.torch, self.n, 32), packed(self.torch, self.n, 32), packed(self.torch, self.n, hl)
        rc = self.A.dev_handshake_split(self.hs, k1=k1.data_ptr(), k2=k2.data_ptr(), handshake_hash=hh.data_ptr(),
                                        stream=self.sp)
        assert rc == 0, (self.name, "split", hex(rc))
        self.torch.cuda.synchronize()
        self.k1, self.k2 = k1, k2
        return packed_rows(k1, self.n, 32), packed_rows(k2, self.n, 32), packed_rows(hh, self.n, hl)

    def status(self):
        return list(peek(self.A.dev_handshake_status(self.hs), self.n))

    def remote_static(self):
        raw = peek(self.A.dev_handshake_remote_static(self.hs), self.n * 32)
        return [raw[i * 32:(i + 1) * 32] for i in range(self.n)]

    def free(self):
        rc = self.A.dev_handshake_free(self.hs)
        assert rc == 0, (self.name, "free", hex(rc))
        self.hs = None


def payload_rows(v, j, n, seed):
    """message j's payloads: the vector's for session 0, random ones of the
    same length for the others"""
    p0 = bytes.fromhex(v["messages"][j]["payload"])
    rng = np.random.default_rng(seed * 31 + j)
    return [p0] + [rng.integers(0, 256, max(len(p0), 1), dtype=np.uint8).tobytes()[:len(p0)] for _ in range(1, n)]


def handshake(A, torch, orc, v, sess, shared=False, tamper=None, seed=0):
    """Both device sides through the whole handshake.  Returns what every
    call wrote: msgs[j] and payloads[j] (rows per session), the split rows and
    the statuses of each side, plus the model's sessions.  tamper(j, rows):
    changes to message j in flight (the model is not consulted then)."""
    n = len(sess)
    ini, res = Side(A, torch, v, sess, True, shared), Side(A, torch, v, sess, False, shared)
    models = None if tamper else [model_pair(orc, v, s) for s in sess]
    out = dict(msgs=[], payloads=[], ini=ini, res=res, models=models)
    j = 0
    while ini.action != A.ACTION_SPLIT:
        w, r = (ini, res) if ini.action == A.ACTION_WRITE_MESSAGE else (res, ini)
        assert r.action == A.ACTION_READ_MESSAGE, (v["name"], "message", j, "the reader's action", r.action)
        rows = payload_rows(v, j, n, seed)
        plen = len(rows[0])
        mlen = plen + w.overhead
        assert w.overhead == r.overhead, (v["name"], "message", j, "overheads", w.overhead, r.overhead)
        payload = Buf(torch, n, max(plen, 1), [p or b"\0" for p in rows])
        msg = Buf(torch, n, mlen)
        rc = w.write(payload, plen, msg)
        assert rc == 0, (v["name"], "write of message", j, hex(rc))
        sent = msg.read()
        if tamper:
            changed = tamper(j, sent)
            if changed:
                msg = Buf(torch, n, mlen, changed)
        got = Buf(torch, n, max(plen, 1))
        rc = r.read(msg, mlen, got)
        assert rc == 0, (v["name"], "read of message", j, hex(rc))
        back = [g[:plen] for g in got.read()]
        out["msgs"].append(sent)
        out["payloads"].append(back)
        if models:
            for i, (mi, mr) in enumerate(models):
                mw, mrd = (mi, mr) if w is ini else (mr, mi)
                want = mw.write(rows[i])
                assert sent[i] == want, (v["name"], "message", j, "session", i)
                assert mrd.read(want) == rows[i] and back[i] == rows[i], (v["name"], "payload", j, i)
        j += 1
    assert res.action == A.ACTION_SPLIT, (v["name"], "the responder's action after the messages", res.action)
    out["n_handshake"] = j
    out["ini_split"], out["res_split"] = ini.split(), res.split()
    assert ini.action == res.action == A.ACTION_COMPLETE, (v["name"], "actions after split", ini.action, res.action)
    out["ini_status"], out["res_status"] = ini.status(), res.status()
    return out
