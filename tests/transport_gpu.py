"""Device transport objects beside their models: the sessions' streams in one
canary-filled device buffer (Wire), an object of sessions beside
tests/transport_model.py (Side), and an object of slots beside
tests/transport_table_model.py (Table).  Importable without pytest and without
torch (the callers pass torch in)."""
import numpy as np

import transport_model as T
import transport_table_model as M
from gpu_support import dev_bytes, dev_u32, peek_u8, peek_u64, poke_u64, prepared

N = 67
CANARY = 0xEE
LENS = (16, 17, 80, 1416, 65535)
CIPHERS = [T.CHACHAPOLY, T.AESGCM]
PERM = [(29 * j + 5) % N for j in range(N)]  # every slot once, unsorted


def keys_for(seed, n=N):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
            for _ in range(n)]


def plain_streams(seed, n=N, big=True):
    """Seal-ready streams: session i has i % 6 frames, lengths cycling through
    LENS (65535 kept to every third session so that the batch stays small);
    every fifth session ends with one byte of a next header."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        lens = [LENS[(i + 2 * k) % 5] for k in range(i % 6)]
        lens = [L if (L != 65535 or (big and i % 3 == 2)) else 80 for L in lens]
        s = b"".join(T.frame(rng.integers(0, 256, L - 16, dtype=np.uint8).tobytes() + bytes(16)) for L in lens)
        out.append(s + (b"\x07" if i % 5 == 3 else b""))
    return out


def offsets(streams):
    """odd, even and 16-byte aligned offsets in turn, with unequal gaps"""
    offs, cur = [], 1
    for i, s in enumerate(streams):
        cur += (3, 8, 13, 1, 22)[i % 5]
        if i % 3 == 0:
            cur |= 1
        elif i % 3 == 1:
            cur += (cur & 1) + (2 if (cur + (cur & 1)) % 16 == 0 else 0)
        else:
            cur = (cur + 15) & ~15
        offs.append(cur)
        cur += len(s)
    return offs, cur + 9


def total_frames(streams):
    return sum(len(T.walk(s, 0)[0]) for s in streams)


def differing(got, want):
    """where two lists differ, for a failure message: the first few (index, got, want)"""
    return [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4] or (len(got), len(want))


class Wire:
    """The sessions' streams in one canary-filled device buffer."""

    def __init__(self, torch, streams):
        self.torch, self.n = torch, len(streams)
        self.offs, total = offsets(streams)
        assert {o % 2 for o in self.offs} == {0, 1} and any(o % 16 == 0 for o in self.offs) or self.n < 3, \
            ("the offsets are not odd, even and 16-byte aligned in turn", self.offs[:6])
        self.lens = [len(s) for s in streams]
        host = np.full(total, CANARY, dtype=np.uint8)
        for o, s in zip(self.offs, streams):
            host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.dev = torch.from_numpy(host).cuda()
        self.result = torch.full((self.n + 1, 4), 0x55555555, dtype=torch.int32, device="cuda")
        self.pos = [0] * self.n  # bytes of each stream already consumed (the cap tests)

    def call(self, A, fn, tr):
        """one call on what is left of every stream; [(frames, consumed, error)]"""
        torch = self.torch
        off = torch.tensor([o + p for o, p in zip(self.offs, self.pos)] or [0], dtype=torch.int64, device="cuda")
        ln = torch.tensor([l - p for l, p in zip(self.lens, self.pos)] or [0], dtype=torch.int32, device="cuda")
        sp = torch.cuda.current_stream().cuda_stream
        rc = fn(tr, wire=self.dev.data_ptr(), off=off.data_ptr(), length=ln.data_ptr(), result=self.result.data_ptr(),
                stream=sp)
        assert rc == 0, ("the frame call over %d streams" % self.n, hex(rc))
        torch.cuda.synchronize()
        r = self.result.cpu().numpy()
        assert (r[self.n] == 0x55555555).all() and (r[:self.n, 3] == 0).all(), \
            ("result rows: the row past the last, or a fourth word", r[self.n].tolist(), np.nonzero(r[:self.n, 3])[0][:4])
        return [(int(np.uint32(x[0])), int(np.uint32(x[1])), int(x[2])) for x in r[:self.n]]

    def streams(self):
        """every stream as it is now; checks every byte between and around them"""
        h = self.dev.cpu().numpy()
        mask = np.ones(len(h), dtype=bool)
        out = []
        for o, l in zip(self.offs, self.lens):
            out.append(h[o:o + l].tobytes())
            mask[o:o + l] = False
        assert (h[mask] == CANARY).all(), ("wrote outside a stream, at bytes", np.nonzero(mask & (h != CANARY))[0][:4])
        return out

    def rest(self):
        return [s[p:] for s, p in zip(self.streams(), self.pos)]


class Side:
    """One device transport object beside its model sessions."""

    def __init__(self, A, torch, orc, cipher, initiator, keys, max_frames, k1_ptr=None, k2_ptr=None):
        self.A, self.torch, self.n = A, torch, len(keys)
        if k1_ptr is None:
            self.k1 = torch.tensor(list(b"".join(k[0] for k in keys)), dtype=torch.uint8, device="cuda")
            self.k2 = torch.tensor(list(b"".join(k[1] for k in keys)), dtype=torch.uint8, device="cuda")
            k1_ptr, k2_ptr = self.k1.data_ptr(), self.k2.data_ptr()
        rc, self.tr = A.dev_transport_new(cipher, A.ROLE_INITIATOR if initiator else A.ROLE_RESPONDER, self.n, k1=k1_ptr,
                                          k2=k2_ptr, max_frames=max_frames, stream=torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and self.tr, hex(rc)
        self.max_frames = max_frames
        self.model = [T.Session.of_role(orc, cipher, initiator, *k) for k in keys]

    def nonces(self, direction):
        return peek_u64(self.A.dev_transport_nonces(self.tr, direction), self.n)

    def set_nonces(self, direction, values):
        """through the object's own device array, and in the model"""
        cur = self.nonces(direction)
        for i, v in values.items():
            cur[i] = v
            setattr(self.model[i], "recv" if direction else "send", v)
        poke_u64(self.A.dev_transport_nonces(self.tr, direction), cur)

    def run(self, mode, wire: Wire, exact=True):
        """One call on the device and in the model.  exact: every byte, result
        and nonce must equal the model's; else returns both for the caller."""
        fn = getattr(self.A, f"dev_transport_{mode}_frames")
        before = wire.rest()
        want = T.run_batch(self.model, mode, before, self.max_frames)
        got_results = wire.call(self.A, fn, self.tr)
        got = wire.rest()
        for direction, name, attr in ((0, "send nonces", "send"), (1, "receive nonces", "recv")):
            have, model = self.nonces(direction), [getattr(m, attr) for m in self.model]
            assert have == model, (mode, name, differing(have, model))
        assert got_results == [w[1] for w in want], (mode, "results", differing(got_results, [w[1] for w in want]))
        if exact:
            for i in range(self.n):
                assert got[i] == want[i][0], (mode, "stream", i, "of %d bytes differs from the model's" % len(got[i]))
        return got, got_results, want

    def free(self):
        rc = self.A.dev_transport_free(self.tr)
        assert rc == 0, ("dev_transport_free", hex(rc))
        self.tr = None


class Table:
    """One device transport object beside its model: a T.Session per keyed
    slot, None for an unkeyed one (whose nonces the test tracks itself)."""

    def __init__(self, A, torch, orc, cipher, initiator, max_frames, keys=None, n=N):
        self.A, self.torch, self.orc, self.cipher, self.initiator, self.n = A, torch, orc, cipher, initiator, n
        self.max_frames = max_frames
        self.sp = torch.cuda.current_stream().cuda_stream
        role = A.ROLE_INITIATOR if initiator else A.ROLE_RESPONDER
        if keys is None:
            rc, self.tr = A.dev_transport_new_unkeyed(cipher, role, n, max_frames=max_frames, stream=self.sp)
            self.model = [None] * n
        else:
            k1, k2 = dev_bytes(b"".join(k[0] for k in keys)), dev_bytes(b"".join(k[1] for k in keys))
            rc, self.tr = A.dev_transport_new(cipher, role, n, k1=k1.data_ptr(), k2=k2.data_ptr(), max_frames=max_frames,
                                              stream=self.sp)
            torch.cuda.synchronize()
            self.model = [T.Session.of_role(orc, cipher, initiator, *k) for k in keys]
        assert rc == 0 and self.tr, hex(rc)
        self.loose = [[0] * n, [0] * n]  # the nonces of the unkeyed slots

    # ---- what the device holds
    def nonces(self, direction):
        return peek_u64(self.A.dev_transport_nonces(self.tr, direction), self.n)

    def has_key(self):
        return list(peek_u8(self.A.dev_transport_has_key(self.tr), self.n))

    def ctx(self, direction):
        ptr, cb = self.A.debug_transport_ctx(self.tr, direction)
        assert ptr and cb == self.A.dev_ctx_bytes(self.cipher), ("debug_transport_ctx", direction, ptr, cb)
        return peek_u8(ptr, self.n * cb).reshape(self.n, cb)

    # ---- what the model says it holds
    def want_nonces(self, direction):
        return [(m.recv if direction else m.send) if m else self.loose[direction][i] for i, m in enumerate(self.model)]

    def check_state(self):
        have, model = self.has_key(), [1 if m else 0 for m in self.model]
        assert have == model, ("state bytes", differing(have, model))
        for direction, name in ((0, "send nonces"), (1, "receive nonces")):
            have, model = self.nonces(direction), self.want_nonces(direction)
            assert have == model, (name, differing(have, model))

    def check_contexts(self):
        """both context arrays, every byte: prepare of the right key, or zero"""
        for direction, attr in ((0, "send_key"), (1, "recv_key")):
            want = prepared(self.A, self.cipher, [getattr(m, attr) if m else None for m in self.model])
            got = self.ctx(direction)
            assert got.shape == want.shape, ("context array shapes", direction, got.shape, want.shape)
            for i in range(self.n):
                assert (got[i] == want[i]).all(), ("context", direction, i)

    def set_nonces(self, direction, values):
        cur = self.nonces(direction)
        for i, v in values.items():
            cur[i] = v
            if self.model[i]:
                setattr(self.model[i], "recv" if direction else "send", v)
            else:
                self.loose[direction][i] = v
        poke_u64(self.A.dev_transport_nonces(self.tr, direction), cur)

    # ---- the calls
    def set_keys(self, slots, keys, status=None, ptrs=None):
        """entry j: slot slots[j], keys[j] = (k1, k2); status: one byte per entry
        or None.  ptrs = (k1, k2, status) device pointers to use instead of
        copies of these."""
        d_slots = dev_u32(slots)
        if ptrs is None:
            k1, k2 = dev_bytes(b"".join(k[0] for k in keys)), dev_bytes(b"".join(k[1] for k in keys))
            st = dev_bytes(bytes(status)) if status is not None else None
            ptrs = (k1.data_ptr(), k2.data_ptr(), st.data_ptr() if st is not None else 0)
        rc = self.A.dev_transport_set_keys(self.tr, slots=d_slots.data_ptr(), m=len(slots), k1=ptrs[0], k2=ptrs[1],
                                           status=ptrs[2], stream=self.sp)
        assert rc == 0, ("dev_transport_set_keys of %d entries" % len(slots), hex(rc))
        self.torch.cuda.synchronize()
        for j, i in enumerate(slots):
            if i < self.n:
                failed = status is not None and status[j] != 0
                self.model[i] = None if failed else T.Session.of_role(self.orc, self.cipher, self.initiator, *keys[j])
                self.loose[0][i] = self.loose[1][i] = 0

    def clear_keys(self, slots):
        d_slots = dev_u32(slots)
        rc = self.A.dev_transport_clear_keys(self.tr, slots=d_slots.data_ptr(), m=len(slots), stream=self.sp)
        assert rc == 0, ("dev_transport_clear_keys of %d entries" % len(slots), hex(rc))
        self.torch.cuda.synchronize()
        for i in slots:
            if i < self.n:
                self.model[i] = None
                self.loose[0][i] = self.loose[1][i] = 0

    def run(self, mode, wire, slots=None, max_frames=0):
        """One call on the device and in the model: the full call (slots None),
        or the _of call over `slots` under this call's cap.  Every byte, result,
        nonce and state byte must equal the model's."""
        A = self.A
        if slots is None:
            fn, cap = getattr(A, f"dev_transport_{mode}_frames"), self.max_frames
        else:
            of, d_slots = getattr(A, f"dev_transport_{mode}_frames_of"), dev_u32(slots)
            cap = max_frames or self.max_frames

            def fn(tr, **kw):
                return of(tr, slots=d_slots.data_ptr(), m=len(slots), max_frames=max_frames, **kw)
        before = wire.rest()
        want = M.run_table(self.model, mode, before, cap, slots)
        results = wire.call(A, fn, self.tr)
        got = wire.rest()
        assert results == [w[1] for w in want], (mode, "results", differing(results, [w[1] for w in want]))
        for j in range(len(before)):
            assert got[j] == want[j][0], (mode, "stream", j, "of %d bytes differs from the model's" % len(got[j]))
        self.check_state()
        return results

    def free(self):
        rc = self.A.dev_transport_free(self.tr)
        assert rc == 0, ("dev_transport_free", hex(rc))
        self.tr = None
