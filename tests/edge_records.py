"""Crafted AEAD records that sit on the arithmetic edges random bytes never reach.

Random test data reaches the Poly1305 final subtraction with probability
5 * 2^-130, a carry through an all-ones word with 2^-32, and a GHASH value of 0
never.  The builders here solve one 16-byte block of a record so that a chosen
intermediate or final value comes out exactly:

ChaChaPoly (r, s = chacha20_block(key, 0, nonce)[:32], r clamped; the Poly1305
input is pad16(AD) || pad16(CT) || le64(|AD|) || le64(L); reference = Python
big integers, h = (h + b + 2^128) * r mod p):
  final     the value before the reduction is v in FINAL_TARGETS
  tagcarry  tag = (v + s) mod 2^128 is T in TAG_TARGETS, v the largest such < p
  prefix    the serial Horner value after one block is v in PREFIX_TARGETS and
            the next block is sixteen 0xFF bytes
AES-GCM (H = AES(key, 0), tag = AES(key, J0) xor GHASH, products through
oracle.gf128_mul, H^-1 = H^(2^128 - 2)):
  ghash_final    the final GHASH is one of GHASH_PATTERNS
  ghash_prefix   one multiplier input Y xor C_j is one of GHASH_PATTERNS
  ghash_pattern  every ciphertext block is one pattern, one block solved so
                 that the final GHASH is an edge too

A solved Poly1305 block must be < 2^128 (about one draw in four): the rest
bytes (and the AD) are redrawn, the solved block moves, and — where a record
has nothing else to vary — the target does, up to MAX_TRIES times.  Pure
Python plus the oracle; every choice comes from random.Random(seed).

Used by tests/test_edge_records_host.py (pins the builders against the oracle
and the reference on the CPU) and tests/test_gpu_edge_values.py.
"""
import hashlib
import random

import numpy as np

CHACHA, AES = 0x4301, 0x4302
P = 2**130 - 5
M128 = 2**128
MAX_TRIES = 64

FINAL_TARGETS = [("0", 0), ("1", 1), ("4", 4), ("p-1", P - 1), ("p-2", P - 2), ("p-5", P - 5),
                 ("2^128-1", M128 - 1), ("2^128", M128), ("2^129", 2**129), ("2^130-6", 2**130 - 6)]
TAG_TARGETS = [("0", 0), ("2^128-1", M128 - 1),
               ("00000000FFFFFFFF x2", 0x00000000FFFFFFFF00000000FFFFFFFF), ("2^96", 2**96)]
PREFIX_TARGETS = [("0", 0), ("4", 4), ("p-1", P - 1)]
POSITIONS = ["first", "middle", "late"]
RESTS = ["random", "ff", "00"]
GHASH_PATTERNS = [("zero", bytes(16)), ("ones", b"\xff" * 16), ("80 00..", b"\x80" + bytes(15)),
                  ("..00 01", bytes(15) + b"\x01"), ("0F..", b"\x0f" * 16), ("F0..", b"\xf0" * 16)]

CHACHA_CLASSES = ("final", "tagcarry", "prefix")
AES_CLASSES = ("ghash_final", "ghash_prefix", "ghash_pattern")


def classes_of(cipher):
    return CHACHA_CLASSES if cipher == CHACHA else AES_CLASSES


def _rbytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


def pad16(b):
    return bytes(b) + bytes(-len(b) % 16)


def _fill(rng, rest, n):
    return _rbytes(rng, n) if rest == "random" else (b"\xff" if rest == "ff" else b"\0") * n


def _positions(n_full, need_next):
    """Indices of the first, a middle and a late full CT block; with
    need_next the block after each must be a full one too."""
    last = n_full - (2 if need_next else 1)
    if last < 0:
        return {}
    return {"first": 0, "middle": last // 2, "late": last}


# ------------------------------------------------------------ Poly1305 side

def poly_key(oracle, key, nonce):
    ks = oracle.chacha20_block(key, 0, nonce)
    r = int.from_bytes(ks[:16], "little") & 0x0ffffffc0ffffffc0ffffffc0fffffff
    return r, int.from_bytes(ks[16:32], "little")


def poly_blocks(ad, ct):
    """The Poly1305 input as integers, each with its 2^128 bit."""
    msg = pad16(ad) + pad16(ct) + len(ad).to_bytes(8, "little") + len(ct).to_bytes(8, "little")
    return [int.from_bytes(msg[i:i + 16], "little") + M128 for i in range(0, len(msg), 16)]


def horner(blocks, r, h=0):
    for b in blocks:
        h = (h + b) * r % P
    return h


def tag_target_value(T, s, drop=0):
    """The largest v < p with (v + s) mod 2^128 == T (drop: the drop-th one
    below it; drop <= 2 always exists)."""
    v = (T - s) % M128 + 3 * M128
    return (v if v < P else v - M128) - drop * M128


def _solve_poly(r, blocks, blk, v, prefix):
    """blocks[blk] (with its 2^128 bit) such that the value after block blk
    (prefix) or after the last block is v; None when it has no 128-bit
    solution."""
    before = horner(blocks[:blk], r)
    if prefix:
        x = v * pow(r, -1, P) - before
    else:
        x = (v - horner(blocks[blk + 1:], r)) * pow(r, -(len(blocks) - blk), P) - before
    c = (x - M128) % P
    return c if c < M128 else None


def chacha_targets(n_full):
    t = [("final", n, v) for n, v in FINAL_TARGETS] + [("tagcarry", n, v) for n, v in TAG_TARGETS]
    if n_full >= 3:
        t += [("prefix", n + "@" + pos, v) for n, v in PREFIX_TARGETS for pos in POSITIONS]
    return t


def craft_chacha(oracle, rng, key, nonce, L, ad_len, targets, rest, free):
    """One record towards targets[0].  key/nonce are kept unless free.
    Returns (key, nonce, ad, ct || tag, label) or None after MAX_TRIES."""
    n_ad, n_full = (ad_len + 15) // 16, L // 16
    solvable = [n_ad + i for i in range(n_full)] or list(range(ad_len // 16))
    if not solvable:
        return None
    vary = free or ad_len > 0 or (rest == "random" and L > 16)
    # a record with nothing to redraw walks the target list instead, and after
    # it the tag targets again with the next smaller v (same tag, one 2^128 less)
    cands = [t + (0,) for t in targets]
    if not vary:
        cands += [t + (d,) for d in (1, 2) for t in targets if t[0] == "tagcarry"]
    for t in range(MAX_TRIES):
        if free and t:
            key, nonce = _rbytes(rng, 32), rng.getrandbits(64) % (2**64 - 1)
        cls, name, val, drop = cands[0] if vary else cands[(t // len(solvable)) % len(cands)]
        r, s = poly_key(oracle, key, nonce)
        if r == 0:
            continue
        ad = _rbytes(rng, ad_len)
        ct = bytearray(_fill(rng, rest, L))
        if cls == "prefix":
            pos = _positions(n_full, True)[name.split("@")[1]]
            if n_ad == 0 and pos == 0:
                pos = 1  # nothing precedes CT block 0: (c + 2^128) r = v has no free byte
            # when nothing else can vary, walk the solved block instead
            pos = pos if vary else 1 + (pos - 1 + t) % (n_full - 2)
            blk = n_ad + pos
            ct[16 * pos + 16:16 * pos + 32] = b"\xff" * 16
            v = val
        else:
            blk = solvable[(t + rng.getrandbits(16)) % len(solvable)] if vary else solvable[t % len(solvable)]
            v = val if cls == "final" else tag_target_value(val, s, drop)
        blocks = poly_blocks(ad, ct)
        c = _solve_poly(r, blocks, blk, v, cls == "prefix")
        if c is None:
            continue
        cb = c.to_bytes(16, "little")
        if blk < n_ad:
            ad = ad[:16 * blk] + cb + ad[16 * blk + 16:]
        else:
            ct[16 * (blk - n_ad):16 * (blk - n_ad) + 16] = cb
        blocks[blk] = c + M128
        tag = ((horner(blocks, r) + s) % M128).to_bytes(16, "little")
        return key, nonce, ad, bytes(ct) + tag, dict(cls=cls, name=name, value=val, blk=blk, rest=rest, drop=drop)
    return None


# --------------------------------------------------------------- GHASH side

class GcmKey:
    """H, H^-1 and E(J0) of one key through the oracle."""

    def __init__(self, oracle, key):
        self.o, self.key = oracle, key
        self.H = oracle.aes256(key, bytes(16))
        # H^-1 = H^(2^128 - 2): bits 1..127 of the exponent set
        inv, sq = None, self.H
        for _ in range(127):
            sq = oracle.gf128_mul(sq, sq)
            inv = sq if inv is None else oracle.gf128_mul(inv, sq)
        self.Hinv = inv

    def ej0(self, nonce):
        return self.o.aes256(self.key, bytes(4) + nonce.to_bytes(8, "big") + b"\0\0\0\1")

    def ghash(self, blocks, y=bytes(16)):
        for b in blocks:
            y = self.o.gf128_mul(xor16(y, b), self.H)
        return y

    def times_hinv(self, x, n):
        for _ in range(n):
            x = self.o.gf128_mul(x, self.Hinv)
        return x


def xor16(a, b):
    return (int.from_bytes(a, "big") ^ int.from_bytes(b, "big")).to_bytes(16, "big")


def ghash_blocks(ad, ct):
    msg = pad16(ad) + pad16(ct) + (8 * len(ad)).to_bytes(8, "big") + (8 * len(ct)).to_bytes(8, "big")
    return [msg[i:i + 16] for i in range(0, len(msg), 16)]


def aes_targets(n_full):
    t = [("ghash_final", n, p) for n, p in GHASH_PATTERNS] + [("ghash_prefix", n, p) for n, p in GHASH_PATTERNS]
    if n_full >= 2:
        t += [("ghash_pattern", n, p) for n, p in GHASH_PATTERNS]
    return t


def craft_aes(gk, rng, nonce, L, ad_len, target, rest, salt):
    """One AES-GCM record; always solves.  Returns (ad, ct || tag, label) or
    None when the record has no full block to solve."""
    cls, name, pat = target
    n_ad, n_full = (ad_len + 15) // 16, L // 16
    pos = _positions(n_full, False)
    ad = _rbytes(rng, ad_len)
    if n_full:
        blk = n_ad + pos[POSITIONS[salt % 3]]
    elif ad_len >= 16:
        blk = 0
    else:
        return None
    final = pat
    if cls == "ghash_pattern":
        ct = bytearray((pat * (L // 16 + 1))[:L])
        rest = name
        final = GHASH_PATTERNS[salt % len(GHASH_PATTERNS)][1]
    else:
        ct = bytearray(_fill(rng, rest, L))
    blocks = ghash_blocks(ad, ct)
    before = gk.ghash(blocks[:blk])
    if cls == "ghash_prefix":
        c = xor16(pat, before)
    else:
        after = gk.ghash(blocks[blk + 1:])
        c = xor16(gk.times_hinv(xor16(final, after), len(blocks) - blk), before)
    if blk < n_ad:
        ad = ad[:16 * blk] + c + ad[16 * blk + 16:]
    else:
        ct[16 * (blk - n_ad):16 * (blk - n_ad) + 16] = c
    blocks[blk] = c
    tag = xor16(gk.ej0(nonce), gk.ghash(blocks))
    label = dict(cls=cls, name=name, value=pat, blk=blk, rest=rest, final=final if cls != "ghash_prefix" else None)
    return ad, bytes(ct) + tag, label


# ------------------------------------------------------------------ batches

class Batch:
    """records[i] = dict(key, nonce, ad, sealed = CT || tag, pt, label);
    label is None for a record left uncrafted (an ordinary sealed record)."""

    def __init__(self, cipher, records, keys, key_idx, nonce_base=None, rps=0):
        self.cipher, self.records, self.keys, self.key_idx = cipher, records, keys, key_idx
        self.nonce_base, self.rps = nonce_base, rps
        self.count = len(records)
        self.labels = [r["label"] for r in records]
        self.uncrafted = [i for i, r in enumerate(records) if r["label"] is None]

    def classes(self):
        return {l["cls"] for l in self.labels if l}

    def names(self, cls):
        return {l["name"] for l in self.labels if l and l["cls"] == cls}

    def strided(self, field, stride, fill=0, slack=64):
        """The records' `field` bytes laid out at i * stride."""
        return layout(self.records, field, [i * stride for i in range(self.count)],
                      self.count * stride + slack, fill)

    def digest(self):
        h = hashlib.sha256()
        for r in self.records:
            h.update(r["key"] + r["nonce"].to_bytes(8, "little") + r["ad"] + r["sealed"] + r["pt"])
        return h.hexdigest()


def _finish(oracle, cipher, rng, key, nonce, L, ad_len, made):
    """The record dict of a crafted result, or an ordinary sealed record."""
    if made is None:
        ad, pt = _rbytes(rng, ad_len), _rbytes(rng, L)
        return dict(key=key, nonce=nonce, ad=ad, pt=pt, label=None,
                    sealed=oracle.encrypt(cipher, key, nonce, pt, ad))
    key, nonce, ad, sealed, label = made
    rc, pt = oracle.decrypt(cipher, key, nonce, sealed, ad)
    assert rc == 0, ("the oracle rejects a crafted record", label)
    return dict(key=key, nonce=nonce, ad=ad, pt=pt, label=label, sealed=sealed)


def _plan(rng, cipher, L, count):
    """Target and rest pattern of every record: each target in turn, in a
    seeded order, against each rest pattern."""
    targets = chacha_targets(L // 16) if cipher == CHACHA else aes_targets(L // 16)
    order = list(range(len(targets)))
    rng.shuffle(order)
    return [(order[i % len(order)], RESTS[(i % len(order) + i // len(order)) % 3]) for i in range(count)], targets


def nonce_bases(rng, count, rps):
    """(hi << 32) | (2^32 - d): the low word carries inside every state's run
    (d in [1, run - 1], never on a wave boundary); state 0 has hi = 0xFFFFFFFE."""
    S = (count + rps - 1) // rps
    out = []
    for s in range(S):
        run = min(rps, count - s * rps)
        d = 1 + rng.randrange(max(1, run - 1))
        if run > 64 and d % 64 == 0:
            d += 5
        hi = 0xFFFFFFFE if s == 0 else rng.getrandbits(32) % 0xFFFFFFFE
        out.append((hi << 32) | (2**32 - d))
        assert out[-1] + rps < 2**64
    return np.array(out, dtype=np.uint64)


_CACHE = {}


def uniform_batch(oracle, cipher, seed, count, rps, L, ad_len=0):
    """count records of L bytes (ad_len bytes of AD each), rps per state:
    fixed keys and nonce bases, crafted by redrawing rest bytes only."""
    k = ("u", cipher, seed, count, rps, L, ad_len)
    if k in _CACHE:
        return _CACHE[k]
    rng = random.Random(seed * 1000003 + cipher + 7 * L + 131 * ad_len + 17 * count + rps)
    S = (count + rps - 1) // rps
    keys = [_rbytes(rng, 32) for _ in range(S)]
    nb = nonce_bases(rng, count, rps)
    plan, targets = _plan(rng, cipher, L, count)
    gks = {}
    records = []
    for i, (ti, rest) in enumerate(plan):
        s = i // rps
        key, nonce = keys[s], int(nb[s]) + i % rps
        if cipher == CHACHA:
            made = craft_chacha(oracle, rng, key, nonce, L, ad_len, targets[ti:] + targets[:ti], rest, False)
        else:
            if s not in gks:
                gks[s] = GcmKey(oracle, key)
            m = craft_aes(gks[s], rng, nonce, L, ad_len, targets[ti], rest, i)
            made = m and (key, nonce) + m
        records.append(_finish(oracle, cipher, rng, key, nonce, L, ad_len, made))
    b = Batch(cipher, records, np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(S, 32).copy(),
              np.arange(count) // rps, nb, rps)
    b.L, b.ad_len = L, ad_len
    _CACHE[k] = b
    return b


def ragged_batch(oracle, cipher, seed, lens, ad_lens):
    """One record per (lens[i], ad_lens[i]), each with a key and a nonce of its
    own (records[i]["key"] is keys[i]), both redrawn until the target solves."""
    k = ("r", cipher, seed, tuple(lens), tuple(ad_lens))
    if k in _CACHE:
        return _CACHE[k]
    rng = random.Random(seed * 1000003 + cipher + 3)
    records = []
    for i, (L, A) in enumerate(zip(lens, ad_lens)):
        L, A = int(L), int(A)
        key, nonce = _rbytes(rng, 32), rng.getrandbits(64) % (2**64 - 1)
        rest = RESTS[(i + i // 7) % 3]
        if cipher == CHACHA:
            targets = chacha_targets(L // 16)
            ti = (5 * i + seed) % len(targets)
            made = craft_chacha(oracle, rng, key, nonce, L, A, targets[ti:] + targets[:ti], rest, True)
        else:
            targets = aes_targets(L // 16)
            m = craft_aes(GcmKey(oracle, key), rng, nonce, L, A, targets[(5 * i + seed) % len(targets)], rest, i)
            made = m and (key, nonce) + m
        if made:
            key, nonce = made[0], made[1]
        records.append(_finish(oracle, cipher, rng, key, nonce, L, A, made))
    keys = np.frombuffer(b"".join(r["key"] for r in records), dtype=np.uint8).reshape(len(records), 32).copy()
    b = Batch(cipher, records, keys, np.arange(len(records)))
    _CACHE[k] = b
    return b


def layout(records, field, offs, total, fill=0):
    """records[i][field] at byte offs[i] of a `total`-byte array of `fill`."""
    out = np.full(total, fill, dtype=np.uint8)
    for r, o in zip(records, offs):
        b = r[field]
        out[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return out


# ---------------------------------------------- the shapes the GPU file uses
# (cipher, count, rps, L, ad_len) of every uniform batch and the length lists
# of every ragged one; tests/test_edge_records_host.py walks them all on the
# CPU first.  A batch whose records have a single full block, no AD and fixed
# keys can only vary the target per record; the targets are multiples of 2^128
# plus a little, so their solutions are correlated and about 1 % of such
# records solve for none of them: those shapes carry a seed picked so that
# every record crafts (the host test fails when one does not).

CHACHA_GENERIC = [(CHACHA, 150, 13, L, A) for L in (16, 17, 64, 1400, 4096) for A in (0, 21)]
CHACHA_STAGED = [(CHACHA, 300, 256, L, A) for L in (16, 100, 1400, 4096) for A in (0, 32)]
CHACHA_SEG2 = [(CHACHA, n, rps, L, 0) for rps in (13, 64) for n in (70, 95) for L in (64, 1400, 4096)]
CHACHA_SOLO = [(CHACHA, 600, 64, 100, 0), (CHACHA, 610, 64, 1400, 0)]
AES_UNIFORM = [(AES, n, rps, L, A) for n, rps in ((150, 13), (300, 256)) for L in (16, 100, 1400, 4096)
               for A in (0, 21)]
UNIFORM_SHAPES = CHACHA_GENERIC + CHACHA_STAGED + CHACHA_SEG2 + CHACHA_SOLO + AES_UNIFORM

SEEDS = {(CHACHA, 150, 13, 16, 0): 13, (CHACHA, 150, 13, 17, 0): 6, (CHACHA, 300, 256, 16, 0): 4}


def shaped(oracle, shape):
    return uniform_batch(oracle, shape[0], SEEDS.get(shape, 1), *shape[1:])


def _ragged_lens(base, n):
    lens = [base[i % len(base)] for i in range(n)]
    ads = [(16, 32, 21, 48)[i % 4] if L == 0 else (0, 0, 5, 32, 16)[(i // 2) % 5] for i, L in enumerate(lens)]
    return lens, ads


RAGGED_SHAPES = {
    # L = 16 and L = 0 with AD (the AD block is the solved one) among the rest
    "chacha": (CHACHA, 7) + _ragged_lens([16, 0, 17, 64, 100, 1400, 0, 16, 48, 4096, 255, 256, 1984], 208),
    "aes": (AES, 7) + _ragged_lens([16, 0, 17, 64, 100, 1400, 0, 16, 48, 4096, 255, 256, 1985], 198),
    # chachapoly_seg_ragged: every ChaChaPoly target at each length
    "seg": (CHACHA, 11, [L for L in (1400, 1984, 1985, 4096, 16384, 65519) for _ in range(23)], [0] * 138),
    # the resident worker: fast path, multi-pass path, gcm_wide_record
    "worker_chacha": (CHACHA, 13, [L for L in (16, 1400, 4032, 4033, 16384) for _ in range(23)],
                      [(0, 13, 32)[i % 3] for i in range(115)]),
    "worker_aes": (AES, 13, [L for L in (16, 1400, 4096) for _ in range(18)], [(0, 13, 32)[i % 3] for i in range(54)]),
    "worker_matrix": (CHACHA, 17, [64, 64], [0, 0]),
    "worker_matrix_aes": (AES, 17, [64, 64], [0, 0]),
}


def ragged_shaped(oracle, name):
    cipher, seed, lens, ads = RAGGED_SHAPES[name]
    return ragged_batch(oracle, cipher, seed, lens, ads)
