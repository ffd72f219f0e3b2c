"""Which geometric case of a batch kernel a record's length puts it in.

Every batch kernel cuts a record into 64-byte ChaCha units or 16-byte GHASH
blocks and deals them to 1..64 lanes; the record's length decides which lane
starts the chain, absorbs the AD or holds the tail, how many Poly1305 blocks
the tail has, and which power of r or H each lane is scaled by.  This module
restates that partition arithmetic — the kernels' own lines, named at each
function — in plain Python integers (host only, no GPU, no numpy), gives each
family's universe of cases over a stated length range, and derives the length
lists the GPU sweep runs (tests/test_gpu_length_classes.py): the first length,
in ascending order, that adds a case not seen before.  Nothing here is picked
by hand; tests/test_length_classes_host.py proves that the lists reach what
they claim and counts how little the older hand-written lists reached.

The resident single-record worker (worker_chacha.h, aead_worker in
worker.hip) has its own section at the end: its two ChaChaPoly engines and
its transport share none of the batch kernels' arithmetic, and
tests/test_gpu_worker.py runs those lists (tests/worker_mode_check.py
--classes).
"""
from functools import lru_cache

MAX_LEN = 65519  # NOISE_MAX_PAYLOAD_LEN - 16

IL_LANES = (4, 8, 16, 32, 64)
GCM_LANES = (4, 8)
GCM_ADS = (0, 5, 16, 21, 32, 48)
GCM_MAX_LEN = 599


def _tail(length):
    """(J, tail, q, partial): 64-byte units, bytes of the last one, its
    Poly1305 blocks, and whether its last block is short."""
    J = (length + 63) // 64
    tail = length - 64 * (J - 1) if J else 0
    return J, tail, (tail + 15) // 16, tail % 16 != 0


# ------------------------------------------------ interleaved ChaChaPoly

def il(K, length):
    """chachapoly.hip group_ctx<K>: J + 1 blocks (the key block first) are
    dealt end-aligned to K lanes over `steps` steps; o = the padding slots in
    front (lane o holds the key block, lane (o + 1) % K unit 0 and the AD —
    il_poly_setup), q = the tail's Poly1305 blocks (poly_powers' Q = r^(q+2),
    poly_tree_close's rq), steps 1 / 2 / 3+ = no jump (and, K >= 16, the
    tree close) / one r^(4K-3) jump / repeated jumps; a short last block is
    masked (mask_unit) and stored by another route (last_unit_out)."""
    J, _tail_bytes, q, partial = _tail(length)
    nblk = J + 1
    steps = (nblk + K - 1) // K
    o = steps * K - nblk
    return (o, q, min(steps, 3), partial)


def il_steps(K, length):
    return ((length + 63) // 64 + 1 + K - 1) // K


def il_range(K):
    return range(0, 3 * 64 * K + 64 + 1)


# --------------------------------------------------- one lane per record

def solo(length):
    """chachapoly.hip solo_rec and solo_pass: S = ceil(J / 2) steps of two
    units; J odd = the last step holds one unit (solo_dma's `off >= lim`
    re-read of the second), S 1 / 2 / 3+ = the first tile only / both tiles /
    the steady state (a tile refilled while the other is stored); q and a
    short last block as above."""
    J, _tail_bytes, q, partial = _tail(length)
    return (J % 2, min((J + 1) // 2, 3), q, partial)


# ------------------------------------------------------------- segmented

SEG_TARGET, SEG_KMAX = 32, 16
SEG_LANES = (1, 2, 4, 8, 16)


def seg_k_of(J):
    """chachapoly_seg.hip seg_k_of"""
    B, K = J + 1, 1
    while K < SEG_KMAX and (B + K - 1) // K > SEG_TARGET:
        K <<= 1
    return K


def seg_lanes(K, length):
    """chachapoly_seg.hip seg_blocks: (per, [nb of lane 0..K-1])"""
    J = (length + 63) // 64
    B = J + 1
    per = (B + K - 1) // K
    c = (per + 1) & ~1
    return per, [min(c, B - k * c) if B > k * c else 0 for k in range(K)]


def seg(K, length):
    """chachapoly_seg.hip seg_blocks / seg_suffix / seg_combine: each lane
    takes c = per rounded up to even blocks, so per odd = the last lanes run
    short or empty; the lanes with nb == 0 (none, one, more) neither hold r^e
    nor DMA; the last non-empty lane holds the tail after nb - 1 other blocks
    (1: the tail or the key block alone; 2; an odd or an even count of two-
    block steps beyond); q = the tail's part of every other lane's suffix
    exponent 4 (J - 1 - end) + q."""
    J, _tail_bytes, q, partial = _tail(length)
    per, nbs = seg_lanes(K, length)
    empty = sum(1 for nb in nbs if nb == 0)
    last = [nb for nb in nbs if nb][-1]
    kind = last if last <= 2 else (3 if last % 2 else 4)
    return (K, per % 2, min(empty, 2), kind, q, partial)


def seg_ragged(length):
    return seg(seg_k_of((length + 63) // 64), length)


# --------------------------------------------------------------- AES-GCM

def gcm(K, length, ad_len):
    """aesgcm.hip gcm_record_staged (and gcm_lane, gcm_uniform's body): the
    n = A + M + 1 GHASH blocks are dealt end-aligned, lane l starting at
    c0 = (l + n) % K and scaled by H^(K - l) (gh_scale's K - 1 - l), over
    ceil(n / K) rounds; M == 0 = no CT block; the seal's tag store takes one
    of three routes (len % 16 == 0, len % 8 == 0, bytes); the AD is absent,
    whole blocks, or ends in a short block."""
    A, M = (ad_len + 15) // 16, (length + 15) // 16
    n = A + M + 1
    store = 0 if length % 16 == 0 else (1 if length % 8 == 0 else 2)
    ad_kind = 0 if ad_len == 0 else (1 if ad_len % 16 == 0 else 2)
    return (n % K, min((n + K - 1) // K, 3), M == 0, store, ad_kind)


def gcm_early(ct):
    """aesgcm.hip gcm_wide_record: EARLY = 256 - GH, GH = 64 GHASH threads
    under the constant-time GHASH, 16 * 8 with the tables"""
    return 192 if ct else 128


def gcm_wide(length, ad_len, ct):
    """aesgcm.hip gcm_wide_record (8 GHASH chains): the open's waves beside
    GHASH compute the first EARLY key-stream blocks (`early = v <= M &&
    v < EARLY`, the rest by `for (b = EARLY - 1 + t; b < M; b += 256)`), and
    the seal's `for (v = t; v <= M; v += 256)` takes a second round from
    M = 256."""
    M = (length + 15) // 16
    e = gcm_early(ct)
    return gcm(8, length, ad_len) + ((M > e) - (M < e), M >= 256)


def gcm_wide_boundary(ct):
    """the lengths 16 M and 16 M - 9 around EARLY and the second round"""
    e = gcm_early(ct)
    return sorted({x for M in (e - 1, e, e + 1, 255, 256, 257) for x in (16 * M - 9, 16 * M)})


# -------------------------------------------- universes and covering lists

def universe(case, items):
    """the set of cases `items` reaches"""
    return {case(x) for x in items}


def covering(case, items):
    """the items, in order, that each add a case not seen before"""
    seen, out = set(), []
    for x in items:
        c = case(x)
        if c not in seen:
            seen.add(c)
            out.append(x)
    return out


def il_marginals(K, length):
    """what the `reduced` list covers: the pair (o, min(steps, 2)) — which
    lane holds the key block and the AD, with and without a jump — and the
    triple (q, partial, min(steps, 3)), the one-step triples once for a record
    of one unit and once for a longer one: q reaches the tag only through the
    scale of the full units before the tail (poly_powers' Q, poly_tree_close's
    rq: "any value when there is no full unit"), so a one-unit record alone
    would leave r^(q+2) of the one-step close unchecked."""
    o, q, steps, partial = il(K, length)
    return ("lane", o, min(steps, 2)), ("tail", q, partial, steps, length > 64)


def _gcm_items():
    return [(L, a) for L in range(GCM_MAX_LEN + 1) for a in GCM_ADS]


@lru_cache(maxsize=None)
def full(family, K=0, ct=False):
    """One length (gcm: one (len, ad_len)) per case of the family's universe:
    il over 0 .. 3*64*K + 64; solo, seg (uniform, K = 2) and seg_ragged
    (K = seg_k_of(J)) over 0 .. 65519; gcm over 0 .. 599 x GCM_ADS; gcm_wide
    the K = 8 list with the boundary lengths (no AD, and 21 bytes) on top;
    the resident worker's wfast, wmulti and wtransport (K = the placement)
    as _worker_full() says."""
    if family == "il":
        return tuple(covering(lambda L: il(K, L), il_range(K)))
    if family == "solo":
        return tuple(covering(solo, range(MAX_LEN + 1)))
    if family == "seg":
        return tuple(covering(lambda L: seg(K, L), range(MAX_LEN + 1)))
    if family == "seg_ragged":
        return tuple(covering(seg_ragged, range(MAX_LEN + 1)))
    if family == "gcm":
        return tuple(covering(lambda x: gcm(K, *x), _gcm_items()))
    if family == "gcm_wide":
        # every boundary length is kept, also where two of them share a case
        return full("gcm", 8) + tuple((L, a) for L in gcm_wide_boundary(ct) for a in (0, 21))
    if family in ("wfast", "wmulti", "wtransport"):
        return _worker_full(family, K)  # K: the placement (wtransport)
    raise ValueError(family)


@lru_cache(maxsize=None)
def cases(family, K=0, ct=False):
    """the family's universe (what full() covers, by construction of
    covering(); tests/test_length_classes_host.py recounts it directly)"""
    f = {"il": lambda L: il(K, L), "solo": solo, "seg": lambda L: seg(K, L), "seg_ragged": seg_ragged,
         "gcm": lambda x: gcm(K, *x), "gcm_wide": lambda x: gcm_wide(x[0], x[1], ct),
         "wfast": lambda x: wfast(*x), "wmulti": None, "wtransport": lambda x: wtransport(K, *x)}[family]
    if family in _WORKER_MARGINALS:  # families of marginals: their union
        return frozenset(m for x in full(family, K) for m in _WORKER_MARGINALS[family](K, x))
    return frozenset(f(x) for x in full(family, K, ct if family.startswith("gcm") else False))


@lru_cache(maxsize=None)
def reduced(K):
    """The uniform interleaved kernels take one length per launch: the
    lengths, ascending, that each add a value of one of il_marginals()."""
    seen, out = set(), []
    for L in il_range(K):
        new = set(il_marginals(K, L)) - seen
        if new:
            seen |= new
            out.append(L)
    return tuple(out)


def with_ad(lengths):
    """Each length once without AD and once with an AD length cycling through
    1, 16, 17, 48 (the AD lane depends on o): [(len, ad_len)]."""
    cyc = (1, 16, 17, 48)
    return [(L, 0) for L in lengths] + [(L, cyc[i % 4]) for i, L in enumerate(lengths)]


# ------------------------------------------- the resident worker (one record)
#
# The single-record worker behind noise_cipherstate_encrypt_with_ad /
# _decrypt_with_ad shares none of the partition arithmetic above: its two
# ChaChaPoly engines (worker_chacha.h) and its transport (aead_worker in
# worker.hip, worker_proto.h) are restated here the same way.

WORKER_ADS = (0, 1, 16, 17, 48, 49, 255, 256)  # none, short, whole, 256-block corner, WORKER_MAX_AD
WFAST_MAX_LEN = 4032                           # 63 units: WFAST_BLOCKS - 1
WORKER_HEAD = {0: 3072, 1: 2048}               # worker_proto.h WORKER_HEAD, VWORKER_HEAD
WORKER_CHUNK = {0: 12, 1: 8}                   # WCHUNK_BYTES, VCHUNK_BYTES
WORKER_STRIDE = 256                            # 16-byte pieces per round of the tail and result loops


def _poly_blocks(length, ad_len):
    """(a, m, n): AD blocks, CT blocks and all Poly1305 blocks with the
    length block (worker_chacha.h: `n = a + m + 1` in both engines)"""
    a, m = (ad_len + 15) // 16, (length + 15) // 16
    return a, m, a + m + 1


def _pow2(n):
    """worker_chacha.h: N = n <= 1 ? 1 : 1 << (32 - clz(n - 1))"""
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def _ad_kind(ad_len):
    return 0 if ad_len == 0 else (1 if ad_len % 16 == 0 else 2)


def worker_fast_fits(length, ad_len):
    """worker_chacha.h worker_fast_fits: blocks = J + 1 <= WFAST_BLOCKS (64)
    and n <= 256"""
    return (length + 63) // 64 + 1 <= 64 and _poly_blocks(length, ad_len)[2] <= 256


def wfast(length, ad_len):
    """worker_chacha.h worker_chacha_fast: the n Poly1305 blocks sit right-
    justified in N = 2^ceil(log2 n) lanes (`i = t - (N - n)`) and tree_level
    sums them at levels 1, 2, 4, 8 (DPP), 16, 32 (shuffle), 64, 128 (LDS),
    squaring mP only while 2L < N.  fill: 0 = every lane holds a block
    (n == N), 1 = one block past the half (n == N/2 + 1: the most empty
    leading lanes), 2 = between; the AD absent / whole blocks / ending short
    (lds_block's mask); q = Poly1305 blocks of the last 64-byte unit (the
    ChaCha quad `q <= J` that is partly used), 0 for an empty record; a short
    last block."""
    _a, _m, n = _poly_blocks(length, ad_len)
    N = _pow2(n)
    fill = 0 if n == N else (1 if n == N // 2 + 1 else 2)
    _J, _tail_bytes, q, partial = _tail(length)
    return (N.bit_length() - 1, fill, _ad_kind(ad_len), q, partial)


def wmulti_geometry(length, ad_len):
    """worker_chacha.h worker_chacha_multi: (J, P, n, G, NL, pad) —
    P = ceil((J + 1) / 64) ChaCha passes, G = ceil(n / 256) Horner blocks per
    lane over NL = ceil(n / G) lanes, pad = NL G - n holes leading chunk 0."""
    J = (length + 63) // 64
    _a, _m, n = _poly_blocks(length, ad_len)
    G = (n + 255) // 256
    NL = (n + G - 1) // G
    return J, (J + 1 + 63) // 64, n, G, NL, NL * G - n


def wmulti(length, ad_len):
    """worker_chacha_multi's three marginals:
    ("chunk", G, pad class, NL == 256): the chunk loop's `idx < 0` skips
    pad = 0 / some / G - 1 holes (G - 1: chunk 0 holds one block), R = r^G by
    the square-and-multiply over G's bits, and the tree over NL lanes reaches
    level 128 fully only at NL == 256;
    ("pass", P, last-pass class): multi_xor_passes takes passes 1.. two at a
    time (chacha_quad_x2 while `p + 1 < P`) and a single one when P is even;
    the last pass holds blocks 64 (P - 1) .. J: one block on quad 0
    (J % 64 == 0), all 64 (J % 64 == 63) or some;
    ("tail", AD kind, short last block, q): as for the fast path."""
    J, P, _n, G, NL, pad = wmulti_geometry(length, ad_len)
    padc = 0 if pad == 0 else (2 if pad == G - 1 else 1)
    last = 0 if J % 64 == 0 else (2 if J % 64 == 63 else 1)
    _J, _tail_bytes, q, partial = _tail(length)
    return (("chunk", G, padc, NL == 256), ("pass", P, last), ("tail", _ad_kind(ad_len), partial, q))


def wmulti_flips(length, ad_len):
    """Where a flipped bit lands in (0) chunk 0, (1) the last chunk and (2) a
    block of the last ChaCha pass of a multi-path record, each as (field,
    lo, hi): a byte range of the "ad", the "ct" or the "tag".  Chunk 0 holds
    the Poly1305 blocks 0 .. G - pad - 1 (the AD's first, else the record's);
    the last chunk the record's blocks m - G + 1 .. m - 1 before the length
    block (with G == 1 the length block alone: the tag stands in for it, the
    chunk's value meets nothing else before the comparison); the last pass
    the units max(64 (P - 1), 1) .. J."""
    J, P, _n, G, _NL, pad = wmulti_geometry(length, ad_len)
    _a, m, _n = _poly_blocks(length, ad_len)
    first = 16 * (G - pad)
    c0 = ("ad", 0, min(ad_len, first)) if ad_len else ("ct", 0, min(length, first))
    last = ("ct", 16 * (m - G + 1), length) if G > 1 else ("tag", 0, 16)
    return (c0, last, ("ct", 64 * (max(64 * (P - 1), 1) - 1), length))


def _pieces(nbytes):
    """the 16-byte pieces a loop `for (o = 16 t; o < nbytes; o += 16 * 256)`
    moves: (none / one round of the 256 threads / a second stride, last piece
    short)"""
    k = (nbytes + 15) // 16
    return (0 if k == 0 else (1 if k <= WORKER_STRIDE else 2), nbytes % 16 != 0)


def wtransport(vram, op, length, ad_len):
    """worker.hip aead_worker (restating worker_proto.h stream_total,
    chunk_fresh, chunk_unpack): the stream key || AD padded to 16 || record
    [|| tag for open] of `total` bytes; its first `head` bytes arrive as
    chunks of 12 (host memory) or 8 (device memory) stream bytes, the rest
    raw in 16-byte pieces, 256 per round; the result (len + 16 sealed, len
    opened) leaves in the same rounds.  The case: (below / equal / above the
    head, total % chunk below the head — the last chunk's bytes past the
    stream — else None, the raw tail's _pieces(), the result's _pieces())."""
    total = 32 + ((ad_len + 15) & ~15) + length + (16 if op else 0)
    head, chunk = WORKER_HEAD[vram], WORKER_CHUNK[vram]
    return ((total > head) - (total < head), total % chunk if total < head else None) \
        + _pieces(max(total - head, 0)) + _pieces(length if op else length + 16)


def _worker_items(fits, max_len):
    return [(L, a) for L in range(max_len + 1) for a in WORKER_ADS if worker_fast_fits(L, a) == fits]


def _marginal_covering(case, items):
    """the items, in order, that each add a marginal not seen before"""
    seen, out = set(), []
    for x in items:
        new = set(case(x)) - seen
        if new:
            seen |= new
            out.append(x)
    return out


@lru_cache(maxsize=None)
def _worker_full(family, vram=0):
    """full() of the worker's families: "wfast" one (len, ad_len) per case over
    0 .. 4032 x WORKER_ADS where the record fits; "wmulti" the (len, ad_len)
    that each add a marginal over every record that does not fit up to 65519;
    "wtransport" one (op, len, ad_len) per case of the placement, over
    0 .. 8192 (both loops' second stride starts below it) and AD 0 and 17."""
    if family == "wfast":
        return tuple(covering(lambda x: wfast(*x), _worker_items(True, WFAST_MAX_LEN)))
    if family == "wmulti":
        return tuple(_marginal_covering(lambda x: wmulti(*x), _worker_items(False, MAX_LEN)))
    if family == "wtransport":
        return tuple(covering(lambda x: wtransport(vram, *x), _wtransport_items()))
    raise ValueError(family)


def _wtransport_items():
    return [(op, L, a) for L in range(8192 + 1) for a in (0, 17) for op in (0, 1)]


_WORKER_MARGINALS = {"wmulti": lambda _vram, x: wmulti(*x)}


def wfast_border():
    """worker_fast_fits's border: for each AD length the longest record that
    fits and the next one (which does not), and, where the Poly1305 limit
    binds first, the 63-unit record as well (4032 bytes with 48 bytes of AD is
    n = 256 and fits, with 49 it is n = 257: G = 2, pad = 1 — the corner where
    both limits meet); every one kept: [(len, ad_len)]"""
    out = []
    for a in WORKER_ADS:
        L = max(L for L in range(WFAST_MAX_LEN + 1) if worker_fast_fits(L, a))
        out += [(L, a), (L + 1, a)]
        if L < WFAST_MAX_LEN:
            out.append((WFAST_MAX_LEN, a))
    return out
