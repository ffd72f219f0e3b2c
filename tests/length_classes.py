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
    the K = 8 list with the boundary lengths (no AD, and 21 bytes) on top."""
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
    raise ValueError(family)


@lru_cache(maxsize=None)
def cases(family, K=0, ct=False):
    """the family's universe (what full() covers, by construction of
    covering(); tests/test_length_classes_host.py recounts it directly)"""
    f = {"il": lambda L: il(K, L), "solo": solo, "seg": lambda L: seg(K, L), "seg_ragged": seg_ragged,
         "gcm": lambda x: gcm(K, *x), "gcm_wide": lambda x: gcm_wide(x[0], x[1], ct)}[family]
    return frozenset(f(x) for x in full(family, K, ct))


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
