"""Operands that put the X25519 field arithmetic (noise-c_amd/csrc/fe25519.h) on
the carry paths random data never takes, and a classifier that proves they do.

fe25519.h keeps any 256-bit number as a field element (M = 2^256 stands for 38
mod p = 2^255 - 19) and reduces nothing between operations.  Its rare steps —
the second wrap of f25_fold, the second borrow of f25_sub, a freeze argument in
[p, 2^255) or one whose +19 carries back into bit 255 — are each taken by about
one random operand pair in 2^220, so only chosen operands test them.

EDGES is the chosen set E.  vectors(op) is E x E (E for a one-operand
operation) followed by RANDOM_PAIRS seeded random operands.  paths(op, a, b)
restates the operation on Python integers, step by step at the level of whole
256-bit values (not limbs), and names the branches it takes; its value must be
congruent to expected(op, a, b), which tests/test_dh_host.py checks for every
vector.  The same test holds the coverage condition: every name in PATHS[op]
is taken by a vector of E alone, and no random vector takes one of RARE.

Used by tests/test_dh_host.py (the header on the CPU under ASan/UBSan, through
asan/dh_check) and tests/test_gpu_f25.py (noise_aead_debug_f25_op).
"""
import functools
import random

M = 2**256
P = 2**255 - 19
B255 = 2**255
RANDOM_PAIRS = 2000
KMAX = 2**26 - 1  # the largest constant f25_mul_small takes


def _ceil_div(a, b):
    return -(-a // b)


def _edges():
    named = [(str(v), v) for v in (0, 1, 2, 18, 19, 20, 37, 38, 39)]
    named += [("p-1", P - 1), ("p", P), ("p+1", P + 1)]
    named += [("2^255-1", B255 - 1), ("2^255", B255), ("2^255+18", B255 + 18), ("2^255+19", B255 + 19)]
    named += [("2p-1", 2 * P - 1), ("2p", 2 * P), ("2p+1", 2 * P + 1)]
    named += [(f"M-{d}", M - d) for d in (39, 38, 37, 20, 19, 1)]
    named += [("2^32-1", 2**32 - 1), ("2^32", 2**32), ("M-2^32", M - 2**32), ("M-2^224", M - 2**224),
              ("2^224-1", 2**224 - 1)]
    named += [("(M-1)/3", (M - 1) // 3), ("2(M-1)/3", 2 * (M - 1) // 3)]
    # (M - 1) b = b M - b: with b just above k M / 37 the x38 fold of the high
    # half lands the sum just below a multiple of M
    for k in (1, 2, 17, 36, 37):
        c = _ceil_div(k * M, 37)
        named += [(f"ceil({k}M/37)", c), (f"ceil({k}M/37)-1", c - 1)]
    out, seen = [], set()
    for name, v in named:
        if 0 <= v < M and v not in seen:  # 2p = M - 38 and the like come twice, ceil(37M/37) = M is no operand
            seen.add(v)
            out.append((name, v))
    return out


EDGES = _edges()
E = [v for _, v in EDGES]

# name -> (op number of noise_aead_debug_f25_op or None when only the CPU
# check offers it, operands, the constant of a mul_small)
OPS = {
    "add": (0, 2, None),
    "sub": (1, 2, None),
    "mul": (2, 2, None),
    "sq": (3, 1, None),
    "mul_small_121665": (4, 1, 121665),
    "mul_small_9": (5, 1, 9),
    "freeze": (6, 1, None),
    "invert": (7, 1, None),
    f"mul_small_{KMAX}": (None, 1, KMAX),
}
DEVICE_OPS = [name for name, (num, _, _) in OPS.items() if num is not None]

PATHS = {
    "add": ("carry", "fold_wrap"),
    "sub": ("borrow", "second_borrow"),
    "mul": ("hi2", "fold_wrap"),
    "sq": ("hi2", "fold_wrap"),
    "mul_small_121665": ("fold_wrap",),
    "mul_small_9": ("fold_wrap",),
    f"mul_small_{KMAX}": ("fold_wrap",),
    "freeze": ("bit255", "recarry", "ge_p"),
    # the chain's first step is sq(a), so E's sq vectors carry over
    "invert": ("zero", "noncanonical", "inner_hi2", "inner_fold_wrap"),
}
RARE = ("fold_wrap", "second_borrow", "recarry", "ge_p", "inner_fold_wrap")


# ------------------------------------------------- the operations, restated

def _fold(r, hi, taken):
    """r + hi M as r + 38 hi; a sum that passes M drops M and adds 38 once
    more, which must fit the lowest 32-bit word (what is left is below 38 hi)."""
    r += 38 * hi
    if r >= M:
        taken.add("fold_wrap")
        r -= M
        assert r + 38 < 2**32
        r += 38
    return r


def _add(a, b, taken):
    s = a + b
    if s >= M:
        taken.add("carry")
    return _fold(s % M, s // M, taken)


def _sub(a, b, taken):
    d = a - b
    if d < 0:
        taken.add("borrow")
        d += M - 38
        if d < 0:
            taken.add("second_borrow")
            d += M - 38
            assert d >= 0
    return d


def _mul(a, b, taken):
    w = a * b
    t = w % M + 38 * (w // M)
    if t >= M:
        taken.add("hi2")
    assert t // M <= 38
    return _fold(t % M, t // M, taken)


def _mul_small(a, k, taken):
    t = a * k
    assert t // M < 2**26
    return _fold(t % M, t // M, taken)


def _freeze(a, taken):
    top = a // B255
    if top:
        taken.add("bit255")
    a = a % B255 + 19 * top
    if a >= B255:
        taken.add("recarry")
    elif a >= P:
        taken.add("ge_p")
    b = a + 19  # a >= p exactly when this reaches 2^255
    return b - B255 if b >= B255 else a


def _invert(z, taken):
    """z^(2^255 - 21) by the chain 2, 9, 11, 2^5 - 1, 2^10 - 1, 2^20 - 1,
    2^40 - 1, 2^50 - 1, 2^100 - 1, 2^200 - 1, 2^250 - 1."""
    inner = set()
    if z % P == 0:
        taken.add("zero")
    if z >= P:
        taken.add("noncanonical")

    def sqn(x, n):
        for _ in range(n):
            x = _mul(x, x, inner)
        return x

    def mul(x, y):
        return _mul(x, y, inner)

    z2 = sqn(z, 1)
    z9 = mul(sqn(z2, 2), z)
    z11 = mul(z9, z2)
    e5 = mul(sqn(z11, 1), z9)
    e10 = mul(sqn(e5, 5), e5)
    e20 = mul(sqn(e10, 10), e10)
    e40 = mul(sqn(e20, 20), e20)
    e50 = mul(sqn(e40, 10), e10)
    e100 = mul(sqn(e50, 50), e50)
    e200 = mul(sqn(e100, 100), e100)
    e250 = mul(sqn(e200, 50), e50)
    taken.update("inner_" + p for p in inner)
    return mul(sqn(e250, 5), z11)


def paths(op, a, b=0):
    """(the raw 256-bit value the restated steps give, the set of path names taken)"""
    taken = set()
    k = OPS[op][2]
    if op == "add":
        r = _add(a, b, taken)
    elif op == "sub":
        r = _sub(a, b, taken)
    elif op == "mul":
        r = _mul(a, b, taken)
    elif op == "sq":
        r = _mul(a, a, taken)
    elif k is not None:
        r = _mul_small(a, k, taken)
    elif op == "freeze":
        r = _freeze(a, taken)
    else:
        r = _invert(a, taken)
    assert 0 <= r < M
    return r, taken


def expected(op, a, b=0):
    """The canonical answer, from Python's own integer arithmetic."""
    k = OPS[op][2]
    if op == "add":
        return (a + b) % P
    if op == "sub":
        return (a - b) % P
    if op == "mul":
        return a * b % P
    if op == "sq":
        return a * a % P
    if k is not None:
        return a * k % P
    if op == "freeze":
        return a % P
    return pow(a, P - 2, P)  # 0 -> 0


# ---------------------------------------------------------------- the vectors

def edge_vectors(op):
    if OPS[op][1] == 2:
        return [(a, b) for a in E for b in E]
    return [(a, 0) for a in E]


@functools.lru_cache(maxsize=None)
def random_vectors(op):
    rng = random.Random(0xF25 * 1000 + list(OPS).index(op))
    binary = OPS[op][1] == 2
    return tuple((rng.getrandbits(256), rng.getrandbits(256) if binary else 0) for _ in range(RANDOM_PAIRS))


@functools.lru_cache(maxsize=None)
def vectors(op):
    """Every (a, b) of one launch of op: the edges, then the random ones."""
    return tuple(edge_vectors(op)) + random_vectors(op)


def le32(v):
    return v.to_bytes(32, "little")


def pack(values):
    return b"".join(le32(v) for v in values)


def check_lines(op):
    """The vectors of op as asan/dh_check reads them: f25 <op> <a> <b>
    <canonical result>, each the hex of 32 little-endian bytes."""
    return "".join(f"f25 {op} {le32(a).hex()} {le32(b).hex()} {le32(expected(op, a, b)).hex()}\n"
                   for a, b in vectors(op))
