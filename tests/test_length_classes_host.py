"""tests/length_classes.py on the CPU: the universes have the sizes counted
from the kernels' partition arithmetic, the derived lists cover them, the older
hand-written lists did not, and the oracle seals and opens every fixture."""
import numpy as np
import pytest

import length_classes as C
from aead_gpu import EDGE_LENS, LENS
from gpu_support import AES, CHACHA

IL_CASES = {4: 89, 8: 185, 16: 377, 32: 761, 64: 1529}      # 24 K - 7
# the pairs (o, steps) and triples (q, partial, steps) alone take 30 / 38 / 54 / 86 / 150
# lengths; the one-step triples of a record with a full unit before its tail add 7
IL_REDUCED = {4: 37, 8: 45, 16: 61, 32: 93, 64: 157}
SEG_RAGGED_CASES = {1: 25, 2: 32, 4: 32, 8: 32, 16: 64}
GCM_CASES = {4: (99, 176), 8: (207, 368)}                    # cases, the longest record


def test_seg_k_of_restates_the_kernel():
    """seg_k_of: the smallest power of two K <= 16 with ceil((J + 1) / K) <= 32"""
    for J in range(0, 1025):
        K = C.seg_k_of(J)
        assert K in C.SEG_LANES and (K == 16 or (J + 1 + K - 1) // K <= 32)
        assert K == 1 or (J + 1 + K // 2 - 1) // (K // 2) > 32
    # seg_blocks: the lanes' blocks are the record's J + 1, in order, even runs first
    for L in (0, 1, 64, 65, 1400, 2047, 2048, 4096, 30000, C.MAX_LEN):
        for K in C.SEG_LANES:
            per, nbs = C.seg_lanes(K, L)
            live = [nb for nb in nbs if nb]
            assert sum(nbs) == (L + 63) // 64 + 1 and nbs[:len(live)] == live
            assert all(nb == (per + 1) // 2 * 2 for nb in live[:-1])


@pytest.mark.parametrize("K", C.IL_LANES)
def test_il_universe_and_lists(K):
    uni = C.universe(lambda L: C.il(K, L), C.il_range(K))
    assert len(uni) == IL_CASES[K] == 24 * K - 7
    full = C.full("il", K)
    assert len(full) == len(uni) and C.universe(lambda L: C.il(K, L), full) == uni
    assert list(full) == sorted(full) and max(full) <= 3 * 64 * K + 64
    # the universe is closed: longer records fall into the three-step cases
    assert C.universe(lambda L: C.il(K, L), range(3 * 64 * K + 65, 3 * 64 * K + 65 + 64 * K)) <= uni
    red = C.reduced(K)
    assert len(red) == IL_REDUCED[K]
    want = {m for L in C.il_range(K) for m in C.il_marginals(K, L)}
    assert {m for L in red for m in C.il_marginals(K, L)} == want
    assert len([m for m in want if m[0] == "lane"]) == 2 * K
    assert len([m for m in want if m[0] == "tail"]) == 33
    assert len({m[:4] for m in want if m[0] == "tail"}) == 25
    # each one-step q on a record where it reaches the tag: a full unit before the tail
    assert {C.il(K, L)[1] for L in red if C.il_steps(K, L) == 1 and L > 64} == {1, 2, 3, 4}
    # every (lane, jump) pair and every tail at one, two and three steps
    for lst in (full, red):
        assert {C.il(K, L)[2] for L in lst} == {1, 2, 3}


@pytest.mark.parametrize("K", [16, 32, 64])
def test_il_lists_reach_every_tree_level(K):
    """poly_tree_close runs level L (1, 2, 4, .. < K - 1) only when a group
    has more than L full units (J - 1 > L) in a one-step record."""
    levels = [1 << i for i in range(7) if (1 << i) < K - 1]
    assert levels[-1] == K // 2
    for lst in (C.full("il", K), C.reduced(K)):
        for lvl in levels:
            assert any(C.il_steps(K, L) == 1 and (L + 63) // 64 - 1 > lvl for L in lst), (K, lvl)
    # the widest level of a 64-lane group: a one-step record of 2113 .. 4032 bytes
    if K == 64:
        assert [L for L in (2112, 2113, 4032, 4033) if C.il_steps(64, L) == 1 and (L + 63) // 64 - 1 > 32] == [2113, 4032]


def test_solo_universe_and_list():
    uni = C.universe(C.solo, range(C.MAX_LEN + 1))
    full = C.full("solo")
    assert len(uni) == len(full) == 49 and max(full) <= 384
    assert C.universe(C.solo, full) == uni


def test_seg_universes_and_lists():
    uni2 = C.universe(lambda L: C.seg(2, L), range(C.MAX_LEN + 1))
    full2 = C.full("seg", 2)
    assert len(uni2) == len(full2) == 73 and max(full2) <= 576
    assert C.universe(lambda L: C.seg(2, L), full2) == uni2
    uni = C.universe(C.seg_ragged, range(C.MAX_LEN + 1))
    full = C.full("seg_ragged")
    assert len(uni) == len(full) == 185 and C.universe(C.seg_ragged, full) == uni
    assert {K: sum(1 for c in uni if c[0] == K) for K in C.SEG_LANES} == SEG_RAGGED_CASES
    assert 1.5e6 < sum(full) < 1.7e6


@pytest.mark.parametrize("K", C.GCM_LANES)
def test_gcm_universe_and_list(K):
    items = [(L, a) for L in range(C.GCM_MAX_LEN + 1) for a in C.GCM_ADS]
    uni = C.universe(lambda x: C.gcm(K, *x), items)
    full = C.full("gcm", K)
    assert (len(uni), max(L for L, _a in full)) == GCM_CASES[K] and len(full) == len(uni)
    assert C.universe(lambda x: C.gcm(K, *x), full) == uni


@pytest.mark.parametrize("ct", [False, True])
def test_gcm_wide_list(ct):
    e = C.gcm_early(ct)
    assert e == (192 if ct else 128)
    lst = C.full("gcm_wide", 0, ct)
    items = [(L, a) for L in range(C.GCM_MAX_LEN + 1) for a in C.GCM_ADS]
    items += [(L, a) for L in C.gcm_wide_boundary(ct) for a in (0, 21)]
    wide = lambda x: C.gcm_wide(x[0], x[1], ct)
    assert C.universe(wide, lst) == C.universe(wide, items) and len(lst) <= 512
    assert set(C.full("gcm", 8)) <= set(lst)
    Ms = {(L + 15) // 16 for L, _a in lst}
    assert {e - 1, e, e + 1, 255, 256, 257} <= Ms
    assert {c[-2:] for c in C.universe(wide, lst)} == {(-1, False), (0, False), (1, False), (1, True)}
    for M in (e - 1, e, e + 1, 255, 256, 257):
        assert (16 * M, 0) in lst and (16 * M - 9, 0) in lst


def test_the_hand_written_lists_were_thin():
    """The gap the derived lists close, as assertions: were the new lists to
    shrink to what the old ones reached, this would say so."""
    for K in C.IL_LANES:
        reached = C.universe(lambda L: C.il(K, L), LENS) & C.cases("il", K)
        assert len(reached) == 20 and 4 * len(reached) < IL_CASES[K], (K, len(reached))
    wide = {c for c in C.cases("seg_ragged") if c[0] >= 4}
    reached = C.universe(C.seg_ragged, EDGE_LENS) & wide
    assert len(wide) == 128 and len(reached) == 11 and 4 * len(reached) < len(wide)
    # the 1500 random lengths below 4000 (and 16384) of the windowed ragged
    # test: no two- or three-step case of a 64-lane group but 16384's
    assert {C.il(64, L)[2] for L in range(4000)} == {1}


def _round_trip(oracle, cipher, pairs, seed):
    rng = np.random.default_rng(seed)
    key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    for i, (L, adl) in enumerate(pairs):
        pt = bytes(rng.integers(0, 256, L, dtype=np.uint8))
        ad = bytes(rng.integers(0, 256, adl, dtype=np.uint8))
        ct = oracle.encrypt(cipher, key, 1000 + i, pt, ad)
        assert len(ct) == L + 16
        rc, back = oracle.decrypt(cipher, key, 1000 + i, ct, ad)
        assert rc == 0 and back == pt, (L, adl)
        bad = bytearray(ct)
        bad[L + (i % 16)] ^= 1 << (i % 8)
        rc, _ = oracle.decrypt(cipher, key, 1000 + i, bytes(bad), ad)
        assert rc != 0, (L, adl)


@pytest.mark.parametrize("name", ["il4", "il8", "il16", "il32", "il64", "solo", "seg2", "seg_ragged",
                                  "gcm4", "gcm8", "gcm_wide", "gcm_wide_ct"])
def test_oracle_round_trips_every_fixture(oracle, name):
    """Each (len, ad_len) the GPU sweep uses: sealed, opened back, and one
    flipped tag bit rejected, by the CPU oracle alone."""
    if name.startswith("il"):
        K = int(name[2:])
        pairs = C.with_ad(C.full("il", K)) + C.with_ad(C.reduced(K))
        cipher = CHACHA
    elif name.startswith("gcm_wide"):
        pairs, cipher = list(C.full("gcm_wide", 0, name.endswith("ct"))), AES
    elif name.startswith("gcm"):
        pairs, cipher = list(C.full("gcm", int(name[3:]))), AES
    else:
        lst = {"solo": C.full("solo"), "seg2": C.full("seg", 2), "seg_ragged": C.full("seg_ragged")}[name]
        pairs, cipher = C.with_ad(lst), CHACHA
    _round_trip(oracle, cipher, pairs, len(pairs))


# ------------------------------------------------ the resident worker's lists

WMULTI_MARGINALS = {"chunk": 93, "pass": 48, "tail": 24}
WTRANSPORT = {0: 24, 1: 17}  # host memory (12-byte chunks, head 3072), device memory (8, 2048)


def _old_worker_records():
    """the hand-written (len, ad_len) of the worker's older ChaChaPoly tests,
    imported from where they are used"""
    import edge_records as E
    import worker_mode_check as M
    from aead_gpu import worker_cases
    old = set(worker_cases())
    old |= {(L, A) for L in M.MAIN_LENS for A in M.MAIN_ADS}
    old |= {(L, A) for A in M.HEAD_EDGE_ADS for L in M.head_edge_lens(A)}
    for name, (cipher, _seed, lens, ads) in E.RAGGED_SHAPES.items():
        if name.startswith("worker") and cipher == E.CHACHA:
            old |= set(zip(lens, ads))
    return old


def test_worker_fast_fits_restates_the_kernel():
    """worker_fast_fits: at most 63 units and at most 256 Poly1305 blocks"""
    assert C.worker_fast_fits(4032, 48) and not C.worker_fast_fits(4033, 0)
    assert not C.worker_fast_fits(4032, 49) and C.worker_fast_fits(4016, 49)
    assert C.worker_fast_fits(3824, 256) and not C.worker_fast_fits(3825, 256)
    for L, a in ((0, 0), (4032, 0), (4032, 48), (3824, 256), (65519, 256)):
        _a, _m, n = C._poly_blocks(L, a)
        assert C.worker_fast_fits(L, a) == (L <= 4032 and n <= 256)
    assert [C._pow2(n) for n in (1, 2, 3, 4, 5, 33, 64, 65, 256)] == [1, 2, 4, 4, 8, 64, 64, 128, 256]


def test_wfast_universe_and_list():
    items = [(L, a) for L in range(C.WFAST_MAX_LEN + 1) for a in C.WORKER_ADS if C.worker_fast_fits(L, a)]
    uni = C.universe(lambda x: C.wfast(*x), items)
    full = C.full("wfast")
    assert len(uni) == len(full) == 312 and C.universe(lambda x: C.wfast(*x), full) == uni == C.cases("wfast")
    assert max(L for L, _a in full) == 4032 and all(C.worker_fast_fits(*x) for x in full)
    # every tree width, N = 64 (n = 33 .. 64: the level-32 shuffle is the last) by name
    assert {c[0] for c in uni} == set(range(9))
    assert any(C.wfast(*x)[0] == 6 for x in full)
    # each width above 2 full, one block past the half, and between (N = 4: n = 3 or 4 only)
    for lg in range(2, 9):
        assert {c[1] for c in uni if c[0] == lg} == ({0, 1} if lg == 2 else {0, 1, 2})
    assert {c[3] for c in uni} == {0, 1, 2, 3, 4} and {c[2] for c in uni} == {0, 1, 2}


def test_wfast_border_keeps_both_sides_and_the_corner():
    border = C.wfast_border()
    assert len(border) == 19 and len(set(border)) == 19
    for a in C.WORKER_ADS:
        fit = [L for L, x in border if x == a and C.worker_fast_fits(L, a)]
        over = [L for L, x in border if x == a and not C.worker_fast_fits(L, a)]
        assert len(fit) == 1 and fit[0] + 1 in over
        assert not C.worker_fast_fits(fit[0] + 1, a)
    # where both limits meet: 63 units with n = 256 against n = 257 (G = 2, pad = 1)
    assert (4032, 48) in border and C.worker_fast_fits(4032, 48) and C._poly_blocks(4032, 48)[2] == 256
    assert (4032, 49) in border and not C.worker_fast_fits(4032, 49)
    assert C.wmulti_geometry(4032, 49)[2:] == (257, 2, 129, 1)


def test_wmulti_universe_and_list():
    items = [(L, a) for L in range(C.MAX_LEN + 1) for a in C.WORKER_ADS if not C.worker_fast_fits(L, a)]
    uni = set()
    for x in items:
        uni.update(C.wmulti(*x))
    full = C.full("wmulti")
    assert {k: sum(1 for m in uni if m[0] == k) for k in WMULTI_MARGINALS} == WMULTI_MARGINALS
    assert len(uni) == 165 and C.cases("wmulti") == uni
    assert len(full) == 160 and list(full) == sorted(full) and not any(C.worker_fast_fits(*x) for x in full)
    assert 4.9e6 < sum(L for L, _a in full) < 5.1e6
    # every Horner depth (12 .. 15: bit 2 set below the top bit of the r^G
    # ladder) and every number of ChaCha passes (3: a pair alone, 4: the
    # smallest pair and a single)
    assert {m[1] for m in uni if m[0] == "chunk"} == set(range(1, 18))
    assert {m[1] for m in uni if m[0] == "pass"} == set(range(1, 18))
    assert {C.wmulti_geometry(*x)[3] for x in full} == set(range(1, 18))
    assert {C.wmulti_geometry(*x)[1] for x in full} == set(range(1, 18))
    # P = 1 has no one-block last pass (J = 0 fits), P = 17 only that (J = 1024)
    assert {m[2] for m in uni if m[:2] == ("pass", 1)} == {1, 2}
    assert {m[2] for m in uni if m[:2] == ("pass", 17)} == {0}
    # the tampered bit's three places lie inside the record and its AD
    for L, a in full:
        for field, lo, hi in C.wmulti_flips(L, a):
            assert 0 <= lo < hi <= {"ad": a, "ct": L, "tag": 16}[field], (L, a, field)
        J, P, n, G, NL, pad = C.wmulti_geometry(L, a)
        assert 1 <= G <= 17 and 1 <= P <= 17 and NL <= 256 and 0 <= pad < G and NL * G - pad == n


@pytest.mark.parametrize("vram", [0, 1])
def test_wtransport_universe_and_list(vram):
    items = [(op, L, a) for L in range(8193) for a in (0, 17) for op in (0, 1)]
    uni = C.universe(lambda x: C.wtransport(vram, *x), items)
    full = C.full("wtransport", vram)
    assert len(uni) == len(full) == WTRANSPORT[vram] and C.cases("wtransport", vram) == uni
    chunk, head = C.WORKER_CHUNK[vram], C.WORKER_HEAD[vram]
    assert (chunk, head) == ((8, 2048) if vram else (12, 3072)) and head == 256 * chunk
    assert {c[1] for c in uni if c[0] < 0} == set(range(chunk)) and {c[1] for c in uni if c[0] >= 0} == {None}
    assert {c[0] for c in uni} == {-1, 0, 1}
    for k in (2, 4):  # the raw tail's pieces, the result's
        assert {c[k:k + 2] for c in uni} == {(0, False), (1, False), (1, True), (2, False), (2, True)}
    # closed: the longest record adds nothing
    assert {C.wtransport(vram, op, C.MAX_LEN, a) for op in (0, 1) for a in (0, 17)} <= uni


def test_the_workers_hand_written_lists_were_thin():
    """What LENS x ADS (sampled), worker_mode_check.py's lengths and the
    worker shapes of edge_records.py reach of the above."""
    old = _old_worker_records()
    fast = {x for x in old if C.worker_fast_fits(*x)}
    multi = old - fast
    reached = C.universe(lambda x: C.wfast(*x), fast)
    assert sorted({1 << c[0] for c in reached}) == [1, 2, 4, 8, 16, 32, 128, 256]  # no N = 64
    assert not any(33 <= C._poly_blocks(*x)[2] <= 64 for x in fast)
    # 93 cases, 88 of them among the 312 (the others come with the old lists' 13 and 32 bytes of AD)
    assert len(reached) == 93 and len(reached & C.cases("wfast")) == 88
    m = set()
    for x in multi:
        m.update(C.wmulti(*x))
    assert m <= C.cases("wmulti")
    assert sorted({c[1] for c in m if c[0] == "chunk"}) == [1, 2, 3, 5, 10, 16, 17]
    assert sorted({c[1] for c in m if c[0] == "pass"}) == [1, 2, 5, 10, 17]
    assert {k: sum(1 for c in m if c[0] == k) for k in WMULTI_MARGINALS} == {"chunk": 13, "pass": 8, "tail": 13}
    # the border: 4032 bytes was never run with 48 or 49 bytes of AD
    assert not {(4032, 48), (4032, 49), (4016, 49), (4017, 49)} & old
    # the transport: the head edges were there; not every residue of the last
    # chunk, nor a short last piece in both of a two-round record's loops
    for vram, reached, missing in ((0, 20, {2, 6, 10}), (1, 12, {2, 3, 5, 6})):
        gap = C.cases("wtransport", vram) - {C.wtransport(vram, op, L, a) for (L, a) in old for op in (0, 1)}
        assert len(C.cases("wtransport", vram)) - len(gap) == reached
        assert {c[1] for c in gap if c[0] < 0} == missing
        assert {c for c in gap if c[0] >= 0} == {(1, None, 1, True, 2, True)}


@pytest.mark.parametrize("name", ["wfast", "wmulti", "wtransport0", "wtransport1"])
def test_oracle_round_trips_every_worker_fixture(oracle, name):
    """as test_oracle_round_trips_every_fixture, for the worker's records"""
    if name == "wfast":
        pairs = list(C.full("wfast")) + C.wfast_border()
    elif name == "wmulti":
        pairs = list(C.full("wmulti"))
    else:
        pairs = sorted({x[1:] for x in C.full("wtransport", int(name[-1]))})
    _round_trip(oracle, CHACHA, pairs, len(pairs))
