"""The crafted edge records (tests/edge_records.py) against the CPU checkers.

Before tests/test_gpu_edge_values.py trusts a crafted record, every record of
every batch it uses — same shapes, same seeds — is checked here without a GPU:
the oracle accepts it and re-encrypts its plaintext to the same bytes, the
oracle's Poly1305 gives the big-integer tag, the label is recomputed from the
record's bytes (final value, prefix value, tag, GHASH value), and the
reference itself agrees where it has been built.
"""
import pytest

import edge_records as E
from edge_records import AES, CHACHA, M128, P


def _shape_id(s):
    return "%s-n%d-rps%d-L%d-ad%d" % ("chacha" if s[0] == CHACHA else "aes", *s[1:])


def check_label(oracle, rec):
    """The label of a crafted record, recomputed from its bytes."""
    lab, ad = rec["label"], rec["ad"]
    ct, tag = rec["sealed"][:-16], rec["sealed"][-16:]
    n_ad = (len(ad) + 15) // 16
    if lab["cls"] in E.CHACHA_CLASSES:
        ks = oracle.chacha20_block(rec["key"], 0, rec["nonce"])
        r, s = E.poly_key(oracle, rec["key"], rec["nonce"])
        blocks = E.poly_blocks(ad, ct)
        v = E.horner(blocks, r)
        assert ((v + s) % M128).to_bytes(16, "little") == tag
        msg = E.pad16(ad) + E.pad16(ct) + len(ad).to_bytes(8, "little") + len(ct).to_bytes(8, "little")
        assert oracle.poly1305(ks[:32], msg) == tag
        if lab["cls"] == "final":
            assert v == lab["value"] % P
        elif lab["cls"] == "tagcarry":
            assert int.from_bytes(tag, "little") == lab["value"]
            assert v == E.tag_target_value(lab["value"], s, lab["drop"]) and v + (lab["drop"] + 1) * M128 >= P
        else:
            j = lab["blk"]
            assert E.horner(blocks[:j + 1], r) == lab["value"] % P
            assert j >= n_ad and ct[16 * (j + 1 - n_ad):16 * (j + 2 - n_ad)] == b"\xff" * 16
    else:
        gk = E.GcmKey(oracle, rec["key"])
        blocks = E.ghash_blocks(ad, ct)
        y = gk.ghash(blocks)
        assert E.xor16(gk.ej0(rec["nonce"]), y) == tag
        if lab["cls"] == "ghash_prefix":
            j = lab["blk"]
            assert E.xor16(gk.ghash(blocks[:j]), blocks[j]) == lab["value"]
        else:
            assert y == lab["final"]
        if lab["cls"] == "ghash_pattern":
            j = lab["blk"] - n_ad
            for i in range(0, len(ct), 16):
                assert i == 16 * j or ct[i:i + 16] == lab["value"][:len(ct) - i]


def check_batch(oracle, b):
    assert not b.uncrafted, b.uncrafted
    for i, rec in enumerate(b.records):
        a = (b.cipher, rec["key"], rec["nonce"])
        rc, pt = oracle.decrypt(*a, rec["sealed"], rec["ad"])
        assert rc == 0 and pt == rec["pt"], (i, rec["label"])
        assert oracle.encrypt(*a, rec["pt"], rec["ad"]) == rec["sealed"], (i, rec["label"])
        check_label(oracle, rec)


@pytest.mark.parametrize("shape", E.UNIFORM_SHAPES, ids=_shape_id)
def test_uniform_batches(oracle, shape):
    cipher, count, rps, L, ad_len = shape
    b = E.shaped(oracle, shape)
    assert b.count == count and all(len(r["pt"]) == L and len(r["ad"]) == ad_len for r in b.records)
    check_batch(oracle, b)
    # the batch is a uniform one: fixed keys, nonce = base + index in the run
    for i, rec in enumerate(b.records):
        assert rec["key"] == bytes(b.keys[i // rps]) and rec["nonce"] == int(b.nonce_base[i // rps]) + i % rps
    # the low nonce word carries inside every state's run that has two records
    assert int(b.nonce_base[0]) >> 32 == 0xFFFFFFFE
    for s, base in enumerate(b.nonce_base):
        run = min(rps, count - s * rps)
        d = 2**32 - (int(base) & 0xFFFFFFFF)
        assert int(base) + rps < 2**64 and 1 <= d and (d < run or run == 1), (s, d, run)
        assert run <= 64 or d % 64
    if L >= 32:
        want = set(E.classes_of(cipher))
        if cipher == CHACHA and L < 48:
            want.discard("prefix")
        assert b.classes() == want
    elif cipher == CHACHA:
        assert len({dict(E.FINAL_TARGETS)[n] for n in b.names("final")}) >= 5 and len(b.names("tagcarry")) >= 2
    if cipher == CHACHA:
        # both sides of p reach the final reduction in every batch
        finals = {l["value"] for l in b.labels if l["cls"] == "final"}
        assert finals & {0, 1, 4} and P - 1 in finals


@pytest.mark.parametrize("name", sorted(E.RAGGED_SHAPES))
def test_ragged_batches(oracle, name):
    cipher, _seed, lens, ads = E.RAGGED_SHAPES[name]
    b = E.ragged_shaped(oracle, name)
    assert [len(r["pt"]) for r in b.records] == list(lens) and [len(r["ad"]) for r in b.records] == list(ads)
    check_batch(oracle, b)
    if b.count > 20:
        assert b.classes() == set(E.classes_of(cipher))
    if name in ("chacha", "seg", "worker_chacha"):
        finals = {l["value"] for l in b.labels if l["cls"] == "final"}
        assert finals & {0, 1, 4} and P - 1 in finals
    if name in ("chacha", "aes"):  # single-block and AD-only records are crafted too
        assert any(len(r["pt"]) == 16 for r in b.records) and any(len(r["pt"]) == 0 for r in b.records)


def test_reference_agrees(oracle, reflib):
    """The reference's own CipherState seals every crafted plaintext to the
    crafted bytes and opens them back: every record of every batch."""
    batches = [E.shaped(oracle, s) for s in E.UNIFORM_SHAPES] + [E.ragged_shaped(oracle, n) for n in E.RAGGED_SHAPES]
    for b in batches:
        for rec in b.records:
            a = (b.cipher, rec["key"], rec["nonce"])
            assert reflib.encrypt(*a, rec["pt"], rec["ad"]) == rec["sealed"], rec["label"]
            rc, pt = reflib.decrypt(*a, rec["sealed"], rec["ad"])
            assert rc == 0 and pt == rec["pt"], rec["label"]


def test_same_seed_same_bytes(oracle):
    for shape in [(CHACHA, 150, 13, 64, 21), (CHACHA, 150, 13, 16, 0), (AES, 150, 13, 100, 21)]:
        first = E.shaped(oracle, shape).digest()
        E._CACHE.clear()
        assert E.shaped(oracle, shape).digest() == first
    for name in ("chacha", "aes"):
        first = E.ragged_shaped(oracle, name).digest()
        E._CACHE.clear()
        assert E.ragged_shaped(oracle, name).digest() == first
    assert E.uniform_batch(oracle, CHACHA, 2, 150, 13, 64, 21).digest() != E.shaped(oracle, (CHACHA, 150, 13, 64, 21)).digest()


def test_edge_values_are_edges(oracle):
    """The targets themselves: p - 1 is the largest value fe_finish must not
    reduce, 2^130 - 6 is the same number, and every tag target's v is the
    largest below p."""
    assert dict(E.FINAL_TARGETS)["p-1"] == dict(E.FINAL_TARGETS)["2^130-6"] == P - 1
    for _n, T in E.TAG_TARGETS:
        for s in (0, 1, 5, 6, M128 - 1, T, (T + 5) % M128, (T + 6) % M128):
            v = E.tag_target_value(T, s)
            assert v < P <= v + M128 and (v + s) % M128 == T
