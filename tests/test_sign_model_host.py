"""The Ed25519 model of tests/ed25519_model.py — the checker the GPU tests use
for random entries — against every record of tests/golden/ed25519.json, which
the reference's NoiseSignState wrote (tests/golden/gen_ed25519.py): bytes and
verdicts, and the conditions that keep the fixture from being passed by a
device that refuses, or accepts, everything unusual."""
import ed25519_model as M


def test_model_signs_as_the_reference():
    cases = M.fixture_sign_cases()
    assert len(cases) == 5 + 24 and len({c[0] for c in cases}) == len(cases)
    assert cases[0][2].hex() == "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a"
    assert len(cases[3][3]) == 1023
    assert {len(c[3]) for c in cases[5:]} == set(M.MESSAGE_LENGTHS)
    for name, seed, pub, msg, sig in cases:
        assert M.publickey(seed) == pub, name
        assert M.sign(msg, seed, pub) == sig, name
        assert M.verify(msg, pub, sig), name


def test_model_verifies_as_the_reference():
    fx = M.fixture()["verify"]
    cases = M.fixture_verify_cases()
    assert len(cases) == len(fx) >= 250 and len({c[0] for c in cases}) == len(cases)
    assert {c["rc"] for c in fx} == {0, M.ERROR_INVALID_SIGNATURE}
    for name, msg, pub, sig, ok in cases:
        assert M.verify(msg, pub, sig) == ok, name
        assert M.status(msg, pub, sig) == (0 if ok else 6), name


def test_fixture_groups_hold_both_verdicts():
    fx = M.fixture()["verify"]
    groups = {}
    for c in fx:
        groups.setdefault(c["group"], set()).add(c["rc"])
    for g in ("s_plus_l", "noncanonical_y", "small_order", "noncanonical_r", "y_edges"):
        assert groups[g] == {0, M.ERROR_INVALID_SIGNATURE}, g
    for g in ("tampered", "s_top_bits", "s_edges", "no_root"):
        assert groups[g] == {M.ERROR_INVALID_SIGNATURE}, g
    assert groups["valid"] == {0}
    by = {c["name"]: c for c in fx}
    # the leniencies the header names, as the reference decided them
    assert by["random-0-S+L"]["rc"] == 0 and by["random-0-S+2L"]["rc"] != 0
    assert by["y=p+1-identity-sig"]["rc"] == 0 and by["y=1-signbit-identity-sig"]["rc"] == 0
    assert by["R=identity"]["rc"] == 0 and by["R=p+1"]["rc"] != 0
    assert sum(c["group"] == "small_order" and c["name"].endswith("-identity-sig") for c in fx) == 8


def test_constants_are_derived():
    assert M.encode(M.B) == bytes([0x58]) + bytes([0x66]) * 31
    assert (-M.BX * M.BX + M.BY * M.BY - 1 - M.D * M.BX * M.BX * M.BY * M.BY) % M.P == 0
    assert M.D * 121666 % M.P == M.P - 121665 and M.BX % 2 == 0
    assert M.encode(M.mul(M.L, M.B)) == M.encode(M.IDENTITY)
    assert M.SIGN_ED25519 == (ord("S") << 8 | 1) and M.ERROR_INVALID_SIGNATURE == (ord("E") << 8 | 17)
